// Vector quantisation for a VQ first stage: nearest codebook entry per channels-last row, alone (gg_vq_nearest) or inside one reverse
// step of the LDM samplers (gg_ddim_step_vq).  The quantiser is taming's VectorQuantizer (beta has no part in inference):
//   d[m, k] = sum_c z[m,c]^2 + sum_c E[k,c]^2 - 2 sum_c z[m,c] E[k,c];  idx[m] = argmin_k d[m, k], the FIRST minimum on a tie;
//   returned rows are the straight-through expression z + (E[idx] - z), which differs from E[idx] by a rounding.
//
// Evaluation order (all fp32, no contraction: every product and every sum is rounded on its own):
//   zz  = z0*z0; zz = zz + z1*z1; ...            ascending c
//   ee  = e0*e0; ee = ee + e1*e1; ...            ascending c, once per code and tile while the tile is staged
//   dot = z0*e0; dot = dot + z1*e1; ...          ascending c
//   d   = (zz + ee) - 2*dot                      (2*dot is exact, so a fused multiply-add here would give the same bits)
//   q_c = z_c + (E[idx,c] - z_c)
//
// Mapping: a block of 256 threads owns VQ_ROWS = 16 rows.  Thread t handles row r = t % 16 and code segment g = t / 16: of every staged
// tile of VQ_TILE codes it scans the codes kk = g, g + 16, g + 32, ... (ascending), keeping a running (min, index) pair under the strict
// `<`, so that each lane holds the first minimum of its own codes.  The 16 pairs of a row are then merged by (d, index) in lexicographic
// order, which is the first minimum over the whole codebook whatever the interleaving.  The codebook passes through LDS in tiles, stored
// channel-major ([c][kk]) with ee[kk] beside it.  A wave holds 4 segments x 16 rows: the 16 lanes of a segment read the same float (a
// broadcast), the wave's 4 segments read 4 consecutive floats, so an LDS read is free of bank conflicts.  A code past n_embed is never
// staged and never read.  16 rows per block (not 64 or 256) because the chain's batch-1 latent has 4096 rows: 256 blocks keep every CU
// busy, at the price of one pass over the codebook (L2-resident) per 16 rows.
#include "gg_common.h"
#include "gg_step.h"

namespace {

constexpr int VQ_ROWS = 16;
constexpr int VQ_SEGS = 16;
constexpr int VQ_TILE = 1024;
constexpr int VQ_NONE = 0x7fffffff;

enum { VQ_NEAREST = 0, VQ_DDIM = 1, VQ_ANCESTRAL = 2 };

struct VqStep {
    float *x;                 // [M, C] in / out
    const float *eps;         // [M, eps_stride]
    const float *noise;       // [M, C] or NULL
    const float *sc;          // device fp32[5]
    float *pred_x0;           // [M, C] or NULL
    bf16_t *unet_in;          // [M, unet_in_stride] or NULL
    int eps_stride, unet_in_stride;
};

template <int C, int MODE>
__global__ __launch_bounds__(256) void vq_kernel(const float *rows, int row_stride, const float *__restrict__ E, int n_embed, long long M,
                                                 int *idx_out, float *st_out, int st_stride, VqStep s)
{
#pragma clang fp contract(off)
    __shared__ float lds_e[C * VQ_TILE];
    __shared__ float lds_n[VQ_TILE];
    __shared__ float red_d[VQ_SEGS][VQ_ROWS];
    __shared__ int red_i[VQ_SEGS][VQ_ROWS];
    const int tid = threadIdx.x;
    const int r = tid & (VQ_ROWS - 1), g = tid >> 4;
    const long long m = (long long)blockIdx.x * VQ_ROWS + r;
    const bool live = m < M;

    // the row to quantise: loaded (VQ_NEAREST) or the step's prediction of x_0 (every lane of a row computes the same values)
    float z[C], xv[C], ev[C];
    float k0 = 0.f, k1 = 0.f, k2 = 0.f, k3 = 0.f, k4 = 0.f;                     // the step's constants (gg_step.h), k4 the noise coefficient
    if constexpr (MODE == VQ_DDIM) {
        k0 = s.sc[3];                                   // sqrt(1 - a_t)
        ddim_roots(s.sc[0], s.sc[1], s.sc[2], k1, k2, k3);
        k4 = s.sc[4];
    } else if constexpr (MODE == VQ_ANCESTRAL) {
        k0 = s.sc[0]; k1 = s.sc[1]; k2 = s.sc[2]; k3 = s.sc[3]; k4 = s.sc[4];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        xv[c] = 0.f;
        ev[c] = 0.f;
        if constexpr (MODE == VQ_NEAREST) {
            z[c] = live ? rows[m * row_stride + c] : 0.f;
        } else {
            if (live) {
                xv[c] = s.x[m * C + c];
                ev[c] = s.eps[m * s.eps_stride + c];
            }
            if constexpr (MODE == VQ_DDIM) z[c] = ddim_pred_x0(xv[c], ev[c], k0, k1);
            else z[c] = ddpm_x_recon(xv[c], ev[c], k0, k1, 0);
        }
    }
    float zz = z[0] * z[0];
#pragma unroll
    for (int c = 1; c < C; ++c) zz = zz + z[c] * z[c];

    float best = INFINITY;
    int bi = VQ_NONE;
    for (int t0 = 0; t0 < n_embed; t0 += VQ_TILE) {
        const int nt = min(VQ_TILE, n_embed - t0);
        __syncthreads();                                 // the previous tile has been read by every lane
        for (int kk = tid; kk < nt; kk += 256) {
            const float *e = E + (long long)(t0 + kk) * C;
            float ee = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float v = e[c];
                lds_e[c * VQ_TILE + kk] = v;
                ee = c ? ee + v * v : v * v;
            }
            lds_n[kk] = ee;
        }
        __syncthreads();
        for (int kk = g; kk < nt; kk += VQ_SEGS) {
            float dot = z[0] * lds_e[kk];
#pragma unroll
            for (int c = 1; c < C; ++c) dot = dot + z[c] * lds_e[c * VQ_TILE + kk];
            const float d = (zz + lds_n[kk]) - 2.0f * dot;
            if (d < best) { best = d; bi = t0 + kk; }
        }
    }
    red_d[g][r] = best;
    red_i[g][r] = bi;
    __syncthreads();
    if (g != 0 || !live) return;

    // lane (r, 0): merge the row's 16 segments, then the epilogue of the row
    for (int j = 1; j < VQ_SEGS; ++j) {
        const float d = red_d[j][r];
        const int i = red_i[j][r];
        if (d < best || (d == best && i < bi)) { best = d; bi = i; }
    }
    if (bi == VQ_NONE) bi = 0;                           // a row of NaNs compares false everywhere: code 0, never out of range
    float q[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float t = E[(long long)bi * C + c] - z[c];
        q[c] = z[c] + t;
    }
    if (idx_out) idx_out[m] = bi;
    if constexpr (MODE == VQ_NEAREST) {
        if (st_out) {
#pragma unroll
            for (int c = 0; c < C; ++c) st_out[m * st_stride + c] = q[c];
        }
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float xn;
            if constexpr (MODE == VQ_DDIM) xn = ddim_x_prev(q[c], ev[c], k2, k3);
            else xn = ddpm_mean(q[c], xv[c], k2, k3);
            if (s.noise) xn = step_add_noise(xn, k4, s.noise[m * C + c]);
            s.x[m * C + c] = xn;
            if (s.pred_x0) s.pred_x0[m * C + c] = q[c];
            if (s.unet_in) s.unet_in[m * s.unet_in_stride + c] = (bf16_t)xn;
        }
    }
}

template <int MODE>
int vq_launch(int C, const float *rows, int row_stride, const float *E, int n_embed, long long M, int *idx_out, float *st_out, int st_stride,
              const VqStep &s, hipStream_t stream)
{
    const long long blocks = (M + VQ_ROWS - 1) / VQ_ROWS;
    if (blocks > 0x7fffffffLL) GG_FAIL(GG_ERR_UNSUPPORTED, "vq: M=%lld rows exceed the grid", M);
    const dim3 grid((unsigned)blocks), block(256);
#define VQ_CASE(CC)                                                                                                                  \
    case CC:                                                                                                                         \
        hipLaunchKernelGGL((vq_kernel<CC, MODE>), grid, block, 0, stream, rows, row_stride, E, n_embed, M, idx_out, st_out, st_stride, s); \
        break;
    switch (C) {
        VQ_CASE(1) VQ_CASE(2) VQ_CASE(3) VQ_CASE(4) VQ_CASE(5) VQ_CASE(6) VQ_CASE(7) VQ_CASE(8)
    default:
        GG_FAIL(GG_ERR_UNSUPPORTED, "vq: C=%d outside [1, 8]", C);
    }
#undef VQ_CASE
    GG_CHECK_LAUNCH();
    return GG_OK;
}

}  // namespace

extern "C" int gg_vq_nearest(const float *rows, int32_t row_stride, const float *codebook, int32_t n_embed, int32_t C, int64_t M,
                             int32_t *idx_out, float *st_out, int32_t st_stride, void *stream_)
{
    if (!rows || !codebook) GG_FAIL(GG_ERR_BAD_SHAPE, "vq_nearest: null pointer");
    if (!idx_out && !st_out) GG_FAIL(GG_ERR_BAD_SHAPE, "vq_nearest: neither idx_out nor st_out");
    if (C < 1 || C > 8) GG_FAIL(GG_ERR_UNSUPPORTED, "vq_nearest: C=%d outside [1, 8]", C);
    if (n_embed < 1) GG_FAIL(GG_ERR_BAD_SHAPE, "vq_nearest: n_embed=%d", n_embed);
    if (row_stride < C || (st_out && st_stride < C)) GG_FAIL(GG_ERR_BAD_SHAPE, "vq_nearest: stride < C");
    if (M <= 0) return GG_OK;
    return vq_launch<VQ_NEAREST>(C, rows, row_stride, codebook, n_embed, (long long)M, idx_out, st_out, st_stride, VqStep{}, (hipStream_t)stream_);
}

extern "C" int gg_ddim_step_vq(float *x, const float *eps, int32_t eps_stride, const float *noise, const float *scalars_dev, int32_t ancestral,
                               const float *codebook, int32_t n_embed, int64_t M, int32_t C, int32_t *idx_out, float *pred_x0_out,
                               void *unet_in, int32_t unet_in_stride, void *stream_)
{
    if (!x || !eps || !scalars_dev) GG_FAIL(GG_ERR_BAD_SHAPE, "ddim_step_vq: null pointer");
    if (C < 1 || C > 8) GG_FAIL(GG_ERR_UNSUPPORTED, "ddim_step_vq: C=%d outside [1, 8]", C);
    if (n_embed < 0 || (n_embed > 0 && !codebook)) GG_FAIL(GG_ERR_BAD_SHAPE, "ddim_step_vq: n_embed=%d without a codebook", n_embed);
    if (!codebook) n_embed = 0;
    if (idx_out && n_embed == 0) GG_FAIL(GG_ERR_BAD_SHAPE, "ddim_step_vq: idx_out without a codebook");
    if (eps_stride < C || (unet_in && unet_in_stride < C)) GG_FAIL(GG_ERR_BAD_SHAPE, "ddim_step_vq: stride < C");
    if (M <= 0) return GG_OK;
    if (n_embed == 0)                                    // nothing to quantise: the pointwise step, its noise coefficient the fifth scalar
        return gg_step_launch(ancestral, x, eps, eps_stride, noise, scalars_dev, 4, 0, (long long)M, C, pred_x0_out, unet_in, unet_in_stride,
                              (hipStream_t)stream_);
    VqStep s{x, eps, noise, scalars_dev, pred_x0_out, (bf16_t *)unet_in, eps_stride, unet_in_stride};
    if (ancestral)
        return vq_launch<VQ_ANCESTRAL>(C, nullptr, 0, codebook, n_embed, (long long)M, idx_out, nullptr, 0, s, (hipStream_t)stream_);
    return vq_launch<VQ_DDIM>(C, nullptr, 0, codebook, n_embed, (long long)M, idx_out, nullptr, 0, s, (hipStream_t)stream_);
}
