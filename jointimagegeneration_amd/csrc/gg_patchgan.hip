// The first stage's held-out objective (ldm/modules/losses/contperceptual.py), forward only: what LPIPSWithDiscriminator needs beyond
// LPIPS (gg_lpips.hip) and the per-sample l1 / l2 means (gg_loss_rows).
//   gg_patch_conv_forward(_f32)  the PatchGAN convolutions: kernel extent 4, zero padding 2, stride 2 or 1, 2-D and 3-D, with the folded
//                                conv bias + eval-mode BatchNorm (alpha, beta) and LeakyReLU in the epilogue   contperceptual.py:296-406
//   gg_gauss_kl_rows             DiagonalGaussianDistribution.kl()      ldm/modules/distributions/distributions.py:44-51
//   gg_gauss_sample_rows         DiagonalGaussianDistribution.sample()  distributions.py:35-37
//   gg_logit_stats               mean, hinge and softplus terms of a discriminator's logits   contperceptual.py:14-25,140,176
// The bf16 convolution is an implicit GEMM on MFMA with the tile and operand layout of conv_gather_kernel (gg_conv.hip): 128 positions x
// 32 * NT output channels per workgroup, weights in the packed tile order of gg_conv_pack_weight, k-steps walked (chunk outer, tap inner).
// The reductions are the two-stage fp64 ones of gg_reduce.h.
#include "gg_conv.h"
#include "gg_reduce.h"

namespace {

struct PatchParams {
    int N, D, H, W, Cin, Cout, Cout_pad, kd, stride, Do, Ho, Wo, out_dtype, ntaps, nchunk;
    long long M;
    const void *src, *weight;
    const float *alpha, *beta;
    float slope;
    void *out;
};

// y = acc * alpha + beta, LeakyReLU: every step rounded to fp32 once (nothing contracted); pad lanes store zero
__device__ __forceinline__ f32x4 patch_epilogue(f32x4 acc, const PatchParams &p, int co)
{
#pragma clang fp contract(off)
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float y = 0.f;
        if (co + j < p.Cout) {
            y = acc[j];
            if (p.alpha) y = y * p.alpha[co + j];
            y = y + p.beta[co + j];
            if (p.slope != 1.0f) y = y >= 0.f ? y : y * p.slope;
        }
        r[j] = y;
    }
    return r;
}

// output row m -> sample and the input coordinate of tap (0, 0, 0); the D axis of a 2-D conv (kd == 1) is a batch axis
struct PatchRow { int n, bd, bh, bw; };
__device__ __forceinline__ PatchRow patch_row(const PatchParams &p, unsigned m)
{
    const unsigned osp = (unsigned)(p.Do * p.Ho * p.Wo), ohw = (unsigned)(p.Ho * p.Wo);
    const unsigned n = m / osp;
    unsigned r = m - n * osp;
    const unsigned od = r / ohw;
    r -= od * ohw;
    const unsigned oh = r / (unsigned)p.Wo, ow = r - oh * (unsigned)p.Wo;
    return {(int)n, p.kd == 1 ? (int)od : (int)od * p.stride - 2, (int)oh * p.stride - 2, (int)ow * p.stride - 2};
}

template <int NT>
__global__ __launch_bounds__(256) void patch_conv_kernel(const PatchParams p)
{
    constexpr int BM = 128;
    constexpr int XBYTES = BM * 64;
    constexpr int WBYTES = NT * 32 * 64;
    constexpr int STAGE = XBYTES + WBYTES;
    constexpr int WITER = (NT * 128 + 255) / 256;
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long m0 = (long long)blockIdx.x * BM;
    const int g0 = blockIdx.y * NT;
    const bf16_t *src = (const bf16_t *)p.src, *weight = (const bf16_t *)p.weight;

    // gather duties: rows (tid >> 2) and (tid >> 2) + 64, 16-byte piece tid & 3 of the 64-byte channel chunk
    const int xq = tid & 3;
    PatchRow row[2];
    bool rv[2];
    const bf16_t *rb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long long m = m0 + (tid >> 2) + 64 * i;
        rv[i] = m < p.M;
        row[i] = patch_row(p, rv[i] ? (unsigned)m : 0u);              // host guarantees M < 2^31
        rb[i] = src + (long long)row[i].n * p.D * p.H * p.W * p.Cin + xq * 8;
    }
    const long long wgroup = ((long long)p.ntaps * p.nchunk) << 10;
    const int KS = p.ntaps * p.nchunk;
    const int tshift = p.kd == 1 ? 4 : 6;                            // ntaps = 16 or 64

    u32x4 xreg[2][2], wreg[2][WITER];
    auto load_regs = [&](int ks, u32x4 (&xr)[2], u32x4 (&wr)[WITER]) {
        const int chunk = ks >> tshift, tap = ks - (chunk << tshift);
        const int tkd = tap >> 4, tkh = (tap >> 2) & 3, tkw = tap & 3;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const unsigned ud = (unsigned)(row[i].bd + tkd), uh = (unsigned)(row[i].bh + tkh), uw = (unsigned)(row[i].bw + tkw);
            u32x4 v = {0u, 0u, 0u, 0u};
            if (rv[i] && ud < (unsigned)p.D && uh < (unsigned)p.H && uw < (unsigned)p.W) {      // unsigned compare also rejects negatives
                const unsigned pos = (ud * (unsigned)p.H + uh) * (unsigned)p.W + uw;
                v = *reinterpret_cast<const u32x4 *>(rb[i] + (pos * (unsigned)p.Cin + (unsigned)(chunk * 32)));
            }
            xr[i] = v;
        }
        const long long woff = (((long long)g0 * p.ntaps + tap) * p.nchunk + chunk) << 10;
#pragma unroll
        for (int j = 0; j < WITER; ++j) {
            const int i = tid + 256 * j;
            if (i < NT * 128) wr[j] = *reinterpret_cast<const u32x4 *>(weight + woff + (long long)(i >> 7) * wgroup + (i & 127) * 8);
        }
    };
    auto write_lds = [&](int buf, u32x4 (&xr)[2], u32x4 (&wr)[WITER]) {
        char *xb = smem + buf * STAGE;
        char *wb = xb + XBYTES;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = (tid >> 2) + 64 * i;
            *reinterpret_cast<u32x4 *>(xb + r * 64 + swz64(r, xq) * 16) = xr[i];
        }
#pragma unroll
        for (int j = 0; j < WITER; ++j) {
            const int i = tid + 256 * j;
            if (i < NT * 128) *reinterpret_cast<u32x4 *>(wb + i * 16) = wr[j];   // image pre-swizzled at pack time
        }
    };

    f32x4 acc[2][2 * NT];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2 * NT; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fq = lane >> 4;
    auto compute = [&](int buf) {
        const char *xb = smem + buf * STAGE;
        const char *wb = xb + XBYTES;
        bf16x8 xf[2];
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
            const int r = wave * 32 + pt * 16 + fr;
            xf[pt] = *reinterpret_cast<const bf16x8 *>(xb + r * 64 + swz64(r, fq) * 16);
        }
#pragma unroll
        for (int ct = 0; ct < 2 * NT; ++ct) {
            const int r = ct * 16 + fr;
            const bf16x8 wf = *reinterpret_cast<const bf16x8 *>(wb + r * 64 + swz64(r, fq) * 16);
#pragma unroll
            for (int pt = 0; pt < 2; ++pt)
                acc[pt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf[pt], acc[pt][ct], 0, 0, 0);
        }
    };

    // two k-steps of global loads in flight, two LDS stages, one barrier per k-step: a wave that passed barrier(ks + 1) knows every
    // wave finished compute(ks), so stage ks & 1 may be rewritten at ks + 2
    load_regs(0, xreg[0], wreg[0]);
    if (KS > 1) load_regs(1, xreg[1], wreg[1]);
    for (int ks0 = 0; ks0 < KS; ks0 += 2) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ks = ks0 + j;
            if (ks < KS) {
                write_lds(j, xreg[j], wreg[j]);
                __syncthreads();
                if (ks + 2 < KS) load_regs(ks + 2, xreg[j], wreg[j]);
                compute(j);
            }
        }
    }

#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
        const long long m = m0 + wave * 32 + pt * 16 + fr;
        if (m >= p.M) continue;
#pragma unroll
        for (int ct = 0; ct < 2 * NT; ++ct) {
            const int co = (g0 * 32) + ct * 16 + fq * 4;
            const f32x4 v = patch_epilogue(acc[pt][ct], p, co);
            const long long o = m * p.Cout_pad + co;
            if (p.out_dtype == GG_F32) {
                *reinterpret_cast<f32x4 *>((float *)p.out + o) = v;
            } else {
                bf16x4 ob;
#pragma unroll
                for (int j = 0; j < 4; ++j) ob[j] = (bf16_t)v[j];
                *reinterpret_cast<bf16x4 *>((bf16_t *)p.out + o) = ob;
            }
        }
    }
}

// fp32 validation form, the tiling of conv_f32_kernel (gg_f32.hip): 64 positions x 32 output channels per workgroup, fp32 weights
// [taps][Cin][Cout_pad], accumulation order taps outer, input channels inner, one fp32 FMA each
__global__ __launch_bounds__(256) void patch_conv_f32_kernel(const PatchParams p)
{
    __shared__ float xs[32][65];          // [ci][position]
    __shared__ float ws[32][32];          // [ci][co]
    const int tid = threadIdx.x;
    const long long m0 = (long long)blockIdx.x * 64;
    const int co0 = blockIdx.y * 32;
    const float *src = (const float *)p.src, *weight = (const float *)p.weight;
    const int sp = tid >> 2, sc = (tid & 3) * 8;
    const bool mvalid = m0 + sp < p.M;
    const PatchRow row = patch_row(p, mvalid ? (unsigned)(m0 + sp) : 0u);
    const int pq = tid & 31, cg = tid >> 5;
    float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int tap = 0; tap < p.ntaps; ++tap) {
        const int zd = row.bd + (tap >> 4), zh = row.bh + ((tap >> 2) & 3), zw = row.bw + (tap & 3);
        const bool inb = mvalid && (unsigned)zd < (unsigned)p.D && (unsigned)zh < (unsigned)p.H && (unsigned)zw < (unsigned)p.W;
        const long long pos = (((long long)row.n * p.D + zd) * p.H + zh) * p.W + zw;
        for (int c0 = 0; c0 < p.Cin; c0 += 32) {
            f32x4 v0 = f32x4{0.f, 0.f, 0.f, 0.f}, v1 = v0;
            if (inb) {
                const float *s = src + pos * p.Cin + c0 + sc;
                v0 = *reinterpret_cast<const f32x4 *>(s);
                v1 = *reinterpret_cast<const f32x4 *>(s + 4);
            }
            const f32x4 wv = *reinterpret_cast<const f32x4 *>(weight + ((long long)tap * p.Cin + c0 + (tid >> 3)) * p.Cout_pad + co0 + (tid & 7) * 4);
            __syncthreads();                                 // the previous tile has been consumed
#pragma unroll
            for (int j = 0; j < 4; ++j) { xs[sc + j][sp] = v0[j]; xs[sc + 4 + j][sp] = v1[j]; }
            *reinterpret_cast<f32x4 *>(&ws[tid >> 3][(tid & 7) * 4]) = wv;
            __syncthreads();
#pragma unroll 8
            for (int ci = 0; ci < 32; ++ci) {
                const float x0 = xs[ci][pq], x1 = xs[ci][pq + 32];
                const f32x4 w = *reinterpret_cast<const f32x4 *>(&ws[ci][cg * 4]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[0][j] = __builtin_fmaf(x0, w[j], acc[0][j]);
                    acc[1][j] = __builtin_fmaf(x1, w[j], acc[1][j]);
                }
            }
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const long long m = m0 + pq + 32 * h;
        if (m >= p.M) continue;
        const int co = co0 + cg * 4;
        *reinterpret_cast<f32x4 *>((float *)p.out + m * p.Cout_pad + co) = patch_epilogue(f32x4{acc[h][0], acc[h][1], acc[h][2], acc[h][3]}, p, co);
    }
}

int patch_fill(PatchParams &p, const char *who, const void *src, const void *weight, const float *alpha, const float *beta, float slope,
               int N, int D, int H, int W, int Cin_pad, int Cout, int kd, int stride, int Do, int Ho, int Wo, void *out, int out_dtype)
{
    if (!src || !weight || !beta || !out) GG_FAIL(GG_ERR_BAD_SHAPE, "%s: null pointer", who);
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cout <= 0) GG_FAIL(GG_ERR_BAD_SHAPE, "%s: empty extent", who);
    if (Cin_pad <= 0 || Cin_pad % 32) GG_FAIL(GG_ERR_BAD_SHAPE, "%s: Cin_pad %d must be a multiple of 32", who, Cin_pad);
    if (kd != 1 && kd != 4) GG_FAIL(GG_ERR_UNSUPPORTED, "%s: kd must be 1 (2-D) or 4, got %d", who, kd);
    if (stride != 1 && stride != 2) GG_FAIL(GG_ERR_UNSUPPORTED, "%s: stride must be 1 or 2, got %d", who, stride);
    if (out_dtype != GG_BF16 && out_dtype != GG_F32) GG_FAIL(GG_ERR_BAD_DTYPE, "%s: out dtype", who);
    // kernel 4, padding 2: floor((e + 4 - 4) / stride) + 1
    if (Do != (kd == 1 ? D : D / stride + 1) || Ho != H / stride + 1 || Wo != W / stride + 1)
        GG_FAIL(GG_ERR_BAD_SHAPE, "%s: output extent (%d,%d,%d) inconsistent with input (%d,%d,%d) kd %d stride %d", who, Do, Ho, Wo, D, H, W, kd, stride);
    p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = Cin_pad; p.Cout = Cout; p.Cout_pad = (Cout + 31) / 32 * 32;
    p.kd = kd; p.stride = stride; p.Do = Do; p.Ho = Ho; p.Wo = Wo; p.out_dtype = out_dtype;
    p.ntaps = kd * 16; p.nchunk = Cin_pad / 32;
    p.M = (long long)N * Do * Ho * Wo;
    p.src = src; p.weight = weight; p.alpha = alpha; p.beta = beta; p.slope = slope; p.out = out;
    if (p.M >= (1LL << 31) || (long long)D * H * W * Cin_pad >= (1LL << 31)) GG_FAIL(GG_ERR_UNSUPPORTED, "%s: tensor too large for 32-bit in-sample offsets", who);
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------------------
// posterior: one thread per (n, s); moments rows fp32 [N * S, stride], mean lanes [0, C), logvar lanes [C, 2C)
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gauss_clamp(float lv) { return fminf(fmaxf(lv, -30.0f), 20.0f); }
// exp rounded to fp32 from the fp64 value: at the upper clamp edge one term is e^20, and an ulp of it is more than a sample's other terms
__device__ __forceinline__ float gauss_exp(float v) { return (float)exp((double)v); }

__global__ __launch_bounds__(LS_THREADS) void gauss_kl_rows_kernel(const float *__restrict__ mom, int stride, int C, long long S,
                                                                   double *__restrict__ partials)
{
#pragma clang fp contract(off)
    __shared__ double lds[LS_THREADS / GG_WAVE];
    const long long n = blockIdx.y;
    double acc = 0.0;
    for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += (long long)gridDim.x * blockDim.x) {
        const float *r = mom + (n * S + s) * stride;
        for (int c = 0; c < C; ++c) {
            const float m = r[c], lv = gauss_clamp(r[C + c]);
            const float t = ((m * m + gauss_exp(lv)) - 1.0f) - lv;          // mean^2 + var - 1.0 - logvar, left to right
            acc += (double)t;
        }
    }
    const double bs = ls_block_sum(acc, lds);
    if (threadIdx.x == 0) partials[n * gridDim.x + blockIdx.x] = bs;
}

template <typename T>
__global__ __launch_bounds__(LS_THREADS) void gauss_sample_rows_kernel(const float *__restrict__ mom, int stride, const float *__restrict__ noise,
                                                                       int N, int C, long long S, float *__restrict__ out, T *__restrict__ z_in,
                                                                       int z_in_stride)
{
#pragma clang fp contract(off)
    const long long total = (long long)N * S;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / S, s = i - n * S;
        const float *r = mom + i * stride;
        for (int c = 0; c < C; ++c) {
            const long long e = (n * C + c) * S + s;
            const float h = 0.5f * gauss_clamp(r[C + c]);
            const float t = gauss_exp(h) * noise[e];
            const float z = r[c] + t;
            if (out) out[e] = z;
            if (z_in) z_in[i * z_in_stride + c] = (T)z;
        }
    }
}

// logits: lane 0 of fp32 rows [M, stride]; partials [blocks][5] = sums of l, relu(1 - l), relu(1 + l), softplus(-l), softplus(l)
__device__ __forceinline__ float softplus_f32(float x) { return x > 20.0f ? x : log1pf(expf(x)); }      // F.softplus, beta 1, threshold 20

__global__ __launch_bounds__(LS_THREADS) void logit_stats_kernel(const float *__restrict__ logits, int stride, long long M, double *__restrict__ partials)
{
#pragma clang fp contract(off)
    __shared__ double lds[LS_THREADS / GG_WAVE];
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (long long)gridDim.x * blockDim.x) {
        const float l = logits[m * stride];
        a[0] += (double)l;
        a[1] += (double)fmaxf(1.0f - l, 0.f);
        a[2] += (double)fmaxf(1.0f + l, 0.f);
        a[3] += (double)softplus_f32(-l);
        a[4] += (double)softplus_f32(l);
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double bs = ls_block_sum(a[k], lds);
        if (threadIdx.x == 0) partials[(long long)blockIdx.x * 5 + k] = bs;
    }
}

}  // namespace

extern "C" int gg_patch_conv_forward(const void *src, const void *weight, const float *alpha, const float *beta, float slope, int32_t N,
                                     int32_t D, int32_t H, int32_t W, int32_t Cin_pad, int32_t Cout, int32_t kd, int32_t stride, int32_t Do,
                                     int32_t Ho, int32_t Wo, void *out, int32_t out_dtype, void *stream_)
{
    PatchParams p;
    if (int rc = patch_fill(p, "patch_conv", src, weight, alpha, beta, slope, N, D, H, W, Cin_pad, Cout, kd, stride, Do, Ho, Wo, out, out_dtype)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int G = p.Cout_pad / 32;
    const unsigned mb = (unsigned)((p.M + 127) / 128);
    if (G % 4 == 0) hipLaunchKernelGGL(patch_conv_kernel<4>, dim3(mb, (unsigned)(G / 4)), dim3(256), 0, stream, p);
    else if (G % 2 == 0) hipLaunchKernelGGL(patch_conv_kernel<2>, dim3(mb, (unsigned)(G / 2)), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(patch_conv_kernel<1>, dim3(mb, (unsigned)G), dim3(256), 0, stream, p);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_patch_conv_forward_f32(const float *src, const float *weight, const float *alpha, const float *beta, float slope, int32_t N,
                                         int32_t D, int32_t H, int32_t W, int32_t Cin_pad, int32_t Cout, int32_t kd, int32_t stride,
                                         int32_t Do, int32_t Ho, int32_t Wo, float *out, void *stream_)
{
    PatchParams p;
    if (int rc = patch_fill(p, "patch_conv_f32", src, weight, alpha, beta, slope, N, D, H, W, Cin_pad, Cout, kd, stride, Do, Ho, Wo, out, GG_F32)) return rc;
    hipLaunchKernelGGL(patch_conv_f32_kernel, dim3((unsigned)((p.M + 63) / 64), (unsigned)(p.Cout_pad / 32)), dim3(256), 0, (hipStream_t)stream_, p);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_gauss_kl_rows(const float *moments, int32_t stride, int32_t N, int32_t C, int64_t S, double *out, void *workspace,
                                int64_t workspace_bytes, void *stream_)
{
    if (!moments || !out || !workspace) GG_FAIL(GG_ERR_BAD_SHAPE, "gauss_kl_rows: null pointer");
    if (N < 1 || N > 65535 || C < 1 || S < 1) GG_FAIL(GG_ERR_BAD_SHAPE, "gauss_kl_rows: N=%d C=%d S=%lld", N, C, (long long)S);
    if (stride < 2 * C) GG_FAIL(GG_ERR_BAD_SHAPE, "gauss_kl_rows: row stride %d < 2 * C = %d", stride, 2 * C);
    const int blocks = ls_blocks(S);
    if (workspace_bytes < (int64_t)N * blocks * (int64_t)sizeof(double))
        GG_FAIL(GG_ERR_WORKSPACE_TOO_SMALL, "gauss_kl_rows: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)N * blocks * 8);
    hipStream_t stream = (hipStream_t)stream_;
    double *ws = (double *)workspace;
    hipLaunchKernelGGL(gauss_kl_rows_kernel, dim3((unsigned)blocks, (unsigned)N), dim3(LS_THREADS), 0, stream, moments, stride, C, (long long)S, ws);
    hipLaunchKernelGGL(ls_finish_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, stream, (const double *)ws, N, 1, blocks, 0.5, out);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_gauss_sample_rows(const float *moments, int32_t stride, const float *noise, int32_t N, int32_t C, int64_t S, float *out,
                                    void *z_in, int32_t z_in_dtype, int32_t z_in_stride, void *stream_)
{
    if (!moments || !noise) GG_FAIL(GG_ERR_BAD_SHAPE, "gauss_sample_rows: null pointer");
    if (!out && !z_in) GG_FAIL(GG_ERR_BAD_SHAPE, "gauss_sample_rows: no output");
    if (N < 1 || C < 1 || S < 1) GG_FAIL(GG_ERR_BAD_SHAPE, "gauss_sample_rows: N=%d C=%d S=%lld", N, C, (long long)S);
    if (stride < 2 * C) GG_FAIL(GG_ERR_BAD_SHAPE, "gauss_sample_rows: row stride %d < 2 * C = %d", stride, 2 * C);
    if (z_in && z_in_stride < C) GG_FAIL(GG_ERR_BAD_SHAPE, "gauss_sample_rows: z_in_stride %d < C=%d", z_in_stride, C);
    if (z_in && z_in_dtype != GG_BF16 && z_in_dtype != GG_F32) GG_FAIL(GG_ERR_BAD_DTYPE, "gauss_sample_rows: z_in dtype");
    const unsigned blocks = gg_blocks256((long long)N * S, 4096);
    hipStream_t stream = (hipStream_t)stream_;
    if (z_in && z_in_dtype == GG_F32)
        hipLaunchKernelGGL(gauss_sample_rows_kernel<float>, dim3(blocks), dim3(LS_THREADS), 0, stream, moments, stride, noise, N, C, (long long)S, out,
                           (float *)z_in, z_in_stride);
    else
        hipLaunchKernelGGL(gauss_sample_rows_kernel<bf16_t>, dim3(blocks), dim3(LS_THREADS), 0, stream, moments, stride, noise, N, C, (long long)S, out,
                           (bf16_t *)z_in, z_in_stride);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_logit_stats(const float *logits, int32_t stride, int64_t M, double *out, void *workspace, int64_t workspace_bytes, void *stream_)
{
    if (!logits || !out || !workspace) GG_FAIL(GG_ERR_BAD_SHAPE, "logit_stats: null pointer");
    if (M < 1 || stride < 1) GG_FAIL(GG_ERR_BAD_SHAPE, "logit_stats: M=%lld stride=%d", (long long)M, stride);
    const int blocks = ls_blocks(M);
    if (workspace_bytes < (int64_t)blocks * 5 * (int64_t)sizeof(double))
        GG_FAIL(GG_ERR_WORKSPACE_TOO_SMALL, "logit_stats: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)blocks * 40);
    hipStream_t stream = (hipStream_t)stream_;
    double *ws = (double *)workspace;
    hipLaunchKernelGGL(logit_stats_kernel, dim3((unsigned)blocks), dim3(LS_THREADS), 0, stream, logits, stride, (long long)M, ws);
    hipLaunchKernelGGL(ls_finish_kernel, dim3(1), dim3(64), 0, stream, (const double *)ws, 5, 5, blocks, 1.0 / (double)M, out);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
