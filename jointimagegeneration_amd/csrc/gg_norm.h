// GroupNorm(32) and LayerNorm arithmetic, each formula written once.  fp32 unless said otherwise; products and sums contract to FMAs as
// the compiler likes (tests/norm_exact.py uses inputs on which either rounding gives the same bits).
// Callers: every kernel of gg_norm.hip; resample2x_kernel (gg_resample.hip); layernorm_rows_kernel (gg_cond.hip); the statistics epilogues
// of gg_conv.hip, gg_conv_halo.hip, gg_conv_halo3.hip and gg_conv_box_kernel.h, and the accumulator prologue of gg_conv_box_kernel.h.
// A function is optimised on its own before it is inlined, so a call can cost a kernel another instruction order or another multiply
// than the same text in place.  Where it did, the site keeps the text and names the function in a comment (three sites in gg_norm.hip,
// gn_f32_stats_kernel in gg_f32.hip, the accumulator addresses of the four conv epilogues, the moments of the box conv's prologue).
#pragma once
#include "gg_conv.h"

typedef __attribute__((ext_vector_type(2))) long long i64x2;

// (sum, sumsq, count) -> mean, rstd = 1 / sqrt(max(sumsq / cnt - mean^2, 0) + eps), in fp64.  fast: 1 / cnt as the fp32 reciprocal + one
// Newton step in fp64 (error ~1e-14: mean^2 is not polluted when |mean| >> std) and v_rsq_f32 -- an fp64 division or square root is a
// 50-100-instruction sequence on the critical path of a launch-bound kernel.  ieee: fp64 division and square root.
__device__ __forceinline__ void gn_moments_fast(double sum, double sumsq, double cnt, float eps, float &mean, float &rstd)
{
    double inv = (double)(1.0f / (float)cnt);
    inv = inv * (2.0 - cnt * inv);
    const double m = sum * inv;
    double var = sumsq * inv - m * m;
    if (var < 0.0) var = 0.0;
    mean = (float)m;
    rstd = rsqrtf((float)var + eps);
}
__device__ __forceinline__ void gn_moments_ieee(double sum, double sumsq, double cnt, float eps, float &mean, float &rstd)
{
    const double m = sum / cnt;
    double var = sumsq / cnt - m * m;
    if (var < 0.0) var = 0.0;
    mean = (float)m;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
}

// y = x * scale + shift with scale = rstd * gamma, shift = beta - mean * scale (two functions: a kernel that tabulates the pair stores
// the scale before it needs beta); SiLU (gg_silu) of y if act.  gn_affine8: channels c0 .. c0 + 7, coefficients as 16-byte halves.
__device__ __forceinline__ float gn_scale(float rstd, float gamma) { return rstd * gamma; }
__device__ __forceinline__ float gn_shift(float beta, float mean, float scale) { return beta - mean * scale; }
__device__ __forceinline__ float gn_lin(float x, float scale, float shift) { return x * scale + shift; }
__device__ __forceinline__ float gn_affine(float x, float scale, float shift, int act)
{
    float y = gn_lin(x, scale, shift);
    if (act) y = gg_silu(y);
    return y;
}
__device__ __forceinline__ bf16x8 gn_affine8(bf16x8 v, f32x4 sc0, f32x4 sc1, f32x4 sh0, f32x4 sh1, int act)
{
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float y0 = gn_lin((float)v[j], sc0[j], sh0[j]), y1 = gn_lin((float)v[j + 4], sc1[j], sh1[j]);
        if (act) { y0 = gg_silu(y0); y1 = gg_silu(y1); }
        o[j] = (bf16_t)y0;
        o[j + 4] = (bf16_t)y1;
    }
    return o;
}

// channel c0 of row `row` of cat[s1 (C1 channels), s2 (C2 channels)]; I: the type of the element offsets (unsigned where the host gates
// on < 2^31 elements)
template <class I, class T>
__device__ __forceinline__ const T *gn_piece_ptr(const T *s1, int C1, const T *s2, int C2, I row, int c0)
{ return (c0 >= C1) ? s2 + row * (I)C2 + (I)(c0 - C1) : s1 + row * (I)C1 + (I)c0; }

// coefficient tables [N][C] keep zeros in the lanes >= C_logical: row n, by the 256 threads of a block
__device__ __forceinline__ void gn_zero_pad_lanes(float *scale, float *shift, int n, int C, int C_logical, int tid)
{
    for (int c = C_logical + tid; c < C; c += 256) { scale[(long long)n * C + c] = 0.f; shift[(long long)n * C + c] = 0.f; }
}

// x + (x of the DPP-selected lane) in fp64: two DPP moves + one add, no LDS round trip (a 64-bit __shfl_xor is two ds_bpermute, ~150 cycles
// of dependent latency per butterfly step: six steps were ~0.4 us of a 3.4 us kernel)
template <int CTRL>
__device__ __forceinline__ double gg_dpp_add_f64(double x)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)u, CTRL, 0xF, 0xF, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)(u >> 32), CTRL, 0xF, 0xF, true);
    return x + __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// sum over the 64 lanes of a wave, fixed order (deterministic): the 16 lanes of a row by DPP (quad xor 1, quad xor 2, half-row mirror,
// row mirror), the four rows by two xor shuffles
__device__ __forceinline__ double gg_wave_sum_f64(double x)
{
    x = gg_dpp_add_f64<0xB1>(x);
    x = gg_dpp_add_f64<0x4E>(x);
    x = gg_dpp_add_f64<0x141>(x);
    x = gg_dpp_add_f64<0x140>(x);
    x += __shfl_xor(x, 16);
    x += __shfl_xor(x, 32);
    return x;
}
// (sum, sumsq) of a 256-thread block's fp32 partials, to every thread: the fp64 butterfly inside each wave, then the 4 waves through LDS
// in a fixed order: one barrier, not eight
__device__ __forceinline__ void gn_block_sum2_f64(float a, float b, double &sa, double &sb)
{
    const int tid = threadIdx.x;
    const double da = gg_wave_sum_f64((double)a), db = gg_wave_sum_f64((double)b);
    __shared__ double ra[4], rb[4];
    if ((tid & 63) == 0) { ra[tid >> 6] = da; rb[tid >> 6] = db; }
    __syncthreads();
    sa = (ra[0] + ra[1]) + (ra[2] + ra[3]);
    sb = (rb[0] + rb[1]) + (rb[2] + rb[3]);
}

// Accumulators: per-channel fixed-point (sum, sumsq) left by the conv epilogues, [N][stripes][C][2] int64, scales in gg_conv.h.
// gn_acc_index: element (n, stripe, c, which), which = 0 sum, 1 sumsq.  gn_acc_from_f32: a conv's fp32 partial -> fixed point.
// gn_acc_fold_channel: adds one channel's GG_ACC_STRIPES stripes to sum / sumsq (q: its entry of stripe 0, cs: the stripe pitch, 2 * C).
__device__ __forceinline__ long long gn_acc_index(long long n, int stripes, int stripe, int C, int c, int which = 0) { return ((n * stripes + stripe) * C + c) * 2 + which; }
__device__ __forceinline__ long long gn_acc_from_f32(float t, int which) { return __double2ll_rn((double)t * (double)(which ? GG_ACC_SQ_SCALE : GG_ACC_SUM_SCALE)); }
__device__ __forceinline__ double gn_acc_to_f64(long long fx, int which) { return (double)fx * (which ? 1.0 / (double)GG_ACC_SQ_SCALE : 1.0 / (double)GG_ACC_SUM_SCALE); }
__device__ __forceinline__ void gn_acc_fold_channel(const long long *q, long long cs, long long &sum, long long &sumsq)
{
#pragma unroll
    for (int st = 0; st < GG_ACC_STRIPES; ++st) { const i64x2 v = *reinterpret_cast<const i64x2 *>(q + st * cs); sum += v[0]; sumsq += v[1]; }
}

// LayerNorm: the wave's sum by the xor butterfly, and the normalise step
__device__ __forceinline__ float gg_wave_sum_f32(float x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
__device__ __forceinline__ float ln_normalise(float x, float mean, float rstd, float gamma, float beta) { return (x - mean) * rstd * gamma + beta; }
