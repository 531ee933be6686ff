// Shared device/host helpers for libguidegen_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/guidegen_hip.h"

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) float f32x8;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

#define GG_WAVE 64

// thread-local error message (error convention)
void gg_set_error(const char *fmt, ...);

#define GG_FAIL(code, ...)            \
    do {                              \
        gg_set_error(__VA_ARGS__);    \
        return (code);                \
    } while (0)

#define GG_CHECK_LAUNCH()                                                              \
    do {                                                                               \
        hipError_t e_ = hipGetLastError();                                             \
        if (e_ != hipSuccess) GG_FAIL(GG_ERR_HIP, "HIP launch: %s", hipGetErrorString(e_)); \
    } while (0)

// Kernel arguments reach a wave through scalar loads from the kernarg segment, and the compiler sinks each load to its first use: a
// kernel that touches its arguments in four places pays four SERIAL scalar round trips before its first memory instruction.
// gg_pin launders a wave-uniform value through an SGPR: the pinned arguments are fetched in one batch where the pins stand and
// cannot be re-materialised from the kernarg segment later.  (Pin only what the first memory instructions need: pinning all ~50
// dwords of a conv descriptor raised the SGPR pressure and was slower.)
template <class T>
__device__ __forceinline__ T gg_pin(T v)
{
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "gg_pin: 32- or 64-bit scalars");
    if constexpr (sizeof(T) == 4) {
        unsigned u = __builtin_bit_cast(unsigned, v);
        asm volatile("" : "+s"(u));
        return __builtin_bit_cast(T, u);
    } else {
        unsigned long long u = __builtin_bit_cast(unsigned long long, v);
        asm volatile("" : "+s"(u));
        return __builtin_bit_cast(T, u);
    }
}

// Weights of the latent UNet's batch-1 convs are read ONCE per forward (535 MB per forward against 8 x 4 MB of L2 and 256 MB of MALL):
// loaded with the default policy they evict the activations, accumulators and parameters the NEXT kernels are about to read.
// GG_STREAM_LOAD marks them non-temporal (measured: tools/experiments/README.md, "non-temporal weight loads").
#ifndef GG_STREAM_WEIGHTS
#define GG_STREAM_WEIGHTS 1
#endif
#if GG_STREAM_WEIGHTS
#define GG_STREAM_LOAD(P) __builtin_nontemporal_load(P)
#else
#define GG_STREAM_LOAD(P) (*(P))
#endif

// Integer division is a ~30 (32-bit) to ~150 (64-bit) instruction sequence on this ISA, and a wave issues its instructions one by
// one: in the launch-bound kernels of the latent UNet an index division IS microseconds.
// gg_fastdiv: n / d through one multiply-high; exact for 0 <= n, n * d < 2^32 (gg_magic_u32 returns 0 when that does not hold or
// d == 1: plain division then).  gg_div_small: n / d for 0 <= n < 2^21 through the fp32 reciprocal (rcp = v_rcp_f32 of d, 1 ulp).
__device__ __forceinline__ long long gg_fastdiv(long long n, int d, unsigned magic)
{
    return magic ? (long long)__umulhi((unsigned)n, magic) : n / d;
}
__device__ __forceinline__ int gg_div_small(int n, float rcp) { return (int)(((float)n + 0.5f) * rcp); }
static inline unsigned gg_magic_u32(long long nmax, int d)
{
    return (d > 1 && nmax * (long long)d < (1LL << 32)) ? (unsigned)(((1ULL << 32) + (unsigned)d - 1) / (unsigned)d) : 0u;
}

// SiLU with the hardware exp2 and reciprocal (v_exp_f32, v_rcp_f32: 1 ulp each), the one definition every bf16 site calls (GroupNorm
// kernels, resample, every conv staging pass): an IEEE division is ~10 VALU instructions per element, 16 elements per thread in the
// launch-bound GroupNorm kernels.
// Written as (y / 2) * rcp((1 + exp(-y)) / 2): v_rcp_f32 flushes a subnormal RESULT to zero, so y * rcp(1 + exp(-y)) returned 0 once
// exp(-y) passed 2^126 (y = -87.5: SiLU = -8.7e-37, a normal number; found by the exhaustive sweep of tests/test_act_sweep_gpu.py).
// With the halves the reciprocal stays normal up to exp(-y) < 2^127 (y > -88.03; below that |SiLU| < 5.3e-37).  Every other result is,
// bit for bit, that of the plain form: the exponential is the same instruction pair, fma(e, 0.5, 0.5) is round(1 + e) / 2 exactly,
// and a power of two moves through the reciprocal and the products without touching a rounding (only y below 2^-125 can lose a bit
// in y / 2; q * (-2 log2 e) below rounds as y * (-log2 e) does in __expf(-y)).  gg_silu is one multiply longer than the plain form.
// gg_silu_of_half takes q = y / 2 and is as long as the plain form: a staging pass whose scale / shift stay in registers over many
// elements halves them once, x * (scale / 2) + shift / 2 is y / 2 exactly, and every result equals gg_silu(y) bit for bit.
__device__ __forceinline__ float gg_silu_of_half(float q)
{
    const float half_d = fmaf(__builtin_amdgcn_exp2f(q * (-2.0f * 1.4426950408889634f)), 0.5f, 0.5f);      // (1 + exp(-y)) / 2
    return q * __builtin_amdgcn_rcpf(half_d);
}
__device__ __forceinline__ float gg_silu(float y) { return gg_silu_of_half(0.5f * y); }

__device__ __forceinline__ f32x8 gg_bf16x8_to_f32(bf16x8 v)
{
    f32x8 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = (float)v[i];
    return r;
}
__device__ __forceinline__ bf16x8 gg_f32_to_bf16x8(f32x8 v)
{
    bf16x8 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = (bf16_t)v[i];
    return r;
}

static inline int gg_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// Host side of the pointwise LDM steps (gg_sampler.hip, for gg_vq.hip's codebook-free step): one launch of the per-element DDIM
// (ancestral == 0) or ancestral update over [M, C] rows, the noise coefficient read from scalars[noise_idx].  No argument checks: the
// extern "C" entries do theirs and then call this.
int gg_step_launch(int ancestral, float *x, const float *out, int out_stride, const float *noise, const float *scalars_dev, int noise_idx,
                   int flags, long long M, int C, float *pred_x0_out, void *unet_in, int unet_in_stride, hipStream_t stream);

// grid of a grid-stride kernel with 256 threads per block: one thread per unit of work, at most cap blocks (0 when there is no work)
static inline unsigned gg_blocks256(long long work, long long cap)
{
    const long long blocks = work > 0 ? (work + 255) / 256 : 0;
    return (unsigned)(blocks > cap ? cap : blocks);
}
