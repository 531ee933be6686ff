// Conv-free 2x resampling and the ResBlock FiLM coefficient fold (include/guidegen_hip.h "resampling / FiLM").
//
//   resample2x_kernel   nearest x2 upsample (F.interpolate(mode="nearest")) or 2x average pool (nn.AvgPool{2,3}d(2)) of a channels-last
//                       [N, D, H, W, Cpad] tensor, H and W always, D too for 3-D networks (unet.py:85-145; the reference's Downsample uses
//                       stride (2, 2, 2) when dims == 3).  Optional per-(n, c) x * scale + shift (+ SiLU) prologue applied to every input
//                       element before pooling: the h path of a down ResBlock, avgpool(SiLU(GN(x))), in one launch.
//   film_fold_kernel    scale' = scale * (1 + s), shift' = shift * (1 + s) + t for the ResBlock's per-sample FiLM row [s | t] (unet.py:254-257)
//
// Memory-bound: one thread per output position and 8 channels, 16-byte channel vectors (bf16; two per fp32 vector), fp32 arithmetic.
#include "gg_norm.h"

template <class T> struct Vec8;
template <> struct Vec8<bf16_t> {
    static __device__ __forceinline__ f32x8 load(const bf16_t *p) { return gg_bf16x8_to_f32(*reinterpret_cast<const bf16x8 *>(p)); }
    static __device__ __forceinline__ void store(bf16_t *p, f32x8 v) { *reinterpret_cast<bf16x8 *>(p) = gg_f32_to_bf16x8(v); }
};
template <> struct Vec8<float> {
    static __device__ __forceinline__ f32x8 load(const float *p)
    {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(p), b = *reinterpret_cast<const f32x4 *>(p + 4);
        f32x8 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) { r[i] = a[i]; r[i + 4] = b[i]; }
        return r;
    }
    static __device__ __forceinline__ void store(float *p, f32x8 v)
    {
        f32x4 a, b;
#pragma unroll
        for (int i = 0; i < 4; ++i) { a[i] = v[i]; b[i] = v[i + 4]; }
        *reinterpret_cast<f32x4 *>(p) = a;
        *reinterpret_cast<f32x4 *>(p + 4) = b;
    }
};

// mode 0: nearest upsample, output (od, oh, ow) reads input (od >> rd, oh >> 1, ow >> 1).
// mode 1: average pool, output (od, oh, ow) averages the 2 x 2 (x 2) block at (od << rd, oh << 1, ow << 1); the sum runs in fp32 in a
// fixed order and is multiplied by 1/4 or 1/8 (exact).  Channels >= C_logical are written as zeros (the pad-lane invariant).
template <class T, int MODE>
__global__ __launch_bounds__(256) void resample2x_kernel(const T *__restrict__ src, int D, int H, int W, int Cpad, int C_logical, int rd,
                                                         int Do, int Ho, int Wo, long long total, const float *__restrict__ scale,
                                                         const float *__restrict__ shift, int act, T *__restrict__ dst)
{
    const int P = Cpad >> 3;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long pos = i / P;                       // output position over N * Do * Ho * Wo
        const int c0 = (int)(i - pos * P) * 8;
        long long r = pos;
        const int ow = (int)(r % Wo); r /= Wo;
        const int oh = (int)(r % Ho); r /= Ho;
        const int od = (int)(r % Do);
        const int n = (int)(r / Do);
        f32x8 a = {}, b = {};
        if (scale) {
            const float *sc = scale + (long long)n * Cpad + c0, *sh = shift + (long long)n * Cpad + c0;
            a = Vec8<float>::load(sc);
            b = Vec8<float>::load(sh);
        }
        auto pro = [&](f32x8 v) {
            if (scale) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = gn_affine(v[j], a[j], b[j], act);
            }
            return v;
        };
        f32x8 o;
        if (MODE == 0) {
            const long long ip = (((long long)n * D + (od >> rd)) * H + (oh >> 1)) * W + (ow >> 1);
            o = pro(Vec8<T>::load(src + ip * Cpad + c0));
        } else {
            const int nd = rd ? 2 : 1;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = 0.f;
            for (int dz = 0; dz < nd; ++dz)
#pragma unroll
                for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        const long long ip = (((long long)n * D + ((od << rd) + dz)) * H + (oh * 2 + dy)) * W + (ow * 2 + dx);
                        o += pro(Vec8<T>::load(src + ip * Cpad + c0));
                    }
            const float inv = rd ? 0.125f : 0.25f;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] *= inv;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (c0 + j >= C_logical) o[j] = 0.f;
        Vec8<T>::store(dst + pos * Cpad + c0, o);
    }
}

extern "C" int gg_resample2x(const void *src, int32_t dtype, int32_t N, int32_t D, int32_t H, int32_t W, int32_t C_pad, int32_t C_logical,
                             int32_t resample_d, int32_t mode, const float *scale, const float *shift, int32_t act, void *dst, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (dtype != GG_BF16 && dtype != GG_F32) GG_FAIL(GG_ERR_BAD_DTYPE, "resample2x: dtype must be GG_BF16 or GG_F32");
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0) GG_FAIL(GG_ERR_BAD_SHAPE, "resample2x: empty tensor");
    if (C_pad <= 0 || C_pad % 32) GG_FAIL(GG_ERR_BAD_SHAPE, "resample2x: C_pad %d must be a positive multiple of 32", C_pad);
    if (C_logical <= 0 || C_logical > C_pad) GG_FAIL(GG_ERR_BAD_SHAPE, "resample2x: logical channels %d outside (0, %d]", C_logical, C_pad);
    if (mode != 0 && mode != 1) GG_FAIL(GG_ERR_BAD_SHAPE, "resample2x: mode must be 0 (nearest up) or 1 (average pool)");
    if (resample_d != 0 && resample_d != 1) GG_FAIL(GG_ERR_BAD_SHAPE, "resample2x: resample_d must be 0 or 1");
    if (!src || !dst || (!scale) != (!shift)) GG_FAIL(GG_ERR_BAD_SHAPE, "resample2x: null pointer (scale and shift go together)");
    if (mode == 1 && (H % 2 || W % 2 || (resample_d && D % 2)))
        GG_FAIL(GG_ERR_UNSUPPORTED, "resample2x: average pool of odd extents (%d, %d, %d) is not supported", resample_d ? D : 2, H, W);
    const int Do = mode == 0 ? (resample_d ? 2 * D : D) : (resample_d ? D / 2 : D);
    const int Ho = mode == 0 ? 2 * H : H / 2, Wo = mode == 0 ? 2 * W : W / 2;
    const long long total = (long long)N * Do * Ho * Wo * (C_pad / 8);
    const unsigned blocks = gg_blocks256(total, 16384);
    const dim3 g(blocks), b(256);
    if (dtype == GG_BF16) {
        const bf16_t *s = (const bf16_t *)src;
        bf16_t *o = (bf16_t *)dst;
        if (mode == 0) hipLaunchKernelGGL((resample2x_kernel<bf16_t, 0>), g, b, 0, stream, s, D, H, W, C_pad, C_logical, resample_d, Do, Ho, Wo, total, scale, shift, act, o);
        else hipLaunchKernelGGL((resample2x_kernel<bf16_t, 1>), g, b, 0, stream, s, D, H, W, C_pad, C_logical, resample_d, Do, Ho, Wo, total, scale, shift, act, o);
    } else {
        const float *s = (const float *)src;
        float *o = (float *)dst;
        if (mode == 0) hipLaunchKernelGGL((resample2x_kernel<float, 0>), g, b, 0, stream, s, D, H, W, C_pad, C_logical, resample_d, Do, Ho, Wo, total, scale, shift, act, o);
        else hipLaunchKernelGGL((resample2x_kernel<float, 1>), g, b, 0, stream, s, D, H, W, C_pad, C_logical, resample_d, Do, Ho, Wo, total, scale, shift, act, o);
    }
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------------------ FiLM fold
// One thread per (n, c < C): s = film[n, c], t = film[n, C + c].  Pad lanes c >= C keep their (zero) coefficients.
__global__ __launch_bounds__(256) void film_fold_kernel(float *__restrict__ scale, float *__restrict__ shift, int coef_stride, int N, int C,
                                                        const float *__restrict__ film, long long film_stride)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N * C) return;
    const int n = i / C, c = i - n * C;
    const float s1 = 1.0f + film[n * film_stride + c], t = film[n * film_stride + C + c];
    const long long k = (long long)n * coef_stride + c;
    scale[k] = scale[k] * s1;
    shift[k] = __builtin_fmaf(shift[k], s1, t);
}

extern "C" int gg_film_fold(float *scale, float *shift, int32_t coef_stride, int32_t N, int32_t C, const float *film, int64_t film_stride,
                            void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (N <= 0 || C <= 0 || coef_stride < C || film_stride < 2LL * C) GG_FAIL(GG_ERR_BAD_SHAPE, "film_fold: bad N / C / strides");
    if (!scale || !shift || !film) GG_FAIL(GG_ERR_BAD_SHAPE, "film_fold: null pointer");
    hipLaunchKernelGGL(film_fold_kernel, dim3((unsigned)gg_cdiv((int64_t)N * C, 256)), dim3(256), 0, stream, scale, shift, coef_stride, N, C,
                       film, (long long)film_stride);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
