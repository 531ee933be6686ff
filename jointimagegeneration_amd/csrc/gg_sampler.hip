// Sampler-side kernels: CCDM fused posterior+sample, DDIM update, layout movers, small fp32 linears.
#include "gg_common.h"
#include "gg_posterior.h"
#include "gg_step.h"

// ------------------------------------------------------------------------------------------------------------
// CCDM reverse step, one voxel per thread (gg_posterior.h holds the arithmetic).
// ------------------------------------------------------------------------------------------------------------
// PS: ccdm_key_row's (0: the single key `seed`; 1: one key per sample of rows_per_sample rows).
template <int KMAX, int KS = 0, int PS = 0>
__global__ __launch_bounds__(256) void ccdm_posterior_kernel(const float *__restrict__ head, int head_stride, int is_logits,
                                                             const int *__restrict__ xt, const float *__restrict__ E,
                                                             uint64_t seed, const long long *__restrict__ offset_dev, int draw,
                                                             const float *__restrict__ scalars, int K, long long M,
                                                             int *__restrict__ labels_out, float *__restrict__ probs_out,
                                                             bf16_t *__restrict__ onehot_out, int onehot_stride,
                                                             const unsigned long long *__restrict__ seeds, long long rows_per_sample)
{
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    float p0[KMAX];
    const float *hp = head + m * head_stride;
#pragma unroll
    for (int c = 0; c < KMAX; ++c) p0[c] = (c < (KS > 0 ? KS : K)) ? hp[c] : 0.f;
    const long long off = (draw && !E && offset_dev) ? offset_dev[0] : 0;
    uint64_t key;
    long long row;
    ccdm_key_row<PS>(seed, seeds, rows_per_sample, m, key, row);
    const int best = ccdm_posterior_voxel<KMAX, KS>(p0, is_logits, xt[m], scalars[0], scalars[1], K, row, draw, E ? E + m * K : nullptr, key, off,
                                                probs_out ? probs_out + m * K : nullptr);
    labels_out[m] = best;
    if (onehot_out) ccdm_onehot_row<KMAX, KS>(onehot_out + m * onehot_stride, best, K);
}

template <int PS>
static int ccdm_posterior_launch(const float *head, int32_t head_stride, int32_t head_is_logits, const int32_t *xt, const float *E,
                                 uint64_t philox_seed, const int64_t *philox_offset_dev, int32_t draw, const float *scalars_dev, int32_t K,
                                 int64_t M, int32_t *labels_out, float *probs_out, void *onehot_out, int32_t onehot_stride,
                                 const uint64_t *seeds, int64_t rows_per_sample, hipStream_t stream)
{
    if (!head || !xt || !scalars_dev || !labels_out) GG_FAIL(GG_ERR_BAD_SHAPE, "ccdm_posterior_sample: null pointer");
    if (K < 2 || K > 32) GG_FAIL(GG_ERR_UNSUPPORTED, "ccdm_posterior_sample: K=%d outside [2, 32]", K);
    if (head_stride < K) GG_FAIL(GG_ERR_BAD_SHAPE, "ccdm_posterior_sample: head_stride < K");
    // no least row count: M <= 0 is an empty launch, below
    if (int rc = ccdm_check_rows("ccdm_posterior_sample", M, INT64_MIN, PS ? rows_per_sample : 1, K, onehot_out, onehot_stride)) return rc;
    if (M <= 0) return GG_OK;
    const unsigned long long *sd = (const unsigned long long *)seeds;
    dim3 grid((unsigned)((M + 255) / 256));
    if (K == 14)        // the class count of the shipped configs (13 organs + background), compiled in
        hipLaunchKernelGGL((ccdm_posterior_kernel<16, 14, PS>), grid, dim3(256), 0, stream, head, head_stride, head_is_logits, xt, E,
                           philox_seed, (const long long *)philox_offset_dev, draw, scalars_dev, K, (long long)M, labels_out,
                           probs_out, (bf16_t *)onehot_out, onehot_stride, sd, (long long)rows_per_sample);
    else if (K <= 16)
        hipLaunchKernelGGL((ccdm_posterior_kernel<16, 0, PS>), grid, dim3(256), 0, stream, head, head_stride, head_is_logits, xt, E,
                           philox_seed, (const long long *)philox_offset_dev, draw, scalars_dev, K, (long long)M, labels_out,
                           probs_out, (bf16_t *)onehot_out, onehot_stride, sd, (long long)rows_per_sample);
    else
        hipLaunchKernelGGL((ccdm_posterior_kernel<32, 0, PS>), grid, dim3(256), 0, stream, head, head_stride, head_is_logits, xt, E,
                           philox_seed, (const long long *)philox_offset_dev, draw, scalars_dev, K, (long long)M, labels_out,
                           probs_out, (bf16_t *)onehot_out, onehot_stride, sd, (long long)rows_per_sample);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_ccdm_posterior_sample(const float *head, int32_t head_stride, int32_t head_is_logits, const int32_t *xt,
                                        const float *E, uint64_t philox_seed, const int64_t *philox_offset_dev, int32_t draw,
                                        const float *scalars_dev, int32_t K, int64_t M, int32_t *labels_out, float *probs_out,
                                        void *onehot_out, int32_t onehot_stride, void *stream_)
{
    return ccdm_posterior_launch<0>(head, head_stride, head_is_logits, xt, E, philox_seed, philox_offset_dev, draw, scalars_dev, K, M,
                                    labels_out, probs_out, onehot_out, onehot_stride, nullptr, 0, (hipStream_t)stream_);
}

extern "C" int gg_ccdm_posterior_sample_seeds(const float *head, int32_t head_stride, int32_t head_is_logits, const int32_t *xt,
                                              const float *E, const uint64_t *philox_seeds_dev, int64_t rows_per_sample,
                                              const int64_t *philox_offset_dev, int32_t draw, const float *scalars_dev, int32_t K, int64_t M,
                                              int32_t *labels_out, float *probs_out, void *onehot_out, int32_t onehot_stride, void *stream_)
{
    if (!philox_seeds_dev) GG_FAIL(GG_ERR_BAD_SHAPE, "ccdm_posterior_sample_seeds: null seeds");
    if (int rc = ccdm_check_rows("ccdm_posterior_sample_seeds", M, INT64_MIN, rows_per_sample, K, nullptr, 0)) return rc;
    return ccdm_posterior_launch<1>(head, head_stride, head_is_logits, xt, E, 0, philox_offset_dev, draw, scalars_dev, K, M, labels_out,
                                    probs_out, onehot_out, onehot_stride, philox_seeds_dev, rows_per_sample, (hipStream_t)stream_);
}

// The tape of a Philox run, one row per thread: the words and exponentials ccdm_draw_row gives row m under ccdm_key_row's rule (seeds !=
// nullptr: the per-sample one), or with bits_in the exponentials of those words instead.
template <int KMAX>
__global__ __launch_bounds__(256) void ccdm_draw_tape_kernel(uint64_t seed, const unsigned long long *__restrict__ seeds, long long rows_per_sample,
                                                             const long long *__restrict__ offset_dev, long long M,
                                                             const uint32_t *__restrict__ bits_in, uint32_t *__restrict__ bits_out,
                                                             float *__restrict__ E_out)
{
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    uint32_t w[KMAX];
    float Ev[KMAX];
    if (bits_in) {
#pragma unroll
        for (int c = 0; c < KMAX; ++c) { w[c] = bits_in[m * KMAX + c]; Ev[c] = ccdm_word_to_exp(w[c]); }
    } else {
        uint64_t key;
        long long row;
        if (seeds) ccdm_key_row<1>(seed, seeds, rows_per_sample, m, key, row);
        else ccdm_key_row<0>(seed, seeds, rows_per_sample, m, key, row);
        ccdm_draw_row<KMAX>(Ev, key, row, offset_dev ? offset_dev[0] : 0, w);
    }
#pragma unroll
    for (int c = 0; c < KMAX; ++c) {
        if (bits_out) bits_out[m * KMAX + c] = w[c];
        if (E_out) E_out[m * KMAX + c] = Ev[c];
    }
}

extern "C" int gg_ccdm_draw_tape(uint64_t philox_seed, const uint64_t *philox_seeds_dev, int64_t rows_per_sample,
                                 const int64_t *philox_offset_dev, int32_t kmax, int64_t M, const uint32_t *bits_in, uint32_t *bits_out,
                                 float *E_out, void *stream_)
{
    if (!bits_out && !E_out) GG_FAIL(GG_ERR_BAD_SHAPE, "ccdm_draw_tape: no output");
    if (kmax != 16 && kmax != 32) GG_FAIL(GG_ERR_UNSUPPORTED, "ccdm_draw_tape: kmax=%d is neither 16 nor 32", kmax);
    if (M < 0) GG_FAIL(GG_ERR_BAD_SHAPE, "ccdm_draw_tape: M=%lld", (long long)M);
    if (philox_seeds_dev && !bits_in && (rows_per_sample <= 0 || M % rows_per_sample))
        GG_FAIL(GG_ERR_BAD_SHAPE, "ccdm_draw_tape: M=%lld is not a multiple of rows_per_sample=%lld", (long long)M, (long long)rows_per_sample);
    if (M == 0) return GG_OK;
    const long long blocks = (M + 255) / 256;
    if (blocks > 0x7fffffffLL) GG_FAIL(GG_ERR_UNSUPPORTED, "ccdm_draw_tape: M=%lld rows exceed the grid", (long long)M);
    const unsigned long long *sd = (const unsigned long long *)philox_seeds_dev;
    if (kmax == 16)
        hipLaunchKernelGGL(ccdm_draw_tape_kernel<16>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, philox_seed, sd,
                           (long long)rows_per_sample, (const long long *)philox_offset_dev, (long long)M, bits_in, bits_out, E_out);
    else
        hipLaunchKernelGGL(ccdm_draw_tape_kernel<32>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, philox_seed, sd,
                           (long long)rows_per_sample, (const long long *)philox_offset_dev, (long long)M, bits_in, bits_out, E_out);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

__global__ __launch_bounds__(256) void labels_to_onehot_kernel(const int *__restrict__ labels, long long M, int K,
                                                               bf16_t *__restrict__ out, int stride)
{
    // one thread per (voxel, 8-channel piece): writes the full padded row (zeros beyond K)
    const int P = stride >> 3;
    const long long total = M * P;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        long long m = i / P;
        int c0 = (int)(i - m * P) * 8;
        int lab = labels[m];
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (bf16_t)((c0 + j == lab && c0 + j < K) ? 1.0f : 0.0f);
        *reinterpret_cast<bf16x8 *>(out + m * stride + c0) = o;
    }
}

extern "C" int gg_labels_to_onehot(const int32_t *labels, int64_t M, int32_t K, void *onehot_out, int32_t stride, void *stream_)
{
    if (!labels || !onehot_out) GG_FAIL(GG_ERR_BAD_SHAPE, "labels_to_onehot: null pointer");
    if (stride % 8 || stride < K) GG_FAIL(GG_ERR_BAD_SHAPE, "labels_to_onehot: stride %d (K=%d)", stride, K);
    if (M <= 0) return GG_OK;
    long long total = (long long)M * (stride / 8);
    const unsigned blocks = gg_blocks256(total, 8192);
    hipLaunchKernelGGL(labels_to_onehot_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, labels, (long long)M, K,
                       (bf16_t *)onehot_out, stride);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------------------
// Pointwise reverse steps of the LDM samplers, fp32 (gg_step.h holds the arithmetic): the DDIM update and the ancestral update with the
// reference's options (x0 parameterisation, clip_denoised, the prediction of x_0 as an output), one kernel templated on the formula, and
// the row-per-lane kernel of gg_ddpm_step_x0 at C == 4.
// ------------------------------------------------------------------------------------------------------------
enum { STEP_DDIM = 0, STEP_ANCESTRAL = 1 };

// the four constants of a step in the order step_one takes them: DDIM {sqrt(1 - a_t), the three roots}, ancestral the scalar row itself
template <int F>
__device__ __forceinline__ void step_consts(const float *__restrict__ sc, float (&k)[4])
{
    if constexpr (F == STEP_DDIM) {
        k[0] = sc[3];
        ddim_roots(sc[0], sc[1], sc[2], k[1], k[2], k[3]);
    } else {
        k[0] = sc[0]; k[1] = sc[1]; k[2] = sc[2]; k[3] = sc[3];
    }
}

// -> x_prev before its noise term; p: the prediction of x_0
template <int F>
__device__ __forceinline__ float step_one(float xv, float ov, const float (&k)[4], int flags, float &p)
{
    if constexpr (F == STEP_DDIM) {
        p = ddim_pred_x0(xv, ov, k[0], k[1]);
        return ddim_x_prev(p, ov, k[2], k[3]);
    } else {
        p = ddpm_x_recon(xv, ov, k[0], k[1], flags);
        return ddpm_mean(p, xv, k[2], k[3]);
    }
}

// Ancestral form at C == 4: one row per lane, 16-byte accesses of x / out / noise / pred_x0_out, one 8-byte bf16x4 store into the UNet
// input (the layout of inpaint_blend_c4_kernel).  gg_ddpm_step_x0 alone launches it, after checking the alignment these accesses need:
// the other entries run per element, which measured faster at the latent sizes.
__global__ __launch_bounds__(256) void ddpm_step_c4_kernel(float *__restrict__ x, const float *__restrict__ out, int out_stride,
                                                           const float *__restrict__ noise, const float *__restrict__ sc, int flags,
                                                           long long M, float *__restrict__ pred_x0_out, bf16_t *__restrict__ unet_in,
                                                           int unet_in_stride)
{
    float k[4];
    step_consts<STEP_ANCESTRAL>(sc, k);
    const float kn = sc[4];
    for (long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (long long)gridDim.x * blockDim.x) {
        const f32x4 xv = *reinterpret_cast<const f32x4 *>(x + m * 4);
        const f32x4 ov = *reinterpret_cast<const f32x4 *>(out + m * out_stride);
        f32x4 nv = f32x4{0.f, 0.f, 0.f, 0.f};
        if (noise) nv = *reinterpret_cast<const f32x4 *>(noise + m * 4);
        f32x4 r, p;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float pc;
            float xn = step_one<STEP_ANCESTRAL>(xv[c], ov[c], k, flags, pc);
            if (noise) xn = step_add_noise(xn, kn, nv[c]);
            r[c] = xn;
            p[c] = pc;
        }
        *reinterpret_cast<f32x4 *>(x + m * 4) = r;
        if (pred_x0_out) *reinterpret_cast<f32x4 *>(pred_x0_out + m * 4) = p;
        if (unet_in) {
            bf16x4 o;
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = (bf16_t)r[c];
            *reinterpret_cast<bf16x4 *>(unet_in + m * unet_in_stride) = o;
        }
    }
}

template <int F>
__global__ __launch_bounds__(256) void step_kernel(float *__restrict__ x, const float *__restrict__ out, int out_stride,
                                                   const float *__restrict__ noise, const float *__restrict__ sc, int noise_idx, int flags,
                                                   long long M, int C, float *__restrict__ pred_x0_out, bf16_t *__restrict__ unet_in,
                                                   int unet_in_stride)
{
    float k[4];
    step_consts<F>(sc, k);
    const float kn = sc[noise_idx];
    const long long total = M * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / C;
        const int c = (int)(i - m * C);
        float p;
        float xn = step_one<F>(x[i], out[m * out_stride + c], k, flags, p);
        if (noise) xn = step_add_noise(xn, kn, noise[i]);
        x[i] = xn;
        if (pred_x0_out) pred_x0_out[i] = p;
        if (unet_in) unet_in[m * unet_in_stride + c] = (bf16_t)xn;
    }
}

template <int F>
static int step_launch(float *x, const float *out, int out_stride, const float *noise, const float *scalars_dev, int noise_idx, int flags,
                       long long M, int C, float *pred_x0_out, void *unet_in, int unet_in_stride, hipStream_t stream)
{
    if (M <= 0 || C <= 0) return GG_OK;
    hipLaunchKernelGGL(step_kernel<F>, dim3(gg_blocks256(M * C, 4096)), dim3(256), 0, stream, x, out, out_stride, noise, scalars_dev, noise_idx,
                       flags, M, C, pred_x0_out, (bf16_t *)unet_in, unet_in_stride);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

int gg_step_launch(int ancestral, float *x, const float *out, int out_stride, const float *noise, const float *scalars_dev, int noise_idx,
                   int flags, long long M, int C, float *pred_x0_out, void *unet_in, int unet_in_stride, hipStream_t stream)
{
    if (ancestral)
        return step_launch<STEP_ANCESTRAL>(x, out, out_stride, noise, scalars_dev, noise_idx, flags, M, C, pred_x0_out, unet_in, unet_in_stride, stream);
    return step_launch<STEP_DDIM>(x, out, out_stride, noise, scalars_dev, noise_idx, flags, M, C, pred_x0_out, unet_in, unet_in_stride, stream);
}

// scalars device fp32[4] = {a_t, a_prev, sigma_t, sqrt(1 - a_t)}: the noise coefficient is sigma_t
extern "C" int gg_ddim_step(float *x, const float *eps, int32_t eps_stride, const float *noise, const float *scalars_dev,
                            int64_t M, int32_t C, float *pred_x0_out, void *unet_in, int32_t unet_in_stride, void *stream_)
{
    if (!x || !eps || !scalars_dev) GG_FAIL(GG_ERR_BAD_SHAPE, "ddim_step: null pointer");
    if (eps_stride < C || (unet_in && unet_in_stride < C)) GG_FAIL(GG_ERR_BAD_SHAPE, "ddim_step: stride < C");
    return step_launch<STEP_DDIM>(x, eps, eps_stride, noise, scalars_dev, 2, 0, M, C, pred_x0_out, unet_in, unet_in_stride, (hipStream_t)stream_);
}

// scalars device fp32[5]: the ancestral row of gg_step.h
extern "C" int gg_ddpm_step(float *x, const float *eps, int32_t eps_stride, const float *noise, const float *scalars_dev, int64_t M,
                            int32_t C, void *unet_in, int32_t unet_in_stride, void *stream_)
{
    if (!x || !eps || !scalars_dev) GG_FAIL(GG_ERR_BAD_SHAPE, "ddpm_step: null pointer");
    if (eps_stride < C || (unet_in && unet_in_stride < C)) GG_FAIL(GG_ERR_BAD_SHAPE, "ddpm_step: stride < C");
    return step_launch<STEP_ANCESTRAL>(x, eps, eps_stride, noise, scalars_dev, 4, 0, M, C, nullptr, unet_in, unet_in_stride, (hipStream_t)stream_);
}

extern "C" int gg_ddpm_step_x0(float *x, const float *out, int32_t out_stride, const float *noise, const float *scalars_dev, int32_t flags,
                               int64_t M, int32_t C, float *pred_x0_out, void *unet_in, int32_t unet_in_stride, void *stream_)
{
    if (!x || !out || !scalars_dev) GG_FAIL(GG_ERR_BAD_SHAPE, "ddpm_step_x0: null pointer");
    if (C <= 0 || out_stride < C) GG_FAIL(GG_ERR_BAD_SHAPE, "ddpm_step_x0: out_stride %d < C=%d", out_stride, C);
    if (unet_in && unet_in_stride < C) GG_FAIL(GG_ERR_BAD_SHAPE, "ddpm_step_x0: unet_in_stride %d < C=%d", unet_in_stride, C);
    if (flags & ~(GG_DDPM_PREDICTS_X0 | GG_DDPM_CLIP)) GG_FAIL(GG_ERR_UNSUPPORTED, "ddpm_step_x0: unknown flag bits 0x%x", flags);
    const auto al = [](const void *p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; };
    const bool vec = C == 4 && al(x, 16) && al(out, 16) && out_stride % 4 == 0 && (!noise || al(noise, 16)) &&
                     (!pred_x0_out || al(pred_x0_out, 16)) && (!unet_in || (al(unet_in, 8) && unet_in_stride % 4 == 0));
    if (!vec || M <= 0)
        return step_launch<STEP_ANCESTRAL>(x, out, out_stride, noise, scalars_dev, 4, flags, M, C, pred_x0_out, unet_in, unet_in_stride, (hipStream_t)stream_);
    hipLaunchKernelGGL(ddpm_step_c4_kernel, dim3(gg_blocks256(M, 4096)), dim3(256), 0, (hipStream_t)stream_, x, out, out_stride, noise, scalars_dev,
                       flags, (long long)M, pred_x0_out, (bf16_t *)unet_in, unet_in_stride);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------------------
// DPM-Solver++ (2M) reverse step, fp32 (dpm_pred_x0 / dpm_combine / dpm_x_next of gg_step.h).  One unit per lane over an exact grid (the
// entry refuses more workgroups than a grid holds): a row at C == 4 with 16-byte rows, an element otherwise, as gg_ddpm_step_x0 splits.
// scalars device fp32[6] = {alpha_s, sigma_s, k_x, k_d, c0, c1}; hist is read on a second-order step (c1 != 0) only.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dpm_step_c4_kernel(float *__restrict__ x, const float *__restrict__ out, int out_stride,
                                                          const float *__restrict__ sc, int flags, long long M, float *__restrict__ hist,
                                                          float *__restrict__ pred_x0_out, bf16_t *__restrict__ unet_in, int unet_in_stride)
{
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const float alpha_s = sc[0], sigma_s = sc[1], k_x = sc[2], k_d = sc[3], c0 = sc[4], c1 = sc[5];
    const f32x4 xv = *reinterpret_cast<const f32x4 *>(x + m * 4);
    const f32x4 ov = *reinterpret_cast<const f32x4 *>(out + m * out_stride);
    f32x4 hv = f32x4{0.f, 0.f, 0.f, 0.f};
    if (c1 != 0.0f) hv = *reinterpret_cast<const f32x4 *>(hist + m * 4);
    f32x4 r, p;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        p[c] = dpm_pred_x0(xv[c], ov[c], sigma_s, alpha_s, flags);
        const float D = c1 != 0.0f ? dpm_combine(p[c], hv[c], c0, c1) : p[c];
        r[c] = dpm_x_next(xv[c], D, k_x, k_d);
    }
    *reinterpret_cast<f32x4 *>(hist + m * 4) = p;
    if (pred_x0_out) *reinterpret_cast<f32x4 *>(pred_x0_out + m * 4) = p;
    *reinterpret_cast<f32x4 *>(x + m * 4) = r;
    if (unet_in) {
        bf16x4 o;
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = (bf16_t)r[c];
        *reinterpret_cast<bf16x4 *>(unet_in + m * unet_in_stride) = o;
    }
}

__global__ __launch_bounds__(256) void dpm_step_kernel(float *__restrict__ x, const float *__restrict__ out, int out_stride,
                                                       const float *__restrict__ sc, int flags, long long total, int C,
                                                       float *__restrict__ hist, float *__restrict__ pred_x0_out,
                                                       bf16_t *__restrict__ unet_in, int unet_in_stride)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const float alpha_s = sc[0], sigma_s = sc[1], k_x = sc[2], k_d = sc[3], c0 = sc[4], c1 = sc[5];
    const long long m = i / C;
    const int c = (int)(i - m * C);
    const float xv = x[i];
    const float p = dpm_pred_x0(xv, out[m * out_stride + c], sigma_s, alpha_s, flags);
    const float D = c1 != 0.0f ? dpm_combine(p, hist[i], c0, c1) : p;
    const float xn = dpm_x_next(xv, D, k_x, k_d);
    hist[i] = p;
    if (pred_x0_out) pred_x0_out[i] = p;
    x[i] = xn;
    if (unet_in) unet_in[m * unet_in_stride + c] = (bf16_t)xn;
}

extern "C" int gg_dpm_solver_step(float *x, const float *out, int32_t out_stride, const float *scalars_dev, int32_t flags, int64_t M,
                                  int32_t C, float *hist, float *pred_x0_out, void *unet_in, int32_t unet_in_stride, void *stream_)
{
    if (!x || !out || !scalars_dev || !hist) GG_FAIL(GG_ERR_BAD_SHAPE, "dpm_solver_step: null pointer");
    if (C <= 0 || out_stride < C) GG_FAIL(GG_ERR_BAD_SHAPE, "dpm_solver_step: out_stride %d < C=%d", out_stride, C);
    if (unet_in && unet_in_stride < C) GG_FAIL(GG_ERR_BAD_SHAPE, "dpm_solver_step: unet_in_stride %d < C=%d", unet_in_stride, C);
    if (M < 0) GG_FAIL(GG_ERR_BAD_SHAPE, "dpm_solver_step: M=%lld", (long long)M);
    if (flags & ~(GG_DDPM_PREDICTS_X0 | GG_DDPM_CLIP)) GG_FAIL(GG_ERR_UNSUPPORTED, "dpm_solver_step: unknown flag bits 0x%x", flags);
    if (M == 0) return GG_OK;
    const auto al = [](const void *p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; };
    const bool vec = C == 4 && al(x, 16) && al(out, 16) && out_stride % 4 == 0 && al(hist, 16) && (!pred_x0_out || al(pred_x0_out, 16)) &&
                     (!unet_in || (al(unet_in, 8) && unet_in_stride % 4 == 0));
    const long long max_units = 0x7fffffffLL * 256;          // one unit per lane: the grid is exact, there is no loop to fall back on
    if ((long long)M > max_units / (vec ? 1 : C))
        GG_FAIL(GG_ERR_UNSUPPORTED, "dpm_solver_step: M=%lld rows of %d channels exceed the grid", (long long)M, C);
    if (vec) {
        hipLaunchKernelGGL(dpm_step_c4_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, x, out, out_stride,
                           scalars_dev, flags, (long long)M, hist, pred_x0_out, (bf16_t *)unet_in, unet_in_stride);
    } else {
        const long long total = (long long)M * C;
        hipLaunchKernelGGL(dpm_step_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, x, out, out_stride,
                           scalars_dev, flags, total, C, hist, pred_x0_out, (bf16_t *)unet_in, unet_in_stride);
    }
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------------------
// Inpainting blend x <- q_sample(x0, t, noise) * mask + (1 - mask) * x, fp32 (inpaint_blend_one of gg_step.h).
// scalars device fp32[2] = {sqrt_alphas_cumprod[t], sqrt_one_minus_alphas_cumprod[t]}; mask has 1 or C channels.
// ------------------------------------------------------------------------------------------------------------

// C == 4 (the latent channels of every shipped config): one row per lane, 16-byte loads of x / x0 / noise (and of a 4-channel mask),
// one 8-byte bf16x4 store into the UNet input.  The host checks the alignment these accesses need.
template <int MC>
__global__ __launch_bounds__(256) void inpaint_blend_c4_kernel(float *__restrict__ x, const float *__restrict__ x0,
                                                               const float *__restrict__ mask, const float *__restrict__ noise,
                                                               const float *__restrict__ sc, long long M, bf16_t *__restrict__ unet_in,
                                                               int unet_in_stride)
{
    const float a = sc[0], b = sc[1];
    for (long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (long long)gridDim.x * blockDim.x) {
        const f32x4 xv = *reinterpret_cast<const f32x4 *>(x + m * 4);
        const f32x4 x0v = *reinterpret_cast<const f32x4 *>(x0 + m * 4);
        const f32x4 nv = *reinterpret_cast<const f32x4 *>(noise + m * 4);
        f32x4 mv;
        if constexpr (MC == 4) {
            mv = *reinterpret_cast<const f32x4 *>(mask + m * 4);
        } else {
            const float m1 = mask[m];
            mv = f32x4{m1, m1, m1, m1};
        }
        f32x4 r;
#pragma unroll
        for (int c = 0; c < 4; ++c) r[c] = inpaint_blend_one(xv[c], x0v[c], nv[c], mv[c], a, b);
        *reinterpret_cast<f32x4 *>(x + m * 4) = r;
        if (unet_in) {
            bf16x4 o;
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = (bf16_t)r[c];
            *reinterpret_cast<bf16x4 *>(unet_in + m * unet_in_stride) = o;
        }
    }
}

__global__ __launch_bounds__(256) void inpaint_blend_kernel(float *__restrict__ x, const float *__restrict__ x0, const float *__restrict__ mask,
                                                            int mask_C, const float *__restrict__ noise, const float *__restrict__ sc,
                                                            long long M, int C, bf16_t *__restrict__ unet_in, int unet_in_stride)
{
    const float a = sc[0], b = sc[1];
    const long long total = M * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / C;
        const int c = (int)(i - m * C);
        const float r = inpaint_blend_one(x[i], x0[i], noise[i], mask[m * mask_C + (mask_C == 1 ? 0 : c)], a, b);
        x[i] = r;
        if (unet_in) unet_in[m * unet_in_stride + c] = (bf16_t)r;
    }
}

extern "C" int gg_inpaint_blend(float *x, const float *x0, const float *mask, int32_t mask_C, const float *noise, const float *scalars_dev,
                                int64_t M, int32_t C, void *unet_in, int32_t unet_in_stride, void *stream_)
{
    if (!x || !x0 || !mask || !noise || !scalars_dev) GG_FAIL(GG_ERR_BAD_SHAPE, "inpaint_blend: null pointer");
    if (C <= 0 || (mask_C != 1 && mask_C != C)) GG_FAIL(GG_ERR_BAD_SHAPE, "inpaint_blend: mask_C=%d must be 1 or C=%d", mask_C, C);
    if (unet_in && unet_in_stride < C) GG_FAIL(GG_ERR_BAD_SHAPE, "inpaint_blend: unet_in_stride %d < C=%d", unet_in_stride, C);
    if (M <= 0) return GG_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const auto al = [](const void *p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; };
    const bool vec = C == 4 && al(x, 16) && al(x0, 16) && al(noise, 16) && (mask_C == 1 || al(mask, 16)) &&
                     (!unet_in || (al(unet_in, 8) && unet_in_stride % 4 == 0));
    const long long work = vec ? (long long)M : (long long)M * C;
    const unsigned blocks = gg_blocks256(work, 4096);
    if (vec && mask_C == 4)
        hipLaunchKernelGGL(inpaint_blend_c4_kernel<4>, dim3(blocks), dim3(256), 0, stream, x, x0, mask, noise, scalars_dev,
                           (long long)M, (bf16_t *)unet_in, unet_in_stride);
    else if (vec)
        hipLaunchKernelGGL(inpaint_blend_c4_kernel<1>, dim3(blocks), dim3(256), 0, stream, x, x0, mask, noise, scalars_dev,
                           (long long)M, (bf16_t *)unet_in, unet_in_stride);
    else
        hipLaunchKernelGGL(inpaint_blend_kernel, dim3(blocks), dim3(256), 0, stream, x, x0, mask, mask_C, noise, scalars_dev,
                           (long long)M, C, (bf16_t *)unet_in, unet_in_stride);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------------------
// PLMS noise-estimate combination (ldm/models/diffusion/plms.py:218-232), fp32, same left-to-right order as the reference
// expression:  out = (c0*e0 + c1*e1 + c2*e2 + c3*e3) / denom   (terms with a NULL pointer are skipped)
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lincomb4_kernel(const float *__restrict__ e0, const float *__restrict__ e1,
                                                       const float *__restrict__ e2, const float *__restrict__ e3, float c0, float c1,
                                                       float c2, float c3, float denom, long long n, float *__restrict__ out)
{
#pragma clang fp contract(off)
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float a = c0 * e0[i];
        if (e1) a = a + c1 * e1[i];
        if (e2) a = a + c2 * e2[i];
        if (e3) a = a + c3 * e3[i];
        out[i] = a / denom;
    }
}

extern "C" int gg_lincomb4(const float *e0, const float *e1, const float *e2, const float *e3, float c0, float c1, float c2, float c3,
                           float denom, int64_t n, float *out, void *stream_)
{
    if (!e0 || !out) GG_FAIL(GG_ERR_BAD_SHAPE, "lincomb4: null pointer");
    if (n <= 0) return GG_OK;
    const unsigned blocks = gg_blocks256(n, 4096);
    hipLaunchKernelGGL(lincomb4_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, e0, e1, e2, e3, c0, c1, c2, c3, denom,
                       (long long)n, out);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------------------
// min-max normalisation (ordered-uint atomics; deterministic): segment n = blockIdx.y of N holds n_per values, its min / max go to
// ws[2 * n], ws[2 * n + 1].  A whole tensor is one segment.
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t f2ord(float f) { uint32_t b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float ord2f(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }

__global__ __launch_bounds__(256) void minmax_seg_init_kernel(uint32_t *ws, int N)
{
    for (int i = threadIdx.x; i < N; i += blockDim.x) { ws[2 * i] = 0xFFFFFFFFu; ws[2 * i + 1] = 0u; }
}

__global__ __launch_bounds__(256) void minmax_seg_reduce_kernel(const float *__restrict__ src, long long n_per, uint32_t *ws)
{
    const int n = blockIdx.y;
    const float *s = src + (long long)n * n_per;
    float mn = INFINITY, mx = -INFINITY;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_per; i += (long long)gridDim.x * blockDim.x) {
        float v = s[i];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
    if ((threadIdx.x & 63) == 0) { atomicMin(&ws[2 * n], f2ord(mn)); atomicMax(&ws[2 * n + 1], f2ord(mx)); }
}

__global__ __launch_bounds__(256) void minmax_apply_kernel(const float *__restrict__ src, long long n, const uint32_t *ws,
                                                           float *__restrict__ dst)
{
#pragma clang fp contract(off)
    const float mn = ord2f(ws[0]), mx = ord2f(ws[1]);
    const float den = mx - mn;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dst[i] = (src[i] - mn) / den;
}

extern "C" int gg_minmax_normalise(const float *src, int64_t n, float *dst, float *workspace2, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!src || !dst || !workspace2) GG_FAIL(GG_ERR_BAD_SHAPE, "minmax_normalise: null pointer");
    if (n <= 0) return GG_OK;
    const dim3 grid(gg_blocks256(n, 2048)), block(256);
    hipLaunchKernelGGL(minmax_seg_init_kernel, dim3(1), block, 0, stream, (uint32_t *)workspace2, 1);
    hipLaunchKernelGGL(minmax_seg_reduce_kernel, grid, block, 0, stream, src, (long long)n, (uint32_t *)workspace2);
    hipLaunchKernelGGL(minmax_apply_kernel, grid, block, 0, stream, src, (long long)n, (const uint32_t *)workspace2, dst);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------------------
// Stage glue: CCDM label volume -> conditioning slice of the LDM loop, on the device.
//   up[d,y,x]  = labels[n, floor(d*Dm/D), floor(y*Hm/H), floor(x*Wm/W)]      nearest (order-0) upsample
//   rot[i,j]   = up[slice, H-1-j, i]                                          torch.rot90(k=3) on (H, W)
//   cond[n,i,j,0] = prev[n,i,j] (previous generated slice, [0,1]) ; cond[n,i,j,1] = rot[i,j]/255 ; other lanes 0
// (latentdiffusion/sample_diffusion.py:199-210; value convention ldm/data/ruijin_pimage_and_mask.py:127-131)
// ------------------------------------------------------------------------------------------------------------
// Index rule of scipy.ndimage.zoom(order=0) with its defaults (mode="constant", grid_mode=False), which is what the reference's
// stage-glue recipe calls (latentdiffusion/sample_diffusion.py:199-200): output index o reads input index
//   floor(o * zf + 0.5),  zf = (in - 1) / (out - 1)  in IEEE double  (NI_ZoomShift: cc = o * zoom; start = floor(cc + 0.5)).
// It differs from F.interpolate(nearest)'s floor(o * in / out) on 16 % of the indices at 128 -> 512.  The product and the sum are
// rounded separately (no FMA contraction), as the C code of scipy does, so that the index is bit-identical.
__device__ __forceinline__ int zoom0_index(int o, double zf, int n_in)
{
    const int i = (int)floor(__dadd_rn(__dmul_rn((double)o, zf), 0.5));
    return i < 0 ? 0 : (i > n_in - 1 ? n_in - 1 : i);
}

struct MaskGrid {             // the label volume [N][Dm][Hm][Wm], the slice extent (H == W) and the three zoom factors
    const int *labels;
    int Dm, Hm, Wm, H, W;
    double zd, zh, zw;
};

// The zoomed, rotated label of pixel r = i * W + j of sample n's slice `slice` (the one place the glue's index rule and rotation stand).
__device__ __forceinline__ int glue_label(const MaskGrid &g, int n, int slice, long long r)
{
    const int sd = zoom0_index(slice, g.zd, g.Dm);
    const int j = (int)(r % g.W), i = (int)(r / g.W);
    const int y = g.H - 1 - j, x = i;                     // rot90(k=3) on (H, W): out[i][j] = up[H-1-j][i]  (H == W)
    const int sy = zoom0_index(y, g.zh, g.Hm), sx = zoom0_index(x, g.zw, g.Wm);
    return g.labels[(((long long)n * g.Dm + sd) * g.Hm + sy) * g.Wm + sx];
}

// One conditioning row: pixel r = i * W + j of sample n's slice `slice`; pv: that pixel of the previous generated slice.  Writes the
// whole padded row and returns the mask value.
__device__ __forceinline__ float mask_to_cond_row(const MaskGrid &g, int n, int slice, long long r, float pv, bf16_t *__restrict__ row, int stride)
{
    const int lab = glue_label(g, n, slice, r);
    const float mv = (float)lab / 255.0f;
    bf16x8 o = {(bf16_t)pv, (bf16_t)mv, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
    *reinterpret_cast<bf16x8 *>(row) = o;
    bf16x8 z = {(bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
    for (int c = 8; c < stride; c += 8) *reinterpret_cast<bf16x8 *>(row + c) = z;
    return mv;
}

__global__ __launch_bounds__(256) void mask_to_cond_slice_kernel(const int *__restrict__ labels, int N, int Dm, int Hm, int Wm,
                                                                 int slice, int D, int H, int W, double zd, double zh, double zw,
                                                                 const float *__restrict__ prev, bf16_t *__restrict__ cond, int stride,
                                                                 float *__restrict__ mask_out)
{
    const MaskGrid g{labels, Dm, Hm, Wm, H, W, zd, zh, zw};
    const long long HW = (long long)H * W, total = (long long)N * HW;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int n = (int)(t / HW);
        const float mv = mask_to_cond_row(g, n, slice, t - n * HW, prev ? prev[t] : 0.f, cond + t * stride, stride);
        if (mask_out) mask_out[t] = mv;
    }
}

static double zoom0_factor(int n_in, int n_out) { return n_out > 1 ? (double)(n_in - 1) / (double)(n_out - 1) : 1.0; }

extern "C" int gg_mask_to_cond_slice(const int32_t *labels, int32_t N, int32_t Dm, int32_t Hm, int32_t Wm, int32_t slice, int32_t D,
                                     int32_t H, int32_t W, const float *prev, void *cond_cl, int32_t stride, float *mask_out,
                                     void *stream_)
{
    if (!labels || !cond_cl) GG_FAIL(GG_ERR_BAD_SHAPE, "mask_to_cond_slice: null pointer");
    if (H != W) GG_FAIL(GG_ERR_UNSUPPORTED, "mask_to_cond_slice: rot90 needs H == W");
    if (stride % 8 || stride < 8) GG_FAIL(GG_ERR_BAD_SHAPE, "mask_to_cond_slice: stride");
    if (slice < 0 || slice >= D) GG_FAIL(GG_ERR_BAD_SHAPE, "mask_to_cond_slice: slice %d outside [0,%d)", slice, D);
    if (N < 1 || Dm < 1 || Hm < 1 || Wm < 1) GG_FAIL(GG_ERR_BAD_SHAPE, "mask_to_cond_slice: empty label volume");
    long long total = (long long)N * H * W;
    const unsigned blocks = gg_blocks256(total, 4096);
    hipLaunchKernelGGL(mask_to_cond_slice_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, labels, N, Dm, Hm, Wm, slice,
                       D, H, W, zoom0_factor(Dm, D), zoom0_factor(Hm, H), zoom0_factor(Wm, W), prev, (bf16_t *)cond_cl, stride, mask_out);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------------------
// Batched slice loop of independent volumes (GuideGenPipeline.sample_ct_volumes): N volumes, each with its own slice window, run as one
// batch.  A device schedule int32 [iterations][N][3] = (slice, previous slice, active) and a device iteration counter make the per-slice
// work graph-capturable: the glue reads row iter_dev[0], the normalise+scatter reads it too and (advance != 0) moves the counter on.
// volume fp32 [D][N][H*W] (slice-major, sample n's slice s at (s * N + n) * H * W).  Every sample reads and writes only its own rows.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_to_cond_slices_kernel(const int *__restrict__ labels, int N, int Dm, int Hm, int Wm, int D, int H,
                                                                  int W, double zd, double zh, double zw, const int *__restrict__ sched,
                                                                  int iterations, const int *__restrict__ iter_dev,
                                                                  const float *__restrict__ volume, bf16_t *__restrict__ cond, int stride)
{
    const int it = iter_dev[0];
    if (it < 0 || it >= iterations) return;                // a schedule overrun writes nothing
    const MaskGrid g{labels, Dm, Hm, Wm, H, W, zd, zh, zw};
    const long long HW = (long long)H * W, total = (long long)N * HW;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int n = (int)(t / HW);
        const long long r = t - n * HW;
        const int *row = sched + ((long long)it * N + n) * 3;
        const int slice = min(max(row[0], 0), D - 1), prev = min(max(row[1], 0), D - 1);
        mask_to_cond_row(g, n, slice, r, volume[((long long)prev * N + n) * HW + r], cond + t * stride, stride);
    }
}

extern "C" int gg_mask_to_cond_slices(const int32_t *labels, int32_t N, int32_t Dm, int32_t Hm, int32_t Wm, int32_t D, int32_t H, int32_t W,
                                      const int32_t *schedule_dev, int32_t iterations, const int32_t *iter_dev, const float *volume,
                                      void *cond_cl, int32_t stride, void *stream_)
{
    if (!labels || !schedule_dev || !iter_dev || !volume || !cond_cl) GG_FAIL(GG_ERR_BAD_SHAPE, "mask_to_cond_slices: null pointer");
    if (H != W) GG_FAIL(GG_ERR_UNSUPPORTED, "mask_to_cond_slices: rot90 needs H == W");
    if (stride % 8 || stride < 8) GG_FAIL(GG_ERR_BAD_SHAPE, "mask_to_cond_slices: stride");
    if (N < 1 || Dm < 1 || Hm < 1 || Wm < 1 || D < 1 || H < 1 || iterations < 1) GG_FAIL(GG_ERR_BAD_SHAPE, "mask_to_cond_slices: empty extent");
    long long total = (long long)N * H * W;
    const unsigned blocks = gg_blocks256(total, 4096);
    hipLaunchKernelGGL(mask_to_cond_slices_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, labels, N, Dm, Hm, Wm, D, H, W,
                       zoom0_factor(Dm, D), zoom0_factor(Hm, H), zoom0_factor(Wm, W), schedule_dev, iterations, iter_dev, volume,
                       (bf16_t *)cond_cl, stride);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// Segmented form of gg_minmax_normalise: sample n's min / max over its own n_per values (workspace [N][2], ordered uints), then
// (src - mn) / den with the same operands and the same rounding, so that each segment is bit-equal to gg_minmax_normalise on that sample
// alone.  The result goes to volume[slice_n][n] for the samples whose schedule row is active; the others are left untouched.
__global__ __launch_bounds__(256) void minmax_seg_scatter_kernel(const float *__restrict__ src, int N, long long n_per, const uint32_t *ws,
                                                                 const int *__restrict__ sched, int iterations, const int *__restrict__ iter_dev,
                                                                 int depth, float *__restrict__ volume)
{
#pragma clang fp contract(off)
    const int n = blockIdx.y;
    const int it = iter_dev[0];
    if (it < 0 || it >= iterations) return;
    const int *row = sched + ((long long)it * N + n) * 3;
    if (!row[2]) return;
    const int slice = row[0];
    if (slice < 0 || slice >= depth) return;
    const float mn = ord2f(ws[2 * n]), mx = ord2f(ws[2 * n + 1]);
    const float den = mx - mn;
    const float *s = src + (long long)n * n_per;
    float *d = volume + ((long long)slice * N + n) * n_per;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_per; i += (long long)gridDim.x * blockDim.x)
        d[i] = (s[i] - mn) / den;
}

__global__ void schedule_advance_kernel(int *iter_dev) { iter_dev[0] += 1; }

extern "C" int gg_minmax_normalise_scatter(const float *src, int32_t N, int64_t n_per_sample, float *workspace2n, const int32_t *schedule_dev,
                                           int32_t iterations, int32_t *iter_dev, int32_t advance, int32_t depth, float *volume, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!src || !workspace2n || !schedule_dev || !iter_dev || !volume) GG_FAIL(GG_ERR_BAD_SHAPE, "minmax_normalise_scatter: null pointer");
    if (N < 1 || N > 65535 || n_per_sample <= 0 || depth < 1 || iterations < 1) GG_FAIL(GG_ERR_BAD_SHAPE, "minmax_normalise_scatter: bad extent");
    const unsigned bx = gg_blocks256(n_per_sample, 2048 / N > 1 ? 2048 / N : 1);       // about gg_minmax_normalise's grid over the whole batch
    hipLaunchKernelGGL(minmax_seg_init_kernel, dim3(1), dim3(256), 0, stream, (uint32_t *)workspace2n, N);
    hipLaunchKernelGGL(minmax_seg_reduce_kernel, dim3(bx, (unsigned)N), dim3(256), 0, stream, src, (long long)n_per_sample,
                       (uint32_t *)workspace2n);
    hipLaunchKernelGGL(minmax_seg_scatter_kernel, dim3(bx, (unsigned)N), dim3(256), 0, stream, src, N, (long long)n_per_sample,
                       (const uint32_t *)workspace2n, schedule_dev, iterations, iter_dev, depth, volume);
    if (advance) hipLaunchKernelGGL(schedule_advance_kernel, dim3(1), dim3(1), 0, stream, iter_dev);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------------------
// CT editing (GuideGenPipeline.sample_ct_volumes with known_ct / keep): the same schedule and counter as above.
// known fp32 / keep uint8 [D][N][H*W] in the layout of `volume`; keep != 0 keeps the known voxel.
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool keep4_all(uint32_t w) { return (w & 0xFFu) && (w & 0xFF00u) && (w & 0xFF0000u) && (w & 0xFF000000u); }

// Per sample n at its own slice: (a) the first-stage input row of every pixel, channel 0 = the known slice, other lanes 0; (b) the latent
// keep mask: cell (i, j) is 1 iff every pixel of [f (i - r), f (i + 1 + r)) x [f (j - r), f (j + 1 + r)) inside the image is kept.  An
// inactive row gives a zero image and mask 0.  vec4: the window's row pieces are read as aligned 4-byte words (f % 4 == 0, H % 4 == 0).
__global__ __launch_bounds__(256) void ct_edit_glue_kernel(const float *__restrict__ known, const uint8_t *__restrict__ keep, int N, int D, int H,
                                                           int lat, int f, int margin, const int *__restrict__ sched, int iterations,
                                                           const int *__restrict__ iter_dev, bf16_t *__restrict__ img, int stride,
                                                           float *__restrict__ mask, int vec4)
{
    const int it = iter_dev[0];
    if (it < 0 || it >= iterations) return;                // a schedule overrun writes nothing
    const long long HW = (long long)H * H, total = (long long)N * HW;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, step = (long long)gridDim.x * blockDim.x;
    const int *rows = sched + (long long)it * N * 3;
    const bf16x8 z = {(bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
    for (long long t = tid; t < total; t += step) {
        const int n = (int)(t / HW);
        const long long r = t - n * HW;
        const int slice = min(max(rows[3 * n], 0), D - 1);
        const float kv = rows[3 * n + 2] ? known[((long long)slice * N + n) * HW + r] : 0.f;
        bf16x8 o = z;
        o[0] = (bf16_t)kv;
        bf16_t *row = img + t * stride;
        *reinterpret_cast<bf16x8 *>(row) = o;
        for (int c = 8; c < stride; c += 8) *reinterpret_cast<bf16x8 *>(row + c) = z;
    }
    const int LL = lat * lat;
    for (long long c = tid; c < (long long)N * LL; c += step) {
        const int n = (int)(c / LL), q = (int)(c - (long long)n * LL);
        const int i = q / lat, j = q - i * lat;
        bool all = rows[3 * n + 2] != 0;
        if (all) {
            const int slice = min(max(rows[3 * n], 0), D - 1);
            const uint8_t *kp = keep + ((long long)slice * N + n) * HW;
            const int y0 = max(f * (i - margin), 0), y1 = min(f * (i + 1 + margin), H);
            const int x0 = max(f * (j - margin), 0), x1 = min(f * (j + 1 + margin), H);
            for (int y = y0; y < y1 && all; ++y) {
                const uint8_t *p = kp + (long long)y * H;
                if (vec4) {
                    for (int x = x0; x < x1; x += 4) all = all && keep4_all(*reinterpret_cast<const uint32_t *>(p + x));
                } else {
                    for (int x = x0; x < x1; ++x) all = all && p[x] != 0;
                }
            }
        }
        mask[c] = all ? 1.0f : 0.0f;
    }
}

extern "C" int gg_ct_edit_glue(const float *known, const uint8_t *keep, int32_t N, int32_t D, int32_t H, int32_t W, int32_t lat, int32_t margin,
                               const int32_t *schedule_dev, int32_t iterations, const int32_t *iter_dev, void *image_cl, int32_t stride,
                               float *latent_keep, void *stream_)
{
    if (!known || !keep || !schedule_dev || !iter_dev || !image_cl || !latent_keep) GG_FAIL(GG_ERR_BAD_SHAPE, "ct_edit_glue: null pointer");
    if (H != W) GG_FAIL(GG_ERR_UNSUPPORTED, "ct_edit_glue: the slice must be square, got %d x %d", H, W);
    if (stride % 8 || stride < 8) GG_FAIL(GG_ERR_BAD_SHAPE, "ct_edit_glue: stride");
    if (N < 1 || D < 1 || H < 1 || iterations < 1 || lat < 1 || H % lat) GG_FAIL(GG_ERR_BAD_SHAPE, "ct_edit_glue: bad extent (H=%d, lat=%d)", H, lat);
    const int f = H / lat;
    if (margin < 0 || (long long)f * (2LL * margin + 1) > H) GG_FAIL(GG_ERR_BAD_SHAPE, "ct_edit_glue: margin %d: the window is wider than the image", margin);
    const int vec4 = (f % 4 == 0 && H % 4 == 0 && ((uintptr_t)keep & 3) == 0) ? 1 : 0;
    const unsigned blocks = gg_blocks256((long long)N * H * W, 4096);
    hipLaunchKernelGGL(ct_edit_glue_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, known, keep, N, D, H, lat, f, margin, schedule_dev,
                       iterations, iter_dev, (bf16_t *)image_cl, stride, latent_keep, vec4);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// minmax_seg_scatter_kernel with the pixel composite: kept pixels receive the known value, the others the normalised one (the same
// operands and rounding, so bit-equal to gg_minmax_normalise on that sample alone).  vec4: 16-byte rows (n_per % 4 == 0, aligned bases).
__global__ __launch_bounds__(256) void minmax_seg_keep_scatter_kernel(const float *__restrict__ src, int N, long long n_per, const uint32_t *ws,
                                                                      const int *__restrict__ sched, int iterations,
                                                                      const int *__restrict__ iter_dev, int depth,
                                                                      const float *__restrict__ known, const uint8_t *__restrict__ keep,
                                                                      float *__restrict__ volume, int vec4)
{
#pragma clang fp contract(off)
    const int n = blockIdx.y;
    const int it = iter_dev[0];
    if (it < 0 || it >= iterations) return;
    const int *row = sched + ((long long)it * N + n) * 3;
    if (!row[2]) return;
    const int slice = row[0];
    if (slice < 0 || slice >= depth) return;
    const float mn = ord2f(ws[2 * n]), mx = ord2f(ws[2 * n + 1]);
    const float den = mx - mn;
    const float *s = src + (long long)n * n_per;
    const long long off = ((long long)slice * N + n) * n_per;
    const float *kn = known + off;
    const uint8_t *kp = keep + off;
    float *d = volume + off;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, step = (long long)gridDim.x * blockDim.x;
    if (vec4) {
        for (long long i = tid; i < n_per / 4; i += step) {
            const f32x4 sv = *reinterpret_cast<const f32x4 *>(s + 4 * i);
            const f32x4 kv = *reinterpret_cast<const f32x4 *>(kn + 4 * i);
            const uint32_t kb = *reinterpret_cast<const uint32_t *>(kp + 4 * i);
            f32x4 o;
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = ((kb >> (8 * c)) & 0xFFu) ? kv[c] : (sv[c] - mn) / den;
            *reinterpret_cast<f32x4 *>(d + 4 * i) = o;
        }
    } else {
        for (long long i = tid; i < n_per; i += step) d[i] = kp[i] ? kn[i] : (s[i] - mn) / den;
    }
}

extern "C" int gg_minmax_normalise_keep_scatter(const float *src, int32_t N, int64_t n_per_sample, float *workspace2n, const int32_t *schedule_dev,
                                                int32_t iterations, int32_t *iter_dev, int32_t advance, int32_t depth, const float *known,
                                                const uint8_t *keep, float *volume, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!src || !workspace2n || !schedule_dev || !iter_dev || !known || !keep || !volume)
        GG_FAIL(GG_ERR_BAD_SHAPE, "minmax_normalise_keep_scatter: null pointer");
    if (N < 1 || N > 65535 || n_per_sample <= 0 || depth < 1 || iterations < 1) GG_FAIL(GG_ERR_BAD_SHAPE, "minmax_normalise_keep_scatter: bad extent");
    const auto al = [](const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
    const int vec4 = (n_per_sample % 4 == 0 && al(src, 16) && al(known, 16) && al(volume, 16) && al(keep, 4)) ? 1 : 0;
    const unsigned bx = gg_blocks256(n_per_sample, 2048 / N > 1 ? 2048 / N : 1);       // the grid of gg_minmax_normalise_scatter
    hipLaunchKernelGGL(minmax_seg_init_kernel, dim3(1), dim3(256), 0, stream, (uint32_t *)workspace2n, N);
    hipLaunchKernelGGL(minmax_seg_reduce_kernel, dim3(bx, (unsigned)N), dim3(256), 0, stream, src, (long long)n_per_sample,
                       (uint32_t *)workspace2n);
    hipLaunchKernelGGL(minmax_seg_keep_scatter_kernel, dim3(bx, (unsigned)N), dim3(256), 0, stream, src, N, (long long)n_per_sample,
                       (const uint32_t *)workspace2n, schedule_dev, iterations, iter_dev, depth, known, keep, volume, vec4);
    if (advance) hipLaunchKernelGGL(schedule_advance_kernel, dim3(1), dim3(1), 0, stream, iter_dev);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// keep[d][n][i][j] = (the glue's zoomed, rotated label of the new volume == that of the old one): glue_label on both volumes.
__global__ __launch_bounds__(256) void label_keep_volume_kernel(const int *__restrict__ old_labels, const int *__restrict__ new_labels, int N, int Dm,
                                                                int Hm, int Wm, int D, int H, int W, double zd, double zh, double zw,
                                                                uint8_t *__restrict__ keep, int vec4)
{
    const MaskGrid go{old_labels, Dm, Hm, Wm, H, W, zd, zh, zw}, gn{new_labels, Dm, Hm, Wm, H, W, zd, zh, zw};
    const long long HW = (long long)H * W, total = (long long)D * N * HW;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, step = (long long)gridDim.x * blockDim.x;
    const int per = vec4 ? 4 : 1;                          // HW % 4 == 0: the 4 pixels of a word lie in one slice of one sample
    for (long long t = tid * per; t < total; t += step * per) {
        const int d = (int)(t / (N * HW));
        const long long rem = t - (long long)d * N * HW;
        const int n = (int)(rem / HW);
        const long long r = rem - n * HW;
        if (vec4) {
            uint32_t w = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) w |= (glue_label(go, n, d, r + c) == glue_label(gn, n, d, r + c) ? 1u : 0u) << (8 * c);
            *reinterpret_cast<uint32_t *>(keep + t) = w;
        } else {
            keep[t] = glue_label(go, n, d, r) == glue_label(gn, n, d, r) ? 1 : 0;
        }
    }
}

extern "C" int gg_label_keep_volume(const int32_t *old_labels, const int32_t *new_labels, int32_t N, int32_t Dm, int32_t Hm, int32_t Wm, int32_t D,
                                    int32_t H, int32_t W, uint8_t *keep, void *stream_)
{
    if (!old_labels || !new_labels || !keep) GG_FAIL(GG_ERR_BAD_SHAPE, "label_keep_volume: null pointer");
    if (H != W) GG_FAIL(GG_ERR_UNSUPPORTED, "label_keep_volume: rot90 needs H == W");
    if (N < 1 || Dm < 1 || Hm < 1 || Wm < 1 || D < 1 || H < 1) GG_FAIL(GG_ERR_BAD_SHAPE, "label_keep_volume: empty extent");
    const long long HW = (long long)H * W, total = (long long)D * N * HW;
    const int vec4 = (HW % 4 == 0 && ((uintptr_t)keep & 3) == 0) ? 1 : 0;
    const unsigned blocks = gg_blocks256(vec4 ? total / 4 : total, 4096);
    hipLaunchKernelGGL(label_keep_volume_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, old_labels, new_labels, N, Dm, Hm, Wm, D, H, W,
                       zoom0_factor(Dm, D), zoom0_factor(Hm, H), zoom0_factor(Wm, W), keep, vec4);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------------------
// layout movers
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nchw_to_cl_kernel(const float *__restrict__ src, int N, int C, long long S,
                                                         bf16_t *__restrict__ dst, int C_pad, int c_off, int zero_fill)
{
    // thread per (n, s, 8-channel piece of the padded row)
    const int P = C_pad >> 3;
    const long long total = (long long)N * S * P;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        // order: piece slowest within (n), s fastest -> coalesced fp32 reads along s
        long long ns = i % ((long long)N * S);
        int piece = (int)(i / ((long long)N * S));
        long long n = ns / S, s = ns - n * S;
        int c0 = piece * 8;
        bool any = false;
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int c = c0 + j - c_off;
            float v = 0.f;
            if (c >= 0 && c < C) { v = src[(n * C + c) * S + s]; any = true; }
            o[j] = (bf16_t)v;
        }
        bf16_t *d = dst + (n * S + s) * C_pad + c0;
        if (zero_fill) {
            *reinterpret_cast<bf16x8 *>(d) = o;
        } else if (any) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                int c = c0 + j - c_off;
                if (c >= 0 && c < C) d[j] = o[j];
            }
        }
    }
}

extern "C" int gg_nchw_f32_to_cl_bf16(const float *src, int32_t N, int32_t C, int64_t S, void *dst, int32_t C_pad,
                                      int32_t c_offset, int32_t zero_fill, void *stream_)
{
    if (!src || !dst) GG_FAIL(GG_ERR_BAD_SHAPE, "nchw_to_cl: null pointer");
    if (C_pad % 8 || c_offset < 0 || c_offset + C > C_pad) GG_FAIL(GG_ERR_BAD_SHAPE, "nchw_to_cl: C=%d offset=%d C_pad=%d", C, c_offset, C_pad);
    long long total = (long long)N * S * (C_pad / 8);
    if (total <= 0) return GG_OK;
    const unsigned blocks = gg_blocks256(total, 8192);
    hipLaunchKernelGGL(nchw_to_cl_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, src, N, C, (long long)S,
                       (bf16_t *)dst, C_pad, c_offset, zero_fill);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

template <typename T>
__global__ __launch_bounds__(256) void cl_to_nchw_kernel(const T *__restrict__ src, int N, int C, long long S, int C_pad,
                                                         float *__restrict__ dst)
{
    const long long total = (long long)N * C * S;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        long long s = i % S;
        long long nc = i / S;
        int c = (int)(nc % C);
        long long n = nc / C;
        dst[i] = (float)src[(n * S + s) * C_pad + c];
    }
}

extern "C" int gg_cl_to_nchw_f32(const void *src, int32_t src_dtype, int32_t N, int32_t C, int64_t S, int32_t C_pad, float *dst,
                                 void *stream_)
{
    if (!src || !dst) GG_FAIL(GG_ERR_BAD_SHAPE, "cl_to_nchw: null pointer");
    if (C > C_pad) GG_FAIL(GG_ERR_BAD_SHAPE, "cl_to_nchw: C > C_pad");
    long long total = (long long)N * C * S;
    if (total <= 0) return GG_OK;
    const unsigned blocks = gg_blocks256(total, 8192);
    if (src_dtype == GG_BF16)
        hipLaunchKernelGGL(cl_to_nchw_kernel<bf16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, (const bf16_t *)src, N, C,
                           (long long)S, C_pad, dst);
    else if (src_dtype == GG_F32)
        hipLaunchKernelGGL(cl_to_nchw_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, (const float *)src, N, C,
                           (long long)S, C_pad, dst);
    else
        GG_FAIL(GG_ERR_BAD_DTYPE, "cl_to_nchw: dtype");
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// Sampler log entry: the fp32 channels-last state [N * S, C] into one [N, C, S] slot of a caller-owned log buffer.  This is
// cl_to_nchw_kernel<float> on dense rows (C_pad == C), which already writes into a given destination: no second transpose kernel.
extern "C" int gg_log_rows(const float *state, int32_t N, int32_t C, int64_t S, float *slot, void *stream_)
{
    if (!state || !slot) GG_FAIL(GG_ERR_BAD_SHAPE, "log_rows: null pointer");
    if (N < 0 || C <= 0 || S < 0) GG_FAIL(GG_ERR_BAD_SHAPE, "log_rows: N=%d C=%d S=%lld", N, C, (long long)S);
    long long total = (long long)N * C * S;
    if (total <= 0) return GG_OK;
    const unsigned blocks = gg_blocks256(total, 8192);
    hipLaunchKernelGGL(cl_to_nchw_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, state, N, C, (long long)S, C, slot);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------------------
// small fp32 linear (one wave per output element) and sinusoidal embedding
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void linear_f32_kernel(const float *__restrict__ in, int M, int I, const float *__restrict__ W,
                                                         const float *__restrict__ b, int O, int act_in, float *__restrict__ out,
                                                         long long out_stride)
{
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= (long long)M * O) return;
    const int m = (int)(w / O), o = (int)(w - (long long)m * O);
    float acc = 0.f;
    for (int i = lane; i < I; i += 64) {
        float v = in[(long long)m * I + i];
        if (act_in) v = v / (1.0f + expf(-v));
        acc += v * W[(long long)o * I + i];
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s);
    if (lane == 0) out[(long long)m * out_stride + o] = acc + (b ? b[o] : 0.f);
}

extern "C" int gg_linear_f32(const float *in, int32_t M, int32_t I, const float *W, const float *b, int32_t O, int32_t act_in,
                             float *out, int64_t out_stride, void *stream_)
{
    if (!in || !W || !out) GG_FAIL(GG_ERR_BAD_SHAPE, "linear_f32: null pointer");
    if (M <= 0 || I <= 0 || O <= 0 || out_stride < O) GG_FAIL(GG_ERR_BAD_SHAPE, "linear_f32: bad shape");
    long long waves = (long long)M * O;
    hipLaunchKernelGGL(linear_f32_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream_, in, M, I, W, b, O, act_in,
                       out, (long long)out_stride);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

__global__ void timestep_embedding_kernel(const float *__restrict__ t, int M, int dim, float max_period, float *__restrict__ out)
{
    const int half = dim / 2;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * dim) return;
    const int m = i / dim, j = i - m * dim;
    float v = 0.f;
    if (j < 2 * half) {
        int f = (j < half) ? j : j - half;
        float freq = expf(-logf(max_period) * (float)f / (float)half);
        float arg = t[m] * freq;
        v = (j < half) ? cosf(arg) : sinf(arg);
    }
    out[i] = v;
}

extern "C" int gg_timestep_embedding(const float *t, int32_t M, int32_t dim, float max_period, float *out, void *stream_)
{
    if (!t || !out || M <= 0 || dim <= 0) GG_FAIL(GG_ERR_BAD_SHAPE, "timestep_embedding: bad args");
    int total = M * dim;
    hipLaunchKernelGGL(timestep_embedding_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream_, t, M, dim, max_period, out);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// ------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void gg_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char *gg_last_error(void) { return g_err; }
extern "C" int gg_version(void) { return 100; }
