// Held-out objectives, forward only: the noising kernels and the reductions around ONE UNet forward.
//   gg_q_sample_rows    q_sample with per-sample scalars (ldm/models/diffusion/ddpm.py:275-278), into fp32 NC(D)HW and / or the UNet input
//   gg_loss_rows        per-sample mean of (target - pred)^2, |target - pred| (ddpm.py:280-293,1040) or the prior-KL integrand (ddpm.py:1011-1023)
//   gg_ccdm_q_sample    q_xt_given_x0(x0, t).sample() on labels (ccdm/ddpm/models/diffusion_denoising.py:82-89, one_hot_categorical.py)
//   gg_ccdm_inpaint_blend  the same kernel around known labels, written into the reverse chain's state where keep != 0 (mask editing)
//   gg_ccdm_step_loss   per-sample sums of the weighted KL and the cross-entropy of ccdm/ddpm/trainer.py:305-327
// Reductions use NO floating-point atomics and are two-stage: every fp32 term is added into an fp64 per-thread sum in a fixed (grid-stride)
// order, the 256 sums of a workgroup are combined by a fixed shuffle tree and a fixed loop over its 4 waves, one fp64 partial per workgroup
// goes to the caller's workspace, and a second launch adds a sample's partials in index order.  The grid depends on the shape alone, so two
// runs on the same input give the same bits.  A workgroup never spans two samples (grid.y = sample).
#include "gg_reduce.h"
#include "gg_posterior.h"

namespace {

// ------------------------------------------------------------------------------------------------------------
// q_sample: one thread per (n, s), all C channels; reads coalesced along s, one channels-last row written per thread
// ------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(LS_THREADS) void q_sample_rows_kernel(const float *__restrict__ x, const float *__restrict__ noise,
                                                                   const float *__restrict__ sc, int N, int C, long long S,
                                                                   float *__restrict__ out, T *__restrict__ unet_in, int unet_in_stride)
{
#pragma clang fp contract(off)
    const long long total = (long long)N * S;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / S, s = i - n * S;
        const float s0 = sc[2 * n], s1 = sc[2 * n + 1];
        for (int c = 0; c < C; ++c) {
            const long long e = (n * C + c) * S + s;
            const float t1 = s0 * x[e];
            const float t2 = s1 * noise[e];
            const float r = t1 + t2;
            if (out) out[e] = r;
            if (unet_in) unet_in[i * unet_in_stride + c] = (T)r;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// per-sample mean of an elementwise term; grid = (blocks, N); one thread per spatial position, C channels each
// ------------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(LS_THREADS) void loss_rows_kernel(const float *__restrict__ pred, int pred_stride, const float *__restrict__ target,
                                                               const float *__restrict__ x_start, const float *__restrict__ sc, int C,
                                                               long long S, double *__restrict__ partials)
{
#pragma clang fp contract(off)
    __shared__ double lds[LS_THREADS / GG_WAVE];
    const long long n = blockIdx.y;
    double acc = 0.0;
    float sn = 0.f, lv = 0.f, elv = 0.f;
    // exp(lv) once per workgroup, rounded to fp32 from the fp64 value: at t = T - 1 the term -1 - lv + exp(lv) cancels to ~lv^2 / 2, and one
    // ulp of exp(lv) would be the whole of it
    if (MODE == GG_LOSS_PRIOR_KL) { sn = sc[2 * n]; lv = sc[2 * n + 1]; elv = (float)exp((double)lv); }
    for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += (long long)gridDim.x * blockDim.x) {
        for (int c = 0; c < C; ++c) {
            const long long e = (n * C + c) * S + s;
            float term;
            if (MODE == GG_LOSS_PRIOR_KL) {
                const float m = sn * x_start[e];
                term = 0.5f * (((-1.0f - lv) + elv) + m * m);
            } else {
                const float d = target[e] - pred[(n * S + s) * pred_stride + c];
                term = MODE == GG_LOSS_L2 ? d * d : fabsf(d);
            }
            acc += (double)term;
        }
    }
    const double bs = ls_block_sum(acc, lds);
    if (threadIdx.x == 0) partials[n * gridDim.x + blockIdx.x] = bs;
}

// ------------------------------------------------------------------------------------------------------------
// categorical forward noising, one voxel per thread: labels[m] takes a draw of q(x_t | x_0 = known[m]).  keep: only the rows with
// keep[m] != 0 are drawn (mask editing), every other row returns before it writes anything; nullptr: every row.  A row's known label is read
// before its label is written, so known may be the labels buffer itself (no __restrict__ on either).  PS: ccdm_key_row's.
// ------------------------------------------------------------------------------------------------------------
template <int KMAX, int PS>
__global__ __launch_bounds__(LS_THREADS) void ccdm_q_sample_kernel(int *labels, const int *known, const unsigned char *__restrict__ keep,
                                                                   const float *__restrict__ mix, long long rows_per_sample, int K,
                                                                   const float *__restrict__ E, uint64_t seed,
                                                                   const unsigned long long *__restrict__ seeds,
                                                                   const long long *__restrict__ offset_dev, long long M,
                                                                   bf16_t *__restrict__ onehot_out, int onehot_stride)
{
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    if (keep && keep[m] == 0) return;
    const long long n = m / rows_per_sample;
    uint64_t key = 0;
    long long row = 0;
    if (!E) ccdm_key_row<PS>(seed, seeds, rows_per_sample, m, key, row);      // with a tape there may be no keys to load
    float Ev[KMAX];
    ccdm_exp_row<KMAX>(Ev, E ? E + m * K : nullptr, K, key, row, (!E && offset_dev) ? offset_dev[0] : 0);
    const int best = ccdm_q_sample_voxel<KMAX>(known[m], mix[2 * n], mix[2 * n + 1], K, Ev);
    labels[m] = best;
    if (onehot_out) ccdm_onehot_row<KMAX, 0>(onehot_out + m * onehot_stride, best, K);
}

// ------------------------------------------------------------------------------------------------------------
// CCDM objective: grid = (blocks, N), one voxel per thread and grid-stride step; partials [N][blocks][2] = (weighted kl, ce)
// ------------------------------------------------------------------------------------------------------------
template <int KMAX>
__global__ __launch_bounds__(LS_THREADS) void ccdm_step_loss_kernel(const float *__restrict__ logits, int stride, const int *__restrict__ xt,
                                                                    const int *__restrict__ x0, const float *__restrict__ sc,
                                                                    long long rows_per_sample, const float *__restrict__ cw, int K,
                                                                    double *__restrict__ partials)
{
    __shared__ double lds[LS_THREADS / GG_WAVE];
    const long long n = blockIdx.y;
    const float a = sc[2 * n], abar = sc[2 * n + 1];
    double akl = 0.0, ace = 0.0;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < rows_per_sample; r += (long long)gridDim.x * blockDim.x) {
        const long long m = n * rows_per_sample + r;
        float lg[KMAX];
        const float *hp = logits + m * stride;
#pragma unroll
        for (int c = 0; c < KMAX; ++c) lg[c] = (c < K) ? hp[c] : 0.f;
        int l0 = x0[m], lt = xt[m];
        l0 = min(max(l0, 0), K - 1);          // a label outside [0, K) is the caller's error; the weight table is never read outside
        lt = min(max(lt, 0), K - 1);
        float kl, ce;
        ccdm_loss_voxel<KMAX>(lg, lt, l0, a, abar, K, cw[l0], kl, ce);
        akl += (double)kl;
        ace += (double)ce;
    }
    const double skl = ls_block_sum(akl, lds);
    const double sce = ls_block_sum(ace, lds);
    if (threadIdx.x == 0) {
        double *p = partials + (n * gridDim.x + blockIdx.x) * 2;
        p[0] = skl;
        p[1] = sce;
    }
}

}  // namespace

extern "C" int64_t gg_loss_workspace_bytes(int32_t N, int64_t rows_per_sample)
{
    if (N < 1 || rows_per_sample < 1) return 0;
    return (int64_t)N * ls_blocks(rows_per_sample) * 2 * (int64_t)sizeof(double);
}

extern "C" int gg_q_sample_rows(const float *x, const float *noise, const float *scalars_dev, int32_t N, int32_t C, int64_t S, float *out,
                                void *unet_in, int32_t unet_in_dtype, int32_t unet_in_stride, void *stream_)
{
    if (!x || !noise || !scalars_dev) GG_FAIL(GG_ERR_BAD_SHAPE, "q_sample_rows: null pointer");
    if (!out && !unet_in) GG_FAIL(GG_ERR_BAD_SHAPE, "q_sample_rows: no output");
    if (N < 1 || C < 1 || S < 1) GG_FAIL(GG_ERR_BAD_SHAPE, "q_sample_rows: N=%d C=%d S=%lld", N, C, (long long)S);
    if (unet_in && unet_in_stride < C) GG_FAIL(GG_ERR_BAD_SHAPE, "q_sample_rows: unet_in_stride %d < C=%d", unet_in_stride, C);
    if (unet_in && unet_in_dtype != GG_BF16 && unet_in_dtype != GG_F32) GG_FAIL(GG_ERR_BAD_DTYPE, "q_sample_rows: unet_in dtype");
    long long blocks = ((long long)N * S + LS_THREADS - 1) / LS_THREADS;
    if (blocks > 4096) blocks = 4096;
    hipStream_t stream = (hipStream_t)stream_;
    if (unet_in && unet_in_dtype == GG_F32)
        hipLaunchKernelGGL(q_sample_rows_kernel<float>, dim3((unsigned)blocks), dim3(LS_THREADS), 0, stream, x, noise, scalars_dev, N, C,
                           (long long)S, out, (float *)unet_in, unet_in_stride);
    else
        hipLaunchKernelGGL(q_sample_rows_kernel<bf16_t>, dim3((unsigned)blocks), dim3(LS_THREADS), 0, stream, x, noise, scalars_dev, N, C,
                           (long long)S, out, (bf16_t *)unet_in, unet_in_stride);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_loss_rows(const float *pred, int32_t pred_stride, const float *target, const float *x_start, const float *scalars_dev,
                            int32_t mode, int32_t N, int32_t C, int64_t S, double *out, void *workspace, int64_t workspace_bytes, void *stream_)
{
    if (!out || !workspace) GG_FAIL(GG_ERR_BAD_SHAPE, "loss_rows: null pointer");
    if (N < 1 || N > 65535 || C < 1 || S < 1) GG_FAIL(GG_ERR_BAD_SHAPE, "loss_rows: N=%d C=%d S=%lld", N, C, (long long)S);
    if (mode == GG_LOSS_L2 || mode == GG_LOSS_L1) {
        if (!pred || !target) GG_FAIL(GG_ERR_BAD_SHAPE, "loss_rows: l1 / l2 need pred and target");
        if (pred_stride < C) GG_FAIL(GG_ERR_BAD_SHAPE, "loss_rows: pred_stride %d < C=%d", pred_stride, C);
    } else if (mode == GG_LOSS_PRIOR_KL) {
        if (!x_start || !scalars_dev) GG_FAIL(GG_ERR_BAD_SHAPE, "loss_rows: prior_kl needs x_start and scalars");
    } else {
        GG_FAIL(GG_ERR_UNSUPPORTED, "loss_rows: mode %d", mode);
    }
    const int blocks = ls_blocks(S);
    if (workspace_bytes < (int64_t)N * blocks * (int64_t)sizeof(double))
        GG_FAIL(GG_ERR_WORKSPACE_TOO_SMALL, "loss_rows: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)N * blocks * 8);
    hipStream_t stream = (hipStream_t)stream_;
    double *ws = (double *)workspace;
    const dim3 grid((unsigned)blocks, (unsigned)N);
#define LS_CASE(M_)                                                                                                              \
    hipLaunchKernelGGL(loss_rows_kernel<M_>, grid, dim3(LS_THREADS), 0, stream, pred, pred_stride, target, x_start, scalars_dev, C, \
                       (long long)S, ws)
    if (mode == GG_LOSS_L2) LS_CASE(GG_LOSS_L2);
    else if (mode == GG_LOSS_L1) LS_CASE(GG_LOSS_L1);
    else LS_CASE(GG_LOSS_PRIOR_KL);
#undef LS_CASE
    hipLaunchKernelGGL(ls_finish_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, stream, (const double *)ws, N, 1, blocks,
                       1.0 / ((double)C * (double)S), out);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_ccdm_q_sample(const int32_t *x0, const float *mix_dev, int64_t rows_per_sample, int32_t K, const float *E,
                                const uint64_t *philox_seeds_dev, const int64_t *philox_offset_dev, int64_t M, int32_t *labels_out,
                                void *onehot_out, int32_t onehot_stride, void *stream_)
{
    if (!x0 || !mix_dev || !labels_out) GG_FAIL(GG_ERR_BAD_SHAPE, "ccdm_q_sample: null pointer");
    if (!E && !philox_seeds_dev) GG_FAIL(GG_ERR_BAD_SHAPE, "ccdm_q_sample: neither a tape nor Philox keys");
    if (K < 2 || K > 16) GG_FAIL(GG_ERR_UNSUPPORTED, "ccdm_q_sample: K=%d outside [2, 16]", K);
    if (int rc = ccdm_check_rows("ccdm_q_sample", M, 1, rows_per_sample, K, onehot_out, onehot_stride)) return rc;
    hipLaunchKernelGGL((ccdm_q_sample_kernel<16, 1>), dim3((unsigned)((M + LS_THREADS - 1) / LS_THREADS)), dim3(LS_THREADS), 0, (hipStream_t)stream_,
                       labels_out, x0, (const unsigned char *)nullptr, mix_dev, (long long)rows_per_sample, K, E, (uint64_t)0,
                       (const unsigned long long *)philox_seeds_dev, (const long long *)philox_offset_dev, (long long)M, (bf16_t *)onehot_out,
                       onehot_stride);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_ccdm_inpaint_blend(int32_t *labels, const int32_t *known, const uint8_t *keep, const float *mix_dev, int64_t rows_per_sample,
                                     int32_t K, const float *E, uint64_t philox_seed, const uint64_t *philox_seeds_dev,
                                     const int64_t *philox_offset_dev, int64_t M, void *onehot_out, int32_t onehot_stride, void *stream_)
{
    if (!labels || !known || !keep || !mix_dev) GG_FAIL(GG_ERR_BAD_SHAPE, "ccdm_inpaint_blend: null pointer");
    if (K < 2 || K > 32) GG_FAIL(GG_ERR_BAD_SHAPE, "ccdm_inpaint_blend: K=%d outside [2, 32]", K);
    if (int rc = ccdm_check_rows("ccdm_inpaint_blend", M, 1, rows_per_sample, K, onehot_out, onehot_stride)) return rc;
    const long long blocks = (M + LS_THREADS - 1) / LS_THREADS;
#define IB_CASE(KMAX_, PS_)                                                                                                              \
    hipLaunchKernelGGL((ccdm_q_sample_kernel<KMAX_, PS_>), dim3((unsigned)blocks), dim3(LS_THREADS), 0, (hipStream_t)stream_, labels,      \
                       known, keep, mix_dev, (long long)rows_per_sample, K, E, philox_seed,                                             \
                       (const unsigned long long *)philox_seeds_dev, (const long long *)philox_offset_dev, (long long)M,                \
                       (bf16_t *)onehot_out, onehot_stride)
    if (K <= 16) { if (philox_seeds_dev) IB_CASE(16, 1); else IB_CASE(16, 0); }
    else         { if (philox_seeds_dev) IB_CASE(32, 1); else IB_CASE(32, 0); }
#undef IB_CASE
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_ccdm_step_loss(const float *logits, int32_t logits_stride, const int32_t *xt, const int32_t *x0, const float *scalars_dev,
                                 int64_t rows_per_sample, const float *class_weights, int32_t K, int64_t M, double *out, void *workspace,
                                 int64_t workspace_bytes, void *stream_)
{
    if (!logits || !xt || !x0 || !scalars_dev || !class_weights || !out || !workspace) GG_FAIL(GG_ERR_BAD_SHAPE, "ccdm_step_loss: null pointer");
    if (K < 2 || K > 16) GG_FAIL(GG_ERR_UNSUPPORTED, "ccdm_step_loss: K=%d outside [2, 16]", K);
    if (logits_stride < K) GG_FAIL(GG_ERR_BAD_SHAPE, "ccdm_step_loss: logits_stride < K");
    if (int rc = ccdm_check_rows("ccdm_step_loss", M, 1, rows_per_sample, K, nullptr, 0)) return rc;
    const long long N = M / rows_per_sample;
    if (N > 65535) GG_FAIL(GG_ERR_UNSUPPORTED, "ccdm_step_loss: %lld samples exceed the grid", N);
    const int blocks = ls_blocks(rows_per_sample);
    if (workspace_bytes < N * blocks * 2 * (int64_t)sizeof(double))
        GG_FAIL(GG_ERR_WORKSPACE_TOO_SMALL, "ccdm_step_loss: workspace %lld < %lld bytes", (long long)workspace_bytes, N * blocks * 16);
    hipStream_t stream = (hipStream_t)stream_;
    double *ws = (double *)workspace;
    hipLaunchKernelGGL(ccdm_step_loss_kernel<16>, dim3((unsigned)blocks, (unsigned)N), dim3(LS_THREADS), 0, stream, logits, logits_stride, xt,
                       x0, scalars_dev, (long long)rows_per_sample, class_weights, K, ws);
    hipLaunchKernelGGL(ls_finish_kernel, dim3((unsigned)((2 * N + 63) / 64)), dim3(64), 0, stream, (const double *)ws, (int)(2 * N), 2, blocks,
                       1.0, out);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
