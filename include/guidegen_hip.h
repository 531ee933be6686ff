/* guidegen_hip.h -- C-ABI of libguidegen_hip.so (MI355X / gfx950 only).
 *
 * The reference (OvO1111/JointImageGeneration) has no native boundary: every hot-path "kernel" is an
 * ATen op dispatched from Python.  Each entry point below replaces the ATen call sites
 * cited beside it; the Python modules in jointimagegeneration_amd/ call these through ctypes exactly
 * where the reference modules call torch (see INTEGRATION.md for the binding a maintainer would add).
 *
 * Conventions:
 *   - plain C: device pointers as void*, explicit sizes, no torch / HIP types in signatures
 *     (`stream` is a hipStream_t passed as void*; NULL = default stream);
 *   - the library never allocates, frees or retains device memory and never synchronises the device:
 *     every call only enqueues kernels on `stream`, so it is legal inside hipGraph capture;
 *   - every function returns 0 (GG_OK) or a negative gg_status; gg_last_error() gives a thread-local message;
 *   - activations are channels-last ("CL"): [N, D, H, W, C] with C contiguous, bf16 unless stated,
 *     2-D tensors use D == 1; the channel count of a bf16 CL tensor is padded to a multiple of 32
 *     and the pad lanes hold zeros.
 */
#ifndef GUIDEGEN_HIP_H
#define GUIDEGEN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    GG_OK = 0,
    GG_ERR_BAD_SHAPE = -1,
    GG_ERR_BAD_DTYPE = -2,
    GG_ERR_UNSUPPORTED = -3,
    GG_ERR_WORKSPACE_TOO_SMALL = -4,
    GG_ERR_HIP = -5
} gg_status;

typedef enum { GG_BF16 = 0, GG_F32 = 1 } gg_dtype;

const char *gg_last_error(void);
int gg_version(void);

/* ------------------------------------------------------------------------------------------------
 * Convolution as implicit GEMM on MFMA (v_mfma_f32_16x16x32_bf16), bf16 in / fp32 accumulate.
 * Replaces nn.Conv{1,2,3}d call sites:
 *   ResBlock in_layers[2]/out_layers[3]/skip_connection  ccdm/.../unet_openai/unet.py:188-228, ldm/.../openaimodel.py:204-244
 *   stem / head conv                                      unet.py:522,719 ; openaimodel.py:522,688
 *   Downsample.op (stride 2, pad 1)                       unet.py:135-139 ; openaimodel.py:152-156
 *   Upsample: F.interpolate(nearest x2) + conv            unet.py:106-116 ; openaimodel.py:109-119 (fused: upsample=1)
 *   AttentionBlock qkv / proj_out (1x1)                   unet.py:291-301 ; openaimodel.py:307-317
 *   AE ResnetBlock / Downsample(pad (0,1)) / Upsample     ldm/modules/diffusionmodules/model.py:42-145
 *   nn.Linear on token rows (SpatialTransformer)          ldm/modules/attention.py:152-215 (ksize=1)
 *   th.cat([h, hs.pop()], 1) before a conv                unet.py:812 ; openaimodel.py:739 (fused: src2/C2)
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t N, D, H, W;        /* input extent (before the fused x2 upsample); D = 1 for 2-D            */
    int32_t C1, C2;            /* channels of src1 / src2 (C2 = 0: single source); padded, multiple of 32 */
    int32_t Cout;              /* logical output channels                                                */
    int32_t Cout_pad;          /* channel stride of `out` (multiple of 32 for bf16 outputs)              */
    int32_t kd, kh, kw;        /* kernel extent per dim: 1 or 3 (kd = 1 for 2-D)                         */
    int32_t stride;            /* 1 or 2 (applied to every dim with k > 1 or to all dims if k == 1)     */
    int32_t pad;               /* leading zero padding per dim with k == 3 (1 = 'same'; 0 = AE Downsample) */
    int32_t upsample;          /* 1: nearest-neighbour x2 on D(if kd==3),H,W is fused in front of the conv */
    int32_t Do, Ho, Wo;        /* output extent                                                          */
    int32_t out_dtype;         /* GG_BF16 or GG_F32                                                      */
    int32_t prologue_act;      /* fused GroupNorm prologue applied while gathering (zero padding stays zero):
                                  0 none, 1: silu(x*gn_scale + gn_shift), 2: x*gn_scale + gn_shift        */
    int32_t path_hint;         /* 0 = production dispatch.  1 (tests only) = take the halo-tile kernel whenever the shape is inside
                                  its envelope, even when the grid would under-fill the chip (the production gate then prefers
                                  the box / split-K kernels): lets small test shapes exercise the kernel the big shapes use, with its
                                  512-position box.  4 / 6 (tests only) = the same with the 256-position box the production dispatch
                                  picks for 3-D grids of <= 256 workgroups / the 1024-position box it picks for grids of >= 512 */
    const void *src1;          /* bf16 CL [N,D,H,W,C1]                                                   */
    const void *src2;          /* bf16 CL [N,D,H,W,C2] or NULL                                           */
    const void *weight;        /* packed by gg_conv_pack_weight                                          */
    const float *bias;         /* fp32 [*, Cout_pad]; row n * bias_stride is added to sample n           */
    int64_t bias_stride;       /* 0: one row shared by the batch (plain conv bias);
                                  Cout_pad: per-sample rows (conv bias + timestep-embedding projection) */
    const void *residual;      /* optional bf16 CL [N,Do,Ho,Wo,Cout_pad] added in the epilogue          */
    void *out;                 /* CL [N,Do,Ho,Wo,Cout_pad]                                              */
    const float *gn_scale;     /* fp32 [N, C1+C2] or NULL (see prologue_act)                             */
    const float *gn_shift;
    void *workspace;           /* caller-owned scratch (split-K slabs); size from gg_conv_workspace_bytes */
    int64_t workspace_bytes;
    void *reserved_ptr;        /* must be NULL (was: tickets of an in-launch split-K combine, measured slower and removed) */
    int64_t *gn_acc;           /* optional [N][S][Cout_pad][2] int64 (S = gg_conv_emits_stats(desc) stripes by position tile, summed by the consumer), caller-zeroed: the epilogue adds, per output channel, the sum
                                  and the sum of squares of the bf16-rounded outputs in fixed point (2^28 / 2^20 fractional
                                  bits; integer atomics commute, so the result is bit-reproducible).  It is the GroupNorm
                                  statistics of the NEXT norm, consumed by gg_groupnorm_apply_acc (the 1-stripe layout of the box / 160-step kernels) or gg_groupnorm_scale_shift_acc.
                                  Only filled when gg_conv_emits_stats(desc) != 0, which also gives the stripe count (1: box / 160-step
                                  kernels without split-K; 32: halo-tile kernel); bf16 output only. */
    /* Optional fused DDIM update as the epilogue of the UNet HEAD conv (ldm/models/diffusion/ddim.py:190-204; replaces a separate
     * gg_ddim_step launch).  Only when gg_conv_fuses_ddim(desc) == 1 (box kernel, Cout == 4 == channels of the state, fp32 output): for
     * every output position the epilogue, besides storing eps, computes pred_x0 = (x - sqrt(1-a_t) eps) / sqrt(a_t) and x_prev =
     * sqrt(a_prev) pred_x0 + sqrt(1 - a_prev - sigma^2) eps (sigma-noise NOT added: deterministic eta = 0 steps only) with the same
     * fp32 expression order as gg_ddim_step, and writes x_prev over ddim_x, pred_x0 to ddim_pred_x0, bf16(x_prev) into channels [0, 4)
     * of ddim_unet_in.  All NULL = plain conv. */
    float *ddim_x;               /* fp32 CL [M, 4] state, updated in place                                 */
    const float *ddim_scalars;   /* device fp32[4]: a_t, a_prev, sigma, sqrt(1 - a_t)                      */
    float *ddim_pred_x0;         /* fp32 CL [M, 4] or NULL                                                 */
    void *ddim_unet_in;          /* bf16 CL [M, ddim_unet_in_stride] or NULL                               */
    int64_t ddim_unet_in_stride;
    /* Optional fused GEGLU epilogue of the feed-forward projection (ldm/modules/attention.py:37-44 `x, gate = proj(x).chunk(2);
     * x * gelu(gate)`; replaces a separate gg_geglu launch and the round trip of the [M, 2*inner] projection).  1x1(x1) conv, bf16
     * output, Cout = 2*inner with inner % 16 == 0, no residual, and the weight / bias rows arranged in groups of 32 as [16 value rows
     * j0..j0+15 | their 16 gate rows inner+j0..inner+j0+15]: the output then has inner channels, out[m, j] =
     * (acc_value + bias_value)[j] * gelu_erf((acc_gate + bias_gate)[j]) from the fp32 accumulators, row stride Cout_pad / 2.
     * 0 = plain conv. */
    int32_t epilogue_geglu;
    /* Optional GroupNorm prologue computed FROM ACCUMULATORS inside the conv (no statistics launch, no scale / shift launch, no apply
     * launch): with prologue_act != 0, gn_scale == gn_shift == NULL and pro_acc1 != NULL, every workgroup folds the per-channel
     * fixed-point (sum, sumsq) accumulators the PRODUCING convs left for src1 / src2 (the 1-stripe layout [N][1][C][2] of
     * gg_conv_desc.gn_acc, i.e. producers with gg_conv_emits_stats == 1) into the GroupNorm(32) scale / shift table in LDS and applies
     * normalise * affine (* SiLU) in place to its staged input box.  Only where gg_conv_prologue_from_acc(desc) == 1 (box kernel:
     * affine-only norms always, SiLU norms where few cout tiles share a box or the image is tiny). */
    int32_t pro_c_logical;       /* logical channels of cat[src1, src2] (multiple of 32 groups)            */
    const int64_t *pro_acc1;     /* [N][1][C1][2]                                                          */
    const int64_t *pro_acc2;     /* [N][1][C2][2] or NULL (C2 == 0)                                        */
    const float *pro_gamma;      /* fp32 [pro_c_logical]                                                   */
    const float *pro_beta;
    float pro_eps;
    /* Optional K-concatenated 1x1 skip projection of a ResBlock (out = conv3x3(h) + conv1x1(x): unet.py:228-262, openaimodel.py:244-278
     * `self.skip_connection(x) + h`): the conv takes x (one or two sources, the skip concat) as extra input channels at the centre
     * tap, so the separate skip-conv launch and the residual read disappear.  skip_weight: the 1x1 weight packed by gg_conv_pack_weight
     * (ntaps = 1, Cin_pad = skip_C1 + skip_C2); `bias` must already hold conv bias + skip bias; `residual` must be NULL.  Only where
     * gg_conv_fuses_skip(desc) == 1 (box kernel, 3x3, stride 1, no upsample).  skip_C1 == 0: plain conv. */
    int32_t skip_C1, skip_C2;    /* channels of skip_src1 / skip_src2 (padded, multiples of 32)             */
    int32_t reserved_tail;
    const void *skip_src1;       /* bf16 CL [N,D,H,W,skip_C1] (same extent as the conv's input)            */
    const void *skip_src2;       /* bf16 CL [N,D,H,W,skip_C2] or NULL                                      */
    const void *skip_weight;
    /* Optional fused CCDM reverse step as the epilogue of the UNet HEAD conv (ccdm/ddpm/models/DenoisingModel: softmax of the head,
     * posterior q(x_{t-1} | x_t, x_0) summed over the predicted x_0, categorical draw; replaces a separate gg_ccdm_posterior_sample launch and
     * the round trip of the fp32 logits, 128 B per voxel).  Only when gg_conv_fuses_posterior(desc) == 1 (halo-tile kernel with the
     * 1024-position 3-D box, Cout = K <= 16, fp32 output, no residual).  For every output position m (= voxel index n, d, h, w) the
     * epilogue runs, on the fp32 accumulator + bias (the logits), exactly the arithmetic of gg_ccdm_posterior_sample (same device
     * function, so the same labels bit for bit), writes the new label to post_labels_out[m] (may alias post_xt) and, when
     * post_onehot_out != NULL, channels [0, K) of row m of the one-hot UNet input (bf16, row stride post_onehot_stride, even).
     * `out` is NOT written in this mode (may be NULL).  post_xt == NULL: plain conv. */
    const int32_t *post_xt;        /* int32 [M] current labels x_t                                            */
    int32_t *post_labels_out;      /* int32 [M]                                                               */
    const float *post_scalars;     /* device fp32[2], as gg_ccdm_posterior_sample's scalars_dev               */
    const float *post_E;           /* optional fp32 [M, K] exponentials (a tape); NULL: Philox                */
    uint64_t post_philox_seed;
    const int64_t *post_philox_offset_dev;   /* device int64[1] step offset of the Philox counter, or NULL (0)  */
    void *post_onehot_out;         /* bf16 [M, post_onehot_stride] or NULL                                    */
    int64_t post_onehot_stride;
    int32_t post_draw;             /* 1: categorical draw (exponential race); 0: argmax of the posterior      */
    int32_t reserved_tail2;
    /* Per-sample Philox keys of the fused reverse step (batches of independent volumes).  NULL: post_philox_seed keys every voxel
     * and the counter is the voxel index m over the whole batch (the single-key mode).  Set: sample n = m / post_rows_per_sample draws
     * with key post_philox_seeds[n] and counter row m - n * post_rows_per_sample, so its labels do not depend on its batch slot;
     * post_rows_per_sample must be Do * Ho * Wo.  At N = 1 with post_philox_seeds[0] == post_philox_seed both modes give the same bits. */
    const uint64_t *post_philox_seeds;   /* device uint64 [N] or NULL                                             */
    int64_t post_rows_per_sample;
} gg_conv_desc;

/* Bytes of the packed weight for a conv with the given logical shape. */
int64_t gg_conv_packed_weight_bytes(int32_t Cout, int32_t Cin_pad, int32_t ntaps);
/* Repack an fp32 OI[D]HW weight (the checkpoint layout) into the MFMA tile order
 * [Cout_pad/32][tap][Cin_pad/32][32 co][32 ci] bf16, zero-filling padded rows/cols.
 * `w_f32` is a device pointer, logical shape [Cout, Cin, ntaps]; cin_map (host, may be NULL) is not used. */
int gg_conv_pack_weight(const float *w_f32, int32_t Cout, int32_t Cin, int32_t Cin_pad, int32_t ntaps,
                        void *packed_bf16, void *stream);
/* Scratch bytes gg_conv_forward needs for this shape (0 for most; > 0 when the under-filled grid is split over K). */
int64_t gg_conv_workspace_bytes(const gg_conv_desc *desc);
/* 1 if the caller should hand the GroupNorm (* SiLU) in front of this conv to the conv (gn_scale / gn_shift + prologue_act: applied
 * once per staged element, the normalised activation never written to HBM), 0 if a separate gg_groupnorm_apply pass in front of a
 * prologue-free conv is the faster form.  Halo-tile shapes CAN always fuse it (path_hint != 0 answers that); with path_hint 0 the answer
 * follows the measured rule in gg_conv_halo.hip (separate where a box is re-staged by several cout groups).  Box-kernel shapes: where the box is staged by at most two cout tiles.  Pointers are not read. */
int gg_conv_fuses_prologue(const gg_conv_desc *desc);
/* 1 if gg_conv_forward(desc) can run the CCDM reverse step as this (head) conv's epilogue (gg_conv_desc.post_xt).  Pointers are not
 * dereferenced; residual, gn_acc, ddim_x and the skip projection must be unset (they have no meaning on a head conv with this epilogue). */
int gg_conv_fuses_posterior(const gg_conv_desc *desc);
/* 1 if gg_conv_forward(desc) runs this shape on the halo-tile kernel (3x3(x3), stride 1, filled grid). Pointers are not read. */
int gg_conv_runs_halo_tile(const gg_conv_desc *desc);
/* 1 if gg_conv_forward(desc) runs this shape on the streaming 1x1 tile kernel (stride 1, one or two power-of-two sources, Cout_pad 64 /
 * 128, bf16 output, no prologue / residual / fused epilogue, at least 64^3 positions), else 0.  path_hint 12 (tests, A/B) is production
 * dispatch with this kernel switched off: the gather kernel then runs these shapes, with byte-identical results.  Pointers are not read. */
int gg_conv_runs_tile(const gg_conv_desc *desc);
/* 0 if gg_conv_forward(desc) does not run this shape on the split halo path, else its number of K slabs (the gather plan's split, so
 * gg_conv_workspace_bytes(desc) == slabs * M * Cout_pad * 4 as before): 3x3x3, stride 1, pad 1, extents multiples of the 4x4x16 box, a grid
 * too small for the halo-tile gate, no prologue / upsample / fused epilogue, whole chunks per slab.  path_hint 13 (tests, A/B) is production
 * dispatch with this path switched off: the split gather kernel then runs these shapes, with byte-identical results.  Pointers are not read. */
int gg_conv_runs_halo_split(const gg_conv_desc *desc);
/* 1 if gg_conv_forward(desc) runs this shape on the stride-2 3x3x3 tile kernel: pad 1, even input extents, output extents multiples of the
 * 2x4x16 tile, Cout_pad 128, no prologue / upsample / fused epilogue, and a grid that the gather kernel runs without a K split.
 * path_hint 14 (or 12; tests, A/B) is production dispatch with this kernel switched off: the gather kernel then runs these shapes, with
 * byte-identical results; path_hint 15 (tests only) lifts the grid condition.  Pointers are not read. */
int gg_conv_runs_tile_s2(const gg_conv_desc *desc);
/* 0 if gg_conv_forward(desc) will not fill desc->gn_acc, else the number of stripes S of the [N][S][Cout_pad][2] accumulator it fills
 * (1 for the box / 160-step kernels, 32 for the halo-tile kernel); pointers are not read. */
int gg_conv_emits_stats(const gg_conv_desc *desc);
/* 1 if gg_conv_forward(desc) can compute the GroupNorm prologue desc->prologue_act from accumulators (gg_conv_desc.pro_acc1) on its
 * own; pointers are not read. */
int gg_conv_prologue_from_acc(const gg_conv_desc *desc);
/* 1 if gg_conv_forward(desc) can take desc->skip_C1 / skip_C2 channels of a K-concatenated 1x1 skip projection; pointers are not read. */
int gg_conv_fuses_skip(const gg_conv_desc *desc);
/* 1 if gg_conv_forward(desc) can run the fused DDIM epilogue (see gg_conv_desc.ddim_x); pointers are not read. */
int gg_conv_fuses_ddim(const gg_conv_desc *desc);
int gg_conv_forward(const gg_conv_desc *desc, void *stream);

/* ------------------------------------------------------------------------------------------------
 * GroupNorm(32 groups) statistics and fused normalise*affine(+SiLU).
 * Replaces GroupNorm32 / Normalize + nn.SiLU / nonlinearity:
 *   ccdm/.../unet_openai/nn.py:17-19,93-100 ; ldm/modules/diffusionmodules/util.py:199-216 ;
 *   ldm/modules/diffusionmodules/model.py:33-39 ; ldm/modules/attention.py:76-77
 * Two-source aware (fuses the skip concat).  Statistics are accumulated in fp32 per block and combined
 * in fp64; results are written as per-(n,c) fp32 scale/shift so that y = x*scale + shift.
 * ------------------------------------------------------------------------------------------------ */
int64_t gg_groupnorm_workspace_bytes(int32_t N, int64_t S, int32_t C);
int gg_groupnorm_stats(const void *src1, int32_t C1, const void *src2, int32_t C2, int32_t N, int64_t S,
                       int32_t C_logical, const float *gamma, const float *beta, float eps,
                       float *scale_out, float *shift_out, void *workspace, int64_t workspace_bytes, void *stream);
/* y = act(x*scale[n,c] + shift[n,c]) ; act: 0 none, 1 SiLU.  out: bf16 CL [N,S,C1+C2]. */
int gg_groupnorm_apply(const void *src1, int32_t C1, const void *src2, int32_t C2, int32_t N, int64_t S,
                       const float *scale, const float *shift, int32_t act, void *out, void *stream);
/* Statistics + normalise*affine(+SiLU) in ONE launch for small tensors (the <= 16x16 UNet levels): a block keeps its group in registers
 * between the two phases.  gg_groupnorm_fused_supported says whether (S, C1, C2, C_logical) fits (C_logical == C1 + C2 required);
 * same result as gg_groupnorm_stats + gg_groupnorm_apply. */
int gg_groupnorm_fused_supported(int64_t S, int32_t C1, int32_t C2, int32_t C_logical);
int gg_groupnorm_fused(const void *src1, int32_t C1, const void *src2, int32_t C2, int32_t N, int64_t S, int32_t C_logical,
                       const float *gamma, const float *beta, float eps, int32_t act, void *out, void *stream);
/* The same normalise*affine(+SiLU), with the statistics taken from the per-channel fixed-point accumulators that the producing
 * convs left behind (gg_conv_desc.gn_acc): acc1 [N][1][C1][2], acc2 [N][1][C2][2] (NULL iff C2 == 0) -- ONLY the 1-stripe layout,
 * i.e. accumulators of convs for which gg_conv_emits_stats(desc) == 1 (box / 160-step kernels); the call has no stripe arguments,
 * so the 32-stripe accumulators of the halo-tile kernel (gg_conv_emits_stats == 32) must go through gg_groupnorm_scale_shift_acc
 * instead (handing them here would read 1/32 of the sums without an error).  Every block folds the accumulators into the
 * per-channel scale/shift table in LDS (fp64), so no statistics launch is needed. */
int gg_groupnorm_apply_acc(const void *src1, int32_t C1, const int64_t *acc1, const void *src2, int32_t C2, const int64_t *acc2,
                           int32_t N, int64_t S, int32_t C_logical, const float *gamma, const float *beta, float eps,
                           int32_t act, void *out, void *stream);

/* Per-(n, c) fp32 scale / shift (y = x*scale + shift == GroupNorm(32)(cat[src1, src2])) folded from the accumulators the producing convs
 * left (acc1 [N][stripes1][C1][2], acc2 [N][stripes2][C2][2] or NULL), for consumers that apply the norm themselves (the halo-tile conv's
 * fused prologue).  Replaces the gg_groupnorm_stats pass over the tensor. */
int gg_groupnorm_scale_shift_acc(const int64_t *acc1, int32_t stripes1, int32_t C1, const int64_t *acc2, int32_t stripes2, int32_t C2,
                                 int32_t N, int64_t S, int32_t C_logical, const float *gamma, const float *beta, float eps,
                                 float *scale_out, float *shift_out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Resampling / FiLM (gg_resample.hip): the conv-free Upsample / Downsample (conv_resample=False) and the ResBlock up / down steps
 * (resblock_updown), and the ResBlock's FiLM term (use_scale_shift_norm).  unet.py:85-145,254-257 ; openaimodel.py:93-160,270-274
 * ------------------------------------------------------------------------------------------------ */
/* dst = resample(act(src * scale[n, c] + shift[n, c])) on channels-last [N, D, H, W, C_pad] tensors (dtype GG_BF16 or GG_F32, fp32
 * arithmetic).  mode 0: nearest x2 upsample; mode 1: 2x average pool (odd pooled extents: GG_ERR_UNSUPPORTED).  H and W always, D too
 * iff resample_d (3-D networks).  scale / shift: optional fp32 [N, C_pad] (both or neither), act 1 = SiLU (only with scale / shift).
 * dst [N, Do, Ho, Wo, C_pad], channels >= C_logical written as zeros. */
int gg_resample2x(const void *src, int32_t dtype, int32_t N, int32_t D, int32_t H, int32_t W, int32_t C_pad, int32_t C_logical,
                  int32_t resample_d, int32_t mode, const float *scale, const float *shift, int32_t act, void *dst, void *stream);
/* In place, for c < C: scale[n, c] *= 1 + s, shift[n, c] = shift[n, c] * (1 + s) + t with s = film[n, c], t = film[n, C + c]
 * (scale / shift fp32 rows of coef_stride, film fp32 rows of film_stride >= 2 C).  One launch, no host synchronisation: the per-(n, c)
 * GroupNorm coefficients of a FiLM out-norm, for every consumer that takes coefficients (conv prologue, gg_groupnorm_apply). */
int gg_film_fold(float *scale, float *shift, int32_t coef_stride, int32_t N, int32_t C, const float *film, int64_t film_stride, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Attention: out = softmax(scale * Q K^T) V, flash-style (no TxT buffer), MFMA 16x16x32 bf16, fp32 softmax.
 * Replaces QKVAttentionLegacy (unet.py:334-360, openaimodel.py:349-371), CrossAttention
 * (ldm/modules/attention.py:170-193) and AttnBlock2d's bmm/softmax/bmm (model.py:243-257).
 * Element (n, t, h, d) of X in {Q,K,V,O} lives at X + ((n*T + t)*ld + h*hs + d).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t N, heads, head_dim;     /* head_dim in {32, 64, 128, 256, 384, 512}                          */
    int32_t Tq, Tkv;
    int64_t ldq, hsq, ldk, hsk, ldv, hsv, ldo, hso;
    float scale;
    int32_t reserved;
    const void *q, *k, *v;          /* bf16 */
    void *out;                      /* bf16 */
    void *workspace;                /* optional caller-owned scratch of gg_attention_workspace_bytes(desc) bytes: under-filled single-head
                                       grids (AE mid-block attention, one head of 384 / 512 channels over 4096 tokens) then split the KEYS over
                                       several workgroups and merge the online-softmax states in a second launch; NULL / too small: unsplit */
    int64_t workspace_bytes;
} gg_attention_desc;
int gg_attention_forward(const gg_attention_desc *desc, void *stream);
/* Scratch bytes with which gg_attention_forward splits the keys of this shape (0: it never splits it); pointers are not read. */
int64_t gg_attention_workspace_bytes(const gg_attention_desc *desc);
/* The launch gg_attention_forward makes for this shape: plan = {keys per K/V tile, key ranges split over workgroups when the
 * workspace is handed in (1: never), in-workgroup key split 0/1, K/V tiles staged by LDS-DMA 0/1}.  Pointers are not read and
 * nothing is launched; gg_attention_forward takes its decisions from the same function. */
int gg_attention_plan(const gg_attention_desc *desc, int32_t plan[4]);
/* Attention under a padding mask that is a prefix of ones (BERT): sample n attends to keys [0, kv_len[n]) only.  kv_len: int32 [N] on
 * the DEVICE, 1 <= kv_len[n] <= Tkv (the caller checks the host values it uploaded; the kernel clamps a value outside the range into
 * it and never reads past row Tkv - 1).  Keys j >= kv_len[n] have weight exactly 0 and their K / V rows are not read; whole key tiles
 * past the length are not walked.  All Tq query rows are computed; Tkv stays the row stride of the K / V buffers.  Runs the plain
 * register-staged kernel (no key split of either kind, desc->workspace is ignored): head_dim 32, 64 or 128, others
 * GG_ERR_UNSUPPORTED.  With kv_len[n] == Tkv for all n the result equals gg_attention_forward's wherever that runs the plain kernel.
 * Like every entry point here it reads no device memory on the host, allocates nothing and never synchronises (capture-safe). */
int gg_attention_forward_kvlen(const gg_attention_desc *desc, const int32_t *kv_len, void *stream);

/* LayerNorm over the last dim (nn.LayerNorm eps 1e-5, attention.py:203-205), bf16 rows -> bf16 rows. */
int gg_layernorm(const void *x, int64_t rows, int32_t C, const float *gamma, const float *beta, float eps,
                 void *out, void *stream);
/* GEGLU: out[r, j] = h[r, j] * gelu_erf(h[r, inner + j]) (attention.py:37-44). */
int gg_geglu(const void *h, int64_t rows, int32_t inner, void *out, void *stream);
/* out = a + b (bf16, elementwise; residual adds of SpatialTransformer / attention). */
int gg_add(const void *a, const void *b, int64_t n, void *out, void *stream);

/* Small fp32 linear: out[m, o] = sum_i act(in[m, i]) * W[o, i] + b[o]; act: 0 none, 1 SiLU on the input.
 * Replaces time_embed / emb_layers (unet.py:205-211,511-515 ; openaimodel.py:221-227,510-514). */
int gg_linear_f32(const float *in, int32_t M, int32_t I, const float *W, const float *b, int32_t O,
                  int32_t act_in, float *out, int64_t out_stride, void *stream);
/* Sinusoidal embedding cos||sin (nn.py:103-121 ; util.py:151-171), t as fp32. */
int gg_timestep_embedding(const float *t, int32_t M, int32_t dim, float max_period, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Layout / dtype movers at the module boundary (NC[D]HW fp32 <-> CL bf16/fp32).
 * ------------------------------------------------------------------------------------------------ */
int gg_nchw_f32_to_cl_bf16(const float *src, int32_t N, int32_t C, int64_t S, void *dst, int32_t C_pad,
                           int32_t c_offset, int32_t zero_fill, void *stream);
int gg_cl_to_nchw_f32(const void *src, int32_t src_dtype, int32_t N, int32_t C, int64_t S, int32_t C_pad,
                      float *dst, void *stream);

/* ------------------------------------------------------------------------------------------------
 * CCDM categorical reverse step (per voxel, fully fused):
 *   [softmax over K logits] -> theta_post_prob -> clamp 1e-12 -> renormalise -> argmax_k p_k/E_k
 * Replaces nn.Softmax head (unet.py:715-721), DiffusionModel.theta_post_prob
 * (ccdm/ddpm/models/diffusion_denoising.py:105-139), torch.clamp (:216) and
 * OneHotCategoricalBCHW.sample/max_prob_sample/prob_sample (one_hot_categorical.py:30-55).
 *   head       fp32 CL [M, head_stride]: probabilities (head_is_logits = 0) or logits (1)
 *   xt         int32 [M] current labels
 *   E          fp32 [M, K] exponential tape, or NULL
 *   philox_seed/philox_offset: used when E == NULL and draw != 0 (counter-based Exp(1) generator)
 *   draw       1: sample (t > 1); 0: argmax of the normalised posterior (t == 1)
 *   scalars    device fp32[2] = {alphas[t-1] (0 at t==1), cumalphas[t-2] (1 at t==1)}
 * Outputs: labels_out int32 [M] (may alias xt); probs_out fp32 [M, K] normalised posterior or NULL;
 *          onehot_out bf16 CL [M, onehot_stride] (channels < K one-hot, rest untouched; onehot_stride even, rows 4-byte aligned) or NULL.
 * ------------------------------------------------------------------------------------------------ */
int gg_ccdm_posterior_sample(const float *head, int32_t head_stride, int32_t head_is_logits, const int32_t *xt,
                             const float *E, uint64_t philox_seed, const int64_t *philox_offset_dev, int32_t draw,
                             const float *scalars_dev, int32_t K, int64_t M, int32_t *labels_out, float *probs_out,
                             void *onehot_out, int32_t onehot_stride, void *stream);
/* gg_ccdm_posterior_sample with one Philox key per sample: row m belongs to sample n = m / rows_per_sample (M must be a multiple of it)
 * and draws with key philox_seeds_dev[n] (device uint64 [M / rows_per_sample]) and counter row m - n * rows_per_sample instead of m.
 * At one sample with philox_seeds_dev[0] == philox_seed the labels are bit-identical to gg_ccdm_posterior_sample's. */
int gg_ccdm_posterior_sample_seeds(const float *head, int32_t head_stride, int32_t head_is_logits, const int32_t *xt,
                                   const float *E, const uint64_t *philox_seeds_dev, int64_t rows_per_sample,
                                   const int64_t *philox_offset_dev, int32_t draw, const float *scalars_dev, int32_t K, int64_t M,
                                   int32_t *labels_out, float *probs_out, void *onehot_out, int32_t onehot_stride, void *stream);
/* The tape of a Philox run: what the kernels above (and gg_ccdm_q_sample, and the fused head conv) draw when E == NULL, so that the run
 * can be replayed teacher-forced (E = the first K columns of E_out's rows, repacked to [M, K]) here or elsewhere.
 *   Row m draws kmax / 4 Philox4x32-10 blocks; block q4 has counter (row lo, row hi, q4, LOW 32 BITS of philox_offset_dev[0], 0 when
 *   NULL) and key (seed lo, seed hi); its four words are the classes 4 * q4 .. 4 * q4 + 3.  philox_seeds_dev == NULL: key philox_seed,
 *   row = m (gg_ccdm_posterior_sample); else key philox_seeds_dev[m / rows_per_sample], row = m % rows_per_sample (M a multiple).
 *   A word w gives u = ((w >> 8) + 1) * 2^-24 in (0, 1] and E = -log(u) + 1e-30 (hardware logarithm).
 *   kmax: 16 (the kernels' draw at K <= 16) or 32 (K > 16): the first 16 columns of the two agree.
 *   bits_in: uint32 [M, kmax] or NULL; given, those words are mapped instead of drawn (keys and offset unused).
 * Outputs, either may be NULL but not both: bits_out uint32 [M, kmax] the words; E_out fp32 [M, kmax] the exponentials. */
int gg_ccdm_draw_tape(uint64_t philox_seed, const uint64_t *philox_seeds_dev, int64_t rows_per_sample, const int64_t *philox_offset_dev,
                      int32_t kmax, int64_t M, const uint32_t *bits_in, uint32_t *bits_out, float *E_out, void *stream);
/* labels -> one-hot bf16 CL rows (x_T assembly; evaluator.py:135-136 + unet.py:774-775 concat with zeros). */
int gg_labels_to_onehot(const int32_t *labels, int64_t M, int32_t K, void *onehot_out, int32_t stride, void *stream);

/* ------------------------------------------------------------------------------------------------
 * DDIM update (ldm/models/diffusion/ddim.py:190-204), fp32, elementwise on CL tensors:
 *   pred_x0 = (x - sqrt(1-a_t) e)/sqrt(a_t);  x_prev = sqrt(a_prev) pred_x0 + sqrt(1-a_prev-sigma^2) e + sigma*noise
 *   scalars device fp32[4] = {a_t, a_prev, sigma_t, sqrt_one_minus_a_t};  noise may be NULL (treated as 0).
 *   x [M, C] fp32 (in/out), eps [M, eps_stride] fp32, pred_x0_out optional;
 *   unet_in optional bf16 CL [M, unet_in_stride]: channels [0, C) are refreshed with x_prev.
 * ------------------------------------------------------------------------------------------------ */
int gg_ddim_step(float *x, const float *eps, int32_t eps_stride, const float *noise, const float *scalars_dev,
                 int64_t M, int32_t C, float *pred_x0_out, void *unet_in, int32_t unet_in_stride, void *stream);

/* Ancestral DDPM step (LatentDiffusion.p_sample: ldm/models/diffusion/ddpm.py:217-230,1060-1120), fp32 elementwise:
 *   x_recon = s[0]*x - s[1]*eps ; mean = s[2]*x_recon + s[3]*x ; x <- mean + s[4]*noise   (scalars device fp32[5],
 *   s[4] = (t > 0) * exp(0.5 * posterior_log_variance_clipped[t]); noise may be NULL). unet_in as in gg_ddim_step. */
int gg_ddpm_step(float *x, const float *eps, int32_t eps_stride, const float *noise, const float *scalars_dev, int64_t M, int32_t C,
                 void *unet_in, int32_t unet_in_stride, void *stream);

/* Ancestral step with the reference's options (p_mean_variance, ddpm.py:1072-1083, + p_sample :1109-1120), fp32 elementwise on CL rows:
 *   xr = s[0]*x - s[1]*out;  flags & GG_DDPM_PREDICTS_X0: xr = out (parameterization "x0");  flags & GG_DDPM_CLIP: xr clamped to [-1, 1];
 *   pred_x0_out <- xr;  xn = s[2]*xr + s[3]*x;  noise != NULL: xn = xn + s[4]*noise;  x <- xn;  unet_in channels [0, C) <- bf16(xn).
 *   Evaluated in that order without contraction; scalars device fp32[5] as in gg_ddpm_step.  With flags == 0 and pred_x0_out == NULL the
 *   result is bit-equal to gg_ddpm_step's.  x fp32 [M, C] (in/out), out fp32 [M, out_stride] (the UNet's output), noise fp32 [M, C] or
 *   NULL, pred_x0_out fp32 [M, C] or NULL, unet_in bf16 CL [M, unet_in_stride] or NULL (pad lanes are not touched).
 *   GG_ERR_BAD_SHAPE: NULL x / out / scalars, out_stride < C, unet_in_stride < C; GG_ERR_UNSUPPORTED: flag bits other than the two.
 *   M == 0 returns GG_OK without a launch.  C == 4 with 16-byte aligned rows (out_stride and unet_in_stride multiples of 4, 8-byte
 *   unet_in rows) runs one row per lane; any other case a grid-stride loop per element.  A NaN through the clamp is unspecified.
 *   No allocation, no synchronisation. */
#define GG_DDPM_PREDICTS_X0 1
#define GG_DDPM_CLIP 2
int gg_ddpm_step_x0(float *x, const float *out, int32_t out_stride, const float *noise, const float *scalars_dev, int32_t flags,
                    int64_t M, int32_t C, float *pred_x0_out, void *unet_in, int32_t unet_in_stride, void *stream);

/* One reverse step of DPM-Solver++ in its multistep second-order data-prediction form ("2M": Lu et al. 2022, Algorithm 2), fp32
 * elementwise on CL rows, from the current point s of the schedule to the next point t.  scalars device fp32[6] =
 * {alpha_s, sigma_s, k_x, k_d, c0, c1} with alpha = sqrt(a), sigma = sqrt(1 - a), lambda = log(alpha / sigma), h = lambda_t - lambda_s,
 * k_x = sigma_t / sigma_s, k_d = -alpha_t * expm1(-h); a first-order step has c0 = 1, c1 = 0, a second-order step c0 = 1 + 1/(2r),
 * c1 = -1/(2r) with r = h_prev / h (the host computes the row in fp64 and rounds it once).
 *   p = (x - s[1]*out) / s[0];  flags & GG_DDPM_PREDICTS_X0: p = out (parameterization "x0");  flags & GG_DDPM_CLIP: p clamped to [-1, 1];
 *   D = p when s[5] == 0, else s[4]*p + s[5]*hist (hist is then the previous step's p; when s[5] == 0 it does not enter the result,
 *   whatever it holds, NaN included);  xn = s[2]*x + s[3]*D;  hist <- p;  pred_x0_out <- p;  x <- xn;  unet_in channels [0, C) <- bf16(xn).
 *   Evaluated in that order without contraction, every product and sum rounded on its own, IEEE division, the fp32 -> bf16 cast of
 *   gg_ddim_step; with s[5] == 0 and {k_x, k_d} of a DDIM pair the step is DDIM's at eta 0 up to rounding.
 *   x fp32 [M, C] (in/out), out fp32 [M, out_stride] (the UNet's output), hist fp32 [M, C] (in/out, the caller keeps it between the
 *   steps of one chain), pred_x0_out fp32 [M, C] or NULL, unet_in bf16 CL [M, unet_in_stride] or NULL (pad lanes are not touched).
 *   GG_ERR_BAD_SHAPE: NULL x / out / scalars / hist, out_stride < C, unet_in_stride < C, M < 0; GG_ERR_UNSUPPORTED: flag bits other than
 *   the two, or more units than one grid of 2^31 - 1 workgroups of 256 lanes holds (the kernels run one unit per lane, without a loop).
 *   M == 0 returns GG_OK without a launch.  C == 4 with 16-byte aligned rows (out_stride and unet_in_stride multiples of 4, 8-byte
 *   unet_in rows) runs one row per lane; any other case one element per lane.  A NaN through the clamp is unspecified.
 *   No allocation, no synchronisation: capturable. */
int gg_dpm_solver_step(float *x, const float *out, int32_t out_stride, const float *scalars_dev, int32_t flags, int64_t M, int32_t C,
                       float *hist, float *pred_x0_out, void *unet_in, int32_t unet_in_stride, void *stream);

/* Sampler log entry: the fp32 channels-last state [N * S, C] (dense rows; S voxels per sample) -> slot fp32 [N, C, S], one entry of a
 * caller-allocated log buffer.  It runs gg_cl_to_nchw_f32's kernel with C_pad == C, at a fixed destination: no allocation, no
 * synchronisation, so it can sit inside a captured chain.  GG_ERR_BAD_SHAPE: NULL pointers, C <= 0, negative N or S; an empty extent
 * returns GG_OK without a launch. */
int gg_log_rows(const float *state, int32_t N, int32_t C, int64_t S, float *slot, void *stream);

/* Inpainting blend of the LDM samplers (ddim.py:144-148, plms.py:147-150, ddpm.py:1212-1214), fp32 elementwise on CL rows [M, C]:
 *   x <- (s[0]*x0 + s[1]*noise) * mask + (1 - mask) * x      (the q_sample of ddpm.py:275-278, then the blend; mask 1 keeps x0)
 *   evaluated without contraction in the reference's order: t1 = s0*x0; t2 = s1*n; o = t1 + t2; p = o*m; q = (1 - m)*x; x = p + q.
 *   scalars device fp32[2] = {sqrt_alphas_cumprod[t], sqrt_one_minus_alphas_cumprod[t]} (a captured chain reads its row in place).
 *   x, x0, noise fp32 [M, C]; mask fp32 [M, mask_C] with mask_C 1 (broadcast over channels) or C; otherwise GG_ERR_BAD_SHAPE, as for
 *   NULL operands or unet_in_stride < C.  unet_in optional bf16 CL [M, unet_in_stride]: channels [0, C) are refreshed with bf16(x), the
 *   pad lanes are not touched.  C == 4 with 16-byte aligned rows (8-byte unet_in rows) runs one row per lane; any other case a
 *   grid-stride loop per element.  No allocation, no synchronisation. */
int gg_inpaint_blend(float *x, const float *x0, const float *mask, int32_t mask_C, const float *noise, const float *scalars_dev,
                     int64_t M, int32_t C, void *unet_in, int32_t unet_in_stride, void *stream);

/* Vector quantisation of a VQ first stage (taming's VectorQuantizer as ldm/models/autoencoder.py:45 builds it), gg_vq.hip.
 * gg_vq_nearest: rows fp32 channels-last [M, row_stride] (channels [0, C) are read), codebook fp32 [n_embed, C]:
 *   d[m,k] = sum_c z[m,c]^2 + sum_c E[k,c]^2 - 2 sum_c z[m,c] E[k,c];  idx[m] = argmin_k d[m,k], the first minimum on a tie.
 *   All fp32, no contraction: zz, ee and dot are each summed over ascending c (product rounded, then added), d = (zz + ee) - 2*dot.
 *   idx_out (optional) int32 [M]; st_out (optional) fp32 [M, st_stride]: channels [0, C) <- the straight-through rows
 *   z + (E[idx] - z), evaluated in that order (not E[idx]: the two differ by a rounding); st_out may be `rows` itself.
 *   C outside [1, 8]: GG_ERR_UNSUPPORTED; n_embed >= 1 is arbitrary (the codebook is staged through LDS in tiles of 1024 codes, codes
 *   past n_embed are never read).  No allocation, no host readback, no synchronisation: capturable.
 * gg_ddim_step_vq: one reverse step with the prediction of x_0 quantised (ddim.py:196-204 with quantize_denoised; ancestral != 0:
 *   ddpm.py:1073-1083 + p_sample).  x, eps, noise, pred_x0_out, unet_in as in gg_ddim_step; scalars device fp32[5]:
 *   ancestral == 0: {a_t, a_prev, sigma_t, sqrt(1 - a_t), noise coefficient (sigma_t * temperature)}
 *     p = (x - s[3]*eps)/sqrt(a_t);  q = quantise(p);  x <- sqrt(a_prev)*q + sqrt(1 - a_prev - sigma_t^2)*eps + s[4]*noise
 *   ancestral != 0: {sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, posterior_mean_coef1, posterior_mean_coef2, sigma}
 *     p = s[0]*x - s[1]*eps;          q = quantise(p);  x <- s[2]*q + s[3]*x + s[4]*noise
 *   each line left to right without contraction, as gg_ddim_step / gg_ddpm_step evaluate theirs.  pred_x0_out receives q (the
 *   straight-through rows), idx_out (optional) the indices.  codebook NULL (n_embed 0): no quantisation, q = p -- the plain step with a
 *   noise coefficient of its own (temperature != 1).  Same envelope and guarantees as gg_vq_nearest. */
int gg_vq_nearest(const float *rows, int32_t row_stride, const float *codebook, int32_t n_embed, int32_t C, int64_t M,
                  int32_t *idx_out, float *st_out, int32_t st_stride, void *stream);
int gg_ddim_step_vq(float *x, const float *eps, int32_t eps_stride, const float *noise, const float *scalars_dev, int32_t ancestral,
                    const float *codebook, int32_t n_embed, int64_t M, int32_t C, int32_t *idx_out, float *pred_x0_out,
                    void *unet_in, int32_t unet_in_stride, void *stream);

/* Pairwise confusion matrices of label volumes (gg_metrics.hip): the one pass over the voxels behind Dice (ccdm/ddpm/evaluator.py:188-190)
 * and the ensemble scores of ccdm/ddpm/utils.py:190-236 (generalised energy distance, Hungarian-matched IoU), which are fp64 formulas on
 * these counts (jointimagegeneration_amd/metrics.py).  a int32 [Sa, M], b int32 [Sb, M], contiguous, on the device; a == b (self pairs
 * on one buffer) is allowed.
 *   cm_out[i, j, p, q] = #{ m : a[i, m] == p and b[j, m] == q }                      int64 [Sa, Sb, K, K]
 *   skipped_out[i, j]  = #{ m : a[i, m] or b[j, m] outside [0, K) }                  int64 [Sa, Sb], optional (NULL: not reported)
 *   A voxel with a label outside [0, K) is counted in skipped_out alone and never indexes a histogram.  Both outputs are zeroed by the
 *   call (hipMemsetAsync on `stream`, ahead of the launch): a second call into the same buffers gives the same answer.  Exact integer
 *   counts, independent of the order of execution.  A workgroup takes a chunk of voxels and a tile of up to T x T pairs (T from K:
 *   6 for K <= 16, 3 for K = 32) and reads each of its volumes once; uint32 histograms in LDS (a chunk has at most 2^24 voxels),
 *   flushed with 64-bit atomic adds.  GG_CONFUSION_UNIFORM=0 in the environment disables the one-add-per-wave path of waves whose
 *   labels are uniform (measurement switch; same counts).
 *   NULL a, b or cm_out, Sa < 1, Sb < 1, M < 1, K outside [1, 32]: GG_ERR_BAD_SHAPE before any launch.  No allocation, no host
 *   readback, no synchronisation: capturable. */
int gg_label_confusion(const int32_t *a, int32_t Sa, const int32_t *b, int32_t Sb, int64_t M, int32_t K, int64_t *cm_out,
                       int64_t *skipped_out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Cleaning sampled label volumes (gg_components.hip).  gg_label_confusion's rules: labels are contiguous int32 on the
 * device, memory and workspace are the caller's, all work is on the passed stream, no allocation, no host read-back, no
 * synchronisation: capturable.  Integer atomics only: every output is exact and independent of scheduling.  No counterpart in the
 * reference (it hands a raw sample to the CT stage).
 * ------------------------------------------------------------------------------------------------ */
/* Per-voxel vote of S samples: labels [S, M], 1 <= S <= 64, 1 <= K <= 32, 1 <= M < 2^31.
 *   winner    int32 [M]  the most-voted label; on a tie the smallest label among the most voted
 *   agreement int32 [M]  the winner's votes
 *   entropy   fp32 [M]   H = ln S - (1 / S) sum_k c_k ln c_k over the vote counts c_k, formed as
 *                        acc = 0; for k = 0 .. K-1: acc = fp32(acc + table[c_k]);  H = fp32(ln_s - fp32(acc * inv_s))
 *                        (no contraction), with table_dev fp32 [S + 1] on the device, table[c] = fp32(c ln c) computed in fp64
 *                        (table[0] = 0), ln_s = fp32(ln S), inv_s = fp32(1 / S): the caller's three operands, so that a host
 *                        restatement in fp32 gives the same bits
 *   skipped   int64 [1]  votes with a label outside [0, K): they are not cast
 * A voxel with no valid vote gets winner 0, agreement 0, entropy 0. */
int gg_label_vote(const int32_t *labels, int32_t S, int64_t M, int32_t K, const float *table_dev, float ln_s, float inv_s, int32_t *winner,
                  int32_t *agreement, float *entropy, int64_t *skipped, void *stream);
/* Connected components of labels [B, D, H, W] (M = D * H * W < 2^31, B <= 65535, 1 <= K <= 32) under connectivity 6 (faces) or 26
 * (faces, edges, corners).  root int32 [B, M]: for a voxel whose label lies in [0, K) and is not `background` (-1: no background
 * class) the smallest linear index, within its own volume, of its component -- the maximal set of equal-labelled voxels joined under
 * the connectivity; -1 for every other voxel.  Volumes never join and rows never wrap.
 * workspace: gg_label_components_workspace_bytes(B, M) bytes (the union-find's parent array).  status: one int32 on the device that
 * the caller zeroed; a thread whose find or union reaches its bound of M steps (impossible unless the algorithm is wrong) sets it to a
 * non-zero value and returns, and the caller reads it whenever it next reads results back. */
int64_t gg_label_components_workspace_bytes(int32_t B, int64_t M);
int gg_label_components(const int32_t *labels, int32_t B, int32_t D, int32_t H, int32_t W, int32_t K, int32_t connectivity,
                        int32_t background, int32_t *root, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
/* From labels and gg_label_components' root (both [B, M]):
 *   size  int32 [B, M]     the component's voxel count at its root position, 0 elsewhere
 *   stats int64 [B, K, 4]  per class (components, voxels in components, size of the largest, root of the largest; -1 when none);
 *                          among equal sizes the component with the smaller root is the largest */
int gg_component_stats(const int32_t *labels, const int32_t *root, int32_t B, int64_t M, int32_t K, int32_t *size, int64_t *stats,
                       void *stream);
/* out_labels[v] = labels[v] when the class c of v is `background`, or when (keep_largest[c] == 0 or root[v] is the root of c's largest
 * component) and size[root[v]] >= min_size[c]; `fill` (in [0, K)) otherwise, and for a label outside [0, K).  keep_largest, min_size:
 * int32 [K] on the device.  kept uint8 [B, M]: 1 where the label was left as it was. */
int gg_component_filter(const int32_t *labels, const int32_t *root, const int32_t *size, const int64_t *stats, int32_t B, int64_t M,
                        int32_t K, const int32_t *keep_largest, const int32_t *min_size, int32_t background, int32_t fill,
                        int32_t *out_labels, uint8_t *kept, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Surface distances of label volumes (gg_surface.hip): the class borders, an exact Euclidean distance transform and the
 * per-volume reduction that Hausdorff distance, HD95 and the average surface distances are read from (medpy.metric.binary's
 * definitions, the module the reference's evaluator takes dc / precision / recall from).  The rules of the entries above: labels are
 * contiguous int32 [B, D, H, W] on the device (M = D * H * W < 2^31, B <= 65535), memory and workspace are the caller's, all work is on
 * the passed stream, no allocation, no host read-back, no synchronisation: capturable.  No atomics: every output is a fixed function
 * of the inputs, bit for bit, whatever the order the workgroups run in.  Volumes never mix and rows never wrap.
 *
 * gg_label_border: border uint8 [B, M] = 1 where labels[v] lies in [0, K) and some neighbour of v under scipy's
 *   generate_binary_structure(3, connectivity) -- the offsets in {-1, 0, 1}^3 with 1 <= |dd| + |dh| + |dw| <= connectivity; 1: faces,
 *   2: and edges, 3: and corners -- carries another label or lies outside the volume; 0 everywhere else.  For every class c at once this
 *   is m ^ binary_erosion(m, structure, iterations=1, border_value=0) with m = labels == c; an axis of extent 1 makes every voxel of a
 *   class a border voxel.  1 <= K <= 32, connectivity 1, 2 or 3. */
int gg_label_border(const int32_t *labels, int32_t B, int32_t D, int32_t H, int32_t W, int32_t K, int32_t connectivity, uint8_t *border,
                    void *stream);
/* gg_edt_squared: sq fp64 [B, M], sq[v] = min over the sites u of v's own volume of (sd dd)^2 + (sh dh)^2 + (sw dw)^2, +inf in a volume
 *   without sites.  A site is a voxel with labels == cls and border != 0; border == NULL makes every voxel of class cls a site (the
 *   general-purpose form).  sd, sh, sw: finite spacings > 0.  Exact and separable: three passes, along W, H and D, each the lower
 *   envelope of the parabolas of one line, every line staged whole in LDS, each output scanning outwards from its own position until
 *   (s k)^2 alone reaches its best value.  Each term is formed as (s * k) * (s * k) and added without contraction, so with unit spacing
 *   -- or any spacing whose products stay exactly representable -- sq is the integer answer bit for bit.
 *   No extent D, H or W may exceed 1024, the line length the LDS tile is sized for (8192 fp64 values: at least 8 lines of 1024 side by
 *   side): a longer one is GG_ERR_UNSUPPORTED, by name.  workspace: gg_edt_squared_workspace_bytes(B, D, H, W) bytes (one fp64 volume
 *   set, the other side of the passes' ping-pong); 0 for extents outside the supported range. */
int64_t gg_edt_squared_workspace_bytes(int32_t B, int32_t D, int32_t H, int32_t W);
int gg_edt_squared(const int32_t *labels, const uint8_t *border, int32_t cls, int32_t B, int32_t D, int32_t H, int32_t W, double sd,
                   double sh, double sw, double *sq, void *workspace, int64_t workspace_bytes, void *stream);
/* gg_surface_reduce: over the voxels v of volume b with border_a[v] != 0 and labels_a[v] == cls (border_a == NULL: labels_a[v] == cls),
 *   dist2 fp64 [B, M] = sq_b[v] there and -1 at every other voxel; stats fp64 [B, 3] = (their count, the sum of sqrt(sq_b) over them, the
 *   maximum of sq_b over them; (0, 0, -1) when there is none).  Two stages: one workgroup per chunk of 4096 voxels (each thread adds its
 *   16 voxels in index order, the workgroup combines by a fixed tree), then one workgroup per volume adds the chunks' partials in a fixed
 *   order; the chunk count is an argument of the second kernel.  Two runs on one input give the same bits.
 *   workspace: gg_surface_reduce_workspace_bytes(B, M) bytes (three fp64 per chunk). */
int64_t gg_surface_reduce_workspace_bytes(int32_t B, int64_t M);
int gg_surface_reduce(const int32_t *labels_a, const uint8_t *border_a, const double *sq_b, int32_t cls, int32_t B, int64_t M, double *dist2,
                      double *stats, void *workspace, int64_t workspace_bytes, void *stream);

/* Three-view LPIPS of CT volumes (ldm/modules/losses/lpips.py; latentdiffusion/sample_diffusion.py:437-475), gg_lpips.hip: the kernels
 * around the VGG16 convolutions (which are gg_conv_forward / gg_conv_forward_f32 calls).  All three: the caller's stream, no allocation,
 * no synchronisation, capturable.
 * gg_volume_views_cl: x fp32 [B, D, H, W] -> out channels-last [n1 - n0, 1, hh, ww, 32] (GG_BF16 or GG_F32), the images [n0, n1) of one
 *   axis view: view 0 = "(b d) 1 h w" (B * D images of H x W), 1 = "(b h) 1 d w" (B * H images of D x W), 2 = "(b w) 1 d h" (B * W
 *   images of D x H); view 3 reads x as [B, 3, H, W] three-channel images (D must be 3).  Channel c < 3 of a pixel is
 *   (x - shift[c]) / scale[c] (views 0..2: the same x for the three channels, ScalingLayer's broadcast of a 1-channel slice), fp32
 *   subtraction and IEEE fp32 division, rounded once to the output type; channels 3..31 are zero.  shift, scale: device fp32[3].
 *   Views 0, 1, 3 read along W directly; view 2 stages 32 images x 32 pixels through LDS so that reads and writes both stay
 *   coalesced.  An image range outside the view, a view outside 0..3: GG_ERR_BAD_SHAPE.
 * gg_relu_cl: x = max(x, 0) in place on n elements (n % 32 == 0: whole channels-last rows), GG_BF16 or GG_F32.
 * gg_lpips_tap: a, b channels-last [n, h, w, C] (C % 32 == 0, C <= 2048 bf16 / 1024 fp32), the PRE-ReLU conv outputs of the two images
 *   at a tap; lin_w device fp32 [C].  Per image
 *     v = (1 / (h w)) sum_pixels sum_c lin_w[c] * (A_c / (|A| + 1e-10) - B_c / (|B| + 1e-10))^2,  A = relu(a), |A| = sqrt(sum_c A_c^2),
 *   accumulated in fp32 (an all-zero row contributes through 0 / 1e-10 = 0).  tap_out[i] = v (optional); total[i] = v, or total[i] + v
 *   with accumulate != 0 (optional).  pool_a / pool_b (both or neither): [n, h / 2, w / 2, C] = MaxPool2d(2, 2)(relu(.)), floor
 *   semantics, exact.  Deterministic: per-workgroup partial sums (fixed tree), added per image in index order by a second kernel; no
 *   floating-point atomics; the partition depends on (h, w, C, dtype) only, so an image's value does not depend on n.
 *   workspace: gg_lpips_tap_workspace_bytes(n, h, w, C, dtype) bytes (a negative gg_status for a refused shape). */
int gg_volume_views_cl(const float *x, int32_t B, int32_t D, int32_t H, int32_t W, int32_t view, int64_t n0, int64_t n1, const float *shift,
                       const float *scale, void *out, int32_t out_dtype, void *stream);
int gg_relu_cl(void *x, int32_t dtype, int64_t n, void *stream);
int64_t gg_lpips_tap_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t C, int32_t dtype);
int gg_lpips_tap(const void *a, const void *b, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t C, const float *lin_w, void *pool_a,
                 void *pool_b, float *tap_out, float *total, int32_t accumulate, float *workspace, int64_t workspace_bytes, void *stream);

/* Patch-wise evaluation (LatentDiffusion.split_input_params, ddpm.py:573-660), gg_fold.hip.  Geometry of torch.nn.Unfold / Fold with
 * dilation 1 and padding 0: Ly = (H - kh) / sy + 1, Lx = (W - kw) / sx + 1, crop l = ly * Lx + lx starts at (ly * sy, lx * sx); crop l
 * of sample n is row l * N + n of the crop batch.
 * gg_unfold_cl: src channels-last [N, H, W, src_stride] (GG_F32 or GG_BF16, channels [0, C) are read) -> dst channels-last
 *   [L * N, kh, kw, dst_stride], channels [dst_c_offset, dst_c_offset + C); every other lane of dst is left as it is.  A pure copy;
 *   fp32 -> bf16 converts with the cast gg_ddim_step uses for its unet_in rows (fp32 -> fp32, fp32 -> bf16, bf16 -> bf16; any other
 *   pair: GG_ERR_UNSUPPORTED).  Pixels past the last whole crop are not read.
 * gg_fold_weighted_cl: crops fp32 [L * N, kh, kw, crop_stride] -> out fp32 [N, H, W, out_stride], channels [0, C):
 *   out = sum_l(o[l] * w[l]) / sum_l(w[l]) over the crops covering a pixel, w[l][ky, kx] = weight[ky * kw + kx] * tie[l] (that product
 *   rounded to fp32 first; tie NULL: w = weight).  Both sums start from 0.0f and visit the crops in DESCENDING l (descending ly, then
 *   descending lx); every product is rounded before it is added (no contraction); the last operation is an IEEE fp32 division.  This
 *   is the order of ATen's CPU col2im, so identical fp32 crops give the reference's fold(o * weighting) / normalization bit for bit.
 *   A gather (one work item per output pixel and 16-byte channel vector): no atomics, deterministic.  A geometry that leaves a pixel
 *   uncovered ((H - kh) % sy != 0, (W - kw) % sx != 0, or a stride above the crop extent) is GG_ERR_BAD_SHAPE.  Lanes of out past C
 *   are not written.  Both: no allocation, no synchronisation, capturable; unaligned rows take an element-wise path. */
int gg_unfold_cl(const void *src, int32_t src_dtype, int32_t N, int32_t H, int32_t W, int32_t src_stride, int32_t C, void *dst,
                 int32_t dst_dtype, int32_t dst_stride, int32_t dst_c_offset, int32_t kh, int32_t kw, int32_t sy, int32_t sx, void *stream);
int gg_fold_weighted_cl(const float *crops, int32_t crop_stride, const float *weight, const float *tie, float *out, int32_t out_stride,
                        int32_t N, int32_t H, int32_t W, int32_t C, int32_t kh, int32_t kw, int32_t sy, int32_t sx, void *stream);

/* PLMS multistep combination of noise estimates (ldm/models/diffusion/plms.py:218-232), fp32, evaluated left to right:
 *   out = (c0*e0 + c1*e1 + c2*e2 + c3*e3) / denom ; e1..e3 may be NULL (skipped). */
int gg_lincomb4(const float *e0, const float *e1, const float *e2, const float *e3, float c0, float c1, float c2, float c3,
                float denom, int64_t n, float *out, void *stream);

/* Slice normalisation (ds - min)/(max - min) over the whole tensor (latentdiffusion/sample_diffusion.py:222).
 * workspace: >= 2 floats, zero-initialised by the call. */
int gg_minmax_normalise(const float *src, int64_t n, float *dst, float *workspace2, void *stream);

/* Stage glue: CCDM labels -> LDM conditioning slice on the device, replacing the host recipe
 * rot90(scipy.ndimage.zoom(mask, target / shape, order=0), k=3) / 255 (latentdiffusion/sample_diffusion.py:199-200):
 * order-0 zoom of the label volume [N,Dm,Hm,Wm] to (D,H,W) with scipy's index rule (output o reads input
 * floor(o * (in-1)/(out-1) + 0.5) in IEEE double, NOT F.interpolate's floor(o*in/out)), torch.rot90(k=3) on (H,W), value
 * label/255 in channel 1, previous generated slice `prev` fp32 [N,H,W] (or NULL = zeros) in channel 0, remaining lanes of
 * the bf16 CL row zeroed (sample_diffusion.py:208-210). mask_out (optional) receives the fp32 mask slice. */
int gg_mask_to_cond_slice(const int32_t *labels, int32_t N, int32_t Dm, int32_t Hm, int32_t Wm, int32_t slice, int32_t D,
                          int32_t H, int32_t W, const float *prev, void *cond_cl, int32_t stride, float *mask_out,
                          void *stream);

/* Batched slice loop of N independent volumes, each with its own slice window.  schedule_dev: device int32 [iterations][N][3] of
 * (slice, previous slice, active) per sample; iter_dev: device int32[1], the current row (read by both calls, so that one captured graph
 * serves every iteration); volume: fp32 [D][N][H*W], sample n's slice s at (s * N + n) * H * W.
 * gg_mask_to_cond_slices: gg_mask_to_cond_slice of every sample n at its own slice, with prev = volume[prev_n][n]; the same index rule,
 * rot90 and bf16 row, so that each sample's rows are bit-equal to an N = 1 gg_mask_to_cond_slice call (active or not).
 * gg_minmax_normalise_scatter: src fp32 [N][n_per_sample]; sample n is normalised over its own values, bit-equal to gg_minmax_normalise
 * on that sample alone, and written to volume[slice_n][n] only where its row is active.  workspace2n >= 2N floats.  advance != 0: then
 * increments *iter_dev.  A counter outside [0, iterations) makes both calls write nothing. */
int gg_mask_to_cond_slices(const int32_t *labels, int32_t N, int32_t Dm, int32_t Hm, int32_t Wm, int32_t D, int32_t H, int32_t W,
                           const int32_t *schedule_dev, int32_t iterations, const int32_t *iter_dev, const float *volume,
                           void *cond_cl, int32_t stride, void *stream);
int gg_minmax_normalise_scatter(const float *src, int32_t N, int64_t n_per_sample, float *workspace2n, const int32_t *schedule_dev,
                                int32_t iterations, int32_t *iter_dev, int32_t advance, int32_t depth, float *volume, void *stream);

/* CT editing in the batched slice loop: the schedule, the counter and the volume layout of the two calls above.
 * known fp32 and keep uint8 are volumes [D][N][H*W] like `volume`; keep != 0 keeps the known voxel.  All three: vector loads and stores
 * where the extents allow, no atomics on floats, no allocation, no synchronisation, capturable.
 * gg_ct_edit_glue: for each sample n at its own slice, (a) image_cl, the bf16 channels-last first-stage input [N][H*W][stride]: channel 0
 * = the known slice, every other lane 0; (b) latent_keep fp32 [N][lat][lat]: cell (i, j) is 1 iff every pixel of
 * [f (i - margin), f (i + 1 + margin)) x [f (j - margin), f (j + 1 + margin)) that lies inside the image is kept, f = H / lat (pixels
 * outside the image count as kept), else 0.  An inactive row gives a zero image and mask 0.  A counter outside [0, iterations) writes
 * nothing.  H == W, H % lat == 0, f (2 margin + 1) <= H, else GG_ERR_BAD_SHAPE / GG_ERR_UNSUPPORTED.
 * gg_minmax_normalise_keep_scatter: gg_minmax_normalise_scatter with the pixel composite -- the min / max are taken over all of the
 * sample's values as there; of the active row's slice, kept pixels receive known bit for bit, the others the normalised value, bit-equal
 * to gg_minmax_normalise on that sample alone.  advance as there.
 * gg_label_keep_volume: keep[d][n][i][j] = 1 iff the stage glue's label (order-0 zoom of [N,Dm,Hm,Wm] to (D,H,W) by the index rule of
 * gg_mask_to_cond_slice, then rot90(k=3)) of new_labels equals that of old_labels, else 0; the device function of the glue, not a copy. */
int gg_ct_edit_glue(const float *known, const uint8_t *keep, int32_t N, int32_t D, int32_t H, int32_t W, int32_t lat, int32_t margin,
                    const int32_t *schedule_dev, int32_t iterations, const int32_t *iter_dev, void *image_cl, int32_t stride,
                    float *latent_keep, void *stream);
int gg_minmax_normalise_keep_scatter(const float *src, int32_t N, int64_t n_per_sample, float *workspace2n, const int32_t *schedule_dev,
                                     int32_t iterations, int32_t *iter_dev, int32_t advance, int32_t depth, const float *known,
                                     const uint8_t *keep, float *volume, void *stream);
int gg_label_keep_volume(const int32_t *old_labels, const int32_t *new_labels, int32_t N, int32_t Dm, int32_t Hm, int32_t Wm, int32_t D,
                         int32_t H, int32_t W, uint8_t *keep, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Cond stages (ldm/modules/encoders/modules.py:22-136: ClassEmbedder, TransformerEmbedder / BERTEmbedder, SpatialRescaler), gg_cond.hip.
 * All four: no allocation, no synchronisation, capturable; a refused shape is GG_ERR_BAD_SHAPE.
 * ------------------------------------------------------------------------------------------------ */
/* Embedding gather: for each of rows = B * T int32 ids, out[r, d] = tok[ids[r], d] (+ pos[r % T, d] when pos != NULL), d < D.
 * tok fp32 [V, D], pos fp32 [P, D] (T <= P); out: rows of out_stride >= D elements, GG_F32 or GG_BF16; lanes [D, out_stride) are
 * written as zeros.  The add is one fp32 add, then one round-to-nearest-even to bf16.  An id outside [0, V) gives a zero row and
 * reads neither table (the callers check the range on the host; the kernel never reads out of bounds). */
int gg_embed_rows(const int32_t *ids, int64_t rows, int32_t T, const float *tok, int32_t V, int32_t D, const float *pos, int32_t P,
                  void *out, int32_t out_dtype, int32_t out_stride, void *stream);
/* transformers' BertEmbeddings in one launch: out[r, :] = LayerNorm((word[ids[r]] + type[type_ids[r]]) + pos[r % T]), rows = B * T.
 * word fp32 [V, D], pos fp32 [P, D] (T <= P), type fp32 [NT, D], gamma / beta fp32 [D]; type_ids NULL: type 0 everywhere.  Sums and
 * statistics in fp32 (mean, then the centred sum of squares; biased variance; eps from the model's config), one rounding to bf16.
 * out: bf16 rows of out_stride >= D elements, lanes [D, out_stride) written as zeros.  ids_host / type_ids_host: optional HOST copies
 * of the ids (they come from a host tokenizer); an id outside its table there returns GG_ERR_BAD_SHAPE before anything is launched.
 * The device copies are never read back: without the host copies an id outside its table gives a zero row and reads no table, as in
 * gg_embed_rows. */
int gg_bert_embed(const int32_t *ids, const int32_t *type_ids, int64_t rows, int32_t T, const float *word, int32_t V, const float *pos,
                  int32_t P, const float *type, int32_t NT, int32_t D, const float *gamma, const float *beta, float eps, void *out,
                  int32_t out_stride, const int32_t *ids_host, const int32_t *type_ids_host, void *stream);
/* Elementwise erf-form GELU (nn.GELU, F.gelu): bf16 in, bf16 out, fp32 arithmetic, 0.5 x erfc(-x / sqrt 2) (the left tail keeps its
 * relative accuracy).  n > 0 elements, any n; x and out 16-byte aligned. */
int gg_gelu(const void *x, int64_t n, void *out, void *stream);
/* LayerNorm over the first C lanes of bf16 rows `stride` >= C lanes apart (channels-last token rows whose width is padded to a multiple
 * of 32); lanes [C, stride) of out are written as zeros.  gamma, beta fp32 [C]; fp32 arithmetic in gg_layernorm's order.  Not in place. */
int gg_layernorm_rows(const void *x, int64_t rows, int32_t C, int32_t stride, const float *gamma, const float *beta, float eps, void *out,
                      void *stream);
/* torch.nn.functional.interpolate(x, scale_factor=s, mode=...) with align_corners=False and no recompute_scale_factor on `planes` =
 * N * C independent fp32 H x W planes (NCHW in, NCHW out), as ATen's fp32 CPU kernels compute it.  The caller passes the output extent
 * Ho = floor(H * s), Wo = floor(W * s) (the product in double) and the coordinate scales scale_h = scale_w = float(1.0 / s) -- the value
 * ATen uses when a scale factor is given, NOT H / Ho.  mode:
 *   0 nearest:  source index min(floorf(dst * scale), in - 1) per axis
 *   1 bilinear: src = scale * (dst + 0.5) - 0.5, clamped below at 0; i0 = min(int(src), in - 1), i1 = i0 + 1 only when i0 < in - 1,
 *               weights (1 - l, l) with l = src - i0; (row i0 interpolated along W) * (1 - ly) + (row i1 ...) * ly
 *   2 bicubic:  the same src NOT clamped, i = floorf(src), t = src - i, four taps i - 1 .. i + 2 with indices clamped to [0, in - 1]
 *               and the cubic convolution weights of A = -0.75; rows along W first, then along H, taps added in ascending order
 *   3 area:     adaptive average pooling, window [floor(i * in / out), ceil((i + 1) * in / out)) per axis (integer arithmetic), summed
 *               in row-major order in fp32, then sum / kh / kw (two IEEE divisions, ATen's order); the scales are not read
 * Every source index is clamped into the plane, whatever the scales. */
int gg_interpolate2d_f32(const float *src, int64_t planes, int32_t H, int32_t W, int32_t Ho, int32_t Wo, float scale_h, float scale_w,
                         int32_t mode, float *dst, void *stream);

/* Rendering of sampled volumes (gg_render.hip): the picture latentdiffusion/sample_diffusion.py:241-261 saves, bit for bit.  Both: the
 * caller's stream, no allocation, no workspace, no atomics on global memory, no synchronisation: capturable.
 * gg_mask_overlay: combine_mask_and_im (sample_diffusion.py:23-58).  x fp32 [N, 2, D, H, W] (channel 0 the CT, channel 1 the mask as
 *   label / 11), out fp32 [N, D, 3, H, W], both contiguous on the device; colors: 12 x 3 int32 on the HOST (read during the call).  Per
 *   voxel, every step one correctly rounded fp32 operation (nothing is contracted into an FMA):
 *     image = 255 * clamp(x0, 0, 1);  m = x1 * 11, and m = 11 where m == 255
 *     colored = colors[trunc(m)] where m > 0, image where m == 0 (and 0 where m < 0);  im = colored * coef + image * rest, with
 *     coef = (float)overlay_coef and rest = (float)(1.0 - overlay_coef), the two Python floats of the reference
 *     out = colors[i] when the voxel is a boundary voxel of class i, the lowest such i in 1..11; im otherwise
 *   Boundary voxel of class i: with b = (m == i) and zeros outside the volume, one of the three integer Sobel responses of b ([-1, 0, 1]
 *   along one axis, [1, 2, 1] along the two others) is non-zero -- what scipy.ndimage.sobel(mode='constant') leaves in a bool array.
 *   trunc(m) outside 0..11 is the caller's error (the reference raises IndexError); the kernel clamps the index and never reads outside
 *   the table.  Tiles of 8 x 8 x 64 voxels with a one-voxel halo of class ids in LDS; no extent need be a multiple of the tile; a tile
 *   whose halo holds one class id skips the stencil.
 * gg_make_grid_u8: torchvision.utils.make_grid(imgs, nrow, padding, pad_value) followed by permute(1, 2, 0) and .astype(uint8).  imgs
 *   fp32 [B, C, H, W], C 1 (repeated to three channels) or 3; out uint8 [Hg, Wg, 3].  B == 1: the image itself (Hg = H, Wg = W, no
 *   padding).  Otherwise xmaps = min(nrow, B), ymaps = ceil(B / xmaps), Hg = ymaps * (H + padding) + padding, Wg = xmaps * (W + padding)
 *   + padding, image k at (k / xmaps * (H + padding) + padding, k % xmaps * (W + padding) + padding), pad_value elsewhere.  The cast
 *   truncates toward zero and saturates to [0, 255] (NaN gives 0).
 *   N, D, H, W, B < 1, C outside {1, 3}, nrow < 1, padding < 0, a null pointer: GG_ERR_BAD_SHAPE before any launch. */
int gg_mask_overlay(const float *x, int32_t N, int32_t D, int32_t H, int32_t W, double overlay_coef, const int32_t *colors, float *out,
                    void *stream);
int gg_make_grid_u8(const float *imgs, int32_t B, int32_t C, int32_t H, int32_t W, int32_t nrow, int32_t padding, float pad_value,
                    uint8_t *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Held-out objectives, forward only (gg_loss.hip): noise a sample to step t, run ONE UNet forward, reduce.  All four: the caller's
 * stream, caller-owned buffers, no allocation, no readback, no floating-point atomics: capturable, and two runs on the same input
 * give the same bits (every reduction: fp32 term -> fp64 sum per workgroup -> one fp64 partial in the workspace -> a second launch adds
 * the partials in index order).  gg_loss_workspace_bytes(N, rows_per_sample) is enough workspace for either reduction.
 * Replaces: q_sample + get_loss + mean of p_losses and the integrand of _prior_bpd (ldm/models/diffusion/ddpm.py:275-322,1011-1058);
 * q_xt_given_x0(x0, t).sample(), theta_post, kl_div and cross_entropy of ccdm/ddpm/trainer.py:299-327.
 * ------------------------------------------------------------------------------------------------ */
typedef enum { GG_LOSS_L2 = 0, GG_LOSS_L1 = 1, GG_LOSS_PRIOR_KL = 2 } gg_loss_mode;
int64_t gg_loss_workspace_bytes(int32_t N, int64_t rows_per_sample);
/* x_noisy[n] = s0[n] * x[n] + s1[n] * noise[n]: two multiplies and one add, each rounded to fp32 (nothing contracted), which is q_sample
 * on the CPU.  x, noise fp32 [N, C, S] (NC(D)HW); scalars_dev fp32 [N, 2] = (s0, s1).  out: fp32 [N, C, S] or NULL.  unet_in: channels
 * [0, C) of a channels-last [N * S, unet_in_stride] buffer of unet_in_dtype (GG_BF16, or GG_F32 in validation mode) or NULL; other lanes
 * are not touched.  At least one output. */
int gg_q_sample_rows(const float *x, const float *noise, const float *scalars_dev, int32_t N, int32_t C, int64_t S, float *out,
                     void *unet_in, int32_t unet_in_dtype, int32_t unet_in_stride, void *stream);
/* out[n] (fp64) = mean over the C * S elements of sample n of
 *   GG_LOSS_L2        (target - pred)^2          GG_LOSS_L1   |target - pred|
 *   GG_LOSS_PRIOR_KL  0.5 * (-1 - lv + exp(lv) + m^2),  m = s[n] * x_start, scalars_dev fp32 [N, 2] = (s, lv); pred / target unused
 * pred: the UNet head's fp32 channels-last output [N * S, pred_stride], C logical channels; target, x_start fp32 [N, C, S].  Every term is
 * computed in fp32 (nothing contracted).  workspace: gg_loss_workspace_bytes(N, S). */
int gg_loss_rows(const float *pred, int32_t pred_stride, const float *target, const float *x_start, const float *scalars_dev, int32_t mode,
                 int32_t N, int32_t C, int64_t S, double *out, void *workspace, int64_t workspace_bytes, void *stream);
/* Forward categorical noising of labels: p_c = keep[n] * [c == x0] + unif[n] / K, pn_c = p_c / sum(p) (summed left to right),
 * label = argmax_c pn_c / E_c (first maximum on a tie).  x0 int32 [M], sample n = row / rows_per_sample; mix_dev fp32 [N, 2] = (keep,
 * unif): (cumalphas[t_n - 1], 1 - cumalphas[t_n - 1]) for q(x_t | x_0), (1 - betas[t_n - 1], betas[t_n - 1]) for q(x_t | x_{t-1}) -- the
 * reference's own two operands, so that neither is re-derived from the other in fp32.  E: fp32 [M, K] exponentials, or NULL: Philox4x32-10 with key philox_seeds_dev[n] (uint64 [N]) and the counter of
 * gg_ccdm_posterior_sample_seeds (row within the sample, draw index, philox_offset_dev[0] or 0).  labels_out int32 [M]; onehot_out: bf16
 * rows [M, onehot_stride], channels [0, K) written, or NULL.  2 <= K <= 16. */
int gg_ccdm_q_sample(const int32_t *x0, const float *mix_dev, int64_t rows_per_sample, int32_t K, const float *E,
                     const uint64_t *philox_seeds_dev, const int64_t *philox_offset_dev, int64_t M, int32_t *labels_out, void *onehot_out,
                     int32_t onehot_stride, void *stream);
/* Mask editing of the CCDM reverse chain (the blend of ldm/models/diffusion/ddim.py:144-148 with the categorical operands of
 * diffusion_denoising.py:82-89): every row m with keep[m] != 0 takes labels[m] = a draw of q(x_t | x_0 = known[m]), formed and drawn
 * exactly as gg_ccdm_q_sample does (same expressions, same order, first maximum on a tie); a row with keep[m] == 0 is not written at
 * all, neither its label nor its one-hot row.
 *   labels     int32 [M], in/out: only rows with keep != 0 are written, none is read
 *   known      int32 [M] in 0 .. K-1 (the caller's check; a value outside reads nothing out of bounds).  known may be the labels buffer
 *              itself: a row reads its known label before it writes, so kept rows are then re-noised in place
 *   keep       uint8 [M], non-zero = keep the known value
 *   mix_dev    fp32 [N, 2] = (keep, unif) of sample n = m / rows_per_sample, read on the device: (cumalphas[t-1], 1 - cumalphas[t-1]) at
 *              step t; (1, 0) returns known on the kept rows whatever is drawn
 *   E          fp32 [M, K] exponentials (rows with keep == 0 unused), or NULL: Philox4x32-10 with gg_ccdm_draw_tape's counter and
 *              philox_offset_dev[0] (0 when NULL); philox_seeds_dev == NULL: key philox_seed, row = m (gg_ccdm_posterior_sample's rule);
 *              else key philox_seeds_dev[n], row = m % rows_per_sample (gg_ccdm_posterior_sample_seeds' rule)
 *   onehot_out bf16 rows [M, onehot_stride] or NULL: channels [0, K) of the kept rows written, channels >= K never
 * 2 <= K <= 32 (16 or 32 exponentials drawn per row, as the posterior kernel).  No allocation, no synchronisation: one launch that a
 * captured step can hold, since the mix row and the offset are read from device memory.
 * GG_ERR_BAD_SHAPE: labels, known, keep or mix_dev NULL; K outside [2, 32]; M < 1, rows_per_sample < 1 or M not a multiple of
 * rows_per_sample; onehot_out with onehot_stride < K, an odd onehot_stride or rows that are not 4-byte aligned. */
int gg_ccdm_inpaint_blend(int32_t *labels, const int32_t *known, const uint8_t *keep, const float *mix_dev, int64_t rows_per_sample,
                          int32_t K, const float *E, uint64_t philox_seed, const uint64_t *philox_seeds_dev,
                          const int64_t *philox_offset_dev, int64_t M, void *onehot_out, int32_t onehot_stride, void *stream);
/* out fp64 [N, 2] = per-sample sums over the voxels of (class_weights[x0] * KL, CE), trainer.py:305-320 with its quirks kept:
 *   p = softmax(logits);  q_pred = max(theta_post_prob(xt, p), 1e-12) NOT renormalised;  q_true = theta_post(xt, x0);
 *   KL = sum_c (q_true > 0 ? q_true * log(q_true) : 0) - q_true * log(q_pred);  CE = cross_entropy(p, x0) on the PROBABILITIES.
 * logits fp32 [M, logits_stride]; xt, x0 int32 [M]; scalars_dev fp32 [N, 2] = (alphas[t-1], cumalphas[t-2]), (0, 1) at t == 1;
 * class_weights fp32 [K]; 2 <= K <= 16.  workspace: gg_loss_workspace_bytes(N, rows_per_sample). */
int gg_ccdm_step_loss(const float *logits, int32_t logits_stride, const int32_t *xt, const int32_t *x0, const float *scalars_dev,
                      int64_t rows_per_sample, const float *class_weights, int32_t K, int64_t M, double *out, void *workspace,
                      int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * The first stage's held-out objective, forward only (gg_patchgan.hip): what LPIPSWithDiscriminator of
 * ldm/modules/losses/contperceptual.py needs beyond gg_lpips_tap and gg_loss_rows.  Same rules as above: the caller's stream,
 * caller-owned buffers and workspace, no allocation, no readback, no floating-point atomics; the reductions are two-stage fp64 sums in
 * a fixed order (two runs give the same bits).
 * ------------------------------------------------------------------------------------------------ */
/* PatchGAN convolution (NLayerDiscriminator / NLayerDiscriminator3D, contperceptual.py:296-406): kernel extent 4 on H and W, and on D when
 * kd == 4 (kd == 1: 2-D, the D axis is a batch axis), zero padding 2 on both sides of every 4-wide axis, one stride in {1, 2} on them:
 * Ho = H / stride + 1 (Wo, and Do for kd == 4, alike; Do = D for kd == 1).  src: channels-last bf16 [N, D, H, W, Cin_pad], Cin_pad % 32 == 0;
 * weight: gg_conv_pack_weight with ntaps = 16 * kd; out: channels-last [N, Do, Ho, Wo, pad32(Cout)] of out_dtype, pad lanes zero.
 * bf16 MFMA with fp32 accumulation, then in fp32, each step rounded once: y = acc * alpha[c] + beta[c] (alpha NULL: y = acc + beta[c]),
 * y = y >= 0 ? y : y * slope (slope == 1: none).  alpha, beta: fp32 [pad32(Cout)], the conv bias and the eval-mode BatchNorm folded by
 * the caller: alpha = gamma / sqrt(running_var + eps), beta = (bias - running_mean) * alpha + beta_bn.
 * The _f32 form (validation mode) takes fp32 src, fp32 weight [taps][Cin_pad][pad32(Cout)] and accumulates with fp32 FMA, taps outer,
 * channels inner.  A wrong extent, Cin_pad % 32, a stride outside {1, 2}, kd outside {1, 4}, a null pointer: GG_ERR_* before any launch. */
int gg_patch_conv_forward(const void *src, const void *weight, const float *alpha, const float *beta, float slope, int32_t N, int32_t D,
                          int32_t H, int32_t W, int32_t Cin_pad, int32_t Cout, int32_t kd, int32_t stride, int32_t Do, int32_t Ho, int32_t Wo,
                          void *out, int32_t out_dtype, void *stream);
int gg_patch_conv_forward_f32(const float *src, const float *weight, const float *alpha, const float *beta, float slope, int32_t N, int32_t D,
                              int32_t H, int32_t W, int32_t Cin_pad, int32_t Cout, int32_t kd, int32_t stride, int32_t Do, int32_t Ho,
                              int32_t Wo, float *out, void *stream);
/* DiagonalGaussianDistribution.kl() (distributions.py:44-51): out[n] (fp64) = 0.5 * sum over the C * S elements of sample n of
 * m^2 + exp(lv) - 1 - lv, lv clamped to [-30, 20], every term in fp32 (left to right, nothing contracted; exp rounded to fp32 from its
 * fp64 value).  moments: fp32 channels-last rows [N * S, stride], mean in lanes [0, C), logvar in lanes [C, 2C).
 * workspace: gg_loss_workspace_bytes(N, S). */
int gg_gauss_kl_rows(const float *moments, int32_t stride, int32_t N, int32_t C, int64_t S, double *out, void *workspace,
                     int64_t workspace_bytes, void *stream);
/* DiagonalGaussianDistribution.sample() (distributions.py:35-37): z = m + exp(0.5 * lv) * noise with the same clamp, each step rounded to
 * fp32.  moments as above; noise fp32 [N, C, S].  out: fp32 [N, C, S] or NULL; z_in: channels [0, C) of a channels-last
 * [N * S, z_in_stride] buffer of z_in_dtype (GG_BF16, or GG_F32 in validation mode) or NULL, other lanes untouched.  At least one output. */
int gg_gauss_sample_rows(const float *moments, int32_t stride, const float *noise, int32_t N, int32_t C, int64_t S, float *out, void *z_in,
                         int32_t z_in_dtype, int32_t z_in_stride, void *stream);
/* out fp64 [5] = means over the M logits l of  l, relu(1 - l), relu(1 + l), softplus(-l), softplus(l)  (hinge_d_loss / vanilla_d_loss /
 * g_loss of contperceptual.py:14-25,140; softplus as F.softplus: x > 20 ? x : log1p(exp(x))).  logits: lane 0 of fp32 rows [M, stride].
 * Each term in fp32.  workspace: 5 doubles per workgroup; gg_loss_workspace_bytes(3, M) is enough. */
int gg_logit_stats(const float *logits, int32_t stride, int64_t M, double *out, void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * fp32 VALIDATION mode of the CCDM path (gg_f32.hip): the same network functions on fp32 channels-last tensors with fp32 weights
 * and fp32 FMA accumulation in a fixed order, so that integer outputs (labels) can be compared exactly with the fp32 CPU
 * reference (the reference's own precision switch: ccdm/ddpm/models/unet_openai/unet.py:447,742-756).  Not a fast path.
 * ------------------------------------------------------------------------------------------------ */
/* gg_conv_desc with fp32 tensors: src1 / src2 / residual / out are fp32 CL, out_dtype must be GG_F32, `weight` is fp32
 * [taps][C1+C2][Cout_pad] (tap-major, zero padded), bias as in gg_conv_forward; prologue_act, gn_acc, ddim_x, epilogue_geglu must be 0. */
int gg_conv_forward_f32(const gg_conv_desc *desc, void *stream);
/* act(GroupNorm(32)(cat[src1, src2])) on fp32 CL tensors: statistics in fp64, (x - mean) * rstd * gamma + beta in fp32 (ATen's
 * order), act 1 = SiLU with an IEEE division.  out fp32 CL [N, S, C1+C2] (pad lanes zero); workspace: 64 * N floats. */
int gg_groupnorm_f32(const float *src1, int32_t C1, const float *src2, int32_t C2, int32_t N, int64_t S, int32_t C_logical,
                     const float *gamma, const float *beta, float eps, int32_t act, float *out, float *workspace, void *stream);
/* gg_attention_desc with fp32 q / k / v / out (head_dim <= 64): softmax((q a)(k a)^T) v, a = sqrt(scale), all fp32. */
/* The ResBlock out-norm under use_scale_shift_norm in the reference's order: act(GroupNorm(32)(src) * (1 + s) + t) with s = film[n, c],
 * t = film[n, C_logical + c] (film fp32, row stride film_stride >= 2 * C_logical), every step rounded to fp32; single source.  out fp32 CL
 * [N, S, C_pad] (pad lanes zero); workspace: 64 * N floats. */
int gg_groupnorm_f32_film(const float *src, int32_t C_pad, int32_t N, int64_t S, int32_t C_logical, const float *gamma, const float *beta,
                          float eps, const float *film, int64_t film_stride, int32_t act, float *out, float *workspace, void *stream);
int gg_attention_forward_f32(const gg_attention_desc *desc, void *stream);
/* gg_attention_forward_kvlen on the fp32 validation kernel (head_dim <= 64): the key loop of sample n ends at kv_len[n]. */
int gg_attention_forward_kvlen_f32(const gg_attention_desc *desc, const int32_t *kv_len, void *stream);

/* ------------------------------------------------------------------------------------------------
 * On-box peak measurements for the benchmark's roofline (gg_ubench.hip; SURVEY.md 8d, BASELINE.md 3: fractions are quoted against
 * the vendor peaks AND against what this box delivers).  Measurement infrastructure: nothing on the sampling path calls them.
 * No counterpart in the reference (it publishes no numbers: README.md:1-41).
 * ------------------------------------------------------------------------------------------------ */
/* Register-resident bf16 MFMA loop on every CU: cus * waves_per_simd workgroups of 256 threads, `iters` iterations of 262 144 FLOP
 * per wave (shape 0: 16 x v_mfma_f32_16x16x32_bf16, shape 1: 8 x v_mfma_f32_32x32x16_bf16), random non-zero operands.  The caller
 * times the launch with events on `stream`; *flops_out (host) receives the FLOP count of the launch.  sink: >= 1 float (device). */
int gg_ubench_mfma_bf16(int32_t shape, int32_t iters, int32_t waves_per_simd, float *sink, double *flops_out, void *stream);
/* 16 bytes per lane grid-stride copy src -> dst (device pointers, 16-byte aligned, bytes % 16 == 0): moves 2 * bytes through HBM. */
int gg_ubench_stream_copy(const void *src, void *dst, int64_t bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GUIDEGEN_HIP_H */
