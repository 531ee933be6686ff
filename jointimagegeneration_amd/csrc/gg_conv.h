// Shared between gg_conv.hip (generic gather kernel) and gg_conv_halo.hip (halo-tile kernel).
#pragma once
#include "gg_common.h"

struct ConvParams {
    int N, D, H, W, C1, C2, Cout, Cout_pad;
    int kd, kh, kw, stride, pad, upsample;
    int Do, Ho, Wo, out_dtype, prologue_act;
    int path_hint;            // gg_conv_desc.path_hint (0: production; halo kernel: GG_HALO_HINT_*; box kernel: GG_BOX_HINT_*, below)
    int nchunk1, nchunk, ntaps;
    long long M;              // N*Do*Ho*Wo
    long long bias_stride;
    const bf16_t *src1, *src2, *weight, *residual;
    const float *bias, *gn_scale, *gn_shift;
    void *out;
    float *ws;                // split-K slabs [splitk][M][Cout_pad] fp32 (splitk > 1)
    int splitk;
    long long *gn_acc;        // per-channel fixed-point (sum, sumsq) accumulators of the outputs [N][Cout_pad][2], or nullptr
    float *ddim_x, *ddim_pred_x0;      // fused DDIM epilogue of the UNet head conv (gg_conv_desc.ddim_x), box kernel only
    const float *ddim_scalars;
    bf16_t *ddim_unet_in;
    long long ddim_unet_in_stride;
    // multiply-high magics (gg_fastdiv) of the output-position decode m -> (n, od, oh, ow); 0 where M * divisor >= 2^32
    unsigned mg_osp, mg_ohw, mg_wo;
    int epi_geglu;            // gg_conv_desc.epilogue_geglu (generic gather kernel without split-K only)
    // GroupNorm prologue from accumulators (gg_conv_desc.pro_acc1; box kernel only)
    const long long *pro_acc1, *pro_acc2;
    const float *pro_gamma, *pro_beta;
    float pro_eps;
    int pro_clog;
    // K-concatenated 1x1 skip projection (gg_conv_desc.skip_src1; box kernel, 3x3 stride 1 only)
    const bf16_t *skip_src1, *skip_src2, *skip_weight;
    int skip_C1, skip_C2;
    // fused CCDM reverse step of the UNet head conv (gg_conv_desc.post_xt; halo-tile kernel, 1024-position 3-D box only)
    const int *post_xt;
    int *post_labels_out;
    const float *post_scalars, *post_E;
    unsigned long long post_seed;
    const long long *post_offset_dev;
    bf16_t *post_onehot_out;
    long long post_onehot_stride;
    int post_draw;
    const unsigned long long *post_seeds;     // per-sample Philox keys [N] or nullptr (post_seed for every sample)
    long long post_rows_per_sample;
};

// path_hint values of the box kernel (tests, A/B): run the generic kernel even where a shape-specialised one is listed / fail a box conv
// that has no shape-specialised kernel
#define GG_BOX_HINT_GENERIC 10
#define GG_BOX_HINT_SPEC_ONLY 11
// path_hint values of the halo-tile kernel (tests, A/B; 0 is production).  The first four lift the grid-fill gate, so that small shapes run
// on the kernel; the BOX ones also fix the box size wherever that size is instantiated.
#define GG_HALO_HINT_BOX512 1
#define GG_HALO_HINT_BOX256 4
#define GG_HALO_HINT_BOX1024 6
#define GG_HALO_HINT_TEAM 7        /* the team kernel (gg_conv_halo3.hip) wherever its envelope allows */
#define GG_HALO_HINT_NO_TEAM 8     /* production dispatch without the team kernel */
// path_hint of the tile kernels (gg_conv_tile.hip; tests, A/B): production dispatch in every other respect, but the tile kernels decline,
// so that their shapes run on the gather kernel as they did before
#define GG_CONV_HINT_GATHER 12
// path_hint of the split halo path (gg_conv_runs_halo_split; tests, A/B): production dispatch in every other respect, but that path declines,
// so that its shapes run on the split gather kernel as they did before
#define GG_CONV_HINT_NO_HALO_SPLIT 13
// path_hint of the stride-2 tile kernel (gg_conv_runs_tile_s2; tests, A/B): production dispatch with that kernel switched off (12 does the same)
#define GG_CONV_HINT_NO_TILE_S2 14
// tests only: the stride-2 tile kernel wherever its shape envelope allows, whatever the gather plan says (small shapes for the fp64 exact regimes)
#define GG_CONV_HINT_TILE_S2 15
static inline bool gg_hint_is_production(int hint)
{
    return hint == 0 || hint == GG_CONV_HINT_GATHER || hint == GG_CONV_HINT_NO_HALO_SPLIT || hint == GG_CONV_HINT_NO_TILE_S2;
}

// fixed-point scales of the GroupNorm accumulators: |sum| < 2^35, sumsq < 2^43 per channel and sample
#define GG_ACC_SUM_SCALE 268435456.0f   /* 2^28 */
#define GG_ACC_SQ_SCALE 1048576.0f      /* 2^20 */
// accumulators of the box / 160-step kernels: [N][GG_ACC_STRIPES][C][2].  One stripe: at most a few dozen position tiles add to
// one address, and every block of gn_apply_acc re-reads all stripes (4 stripes: 1606 us per latent-UNet forward, 1 stripe: 1595)
#ifndef GG_ACC_STRIPES
#define GG_ACC_STRIPES 1
#endif
// the halo-tile kernel (thousands of workgroups per launch) stripes 32-way: at most P/32 workgroups add to one address
#define GG_ACC_STRIPES_HALO 32

// 16-byte chunk swizzle for 64-byte LDS rows read by ds_read_b128 with lane -> (row = r0 + (l&15), chunk = l>>4).
// chunk ^ ((row>>1)&2) puts the 16 lanes of every ds_read_b128 lane group ({0-3,12-15,20-27}, {4-11,16-19,28-31}, +32) on 16
// distinct 16-byte slots of the 256-byte bank row for EVERY start row r0 (exhaustive search over r0 = 0..15):
// the shifted reads of the conv taps (row offsets +1, +18, +180) stay conflict-free, not only the aligned ones.
__device__ __forceinline__ int swz64(int row, int chunk) { return chunk ^ ((row >> 1) & 2); }


// Sum over the 16 lanes of a row (lanes with equal l >> 4) with DPP moves only: quad xor 1, quad xor 2, half-row mirror, row
// mirror.  Every lane of the row ends up with the row total (fixed order: deterministic).  4 VALU ops instead of 4 ds_bpermute.
__device__ __forceinline__ float gg_row16_sum(float x)
{
    x += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    x += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    x += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x141, 0xF, 0xF, true));   // row_half_mirror
    x += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x140, 0xF, 0xF, true));   // row_mirror
    return x;
}

// ---- the bf16 / fp32 epilogue value of the single-pass kernels (conv_gather_kernel, gg_conv_tile.hip), stated once so that the two cannot
// drift: accumulator + bias row (+ residual), channels beyond Cout zeroed; then round-to-nearest-even to bf16.
__device__ __forceinline__ f32x4 gg_conv_epi_value(f32x4 acc, bool has_bias, f32x4 bv, bool has_res, bf16x4 res, int co, int Cout)
{
    f32x4 v = acc;
    if (has_bias) v += bv;
    if (has_res) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] += (float)res[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (co + j >= Cout) v[j] = 0.f;
    return v;
}
__device__ __forceinline__ bf16x4 gg_conv_epi_bf16(f32x4 v)
{
    bf16x4 ob;
#pragma unroll
    for (int j = 0; j < 4; ++j) ob[j] = (bf16_t)v[j];
    return ob;
}

// ---- host entry points of the conv units, each declared here once; conv_walk (gg_conv.hip) asks them in gg_conv_forward's one order.
// *_try: GG_OK where the kernel takes the conv, GG_ERR_UNSUPPORTED (silently, no error text) where it declines; launch == false plans and returns
int gg_conv_halo_try(const ConvParams &p, hipStream_t stream, bool launch);        // halo-tile kernel (gg_conv_halo.hip)
int gg_conv_halo3_try(const ConvParams &p, hipStream_t stream, bool launch);       // team kernel for filled 3-D grids (gg_conv_halo3.hip), asked by gg_conv_halo_try
int gg_conv_box_try(const ConvParams &p, hipStream_t stream, bool launch);         // box-resident 2-D kernel for under-filled grids (gg_conv_box.hip)
int gg_conv_tile_try(const ConvParams &p, hipStream_t stream, bool launch);        // streaming 1x1 tile kernel (gg_conv_tile.hip)
bool gg_conv_halo_prefers_separate_norm(const ConvParams &p);                       // kernel-specific rules, for a conv that the kernel takes
bool gg_conv_halo_fuses_posterior(const ConvParams &p);
bool gg_conv_box_fuses_prologue(const ConvParams &p);
bool gg_conv_box_emits_stats(const ConvParams &p);
bool gg_conv_box_prologue_from_acc(const ConvParams &p);
int gg_conv_tile_family(const ConvParams &p);                                       // 0 = declines, 1 = streaming 1x1
// stride-2 3x3x3 tile kernel (gg_conv_tile.hip): the shape envelope, and the launch for a shape that conv_walk has vetted
bool gg_conv_tile_s2_family(const ConvParams &p);
int gg_conv_tile_s2_launch(const ConvParams &p, hipStream_t stream);
// one K slab per blockIdx.z on the 256-position 3-D halo box (gg_conv_halo.hip): p.splitk slabs of whole chunks into p.ws, no epilogue
bool gg_conv_halo_split_box_fits(const ConvParams &p);
int gg_conv_halo_split_launch(const ConvParams &p, hipStream_t stream);
// tiny-M weight-streaming kernel (gg_conv_tiny.hip): plan returns 0 (not applicable) or the K split
int gg_conv_tiny_plan(long long M, int Cout_pad, int KS, int prologue_act);
int gg_conv_tiny_launch(const ConvParams &p, hipStream_t stream);
int gg_conv_box_spec_launch(const ConvParams &p, const struct BoxPlan &pl, hipStream_t stream);       // gg_conv_box_spec.hip, asked by gg_conv_box_try
