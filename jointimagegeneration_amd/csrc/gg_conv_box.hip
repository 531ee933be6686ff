// Box-resident 2-D convolution for UNDER-FILLED grids (latent UNet levels at batch 1: 64x64 .. 16x16, 160..1280 channels):
// 3x3 (stride 1, pad 1, optional fused nearest x2 upsample) and 1x1, bf16 in / fp32 accumulate on v_mfma_f32_16x16x32_bf16.
//
// These layers are 1-8 GFLOP each: neither MFMA nor HBM bound, but bound by (1) what ONE CU can take in (tools/experiments/
// ubench_intake.hip: 48 GB/s per CU for 64-byte rows, 70 for 128-byte lines, ~80 contiguous, L2-resident, 240 workgroups) and (2) the
// number of instructions a wave has to issue, one by one, in front of and between its memory instructions (~2 ns each at one or two
// waves per SIMD: phase stamps, -DGG_BOX_STAMPS).  The kernel therefore moves the minimum number of bytes into each CU, has every
// byte of the box in flight at once, has no barrier in its main loop, and keeps its scalar bookkeeping out of the inner loops:
//   * a workgroup (8 waves) owns MT position tiles (16 positions each: 1x16, 2x8 or 4x4, so 8x8 and 4x4 levels fit too) x 16*CT
//     output channels; the plan (plan_box) picks MT and CT so that max-over-CUs of (weight slice + input box) bytes is smallest for
//     a single round of <= 256 workgroups; block ids decode by multiply-high with host-provided magics, and the arguments the
//     first DMAs need are pinned into one scalar-load batch (gg_pin);
//   * the input box the 9 taps touch ((TH+2) x 18 rows; upsample: (TH/2+2) x 10) is staged into LDS ONCE for ALL input channels
//     of a stage (<= 128 KiB; two-source concat and zero padding applied here) as one swizzled 64-byte-row plane per 32-channel
//     chunk, by global_load_lds (1 KiB = 16 rows per wave instruction, no VGPRs).  Units (16-row block, chunk) are walked
//     block-major in runs: consecutive chunks are +64 B in memory (the two halves of a 128-byte line go out back to back) and
//     +PLANE in LDS, 6.5 instructions per unit; padding slots are zeroed by the issuing wave after its DMAs have landed.
//     GroupNorm affine (* SiLU), where fused (<= 2 cout tiles per box), then runs IN PLACE in LDS, once per staged element;
//   * the k-steps of the stage are split evenly over the 8 waves as (kh, chunk) units with the three kw taps unrolled (kw is a
//     compile-time constant: operand addresses are lane constant + uniform + immediate, the bookkeeping is paid once per three
//     k-steps).  Each wave streams the weight tiles of ITS units straight from L2 into VGPRs (ring of 2 units, counted vmcnt; no
//     LDS copy, no redundancy between waves; deeper rings are slower: the stream is intake-bound) and reads the activation operand
//     from the LDS box at a shifted row, all MT reads of a k-step ahead of its MFMAs;
//   * the partial accumulators of the 8 waves are combined through LDS in a fixed order (deterministic), then bias / residual /
//     store (+ GroupNorm sums of the next norm, + the fused DDIM update on the UNet head);
//   * workgroups are renumbered so that the ones sharing a weight slice (weight-heavy layers) or an input box
//     (activation-heavy layers) run on the same XCD and hit its L2 (blockIdx round-robins over the 8 XCDs).
#include "gg_conv_box_kernel.h"

// Cost model: bytes one CU has to take in (its weight slice + its input box), times the number of rounds the grid needs on
// 256 CUs.  Smallest wins; ties go to the larger tile (fewer redundant halo bytes overall).
static bool plan_box(const ConvParams &p, BoxPlan &pl)
{
    constexpr long long max_blocks = 1024, lds_cap = 131072;     // <= 4 rounds of 256 workgroups; box + GroupNorm rows <= 128 KiB
    const bool k3 = p.kh == 3 && p.kw == 3 && p.pad == 1, k1 = p.kh == 1 && p.kw == 1 && p.pad == 0 && !p.upsample;
    const bool s2 = GG_BOX_STRIDE2 && p.stride == 2 && k3 && !p.upsample && p.skip_C1 == 0;      // the UNet's Downsample convs
    if (!(p.kd == 1 && p.D == 1 && (p.stride == 1 || s2) && (k3 || k1))) return false;
    const int halo = k3 ? 2 : 0;
    // 1x1: only where the grid is under-filled (measured: 8x8 4.2 vs 8.6 us on the tiny-M kernel, but 64x64 12.0 vs 7.8 us on gather5)
    constexpr long long k1_max_m = 256;
    // ... unless the conv folds a GroupNorm from accumulators itself: then the box kernel also replaces the norm's launch
    const long long k1_lim = (p.prologue_act && p.pro_clog > 0) ? GG_BOX_K1_MAX_M_ACC : k1_max_m;
    if (k1 && p.M > k1_lim) return false;
    const int TWI = p.Wo % 16 == 0 ? 16 : p.Wo % 8 == 0 ? 8 : p.Wo % 4 == 0 ? 4 : 0;   // width of a 16-position MFMA tile
    if (!TWI) return false;
    const int RPT = 16 / TWI;
    const long long wbytes16 = 16LL * (k3 ? 9 : 1) * p.nchunk * 32 * 2;   // weight slice of 16 output channels
    double best = 0;
    int bMT = 0, bCT = 0, bNS = 1;
    // tile heights: powers of two, plus 12 / 6 / 3 rows for 16-wide tiles so that 240 (not 160 or 320) workgroups cover the
    // 64 / 32 / 16-row levels; the last row tile may be ragged (rows >= Ho are computed on zero padding and not stored)
    for (int MT : {12, 8, 6, 4, 3, 2, 1}) {
        const int TH = MT * RPT;
        if ((p.upsample && (TH & 1)) || TH > p.Ho) continue;
        if (TWI != 16 && (MT == 12 || MT == 6 || MT == 3 || p.Ho % TH)) continue;
        if ((TWI == 16 && MT == 1) || (TWI == 8 && MT == 8) || (TWI == 4 && MT != 1)) continue;   // instantiated shapes only
        const int rows = p.upsample ? (TH / 2 + 2) * (TWI / 2 + 2) : s2 ? (2 * TH + 1) * (2 * TWI + 1) : (TH + halo) * (TWI + halo);
        const long long boxb = (long long)rows * p.nchunk * 64;
        for (int CT : {2, 1}) {
            const long long blocks = (long long)p.N * ((p.Ho + TH - 1) / TH) * (p.Wo / TWI) * (p.Cout_pad / (16 * CT));
            if (blocks > max_blocks || (GG_BOX_NW == 8 && MT * CT > 16 ? 4LL : (long long)(GG_BOX_NW < 8 ? GG_BOX_NW : 8)) * MT * CT * 1024 > lds_cap) continue;      // grid cap; the combine area (8 slabs, or 4 in two phases) must fit
            // every extra LDS stage is another exposed staging round trip
            const long long plane_c = (long long)((rows + 15) / 16) * 1024;
            const long long cap_c = lds_cap / plane_c > 0 ? lds_cap / plane_c : 1;
            const long long nst = (p.nchunk + cap_c - 1) / cap_c;
            const double cost = (double)(wbytes16 * CT + boxb) * (double)((blocks + 255) / 256) * (1.0 + 0.15 * (double)(nst - 1));
            if (!bMT || cost < best * 0.97) { best = cost; bMT = MT; bCT = CT; bNS = 1; }
            // cout sub-split (weight-bound 3x3 convs of the 8x8 / 4x4 levels; instantiated shapes only): NS workgroups per 16-cout tile,
            // each taking in 1 / NS of its weight rows and the whole box
            if (GG_BOX_COUT_SUBSPLIT && CT == 1 && k3 && !p.upsample && !s2 && ((TWI == 4 && MT == 1) || (TWI == 8 && MT == 2)))
                for (int NS : {2, 4}) {
                    if (blocks * NS > 256) continue;                       // one round only
                    const double cs = (double)(wbytes16 / NS + boxb) * (1.0 + 0.15 * (double)(nst - 1));
                    if (cs < best * 0.97) { best = cs; bMT = MT; bCT = CT; bNS = NS; }
                }
        }
    }
    if (!bMT) return false;                                          // filled grids: the halo / wide-tile kernels win
    const int MT = bMT, CT = bCT, NS = bNS, TH = MT * RPT;
    const int rows = p.upsample ? (TH / 2 + 2) * (TWI / 2 + 2) : s2 ? (2 * TH + 1) * (2 * TWI + 1) : (TH + halo) * (TWI + halo);
    const long long plane = (long long)((rows + 15) / 16) * 1024;   // whole 16-row DMA blocks
    long long cap = lds_cap / plane;
    if (cap < 1) return false;
    const int nstage = (int)((p.nchunk + cap - 1) / cap);
    if (TWI == 4 && nstage > 1) return false;                        // 4x4 levels with > 1 stage: the split-K tiny kernel fills more CUs
    const int nch_stage = (p.nchunk + nstage - 1) / nstage;
    long long smem = nch_stage * plane;
    const long long red = (GG_BOX_NW == 8 && MT * CT > 16 ? 4LL : (long long)GG_BOX_NW) * MT * CT * 64 * 16;      // [wave][tt][ct][lane] f32x4 (two-phase combine above 16 tiles)
    if (smem < red) smem = red;
    // scale / shift rows in front of the box: external tables are DMA'd per stage, the accumulator fold keeps all chunks of the conv
    const int gn_bytes = p.prologue_act ? ((p.pro_acc1 ? p.nchunk : nch_stage) * 32 * 8 + 1023) / 1024 * 1024 : 0;
    // XCD locality: a run of workgroups shares weights (cout-major) when the weights are the bigger re-fetch, else boxes
    const long long P = (long long)p.N * ((p.Ho + TH - 1) / TH) * (p.Wo / TWI), Q = p.Cout_pad / (16 * CT);
    const long long wtot = wbytes16 * (p.Cout_pad / 16), xtot = (long long)p.N * p.H * p.W * p.nchunk * 64;
    const long long cost_q = wtot + xtot * (Q < 8 ? Q : 8), cost_p = wtot * (P < 8 ? P : 8) + xtot;
    // K-concatenated 1x1 skip projection: stages of the x tile (MT KiB per chunk) in the same region
    int nstage_s = 0, nch_stage_s = 0;
    if (p.skip_C1 > 0) {
        if (!k3 || p.upsample || p.skip_C1 % 32 || p.skip_C2 % 32) return false;
        const long long plane1 = (long long)MT * 1024, nck = (p.skip_C1 + p.skip_C2) / 32;
        const long long cap1 = lds_cap / plane1;
        nstage_s = (int)((nck + cap1 - 1) / cap1);
        nch_stage_s = (int)((nck + nstage_s - 1) / nstage_s);
        if (smem < nch_stage_s * plane1) smem = nch_stage_s * plane1;
    }
    pl = {TWI, MT, CT, nstage, nch_stage, gn_bytes, cost_q <= cost_p ? 1 : 0, smem + gn_bytes, nstage_s, nch_stage_s, NS};
    return true;
}

template <int CT, int UP, int K3, int SK = 0>
static int dispatch_box(const ConvParams &p, const BoxPlan &pl, hipStream_t stream)
{
    switch (pl.TWI * 10 + pl.MT) {
        case 172: return launch_box<16, 12, CT, UP, K3, SK>(p, pl, stream);
        case 168: return launch_box<16, 8, CT, UP, K3, SK>(p, pl, stream);
        case 166: return launch_box<16, 6, CT, UP, K3, SK>(p, pl, stream);
        case 163: return launch_box<16, 3, CT, UP, K3, SK>(p, pl, stream);
        case 164: return launch_box<16, 4, CT, UP, K3, SK>(p, pl, stream);
        case 162: return launch_box<16, 2, CT, UP, K3, SK>(p, pl, stream);
        case 84: return launch_box<8, 4, CT, UP, K3, SK>(p, pl, stream);
        case 82:
            if constexpr (CT == 1 && UP == 0 && K3 == 1) {
                if (pl.NS == 2) return launch_box<8, 2, CT, UP, K3, SK, 2>(p, pl, stream);
                if (pl.NS == 4) return launch_box<8, 2, CT, UP, K3, SK, 4>(p, pl, stream);
            }
            return pl.NS == 1 ? launch_box<8, 2, CT, UP, K3, SK>(p, pl, stream) : GG_ERR_UNSUPPORTED;
        case 81: return launch_box<8, 1, CT, UP, K3, SK>(p, pl, stream);
        case 41:
            if constexpr (CT == 1 && UP == 0 && K3 == 1) {
                if (pl.NS == 2) return launch_box<4, 1, CT, UP, K3, SK, 2>(p, pl, stream);
                if (pl.NS == 4) return launch_box<4, 1, CT, UP, K3, SK, 4>(p, pl, stream);
            }
            return pl.NS == 1 ? launch_box<4, 1, CT, UP, K3, SK>(p, pl, stream) : GG_ERR_UNSUPPORTED;
        default: return GG_ERR_UNSUPPORTED;
    }
}

// The in-place prologue activates the whole box once per workgroup, i.e. once per cout tile: with Q cout tiles it is Q x 1.4
// times the work of a separate GroupNorm-apply launch, and transcendental-bound (2 per element).  Fusing pays only when few
// cout tiles share a box (measured: Q = 5 breaks even with the 3 us apply launch, Q = 20 costs +6 us).
bool gg_conv_box_fuses_prologue(const ConvParams &p)
{
    constexpr int fuse_q = 2;
    BoxPlan pl;
    if (!plan_box(p, pl)) return false;
    return p.Cout_pad / (16 * pl.CT) <= fuse_q;
}

bool gg_conv_box_emits_stats(const ConvParams &p) { return p.out_dtype != GG_F32; }

// Prologue computed from accumulators inside the conv (gg_conv_desc.pro_acc1).  The fold itself is ~0.5 us per workgroup; what decides
// is the in-place transform, redone by every cout tile that shares a box: an affine-only norm (attention / SpatialTransformer: no
// SiLU) is a handful of VALU per 16-byte piece and always pays against the ~4.5 us GroupNorm launch it removes; a SiLU norm is
// transcendental-bound (2 per element) and pays only where few cout tiles share a box (as with external tables) or the workgroup's box
// is small (GG_BOX_ACC_SILU_MAX_ELEMS elements; A/B in tools/experiments/README.md).
bool gg_conv_box_prologue_from_acc(const ConvParams &p)
{
    BoxPlan pl;
    if (!plan_box(p, pl) || p.C1 + p.C2 > 2048 || !p.prologue_act) return false;
    if (p.prologue_act == 2) return true;
    // SiLU norm: what a workgroup pays is the in-place pass over ITS box (rows x input channels, 2 transcendentals per element)
    const int RPT = 16 / pl.TWI, TH = pl.MT * RPT;
    const long long rows = p.upsample ? (long long)(TH / 2 + 2) * (pl.TWI / 2 + 2) : (long long)(TH + 2 * (p.kh == 3)) * (pl.TWI + 2 * (p.kw == 3));
    constexpr long long silu_max_elems = GG_BOX_ACC_SILU_MAX_ELEMS;
    return p.Cout_pad / (16 * pl.CT) <= 2 || rows * (p.C1 + p.C2) <= silu_max_elems;
}

// the box rung of conv_walk (contract: gg_conv.h)
int gg_conv_box_try(const ConvParams &p, hipStream_t stream, bool launch)
{
    BoxPlan pl;
    if (!plan_box(p, pl)) return GG_ERR_UNSUPPORTED;
    if (!launch) return GG_OK;
    const int rs = gg_conv_box_spec_launch(p, pl, stream);     // a batch-1 latent-UNet layer listed in gg_conv_box_specs.inc
    if (rs != GG_ERR_UNSUPPORTED) return rs;
    if (p.skip_C1 > 0) return pl.CT == 2 ? dispatch_box<2, 0, 1, 1>(p, pl, stream) : dispatch_box<1, 0, 1, 1>(p, pl, stream);     // (plan_box: 3x3, no upsample)
    if (p.kh == 1) return pl.CT == 2 ? dispatch_box<2, 0, 0>(p, pl, stream) : dispatch_box<1, 0, 0>(p, pl, stream);
    if (p.stride == 2) return pl.CT == 2 ? dispatch_box<2, 2, 1>(p, pl, stream) : dispatch_box<1, 2, 1>(p, pl, stream);
    if (pl.CT == 2) return p.upsample ? dispatch_box<2, 1, 1>(p, pl, stream) : dispatch_box<2, 0, 1>(p, pl, stream);
    return p.upsample ? dispatch_box<1, 1, 1>(p, pl, stream) : dispatch_box<1, 0, 1>(p, pl, stream);
}
