// Shape-specialised box convs for the latent UNet's batch-1 layers (BoxSpec, gg_conv_box_kernel.h).
//
// At batch 1 a box-conv wave issues 1400-2200 instructions, 900-1300 of them scalar bookkeeping on values that are fixed for the layer
// (the block decode by multiply-high magics, stage and unit ranges, the (kh, chunk) walk, kernel-argument loads, feature branches), one
// by one at ~2 ns each: the instruction stream, not data, is the critical path.  Every configuration that the batch-1 latent UNet
// runs is listed in gg_conv_box_specs.inc (tools/gen_box_specs.py) and compiled with all of it as constants.  The table is keyed on
// the shape, the plan plan_box chose and the feature set; a launch whose (params, plan) match an entry exactly runs that entry, every
// other one the generic kernel.  path_hint GG_BOX_HINT_GENERIC forces the generic kernel (tests, A/B), GG_BOX_HINT_SPEC_ONLY makes a
// box conv without an entry an error (tests: the table covers the layers).
#include <stdio.h>
#include <stdlib.h>
#include "gg_conv_box_kernel.h"

static int box_up(const ConvParams &p) { return p.stride == 2 ? 2 : p.upsample ? 1 : 0; }

template <class S>
static bool box_spec_matches(const ConvParams &p, const BoxPlan &pl)
{
    return p.N == 1 && p.H == S::H && p.W == S::W && p.C1 == S::C1 && p.C2 == S::C2 && p.Cout == S::Cout && p.Cout_pad == S::Cout_pad &&
           p.Ho == S::Ho && p.Wo == S::Wo && (p.kh == 3 ? 1 : 0) == S::K3 && box_up(p) == S::UP &&
           pl.TWI == S::TWI && pl.MT == S::MT && pl.CT == S::CT && pl.NS == S::NS && pl.nstage == S::nstage && pl.nch_stage == S::nch_stage &&
           pl.gn_bytes == S::gn_bytes && pl.q_major == S::q_major &&
           p.skip_C1 == S::skip_C1 && p.skip_C2 == S::skip_C2 && pl.nstage_s == S::nstage_s && pl.nch_stage_s == S::nch_stage_s &&
           p.prologue_act == S::pro && (p.pro_acc1 != nullptr) == S::acc && (p.bias != nullptr) == S::bias && (p.residual != nullptr) == S::res &&
           (p.gn_acc != nullptr) == S::stats && (p.out_dtype == GG_F32) == S::out_f32 && (p.ddim_x != nullptr) == S::ddim &&
           (p.ddim_pred_x0 != nullptr) == S::ddim_px0 && (p.ddim_unet_in != nullptr) == S::ddim_uin;
}

template <class S>
static int box_spec_launch(const ConvParams &p, const BoxPlan &pl, hipStream_t stream)
{
    return launch_box<S::TWI, S::MT, S::CT, S::UP, S::K3, S::SK, S::NS, S>(p, pl, stream);
}

struct BoxSpecEntry {
    bool (*match)(const ConvParams &, const BoxPlan &);
    int (*launch)(const ConvParams &, const BoxPlan &, hipStream_t);
};

#define GG_BOX_SPEC(...) {&box_spec_matches<BoxSpec<__VA_ARGS__>>, &box_spec_launch<BoxSpec<__VA_ARGS__>>},
static const BoxSpecEntry box_specs[] = {
#include "gg_conv_box_specs.inc"
};
#undef GG_BOX_SPEC

// GG_BOX_SPEC_TRACE=1 (tools/gen_box_specs.py): every batch-1 box launch prints its table key to stderr
static void box_spec_trace(const ConvParams &p, const BoxPlan &pl)
{
    static const int on = getenv("GG_BOX_SPEC_TRACE") != nullptr;
    if (!on || p.N != 1) return;
    fprintf(stderr, "GG_BOX_SPEC(%d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d)\n",
            p.H, p.W, p.C1, p.C2, p.Cout, p.Cout_pad, p.Ho, p.Wo, p.kh == 3 ? 1 : 0, box_up(p), pl.TWI, pl.MT, pl.CT, pl.NS, pl.nstage, pl.nch_stage,
            pl.gn_bytes, pl.q_major, p.skip_C1, p.skip_C2, pl.nstage_s, pl.nch_stage_s, p.prologue_act, p.pro_acc1 != nullptr, p.bias != nullptr,
            p.residual != nullptr, p.gn_acc != nullptr, p.out_dtype == GG_F32, p.ddim_x != nullptr, p.ddim_pred_x0 != nullptr, p.ddim_unet_in != nullptr);
}

// GG_ERR_UNSUPPORTED (silently): no entry for this launch, the caller runs the generic kernel.  (GG_BOX_HINT_SPEC_ONLY fails with
// GG_ERR_BAD_SHAPE instead: UNSUPPORTED would send gg_conv_forward on to the next kernel family.)
int gg_conv_box_spec_launch(const ConvParams &p, const BoxPlan &pl, hipStream_t stream)
{
    box_spec_trace(p, pl);
    if (p.path_hint == GG_BOX_HINT_GENERIC) return GG_ERR_UNSUPPORTED;
    for (const BoxSpecEntry &e : box_specs)
        if (e.match(p, pl)) return e.launch(p, pl, stream);
    if (p.path_hint == GG_BOX_HINT_SPEC_ONLY)
        GG_FAIL(GG_ERR_BAD_SHAPE, "conv: box conv %dx%d %d+%d -> %d (k%d up %d) has no shape-specialised kernel (path_hint %d)", p.H, p.W, p.C1, p.C2,
                p.Cout, p.kh, box_up(p), GG_BOX_HINT_SPEC_ONLY);
    return GG_ERR_UNSUPPORTED;
}
