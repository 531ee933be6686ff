"""CPU suite: the gate of the streaming 1x1 tile kernel (csrc/gg_conv_tile.hip) is host logic -- gg_conv_runs_tile reads no pointer and makes
no HIP call.  The seven 1x1 skip projections of the CCDM UNet @128^3 and @64^3 answer "taken"; their siblings at 32^3, 16^3 and 8^3, the
stride-2 convs (which stay on the gather kernel), every descriptor under path_hint 12 and everything with a prologue, a residual, fp32
output or a fused epilogue answer "not taken".  The other dispatch predicates keep their answers for these shapes."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from util import load_lib
    return load_lib()


def desc(N, sp, C1, C2, cout, k=1, stride=1, hint=0, **extra):
    from jointimagegeneration_amd import _lib, ops
    d = _lib.ConvDesc()
    d.N, (d.D, d.H, d.W) = N, sp
    d.C1, d.C2, d.Cout, d.Cout_pad = C1, C2, cout, ops.pad32(cout)
    d.kd = d.kh = d.kw = k
    d.stride, d.pad = stride, (1 if k == 3 else 0)
    d.Do, d.Ho, d.Wo = ops.conv_out_extent(sp, (k, k, k), stride, d.pad, False)
    d.path_hint = hint
    for f, v in extra.items():
        setattr(d, f, v)
    return d


# the seven launches of one CCDM forward the kernel is for: (cube, C1, C2, Cout)
TAKEN = [(128, 128, 64, 64), (128, 64, 64, 64), (128, 64, 64, 64), (64, 128, 128, 128), (64, 128, 128, 128), (64, 128, 64, 128), (64, 64, 0, 128)]


def test_the_seven_skip_projections_are_taken(lib):
    for cube, C1, C2, cout in TAKEN:
        d = desc(1, (cube,) * 3, C1, C2, cout)
        assert lib.gg_conv_runs_tile(C.byref(d)) == 1, (cube, C1, C2, cout)
        # its own family: the answers the dispatch fixture pins for these shapes stay what they were
        assert lib.gg_conv_runs_halo_tile(C.byref(d)) == 0 and lib.gg_conv_emits_stats(C.byref(d)) == 0
        assert lib.gg_conv_workspace_bytes(C.byref(d)) == 0 and lib.gg_conv_fuses_prologue(C.byref(d)) == 0
        d.path_hint = 12
        assert lib.gg_conv_runs_tile(C.byref(d)) == 0


def test_small_grids_and_other_convs_are_not_taken(lib):
    from jointimagegeneration_amd._lib import GG_F32
    for cube in (32, 16, 8):
        for _, C1, C2, cout in TAKEN:
            assert lib.gg_conv_runs_tile(C.byref(desc(1, (cube,) * 3, C1, C2, cout))) == 0, (cube, C1, C2, cout)
    assert lib.gg_conv_runs_tile(C.byref(desc(2, (32, 64, 64), 128, 64, 64))) == 1                 # the gate: 64^3 = 262144 positions
    assert lib.gg_conv_runs_tile(C.byref(desc(1, (64, 64, 63), 128, 64, 64))) == 0
    assert lib.gg_conv_runs_tile(C.byref(desc(1, (32, 32, 32), 128, 128, 128))) == 0               # @32^3 the gather kernel was measured faster
    for cube, c in ((128, 64), (64, 128), (32, 128), (16, 256)):                                       # the stride-2 convs stay on the gather kernel
        assert lib.gg_conv_runs_tile(C.byref(desc(1, (cube,) * 3, c, 0, c, k=3, stride=2))) == 0
    base = dict(N=1, sp=(64, 64, 64), C1=128, C2=128, cout=128)
    assert lib.gg_conv_runs_tile(C.byref(desc(**base))) == 1
    for extra in (dict(prologue_act=1), dict(prologue_act=2), dict(residual=64), dict(out_dtype=GG_F32), dict(epilogue_geglu=1), dict(skip_C1=64),
                  dict(ddim_x=64), dict(post_xt=64), dict(stride=2), dict(k=3)):
        kw = dict(base)
        kw.update({f: v for f, v in extra.items() if f in ("stride", "k")})
        rest = {f: v for f, v in extra.items() if f not in ("stride", "k")}
        assert lib.gg_conv_runs_tile(C.byref(desc(**kw, **rest))) == 0, extra
    # channel counts outside the instantiated set, 2-D token grids of other widths
    assert lib.gg_conv_runs_tile(C.byref(desc(1, (64, 64, 64), 192, 0, 128))) == 0                 # 192 channels in ONE source: no power of two
    assert lib.gg_conv_runs_tile(C.byref(desc(1, (64, 64, 64), 256, 128, 128))) == 0
    assert lib.gg_conv_runs_tile(C.byref(desc(1, (64, 64, 64), 128, 128, 256))) == 0
