"""CPU suite: the gate of the stride-2 3x3x3 tile kernel (gg_conv_runs_tile_s2, csrc/gg_conv.hip + gg_conv_tile.hip) is host logic.  The two
128-cout Downsample conv of the CCDM UNet's 64^3 level answers yes; 64 couts (a measured tie), 32^3 -> 16^3 and deeper, where the gather kernel splits K (and is then no bit
reference for a one-pass kernel), answer no, as does everything under path_hint 12 / 14.  The shapes of tests/test_conv_tile_s2_gpu.py are
checked here against the gather plan: no K split (gg_conv_workspace_bytes == 0) wherever the comparison is word for word."""
import ctypes as C

import pytest

from test_conv_tile_cpu import desc


@pytest.fixture(scope="module")
def lib():
    from util import load_lib
    return load_lib()


def s2(N, sp, C1, cout, hint=0, C2=0, **kw):
    return desc(N, sp, C1, C2, cout, k=3, stride=2, hint=hint, **kw)


def test_the_128_cout_downsample_is_taken(lib):
    # 64 -> 64 @128^3 was measured a tie with the gather kernel (172 us both): 64 couts are not instantiated
    assert lib.gg_conv_runs_tile_s2(C.byref(s2(1, (128,) * 3, 64, 64))) == 0
    for cube, c in ((64, 128),):
        d = s2(1, (cube,) * 3, c, c)
        assert lib.gg_conv_runs_tile_s2(C.byref(d)) == 1, (cube, c)
        assert lib.gg_conv_workspace_bytes(C.byref(d)) == 0 and lib.gg_conv_runs_halo_tile(C.byref(d)) == 0
        assert lib.gg_conv_emits_stats(C.byref(d)) == 0 and lib.gg_conv_runs_tile(C.byref(d)) == 0 and lib.gg_conv_fuses_prologue(C.byref(d)) == 0
        for hint in (12, 14):
            assert lib.gg_conv_runs_tile_s2(C.byref(s2(1, (cube,) * 3, c, c, hint=hint))) == 0


def test_split_k_grids_and_other_convs_are_not_taken(lib):
    from jointimagegeneration_amd._lib import GG_F32
    no = lambda d: lib.gg_conv_runs_tile_s2(C.byref(d)) == 0
    for cube, c in ((32, 128), (16, 256), (8, 320)):
        d = s2(1, (cube,) * 3, c, c)
        assert no(d) and (cube == 8 or lib.gg_conv_workspace_bytes(C.byref(d)) > 0)
    # the smallest grids that the gather kernel runs in one pass: 192 blocks of 128 positions for 64 and for 128 couts
    assert lib.gg_conv_runs_tile_s2(C.byref(s2(1, (32, 64, 96), 64, 128))) == 1 and lib.gg_conv_workspace_bytes(C.byref(s2(1, (32, 64, 96), 64, 128))) == 0
    assert lib.gg_conv_runs_tile_s2(C.byref(s2(1, (32, 64, 96), 128, 128))) == 1 and lib.gg_conv_runs_tile_s2(C.byref(s2(1, (32, 64, 96), 128, 100))) == 1
    assert lib.gg_conv_runs_tile_s2(C.byref(s2(2, (16, 64, 96), 128, 128))) == 1 and lib.gg_conv_workspace_bytes(C.byref(s2(2, (16, 64, 96), 128, 128))) == 0
    assert no(s2(1, (16, 32, 96), 128, 128)) and lib.gg_conv_workspace_bytes(C.byref(s2(1, (16, 32, 96), 128, 128))) > 0      # 48 blocks: split K
    assert lib.gg_conv_runs_tile_s2(C.byref(s2(1, (16, 32, 96), 128, 128, hint=15))) == 1                                       # (tests: gate lifted)
    assert lib.gg_conv_runs_tile_s2(C.byref(s2(1, (8, 8, 32), 64, 128, hint=15))) == 1 and no(s2(1, (8, 8, 32), 64, 64, hint=15))
    base = dict(N=1, sp=(32, 64, 96), C1=64, cout=128)
    for extra in (dict(prologue_act=1), dict(prologue_act=2), dict(epilogue_geglu=1), dict(skip_C1=64), dict(ddim_x=64), dict(post_xt=64),
                  dict(hint=12), dict(hint=14), dict(hint=1), dict(hint=13 + 100)):
        assert no(s2(**base, **extra)), extra
    assert lib.gg_conv_runs_tile_s2(C.byref(s2(**base, residual=64))) == 1 and lib.gg_conv_runs_tile_s2(C.byref(s2(**base, out_dtype=GG_F32))) == 1
    assert lib.gg_conv_runs_tile_s2(C.byref(s2(**base, hint=13))) == 1                            # (13 switches the split halo path off, nothing else)
    assert no(s2(1, (32, 64, 94), 64, 128)) and no(s2(1, (32, 60, 96), 64, 128)) and no(s2(1, (34, 64, 96), 64, 128))     # output extents off the 2x4x16 tile
    assert no(s2(1, (31, 64, 96), 64, 128))                                                        # odd input extent
    assert no(s2(1, (64, 64, 96), 32, 32)) and no(s2(1, (32, 64, 96), 64, 256)) and no(s2(1, (32, 64, 96), 64, 64))      # Cout_pad 128 only
    assert no(desc(1, (32, 64, 96), 64, 0, 128, k=3, stride=1)) and no(desc(1, (32, 64, 96), 64, 0, 128, k=1, stride=2))
    p0 = s2(1, (32, 64, 96), 64, 128)
    p0.pad = 0
    assert no(p0)
