"""CPU suite: the gate of the split halo path (gg_conv_runs_halo_split, csrc/gg_conv.hip) is host logic -- it reads no pointer and makes no
HIP call.  It answers with the number of K slabs (0: the path declines), which must be the split the gather plan chose, because the
workspace is still sized by gg_conv_workspace_bytes.

The five 3x3x3 shapes of the CCDM UNet's 16^3 level answer yes at batch 1.  At batch 2 the same shapes answer NO: their grid is then large
enough for the halo-tile kernel's own gate (gg_conv_runs_halo_tile == 1, recorded in tests/golden/conv_dispatch.json), gg_conv_forward asks
that kernel first, and it also leaves GroupNorm statistics there, which a split path cannot.  Batch 2 reaches the split path at half the
depth, (8, 16, 16), which has the batch-1 16^3 level's position count.
"""
import ctypes as C

import pytest

from test_conv_tile_cpu import desc

# (C1, C2) of the eleven launches' five distinct shapes; all to 256 couts
CCDM_16 = [(128, 0), (256, 0), (320, 256), (256, 256), (256, 128)]
HINT_OFF = 13


@pytest.fixture(scope="module")
def lib():
    from util import load_lib
    return load_lib()


def slabs_of_workspace(lib, d):
    M = d.N * d.Do * d.Ho * d.Wo
    ws = lib.gg_conv_workspace_bytes(C.byref(d))
    assert ws % (M * d.Cout_pad * 4) == 0
    return ws // (M * d.Cout_pad * 4)


def d3(N, sp, C1, C2, cout, **kw):
    return desc(N, sp, C1, C2, cout, k=3, **kw)


def test_ccdm_16_level_is_taken_at_batch_1(lib):
    for C1, C2 in CCDM_16:
        d = d3(1, (16, 16, 16), C1, C2, 256)
        s = lib.gg_conv_runs_halo_split(C.byref(d))
        assert s == 2, (C1, C2, s)
        assert s == slabs_of_workspace(lib, d)
        assert ((C1 + C2) // 32) % s == 0
        # the recorded predicates keep the parent's answers for these shapes
        assert lib.gg_conv_runs_halo_tile(C.byref(d)) == 0 and lib.gg_conv_emits_stats(C.byref(d)) == 0
        assert lib.gg_conv_runs_tile(C.byref(d)) == 0 and lib.gg_conv_fuses_prologue(C.byref(d)) == 0
        assert lib.gg_conv_workspace_bytes(C.byref(d)) == 2 * 4096 * 256 * 4
        # residual and fp32 output are the reduce kernel's business: same answer
        from jointimagegeneration_amd._lib import GG_F32
        assert lib.gg_conv_runs_halo_split(C.byref(d3(1, (16, 16, 16), C1, C2, 256, residual=64))) == 2
        assert lib.gg_conv_runs_halo_split(C.byref(d3(1, (16, 16, 16), C1, C2, 256, out_dtype=GG_F32))) == 2
        assert lib.gg_conv_runs_halo_split(C.byref(d3(1, (16, 16, 16), C1, C2, 256, hint=HINT_OFF))) == 0
        off = d3(1, (16, 16, 16), C1, C2, 256, hint=HINT_OFF)
        assert lib.gg_conv_workspace_bytes(C.byref(off)) == lib.gg_conv_workspace_bytes(C.byref(d))
        assert lib.gg_conv_runs_halo_tile(C.byref(off)) == 0 and lib.gg_conv_emits_stats(C.byref(off)) == 0


def test_batch_2(lib):
    for C1, C2 in CCDM_16:
        d = d3(2, (16, 16, 16), C1, C2, 256)
        # the halo-tile kernel's own gate passes (128 workgroups): gg_conv_forward never gets as far as the split path
        assert lib.gg_conv_runs_halo_tile(C.byref(d)) == 1 and lib.gg_conv_emits_stats(C.byref(d)) == 32
        assert lib.gg_conv_runs_halo_split(C.byref(d)) == 0
        h = d3(2, (8, 16, 16), C1, C2, 256)
        s = lib.gg_conv_runs_halo_split(C.byref(h))
        assert s == 2 and s == slabs_of_workspace(lib, h) and lib.gg_conv_runs_halo_tile(C.byref(h)) == 0


def test_other_splits(lib):
    # splits that plan_gather derives for smaller grids: one chunk per slab, and four slabs
    for N, sp, C1, cout, want in ((1, (4, 8, 16), 512, 256, 16), (1, (8, 16, 16), 128, 256, 4), (1, (8, 8, 16), 256, 256, 8)):
        d = d3(N, sp, C1, 0, cout)
        s = lib.gg_conv_runs_halo_split(C.byref(d))
        assert s == want == slabs_of_workspace(lib, d), (sp, C1, cout, s)
        assert (C1 // 32) % s == 0


def test_declined(lib):
    no = lambda d: lib.gg_conv_runs_halo_split(C.byref(d)) == 0
    assert no(d3(1, (8, 8, 8), 320, 0, 256))                                   # 160-step gather; W = 8 is no multiple of the box either
    assert no(d3(1, (8, 8, 16), 320, 0, 320))                                  # 160-step gather on a grid the box divides
    assert no(d3(1, (32, 32, 32), 256, 0, 256))                                # the halo-tile kernel takes it
    assert lib.gg_conv_runs_halo_tile(C.byref(d3(1, (32, 32, 32), 256, 0, 256))) == 1
    d = d3(1, (4, 4, 16), 64, 0, 32)                                           # splitk 6, nchunk 2: a slab would end inside a chunk
    assert slabs_of_workspace(lib, d) == 6 and no(d)
    assert no(d3(1, (16, 16, 16), 64, 0, 64))                                  # splitk 8 (64 gather blocks), nchunk 2
    assert no(d3(1, (16, 16, 15), 256, 0, 256)) and no(d3(1, (16, 18, 16), 256, 0, 256)) and no(d3(1, (18, 16, 16), 256, 0, 256))
    assert no(d3(1, (4, 4, 4), 256, 0, 256))                                   # tiny-M kernel
    base = dict(N=1, sp=(16, 16, 16), C1=256, C2=0, cout=256)
    assert lib.gg_conv_runs_halo_split(C.byref(d3(**base))) == 2
    for extra in (dict(prologue_act=1), dict(prologue_act=2), dict(upsample=1), dict(epilogue_geglu=1), dict(skip_C1=64), dict(ddim_x=64),
                  dict(post_xt=64), dict(hint=HINT_OFF), dict(hint=1), dict(hint=4), dict(hint=7)):
        assert no(d3(**base, **extra)), extra
    assert no(desc(1, (16, 16, 16), 256, 0, 256, k=3, stride=2))
    assert no(desc(1, (16, 16, 16), 256, 0, 256, k=1))
    k133 = desc(1, (16, 16, 16), 256, 0, 256, k=3)
    k133.kd, k133.Do = 1, 16
    assert no(k133)
