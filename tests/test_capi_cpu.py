"""CPU suite: the C-ABI library loads and exports every symbol include/guidegen_hip.h declares (no compute calls)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "guidegen_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as ge
    from jointimagegeneration_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    lib = _lib.load()
    syms = declared_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in guidegen_hip.h but not exported"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature in _lib.py"
    assert lib.gg_version() >= 100


def test_product_refuses_cpu_tensors():
    """No CPU fallback: the product path must fail loudly off-GPU."""
    import torch
    from jointimagegeneration_amd.unet import UNetModel
    from util import LDM_SMALL
    u = UNetModel(**LDM_SMALL).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        u(torch.zeros(1, 8, 16, 16), torch.tensor([1]))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "jointimagegeneration_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f"{f} imports the oracle"


def _desc(lib_mod, N, D, H, W, cin, cout, k, stride=1, pad=1, upsample=False, out_f32=False, act=0):
    import ctypes as C
    d = lib_mod.ConvDesc()
    up = 2 if upsample else 1
    d.N, d.D, d.H, d.W = N, D, H, W
    d.C1, d.C2 = (cin + 31) // 32 * 32, 0
    d.Cout, d.Cout_pad = cout, (cout + 31) // 32 * 32
    d.kd, d.kh, d.kw = k
    d.stride, d.pad, d.upsample = stride, pad, 1 if upsample else 0
    ext = lambda n, kk: (n * up if kk == 3 or upsample else n) if stride == 1 else (n + 2 * pad - 3) // 2 + 1
    d.Do, d.Ho, d.Wo = (D * up if (k[0] == 3 and upsample) else D), ext(H, k[1]), ext(W, k[2])
    d.out_dtype = 1 if out_f32 else 0
    d.prologue_act = act
    return d, C.byref(d)


def test_dispatch_predicates_are_host_logic_and_follow_the_documented_rules():
    """gg_conv_runs_halo_tile / gg_conv_fuses_prologue / gg_conv_fuses_posterior read no pointers and launch nothing: they are the
    host-side dispatch rules (gg_conv_halo.hip) and can be pinned without a GPU."""
    import __graft_entry__ as ge
    from jointimagegeneration_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    lib = _lib.load()
    GG_F32 = 1
    assert _lib.ConvDesc().out_dtype == 0                       # GG_BF16 == 0 (guidegen_hip.h)
    # CCDM 128^3: 64 -> 64 3x3x3 runs on the halo-tile kernel and keeps its GroupNorm*SiLU fused (one cout group)
    d, ref = _desc(_lib, 1, 128, 128, 128, 64, 64, (3, 3, 3))
    assert lib.gg_conv_runs_halo_tile(ref) == 1 and lib.gg_conv_fuses_prologue(ref) == 1 and lib.gg_conv_fuses_posterior(ref) == 0
    # ... its head conv (K = 14 classes, fp32 logits) can take the reverse step as its epilogue; at 32^3 (other kernels) it cannot
    d, ref = _desc(_lib, 1, 128, 128, 128, 64, 14, (3, 3, 3), out_f32=True)
    assert d.out_dtype == GG_F32 and lib.gg_conv_fuses_posterior(ref) == 1
    d, ref = _desc(_lib, 1, 32, 32, 32, 64, 14, (3, 3, 3), out_f32=True)
    assert lib.gg_conv_fuses_posterior(ref) == 0
    d, ref = _desc(_lib, 1, 128, 128, 128, 64, 20, (3, 3, 3), out_f32=True)          # more classes than one 16-cout tile
    assert lib.gg_conv_fuses_posterior(ref) == 0
    # autoencoder: 128 -> 128 @512^2 (one cout group of the 128-cout tile) fused; 512 -> 512 @128^2 (four groups re-stage a box) separate
    d, ref = _desc(_lib, 1, 1, 512, 512, 128, 128, (1, 3, 3))
    assert lib.gg_conv_runs_halo_tile(ref) == 1 and lib.gg_conv_fuses_prologue(ref) == 1
    d, ref = _desc(_lib, 1, 1, 128, 128, 512, 512, (1, 3, 3))
    assert lib.gg_conv_runs_halo_tile(ref) == 1 and lib.gg_conv_fuses_prologue(ref) == 0
    d.path_hint = 1                                                                  # tests: "can it" rather than "should it"
    assert lib.gg_conv_fuses_prologue(ref) == 1
    # a 1x1 conv and a stride-2 conv never run on the halo-tile kernel
    d, ref = _desc(_lib, 1, 128, 128, 128, 128, 64, (1, 1, 1), pad=0)
    assert lib.gg_conv_runs_halo_tile(ref) == 0
    d, ref = _desc(_lib, 1, 128, 128, 128, 64, 64, (3, 3, 3), stride=2)
    assert lib.gg_conv_runs_halo_tile(ref) == 0


def test_attention_plan_is_host_logic_and_pins_the_production_shapes():
    """gg_attention_plan reads no pointers and launches nothing; gg_attention_forward takes its decisions from the same function.
    plan = {key tile, key ranges over workgroups given a workspace, in-workgroup key split, LDS-DMA staging}."""
    import ctypes as C
    import __graft_entry__ as ge
    from jointimagegeneration_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    lib = _lib.load()

    def plan(N, heads, D, Tq, Tkv):
        d = _lib.AttentionDesc()
        d.N, d.heads, d.head_dim, d.Tq, d.Tkv = N, heads, D, Tq, Tkv
        out = (C.c_int32 * 4)()
        rc = lib.gg_attention_plan(C.byref(d), out)
        ws = lib.gg_attention_workspace_bytes(C.byref(d))
        if rc == 0:                                      # the workspace query is the same decision
            assert ws == (N * heads * out[1] * Tq * (D + 2) * 4 if out[1] > 1 else 0)
        return rc, tuple(out)

    # latent UNet, 32x32 level at batch 1 (10 heads of 32 channels, T = 1024): 160 workgroups -> the in-workgroup key split
    assert plan(1, 10, 32, 1024, 1024) == (0, (256, 1, 1, 0))
    assert plan(8, 10, 32, 1024, 1024) == (0, (256, 1, 0, 0))           # batch 8 fills the chip: plain kernel
    assert plan(1, 20, 32, 256, 256) == (0, (256, 1, 0, 0))             # 16x16 level: one key tile
    # autoencoder mid-block attention: one head of 512 channels over 64x64 tokens: LDS-DMA, keys split four ways
    assert plan(1, 1, 512, 4096, 4096) == (0, (32, 4, 0, 1))
    assert plan(4, 1, 512, 4096, 4096) == (0, (32, 1, 0, 1))            # 256 workgroups: no split
    assert plan(1, 1, 384, 1030, 1030) == (0, (32, 8, 0, 1))
    assert plan(1, 1, 512, 255, 255) == (0, (32, 1, 0, 1))              # fewer than 8 key tiles: never split
    # cross attention (SpatialTransformer): Tq != Tkv, a short context
    assert plan(1, 5, 64, 1024, 77) == (0, (64, 1, 0, 0))
    assert plan(1, 5, 64, 1024, 256) == (0, (64, 1, 1, 0))
    assert plan(1, 2, 128, 130, 130) == (0, (64, 1, 0, 0))
    assert plan(1, 1, 48, 64, 64)[0] < 0 and plan(1, 1, 64, 0, 64)[0] < 0          # unsupported head dim, empty extent
