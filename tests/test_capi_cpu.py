"""CPU suite: the one check of the C-ABI boundary.  include/guidegen_hip.h is the only statement of it; jointimagegeneration_amd/_lib.py
derives the ctypes binding from its text.  Here the derived binding is compared with a second, separate reading of every declaration
(the small rule below, not the product parser), with signatures written out by hand, with the layouts the C compiler gives the
descriptor structs, and with the pins the feature suites used to hold one by one (argument counts, parameter names, build list).
No compute calls; the dispatch predicates and the attention plan are host logic and are pinned here too."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import pytest

from jointimagegeneration_amd import _lib
from util import load_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jointimagegeneration_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")


@functools.lru_cache(maxsize=None)
def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "guidegen_hip.h")).read(), flags=re.S)


def declared_symbols():
    return sorted(set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", header_text())))


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def test_library_exports_every_declared_symbol(lib):
    syms = declared_symbols()
    assert len(syms) >= 92 and syms == sorted(_lib.SIGNATURES)
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in guidegen_hip.h but not exported"
    assert lib.gg_version() >= 100


# ------------------------------------------------------------------------------------------------ every declaration
# The test's own rule: a parameter with '*' (or an array) is a pointer -- to a descriptor struct POINTER(its class), else c_void_p --
# and anything else maps by the first word after `const`.  Kept apart from _lib.parse_header so that each checks the other.
_CT = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
_RES = {"int": C.c_int, "int64_t": C.c_int64, "const char *": C.c_char_p}
_DESC = {"gg_conv_desc": _lib.ConvDesc, "gg_attention_desc": _lib.AttentionDesc}


def declaration(name):
    """(result text, [parameter text, ...]) of `name` as the header declares it."""
    m = re.search(r"(\bconst char \*|\b\w+)\s*\b" + name + r"\s*\(([^)]*)\)\s*;", header_text())
    assert m, f"{name} is not declared in guidegen_hip.h"
    return m.group(1), [] if m.group(2).strip() == "void" else [p.strip() for p in m.group(2).split(",")]


def expected_signature(name):
    res, params = declaration(name)
    want = []
    for p in params:
        toks = p.replace("const", "").split()
        want.append((C.POINTER(_DESC[toks[0]]) if toks[0] in _DESC else C.c_void_p) if "*" in p or "[" in p else _CT[toks[0]])
    return _RES[res], want


@pytest.mark.parametrize("name", declared_symbols())
def test_declaration_matches_the_binding(name, lib):
    res, args = expected_signature(name)
    assert _lib.SIGNATURES[name] == (res, args)
    fn = getattr(lib, name)
    assert fn.restype is res and list(fn.argtypes) == args


# ------------------------------------------------------------------------------------------------ the parser, pinned by hand
vp, i32, i64, u64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float
HAND = {
    "gg_last_error": (C.c_char_p, []),
    "gg_conv_packed_weight_bytes": (i64, [i32, i32, i32]),
    "gg_conv_forward": (C.c_int, [C.POINTER(_lib.ConvDesc), vp]),
    "gg_attention_plan": (C.c_int, [C.POINTER(_lib.AttentionDesc), vp]),
    "gg_mask_overlay": (C.c_int, [vp, i32, i32, i32, i32, C.c_double, vp, vp, vp]),
    "gg_ccdm_posterior_sample": (C.c_int, [vp, i32, i32, vp, vp, u64, vp, i32, vp, i32, i64, vp, vp, vp, i32, vp]),
    "gg_lincomb4": (C.c_int, [vp, vp, vp, vp, f32, f32, f32, f32, f32, i64, vp, vp]),
    "gg_ubench_mfma_bf16": (C.c_int, [i32, i32, i32, vp, vp, vp]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_signature_equals_the_hand_written_one(name):
    assert _lib.SIGNATURES[name] == HAND[name]


def test_hand_written_signatures_cover_every_mapped_type():
    used = {t for res, args in HAND.values() for t in [res] + args}
    assert used == set(_lib._SCALARS.values()) | {C.c_char_p, vp, C.POINTER(_lib.ConvDesc), C.POINTER(_lib.AttentionDesc)}


# ------------------------------------------------------------------------------------------------ pins of the feature suites
# entry -> (result, argument count, parameter names, unit in build.sh's list, source file that defines it); None: not pinned
PINS = {
    "gg_unfold_cl": ("int", None, None, None, None),
    "gg_fold_weighted_cl": ("int", None, None, None, None),
    "gg_volume_views_cl": ("int", 13, None, "gg_lpips", None),
    "gg_relu_cl": ("int", 4, None, "gg_lpips", None),
    "gg_lpips_tap": ("int", 16, None, "gg_lpips", None),
    "gg_lpips_tap_workspace_bytes": ("int64_t", 5, None, "gg_lpips", None),
    "gg_ddpm_step_x0": ("int", None, ["x", "out", "out_stride", "noise", "scalars_dev", "flags", "M", "C", "pred_x0_out", "unet_in",
                                      "unet_in_stride", "stream"], None, None),
    "gg_log_rows": ("int", None, ["state", "N", "C", "S", "slot", "stream"], None, None),
    "gg_mask_overlay": ("int", 9, None, "gg_render", None),
    "gg_make_grid_u8": ("int", 10, None, "gg_render", None),
    "gg_vq_nearest": ("int", None, None, None, None),
    "gg_ddim_step_vq": ("int", None, None, None, None),
    "gg_label_confusion": ("int", 9, None, "gg_metrics", None),
    "gg_q_sample_rows": ("int", None, None, "gg_loss", "gg_loss.hip"),
    "gg_loss_rows": ("int", None, None, "gg_loss", "gg_loss.hip"),
    "gg_ccdm_q_sample": ("int", None, None, "gg_loss", "gg_loss.hip"),
    "gg_ccdm_step_loss": ("int", None, None, "gg_loss", "gg_loss.hip"),
    "gg_loss_workspace_bytes": ("int64_t", None, None, "gg_loss", "gg_loss.hip"),
    "gg_inpaint_blend": ("int", None, ["x", "x0", "mask", "mask_C", "noise", "scalars_dev", "M", "C", "unet_in", "unet_in_stride", "stream"],
                         None, None),
    "gg_patch_conv_forward": ("int", None, None, "gg_patchgan", None),
    "gg_patch_conv_forward_f32": ("int", None, None, "gg_patchgan", None),
    "gg_gauss_kl_rows": ("int", None, None, "gg_patchgan", None),
    "gg_gauss_sample_rows": ("int", None, None, "gg_patchgan", None),
    "gg_logit_stats": ("int", None, None, "gg_patchgan", None),
    "gg_embed_rows": ("int", None, None, None, None),
    "gg_gelu": ("int", None, None, None, None),
    "gg_layernorm_rows": ("int", None, None, None, None),
    "gg_interpolate2d_f32": ("int", None, None, None, None),
}
# source file -> words it must not hold outside // comments (its reductions are two-stage sums; the library never allocates or copies)
SOURCE_BANS = {"gg_loss.hip": ("atomic",), "gg_patchgan.hip": ("atomic", "hipMalloc", "hipMemcpy")}
CONSTANTS = dict(GG_OK=0, GG_ERR_BAD_SHAPE=-1, GG_ERR_BAD_DTYPE=-2, GG_ERR_UNSUPPORTED=-3, GG_ERR_WORKSPACE_TOO_SMALL=-4, GG_ERR_HIP=-5,
                 GG_BF16=0, GG_F32=1, GG_LOSS_L2=0, GG_LOSS_L1=1, GG_LOSS_PRIOR_KL=2, GG_DDPM_PREDICTS_X0=1, GG_DDPM_CLIP=2)


@pytest.mark.parametrize("name", sorted(PINS))
def test_pinned_entry(name, lib):
    res, nargs, names, unit, defined_in = PINS[name]
    got_res, params = declaration(name)
    assert got_res == res and _lib.SIGNATURES[name][0] is _RES[res] and hasattr(lib, name)
    assert len(_lib.SIGNATURES[name][1]) == len(params)
    if nargs is not None:
        assert len(params) == nargs
    if names is not None:
        assert [re.findall(r"\w+", p)[-1] for p in params] == names
    if unit is not None:
        assert re.search(r"for f in [^;]*\b%s\b" % unit, open(os.path.join(CSRC, "build.sh")).read())
    if defined_in is not None:
        assert re.search(r'extern "C" %s %s\(' % (res, name), open(os.path.join(CSRC, defined_in)).read()), f"{name} is not defined in {defined_in}"


@pytest.mark.parametrize("unit", sorted(SOURCE_BANS))
def test_pinned_source_holds_no_banned_call(unit):
    src = open(os.path.join(CSRC, unit)).read()
    assert "atomicAdd" not in src
    for word in SOURCE_BANS[unit]:
        assert word not in re.sub(r"//.*", "", src), word


def test_constants_are_the_header_ones():
    from jointimagegeneration_amd import ops
    for name, value in CONSTANTS.items():
        assert getattr(_lib, name) == value, name
    assert set(_lib.CONSTANTS) == set(CONSTANTS)
    assert ops.LOSS_MODES == {"l2": 0, "l1": 1, "prior_kl": 2} and (ops.DDPM_PREDICTS_X0, ops.DDPM_CLIP) == (1, 2)
    assert _lib.ConvDesc().out_dtype == _lib.GG_BF16


# ------------------------------------------------------------------------------------------------ struct layouts against the compiler
def test_descriptor_anchors():
    assert len(_lib.ConvDesc._fields_) == 63 and C.sizeof(_lib.ConvDesc) == 392
    assert len(_lib.AttentionDesc._fields_) == 21 and C.sizeof(_lib.AttentionDesc) == 144
    assert _lib.ConvDesc.src1.offset == 80 and _lib.ConvDesc.post_rows_per_sample.offset == 384
    assert sorted(_lib.STRUCTS) == ["gg_attention_desc", "gg_conv_desc"]


@pytest.mark.parametrize("cname", sorted(_lib.STRUCTS))
def test_struct_layout_equals_the_compilers(cname, tmp_path):
    """A host C program that includes the header prints sizeof the struct, then offsetof and the size of every field."""
    cls = _lib.STRUCTS[cname]
    fields = [f for f, _ in cls._fields_]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "guidegen_hip.h"', 'int main(void) {',
             '    printf("%%zu\\n", sizeof(%s));' % cname]
    lines += ['    printf("%%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (cname, f, cname, f) for f in fields]
    lines += ['    return 0;', '}', '']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    cc = [shutil.which("cc")] if shutil.which("cc") else [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c"]   # build.sh's compiler
    subprocess.check_call(cc + ["-I", INCLUDE, "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")])
    out = subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")
    assert int(out[0]) == C.sizeof(cls)
    got = [tuple(int(v) for v in ln.split()) for ln in out[1:] if ln]
    assert got == [(getattr(cls, f).offset, getattr(cls, f).size) for f in fields]


# ------------------------------------------------------------------------------------------------ refusals
def test_parser_refuses_a_type_outside_its_map():
    ok = "typedef struct { int32_t n; const float *w; } gg_desc;\nint gg_run(const gg_desc *d, void *stream);\n"
    consts, structs, sigs = _lib.parse_header("typedef enum { GG_A = 3, GG_B } gg_e;\n#define GG_C 0x10\n" + ok)
    assert consts == dict(GG_A=3, GG_B=4, GG_C=16) and structs["gg_desc"]._fields_ == [("n", i32), ("w", vp)]
    assert sigs == {"gg_run": (C.c_int, [C.POINTER(structs["gg_desc"]), vp])}
    with pytest.raises(ValueError, match=r"gg_bad\(uint16_t x\).*'uint16_t'"):
        _lib.parse_header(ok + "int gg_bad(uint16_t x);\n")
    with pytest.raises(ValueError, match=r"gg_desc\.bytes.*'size_t'"):
        _lib.parse_header("typedef struct { int32_t n; size_t bytes; } gg_desc;\nint gg_run(const gg_desc *d, void *stream);\n")
    with pytest.raises(ValueError, match=r"gg_bad.*'long'"):
        _lib.parse_header(ok + "long gg_bad(void);\n")
    with pytest.raises(ValueError, match="cannot read"):
        _lib.parse_header(ok + "int gg_bad(unsigned int x);\n")


def test_a_missing_header_is_refused_by_path(tmp_path):
    with pytest.raises(RuntimeError, match=r"no_such\.h not found"):
        _lib._header_text(str(tmp_path / "no_such.h"))
    assert os.path.samefile(_lib.HEADER_PATH, os.path.join(INCLUDE, "guidegen_hip.h"))


# ------------------------------------------------------------------------------------------------ the product
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


def test_dispatch_predicates_are_host_logic_and_follow_the_documented_rules(lib):
    """gg_conv_runs_halo_tile / gg_conv_fuses_prologue / gg_conv_fuses_posterior read no pointers and launch nothing: they are the
    host-side dispatch rules (gg_conv_halo.hip) and can be pinned without a GPU."""
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


def test_attention_plan_is_host_logic_and_pins_the_production_shapes(lib):
    """gg_attention_plan reads no pointers and launches nothing; gg_attention_forward takes its decisions from the same function.
    plan = {key tile, key ranges over workgroups given a workspace, in-workgroup key split, LDS-DMA staging}."""
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
