"""Inventory of the capped grid-stride launches of csrc/*.hip, the shapes that take each of them past its cap, and the helpers the
tests around it share (tests/test_grid_caps_cpu.py keeps the table honest without a GPU, tests/test_grid_caps_gpu.py runs the shapes).

A grid-stride kernel launched with at most `cap` blocks of 256 threads runs its loop body once per thread while the work is at most
cap * 256 units.  Only above that do some threads take a second trip, and only then can a wrong stride, a per-trip value that is not
reset, a flat-index decode that is wrong after the first trip, or a partial sum that loses its second trip show.  Every row below names
the kernel, its C entry point, the unit one thread handles per trip, the cap in blocks, whether the grid is per sample (grid.y = n), and
either the gpu test that runs it past the cap (with the work per grid of that test's shapes, from which the cpu test re-derives "past
the cap, ragged end" by plain arithmetic) or the reason it needs none.

Shape rules (the smallest shapes at which the later trips differ from the first):
  past_cap(cap)      cap * 256 + 259 units: every thread takes one trip, one whole block plus three threads a second one, and the end
                     falls inside a wave.
  sample_units(cap)  cap * 128 + 129 units per sample at N = 3: the border between samples 1 and 2 lies at unit cap * 256 + 258, which
                     only a second trip reads, so an `n = i / S` decode that is wrong after the first trip shows.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

THREADS = 256
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jointimagegeneration_amd", "csrc")
GPU_TESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_grid_caps_gpu.py")


def past_cap(cap: int, unit: int = 1) -> int:
    """Elements of the smallest work size that takes a grid of `cap` blocks into a second trip with a ragged end: cap * 256 + 259 units
    of `unit` elements each."""
    return (cap * THREADS + THREADS + 3) * unit


def sample_units(cap: int) -> int:
    """Units per sample, at N = 3, for which the border between samples 1 and 2 lies in the second trip of a grid of `cap` blocks."""
    return cap * (THREADS // 2) + THREADS // 2 + 1


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the shapes of the gpu tests
LS_CAP, LP_CAP = 1024, 128                       # LS_MAX_BLOCKS (gg_reduce.h), LP_MAX_BLOCKS (gg_lpips.hip): pinned by the cpu test
S_RED = past_cap(LS_CAP)                         # 262 403 rows per sample for every per-sample reduction
N_RED = 2
S3_4096, S3_8192, S3_16384 = sample_units(4096), sample_units(8192), sample_units(16384)      # 524 417, 1 048 705, 2 097 281
MM_N = 3
MM_CAP = 2048 // MM_N                            # 682 blocks per sample in the min-max scatter kernels

STEP_C4_M = past_cap(4096)                       # row-per-lane kernels at C = 4: unit = row
STEP_C3_M = ceil_div(past_cap(4096), 3)          # per-element kernels at C = 3: 349 613 rows, 1 048 839 elements
STEP_E4_M = ceil_div(past_cap(4096), 4)          # per-element kernels at C = 4: 262 209 rows, 1 048 836 elements
GLUE_HW = 725                                    # 3 x 725^2 pixels: the border of samples 1 and 2 at pixel 1 051 250
CT_HW = ((728, 91, 1), (725, 29, 0))             # (H = W, latent extent, margin): f = 8 reads keep as words, f = 25 as bytes
KEEP_VEC = (8, 2, 530)                           # label_keep_volume (D, N, H = W): HW % 4 == 0, one word of 4 pixels per thread
KEEP_SCALAR = (8, 2, 363)                        # HW odd: one pixel per thread
ROWS_C2 = (3, 2, S3_4096)                        # (N, C, S) of gg_q_sample_rows and gg_gauss_sample_rows
CC_M = past_cap(4096)                            # voxels of the one volume whose size words cc_zero_kernel clears

GN_APPLY = (3, 262178, 32)                       # (N, S, C): 4 pieces per row; the border of samples 1 and 2 at piece 2 097 424
GEGLU = (524353, 32)                             # (rows, inner): 4 pieces per row
ADD_N = past_cap(8192, 8)
ONEHOT = (1048706, 14, 16)                       # (M, K, stride): 2 pieces per row
TO_CL = (2, 9, 524353, 16)                       # (N, C, S, C_pad): 2 pieces per row, the second one read in the second trip only
FROM_CL = (2, 3, 349569, 8)                      # (N, C, S, C_pad)
EMBED_BF16 = (2521, 13, 48, 64)                  # (B, T, D, stride)
EMBED_F32 = (1181, 37, 48, 48)
GELU_N = past_cap(8192, 8) - 3                   # the last group of 8 is a 5-element scalar tail, in the second trip

RES_UP2D = (3, 1, 363, 363, False)               # (N, D, H, W, resample_d) of the INPUT; 32 channels = 4 pieces per position
RES_UP3D = (3, 1, 257, 257, True)
RES_POOL2D = (3, 1, 1450, 1450, False)
RES_POOL3D = (3, 2, 1450, 1450, True)
GN_F32 = (3, 65542, 32)                          # (N, S, C): unit = element
INTERP = (3, 1, 725, 725)                        # NCHW input of the x2 cases; the x0.5 case reads (3, 1, 2900, 2900)

MINMAX_N = past_cap(2048)
MM_SCALAR = past_cap(MM_CAP)                     # odd: the scalar composite, one element per thread
MM_VEC = past_cap(MM_CAP, 4)                     # n_per % 4 == 0: the vec4 composite, 4 elements per thread

SPLITK = (3, 512, 320, 59, 61)                   # (N, Cin, Cout, H, W) of a 1x1 conv: plan_gather goes NT 5 -> 2 on 85 * 5 = 425 blocks and splits K in
                                                 # two; the reduce has 10 797 * 80 = 863 760 units, the border of samples 1 and 2 at unit 575 840
ACC_GENERAL = (2, 524353, 32)                    # (N, S, C): 2 097 412 pieces per sample, past the two prefetched trips of gn_apply_acc

LPIPS_SHAPES = ((512, 46, 46), (64, 182, 182))   # (C, h, w)


def lpips_lanes(C: int, vec: int) -> int:
    """tap_plan's rule (gg_lpips.hip): lanes per quad, the largest power of two L <= 64 with L * vec <= C."""
    L = 1
    while L * 2 <= 64 and L * 2 * vec <= C:
        L *= 2
    return L


def _res_units(shape, up: bool) -> int:
    """output (position, 8-channel piece) units per sample of a resample2x case with 32 channels"""
    _, D, H, W, rd = shape
    pos = (D * (2 if rd else 1)) * 2 * H * 2 * W if up else (D // (2 if rd else 1)) * (H // 2) * (W // 2)
    return pos * 4


# ------------------------------------------------------------------------------------------------ the table
@dataclass(frozen=True)
class Row:
    kernel: str                    # __global__ function
    file: str                      # csrc file
    entry: str                     # C entry point(s) that launch it
    unit: str                      # what one thread handles per trip
    cap: object                    # blocks: an int, "2048/N", "cus*per_cu", or None where the launch has no cap
    per_sample: bool               # grid.y = sample: the cap and the work are per sample
    test: Optional[str] = None     # function of tests/test_grid_caps_gpu.py that takes it past the cap
    work: Tuple = ()               # units per grid (per sample where per_sample) of that test's shapes; an entry is a number of units
                                   # against the row's cap and 256 units per block and trip, or (units, units per block and trip, cap)
    exempt: Optional[str] = None   # or: why no case is needed


def _r(kernel, file, entry, unit, cap, per_sample, test, *work):
    return Row(kernel, file, entry, unit, cap, per_sample, test, tuple(work))


def _x(kernel, file, entry, unit, cap, per_sample, why):
    return Row(kernel, file, entry, unit, cap, per_sample, exempt=why)


def lpips_quads(h: int, w: int) -> int:
    return ceil_div(h, 2) * ceil_div(w, 2)


# (quads, quads per workgroup and trip = 256 / L, cap): bf16 at both shapes, fp32 at the first
_LP = [(lpips_quads(h, w), THREADS // lpips_lanes(C, 8), LP_CAP) for C, h, w in LPIPS_SHAPES] + \
      [(lpips_quads(*LPIPS_SHAPES[0][1:]), THREADS // lpips_lanes(LPIPS_SHAPES[0][0], 4), LP_CAP)]

ROWS: List[Row] = [
    # ---- cap 4096
    _r("step_kernel", "gg_sampler.hip", "gg_ddim_step gg_ddpm_step gg_ddpm_step_x0", "element", 4096, False, "test_ldm_steps",
       STEP_E4_M * 4, STEP_C3_M * 3),
    _r("ddpm_step_c4_kernel", "gg_sampler.hip", "gg_ddpm_step_x0", "row", 4096, False, "test_ldm_steps", STEP_C4_M),
    _r("inpaint_blend_c4_kernel", "gg_sampler.hip", "gg_inpaint_blend", "row", 4096, False, "test_inpaint_blend", STEP_C4_M),
    _r("inpaint_blend_kernel", "gg_sampler.hip", "gg_inpaint_blend", "element", 4096, False, "test_inpaint_blend", STEP_C3_M * 3),
    _r("lincomb4_kernel", "gg_sampler.hip", "gg_lincomb4", "element", 4096, False, "test_lincomb4", past_cap(4096)),
    _r("mask_to_cond_slice_kernel", "gg_sampler.hip", "gg_mask_to_cond_slice", "row", 4096, False, "test_mask_to_cond", 3 * GLUE_HW ** 2),
    _r("mask_to_cond_slices_kernel", "gg_sampler.hip", "gg_mask_to_cond_slices", "row", 4096, False, "test_mask_to_cond", 3 * GLUE_HW ** 2),
    _r("ct_edit_glue_kernel", "gg_sampler.hip", "gg_ct_edit_glue", "row", 4096, False, "test_ct_edit_glue",
       *(3 * hw * hw for hw, _, _ in CT_HW)),
    _r("label_keep_volume_kernel", "gg_sampler.hip", "gg_label_keep_volume", "quad", 4096, False, "test_label_keep_volume",
       KEEP_VEC[0] * KEEP_VEC[1] * KEEP_VEC[2] ** 2 // 4, KEEP_SCALAR[0] * KEEP_SCALAR[1] * KEEP_SCALAR[2] ** 2),
    _r("gauss_sample_rows_kernel", "gg_patchgan.hip", "gg_gauss_sample_rows", "row", 4096, False, "test_gauss_sample_rows",
       ROWS_C2[0] * ROWS_C2[2]),
    _r("q_sample_rows_kernel", "gg_loss.hip", "gg_q_sample_rows", "row", 4096, False, "test_q_sample_rows", ROWS_C2[0] * ROWS_C2[2]),
    _r("cc_zero_kernel", "gg_components.hip", "gg_component_stats gg_label_vote", "element", 4096, False, "test_component_stats_zeroing", CC_M),
    _r("gn_apply_acc_kernel", "gg_norm.hip", "gg_groupnorm_apply_acc", "8-channel piece", 4096, True, "test_groupnorm_apply_acc_general",
       ACC_GENERAL[1] * ACC_GENERAL[2] // 8),
    # ---- cap 8192
    _r("gn_apply_kernel", "gg_norm.hip", "gg_groupnorm_apply", "8-channel piece", 8192, False, "test_groupnorm_apply",
       GN_APPLY[0] * GN_APPLY[1] * GN_APPLY[2] // 8),
    _r("geglu_kernel", "gg_norm.hip", "gg_geglu", "8-channel piece", 8192, False, "test_geglu", GEGLU[0] * GEGLU[1] // 8),
    _r("add_kernel", "gg_norm.hip", "gg_add", "8-channel piece", 8192, False, "test_add", ADD_N // 8),
    _r("labels_to_onehot_kernel", "gg_sampler.hip", "gg_labels_to_onehot", "8-channel piece", 8192, False, "test_labels_to_onehot",
       ONEHOT[0] * ONEHOT[2] // 8),
    _r("nchw_to_cl_kernel", "gg_sampler.hip", "gg_nchw_f32_to_cl_bf16", "8-channel piece", 8192, False, "test_layout_movers",
       TO_CL[0] * TO_CL[2] * TO_CL[3] // 8),
    _r("cl_to_nchw_kernel", "gg_sampler.hip", "gg_cl_to_nchw_f32 gg_log_rows", "element", 8192, False, "test_layout_movers",
       FROM_CL[0] * FROM_CL[1] * FROM_CL[2]),
    _r("embed_rows_kernel", "gg_cond.hip", "gg_embed_rows", "element", 8192, False, "test_embed_rows",
       EMBED_BF16[0] * EMBED_BF16[1] * EMBED_BF16[3], EMBED_F32[0] * EMBED_F32[1] * EMBED_F32[3]),
    _r("gelu_kernel", "gg_cond.hip", "gg_gelu", "8-channel piece", 8192, False, "test_gelu", ceil_div(GELU_N, 8)),
    # ---- cap 16384
    _r("resample2x_kernel", "gg_resample.hip", "gg_resample2x", "8-channel piece", 16384, False, "test_resample2x",
       3 * _res_units(RES_UP2D, True), 3 * _res_units(RES_UP3D, True), 3 * _res_units(RES_POOL2D, False), 3 * _res_units(RES_POOL3D, False)),
    _r("gn_f32_apply_kernel", "gg_f32.hip", "gg_groupnorm_f32", "element", 16384, False, "test_groupnorm_f32",
       GN_F32[0] * GN_F32[1] * GN_F32[2]),
    _r("gn_f32_apply_film_kernel", "gg_f32.hip", "gg_groupnorm_f32_film", "element", 16384, False, "test_groupnorm_f32",
       GN_F32[0] * GN_F32[1] * GN_F32[2]),
    _r("interpolate2d_kernel", "gg_cond.hip", "gg_interpolate2d_f32", "element", 16384, False, "test_interpolate2d",
       INTERP[0] * INTERP[1] * (2 * INTERP[2]) * (2 * INTERP[3])),
    # ---- cap 2048 and 2048 / N
    _r("minmax_apply_kernel", "gg_sampler.hip", "gg_minmax_normalise", "element", 2048, False, "test_minmax_normalise", MINMAX_N),
    _r("minmax_seg_reduce_kernel", "gg_sampler.hip", "gg_minmax_normalise gg_minmax_normalise_scatter gg_minmax_normalise_keep_scatter",
       "element", (2048, "2048/N"), True, "test_minmax_normalise test_minmax_scatter", (MINMAX_N, THREADS, 2048), MM_SCALAR, MM_VEC),
    _r("minmax_seg_scatter_kernel", "gg_sampler.hip", "gg_minmax_normalise_scatter", "element", "2048/N", True, "test_minmax_scatter",
       MM_SCALAR, MM_VEC),
    _r("minmax_seg_keep_scatter_kernel", "gg_sampler.hip", "gg_minmax_normalise_keep_scatter", "element or quad", "2048/N", True,
       "test_minmax_scatter", MM_SCALAR, MM_VEC // 4),
    _r("conv_splitk_reduce_kernel", "gg_conv.hip", "gg_conv_forward", "4 couts", 2048, False, "test_splitk_reduce",
       SPLITK[0] * SPLITK[3] * SPLITK[4] * ((SPLITK[2] + 31) // 32 * 32) // 4),
    # ---- reductions: LS_MAX_BLOCKS workgroups per sample, LP_MAX_BLOCKS per image
    _r("loss_rows_kernel", "gg_loss.hip", "gg_loss_rows", "row", LS_CAP, True, "test_loss_rows_exact_integers test_loss_rows_prior_kl", S_RED),
    _r("ccdm_step_loss_kernel", "gg_loss.hip", "gg_ccdm_step_loss", "voxel", LS_CAP, True, "test_ccdm_step_loss", S_RED),
    _r("gauss_kl_rows_kernel", "gg_patchgan.hip", "gg_gauss_kl_rows", "row", LS_CAP, True, "test_gauss_kl_rows", S_RED),
    _r("logit_stats_kernel", "gg_patchgan.hip", "gg_logit_stats", "row", LS_CAP, False, "test_logit_stats", S_RED),
    _r("lpips_tap_kernel", "gg_lpips.hip", "gg_lpips_tap", "quad", LP_CAP, True, "test_lpips_tap", *_LP),
    # ---- no case needed
    _x("gn_partial_kernel", "gg_norm.hip", "gg_groupnorm_stats", "row block", None, True,
       "no grid-stride loop: every workgroup walks its own rows_per_block rows and gridDim only addresses its partial; the capped grid of "
       "1024 workgroups runs in tests/test_norm_exact_gpu.py::test_groupnorm_bit_exact[partial_c64_362x363-n1] (131 406 rows)"),
    _x("gn_apply_acc_lean_kernel", "gg_norm.hip", "gg_groupnorm_apply_acc", "8-channel piece", 4096, True,
       "one piece per thread by the host gate blocks * 256 >= pieces; gridDim only feeds the XCD block swizzle, which "
       "tests/test_norm_exact_gpu.py runs swizzled and unswizzled (lean1..lean8 cases)"),
    _x("conv_pack_weight_kernel", "gg_conv.hip", "gg_conv_pack_weight", "element", 4096, False,
       "already several trips, bit for bit against fp64, in tests/test_conv_exact_gpu.py::test_box_kernel_generic[box_w8-*]: 640 x 640 x 9 "
       "= 3 686 400 elements against 4096 * 256 = 1 048 576 (a wrong packed weight is a wrong conv output)"),
    _x("conv_tile1x1_kernel", "gg_conv_tile.hip", "gg_conv_forward", "32-row tile per wave", "cus*per_cu", False,
       "already several trips in tests/test_conv_tile_gpu.py::test_tile_equals_gather[n1_64to128_whole_tiles]: 8192 tiles over at most "
       "2048 resident waves, every stored word compared"),
    _x("conv_halo_kernel", "gg_conv_halo.hip", "gg_conv_forward", "tile", None, False,
       "one tile per workgroup, no cap; gridDim only feeds the XCD block remap, run by the HALO cases of tests/test_conv_exact_gpu.py"),
    _x("conv_halo3_team_kernel", "gg_conv_halo3.hip", "gg_conv_forward", "item", None, False,
       "persistent workgroups over an item list (grid = min(items, CUs), no literal cap): several items per workgroup in "
       "tests/test_conv_exact_gpu.py::test_team_kernel[team_ragged_persistent-*] (32 x 64 x 64 positions)"),
    _x("ubench_copy_kernel", "gg_ubench.hip", "gg_ubench_copy", "16 bytes", None, False, "micro-benchmark, not product"),
]
BY_KERNEL: Dict[str, Row] = {r.kernel: r for r in ROWS}
assert len(BY_KERNEL) == len(ROWS)


def cap_blocks(row: Row) -> Optional[int]:
    """the cap as a number of blocks for the arithmetic of the cpu test (of a kernel with two launch sites: the per-sample one)"""
    caps = row.cap if isinstance(row.cap, tuple) else (row.cap,)
    if "2048/N" in caps:
        return MM_CAP
    return caps[0] if isinstance(caps[0], int) else None


# ------------------------------------------------------------------------------------------------ reading the sources (cpu test)
_GLOBAL = re.compile(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(")
_LAUNCH = re.compile(r"hipLaunchKernelGGL\(\s*\(?\s*(\w+)\b")
_CLAMP = re.compile(r"\b(\w+) > (\d+)\) \1 = \2;")


def _match(text: str, i: int, open_: str, close: str) -> int:
    """index just past the bracket that closes text[i] == open_"""
    depth = 0
    for j in range(i, len(text)):
        if text[j] == open_:
            depth += 1
        elif text[j] == close:
            depth -= 1
            if depth == 0:
                return j + 1
    raise ValueError("unbalanced " + open_)


def _strip_comments(text: str) -> str:
    text = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group()), text, flags=re.S)
    return re.sub(r"//[^\n]*", lambda m: " " * len(m.group()), text)


def grid_stride_kernels(csrc: str = CSRC) -> Dict[str, str]:
    """kernel name -> file, for every __global__ function of csrc/*.hip whose body mentions gridDim"""
    out = {}
    for name in sorted(os.listdir(csrc)):
        if not name.endswith(".hip"):
            continue
        text = _strip_comments(open(os.path.join(csrc, name)).read())
        for m in _GLOBAL.finditer(text):
            sig_end = _match(text, m.end() - 1, "(", ")")
            brace = text.index("{", sig_end)
            body = text[brace:_match(text, brace, "{", "}")]
            if "gridDim" in body:
                out[m.group(1)] = name
    return out


def _constant(csrc: str, file: str, name: str) -> int:
    m = re.search(r"constexpr int " + name + r" = (\d+);", open(os.path.join(csrc, file)).read())
    assert m, f"{file}: constexpr int {name} not found"
    return int(m.group(1))


def launch_caps(csrc: str, row: Row) -> set:
    """The caps written at the launch sites of row.kernel: for every hipLaunchKernelGGL of the kernel, every cap expression of the host
    function around it (from the end of the previous top-level block to the launch): the literal of gg_blocks256(work, cap), ls_blocks()
    (LS_MAX_BLOCKS), a TapPlan (LP_MAX_BLOCKS), `x > N) x = N;`."""
    text = _strip_comments(open(os.path.join(csrc, row.file)).read())
    caps = set()
    for m in _LAUNCH.finditer(text):
        if m.group(1) != row.kernel:
            continue
        end = _match(text, text.index("(", m.start()), "(", ")")
        window = text[text.rfind("\n}", 0, m.start()) + 1:end]
        for g in re.finditer(r"gg_blocks256\(", window):
            args = window[g.end():_match(window, g.end() - 1, "(", ")") - 1]
            depth, cut = 0, None
            for k, ch in enumerate(args):
                depth += ch == "("
                depth -= ch == ")"
                if ch == "," and depth == 0:
                    cut = k
            cap = " ".join(args[cut + 1:].split())
            caps.add(int(cap) if cap.isdigit() else "2048/N" if cap == "2048 / N > 1 ? 2048 / N : 1" else cap)
        if "ls_blocks(" in window:
            body = open(os.path.join(csrc, "gg_reduce.h")).read()
            assert "b > LS_MAX_BLOCKS ? LS_MAX_BLOCKS : b" in body, "gg_reduce.h: ls_blocks no longer clamps at LS_MAX_BLOCKS"
            caps.add(_constant(csrc, "gg_reduce.h", "LS_MAX_BLOCKS"))
        if "TapPlan" in window:
            assert "nb < LP_MAX_BLOCKS ? nb : LP_MAX_BLOCKS" in text, f"{row.file}: tap_plan no longer clamps at LP_MAX_BLOCKS"
            caps.add(_constant(csrc, row.file, "LP_MAX_BLOCKS"))
        for g in _CLAMP.finditer(window):
            caps.add(int(g.group(2)))
        if "blocks > (long long)cus * per_cu" in window:
            caps.add("cus*per_cu")
    return caps


def gpu_test_names(path: str = GPU_TESTS) -> set:
    import ast
    return {n.name for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}


def inventory_problems(csrc: str = CSRC, rows: Optional[List[Row]] = None) -> List[str]:
    """Every way the table disagrees with the sources, each message naming its kernel; [] when it is honest."""
    rows = ROWS if rows is None else rows
    by = {r.kernel: r for r in rows}
    found = grid_stride_kernels(csrc)
    msgs = [f"{k} ({f}): a __global__ function that reads gridDim has no row in tests/grid_caps.py" for k, f in found.items() if k not in by]
    msgs += [f"{r.kernel}: the table names {r.file}, where no __global__ function of that name reads gridDim" for r in rows
             if found.get(r.kernel) != r.file]
    tests = gpu_test_names()
    for r in rows:
        if found.get(r.kernel) != r.file:
            continue
        caps = launch_caps(csrc, r)
        want = set() if r.cap is None else set(r.cap) if isinstance(r.cap, tuple) else {r.cap}
        if r.exempt is None or r.cap is not None:
            if caps != want:
                msgs.append(f"{r.kernel}: the table says cap {r.cap}, the launch sites in {r.file} say {sorted(caps, key=str)}")
        if (r.exempt is None) == (r.test is None):
            msgs.append(f"{r.kernel}: a row names either a gpu test or an exemption")
        if r.exempt is None:
            missing = [t for t in r.test.split() if t not in tests]
            if missing:
                msgs.append(f"{r.kernel}: tests/test_grid_caps_gpu.py has no {missing}")
            cap = cap_blocks(r)
            if cap is None or not r.work:
                msgs.append(f"{r.kernel}: a covered row needs a numeric cap and the work of its shapes")
                continue
            for w in r.work:
                units, per_block, c = w if isinstance(w, tuple) else (w, THREADS, cap)
                if not (units > c * per_block and units % per_block):
                    msgs.append(f"{r.kernel}: {units} units do not pass {c} * {per_block} = {c * per_block} with a ragged end")
    return msgs


# ------------------------------------------------------------------------------------------------ helpers of the gpu tests
SLACK = 64
NAN16 = 0x7fc1                                    # a bf16 NaN pattern no kernel produces


def slack_buffer(shape, dtype, dev, fill=None):
    """(view of `shape`, slack of 64 elements behind it, check) inside one sentinel-filled allocation: floating types are filled with NaN
    (bf16: the pattern 0x7fc1), integers with `fill`; check() asserts that the slack still holds the fill."""
    import torch
    n = 1
    for v in shape:
        n *= int(v)
    flat = torch.empty(n + SLACK, dtype=dtype, device=dev)
    if dtype == torch.bfloat16:
        flat.view(torch.int16).fill_(NAN16)
    elif dtype.is_floating_point:
        flat.fill_(float("nan"))
    else:
        flat.fill_(-77 if fill is None else fill)
    tail = flat[n:].clone()
    bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[flat.element_size()]

    def check():
        assert torch.equal(flat[n:].view(bits), tail.view(bits)), "the 64 elements behind the output were written"
    return flat[:n].view(shape), check


def same_bits(got, want) -> bool:
    """every stored word equal (a NaN left from the fill is a difference; +0 and -0 differ)"""
    import torch
    bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(got.contiguous().view(bits), want.contiguous().view(bits))


def first_diff(got, want) -> str:
    import torch
    bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    bad = (got.contiguous().view(bits) != want.contiguous().view(bits)).reshape(-1).nonzero().reshape(-1)
    if not bad.numel():
        return ""
    i = int(bad[0])
    return (f"{bad.numel()} of {got.numel()} words differ; first at flat index {i} (trip {i // THREADS}): got "
            f"{float(got.reshape(-1)[i])!r} want {float(want.reshape(-1)[i])!r}; last at {int(bad[-1])}")


def ints(shape, lo, hi, seed, dev, dtype=None):
    """integer-valued tensor drawn on the device (10^7..10^8 values): exact in bf16 and fp32 for |v| <= 256"""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    small = -128 <= lo and hi <= 127                 # drawn as bytes where they fit: the temporary is a quarter of an fp32 tensor
    t = torch.randint(lo, hi + 1, tuple(shape), generator=g, device=dev, dtype=torch.int8 if small else torch.int32)
    return t.to(torch.float32 if dtype is None else dtype)


def planted_rows(S: int, sample: int) -> List[int]:
    """Rows of a per-sample reduction of S = past_cap(1024) rows that carry a large term: the first row, the last row of trip one, the
    first row of trip two (262 144), its workgroup's last row (+ 255), the first row of the ragged last workgroup and the last row.
    Sample 1 takes the neighbours of sample 0's rows, so that the two samples' partials differ in every planted position."""
    edge = LS_CAP * THREADS
    assert S == edge + THREADS + 3
    rows = [0, edge - 1, edge, edge + 255, edge + 256, S - 1]
    return rows if sample == 0 else [1, edge - 2, edge + 1, edge + 254, edge + 257, S - 2]


def single_deletions_move(full, deleted, tol: float, what: str) -> None:
    """The condition on the reference alone: `full` is the reference of the input, deleted[k] that of the input with planted row k put
    back to the background; each must lie more than 10 tol (relative) from `full`."""
    import numpy as np
    full = np.asarray(full, dtype=np.float64)
    for k, d in enumerate(deleted):
        move = np.abs(np.asarray(d, dtype=np.float64) / full - 1)
        assert (move > 10 * tol).all(), f"{what}: deleting planted row {k} moves the reference by {move.tolist()}, not more than {10 * tol:.3e}"


def glue_reference(labels, slices, prev, H: int, W: int, D: int):
    """The CCDM -> LDM stage glue on the CPU (oracle.samplers' zoom0 index rule, rot90(k=3), / 255): labels int [N, Dm, Hm, Wm], one slice
    index per sample, prev fp32 [N, H, W] or None -> (cond channel 0 bf16, channel 1 bf16, mask fp32), each [N, H, W]."""
    import torch
    from oracle import samplers as S
    N, Dm, Hm, Wm = labels.shape
    idd, ih, iw = (torch.from_numpy(S.zoom0_index(a, b)).long() for a, b in ((Dm, D), (Hm, H), (Wm, W)))
    mask = torch.stack([torch.rot90(labels[n, idd[s]][ih][:, iw], k=3, dims=(0, 1)).float() / 255.0 for n, s in enumerate(slices)])
    p = torch.zeros(N, H, W) if prev is None else prev
    return p.bfloat16(), mask.bfloat16(), mask
