"""Keeps tests/grid_caps.py honest without a GPU: every __global__ function of csrc/*.hip that reads gridDim has a row, the cap of the row
is the cap written at the kernel's launch sites, every covered row names gpu tests that exist, and the recorded shapes pass the cap with
a ragged end by plain arithmetic.  Two scratch copies of the sources show that the check bites: a removed row and a changed cap
literal each fail with a message that names the kernel."""
import os
import shutil

import grid_caps as G


def test_the_inventory_matches_the_sources():
    found = G.grid_stride_kernels()
    assert len(found) >= 40, sorted(found)                # the parser still finds the kernels (42 when this was written)
    problems = G.inventory_problems()
    assert not problems, "\n".join(problems)


def test_past_cap_and_sample_units():
    for cap in (682, 1024, 2048, 4096, 8192, 16384):
        n = G.past_cap(cap)
        assert n == cap * 256 + 259 and n // 256 == cap + 1 and n % 256 == 3 and n % 64 == 3
        assert G.past_cap(cap, 8) == 8 * n
    for cap in (4096, 8192, 16384):
        s = G.sample_units(cap)
        assert 2 * s >= cap * 256 and s % 256 and (3 * s) % 256 and (2 * s - cap * 256) % 64          # the border of samples 1 and 2: second trip, inside a wave
    assert G.S_RED == 262403 and G.MM_CAP == 682


def test_every_covered_shape_passes_its_cap_with_a_ragged_end():
    covered = [r for r in G.ROWS if r.exempt is None]
    assert len(covered) >= 30
    for r in covered:
        cap = G.cap_blocks(r)
        assert cap and r.work, r.kernel
        for w in r.work:
            units, per_block, c = w if isinstance(w, tuple) else (w, G.THREADS, cap)
            assert units > c * per_block, f"{r.kernel}: {units} units stay within {c} blocks of {per_block}"
            assert units % per_block, f"{r.kernel}: {units} units end on a block border"


def test_sample_borders_lie_in_the_second_trip():
    """the entries that decode a sample (or plane, or slice) index from a flat index: the last border lies at or past cap * 256 units"""
    t = G.THREADS
    assert 2 * G.GLUE_HW ** 2 >= 4096 * t and all(2 * hw * hw >= 4096 * t for hw, _, _ in G.CT_HW)
    D, N, hw = G.KEEP_VEC
    assert hw * hw % 4 == 0 and (D * N - 1) * hw * hw // 4 >= 4096 * t
    D, N, hw = G.KEEP_SCALAR
    assert hw * hw % 4 and (D * N - 1) * hw * hw >= 4096 * t
    assert 2 * G.ROWS_C2[2] >= 4096 * t
    N, S, C = G.GN_APPLY
    assert (N - 1) * S * C // 8 >= 8192 * t and S * C % 2 == 0
    N, S, C = G.GN_F32
    assert (N - 1) * S * C >= 16384 * t and S % 2 == 0                      # regime E of norm_exact needs an even element count per group
    for shape, up in ((G.RES_UP2D, True), (G.RES_UP3D, True), (G.RES_POOL2D, False), (G.RES_POOL3D, False)):
        assert 2 * G._res_units(shape, up) >= 16384 * t
    assert 2 * (2 * G.INTERP[2]) * (2 * G.INTERP[3]) >= 16384 * t
    N, C, S, cp = G.TO_CL
    assert N * S < 8192 * t < N * S * cp // 8                                # the second piece of a row: second trip only
    assert G.GELU_N % 8 == 5 and G.ACC_GENERAL[1] * G.ACC_GENERAL[2] // 8 > 2 * 4096 * t


def test_lpips_lane_rule_is_the_sources():
    """grid_caps.lpips_lanes restates tap_plan's rule; the source text it restates is pinned here"""
    text = open(os.path.join(G.CSRC, "gg_lpips.hip")).read()
    assert "while (L * 2 <= 64 && L * 2 * vec <= C)" in text and "const int vec = dtype == GG_F32 ? 4 : 8;" in text
    assert "const int G = LP_THREADS / L;" in text and "constexpr int LP_THREADS = 256;" in text
    assert [G.lpips_lanes(512, 8), G.lpips_lanes(512, 4), G.lpips_lanes(64, 8)] == [64, 64, 8]
    for C, h, w in G.LPIPS_SHAPES:
        assert G.lpips_quads(h, w) > G.LP_CAP * (256 // G.lpips_lanes(C, 8))
    assert G.LS_CAP == G._constant(G.CSRC, "gg_reduce.h", "LS_MAX_BLOCKS") and G.LP_CAP == G._constant(G.CSRC, "gg_lpips.hip", "LP_MAX_BLOCKS")


def test_a_removed_row_is_reported_by_kernel_name():
    rows = [r for r in G.ROWS if r.kernel != "lincomb4_kernel"]
    problems = G.inventory_problems(rows=rows)
    assert len(problems) == 1 and problems[0].startswith("lincomb4_kernel (gg_sampler.hip)") and "no row" in problems[0], problems


def test_a_changed_cap_literal_is_reported_by_kernel_name(tmp_path):
    """scratch copies of csrc with one cap literal changed each: a gg_blocks256 literal, an `x > N` clamp, LS_MAX_BLOCKS, the 2048 / N rule"""
    edits = [("gg_resample.hip", "gg_blocks256(total, 16384)", "gg_blocks256(total, 8192)", ["resample2x_kernel"]),
             ("gg_loss.hip", "if (blocks > 4096) blocks = 4096;", "if (blocks > 2048) blocks = 2048;", ["q_sample_rows_kernel"]),
             ("gg_reduce.h", "LS_MAX_BLOCKS = 1024;", "LS_MAX_BLOCKS = 512;",
              ["ccdm_step_loss_kernel", "gauss_kl_rows_kernel", "logit_stats_kernel", "loss_rows_kernel"]),
             ("gg_sampler.hip", "gg_blocks256(n, 2048)", "gg_blocks256(n, 1024)", ["minmax_apply_kernel", "minmax_seg_reduce_kernel"]),
             ("gg_lpips.hip", "LP_MAX_BLOCKS = 128;", "LP_MAX_BLOCKS = 256;", ["lpips_tap_kernel"])]
    for i, (name, old, new, kernels) in enumerate(edits):
        scratch = tmp_path / f"csrc{i}"
        shutil.copytree(G.CSRC, scratch)
        text = (scratch / name).read_text()
        assert text.count(old) >= 1, (name, old)
        (scratch / name).write_text(text.replace(old, new))
        problems = G.inventory_problems(str(scratch))
        assert sorted(p.split(":")[0] for p in problems) == kernels, (name, problems)
        assert all("the launch sites" in p for p in problems)


def test_a_new_capped_kernel_without_a_row_is_reported(tmp_path):
    scratch = tmp_path / "csrc"
    shutil.copytree(G.CSRC, scratch)
    with open(scratch / "gg_cond.hip", "a") as f:
        f.write("\n__global__ void brand_new_kernel(float *p, long long n)\n{\n    for (long long i = blockIdx.x * 256 + threadIdx.x; i < n; "
                "i += (long long)gridDim.x * 256) p[i] = 0.f;\n}\n")
    problems = G.inventory_problems(str(scratch))
    assert len(problems) == 1 and problems[0].startswith("brand_new_kernel (gg_cond.hip)"), problems
