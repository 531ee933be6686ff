"""CPU suite: the exact-arithmetic norm inputs (tests/norm_exact.py) satisfy their preconditions for every GPU case, every case reaches
the kernel it is named for through the Python mirrors of the host gates, the fp64 reference rounds to the closed form, an fp32
emulation of each kernel's walk reproduces the expected bits, and the comparators reject defects injected into that emulation.
No GPU: the gates are host logic (gg_groupnorm_fused_supported is called directly)."""
import pytest
import torch

import norm_exact as X
import shadow

torch.set_grad_enabled(False)

_CACHE = {}
BIG = 1 << 22                # elements: the two largest shapes run one (act, eps) leg of the emulation here


def prepared(case, N, act):
    key = (case.name, N, act)
    if key not in _CACHE:
        inp = X.build(case, N, act)
        _CACHE[key] = (inp, X.pack(inp))
    return _CACHE[key]


GN = [pytest.param(c, n, id=f"{c.name}-n{n}") for c in X.CASES for n in c.Ns]


def legs(case, N):
    if case.path in ("f32", "film"):
        return [(False, 0.0)]
    if N * case.S * case.C > BIG:
        return [(True, 1e-5)]
    return [(a, e) for a in (False, True) for e in X.EPS]


@pytest.mark.parametrize("case,N", GN)
def test_case_reaches_the_path_it_is_named_for(case, N):
    X.assert_path(case, N)


def test_the_table_covers_every_path_and_edge():
    paths = {c.path for c in X.CASES}
    assert paths == {"small", "partial", "fused", "lean1", "lean2", "lean4", "lean8", "general", "ssacc", "f32", "film"}
    for k in ("lean1", "lean2", "lean4", "lean8"):
        assert {c.swz for c in X.CASES if c.path == k} == {True, False}, k
    assert any(c.S * c.C == 1 << 19 for c in X.CASES if c.path == "small")
    assert any(c.S * X.fused_np(c.C) == 512 for c in X.CASES if c.path == "fused")
    assert any(c.S * (c.C // 8) > 1 << 20 for c in X.CASES if c.path == "general")
    assert any(X.gn_nblk(1, c.S) == 1024 and 1024 * c.cpg > 1024 for c in X.CASES if c.path == "partial")
    assert any((c.C1 % c.cpg) and c.C2 for c in X.CASES if c.path in ("small", "partial", "fused", "lean2"))       # a group straddles the sources
    assert {c.stripes for c in X.CASES if c.path == "ssacc"} == {(1, 1), (32, 32), (32, 1)}
    assert all(2 in c.Ns or c.Ns in ((1, 3), (1,)) for c in X.CASES)


def test_fused_gate_mirror_matches_the_library():
    from jointimagegeneration_amd import _lib
    lib = _lib.load()
    for args in X.FUSED_ON_EDGE:
        assert lib.gg_groupnorm_fused_supported(*args) == 1 and X.fused_small_ok(*args), args
    for args in X.FUSED_PAST_EDGE:
        assert lib.gg_groupnorm_fused_supported(*args) == 0 and not X.fused_small_ok(*args), args
    for S in (1, 16, 64, 100, 256, 512, 513):
        for C1, C2 in ((32, 0), (64, 0), (160, 0), (320, 160), (160, 320), (800, 0), (1440, 0), (2048, 0), (2080, 0)):
            assert bool(lib.gg_groupnorm_fused_supported(S, C1, C2, C1 + C2)) == X.fused_small_ok(S, C1, C2, C1 + C2), (S, C1, C2)


def test_silu_palette_drops_the_values_next_to_a_rounding_boundary():
    plain, act = X.palette(False), X.palette(True)
    outs = lambda pal: {s * g + b for g, b in pal for s in (1.0, -1.0)}
    assert len(outs(plain)) == 24 and min(abs(t) for t in outs(plain)) == X.FLOOR
    assert 2.0 in outs(plain) and -1.25 in outs(plain)
    assert 2.0 not in outs(act) and -1.25 not in outs(act)
    assert len(outs(act)) >= 20 and set(act) <= set(plain)


@pytest.mark.parametrize("case,N", GN)
def test_preconditions_and_reference_equals_closed_form(case, N):
    for act in ((False,) if case.path in ("f32", "film") else (False, True)):
        inp, p = prepared(case, N, act)                    # build() asserts the preconditions
        for eps in ((0.0,) if case.path in ("f32", "film") else X.EPS):
            X.check_reference(inp, eps)
        # the packer: guards and coefficient pad lanes are NaN, the body holds the inputs
        assert bool(torch.isnan(p.x1[:X.GUARD]).all()) and bool(torch.isnan(p.x1[-X.GUARD:]).all()) and not bool(torch.isnan(X.body(p.x1)).any())
        assert int(torch.isnan(X.body(p.gamma)).sum()) == case.C - case.clog
        if p.acc1 is not None:
            assert bool((p.acc1[:X.GUARD] == X.I64_POISON).all())


@pytest.mark.parametrize("case,N", GN)
def test_kernel_emulation_reproduces_the_expected_bits(case, N):
    for act, eps in legs(case, N):
        inp, p = prepared(case, N, act)
        res = X.emulate(case.path, p, eps, act)
        bad = X.check_result(inp, eps, res)
        assert not bad, f"{case.name} N={N} act={act} eps={eps}: {bad}"


# Injected defects (the issue's table) and the comparator that must reject each: "out" the bit comparison of the bf16 output (or the
# guards around it), "tables" the fp32 scale / shift allowance.  "-" records a comparator that cannot see the defect (asserted too).
DEFECT_TABLE = [
    # id, defect, case, N, (out, tables)
    ("a", "drop_last", "small_c160_2x3", 1, "++"),
    ("a", "drop_last", "fused_c160_7x8", 1, "+ "),
    ("a", "drop_last", "partial_c160_58x58", 1, "++"),                # 1 of 16820 elements: 24 % of the variance
    ("b", "foreign_lane", "small_c160_2x3", 1, "++"),
    ("b", "foreign_lane", "fused_c160p320_6x6", 1, "+ "),
    ("c", "group_round", "lean1_c160_5x6", 1, "+ "),
    ("c", "group_round", "lean2_c160p320_2x17", 3, "+ "),
    ("d", "second_src_at_c", "small_c160p320_2x3", 1, "++"),
    ("d", "second_src_at_c", "fused_c320p320_8x8", 3, "+ "),
    ("e", "sample0_stats", "small_c320_7x9", 3, "++"),
    ("e", "sample0_stats", "lean4_c640_1x5", 3, "+ "),
    ("e", "sample0_stats", "fused_c640_8x8", 3, "+ "),
    ("f", "cnt_from_C", "small_c192_l160_2x3", 1, "++"),
    ("f", "cnt_from_C", "lean1_c192_l160_4x5", 1, "+ "),
    ("f", "cnt_from_C", "ssacc_c192_l160_2x3_st32_32", 1, " +"),
    ("g", "fold_missing", "lean2_c320_2x5", 1, "+ "),
    ("g", "fold_missing", "ssacc_c96p64_2x3_st32_1", 3, " +"),
    ("g", "fold_missing", "partial_c160_58x58", 1, "++"),
    ("h", "store_whole", "fused_c160_7x8", 1, "+ "),
    ("h", "store_whole", "fused_c160p320_6x6", 3, "+ "),
    ("i", "fp32_inv_cnt", "small_c160_2x3", 1, "-+"),                 # caught by the tables only: rstd moves by ~1e-4, 1 / 50 of a bf16 ulp
    ("i", "fp32_inv_cnt", "ssacc_c160p320_2x3_st1_1", 1, " +"),
]


@pytest.mark.parametrize("tag,defect,name,N,verdicts", DEFECT_TABLE, ids=[f"{t}-{d}-{n}" for t, d, n, _, _ in DEFECT_TABLE])
def test_comparators_reject_injected_defects(tag, defect, name, N, verdicts):
    case = X.CASE[name]
    act, eps = False, 0.0
    inp, p = prepared(case, N, act)
    assert not X.check_result(inp, eps, X.emulate(case.path, p, eps, act))
    res = X.emulate(case.path, p, eps, act, defect=defect)
    for which, verdict in zip(("out", "tables"), verdicts):
        bad = X.check_result(inp, eps, res, tables=which == "tables", out=which == "out")
        if verdict == "+":
            assert bad, f"{defect} on {name} passes the {which} comparator"
        elif verdict == "-":
            assert not bad, f"{defect} on {name}: the {which} comparator was recorded as blind to it: {bad}"
    assert "+" in verdicts


def test_defect_table_is_complete():
    assert {d for _, d, _, _, _ in DEFECT_TABLE} | {"next_row_mean"} == set(X.DEFECTS)
    assert {t for t, _, _, _, _ in DEFECT_TABLE} == set("abcdefghi")       # j: test_layernorm_defect_next_row_mean


@pytest.mark.parametrize("C,stride", [(c, c) for c in X.LN_WIDTHS] + list(X.LNR_SHAPES))
def test_layernorm_inputs_reference_and_emulation(C, stride):
    for rows in (X.LN_ROWS if C == stride else X.LNR_ROWS):
        ln = X.build_layernorm(rows, C, stride)
        for eps in X.EPS:
            assert not X.mismatches(X.layernorm_reference(ln, eps).to(torch.bfloat16), ln.want)
            bad = X.check_layernorm(ln, X.emulate_layernorm(ln, eps))
            assert not bad, f"C={C} stride={stride} rows={rows} eps={eps}: {bad}"


@pytest.mark.parametrize("C,stride", [(520, 520), (50, 64)])
def test_layernorm_defect_next_row_mean(C, stride):
    """defect j: row r + 1's mean used for row r"""
    ln = X.build_layernorm(5, C, stride)
    assert not X.check_layernorm(ln, X.emulate_layernorm(ln, 0.0))
    assert X.check_layernorm(ln, X.emulate_layernorm(ln, 0.0, defect="next_row_mean"))


def test_comparators_signed_zero_guards_and_pad_lanes():
    a = torch.tensor([0.0, -0.0, 1.0, 3.0]).bfloat16()
    assert not X.mismatches(a, torch.tensor([-0.0, 0.0, 1.0, 3.0]).bfloat16())
    assert X.mismatches(a, torch.tensor([0.0, 0.0, 1.0, 3.015625]).bfloat16())          # one bf16 ulp
    assert X.mismatches(a, torch.tensor([0.0, 0.0, float("nan"), 3.0]).bfloat16())
    case = X.CASE["small_c192_l160_2x3"]
    inp, p = prepared(case, 1, False)
    res = X.emulate(case.path, p, 0.0, False)
    assert not X.check_result(inp, 0.0, res)
    for buf, where in ((res.out, X.GUARD - 1), (res.out, res.out.numel() - X.GUARD), (res.scale, 0), (res.shift, res.shift.numel() - 1)):
        keep = buf[where].clone()
        buf[where] = 1.0
        assert "guard" in X.check_result(inp, 0.0, res)
        buf[where] = keep
    X.body(res.scale).view(1, case.C)[0, 170] = 2.0 ** -20                               # a pad lane of a table
    assert "pad lanes" in X.check_result(inp, 0.0, res)
    X.body(res.scale).view(1, case.C)[0, 170] = 0.0
    X.body(res.out).view(1, case.S, case.C)[0, 3, 161] = 2.0 ** -20                      # a pad lane of the output
    assert X.check_result(inp, 0.0, res)
    # the table allowance: 2 ulp pass, 3 ulp fail
    X.body(res.out).view(1, case.S, case.C)[0, 3, 161] = 0.0
    sc = X.body(res.scale).view(1, case.C)
    ref = sc[0, 7].clone()
    step = float(X._ulp32(ref.double().reshape(1)))
    sc[0, 7] = ref + 2 * step
    assert not X.check_result(inp, 0.0, res)
    sc[0, 7] = ref + 3 * step
    assert "scale" in X.check_result(inp, 0.0, res)


def test_accumulators_are_exact_uneven_and_signed():
    case = X.CASE["ssacc_c160p320_2x3_st32_1"]
    inp, p = prepared(case, 3, False)
    a1 = X.body(p.acc1).view(3, 32, case.C1, 2)
    assert bool((a1 < 0).any()) and bool((a1 == 0).any()) and len(torch.unique(a1[0, :, 0, 0])) > 8
    tot = torch.cat([a1.sum(1), X.body(p.acc2).view(3, 1, case.C2, 2).sum(1)], 1).reshape(3, 32, case.cpg, 2).sum(2).double()
    assert bool((tot[:, :, 0] / X.ACC_SUM_SCALE == case.cnt * inp.m).all())
    assert bool((tot[:, :, 1] / X.ACC_SQ_SCALE == case.cnt * (inp.m ** 2 + inp.s ** 2)).all())


@pytest.mark.parametrize("ratio", X.R_RATIOS)
def test_random_regime_reference_passes_its_own_bounds(ratio):
    """regime R on the CPU: the emulation of the small path on random data sits inside the shadow bounds"""
    N, C1, C2, sp = X.R_SHAPES[2]
    x, gamma, beta = X.build_random(N, C1, C2, sp, ratio, True)
    assert (x.shape[1] * ((C1 + C2) // 32)) % 2 == 1
    for path in X.random_paths(N, x.shape[1], C1, C2):
        st = (32, 1) if path == "ssacc" else (1, 1) if path.startswith("lean") else None
        p = X.pack_raw(x, C1, C2, C1 + C2, gamma, beta, st, exact=False)
        res = X.emulate(path, p, 1e-5, True)
        for what, r in X.random_ratios(path, x, C1, gamma, beta, 1e-5, True, res).items():
            assert r <= 1.0, (path, what, r)
