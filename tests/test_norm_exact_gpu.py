"""GPU suite (-m gpu): every GroupNorm / LayerNorm kernel path bit for bit against the closed form of regime E (tests/norm_exact.py: the
inputs, their preconditions, the comparators, the packer with guarded buffers), which is the fp64 reference rounded to the storage type.
The exact tests have no tolerance on the outputs; the fp32 scale / shift tables carry the allowance derived in norm_exact.py.

Paths, each proven by the Python mirror of the host gates on the shape of the launch itself (norm_exact.assert_path):
  small     gn_stats_small + gn_apply                    partial   gn_partial + gn_finalize + gn_apply
  fused     gn_fused_small (one launch)                  lean<CPT> gn_apply_acc_lean<1, 2, 4, 8>, swizzled and unswizzled grids
  general   gn_apply_acc (more than 2^20 pieces)         ssacc     gn_scale_shift_acc (tables only; 1 and 32 stripes)
  f32/film  gn_f32_stats + gn_f32_apply / _film (fp32 storage, eps = 0, act off: fp32 SiLU is not exact)
  layernorm_kernel, layernorm_rows_kernel
Every GroupNorm case runs with N in {1, 3} (unless the table says otherwise), act off and on, eps in {0, 1e-5}.  Inputs sit between NaN
guards, outputs are sentinel-filled with 256 guard elements on either side, coefficient pad lanes are NaN.

v_rsq_f32 on powers of 4 (test_rsqrt_on_powers_of_four, read back through a gamma = 1 scale table of gn_stats_small, eps = 0).
Measured on an MI355X: the largest deviation from 1 / s is 0 ulp for every s^2 in {1/16, 1/4, 1, 4}: v_rsq_f32 is exact on these powers
of 4 (the test asserts <= 1 ulp; the bf16 outputs do not depend on it).  Every case of every path is bit exact.

Regime R (odd element counts, odd LayerNorm widths, random data at mean / std 0 and 200) is held to the bounds of tests/shadow.py.
"""
import pytest
import torch

import norm_exact as X
import shadow

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


GN = [pytest.param(c, n, id=f"{c.name}-n{n}") for c in X.CASES for n in c.Ns]


@pytest.mark.parametrize("case,N", GN)
def test_groupnorm_bit_exact(case, N, dev):
    X.assert_path(case, N)
    f32 = case.path in ("f32", "film")
    for act in ((False,) if f32 else (False, True)):
        inp = X.build(case, N, act)                        # asserts the preconditions
        p = X.pack(inp).to(dev)
        for eps in ((0.0,) if f32 else X.EPS):
            X.check_reference(inp, eps, dev)
            res = X.launch(case.path, p, eps, act)
            bad = X.check_result(inp, eps, res)
            assert not bad, f"{case.name} N={N} act={act} eps={eps}: {bad}"


def test_fused_gate_one_step_past_each_edge(dev):
    from jointimagegeneration_amd import _lib
    lib = _lib.load()
    for args in X.FUSED_ON_EDGE:
        assert lib.gg_groupnorm_fused_supported(*args) == 1 and X.fused_small_ok(*args), args
    for args in X.FUSED_PAST_EDGE:
        assert lib.gg_groupnorm_fused_supported(*args) == 0 and not X.fused_small_ok(*args), args


def test_rsqrt_on_powers_of_four(dev):
    """rstd of every spread in use, read back through a gamma = 1, beta = 0 scale table: at most 1 ulp from 1 / s"""
    case = X.CASE["small_c64_2x3x5"]
    inp = X.build(case, 3, False)
    p = X.pack_raw(inp.x, case.C1, 0, case.clog, torch.ones(case.clog), torch.zeros(case.clog)).to(dev)
    res = X.launch("small", p, 0.0, False)
    rstd = X.body(res.scale).view(3, case.C).double().cpu()
    want = (1.0 / inp.s).repeat_interleave(case.cpg, 1)
    assert {float(v) for v in inp.s.flatten()} == set(X.SPREADS)
    dev_ulp = ((rstd - want).abs() / X._ulp32(want))
    for sp in X.SPREADS:
        print(f"v_rsq_f32({sp * sp}): deviation {float(dev_ulp[want == 1.0 / sp].max())} ulp from {1.0 / sp}")
    print(f"v_rsq_f32 on powers of 4: largest deviation {float(dev_ulp.max())} ulp")
    assert float(dev_ulp.max()) <= 1.0


@pytest.mark.parametrize("C", X.LN_WIDTHS)
def test_layernorm_bit_exact(C, dev):
    for rows in X.LN_ROWS:
        ln = X.build_layernorm(rows, C, C)
        d = ln.to(dev)
        for eps in X.EPS:
            assert not X.mismatches(X.layernorm_reference(ln, eps).to(torch.bfloat16), ln.want)
            out = X.launch_layernorm(d.x, rows, C, C, d.gamma, d.beta, eps)
            bad = X.check_layernorm(d, out)
            assert not bad, f"layernorm C={C} rows={rows} eps={eps}: {bad}"


@pytest.mark.parametrize("C,stride", X.LNR_SHAPES)
def test_layernorm_rows_bit_exact(C, stride, dev):
    for rows in X.LNR_ROWS:
        ln = X.build_layernorm(rows, C, stride)
        d = ln.to(dev)
        for eps in X.EPS:
            assert not X.mismatches(X.layernorm_reference(ln, eps).to(torch.bfloat16), ln.want)
            out = X.launch_layernorm(d.x, rows, C, stride, d.gamma, d.beta, eps)
            bad = X.check_layernorm(d, out)                # pad lanes [C, stride) are 0 in the closed form
            assert not bad, f"layernorm_rows C={C} stride={stride} rows={rows} eps={eps}: {bad}"


@pytest.mark.parametrize("ratio", X.R_RATIOS)
@pytest.mark.parametrize("N,C1,C2,sp", X.R_SHAPES, ids=[f"n{s[0]}_c{s[1]}p{s[2]}" for s in X.R_SHAPES])
def test_random_data_within_the_shadow_bounds(N, C1, C2, sp, ratio, dev):
    """regime R: odd element counts and generic data through every bf16 path that accepts the shape"""
    for act in (False, True):
        x, gamma, beta = X.build_random(N, C1, C2, sp, ratio, act)
        S, C = x.shape[1], C1 + C2
        assert (S * (C // 32)) % 2 == 1                    # what regime E cannot express
        xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
        for path in X.random_paths(N, S, C1, C2):
            st = (32, 1) if path == "ssacc" else (X.ACC_STRIPES, X.ACC_STRIPES) if path not in ("small", "partial", "fused") else None
            p = X.pack_raw(x, C1, C2, C, gamma, beta, st, exact=False).to(dev)
            for eps in X.EPS:
                res = X.launch(path, p, eps, act)
                for what, r in X.random_ratios(path, xd, C1, gd, bd, eps, act, res).items():
                    print(f"regime R {path} {what} N={N} C={C1}+{C2} ratio={ratio} act={act} eps={eps}: {r:.3f}")
                    assert r <= 1.0, (path, what, r)


@pytest.mark.parametrize("ratio", X.R_RATIOS)
@pytest.mark.parametrize("C,stride", X.R_LN)
def test_random_rows_of_odd_width_within_the_shadow_bound(C, stride, ratio, dev):
    gen = torch.Generator().manual_seed(C + int(ratio))
    rows = 5
    x = torch.zeros(rows, stride, dtype=torch.bfloat16)
    x[:, :C] = (torch.randn(rows, C, generator=gen) + ratio).to(torch.bfloat16)
    gamma, beta = 1.0 + 0.5 * torch.randn(C, generator=gen), 0.5 * torch.randn(C, generator=gen)
    nan = float("nan")
    xg, gg, bg = (X.guarded(t, nan).to(dev) for t in (x, gamma, beta))
    for eps in X.EPS:
        out = X.launch_layernorm(xg, rows, C, stride, gg, bg, eps)
        assert X.guards_intact(out)
        got = X.body(out).view(rows, stride)
        assert not bool((got[:, C:] != 0).any())
        r = shadow.layernorm_ratio(x[:, :C].to(dev), gamma.to(dev), beta.to(dev), eps, got[:, :C])
        print(f"regime R layernorm_rows C={C} ratio={ratio} eps={eps}: {r:.3f}")
        assert r <= 1.0, r
