"""CPU suite: the exact-arithmetic attention inputs (tests/attn_exact.py) satisfy their preconditions for every GPU case, the fp64
reference equals the closed form, an fp32 emulation of the kernel's step structure reproduces the expected bits for every plan the
cases use, and the comparators reject defects injected into that emulation.  No GPU: gg_attention_plan is host logic."""
import pytest
import torch

import attn_exact as X

torch.set_grad_enabled(False)

_CACHE = {}


def prepared(case, regime):
    key = (case.name, regime)
    if key not in _CACHE:
        inp = X.build(case, regime)
        _CACHE[key] = (inp, X.pack(case, inp))
    return _CACHE[key]


PAIRS = [pytest.param(c, r, id=f"{c.name}-{r}") for c in X.CASES for r in c.regimes()]


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.name)
def test_case_reaches_the_path_it_is_named_for(case):
    X.assert_path(case)


def test_every_path_has_all_regimes_layouts_and_head_dims():
    for path in ("plain", "ws2", "dma", "split"):
        cs = [c for c in X.CASES if c.path == path]
        assert {r for c in cs for r in c.regimes()} == set(X.REGIMES)
        assert {c.layout for c in cs} >= {"legacy", "new", "kv", "ae"}, path
        assert {c.D for c in cs} == ({32, 64, 128} if path in ("plain", "ws2") else {256, 384, 512})
        assert any(c.name in X.PEAKED for c in cs)
    assert {c.D for c in X.CASES if c.layout == "kv" and c.Tq != c.Tkv} >= {64, 128, 384}


@pytest.mark.parametrize("case,regime", PAIRS)
def test_preconditions_and_reference_equals_closed_form(case, regime):
    inp, p = prepared(case, regime)                       # build() asserts the preconditions
    if case.Tq * case.Tkv * case.D > 1 << 28:             # the two largest shapes: the reference of the first 512 queries
        sub = X.Inputs(inp.q[:, :512], inp.k, inp.v, inp.want[:, :512], inp.gid, inp.tgt[:, :, :512], inp.scale)
        X.check_reference(regime, sub, X.reference(sub))
    else:
        X.check_reference(regime, inp, X.reference(inp))
    # the packer: the addressed slots hold the inputs, everything else is NaN / the sentinel
    assert int(torch.isnan(p.q).sum()) == p.q.numel() - (inp.q.numel() + (0 if p.k is not p.q else inp.k.numel() + inp.v.numel()))
    assert X.stray_writes(case, p.out) == 0 and bool((X.out_view(case, p.out) == X.SENTINEL).all())


@pytest.mark.parametrize("case,regime", PAIRS)
def test_kernel_emulation_reproduces_the_expected_bits(case, regime):
    inp, p = prepared(case, regime)
    out = X.emulate(case, p, inp.scale)
    assert not X.check_output(case, inp, out), X.check_output(case, inp, out)
    if case.ks > 1:                                       # no workspace: the unsplit kernel, bit-identical on exact inputs
        out1 = X.emulate(case, p, inp.scale, workspace=False)
        assert not X.check_output(case, inp, out1)
        assert not X.mismatches(X.out_view(case, out1), X.out_view(case, out))


@pytest.mark.parametrize("case", X.F32_CASES, ids=lambda c: c.name)
def test_fp32_validation_inputs(case):
    for regime in case.regimes():
        inp = X.build(case, regime, dtype=torch.float32, scale=X.F32_SCALE)
        X.check_reference(regime, inp, X.reference(inp))


# What each defect does to the three regimes.  "+" the regime must reject it; "-" the regime cannot see it (asserted too, so that the
# table stays true).  Every defect is rejected by at least one regime that runs on every path.
#
# The gap being closed: would `rel_err < 2e-2` of tests/test_hip_parity.py (max |got - ref| / max |ref|, N(0,1) inputs) have passed
# the same defect?  Measured once with this emulation on N(0,1) inputs of the same shapes (worst (sample, head)); clean emulation
# 2.8e-3 (ws2_d64_t300_n2h3), 2.3e-3 (dma_d256_t100), 2.9e-3 (split_d512_t256).  At these small T a whole key weighs about 1 / 300 of
# a row, so the gross defects fail parity here; the issue's measurements at the production shapes (D512 T4096: one key never counted
# 3.0e-2 against the limit 2e-2) are where a whole key sits at the tolerance.  The two that pass even here are the subtle ones:
#   defect                         shape                  rel_err     parity verdict
#   drop_key                       ws2_d64_t300_n2h3      1.1e-1      fails
#   drop_key_16q                   ws2_d64_t300_n2h3      2.0e-2      passes
#   mask_off_by_one (zero pad row) ws2_d64_t300_n2h3      4.2e-3      passes
#   mask_off_by_one (clamped row)  dma_d256_t100          3.5e-1      fails
#   v_shift16                      ws2_d64_t300_n2h3      1.6         fails
#   swap_merge (two halves)        ws2_d64_t300_n2h3      1.1         fails
#   swap_merge (key ranges)        split_d512_t256        9.3e-1      fails
#   skip_rescale                   ws2_d64_t300_n2h3      3.8         fails
#   head_slip                      ws2_d64_t300_n2h3      1.5         fails
#   no_inv_l                       ws2_d64_t300_n2h3      3.3e+1      fails
#   untouched_row                  ws2_d64_t300_n2h3      3.3e-1      fails (output prefilled with 0)
DEFECT_TABLE = [
    # defect, case, verdict per regime (sel, grp, uni)
    ("drop_key", "ws2_d64_t300_n2h3", "+++"),
    ("drop_key_16q", "ws2_d64_t300_n2h3", "+++"),
    ("mask_off_by_one", "ws2_d64_t300_n2h3", "++-"),      # a zero pad row counted as live: l one too large, numerator unchanged
    ("mask_off_by_one", "dma_d256_t100", "-++"),          # the clamped last row counted twice: sel sees 2 v / 2
    ("v_shift16", "ws2_d64_t300_n2h3", "++ "),
    ("swap_merge", "ws2_d64_t300_n2h3", "+--"),           # grp / uni: both halves hold m = 0, the weights are 1 either way
    ("swap_merge", "split_d512_t256", "+--"),
    ("skip_rescale", "ws2_d64_t300_n2h3", "+  "),
    ("head_slip", "ws2_d64_t300_n2h3", "+++"),
    ("no_inv_l", "ws2_d64_t300_n2h3", "-+-"),             # sel: l = 1; uni: 0 / l
    ("untouched_row", "ws2_d64_t300_n2h3", "+++"),
]


@pytest.mark.parametrize("defect,name,verdicts", DEFECT_TABLE, ids=[f"{d}-{n}" for d, n, _ in DEFECT_TABLE])
def test_comparators_reject_injected_defects(defect, name, verdicts):
    case = X.CASE[name]
    for regime, verdict in zip(X.REGIMES, verdicts):
        inp, p = prepared(case, regime)
        assert not X.check_output(case, inp, X.emulate(case, p, inp.scale))
        bad = X.check_output(case, inp, X.emulate(case, p, inp.scale, defect=defect, key=inp.probe_key(0, 0, 20)))
        if verdict == "+":
            assert bad, f"{defect} on {name} passes the {regime} regime"
        elif verdict == "-":
            assert not bad, f"{defect} on {name}: the {regime} regime was recorded as blind to it: {bad}"
    assert "+" in verdicts
    assert set(d for d, _, _ in DEFECT_TABLE) == set(X.DEFECTS)


def test_comparator_treats_signed_zero_as_equal_and_nothing_else():
    a = torch.tensor([0.0, -0.0, 1.0, 3.0]).bfloat16().view(1, 1, 1, 4)
    assert not X.mismatches(a, torch.tensor([-0.0, 0.0, 1.0, 3.0]).bfloat16().view(1, 1, 1, 4))
    assert X.mismatches(a, torch.tensor([0.0, 0.0, 1.0, 3.015625]).bfloat16().view(1, 1, 1, 4))          # one bf16 ulp
    assert X.mismatches(a, torch.tensor([0.0, 0.0, float("nan"), 3.0]).bfloat16().view(1, 1, 1, 4))


@pytest.mark.parametrize("name", X.PEAKED)
def test_peaked_inputs_hold_their_preconditions_and_the_emulation_the_bound(name):
    case = X.CASE[name]
    inp = X.peaked(case)                                  # asserts: every tile max rises, score spread
    p = X.pack(case, inp)
    out = X.emulate(case, p, inp.scale)
    assert X.stray_writes(case, out) == 0
    assert X.peaked_ratio(case, inp, out) <= 1.0
