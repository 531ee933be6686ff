"""CPU suite: the exact-arithmetic conv helper (tests/conv_exact.py) itself.  The regime builders meet their preconditions for every
case the GPU module runs, the fp64 reference alone stays inside the regime's condition, torch's own fp32 conv is bit-equal to fp64 on
such inputs, and each comparator passes a clean kernel-like output (the reference rounded to the output type) but fails on each
injected defect -- among them the single dropped product that both tolerance-based checks of the suite let through."""
import pytest
import torch
import torch.nn.functional as F

import conv_exact as X
import shadow as SH
from test_shadow_cpu import kernel_like, torch_conv
from util import rel_err

torch.set_grad_enabled(False)
ALL_PAIRS = [cr for g in X.GROUPS.values() for cr in g]
REF_BUDGET = 4e9            # positions x K x Cout of a reference evaluated here (at most a second or two of fp64 on a few cores)


@pytest.mark.parametrize("cr", ALL_PAIRS, ids=X.case_id)
def test_regime_builders_meet_their_preconditions(cr):
    """build_inputs asserts the value-level preconditions itself; where the fp64 reference is affordable here (small chunks), it is
    evaluated and must satisfy the regime's condition: integer |y| <= 120 in regime S, a multiple of 1/8 below 2^24 quanta otherwise.
    (For the larger shapes the same follows from the asserted structure: at most 96 products of magnitude 1 plus bias and residual.)"""
    case, regime = cr
    inp = X.build_inputs(case, regime)
    assert inp.w.shape == (case.cout, case.cin_w, case.taps) and [s.shape[-1] % 32 for s in inp.srcs] == [0] * len(inp.srcs)
    if case.M * case.K * case.cout <= REF_BUDGET:
        ref = X.reference(case, inp, chunk=1 << 21)
        assert tuple(ref.shape) == (case.N,) + tuple(case.out_sp) + (case.cout,)
        X.check_reference(regime, ref)
        if regime == "S":
            assert float(ref.abs().max()) > 8            # not degenerate


def test_case_lists_cover_the_listed_paths():
    paths = {c.path for c, _ in ALL_PAIRS}
    assert paths == {"gather", "gather5", "tiny", "halo", "team", "box", "spec", "f32"}
    assert len({(c.name, r) for c, r in ALL_PAIRS}) == len(ALL_PAIRS)
    assert sum(1 for c, _ in X.GROUPS["spec"] if _ == "D") == len(X.SPEC_CASES) >= 40
    assert {r for _, r in X.GROUPS["team"]} == {"D", "S", "P"} and {r for _, r in X.GROUPS["halo"]} == {"D", "S", "P"}


def test_host_predicates_place_every_case_on_its_kernel():
    """The path assertion of the GPU module, on the descriptors the cases produce (host code only; the team kernel's dry run asks the
    device for its CU count, so path_hint 7 is left to the GPU module)."""
    from jointimagegeneration_amd import _lib
    lib = _lib.load()
    for case, regime in ALL_PAIRS:
        if case.path in ("f32", "team"):
            continue
        for hint in ((1, 4, 6) if case.hint is None else (case.hint,)):
            X.assert_path(lib, X.case_desc(case, regime, hint), case)


def test_torch_fp32_conv_is_bitwise_fp64_on_regime_d():
    """The premise: K = 17 280 products per output, every partial sum exact in fp32, in whatever order ATen adds them."""
    case = X.c3("premise", "gather", 1, 640, 0, 32, (4, 4, 4))
    inp = X.build_inputs(case, "D")
    x = inp.srcs[0].float().permute(0, 4, 1, 2, 3)
    w = inp.w.view(32, 640, 3, 3, 3)
    y32 = F.conv3d(x, w, inp.bias[:32], padding=1)
    y64 = F.conv3d(x.double(), w.double(), inp.bias[:32].double(), padding=1)
    assert torch.equal(y32.double(), y64)
    assert torch.equal(X.reference(case, inp), y64.permute(0, 2, 3, 4, 1))
    assert float(y64.abs().max()) * 8 <= case.K * 16 + 8


# ------------------------------------------------------------------------------------------------ comparators and injected defects
SMALL = {
    "plain": X.c2("m_plain", "box", 2, 64, 0, 40, (9, 10), bias="per_sample"),
    "3d": X.c3("m_3d", "halo", 1, 32, 32, 24, (4, 5, 6), residual=True),
    "skip": X.c2("m_skip", "box", 1, 32, 0, 40, (6, 8), skip=(64, 32)),
    "f32": X.c2("m_f32", "box", 1, 96, 0, 14, (5, 7), out_f32=True),
}


def clean(case, regime):
    inp = X.build_inputs(case, regime)
    ref = X.reference(case, inp, chunk=1 << 20)
    return inp, ref


def rejects(case, regime, ref, y_bad):
    """y_bad stored as a kernel would store it (rounded to the output type, zero pad lanes) must not pass"""
    out = torch.zeros(tuple(y_bad.shape[:-1]) + (SH.pad32(case.cout),), dtype=torch.float32 if case.out_f32 else torch.bfloat16)
    out[..., :case.cout] = y_bad.to(out.dtype)
    with pytest.raises(AssertionError):
        X.check_output(out, ref, regime)


@pytest.mark.parametrize("name, regime", [(n, r) for n in ("plain", "3d", "f32") for r in "DSP"] + [("skip", "D")])      # (the skip projection: regime D only)
def test_comparator_passes_clean_output_and_reference_equals_torch(name, regime):
    case = SMALL[name]
    inp, ref = clean(case, regime)
    X.check_reference(regime, ref)
    call = X.conv_call(case, inp)
    assert torch.equal(torch_conv(call), ref)                       # F.conv3d in fp64: exact inputs leave no 1e-12 either
    out = kernel_like(call, ref, torch.float32 if case.out_f32 else torch.bfloat16)
    X.check_output(out, ref, regime)
    if regime == "S":
        acc = torch.zeros(case.N, 32, SH.pad32(case.cout), 2, dtype=torch.int64)
        want = X.expected_acc(ref)
        acc[:, 3, :case.cout], acc[:, 17, :case.cout] = want - 5, 5                    # striped: only the sum over stripes counts
        X.check_acc(acc, ref)


def _mutated(case, regime, mutate):
    inp, ref = clean(case, regime)
    bad = X.build_inputs(case, regime)
    mutate(bad)
    return ref, torch_conv(X.conv_call(case, bad))


@pytest.mark.parametrize("regime", ["D", "S"])
@pytest.mark.parametrize("name", ["plain", "3d", "f32"])
def test_comparator_fails_on_a_dropped_product_channel_or_chunk(name, regime):
    case = SMALL[name]
    inp, _ = clean(case, regime)
    nz = inp.w.ne(0).nonzero()
    o, c, t = (int(v) for v in nz[len(nz) // 2])

    def one(b): b.w[o, c, t] = 0                                     # one (cout, cin, tap) product
    def last_channel(b): b.w[:, -1, :] = 0                           # last input channel in every tap
    def last_chunk(b): b.w[:, -32:, -1] = 0                          # last 32-channel chunk of the last tap
    for mutate in (one, last_channel, last_chunk):
        ref, y_bad = _mutated(case, regime, mutate)
        assert not torch.equal(y_bad, ref)
        rejects(case, regime, ref, y_bad)


@pytest.mark.parametrize("regime", ["D", "S"])
def test_comparator_fails_on_a_border_tap_that_was_not_zero_padded(regime):
    """The W = -1 column of the padded input holds column 0 instead of zeros (one tap column at one border)."""
    case = SMALL["plain"]
    inp, ref = clean(case, regime)
    x = inp.srcs[0].double().permute(0, 4, 1, 2, 3)[:, :, 0]
    xp = F.pad(x, (1, 1, 1, 1))
    xp[..., 1:-1, 0] = xp[..., 1:-1, 1]
    W = torch.zeros(case.cout, x.shape[1], 3, 3, dtype=torch.float64)
    W[:, :case.cin_w] = inp.w.double().view(case.cout, case.cin_w, 3, 3)
    y = F.conv2d(xp, W).permute(0, 2, 3, 1)[:, None] + inp.bias.double()[:, None, None, None, :case.cout]
    assert torch.equal(y[..., 1:, :], ref[..., 1:, :]) and not torch.equal(y, ref)
    rejects(case, regime, ref, y)


@pytest.mark.parametrize("name", ["plain", "3d"])
def test_comparator_fails_on_a_prologue_applied_to_padded_taps(name):
    case = SMALL[name]
    inp, ref = clean(case, "P")
    y_bad = torch_conv(X.conv_call(case, inp), pad_prologue_bug=True)
    inner = (slice(None),) + tuple(slice(1, -1) if e > 1 else slice(None) for e in case.out_sp)
    assert torch.equal(y_bad[inner], ref[inner]) and not torch.equal(y_bad, ref)
    rejects(case, "P", ref, y_bad)


def test_comparator_fails_on_a_missing_skip_channel_and_a_swapped_bias_row():
    case = SMALL["skip"]
    def no_last_skip_channel(b): b.skip_w[:, -1] = 0
    ref, y_bad = _mutated(case, "D", no_last_skip_channel)
    rejects(case, "D", ref, y_bad)
    case = SMALL["plain"]
    for regime in ("D", "S"):
        inp, ref = clean(case, regime)
        assert not torch.equal(inp.bias[0], inp.bias[1])
        rejects(case, regime, ref, torch_conv(X.conv_call(case, inp), bias_swap=True))


def test_comparator_fails_on_a_non_zero_pad_lane_and_a_wrong_rounding():
    case = SMALL["plain"]
    inp, ref = clean(case, "D")
    out = kernel_like(X.conv_call(case, inp), ref)
    X.check_output(out, ref, "D")
    bad = out.clone()
    bad[1, 0, 3, 4, case.cout] = 2.0 ** -20
    with pytest.raises(AssertionError, match="pad lanes"):
        X.check_output(bad, ref, "D")
    # truncation instead of round-to-nearest-even differs somewhere on regime D data (values with more than 8 significant bits)
    trunc = out.clone()
    trunc[..., :case.cout] = (ref.float().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    assert not torch.equal(trunc, out)
    with pytest.raises(AssertionError, match="round-to-nearest-even"):
        X.check_output(trunc, ref, "D")


def test_accumulator_comparator_fails_one_quantum_off():
    case = SMALL["plain"]
    inp, ref = clean(case, "S")
    acc = torch.zeros(case.N, 1, SH.pad32(case.cout), 2, dtype=torch.int64)
    acc[:, 0, :case.cout] = X.expected_acc(ref)
    X.check_acc(acc, ref)
    # the fixed-point sums are what the kernels' scales say
    y = ref.reshape(case.N, -1, case.cout)
    assert torch.equal(acc[:, 0, :case.cout, 0].double(), y.sum(1) * SH.ACC_SUM_SCALE) and torch.equal(acc[:, 0, :case.cout, 1].double(), (y * y).sum(1) * SH.ACC_SQ_SCALE)
    for j in (0, 1):
        bad = acc.clone()
        bad[1, 0, 7, j] += 1
        with pytest.raises(AssertionError, match="accumulators differ"):
            X.check_acc(bad, ref)
    bad = acc.clone()
    bad[0, 0, case.cout, 0] = 1
    with pytest.raises(AssertionError, match="pad lanes"):
        X.check_acc(bad, ref)


def test_preconditions_reject_inputs_outside_the_regime():
    case = SMALL["plain"]
    for regime, spoil in (("D", lambda b: b.w.__setitem__((0, 0, 0), 0.3)), ("D", lambda b: b.srcs[0].__setitem__((0, 0, 0, 0, 0), 0.0)),
                          ("S", lambda b: b.w.__setitem__((0, 0, 0), 1.0 - b.w[0, 0, 0].abs())), ("P", lambda b: b.prologue[1].__setitem__((0, 3), 0.0)),
                          ("P", lambda b: b.prologue[0].__setitem__((0, 3), 0.3))):
        b = X.build_inputs(case, regime)
        spoil(b)
        with pytest.raises(AssertionError):
            X.check_preconditions(case, regime, b)
    with pytest.raises(AssertionError):
        X.check_preconditions(X.c2("too_deep", "box", 1, 160 * 1024, 0, 32, (4, 4)), "D", X.build_inputs(SMALL["plain"], "D"))


def test_the_gap_a_single_dropped_product_passes_both_tolerance_checks():
    """640 -> 32, 3x3x3, K = 17 280: one weight of one (cout, cin, tap) set to zero.  rel_err < 1e-2 (tests/test_hip_parity.py) and the
    shadow's bound (err / bound <= 1) both accept the defective output; the exact comparator does not."""
    case = X.c3("gap", "gather", 1, 640, 0, 32, (4, 4, 4), out_f32=True)
    inp = X.build_inputs(case, "D")
    ref = X.reference(case, inp)
    bad = X.build_inputs(case, "D")
    bad.w[5, 333, 13] = 0                                            # centre tap: every output position loses one product
    y_bad = X.reference(case, bad)
    call = X.conv_call(case, inp)
    out = kernel_like(call, y_bad, torch.float32)
    assert int((y_bad != ref).sum()) == 64
    e = rel_err(out[..., :32], ref)
    ratio = SH.conv_ratio(call, out)[0]
    print(f"single dropped product: rel_err {e:.2e} (limit 1e-2), shadow err / bound {ratio:.3f} (limit 1)")
    assert 0 < e < 1e-2 and 0 < ratio <= 1.0
    with pytest.raises(AssertionError, match="64 of"):
        X.check_output(out, ref, "D")
    X.check_output(kernel_like(call, ref, torch.float32), ref, "D")
