"""The criterion of the exhaustive activation sweeps (tests/act_sweep.py), tested on the CPU: the kernels' formulas restated with torch
fp32 ops pass it, the known-lossy 1 + erf form of GELU passes it only with its derived allowance, every planted wrong variant is
rejected, and the sizes of the sets the criterion exempts are pinned.  No GPU.

Figures printed by this module with torch fp64 / fp32 on the CPU (the assertions are the issue's, the counts are for the reader):
  SiLU  y * (1 / (1 + exp(-y)))        0 fail, worst 0.500 ulp, 0 outputs != RN_bf16(r); the same for gg_silu's halved arrangement
        ... with v_rcp_f32's flush      1 fail: x = -87.5 (the defect the GPU sweep found in the plain form)
  GELU  0.5 y erfc(-y / sqrt 2)        0 fail, worst 0.500 ulp, 0 outputs != RN_bf16(r)
  GELU  0.5 y (1 + erf(y / sqrt 2))    allow=None: 180 fail, x in [-12.81, -4.69]; with |x| * 2^-22: 0 fail
"""
import math

import pytest
import torch

import act_sweep as A

torch.set_grad_enabled(False)


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def _x32():
    return A.all_finite_bf16().float()


def _bf(y32):
    """what a kernel stores: the fp32 result rounded to bf16"""
    return y32.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ the inputs and the exempt sets
def test_all_finite_bf16_is_every_finite_value_once():
    x = A.all_finite_bf16()
    assert x.dtype == torch.bfloat16 and x.numel() == A.N_FINITE == 65280
    bits = x.view(torch.int16).int() & 0xFFFF
    assert bool((bits[1:] > bits[:-1]).all()), "fixed order: ascending bit pattern"
    assert bits[0] == 0 and bool((bits == 0x8000).any()), "both zeros"
    assert int(((bits & 0x7F80) == 0).sum()) == 256, "2 zeros and 254 subnormals"
    assert not bool(((bits & 0x7F80) == 0x7F80).any()), "no Inf, no NaN"
    assert A.all_finite_bf16() is x


def test_ulp_and_rounding_helpers():
    r = torch.tensor([1.0, 1.5, -3.0, 2.0 ** -126, 2.0 ** -140, 0.0], dtype=torch.float64)
    assert A.ulp_bf16(r).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133, 2.0 ** -133, 2.0 ** -133]
    assert A.ulp_f32(r).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -149, 2.0 ** -149, 2.0 ** -149]
    mid = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 0.04 * 2.0 ** -7, 1.0 + 2.0 ** -8 + 0.06 * 2.0 ** -7, 1.0], dtype=torch.float64)
    m = A.midpoint_margin(mid)
    assert abs(float(m[0])) < 1e-9 and abs(float(m[1]) - 0.04) < 1e-9 and abs(float(m[2]) - 0.06) < 1e-9 and float(m[3]) == 0.5
    near, floor = A.reference_sets(torch.cat([mid, torch.tensor([2.0 ** -120, 2.0 ** -119, 0.0], dtype=torch.float64)]))
    assert near.tolist() == [True, True, False, False, False, False, False] and floor.tolist() == [False] * 4 + [True, False, True]


@pytest.mark.parametrize("name, n_near, n_floor", [("silu", 362, 17618), ("gelu", 337, 17972)])
def test_exempt_set_sizes(name, n_near, n_floor):
    """The inputs conditions 2 / 3 go easy on are properties of the fp64 references alone; their sizes are pinned."""
    x, s64, g64 = A.references()
    near, floor = A.reference_sets(s64 if name == "silu" else g64)
    print(f"{name}: {int(near.sum())} inputs within {A.SILU_MARGIN} bf16 ulp of a midpoint, {int(floor.sum())} with |r| <= 2^-120")
    assert int(near.sum()) == n_near and int(floor.sum()) == n_floor
    assert not bool((near & floor).any())
    if name == "silu":
        # x < -88.7: fp32 exp(-x) overflows, an fp32 SiLU returns 0 where fp64 has a bf16-normal number; FLOOR covers exactly these
        deep = (x.double() < -88.7) & (s64.abs() >= 2.0 ** -126)
        assert int(deep.sum()) == 6 and float(s64[deep].abs().max()) < A.FLOOR and abs(float(s64[deep].abs().max()) - 1.98e-37) < 1e-39


def test_host_predicates_place_every_conv_site_on_its_kernel():
    """The path assertion of the GPU module on the descriptors of the swept convs with a SiLU prologue (host code only; the team
    kernel's dry run asks the device for its CU count, so path_hint 7 is left to the GPU module)."""
    import conv_exact as X
    from jointimagegeneration_amd import _lib
    lib = _lib.load()
    sites = A.conv_sites()
    assert set(sites) == {"gather", "gather5", "halo", "team", "box"}
    for path, case in sites.items():
        if path == "team":
            continue
        for out_f32 in (False, True):
            for hint in ((1, 4, 6) if case.hint is None else (case.hint,)):
                d = X.case_desc(case, "D", hint)
                d.prologue_act, d.out_dtype = 1, 1 if out_f32 else 0
                X.assert_path(lib, d, case)
    g5 = sites["gather5"]
    assert (g5.out_sp[0] * g5.out_sp[1] * g5.out_sp[2]) % 64 == 0, "the 160-step kernel takes a prologue only then"
    for case, e in A.spec_silu_sites():
        assert e["prologue_act"] == 1 and not e["pro_acc"] and case.cout >= case.C1 and case.path == "spec"


# ------------------------------------------------------------------------------------------------ what the kernels compute passes
def test_fp32_silu_restatement_passes():
    """The plain fp32 formula y * (1 / (1 + exp(-y))) with IEEE ops (gg_silu's own arrangement: test_fp32_silu_halved_restatement_passes)."""
    x, s64, _ = A.references()
    y = _x32()
    got = _bf(y * (_f32(1.0) / (_f32(1.0) + torch.exp(-y))))
    st = A.check(got, x, s64)
    print(f"fp32 SiLU restatement: worst {st['worst_ulp']:.3f} ulp, {st['not_rn']} outputs != RN_bf16(r)")
    assert st["worst_ulp"] <= 0.5 + 1e-3 and st["not_rn"] == 0


def _flushed(rcp):
    return torch.where(rcp.abs() < 2.0 ** -126, torch.zeros_like(rcp), rcp)              # v_rcp_f32 returns 0 for a subnormal result


def test_fp32_silu_halved_restatement_passes():
    """gg_silu as written, (y / 2) * rcp(fma(exp(-y), 1/2, 1/2)): the reciprocal of a denominator above 2^126 is subnormal, and
    v_rcp_f32 returns 0 for it; the halves keep it normal wherever the reference is above FLOOR, and change no other result: with the
    same flush, the halved and the plain arrangement agree bit for bit at every input but x = -87.5 and -88.0, where the plain one returns 0;
    -87.5 is above FLOOR and misses check (what the sweep measured on an MI355X at every bf16 SiLU site before the halves)."""
    x, s64, _ = A.references()
    y = _x32()
    e = torch.exp(-y)
    half_d = (e.double() * 0.5 + 0.5).float()                                          # fma: exact in fp64, one rounding
    halved = (_f32(0.5) * y) * _flushed(_f32(1.0) / half_d)
    st = A.check(_bf(halved), x, s64)
    print(f"fp32 SiLU, halved: worst {st['worst_ulp']:.3f} ulp, {st['not_rn']} outputs != RN_bf16(r)")
    assert st["worst_ulp"] <= 0.5 + 1e-3 and st["not_rn"] == 0
    rcp = _flushed(_f32(1.0) / (_f32(1.0) + e))
    differ = (halved.view(torch.int32) != (y * rcp).view(torch.int32)) & (y.abs() >= 2.0 ** -125)
    assert x.double()[differ].tolist() == [-87.5, -88.0]          # (-88.0: 5.3e-37, under FLOOR; from -88.5 on both flush)
    st = A.measure(_bf(y * rcp), x, s64)
    assert st["fail"] == 1 and st["bad_x"] == [-87.5]
    with pytest.raises(AssertionError):
        A.check(_bf(y * rcp), x, s64)


def test_fp32_silu_ieee_division_passes_check_f32():
    """v / (1 + expf(-v)) of gg_linear_f32 / gg_f32.hip against the 4-ulp criterion, and after rounding against the bf16 one."""
    x, s64, _ = A.references()
    y = _x32()
    got = y / (_f32(1.0) + torch.exp(-y))
    st = A.check_f32(got, x, s64)
    print(f"fp32 SiLU, IEEE division: worst {st['worst_ulp']:.3f} fp32 ulp")
    A.check(_bf(got), x, s64)


def test_fp32_gelu_erfc_restatement_passes():
    x, _, g64 = A.references()
    y = _x32()
    got = _bf(_f32(0.5) * y * torch.special.erfc(-y * _f32(A.SQRT1_2)))
    st = A.check(got, x, g64)
    print(f"fp32 erfc GELU restatement: worst {st['worst_ulp']:.3f} ulp, {st['not_rn']} outputs != RN_bf16(r)")
    assert st["worst_ulp"] <= 0.5 + 1e-3 and st["not_rn"] == 0


def _gelu_1p_erf(y):
    return _f32(0.5) * y * (_f32(1.0) + torch.erf(y * _f32(A.SQRT1_2)))


def test_fp32_gelu_one_plus_erf_needs_its_allowance():
    """The 1 + erf form (gg_geglu, the GEGLU epilogue, ATen's fp32 F.gelu) cancels in the left tail: rejected without an allowance,
    every failure in the tail; accepted with |x| * 2^-22 (act_sweep.geglu_allow)."""
    x, _, g64 = A.references()
    got = _bf(_gelu_1p_erf(_x32()))
    st = A.measure(got, x, g64)
    ulp = A.ulp_bf16(g64)
    bad = ((got.double() - g64).abs() > ulp) & ((got.double() - g64).abs() > A.FLOOR)
    xs = x.double()[bad]
    print(f"fp32 1 + erf GELU, no allowance: {st['fail']} fail, x in [{float(xs.min()):.2f}, {float(xs.max()):.2f}], worst {st['worst_ulp']:.1f} ulp")
    assert st["nonfinite"] == 0 and st["fail"] == int(bad.sum()) > 0
    assert float(xs.min()) > -13.0 and float(xs.max()) <= -4.0       # the tail only; below -12.9 the reference is under FLOOR
    with pytest.raises(AssertionError):
        A.check(got, x, g64)
    A.check(got, x, g64, allow=A.geglu_allow(x))
    assert float(A.geglu_allow(x)[x.double().abs() <= 12].max()) < 3e-6
    for value in (1.0, -1.5):           # the two legs of the gg_geglu sweep: value * gelu(gate), the product rounded once
        A.check(_bf(_f32(value) * _gelu_1p_erf(_x32())), x, value * g64, allow=A.geglu_allow(x, value))
    # -1.5 * gelu(x) leaves bf16's range at the 85 largest x: there, and only there, check wants the Inf itself
    over = torch.isinf(A.rn_bf16(-1.5 * g64))
    assert int(over.sum()) == 85 and float(x.double()[over].min()) > 2.2e38 and not bool(torch.isinf(A.rn_bf16(g64)).any())
    wrong = _bf(_f32(-1.5) * _gelu_1p_erf(_x32()))
    wrong[over] = -3.3895e38                                       # saturating instead of overflowing is an error there
    with pytest.raises(AssertionError):
        A.check(wrong, x, -1.5 * g64, allow=A.geglu_allow(x, -1.5))


# ------------------------------------------------------------------------------------------------ planted wrong variants are rejected
def _silu_exp2_truncated(y):
    return y * (_f32(1.0) / (_f32(1.0) + torch.exp2(-y * _f32(1.4375))))            # log2 e = 1.442695 truncated to 5 bits


def _silu_bf16_exp(y):
    e = torch.exp((-y).to(torch.bfloat16).float()).to(torch.bfloat16).float()          # argument and result of exp rounded to bf16
    return y * (_f32(1.0) / (_f32(1.0) + e))


def _silu_tanh(y):
    return _f32(0.5) * y * (_f32(1.0) + torch.tanh(y * _f32(0.5)))


def _silu_exp_pos(y):
    e = torch.exp(y)
    return y * e / (_f32(1.0) + e)                                                    # e^y overflows: Inf / Inf


def _hard_swish(y):
    return y * torch.clamp(y + _f32(3.0), 0.0, 6.0) / _f32(6.0)


def _gelu_tanh(y):
    return _f32(0.5) * y * (_f32(1.0) + torch.tanh(_f32(math.sqrt(2.0 / math.pi)) * (y + _f32(0.044715) * y * y * y)))


def _gelu_sigmoid(y):
    return y * torch.sigmoid(_f32(1.702) * y)


@pytest.mark.parametrize("variant, key", [(_silu_exp2_truncated, "fail"), (_silu_bf16_exp, "fail_rn"), (_silu_tanh, "fail"),
                                          (_silu_exp_pos, "nonfinite"), (_hard_swish, "fail")],
                         ids=["exp2_truncated_log2e", "bf16_exp", "tanh_form", "exp_of_plus_y", "hard_swish"])
def test_planted_silu_variants_are_rejected(variant, key):
    """Plausible rewrites of the SiLU staging line; `key` names the condition that does most of the work against the variant."""
    x, s64, _ = A.references()
    got = _bf(variant(_x32()))
    st = A.measure(got, x, s64)
    print(f"{variant.__name__}: {st['nonfinite']} non-finite, {st['fail']} beyond 1 ulp, {st['fail_rn']} not correctly rounded away from midpoints, worst {st['worst_ulp']:.2f} ulp")
    assert st[key] > 0
    with pytest.raises(AssertionError):
        A.check(got, x, s64)


@pytest.mark.parametrize("variant", [_gelu_tanh, _gelu_sigmoid], ids=["tanh_approximation", "sigmoid_1702"])
def test_planted_gelu_variants_are_rejected_under_the_geglu_allowance(variant):
    x, _, g64 = A.references()
    got = _bf(variant(_x32()))
    st = A.measure(got, x, g64, allow=A.geglu_allow(x))
    print(f"{variant.__name__}: {st['fail']} beyond 1 ulp + allowance, {st['fail_rn']} not correctly rounded away from midpoints, worst {st['worst_ulp']:.2f} ulp")
    assert st["fail"] > 0
    with pytest.raises(AssertionError):
        A.check(got, x, g64, allow=A.geglu_allow(x))


def test_check_f32_rejects_a_bf16_grade_result():
    x, s64, _ = A.references()
    with pytest.raises(AssertionError):
        A.check_f32(_silu_tanh(_x32()), x, s64)
    with pytest.raises(AssertionError):
        A.check_f32(torch.full((A.N_FINITE,), math.nan), x, s64)
