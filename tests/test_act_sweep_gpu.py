"""GPU suite (-m gpu): every finite bf16 value through every SiLU and GELU site of the kernels, against fp64 (tests/act_sweep.py: the
65280 inputs, the references, check / check_f32; tests/test_act_sweep_cpu.py tests that criterion).

Each test arranges the 65280 values so that the site's output is round(act(x)) and nothing else:
  SiLU, bf16 storage   identity tables (scale 1, shift 0 on logical channels: y = x exactly, whatever the contraction of the affine)
                       into gg_groupnorm_apply and gg_resample2x (gn_affine -> gg_silu);
  SiLU, conv staging   the same tables as ops.conv's prologue with prologue_silu=True, and a weight that is 1 on the centre tap of
                       the diagonal: one product per output is non-zero, every other term an exact zero, so the output IS the staged
                       bf16 value, in bf16 or fp32 output alike.  Paths gather, gather5 (160-step), halo, team, box and spec, each
                       proven on the captured descriptor (conv_exact.assert_path) as tests/test_conv_exact_gpu.py does.  The gather
                       kernels take the prologue when a caller passes one (their PRO instantiations), although
                       gg_conv_fuses_prologue advises against it: that is the C API surface under test.  The tiny-M kernel is not
                       swept: it takes no prologue and has no SiLU site;
  SiLU, fp32           gg_linear_f32 with W = I and act_in (v / (1 + expf(-v))), held to check_f32;
  GELU                 gg_gelu (erfc form, no allowance), gg_geglu and the GEGLU epilogue of the 1x1 conv (1 + erf form, allowance
                       |value| |x| 2^-22: act_sweep.geglu_allow).
Not swept, so that nobody assumes coverage: the SiLU of gn_f32_apply / gn_f32_apply_film (their statistics cannot be made the identity
without the norm_exact machinery), the softplus of gg_patchgan.hip (visible only through a reduction) and the accumulator-prologue
variant of the box kernel (it shares the SiLU site swept here).

Every test prints, per site, the worst error in bf16 ulps, the number of outputs different from RN_bf16(r) and the number different
from the groupnorm_apply site's outputs (GELU sites: from gg_gelu's); only what check implies is asserted about the last two.
"""
import pytest
import torch

import act_sweep as A
import conv_exact as X

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

N_VAL = A.N_FINITE
ROWS, CH = 1020, 64                     # 1020 x 64 = 65280
_BASE = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _tables(dev, n, cpad, c_log):
    """identity affine on the logical channels, zero rows on the pad lanes"""
    scale = torch.zeros(n, cpad, dtype=torch.float32, device=dev)
    scale[:, :c_log] = 1.0
    return scale, torch.zeros(n, cpad, dtype=torch.float32, device=dev)


def _rows(dev, sp, cpad, dtype=torch.bfloat16):
    """channels-last [1, *sp, cpad] holding the sweep on its 64 logical channels (1020 positions), zero pad lanes"""
    t = torch.zeros((1,) + tuple(sp) + (cpad,), dtype=dtype, device=dev)
    t[..., :CH] = A.all_finite_bf16().to(dev).to(dtype).view((1,) + tuple(sp) + (CH,))
    return t


def _silu_base(dev):
    """bf16 [65280] on the CPU: what gg_groupnorm_apply makes of the sweep (the site every other SiLU site is counted against)"""
    if "silu" not in _BASE:
        from jointimagegeneration_amd import ops
        src = ops.CL(_rows(dev, (1, 1, ROWS), 96), CH)
        out = ops.groupnorm_apply(src, *_tables(dev, 1, 96, CH), act=True)
        torch.cuda.synchronize()
        assert out.C == CH and tuple(out.t.shape) == (1, 1, 1, ROWS, 96) and out.t.dtype == torch.bfloat16
        assert not bool(out.t[..., CH:].ne(0).any()), "pad lanes must come out zero"
        _BASE["silu"] = out.t[..., :CH].reshape(-1).cpu()
    return _BASE["silu"]


def _gelu_base(dev):
    if "gelu" not in _BASE:
        from jointimagegeneration_amd import ops
        out = ops.gelu(A.all_finite_bf16().to(dev))
        torch.cuda.synchronize()
        _BASE["gelu"] = out.cpu()
    return _BASE["gelu"]


def _report(site, st, got, base):
    """the three figures of a site; base None: the site computes another function than the base site (value * gelu, value != 1)"""
    diff = "n/a" if base is None else int((got.reshape(-1)[:N_VAL].cpu().double() != base.double()).sum())
    print(f"{site}: worst {st['worst_ulp']:.3f} bf16 ulp, {st['not_rn']} outputs != RN_bf16(r), {diff} != base site")


# ------------------------------------------------------------------------------------------------ SiLU, bf16 storage
def test_silu_groupnorm_apply(dev):
    """gg_groupnorm_apply, N = 1, S = 1020, 64 logical channels of 96 (gn_affine8 -> gg_silu); pad lanes come out zero.
    Measured on an MI355X: worst 0.500 bf16 ulp, 1 output != RN_bf16(r) (a near-midpoint input), 0 != base site (this is the base)."""
    x, s64, _ = A.references()
    got = _silu_base(dev)
    st = A.check(got, x, s64)
    _report("groupnorm_apply", st, got, got)


def test_silu_resample2x(dev):
    """gg_resample2x, nearest x2 with the prologue: all four copies equal the groupnorm_apply result element for element; a second leg
    with fp32 storage (ops.fp32_validation()) is held to check after rounding its output to bf16.
    Measured on an MI355X, both legs: worst 0.500 bf16 ulp, 1 output != RN_bf16(r), 0 != base site."""
    from jointimagegeneration_amd import ops
    x, s64, _ = A.references()
    base = _silu_base(dev)
    H, W = 30, 34
    up = ops.resample2x(ops.CL(_rows(dev, (1, H, W), 96), CH), True, False, prologue=_tables(dev, 1, 96, CH), act=True)
    torch.cuda.synchronize()
    assert tuple(up.t.shape) == (1, 1, 2 * H, 2 * W, 96) and up.t.dtype == torch.bfloat16 and not bool(up.t[..., CH:].ne(0).any())
    copies = up.t[..., :CH].reshape(H, 2, W, 2, CH).permute(1, 3, 0, 2, 4).reshape(4, -1).cpu()
    st = A.check(copies[0], x, s64)
    _report("resample2x bf16", st, copies[0], base)
    for c in range(4):
        assert torch.equal(copies[c].view(torch.int16), base.view(torch.int16)), f"copy {c} differs from the groupnorm_apply result"
    with ops.fp32_validation():
        up32 = ops.resample2x(ops.CL(_rows(dev, (1, H, W), 96, torch.float32), CH), True, False, prologue=_tables(dev, 1, 96, CH), act=True)
    torch.cuda.synchronize()
    assert up32.t.dtype == torch.float32 and not bool(up32.t[..., CH:].ne(0).any())
    c32 = up32.t[..., :CH].reshape(H, 2, W, 2, CH).permute(1, 3, 0, 2, 4).reshape(4, -1).cpu()
    for c in range(4):
        assert torch.equal(c32[c], c32[0])
    got = c32[0].to(torch.bfloat16)
    st = A.check(got, x, s64)
    _report("resample2x fp32 storage", st, got, base)


# ------------------------------------------------------------------------------------------------ SiLU in the conv staging paths
def _conv_site(dev, case, monkeypatch, out_f32, site):
    """The sweep through the SiLU of the staging pass of `case`'s kernel: identity prologue tables, identity weight on the centre tap, as
    many launches as the 65280 values need (the values repeat to fill the last one); every launch's descriptor must name the path."""
    from jointimagegeneration_amd import _lib, ops
    if case.hint is not None:
        monkeypatch.setattr(ops, "PATH_HINT", case.hint)
    x, s64, _ = A.references()
    cin, cout, taps = case.C1, case.cout, case.taps
    per = case.N * case.sp[0] * case.sp[1] * case.sp[2] * cin
    launches = -(-N_VAL // per)
    idx = torch.arange(launches * per) % N_VAL
    xs, ref = x[idx], s64[idx]
    w = torch.zeros(cout, cin, taps)
    w[torch.arange(cin), torch.arange(cin), taps // 2] = 1.0
    pw = ops.pack_conv_weight(w.view((cout, cin) + case.k).to(dev), cin)
    tables = _tables(dev, case.N, cin, cin)
    bias = torch.zeros(ops.pad32(cout), device=dev) if case.bias != "none" and case.path == "spec" else None
    lib = _lib.load()
    got = []
    for i in range(launches):
        src = ops.CL(xs[i * per:(i + 1) * per].view((case.N,) + case.sp + (cin,)).to(dev), cin)
        res = ops.CL(torch.zeros((case.N,) + case.out_sp + (ops.pad32(cout),), dtype=torch.bfloat16, device=dev), cout) if case.residual else None
        sink = []
        if case.stats:
            ops.stats_begin(dev)
        try:
            with X.captured_descs(sink):
                y = ops.conv(src, pw, bias, cout, k=case.k, stride=1, pad=case.pad, residual=res, out_f32=out_f32, prologue=tables,
                             prologue_silu=True, want_stats=case.stats)
        finally:
            if case.stats:
                ops.stats_end(dev)
        torch.cuda.synchronize()
        assert len(sink) == 1 and sink[0].prologue_act == 1 and not sink[0].pro_acc1
        X.assert_path(lib, sink[0], case)
        assert y.t.dtype == (torch.float32 if out_f32 else torch.bfloat16) and tuple(y.t.shape[:-1]) == (case.N,) + tuple(case.out_sp)
        assert not bool(y.t[..., cin:].ne(0).any()), "output channels without a weight must be zero"
        got.append(y.t[..., :cin].reshape(-1).cpu())
    got = torch.cat(got)
    if out_f32:
        assert torch.equal(got, got.to(torch.bfloat16).float()), "fp32 output of a single bf16 product must be a bf16 value"
    A.check(got, xs, ref)                                                 # every launch in full, the repeated values included
    st = A.measure(got[:N_VAL], x, s64)                                   # the figures: each value once
    _report(site, st, got, _silu_base(dev))
    return st


_OUT = pytest.mark.parametrize("out_f32", [False, True], ids=["bf16", "f32"])


@_OUT
def test_silu_conv_gather(dev, monkeypatch, out_f32):
    """conv_gather_kernel<NT, PF, 1>, write_lds: g3d_same (64 -> 96 at 5x6x7), 5 launches.
    Measured on an MI355X, bf16 and fp32 output: worst 0.500 bf16 ulp, 1 output != RN_bf16(r), 0 != base site."""
    _conv_site(dev, A.conv_sites()["gather"], monkeypatch, out_f32, "conv gather")


@_OUT
def test_silu_conv_gather5(dev, monkeypatch, out_f32):
    """conv_gather5_kernel<1>, the 160-step staging: 160 -> 160 at (64, 9), one launch (split-K slabs: every partial sum is exact).
    Measured on an MI355X, bf16 and fp32 output: worst 0.500 bf16 ulp, 1 output != RN_bf16(r), 0 != base site."""
    _conv_site(dev, A.conv_sites()["gather5"], monkeypatch, out_f32, "conv gather5")


@_OUT
def test_silu_conv_halo(dev, monkeypatch, out_f32, halo_hint):
    """conv_halo_kernel's box staging with 512-, 256- and 1024-position boxes: h3d_nt2 (64 -> 64 at 8x8x32), one launch.
    Measured on an MI355X, all three boxes, bf16 and fp32 output: worst 0.500 bf16 ulp, 1 output != RN_bf16(r), 0 != base site."""
    _conv_site(dev, A.conv_sites()["halo"], monkeypatch, out_f32, "conv halo")


def test_silu_conv_team(dev, monkeypatch):
    """gg_conv_halo3.hip (path_hint 7; bf16 output only): team_one_item (64 -> 64 at 8x8x16), one launch.
    Measured on an MI355X: worst 0.500 bf16 ulp, 1 output != RN_bf16(r), 0 != base site."""
    _conv_site(dev, A.conv_sites()["team"], monkeypatch, False, "conv team")


@_OUT
def test_silu_conv_box_generic(dev, monkeypatch, out_f32):
    """gg_conv_box_kernel.h, the in-place prologue of the generic instantiation (path_hint 10): box_th2 (160 -> 160 at 16x16), 2 launches.
    Measured on an MI355X, bf16 and fp32 output: worst 0.500 bf16 ulp, 1 output != RN_bf16(r), 0 != base site."""
    _conv_site(dev, A.conv_sites()["box"], monkeypatch, out_f32, "conv box")


def test_silu_conv_box_shape_specialised(dev, monkeypatch):
    """gg_conv_box_kernel.h compiled for an entry of gg_conv_box_specs.inc (path_hint 11).  Every entry of today's table that has a
    prologue takes it from accumulators (pro_acc = 1: the variant named out of scope above, which shares the SiLU line swept by
    test_silu_conv_box_generic); an entry with an external-table SiLU prologue is swept as soon as the table has one."""
    sites = A.spec_silu_sites()
    if not sites:
        pytest.skip("gg_conv_box_specs.inc has no entry with an external-table SiLU prologue (prologue_act 1, pro_acc 0): no such kernel is compiled")
    for case, e in sites:
        _conv_site(dev, case, monkeypatch, case.out_f32, f"conv spec {case.name}")


# ------------------------------------------------------------------------------------------------ SiLU, fp32
def test_silu_linear_f32(dev):
    """gg_linear_f32 with act_in: v / (1 + expf(-v)), IEEE division; W = I_64, so out = SiLU(x) plus exact zeros.
    Measured on an MI355X: worst 1.754 fp32 ulp; rounded to bf16, 0 outputs != RN_bf16(r) and 2 != base site."""
    from jointimagegeneration_amd import ops
    x, s64, _ = A.references()
    got = ops.linear_f32(x.float().view(ROWS, CH).to(dev), torch.eye(CH, device=dev), None, act_in=True)
    torch.cuda.synchronize()
    got = got.reshape(-1).cpu()
    st = A.check_f32(got, x, s64)
    b = got.to(torch.bfloat16)
    print(f"linear_f32: worst {st['worst_ulp']:.3f} fp32 ulp; rounded to bf16: {int((b.double() != A.rn_bf16(s64))[s64.abs() > A.FLOOR].sum())} outputs != RN_bf16(r), "
          f"{int((b.double() != _silu_base(dev).double()).sum())} != base site")


# ------------------------------------------------------------------------------------------------ GELU
def _tail_ulps(got, x, ref):
    """largest |got - ref| in bf16 ulps over x in [-12, -4]"""
    m = (x.double() >= -12) & (x.double() <= -4)
    return float(((got.double() - ref).abs() / A.ulp_bf16(ref))[m].max())


def test_gelu_all_values(dev):
    """gg_gelu (gelu_erf: the erfc form), all 65280 values in one call, no allowance.
    Measured on an MI355X: worst 0.500 bf16 ulp, 0 outputs != RN_bf16(r), 0 != base site (this is the GELU base)."""
    x, _, g64 = A.references()
    got = _gelu_base(dev)
    st = A.check(got, x, g64)
    _report("gelu", st, got, got)


@pytest.mark.parametrize("value", [1.0, -1.5])
def test_geglu_gate_sweep(dev, value):
    """gg_geglu: h [1020, 128], the gate half is the sweep, the value half a constant; reference value * gelu64(gate).
    Measured on an MI355X.  value 1: inside the allowance; without it 180 outputs are beyond 1 ulp (163 not correctly rounded away from
    midpoints), all in the left tail, where 1 + erf cancels to 0: the largest deviation over x in [-12, -4] is 254.9 bf16 ulp (an
    output of 0 for a reference that is a normal bf16 number); 186 outputs != RN_bf16(r), 197 != gg_gelu's.  value -1.5: 182 / 167
    without the allowance, 255.9 bf16 ulp in the tail, 212 outputs != RN_bf16(r).  Both legs stay inside |value| |x| 2^-22, so the kernel keeps
    the form of ATen's fp32 F.gelu; the tail deviation is the known cost of that form."""
    from jointimagegeneration_amd import ops
    x, _, g64 = A.references()
    h = torch.full((ROWS, 2 * CH), value, dtype=torch.bfloat16, device=dev)
    h[:, CH:] = x.to(dev).view(ROWS, CH)
    out = ops.geglu(h, CH)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (ROWS, CH) and out.dtype == torch.bfloat16
    got, ref = out.reshape(-1).cpu(), value * g64
    free = A.measure(got, x, ref)
    print(f"geglu value {value}: without the allowance {free['fail']} outputs beyond 1 ulp, {free['fail_rn']} not correctly rounded away from midpoints; "
          f"largest deviation over x in [-12, -4]: {_tail_ulps(got, x, ref):.1f} bf16 ulp")
    st = A.check(got, x, ref, allow=A.geglu_allow(x, value))
    _report(f"geglu value {value}", st, got, _gelu_base(dev) if value == 1.0 else None)


def test_geglu_conv_epilogue(dev):
    """The GEGLU epilogue of the 1x1 conv (gg_conv_desc.epilogue_geglu): Linear(64, 128) whose value rows have zero weight and bias 1 and
    whose gate rows are the identity with bias 0, tokens (1, 1, 1020): the output is bf16(1 * gelu(x)).
    Measured on an MI355X: as gg_geglu at value 1, output for output -- inside the allowance; without it 180 beyond 1 ulp (163 not
    correctly rounded away from midpoints), 254.9 bf16 ulp over x in [-12, -4], 186 outputs != RN_bf16(r), 197 != gg_gelu's."""
    from jointimagegeneration_amd import blocks, ops
    x, _, g64 = A.references()
    proj = torch.nn.Linear(CH, 2 * CH)
    proj.weight.zero_(); proj.bias.zero_()
    proj.weight[CH:] = torch.eye(CH)
    proj.bias[:CH] = 1.0
    proj = proj.to(dev)
    pw, pb = blocks.packed_geglu(proj, CH)
    sink = []
    with X.captured_descs(sink):
        y = ops.conv(ops.CL(x.to(dev).view(1, 1, 1, ROWS, CH), CH), pw, pb, 2 * CH, k=(1, 1, 1), pad=0, geglu=True)
    torch.cuda.synchronize()
    assert len(sink) == 1 and sink[0].epilogue_geglu == 1
    assert y.C == CH and tuple(y.t.shape) == (1, 1, 1, ROWS, CH) and y.t.dtype == torch.bfloat16
    got = y.t.reshape(-1).cpu()
    free = A.measure(got, x, g64)
    print(f"geglu epilogue: without the allowance {free['fail']} outputs beyond 1 ulp, {free['fail_rn']} not correctly rounded away from midpoints; "
          f"largest deviation over x in [-12, -4]: {_tail_ulps(got, x, g64):.1f} bf16 ulp")
    st = A.check(got, x, g64, allow=A.geglu_allow(x))
    _report("geglu epilogue", st, got, _gelu_base(dev))
