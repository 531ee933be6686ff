"""GPU suite (-m gpu): every conv kernel path bit for bit against the fp64 reference (tests/conv_exact.py: the regimes, the
preconditions and the comparators; tests/shadow.py: conv_reference).  There is no tolerance in this module.

Kernel paths covered, and the host predicate, asked about the descriptor of the launch itself, that proves the path was taken
(conv_exact.kernel_path / assert_path):
  gather / 160-step gather   not halo (gg_conv_runs_halo_tile == 0), not box, M > 128; 160-step: both sources multiples of 160 channels
  split-K                    gg_conv_workspace_bytes > 0 on a gather / 160-step / tiny-M descriptor
  tiny-M (gg_conv_tiny.hip)  not halo, not box, M <= 128 and no prologue
  halo-tile                  gg_conv_runs_halo_tile == 1 under path_hint 1 / 4 / 6 (the halo_hint fixture); regime S: 32-stripe accumulators
  team (gg_conv_halo3.hip)   gg_conv_runs_halo_tile == 1 under path_hint 7 on a descriptor inside gg_conv_halo3_try's envelope
  box, generic               not halo and plan_box accepts (gg_conv_fuses_ddim on the descriptor as a 4-channel fp32 head), path_hint 10
                             (or N > 1), so that the shape table is not consulted; gg_conv_fuses_skip for the K-concatenated skip
  box, shape-specialised     path_hint 11: a launch whose shape, plan and flags match no entry of gg_conv_box_specs.inc is an error
  fp32 validation conv       fp32 tensors inside ops.fp32_validation(): ops.conv calls gg_conv_forward_f32 only
plus the layout movers, labels_to_onehot, resample2x, add and linear_f32 on inputs where they, too, are exact.

The fp64 references are computed on the device, once per (case, regime), and shared by the tests that need them.
"""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import conv_exact as X

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

_CACHE = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def prepared(case, regime, dev):
    """(device inputs, fp64 reference) of a case, built and checked once"""
    key = (case.name, regime)
    if key not in _CACHE:
        inp = X.build_inputs(case, regime).to(dev)
        ref = X.reference(case, inp)
        X.check_reference(regime, ref)
        _CACHE[key] = (inp, ref)
    return _CACHE[key]


def launch(case, regime, inp, monkeypatch):
    """ops.conv of the case -> (CL result, descriptor of the launch or None for the fp32 validation conv)"""
    from jointimagegeneration_amd import ops
    if case.hint is not None:
        monkeypatch.setattr(ops, "PATH_HINT", case.hint)
    f32 = case.path == "f32"
    dev = inp.w.device
    with (ops.fp32_validation() if f32 else contextlib.nullcontext()):
        srcs = [ops.CL(t, c) for t, c in zip(inp.srcs, (case.C1, case.C2))]
        pw = ops.pack_conv_weight(inp.w.view((case.cout, case.cin_w) + case.k), sum(s.Cpad for s in srcs))
        skip = None
        if case.skip:
            sk = [ops.CL(t, c) for t, c in zip(inp.skip_srcs, case.skip)]
            pws = ops.pack_conv_weight(inp.skip_w.view(case.cout, sum(case.skip), 1, 1), sum(s.Cpad for s in sk))
            assert ops.conv_fuses_skip(srcs[0], case.cout, sk[0], sk[1] if len(sk) > 1 else None, k=case.k)
            skip = (sk[0], sk[1] if len(sk) > 1 else None, pws)
        if regime == "P":
            assert ops.conv_fuses_prologue(srcs[0], case.cout, k=case.k, src2=srcs[1] if len(srcs) > 1 else None)
        want_stats = (regime == "S" or case.stats) and not case.out_f32
        sink = []
        if want_stats:
            ops.stats_begin(dev)
        try:
            with X.captured_descs(sink):
                y = ops.conv(srcs[0], pw, inp.bias, case.cout, k=case.k, stride=case.stride, pad=case.pad, upsample=case.up,
                             src2=srcs[1] if len(srcs) > 1 else None, residual=ops.CL(inp.residual, case.cout) if inp.residual is not None else None,
                             out_f32=case.out_f32, bias_per_sample=case.bias == "per_sample", prologue=inp.prologue, prologue_silu=False,
                             want_stats=want_stats, skip=skip)
        finally:
            if want_stats:
                ops.stats_end(dev)
        torch.cuda.synchronize()
    if f32:
        assert not sink and y.t.dtype == torch.float32 and all(s.t.dtype == torch.float32 for s in srcs)
        return y, None
    assert len(sink) == 1
    return y, sink[0]


def run_exact(case, regime, dev, monkeypatch):
    from jointimagegeneration_amd import _lib, ops
    inp, ref = prepared(case, regime, dev)
    y, d = launch(case, regime, inp, monkeypatch)
    if d is not None:
        lib = _lib.load()
        X.assert_path(lib, d, case)
        stripes = lib.gg_conv_emits_stats(X.C.byref(d))
        osp = case.out_sp
        leaves = (regime == "S" or case.stats) and not case.out_f32 and (stripes == 32 or (stripes and osp[0] * osp[1] * osp[2] * y.Cpad <= ops.GN_ACC_MAX_ELEMS))
        assert (y.acc is not None) == bool(leaves), f"{case.name}: accumulators expected {bool(leaves)} ({stripes} stripes)"
        if y.acc is not None:
            assert y.acc.shape[1] == stripes and (stripes == 32) == (case.path in ("halo", "team"))
    assert y.t.dtype == (torch.float32 if case.out_f32 else torch.bfloat16) and y.C == case.cout
    X.check_output(y.t, ref, regime)
    if regime == "S" and y.acc is not None:
        X.check_acc(y.acc, ref)
    return y


def _params(group):
    return pytest.mark.parametrize("cr", X.GROUPS[group], ids=X.case_id)


@_params("gather")
def test_gather_kernels_production_dispatch(dev, cr, monkeypatch):
    """Gather, 160-step gather and (where production sends the listed edge shape there) tiny-M / box kernels under path_hint 0."""
    run_exact(cr[0], cr[1], dev, monkeypatch)


@_params("splitk")
def test_splitk_slabs_and_reduce(dev, cr, monkeypatch):
    """Every split-K slab term, the bias and the residual of the reduce: a missing slab changes every output."""
    run_exact(cr[0], cr[1], dev, monkeypatch)


@_params("tiny")
def test_tiny_m_kernel(dev, cr, monkeypatch):
    run_exact(cr[0], cr[1], dev, monkeypatch)


@_params("halo")
def test_halo_tile_kernel(dev, cr, monkeypatch, halo_hint):
    """The halo-tile kernel with its 512-, 256- and 1024-position boxes; regime S also the 32-stripe GroupNorm accumulators."""
    y = run_exact(cr[0], cr[1], dev, monkeypatch)
    if cr[1] == "S" and not cr[0].out_f32:
        assert y.acc is not None and y.acc.shape[1] == 32


@_params("team")
def test_team_kernel(dev, cr, monkeypatch):
    """The hand-scheduled team kernel against arithmetic (test_team_halo_conv_bit_identical_to_halo_kernel compares it with its sibling)."""
    run_exact(cr[0], cr[1], dev, monkeypatch)


@_params("box")
def test_box_kernel_generic(dev, cr, monkeypatch):
    """Generic box kernel (the shape table is bypassed): tile widths 16 / 8 / 4, ragged row tiles, LDS stages, cout sub-split, upsample,
    stride 2, 1x1 with residual, the K-concatenated skip projection (`bias` carries the skip's bias) and the in-place affine prologue."""
    run_exact(cr[0], cr[1], dev, monkeypatch)


@_params("spec")
def test_box_kernel_shape_specialised(dev, cr, monkeypatch):
    """Every prologue-free, DDIM-free entry of gg_conv_box_specs.inc, its flags reproduced through ops.conv's arguments; path_hint 11
    turns a launch that matches no entry into an error."""
    run_exact(cr[0], cr[1], dev, monkeypatch)


def test_spec_cases_are_the_table():
    import re
    keys = X._gen_box_specs().table_keys()
    plain = [k for k in keys if re.fullmatch(r"GG_BOX_SPEC\((\d+, ){22}0, 0, (\d+, ){4}0, 0, 0\)", k)]
    assert len(X.SPEC_CASES) == len(plain) > 40
    assert any(c.up for c in X.SPEC_CASES) and any(c.stride == 2 for c in X.SPEC_CASES) and any(c.residual for c in X.SPEC_CASES)
    assert any(c.skip and c.skip[1] for c in X.SPEC_CASES) and any(c.stats for c in X.SPEC_CASES)


@_params("f32")
def test_fp32_validation_conv(dev, cr, monkeypatch):
    run_exact(cr[0], cr[1], dev, monkeypatch)


# ------------------------------------------------------------------------------------------------ small ops, exact as well
def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("C", [1, 2, 15, 33])
def test_to_cl_exact(dev, C):
    """NC[D]HW fp32 -> channels-last bf16 == x.bfloat16() permuted (values that do need rounding); zero_fill zeroes the rest,
    c_offset > 0 with zero_fill=False leaves every other channel of the buffer as it was, byte for byte."""
    from jointimagegeneration_amd import ops
    g = torch.Generator().manual_seed(C)
    x = torch.randn(2, C, 5, 7, generator=g).to(dev)                                  # S = 35
    want = x.bfloat16().permute(0, 2, 3, 1).reshape(2, 1, 5, 7, C)
    y = ops.to_cl(x)
    assert y.C == C and y.t.dtype == torch.bfloat16 and y.Cpad == ops.pad32(C)
    assert torch.equal(y.t[..., :C], want) and not bool(y.t[..., C:].ne(0).any())
    off, cp = 3, ops.pad32(C + 3) + 32
    buf = torch.randn(2, 1, 5, 7, cp, generator=g).to(dev).bfloat16()
    keep = buf.clone()
    z = ops.to_cl(x, out=buf, c_offset=off, zero_fill=False)
    assert z.C == C + off and z.t.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[..., off:off + C], want)
    assert torch.equal(buf[..., :off].view(torch.int16), keep[..., :off].view(torch.int16))
    assert torch.equal(buf[..., off + C:].view(torch.int16), keep[..., off + C:].view(torch.int16))
    buf2 = keep.clone()
    ops.to_cl(x, out=buf2, c_offset=off, zero_fill=True)
    assert torch.equal(buf2[..., off:off + C], want) and not bool(buf2[..., :off].ne(0).any()) and not bool(buf2[..., off + C:].ne(0).any())


@pytest.mark.parametrize("C", [1, 2, 15, 33])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_from_cl_exact(dev, C, dtype):
    from jointimagegeneration_amd import ops
    cp = ops.pad32(C) + (32 if C == 15 else 0)
    t = torch.randn(2, 1, 5, 7, cp, generator=torch.Generator().manual_seed(C)).to(dev).to(dtype)      # pad lanes hold data: must not leak
    got = ops.from_cl(ops.CL(t, C), 2)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, C, 5, 7)
    assert torch.equal(got, t[..., :C].float().reshape(2, 5, 7, C).permute(0, 3, 1, 2))
    got3 = ops.from_cl(ops.CL(t.view(2, 5, 7, 1, cp), C), 3)
    assert torch.equal(got3, t[..., :C].float().reshape(2, 5, 7, 1, C).permute(0, 4, 1, 2, 3))


@pytest.mark.parametrize("M", [1, 255, 4099])
@pytest.mark.parametrize("K, stride", [(6, 8), (6, 32), (6, 40), (14, 32), (14, 40)])
def test_labels_to_onehot_exact(dev, M, K, stride):
    from jointimagegeneration_amd import ops
    lab = torch.randint(0, K, (M,), generator=torch.Generator().manual_seed(M + K)).int().to(dev)
    lab[0], lab[-1] = K - 1, 0
    out = torch.full((M, stride), 7.0, dtype=torch.bfloat16, device=dev)
    ops.labels_to_onehot(lab, K, out)
    assert torch.equal(out[:, :K], F.one_hot(lab.long(), K).to(torch.bfloat16))
    assert not bool(out[:, K:].ne(0).any())


@pytest.mark.parametrize("C", [32, 96])
@pytest.mark.parametrize("three_d", [False, True], ids=["2d", "3d"])
def test_resample2x_exact(dev, C, three_d):
    """Integer inputs in [-8, 8], no prologue: nearest x2 copies; the 2x average pool is sum / 4 (sum / 8 in 3-D), a multiple of 1/8 with
    |.| <= 8, which bf16 holds exactly."""
    from jointimagegeneration_amd import ops
    sp = (4, 6, 10) if three_d else (1, 6, 10)
    cp = ops.pad32(C) + 32                                                     # pad lanes
    t = torch.zeros((2,) + sp + (cp,), dtype=torch.bfloat16)
    t[..., :C] = _ints((2,) + sp + (C,), -8, 8, C).bfloat16()
    src = ops.CL(t.to(dev), C)
    up = ops.resample2x(src, True, three_d)
    want = src.t.repeat_interleave(2, 2).repeat_interleave(2, 3)
    want = want.repeat_interleave(2, 1) if three_d else want
    assert up.C == C and torch.equal(up.t, want)
    down = ops.resample2x(src, False, three_d)
    D, H, W = sp
    kd = 2 if three_d else 1
    ref = src.t.double().reshape(2, D // kd, kd, H // 2, 2, W // 2, 2, cp).sum((2, 4, 6)) / (4 * kd)
    assert torch.equal(ref.float().bfloat16().double(), ref)                  # the test's own precondition
    assert down.t.dtype == torch.bfloat16 and torch.equal(down.t.double(), ref)


def test_add_exact(dev):
    from jointimagegeneration_amd import ops
    a, b = _ints((3, 51, 264), -64, 64, 1).bfloat16().to(dev), _ints((3, 51, 264), -64, 64, 2).bfloat16().to(dev)      # (gg_add: n % 8 == 0)
    assert torch.equal(ops.add(a, b).double(), a.double() + b.double())


@pytest.mark.parametrize("I", [7, 160, 1280])
def test_linear_f32_exact(dev, I):
    """Integer fp32 operands: |sum| <= 1280 * 64 + 8 < 2^24, so every fp32 partial sum is exact; `out` rows wider than O keep their tail."""
    from jointimagegeneration_amd import ops
    M, O = 5, 96
    x, W, b = _ints((M, I), -8, 8, I).to(dev), _ints((O, I), -8, 8, I + 1).to(dev), _ints((O,), -8, 8, I + 2).to(dev)
    ref = x.double() @ W.double().t() + b.double()
    assert float(ref.abs().max()) < X.LIMIT
    got = ops.linear_f32(x, W, b, act_in=False)
    assert torch.equal(got.double(), ref)
    wide = torch.full((M, O + 32), -3.0, device=dev)
    out = wide[:, :O]
    ops.linear_f32(x, W, None, act_in=False, out=out)
    assert torch.equal(wide[:, :O].double(), x.double() @ W.double().t()) and bool((wide[:, O:] == -3.0).all())
