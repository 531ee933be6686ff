"""GPU suite (-m gpu): the stride-2 3x3x3 tile kernel (conv_tile_s2_kernel, csrc/gg_conv_tile.hip) against the gather kernel it replaces,
bit for bit.

Every comparison here is an equality of stored words; there is no tolerance in this module.
  * test_s2_equals_gather: each case runs through gg_conv_forward (ops.conv) on production dispatch and under path_hint 14
    (ops.HINT_NO_TILE_S2: the kernel declines), with and without a residual, bf16 and fp32 output.  Seeded N(0, 1) bf16 inputs.  The
    descriptor of each launch is captured and gg_conv_runs_tile_s2 asked about it: 1 on production dispatch, 0 under the hint.
    Neither kernel leaves GroupNorm sums: the accumulator handed to both launches comes back as it went in.
  * test_s2_exact: regimes D and S of tests/conv_exact.py against the fp64 reference, at (8, 8, 32) and (16, 16, 64) inputs under
    path_hint 15 (the grid condition lifted: production dispatch sends grids this small to the split gather kernel).
  * test_ccdm_chain_labels: 5 captured CCDM reverse steps at 128^3, production dispatch against path_hint 14; not one label may differ.
    128^3 because the chain's only 128-cout Downsample on a grid that the gather kernel runs in one pass is the one at its 64^3 level.

Shapes of the word-for-word cases.  The gather kernel is a bit reference only where it does not split K: plan_gather wants 192 blocks of
128 positions (x 1 cout group at both widths: NT 2 for 64 couts, NT 4 for 128), i.e. M >= 24576 -- checked on the CPU in
tests/test_conv_tile_s2_cpu.py ((16, 32, 96) -> M = 6144 splits K).  (32, 64, 96) -> (16, 32, 48) is exactly 24576: 8 x 8 x 3 tiles, so every
tile coordinate takes odd and even values, first and last tiles touch the zero padding at -1, and with N = 2 ((16, 64, 96) per sample) the
tile index crosses the sample border.  The kernel is instantiated for 128 couts (Cout_pad 128) only -- 64 couts were measured a tie with the
gather kernel and are not taken -- so the two channel widths are those of the INPUT (64: two chunks, 128: four), plus a padded Cout;
shared / per-sample / no bias.
"""
import ctypes as C

import pytest
import torch

import conv_exact as X

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

K3S2 = dict(k=(3, 3, 3), stride=2, pad=1)
HINT_OFF, HINT_FORCE = 14, 15
# name, N, C, cout, input spatial, bias
BIT_CASES = [
    ("n1_64to128", 1, 64, 128, (32, 64, 96), "shared"),
    ("n1_128to128", 1, 128, 128, (32, 64, 96), "per_sample"),
    ("n2_64to128", 2, 64, 128, (16, 64, 96), "per_sample"),
    ("n2_128to128", 2, 128, 128, (16, 64, 96), "none"),
    ("n1_128to100_padded_cout", 1, 128, 100, (32, 64, 96), "shared"),
]
_E1 = X.Case("s2_64to128", "gather", 1, 64, 0, 128, (8, 8, 32), hint=HINT_FORCE, **K3S2)
_E2 = X.Case("s2_128to128_res", "gather", 1, 128, 0, 128, (8, 8, 32), residual=True, hint=HINT_FORCE, **K3S2)
_E3 = X.Case("s2_n2_128to128_res", "gather", 2, 128, 0, 128, (16, 16, 64), residual=True, bias="per_sample", hint=HINT_FORCE, **K3S2)
_E4 = X.Case("s2_64to128_f32", "gather", 1, 64, 0, 128, (16, 16, 64), out_f32=True, hint=HINT_FORCE, **K3S2)
EXACT_CASES = [(_E1, "D"), (_E1, "S"), (_E2, "D"), (_E2, "S"), (_E3, "D"), (_E3, "S"), (_E4, "D")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _launch(ops, src, pw, bias, cout, per_sample, hint, monkeypatch, residual=None, out_f32=False):
    """one ops.conv under path_hint `hint` -> (output CL, descriptor of the launch)"""
    monkeypatch.setattr(ops, "PATH_HINT", hint)
    sink = []
    with X.captured_descs(sink):
        y = ops.conv(src, pw, bias, cout, bias_per_sample=per_sample, residual=residual, out_f32=out_f32, **K3S2)
    torch.cuda.synchronize()
    assert len(sink) == 1
    return y, sink[0]


@pytest.mark.parametrize("case", BIT_CASES, ids=[c[0] for c in BIT_CASES])
def test_s2_equals_gather(dev, case, monkeypatch):
    from jointimagegeneration_amd import _lib, ops
    name, N, Cin, cout, sp, bias_kind = case
    lib = _lib.load()
    g = torch.Generator().manual_seed(sum(name.encode()))
    gd = torch.Generator(device=dev).manual_seed(sum(name.encode()))
    src = ops.CL(torch.randn((N,) + sp + (Cin,), generator=gd, device=dev).bfloat16(), Cin)
    w = torch.randn((cout, Cin, 3, 3, 3), generator=g).to(dev)
    pw = ops.pack_conv_weight(w, Cin)
    cp = ops.pad32(cout)
    osp = tuple(s // 2 for s in sp)
    bias = None
    if bias_kind != "none":
        bias = torch.zeros((N if bias_kind == "per_sample" else 1, cp))
        bias[:, :cout] = torch.randn((bias.shape[0], cout), generator=g)
        bias = (bias if bias_kind == "per_sample" else bias[0]).to(dev)
    res_t = torch.zeros((N,) + osp + (cp,), device=dev)
    res_t[..., :cout] = torch.randn((N,) + osp + (cout,), generator=gd, device=dev)
    res = ops.CL(res_t.bfloat16(), cout)
    M = N * osp[0] * osp[1] * osp[2]
    assert M == 24576

    def run(hint, residual, out_f32):
        y, d = _launch(ops, src, pw, bias, cout, bias_kind == "per_sample", hint, monkeypatch, residual=residual, out_f32=out_f32)
        acc = torch.full((N, 1, cp, 2), 7, dtype=torch.int64, device=dev)
        out = torch.empty_like(y.t)
        out.view(torch.int16).fill_(0x7fc1)                      # NaN pattern (both dtypes): an element that is not stored shows
        d2 = _lib.ConvDesc.from_buffer_copy(d)
        d2.out, d2.gn_acc = out.data_ptr(), acc.data_ptr()
        _lib.check(lib.gg_conv_forward(C.byref(d2), ops._stream()), "gg_conv_forward")
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), y.t.view(torch.int16)), "the same launch twice differs"
        assert bool((acc == 7).all())
        return out, d

    for residual in (None, res):
        for out_f32 in (False, True):
            what = f"{name} res={residual is not None} f32={out_f32}"
            y_tile, d_tile = run(0, residual, out_f32)
            y_gather, d_gather = run(HINT_OFF, residual, out_f32)
            assert lib.gg_conv_runs_tile_s2(C.byref(d_tile)) == 1, f"{what}: production dispatch did not take the stride-2 tile kernel"
            assert lib.gg_conv_runs_tile_s2(C.byref(d_gather)) == 0 and d_gather.path_hint == HINT_OFF == ops.HINT_NO_TILE_S2
            assert lib.gg_conv_workspace_bytes(C.byref(d_tile)) == lib.gg_conv_workspace_bytes(C.byref(d_gather)) == 0, "the gather kernel splits K here"
            assert lib.gg_conv_emits_stats(C.byref(d_tile)) == lib.gg_conv_emits_stats(C.byref(d_gather)) == 0
            assert tuple(y_tile.shape) == (N,) + osp + (cp,)
            a, b = y_tile.view(torch.int16), y_gather.view(torch.int16)
            if not torch.equal(a, b):
                bad = (a != b).nonzero()
                raise AssertionError(f"{what}: {bad.shape[0]} of {a.numel()} words differ, first (n, d, h, w, word) {bad[0].tolist()}")
            assert not bool(torch.isnan(y_tile.float()).any()), what
            assert not bool(y_tile[..., cout:].ne(0).any()), what


_REF = {}


@pytest.mark.parametrize("cr", EXACT_CASES, ids=X.case_id)
def test_s2_exact(dev, cr, monkeypatch):
    from jointimagegeneration_amd import _lib, ops
    case, regime = cr
    lib = _lib.load()
    key = (case.name, regime)
    if key not in _REF:
        inp = X.build_inputs(case, regime).to(dev)
        ref = X.reference(case, inp)
        X.check_reference(regime, ref)
        _REF[key] = (inp, ref)
    inp, ref = _REF[key]
    src = ops.CL(inp.srcs[0], case.C1)
    pw = ops.pack_conv_weight(inp.w.view((case.cout, case.cin_w) + case.k), src.Cpad)
    residual = ops.CL(inp.residual, case.cout) if inp.residual is not None else None
    y, d = _launch(ops, src, pw, inp.bias, case.cout, case.bias == "per_sample", HINT_FORCE, monkeypatch, residual=residual, out_f32=case.out_f32)
    assert lib.gg_conv_runs_tile_s2(C.byref(d)) == 1 and d.path_hint == HINT_FORCE == ops.HINT_TILE_S2
    assert y.acc is None and y.t.dtype == (torch.float32 if case.out_f32 else torch.bfloat16)
    X.check_output(y.t, ref, regime)


def test_ccdm_chain_labels(dev, monkeypatch):
    """5 captured reverse steps at 128^3: the Downsample of the 64^3 level (128 -> 128) takes the kernel."""
    from jointimagegeneration_amd import _lib, ops
    from jointimagegeneration_amd.pipeline import build_ccdm
    lib = _lib.load()
    ccdm = build_ccdm(14, 250, 1024, dev)
    g = torch.Generator().manual_seed(3)
    x_T = torch.randint(0, 14, (1, 128, 128, 128), generator=g, dtype=torch.int32).to(dev)
    cond = torch.zeros((1, 1, 128, 128, 128), device=dev)

    def chain(hint):
        monkeypatch.setattr(ops, "PATH_HINT", hint)
        ccdm.philox_seed = 12
        sink = []
        with X.captured_descs(sink):
            lab, _ = ccdm.sample_labels(x_T, cond, 10005)
        torch.cuda.synchronize()
        return lab, sum(1 for d in sink if lib.gg_conv_runs_tile_s2(C.byref(d)) == 1), len(sink)

    lab_tile, n_tile, n_all = chain(0)
    lab_gather, n_tile_hint, n_all_hint = chain(HINT_OFF)
    assert n_tile >= 1 and n_tile_hint == 0 and n_all == n_all_hint, (n_tile, n_tile_hint, n_all, n_all_hint)
    diff = int((lab_tile != lab_gather).sum())
    assert diff == 0, f"{diff} of {lab_tile.numel()} labels differ between the stride-2 tile and the gather dispatch"
    assert int(lab_tile.min()) >= 0 and int(lab_tile.max()) < 14 and len(torch.unique(lab_tile)) > 1
