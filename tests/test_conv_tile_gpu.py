"""GPU suite (-m gpu): the streaming 1x1 tile kernel (csrc/gg_conv_tile.hip) against the gather kernel it replaces, bit for bit.

Every comparison here is an equality of stored words; there is no tolerance in this module.
  * test_tile_equals_gather: each case runs twice through gg_conv_forward (ops.conv), on production dispatch and under path_hint 12
    (ops.HINT_GATHER: the tile kernel declines).  Seeded N(0, 1) bf16 inputs; the outputs must be equal as 16-bit words.  The descriptor of
    each launch is captured and gg_conv_runs_tile asked about it: 1 on production dispatch, 0 under the hint, so a gate that silently
    declines fails the test.  Neither kernel leaves GroupNorm sums on these shapes (gg_conv_emits_stats == 0 on both descriptors): the
    accumulator handed to both launches must come back as it went in, int64 for int64.
  * test_tile_exact: regimes D and S of tests/conv_exact.py (inputs without any rounding) against the fp64 reference; regime P (a
    GroupNorm prologue) is outside the kernel's envelope: the case asserts that the tile kernel declines and that the gather kernel's
    result is exact.
  * test_ccdm_chain_labels: 5 captured CCDM reverse steps with the production UNet widths, production dispatch against the same chain
    under path_hint 12.  The cube is 64^3, not 32^3: the kernel's gate is 64^3 positions (at 32^3 it was measured slower than the gather
    kernel), so 64^3 is the smallest cube at which a conv of the chain takes the new path -- the three 1x1 skip projections of its
    first level.  Not one label may differ.

Shapes: the gate is M >= 262144 positions, so every case has between 262144 and 275766 of them (the smallest that reach the kernel on
production dispatch): N = 1 and 2, whole 32-position tiles and a ragged last tile, a last tile of sample 0 that borders sample 1
(137883 positions per sample), every instantiated (Cout_pad, channel) pair, and a logical Cout below Cout_pad.  With 8192+ tiles over
at most 2048 resident waves every wave walks several tiles (register double buffer, stage reuse).
"""
import ctypes as C

import pytest
import torch

import conv_exact as X

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

K1 = dict(k=(1, 1, 1), pad=0)
# name, N, C1, C2, cout, spatial, bias
BIT_CASES = [
    ("n1_64to128_whole_tiles", 1, 64, 0, 128, (64, 64, 64), "shared"),                 # one source; M = 262144 = 8192 tiles
    ("n2_128p64to64_ragged_border", 2, 128, 64, 64, (41, 57, 59), "per_sample"),       # 137883 per sample: tile 4308 holds rows of both samples; M % 32 = 22
    ("n2_128p128to128", 2, 128, 128, 128, (32, 64, 65), "per_sample"),                 # whole tiles, the sample border on a tile border
    ("n1_64p64to64", 1, 64, 64, 64, (64, 64, 65), "shared"),
    ("n1_128p64to128", 1, 128, 64, 128, (64, 65, 65), "shared"),
    ("n2_64p64to50_padded_cout", 2, 64, 64, 50, (41, 57, 59), "per_sample"),           # Cout 50 in Cout_pad 64: pad lanes stored as zeros
    ("n1_128p64to64_nobias", 1, 128, 64, 64, (64, 64, 64), "none"),
]
_E1 = X.Case("t1_64to128", "gather", 1, 64, 0, 128, (64, 64, 64), **K1)
_E2 = X.Case("t1_n2_64p64to64", "gather", 2, 64, 64, 64, (41, 57, 59), bias="per_sample", **K1)
_E3 = X.Case("t1_128p64to128", "gather", 1, 128, 64, 128, (64, 64, 65), **K1)
EXACT_CASES = [(_E1, "D"), (_E1, "S"), (_E2, "D"), (_E2, "S"), (_E2, "P"), (_E3, "D")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _launch(ops, lib, srcs, pw, bias, cout, per_sample, hint, monkeypatch, prologue=None):
    """one ops.conv under path_hint `hint` -> (output tensor, accumulator handed to the launch, descriptor of the launch)"""
    monkeypatch.setattr(ops, "PATH_HINT", hint)
    sink = []
    with X.captured_descs(sink):
        y = ops.conv(srcs[0], pw, bias, cout, src2=srcs[1] if len(srcs) > 1 else None, bias_per_sample=per_sample, prologue=prologue,
                     prologue_silu=False, **K1)
    torch.cuda.synchronize()
    assert len(sink) == 1
    return y, sink[0]


@pytest.mark.parametrize("case", BIT_CASES, ids=[c[0] for c in BIT_CASES])
def test_tile_equals_gather(dev, case, monkeypatch):
    from jointimagegeneration_amd import _lib, ops
    name, N, C1, C2, cout, sp, bias_kind = case
    lib = _lib.load()
    g = torch.Generator().manual_seed(sum(name.encode()))
    gd = torch.Generator(device=dev).manual_seed(sum(name.encode()))                  # (the activations are drawn on the device: 10^7..10^8 values)
    srcs = [ops.CL(torch.randn((N,) + sp + (c,), generator=gd, device=dev).bfloat16(), c) for c in (C1, C2) if c]
    w = torch.randn((cout, C1 + C2, 1, 1, 1), generator=g).to(dev)
    pw = ops.pack_conv_weight(w, C1 + C2)
    cp = ops.pad32(cout)
    bias = None
    if bias_kind != "none":
        bias = torch.zeros((N if bias_kind == "per_sample" else 1, cp))
        bias[:, :cout] = torch.randn((bias.shape[0], cout), generator=g)
        bias = (bias if bias_kind == "per_sample" else bias[0]).to(dev)
    M = N * sp[0] * sp[1] * sp[2]

    def run(hint):
        # raw launch through the C-ABI with an accumulator attached: whatever the kernel does with gn_acc is visible
        y, d = _launch(ops, lib, srcs, pw, bias, cout, bias_kind == "per_sample", hint, monkeypatch)
        acc = torch.full((N, 1, cp, 2), 7, dtype=torch.int64, device=dev)
        out = torch.empty_like(y.t)
        out.view(torch.int16).fill_(0x7fc1)                      # NaN pattern: an element that is not stored shows
        d2 = _lib.ConvDesc.from_buffer_copy(d)
        d2.out, d2.gn_acc = out.data_ptr(), acc.data_ptr()
        _lib.check(lib.gg_conv_forward(C.byref(d2), ops._stream()), "gg_conv_forward")
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), y.t.view(torch.int16)), "the same launch twice differs"
        return out, acc, d

    y_tile, acc_tile, d_tile = run(0)
    y_gather, acc_gather, d_gather = run(ops.HINT_GATHER)
    assert lib.gg_conv_runs_tile(C.byref(d_tile)) == 1, f"{name}: production dispatch did not take the tile kernel"
    assert lib.gg_conv_runs_tile(C.byref(d_gather)) == 0 and d_gather.path_hint == 12
    assert lib.gg_conv_runs_halo_tile(C.byref(d_tile)) == 0
    assert lib.gg_conv_emits_stats(C.byref(d_tile)) == lib.gg_conv_emits_stats(C.byref(d_gather)) == 0
    assert lib.gg_conv_workspace_bytes(C.byref(d_tile)) == lib.gg_conv_workspace_bytes(C.byref(d_gather)) == 0
    assert tuple(y_tile.shape) == (N,) + sp + (cp,) and y_tile.numel() == M * cp
    a, b = y_tile.view(torch.int16), y_gather.view(torch.int16)
    if not torch.equal(a, b):
        bad = (a != b).nonzero()
        raise AssertionError(f"{name}: {bad.shape[0]} of {a.numel()} words differ, first (n, d, h, w, c) {bad[0].tolist()}")
    assert not bool(torch.isnan(y_tile.float()).any())
    assert torch.equal(acc_tile, acc_gather) and bool((acc_tile == 7).all())
    assert not bool(y_tile[..., cout:].ne(0).any())


_REF = {}


@pytest.mark.parametrize("cr", EXACT_CASES, ids=X.case_id)
def test_tile_exact(dev, cr, monkeypatch):
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
    srcs = [ops.CL(t, c) for t, c in zip(inp.srcs, (case.C1, case.C2))]
    pw = ops.pack_conv_weight(inp.w.view((case.cout, case.cin_w) + case.k), sum(s.Cpad for s in srcs))
    y, d = _launch(ops, lib, srcs, pw, inp.bias, case.cout, case.bias == "per_sample", 0, monkeypatch, prologue=inp.prologue)
    # regime P: a prologue is outside the envelope -- the kernel declines without an error and the gather kernel runs
    assert lib.gg_conv_runs_tile(C.byref(d)) == (0 if regime == "P" else 1)
    assert d.prologue_act == (2 if regime == "P" else 0)
    assert y.acc is None and y.t.dtype == torch.bfloat16
    X.check_output(y.t, ref, regime)


def test_ccdm_chain_labels(dev, monkeypatch):
    """5 captured reverse steps at 64^3 (the smallest cube whose first level passes the kernel's 64^3-position gate)."""
    from jointimagegeneration_amd import _lib, ops
    from jointimagegeneration_amd.pipeline import build_ccdm
    lib = _lib.load()
    ccdm = build_ccdm(14, 250, 1024, dev)
    g = torch.Generator().manual_seed(3)
    x_T = torch.randint(0, 14, (1, 64, 64, 64), generator=g, dtype=torch.int32).to(dev)
    cond = torch.zeros((1, 1, 64, 64, 64), device=dev)

    def chain(hint):
        monkeypatch.setattr(ops, "PATH_HINT", hint)
        ccdm.philox_seed = 12
        sink = []
        with X.captured_descs(sink):
            lab, _ = ccdm.sample_labels(x_T, cond, 10005)
        torch.cuda.synchronize()
        return lab, sum(1 for d in sink if lib.gg_conv_runs_tile(C.byref(d)) == 1), len(sink)

    lab_tile, n_tile, n_all = chain(0)
    lab_gather, n_tile_hint, n_all_hint = chain(ops.HINT_GATHER)
    assert n_tile >= 3 and n_tile_hint == 0 and n_all == n_all_hint, (n_tile, n_tile_hint, n_all, n_all_hint)
    assert ccdm.use_graph, "the chain is meant to run as a captured step"
    diff = int((lab_tile != lab_gather).sum())
    assert diff == 0, f"{diff} of {lab_tile.numel()} labels differ between the tile and the gather dispatch"
    assert int(lab_tile.min()) >= 0 and int(lab_tile.max()) < 14 and len(torch.unique(lab_tile)) > 1
