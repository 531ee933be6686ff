"""GPU suite (-m gpu): the split halo path (conv_halo_kernel with the K split as blockIdx.z + conv_splitk_reduce_kernel) against the split
gather kernel it replaces, bit for bit.

Every comparison here is an equality of stored words; there is no tolerance in this module.
  * test_split_equals_gather: each case runs through gg_conv_forward (ops.conv) on production dispatch and under path_hint 13
    (ops.HINT_NO_HALO_SPLIT: the path declines and the gather kernel splits K the same way), with and without a residual, bf16 and fp32
    output.  Seeded N(0, 1) bf16 inputs.  The descriptor of each launch is captured and gg_conv_runs_halo_split asked about it: the
    expected slab count on production dispatch, 0 under the hint, so a gate that silently declines fails the test.  Neither path
    leaves GroupNorm sums (gg_conv_emits_stats == 0): the accumulator handed to both launches comes back as it went in.
  * test_split_exact: regimes D and S of tests/conv_exact.py (inputs without any rounding) against the fp64 reference.
  * test_ccdm_chain_labels: 5 captured CCDM reverse steps with the production UNet widths, production dispatch against the same chain
    under path_hint 13; not one label may differ.

Shapes.  The five 3x3x3 shapes of the CCDM UNet's 16^3 level (128, 256, 320+256, 256+256, 256+128 -> 256 channels) at batch 1: two slabs of
whole chunks each, 16 boxes x 8 cout groups x 2 slabs.  At batch 2 the 16^3 grid passes the halo-tile kernel's own gate (recorded dispatch,
tests/test_halo_split_cpu.py), so batch 2 runs the same channel counts at (8, 16, 16): the same 4096 positions, two samples per launch, the
box index crossing the sample border.  Two smaller grids reach the other splits that plan_gather derives (checked on the CPU in
tests/test_halo_split_cpu.py): (4, 8, 16) 512->256 = 16 slabs of ONE chunk each, (8, 16, 16) 128->256 = 4 slabs of one chunk each; and a
logical Cout below Cout_pad.
The chain runs at 64^3, not at 16^3: at a 16^3 input no conv of the UNet passes the gate (64 channels at 16^3: the gather plan's split does
not divide the two chunks; every deeper level is narrower than the 16-wide box).  64^3 is the smallest cube at which a level is 16^3 with
more than 64 channels (128 and 256 -> 128 channels, 4 slabs).
"""
import ctypes as C

import pytest
import torch

import conv_exact as X

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

K3 = dict(k=(3, 3, 3), stride=1, pad=1)
HINT_OFF = 13
# name, N, C1, C2, cout, spatial, bias, slabs
BIT_CASES = [
    ("n1_128to256", 1, 128, 0, 256, (16, 16, 16), "shared", 2),
    ("n1_256to256", 1, 256, 0, 256, (16, 16, 16), "shared", 2),
    ("n1_320p256to256", 1, 320, 256, 256, (16, 16, 16), "per_sample", 2),
    ("n1_256p256to256", 1, 256, 256, 256, (16, 16, 16), "none", 2),
    ("n1_256p128to256", 1, 256, 128, 256, (16, 16, 16), "shared", 2),
    ("n2_128to256", 2, 128, 0, 256, (8, 16, 16), "per_sample", 2),
    ("n2_256to256", 2, 256, 0, 256, (8, 16, 16), "per_sample", 2),
    ("n2_320p256to256", 2, 320, 256, 256, (8, 16, 16), "shared", 2),
    ("n2_256p256to256", 2, 256, 256, 256, (8, 16, 16), "per_sample", 2),
    ("n2_256p128to256", 2, 256, 128, 256, (8, 16, 16), "none", 2),
    ("n1_512to256_16slabs", 1, 512, 0, 256, (4, 8, 16), "shared", 16),
    ("n1_128to256_4slabs", 1, 128, 0, 256, (8, 16, 16), "shared", 4),
    ("n1_256to250_padded_cout", 1, 256, 0, 250, (16, 16, 16), "shared", 2),
]
_E1 = X.Case("hs_256to256_res", "gather", 1, 256, 0, 256, (16, 16, 16), residual=True, splitk=True, **K3)
_E2 = X.Case("hs_n2_320p256to256", "gather", 2, 320, 256, 256, (8, 16, 16), bias="per_sample", splitk=True, **K3)
_E3 = X.Case("hs_512to256_f32", "gather", 1, 512, 0, 256, (4, 8, 16), out_f32=True, splitk=True, **K3)
EXACT_CASES = [(_E1, "D"), (_E1, "S"), (_E2, "D"), (_E2, "S"), (_E3, "D")]
EXACT_SLABS = {_E1.name: 2, _E2.name: 2, _E3.name: 16}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _launch(ops, srcs, pw, bias, cout, per_sample, hint, monkeypatch, residual=None, out_f32=False):
    """one ops.conv under path_hint `hint` -> (output CL, descriptor of the launch)"""
    monkeypatch.setattr(ops, "PATH_HINT", hint)
    sink = []
    with X.captured_descs(sink):
        y = ops.conv(srcs[0], pw, bias, cout, src2=srcs[1] if len(srcs) > 1 else None, bias_per_sample=per_sample, residual=residual,
                     out_f32=out_f32, **K3)
    torch.cuda.synchronize()
    assert len(sink) == 1
    return y, sink[0]


@pytest.mark.parametrize("case", BIT_CASES, ids=[c[0] for c in BIT_CASES])
def test_split_equals_gather(dev, case, monkeypatch):
    from jointimagegeneration_amd import _lib, ops
    name, N, C1, C2, cout, sp, bias_kind, slabs = case
    lib = _lib.load()
    g = torch.Generator().manual_seed(sum(name.encode()))
    srcs = [ops.CL(torch.randn((N,) + sp + (c,), generator=g).bfloat16().to(dev), c) for c in (C1, C2) if c]
    w = torch.randn((cout, C1 + C2, 3, 3, 3), generator=g).to(dev)
    pw = ops.pack_conv_weight(w, C1 + C2)
    cp = ops.pad32(cout)
    bias = None
    if bias_kind != "none":
        bias = torch.zeros((N if bias_kind == "per_sample" else 1, cp))
        bias[:, :cout] = torch.randn((bias.shape[0], cout), generator=g)
        bias = (bias if bias_kind == "per_sample" else bias[0]).to(dev)
    res_t = torch.zeros((N,) + sp + (cp,))
    res_t[..., :cout] = torch.randn((N,) + sp + (cout,), generator=g)
    res = ops.CL(res_t.bfloat16().to(dev), cout)
    M = N * sp[0] * sp[1] * sp[2]

    def run(hint, residual, out_f32):
        # raw launch through the C-ABI with an accumulator attached: whatever the kernels do with gn_acc is visible
        y, d = _launch(ops, srcs, pw, bias, cout, bias_kind == "per_sample", hint, monkeypatch, residual=residual, out_f32=out_f32)
        acc = torch.full((N, 1, cp, 2), 7, dtype=torch.int64, device=dev)
        out = torch.empty_like(y.t)
        out.view(torch.int16).fill_(0x7fc1)                      # NaN pattern (both dtypes): an element that is not stored shows
        ws = torch.full((d.workspace_bytes // 4,), float("nan"), device=dev)       # a slab element that is not written shows
        d2 = _lib.ConvDesc.from_buffer_copy(d)
        d2.out, d2.gn_acc, d2.workspace = out.data_ptr(), acc.data_ptr(), ws.data_ptr()
        _lib.check(lib.gg_conv_forward(C.byref(d2), ops._stream()), "gg_conv_forward")
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), y.t.view(torch.int16)), "the same launch twice differs"
        assert bool((acc == 7).all())
        return out, d

    for residual in (None, res):
        for out_f32 in (False, True):
            what = f"{name} res={residual is not None} f32={out_f32}"
            y_split, d_split = run(0, residual, out_f32)
            y_gather, d_gather = run(HINT_OFF, residual, out_f32)
            assert lib.gg_conv_runs_halo_split(C.byref(d_split)) == slabs, f"{what}: production dispatch did not take the split halo path"
            assert lib.gg_conv_runs_halo_split(C.byref(d_gather)) == 0 and d_gather.path_hint == HINT_OFF == ops.HINT_NO_HALO_SPLIT
            assert lib.gg_conv_runs_halo_tile(C.byref(d_split)) == lib.gg_conv_runs_halo_tile(C.byref(d_gather)) == 0
            assert lib.gg_conv_emits_stats(C.byref(d_split)) == lib.gg_conv_emits_stats(C.byref(d_gather)) == 0
            assert lib.gg_conv_workspace_bytes(C.byref(d_split)) == lib.gg_conv_workspace_bytes(C.byref(d_gather)) == slabs * M * cp * 4
            assert tuple(y_split.shape) == (N,) + sp + (cp,)
            a, b = y_split.view(torch.int16), y_gather.view(torch.int16)
            if not torch.equal(a, b):
                bad = (a != b).nonzero()
                raise AssertionError(f"{what}: {bad.shape[0]} of {a.numel()} words differ, first (n, d, h, w, word) {bad[0].tolist()}")
            assert not bool(torch.isnan(y_split.float()).any()), what
            assert not bool(y_split[..., cout:].ne(0).any()), what


_REF = {}


@pytest.mark.parametrize("cr", EXACT_CASES, ids=X.case_id)
def test_split_exact(dev, cr, monkeypatch):
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
    residual = ops.CL(inp.residual, case.cout) if inp.residual is not None else None
    y, d = _launch(ops, srcs, pw, inp.bias, case.cout, case.bias == "per_sample", 0, monkeypatch, residual=residual, out_f32=case.out_f32)
    assert lib.gg_conv_runs_halo_split(C.byref(d)) == EXACT_SLABS[case.name]
    assert y.acc is None and y.t.dtype == (torch.float32 if case.out_f32 else torch.bfloat16)
    X.check_output(y.t, ref, regime)


def test_ccdm_chain_labels(dev, monkeypatch):
    """5 captured reverse steps at 64^3 (the smallest cube with a level that passes the gate, see the module text)."""
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
        return lab, sum(1 for d in sink if lib.gg_conv_runs_halo_split(C.byref(d)) > 0), len(sink)

    lab_split, n_split, n_all = chain(0)
    lab_gather, n_split_hint, n_all_hint = chain(HINT_OFF)
    assert n_split >= 1 and n_split_hint == 0 and n_all == n_all_hint, (n_split, n_split_hint, n_all, n_all_hint)
    assert ccdm.use_graph, "the chain is meant to run as a captured step"
    diff = int((lab_split != lab_gather).sum())
    assert diff == 0, f"{diff} of {lab_split.numel()} labels differ between the split halo and the gather dispatch"
    assert int(lab_split.min()) >= 0 and int(lab_split.max()) < 14 and len(torch.unique(lab_split)) > 1
