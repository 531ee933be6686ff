"""Exact-arithmetic conv checks: inputs on which a bf16 conv has NO rounding, the fp64 reference, and comparators without a tolerance.

bf16 x bf16 products are exact in fp32.  If activations, weights, bias and residual are small integers times a power of two, every
partial sum -- in any order, over any split-K slab or MFMA grouping -- is an integer number of quanta below 2^24, so fp32 accumulation
is exact too: an fp32-output conv must equal the fp64 reference (shadow.conv_reference) bit for bit, a bf16-output conv its
round-to-nearest-even rounding.  A single lost product, a tap that was not zero padded, a missing split-K slab or skip channel changes
stored bits.

Regimes (build_inputs asserts the preconditions on the host; a violated precondition is an error of the test, never a skip):
  D  dense: activations in {+-1..+-4} (no zeros: no product can be dropped unseen), weights in {+-1..+-4}/8, bias in {-8..8}/8,
     integer residual in [-8, 8].  Quantum 1/8; |sum| <= K * 16 + 8 + 64 quanta (K = taps x all concatenated input channels,
     skip projection included), asserted < 2^24.
  S  sparse weights: activations +-1, every output channel has exactly min(K, 96) weights +-1 (seeded; half of them forced onto the
     first / last channel of every source and the last channel in front of every 32- / 160-channel chunk boundary, in every tap),
     integer bias and residual in [-8, 8]: |y| <= 96 + 8 + 8 < 120 is an integer, so the bf16 output is exact as well, and the
     epilogue's fp32 sums of y and y^2 over tiles of <= 1024 rows (1024 * 120^2 < 2^24) are exact: the GroupNorm accumulators must
     be sum(y) * 2^28 and sum(y^2) * 2^20 as integers.
  P  exact prologue: regime D activations, per-(n, c) scale in {+-0.5, +-1, +-2} and a NON-ZERO integer shift in [-4, 4], affine only
     (prologue_silu=False).  The staged value x * scale + shift is a half-integer with |.| <= 12: exact in bf16; 48 replaces 16 in
     the bound, and the quantum of the sums is 1/16.  A padded tap that received the prologue instead of 0 changes the sum by shift * w != 0.

Kernel paths are identified on the descriptor of the launch itself (captured as the shadow captures it) with the library's host
predicates: kernel_path().
"""
from __future__ import annotations

import contextlib
import ctypes as C
import importlib.util
import os
import zlib
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

import shadow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINT_TEAM, HINT_GENERIC, HINT_SPEC_ONLY = 7, 10, 11          # gg_conv_desc.path_hint (gg_conv_halo.hip, gg_conv.h)
NNZ = 96                                                      # regime S: non-zero weights per output channel
Y_MAX = 120                                                   # regime S: |y| bound
TILE_ROWS = 1024                                              # largest epilogue tile whose fp32 sums feed one accumulator add
LIMIT = 1 << 24                                               # integers below this are exact in fp32


@dataclass(frozen=True)
class Case:
    name: str
    path: str                     # gather | gather5 | tiny | halo | team | box | spec | f32
    N: int
    C1: int
    C2: int
    cout: int
    sp: Tuple[int, int, int]      # input (D, H, W)
    k: Tuple[int, int, int] = (1, 3, 3)
    stride: int = 1
    pad: int = 1
    up: bool = False
    out_f32: bool = False
    bias: str = "shared"          # none | shared | per_sample
    residual: bool = False
    skip: Optional[Tuple[int, int]] = None      # channels of the K-concatenated skip projection's sources
    hint: int = 0                 # ops.PATH_HINT of the launch (None: whatever a fixture set)
    splitk: Optional[bool] = None  # expected gg_conv_workspace_bytes > 0 (gather / gather5 / tiny paths)
    stats: bool = False           # ask for the GroupNorm accumulators (want_stats) in every regime (table entries with gn_acc)

    @property
    def taps(self):
        return self.k[0] * self.k[1] * self.k[2]

    @property
    def cin_w(self):
        """input channels of the weight: the first source padded (a second source follows it), the last one logical"""
        return (shadow.pad32(self.C1) + self.C2) if self.C2 else self.C1

    @property
    def K(self):
        return self.taps * self.cin_w + (sum(self.skip) if self.skip else 0)

    @property
    def out_sp(self):
        from jointimagegeneration_amd import ops
        return ops.conv_out_extent(self.sp, self.k, self.stride, self.pad, self.up)

    @property
    def M(self):
        o = self.out_sp
        return self.N * o[0] * o[1] * o[2]


def c2(name, path, N, C1, C2, cout, hw, **kw):
    return Case(name, path, N, C1, C2, cout, (1,) + tuple(hw), **kw)


def c3(name, path, N, C1, C2, cout, dhw, **kw):
    return Case(name, path, N, C1, C2, cout, tuple(dhw), k=kw.pop("k", (3, 3, 3)), **kw)


# ------------------------------------------------------------------------------------------------ inputs
@dataclass
class Inputs:
    srcs: List[torch.Tensor]                      # channels-last [N, D, H, W, Cpad], zero pad lanes (bf16; fp32 for the validation conv)
    w: torch.Tensor                               # fp32 [Cout, cin_w, taps]
    bias: Optional[torch.Tensor]                  # fp32 [Cout_pad] or [N, Cout_pad]
    residual: Optional[torch.Tensor]              # channels-last [N, Do, Ho, Wo, Cout_pad]
    prologue: Optional[Tuple[torch.Tensor, torch.Tensor]] = None      # fp32 [N, sum Cpad] scale, shift (0 on pad lanes)
    skip_srcs: Optional[List[torch.Tensor]] = None
    skip_w: Optional[torch.Tensor] = None         # fp32 [Cout, Cs, 1]

    def to(self, dev):
        mv = lambda t: None if t is None else t.to(dev)
        return Inputs([mv(s) for s in self.srcs], mv(self.w), mv(self.bias), mv(self.residual),
                      None if self.prologue is None else (mv(self.prologue[0]), mv(self.prologue[1])),
                      None if self.skip_srcs is None else [mv(s) for s in self.skip_srcs], mv(self.skip_w))


def _signed(g, shape, hi):
    """integers in {+-1..+-hi}, no zeros"""
    return torch.randint(1, hi + 1, shape, generator=g).float() * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


def _cl(vals: torch.Tensor, dtype) -> torch.Tensor:
    """[N, D, H, W, C] values -> zero-padded channels-last tensor"""
    out = torch.zeros(tuple(vals.shape[:-1]) + (shadow.pad32(vals.shape[-1]),), dtype=dtype)
    out[..., :vals.shape[-1]] = vals.to(dtype)
    return out


def special_channels(case: Case) -> List[int]:
    """weight input channels a chunk walk can lose: first / last of every source, last in front of a 32- / 160-channel boundary"""
    c1p = shadow.pad32(case.C1)
    ch = {0, case.C1 - 1}
    if case.C2:
        ch |= {c1p, c1p + case.C2 - 1}
    ch |= {c for c in range(case.cin_w) if c % 32 == 31 or c % 160 == 159}
    if case.C2 == 0:
        ch = {c for c in ch if c < case.C1}
    else:
        ch = {c for c in ch if c < case.C1 or c >= c1p}
    return sorted(ch)


def _sparse_weight(case: Case, g) -> torch.Tensor:
    cin, T, K = case.cin_w, case.taps, case.taps * case.cin_w
    nnz = min(K, NNZ)
    score = torch.rand((case.cout, cin * T), generator=g)
    if case.C2 and shadow.pad32(case.C1) != case.C1:
        raise AssertionError("two sources need an unpadded first source")
    forced = torch.tensor([c * T + t for c in special_channels(case) for t in range(T)])
    f = min(nnz // 2, forced.numel())
    rot = (torch.arange(case.cout)[:, None] * f + torch.arange(f)[None]) % forced.numel()
    score.scatter_(1, forced[rot], 2.0)
    idx = score.topk(nnz, dim=1).indices
    w = torch.zeros((case.cout, cin * T))
    w.scatter_(1, idx, torch.randint(0, 2, idx.shape, generator=g).float() * 2 - 1)
    return w.view(case.cout, cin, T)


def build_inputs(case: Case, regime: str, seed: int = 0) -> Inputs:
    """CPU tensors of one case in regime D / S / P, preconditions asserted (check_preconditions)."""
    assert regime in ("D", "S", "P")
    g = torch.Generator().manual_seed((zlib.crc32(f"{case.name}/{regime}".encode()) + seed) % (1 << 31))
    f32 = case.path == "f32"
    adt = torch.float32 if f32 else torch.bfloat16
    N, cp = case.N, shadow.pad32(case.cout)
    amax = 1 if regime == "S" else 4
    srcs = [_cl(_signed(g, (N,) + case.sp + (c,), amax), adt) for c in (case.C1, case.C2) if c]
    w = _sparse_weight(case, g) if regime == "S" else _signed(g, (case.cout, case.cin_w, case.taps), 4) / 8
    bias = None
    if case.bias != "none":
        rows = N if case.bias == "per_sample" else 1
        bias = torch.zeros(rows, cp)
        bv = torch.randint(-8, 9, (rows, case.cout), generator=g).float()
        bias[:, :case.cout] = bv if regime == "S" else bv / 8
        bias = bias if case.bias == "per_sample" else bias[0]
    residual = None
    if case.residual:
        residual = _cl(torch.randint(-8, 9, (N,) + case.out_sp + (case.cout,), generator=g).float(), adt)
    inp = Inputs(srcs, w, bias, residual)
    if regime == "P":
        ct = sum(s.shape[-1] for s in srcs)
        scale, shift = torch.zeros(N, ct), torch.zeros(N, ct)
        off = 0
        for s, c in zip(srcs, (case.C1, case.C2)):
            scale[:, off:off + c] = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N, c), generator=g)] * (torch.randint(0, 2, (N, c), generator=g).float() * 2 - 1)
            shift[:, off:off + c] = _signed(g, (N, c), 4)
            off += s.shape[-1]
        inp.prologue = (scale, shift)
    if case.skip:
        assert regime == "D", "the K-concatenated skip projection is checked in regime D"
        inp.skip_srcs = [_cl(_signed(g, (N,) + case.out_sp + (c,), 4), adt) for c in case.skip if c]
        inp.skip_w = _signed(g, (case.cout, sum(case.skip), 1), 4) / 8
    check_preconditions(case, regime, inp)
    return inp


def _bf16_exact(t: torch.Tensor) -> bool:
    return torch.equal(t.float().to(torch.bfloat16).float(), t.float())


def check_preconditions(case: Case, regime: str, inp: Inputs) -> None:
    """The value-level preconditions of the regime (what makes every fp32 partial sum exact); AssertionError otherwise."""
    tensors = inp.srcs + [inp.w] + [t for t in (inp.bias, inp.residual, inp.skip_w) if t is not None] + (inp.skip_srcs or [])
    assert all(_bf16_exact(t) for t in tensors), "a value does not survive the bf16 round trip"
    c_log = [case.C1] + ([case.C2] if case.C2 else [])
    for s, c in zip(inp.srcs, c_log):
        assert bool((s[..., :c] != 0).all()) and not bool((s[..., c:] != 0).any()), "activations: non-zero on logical lanes, zero on pad lanes"
    if regime == "S":
        K = case.taps * case.cin_w
        assert all(bool((s[..., :c].float().abs() == 1).all()) for s, c in zip(inp.srcs, c_log))
        assert bool(((inp.w != 0).sum((1, 2)) == min(K, NNZ)).all()) and bool((inp.w.abs() <= 1).all())
        assert torch.equal(inp.w, inp.w.round()) and (inp.bias is None or torch.equal(inp.bias, inp.bias.round()))
        covered = (inp.w != 0).any(0)                                  # [cin_w, taps]
        if case.cout * (min(K, NNZ) // 2) >= len(special_channels(case)) * case.taps:
            assert bool(covered[special_channels(case)].all()), "regime S: a (special channel, tap) pair has no weight on any output channel"
        ymax = min(K, NNZ) + (8 if inp.bias is not None else 0) + (8 if inp.residual is not None else 0)
        assert ymax <= Y_MAX and TILE_ROWS * Y_MAX * Y_MAX < LIMIT
        return
    a = 12 if regime == "P" else 4
    assert all(bool((s.float().abs() <= 4).all()) for s in inp.srcs + (inp.skip_srcs or []))
    assert bool(((inp.w * 8).abs() <= 4).all()) and torch.equal(inp.w * 8, (inp.w * 8).round()) and bool((inp.w != 0).all())
    if regime == "P":
        sc, sh = inp.prologue
        off = 0
        for s, c in zip(inp.srcs, c_log):
            z = s[..., :c].float() * sc[:, None, None, None, off:off + c] + sh[:, None, None, None, off:off + c]
            assert _bf16_exact(z) and bool((z.abs() <= 12).all()) and bool((sh[:, off:off + c] != 0).all()), "regime P: staged value not an exact bf16 half-integer"
            off += s.shape[-1]
    # in quanta of 1/8 (regime P: the staged half-integers make the quantum 1/16, so twice as many)
    quanta = (case.taps * case.cin_w * a * 4 + (sum(case.skip) * 16 if case.skip else 0) + 8 + 64) * (2 if regime == "P" else 1)
    assert quanta < LIMIT and case.K * (48 if regime == "P" else 16) + 16 < LIMIT, f"{case.name}: {quanta} quanta do not fit fp32"


# ------------------------------------------------------------------------------------------------ reference and comparators
def conv_call(case: Case, inp: Inputs) -> shadow.ConvCall:
    skip = (inp.skip_srcs, inp.skip_w) if inp.skip_srcs is not None else None
    return shadow.ConvCall(srcs=inp.srcs, w=inp.w, bias=inp.bias, bias_per_sample=case.bias == "per_sample", cout=case.cout, k=case.k,
                           stride=case.stride, pad=case.pad, upsample=case.up, residual=inp.residual, prologue=inp.prologue, act=False, skip=skip)


def reference(case: Case, inp: Inputs, chunk: Optional[int] = None) -> torch.Tensor:
    """fp64 [N, Do, Ho, Wo, Cout] of shadow.conv_reference at EVERY output position of every sample (its bound is ignored), on the
    device the inputs live on.  chunk: fp64 elements per gather chunk (shadow.CHUNK by default)."""
    call = conv_call(case, inp)
    osp = case.out_sp
    pos = shadow._all_positions(osp).to(inp.w.device)
    old = shadow.CHUNK
    try:
        if chunk:
            shadow.CHUNK = chunk
        ref = torch.stack([shadow.conv_reference(call, n, pos)[0] for n in range(case.N)])
    finally:
        shadow.CHUNK = old
    return ref.view((case.N,) + tuple(osp) + (case.cout,))


def check_reference(regime: str, ref: torch.Tensor) -> None:
    """What the reference alone must satisfy for the regime's exactness argument."""
    if regime == "S":
        assert torch.equal(ref, ref.round()) and float(ref.abs().max()) <= Y_MAX, f"regime S: max |y| = {float(ref.abs().max())}"
        assert TILE_ROWS * float(ref.abs().max()) ** 2 < LIMIT
    else:
        q = 16 if regime == "P" else 8
        assert torch.equal(ref * q, (ref * q).round()) and float(ref.abs().max()) * q < LIMIT


def _first_mismatches(got: torch.Tensor, want: torch.Tensor, what: str) -> str:
    bad = (got != want) | torch.isnan(got)
    idx = bad.nonzero()[:5].tolist()
    rows = ", ".join(f"{tuple(i)}: got {float(got[tuple(i)])!r} want {float(want[tuple(i)])!r}" for i in idx)
    return f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first (n, d, h, w, c): {rows}"


def check_output(got: torch.Tensor, ref: torch.Tensor, regime: str) -> None:
    """got: channels-last [N, Do, Ho, Wo, Cout_pad] (bf16 or fp32); ref: fp64 [N, Do, Ho, Wo, Cout].  No tolerance."""
    cout = ref.shape[-1]
    assert tuple(got.shape[:-1]) == tuple(ref.shape[:-1]) and got.shape[-1] >= cout, (tuple(got.shape), tuple(ref.shape))
    assert shadow.pad_lanes_zero(got, cout), f"pad lanes [{cout}, {got.shape[-1]}) are not all 0"
    g = got[..., :cout]
    if got.dtype == torch.float32:
        assert torch.equal(g.double(), ref), _first_mismatches(g.double(), ref, "fp32 output vs fp64 reference")
        return
    assert got.dtype == torch.bfloat16
    want = ref.float().to(torch.bfloat16)          # round to nearest even; ref is exact in fp32 (check_reference)
    assert torch.equal(g, want), _first_mismatches(g.double(), want.double(), "bf16 output vs round-to-nearest-even of the fp64 reference")
    if regime == "S":
        assert torch.equal(g.double(), ref), _first_mismatches(g.double(), ref, "bf16 output vs fp64 reference (exact integers)")


def expected_acc(ref: torch.Tensor) -> torch.Tensor:
    """int64 [N, Cout, 2]: (sum y * 2^28, sum y^2 * 2^20) of integer outputs"""
    y = ref.round().long().reshape(ref.shape[0], -1, ref.shape[-1])
    return torch.stack([y.sum(1) * int(shadow.ACC_SUM_SCALE), (y * y).sum(1) * int(shadow.ACC_SQ_SCALE)], -1)


def check_acc(acc: torch.Tensor, ref: torch.Tensor) -> None:
    """acc: int64 [N, stripes, Cout_pad, 2] left by the conv's epilogue; regime S only (integer outputs: no rounding anywhere)."""
    cout = ref.shape[-1]
    a = acc.sum(1)
    assert not bool(a[:, cout:].ne(0).any()), "accumulator pad lanes are not 0"
    want = expected_acc(ref).to(a.device)
    bad = (a[:, :cout] != want).nonzero()[:5].tolist()
    assert torch.equal(a[:, :cout], want), f"accumulators differ at (n, c, sum|sumsq) {bad}: got {[int(a[tuple(i)]) for i in bad]} want {[int(want[tuple(i)]) for i in bad]}"


# ------------------------------------------------------------------------------------------------ kernel paths
def _desc_copy(d):
    from jointimagegeneration_amd._lib import ConvDesc
    return ConvDesc.from_buffer_copy(d)


def kernel_path(lib, d) -> str:
    """The kernel family gg_conv_forward runs descriptor d on, from the library's host predicates in gg_conv_forward's own order
    (halo-tile, box, tiny-M, 160-step gather, gather):
      halo / team  gg_conv_runs_halo_tile; under path_hint 7 the team kernel takes what its envelope (gg_conv_halo3_try: bf16 out,
                   3x3x3 stride 1 without upsample, Cout_pad % 64 == 0, Do % 8 == Ho % 8 == Wo % 16 == 0) allows;
      box          not halo, and plan_box accepts: gg_conv_fuses_ddim answers exactly that for a 4-channel fp32 head without residual;
                   plan_box reads Cout_pad, never Cout, so the question is put to a copy of d with those three fields replaced;
      tiny         M <= 128 without prologue (gg_conv_tiny_plan);
      gather5      both sources multiples of 160 channels and fewer than 4096 64x32 tiles (plan_gather5)."""
    if lib.gg_conv_runs_halo_tile(C.byref(d)):
        team = (d.path_hint == HINT_TEAM and d.kd == 3 and not d.upsample and d.out_dtype == 0 and d.Cout_pad % 64 == 0 and d.Do % 8 == 0 and
                d.Ho % 8 == 0 and d.Wo % 16 == 0 and not d.skip_C1 and not d.pro_acc1 and not d.ddim_x)
        return "team" if team else "halo"
    q = _desc_copy(d)
    q.Cout, q.out_dtype, q.residual = 4, 1, None
    if lib.gg_conv_fuses_ddim(C.byref(q)):
        return "box"
    M = d.N * d.Do * d.Ho * d.Wo
    if M <= 128 and d.prologue_act == 0:
        return "tiny"
    if d.C1 % 160 == 0 and d.C2 % 160 == 0 and (M + 63) // 64 * (d.Cout_pad // 32) < 4096:
        return "gather5"
    return "gather"


def case_desc(case: Case, regime: str = "D", hint: Optional[int] = None):
    """The descriptor ops.conv builds for the case (no pointers except the flags the plans read): for host-side path checks."""
    from jointimagegeneration_amd._lib import GG_BF16, GG_F32, ConvDesc
    d = ConvDesc()
    d.N, (d.D, d.H, d.W) = case.N, case.sp
    d.C1, d.C2 = shadow.pad32(case.C1), shadow.pad32(case.C2) if case.C2 else 0
    d.Cout, d.Cout_pad = case.cout, shadow.pad32(case.cout)
    d.kd, d.kh, d.kw = case.k
    d.stride, d.pad, d.upsample = case.stride, case.pad, 1 if case.up else 0
    d.Do, d.Ho, d.Wo = case.out_sp
    d.out_dtype = GG_F32 if case.out_f32 else GG_BF16
    d.prologue_act = 2 if regime == "P" else 0
    d.path_hint = case.hint if hint is None else hint
    if case.skip:
        d.skip_C1, d.skip_C2 = case.skip
    return d


def assert_path(lib, d, case: Case) -> None:
    """The launch whose descriptor is d ran on the kernel path the case is named for."""
    got = kernel_path(lib, d)
    want = "box" if case.path == "spec" else case.path
    assert got == want, f"{case.name}: expected the {want} kernel, the descriptor runs on {got}"
    if case.path == "spec":
        assert d.path_hint == HINT_SPEC_ONLY and d.N == 1         # a box conv without a table entry is an error under this hint
    if case.path == "box":
        assert d.path_hint == HINT_GENERIC or d.N != 1            # ... and under this one the table is not consulted
    if case.splitk is not None:
        assert (lib.gg_conv_workspace_bytes(C.byref(d)) > 0) == case.splitk, f"{case.name}: split-K expected {case.splitk}"
    if case.skip:
        assert lib.gg_conv_fuses_skip(C.byref(d)) == 1


@contextlib.contextmanager
def captured_descs(sink: list):
    """Every gg_conv_forward descriptor launched inside the block is copied into `sink` (the shadow's library proxy)."""
    import pytest
    from jointimagegeneration_amd import _lib
    proxy = shadow._LibProxy(_lib.load(), sink)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_lib, "load", lambda: proxy)
        yield sink


# ------------------------------------------------------------------------------------------------ cases
# Shapes are those of the tolerance-based edge tests (tests/test_hip_parity.py).  Where the dispatch has moved a listed shape to another
# kernel since that test was written, the nearest shape that still reaches the named kernel is used and the comment says so.
GATHER_CASES = [
    c3("g3d_same", "gather", 1, 64, 0, 96, (5, 6, 7)),
    c3("g3d_stride2_odd", "tiny", 1, 32, 0, 32, (5, 7, 9), stride=2),                      # 3x4x5 outputs: M = 60, the tiny-M kernel takes it ...
    c3("g3d_stride2_odd_m210", "gather", 1, 32, 0, 32, (9, 11, 13), stride=2),            # ... so the same conv with 5x6x7 outputs for the gather kernel
    c3("g3d_upsample", "gather", 1, 64, 0, 64, (3, 4, 5), up=True),
    c3("g3d_stem_cin15", "gather", 1, 15, 0, 64, (8, 8, 8)),
    c3("g3d_head_f32", "gather", 1, 64, 0, 14, (8, 8, 8), out_f32=True),
    c2("g2d_ae_down_s2_p0", "tiny", 1, 32, 0, 32, (16, 12), stride=2, pad=0),              # M = 48: tiny-M kernel; (32, 28) below: gather
    c2("g2d_ae_down_s2_p0_m224", "gather", 1, 32, 0, 32, (32, 28), stride=2, pad=0),
    c2("g2d_1x1", "box", 2, 192, 0, 64, (8, 8), k=(1, 1, 1), pad=0),                      # M = 128, 8-wide tiles: production runs the box kernel
    Case("g1d_1x1_tokens", "tiny", 2, 64, 0, 192, (1, 1, 50), k=(1, 1, 1), pad=0),         # M = 100: tiny-M kernel; T = 150 below: gather
    Case("g1d_1x1_tokens_t150", "gather", 2, 64, 0, 192, (1, 1, 150), k=(1, 1, 1), pad=0),
    # 160-step variant.  320+160 -> 160 at (24, 8) and 160 -> 160 stride 2 at 16x16 now run on the box kernel (8-wide tiles, stride-2 boxes);
    # W = 9 / odd extents keep the same channel counts outside its envelope (Wo % 4 != 0)
    c2("g5_two_sources_residual", "gather5", 1, 320, 160, 160, (24, 9), residual=True),
    c2("g5_stride2", "gather5", 2, 160, 0, 160, (18, 18), stride=2, bias="none"),
]

# split-K: the three shapes of test_splitk_reduce_is_deterministic all fit the box kernel today (4-, 4- and 4-wide tiles); one column
# more (W = 5, 21, 13) keeps Cin / Cout / M class and leaves the envelope, so the tiny-M / 160-step split-K slabs are what runs
SPLITK_CASES = [
    c2("sk_1600to800_4x5", "tiny", 1, 1600, 0, 800, (4, 5), residual=True, splitk=True),
    c2("sk_320to160_20x21", "gather5", 1, 320, 0, 160, (20, 21), residual=True, splitk=True),
    c2("sk_n2_640to320_12x13", "gather5", 2, 640, 0, 320, (12, 13), residual=True, splitk=True),
]

TINY_CASES = [
    c2("tiny_1600to800_4x5", "tiny", 1, 1600, 0, 800, (4, 5)),                            # (4x4 is a box shape: see SPLITK_CASES)
    c2("tiny_1600to800_4x5_f32", "tiny", 1, 1600, 0, 800, (4, 5), out_f32=True),
    c2("tiny_1x1_320to96_5x7", "tiny", 1, 320, 0, 96, (5, 7), k=(1, 1, 1), pad=0),
    c2("tiny_1x1_320to96_5x7_f32", "tiny", 1, 320, 0, 96, (5, 7), k=(1, 1, 1), pad=0, out_f32=True),
]

# halo-tile kernel: run under the halo_hint fixture (path_hint 1 / 4 / 6), so hint=None
HALO_CASES = [
    c3("h3d_nt2", "halo", 1, 64, 0, 64, (8, 8, 32), hint=None),
    c3("h3d_nt4", "halo", 2, 32, 0, 128, (4, 8, 16), hint=None),
    c3("h3d_nt3_cin15", "halo", 1, 15, 0, 96, (8, 8, 16), hint=None),
    c3("h3d_head_f32", "halo", 1, 64, 0, 14, (4, 8, 16), out_f32=True, hint=None),
    c3("h3d_up", "halo", 1, 64, 0, 64, (4, 4, 8), up=True, hint=None),
    c2("h2d_nt2", "halo", 1, 160, 0, 320, (32, 32), hint=None),
    c2("h2d_nt4", "halo", 2, 96, 0, 128, (32, 48), hint=None),
    c2("h2d_up", "halo", 1, 128, 0, 128, (16, 8), up=True, hint=None),
    c2("h2d_cout1", "halo", 1, 128, 0, 1, (32, 16), hint=None),
]
HALO_P_CASE = c3("h3d_two_sources", "halo", 2, 64, 32, 64, (4, 8, 16), bias="per_sample", residual=True, hint=None)

TEAM_CASES = [
    c3("team_one_item", "team", 1, 64, 0, 64, (8, 8, 16), hint=HINT_TEAM),
    c3("team_two_sources_n2", "team", 2, 64, 32, 128, (8, 16, 32), bias="per_sample", residual=True, hint=HINT_TEAM),
    c3("team_six_chunks", "team", 1, 128, 64, 64, (24, 8, 48), bias="per_sample", hint=HINT_TEAM),
    c3("team_ragged_persistent", "team", 1, 96, 0, 192, (32, 64, 64), residual=True, hint=HINT_TEAM),
]

_B = dict(hint=HINT_GENERIC)
BOX_CASES = [
    c2("box_th2", "box", 1, 160, 0, 160, (16, 16), **_B),
    c2("box_th4", "box", 2, 32, 0, 512, (20, 16), **_B),
    c2("box_th8_up", "box", 2, 32, 0, 320, (24, 16), up=True, **_B),
    c2("box_cout14_f32", "box", 1, 64, 0, 14, (16, 32), out_f32=True, **_B),
    c2("box_cin15", "box", 1, 15, 0, 64, (12, 16), **_B),
    c2("box_w8", "box", 1, 640, 0, 640, (8, 8), **_B),
    c2("box_w4", "box", 1, 800, 0, 800, (4, 4), **_B),
    c2("box_w8_three_stages", "box", 1, 1280, 0, 64, (8, 8), **_B),
    c2("box_w4_sub4_cout40", "box", 1, 800, 0, 40, (4, 4), **_B),
    c2("box_w8_sub2_cout72", "box", 1, 640, 0, 72, (8, 8), **_B),
    c2("box_ragged12", "box", 1, 160, 0, 160, (64, 64), **_B),
    c2("box_ragged3", "box", 1, 96, 0, 640, (16, 16), **_B),
    c2("box_ragged_up", "box", 1, 64, 0, 320, (16, 16), up=True, **_B),
    # stride 2 (BOX_S2_CASES)
    c2("box_s2_640_8x8", "box", 1, 640, 0, 640, (8, 8), stride=2, **_B),
    c2("box_s2_64to40_24x16", "box", 1, 64, 0, 40, (24, 16), stride=2, **_B),
    c2("box_s2_64_16x8", "box", 1, 64, 0, 64, (16, 8), stride=2, **_B),        # (10, 8) of BOX_S2_CASES has 5x4 outputs: 4-wide tiles need Ho % 4 == 0, it runs on the tiny-M kernel
    c2("box_s2_n3_32to96_12x32", "box", 3, 32, 0, 96, (12, 32), stride=2, **_B),
    # 1x1 with residual.  The box kernel takes 1x1 convs up to M = 256 only: (2, 160, 480, (16, 32)) and (1, 320, 160, (24, 16)) of
    # test_conv_box_kernel_1x1_with_residual run on the 160-step kernel; the same channels at M = 256 stay here
    c2("box_1x1_qkv_8x8", "box", 1, 640, 0, 1920, (8, 8), k=(1, 1, 1), pad=0, residual=True, **_B),
    c2("box_1x1_qkv_8x16_n2", "box", 2, 160, 0, 480, (8, 16), k=(1, 1, 1), pad=0, residual=True, **_B),
    c2("box_1x1_proj_4x4", "box", 1, 800, 0, 800, (4, 4), k=(1, 1, 1), pad=0, residual=True, **_B),
    c2("box_1x1_skip_16x16", "box", 1, 320, 0, 160, (16, 16), k=(1, 1, 1), pad=0, residual=True, **_B),
]
BOX_SKIP_CASES = [            # test_conv_box_kconcat_skip_projection: (N, Cout, Cs1, Cs2, spatial); the 3x3 input has Cout channels
    c2("box_skip_out64_160+160", "box", 1, 160, 0, 160, (64, 64), skip=(160, 160), **_B),
    c2("box_skip_out16_640+640", "box", 1, 640, 0, 640, (16, 16), skip=(640, 640), **_B),
    c2("box_skip_in8_320_n2", "box", 2, 320, 0, 320, (8, 8), skip=(640, 0), **_B),
    c2("box_skip_out4_800+800", "box", 1, 800, 0, 800, (4, 4), skip=(800, 800), **_B),
    c2("box_skip_out32_160+160", "box", 1, 320, 0, 320, (32, 32), skip=(160, 160), **_B),
    c2("box_skip_ragged_20x16", "box", 1, 64, 0, 64, (20, 16), skip=(96, 0), **_B),
]
BOX_P_CASES = [               # regime P where gg_conv_fuses_prologue holds (at most two cout tiles share a box)
    c2("box_p_3x3_160to32", "box", 1, 160, 0, 32, (16, 16), **_B),
    c2("box_p_two_sources", "box", 2, 64, 32, 24, (20, 16), bias="per_sample", residual=True, **_B),
]

F32_CASES = [                 # gg_conv_forward_f32 (inside ops.fp32_validation()), fp32 integer tensors
    c3("f32_same", "f32", 2, 15, 0, 40, (6, 8, 10), out_f32=True),
    c3("f32_stride2", "f32", 2, 15, 0, 64, (6, 8, 10), stride=2, out_f32=True),
    c3("f32_upsample", "f32", 1, 15, 0, 33, (3, 4, 5), up=True, out_f32=True),
    c3("f32_two_sources", "f32", 2, 64, 64, 64, (4, 5, 6), bias="per_sample", residual=True, out_f32=True),
]

SPEC_FIELDS = ("H", "W", "C1", "C2", "Cout", "Cout_pad", "Ho", "Wo", "K3", "UP", "TWI", "MT", "CT", "NS", "nstage", "nch_stage", "gn_bytes",
               "q_major", "skip_C1", "skip_C2", "nstage_s", "nch_stage_s", "prologue_act", "pro_acc", "bias", "residual", "gn_acc", "out_f32",
               "ddim_x", "ddim_pred_x0", "ddim_unet_in")


def _gen_box_specs():
    spec = importlib.util.spec_from_file_location("gen_box_specs", os.path.join(ROOT, "tools", "gen_box_specs.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def spec_cases() -> List[Case]:
    """One case per entry of gg_conv_box_specs.inc without prologue and DDIM fields, its flags reproduced through ops.conv's arguments."""
    out = []
    for key in _gen_box_specs().table_keys():
        v = [int(x) for x in key[len("GG_BOX_SPEC("):-1].split(",")]
        assert len(v) == len(SPEC_FIELDS), key
        e = dict(zip(SPEC_FIELDS, v))
        if e["prologue_act"] or e["pro_acc"] or e["ddim_x"] or e["ddim_pred_x0"] or e["ddim_unet_in"]:
            continue
        k = (1, 3, 3) if e["K3"] else (1, 1, 1)
        flags = "".join(s for s, on in (("r", e["residual"]), ("g", e["gn_acc"]), ("f", e["out_f32"])) if on)
        name = (f"spec_{e['H']}x{e['W']}_{e['C1']}to{e['Cout']}_k{3 if e['K3'] else 1}" + ("_up" if e["UP"] == 1 else "_s2" if e["UP"] == 2 else "") +
                (f"_skip{e['skip_C1']}+{e['skip_C2']}" if e["skip_C1"] else "") + (f"_{flags}" if flags else ""))
        assert e["C2"] == 0 and e["Cout"] == e["Cout_pad"], key
        out.append(Case(name, "spec", 1, e["C1"], 0, e["Cout"], (1, e["H"], e["W"]), k=k, stride=2 if e["UP"] == 2 else 1, pad=1 if e["K3"] else 0,
                        up=e["UP"] == 1, out_f32=bool(e["out_f32"]), bias="shared" if e["bias"] else "none", residual=bool(e["residual"]),
                        skip=(e["skip_C1"], e["skip_C2"]) if e["skip_C1"] else None, hint=HINT_SPEC_ONLY, stats=bool(e["gn_acc"])))
    assert len({c.name for c in out}) == len(out)
    return out


SPEC_CASES = spec_cases()

# (case, regime) pairs the GPU module runs, by group
GROUPS = {
    "gather": [(c, "D") for c in GATHER_CASES],
    "splitk": [(c, "D") for c in SPLITK_CASES],
    "tiny": [(c, "D") for c in TINY_CASES],
    "halo": [(c, r) for c in HALO_CASES for r in ("D", "S")] + [(HALO_P_CASE, "P")],
    "team": [(c, r) for c in TEAM_CASES for r in ("D", "S", "P")],
    "box": [(c, r) for c in BOX_CASES for r in ("D", "S")] + [(c, "D") for c in BOX_SKIP_CASES] + [(c, "P") for c in BOX_P_CASES],
    "spec": [(c, "D") for c in SPEC_CASES] + [(c, "S") for c in SPEC_CASES if c.stats and not c.skip],
    "f32": [(c, "D") for c in F32_CASES],
}


def case_id(cr) -> str:
    return f"{cr[0].name}-{cr[1]}"
