"""Exact-arithmetic attention checks: inputs on which every fp32 operation of the flash-attention kernel (csrc/gg_attn.hip) is exact,
the closed-form result, comparators without a tolerance, a layout packer with poisoned surroundings, and an fp32 emulation of the
kernel's step structure into which defects can be injected.

The inputs.  Head dim D, amplitude A = 64, a group id gid(j) per key and a target group per query.  The first D/2 channels carry a
+-1 code of the id (binary digit 0 -> +1, 1 -> -1, unused digits +1), the last D/2 channels a shift:
    k_j = A * [code(gid(j)), +1 ...]          q_i = A * [code(target(i)), -1 ...]
so q_i . k_j = -2 A^2 hamming(code(target(i)), code(gid(j))): exactly 0 for the keys of the target group and <= -8192 for all
others, all partial sums integers below 2^24.  With the production scale 1/sqrt(D) the best non-target base-2 exponent is -2089 (D = 32)
to -522 (D = 512).  The kernel then computes m = 0, p = exp2(0) = 1 on the group, p = exp2(<= -522) = 0 elsewhere, alpha = 0 whenever
the running max rises to 0 (whatever an earlier step accumulated is wiped), l = |group| and o = the integer sum of the group's V rows.
The target score is exactly 0, so fma(s, scale_log2, -m) has no rounding residual and no special scale is needed.

Regimes (build() asserts the preconditions; a violated precondition is an error of the test, never a skip):
  sel  selection: every key its own group; out[i] == V[want(i)] bit for bit, V random bf16 with distinct rows.  want() is a permutation
       (stride ~0.618 Tkv) when Tq >= Tkv -- every key is the target of a query -- and an even spread from key 0 to key Tkv-1 when
       Tq < Tkv, so that targets lie in the first, middle and last tile and alpha = 0 rescales of a non-empty state happen.
  grp  groups: gid(j) = (j + off) mod G, so a group's 2..8 members are strided across tiles, both in-workgroup halves and the key-split
       ranges.  V = c + delta with an integer c != 0, |c| <= 8, per (group, channel) and non-zero integer deltas that sum to 0 over
       the group: out == c exactly (the fp32 1/l error is far below half a bf16 ulp of an integer <= 8, however the division
       rounds).  One dropped member moves the result by |delta| / (n - 1) >= 1/7, one doubled member by |delta| / (n + 1) >= 1/9, a
       zero row counted as live by |c| / (n + 1) >= 1/9: each more than one bf16 ulp (<= 1/16 at 8).
  uni  uniform zero-sum: one group, V non-zero integers in [-4, 4] whose column sums are 0: out == 0 everywhere (-0 equals +0).  A
       dropped key, a doubled key or (LDS-DMA path) the clamped last row counted as live gives a non-zero output.  A ZERO-filled pad
       row counted as live (register-staged paths) does NOT show here: it adds 0 to the numerator and the quotient stays 0; sel and
       grp catch it on every ragged shape (l is one too large).
Different (sample, head) pairs get different ids, targets and V, so a head or batch mix-up changes bits.

The reference is shadow.attention_reference in fp64.  Rounded to bf16 it must equal the closed form in sel and grp (the non-target
weights are <= e^-361).  In uni the closed form is exactly 0 while the fp64 reference carries its own rounding of 1 / Tkv times
integers: check_reference() holds it to Tkv * 2^-52 * max|v|, the reference's own error, and the kernel is compared with 0.

Hardware facts the regimes rest on (v_exp_f32(0) == 1, v_exp_f32(x <= -500) == 0): see tests/test_attn_exact_gpu.py.

peaked(): the fourth leg, WITH the shadow bound: scores of standard deviation 4 on a staircase of 12 per key tile along a direction shared
by all queries (the last tile at least half full), so that every query's running max rises in every tile (0 < alpha < 1 in every step that opens a tile) and sum p|v| is
of the order of |ref|.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

import shadow

A = 64.0
REGIMES = ("sel", "grp", "uni")
SENTINEL = 12352.0                  # bf16-exact; no regime produces it (|out| <= 12 on exact inputs)
LOG2E_F32 = 1.4426950408889634      # the literal of gg_attention_forward, rounded to fp32 there
RAMP, SIGMA = 12.0, 4.0             # peaked leg: score ramp per key tile, score standard deviation


def _f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32))


@dataclass(frozen=True)
class Case:
    name: str
    path: str                 # plain | ws2 | dma | split
    D: int
    Tq: int
    Tkv: int
    N: int = 1
    heads: int = 1
    layout: str = "legacy"    # legacy | new | kv | ae
    ks: int = 1               # key ranges with a workspace (path split)

    @property
    def KT(self):
        return 256 if self.D == 32 else 64 if self.D <= 128 else 32

    @property
    def plan(self):
        """{key tile, key split with a workspace, in-workgroup split, DMA staging} the case is named for"""
        return (self.KT, self.ks, int(self.path == "ws2"), int(self.path in ("dma", "split")))

    @property
    def scale(self):
        return float(self.D) ** -0.5

    def regimes(self):
        return ("sel",) if self.Tkv < 2 else REGIMES


def _sq(name, path, D, T, **kw):
    return Case(name, path, D, T, T, **kw)


CASES: List[Case] = [
    # ---- plain kernel, D < 256
    _sq("plain_d32_t300", "plain", 32, 300, heads=2),
    _sq("plain_d32_t33", "plain", 32, 33, layout="new", heads=3),
    _sq("plain_d64_t200", "plain", 64, 200, layout="new", heads=2),
    _sq("plain_d128_t130", "plain", 128, 130),
    _sq("plain_d64_t250", "plain", 64, 250, heads=2),
    _sq("plain_d64_t100_n2h3", "plain", 64, 100, N=2, heads=3),
    _sq("plain_d128_t65_ae", "plain", 128, 65, layout="ae"),
] + [Case(f"plain_d64_q17_kv{t}", "plain", 64, 17, t, layout="kv", heads=2) for t in (1, 7, 31, 32, 33, 63, 64, 65)] + [
    Case(f"plain_d32_q65_kv{t}", "plain", 32, 65, t, layout="kv") for t in (1, 33, 255, 256, 257)] + [
    Case(f"plain_d128_q{t}_kv130", "plain", 128, t, 130, layout="kv", heads=2) for t in (1, 17, 65)] + [
    # ---- in-workgroup key split: blocks <= 256 and Tkv >= 4 KT
    _sq("ws2_d32_t1024", "ws2", 32, 1024),
    _sq("ws2_d32_t1100", "ws2", 32, 1100, layout="new", heads=2),          # 5 tiles: halves of 3 and 2 (ragged) tiles
    _sq("ws2_d32_t1500", "ws2", 32, 1500),                                 # 6 tiles
    _sq("ws2_d64_t256", "ws2", 64, 256),
    _sq("ws2_d64_t257", "ws2", 64, 257, layout="new", heads=2),            # 5 tiles, the last one a single key
    _sq("ws2_d64_t300", "ws2", 64, 300, layout="ae"),
    _sq("ws2_d128_t256", "ws2", 128, 256, heads=2),
    _sq("ws2_d128_t333", "ws2", 128, 333, layout="new", heads=2),
    _sq("ws2_d64_t300_n2h3", "ws2", 64, 300, N=2, heads=3),
    Case("ws2_d64_q65_kv300", "ws2", 64, 65, 300, layout="kv", heads=2),
    Case("ws2_d128_q17_kv256", "ws2", 128, 17, 256, layout="kv"),
    Case("ws2_d32_q1_kv1100", "ws2", 32, 1, 1100, layout="kv"),
    # ---- LDS-DMA staging, unsplit
    _sq("dma_d256_t100", "dma", 256, 100),
    _sq("dma_d384_t40", "dma", 384, 40, layout="new"),
    _sq("dma_d256_t125", "dma", 256, 125),
    _sq("dma_d512_t255", "dma", 512, 255, layout="ae"),
    _sq("dma_d256_t65_h2", "dma", 256, 65, layout="new", heads=2),
    Case("dma_d384_q65_kv100", "dma", 384, 65, 100, layout="kv"),
    Case("dma_d256_q8192_kv300", "dma", 256, 8192, 300, layout="kv"),      # 128 workgroups: no split, 10 double-buffered tiles
    # ---- LDS-DMA staging, keys split over workgroups + merge launch
    _sq("split_d256_t777_n2", "split", 256, 777, N=2, ks=6),
    _sq("split_d384_t1030", "split", 384, 1030, layout="new", ks=8),       # ranges of 160 keys: the eighth is empty
    _sq("split_d512_t256", "split", 512, 256, layout="ae", ks=2),
    Case("split_d256_q17_kv300_h2", "split", 256, 17, 300, layout="kv", heads=2, ks=2),
    _sq("split_d512_t4096", "split", 512, 4096, ks=4),                     # the autoencoder's mid-block attention
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)
PEAKED = ("plain_d64_t250", "ws2_d64_t300", "dma_d256_t125", "split_d512_t256")          # one per path
F32_CASES = [Case("f32_d32_t300", "f32", 32, 300, 300, heads=2), Case("f32_d64_q17_kv65", "f32", 64, 17, 65, layout="kv", heads=2),
             Case("f32_d32_t70_n2", "f32", 32, 70, 70, N=2, layout="new", heads=3)]
F32_SCALE = 2.0 ** -4               # the fp32 kernel multiplies q and k by sqrt(scale) each: an even power of two keeps that exact


# ------------------------------------------------------------------------------------------------ plan query
def _desc(case: Case):
    from jointimagegeneration_amd import _lib
    d = _lib.AttentionDesc()
    d.N, d.heads, d.head_dim, d.Tq, d.Tkv = case.N, case.heads, case.D, case.Tq, case.Tkv
    return d


def plan_of(case: Case) -> Tuple[int, int, int, int]:
    """gg_attention_plan of the case's shape (host logic: no GPU needed)"""
    from jointimagegeneration_amd import _lib
    lib = _lib.load()
    plan = (C.c_int32 * 4)()
    d = _desc(case)
    _lib.check(lib.gg_attention_plan(C.byref(d), plan), "gg_attention_plan")
    return tuple(plan)


def assert_path(case: Case) -> None:
    got = plan_of(case)
    assert got == case.plan, f"{case.name}: the shape no longer reaches the {case.path} path: plan {got}, expected {case.plan}"


# ------------------------------------------------------------------------------------------------ inputs
@dataclass
class Inputs:
    q: torch.Tensor           # [N, Tq, heads, D]
    k: torch.Tensor           # [N, Tkv, heads, D]
    v: torch.Tensor
    want: torch.Tensor        # closed form [N, Tq, heads, D] (bf16 values)
    gid: torch.Tensor         # [N, heads, Tkv]
    tgt: torch.Tensor         # [N, heads, Tq]
    scale: float

    def probe_key(self, n: int, h: int, query: int) -> int:
        """a key the query attends to, in the middle of its group"""
        m = (self.gid[n, h] == self.tgt[n, h, query]).nonzero().flatten()
        return int(m[len(m) // 2])


def _code(ids: torch.Tensor, D: int) -> torch.Tensor:
    nb = min(D // 2, 40)
    bits = (ids[..., None] >> torch.arange(nb)) & 1
    out = torch.ones(ids.shape + (D // 2,))
    out[..., :nb] = 1.0 - 2.0 * bits
    return out


def _zero_sum(g: torch.Generator, lead: Tuple[int, ...], n: int, D: int) -> torch.Tensor:
    """[*lead, n, D] non-zero integers in [-4, 4] that sum to 0 over the n axis (n >= 2), in a random order per column"""
    assert n >= 2
    parts = []
    if n % 2:
        a = torch.randint(1, 3, lead + (1, D), generator=g).float()
        b = torch.randint(1, 3, lead + (1, D), generator=g).float()
        sg = torch.randint(0, 2, lead + (1, D), generator=g).float() * 2 - 1
        parts += [sg * a, sg * b, -sg * (a + b)]
    pairs = (n - (3 if n % 2 else 0)) // 2
    if pairs:
        a = torch.randint(1, 5, lead + (pairs, D), generator=g).float() * (torch.randint(0, 2, lead + (pairs, D), generator=g).float() * 2 - 1)
        parts += [a, -a]
    x = torch.cat(parts, -2)
    order = torch.rand(x.shape, generator=g).argsort(-2)
    return x.gather(-2, order)


def _coprime_stride(T: int) -> int:
    s = max(1, int(T * 0.618))
    while math.gcd(s, T) != 1:
        s += 1
    return s


def n_groups(Tkv: int) -> int:
    return max((Tkv + 7) // 8, 2 if Tkv >= 4 else 1)


def build(case: Case, regime: str, dtype=torch.bfloat16, scale: Optional[float] = None) -> Inputs:
    N, H, D, Tq, Tkv = case.N, case.heads, case.D, case.Tq, case.Tkv
    assert regime in case.regimes(), (case.name, regime)
    g = torch.Generator().manual_seed(((case.D * 8209 + case.Tq) * 8209 + case.Tkv) * 64 + case.N * 16 + case.heads * 4 + REGIMES.index(regime))
    gid = torch.zeros(N, H, Tkv, dtype=torch.long)
    tgt = torch.zeros(N, H, Tq, dtype=torch.long)
    v = torch.zeros(N, Tkv, H, D)
    want = torch.zeros(N, Tq, H, D)
    j, i = torch.arange(Tkv), torch.arange(Tq)
    for n in range(N):
        for h in range(H):
            nh = n * H + h
            if regime == "sel":
                gid[n, h] = (j + 7 * nh) % Tkv
                if Tq >= Tkv:
                    key = ((i % Tkv) * _coprime_stride(Tkv) + 3 * nh) % Tkv
                    assert len(torch.unique(key)) == Tkv                               # every key is some query's target
                elif Tq == 1:
                    key = torch.tensor([Tkv - 1])                                      # the last key: every earlier step is wiped
                else:
                    key = torch.round(i.double() * (Tkv - 1) / (Tq - 1)).long()
                    assert key[0] == 0 and key[-1] == Tkv - 1
                tgt[n, h] = gid[n, h][key]
                vv = torch.randn(Tkv, D, generator=g).to(torch.bfloat16).float()
                vv = torch.where(vv == 0, torch.ones_like(vv), vv)
                assert len(torch.unique(vv, dim=0)) == Tkv and bool((vv != 0).all())
                v[n, :, h], want[n, :, h] = vv, vv[key]
            elif regime == "grp":
                G = n_groups(Tkv)
                gid[n, h] = (j + 5 * nh) % G
                tgt[n, h] = (i + 3 * nh) % G
                cc = torch.randint(1, 9, (G, D), generator=g).float() * (torch.randint(0, 2, (G, D), generator=g).float() * 2 - 1)
                vv = torch.zeros(Tkv, D)
                sizes = torch.bincount(gid[n, h], minlength=G)
                assert int(sizes.min()) >= 2 and int(sizes.max()) <= 8, sizes
                for sz in torch.unique(sizes).tolist():
                    ids = (sizes == sz).nonzero().flatten()                             # groups of this size
                    delta = _zero_sum(g, (len(ids),), sz, D)                            # [groups, members, D]
                    members = torch.stack([(gid[n, h] == int(x)).nonzero().flatten() for x in ids])          # [groups, members]
                    vv[members] = cc[ids][:, None, :] + delta
                    assert bool((delta != 0).all()) and bool((delta.sum(1) == 0).all())
                    # one dropped / doubled member, or a zero row counted as live, moves the quotient by more than a bf16 ulp at 8
                    assert float(delta.abs().min()) / (sz + 1) > 2.0 ** -4 and 1.0 / (sz + 1) > 2.0 ** -4
                v[n, :, h], want[n, :, h] = vv, cc[tgt[n, h]]
            else:
                vv = _zero_sum(g, (), Tkv, D)
                assert bool((vv != 0).all()) and bool((vv.sum(0) == 0).all())
                v[n, :, h] = vv
    q = torch.cat([_code(tgt, D), -torch.ones(N, H, Tq, D // 2)], -1).permute(0, 2, 1, 3) * A
    k = torch.cat([_code(gid, D), torch.ones(N, H, Tkv, D // 2)], -1).permute(0, 2, 1, 3) * A
    for n in range(N):                                                                 # every targeted group has a member
        for h in range(H):
            assert bool(torch.isin(tgt[n, h], gid[n, h]).all())
    inp = Inputs(q.contiguous().to(dtype), k.contiguous().to(dtype), v.to(dtype), want.to(dtype), gid, tgt,
                 case.scale if scale is None else scale)
    assert bool((inp.v.float() == v).all()) and bool((inp.want.float() == want).all())   # exact in the storage type
    check_scores(case, inp)
    return inp


def check_scores(case: Case, inp: Inputs) -> None:
    """scores: exactly 0 on the target group; elsewhere the kernel's base-2 exponent is below -500"""
    sl2 = _f32(_f32(inp.scale) * _f32(LOG2E_F32))
    for n in range(case.N):
        for h in range(case.heads):
            q, k = inp.q[n, :min(case.Tq, 512), h].double(), inp.k[n, :, h].double()
            s = q @ k.t()
            on = inp.tgt[n, h, :q.shape[0], None] == inp.gid[n, h][None, :]
            assert bool((s[on] == 0).all()) and bool(on.any(1).all())
            if bool((~on).any()):
                assert float(s[~on].max()) <= -2 * A * A and float(s[~on].max()) * sl2 < -500.0


def reference(inp: Inputs, dev=None) -> torch.Tensor:
    """fp64 shadow.attention_reference of every (sample, head): [N, Tq, heads, D]"""
    q, k, v = (t if dev is None else t.to(dev) for t in (inp.q, inp.k, inp.v))
    out = torch.empty(q.shape, dtype=torch.float64, device=q.device)
    for n in range(q.shape[0]):
        for h in range(q.shape[2]):
            for r0 in range(0, q.shape[1], 2048):
                rows = torch.arange(r0, min(r0 + 2048, q.shape[1]), device=q.device)
                out[n, rows, h] = shadow.attention_reference(q[n, :, h], k[n, :, h], v[n, :, h], inp.scale, rows)[0]
    return out


def check_reference(regime: str, inp: Inputs, ref: torch.Tensor) -> None:
    """the closed form is the fp64 reference rounded to the storage type (uni: within the reference's own rounding of 0)"""
    want = inp.want.to(ref.device)
    if regime == "uni":
        lim = inp.k.shape[1] * 2.0 ** -52 * float(inp.v.float().abs().max())
        assert float(ref.abs().max()) <= lim, (float(ref.abs().max()), lim)
        assert bool((want == 0).all())
    else:
        assert not mismatches(ref.to(want.dtype), want), mismatches(ref.to(want.dtype), want)


# ------------------------------------------------------------------------------------------------ comparators
def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def mismatches(got: torch.Tensor, want: torch.Tensor, limit: int = 4) -> str:
    """'' if got equals want bit for bit (-0 equals +0), else a description of the first differences"""
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = (_bits(got) != _bits(want)) & ~((got == 0) & (want == 0))
    nbad = int(bad.sum())
    if not nbad:
        return ""
    idx = bad.nonzero()[:limit].tolist()
    return f"{nbad} of {bad.numel()} elements differ; first (n, t, h, d): " + "; ".join(
        f"{tuple(ix)} got {float(got[tuple(ix)])!r} want {float(want[tuple(ix)])!r}" for ix in idx)


# ------------------------------------------------------------------------------------------------ layouts
@dataclass
class Packed:
    """buffers of one launch: element (n, t, h, d) at base + off + (n T + t) ld + h hs + d; everything else is NaN (inputs) / SENTINEL (out)"""
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    out: torch.Tensor
    ld_hs_q: Tuple[int, int]
    ld_hs_k: Tuple[int, int]
    ld_hs_v: Tuple[int, int]
    ld_hs_o: Tuple[int, int]
    q_off: int
    k_off: int
    v_off: int

    def to(self, dev):
        q = self.q.to(dev)
        k = q if self.k is self.q else self.k.to(dev)
        v = q if self.v is self.q else k if self.v is self.k else self.v.to(dev)
        return Packed(q, k, v, self.out.to(dev), self.ld_hs_q, self.ld_hs_k, self.ld_hs_v, self.ld_hs_o, self.q_off, self.k_off, self.v_off)


def pack(case: Case, inp: Inputs) -> Packed:
    N, H, D, Tq, Tkv = case.N, case.heads, case.D, case.Tq, case.Tkv
    Cc, dt = H * D, inp.q.dtype
    nan = lambda rows, ld: torch.full(((rows + 2) * ld,), float("nan"), dtype=dt)       # two rows nobody addresses at the end
    if case.layout in ("legacy", "new", "ae"):
        assert Tq == Tkv and (case.layout != "ae" or H == 1)
        ld = 3 * Cc + {"legacy": 0, "new": 8, "ae": 64}[case.layout]
        buf = nan(N * Tq, ld)
        q = k = v = buf
        hs = 3 * D if case.layout == "legacy" else D
        offs = (0, D, 2 * D) if case.layout == "legacy" else (0, Cc, 2 * Cc)
        lds = [(ld, hs)] * 3
    else:
        assert case.layout == "kv"
        q, k = nan(N * Tq, Cc + 8), nan(N * Tkv, 2 * Cc + 16)
        v = k
        offs = (0, 0, Cc)
        lds = [(Cc + 8, D), (2 * Cc + 16, D), (2 * Cc + 16, D)]
    ldo = Cc + 8
    out = torch.full(((N * Tq + 3) * ldo,), SENTINEL, dtype=dt)
    p = Packed(q, k, v, out, lds[0], lds[1], lds[2], (ldo, D), *offs)
    shadow.attention_view(p.q, N, Tq, H, D, *p.ld_hs_q, p.q_off).copy_(inp.q)
    shadow.attention_view(p.k, N, Tkv, H, D, *p.ld_hs_k, p.k_off).copy_(inp.k)
    shadow.attention_view(p.v, N, Tkv, H, D, *p.ld_hs_v, p.v_off).copy_(inp.v)
    return p


def out_view(case: Case, out: torch.Tensor) -> torch.Tensor:
    return shadow.attention_view(out, case.N, case.Tq, case.heads, case.D, case.heads * case.D + 8, case.D, 0)


def stray_writes(case: Case, out: torch.Tensor) -> int:
    """elements outside the (n, t, h, d) slots of the output buffer that no longer hold the sentinel"""
    o = out.clone()
    out_view(case, o).fill_(SENTINEL)
    return int((_bits(o) != _bits(torch.full_like(o, SENTINEL))).sum())


def check_output(case: Case, inp: Inputs, out: torch.Tensor) -> str:
    """'' or what is wrong with the output buffer of a launch"""
    msg = mismatches(out_view(case, out), inp.want.to(out.device))
    n = stray_writes(case, out)
    if n:
        msg += f" {n} elements outside the output slots were written"
    return msg.strip()


def launch(case: Case, p: Packed, scale: float, workspace: bool = True) -> None:
    """ops.attention, or the raw descriptor without a workspace (the unsplit fallback of a key-split shape)"""
    from jointimagegeneration_amd import _lib, ops
    if workspace:
        ops.attention(p.q, p.k, p.v, p.out, case.N, case.heads, case.D, case.Tq, case.Tkv, p.ld_hs_q, p.ld_hs_k, p.ld_hs_v, p.ld_hs_o,
                      scale, q_off=p.q_off, k_off=p.k_off, v_off=p.v_off)
        return
    d = _desc(case)
    d.ldq, d.hsq = p.ld_hs_q
    d.ldk, d.hsk = p.ld_hs_k
    d.ldv, d.hsv = p.ld_hs_v
    d.ldo, d.hso = p.ld_hs_o
    d.scale = scale
    d.q, d.k, d.v = p.q.data_ptr() + 2 * p.q_off, p.k.data_ptr() + 2 * p.k_off, p.v.data_ptr() + 2 * p.v_off
    d.out = p.out.data_ptr()
    d.workspace, d.workspace_bytes = None, 0
    _lib.check(_lib.load().gg_attention_forward(C.byref(d), ops._stream()), "gg_attention_forward")


# ------------------------------------------------------------------------------------------------ kernel emulation
DEFECTS = ("drop_key", "drop_key_16q", "mask_off_by_one", "v_shift16", "swap_merge", "skip_rescale", "head_slip", "no_inv_l", "untouched_row")


def _exp2(x: torch.Tensor) -> torch.Tensor:
    return torch.exp2(x.float())


def _state(q, k, v, sl2: float, kbeg: int, kend: int, step: int, dma: bool, defect, key: int):
    """online-softmax state (o [Tq, D], m [Tq], l [Tq]) of the keys [kbeg, kend) in steps of `step` keys, as one wave group walks them"""
    Tq, Tkv = q.shape[0], k.shape[0]
    o = torch.zeros(Tq, q.shape[1])
    m = torch.full((Tq,), -math.inf)
    l = torch.zeros(Tq)
    for k0 in range(kbeg, kend, step):
        idx = torch.arange(k0, k0 + step)
        live = idx < kend
        if defect == "mask_off_by_one" and kend == Tkv:
            live = idx <= kend                                    # the first pad row counts
        if not bool(live.any()):
            break
        src = idx.clamp(max=Tkv - 1)                              # LDS-DMA: rows past the end re-read the last key
        kk, vsrc = k[src], (src ^ 16 if defect == "v_shift16" else src)
        vv = v[vsrc.clamp(max=Tkv - 1)]
        if not dma:                                               # register staging: rows past the end are zero filled
            kk = torch.where((idx < Tkv)[:, None], kk, torch.zeros_like(kk))
            vv = torch.where((idx < Tkv)[:, None], vv, torch.zeros_like(vv))
        s = q @ kk.t()
        s = torch.where(live[None, :], s, torch.full_like(s, -math.inf))
        m_new = torch.maximum(m, s.amax(1) * torch.tensor(sl2))
        alpha = _exp2(m - m_new)
        p = _exp2((s.double() * sl2 - m_new.double()[:, None]).float())          # fma: one rounding
        if defect in ("drop_key", "drop_key_16q") and k0 <= key < k0 + step:
            rows = slice(None) if defect == "drop_key" else slice(16, 32)
            p[rows, key - k0] = 0
        l = l * alpha + p.sum(1)
        pv = p.to(torch.bfloat16).float() @ vv
        o = (o if defect == "skip_rescale" else o * alpha[:, None]) + pv
        m = m_new
    return o, m, l


def _merge(states, defect):
    """attn_merge_kernel / the two-half merge: sum_s w_s o_s, sum_s w_s l_s with w_s = 2^(m_s - max m)"""
    mm = torch.stack([s[1] for s in states]).amax(0)
    w = [_exp2(s[1] - mm) for s in states]
    if defect == "swap_merge":
        w = w[1:] + w[:1]
    o = sum(s[0] * ww[:, None] for s, ww in zip(states, w))
    l = sum(s[2] * ww for s, ww in zip(states, w))
    return o, mm, l


def emulate_head(q, k, v, scale: float, plan, workspace: bool = True, defect: Optional[str] = None, key: int = -1) -> torch.Tensor:
    """fp32 emulation of attn_kernel (+ attn_merge_kernel) on one head: q [Tq, D], k / v [Tkv, D] -> [Tq, D] in the input dtype"""
    KT, ks, ws2, dma = plan
    dt, (q, k, v) = q.dtype, (t.float() for t in (q, k, v))
    Tkv = k.shape[0]
    sl2 = _f32(_f32(scale) * _f32(LOG2E_F32))
    step = min(KT, 128)
    ks = ks if workspace else 1
    kchunk = ((Tkv + ks - 1) // ks + KT - 1) // KT * KT if ks > 1 else Tkv
    states = []
    for sp in range(ks):
        kbeg = sp * kchunk
        kend = kbeg + kchunk if (ks > 1 and kbeg + kchunk < Tkv) else Tkv
        ntile = max((kend - kbeg + KT - 1) // KT, 0) if kend > kbeg else 0
        if ws2:
            ntile = (ntile + 1) >> 1
            halves = []
            for grp in (0, 1):
                kb = kbeg + grp * ntile * KT
                halves.append(_state(q, k, v, sl2, kb, min(kb + ntile * KT, kend), step, dma, defect, key))
            states.append(_merge(halves, defect))
        else:
            states.append(_state(q, k, v, sl2, kbeg, kend, step, dma, defect, key))
    o, _, l = _merge(states, defect) if ks > 1 else states[0]
    out = o if defect == "no_inv_l" else o * (1.0 / l)[:, None]
    return out.to(dt)


def emulate(case: Case, p: Packed, scale: float, plan=None, workspace: bool = True, defect: Optional[str] = None, key: int = -1) -> torch.Tensor:
    """the launch on the packed buffers: a copy of the output buffer as the kernel would leave it"""
    plan = case.plan if plan is None else plan
    N, H, D, Tq, Tkv = case.N, case.heads, case.D, case.Tq, case.Tkv
    qv = shadow.attention_view(p.q, N, Tq, H, D, *p.ld_hs_q, p.q_off)
    kv = shadow.attention_view(p.k, N, Tkv, H, D, *p.ld_hs_k, p.k_off)
    hsv = p.ld_hs_v[1] + (8 if defect == "head_slip" else 0)
    vv = shadow.attention_view(p.v, N, Tkv, H, D, p.ld_hs_v[0], hsv, p.v_off)
    out = p.out.clone()
    ov = out_view(case, out)
    for n in range(N):
        for h in range(H):
            r = emulate_head(qv[n, :, h], kv[n, :, h], vv[n, :, h], scale, plan, workspace, defect, key if (n, h) == (0, 0) else -1)
            rows = Tq - 1 if (defect == "untouched_row" and (n, h) == (N - 1, H - 1)) else Tq
            ov[n, :rows, h] = r[:rows]
    return out


# ------------------------------------------------------------------------------------------------ peaked leg
def peaked(case: Case, seed: int = 0) -> Inputs:
    """random q / k / v whose scores have standard deviation SIGMA on a ramp of RAMP per key tile shared by all queries"""
    N, H, D, Tq, Tkv = case.N, case.heads, case.D, case.Tq, case.Tkv
    g = torch.Generator().manual_seed(1000 + seed)
    u = torch.randn(D, generator=g, dtype=torch.float64)
    u /= u.norm()
    orth = lambda x: x - (x @ u)[..., None] * u
    alpha = 16.0
    ramp = RAMP * (torch.arange(Tkv) // case.KT).double()                             # score units: a step per key tile
    q = SIGMA * orth(torch.randn(N, Tq, H, D, generator=g, dtype=torch.float64)) + alpha * u
    k = orth(torch.randn(N, Tkv, H, D, generator=g, dtype=torch.float64)) + (ramp * math.sqrt(D) / alpha)[None, :, None, None] * u
    v = torch.randn(N, Tkv, H, D, generator=g)
    inp = Inputs(q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16), torch.zeros(0), torch.zeros(0), torch.zeros(0), case.scale)
    # preconditions on the stored values: every query's tile max rises from tile to tile; the random part has the stated spread
    for n in range(N):
        for h in range(H):
            s = (inp.q[n, :, h].double() @ inp.k[n, :, h].double().t()) * case.scale
            tiles = [s[:, t0:t0 + case.KT].amax(1) for t0 in range(0, Tkv, case.KT)]
            for a, b in zip(tiles[:-1], tiles[1:]):
                assert bool((b > a).all()), "peaked: a tile max does not rise"
            sd = float((s - ramp[None, :]).std())
            assert 0.75 * SIGMA <= sd <= 8.0, sd
    return inp


def peaked_ratio(case: Case, inp: Inputs, out: torch.Tensor) -> float:
    dev = out.device
    return shadow.attention_ratio(inp.q.to(dev), inp.k.to(dev), inp.v.to(dev), out_view(case, out), case.scale)
