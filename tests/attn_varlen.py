"""Exact-arithmetic inputs for attention with per-sample key lengths (gg_attention_forward_kvlen), on top of tests/attn_exact.py.

One launch carries N samples of different lengths L_n <= Tkv_max with Tq = Tkv_max queries each.  Sample n holds the sel / grp / uni
inputs of attn_exact.build at Tkv = L_n (a sample of length 1 has only the sel regime and uses it under every name) in the first L_n
rows of its K / V block of Tkv_max rows.  The rows from L_n on are POISON: K row j is a copy of key j mod L_n, a key of some query's
target group (of every query's in uni), so it would score exactly 0 and get weight 1 if the kernel saw it; its V row is the sentinel,
12352.  A kernel that sees one poison key for a query moves that output from |out| <= 12 by thousands.  The output must equal the closed
form of length L_n bit for bit.  Rows nobody addresses are NaN (inputs) or the sentinel (output), as in attn_exact.pack.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Tuple

import torch

import attn_exact as X
import shadow


@dataclass(frozen=True)
class VCase:
    name: str
    D: int
    Tkv_max: int
    lengths: Tuple[int, ...]
    heads: int

    @property
    def N(self):
        return len(self.lengths)

    @property
    def Tq(self):
        return self.Tkv_max

    def sample(self, n: int) -> X.Case:
        return X.Case(f"{self.name}_L{self.lengths[n]}", "plain", self.D, self.Tq, self.lengths[n], N=1, heads=self.heads, layout="kv")

    def full(self) -> X.Case:
        return X.Case(self.name + "_full", "plain", self.D, self.Tq, self.Tkv_max, N=self.N, heads=self.heads, layout="kv")


# KT = 64 at D = 64, 256 at D = 32: lengths of one key, one below / at / one above a tile, and the whole buffer
CASES: List[VCase] = [
    VCase("d64_t130", 64, 130, (1, 63, 64, 65, 130), 2),
    VCase("d64_t192_n2h3", 64, 192, (64, 129), 3),
    VCase("d32_t300", 32, 300, (1, 255, 256, 257, 300), 2),
]
F32_CASES: List[VCase] = [VCase("f32_d32_t300", 32, 300, (1, 255, 256, 257, 300), 2)]


@dataclass
class VPacked:
    q: torch.Tensor
    kv: torch.Tensor
    out: torch.Tensor
    want: torch.Tensor            # [N, Tq, heads, D]
    ld_hs_q: Tuple[int, int]
    ld_hs_kv: Tuple[int, int]
    ld_hs_o: Tuple[int, int]
    v_off: int
    scale: float


def build(case: VCase, regime: str, dev, dtype=torch.bfloat16, scale=None) -> VPacked:
    N, H, D, Tq, Tm = case.N, case.heads, case.D, case.Tq, case.Tkv_max
    Cc = H * D
    ldq, ldkv, ldo = Cc + 8, 2 * Cc + 16, Cc + 8
    q = torch.full(((N * Tq + 2) * ldq,), float("nan"), dtype=dtype)
    kv = torch.full(((N * Tm + 2) * ldkv,), float("nan"), dtype=dtype)
    out = torch.full(((N * Tq + 3) * ldo,), X.SENTINEL, dtype=dtype)
    qv = shadow.attention_view(q, N, Tq, H, D, ldq, D, 0)
    kview = shadow.attention_view(kv, N, Tm, H, D, ldkv, D, 0)
    vview = shadow.attention_view(kv, N, Tm, H, D, ldkv, D, Cc)
    want = torch.zeros(N, Tq, H, D, dtype=dtype)
    used_scale = None
    for n, L in enumerate(case.lengths):
        sc = case.sample(n)
        inp = X.build(sc, regime if regime in sc.regimes() else "sel", dtype=dtype, scale=scale)
        X.check_reference(regime if regime in sc.regimes() else "sel", inp, X.reference(inp, dev))
        used_scale = inp.scale
        qv[n], want[n] = inp.q[0], inp.want[0]
        kview[n, :L], vview[n, :L] = inp.k[0], inp.v[0]
        src = torch.arange(L, Tm) % L
        kview[n, L:] = inp.k[0][src]                       # a live key's row: scores exactly 0 for that key's queries
        vview[n, L:] = X.SENTINEL
    assert not bool(torch.isnan(kview).any()) and not bool(torch.isnan(vview).any()) and not bool(torch.isnan(qv).any())
    return VPacked(q.to(dev), kv.to(dev), out.to(dev), want, (ldq, D), (ldkv, D), (ldo, D), Cc, used_scale)


def launch(case: VCase, p: VPacked, kv_len, out=None) -> torch.Tensor:
    """ops.attention into a fresh copy of the sentinel-filled output buffer; kv_len: int32 device tensor [N], or None for the plain entry"""
    from jointimagegeneration_amd import ops
    out = p.out.clone() if out is None else out
    ops.attention(p.q, p.kv, p.kv, out, case.N, case.heads, case.D, case.Tq, case.Tkv_max, p.ld_hs_q, p.ld_hs_kv, p.ld_hs_kv, p.ld_hs_o,
                  p.scale, q_off=0, k_off=0, v_off=p.v_off, kv_len=kv_len)
    torch.cuda.synchronize()
    return out


def check_output(case: VCase, p: VPacked, out: torch.Tensor) -> str:
    full = case.full()
    msg = X.mismatches(X.out_view(full, out), p.want.to(out.device))
    n = X.stray_writes(full, out)
    if n:
        msg += f" {n} elements outside the output slots were written"
    return msg.strip()
