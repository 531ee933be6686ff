"""Exact-arithmetic GroupNorm / LayerNorm checks: inputs on which every fp32 operation of the norm kernels (csrc/gg_norm.hip, the
LayerNorm of padded rows in csrc/gg_cond.hip, the fp32 validation norms in csrc/gg_f32.hip) is exact, the closed-form result,
comparators without a tolerance, a packer with guarded buffers, and an fp32 emulation of every kernel's walk into which defects can
be injected.

Regime E ("two-level").  Channels-last bf16 x, 32 groups.  Every (sample n, group g) has a spread s in {1/4, 1/2, 1, 2} and a centre
m = +-64 s, both cycling with n + g, so that neighbouring groups and neighbouring samples differ in sign and in spread.  Exactly half
of the group's cnt = S * cpg elements are m - s, the other half m + s (a seeded random half): cnt must be even.  63 s and 65 s are
bf16-exact.  Then
    sum = cnt m,   sumsq = cnt (m^2 + s^2),   mean = m,   var = s^2,   (x - mean) / sqrt(var) = +-1
and every fp32 partial sum is exact while one fp32 accumulator sees at most 3970 elements (3970 * 65^2 < 2^24): max_terms() derives
that count from the kernel's walk and build() asserts it.  The same sums are multiples of the fixed-point quanta 2^-28 / 2^-20 of the
conv accumulators.  mean and var come out as exactly m and s^2 after the fp64 fold and the cast to fp32: the Newton-corrected
reciprocal of cnt is ~4e-15 off, times (m / s)^2 = 4096 that is far below half an fp32 ulp.

gamma is from +-{1/2, 3/4, 1, 3/2, 2}, beta a multiple of 1/4 up to 1 in size, a different pair on neighbouring channels, and only
pairs with |+-gamma + beta| >= 1/4 are used (an output that should be exactly 0 does not survive eps != 0 or an inexact v_rsq_f32).
The output is +-gamma + beta, exact in bf16; with eps = 1e-5 or v_rsq_f32 off by an ulp the fp32 value moves by at most
eps / (2 s^2) + 2^-22 relative, far from any bf16 rounding boundary of these few-bit values.

SiLU legs: the expected value is bf16(fp64 SiLU(+-gamma + beta)).  palette(act=True) keeps only pairs for which the fp64 SiLU of
t +- (|t| d + 2^-23 * 65 |gamma|) rounds to the same bf16, d = eps / (2 s^2) + 2^-20 at the largest eps and the smallest s (the second
term: the fp32 roundings of x * scale and of beta - m * scale, both of size 64 |gamma|, when scale is not dyadic), and whose SiLU
lies at least 0.05 bf16 ulp from a rounding midpoint: of the 24 output values 2.0 and -1.25 go.  A violated
precondition is an error of the test, never a skip.

The fp32 tables (scale, shift) depend on v_rsq_f32, whose result on powers of 4 is a hardware fact; they get a derived allowance:
    |scale - fl32(gamma / sqrt(s^2 + eps))| <= 2 ulp       (1 the instruction, 1/4 the rounded argument, 1/2 the product)
    |shift - (beta - m scale_ref)| <= 2^-21 (|beta| + |m scale_ref|)
Pad lanes [C_logical, C) of tables and outputs must be exactly 0 and the 256 guard elements on either side of every output untouched.

LayerNorm: a row has C / 2 elements m - s and C / 2 elements m + s, (m, s) cycling with the row: mean = m, the centred sum of squares
is C s^2, the output +-gamma + beta.

fp32 validation norms (gn_f32_stats + gn_f32_apply / _film): fp64 statistics, IEEE division and square root, then
(x - mean) * rstd, * gamma + beta, * (1 + f) + t, every step rounded to fp32 in that order (gg_f32.hip, contraction off).  With
eps = 0 and dyadic FiLM terms every step is exact: the fp32 output equals the closed form bit for bit and no term has to be dropped.
SiLU in fp32 is not exact (expf): the fp32 cases run with act off.

Regime R (what E cannot express: odd cnt, odd LayerNorm widths, generic data): random bf16 data with a mean-to-std ratio of 0 and of
200, the fp64 reference of tests/shadow.py on the stored values and ITS bounds (coeff_ratio, apply_ratio, layernorm_ratio) <= 1.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

import shadow

GROUPS = 32
SPREADS = (0.25, 0.5, 1.0, 2.0)
RATIO = 64.0
GAMMAS = tuple(sg * v for v in (0.5, 0.75, 1.0, 1.5, 2.0) for sg in (1.0, -1.0))
BETAS = (0.0, 0.25, -0.25, 0.5, -0.5, 0.75, -0.75, 1.0, -1.0)
FLOOR = 0.25
SILU_MARGIN = 0.05                  # bf16 ulp between SiLU(+-gamma + beta) and a rounding midpoint (2.0: 0.016, -1.25: 0.028, all others >= 0.075)
EPS = (0.0, 1e-5)
SENTINEL = 12352.0                  # bf16-exact; no regime produces it
GUARD = 256                         # sentinel elements on either side of every buffer
MAX_TERMS = 3970                    # 3970 * 65^2 < 2^24
ACC_STRIPES = 1                     # GG_ACC_STRIPES (gg_conv.h): the layout gg_groupnorm_apply_acc reads
ACC_SUM_SCALE, ACC_SQ_SCALE = 2.0 ** 28, 2.0 ** 20
I64_POISON = 1 << 60


def _f32(x: float) -> torch.Tensor:
    return torch.tensor(x, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ host gates (Python mirrors)
def magic_u32(nmax: int, d: int) -> int:
    """gg_magic_u32 (gg_common.h)"""
    return ((1 << 32) + d - 1) // d if (d > 1 and nmax * d < (1 << 32)) else 0


def stats_kernel(S: int, C_: int) -> str:
    """gg_groupnorm_stats (gg_norm.hip, the gate in front of gn_stats_small_kernel): the single-launch statistics kernel up to S * C == 2^19"""
    return "small" if S * C_ <= (1 << 19) else "partial"


def gn_nblk(N: int, S: int) -> int:
    """gn_nblk (gg_norm.hip)"""
    want, maxb = (2048 + N - 1) // N, (S + 63) // 64
    return max(1, min(want, maxb, 1024))


def fused_np(C_: int) -> int:
    cpg = C_ // 32
    return max((((g + 1) * cpg - 1) >> 3) - ((g * cpg) >> 3) + 1 for g in range(32))


def fused_small_ok(S: int, C1: int, C2: int, c_log: int) -> bool:
    """gn_fused_small_ok + the checks of gg_groupnorm_fused_supported (gg_norm.hip)"""
    C_ = C1 + C2
    if not (C1 > 0 and C1 % 32 == 0 and C2 >= 0 and C2 % 32 == 0):
        return False
    if c_log != C_ or C_ % 32 or C_ // 32 > 64 or S > (1 << 20):
        return False
    return S * fused_np(C_) <= 512


def apply_acc_kernel(N: int, S: int, C_: int, c_log: int) -> str:
    """gg_groupnorm_apply_acc (gg_norm.hip, its gate between the two kernels): lean<CPT> (one piece per thread) or the general kernel"""
    pieces = S * (C_ // 8)
    blocks = min(max((pieces + 255) // 256, 1), 4096)
    pm = magic_u32(pieces, C_ // 8)
    if blocks * 256 >= pieces and N * S * C_ < (1 << 31) and (pm != 0 or C_ == 8) and C_ // 8 > 1:
        return "lean1" if c_log <= 256 else "lean2" if c_log <= 512 else "lean4" if c_log <= 1024 else "lean8"
    return "general"


# ------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    name: str
    path: str                 # small | partial | fused | lean1 | lean2 | lean4 | lean8 | general | ssacc | f32 | film
    C1: int
    sp: Tuple[int, ...]
    C2: int = 0
    c_log: int = 0            # 0: all channels
    Ns: Tuple[int, ...] = (1, 3)
    stripes: Tuple[int, int] = (1, 1)
    swz: Optional[bool] = None          # lean: the grid is a multiple of 8 blocks (XCD block swizzle)

    @property
    def C(self):
        return self.C1 + self.C2

    @property
    def clog(self):
        return self.c_log or self.C

    @property
    def S(self):
        return math.prod(self.sp)

    @property
    def cpg(self):
        return self.clog // GROUPS

    @property
    def cnt(self):
        return self.S * self.cpg


def _c(path, C1, sp, **kw):
    C_ = C1 + kw.get("C2", 0)
    cl = f"_l{kw['c_log']}" if kw.get("c_log") else ""
    nm = f"{path}_c{C1}" + (f"p{kw['C2']}" if kw.get("C2") else "") + cl + "_" + "x".join(str(s) for s in sp)
    if path == "ssacc":
        nm += f"_st{kw['stripes'][0]}_{kw['stripes'][1]}"
    return Case(nm, path, C1, tuple(sp), **kw)


CASES: List[Case] = [
    # ---- gn_stats_small + gn_apply
    _c("small", 32, (1, 2)), _c("small", 64, (1, 1)), _c("small", 64, (2, 3, 5)), _c("small", 160, (8, 8)), _c("small", 160, (2, 3)),
    _c("small", 320, (7, 9)), _c("small", 800, (4, 4)), _c("small", 1440, (8, 8)), _c("small", 1600, (4, 4)),
    _c("small", 2048, (16, 16)),                                   # S * C == 2^19: the last size on this path
    _c("small", 32, (3, 3), C2=32), _c("small", 320, (2, 3), C2=160),
    _c("small", 160, (2, 3), C2=320),                              # cpg = 15: group 10 straddles the source boundary
    _c("small", 192, (2, 3), c_log=160),                           # pad lanes [160, 192)
    # ---- gn_partial + gn_finalize
    _c("partial", 2048, (1, 257)),                                 # first size past the gate; P = 256, rpi = 1
    _c("partial", 160, (58, 58)),                                  # P = 20, rpi = 12, 16 idle threads, ragged last block
    _c("partial", 64, (362, 363), Ns=(1,)),                        # nblk capped at 1024; finalize loops past 1024 partials
    _c("partial", 32, (74, 74), C2=64),                            # cpg = 3, straddle at 32
    # ---- gn_fused_small
    _c("fused", 64, (1, 1)), _c("fused", 160, (7, 8)), _c("fused", 320, (8, 16)), _c("fused", 640, (8, 8)), _c("fused", 800, (4, 4)),
    _c("fused", 1440, (8, 8)), _c("fused", 1600, (4, 4)),
    _c("fused", 2048, (8, 8)),                                     # S * np == 512: the gate's edge
    _c("fused", 320, (8, 8), C2=320), _c("fused", 160, (6, 6), C2=320),
    # ---- gn_apply_acc_lean<CPT>: per CPT one grid that is a multiple of 8 blocks (swizzled) and one that is not; dead tails
    _c("lean1", 160, (10, 10), swz=True), _c("lean1", 160, (5, 6), swz=False),
    _c("lean2", 320, (5, 10), swz=True), _c("lean2", 320, (2, 5), swz=False),
    _c("lean4", 640, (4, 6), swz=True), _c("lean4", 640, (1, 5), swz=False),
    _c("lean8", 1440, (2, 5), swz=True), _c("lean8", 1440, (2, 2), swz=False),
    _c("lean8", 2048, (2, 4), swz=True), _c("lean8", 2048, (1, 3), swz=False),
    _c("lean2", 160, (2, 17), C2=320, swz=True), _c("lean2", 320, (2, 3), C2=160, swz=False),
    _c("lean1", 192, (4, 5), c_log=160, swz=False),
    # ---- gn_apply_acc (general): more than 2^20 pieces
    _c("general", 64, (362, 363), Ns=(2,)),
    # ---- gn_scale_shift_acc (tables only)
    _c("ssacc", 96, (2, 3), C2=64, stripes=(1, 1)), _c("ssacc", 96, (2, 3), C2=64, stripes=(32, 32)), _c("ssacc", 96, (2, 3), C2=64, stripes=(32, 1)),
    _c("ssacc", 2048, (2, 3), stripes=(1, 1)), _c("ssacc", 2048, (2, 3), stripes=(32, 32)),
    _c("ssacc", 160, (2, 3), C2=320, stripes=(1, 1)), _c("ssacc", 160, (2, 3), C2=320, stripes=(32, 32)), _c("ssacc", 160, (2, 3), C2=320, stripes=(32, 1)),
    _c("ssacc", 192, (2, 3), c_log=160, stripes=(32, 32)),
    # ---- fp32 validation norms
    _c("f32", 64, (2, 3)), _c("f32", 160, (2, 3), C2=320), _c("f32", 192, (3, 4), c_log=160), _c("f32", 320, (7, 10)),
    _c("film", 160, (2, 3)), _c("film", 192, (3, 4), c_log=160), _c("film", 320, (7, 10)),
]
CASE: Dict[str, Case] = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)
BF16_PATHS = ("small", "partial", "fused", "lean1", "lean2", "lean4", "lean8", "general", "ssacc")

# one step past each edge of gn_fused_small_ok: (S, C1, C2, C_logical)
FUSED_PAST_EDGE = [(65, 2048, 0, 2048), (257, 160, 0, 160), (171, 640, 0, 640), (1, 2080, 0, 2080), (4, 192, 0, 160), (4, 48, 0, 48),
                   (171, 160, 320, 480), (513, 32, 0, 32)]
FUSED_ON_EDGE = [(64, 2048, 0, 2048), (256, 160, 0, 160), (170, 640, 0, 640), (1, 2048, 0, 2048), (170, 160, 320, 480)]

LN_WIDTHS = (8, 64, 320, 520, 1024, 2048)           # 520: P = 65, lane 0 alone holds a second piece
LN_ROWS = (1, 3, 4, 5, 150)
LNR_SHAPES = ((2, 32), (6, 32), (50, 64), (70, 96), (130, 160))      # (C, stride)
LNR_ROWS = (1, 5)
R_SHAPES = ((3, 160, 0, (7, 9)), (1, 800, 0, (3, 3)), (2, 160, 320, (5, 5)))       # (N, C1, C2, spatial)
R_LN = ((77, 96), (33, 64))                          # odd widths: (C, stride) through layernorm_rows
R_RATIOS = (0.0, 200.0)


def kernel_of(case: Case, N: int) -> str:
    """the kernel the host gates send the case's shape to"""
    if case.path in ("small", "partial"):
        return stats_kernel(case.S, case.C)
    if case.path == "fused":
        return "fused" if fused_small_ok(case.S, case.C1, case.C2, case.clog) else "refused"
    if case.path.startswith("lean") or case.path == "general":
        return apply_acc_kernel(N, case.S, case.C, case.clog)
    return case.path


def lean_blocks(case: Case) -> int:
    return (case.S * (case.C // 8) + 255) // 256


def assert_path(case: Case, N: int) -> None:
    got = kernel_of(case, N)
    assert got == case.path, f"{case.name} N={N}: the shape no longer reaches {case.path}: {got}"
    if case.path == "fused":
        from jointimagegeneration_amd import _lib
        assert _lib.load().gg_groupnorm_fused_supported(case.S, case.C1, case.C2, case.clog) == 1, case.name
    if case.swz is not None:
        pieces = case.S * (case.C // 8)
        assert (lean_blocks(case) % 8 == 0) == case.swz, (case.name, lean_blocks(case))
        assert pieces % 256 or case.C == 2048, f"{case.name}: no dead tail in the last block"


def max_terms(case: Case, N: int) -> int:
    """the most elements any one fp32 accumulator of the case's statistics walk sees"""
    k = case.path
    if k in ("small", "fused"):
        cpg = case.cpg
        np_ = max((((g + 1) * cpg - 1) >> 3) - ((g * cpg) >> 3) + 1 for g in range(32))
        return (case.S * np_ + 255) // 256 * 8                    # per thread: its pieces, 8 lanes each (masked lanes add 0)
    if k == "partial":
        nblk = gn_nblk(N, case.S)
        return (case.S + nblk - 1) // nblk                        # per (block, channel): the block's rows
    return 0                                                      # integer accumulators / fp64 statistics


# ------------------------------------------------------------------------------------------------ inputs
_PALETTE: Dict[bool, List[Tuple[float, float]]] = {}


def _silu64(t: torch.Tensor) -> torch.Tensor:
    return t / (1.0 + torch.exp(-t))


def palette(act: bool) -> List[Tuple[float, float]]:
    """the (gamma, beta) pairs in use: |+-gamma + beta| >= 1/4; with SiLU both outputs away from a bf16 rounding boundary"""
    if act in _PALETTE:
        return _PALETTE[act]
    d = max(EPS) / (2.0 * min(SPREADS) ** 2) + 2.0 ** -20
    out = []
    for gm in GAMMAS:
        for bt in BETAS:
            ok = True
            for t in (gm + bt, -gm + bt):
                if abs(t) < FLOOR:
                    ok = False
                elif act:
                    e = abs(t) * d + 2.0 ** -23 * 65.0 * abs(gm)
                    r = _silu64(torch.tensor([t - e, t, t + e], dtype=torch.float64)).to(torch.bfloat16)
                    z = _silu64(torch.tensor(t, dtype=torch.float64))
                    ulp = 2.0 ** (math.floor(math.log2(abs(float(z)))) - 7)
                    margin = 0.5 - abs(float(z) - float(z.to(torch.bfloat16))) / ulp          # distance from a rounding midpoint, bf16 ulp
                    ok = ok and bool((r == r[1]).all()) and margin >= SILU_MARGIN
            if ok:
                out.append((gm, bt))
    assert len(out) >= 32, len(out)
    _PALETTE[act] = out
    return out


def _stride(n: int) -> int:
    s = 7
    while math.gcd(s, n) != 1:
        s += 1
    return s


def coefficients(clog: int, act: bool, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    pal = palette(act)
    idx = (torch.arange(clog) * _stride(len(pal)) + 3 + seed) % len(pal)
    pt = torch.tensor(pal, dtype=torch.float32)
    g, b = pt[idx, 0].clone(), pt[idx, 1].clone()
    assert bool(((g[1:] != g[:-1]) | (b[1:] != b[:-1])).all())              # neighbouring channels differ
    return g, b


def _half_signs(gen: torch.Generator, lead: Tuple[int, ...], cnt: int) -> torch.Tensor:
    """[*lead, cnt] of +-1, exactly half of each along the last axis, a random half"""
    assert cnt % 2 == 0, f"regime E needs an even element count, got {cnt}"
    rank = torch.rand(lead + (cnt,), generator=gen).argsort(-1).argsort(-1)
    return torch.where(rank < cnt // 2, -1.0, 1.0)


def centres(N: int, G: int = GROUPS, off: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(m, s) fp64 [N, G]: both cycle with n + g"""
    k = torch.arange(N)[:, None] + torch.arange(G)[None, :] + off
    s = torch.tensor(SPREADS, dtype=torch.float64)[k % 4]
    m = RATIO * s * torch.where(k % 2 == 0, 1.0, -1.0)
    return m, s


@dataclass
class Inputs:
    case: Case
    N: int
    act: bool
    x: torch.Tensor           # [N, S, C] storage dtype (pad lanes 0)
    sgn: torch.Tensor         # int8 [N, S, clog] +-1
    m: torch.Tensor           # fp64 [N, 32]
    s: torch.Tensor
    gamma: torch.Tensor       # fp32 [clog]
    beta: torch.Tensor
    want: torch.Tensor        # [N, S, C] closed form in the storage dtype, pad lanes 0
    film: Optional[torch.Tensor] = None        # fp32 [N, 2 clog + 8]


_X_CACHE: Dict[Tuple[str, int], Tuple[torch.Tensor, torch.Tensor]] = {}


def build(case: Case, N: int, act: bool) -> Inputs:
    S, C_, clog, cpg, cnt = case.S, case.C, case.clog, case.cpg, case.cnt
    f32 = case.path in ("f32", "film")
    assert not (f32 and act), "fp32 SiLU is not exact: the fp32 cases run with act off"
    assert cnt % 2 == 0, f"{case.name}: regime E needs an even S * cpg"
    assert max_terms(case, N) <= MAX_TERMS, f"{case.name}: an fp32 accumulator sees {max_terms(case, N)} > {MAX_TERMS} elements"
    m, s = centres(N)
    if (case.name, N) not in _X_CACHE:
        gen = torch.Generator().manual_seed(((case.C1 * 4099 + case.C2) * 4099 + S) * 8 + N)
        sg = _half_signs(gen, (N, GROUPS), cnt).view(N, GROUPS, S, cpg).permute(0, 2, 1, 3).reshape(N, S, clog)
        rep = lambda v: v.repeat_interleave(cpg, 1)[:, None, :]
        x = torch.zeros(N, S, C_, dtype=torch.float64)
        x[:, :, :clog] = rep(m) + rep(s) * sg
        _X_CACHE.clear()                                                     # the latest case only: the act off / on legs share it
        _X_CACHE[(case.name, N)] = (x, sg)
    x, sg = _X_CACHE[(case.name, N)]
    dt = torch.float32 if f32 else torch.bfloat16
    xs = x.to(dt)
    assert bool((xs.double() == x).all())                                   # exact in the storage type
    # closed-form statistics of the stored values
    xg = x[:, :, :clog].reshape(N, S, GROUPS, cpg)
    assert bool((xg.sum((1, 3)) == cnt * m).all()) and bool(((xg * xg).sum((1, 3)) == cnt * (m * m + s * s)).all())
    gamma, beta = coefficients(clog, act)
    t = sg * gamma.double() + beta.double()
    film = None
    if case.path == "film":
        film = torch.full((N, 2 * clog + 8), float("nan"), dtype=torch.float32)
        k = torch.arange(N)[:, None] + torch.arange(clog)[None, :]
        fs = torch.tensor([0.0, 0.5, -0.5, 1.0, -0.25, 0.25])[k % 6]         # 1 + f in {1, 3/2, 1/2, 2, 3/4, 5/4}
        ft = torch.tensor([0.0, 0.25, -0.5, 1.0, -1.0])[(k * 3) % 5]
        film[:, :clog], film[:, clog:2 * clog] = fs, ft
        t = t * (1.0 + fs.double())[:, None, :] + ft.double()[:, None, :]
    want = torch.zeros(N, S, C_, dtype=torch.float64)
    want[:, :, :clog] = _silu64(t) if act else t
    wd = want.to(dt)
    if not act:
        assert bool((wd.double() == want).all())
        assert film is not None or float(want[:, :, :clog].abs().min()) >= FLOOR
    return Inputs(case, N, act, xs, sg.to(torch.int8), m, s, gamma, beta, wd, film)


def reference(inp: Inputs, eps: float, dev=None) -> torch.Tensor:
    """fp64 GroupNorm(32) (+ FiLM) (+ SiLU) of the stored values: [N, S, C], pad lanes 0"""
    c = inp.case
    x = inp.x.double() if dev is None else inp.x.to(dev).double()
    N, S, clog, cpg = inp.N, c.S, c.clog, c.cpg
    xg = x[:, :, :clog].reshape(N, S, GROUPS, cpg)
    mean = xg.mean((1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean((1, 3), keepdim=True)
    y = ((xg - mean) / torch.sqrt(var + eps)).reshape(N, S, clog) * inp.gamma.double().to(x.device) + inp.beta.double().to(x.device)
    if inp.film is not None:
        f = inp.film.double().to(x.device)
        y = y * (1.0 + f[:, None, :clog]) + f[:, None, clog:2 * clog]
    out = torch.zeros_like(x)
    out[:, :, :clog] = _silu64(y) if inp.act else y
    return out


def check_reference(inp: Inputs, eps: float, dev=None) -> None:
    ref = reference(inp, eps, dev)
    bad = mismatches(ref.to(inp.want.dtype), inp.want.to(ref.device))
    assert not bad, f"{inp.case.name} eps={eps}: the fp64 reference does not round to the closed form: {bad}"


# ------------------------------------------------------------------------------------------------ accumulators
def accumulators(x: torch.Tensor, C0: int, Cn: int, stripes: int, seed: int, exact: bool = True) -> torch.Tensor:
    """int64 [N, stripes, Cn, 2]: the fixed-point per-channel (sum, sumsq) of channels [C0, C0 + Cn) of x [N, S, C], split unevenly
    over the stripes (negative and zero stripes included)"""
    xd = x[:, :, C0:C0 + Cn].double()
    a, b = xd.sum(1) * ACC_SUM_SCALE, (xd * xd).sum(1) * ACC_SQ_SCALE
    if exact:
        assert bool((a == a.round()).all()) and bool((b == b.round()).all()) and float(max(a.abs().max(), b.abs().max())) < 2.0 ** 53
    tot = torch.stack([a.round().long(), b.round().long()], -1)                      # [N, Cn, 2]
    acc = torch.zeros(x.shape[0], stripes, Cn, 2, dtype=torch.int64)
    if stripes > 1:
        gen = torch.Generator().manual_seed(977 + seed)
        acc[:, 1:] = torch.randint(-(1 << 40), 1 << 40, (x.shape[0], stripes - 1, Cn, 2), generator=gen)
        acc[:, 2::3] = 0                                                             # zero stripes
        assert bool((acc < 0).any()) and bool((acc[:, 1:] == 0).all(-1).all(-1).any())
    acc[:, 0] = tot - acc[:, 1:].sum(1)
    assert bool((acc.sum(1) == tot).all())
    return acc


# ------------------------------------------------------------------------------------------------ comparators
def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def mismatches(got: torch.Tensor, want: torch.Tensor, limit: int = 4) -> str:
    """'' if got equals want bit for bit (-0 equals +0, nothing else does), else a description of the first differences"""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    bad = (_bits(got) != _bits(want)) & ~((got == 0) & (want == 0))
    nbad = int(bad.sum())
    if not nbad:
        return ""
    idx = bad.nonzero()[:limit].tolist()
    return f"{nbad} of {bad.numel()} elements differ; first: " + "; ".join(
        f"{tuple(ix)} got {float(got[tuple(ix)])!r} want {float(want[tuple(ix)])!r}" for ix in idx)


def _ulp32(ref: torch.Tensor) -> torch.Tensor:
    """spacing of fp32 at |ref| (fp64 tensors)"""
    r = ref.abs().float()
    return (torch.nextafter(r, torch.full_like(r, math.inf)) - r).double()


def table_reference(inp: Inputs, eps: float):
    """fp64 (scale_ref rounded to fp32, shift_ref) [N, clog] of the closed form"""
    cpg = inp.case.cpg
    rep = lambda v: v.repeat_interleave(cpg, 1)
    e = float(_f32(eps))
    sc = (inp.gamma.double()[None, :] / torch.sqrt(rep(inp.s) ** 2 + e)).float().double()
    sh = inp.beta.double()[None, :] - rep(inp.m) * sc
    return sc, sh


def tables_check(inp: Inputs, eps: float, scale: torch.Tensor, shift: torch.Tensor) -> str:
    """'' or what is wrong with fp32 tables [N, C]: the derived allowance on [0, clog), exactly 0 beyond"""
    clog = inp.case.clog
    sc, sh = table_reference(inp, eps)
    sc, sh = sc.to(scale.device), sh.to(scale.device)
    msg = []
    e1 = (scale[:, :clog].double() - sc).abs() / _ulp32(sc)
    if not bool((e1 <= 2.0).all()):
        i = (~(e1 <= 2.0)).nonzero()[0].tolist()
        msg.append(f"scale {tuple(i)}: got {float(scale[tuple(i)])!r} want {float(sc[tuple(i)])!r} ({float(e1[tuple(i)]):.1f} ulp > 2)")
    bt = inp.beta.double().to(scale.device)[None, :]
    lim = 2.0 ** -21 * (bt.abs() + (bt - sh).abs())
    e2 = (shift[:, :clog].double() - sh).abs()
    if not bool((e2 <= lim).all()):
        i = (~(e2 <= lim)).nonzero()[0].tolist()
        msg.append(f"shift {tuple(i)}: got {float(shift[tuple(i)])!r} want {float(sh[tuple(i)])!r} (limit {float(lim[tuple(i)]):.3g})")
    if bool((scale[:, clog:] != 0).any()) or bool((shift[:, clog:] != 0).any()):
        msg.append("pad lanes of the tables are not 0")
    return "; ".join(msg)


# ------------------------------------------------------------------------------------------------ packer
def guarded(t: torch.Tensor, fill) -> torch.Tensor:
    """flat copy of t with GUARD fill elements on either side"""
    flat = torch.full((t.numel() + 2 * GUARD,), fill, dtype=t.dtype)
    flat[GUARD:GUARD + t.numel()] = t.reshape(-1)
    return flat


def fresh(n: int, dtype, dev=None) -> torch.Tensor:
    """a sentinel-filled output buffer of n elements + guards"""
    return torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)


def body(flat: torch.Tensor) -> torch.Tensor:
    return flat[GUARD:flat.numel() - GUARD]


def ptr(flat: Optional[torch.Tensor]) -> Optional[int]:
    return None if flat is None else flat.data_ptr() + GUARD * flat.element_size()


def guards_intact(flat: torch.Tensor) -> bool:
    s = _bits(torch.full((GUARD,), SENTINEL, dtype=flat.dtype, device=flat.device))
    return bool((_bits(flat[:GUARD]) == s).all()) and bool((_bits(flat[flat.numel() - GUARD:]) == s).all())


@dataclass
class Packed:
    """guarded flat buffers of one case: inputs with NaN guards (int64: a poison value), coefficient pad lanes NaN"""
    N: int
    S: int
    C1: int
    C2: int
    clog: int
    x1: torch.Tensor
    x2: Optional[torch.Tensor]
    gamma: torch.Tensor
    beta: torch.Tensor
    acc1: Optional[torch.Tensor] = None
    acc2: Optional[torch.Tensor] = None
    stripes: Tuple[int, int] = (1, 1)
    film: Optional[torch.Tensor] = None
    film_stride: int = 0

    @property
    def C(self):
        return self.C1 + self.C2

    def to(self, dev):
        mv = lambda t: None if t is None else t.to(dev)
        return Packed(self.N, self.S, self.C1, self.C2, self.clog, mv(self.x1), mv(self.x2), mv(self.gamma), mv(self.beta), mv(self.acc1),
                      mv(self.acc2), self.stripes, mv(self.film), self.film_stride)


def pack_raw(x: torch.Tensor, C1: int, C2: int, clog: int, gamma, beta, stripes=None, exact=True, film=None) -> Packed:
    N, S, C_ = x.shape
    nan = float("nan")
    gm = torch.full((C_,), nan, dtype=torch.float32)
    bt = gm.clone()
    gm[:clog], bt[:clog] = gamma, beta
    p = Packed(N, S, C1, C2, clog, guarded(x[:, :, :C1].contiguous(), nan), guarded(x[:, :, C1:].contiguous(), nan) if C2 else None,
               guarded(gm, nan), guarded(bt, nan))
    if stripes is not None:
        p.stripes = stripes
        p.acc1 = guarded(accumulators(x, 0, C1, stripes[0], 1, exact), I64_POISON)
        if C2:
            p.acc2 = guarded(accumulators(x, C1, C2, stripes[1], 2, exact), I64_POISON)
    if film is not None:
        p.film, p.film_stride = guarded(film, nan), film.shape[1]
    return p


def pack(inp: Inputs) -> Packed:
    c = inp.case
    st = c.stripes if c.path == "ssacc" else (ACC_STRIPES, ACC_STRIPES) if (c.path.startswith("lean") or c.path == "general") else None
    return pack_raw(inp.x, c.C1, c.C2, c.clog, inp.gamma, inp.beta, st, True, inp.film)


@dataclass
class Result:
    out: Optional[torch.Tensor] = None        # guarded flat [N * S * C]
    scale: Optional[torch.Tensor] = None      # guarded flat fp32 [N * C]
    shift: Optional[torch.Tensor] = None


def check_result(inp: Inputs, eps: float, res: Result, tables: bool = True, out: bool = True) -> str:
    """'' or what is wrong with the buffers a launch (or its emulation) left"""
    c, msg = inp.case, []
    if res.out is not None and out:
        bad = mismatches(body(res.out).view(inp.N, c.S, c.C), inp.want.to(res.out.device))
        if bad:
            msg.append("out: " + bad)
        if not guards_intact(res.out):
            msg.append("out: a guard element was written")
    if res.scale is not None and tables:
        bad = tables_check(inp, eps, body(res.scale).view(inp.N, c.C), body(res.shift).view(inp.N, c.C))
        if bad:
            msg.append(bad)
        if not (guards_intact(res.scale) and guards_intact(res.shift)):
            msg.append("tables: a guard element was written")
    return "; ".join(msg)


# ------------------------------------------------------------------------------------------------ launches (GPU)
def launch(path: str, p: Packed, eps: float, act: bool) -> Result:
    """the C entry points of the path on the packed buffers, into fresh sentinel-filled outputs"""
    from jointimagegeneration_amd import _lib, ops
    lib, st, dev = _lib.load(), ops._stream(), p.x1.device
    N, S, C1, C2, C_, clog = p.N, p.S, p.C1, p.C2, p.C, p.clog
    f32 = path in ("f32", "film")
    r = Result()
    if path != "ssacc":
        r.out = fresh(N * S * C_, torch.float32 if f32 else torch.bfloat16, dev)
    if path in ("small", "partial", "ssacc"):
        r.scale, r.shift = fresh(N * C_, torch.float32, dev), fresh(N * C_, torch.float32, dev)
    if path in ("small", "partial"):
        wsb = lib.gg_groupnorm_workspace_bytes(N, S, C_)
        ws = fresh(wsb // 4, torch.float32, dev)
        _lib.check(lib.gg_groupnorm_stats(ptr(p.x1), C1, ptr(p.x2), C2, N, S, clog, ptr(p.gamma), ptr(p.beta), eps, ptr(r.scale), ptr(r.shift),
                                          ptr(ws), wsb, st), "gg_groupnorm_stats")
        _lib.check(lib.gg_groupnorm_apply(ptr(p.x1), C1, ptr(p.x2), C2, N, S, ptr(r.scale), ptr(r.shift), int(act), ptr(r.out), st),
                   "gg_groupnorm_apply")
        assert guards_intact(ws), "the statistics workspace's guards were written"
    elif path == "fused":
        _lib.check(lib.gg_groupnorm_fused(ptr(p.x1), C1, ptr(p.x2), C2, N, S, clog, ptr(p.gamma), ptr(p.beta), eps, int(act), ptr(r.out), st),
                   "gg_groupnorm_fused")
    elif path.startswith("lean") or path == "general":
        _lib.check(lib.gg_groupnorm_apply_acc(ptr(p.x1), C1, ptr(p.acc1), ptr(p.x2), C2, ptr(p.acc2), N, S, clog, ptr(p.gamma), ptr(p.beta), eps,
                                              int(act), ptr(r.out), st), "gg_groupnorm_apply_acc")
    elif path == "ssacc":
        _lib.check(lib.gg_groupnorm_scale_shift_acc(ptr(p.acc1), p.stripes[0], C1, ptr(p.acc2), p.stripes[1] if C2 else 0, C2, N, S, clog,
                                                    ptr(p.gamma), ptr(p.beta), eps, ptr(r.scale), ptr(r.shift), st), "gg_groupnorm_scale_shift_acc")
    elif path == "f32":
        ws = fresh(64 * N, torch.float32, dev)
        _lib.check(lib.gg_groupnorm_f32(ptr(p.x1), C1, ptr(p.x2), C2, N, S, clog, ptr(p.gamma), ptr(p.beta), eps, int(act), ptr(r.out), ptr(ws), st),
                   "gg_groupnorm_f32")
        assert guards_intact(ws)
    elif path == "film":
        ws = fresh(64 * N, torch.float32, dev)
        _lib.check(lib.gg_groupnorm_f32_film(ptr(p.x1), C1, N, S, clog, ptr(p.gamma), ptr(p.beta), eps, ptr(p.film), p.film_stride, int(act),
                                             ptr(r.out), ptr(ws), st), "gg_groupnorm_f32_film")
        assert guards_intact(ws)
    else:
        raise AssertionError(path)
    torch.cuda.synchronize()
    return r


def launch_layernorm(x: torch.Tensor, rows: int, C_: int, stride: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> torch.Tensor:
    """gg_layernorm (stride == C) or gg_layernorm_rows on guarded flat buffers; returns the guarded output"""
    from jointimagegeneration_amd import _lib, ops
    lib = _lib.load()
    out = fresh(rows * stride, torch.bfloat16, x.device)
    if stride == C_ and C_ % 8 == 0:
        _lib.check(lib.gg_layernorm(ptr(x), rows, C_, ptr(gamma), ptr(beta), eps, ptr(out), ops._stream()), "gg_layernorm")
    else:
        _lib.check(lib.gg_layernorm_rows(ptr(x), rows, C_, stride, ptr(gamma), ptr(beta), eps, ptr(out), ops._stream()), "gg_layernorm_rows")
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ kernel emulation
DEFECTS = ("drop_last", "foreign_lane", "group_round", "second_src_at_c", "sample0_stats", "cnt_from_C", "fold_missing", "store_whole",
           "fp32_inv_cnt", "next_row_mean")


def _rcp32(d: int) -> torch.Tensor:
    return _f32(1.0) / _f32(float(d))


def _div_small(n: torch.Tensor, rcp: torch.Tensor) -> torch.Tensor:
    """gg_div_small: (int)(((float)n + 0.5f) * rcp) in fp32"""
    return ((n.float() + _f32(0.5)) * rcp).long()


def _fastdiv(i: torch.Tensor, d: int, magic: int) -> torch.Tensor:
    """gg_fastdiv: __umulhi((unsigned)n, magic), or the plain division without a magic"""
    return (i * magic) >> 32 if magic else i // d


def _wave_sum_f64(x: torch.Tensor) -> torch.Tensor:
    """gg_wave_sum_f64 over the last axis of 64 lanes: quad xor 1, quad xor 2, half-row mirror, row mirror, xor 16, xor 32"""
    l = torch.arange(64)
    for perm in (l ^ 1, l ^ 2, (l & ~7) | (7 - (l & 7)), (l & ~15) | (15 - (l & 15)), l ^ 16, l ^ 32):
        x = x + x[..., perm]
    return x


def _block_sum_f64(a: torch.Tensor) -> torch.Tensor:
    """fp32 per-thread values [..., 256] -> the block total in fp64: wave butterflies, then (w0 + w1) + (w2 + w3)"""
    w = _wave_sum_f64(a.double().reshape(a.shape[:-1] + (4, 64)))[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def _mean_rstd(sa, sb, cnt: float, eps: float, fp64_div: bool = False, defect=None):
    """(fmean, frstd) fp32 from the fp64 sums: fp32 reciprocal of the count + one Newton step in fp64 and rsqrtf, or (gn_finalize,
    gn_f32_stats) an fp64 division and square root"""
    if fp64_div:
        mean = sa / cnt
        var = (sb / cnt - mean * mean).clamp_min(0.0)
        return mean.float(), (1.0 / torch.sqrt(var + float(_f32(eps)))).float()
    inv = float((_f32(1.0) / _f32(cnt)).double())
    if defect != "fp32_inv_cnt":
        inv = inv * (2.0 - cnt * inv)
    mean = sa * inv
    var = (sb * inv - mean * mean).clamp_min(0.0)
    return mean.float(), torch.rsqrt(var.float() + _f32(eps))


def _fma(x, a, b):
    """fp32 fma(x, a, b): the product is exact in fp64 and the sum is rounded once more only below 2^-53"""
    return (x.double() * a.double() + b.double()).float()


def _silu32(t: torch.Tensor) -> torch.Tensor:
    return t * (_f32(1.0) / (_f32(1.0) + torch.exp(-t)))


def _src(p: Packed):
    x1 = body(p.x1).float()
    x2 = body(p.x2).float() if p.x2 is not None else None
    return x1, x2


def _gather(p: Packed, x1, x2, n, r, c, defect=None):
    """the element (n, r, c) of the two-source concat, as the kernels address it"""
    first = c < p.C1
    i1 = ((n * p.S + r) * p.C1 + c).clamp(0, x1.numel() - 1)
    v = x1[torch.where(first, i1, torch.zeros_like(i1))]
    if x2 is not None:
        cc = c if defect == "second_src_at_c" else c - p.C1
        i2 = ((n * p.S + r) * p.C2 + cc) % x2.numel()
        v = torch.where(first, v, x2[torch.where(first, torch.zeros_like(i2), i2)])
    return v


def _group_walk(p: Packed, g: int):
    """gn_stats_small / gn_fused_small: work item i -> (row, first channel of its 16-byte piece), lane mask of the group's channels"""
    cpg = p.clog // 32
    c_lo, c_hi = g * cpg, (g + 1) * cpg
    p_lo, p_hi = c_lo >> 3, (c_hi - 1) >> 3
    np_ = p_hi - p_lo + 1
    i = torch.arange(p.S * np_)
    r = _div_small(i, _rcp32(np_))
    pc = p_lo + (i - r * np_)
    assert bool((r >= 0).all()) and bool((r < p.S).all()) and bool((pc >= p_lo).all()) and bool((pc <= p_hi).all())       # in bounds
    c = (pc * 8)[:, None] + torch.arange(8)[None, :]
    return r, c, (c >= c_lo) & (c < c_hi), c_lo, c_hi


def _stats_walk(p: Packed, eps: float, defect=None):
    """fmean, frstd [N, 32] of gn_stats_small / gn_fused_small: fp32 per thread, fp64 butterfly, Newton reciprocal, rsqrtf"""
    x1, x2 = _src(p)
    N, cpg = p.N, p.clog // 32
    sa, sb = torch.zeros(N, 32, dtype=torch.float64), torch.zeros(N, 32, dtype=torch.float64)
    n = torch.arange(N)[:, None, None]
    for g in range(32):
        r, c, mask, c_lo, c_hi = _group_walk(p, g)
        mask = mask.clone()
        if g == 5 and defect == "drop_last":
            last = mask.nonzero()[-1]
            mask[last[0], last[1]] = False
        if g == 5 and defect == "foreign_lane":
            f = (~mask).nonzero()
            assert len(f), "foreign_lane needs a group that shares a piece"
            mask[f[0][0], f[0][1]] = True
        v = _gather(p, x1, x2, n, r[None, :, None], c[None].clamp(max=p.C - 1), defect)
        v = torch.where(mask[None], v, torch.zeros_like(v))
        work = v.shape[1]
        pad = (-work) % 256
        v = torch.cat([v, torch.zeros(N, pad, 8)], 1).view(N, -1, 256, 8)
        a, b = torch.zeros(N, 256), torch.zeros(N, 256)
        for it in range(v.shape[1]):
            for j in range(8):
                f = v[:, it, :, j]
                a = a + f
                b = _fma(f, f, b)
        sa[:, g], sb[:, g] = _block_sum_f64(a), _block_sum_f64(b)
    cnt = float(p.S * ((p.C if defect == "cnt_from_C" else p.clog) // 32))
    return _mean_rstd(sa, sb, cnt, eps, defect=defect)


def _stats_partial(p: Packed, eps: float, defect=None):
    """gn_partial (fp32 per thread over its rows, fp32 over the row slots) + gn_finalize (fp64 fold, fixed tree, fp64 division / sqrt)"""
    x1, x2 = _src(p)
    N, S, C_, cpg = p.N, p.S, p.C, p.clog // 32
    x = torch.cat([x1.view(N, S, p.C1)] + ([x2.view(N, S, p.C2)] if x2 is not None else []), 2)
    P = C_ >> 3
    rpi, nblk = 256 // P, gn_nblk(N, S)
    rpb = (S + nblk - 1) // nblk
    r0 = torch.arange(nblk)[:, None] * rpb
    r1 = (r0 + rpb).clamp(max=S)
    a = torch.zeros(N, nblk, rpi, C_)
    b = torch.zeros(N, nblk, rpi, C_)
    for k in range((rpb + rpi - 1) // rpi):
        rows = r0 + torch.arange(rpi)[None, :] + k * rpi                             # [nblk, rpi]
        live = rows < r1
        if defect == "drop_last":
            live = live & (rows != S - 1)
        f = x[:, rows.clamp(max=S - 1)] * live[None, :, :, None]
        a = a + f
        b = _fma(f, f, b)
    pa, pb = torch.zeros(N, nblk, C_), torch.zeros(N, nblk, C_)
    for k in range(rpi):
        pa, pb = pa + a[:, :, k], pb + b[:, :, k]
    sa, sb = torch.zeros(N, 32, dtype=torch.float64), torch.zeros(N, 32, dtype=torch.float64)
    for g in range(32):
        va, vb = (t[:, :, g * cpg:(g + 1) * cpg].reshape(N, -1).double() for t in (pa, pb))           # i = k * cpg + j
        if defect == "fold_missing" and g == 5:
            va, vb = va.clone(), vb.clone()
            va[:, cpg + 1], vb[:, cpg + 1] = 0.0, 0.0
        pad = (-va.shape[1]) % 256
        for src, dst in ((va, sa), (vb, sb)):
            t = torch.cat([src, torch.zeros(N, pad, dtype=torch.float64)], 1).view(N, -1, 256).sum(1)          # thread tid: every i = tid mod 256
            s = 128
            while s:
                t = t[:, :s] + t[:, s:2 * s]
                s >>= 1
            dst[:, g] = t[:, 0]
    return _mean_rstd(sa, sb, float(S * cpg), eps, fp64_div=True)


def _stats_acc(p: Packed, eps: float, kind: str, defect=None):
    """the integer fold of the accumulators (lean: per-channel sums, 32 threads add their group's; general: LDS atomics keyed by
    gg_div_small(c); scale_shift: (stripe, channel) pairs over the threads), then the Newton reciprocal and rsqrtf"""
    N, cpg, clog = p.N, p.clog // 32, p.clog
    a1 = body(p.acc1).view(N, p.stripes[0], p.C1, 2)
    cs = a1.sum(1)
    if p.acc2 is not None:
        cs = torch.cat([cs, body(p.acc2).view(N, p.stripes[1], p.C2, 2).sum(1)], 1)
    cs = cs[:, :clog].clone()
    if defect == "fold_missing":
        if kind == "ssacc" and p.stripes[0] > 1:
            cs[:, 5 * cpg] -= a1[:, p.stripes[0] - 1, 5 * cpg]                       # one stripe of one channel
        else:
            cs[:, 5 * cpg + cpg - 1] = 0                                             # one channel
    c = torch.arange(clog)
    g = _div_small(c, _rcp32(cpg)) if kind == "general" else c // cpg
    if kind == "ssacc":                                                              # i -> (stripe k, channel) through gg_div_small
        i = torch.arange(cpg * max(p.stripes))
        k = _div_small(i, _rcp32(cpg))
        assert bool((k == i // cpg).all())
    if defect == "group_round":
        g = g.clone()
        g[7 * cpg] = 6
    tot = torch.zeros(N, 32, 2, dtype=torch.int64).index_add_(1, g, cs)
    assert bool((tot.double().long() == tot).all())                                  # the conversion to fp64 is exact
    sa, sb = tot[:, :, 0].double() * (1.0 / ACC_SUM_SCALE), tot[:, :, 1].double() * (1.0 / ACC_SQ_SCALE)
    cnt = float(p.S * ((p.C if defect == "cnt_from_C" else clog) // 32))
    return _mean_rstd(sa, sb, cnt, eps, defect=defect)


def _tables(p: Packed, fmean, frstd, defect=None, approx_group: bool = False):
    """fp32 scale / shift [N, C]: scale = rstd * gamma, shift = beta - mean * scale; pad lanes 0"""
    cpg = p.clog // 32
    c = torch.arange(p.clog)
    g = _div_small(c, _rcp32(cpg)) if approx_group else c // cpg
    if defect == "sample0_stats":
        fmean, frstd = fmean[:1].expand_as(fmean), frstd[:1].expand_as(frstd)
    gm, bt = body(p.gamma)[:p.clog], body(p.beta)[:p.clog]
    sc = frstd[:, g] * gm
    sh = _fma(-fmean[:, g], sc, bt.expand_as(sc))
    scale, shift = torch.zeros(p.N, p.C), torch.zeros(p.N, p.C)
    scale[:, :p.clog], shift[:, :p.clog] = sc, sh
    return scale, shift


def _store(out: torch.Tensor, idx: torch.Tensor, val: torch.Tensor, mask=None) -> None:
    """stores into the guarded flat output; an index outside the buffer is an error of the emulated kernel"""
    if mask is not None:
        idx, val = idx[mask], val[mask]
    assert bool((idx >= -GUARD).all()) and bool((idx < out.numel() - GUARD).all()), "emulated store outside the allocation"
    out[idx.reshape(-1) + GUARD] = val.reshape(-1).to(out.dtype)


def _affine(x, sc, sh, act: bool):
    t = _fma(x, sc, sh)
    return _silu32(t) if act else t


def _apply_table(p: Packed, scale, shift, act: bool, out: torch.Tensor, per_sample_grid: bool) -> None:
    """gn_apply (one grid over N * S * P pieces, n = row / S) or the table form of gn_apply_acc (grid row per sample)"""
    x1, x2 = _src(p)
    P, C_, S, N = p.C >> 3, p.C, p.S, p.N
    j = torch.arange(8)[None, :]
    chunk = 1 << 19
    for n0 in (range(N) if per_sample_grid else (None,)):
        total = S * P if per_sample_grid else N * S * P
        magic = magic_u32(total, P)
        for i0 in range(0, total, chunk):
            i = torch.arange(i0, min(i0 + chunk, total))
            row = _fastdiv(i, P, magic)
            c = ((i - row * P) * 8)[:, None] + j
            assert bool((row >= 0).all()) and bool((c >= 0).all()) and bool((c < C_).all())
            if per_sample_grid:
                n, grow = torch.full_like(row, n0), row + n0 * S
            else:
                n = torch.zeros_like(row) if N == 1 else row // S
                grow = row
            v = _gather(p, x1, x2, torch.zeros_like(grow)[:, None], grow[:, None], c)
            y = _affine(v, scale[n[:, None], c], shift[n[:, None], c], act)
            _store(out, grow[:, None] * C_ + c, y)


def _apply_lean(p: Packed, fmean, frstd, act: bool, out: torch.Tensor, defect=None) -> None:
    """gn_apply_acc_lean: block swizzle, one piece per thread, multiply-high decode, in-register affine with gg_div_small(c) groups"""
    x1, x2 = _src(p)
    P, C_, S, N, cpg = p.C >> 3, p.C, p.S, p.N, p.clog // 32
    pieces = S * P
    grid = (pieces + 255) // 256
    pm = magic_u32(pieces, P)
    blk = torch.arange(grid)
    bx = (blk & 7) * (grid >> 3) + (blk >> 3) if grid % 8 == 0 else blk
    i = (bx[:, None] * 256 + torch.arange(256)[None, :]).reshape(-1)
    i = i[i < pieces]
    row = (i * pm) >> 32
    c = ((i - row * P) * 8)[:, None] + torch.arange(8)[None, :]
    assert bool((row < S).all()) and bool((c >= 0).all()) and bool((c < C_).all())
    logical = c < p.clog
    g = _div_small(c.clamp(max=p.clog - 1), _rcp32(cpg))
    if defect == "group_round":
        g = torch.where(c == 7 * cpg, torch.full_like(g, 6), g)
    gm, bt = body(p.gamma), body(p.beta)
    for n in range(N):
        nn = 0 if defect == "sample0_stats" else n
        sc = torch.where(logical, frstd[nn][g] * gm[c], torch.zeros(1))
        sh = torch.where(logical, _fma(-fmean[nn][g], sc, bt[c]), torch.zeros(1))
        v = _gather(p, x1, x2, torch.full_like(row, n)[:, None], row[:, None], c)
        _store(out, (n * S + row)[:, None] * C_ + c, _affine(v, sc, sh, act))


def _apply_fused(p: Packed, fmean, frstd, act: bool, out: torch.Tensor, defect=None) -> None:
    """gn_fused_small: the registers of the statistics walk, affine with the clamped in-group channel, interior pieces stored whole,
    shared pieces element by element"""
    x1, x2 = _src(p)
    N, S, C_, cpg = p.N, p.S, p.C, p.clog // 32
    gm, bt = body(p.gamma), body(p.beta)
    n = torch.arange(N)[:, None, None]
    for g in (reversed(range(32)) if defect == "store_whole" else range(32)):
        r, c, mask, c_lo, c_hi = _group_walk(p, g)
        assert len(r) <= 512, "more than two pieces per thread"
        cl = (c - c_lo).clamp(0, cpg - 1) + c_lo
        sc = frstd[:, g, None, None] * gm[cl][None]
        sh = _fma(-fmean[:, g, None, None].expand_as(sc), sc, bt[cl][None].expand_as(sc))
        v = _gather(p, x1, x2, n, r[None, :, None], c[None].clamp(max=C_ - 1), defect)
        y = _affine(v, sc, sh, act)
        m = mask if defect != "store_whole" else (c < C_) & (c >= 0)
        _store(out, ((n * S + r[None, :, None]) * C_ + c[None]), y, m[None].expand(N, -1, -1))


def emulate(inp_path: str, p: Packed, eps: float, act: bool, defect: Optional[str] = None) -> Result:
    """what the kernels of the path leave in fresh guarded buffers, computed with their walk in fp32 / fp64 on the CPU"""
    N, S, C_ = p.N, p.S, p.C
    res = Result()
    path = inp_path
    if path in ("small", "partial"):
        fmean, frstd = (_stats_walk if path == "small" else _stats_partial)(p, eps, defect)
        scale, shift = _tables(p, fmean, frstd, defect)
        res.scale, res.shift = guarded(scale, SENTINEL), guarded(shift, SENTINEL)
        res.out = fresh(N * S * C_, torch.bfloat16)
        _apply_table(p, scale, shift, act, res.out, False)
    elif path == "fused":
        fmean, frstd = _stats_walk(p, eps, defect)
        if defect == "sample0_stats":
            fmean, frstd = fmean[:1].expand_as(fmean), frstd[:1].expand_as(frstd)
        res.out = fresh(N * S * C_, torch.bfloat16)
        _apply_fused(p, fmean, frstd, act, res.out, defect)
    elif path.startswith("lean"):
        fmean, frstd = _stats_acc(p, eps, "lean", defect if defect != "group_round" else None)
        res.out = fresh(N * S * C_, torch.bfloat16)
        _apply_lean(p, fmean, frstd, act, res.out, defect)
    elif path == "general":
        fmean, frstd = _stats_acc(p, eps, "general", defect)
        scale, shift = _tables(p, fmean, frstd, defect, approx_group=True)
        res.out = fresh(N * S * C_, torch.bfloat16)
        _apply_table(p, scale, shift, act, res.out, True)
    elif path == "ssacc":
        fmean, frstd = _stats_acc(p, eps, "ssacc", defect)
        scale, shift = _tables(p, fmean, frstd, defect)
        res.scale, res.shift = guarded(scale, SENTINEL), guarded(shift, SENTINEL)
    elif path in ("f32", "film"):
        x1, x2 = _src(p)
        cpg, clog = p.clog // 32, p.clog
        x = torch.cat([x1.view(N, S, p.C1)] + ([x2.view(N, S, p.C2)] if x2 is not None else []), 2)
        xg = x[:, :, :clog].double().reshape(N, S, 32, cpg)
        fmean, frstd = _mean_rstd(xg.sum((1, 3)), (xg * xg).sum((1, 3)), float(S * cpg), eps, fp64_div=True)
        rep = lambda v: v.repeat_interleave(cpg, 1)[:, None, :]
        y = (x[:, :, :clog] - rep(fmean)) * rep(frstd)                               # every step rounded to fp32 (contraction off)
        y = y * body(p.gamma)[:clog] + body(p.beta)[:clog]
        if path == "film":
            f = body(p.film).view(N, p.film_stride)
            y = y * (_f32(1.0) + f[:, None, :clog]) + f[:, None, clog:2 * clog]
        o = torch.zeros(N, S, C_)
        o[:, :, :clog] = y
        res.out = guarded(o, SENTINEL)
    else:
        raise AssertionError(path)
    return res


# ------------------------------------------------------------------------------------------------ LayerNorm
@dataclass
class LNInputs:
    rows: int
    C: int
    stride: int
    x: torch.Tensor           # guarded flat bf16 [rows * stride], pad lanes NaN
    gamma: torch.Tensor       # guarded fp32 [C]
    beta: torch.Tensor
    want: torch.Tensor        # bf16 [rows, stride], pad lanes 0

    def to(self, dev):
        return LNInputs(self.rows, self.C, self.stride, self.x.to(dev), self.gamma.to(dev), self.beta.to(dev), self.want.to(dev))


def build_layernorm(rows: int, C_: int, stride: int) -> LNInputs:
    assert C_ % 2 == 0, "regime E needs an even width"
    assert (C_ + 63) // 64 * (8 if stride == C_ else 1) <= MAX_TERMS
    gen = torch.Generator().manual_seed((C_ * 4099 + stride) * 256 + rows)
    m, s = centres(rows, 1, off=C_ // 2)                                             # a different (m, s) per row
    sg = _half_signs(gen, (rows,), C_)
    x = m + s * sg
    gamma, beta = coefficients(C_, False, seed=1)
    want = torch.zeros(rows, stride, dtype=torch.float64)
    want[:, :C_] = sg * gamma.double() + beta.double()
    xp = torch.full((rows, stride), float("nan"), dtype=torch.float64)
    xp[:, :C_] = x
    xb, wb = xp.to(torch.bfloat16), want.to(torch.bfloat16)
    assert bool((xb[:, :C_].double() == x).all()) and bool((wb.double() == want).all())
    assert bool((x.sum(1, keepdim=True) == C_ * m).all())
    nan = float("nan")
    return LNInputs(rows, C_, stride, guarded(xb, nan), guarded(gamma, nan), guarded(beta, nan), wb)


def layernorm_reference(ln: LNInputs, eps: float) -> torch.Tensor:
    x = body(ln.x).view(ln.rows, ln.stride)[:, :ln.C].double()
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    out = torch.zeros(ln.rows, ln.stride, dtype=torch.float64)
    out[:, :ln.C] = (x - mean) / torch.sqrt(var + eps) * body(ln.gamma).double() + body(ln.beta).double()
    return out


def check_layernorm(ln: LNInputs, out: torch.Tensor) -> str:
    got = body(out).view(ln.rows, ln.stride)
    want = ln.want.to(out.device)
    msg = mismatches(got, want)
    if not guards_intact(out):
        msg += " a guard element was written"
    return msg.strip()


def emulate_layernorm(ln: LNInputs, eps: float, defect: Optional[str] = None) -> torch.Tensor:
    """layernorm_kernel (lane -> 16-byte pieces lane + 64 k) / layernorm_rows_kernel (lane -> channels lane + 64 k): fp32 sums per lane,
    xor butterfly, mean, centred sum of squares, rsqrtf, ((x - mean) * rstd) * gamma + beta"""
    rows, C_, stride = ln.rows, ln.C, ln.stride
    whole = stride == C_ and C_ % 8 == 0
    x = body(ln.x).view(rows, stride).float()
    if whole:                                                                        # element (k, lane, j) = channel (lane + 64 k) * 8 + j
        ch = ((torch.arange(64)[None, :, None] + 64 * torch.arange(4)[:, None, None]) * 8 + torch.arange(8)[None, None, :]).permute(0, 2, 1).reshape(32, 64)
    else:
        ch = torch.arange(64)[None, :] + 64 * torch.arange((C_ + 63) // 64)[:, None]
    live = ch < C_
    v = torch.where(live[None], x[:, ch.clamp(max=C_ - 1)], torch.zeros(1))          # [rows, steps, 64]
    lanes = torch.arange(64)

    def total(t):
        s = torch.zeros(rows, 64)
        for k in range(t.shape[1]):
            s = s + t[:, k]
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
        return s[:, :1]
    mean = total(v) / _f32(float(C_))
    if defect == "next_row_mean":
        mean = mean.roll(-1, 0)
    d = torch.where(live[None], v - mean[:, :, None], torch.zeros(1))
    rstd = torch.rsqrt(total(d * d) / _f32(float(C_)) + _f32(eps))
    y = _fma((x[:, :C_] - mean) * rstd, body(ln.gamma).expand(rows, -1), body(ln.beta).expand(rows, -1))
    o = torch.zeros(rows, stride)
    o[:, :C_] = y
    return guarded(o.to(torch.bfloat16), SENTINEL)


# ------------------------------------------------------------------------------------------------ regime R
def build_random(N: int, C1: int, C2: int, sp, ratio: float, act: bool):
    """random bf16 data with the given mean-to-std ratio, random coefficients: (x [N, S, C], gamma, beta)"""
    S, C_ = math.prod(sp), C1 + C2
    gen = torch.Generator().manual_seed(C_ * 131 + S + int(ratio) + N)
    x = (torch.randn(N, S, C_, generator=gen) + ratio).to(torch.bfloat16)
    gamma = 1.0 + 0.5 * torch.randn(C_, generator=gen)
    beta = 0.5 * torch.randn(C_, generator=gen)
    return x, gamma, beta


def random_ratios(path: str, x: torch.Tensor, C1: int, gamma, beta, eps: float, act: bool, res: Result) -> Dict[str, float]:
    """the shadow harness's ratios (each must be <= 1) of a launch on random data; everything on x's device"""
    N, S, C_ = x.shape
    srcs = [x[:, :, :C1]] + ([x[:, :, C1:]] if C1 < C_ else [])
    sc, sh, dsc, dsh = shadow.gn_reference(srcs, C_, gamma, beta, eps)
    out = {}
    if res.scale is not None:
        gs, gt = body(res.scale).view(N, C_), body(res.shift).view(N, C_)
        out["coeff"] = shadow.coeff_ratio(gs, gt, sc, sh, dsc, dsh, C_)
        assert guards_intact(res.scale) and guards_intact(res.shift)
        if res.out is not None:                                                      # the apply launch with the coefficients it was given
            z = torch.zeros_like(dsc)
            out["apply"] = shadow.apply_ratio(srcs, gs, gt, z, z, act, body(res.out).view(N, S, C_), C_)
    elif res.out is not None:
        out["apply"] = shadow.apply_ratio(srcs, sc, sh, dsc, dsh, act, body(res.out).view(N, S, C_), C_)
    if res.out is not None:
        assert guards_intact(res.out)
    return out


def random_paths(N: int, S: int, C1: int, C2: int) -> List[str]:
    """every bf16 path that accepts the shape"""
    C_ = C1 + C2
    out = [stats_kernel(S, C_)]
    if fused_small_ok(S, C1, C2, C_):
        out.append("fused")
    return out + [apply_acc_kernel(N, S, C_, C_), "ssacc"]
