"""Exhaustive bf16 sweeps of the activation functions: the inputs, the fp64 references and the criterion.

bf16 has 65280 finite values; one launch can push all of them through a SiLU or GELU site, so nothing is left to sampling.
all_finite_bf16() is that input, silu64 / gelu64 the references (fp64, on the bf16 input), check / check_f32 the criterion.

check (bf16-valued outputs) asserts, with r the fp64 reference of an input x:
  1. no output is NaN or Inf: no finite bf16 input may produce one at these sites.  (The one exception is a reference that itself
     rounds to a bf16 Inf -- value * gelu(gate) with |value| > 1 at the 85 largest gates of the GEGLU sweep: there the output must be
     exactly that Inf);
  2. |got - r| <= ulp_bf16(r) + allow  or  |got - r| <= FLOOR.
     FLOOR = 2^-120 is a condition, not a measurement: for x < -88.7 fp32 exp(-x) overflows and an fp32 SiLU returns 0 where fp64 still
     has a bf16-normal number (6 inputs, the largest |r| = 1.98e-37 < 2^-120), and the same floor makes the check independent of
     whether a matrix pipe flushes bf16 subnormals.  +-0 compare equal;
  3. outside the near-midpoint set (and above FLOOR) got is the correctly rounded result: got == RN_bf16(r).  The near-midpoint set is
     the inputs whose r lies within norm_exact.SILU_MARGIN = 0.05 bf16 ulp of a bf16 rounding midpoint.  A correct fp32 evaluation is
     off by about 1e-5 relative (< 0.004 bf16 ulp) and can disagree with correct rounding only next to a midpoint; rounding r through
     fp32 on the way to bf16 moves it by 2^-16 ulp, which cannot cross the margin either.
     With an allowance the condition reads: got lies between RN_bf16(r - allow) and RN_bf16(r + allow) -- the correct rounding of some
     value the allowance permits -- which is got == RN_bf16(r) wherever allow = 0.

`allow` is an absolute, per-input allowance (fp64 tensor) for a site whose FORMULA is known to lose accuracy, derived by the caller
from that formula (the 1 + erf form of GELU: see GEGLU_ALLOW) and never from what the code under test returns.

The near-midpoint set and the |r| <= FLOOR set are properties of the references alone: reference_sets() computes them on the CPU and
tests/test_act_sweep_cpu.py pins their sizes, so that nobody can widen them quietly.

check_f32 (fp32-valued outputs of v / (1 + expf(-v))): |got - r| <= 4 fp32 ulp(r) or <= FLOOR.  expf contributes at most 1 ulp, the add
0.5 ulp plus at most 1 inherited, the IEEE division 0.5 ulp: under 3 in total, 4 leaves one spare.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

import cond_ref
from norm_exact import SILU_MARGIN

FLOOR = 2.0 ** -120
N_FINITE = 65280
SQRT1_2 = 1.0 / math.sqrt(2.0)
ULP_ALLOW_F32 = 4.0

_CACHE: Dict[str, object] = {}


def all_finite_bf16() -> torch.Tensor:
    """The 65280 finite bf16 values in the order of their bit patterns 0x0000..0xFFFF (Inf and NaN dropped; both zeros and every
    subnormal kept).  Cached: treat as read-only."""
    if "x" not in _CACHE:
        b = torch.arange(0, 1 << 16, dtype=torch.int32)
        vals = torch.where(b >= 1 << 15, b - (1 << 16), b).to(torch.int16).view(torch.bfloat16)
        x = vals[torch.isfinite(vals.float())].contiguous()
        assert x.numel() == N_FINITE
        _CACHE["x"] = x
    return _CACHE["x"]


def silu64(x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    return x / (1.0 + torch.exp(-x))


gelu64 = cond_ref.gelu_f64            # 0.5 x erfc(-x / sqrt 2) in fp64
ulp_bf16 = cond_ref.bf16_ulp          # 2^(floor(log2 |r|) - 7), the smallest normal's spacing below it


def ulp_f32(r: torch.Tensor) -> torch.Tensor:
    """Spacing of fp32 numbers at |r| (fp64 tensor), the subnormal spacing 2^-149 below the smallest normal."""
    a = r.abs().double().clamp_min(2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 23)


def rn_bf16(r: torch.Tensor) -> torch.Tensor:
    """Round to nearest even onto bf16, returned as fp64 (through fp32: 2^-16 bf16 ulp, see the module docstring)."""
    return r.float().to(torch.bfloat16).double()


def midpoint_margin(r: torch.Tensor) -> torch.Tensor:
    """Distance of r from the nearest bf16 rounding midpoint, in bf16 ulp (norm_exact.palette's expression)."""
    return 0.5 - (r - rn_bf16(r)).abs() / ulp_bf16(r)


def reference_sets(r: torch.Tensor):
    """(near-midpoint mask, floor mask) of a reference: |r| <= FLOOR, and above it the inputs within SILU_MARGIN of a midpoint."""
    floor = r.abs() <= FLOOR
    near = ~floor & (midpoint_margin(r) < SILU_MARGIN)
    return near, floor


def geglu_allow(x: torch.Tensor, value: float = 1.0) -> torch.Tensor:
    """Allowance of value * 0.5 x (1 + erf(x / sqrt 2)) evaluated in fp32: the cancellation in 1 + erf turns the absolute fp32 error of
    erf near -1 (1 ulp of 1.0 at most: 2^-23) into an absolute error of 0.5 |x| times that, |x| * 2^-24; the allowance is 4 times it
    (below 3e-6 for |x| <= 12), scaled by |value|."""
    return abs(value) * x.double().abs() * 2.0 ** -22


def measure(got: torch.Tensor, x: torch.Tensor, ref: torch.Tensor, allow: Optional[torch.Tensor] = None) -> dict:
    """Statistics of bf16-valued outputs `got` of the inputs `x` against the fp64 reference `ref` (all the same shape, on the CPU):
      nonfinite   outputs that are NaN or Inf (but for the Inf that a reference which overflows bf16 demands)
      fail        outputs that miss condition 2
      not_rn      outputs above FLOOR that differ from RN_bf16(ref) (near-midpoint inputs included)
      fail_rn     outputs that miss condition 3
      worst_ulp   largest |got - ref| / ulp_bf16(ref) over |ref| > FLOOR
      bad_x       up to 5 inputs that miss condition 1, 2 or 3"""
    got, x, r = got.detach().cpu().double().reshape(-1), x.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    assert got.shape == x.shape == r.shape
    al = torch.zeros_like(r) if allow is None else allow.detach().cpu().double().reshape(-1)
    near, floor = reference_sets(r)
    rn = rn_bf16(r)
    over = torch.isinf(rn) & (got == rn)                       # the reference itself overflows bf16 and the output is that Inf
    finite = torch.isfinite(got) | over
    err = torch.where(over, torch.zeros_like(r), torch.where(finite, (got - r).abs(), torch.full_like(r, math.inf)))
    ulp = ulp_bf16(r)
    ok2 = (err <= ulp + al) | (err <= FLOOR)
    lo, hi = rn_bf16(r - al), rn_bf16(r + al)
    ok3 = near | floor | (finite & (got >= lo) & (got <= hi))
    bad = ~finite | ~ok2 | ~ok3
    above = ~floor
    return dict(nonfinite=int((~finite).sum()), fail=int((~ok2).sum()), not_rn=int((above & (got != rn_bf16(r))).sum()),
                fail_rn=int((~ok3).sum()), worst_ulp=float((err / ulp)[above & finite].max()) if bool((above & finite).any()) else 0.0,
                bad_x=[float(v) for v in x[bad][:5]], bad_got=[float(v) for v in got[bad][:5]], bad_ref=[float(v) for v in r[bad][:5]])


def check(got: torch.Tensor, x: torch.Tensor, ref: torch.Tensor, allow: Optional[torch.Tensor] = None) -> dict:
    """Assert conditions 1-3 of the module docstring; returns measure()'s statistics."""
    st = measure(got, x, ref, allow)
    where = f"first inputs {st['bad_x']}: got {st['bad_got']}, fp64 {st['bad_ref']}"
    assert st["nonfinite"] == 0, f"{st['nonfinite']} outputs are NaN or Inf; {where}"
    assert st["fail"] == 0, f"{st['fail']} outputs are more than one bf16 ulp (+ allowance) from the fp64 reference, worst {st['worst_ulp']:.3f} ulp; {where}"
    assert st["fail_rn"] == 0, f"{st['fail_rn']} outputs away from every rounding midpoint are not the correctly rounded result; {where}"
    return st


def check_f32(got: torch.Tensor, x: torch.Tensor, ref: torch.Tensor) -> dict:
    """fp32-valued outputs: finite, and within ULP_ALLOW_F32 fp32 ulp of the fp64 reference or within FLOOR of it."""
    got, x, r = got.detach().cpu().double().reshape(-1), x.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    assert got.shape == x.shape == r.shape
    finite = torch.isfinite(got)
    err = torch.where(finite, (got - r).abs(), torch.full_like(r, math.inf))
    ulp = ulp_f32(r)
    ok = (err <= ULP_ALLOW_F32 * ulp) | (err <= FLOOR)
    above = r.abs() > FLOOR
    st = dict(nonfinite=int((~finite).sum()), fail=int((~ok).sum()),
              worst_ulp=float((err / ulp)[above & finite].max()) if bool((above & finite).any()) else 0.0)
    bad = ~finite | ~ok
    where = f"first inputs {[float(v) for v in x[bad][:5]]}: got {[float(v) for v in got[bad][:5]]}, fp64 {[float(v) for v in r[bad][:5]]}"
    assert st["nonfinite"] == 0, f"{st['nonfinite']} outputs are NaN or Inf; {where}"
    assert st["fail"] == 0, f"{st['fail']} outputs are more than {ULP_ALLOW_F32} fp32 ulp from the fp64 reference, worst {st['worst_ulp']:.3f} ulp; {where}"
    return st


def conv_sites() -> dict:
    """path -> conv_exact.Case whose staging pass is swept: per kernel path the smallest stride-1 shape of conv_exact's case lists with
    Cout >= Cin (an identity weight on the centre tap then returns every staged value).  The 160-step kernel's listed cases have
    Cout < Cin or stride 2; 160 -> 160 at (64, 9) has Do * Ho * Wo % 64 == 0, which that kernel needs for a prologue, and stays outside
    the box envelope (Wo % 4 != 0).  The tiny-M kernel takes no prologue: it has no SiLU site."""
    import conv_exact as X
    by = {c.name: c for c in X.GATHER_CASES + X.HALO_CASES + X.TEAM_CASES + X.BOX_CASES}
    sites = {"gather": by["g3d_same"], "gather5": X.c2("g5_silu_64x9", "gather5", 1, 160, 0, 160, (64, 9), bias="none"),
             "halo": by["h3d_nt2"], "team": by["team_one_item"], "box": by["box_th2"]}
    for path, c in sites.items():
        assert c.path == path and c.C2 == 0 and c.cout >= c.C1 and c.C1 % 32 == 0 and c.stride == 1 and not c.up and c.pad == c.k[1] // 2
    return sites


def spec_silu_sites() -> list:
    """conv_exact.Case (+ its table entry) of every entry of gg_conv_box_specs.inc that takes a SiLU prologue from external tables
    (prologue_act == 1, pro_acc == 0) on a stride-1 conv with Cout >= Cin and without skip or DDIM fields."""
    import conv_exact as X
    out = []
    for key in X._gen_box_specs().table_keys():
        e = dict(zip(X.SPEC_FIELDS, (int(v) for v in key[len("GG_BOX_SPEC("):-1].split(","))))
        if e["prologue_act"] != 1 or e["pro_acc"] or e["UP"] or e["skip_C1"] or e["ddim_x"] or e["C2"] or e["Cout"] < e["C1"]:
            continue
        k = (1, 3, 3) if e["K3"] else (1, 1, 1)
        out.append((X.Case(f"spec_silu_{e['H']}x{e['W']}_{e['C1']}to{e['Cout']}_k{k[1]}", "spec", 1, e["C1"], 0, e["Cout"], (1, e["H"], e["W"]), k=k,
                           pad=1 if e["K3"] else 0, out_f32=bool(e["out_f32"]), bias="shared" if e["bias"] else "none",
                           residual=bool(e["residual"]), hint=X.HINT_SPEC_ONLY, stats=bool(e["gn_acc"])), e))
    return out


def references():
    """(x bf16 [65280], silu64(x), gelu64(x)), computed once and shared; treat as read-only."""
    if "refs" not in _CACHE:
        x = all_finite_bf16()
        _CACHE["refs"] = (x, silu64(x), gelu64(x))
    return _CACHE["refs"]
