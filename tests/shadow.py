"""Shadow harness: check every `ops.*` kernel call of a network run against a plain fp64 reference of the same operation.

While a production network runs eagerly inside `shadow_ops()`, every op the blocks call through `ops.X(...)` is wrapped: the wrapper
runs the real op with identical arguments (so the kernel plan production picks does not change), synchronises, and compares the
device result with an fp64 reference computed from the exact device inputs of that call.  Each call records its worst ratio
err / bound, its shape, its batch size N, how many samples were checked and the host predicates that identify its plan.

The references in this module are pure torch (fp64, explicit gather indexing, no F.conv*), device-agnostic, and are also what
tests/test_shadow_cpu.py pins against torch's CPU operators and feeds with injected defects.

Error bounds (one set, written once here; no per-call or per-test tolerances)
---------------------------------------------------------------------------
conv, per output element (n, position, co), with a = the conv's input after the prologue, w = the recorded fp32 weight rounded to
bf16, sums over taps and input channels:

    |got - ref| <= 2^-8 * sum|w*a| + 2^-8 * |ref| (bf16 outputs only) + E_pro + 2^-20 * (|bias| + |residual|)

  * 2^-8 * sum|w*a| covers three sources: the bf16 rounding of a fused prologue's output (round to nearest: at most 2^-8 relative per
    staged element, with independent signs across the taps and channels of one sum), fp32 accumulation of the MFMA / split-K partial
    sums (K * 2^-24 <= 2^-10 at K <= 17 280 = 27 taps x 640 channels) and the bf16 weights, which the reference rounds exactly as the
    packer does (round to nearest even).  For convs without a prologue it is a worst-case bound; with a prologue the rounding term alone
    can reach 2^-8 * sum|w*a| only if every staged element rounds the same way by a full half ulp;
  * 2^-8 * |ref|: round-to-nearest bf16 output (unit roundoff 2^-8: an elementwise op's worst ratio sits just below 1);
  * E_pro = sum|w| * (1.1 * (|x| * d_scale + d_shift) + 2^-21 * (|x * scale| + |shift|)): the fp32 evaluation of x * scale + shift and of
    SiLU (Lipschitz 1.1) and, for coefficients the kernel derives from statistics itself (prologue_acc), the statistics term below;
  * fp32 additions of bias and residual: 2^-24 relative, stated as 2^-20.
  Pad lanes [Cout, Cout_pad) of the output must be exactly 0.

statistics (the GroupNorm coefficients a kernel derives from a stored tensor, per (n, group) with E|x|, E[x^2] of the group):
    d_mean = 2^-12 * E|x| + 2^-28,   d_var = 2^-11 * E[x^2] + 2^-20 + 2 |mean| d_mean,   d_rstd / rstd = d_var / (2 (var + eps)) + 2^-20
    d_scale = |scale| d_rstd / rstd,   d_shift = |mean| d_scale + |scale| d_mean + 2^-22 (|beta| + |mean * scale|)
  fp32 per-thread sums of at most 2^12 terms (or the 2^-28 / 2^-20 fixed-point quanta of the conv epilogue accumulators, which round
  once per tile) followed by fp64 combination.

conv epilogue accumulators (CL.acc), per (n, channel) over the S positions of the stored output y:
    |sum_got - sum y| <= 2^-14 * sum|y| + S 2^-29,   |sumsq_got - sum y^2| <= 2^-14 * sum y^2 + S 2^-21     (pad lanes exactly 0)
  fp32 tile partial sums (<= 1024 rows: 2^-14) plus one round-to-nearest per tile of the fixed-point quanta.

elementwise GroupNorm apply (groupnorm_apply / _fused / _apply_acc, resample2x prologue), bf16 out:
    2^-8 |ref| + 1.1 (|x| d_scale + d_shift) + 2^-21 (|x scale| + |shift|)        (d_* = 0 for coefficients passed in)
attention, per output element with p = softmax row, e_s = 2^-12 * scale * max_j sum_d |q_d k_jd| (fp32 score accumulation):
    2^-8 |ref| + (2^-8 + 2.2 e_s) * sum_j p_j |v_j|          (P rounded to bf16 for the PV product: 2^-9)
fp32 ops (linear_f32, film_fold, ddim_step and the fused DDIM epilogue): 2^-10 of the summed magnitudes for accumulations (as the
conv), 2^-20 of the operand magnitudes for a few dependent fp32 operations; bf16 copies of fp32 results add 2^-8 |ref|.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import inspect
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

U_BF16 = 2.0 ** -8          # bf16 rounding, with margin
U_ACC = 2.0 ** -10          # fp32 accumulation of up to 17 280 products
U_F32 = 2.0 ** -20          # a few dependent fp32 operations
U_PRO = 2.0 ** -21          # fp32 evaluation of x * scale + shift (+ SiLU)
SILU_LIP = 1.1              # max |silu'|
GELU_LIP = 1.13             # max |gelu'|
ACC_SUM_SCALE = 2.0 ** 28   # GG_ACC_SUM_SCALE (gg_conv.h)
ACC_SQ_SCALE = 2.0 ** 20    # GG_ACC_SQ_SCALE
ALL_POSITIONS = 4096        # samples with at most this many output positions are checked everywhere
RANDOM_POSITIONS = 2048
FACE_POSITIONS = 256        # per face of a volume
CHUNK = 1 << 23             # fp64 elements per gather chunk
EW_CHUNK = 1 << 25          # fp64 elements per chunk of the elementwise checks


def pad32(c: int) -> int:
    return (c + 31) // 32 * 32


def silu(z):
    return z / (1.0 + torch.exp(-z))


def gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def _ratio(err: torch.Tensor, bound: torch.Tensor) -> float:
    """worst err / bound; an error where the bound is 0 is infinite."""
    if err.numel() == 0:
        return 0.0
    r = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    r = torch.where((err > 0) & (bound <= 0), torch.full_like(r, math.inf), r)
    r = torch.where(torch.isnan(err), torch.full_like(r, math.inf), r)
    return float(r.max())


def pad_lanes_zero(t: torch.Tensor, c: int) -> bool:
    return c >= t.shape[-1] or not bool(t[..., c:].ne(0).any())


# ------------------------------------------------------------------------------------------------ positions
_BOUNDARY: Dict[Tuple[int, int, int], torch.Tensor] = {}


def _all_positions(sp) -> torch.Tensor:
    D, H, W = sp
    g = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij")
    return torch.stack([a.reshape(-1) for a in g], 1)


def sample_positions(sp: Sequence[int], seed: int) -> torch.Tensor:
    """int64 [P, 3] output positions (d, h, w) of one sample: all of them when there are <= 4096, otherwise every position of the
    perimeter (2-D) or of the 12 edges (3-D, corners included), FACE_POSITIONS random positions on each face of a volume and
    RANDOM_POSITIONS random positions anywhere (seeded)."""
    sp = tuple(int(s) for s in sp)
    if sp[0] * sp[1] * sp[2] <= ALL_POSITIONS:
        return _all_positions(sp)
    active = [i for i in range(3) if sp[i] > 1]
    b = _BOUNDARY.get(sp)
    if b is None:
        p = _all_positions(sp)
        onb = torch.zeros(p.shape[0], dtype=torch.int64)
        for i in active:
            onb += ((p[:, i] == 0) | (p[:, i] == sp[i] - 1)).long()
        b = _BOUNDARY[sp] = p[onb >= len(active) - 1]
    g = torch.Generator().manual_seed(seed)
    parts = [b, torch.stack([torch.randint(0, s, (RANDOM_POSITIONS,), generator=g) for s in sp], 1)]
    if len(active) == 3:
        for i in active:
            for v in (0, sp[i] - 1):
                f = torch.stack([torch.randint(0, s, (FACE_POSITIONS,), generator=g) for s in sp], 1)
                f[:, i] = v
                parts.append(f)
    return torch.unique(torch.cat(parts), dim=0)


# ------------------------------------------------------------------------------------------------ GroupNorm statistics
def channel_moments(t: torch.Tensor) -> torch.Tensor:
    """fp64 [3, N, Cpad]: per (n, channel) sum, sum of squares and sum of |x| over all positions of a channels-last tensor."""
    N, cp = t.shape[0], t.shape[-1]
    x = t.reshape(N, -1, cp)
    out = torch.zeros((3, N, cp), dtype=torch.float64, device=t.device)
    rows = max(1, EW_CHUNK // cp)
    for n in range(N):
        for r in range(0, x.shape[1], rows):
            xc = x[n, r:r + rows].double()
            out[0, n] += xc.sum(0)
            out[1, n] += (xc * xc).sum(0)
            out[2, n] += xc.abs().sum(0)
    return out


def gn_reference(srcs: Sequence[torch.Tensor], c_log: int, gamma, beta, eps: float, groups: int = 32):
    """GroupNorm(groups)(cat[srcs])[:c_log] as per-(n, c) coefficients from the stored tensors in fp64:
    (scale, shift, d_scale, d_shift), each fp64 [N, sum Cpad] with 0 beyond c_log (d_*: the statistics term of the module doc)."""
    m = torch.cat([channel_moments(s) for s in srcs], 2)
    N, Ct = m.shape[1], m.shape[2]
    S = srcs[0][0].numel() // srcs[0].shape[-1]
    cpg = c_log // groups
    g = m[:, :, :c_log].reshape(3, N, groups, cpg).sum(-1) / float(S * cpg)
    mean, ex2, eabs = g[0], g[1], g[2]
    var = (ex2 - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    d_mean = 2.0 ** -12 * eabs + 2.0 ** -28
    d_var = 2.0 ** -11 * ex2 + 2.0 ** -20 + 2.0 * mean.abs() * d_mean
    d_rel = d_var / (2.0 * (var + eps)) + 2.0 ** -20
    rep = lambda v: v.repeat_interleave(cpg, 1)
    gam = gamma.double().to(m.device)[:c_log]
    bet = beta.double().to(m.device)[:c_log]
    sc = rep(rstd) * gam
    sh = bet - rep(mean) * sc
    dsc = sc.abs() * rep(d_rel)
    dsh = rep(mean).abs() * dsc + sc.abs() * rep(d_mean) + 2.0 ** -22 * (bet.abs() + (rep(mean) * sc).abs())
    out = torch.zeros((4, N, Ct), dtype=torch.float64, device=m.device)
    for i, v in enumerate((sc, sh, dsc, dsh)):
        out[i, :, :c_log] = v
    return out[0], out[1], out[2], out[3]


def coeff_ratio(got_scale, got_shift, scale, shift, d_scale, d_shift, c_log: int) -> float:
    """GroupNorm coefficients (groupnorm_stats / groupnorm_scale_shift_acc) against the fp64 reference of gn_reference."""
    e1 = (got_scale[:, :c_log].double() - scale[:, :c_log]).abs()
    e2 = (got_shift[:, :c_log].double() - shift[:, :c_log]).abs()
    b1 = d_scale[:, :c_log] + 2.0 ** -23 * scale[:, :c_log].abs()
    b2 = d_shift[:, :c_log] + 2.0 ** -23 * shift[:, :c_log].abs()
    return max(_ratio(e1, b1), _ratio(e2, b2))


def apply_ratio(srcs: Sequence[torch.Tensor], scale, shift, d_scale, d_shift, act: bool, got: torch.Tensor, c_log: int) -> float:
    """act(cat[srcs] * scale + shift) elementwise (bf16 out) against fp64; pad lanes [c_log, Ct) of `got` must be 0."""
    if not pad_lanes_zero(got, c_log):
        return math.inf
    N, Ct = got.shape[0], got.shape[-1]
    xs = [s.reshape(N, -1, s.shape[-1]) for s in srcs]
    go = got.reshape(N, -1, Ct)
    rows = max(1, EW_CHUNK // Ct)
    worst = 0.0
    for n in range(N):
        s, t = scale[n, :c_log].double(), shift[n, :c_log].double()
        ds, dt = d_scale[n, :c_log].double(), d_shift[n, :c_log].double()
        for r in range(0, go.shape[1], rows):
            x = torch.cat([a[n, r:r + rows] for a in xs], 1)[:, :c_log].double()
            xs_ = x * s
            z = xs_ + t
            ref = silu(z) if act else z
            bound = U_BF16 * ref.abs() + SILU_LIP * (x.abs() * ds + dt) + U_PRO * (xs_.abs() + t.abs())
            worst = max(worst, _ratio((go[n, r:r + rows, :c_log].double() - ref).abs(), bound))
    return worst


def acc_ratio(out: torch.Tensor, cout: int, acc: torch.Tensor) -> float:
    """The GroupNorm sums a conv epilogue left in `acc` ([N, stripes, Cout_pad, 2] int64 fixed point) against fp64 sums of the
    stored output `out`; pad lanes of the accumulator must be 0."""
    a = acc.sum(1)
    if bool(a[:, cout:].ne(0).any()):
        return math.inf
    m = channel_moments(out)[:, :, :cout]
    S = out[0].numel() // out.shape[-1]
    e1 = (a[:, :cout, 0].double() / ACC_SUM_SCALE - m[0]).abs()
    e2 = (a[:, :cout, 1].double() / ACC_SQ_SCALE - m[1]).abs()
    return max(_ratio(e1, 2.0 ** -14 * m[2] + S * 2.0 ** -29), _ratio(e2, 2.0 ** -14 * m[1] + S * 2.0 ** -21))


# ------------------------------------------------------------------------------------------------ conv
def conv_extent(sp, k, stride: int, pad: int, upsample: bool):
    out = []
    for s, kk in zip(sp, k):
        if kk == 1:
            out.append((s - 1) // stride + 1)
        else:
            e = s * 2 if upsample else s
            out.append((e + 2 * pad - 3) // stride + 1)
    return tuple(out)


@dataclass
class ConvCall:
    """Everything the reference of one conv call needs, as device tensors exactly as the kernel saw them."""
    srcs: List[torch.Tensor]                  # channels-last [N, D, H, W, Cpad] inputs, concatenated along channels
    w: torch.Tensor                           # fp32 [Cout_w, Cin, taps] recorded by pack_conv_weight (rows in packed order)
    bias: Optional[torch.Tensor]              # fp32, rows of Cout_pad
    bias_per_sample: bool
    cout: int                                 # logical Cout of the call (2 * inner for GEGLU)
    k: Tuple[int, int, int] = (1, 3, 3)
    stride: int = 1
    pad: int = 1
    upsample: bool = False
    residual: Optional[torch.Tensor] = None
    prologue: Optional[Tuple[torch.Tensor, torch.Tensor]] = None   # per-(n, c) scale, shift [N, sum Cpad]
    prologue_err: Optional[Tuple[torch.Tensor, torch.Tensor]] = None   # statistics term (d_scale, d_shift) of derived coefficients
    act: bool = True
    skip: Optional[Tuple[List[torch.Tensor], torch.Tensor]] = None      # (sources, fp32 [Cout, Cs, 1] weight) of a K-concatenated 1x1
    geglu: bool = False
    ddim: Optional[Tuple[torch.Tensor, torch.Tensor]] = None          # (x before the step fp32 [M, 4], scalars fp32 [4])

    @property
    def out_extent(self):
        return conv_extent(self.srcs[0].shape[1:4], self.k, self.stride, self.pad, self.upsample)


def _bf16_weight(w: torch.Tensor, cin_pad: int) -> torch.Tensor:
    """fp64 [Cout_w, taps, cin_pad] of the bf16-rounded weight (zero columns beyond the recorded Cin)."""
    wb = w.to(torch.bfloat16).double()
    out = torch.zeros((w.shape[0], w.shape[2], cin_pad), dtype=torch.float64, device=w.device)
    out[:, :, :w.shape[1]] = wb.permute(0, 2, 1)
    return out


def _taps(call: ConvCall, pos: torch.Tensor):
    """Input coordinates [P, taps, 3] (source indices after the x2 upsample) and validity [P, taps] of every tap of `pos`."""
    sp = call.srcs[0].shape[1:4]
    one = all(kk == 1 for kk in call.k)
    coords, valid = [], []
    for i in range(3):
        kk, s = call.k[i], int(sp[i])
        o = pos[:, i:i + 1]
        if kk == 1:
            ci = o * (call.stride if one else 1) + torch.zeros(1, 1, dtype=torch.long, device=pos.device)
            coords.append(ci)
            valid.append(torch.ones_like(ci, dtype=torch.bool))
        else:
            e = s * 2 if call.upsample else s
            ci = o * call.stride - call.pad + torch.arange(3, device=pos.device)[None]
            v = (ci >= 0) & (ci < e)
            ci = ci.clamp(0, e - 1)
            coords.append(ci // 2 if call.upsample else ci)
            valid.append(v)
    kd, kh, kw = call.k
    d = coords[0][:, :, None, None].expand(-1, kd, kh, kw)
    h = coords[1][:, None, :, None].expand(-1, kd, kh, kw)
    w = coords[2][:, None, None, :].expand(-1, kd, kh, kw)
    v = valid[0][:, :, None, None] & valid[1][:, None, :, None] & valid[2][:, None, None, :]
    P = pos.shape[0]
    return d.reshape(P, -1), h.reshape(P, -1), w.reshape(P, -1), v.reshape(P, -1)


def conv_reference(call: ConvCall, n: int, pos: torch.Tensor):
    """fp64 output of sample n at output positions pos [P, 3]: (ref [P, Cout_out], bound [P, Cout_out]) with the bound of the
    module doc except the output rounding term.  Cout_out = inner for GEGLU, else Cout."""
    dev = call.srcs[0].device
    pos = pos.to(dev)
    cin = sum(s.shape[-1] for s in call.srcs)
    W = _bf16_weight(call.w, cin)                          # [Cw, T, Cin]
    Wa = W.abs()
    Cw, T = W.shape[0], W.shape[1]
    if call.prologue is not None:
        s_, t_ = call.prologue[0][n].double(), call.prologue[1][n].double()
        ds, dt = (call.prologue_err[0][n].double(), call.prologue_err[1][n].double()) if call.prologue_err is not None else (0.0, 0.0)
    P = pos.shape[0]
    ref = torch.empty((P, Cw), dtype=torch.float64, device=dev)
    mag = torch.empty_like(ref)
    ext = torch.zeros_like(ref)
    step = max(1, CHUNK // (T * cin))
    for p0 in range(0, P, step):
        pc = pos[p0:p0 + step]
        d, h, w, v = _taps(call, pc)
        x = torch.cat([s[n][d, h, w] for s in call.srcs], -1).double()      # [p, T, Cin]
        if call.prologue is not None:
            xs = x * s_
            z = xs + t_
            a = silu(z) if call.act else z
            e = SILU_LIP * (x.abs() * ds + dt) + U_PRO * (xs.abs() + t_.abs())
            e = e * v[..., None]
            ext[p0:p0 + step] = torch.einsum("ptc,otc->po", e, Wa)
        else:
            a = x
        a = a * v[..., None]                                  # zero padding AFTER the prologue: padded taps contribute 0
        ref[p0:p0 + step] = torch.einsum("ptc,otc->po", a, W)
        mag[p0:p0 + step] = torch.einsum("ptc,otc->po", a.abs(), Wa)
    if call.skip is not None:
        ssrc, sw = call.skip
        cs = sum(s.shape[-1] for s in ssrc)
        Ws = _bf16_weight(sw, cs)[:, 0]
        xs = torch.cat([s[n][pos[:, 0], pos[:, 1], pos[:, 2]] for s in ssrc], -1).double()
        ref += xs @ Ws.t()
        mag += xs.abs() @ Ws.abs().t()
    cp = pad32(Cw)
    small = torch.zeros_like(ref)
    if call.bias is not None:
        b = call.bias.reshape(-1, cp)[n if call.bias_per_sample else 0, :Cw].double()
        ref += b
        small += b.abs()
    if call.residual is not None:
        r = call.residual[n][pos[:, 0], pos[:, 1], pos[:, 2], :Cw].double()
        ref += r
        small += r.abs()
    err = U_BF16 * mag + ext + U_F32 * small
    if call.geglu:
        inner = Cw // 2
        j = torch.arange(inner, device=dev)
        vi, gi = (j // 16) * 32 + j % 16, (j // 16) * 32 + 16 + j % 16
        val, gate = ref[:, vi], ref[:, gi]
        out = val * gelu(gate)
        return out, gelu(gate).abs() * err[:, vi] + GELU_LIP * val.abs() * err[:, gi]
    return ref, err


def conv_ratio(call: ConvCall, got: torch.Tensor, seed: int = 0, ddim_got=None):
    """Worst err / bound of a conv's output `got` (CL tensor [N, Do, Ho, Wo, Cpad], bf16 or fp32) over the sampled positions of
    every sample, all output channels; infinite if a pad lane is not 0.  ddim_got = (x after, pred_x0 or None, unet_in or None) of
    a fused DDIM epilogue: the update is checked against the fp64 update of the fp64 eps.  Returns (ratio, ddim ratio, samples)."""
    Cw = call.w.shape[0]
    cout = Cw // 2 if call.geglu else Cw
    if not pad_lanes_zero(got, cout):
        return math.inf, math.inf if call.ddim is not None else None, 0
    bf16_out = got.dtype == torch.bfloat16
    N = got.shape[0]
    sp = tuple(got.shape[1:4])
    osp = sp[0] * sp[1] * sp[2]
    worst, worst_dd = 0.0, 0.0
    for n in range(N):
        pos = sample_positions(sp, seed * 1000 + n).to(got.device)
        ref, bound = conv_reference(call, n, pos)
        if bf16_out:
            bound = bound + U_BF16 * ref.abs()
        g = got[n][pos[:, 0], pos[:, 1], pos[:, 2], :cout].double()
        worst = max(worst, _ratio((g - ref).abs(), bound))
        if call.ddim is not None:
            m = n * osp + (pos[:, 0] * sp[1] + pos[:, 1]) * sp[2] + pos[:, 2]
            worst_dd = max(worst_dd, ddim_ratio(call.ddim[0][m], ref, bound, call.ddim[1], None,
                                                tuple(None if t is None else t[m] for t in ddim_got)))
    return worst, (worst_dd if call.ddim is not None else None), N


# ------------------------------------------------------------------------------------------------ DDIM update
def ddim_reference(x, eps, d_eps, scalars, noise=None):
    """fp64 DDIM update (ddim.py:190-204) of fp32 state x with eps (and its error bound d_eps): (x_prev, pred_x0, their bounds)."""
    a_t, a_prev, sigma, s1m = (float(v) for v in scalars.double().cpu())
    sa, sp_, dirc = math.sqrt(a_t), math.sqrt(a_prev), math.sqrt(max(1.0 - a_prev - sigma * sigma, 0.0))
    x = x.double()
    px0 = (x - s1m * eps) / sa
    xn = sp_ * px0 + dirc * eps
    d_px0 = (s1m * d_eps + U_F32 * (x.abs() + s1m * eps.abs())) / sa + U_F32 * px0.abs()
    d_xn = sp_ * d_px0 + dirc * d_eps + U_F32 * (sp_ * px0.abs() + dirc * eps.abs())
    if noise is not None:
        xn = xn + sigma * noise.double()
        d_xn = d_xn + U_F32 * (xn.abs() + sigma * noise.double().abs())
    return xn, px0, d_xn, d_px0


def ddim_ratio(x_before, eps, d_eps, scalars, noise, got) -> float:
    """got = (x after [M, C], pred_x0 [M, C] or None, unet_in [M, >= C] bf16 or None) against ddim_reference."""
    Cx = x_before.shape[-1]
    xn, px0, d_xn, d_px0 = ddim_reference(x_before, eps[:, :Cx], d_eps[:, :Cx], scalars, noise)
    x_got, px0_got, uin_got = got
    r = _ratio((x_got.double() - xn).abs(), d_xn)
    if px0_got is not None:
        r = max(r, _ratio((px0_got.double() - px0).abs(), d_px0))
    if uin_got is not None:
        r = max(r, _ratio((uin_got[:, :Cx].double() - xn).abs(), d_xn + U_BF16 * xn.abs()))
    return r


# ------------------------------------------------------------------------------------------------ attention
def attention_reference(q, k, v, scale: float, rows: Optional[torch.Tensor] = None):
    """q [Tq, d], k / v [Tkv, d] (bf16 values) -> fp64 softmax(q k^T scale) v of the query rows `rows` and its bound."""
    q, k, v = q.double(), k.double(), v.double()
    if rows is not None:
        q = q[rows]
    s = (q @ k.t()) * scale
    p = torch.softmax(s, -1)
    ref = p @ v
    es = 2.0 ** -12 * scale * (q.abs() @ k.abs().t()).amax(-1, keepdim=True)
    bound = U_BF16 * ref.abs() + (U_BF16 + 2.2 * es) * (p @ v.abs())
    return ref, bound


def attention_view(t: torch.Tensor, N: int, T: int, heads: int, hd: int, ld: int, hs: int, off: int) -> torch.Tensor:
    """[N, T, heads, hd] view of element (n, t, h, d) at base + off + (n T + t) ld + h hs + d."""
    return t.reshape(-1).as_strided((N, T, heads, hd), (T * ld, ld, hs, 1), t.reshape(-1).storage_offset() + off)


def attention_ratio(qv, kv, vv, ov, scale: float, seed: int = 0) -> float:
    """All (n, head) of [N, T, heads, hd] views; query rows: all if Tq <= 4096, else the first, the last and 2048 random ones."""
    N, Tq, H = qv.shape[0], qv.shape[1], qv.shape[2]
    worst = 0.0
    g = torch.Generator().manual_seed(seed)
    for n in range(N):
        if Tq <= ALL_POSITIONS:
            rows = torch.arange(Tq)
        else:
            rows = torch.unique(torch.cat([torch.tensor([0, Tq - 1]), torch.randint(0, Tq, (RANDOM_POSITIONS,), generator=g)]))
        rows = rows.to(qv.device)
        for h in range(H):
            for r0 in range(0, rows.numel(), 1024):
                rr = rows[r0:r0 + 1024]
                ref, bound = attention_reference(qv[n, :, h], kv[n, :, h], vv[n, :, h], scale, rr)
                worst = max(worst, _ratio((ov[n, rr, h].double() - ref).abs(), bound))
    return worst


# ------------------------------------------------------------------------------------------------ other families
def resample_ratio(src: torch.Tensor, C: int, up: bool, resample_d: bool, prologue, act: bool, got: torch.Tensor) -> float:
    """Nearest x2 / 2x average pool (of act(x * scale + shift) with a prologue) against fp64; pad lanes 0."""
    if not pad_lanes_zero(got, C):
        return math.inf
    N = src.shape[0]
    worst = 0.0
    for n in range(N):
        x = src[n, ..., :C].double()
        if prologue is not None:
            s, t = prologue[0][n, :C].double(), prologue[1][n, :C].double()
            xs = x * s
            a = silu(xs + t) if act else xs + t
            e = U_PRO * (xs.abs() + t.abs())
        else:
            a, e = x, torch.zeros_like(x)
        if up:
            idx = lambda y: y.repeat_interleave(2, 1).repeat_interleave(2, 2)
            ref = idx(a.repeat_interleave(2, 0) if resample_d else a)
            err = idx(e.repeat_interleave(2, 0) if resample_d else e)
            mag = ref.abs()
        else:
            D, H, W = a.shape[:3]
            kd = 2 if resample_d else 1
            sh = (D // kd, kd, H // 2, 2, W // 2, 2, C)
            ref = a[:D // kd * kd, :H // 2 * 2, :W // 2 * 2].reshape(sh).mean((1, 3, 5))
            mag = a.abs()[:D // kd * kd, :H // 2 * 2, :W // 2 * 2].reshape(sh).mean((1, 3, 5))
            err = e[:D // kd * kd, :H // 2 * 2, :W // 2 * 2].reshape(sh).mean((1, 3, 5))
        bound = (U_BF16 if got.dtype == torch.bfloat16 else U_F32) * ref.abs() + U_F32 * mag + err
        worst = max(worst, _ratio((got[n, ..., :C].double() - ref).abs(), bound))
    return worst


def film_ratio(scale0, shift0, film, C: int, scale, shift) -> float:
    """In-place FiLM fold: scale' = scale (1 + s), shift' = shift (1 + s) + t for c < C, unchanged beyond."""
    s, t = film[:, :C].double(), film[:, C:2 * C].double()
    rs = scale0[:, :C].double() * (1 + s)
    rt = shift0[:, :C].double() * (1 + s) + t
    r = _ratio((scale[:, :C].double() - rs).abs(), U_F32 * rs.abs())
    r = max(r, _ratio((shift[:, :C].double() - rt).abs(), U_F32 * ((shift0[:, :C].double() * (1 + s)).abs() + t.abs())))
    if not (torch.equal(scale[:, C:], scale0[:, C:]) and torch.equal(shift[:, C:], shift0[:, C:])):
        return math.inf
    return r


def layernorm_ratio(x, gamma, beta, eps: float, got) -> float:
    Cc = x.shape[-1]
    xr = x.reshape(-1, Cc).double()
    mean = xr.mean(1, keepdim=True)
    var = ((xr - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    gm, bt = gamma.double(), beta.double()
    ref = (xr - mean) * rstd * gm + bt
    ex2 = (xr * xr).mean(1, keepdim=True)
    d_mean = 2.0 ** -12 * xr.abs().mean(1, keepdim=True)
    d_rel = (2.0 ** -11 * ex2 + 2.0 * mean.abs() * d_mean) / (2.0 * (var + eps)) + 2.0 ** -20
    bound = U_BF16 * ref.abs() + gm.abs() * rstd * ((xr - mean).abs() * d_rel + d_mean) + U_F32 * ((xr - mean).abs() * rstd * gm.abs() + bt.abs())
    return _ratio((got.reshape(-1, Cc).double() - ref).abs(), bound)


def geglu_ratio(h, inner: int, got) -> float:
    hr = h.reshape(-1, 2 * inner).double()
    v, g = hr[:, :inner], hr[:, inner:]
    ref = v * gelu(g)
    bound = U_BF16 * ref.abs() + U_F32 * v.abs() * (g.abs() + 1.0)
    return _ratio((got.reshape(-1, inner).double() - ref).abs(), bound)


def linear_ratio(x, W, b, act_in: bool, got) -> float:
    a = x.double()
    if act_in:
        a = silu(a)
    Wd = W.double()
    ref = a @ Wd.t()
    mag = a.abs() @ Wd.abs().t()
    if b is not None:
        ref = ref + b.double()
        mag = mag + b.double().abs()
    return _ratio((got.double() - ref).abs(), U_ACC * mag + U_F32 * ref.abs())


# ------------------------------------------------------------------------------------------------ the harness
@dataclass
class Record:
    family: str
    ratio: float
    N: int
    samples: int
    shape: tuple
    plan: tuple = ()


class _LibProxy:
    """The loaded library with gg_conv_forward intercepted: the exact descriptor of every launched conv is copied, so that the host
    predicates identifying its plan can be asked about the very same descriptor."""

    def __init__(self, lib, sink: list):
        self._lib, self._sink = lib, sink

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def gg_conv_forward(self, dref, stream):
        from jointimagegeneration_amd._lib import ConvDesc
        self._sink.append(ConvDesc.from_buffer_copy(dref._obj))
        return self._lib.gg_conv_forward(dref, stream)


WRAPPED = ("conv", "groupnorm_stats", "groupnorm_apply", "groupnorm_fused", "groupnorm_apply_acc", "groupnorm_scale_shift_acc", "film_fold",
           "attention", "resample2x", "layernorm", "geglu", "linear_f32", "ddim_step", "pack_conv_weight")


class Shadow:
    def __init__(self):
        from jointimagegeneration_amd import _lib, ops
        self.ops, self.lib = ops, _lib.load()
        self.real = {name: getattr(ops, name) for name in WRAPPED}
        self.sig = {name: inspect.signature(f) for name, f in self.real.items()}
        self.weights: Dict[int, torch.Tensor] = {}
        self.records: List[Record] = []
        self.descs: list = []
        self.calls = 0

    # -- plumbing
    def _args(self, name, args, kw):
        b = self.sig[name].bind(*args, **kw)
        b.apply_defaults()
        return b.arguments

    def _pre(self):
        assert not torch.cuda.is_current_stream_capturing(), "shadowed runs are eager only"
        self.calls += 1
        return self.calls

    def _rec(self, family, ratio, N, samples, shape, plan=()):
        self.records.append(Record(family, float(ratio), int(N), int(samples), tuple(shape), tuple(plan)))

    def _weight(self, packed: torch.Tensor) -> torch.Tensor:
        w = self.weights.get(packed.data_ptr())
        if w is None:
            raise RuntimeError("conv weight packed outside the shadow: install it before the model's first forward or call "
                               "ops.invalidate_caches(model)")
        return w

    # -- wrappers
    def pack_conv_weight(self, w, cin_pad):
        out = self.real["pack_conv_weight"](w, cin_pad)
        ww = w.detach().float()
        self.weights[out.data_ptr()] = ww.reshape(ww.shape[0], ww.shape[1], -1).clone()
        return out

    def conv(self, *args, **kw):
        seed = self._pre()
        a = self._args("conv", args, kw)
        if a["post"] is not None:
            raise RuntimeError("the shadow does not check the fused CCDM reverse step: run plain UNet forwards")
        src1, src2, out = a["src1"], a["src2"], a["out"]
        keep = lambda t: t.clone() if (out is not None and t is not None and t.untyped_storage().data_ptr() == out.untyped_storage().data_ptr()) else t
        srcs = [keep(src1.t)] + ([keep(src2.t)] if src2 is not None else [])
        residual = keep(a["residual"].t) if a["residual"] is not None else None
        ddim = a["ddim"]
        x_before = ddim[0].clone() if ddim is not None else None
        n_desc = len(self.descs)
        res = self.real["conv"](*args, **kw)
        torch.cuda.synchronize()
        desc = self.descs[n_desc]
        del self.descs[n_desc:]
        plan = self._conv_plan(desc, a)
        ops = self.ops
        call = ConvCall(srcs=srcs, w=self._weight(a["weight"]), bias=a["bias"], bias_per_sample=a["bias_per_sample"], cout=a["cout"],
                        k=tuple(a["k"]), stride=a["stride"], pad=a["pad"], upsample=a["upsample"], residual=residual,
                        act=a["prologue_silu"], geglu=a["geglu"])
        if a["prologue"] is not None:
            call.prologue = a["prologue"]
        elif a["prologue_acc"] is not None:
            g, b, eps = a["prologue_acc"]
            c_log = src1.C + (src2.C if src2 is not None else 0)
            sc, sh, dsc, dsh = gn_reference(srcs, c_log, g, b, eps)
            call.prologue, call.prologue_err = (sc, sh), (dsc, dsh)
        if a["skip"] is not None:
            x1, x2, pw = a["skip"]
            call.skip = ([x1.t] + ([x2.t] if x2 is not None else []), self._weight(pw))
        ddim_got = None
        if res.fused_ddim:
            call.ddim = (x_before, ddim[1])
            ddim_got = (ddim[0], ddim[2], ddim[3])
        ratio, r_dd, samples = conv_ratio(call, res.t, seed, ddim_got)
        shape = (res.N,) + tuple(src1.t.shape[1:4]) + (sum(s.shape[-1] for s in srcs), a["cout"]) + tuple(a["k"])
        self._rec("conv", ratio, res.N, samples, shape, plan)
        if r_dd is not None:
            self._rec("conv.ddim", r_dd, res.N, samples, shape, plan)
        if res.acc is not None:
            self._rec("conv.stats", acc_ratio(res.t, a["cout"], res.acc), res.N, res.N, shape, plan)
        return res

    def _conv_plan(self, d, a):
        L, r = self.lib, C.byref(d)
        M = d.N * d.Do * d.Ho * d.Wo
        return (("halo", L.gg_conv_runs_halo_tile(r)), ("stats", L.gg_conv_emits_stats(r)), ("ws", L.gg_conv_workspace_bytes(r)),
                ("fuses_prologue", L.gg_conv_fuses_prologue(r)), ("fuses_skip", L.gg_conv_fuses_skip(r)),
                ("fuses_ddim", L.gg_conv_fuses_ddim(r)), ("prologue_from_acc", L.gg_conv_prologue_from_acc(r)),
                ("prologue", d.prologue_act), ("pro_acc", int(bool(d.pro_acc1))), ("skip", d.skip_C1 + d.skip_C2), ("geglu", d.epilogue_geglu),
                ("residual", int(bool(d.residual))), ("bias_per_sample", int(d.bias_stride != 0)), ("gn_acc", int(bool(d.gn_acc))),
                ("upsample", d.upsample), ("stride", d.stride), ("out_f32", d.out_dtype), ("M", M),
                ("tiny_m", int(M <= 128 and d.prologue_act == 0)))

    def _gn_plan(self, src1, src2):
        return (("groupnorm_fused_ok", int(self.ops.groupnorm_fused_ok(src1, src2))), ("has_stats", int(self.ops.has_stats(src1, src2))),
                ("stripes", src1.acc.shape[1] if src1.acc is not None else 0))

    def _gn_coeffs(self, name, args, kw):
        self._pre()
        a = self._args(name, args, kw)
        src1, src2 = a["src1"], a["src2"]
        plan = self._gn_plan(src1, src2)
        scale, shift = self.real[name](*args, **kw)
        torch.cuda.synchronize()
        srcs = [src1.t] + ([src2.t] if src2 is not None else [])
        c_log = src1.C + (src2.C if src2 is not None else 0)
        ref = gn_reference(srcs, c_log, a["gamma"], a["beta"], a["eps"])
        self._rec("groupnorm.coeffs", coeff_ratio(scale, shift, *ref, c_log), src1.N, src1.N, tuple(src1.t.shape) + (c_log,), (("op", name),) + plan)
        return scale, shift

    def groupnorm_stats(self, *args, **kw):
        return self._gn_coeffs("groupnorm_stats", args, kw)

    def groupnorm_scale_shift_acc(self, *args, **kw):
        return self._gn_coeffs("groupnorm_scale_shift_acc", args, kw)

    def _gn_normalise(self, name, args, kw):
        self._pre()
        a = self._args(name, args, kw)
        src1, src2 = a["src1"], a["src2"]
        plan = self._gn_plan(src1, src2)
        res = self.real[name](*args, **kw)
        torch.cuda.synchronize()
        srcs = [src1.t] + ([src2.t] if src2 is not None else [])
        c_log = src1.C + (src2.C if src2 is not None else 0)
        if name == "groupnorm_apply":
            ct = sum(s.shape[-1] for s in srcs)
            z = torch.zeros((src1.N, ct), dtype=torch.float64, device=src1.t.device)
            coeffs = (a["scale"], a["shift"], z, z)
        else:
            coeffs = gn_reference(srcs, c_log, a["gamma"], a["beta"], a["eps"])
        r = apply_ratio(srcs, *coeffs, a["act"], res.t, c_log)
        self._rec("groupnorm.apply", r, src1.N, src1.N, tuple(src1.t.shape) + (c_log,), (("op", name),) + plan)
        return res

    def groupnorm_apply(self, *args, **kw):
        return self._gn_normalise("groupnorm_apply", args, kw)

    def groupnorm_fused(self, *args, **kw):
        return self._gn_normalise("groupnorm_fused", args, kw)

    def groupnorm_apply_acc(self, *args, **kw):
        return self._gn_normalise("groupnorm_apply_acc", args, kw)

    def film_fold(self, scale, shift, film, C):
        self._pre()
        s0, t0 = scale.clone(), shift.clone()
        self.real["film_fold"](scale, shift, film, C)
        torch.cuda.synchronize()
        self._rec("film_fold", film_ratio(s0, t0, film, C, scale, shift), scale.shape[0], scale.shape[0], tuple(scale.shape))
        return None

    def attention(self, *args, **kw):
        seed = self._pre()
        a = self._args("attention", args, kw)
        self.real["attention"](*args, **kw)
        torch.cuda.synchronize()
        N, nh, hd, Tq, Tkv = a["N"], a["heads"], a["head_dim"], a["Tq"], a["Tkv"]
        qv = attention_view(a["q"], N, Tq, nh, hd, *a["ld_hs_q"], a["q_off"])
        kv = attention_view(a["k"], N, Tkv, nh, hd, *a["ld_hs_k"], a["k_off"])
        vv = attention_view(a["v"], N, Tkv, nh, hd, *a["ld_hs_v"], a["v_off"])
        ov = attention_view(a["out"], N, Tq, nh, hd, *a["ld_hs_o"], 0)
        d = self.ops.AttentionDesc()
        d.N, d.heads, d.head_dim, d.Tq, d.Tkv = N, nh, hd, Tq, Tkv
        (d.ldq, d.hsq), (d.ldk, d.hsk), (d.ldv, d.hsv), (d.ldo, d.hso) = a["ld_hs_q"], a["ld_hs_k"], a["ld_hs_v"], a["ld_hs_o"]
        plan = (("ws", self.lib.gg_attention_workspace_bytes(C.byref(d))),)
        self._rec("attention", attention_ratio(qv, kv, vv, ov, a["scale"], seed), N, N, (N, nh, hd, Tq, Tkv), plan)
        return None

    def resample2x(self, *args, **kw):
        self._pre()
        a = self._args("resample2x", args, kw)
        res = self.real["resample2x"](*args, **kw)
        torch.cuda.synchronize()
        src = a["src"]
        r = resample_ratio(src.t, src.C, a["up"], a["resample_d"], a["prologue"], a["act"] and a["prologue"] is not None, res.t)
        self._rec("resample2x", r, src.N, src.N, tuple(src.t.shape), (("up", a["up"]), ("prologue", a["prologue"] is not None)))
        return res

    def layernorm(self, *args, **kw):
        self._pre()
        a = self._args("layernorm", args, kw)
        out = self.real["layernorm"](*args, **kw)
        torch.cuda.synchronize()
        x = a["x"]
        self._rec("layernorm", layernorm_ratio(x, a["gamma"], a["beta"], a["eps"], out), x.shape[0], x.shape[0], tuple(x.shape))
        return out

    def geglu(self, *args, **kw):
        self._pre()
        a = self._args("geglu", args, kw)
        out = self.real["geglu"](*args, **kw)
        torch.cuda.synchronize()
        h = a["h"]
        self._rec("geglu", geglu_ratio(h, a["inner"], out), h.shape[0], h.shape[0], tuple(h.shape))
        return out

    def linear_f32(self, *args, **kw):
        self._pre()
        a = self._args("linear_f32", args, kw)
        out = self.real["linear_f32"](*args, **kw)
        torch.cuda.synchronize()
        x = a["x"].contiguous()
        self._rec("linear_f32", linear_ratio(x, a["W"], a["b"], a["act_in"], out), x.shape[0], x.shape[0], tuple(x.shape) + (a["W"].shape[0],))
        return out

    def ddim_step(self, *args, **kw):
        self._pre()
        a = self._args("ddim_step", args, kw)
        x = a["x"]
        Cx = x.shape[-1]
        M = x.numel() // Cx
        x0 = x.clone().view(M, Cx)
        self.real["ddim_step"](*args, **kw)
        torch.cuda.synchronize()
        eps = a["eps"].reshape(M, -1)[:, :Cx].double()
        noise = a["noise"].reshape(M, Cx) if a["noise"] is not None else None
        got = (x.view(M, Cx), a["pred_x0_out"].view(M, Cx) if a["pred_x0_out"] is not None else None,
               a["unet_in"].view(M, -1) if a["unet_in"] is not None else None)
        self._rec("ddim_step", ddim_ratio(x0, eps, torch.zeros_like(eps), a["scalars"], noise, got), M, M, (M, Cx))
        return None

    # -- results
    def families(self) -> Dict[str, List[Record]]:
        out: Dict[str, List[Record]] = {}
        for r in self.records:
            out.setdefault(r.family, []).append(r)
        return out

    def summary(self, title: str) -> str:
        lines = []
        for fam, rs in sorted(self.families().items()):
            w = max(rs, key=lambda r: r.ratio)
            lines.append(f"{title}: {fam:17s} worst err/bound {w.ratio:.3e} over {len(rs):4d} calls, {len({r.plan for r in rs}):3d} plans "
                         f"(worst at shape {w.shape})")
        return "\n".join(lines)

    def assert_within_bounds(self, N: int) -> None:
        assert self.records, "no kernel call was shadowed"
        bad = [r for r in self.records if not r.ratio <= 1.0]
        assert not bad, "kernel calls outside their bound:\n" + "\n".join(f"  {r.family} ratio {r.ratio:.3e} N={r.N} shape={r.shape} plan={dict(r.plan)}"
                                                                          for r in bad[:20])
        miss = [r for r in self.records if r.family.startswith("conv") or r.family.startswith("groupnorm") or r.family == "attention"]
        miss = [r for r in miss if r.samples != r.N or r.N != N]
        assert not miss, f"calls whose samples were not all checked at N = {N}: " + ", ".join(f"{r.family} {r.shape}" for r in miss[:10])


@contextlib.contextmanager
def shadow_ops():
    """Install the shadow over ops.* (every wrapped function) for the duration of the block; yields the Shadow with its records."""
    import pytest
    from jointimagegeneration_amd import _lib, ops
    sh = Shadow()
    real_load = _lib.load
    proxy = _LibProxy(real_load(), sh.descs)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_lib, "load", lambda: proxy)
        for name in WRAPPED:
            mp.setattr(ops, name, getattr(sh, name))
        yield sh
