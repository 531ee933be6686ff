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

Text, 3-D, GAN and LPIPS networks (the same rules: U_BF16 |ref| for a bf16 store, U_ACC of the summed magnitudes for an fp32 accumulation,
U_F32 of the operand magnitudes for a few dependent fp32 operations, d_mean / d_rel of layernorm_ratio for what normalises, pad lanes 0):
attention with kv_len: the bound above, the reference of sample n over keys [0, clamp(kv_len[n], 1, Tkv)) (kv_len read back from the device).
    The P-rounding term of the bound does not depend on the key count, so key lengths add no term.  Recorded as `attention` and, once
    more, as `attention.kvlen`; the plan of both says whether key lengths were used.
gelu:            2^-8 |ref| + 2^-20 GELU_LIP |x|                         (fp32 erf form of a bf16 input, one bf16 store)
add:             2^-8 |ref| + 2^-20 (|a| + |b|)
layernorm_rows:  layernorm's bound over the C logical lanes of each row; lanes [C, Cpad) of the result exactly 0.
embed_rows:      fp32 out bit-equal to tok[ids] + pos[t] evaluated in fp32 (one IEEE add); bf16 out = that value rounded to nearest even;
                 pad lanes exactly 0.  No tolerance: the ratio is 0 or infinite.
bert_embed:      layernorm's bound for x = word[ids] + type[tt] + pos[t] in fp64, plus the two fp32 additions that form x: with
                 d_x = 2^-20 (|word| + |type| + |pos|), gamma rstd (d_x + mean d_x + |x - mean| rstd rms d_x)  (the first-order change of
                 (x - mean) rstd under a perturbation of x: of x itself, of the mean, and of rstd, |d rstd| / rstd <= rstd rms d_x).
interpolate2d:   every mode is separable, out = Wh x Ww^T with the row weights of ops.interpolate2d's docstring (coordinate scale
                 float(1 / s), extent floor(in * s); nearest floor(dst * scale); bilinear scale (dst + 0.5) - 0.5 clamped at 0; bicubic the
                 same unclamped, A = -0.75, taps clamped into the plane; area the mean over [floor(dst in / out), ceil((dst + 1) in / out))).
                 Bound 2^-20 sum |weight * tap| (fp32 weights and a few fp32 multiply-adds per output).
patch_conv:      acc = the conv gather with kernel 4, padding 2, stride 1 or 2, kd 1 or 4; y = acc * alpha + beta; out = LeakyReLU(y):
                 max(1, slope) * (|alpha| 2^-8 sum|w*a| + 2^-20 (|acc * alpha| + |beta|)) + 2^-8 |out| (bf16 outputs only).
                 2^-8 sum|w*a| is the conv's accumulation term: nothing is staged here (bf16 inputs, weights rounded as the packer does), so
                 it only has to cover fp32 accumulation, K 2^-24 <= 2^-9 in the worst case at the deepest 3-D block (K = 64 taps x 512),
                 with independent signs over K.  Positions as the conv: all up to ALL_POSITIONS, else sample_positions.  Pad lanes 0.
relu_cl:         exact.     lpips_tap pooled output: exactly maxpool2x2(relu(.)) of both inputs, a's images first.
lpips_tap value: |got - ref| <= LPIPS_TAP_RTOL |ref| per image against the fp64 restatement on the same (already rounded) inputs, the
                 project's fp32-validation bound 2e-5 (a normalised fp32 sum over C <= 512 channels and h w pixels, tree-reduced);
                 `total` holds exactly the value, or what it held plus the value in fp32 with accumulate.
volume_views_cl: channel c = (x - shift_c) / scale_c: 2^-20 (|x| + |shift_c|) / |scale_c| (fp32), plus 2^-8 |ref| for a bf16 out; lanes 3..31 0.
vq_nearest:      the index equals the first fp64 argmin of d = |z|^2 + |e|^2 - 2 z.e on every row whose two smallest fp64 distances differ by
                 at least 1e-4 (1 + d_min) (the near-tie margin of DESIGN.md 7c; inside it the kernel's fp32 order may decide, between those two
                 codes only); the straight-through rows are bit-equal to z + (E[idx] - z) in fp32 with the kernel's own index (two IEEE
                 operations, nothing to contract).  The share of rows inside the margin is recorded; above VQ_TIE_CAP = 2 % the record fails.

Operand contract: before a wrapped op runs, contract_violations() checks what the product passed (device, contiguity or exactly the stride
the wrapper forwards, the dtype the C entry reads, at least the extent the kernel reads).  A violation is a record of family `contract`
with ratio inf whose plan names op, operand and what was found.
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
LPIPS_TAP_RTOL = 2e-5       # per-image LPIPS tap value against its fp64 restatement (the project's fp32-validation bound)
VQ_TIE_MARGIN = 1e-4        # near-tie margin of DESIGN.md 7c: fp64 gap below VQ_TIE_MARGIN * (1 + d_min)
VQ_TIE_CAP = 0.02           # largest share of rows allowed inside that margin


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


def attention_ratio(qv, kv, vv, ov, scale: float, seed: int = 0, kv_len: Optional[Sequence[int]] = None) -> float:
    """All (n, head) of [N, T, heads, hd] views; query rows: all if Tq <= 4096, else the first, the last and 2048 random ones.
    kv_len (host integers, one per sample): sample n is judged against attention over keys [0, clamp(kv_len[n], 1, Tkv))."""
    N, Tq, H = qv.shape[0], qv.shape[1], qv.shape[2]
    worst = 0.0
    g = torch.Generator().manual_seed(seed)
    if kv_len is not None:
        assert len(kv_len) == N, (len(kv_len), N)
        lens = [min(max(int(v), 1), kv.shape[1]) for v in kv_len]
        kv, vv = [kv[n, :lens[n]] for n in range(N)], [vv[n, :lens[n]] for n in range(N)]
    for n in range(N):
        if Tq <= ALL_POSITIONS:
            rows = torch.arange(Tq)
        else:
            rows = torch.unique(torch.cat([torch.tensor([0, Tq - 1]), torch.randint(0, Tq, (RANDOM_POSITIONS,), generator=g)]))
        rows = rows.to(qv.device)
        for h in range(H):
            for r0 in range(0, rows.numel(), 1024):
                rr = rows[r0:r0 + 1024]
                ref, bound = attention_reference(qv[n, :, h], kv[n][:, h], vv[n][:, h], scale, rr)
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


def layernorm_reference(xr, gamma, beta, eps: float, d_x=None):
    """fp64 LayerNorm of the rows xr [R, C] (fp64) and its bound for a bf16 output; d_x [R, C]: an error bound of xr itself (the
    bert_embed term of the module doc)."""
    mean = xr.mean(1, keepdim=True)
    var = ((xr - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    gm, bt = gamma.double().reshape(1, -1), beta.double().reshape(1, -1)
    ref = (xr - mean) * rstd * gm + bt
    ex2 = (xr * xr).mean(1, keepdim=True)
    d_mean = 2.0 ** -12 * xr.abs().mean(1, keepdim=True)
    d_rel = (2.0 ** -11 * ex2 + 2.0 * mean.abs() * d_mean) / (2.0 * (var + eps)) + 2.0 ** -20
    bound = U_BF16 * ref.abs() + gm.abs() * rstd * ((xr - mean).abs() * d_rel + d_mean) + U_F32 * ((xr - mean).abs() * rstd * gm.abs() + bt.abs())
    if d_x is not None:
        rms = torch.sqrt((d_x * d_x).mean(1, keepdim=True))
        bound = bound + gm.abs() * rstd * (d_x + d_x.mean(1, keepdim=True) + (xr - mean).abs() * rstd * rms)
    return ref, bound


def layernorm_ratio(x, gamma, beta, eps: float, got) -> float:
    Cc = x.shape[-1]
    ref, bound = layernorm_reference(x.reshape(-1, Cc).double(), gamma, beta, eps)
    return _ratio((got.reshape(-1, Cc).double() - ref).abs(), bound)


def layernorm_rows_ratio(x, C: int, gamma, beta, eps: float, got) -> float:
    """LayerNorm over the C logical lanes of rows Cpad apart (gamma, beta: C values); lanes [C, Cpad) of `got` must be 0."""
    if got.shape != x.shape or not pad_lanes_zero(got, C):
        return math.inf
    return layernorm_ratio(x[..., :C], gamma.reshape(-1)[:C], beta.reshape(-1)[:C], eps, got[..., :C])


def gelu_ratio(x, got) -> float:
    xd = x.double()
    ref = gelu(xd)
    return _ratio((got.double() - ref).abs(), U_BF16 * ref.abs() + U_F32 * GELU_LIP * xd.abs())


def add_ratio(a, b, got) -> float:
    ref = a.double() + b.double()
    return _ratio((got.double() - ref).abs().reshape(-1), (U_BF16 * ref.abs() + U_F32 * (a.double().abs() + b.double().abs())).reshape(-1))


def embed_rows_ratio(ids, tok, pos, got) -> float:
    """got: fp32 [B, T, D] or bf16 [B, 1, 1, T, pad32(D)].  Exact: 0.0 or inf."""
    B, T = ids.shape
    D = tok.shape[1]
    want = tok[ids.long()]
    if pos is not None:
        want = want + pos[:T][None]                            # one fp32 add per element: IEEE, the same bits everywhere
    if got.dtype == torch.float32:
        return 0.0 if tuple(got.shape) == (B, T, D) and torch.equal(got, want) else math.inf
    rows = got.reshape(B, T, -1)
    ok = got.dtype == torch.bfloat16 and rows.shape[-1] == pad32(D) and pad_lanes_zero(rows, D) and torch.equal(rows[..., :D], want.to(torch.bfloat16))
    return 0.0 if ok else math.inf


def bert_embed_ratio(ids, type_ids, word, pos, type_tab, gamma, beta, eps: float, got) -> float:
    """LayerNorm(word[ids] + type[tt] + pos[t]) over D as bf16 rows [B, 1, 1, T, pad32(D)]; tt = 0 without type_ids."""
    B, T = ids.shape
    D = word.shape[1]
    rows = got.reshape(B * T, -1)
    if rows.shape[-1] != pad32(D) or not pad_lanes_zero(rows, D):
        return math.inf
    tt = type_ids.long() if type_ids is not None else torch.zeros_like(ids, dtype=torch.long)
    w, t, p = word[ids.long()].double(), type_tab[tt].double(), pos[:T].double()[None].expand(B, T, D)
    x = (w + t + p).reshape(B * T, D)
    d_x = U_F32 * (w.abs() + t.abs() + p.abs()).reshape(B * T, D)
    ref, bound = layernorm_reference(x, gamma, beta, eps, d_x)
    return _ratio((rows[:, :D].double() - ref).abs(), bound)


# interpolate2d: row weights of one axis, as ops.interpolate2d's docstring states the coordinate rule
def interp_weights(n_in: int, scale_factor: float, mode: str, device=None):
    """(W, |W|) fp64 [n_out, n_in] with out = W @ in along one axis: n_out = floor(n_in * s), coordinate scale float32(1 / s).
    |W| sums the magnitudes of the taps (taps clamped onto one source index add up there)."""
    n_out = int(math.floor(float(n_in) * float(scale_factor)))
    scale = float(torch.tensor(1.0 / float(scale_factor), dtype=torch.float32))
    dst = torch.arange(n_out, dtype=torch.float64)
    taps = []                                                   # (source index int64 [n_out], weight fp64 [n_out])
    if mode == "nearest":
        taps.append((torch.floor(dst * scale).long().clamp(max=n_in - 1), torch.ones_like(dst)))
    elif mode == "bilinear":
        src = (scale * (dst + 0.5) - 0.5).clamp_min(0.0)
        i0 = torch.floor(src).long().clamp(max=n_in - 1)
        lam = src - i0
        taps += [(i0, 1.0 - lam), ((i0 + 1).clamp(max=n_in - 1), lam)]
    elif mode == "bicubic":
        src = scale * (dst + 0.5) - 0.5
        i0 = torch.floor(src)
        t, A = src - i0, -0.75
        near = lambda v: ((A + 2.0) * v - (A + 3.0)) * v * v + 1.0
        far = lambda v: ((A * v - 5.0 * A) * v + 8.0 * A) * v - 4.0 * A
        for off, wgt in ((-1, far(t + 1.0)), (0, near(t)), (1, near(1.0 - t)), (2, far(2.0 - t))):
            taps.append(((i0.long() + off).clamp(0, n_in - 1), wgt))
    elif mode == "area":
        lo = torch.floor(dst * n_in / n_out).long()
        hi = torch.ceil((dst + 1.0) * n_in / n_out).long()
        for j in range(int((hi - lo).max())):
            live = (lo + j < hi).double()
            taps.append(((lo + j).clamp(max=n_in - 1), live / (hi - lo).double()))
    else:
        raise ValueError(mode)
    W = torch.zeros((n_out, n_in), dtype=torch.float64)
    Wa = torch.zeros_like(W)
    r = torch.arange(n_out)
    for idx, wgt in taps:
        W.index_put_((r, idx), wgt, accumulate=True)
        Wa.index_put_((r, idx), wgt.abs(), accumulate=True)
    return W.to(device), Wa.to(device)


def interpolate2d_reference(x, scale_factor: float, mode: str):
    """fp64 F.interpolate(x, scale_factor=s, mode=mode) of NCHW x (align_corners=False) and sum |weight * tap| per output."""
    Wh, Wha = interp_weights(x.shape[2], scale_factor, mode, x.device)
    Ww, Wwa = interp_weights(x.shape[3], scale_factor, mode, x.device)
    xd = x.double()
    return Wh @ xd @ Ww.t(), Wha @ xd.abs() @ Wwa.t()


def interpolate2d_ratio(x, scale_factor: float, mode: str, got) -> float:
    ref, mag = interpolate2d_reference(x, scale_factor, mode)
    if tuple(got.shape) != tuple(ref.shape):
        return math.inf
    return _ratio((got.double() - ref).abs().reshape(-1), (U_F32 * mag).reshape(-1))


# patch_conv: kernel 4, padding 2
def patch_conv_extent(sp, kd: int, stride: int):
    D, H, W = (int(s) for s in sp)
    return (D if kd == 1 else D // stride + 1, H // stride + 1, W // stride + 1)


def patch_conv_reference(src, w, alpha, beta, kd: int, stride: int, slope: float, n: int, pos):
    """fp64 LeakyReLU(acc * alpha + beta) of sample n at output positions pos [P, 3] and its bound without the output rounding term.
    src channels-last [N, D, H, W, Cpad]; w fp32 [Cout, Cin, taps] with the taps in (kd, kh, kw) order; alpha (or None) / beta fp32 rows."""
    dev = src.device
    pos = pos.to(dev)
    sp, cin = src.shape[1:4], src.shape[-1]
    Wt = _bf16_weight(w, cin)                                    # [Cout, T, Cin]
    Cw, T = Wt.shape[0], Wt.shape[1]
    ar = torch.arange(4, device=dev)[None]
    coords, valid = [], []
    for i in range(3):
        o = pos[:, i:i + 1]
        if i == 0 and kd == 1:
            coords.append(o)
            valid.append(torch.ones_like(o, dtype=torch.bool))
        else:
            ci = o * stride - 2 + ar
            valid.append((ci >= 0) & (ci < int(sp[i])))
            coords.append(ci.clamp(0, int(sp[i]) - 1))
    P = pos.shape[0]
    sh = (P, coords[0].shape[1], 4, 4)
    d = coords[0][:, :, None, None].expand(sh).reshape(P, -1)
    h = coords[1][:, None, :, None].expand(sh).reshape(P, -1)
    ww = coords[2][:, None, None, :].expand(sh).reshape(P, -1)
    v = (valid[0][:, :, None, None] & valid[1][:, None, :, None] & valid[2][:, None, None, :]).reshape(P, -1)
    assert d.shape[1] == T, (d.shape, T)
    acc = torch.empty((P, Cw), dtype=torch.float64, device=dev)
    mag = torch.empty_like(acc)
    step = max(1, CHUNK // (T * cin))
    for p0 in range(0, P, step):
        s = slice(p0, p0 + step)
        a = src[n][d[s], h[s], ww[s]].double() * v[s][..., None]
        acc[s] = torch.einsum("ptc,otc->po", a, Wt)
        mag[s] = torch.einsum("ptc,otc->po", a.abs(), Wt.abs())
    al = alpha.reshape(-1)[:Cw].double() if alpha is not None else torch.ones(Cw, dtype=torch.float64, device=dev)
    be = beta.reshape(-1)[:Cw].double()
    y = acc * al + be
    ref = torch.where(y >= 0, y, y * slope)
    bound = max(1.0, abs(slope)) * (al.abs() * U_BF16 * mag + U_F32 * ((acc * al).abs() + be.abs()))
    return ref, bound


def patch_conv_ratio(src, w, alpha, beta, cout: int, kd: int, stride: int, slope: float, got, seed: int = 0):
    """Worst err / bound of a PatchGAN conv's output (CL [N, Do, Ho, Wo, pad32(cout)], bf16 or fp32) and the samples checked."""
    N = src.shape[0]
    if tuple(got.shape) != (N,) + patch_conv_extent(src.shape[1:4], kd, stride) + (pad32(cout),) or not pad_lanes_zero(got, cout):
        return math.inf, 0
    sp = tuple(got.shape[1:4])
    worst = 0.0
    for n in range(N):
        pos = sample_positions(sp, seed * 1000 + n).to(got.device)
        ref, bound = patch_conv_reference(src, w, alpha, beta, kd, stride, slope, n, pos)
        if got.dtype == torch.bfloat16:
            bound = bound + U_BF16 * ref.abs()
        g = got[n][pos[:, 0], pos[:, 1], pos[:, 2], :cout].double()
        worst = max(worst, _ratio((g - ref).abs(), bound))
    return worst, N


# LPIPS
def relu_ratio(before, after) -> float:
    return 0.0 if torch.equal(after, torch.relu(before)) else math.inf


def volume_views_reference(x, view: int, n0: int, n1: int, shift, scale):
    """fp64 [n1 - n0, hh, ww, 3] and its fp32 bound: images [n0, n1) of an axis view of x [B, D, H, W] (view 3: x is [B, 3, H, W])."""
    B, D, H, W = x.shape
    xd, sh, sc = x.double(), shift.double().reshape(-1), scale.double().reshape(-1)
    if view == 3:
        imgs = xd.permute(0, 2, 3, 1)[n0:n1]
    else:
        perm = ((0, 1, 2, 3), (0, 2, 1, 3), (0, 3, 1, 2))[view]
        p = xd.permute(*perm)
        imgs = p.reshape((B * p.shape[1],) + tuple(p.shape[2:]))[n0:n1][..., None].expand(-1, -1, -1, 3)
    return (imgs - sh) / sc, U_F32 * (imgs.abs() + sh.abs()) / sc.abs()


def volume_views_ratio(x, view: int, n0: int, n1: int, shift, scale, got) -> float:
    ref, bound = volume_views_reference(x, view, n0, n1, shift, scale)
    if tuple(got.shape) != (n1 - n0, 1) + tuple(ref.shape[1:3]) + (32,) or not pad_lanes_zero(got, 3):
        return math.inf
    if got.dtype == torch.bfloat16:
        bound = bound + U_BF16 * ref.abs()
    return _ratio((got[:, 0, :, :, :3].double() - ref).abs().reshape(-1), bound.reshape(-1))


def lpips_tap_reference(a, b, lin_w):
    """fp64 [n]: mean_hw sum_c w_c (A_c / (|A| + 1e-10) - B_c / (|B| + 1e-10))^2 with A = relu(a), B = relu(b); a, b [n, 1, h, w, C]."""
    A, B = torch.relu(a.double())[:, 0], torch.relu(b.double())[:, 0]
    na = A / (torch.sqrt((A * A).sum(-1, keepdim=True)) + 1e-10)
    nb = B / (torch.sqrt((B * B).sum(-1, keepdim=True)) + 1e-10)
    return (((na - nb) ** 2) * lin_w.double().reshape(-1)).sum(-1).mean((1, 2))


def lpips_pool_reference(a, b):
    """maxpool2x2(relu(.)) of both inputs as one batch [2 n, 1, h // 2, w // 2, C], a's images first (odd extents drop the last line)."""
    x = torch.relu(torch.cat([a, b]))[:, 0]
    h2, w2 = x.shape[1] // 2, x.shape[2] // 2
    x = x[:, :h2 * 2, :w2 * 2].reshape(x.shape[0], h2, 2, w2, 2, x.shape[-1])
    return x.amax((2, 4))[:, None]


def lpips_tap_ratio(a, b, lin_w, got, pooled=None, total=None, total_before=None) -> float:
    """got fp32 [n] against the restatement under LPIPS_TAP_RTOL; pooled (or None) exact; total (or None) = got, or total_before + got."""
    ref = lpips_tap_reference(a, b, lin_w)
    r = _ratio((got.double() - ref).abs(), LPIPS_TAP_RTOL * ref.abs())
    if pooled is not None and not torch.equal(pooled, lpips_pool_reference(a, b)):
        return math.inf
    if total is not None and not torch.equal(total, got if total_before is None else total_before + got):
        return math.inf
    return r


# vector quantiser
def vq_reference(rows, codebook, chunk: int = 4096):
    """(first fp64 argmin int64 [M], the second-nearest code int64 [M], near-tie bool [M]) of rows [M, C] against codebook [K, C]."""
    idx, second, tie = [], [], []
    e = codebook.double()
    for s in range(0, rows.shape[0], chunk):
        z = rows[s:s + chunk].double()
        d = (z * z).sum(1, keepdim=True) + (e * e).sum(1)[None] - 2.0 * (z @ e.t())
        dmin = d.min(1, keepdim=True).values
        ar = torch.arange(d.shape[1], device=d.device)[None].expand_as(d)
        i = torch.where(d == dmin, ar, torch.full_like(ar, d.shape[1])).min(1).values
        idx.append(i)
        if d.shape[1] > 1:
            d2 = d.scatter(1, i[:, None], math.inf)
            m2 = d2.min(1)
            second.append(m2.indices)
            tie.append((m2.values - dmin[:, 0]) < VQ_TIE_MARGIN * (1.0 + dmin[:, 0]))
        else:
            second.append(i)
            tie.append(torch.zeros_like(i, dtype=torch.bool))
    return torch.cat(idx), torch.cat(second), torch.cat(tie)


def vq_ratio(rows, codebook, idx_got, st_got=None):
    """rows fp32 [M, >= C] as the kernel read them, idx_got int32 [M], st_got fp32 [M, >= C] or None -> (0.0 or inf, near-tie share)."""
    C = codebook.shape[1]
    z = rows[:, :C]
    idx, second, tie = vq_reference(z, codebook)
    got = idx_got.reshape(-1).long()
    share = float(tie.double().mean()) if tie.numel() else 0.0
    ok = got.numel() == idx.numel() and bool(((got == idx) | (tie & (got == second))).all()) and share <= VQ_TIE_CAP
    if ok and st_got is not None:
        ok = torch.equal(st_got[:, :C], z + (codebook[got] - z))
    return (0.0 if ok else math.inf), share


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


# ------------------------------------------------------------------------------------------------ operand contract
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


def _found(t) -> str:
    return f"{str(t.dtype).replace('torch.', '')} {tuple(t.shape)} strides {tuple(t.stride())} on {t.device.type}"


class _Contract:
    """Collects (operand, what was found) of one call."""

    def __init__(self, device_type: Optional[str]):
        self.device_type, self.out = device_type, []

    def bad(self, name: str, what: str) -> None:
        self.out.append((name, what))

    def tensor(self, name, t, dtype=None, numel=None, min_numel=None, shape=None, contiguous=True) -> bool:
        """device, dtype, contiguity and extent of one operand; True if it may be inspected further."""
        if t is None:
            return False
        if not isinstance(t, torch.Tensor):
            self.bad(name, f"not a tensor: {type(t).__name__}")
            return False
        n = len(self.out)
        if self.device_type is not None and t.device.type != self.device_type:
            self.bad(name, f"device: on {t.device.type}, the kernel reads {self.device_type} memory")
        if dtype is not None and t.dtype != dtype:
            self.bad(name, f"dtype: the C entry reads {str(dtype).replace('torch.', '')}, found {_found(t)}")
        if contiguous and not t.is_contiguous():
            self.bad(name, f"stride: not contiguous, found {_found(t)}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            self.bad(name, f"extent: shape {tuple(shape)} expected, found {_found(t)}")
        if numel is not None and t.numel() != numel:
            self.bad(name, f"extent: {numel} elements expected, found {_found(t)}")
        if min_numel is not None and t.numel() < min_numel:
            self.bad(name, f"extent: the kernel reads {min_numel} elements, found {_found(t)}")
        return len(self.out) == n

    def cl(self, name, c, positions=None, n=None, dtype=BF16) -> bool:
        """a channels-last activation [N, D, H, W, Cpad]: contiguous, Cpad a multiple of 32 holding C."""
        if c is None:
            return False
        t = c.t
        ok = self.tensor(name, t, dtype=dtype)
        if t.dim() != 5 or t.shape[-1] % 32 or not 0 < c.C <= t.shape[-1]:
            self.bad(name, f"extent: [N, D, H, W, Cpad] with Cpad % 32 == 0 >= C = {c.C}, found {_found(t)}")
            return False
        if positions is not None and tuple(t.shape[1:4]) != tuple(positions):
            self.bad(name, f"extent: positions {tuple(positions)} expected, found {_found(t)}")
            ok = False
        if n is not None and t.shape[0] != n:
            self.bad(name, f"extent: batch {n} expected, found {_found(t)}")
            ok = False
        return ok

    def gn(self, a, with_affine: bool) -> None:
        s1, s2 = a["src1"], a.get("src2")
        if not self.cl("src1", s1):
            return
        self.cl("src2", s2, positions=s1.t.shape[1:4], n=s1.N)
        c_log = s1.C + (s2.C if s2 is not None else 0)
        if with_affine:
            self.tensor("gamma", a["gamma"], dtype=F32, min_numel=c_log)
            self.tensor("beta", a["beta"], dtype=F32, min_numel=c_log)
        return s1.N, s1.t.shape[-1] + (s2.t.shape[-1] if s2 is not None else 0)

    def attn_view(self, name, t, N, T, heads, hd, ld_hs, off) -> None:
        if not self.tensor(name, t, dtype=BF16):
            return
        ld, hs = ld_hs
        last = off + (N * T - 1) * ld + (heads - 1) * hs + hd
        if off < 0 or ld < 1 or hs < 0 or last > t.numel():
            self.bad(name, f"extent: the view (ld {ld}, hs {hs}, off {off}) of {N} x {T} rows, {heads} heads of {hd} ends at element {last}, found {_found(t)}")


def contract_violations(op: str, a: dict, device_type: Optional[str] = "cuda") -> List[Tuple[str, str]]:
    """What is wrong with the operands `a` (bound arguments by name) of the first-generation wrapper ops.<op>, which forwards data_ptr()
    unchecked: [(operand, what was found)].  device_type None skips the device rule (CPU tests).  The later wrappers check themselves
    and raise; their calls have no rules here."""
    c = _Contract(device_type)
    if op == "conv":
        s1, s2 = a["src1"], a.get("src2")
        if not c.cl("src1", s1):
            return c.out
        N, sp = s1.N, tuple(s1.t.shape[1:4])
        c.cl("src2", s2, positions=sp, n=N)
        c.tensor("weight", a["weight"], dtype=BF16)
        cp = pad32(a["cout"])
        osp = conv_extent(sp, a["k"], a["stride"], a["pad"], a["upsample"])
        c.tensor("bias", a.get("bias"), dtype=F32, min_numel=cp * (N if a.get("bias_per_sample") else 1))
        if a.get("residual") is not None and c.cl("residual", a["residual"]):
            c.tensor("residual", a["residual"].t, shape=(N,) + osp + (cp,))
        ct = s1.t.shape[-1] + (s2.t.shape[-1] if s2 is not None else 0)
        if a.get("prologue") is not None:
            for i, name in enumerate(("prologue[0]", "prologue[1]")):
                c.tensor(name, a["prologue"][i], dtype=F32, shape=(N, ct))
        if a.get("prologue_acc") is not None:
            c_log = s1.C + (s2.C if s2 is not None else 0)
            for i, name in enumerate(("prologue_acc gamma", "prologue_acc beta")):
                c.tensor(name, a["prologue_acc"][i], dtype=F32, min_numel=c_log)
            for name, s in (("src1.acc", s1), ("src2.acc", s2)):
                if s is not None and (s.acc is None or s.acc.dtype != torch.int64 or tuple(s.acc.shape[2:]) != (s.t.shape[-1], 2)):
                    c.bad(name, "extent: prologue_acc needs the producing conv's [N, stripes, Cpad, 2] int64 accumulators")
        if a.get("skip") is not None:
            c.cl("skip[0]", a["skip"][0], positions=osp, n=N)
            c.cl("skip[1]", a["skip"][1], positions=osp, n=N)
            c.tensor("skip[2]", a["skip"][2], dtype=BF16)
        if a.get("out") is not None:
            c.tensor("out", a["out"], shape=(N,) + osp + ((cp // 2) if a.get("geglu") else cp,))
        if a.get("ddim") is not None:
            x, scal, px0, uin = a["ddim"]
            M = N * osp[0] * osp[1] * osp[2]
            c.tensor("ddim x", x, dtype=F32, numel=M * a["cout"])
            c.tensor("ddim scalars", scal, dtype=F32, min_numel=4)
            c.tensor("ddim pred_x0", px0, dtype=F32, numel=M * a["cout"])
            if uin is not None:
                c.tensor("ddim unet_in", uin, dtype=BF16, numel=M * uin.shape[-1])
    elif op in ("groupnorm_stats", "groupnorm_fused", "groupnorm_apply_acc", "groupnorm_scale_shift_acc"):
        c.gn(a, True)
    elif op == "groupnorm_apply":
        hdr = c.gn(a, False)
        if hdr is not None:
            c.tensor("scale", a["scale"], dtype=F32, shape=hdr)
            c.tensor("shift", a["shift"], dtype=F32, shape=hdr)
    elif op == "film_fold":
        sc, sh = a["scale"], a["shift"]
        for name, t in (("scale", sc), ("shift", sh)):
            if c.tensor(name, t, dtype=F32, contiguous=False) and (t.dim() != 2 or t.stride(1) != 1 or t.shape[1] < a["C"]):
                c.bad(name, f"stride: [N, >= {a['C']}] rows with unit column stride, found {_found(t)}")
        if isinstance(sc, torch.Tensor) and isinstance(sh, torch.Tensor) and (sc.shape != sh.shape or sc.stride() != sh.stride()):
            c.bad("shift", f"stride: one row stride is forwarded for both tables, scale has {_found(sc)}, shift {_found(sh)}")
    elif op == "attention":
        N, H, hd = a["N"], a["heads"], a["head_dim"]
        c.attn_view("q", a["q"], N, a["Tq"], H, hd, a["ld_hs_q"], a["q_off"])
        c.attn_view("k", a["k"], N, a["Tkv"], H, hd, a["ld_hs_k"], a["k_off"])
        c.attn_view("v", a["v"], N, a["Tkv"], H, hd, a["ld_hs_v"], a["v_off"])
        c.attn_view("out", a["out"], N, a["Tq"], H, hd, a["ld_hs_o"], 0)
        c.tensor("kv_len", a.get("kv_len"), dtype=I32, shape=(N,))
    elif op == "resample2x":
        src = a["src"]
        if c.cl("src", src) and a.get("prologue") is not None:
            c.tensor("prologue[0]", a["prologue"][0], dtype=F32, shape=(src.N, src.t.shape[-1]))
            c.tensor("prologue[1]", a["prologue"][1], dtype=F32, shape=(src.N, src.t.shape[-1]))
    elif op == "layernorm":
        c.tensor("x", a["x"], dtype=BF16)
        if isinstance(a["x"], torch.Tensor):
            c.tensor("gamma", a["gamma"], dtype=F32, min_numel=a["x"].shape[-1])
            c.tensor("beta", a["beta"], dtype=F32, min_numel=a["x"].shape[-1])
    elif op == "geglu":
        if c.tensor("h", a["h"], dtype=BF16) and a["h"].shape[-1] != 2 * a["inner"]:
            c.bad("h", f"extent: rows of 2 * inner = {2 * a['inner']} expected, found {_found(a['h'])}")
    elif op == "add":
        c.tensor("a", a["a"], dtype=BF16)
        c.tensor("b", a["b"], dtype=BF16, numel=a["a"].numel() if isinstance(a["a"], torch.Tensor) else None)
    elif op == "linear_f32":
        x = a["x"]
        if c.tensor("x", x, dtype=F32, contiguous=False) and x.dim() == 2:      # the wrapper itself makes x contiguous
            O = a["W"].shape[0] if isinstance(a["W"], torch.Tensor) and a["W"].dim() == 2 else -1
            c.tensor("W", a["W"], dtype=F32, shape=(O, x.shape[1]))
            c.tensor("b", a.get("b"), dtype=F32, shape=(O,))
            out = a.get("out")
            if c.tensor("out", out, dtype=F32, contiguous=False) and (tuple(out.shape) != (x.shape[0], O) or out.stride(1) != 1):
                c.bad("out", f"stride: [{x.shape[0]}, {O}] rows with unit column stride, found {_found(out)}")
        elif isinstance(x, torch.Tensor) and x.dim() != 2:
            c.bad("x", f"extent: [M, I] expected, found {_found(x)}")
    elif op == "ddim_step":
        x = a["x"]
        if c.tensor("x", x, dtype=F32):
            Cx = x.shape[-1]
            M = x.numel() // Cx
            eps = a["eps"]
            if c.tensor("eps", eps, dtype=F32) and (eps.shape[-1] < Cx or eps.numel() != M * eps.shape[-1]):
                c.bad("eps", f"extent: {M} rows of >= {Cx} expected, found {_found(eps)}")
            c.tensor("scalars", a["scalars"], dtype=F32, min_numel=4)
            c.tensor("noise", a.get("noise"), dtype=F32, numel=M * Cx)
            c.tensor("pred_x0_out", a.get("pred_x0_out"), dtype=F32, numel=M * Cx)
            uin = a.get("unet_in")
            if c.tensor("unet_in", uin, dtype=BF16) and (uin.shape[-1] < Cx or uin.numel() != M * uin.shape[-1]):
                c.bad("unet_in", f"extent: {M} rows of >= {Cx} expected, found {_found(uin)}")
    return c.out


# ------------------------------------------------------------------------------------------------ the harness
EXEMPT = {
    # predicates and host helpers: no kernel runs
    "CL": "the channels-last container, not a call into the library",
    "pad32": "host arithmetic", "pad_bias": "host-side zero padding of a bias row", "is_f32": "host predicate",
    "require_gpu": "host predicate", "weights_token": "host cache key", "fp32_validation": "context manager of the fp32 validation mode",
    "interpolate_extent": "host arithmetic", "conv_fuses_prologue": "host predicate", "conv_fuses_skip": "host predicate",
    "conv_prologue_from_acc": "host predicate", "groupnorm_fused_ok": "host predicate", "has_stats": "host predicate",
    "has_any_stats": "host predicate", "stats_begin": "allocates the statistics arena", "stats_end": "releases the statistics arena",
    "replay_captured": "graph capture plumbing (shadowed runs are eager)", "timestep_embedding": "small fp32 table, test_sampler_exact_gpu.py",
    # layout movers: exact copies with their own bit-for-bit tests
    "to_cl": "layout copy, bit-for-bit test", "from_cl": "layout copy, bit-for-bit test", "unfold_cl": "layout copy, bit-for-bit test",
    "fold_weighted_cl": "weighted fold, its own exact test (test_split_gpu.py)",
    # fp32 validation mode: out of the shadow's scope (its bounds are for bf16 storage)
    "groupnorm_f32": "fp32 validation kernel, its own exact tests", "groupnorm_f32_film": "fp32 validation kernel, its own exact tests",
    # sampler and loss kernels: covered by their exact tests
    "ccdm_posterior_sample": "sampler kernel, test_sampler_exact_gpu.py", "ddim_step_vq": "sampler kernel, test_vq_gpu.py",
    "ddpm_step": "sampler kernel, test_progressive_gpu.py", "ddpm_step_x0": "sampler kernel, test_progressive_gpu.py",
    "inpaint_blend": "sampler kernel, test_inpaint_gpu.py", "lincomb4": "sampler kernel (PLMS), test_sampler_exact_gpu.py",
    "log_rows": "sampler log copy, test_progressive_gpu.py", "q_sample_rows": "loss kernel, test_losses_gpu.py",
    "loss_rows": "loss kernel, test_losses_gpu.py", "gauss_kl_rows": "loss kernel, test_aeloss_gpu.py",
    "gauss_sample_rows": "loss kernel, test_aeloss_gpu.py", "logit_stats": "loss kernel, test_aeloss_gpu.py",
}


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
           "attention", "resample2x", "layernorm", "geglu", "linear_f32", "ddim_step", "pack_conv_weight",
           "add", "gelu", "layernorm_rows", "embed_rows", "bert_embed", "interpolate2d", "patch_conv", "relu_cl", "lpips_tap", "volume_views_cl",
           "vq_nearest")


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
        for operand, what in contract_violations(name, b.arguments):     # before the real op runs: what the product passed
            self._rec("contract", math.inf, 0, 0, (), (("op", name), ("operand", operand), ("found", what)))
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
        self._args("film_fold", (scale, shift, film, C), {})
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
        lens = None if a["kv_len"] is None else [int(v) for v in a["kv_len"].cpu()]        # read back from the device
        plan = (("ws", 0 if lens is not None else self.lib.gg_attention_workspace_bytes(C.byref(d))), ("kvlen", int(lens is not None)))
        r = attention_ratio(qv, kv, vv, ov, a["scale"], seed, lens)
        self._rec("attention", r, N, N, (N, nh, hd, Tq, Tkv), plan)
        if lens is not None:
            self._rec("attention.kvlen", r, N, N, (N, nh, hd, Tq, Tkv), plan + (("lengths", tuple(lens)),))
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

    # -- text, 3-D, GAN and LPIPS networks
    def add(self, *args, **kw):
        self._pre()
        a = self._args("add", args, kw)
        out = self.real["add"](*args, **kw)
        torch.cuda.synchronize()
        self._rec("add", add_ratio(a["a"], a["b"], out), 1, 1, tuple(a["a"].shape))
        return out

    def gelu(self, *args, **kw):
        self._pre()
        a = self._args("gelu", args, kw)
        out = self.real["gelu"](*args, **kw)
        torch.cuda.synchronize()
        x = a["x"]
        self._rec("gelu", gelu_ratio(x, out), x.shape[0], x.shape[0], tuple(x.shape))
        return out

    def layernorm_rows(self, *args, **kw):
        self._pre()
        a = self._args("layernorm_rows", args, kw)
        out = self.real["layernorm_rows"](*args, **kw)
        torch.cuda.synchronize()
        x = a["x"]
        r = layernorm_rows_ratio(x.t, x.C, a["gamma"], a["beta"], a["eps"], out.t) if out.C == x.C else math.inf
        self._rec("layernorm_rows", r, x.N, x.N, tuple(x.t.shape) + (x.C,))
        return out

    def embed_rows(self, *args, **kw):
        self._pre()
        a = self._args("embed_rows", args, kw)
        out = self.real["embed_rows"](*args, **kw)
        torch.cuda.synchronize()
        ids = a["ids"]
        self._rec("embed_rows", embed_rows_ratio(ids, a["tok"], a["pos"], out), ids.shape[0], ids.shape[0],
                  tuple(ids.shape) + tuple(a["tok"].shape), (("bf16", int(a["bf16"])), ("pos", int(a["pos"] is not None))))
        return out

    def bert_embed(self, *args, **kw):
        self._pre()
        a = self._args("bert_embed", args, kw)
        out = self.real["bert_embed"](*args, **kw)
        torch.cuda.synchronize()
        ids = a["ids"]
        r = bert_embed_ratio(ids, a["type_ids"], a["word"], a["pos"], a["type_tab"], a["gamma"], a["beta"], a["eps"], out)
        self._rec("bert_embed", r, ids.shape[0], ids.shape[0], tuple(ids.shape) + tuple(a["word"].shape))
        return out

    def interpolate2d(self, *args, **kw):
        self._pre()
        a = self._args("interpolate2d", args, kw)
        out = self.real["interpolate2d"](*args, **kw)
        torch.cuda.synchronize()
        x = a["x"]
        self._rec("interpolate2d", interpolate2d_ratio(x, a["scale_factor"], a["mode"], out), x.shape[0], x.shape[0], tuple(x.shape),
                  (("mode", a["mode"]), ("scale_factor", float(a["scale_factor"]))))
        return out

    def patch_conv(self, *args, **kw):
        seed = self._pre()
        a = self._args("patch_conv", args, kw)
        res = self.real["patch_conv"](*args, **kw)
        torch.cuda.synchronize()
        src = a["src"]
        r, samples = patch_conv_ratio(src.t, self._weight(a["weight"]), a["alpha"], a["beta"], a["cout"], a["kd"], a["stride"], a["slope"],
                                      res.t, seed)
        if res.C != a["cout"]:
            r = math.inf
        self._rec("patch_conv", r, src.N, samples, tuple(src.t.shape) + (a["cout"],),
                  (("kd", a["kd"]), ("stride", a["stride"]), ("alpha", int(a["alpha"] is not None)), ("slope", float(a["slope"])),
                   ("out_f32", int(res.t.dtype == torch.float32))))
        return res

    def relu_cl(self, *args, **kw):
        self._pre()
        a = self._args("relu_cl", args, kw)
        before = a["x"].t.clone()
        res = self.real["relu_cl"](*args, **kw)
        torch.cuda.synchronize()
        r = relu_ratio(before, res.t) if res.t.data_ptr() == a["x"].t.data_ptr() else math.inf
        self._rec("relu_cl", r, before.shape[0], before.shape[0], tuple(before.shape))
        return res

    def volume_views_cl(self, *args, **kw):
        self._pre()
        a = self._args("volume_views_cl", args, kw)
        res = self.real["volume_views_cl"](*args, **kw)
        torch.cuda.synchronize()
        r = volume_views_ratio(a["x"], a["view"], a["n0"], a["n1"], a["shift"], a["scale"], a["out"])
        if res.C != 3 or res.t.data_ptr() != a["out"].data_ptr():
            r = math.inf
        n = a["n1"] - a["n0"]
        self._rec("volume_views_cl", r, n, n, tuple(a["x"].shape), (("view", a["view"]), ("n0", a["n0"]), ("n1", a["n1"]),
                                                                     ("bf16", int(a["out"].dtype == torch.bfloat16))))
        return res

    def lpips_tap(self, *args, **kw):
        self._pre()
        a = self._args("lpips_tap", args, kw)
        before = a["total"].clone() if (a["total"] is not None and a["accumulate"]) else None
        got, pooled = self.real["lpips_tap"](*args, **kw)
        torch.cuda.synchronize()
        r = lpips_tap_ratio(a["a"], a["b"], a["lin_w"], got, pooled, a["total"], before)
        if (pooled is not None) != bool(a["pool"]):
            r = math.inf
        n = a["a"].shape[0]
        self._rec("lpips_tap", r, n, n, tuple(a["a"].shape), (("pool", int(bool(a["pool"]))), ("accumulate", int(bool(a["accumulate"]))),
                                                               ("bf16", int(a["a"].dtype == torch.bfloat16))))
        return got, pooled

    def vq_nearest(self, *args, **kw):
        self._pre()
        a = self._args("vq_nearest", args, kw)
        rows = a["rows"]
        z = rows.reshape(-1, rows.shape[-1]).clone()              # st_out may be `rows` itself
        idx, st = self.real["vq_nearest"](*args, **kw)
        torch.cuda.synchronize()
        r, share = vq_ratio(z, a["codebook"], idx, st.reshape(z.shape[0], -1) if st is not None else None)
        self._rec("vq_nearest", r, z.shape[0], z.shape[0], tuple(rows.shape) + tuple(a["codebook"].shape), (("near_tie_share", share),))
        return idx, st

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

    def assert_within_bounds(self, N: Optional[int]) -> None:
        """N: the batch size every conv / GroupNorm / attention / patch_conv call must have run at (None where the network itself cuts
        its batch into chunks of several sizes, as LPIPS does: then only 'every sample of the call was checked' is required)."""
        assert self.records, "no kernel call was shadowed"
        bad = [r for r in self.records if not r.ratio <= 1.0]
        assert not bad, "kernel calls outside their bound:\n" + "\n".join(f"  {r.family} ratio {r.ratio:.3e} N={r.N} shape={r.shape} plan={dict(r.plan)}"
                                                                          for r in bad[:20])
        miss = [r for r in self.records if r.family.startswith(("conv", "groupnorm", "attention", "patch_conv"))]
        miss = [r for r in miss if r.samples != r.N or (N is not None and r.N != N)]
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
