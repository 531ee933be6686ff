"""Network blocks of the two GuideGen UNets and the KL autoencoder, executed by the HIP engine.

torch.nn.{ConvNd, GroupNorm, Linear, LayerNorm} objects appear here ONLY as parameter containers, so that
`state_dict()` has exactly the reference's names and shapes (SURVEY.md 8b "state-dict surface"); their ATen
`forward` is never called.  Each block's `run(...)` enqueues hand-written HIP kernels through `ops`.

Reference blocks mirrored (file:line relative to the reference tree):
  ResBlock / Upsample / Downsample / AttentionBlock / TimestepEmbedSequential
      ccdm/ddpm/models/unet_openai/unet.py:70-360, latentdiffusion/ldm/modules/diffusionmodules/openaimodel.py:74-375
  SpatialTransformer / BasicTransformerBlock / CrossAttention / GEGLU
      latentdiffusion/ldm/modules/attention.py:37-64,152-261
  ResnetBlock / AttnBlock2d / AttnBlock3d / Upsample / Downsample (AE, dims 2 and 3)
      latentdiffusion/ldm/modules/diffusionmodules/model.py:42-261
"""
from __future__ import annotations

import math
import weakref
from typing import List, Optional

import torch
import torch.nn as nn

from . import ops
from .ops import CL, pad32


def conv_nd(dims, *a, **k):
    return {1: nn.Conv1d, 2: nn.Conv2d, 3: nn.Conv3d}[dims](*a, **k)


def zero_module(m):
    """Reference initialisation of the last conv of each block (nn.py:68-74); only matters for fresh models."""
    for p in m.parameters():
        p.detach().zero_()
    return m


def _k3(w: torch.Tensor):
    """(kd, kh, kw) of a conv weight; 1-D and 2-D kernels are left-padded with 1s."""
    ks = tuple(w.shape[2:])
    return (1,) * (3 - len(ks)) + ks


class _Packed:
    """Cache of kernel-friendly repacks (bf16 MFMA tile order, padded fp32 biases) keyed by parameter version.
    Keys hold id(module), which Python reuses once a module is freed, and a new module's parameters can land on the freed storage with
    the same version counters: so a hit also requires the cached parameters to be the very same tensor objects (weak references)."""

    def __init__(self):
        self.store = {}

    def get(self, key, params, build):
        params = [p for p in params if p is not None]
        ver = tuple((p.data_ptr(), p._version) for p in params)
        hit = self.store.get(key)
        if hit is not None and hit[0] == ver and all(r() is p for r, p in zip(hit[2], params)):
            return hit[1]
        val = build()
        self.store[key] = (ver, val, [weakref.ref(p) for p in params])
        return val


PACKED = _Packed()


def packed_conv(mod: nn.Module, cin_pad: int, tag: str = ""):
    """(packed bf16 weight, padded fp32 bias) of a conv/linear container for inputs with `cin_pad` channels."""
    def build():
        w = mod.weight
        if w.ndim == 2:
            w = w[:, :, None]
        pw = ops.pack_conv_weight(w, cin_pad)
        pb = ops.pad_bias(getattr(mod, "bias", None), w.shape[0], w.device)
        return pw, pb
    return PACKED.get((id(mod), cin_pad, tag, ops.FP32), [mod.weight, getattr(mod, "bias", None)], build)


def packed_cat(mods: List[nn.Module], cin_pad: int, tag: str):
    """Several convs/linears sharing an input, fused along Cout (q|k|v projections)."""
    def build():
        ws = [m.weight if m.weight.ndim > 2 else m.weight[:, :, None] for m in mods]
        ws = [w.reshape(w.shape[0], w.shape[1], -1) for w in ws]
        w = torch.cat(ws, 0)
        bs = [m.bias if getattr(m, "bias", None) is not None else torch.zeros(m.weight.shape[0], device=w.device) for m in mods]
        pw = ops.pack_conv_weight(w, cin_pad)
        pb = ops.pad_bias(torch.cat(bs, 0), w.shape[0], w.device)
        return pw, pb
    params = [m.weight for m in mods] + [getattr(m, "bias", None) for m in mods]
    return PACKED.get((id(mods[0]), cin_pad, tag, ops.FP32), params, build)


def packed_geglu(proj: nn.Module, cin_pad: int):
    """GEGLU projection (attention.py:37-44) packed for the fused epilogue (gg_conv_desc.epilogue_geglu): rows in groups of 32 =
    [16 value rows j0..j0+15 | their 16 gate rows inner+j0..inner+j0+15], bias likewise."""
    def build():
        w, b = proj.weight, proj.bias
        inner = w.shape[0] // 2
        assert inner % 16 == 0
        j = torch.arange(inner, device=w.device).view(-1, 16)                       # [inner/16, 16] value rows
        order = torch.cat([j, j + inner], 1).reshape(-1)                            # value block, gate block, value block, ...
        pw = ops.pack_conv_weight(w[order][:, :, None], cin_pad)
        pb = ops.pad_bias(b[order] if b is not None else None, w.shape[0], w.device)
        return pw, pb
    return PACKED.get((id(proj), cin_pad, "geglu"), [proj.weight, getattr(proj, "bias", None)], build)


FUSE_GEGLU = True     # feed-forward projection with the GEGLU as its epilogue (False: projection, then gg_geglu)


def f32(p: torch.Tensor) -> torch.Tensor:
    return p.detach().float().contiguous()


def gn_params(norm: nn.GroupNorm):
    return f32(norm.weight), f32(norm.bias), norm.eps


# The GroupNorm kernel-choice ladder, one implementation per arm (gn_silu, norm_conv, the down ResBlock).  fp32 validation arm: a separate launch
def _gn_f32(h: CL, norm: nn.GroupNorm, act: bool, src2: Optional[CL] = None, film: Optional[torch.Tensor] = None) -> CL:
    return ops.groupnorm_f32_film(h, *gn_params(norm), film, act) if film is not None else ops.groupnorm_f32(h, *gn_params(norm), act, src2)


def _gn_direct(h: CL, norm: nn.GroupNorm, act: bool, src2: Optional[CL]) -> Optional[CL]:
    """No coefficient table: statistics + apply in ONE launch (small tensors), else apply from the producers' accumulators, else None"""
    if ops.groupnorm_fused_ok(h, src2):
        return ops.groupnorm_fused(h, *gn_params(norm), act, src2)
    return ops.groupnorm_apply_acc(h, *gn_params(norm), act, src2) if ops.has_stats(h, src2) else None


def _gn_coeffs(h: CL, norm: nn.GroupNorm, src2: Optional[CL] = None, film: Optional[torch.Tensor] = None, fold_acc: bool = True):
    """Per-(n, c) (scale, shift): the producers' accumulators folded (halo-tile producers: not 17..805 MB re-read) or a statistics pass; FiLM"""
    stats = ops.groupnorm_scale_shift_acc if fold_acc and ops.has_any_stats(h, src2) else ops.groupnorm_stats
    scale, shift = stats(h, *gn_params(norm), src2)
    if film is not None:
        ops.film_fold(scale, shift, film, h.C)
    return scale, shift


def gn_silu(h: CL, norm: nn.GroupNorm, act: bool, src2: Optional[CL] = None) -> CL:
    a = _gn_f32(h, norm, act, src2) if ops.is_f32(h.t) else _gn_direct(h, norm, act, src2)
    # nothing to apply from: ALWAYS a statistics pass here, also where 32-stripe accumulators exist (norm_conv folds those instead;
    # the asymmetry is kept as it was: removing it changes which kernels run)
    return a if a is not None else ops.groupnorm_apply(h, *_gn_coeffs(h, norm, src2, fold_acc=False), act, src2)


def norm_conv(h: CL, norm: nn.GroupNorm, act: bool, weight, bias, cout, src2: Optional[CL] = None, film: Optional[torch.Tensor] = None,
              **conv_kw) -> CL:
    """conv(act(GroupNorm(cat[h, src2]))), or with film (fp32 [N, >= 2C] rows [s | t], use_scale_shift_norm)
    conv(act(GroupNorm(h) * (1 + s) + t)): FiLM takes the coefficient arm, never the kernels that compute the coefficients inside another launch.
    Halo-tile convs (3x3(x3), stride 1, large extents): one stats pass, then normalise*affine(+SiLU) and the skip concat are
    fused into the conv's staging pass (applied once per staged element) -- the activation is never re-written to HBM.
    Gather-kernel convs: separate apply pass (measured: SiLU inside the latency-bound gather loop costs 26 vs 16.6 us/conv)."""
    if ops.is_f32(h.t):                      # (a FiLM norm takes no second source)
        return ops.conv(_gn_f32(h, norm, act, src2, film), weight, bias, cout, **conv_kw)
    if film is None and ops.conv_prologue_from_acc(h, cout, act, src2=src2, **conv_kw):
        # box conv + producers' sums: the conv folds them and normalises its staged box itself -- NO GroupNorm launch of any kind
        return ops.conv(h, weight, bias, cout, src2=src2, prologue_acc=gn_params(norm), prologue_silu=act, **conv_kw)
    fused = ops.conv_fuses_prologue(h, cout, src2=src2, **conv_kw)
    a = _gn_direct(h, norm, act, src2) if film is None and not fused else None
    if a is None:
        scale, shift = _gn_coeffs(h, norm, src2, film)
        if fused:
            return ops.conv(h, weight, bias, cout, src2=src2, prologue=(scale, shift), prologue_silu=act, **conv_kw)
        a = ops.groupnorm_apply(h, scale, shift, act, src2)
    return ops.conv(a, weight, bias, cout, **conv_kw)


def conv_of(mod, h: CL, *, src2: Optional[CL] = None, bias: Optional[torch.Tensor] = None, tag: str = "", norm=None, **conv_kw) -> CL:
    """conv(cat[h, src2]) with the weights of the conv / linear container `mod`, the one statement of "run this container as a conv":
    packed for the inputs' padded width (packed_conv's cache keys; a list of containers is fused along Cout under `tag` as packed_cat
    does, geglu=True packs as packed_geglu does), cout and the kernel extent read from the weight, pad = k // 2 unless given; every
    other keyword goes to ops.conv.  bias= replaces the packed bias (a per-sample time bias, conv2's bias + the skip's).
    norm=(GroupNorm container, act): conv(act(GroupNorm(cat[h, src2]))) through norm_conv, which also takes film=."""
    cin_pad = h.Cpad + (src2.Cpad if src2 is not None else 0)
    if isinstance(mod, (list, tuple)):
        (pw, pb), weights = packed_cat(list(mod), cin_pad, tag), [m.weight for m in mod]
    else:
        (pw, pb), weights = (packed_geglu(mod, cin_pad) if conv_kw.get("geglu") else packed_conv(mod, cin_pad, tag)), [mod.weight]
    k = _k3(weights[0])
    conv_kw.setdefault("pad", k[-1] // 2)
    args = (pw, pb if bias is None else bias, sum(w.shape[0] for w in weights))
    if norm is not None:
        return norm_conv(h, *norm, *args, src2=src2, k=k, **conv_kw)
    return ops.conv(h, *args, src2=src2, k=k, **conv_kw)


def qkv_attention(qkv: CL, heads: int, head_dim: int, scale: float, *, legacy: bool = False, kv_len: Optional[torch.Tensor] = None,
                  dtype=torch.bfloat16) -> CL:
    """Self-attention over fused q|k|v rows (the output of one 1x1 projection): softmax(scale q k^T) v per head, as an unpadded CL of
    heads * head_dim channels at qkv's positions.  Blocked order: q | k | v blocks of all heads' channels, heads of head_dim inside each
    block; legacy order: head-major, q | k | v per head.  kv_len: per-sample key lengths (ops.attention).  dtype: the output buffer's."""
    inner = heads * head_dim
    att = torch.empty(tuple(qkv.t.shape[:4]) + (inner,), dtype=dtype, device=qkv.t.device)
    ld_hs, step = ((qkv.Cpad, 3 * head_dim), head_dim) if legacy else ((qkv.Cpad, head_dim), inner)
    ops.attention(qkv.t, qkv.t, qkv.t, att, qkv.N, heads, head_dim, qkv.S, qkv.S, ld_hs, ld_hs, ld_hs, (inner, head_dim), scale,
                  q_off=0, k_off=step, v_off=2 * step, **({} if kv_len is None else {"kv_len": kv_len}))
    return CL(att, inner)


def layernorm_cl(x: CL, ln: nn.LayerNorm) -> CL:
    """LayerNorm over the logical channels of token rows: whole rows on gg_layernorm, padded rows on gg_layernorm_rows."""
    if x.C == x.Cpad:
        return CL(ops.layernorm(x.t, f32(ln.weight), f32(ln.bias), ln.eps), x.C)
    return ops.layernorm_rows(x, f32(ln.weight), f32(ln.bias), ln.eps)


def token_rows_f32(x: CL) -> torch.Tensor:
    """Plumbing: the logical lanes of bf16 token rows CL [B, 1, 1, T, Cpad] as fp32 [B, T, C]."""
    return x.t[:, 0, 0, :, :x.C].float()


class TimestepBlock(nn.Module):
    pass


class GroupNorm32(nn.GroupNorm):
    """Parameter container; statistics are fp32 in the HIP kernel as in the reference (nn.py:17-19)."""


def normalization(ch):
    return GroupNorm32(32, ch)


# ------------------------------------------------------------------------------------------------ UNet blocks
class Upsample(nn.Module):
    def __init__(self, channels, use_conv, dims=2, out_channels=None):
        super().__init__()
        self.channels, self.out_channels, self.use_conv, self.dims = channels, out_channels or channels, use_conv, dims
        if use_conv:
            self.conv = conv_nd(dims, channels, self.out_channels, 3, padding=1)

    def run(self, h: CL) -> CL:
        if not self.use_conv:                # nearest x2 (D too for dims == 3, unet.py:104-110): the resample kernel
            return ops.resample2x(h, True, self.dims == 3)
        return conv_of(self.conv, h, upsample=True)


class Downsample(nn.Module):
    def __init__(self, channels, use_conv, dims=2, out_channels=None):
        super().__init__()
        self.channels, self.out_channels, self.use_conv, self.dims = channels, out_channels or channels, use_conv, dims
        if use_conv:
            self.op = conv_nd(dims, channels, self.out_channels, 3, stride=2, padding=1)
        else:
            assert self.channels == self.out_channels
            self.op = {1: nn.AvgPool1d, 2: nn.AvgPool2d, 3: nn.AvgPool3d}[dims](2, 2)     # parameter-free container, never called

    def run(self, h: CL) -> CL:
        if not self.use_conv:                # 2x average pool (stride (2, 2, 2) for dims == 3): the resample kernel, no GroupNorm sums
            return ops.resample2x(h, False, self.dims == 3)
        # the output is a skip tensor: a decoder GroupNorm over cat[h, skip] takes its statistics from accumulators only if BOTH sources
        # carry them, so leave the sums behind also below ops.GN_ACC_MIN_ELEMS (the 16x16 x 320 tensor of the latent UNet: otherwise
        # that norm falls back to a statistics launch + an apply launch)
        small = (h.S // (4 if self.dims == 2 else 8)) * pad32(self.out_channels) >= (1 << 16)
        return conv_of(self.op, h, stride=2, want_stats=small)


class ResBlock(TimestepBlock):
    """GN+SiLU -> conv3 (+timestep bias) -> GN+SiLU -> conv3 (+skip).  The timestep projection
    `emb_layers` is folded into conv1's per-sample bias (SURVEY.md 2.3 "timestep-embed epilogue").
    use_scale_shift_norm (FiLM): emb_layers gives per-sample rows [s | t] (2C) instead, conv1 keeps its own bias, and the out-norm is
    GroupNorm(h) * (1 + s) + t through gg_film_fold on its per-(n, c) coefficients.  up / down (resblock_updown): GN+SiLU -> nearest x2
    / 2x average pool -> conv1 on the h path, the same resampling of x as the residual (unet.py:238-245)."""

    def __init__(self, channels, emb_channels, dropout, out_channels=None, use_conv=False, use_scale_shift_norm=False,
                 dims=2, use_checkpoint=False, up=False, down=False):
        super().__init__()
        self.channels, self.emb_channels = channels, emb_channels
        self.out_channels = out_channels or channels
        self.use_scale_shift_norm, self.dims = use_scale_shift_norm, dims
        self.in_layers = nn.Sequential(normalization(channels), nn.SiLU(), conv_nd(dims, channels, self.out_channels, 3, padding=1))
        self.updown = up or down
        if up:
            self.h_upd, self.x_upd = Upsample(channels, False, dims), Upsample(channels, False, dims)
        elif down:
            self.h_upd, self.x_upd = Downsample(channels, False, dims), Downsample(channels, False, dims)
        else:
            self.h_upd = self.x_upd = nn.Identity()
        self.up, self.down = up, down
        self.emb_layers = nn.Sequential(nn.SiLU(), nn.Linear(emb_channels, 2 * self.out_channels if use_scale_shift_norm else self.out_channels))
        self.out_layers = nn.Sequential(normalization(self.out_channels), nn.SiLU(), nn.Dropout(p=dropout),
                                        zero_module(conv_nd(dims, self.out_channels, self.out_channels, 3, padding=1)))
        if self.out_channels == channels:
            self.skip_connection = nn.Identity()
        elif use_conv:
            self.skip_connection = conv_nd(dims, channels, self.out_channels, 3, padding=1)
        else:
            self.skip_connection = conv_nd(dims, channels, self.out_channels, 1)

    @property
    def time_bias_width(self) -> int:
        """fp32 columns per sample of this block's time-bias row: Cout_pad, or 2 * Cout_pad of FiLM rows [s | t] (s, t at 0 and Cout)."""
        return pad32(self.out_channels) * (2 if self.use_scale_shift_norm else 1)

    def time_bias(self, emb: torch.Tensor, out: torch.Tensor) -> None:
        """out[M, Cout_pad] = conv1.bias + Linear(SiLU(emb))  (unet.py:251-260); FiLM: out[M, 2 Cout_pad] = Linear(SiLU(emb)) = [s | t]."""
        lin, c1 = self.emb_layers[1], self.in_layers[2]
        if self.use_scale_shift_norm:
            ops.linear_f32(emb, f32(lin.weight), f32(lin.bias), act_in=True, out=out)
            return
        b = PACKED.get((id(self), "tb"), [lin.bias, c1.bias], lambda: (f32(lin.bias) + f32(c1.bias)))
        ops.linear_f32(emb, f32(lin.weight), b, act_in=True, out=out)

    def run(self, h: CL, tbias: torch.Tensor, src2: Optional[CL] = None, want_stats: bool = False) -> CL:
        """want_stats: the consumer of this block's output folds GroupNorm sums itself (an AttentionBlock's norm in front of its box-kernel
        qkv conv, or a tiny-image ResBlock): conv2 leaves them even for tensors below ops.GN_ACC_MIN_ELEMS."""
        if self.use_scale_shift_norm or self.updown:
            return self._run_options(h, tbias, src2, want_stats)
        c1, c2, sk = self.in_layers[2], self.out_layers[3], self.skip_connection
        # (running the 1x1 skip projection on a side stream beside the GN -> conv1 -> GN chain was measured slower: the fork / join
        # edges in the hipGraph cost more than the overlap saves, 3.03 vs 2.69 ms per latent-UNet forward)
        res, kw2 = h, {}
        if not isinstance(sk, nn.Identity):
            h1_shape = CL(h.t[..., :1].expand(*h.t.shape[:4], pad32(self.out_channels)), self.out_channels)     # shape carrier for the query (no data read)
            if _k3(sk.weight) == (1, 1, 1) and ops.conv_fuses_skip(h1_shape, self.out_channels, h, src2, k=_k3(c1.weight)):
                # 1x1 skip projection K-concatenated into conv2 (gg_conv_desc.skip_src1): no skip launch, no residual round trip
                pws, pbs = packed_conv(sk, h.Cpad + (src2.Cpad if src2 is not None else 0))
                pb2 = packed_conv(c2, pad32(self.out_channels))[1]
                b2s = PACKED.get((id(self), "b2s"), [c2.bias, sk.bias], lambda: pb2 + pbs)            # conv2 bias + skip bias
                res, kw2 = None, {"skip": (h, src2, pws), "bias": b2s}
            else:
                res = conv_of(sk, h, src2=src2)
        h1 = conv_of(c1, h, src2=src2, norm=(self.in_layers[0], True), bias=tbias, bias_per_sample=True)
        assert h1.Cpad == pad32(self.out_channels)
        return conv_of(c2, h1, norm=(self.out_layers[0], True), residual=res, want_stats=want_stats, **kw2)

    def _run_options(self, h: CL, tbias: torch.Tensor, src2: Optional[CL], want_stats: bool) -> CL:
        """The same block with use_scale_shift_norm and / or up / down (unet.py:238-259)."""
        c1, c2, n1, sk = self.in_layers[2], self.out_layers[3], self.in_layers[0], self.skip_connection
        film = tbias.view(h.N, -1) if self.use_scale_shift_norm else None     # per-sample rows [s | t]
        b1 = {} if film is not None else {"bias": tbias, "bias_per_sample": True}       # FiLM: conv1 keeps its own bias
        x = h
        if self.updown:
            if src2 is not None:
                raise RuntimeError("an up / down ResBlock takes no skip concat")
            x = self.x_upd.run(h)                                             # residual source: x_upd(x)
            if self.up:
                # nearest x2 commutes with the pointwise GN+SiLU: normalise at low resolution, conv1 upsamples while it gathers
                h1 = conv_of(c1, h, norm=(n1, True), upsample=True, **b1)
            else:
                # avgpool(SiLU(GN(h))) in one resample launch from the per-(n, c) coefficients, then conv1
                if ops.is_f32(h.t):
                    a = ops.resample2x(_gn_f32(h, n1, True), False, self.dims == 3)
                else:
                    a = ops.resample2x(h, False, self.dims == 3, prologue=_gn_coeffs(h, n1), act=True)
                h1 = conv_of(c1, a, **b1)
        else:
            h1 = conv_of(c1, h, src2=src2, norm=(n1, True), **b1)
        res = x if isinstance(sk, nn.Identity) else conv_of(sk, x, src2=src2)
        return conv_of(c2, h1, norm=(self.out_layers[0], True), residual=res, want_stats=want_stats, film=film)


class AttentionBlock(nn.Module):
    """GN -> qkv 1x1 -> QKVAttentionLegacy -> proj 1x1 + x, with flash attention tiles (no TxT buffer)."""

    def __init__(self, channels, num_heads=1, num_head_channels=-1, use_checkpoint=False, use_new_attention_order=False):
        super().__init__()
        self.new_order = use_new_attention_order
        self.channels = channels
        if num_head_channels == -1:
            self.num_heads = num_heads
        else:
            assert channels % num_head_channels == 0, \
                f"q,k,v channels {channels} is not divisible by num_head_channels {num_head_channels}"
            self.num_heads = channels // num_head_channels
        self.norm = normalization(channels)
        self.qkv = conv_nd(1, channels, channels * 3, 1)
        self.proj_out = zero_module(conv_nd(1, channels, channels, 1))

    def run(self, h: CL) -> CL:
        ch = self.channels // self.num_heads
        qkv = conv_of(self.qkv, h, norm=(self.norm, False))
        # (q ch^-1/4)(k ch^-1/4) == scale 1/sqrt(ch) on q k^T in both orders (unet.py:352-354,379-385); QKVAttention (new order) is the
        # blocked layout, QKVAttentionLegacy the head-major one
        att = qkv_attention(qkv, self.num_heads, ch, 1.0 / math.sqrt(ch), legacy=not self.new_order, dtype=h.t.dtype)
        return conv_of(self.proj_out, att, residual=h)


# ------------------------------------------------------------------------------------------------ SpatialTransformer
class GEGLU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out * 2)


class FeedForward(nn.Module):
    def __init__(self, dim, dim_out=None, mult=4, glu=True, dropout=0.0):
        super().__init__()
        if not glu:
            raise NotImplementedError("non-gated FeedForward is not used by BasicTransformerBlock")
        inner = int(dim * mult)
        self.inner = inner
        self.net = nn.Sequential(GEGLU(dim, inner), nn.Dropout(dropout), nn.Linear(inner, dim_out or dim))


class CrossAttention(nn.Module):
    def __init__(self, query_dim, context_dim=None, heads=8, dim_head=64, dropout=0.0):
        super().__init__()
        inner = dim_head * heads
        self.heads, self.dim_head, self.inner = heads, dim_head, inner
        self.scale = dim_head ** -0.5
        context_dim = context_dim or query_dim
        self.to_q = nn.Linear(query_dim, inner, bias=False)
        self.to_k = nn.Linear(context_dim, inner, bias=False)
        self.to_v = nn.Linear(context_dim, inner, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, query_dim), nn.Dropout(dropout))

    def run(self, xn: CL, context: Optional[CL], residual: CL) -> CL:
        """to_out(attn(to_q(xn), to_k(ctx), to_v(ctx))) + residual; xn/context are token rows as CL [N,1,1,T,C]."""
        inner, hd = self.inner, self.dim_head
        if context is None:
            att = qkv_attention(conv_of([self.to_q, self.to_k, self.to_v], xn, tag="qkv"), self.heads, hd, self.scale)
        else:
            qc, kvc = conv_of(self.to_q, xn), conv_of([self.to_k, self.to_v], context, tag="kv")
            att = CL(torch.empty(tuple(xn.t.shape[:4]) + (inner,), dtype=torch.bfloat16, device=xn.t.device), inner)
            ops.attention(qc.t, kvc.t, kvc.t, att.t, xn.N, self.heads, hd, xn.S, context.S, (qc.Cpad, hd), (kvc.Cpad, hd), (kvc.Cpad, hd),
                          (inner, hd), self.scale, q_off=0, k_off=0, v_off=inner)
        return conv_of(self.to_out[0], att, residual=residual)


class BasicTransformerBlock(nn.Module):
    def __init__(self, dim, n_heads, d_head, dropout=0.0, context_dim=None, gated_ff=True, checkpoint=True):
        super().__init__()
        self.attn1 = CrossAttention(query_dim=dim, heads=n_heads, dim_head=d_head, dropout=dropout)
        self.ff = FeedForward(dim, dropout=dropout, glu=gated_ff)
        self.attn2 = CrossAttention(query_dim=dim, context_dim=context_dim, heads=n_heads, dim_head=d_head, dropout=dropout)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(dim), nn.LayerNorm(dim), nn.LayerNorm(dim)

    def run(self, x: CL, context: Optional[CL]) -> CL:
        x = self.attn1.run(layernorm_cl(x, self.norm1), None, x)
        x = self.attn2.run(layernorm_cl(x, self.norm2), context, x)
        y = layernorm_cl(x, self.norm3)
        proj, lin2 = self.ff.net[0].proj, self.ff.net[2]
        if FUSE_GEGLU and self.ff.inner % 16 == 0:
            ggcl = conv_of(proj, y, geglu=True)                                    # value * gelu(gate) from the fp32 accumulators
        else:
            ggcl = CL(ops.geglu(conv_of(proj, y).t, self.ff.inner), self.ff.inner)
        return conv_of(lin2, ggcl, residual=x)


class SpatialTransformer(nn.Module):
    def __init__(self, in_channels, n_heads, d_head, depth=1, dropout=0.0, context_dim=None):
        super().__init__()
        self.in_channels = in_channels
        inner = n_heads * d_head
        self.inner = inner
        self.norm = nn.GroupNorm(num_groups=32, num_channels=in_channels, eps=1e-6, affine=True)
        self.proj_in = nn.Conv2d(in_channels, inner, kernel_size=1, stride=1, padding=0)
        self.transformer_blocks = nn.ModuleList(
            [BasicTransformerBlock(inner, n_heads, d_head, dropout=dropout, context_dim=context_dim) for _ in range(depth)])
        self.proj_out = zero_module(nn.Conv2d(inner, in_channels, kernel_size=1, stride=1, padding=0))

    def run(self, h: CL, context: Optional[CL]) -> CL:
        x = conv_of(self.proj_in, h, norm=(self.norm, False))                        # 'b c h w -> b (h w) c' is free in CL
        for blk in self.transformer_blocks:
            x = blk.run(x, context)
        return conv_of(self.proj_out, x, residual=h)


class TimestepEmbedSequential(nn.Sequential, TimestepBlock):
    """Dispatches (h, time-bias, context, skip) to the children that take them (unet.py:70-84)."""

    def run(self, h: CL, tbias_of, context: Optional[CL], skip: Optional[CL] = None) -> CL:
        layers = list(self)
        for i, layer in enumerate(layers):
            if isinstance(layer, ResBlock):
                # the next layer's norm can be folded into its (box-kernel) conv from this block's output sums
                nxt = layers[i + 1] if i + 1 < len(layers) else None
                h = layer.run(h, tbias_of(layer), skip, want_stats=isinstance(nxt, (AttentionBlock, SpatialTransformer)))
                skip = None
            elif isinstance(layer, SpatialTransformer):
                h = layer.run(h, context)
            elif isinstance(layer, (AttentionBlock, Upsample, Downsample)):
                h = layer.run(h)
            elif isinstance(layer, (nn.Conv1d, nn.Conv2d, nn.Conv3d)):
                h = conv_of(layer, h)
            else:
                raise TypeError(f"no HIP execution rule for {type(layer).__name__}")
        if skip is not None:
            raise RuntimeError("skip tensor was not consumed by a ResBlock")
        return h


# ------------------------------------------------------------------------------------------------ AE blocks
def Normalize(in_channels, num_groups=32):
    return nn.GroupNorm(num_groups=num_groups, num_channels=in_channels, eps=1e-6, affine=True)


class AEUpsample(nn.Module):
    """nearest x2 then conv3 (model.py:42-58); dims == 3 doubles D as well (the conv's fused upsample with kd == 3)."""

    def __init__(self, in_channels, with_conv, dims=2):
        super().__init__()
        if not with_conv:
            raise NotImplementedError("resamp_with_conv=False is not supported (the conv-free AE resampling is used by no shipped config)")
        self.with_conv, self.dims = with_conv, dims
        self.conv = conv_nd(dims, in_channels, in_channels, kernel_size=3, stride=1, padding=1)

    def run(self, h: CL) -> CL:
        return conv_of(self.conv, h, upsample=True)


class AEDownsample(nn.Module):
    """pad (0,1,0,1[,0,1]) then stride-2 valid conv (model.py:75-79) = conv with leading pad 0, trailing pad 1 on every spatial axis."""

    def __init__(self, in_channels, with_conv, dims=2):
        super().__init__()
        if not with_conv:
            raise NotImplementedError("resamp_with_conv=False is not supported (the conv-free AE resampling is used by no shipped config)")
        self.with_conv, self.dims = with_conv, dims
        self.conv = conv_nd(dims, in_channels, in_channels, kernel_size=3, stride=2, padding=0)

    def run(self, h: CL) -> CL:
        return conv_of(self.conv, h, stride=2, pad=0)


class ResnetBlock(nn.Module):
    def __init__(self, *, in_channels, out_channels=None, conv_shortcut=False, dropout=0.0, temb_channels=0, dims=2):
        super().__init__()
        assert dims in (2, 3) and temb_channels == 0 and not conv_shortcut
        out_channels = in_channels if out_channels is None else out_channels
        self.in_channels, self.out_channels, self.dims = in_channels, out_channels, dims
        self.norm1 = Normalize(in_channels)
        self.conv1 = conv_nd(dims, in_channels, out_channels, 3, 1, 1)
        self.norm2 = Normalize(out_channels)
        self.dropout = nn.Dropout(dropout)
        self.conv2 = conv_nd(dims, out_channels, out_channels, 3, 1, 1)
        if in_channels != out_channels:
            self.nin_shortcut = conv_nd(dims, in_channels, out_channels, 1, 1, 0)

    def run(self, h: CL) -> CL:
        h1 = conv_of(self.conv1, h, norm=(self.norm1, True))
        res = conv_of(self.nin_shortcut, h) if self.in_channels != self.out_channels else h
        return conv_of(self.conv2, h1, norm=(self.norm2, True), residual=res)


ATTN_HEAD_DIMS = (32, 64, 128, 256, 384, 512)          # head dims gg_attention_forward has kernels for


class AttnBlock2d(nn.Module):
    """Single-head attention over c channels, scale c^-1/2 (model.py:209-261); q|k|v fused into one 1x1 conv."""
    dims = 2

    def __init__(self, in_channels):
        super().__init__()
        self.in_channels = in_channels
        self.norm = Normalize(in_channels)
        self.q = conv_nd(self.dims, in_channels, in_channels, 1, 1, 0)
        self.k = conv_nd(self.dims, in_channels, in_channels, 1, 1, 0)
        self.v = conv_nd(self.dims, in_channels, in_channels, 1, 1, 0)
        self.proj_out = conv_nd(self.dims, in_channels, in_channels, 1, 1, 0)

    def run(self, h: CL) -> CL:
        Cc = self.in_channels
        qkv = conv_of([self.q, self.k, self.v], h, tag="qkv", norm=(self.norm, False))
        return conv_of(self.proj_out, qkv_attention(qkv, 1, Cc, int(Cc) ** -0.5, dtype=h.t.dtype), residual=h)


class AttnBlock3d(AttnBlock2d):
    """The same block on volumes (model.py:154-206): 1x1x1 Conv3d containers, T = D * H * W tokens of one head of c channels.  The
    channels-last token order is (d, h, w) where the reference flattens its (h, w, d)-named axes in the same memory order, and attention
    is invariant under a common permutation of queries and keys anyway.  The head dim is the channel count: one the attention kernel has
    no instance for is refused here, on the host."""
    dims = 3

    def __init__(self, in_channels):
        if in_channels not in ATTN_HEAD_DIMS:
            raise NotImplementedError(f"AttnBlock3d: head_dim = {in_channels} is not supported (single-head attention over all channels; "
                                      f"the attention kernel has head_dim in {ATTN_HEAD_DIMS})")
        super().__init__(in_channels)
