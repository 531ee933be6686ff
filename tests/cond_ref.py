"""Independent torch restatement of the cond stages (ldm/modules/encoders/modules.py:22-136 with ldm/modules/x_transformer.py) for
machines without the reference tree: plain fp32 CPU torch on a state_dict, and torch.nn.functional.interpolate's index rules written
out (aten/src/ATen/native/UpSample.h, align_corners=False, scale factor given, no recompute_scale_factor).  Test infrastructure only.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

f32 = np.float32


# ------------------------------------------------------------------------------------------------ embedders
def class_embed(sd, labels, prefix=""):
    return sd[prefix + "embedding.weight"][labels.long()[:, None]]


def transformer_embed(sd, tokens, n_layer, heads=8, dim_head=64, prefix="transformer."):
    """TransformerWrapper(attn_layers=Encoder(dim, depth))(tokens, return_embeddings=True), no mask, eval mode."""
    tokens = tokens.long()
    B, T = tokens.shape
    x = sd[prefix + "token_emb.weight"][tokens] + sd[prefix + "pos_emb.emb.weight"][:T][None]
    dim = x.shape[-1]
    ln = lambda v, p: F.layer_norm(v, (dim,), sd[p + "weight"], sd[p + "bias"], 1e-5)
    for i in range(n_layer):
        a, f = (f"{prefix}attn_layers.layers.{2 * i + j}." for j in (0, 1))
        h = ln(x, a + "0.")
        q, k, v = (F.linear(h, sd[a + f"1.to_{n}.weight"]).view(B, T, heads, dim_head).transpose(1, 2) for n in "qkv")
        att = torch.softmax(q @ k.transpose(-1, -2) * dim_head ** -0.5, -1) @ v
        x = x + F.linear(att.transpose(1, 2).reshape(B, T, heads * dim_head), sd[a + "1.to_out.weight"], sd[a + "1.to_out.bias"])
        h = ln(x, f + "0.")
        h = F.gelu(F.linear(h, sd[f + "1.net.0.0.weight"], sd[f + "1.net.0.0.bias"]))
        x = x + F.linear(h, sd[f + "1.net.2.weight"], sd[f + "1.net.2.bias"])
    return ln(x, prefix + "norm.")


def gelu_f64(x):
    """erf-form GELU in fp64 with the left tail through erfc (1 + erf cancels there)."""
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


# ------------------------------------------------------------------------------------------------ interpolate
def out_extent(n_in, s):
    return int(math.floor(float(n_in) * float(s)))


def coord_scale(s):
    return f32(1.0 / float(s))                      # (float)(1.0 / scale): the division in double, one rounding


def nearest_index(n_in, n_out, scale):
    dst = np.arange(n_out).astype(f32)
    return np.minimum(np.floor(dst * scale).astype(np.int64), n_in - 1)


def _src(n_out, scale):
    dst = np.arange(n_out).astype(f32)
    return (scale * (dst + f32(0.5)) - f32(0.5)).astype(f32)


def linear_taps(n_in, n_out, scale):
    src = np.maximum(_src(n_out, scale), f32(0.0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = np.clip(src - i0.astype(f32), f32(0.0), f32(1.0)).astype(f32)
    return [i0, i1], [(f32(1.0) - l1).astype(f32), l1]


def cubic_taps(n_in, n_out, scale):
    src = _src(n_out, scale)
    i = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    t = np.clip(src - i.astype(f32), f32(0.0), f32(1.0)).astype(f32)
    A = f32(-0.75)
    c1 = lambda x: (((A + f32(2.0)) * x - (A + f32(3.0))) * x * x + f32(1.0)).astype(f32)
    c2 = lambda x: (((A * x - f32(5.0) * A) * x + f32(8.0) * A) * x - f32(4.0) * A).astype(f32)
    one = f32(1.0)
    w = [c2(t + one), c1(t), c1(one - t), c2((one - t) + one)]
    return [np.clip(i - 1 + j, 0, n_in - 1) for j in range(4)], w


def area_windows(n_in, n_out):
    return [((i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)) for i in range(n_out)]


def _separable(x, taps_h, taps_w):
    """sum_j (sum_k x[.., ih_j, iw_k] * ww_k) * wh_j: along W first, taps in ascending order, every product and sum rounded to fp32."""
    (ih, wh), (iw, ww) = taps_h, taps_w
    out = None
    for j in range(len(ih)):
        rows = x[..., torch.from_numpy(ih[j]), :]
        a = None
        for k in range(len(iw)):
            term = rows[..., torch.from_numpy(iw[k])] * torch.from_numpy(ww[k])
            a = term if a is None else a + term
        a = a * torch.from_numpy(wh[j])[:, None]
        out = a if out is None else out + a
    return out


def interpolate(x, s, mode):
    """F.interpolate(x, scale_factor=s, mode=mode) of an [N, C, H, W] CPU tensor, in x's dtype (fp32: each operation rounded once)."""
    H, W = x.shape[-2:]
    Ho, Wo = out_extent(H, s), out_extent(W, s)
    sc = coord_scale(s)
    if mode == "nearest":
        return x[..., torch.from_numpy(nearest_index(H, Ho, sc)), :][..., torch.from_numpy(nearest_index(W, Wo, sc))]
    if mode in ("bilinear", "bicubic"):
        taps = linear_taps if mode == "bilinear" else cubic_taps
        return _separable(x, taps(H, Ho, sc), taps(W, Wo, sc))
    if mode == "area":
        out = torch.empty(x.shape[:-2] + (Ho, Wo), dtype=x.dtype)
        for oh, (h0, h1) in enumerate(area_windows(H, Ho)):
            for ow, (w0, w1) in enumerate(area_windows(W, Wo)):
                acc = torch.zeros(x.shape[:-2], dtype=x.dtype)
                for ih in range(h0, h1):
                    for iw in range(w0, w1):
                        acc = acc + x[..., ih, iw]
                out[..., oh, ow] = acc / float(h1 - h0) / float(w1 - w0)         # ATen: sum / kh / kw, two roundings
        return out
    raise ValueError(mode)


def spatial_rescale(sd, x, n_stages, method, multiplier, prefix=""):
    for _ in range(n_stages):
        x = interpolate(x, multiplier, method)
    w = sd.get(prefix + "channel_mapper.weight")
    if w is not None:
        x = F.conv2d(x, w, sd.get(prefix + "channel_mapper.bias"))
    return x


# ------------------------------------------------------------------------------------------------ shared test cases
MODES = ("nearest", "bilinear", "bicubic", "area")
EXACT_SHAPES = ((1, 1, 12, 8), (2, 3, 12, 8), (1, 1, 13, 10), (2, 3, 13, 10))        # planes 12 x 8 and 13 x 10, N * C in {1, 6}
GENERAL_MULTIPLIERS = (0.75, 1.5, 0.3)


def exact_multipliers(mode):
    """Multipliers at which every tap weight is a small dyadic fraction (bicubic at 4 has weights that are not)."""
    return (0.5, 2, 0.25) if mode == "bicubic" else (0.5, 2, 0.25, 4)


def exact_input(shape, seed=0):
    """Integer-valued fp32 planes in [-8, 8]: with the dyadic weights above every product and partial sum is exact in fp32."""
    return torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(seed)).float()


def bf16_ulp(ref):
    """Spacing of bf16 numbers at |ref| (fp64 tensor): 2^(floor(log2 |ref|) - 7), the smallest normal's spacing below it."""
    a = ref.abs().double().clamp_min(2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 7)
