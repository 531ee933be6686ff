"""Cond stages of the LDM family on the HIP engine: the classes of the reference's ldm/modules/encoders/modules.py that a
`cond_stage_config` can name and that need nothing from outside the checkpoint.

  ClassEmbedder        modules.py:22-34     batch[key] -> embedding rows [B, 1, embed_dim]                 gg_embed_rows (fp32, exact)
  TransformerEmbedder  modules.py:37-51     tokens [B, T] -> TransformerWrapper(Encoder) embeddings        gg_embed_rows (bf16 token rows),
  BERTEmbedder         modules.py:81-104    the same network behind the (refused) BERT tokenizer           LayerNorm, 1x1 convs, attention, gg_gelu
  SpatialRescaler      modules.py:107-136   n_stages x F.interpolate(scale_factor) [+ 1x1 channel_mapper]  gg_interpolate2d_f32 [+ conv]

torch.nn modules appear only as parameter containers, so that `state_dict()` carries the reference's names and shapes (those of
ldm/modules/x_transformer.py: layers at transformer.attn_layers.layers.{2i} / {2i+1}, the norm under .0, the block under .1); their ATen
forward is never called.  Sampling only: eval mode, device tensors, no masks, no cross-attention inside the encoder.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .blocks import f32, packed_cat, packed_conv
from .ops import CL

DIM_HEAD = 64          # x_transformer.DEFAULT_DIM_HEAD; AttentionLayers' default of 8 heads: inner 512 whatever `dim` is
HEADS = 8


def _eval_only(mod: nn.Module) -> None:
    if mod.training:
        raise RuntimeError(f"{type(mod).__name__}: training mode is not supported (this engine implements sampling only; call .eval())")


def _check_tokens(who: str, tokens) -> None:
    if (not isinstance(tokens, torch.Tensor) or tokens.dim() != 2 or tokens.is_floating_point() or tokens.is_complex()
            or tokens.dtype == torch.bool):
        what = f"{tokens.dtype} {tuple(tokens.shape)}" if isinstance(tokens, torch.Tensor) else type(tokens).__name__
        raise ValueError(f"{who}: tokens must be an integer tensor of rank 2 [B, T], got {what} (the caller tokenises)")


# ------------------------------------------------------------------------------------------------ ClassEmbedder
class ClassEmbedder(nn.Module):
    def __init__(self, embed_dim, n_classes=1000, key="class"):
        super().__init__()
        self.key = key
        self.embedding = nn.Embedding(n_classes, embed_dim)

    @torch.no_grad()
    def forward(self, batch, key=None):
        """batch[key] integer [B] -> fp32 [B, 1, embed_dim]: the rows of embedding.weight, copied exactly (for use in crossattn)."""
        _eval_only(self)
        c = batch[self.key if key is None else key]
        if not isinstance(c, torch.Tensor) or c.dim() != 1:
            raise ValueError(f"ClassEmbedder: batch[{(self.key if key is None else key)!r}] must be an integer tensor of rank 1 [B]")
        _check_tokens("ClassEmbedder", c[:, None])
        ops.require_gpu(c, "ClassEmbedder.forward")
        return ops.embed_rows(c[:, None], f32(self.embedding.weight))


# ------------------------------------------------------------------------------------------------ x_transformer containers
class AbsolutePositionalEmbedding(nn.Module):
    def __init__(self, dim, max_seq_len):
        super().__init__()
        self.emb = nn.Embedding(max_seq_len, dim)
        nn.init.normal_(self.emb.weight, std=0.02)


class Attention(nn.Module):
    """Self-attention of x_transformer.Attention with its defaults (no mask, no memory, no talking heads): to_q / to_k / to_v without
    bias, to_out with."""

    def __init__(self, dim, dim_head=DIM_HEAD, heads=HEADS):
        super().__init__()
        self.heads, self.dim_head, self.inner = heads, dim_head, dim_head * heads
        self.scale = dim_head ** -0.5
        self.to_q = nn.Linear(dim, self.inner, bias=False)
        self.to_k = nn.Linear(dim, self.inner, bias=False)
        self.to_v = nn.Linear(dim, self.inner, bias=False)
        self.to_out = nn.Linear(self.inner, dim)

    def run(self, xn: CL, residual: CL) -> CL:
        """to_out(softmax(q k^T / 8) v) + residual on token rows CL [B, 1, 1, T, C] (blocks.CrossAttention.run without a context)."""
        N, T = xn.N, xn.S
        inner, hd = self.inner, self.dim_head
        pw, pb = packed_cat([self.to_q, self.to_k, self.to_v], xn.Cpad, "qkv")
        qkv = ops.conv(xn, pw, pb, 3 * inner, k=(1, 1, 1), pad=0)
        att = torch.empty(tuple(xn.t.shape[:4]) + (inner,), dtype=torch.bfloat16, device=xn.t.device)
        ld = qkv.Cpad
        ops.attention(qkv.t, qkv.t, qkv.t, att, N, self.heads, hd, T, T, (ld, hd), (ld, hd), (ld, hd), (inner, hd), self.scale,
                      q_off=0, k_off=inner, v_off=2 * inner)
        pwo, pbo = packed_conv(self.to_out, inner)
        return ops.conv(CL(att, inner), pwo, pbo, self.to_out.weight.shape[0], k=(1, 1, 1), pad=0, residual=residual)


class FeedForward(nn.Module):
    """x_transformer.FeedForward, non-gated: net = Sequential(Sequential(Linear, GELU), Dropout, Linear)."""

    def __init__(self, dim, mult=4):
        super().__init__()
        inner = int(dim * mult)
        self.inner = inner
        self.net = nn.Sequential(nn.Sequential(nn.Linear(dim, inner), nn.GELU()), nn.Dropout(0.0), nn.Linear(inner, dim))

    def run(self, xn: CL, residual: CL) -> CL:
        lin1, lin2 = self.net[0][0], self.net[2]
        pw, pb = packed_conv(lin1, xn.Cpad)
        h = ops.conv(xn, pw, pb, self.inner, k=(1, 1, 1), pad=0)
        h = CL(ops.gelu(h.t), self.inner)                    # GELU(0) = 0: the pad lanes stay zero
        pw2, pb2 = packed_conv(lin2, h.Cpad)
        return ops.conv(h, pw2, pb2, lin2.weight.shape[0], k=(1, 1, 1), pad=0, residual=residual)


class Residual(nn.Module):
    """Parameter-free third member of each layer triple (x_transformer.py:163-165): the add is the closing conv's `residual=`."""


class Encoder(nn.Module):
    """x_transformer.Encoder(dim, depth) with its defaults: depth x (pre-LayerNorm self-attention, pre-LayerNorm feed-forward), residuals."""

    def __init__(self, dim, depth, heads=HEADS, **unsupported):
        super().__init__()
        if unsupported:
            raise NotImplementedError(f"x_transformer.Encoder options {sorted(unsupported)} are not supported (dim, depth, heads only)")
        self.dim, self.depth = dim, depth
        self.layers = nn.ModuleList()
        for _ in range(depth):
            self.layers.append(nn.ModuleList([nn.LayerNorm(dim), Attention(dim, heads=heads), Residual()]))
            self.layers.append(nn.ModuleList([nn.LayerNorm(dim), FeedForward(dim), Residual()]))


def layernorm_cl(x: CL, ln: nn.LayerNorm) -> CL:
    """LayerNorm over the logical channels of token rows: whole rows on gg_layernorm, padded rows on gg_layernorm_rows."""
    if x.C == x.Cpad:
        return CL(ops.layernorm(x.t, f32(ln.weight), f32(ln.bias), ln.eps), x.C)
    return ops.layernorm_rows(x, f32(ln.weight), f32(ln.bias), ln.eps)


class TransformerWrapper(nn.Module):
    """x_transformer.TransformerWrapper(num_tokens, max_seq_len, attn_layers) as the embedders use it: return_embeddings=True, no mask.
    to_logits is a parameter container only (unused by the embedders, present in every checkpoint)."""

    def __init__(self, *, num_tokens, max_seq_len, attn_layers, emb_dropout=0.0):
        super().__init__()
        dim = attn_layers.dim
        self.max_seq_len, self.num_tokens = max_seq_len, num_tokens
        self.token_emb = nn.Embedding(num_tokens, dim)
        self.pos_emb = AbsolutePositionalEmbedding(dim, max_seq_len)
        self.emb_dropout = nn.Dropout(emb_dropout)
        self.project_emb = nn.Identity()
        self.attn_layers = attn_layers
        self.norm = nn.LayerNorm(dim)
        nn.init.normal_(self.token_emb.weight, std=0.02)
        self.to_logits = nn.Linear(dim, num_tokens)

    def run(self, tokens: torch.Tensor) -> torch.Tensor:
        """tokens integer [B, T] -> fp32 [B, T, dim]."""
        dim = self.attn_layers.dim
        x = CL(ops.embed_rows(tokens, f32(self.token_emb.weight), f32(self.pos_emb.emb.weight), bf16=True), dim)
        for norm, block, _ in self.attn_layers.layers:
            x = block.run(layernorm_cl(x, norm), x)
        x = layernorm_cl(x, self.norm)
        return x.t[:, 0, 0, :, :dim].float()                 # plumbing: the logical lanes of the bf16 rows as fp32 [B, T, dim]


class _Embedder(nn.Module):
    @torch.no_grad()
    def forward(self, tokens):
        _eval_only(self)
        _check_tokens(type(self).__name__, tokens)
        ops.require_gpu(tokens, f"{type(self).__name__}.forward")
        return self.transformer.run(tokens)

    def encode(self, x):
        return self(x)


class TransformerEmbedder(_Embedder):
    """Some transformer encoder layers over caller-made tokens.  `device` is accepted and ignored: the module runs where its weights are."""

    def __init__(self, n_embed, n_layer, vocab_size, max_seq_len=77, device="cuda"):
        super().__init__()
        self.device = device
        self.transformer = TransformerWrapper(num_tokens=vocab_size, max_seq_len=max_seq_len, attn_layers=Encoder(dim=n_embed, depth=n_layer))


class BERTEmbedder(_Embedder):
    """BERTEmbedder without its tokenizer: `use_tokenizer=True` would fetch a pretrained tokenizer by model name and is refused; the caller
    tokenises.  embedding_dropout is accepted: in eval mode it is the identity."""

    def __init__(self, n_embed, n_layer, vocab_size=30522, max_seq_len=77, device="cuda", use_tokenizer=True, embedding_dropout=0.0):
        super().__init__()
        if use_tokenizer:
            raise NotImplementedError("BERTEmbedder: use_tokenizer=True is not supported (the reference fetches its BERT tokenizer by model "
                                      "name; pass use_tokenizer=False and integer tokens [B, T])")
        self.use_tknz_fn = False
        self.device = device
        self.transformer = TransformerWrapper(num_tokens=vocab_size, max_seq_len=max_seq_len, attn_layers=Encoder(dim=n_embed, depth=n_layer),
                                              emb_dropout=embedding_dropout)


# ------------------------------------------------------------------------------------------------ SpatialRescaler
class SpatialRescaler(nn.Module):
    def __init__(self, n_stages=1, method="bilinear", multiplier=0.5, in_channels=3, out_channels=None, bias=False):
        super().__init__()
        assert n_stages >= 0
        assert method in ["nearest", "linear", "bilinear", "trilinear", "bicubic", "area"]
        if method in ("linear", "trilinear"):
            raise NotImplementedError(f"SpatialRescaler: method {method!r} is not supported (3-D / 5-D inputs; nearest, bilinear, bicubic "
                                      "and area resize 4-D images)")
        self.n_stages, self.method, self.multiplier = n_stages, method, multiplier
        self.remap_output = out_channels is not None
        if self.remap_output:
            self.channel_mapper = nn.Conv2d(in_channels, out_channels, 1, bias=bias)

    @torch.no_grad()
    def forward(self, x):
        _eval_only(self)
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise ValueError(f"SpatialRescaler: inputs that are not 4-D [N, C, H, W] are not supported, got "
                             f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
        h, w = int(x.shape[2]), int(x.shape[3])
        for stage in range(self.n_stages):                  # refused on the host, before any launch
            h, w = ops.interpolate_extent(h, self.multiplier), ops.interpolate_extent(w, self.multiplier)
            if h < 1 or w < 1:
                raise ValueError(f"SpatialRescaler: stage {stage + 1} of {self.n_stages} at multiplier {self.multiplier} would give an extent "
                                 f"of 0 from {tuple(x.shape)}")
        ops.require_gpu(x, "SpatialRescaler.forward")
        x = x.float()
        for _ in range(self.n_stages):
            x = ops.interpolate2d(x, self.multiplier, self.method)
        if self.remap_output:
            cm = self.channel_mapper
            src = ops.to_cl(x)
            pw, pb = packed_conv(cm, src.Cpad)
            x = ops.from_cl(ops.conv(src, pw, pb, cm.weight.shape[0], k=(1, 1, 1), pad=0, out_f32=True), 2)
        return x

    def encode(self, x):
        return self(x)
