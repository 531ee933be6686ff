"""Cond stages of the LDM family on the HIP engine: the classes of the reference's ldm/modules/encoders/modules.py that a
`cond_stage_config` can name and that need nothing from outside the checkpoint.

  ClassEmbedder        modules.py:22-34     batch[key] -> embedding rows [B, 1, embed_dim]                 gg_embed_rows (fp32, exact)
  TransformerEmbedder  modules.py:37-51     tokens [B, T] -> TransformerWrapper(Encoder) embeddings        gg_embed_rows (bf16 token rows),
  BERTEmbedder         modules.py:81-104    the same network behind the (refused) BERT tokenizer           LayerNorm, 1x1 convs, attention, gg_gelu
  SpatialRescaler      modules.py:107-136   n_stages x F.interpolate(scale_factor) [+ 1x1 channel_mapper]  gg_interpolate2d_f32 [+ conv]
  FrozenBERTEmbedder   modules.py:205-284   text -> WordPiece ids (tokenizer.py) -> transformers' BertModel      gg_bert_embed, 1x1 convs, attention
                       (ccdm: encoder.py:21-100)  restated here as `BertModel`, loaded from a LOCAL directory  with key lengths, gg_gelu, LayerNorm

torch.nn modules appear only as parameter containers, so that `state_dict()` carries the reference's names and shapes (those of
ldm/modules/x_transformer.py: layers at transformer.attn_layers.layers.{2i} / {2i+1}, the norm under .0, the block under .1); their ATen
forward is never called.  Sampling only: eval mode, device tensors, no cross-attention inside the encoder; the only mask is BERT's
padding mask, a prefix of ones per sample, which runs as per-sample key lengths of the attention kernel.

`python -m jointimagegeneration_amd.cond --bert DIR --text "..." --out feats.npy` writes the [b, hidden, length] features that
PreloadedBERTEncoder (encoder.py) takes: what the reference's datasets cache.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
import torch.nn as nn

from . import io as gio
from . import ops
from .blocks import conv_of, f32, layernorm_cl, qkv_attention, token_rows_f32  # noqa: F401  (layernorm_cl: also imported from here)
from .ops import CL
from .tokenizer import BertWordPieceTokenizer

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
        qkv = conv_of([self.to_q, self.to_k, self.to_v], xn, tag="qkv")
        return conv_of(self.to_out, qkv_attention(qkv, self.heads, self.dim_head, self.scale), residual=residual)


class FeedForward(nn.Module):
    """x_transformer.FeedForward, non-gated: net = Sequential(Sequential(Linear, GELU), Dropout, Linear)."""

    def __init__(self, dim, mult=4):
        super().__init__()
        inner = int(dim * mult)
        self.inner = inner
        self.net = nn.Sequential(nn.Sequential(nn.Linear(dim, inner), nn.GELU()), nn.Dropout(0.0), nn.Linear(inner, dim))

    def run(self, xn: CL, residual: CL) -> CL:
        lin1, lin2 = self.net[0][0], self.net[2]
        h = CL(ops.gelu(conv_of(lin1, xn).t), self.inner)    # GELU(0) = 0: the pad lanes stay zero
        return conv_of(lin2, h, residual=residual)


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
        return token_rows_f32(layernorm_cl(x, self.norm))


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
            x = ops.from_cl(conv_of(self.channel_mapper, ops.to_cl(x), out_f32=True), 2)
        return x

    def encode(self, x):
        return self(x)


# ------------------------------------------------------------------------------------------------ BERT (transformers' BertModel, restated)
ATTN_HEAD_DIMS = (32, 64, 128)        # gg_attention_forward_kvlen: the register-staged kernels


class BertEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.word_embeddings = nn.Embedding(cfg["vocab_size"], cfg["hidden_size"])
        self.position_embeddings = nn.Embedding(cfg["max_position_embeddings"], cfg["hidden_size"])
        self.token_type_embeddings = nn.Embedding(cfg["type_vocab_size"], cfg["hidden_size"])
        self.LayerNorm = nn.LayerNorm(cfg["hidden_size"], eps=cfg["layer_norm_eps"])

    def _load_from_state_dict(self, state_dict, prefix, *args):
        for name in ("position_ids", "token_type_ids"):      # persistent buffers of old checkpoints: index ramps, nothing to load
            state_dict.pop(prefix + name, None)
        super()._load_from_state_dict(state_dict, prefix, *args)


class BertSelfAttention(nn.Module):
    def __init__(self, hidden):
        super().__init__()
        self.query, self.key, self.value = nn.Linear(hidden, hidden), nn.Linear(hidden, hidden), nn.Linear(hidden, hidden)


class BertSelfOutput(nn.Module):
    """dense + LayerNorm pair of attention.output and of output: LayerNorm(dense(h) + x)"""

    def __init__(self, cin, hidden, eps):
        super().__init__()
        self.dense = nn.Linear(cin, hidden)
        self.LayerNorm = nn.LayerNorm(hidden, eps=eps)

    def run(self, h: CL, x: CL) -> CL:
        return layernorm_cl(conv_of(self.dense, h, residual=x), self.LayerNorm)


class BertAttention(nn.Module):
    def __init__(self, hidden, heads, eps):
        super().__init__()
        self.heads, self.head_dim = heads, hidden // heads
        setattr(self, "self", BertSelfAttention(hidden))
        self.output = BertSelfOutput(hidden, hidden, eps)

    def run(self, x: CL, kv_len: torch.Tensor) -> CL:
        sa = getattr(self, "self")
        qkv = conv_of([sa.query, sa.key, sa.value], x, tag="qkv")
        return self.output.run(qkv_attention(qkv, self.heads, self.head_dim, self.head_dim ** -0.5, kv_len=kv_len), x)


class BertIntermediate(nn.Module):
    def __init__(self, hidden, inner):
        super().__init__()
        self.dense = nn.Linear(hidden, inner)


class BertLayer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        hidden, inner, eps = cfg["hidden_size"], cfg["intermediate_size"], cfg["layer_norm_eps"]
        self.attention = BertAttention(hidden, cfg["num_attention_heads"], eps)
        self.intermediate = BertIntermediate(hidden, inner)
        self.output = BertSelfOutput(inner, hidden, eps)

    def run(self, x: CL, kv_len: torch.Tensor) -> CL:
        x = self.attention.run(x, kv_len)
        h = conv_of(self.intermediate.dense, x)
        h = CL(ops.gelu(h.t), h.C)                           # GELU(0) = 0: the pad lanes stay zero
        return self.output.run(h, x)


class BertEncoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layer = nn.ModuleList([BertLayer(cfg) for _ in range(cfg["num_hidden_layers"])])


class BertPooler(nn.Module):
    """Present in every checkpoint, loaded, never run: the embedder returns last_hidden_state."""

    def __init__(self, hidden):
        super().__init__()
        self.dense = nn.Linear(hidden, hidden)


BERT_CONFIG_DEFAULTS = dict(type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu", position_embedding_type="absolute", is_decoder=False,
                            add_cross_attention=False, max_position_embeddings=512)


class BertModel(nn.Module):
    """transformers' BertModel (encoder only, absolute positions, post-LayerNorm) with its state_dict names and shapes.  `config` is the
    dict of the directory's config.json.  Per layer: fused q|k|v 1x1 conv with biases, attention scaled d^-1/2 over the first kv_len[n]
    keys, attention.output.dense + residual, LayerNorm, intermediate.dense, erf GELU, output.dense + residual, LayerNorm."""

    def __init__(self, config: dict):
        super().__init__()
        cfg = dict(BERT_CONFIG_DEFAULTS, **{k: v for k, v in config.items() if v is not None})
        for key in ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size"):
            if key not in cfg:
                raise KeyError(f"BertModel: config.json lacks {key!r}")
        if cfg["position_embedding_type"] != "absolute":
            raise NotImplementedError(f"BertModel: position_embedding_type {cfg['position_embedding_type']!r} is not supported (absolute only)")
        if cfg["hidden_act"] != "gelu":
            raise NotImplementedError(f"BertModel: hidden_act {cfg['hidden_act']!r} is not supported (\"gelu\", the erf form, only)")
        if cfg["is_decoder"] or cfg["add_cross_attention"]:
            raise NotImplementedError("BertModel: is_decoder / add_cross_attention are not supported (the encoder only)")
        hidden, heads = cfg["hidden_size"], cfg["num_attention_heads"]
        if hidden % heads or hidden // heads not in ATTN_HEAD_DIMS:
            raise NotImplementedError(f"BertModel: head dim {hidden}/{heads} is not supported (the key-length attention kernel has "
                                      f"instances for {ATTN_HEAD_DIMS})")
        self.config = cfg
        self.embeddings = BertEmbeddings(cfg)
        self.encoder = BertEncoder(cfg)
        self.pooler = BertPooler(hidden)

    def run(self, ids: torch.Tensor, lengths: Sequence[int], ids_host: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ids int32 [B, T] on the device, lengths[n] real tokens per sample (host ints, 1..T) -> last_hidden_state fp32 [B, T, hidden].
        Rows at and past a sample's length are computed like the others (the reference's are too) and attended to by nobody."""
        B, T = (int(v) for v in ids.shape)
        P = self.config["max_position_embeddings"]
        if T > P:
            raise ValueError(f"BertModel: sequence length {T} exceeds max_position_embeddings {P}")
        lengths = [int(v) for v in lengths]
        if len(lengths) != B or min(lengths) < 1 or max(lengths) > T:
            raise ValueError(f"BertModel: {B} key lengths in [1, {T}] are needed, got {lengths}")
        kv_len = torch.tensor(lengths, dtype=torch.int32).to(ids.device)
        e = self.embeddings
        hidden = self.config["hidden_size"]
        x = CL(ops.bert_embed(ids, None, f32(e.word_embeddings.weight), f32(e.position_embeddings.weight), f32(e.token_type_embeddings.weight),
                              f32(e.LayerNorm.weight), f32(e.LayerNorm.bias), e.LayerNorm.eps, ids_host=ids_host), hidden)
        for layer in self.encoder.layer:
            x = layer.run(x, kv_len)
        return token_rows_f32(x)


def hf_bert_state_dict(sd: dict) -> dict:
    """A BERT checkpoint's tensors under BertModel's names: the `bert.` prefix of task-head checkpoints (BertForMaskedLM, as
    bert-base-chinese ships) is dropped with the heads (`cls.*`), and the LayerNorm.gamma / .beta of the oldest ones are renamed."""
    if any(k.startswith("bert.") for k in sd):
        sd = {k[len("bert."):]: v for k, v in sd.items() if k.startswith("bert.")}
    out = {}
    for k, v in sd.items():
        if k.endswith("LayerNorm.gamma"):
            k = k[:-len("gamma")] + "weight"
        elif k.endswith("LayerNorm.beta"):
            k = k[:-len("beta")] + "bias"
        out[k] = v
    return out


def prefix_lengths(mask: torch.Tensor) -> List[int]:
    """Key lengths of a 0/1 padding mask [B, T] (host values); every row must be a non-empty prefix of ones."""
    m = mask.detach().cpu().long()
    if m.dim() != 2 or bool(((m != 0) & (m != 1)).any()):
        raise ValueError(f"attention_mask must be a 0/1 tensor [B, T], got {tuple(mask.shape)}")
    lengths = m.sum(1)
    T = m.shape[1]
    prefix = (torch.arange(T)[None, :] < lengths[:, None]).long()
    if not torch.equal(prefix, m):
        bad = int((prefix != m).any(1).nonzero()[0])
        raise NotImplementedError(f"attention_mask row {bad} is not a prefix of ones (only right-padding masks are supported)")
    if int(lengths.min()) < 1:
        raise ValueError(f"attention_mask row {int(lengths.argmin())} has length 0 (every sample needs at least one token)")
    return [int(v) for v in lengths]


class FrozenBERTEmbedder(nn.Module):
    """FrozenBERTEmbedder of both halves of the reference: a BERT from a LOCAL Hugging Face directory (config.json, vocab.txt,
    tokenizer_config.json, model.safetensors or pytorch_model.bin; nothing is downloaded and transformers is not imported), texts padded
    to bert_max_length, last_hidden_state under the padding mask, chunks interleaved as "(b x) n l -> b (n x) l" with
    x = bert_encode_batch.  use_text_split, bert_max_length and bert_encode_batch are plain attributes, settable as on the reference."""
    use_text_split = False
    bert_max_length = 512

    def __init__(self, ckpt_path, device="cuda", freeze=True, max_length=512):
        super().__init__()
        self.device = device
        self.max_length = max_length
        self.bert_max_length = 512
        if max_length < self.bert_max_length:
            raise ValueError(f"FrozenBERTEmbedder: max_length {max_length} < {self.bert_max_length} is not supported (bert_encode_batch = "
                             "max_length // 512 would be 0, with which the reference cannot run either)")
        if max_length % self.bert_max_length:
            raise ValueError(f"FrozenBERTEmbedder: max_length {max_length} must be a multiple of {self.bert_max_length}")
        self.bert_encode_batch = max_length // self.bert_max_length
        config, sd, vocab, tok_cfg = gio.load_hf_dir(ckpt_path)
        self.tokenizer = BertWordPieceTokenizer(vocab, do_lower_case=tok_cfg.get("do_lower_case", True))
        self.transformer = BertModel(config)
        self.transformer.load_state_dict(hf_bert_state_dict(sd))
        self.transformer.to(device)
        if freeze:
            self.freeze()

    def freeze(self):
        self.transformer = self.transformer.eval()
        for param in self.parameters():
            param.requires_grad = False

    # ---- the reference's text splitting (ccdm encoder.py:43-82), as far as the reference itself can run it
    def token_split(self, string: str) -> List[str]:
        if len(string) < 512:                                # the reference's default argument is bound to the CLASS attribute: always 512
            return [string]
        raise NotImplementedError(f"FrozenBERTEmbedder: use_text_split with a text of {len(string)} characters (512 or more) is not "
                                  "supported (the reference raises TypeError there: its grouping returns a tuple)")

    def _merge_text_list(self, *ls) -> List[str]:
        x = self.bert_encode_batch
        if x > 2:
            raise NotImplementedError(f"FrozenBERTEmbedder: use_text_split with bert_encode_batch = {x} > 2 is not supported (the reference "
                                      "pads a short text with ONE empty chunk and then fails to interleave)")
        out: List[str] = []
        for l in ls:
            chunks = list(l) if isinstance(l, list) else self.token_split(str(l))
            if len(chunks) < x:
                chunks.append("")
            if len(chunks) > x:
                chunks = chunks[:x]
            if len(chunks) != x:
                raise ValueError(f"FrozenBERTEmbedder: a text of {len(chunks)} chunks cannot fill bert_encode_batch = {x}")
            out += chunks
        return out

    @torch.no_grad()
    def forward(self, text, attention_mask=None):
        """text: a str, a list of str, or integer tokens [B, T] on the device with attention_mask= [B, T] (a prefix of ones per row).
        Returns fp32 [b, n * x, hidden], b = B / x: chunk xi of sample b on rows xi::x."""
        _eval_only(self.transformer)                         # freeze() puts the transformer, not the wrapper, into eval mode (as the reference)
        if ops.FP32:
            raise NotImplementedError("FrozenBERTEmbedder: ops.fp32_validation() is not supported for transformer cond stages")
        dev = self.transformer.embeddings.word_embeddings.weight.device
        if dev.type != "cuda":
            raise RuntimeError(f"FrozenBERTEmbedder.forward: the model is on {dev}; the GuideGen engine runs on MI355X only (no CPU fallback)")
        x, n = int(self.bert_encode_batch), int(self.bert_max_length)
        if x < 1:
            raise ValueError(f"FrozenBERTEmbedder: bert_encode_batch = {x} (max_length < 512) is not supported")
        if isinstance(text, torch.Tensor):
            _check_tokens("FrozenBERTEmbedder", text)
            ops.require_gpu(text, "FrozenBERTEmbedder.forward")
            if attention_mask is None or tuple(attention_mask.shape) != tuple(text.shape):
                raise ValueError("FrozenBERTEmbedder: integer tokens [B, T] need attention_mask= of the same shape")
            lengths = prefix_lengths(attention_mask)
            ids_host = text.detach().cpu().to(torch.int32).contiguous()          # host sync: before the chain, outside any captured graph
        else:
            if attention_mask is not None:
                raise ValueError("FrozenBERTEmbedder: attention_mask= goes with integer tokens, not with text")
            text = [text] if isinstance(text, str) else list(text)
            if self.use_text_split:
                text = self._merge_text_list(*text)
            ids, mask = self.tokenizer.encode(text, n)
            ids_host = torch.tensor(ids, dtype=torch.int32)
            lengths = [sum(m) for m in mask]
        B, T = (int(v) for v in ids_host.shape)
        if B % x:
            raise ValueError(f"FrozenBERTEmbedder: {B} sequences are not whole groups of bert_encode_batch = {x}"
                             + ("" if self.use_text_split else " (set use_text_split, which pads every text to that many chunks)"))
        z = self.transformer.run(ids_host.to(dev), lengths, ids_host=ids_host)          # [(b x), T, hidden]
        b = B // x
        return z.view(b, x, T, -1).permute(0, 2, 1, 3).reshape(b, T * x, -1)

    def encode(self, text, attention_mask=None):
        return self(text, attention_mask=attention_mask)


def _main(argv=None) -> int:
    import argparse
    import numpy as np
    ap = argparse.ArgumentParser(prog="python -m jointimagegeneration_amd.cond",
                                 description="Encode texts with a local BERT and write the [b, hidden, length] features PreloadedBERTEncoder takes.")
    ap.add_argument("--bert", required=True, metavar="DIR", help="local Hugging Face BERT directory")
    ap.add_argument("--text", action="append", default=[], help="a text (repeatable)")
    ap.add_argument("--text-file", metavar="F", help="a UTF-8 file with one text per line")
    ap.add_argument("--out", required=True, help="output .npy")
    a = ap.parse_args(argv)
    texts = list(a.text)
    if a.text_file:
        with open(a.text_file, "r", encoding="utf-8") as f:
            texts += [line.rstrip("\n") for line in f]
    if not texts:
        ap.error("no text: give --text or --text-file")
    z = FrozenBERTEmbedder(a.bert, device="cuda").encode(texts)                                      # [b, length, hidden]
    np.save(a.out, z.permute(0, 2, 1).contiguous().cpu().numpy())
    print(f"wrote {a.out}: {tuple(z.shape[0:1]) + (z.shape[2], z.shape[1])} fp32")
    return 0


if __name__ == "__main__":
    raise SystemExit(_main())
