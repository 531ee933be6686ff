"""Plain-torch restatement of transformers' BertModel (absolute positions, post-LayerNorm, erf GELU) under a right-padding mask given as
per-sample key lengths: the CPU reference of the BERT tests.  tests/golden/make_golden_bert.py asserts that it agrees with the
reference's FrozenBERTEmbedder (transformers' own BertModel) at 2e-5 in fp32.

forward() computes in the dtype of the state dict.  `act` and `wt` are the hooks of the bf16 SHADOW (shadow_bf16): `wt` is applied to
every Linear weight and `act` to every activation the engine keeps in memory, which it stores as bf16: the embedding LayerNorm's output,
q|k|v, the attention output, each dense + residual sum, each LayerNorm output, the intermediate activation and its GELU.  Biases,
LayerNorm coefficients and the embedding tables stay fp32 in the engine and in the shadow.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

TINY = dict(vocab_size=128, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128, max_position_embeddings=40,
            type_vocab_size=2, layer_norm_eps=1e-12)
BASE = dict(vocab_size=21128, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
            max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12)


def surface(cfg):
    """[name, shape] of transformers' BertModel state_dict for `cfg`, in its order"""
    H, I = cfg["hidden_size"], cfg["intermediate_size"]
    out = [["embeddings.word_embeddings.weight", [cfg["vocab_size"], H]], ["embeddings.position_embeddings.weight", [cfg["max_position_embeddings"], H]],
           ["embeddings.token_type_embeddings.weight", [cfg["type_vocab_size"], H]], ["embeddings.LayerNorm.weight", [H]], ["embeddings.LayerNorm.bias", [H]]]
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layer.{i}."
        for name, (o, c) in (("attention.self.query", (H, H)), ("attention.self.key", (H, H)), ("attention.self.value", (H, H)),
                             ("attention.output.dense", (H, H)), ("attention.output.LayerNorm", (H, None)), ("intermediate.dense", (I, H)),
                             ("output.dense", (H, I)), ("output.LayerNorm", (H, None))):
            out += [[p + name + ".weight", [o, c] if c else [o]], [p + name + ".bias", [o]]]
    return out + [["pooler.dense.weight", [H, H]], ["pooler.dense.bias", [H]]]


def seeded_state_dict(cfg, prefix, seed=1024):
    """the seed-recipe weights (jointimagegeneration_amd.synth) under BertModel's names"""
    from jointimagegeneration_amd.synth import synth_tensor
    return {name: synth_tensor(prefix + name, tuple(shape), seed) for name, shape in surface(cfg)}


def forward(sd, ids, lengths, cfg, act=lambda t: t, wt=lambda t: t):
    """sd: BertModel state dict (fp32 or fp64), ids long [B, T], lengths [B] -> last_hidden_state [B, T, hidden] in sd's dtype."""
    B, T = ids.shape
    H, heads, eps = cfg["hidden_size"], cfg["num_attention_heads"], cfg["layer_norm_eps"]
    d = H // heads
    lin = lambda x, name: F.linear(x, wt(sd[name + ".weight"]), sd[name + ".bias"])
    ln = lambda x, name: F.layer_norm(x, (H,), sd[name + ".weight"], sd[name + ".bias"], eps)
    x = sd["embeddings.word_embeddings.weight"][ids] + sd["embeddings.token_type_embeddings.weight"][0] + sd["embeddings.position_embeddings.weight"][:T]
    x = act(ln(x, "embeddings.LayerNorm"))
    dead = torch.arange(T)[None, :] >= torch.as_tensor(lengths)[:, None]                  # [B, Tkv]
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layer.{i}."
        split = lambda t: t.view(B, T, heads, d).transpose(1, 2)
        q, k, v = (split(act(lin(x, p + "attention.self." + n))) for n in ("query", "key", "value"))
        s = (q @ k.transpose(-1, -2)) / math.sqrt(d)
        s = s.masked_fill(dead[:, None, None, :], float("-inf"))
        a = act((torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, T, H))
        x = act(ln(act(lin(a, p + "attention.output.dense") + x), p + "attention.output.LayerNorm"))
        h = act(F.gelu(act(lin(x, p + "intermediate.dense"))))
        x = act(ln(act(lin(h, p + "output.dense") + x), p + "output.LayerNorm"))
    return x


def shadow_bf16(sd, ids, lengths, cfg):
    """forward() in fp32 with the engine's storage roundings: Linear weights and stored activations pass through bf16"""
    r = lambda t: t.bfloat16().float()
    return forward(sd, ids, lengths, cfg, act=r, wt=r)


def interleave(z, x):
    """the reference's rearrange "(b x) n l -> b (n x) l" """
    B, n, l = z.shape
    return z.view(B // x, x, n, l).permute(0, 2, 1, 3).reshape(B // x, n * x, l)


def write_safetensors(path, sd):
    """the tests' own writer of the format jointimagegeneration_amd.io.read_safetensors reads (F32 / F16 / BF16)"""
    import json
    import struct
    names = {torch.float32: "F32", torch.float16: "F16", torch.bfloat16: "BF16"}
    header, blobs, off = {"__metadata__": {"format": "pt"}}, [], 0
    for k, v in sd.items():
        v = v.detach().contiguous().cpu()
        raw = v.view(torch.uint8).numpy().tobytes() if v.numel() else b""
        header[k] = {"dtype": names[v.dtype], "shape": list(v.shape), "data_offsets": [off, off + len(raw)]}
        blobs.append(raw)
        off += len(raw)
    hj = json.dumps(header, separators=(",", ":")).encode("utf-8")
    hj += b" " * (-len(hj) % 8)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(hj)) + hj + b"".join(blobs))
