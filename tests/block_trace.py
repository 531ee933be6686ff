"""Launch-trace recorder for the network blocks: which ops launches a block's run() makes, with which operands, on CPU tensors.

Every launching function of ops is replaced by a stand-in that records its arguments and returns a placeholder of the shape and dtype
the real one returns; the dispatch predicates are pinned to one constant answer.  A trace entry holds the op name and, under the
parameter names of the real function (bound through its signature; an argument equal to the signature's default is left out, so a
default written out is the same entry):
  tensor / CL operands  shape, dtype, logical C, storage offset and where the storage came from: "in:<name>" (a case input),
                        "param:<name>" (a parameter of the module tree), "pack:<module>/<cin_pad>/<tag>#i" (a cached repack),
                        "launch:<i>" (the output of launch i), or "host" with a digest of the bytes (host arithmetic on parameters);
  everything else       as it was passed (k, stride, pad, strides and offsets of attention, scale, flags).
Packing goes through blocks.PACKED: each build of a cache entry is a pack event (the module and parameters by name, the rest of the
key, every pack_conv_weight call inside it).  Pack events are compared as a set, launches in order; a second run packs nothing.

_cases() builds every traced block configuration; tests/golden/make_golden_block_traces.py writes their traces to
tests/golden/block_launch_traces.json as fingerprints (one digest per launch entry and per pack event, see fingerprint) and
tests/test_block_trace_cpu.py compares.  A planted defect (DEFECTS) alters the arguments
inside the stand-in, as if the block had passed them so: the same plant works on any version of the blocks."""
from __future__ import annotations

import contextlib
import hashlib
import inspect
import json

import torch
from torch import nn

PREDICATES = ("conv_prologue_from_acc", "conv_fuses_prologue", "conv_fuses_skip", "groupnorm_fused_ok", "has_stats", "has_any_stats")
DTYPES = {torch.bfloat16: "bf16", torch.float32: "f32", torch.float64: "f64", torch.int32: "i32", torch.int64: "i64"}
OUTPUT_OPERANDS = {"attention": ("out",), "conv": ("out",)}        # buffers the caller allocates and the launch fills
DEFECTS = ("swap_kv_offset", "legacy_stride", "wrong_pad", "wrong_cin_pad")
BF16, F32 = torch.bfloat16, torch.float32


def pad32(c):
    return (c + 31) // 32 * 32


class Recorder:
    def __init__(self, root: nn.Module, inputs: dict, answer: bool, defect=None):
        from jointimagegeneration_amd import blocks, ops
        self.ops, self.blocks, self.answer, self.defect = ops, blocks, answer, defect
        self.labels, self.keep = {}, []
        self.launches, self.packs, self.packing = [], [], None
        self.module_names = {id(m): (n or "<root>") for n, m in root.named_modules()}
        for n, p in list(root.named_parameters()) + list(root.named_buffers()):
            self.label(p, "param:" + n)
        for n, v in inputs.items():
            self.label(v, "in:" + n)

    # ---- provenance
    @staticmethod
    def _key(t):
        return t.untyped_storage().data_ptr()

    def label(self, v, name):
        if isinstance(v, self.ops.CL):
            v = v.t
        if isinstance(v, (tuple, list)):
            for j, x in enumerate(v):
                self.label(x, f"{name}#{j}")
        elif isinstance(v, torch.Tensor) and v.numel():
            self.labels.setdefault(self._key(v), name)
            self.keep.append(v)                                      # alive: the allocator must not hand the storage out again

    def describe(self, v, output=False):
        """Tensors as one string `from|shape|dtype[|C=..][|offset=..][|stride=..][|digest=..]`, everything else as it is."""
        if isinstance(v, self.ops.CL):
            return self.describe(v.t, output) + f"|C={int(v.C)}"
        if isinstance(v, torch.Tensor):
            origin = self.labels.get(self._key(v))
            d = [origin or ("new" if output else "host"), "x".join(str(n) for n in v.shape), DTYPES[v.dtype]]
            if v.storage_offset():
                d.append(f"offset={v.storage_offset()}")
            if not v.is_contiguous():
                d.append("stride=" + "x".join(str(n) for n in v.stride()))
            if origin is None and not output:
                d.append("digest=" + hashlib.sha1(v.detach().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:12])
            return "|".join(d)
        if isinstance(v, (tuple, list)):
            return [self.describe(x, output) for x in v]
        if isinstance(v, dict):
            return {str(k): self.describe(x, output) for k, x in v.items()}
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        raise TypeError(f"block_trace: no description for an argument of type {type(v).__name__}")

    # ---- stand-ins
    def launch(self, name, make):
        sig = inspect.signature(getattr(self.ops, name))             # the real function's: read before it is replaced

        def stand_in(*a, **k):
            b = sig.bind(*a, **k)
            b.apply_defaults()
            args = dict(b.arguments)
            self.plant(name, args)
            outs = OUTPUT_OPERANDS.get(name, ())
            i = len(self.launches)
            entry = {n: self.describe(v, n in outs) for n, v in args.items()}
            # an argument at the real function's default is left out: written out or not, it is the same launch
            self.launches.append({"op": name, **{n: v for n, v in entry.items() if sig.parameters[n].default is inspect.Parameter.empty
                                                 or v != self.describe(sig.parameters[n].default)}})
            ret = make(**args)
            self.label(ret, f"launch:{i}")
            for n in outs:
                if args[n] is not None:
                    self.label(args[n], f"launch:{i}")
            return ret
        return stand_in

    def plant(self, name, args):
        d = self.defect
        if name == "attention" and d == "swap_kv_offset":
            args["k_off"], args["v_off"] = args["v_off"], args["k_off"]
        if name == "attention" and d == "legacy_stride":
            for n in ("ld_hs_q", "ld_hs_k", "ld_hs_v"):
                args[n] = (args[n][0], 3 * args[n][1])
        if name == "conv" and d == "wrong_pad":
            args["pad"] = 1 - args["pad"]

    def packed(self):
        rec = self

        class TracedPacked(self.blocks._Packed):
            def get(self, key, params, build):
                def traced_build():
                    rest = [v + 32 if rec.defect == "wrong_cin_pad" and j == 0 and isinstance(v, int) else v for j, v in enumerate(key[1:])]
                    rec.packing = {"module": rec.module_names[key[0]], "key": rest, "weights": [],
                                   "params": [rec.labels.get(rec._key(p)) for p in params if p is not None]}
                    val = build()
                    ev, rec.packing = rec.packing, None
                    rec.packs.append(ev)
                    rec.label(val, "pack:" + "/".join([ev["module"]] + [str(v) for v in ev["key"]]))
                    return val
                return super().get(key, params, traced_build)
        return TracedPacked()

    def pack_conv_weight(self, w, cin_pad):
        if self.defect == "wrong_cin_pad":
            cin_pad += 32
        assert self.packing is not None, "pack_conv_weight outside the packing cache"
        self.packing["weights"].append({"shape": list(w.shape), "cin_pad": int(cin_pad)})
        return torch.zeros(8, dtype=F32 if self.ops.FP32 else BF16)

    @contextlib.contextmanager
    def patched(self):
        ops, CL = self.ops, self.ops.CL
        e = torch.empty

        def cl_like(src1, Ct, C, dtype=None):
            return CL(e(tuple(src1.t.shape[:4]) + (Ct,), dtype=dtype or src1.t.dtype), C)

        def width(src1, src2):
            return src1.Cpad + (src2.Cpad if src2 is not None else 0), src1.C + (src2.C if src2 is not None else 0)

        def conv(src1, cout, k, stride, pad, upsample, out_f32, out, geglu, **_):
            sp = ops.conv_out_extent(src1.spatial, k, stride, pad, upsample)
            if out is None:
                f32 = ops.is_f32(src1.t) or out_f32
                out = e((src1.N,) + tuple(sp) + (pad32(cout) // (2 if geglu else 1),), dtype=F32 if f32 else BF16)
            return CL(out, cout // 2 if geglu else cout)

        def norm(src1, src2=None, **_):
            return cl_like(src1, *width(src1, src2))

        def tables(src1, src2=None, **_):
            return tuple(e((src1.N, width(src1, src2)[0]), dtype=F32) for _ in range(2))

        def resample2x(src, up, resample_d, **_):
            N, D, H, W, cp = src.t.shape
            f = (lambda v: v * 2) if up else (lambda v: v // 2)
            return CL(e((N, f(D) if resample_d else D, f(H), f(W), cp), dtype=src.t.dtype), src.C)

        def to_cl(x, c_pad, out, c_offset, **_):
            sp = (1,) * (5 - x.ndim) + tuple(x.shape[2:])
            if out is None:
                out = e((x.shape[0],) + sp + (c_pad or pad32(x.shape[1] + c_offset),), dtype=F32 if ops.FP32 else BF16)
            return CL(out, x.shape[1] + c_offset)

        makes = {
            "conv": conv, "attention": lambda **_: None, "film_fold": lambda **_: None,
            "layernorm": lambda x, **_: torch.empty_like(x), "gelu": lambda x: torch.empty_like(x),
            "layernorm_rows": lambda x, **_: CL(torch.empty_like(x.t), x.C),
            "geglu": lambda h, inner: e(tuple(h.shape[:-1]) + (inner,), dtype=BF16),
            "groupnorm_stats": tables, "groupnorm_scale_shift_acc": tables,
            "groupnorm_apply": norm, "groupnorm_fused": norm, "groupnorm_apply_acc": norm,
            "groupnorm_f32": lambda src1, src2=None, **_: cl_like(src1, *width(src1, src2), dtype=F32),
            "groupnorm_f32_film": lambda src, **_: cl_like(src, src.Cpad, src.C, F32),
            "resample2x": resample2x,
            "embed_rows": lambda ids, tok, pos, bf16: (e((ids.shape[0], 1, 1, ids.shape[1], pad32(tok.shape[1])), dtype=BF16) if bf16
                                                        else e(tuple(ids.shape) + (tok.shape[1],), dtype=F32)),
            "bert_embed": lambda ids, word, **_: e((ids.shape[0], 1, 1, ids.shape[1], pad32(word.shape[1])), dtype=BF16),
            "interpolate2d": lambda x, scale_factor, mode: e(tuple(x.shape[:2]) + tuple(ops.interpolate_extent(int(v), scale_factor) for v in x.shape[2:]),
                                                             dtype=F32),
            "to_cl": to_cl,
            "from_cl": lambda cl, ndim_spatial: e((cl.N, cl.C) + tuple(cl.t.shape[4 - ndim_spatial:4]), dtype=F32),
        }
        with pytest_free_patch() as mp:
            for name, make in makes.items():
                mp(ops, name, self.launch(name, make))
            for name in PREDICATES:
                mp(ops, name, lambda *a, **k: self.answer)
            for name in ("require_gpu", "stats_begin", "stats_end"):      # host-side: a device check and the statistics arena
                mp(ops, name, lambda *a, **k: None)
            mp(ops, "pack_conv_weight", self.pack_conv_weight)
            mp(self.blocks, "PACKED", self.packed())
            yield self


@contextlib.contextmanager
def pytest_free_patch():
    """setattr with undo (the generator script runs without pytest's monkeypatch)."""
    undo = []

    def mp(obj, name, value):
        undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)
    try:
        yield mp
    finally:
        for obj, name, old in reversed(undo):
            setattr(obj, name, old)


# ------------------------------------------------------------------------------------------------ cases
def seed_parameters(root: nn.Module) -> None:
    """Closed-form parameter values, exact in bf16 and fp32: sums of two of them (conv2 bias + skip bias) are exact too, so the digest
    of a host-computed operand does not depend on how torch rounds."""
    with torch.no_grad():
        for i, p in enumerate(root.parameters()):
            p.copy_((((torch.arange(p.numel()) * 7 + 3 * i) % 13 - 6).float() / 8).view_as(p))


def cl(N, sp, C, dtype=BF16, cpad=None):
    from jointimagegeneration_amd.ops import CL
    sp = (1,) * (3 - len(sp)) + tuple(sp)
    return CL(torch.zeros((N,) + sp + (cpad or pad32(C),), dtype=dtype), C)


N = 2
EMB = 128


def grid(dims):
    return (4,) * dims


def _cases():
    """name -> builder() -> (root module, inputs by name, run(root, inputs)).  Smallest shapes that tell the idioms apart: N = 2, 4x4 or
    4x4x4 grids, 64 channels as 2 heads of 32, a 48-channel context (a padded row), 7 tokens."""
    from jointimagegeneration_amd import blocks as B
    from jointimagegeneration_amd import cond, ldm, ops, unet
    cases = {}

    def case(name):
        def deco(f):
            assert name not in cases
            cases[name] = f
            return f
        return deco

    def simple(name, make, channels=64, dims=2):
        @case(name)
        def _():
            return make(), {"h": cl(N, grid(dims), channels)}, lambda m, i: m.run(i["h"])

    for dims in (2, 3):
        for use_conv in (False, True):
            simple(f"Upsample-dims{dims}-conv{int(use_conv)}", lambda d=dims, u=use_conv: B.Upsample(64, u, dims=d, out_channels=96 if u else None), dims=dims)
            simple(f"Downsample-dims{dims}-conv{int(use_conv)}", lambda d=dims, u=use_conv: B.Downsample(64, u, dims=d, out_channels=96 if u else None), dims=dims)
        simple(f"AEUpsample-dims{dims}", lambda d=dims: B.AEUpsample(64, True, dims=d), dims=dims)
        simple(f"AEDownsample-dims{dims}", lambda d=dims: B.AEDownsample(64, True, dims=d), dims=dims)
        simple(f"ResnetBlock-dims{dims}", lambda d=dims: B.ResnetBlock(in_channels=64, dims=d), dims=dims)
    simple("ResnetBlock-nin_shortcut", lambda: B.ResnetBlock(in_channels=64, out_channels=96))
    simple("AttentionBlock-legacy", lambda: B.AttentionBlock(64, num_head_channels=32))
    simple("AttentionBlock-new_order", lambda: B.AttentionBlock(64, num_head_channels=32, use_new_attention_order=True))
    simple("AttentionBlock-dims3", lambda: B.AttentionBlock(64, num_heads=2), dims=3)
    simple("AttnBlock2d", lambda: B.AttnBlock2d(64))
    simple("AttnBlock3d", lambda: B.AttnBlock3d(32), channels=32, dims=3)

    def resblock(name, channels=64, src2_channels=0, dims=2, dtype=BF16, **kw):
        @case("ResBlock-" + name)
        def _():
            m = B.ResBlock(channels + src2_channels, EMB, 0.0, dims=dims, **kw)
            inputs = {"h": cl(N, grid(dims), channels, dtype), "tbias": torch.zeros(N * m.time_bias_width)}
            if src2_channels:
                inputs["src2"] = cl(N, grid(dims), src2_channels, dtype)

            def run(m, i):
                with ops.fp32_validation() if dtype == F32 else contextlib.nullcontext():
                    return m.run(i["h"], i["tbias"], i.get("src2"), want_stats=bool(src2_channels))
            return m, inputs, run

    resblock("plain")
    resblock("plain-dims3", dims=3)
    resblock("src2", src2_channels=32, out_channels=64)
    resblock("skip1x1", out_channels=96)
    resblock("skip3x3", out_channels=96, use_conv=True)
    resblock("film", use_scale_shift_norm=True)
    resblock("film-src2-skip1x1", src2_channels=32, out_channels=64, use_scale_shift_norm=True)
    resblock("up", up=True)
    resblock("down", down=True)
    resblock("up-dims3-film", dims=3, up=True, use_scale_shift_norm=True)
    resblock("down-dims3-skip1x1", dims=3, down=True, out_channels=96)
    resblock("film-fp32", dtype=F32, use_scale_shift_norm=True)
    resblock("down-fp32", dtype=F32, down=True)
    resblock("src2-skip1x1-fp32", dtype=F32, src2_channels=32, out_channels=64)

    for with_context in (False, True):
        for fuse in (True, False):
            @case(f"SpatialTransformer-context{int(with_context)}-geglu{int(fuse)}")
            def _(with_context=with_context, fuse=fuse):
                m = B.SpatialTransformer(64, 2, 32, context_dim=48 if with_context else None)
                inputs = {"h": cl(N, grid(2), 64)}
                if with_context:
                    inputs["context"] = cl(N, (7,), 48)

                def run(m, i):
                    with pytest_free_patch() as mp:
                        mp(B, "FUSE_GEGLU", fuse)
                        return m.run(i["h"], i.get("context"))
                return m, inputs, run

    @case("TimestepEmbedSequential-bare-conv")
    def _():
        m = B.TimestepEmbedSequential(B.conv_nd(2, 8, 64, 3, padding=1))
        return m, {"h": cl(N, grid(2), 8)}, lambda m, i: m.run(i["h"], None, None)

    def ddconfig(dims):
        return dict(ch=32, out_ch=1, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[4], in_channels=1, resolution=8, z_channels=4,
                    double_z=True, dims=dims)

    for dims in (2, 3):
        @case(f"Encoder-dims{dims}")
        def _(dims=dims):
            return ldm.Encoder(**ddconfig(dims)), {"x": cl(N, (8,) * dims, 1)}, lambda m, i: m.run(i["x"])

        @case(f"Decoder-dims{dims}")
        def _(dims=dims):
            return ldm.Decoder(**ddconfig(dims)), {"z": cl(N, (4,) * dims, 4)}, lambda m, i: m.run(i["z"])

        @case(f"AutoencoderKL-dims{dims}")
        def _(dims=dims):
            m = ldm.AutoencoderKL(ddconfig(dims), embed_dim=3, dims=dims)
            return m, {"x": cl(N, (8,) * dims, 1), "z": cl(N, (4,) * dims, 3)}, lambda m, i: (m.encode_moments_cl(i["x"]), m.decode_cl(i["z"]))

    @case("VQModel")
    def _():
        m = ldm.VQModel(ddconfig(2), n_embed=16, embed_dim=3, dims=2)
        return m, {"x": cl(N, (8, 8), 1), "z": cl(N, (4, 4), 3)}, lambda m, i: (m.prequant_cl(i["x"]), m.decode_cl(i["z"]))

    def forward_cl(m, i):
        return m.forward_cl(i["x"], i["bias_row"], i.get("context"), head_out=i.get("head_out"), head_ddim=i.get("head_ddim"),
                            head_post=i.get("head_post"))

    @case("UNetModel-forward_cl")
    def _():
        m = unet.UNetModel(image_size=8, in_channels=8, model_channels=32, out_channels=4, num_res_blocks=1, attention_resolutions=[2],
                           channel_mult=[1, 2], num_head_channels=32, dims=2, use_spatial_transformer=True, context_dim=48)
        M = N * 64
        inputs = {"x": cl(N, (8, 8), 8), "bias_row": torch.zeros(m.time_bias_layout(N)[1]), "context": cl(N, (7,), 48),
                  "head_out": torch.zeros(N, 1, 8, 8, 32), "ddim_x": torch.zeros(M, 4), "ddim_scalars": torch.zeros(4),
                  "ddim_pred_x0": torch.zeros(M, 4), "ddim_unet_in": torch.zeros(M, 32, dtype=BF16)}
        inputs["head_ddim"] = (inputs["ddim_x"], inputs["ddim_scalars"], inputs["ddim_pred_x0"], inputs["ddim_unet_in"])
        return m, inputs, forward_cl

    @case("UNetModel-forward_cl-attention-dims3")
    def _():
        m = unet.UNetModel(image_size=4, in_channels=4, model_channels=32, out_channels=4, num_res_blocks=1, attention_resolutions=[2],
                           channel_mult=[1, 2], num_head_channels=32, dims=3, use_scale_shift_norm=True, resblock_updown=True)
        return m, {"x": cl(N, (4, 4, 4), 4), "bias_row": torch.zeros(m.time_bias_layout(N)[1])}, forward_cl

    @case("CCDMUNetModel-forward_cl")
    def _():
        m = unet.CCDMUNetModel(in_channels=15, model_channels=32, out_channels=14, num_res_blocks=1, cond_encoded_shape=None,
                               attention_resolutions=[2], channel_mult=(1, 2), dims=3, num_heads=2)
        M = N * 64
        inputs = {"x": cl(N, (4, 4, 4), 15), "bias_row": torch.zeros(m.time_bias_layout(N)[1]), "post_xt": torch.zeros(M, dtype=torch.int32),
                  "post_scalars": torch.zeros(2), "post_labels_out": torch.zeros(M, dtype=torch.int32),
                  "post_philox_offset": torch.zeros(1, dtype=torch.int64)}
        inputs["head_post"] = dict(xt=inputs["post_xt"], scalars=inputs["post_scalars"], K=14, E=None, philox_seed=7,
                                   philox_offset=inputs["post_philox_offset"], draw=True, labels_out=inputs["post_labels_out"], onehot_out=None)
        return m, inputs, forward_cl

    for dim in (64, 48):
        @case(f"TransformerWrapper-dim{dim}")
        def _(dim=dim):
            m = cond.TransformerWrapper(num_tokens=50, max_seq_len=16, attn_layers=cond.Encoder(dim=dim, depth=1))
            return m, {"tokens": torch.arange(N * 7).view(N, 7) % 50}, lambda m, i: m.run(i["tokens"])

    @case("BertModel")
    def _():
        m = cond.BertModel(dict(vocab_size=50, hidden_size=64, num_hidden_layers=1, num_attention_heads=2, intermediate_size=128,
                                max_position_embeddings=16))
        ids = (torch.arange(N * 7).view(N, 7) % 50).int()
        return m, {"ids": ids, "ids_host": ids.clone()}, lambda m, i: m.run(i["ids"], [7, 3], ids_host=i["ids_host"])

    @case("SpatialRescaler")
    def _():
        m = cond.SpatialRescaler(n_stages=1, in_channels=3, out_channels=8).eval()
        return m, {"x": torch.zeros(N, 3, 8, 8)}, lambda m, i: m(i["x"])

    def fp32(name, make):
        @case(name + "-fp32")
        def _():
            def run(m, i):
                with ops.fp32_validation():
                    return m.run(i["h"])
            return make(), {"h": cl(N, grid(2), 64, F32)}, run

    fp32("AttentionBlock", lambda: B.AttentionBlock(64, num_head_channels=32))
    fp32("AttnBlock2d", lambda: B.AttnBlock2d(64))
    fp32("ResnetBlock", lambda: B.ResnetBlock(in_channels=64, out_channels=96))
    return cases


def case_names():
    return sorted(_cases())


def trace(name: str, answer: bool, defect=None) -> dict:
    """The trace of one case under one answer of the predicates: launches of the first run, the pack events of the first run (sorted),
    and `rerun`: what a second run of the same module adds (its pack events, and whether its launches differ from the first run's)."""
    torch.manual_seed(0)
    root, inputs, run = _cases()[name]()
    root.eval()
    seed_parameters(root)
    rec = Recorder(root, inputs, answer, defect)
    with torch.no_grad(), rec.patched():
        run(root, inputs)
        first, packs = rec.launches, rec.packs
        rec.launches, rec.packs = [], []
        run(root, inputs)
    return {"launches": first, "packs": sorted(packs, key=json.dumps),
            "rerun": {"packs": rec.packs, "same_launches": json.dumps(rec.launches) == json.dumps(first)}}


def settings():
    return [("all_false", False), ("all_true", True)]


def record_all() -> dict:
    return {f"{name}/{label}": trace(name, answer) for name in case_names() for label, answer in settings()}


def digest(v) -> str:
    return hashlib.sha1(json.dumps(v, sort_keys=True, separators=(",", ":")).encode()).hexdigest()[:8]


def fingerprint(t: dict) -> dict:
    """What the fixture keeps of a trace: `op:digest` of every launch entry in order, the sorted digests of the pack events, each list as
    one blank-separated string.  A digest
    covers the whole entry, so any operand, provenance or argument that changes changes it; the entries themselves are not stored
    (1636 of them: the fixture would be half a megabyte)."""
    return {"launches": " ".join(f"{e['op']}:{digest(e)}" for e in t["launches"]), "packs": " ".join(sorted(digest(p) for p in t["packs"]))}


def compare(got: dict, want: dict):
    """Differences between a trace and a fixture fingerprint, each named by launch index and op, with the entry as it is now."""
    fp, want, out = {k: v.split() for k, v in fingerprint(got).items()}, {k: v.split() for k, v in want.items()}, []
    ops_of = lambda launches: [e.split(":")[0] for e in launches]
    if ops_of(fp["launches"]) != ops_of(want["launches"]):
        out.append(f"launch sequence: got {ops_of(fp['launches'])}, fixture {ops_of(want['launches'])}")
    else:
        out += [f"launch {i} {e['op']}: not the fixture's launch; it is now {json.dumps(e)}"
                for i, (e, g, w) in enumerate(zip(got["launches"], fp["launches"], want["launches"])) if g != w]
    out += [f"pack event not in the fixture (module, key = cin_pad / tag, weights): {json.dumps(p)}" for p in got["packs"] if digest(p) not in want["packs"]]
    missing = sorted(set(want["packs"]) - set(fp["packs"]))
    if missing:
        out.append(f"{len(missing)} pack event(s) of the fixture missing (digests {missing})")
    if got["rerun"]["packs"]:
        out.append(f"a second run packed again: {got['rerun']['packs']}")
    if not got["rerun"]["same_launches"]:
        out.append("a second run made other launches than the first")
    return out


def diff_traces(got: dict, want: dict):
    """Differences between two full traces, each named by the argument: `launch 3 attention.k_off: got 64, want 128`."""
    got, want = json.loads(json.dumps(got)), json.loads(json.dumps(want))
    out = []
    gl, wl = got["launches"], want["launches"]
    if [e["op"] for e in gl] != [e["op"] for e in wl]:
        return [f"launch sequence: got {[e['op'] for e in gl]}, want {[e['op'] for e in wl]}"]
    for i, (g, w) in enumerate(zip(gl, wl)):
        out += [f"launch {i} {g['op']}.{f}: got {g.get(f)!r}, want {w.get(f)!r}" for f in sorted(set(g) | set(w)) if g.get(f) != w.get(f)]
    gp, wp = {json.dumps(p, sort_keys=True) for p in got["packs"]}, {json.dumps(p, sort_keys=True) for p in want["packs"]}
    out += [f"pack event added: {p}" for p in sorted(gp - wp)] + [f"pack event missing: {p}" for p in sorted(wp - gp)]
    return out
