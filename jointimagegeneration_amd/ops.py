"""Torch-facing wrappers over the C-ABI.  PyTorch only supplies device memory and the stream (plumbing);
every arithmetic op below is one or more hand-written HIP kernels in libguidegen_hip.so.

Activations travel as `CL` = channels-last bf16 tensors [N, D, H, W, Cpad] (D == 1 for 2-D), Cpad a multiple of 32
with zero pad lanes, plus the logical channel count.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import GG_BF16, GG_F32, AttentionDesc, ConvDesc, call, check


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def require_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what}: tensor is on {t.device}; the GuideGen engine runs on MI355X only "
                           "(no CPU fallback; the CPU restatement lives in oracle/ and is test infrastructure)")


# fp32 VALIDATION mode (gg_f32.hip; include/guidegen_hip.h): inside `with ops.fp32_validation():` the layout movers create fp32
# channels-last tensors and fp32 [taps][Cin][Cout] weight packs, and every op below routes fp32 tensors to the fp32 kernels (fixed-order
# fp32 FMA accumulation, fp64 GroupNorm statistics, fp32 attention).  It exists so that the CCDM sampler's labels can be compared exactly
# with the fp32 reference; nothing on the production path is changed by it, and there is still no CPU path.
FP32 = False


class fp32_validation:
    def __enter__(self):
        global FP32
        self.prev, FP32 = FP32, True
        return self

    def __exit__(self, *exc):
        global FP32
        FP32 = self.prev
        return False


def is_f32(t) -> bool:
    return t.dtype == torch.float32


PATH_HINT = 0        # gg_conv_desc.path_hint: tests set 1 / 4 / 6 to run small shapes on the halo-tile kernel (production: 0)
HINT_GATHER = 12     # production dispatch with the streaming 1x1 tile kernel switched off (tests, A/B)
HINT_TILE_S2 = 15        # tests: the stride-2 tile kernel wherever its shape envelope allows (the grid condition lifted)
HINT_NO_TILE_S2 = 14     # production dispatch with the stride-2 3x3x3 tile kernel (gg_conv_runs_tile_s2) switched off (tests, A/B)
HINT_NO_HALO_SPLIT = 13     # production dispatch with the split halo path (gg_conv_runs_halo_split) switched off (tests, A/B)
def weights_token(module) -> Tuple[int, int, int]:
    """Cheap identity of a module's current weights: (#tensors, sum of in-place version counters, sum of storage addresses).
    load_state_dict, LitEma.copy_to / restore and optimizer steps write in place (version bump); .to(device) moves storage.
    NOT detected: writes through `p.data` (`p.data.copy_(...)`, as the reference's own ema.py:57-65 does) -- they bypass the
    version counter.  Code that writes that way must call `invalidate_caches(module)` afterwards."""
    n = v = a = 0
    for p in module.parameters():
        n += 1
        v += p._version
        a += p.data_ptr()
    return n, v, a


def invalidate_caches(module) -> None:
    """Bump the version counter of every parameter (an in-place no-op write), so that every cache keyed by `weights_token` or by
    (data_ptr, _version) -- repacked weights, time-bias tables, captured hipGraphs -- is rebuilt on the next forward.  For callers
    that changed weights through `p.data` (invisible to autograd's version counter)."""
    with torch.no_grad():
        for p in module.parameters():
            p.add_(0)


def capture_graph(fn) -> "torch.cuda.CUDAGraph":
    """Capture `fn()` (launches on the current stream) into a hipGraph.  The cyclic garbage collector must not run inside the
    capture: if it frees an older CUDAGraph object there, hipGraphDestroy is refused ("operation not permitted when stream is
    capturing") inside a destructor and the process aborts.  So: collect first, keep the collector off while capturing."""
    import gc
    g = torch.cuda.CUDAGraph()
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g):
            fn()
    finally:
        if was_enabled:
            gc.enable()
    return g


def replay_captured(holder: dict, slot: str, body) -> None:
    """The one ladder of a graphable launch sequence `body`, its state in `holder` ("warmed" and `slot`): the first call runs `body`
    eagerly (that fills the weight-repack caches, which a capture must not do), the second captures it into holder[slot] and
    replays, every later one replays.  Callers keep their own eager branch for what is not graphable."""
    if not holder["warmed"]:
        body()
        holder["warmed"] = True
        return
    if holder[slot] is None:
        holder[slot] = capture_graph(body)
    holder[slot].replay()


def pad32(c: int) -> int:
    return (c + 31) // 32 * 32


@dataclass
class CL:
    """Channels-last activation: t is [N, D, H, W, Cpad] (bf16, or fp32 for head outputs); C = logical channels."""
    t: torch.Tensor
    C: int
    acc: Optional[torch.Tensor] = None      # int64 [N, stripes, Cpad, 2]: striped fixed-point per-channel (sum, sumsq) left by the producing conv
    fused_ddim: bool = False                # the producing (head) conv already applied the DDIM update (gg_conv_desc.ddim_x)
    fused_post: bool = False                # the producing (head) conv already ran the CCDM reverse step (gg_conv_desc.post_xt)

    @property
    def N(self): return self.t.shape[0]
    @property
    def spatial(self) -> Tuple[int, int, int]: return tuple(self.t.shape[1:4])
    @property
    def S(self) -> int: return self.t.shape[1] * self.t.shape[2] * self.t.shape[3]
    @property
    def Cpad(self) -> int: return self.t.shape[4]


# ----------------------------------------------------------------------------------------------- layout movers
def to_cl(x: torch.Tensor, c_pad: Optional[int] = None, out: Optional[torch.Tensor] = None, c_offset: int = 0,
          zero_fill: bool = True) -> CL:
    """NC[D]HW fp32 -> CL bf16 (optionally into channels [c_offset, c_offset+C) of an existing buffer)."""
    require_gpu(x, "to_cl")
    x = x.contiguous().float()
    N, Cc = x.shape[:2]
    sp = tuple(x.shape[2:])
    sp3 = (1,) * (3 - len(sp)) + sp
    S = sp3[0] * sp3[1] * sp3[2]
    if (out is None and FP32) or (out is not None and is_f32(out)):      # validation mode: fp32 channels-last (layout copy = plumbing)
        if out is None:
            out = torch.zeros((N,) + sp3 + (c_pad or pad32(Cc + c_offset),), dtype=torch.float32, device=x.device)
        elif zero_fill:
            out.zero_()
        out[..., c_offset:c_offset + Cc] = x.reshape(N, Cc, S).permute(0, 2, 1).reshape((N,) + sp3 + (Cc,))
        return CL(out, Cc + c_offset)
    if out is None:
        cp = c_pad or pad32(Cc + c_offset)
        out = torch.empty((N,) + sp3 + (cp,), dtype=torch.bfloat16, device=x.device)
    cp = out.shape[-1]
    call("gg_nchw_f32_to_cl_bf16", x.data_ptr(), N, Cc, S, out.data_ptr(), cp, c_offset, 1 if zero_fill else 0, _stream())
    return CL(out, Cc + c_offset)


def from_cl(cl: CL, ndim_spatial: int) -> torch.Tensor:
    """CL (bf16 or fp32) -> NC[D]HW fp32."""
    t = cl.t
    N, D, H, W, cp = t.shape
    sp = (D, H, W)[3 - ndim_spatial:]
    out = torch.empty((N, cl.C) + sp, dtype=torch.float32, device=t.device)
    dt = GG_BF16 if t.dtype == torch.bfloat16 else GG_F32
    call("gg_cl_to_nchw_f32", t.data_ptr(), dt, N, cl.C, D * H * W, cp, out.data_ptr(), _stream())
    return out


# ----------------------------------------------------------------------------------------------- conv
def pack_conv_weight(w: torch.Tensor, cin_pad: int) -> torch.Tensor:
    """fp32 OI[D]HW / OI (linear) -> MFMA tile order bf16 (device)."""
    require_gpu(w, "pack_conv_weight")
    lib = _lib.load()
    w = w.detach().contiguous().float()
    Cout, Cin = w.shape[:2]
    if FP32:                                     # validation mode: fp32 [taps][Cin_pad][Cout_pad], zero padded (layout copy = plumbing)
        wt = w.reshape(Cout, Cin, -1).permute(2, 1, 0)
        out = torch.zeros((wt.shape[0], cin_pad, pad32(Cout)), dtype=torch.float32, device=w.device)
        out[:, :Cin, :Cout] = wt
        return out
    ntaps = 1
    for s in w.shape[2:]:
        ntaps *= s
    nbytes = lib.gg_conv_packed_weight_bytes(Cout, cin_pad, ntaps)
    out = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=w.device)
    call("gg_conv_pack_weight", w.data_ptr(), Cout, Cin, cin_pad, ntaps, out.data_ptr(), _stream())
    return out


def pad_bias(b: Optional[torch.Tensor], cout: int, device) -> torch.Tensor:
    out = torch.zeros(pad32(cout), dtype=torch.float32, device=device)
    if b is not None:
        out[:cout] = b.detach().float()
    return out


def conv_out_extent(in_sp: Sequence[int], k: Sequence[int], stride: int, pad: int, upsample: bool):
    out = []
    for s, kk in zip(in_sp, k):
        if kk == 1:
            out.append((s - 1) // stride + 1)
        else:
            e = s * 2 if upsample else s
            if stride == 1:
                out.append(e + 2 * pad - 2)
            else:
                out.append((e + 2 - 3) // 2 + 1 if pad == 1 else (e + 1 - 3) // 2 + 1)
    return tuple(out)


def _shape_desc(src1: CL, cout: int, k, stride: int, pad: int, upsample: bool, src2: Optional[CL]) -> "ConvDesc":
    """The descriptor of conv(src1 | src2 -> cout): every shape field and path_hint, nothing else.  The dispatch predicates below and
    conv() all start from this one, so each of them answers for the convolution that conv() launches."""
    N, D, H, W, C1 = src1.t.shape
    Do, Ho, Wo = conv_out_extent((D, H, W), k, stride, pad, upsample)
    d = ConvDesc()
    d.N, d.D, d.H, d.W = N, D, H, W
    d.C1, d.C2 = C1, (src2.t.shape[-1] if src2 is not None else 0)
    d.Cout, d.Cout_pad = cout, pad32(cout)
    d.kd, d.kh, d.kw = k
    d.stride, d.pad, d.upsample = stride, pad, 1 if upsample else 0
    d.Do, d.Ho, d.Wo = Do, Ho, Wo
    d.path_hint = PATH_HINT
    return d


def conv_prologue_from_acc(src1: CL, cout: int, act: bool, k=(1, 3, 3), stride: int = 1, pad: int = 1, upsample: bool = False,
                           src2: Optional[CL] = None, **_ignored) -> bool:
    """True if this conv can compute act(GroupNorm(cat[src1, src2])) itself from the accumulators its producers left (CL.acc, 1-stripe
    layout): no statistics, scale / shift or apply launch at all (gg_conv_desc.pro_acc1)."""
    if not PROLOGUE_FROM_ACC or is_f32(src1.t) or not has_stats(src1, src2):
        return False
    if src2 is not None and src1.C != src1.Cpad:        # the in-kernel fold indexes channel c - C1 of the second source: C1 must be all logical
        return False
    d = _shape_desc(src1, cout, k, stride, pad, upsample, src2)
    d.prologue_act = 1 if act else 2
    d.pro_c_logical = src1.C + (src2.C if src2 is not None else 0)
    return bool(_lib.load().gg_conv_prologue_from_acc(C.byref(d)))


SKIP_KCONCAT = True                 # ResBlock 1x1 skip projections K-concatenated into conv2 where gg_conv_fuses_skip says so (A/B switch)


def conv_fuses_skip(src1: CL, cout: int, skip1: CL, skip2: Optional[CL] = None, k=(1, 3, 3), stride: int = 1, pad: int = 1, upsample: bool = False,
                    **_ignored) -> bool:
    """True if this conv (input src1, no second source) can take a K-concatenated 1x1 skip projection of cat[skip1, skip2]
    (gg_conv_desc.skip_src1): box kernel, 3x3, stride 1."""
    if not SKIP_KCONCAT or is_f32(src1.t) or (skip2 is not None and skip1.C != skip1.Cpad):
        return False
    d = _shape_desc(src1, cout, k, stride, pad, upsample, None)
    d.skip_C1, d.skip_C2 = skip1.Cpad, (skip2.Cpad if skip2 is not None else 0)
    return bool(_lib.load().gg_conv_fuses_skip(C.byref(d)))


def conv_runs_halo_tile(src1: CL, cout: int, k=(1, 3, 3), stride: int = 1, pad: int = 1, upsample: bool = False,
                        src2: Optional[CL] = None, **_ignored) -> bool:
    """True if gg_conv_forward runs this shape on the halo-tile kernel."""
    if is_f32(src1.t):
        return False
    return bool(_lib.load().gg_conv_runs_halo_tile(C.byref(_shape_desc(src1, cout, k, stride, pad, upsample, src2))))


def conv_fuses_prologue(src1: CL, cout: int, k=(1, 3, 3), stride: int = 1, pad: int = 1, upsample: bool = False,
                        src2: Optional[CL] = None, **_ignored) -> bool:
    """True if the GroupNorm (* SiLU) in front of this conv should be handed to the conv as its prologue (applied once per element while
    staging); False: a separate apply pass + the prologue-free conv is faster (gg_conv_fuses_prologue, measured rule in gg_conv_halo.hip)."""
    if is_f32(src1.t):
        return False
    return bool(_lib.load().gg_conv_fuses_prologue(C.byref(_shape_desc(src1, cout, k, stride, pad, upsample, src2))))


# ---- GroupNorm statistics emitted by conv epilogues (gg_conv_desc.gn_acc).  One int64 arena per device, bump-allocated per
# network forward and zeroed by ONE memset at the start of the next forward (static addresses: hipGraph friendly).
GN_ACC = True
TINY_IMAGE_POSITIONS = 0            # > 0: outputs with at most this many positions per sample also leave their sums, so that the next SiLU norm is folded into
                                    # its conv (16 = the 4x4 level: measured SLOWER, 1558 vs 1548 us per latent-UNet forward: producer epilogues + transform > launch)
# CCDM reverse step as the head conv's epilogue (gg_conv_desc.post_xt) where gg_conv_fuses_posterior says so (the 128^3 head).  Bit-identical
# to the two-launch form (tests).  What it buys is the 0.27 GB logit round trip only: the reverse step itself is ~3 k dependent vector
# instructions per voxel (IEEE divisions, Philox, exp) and VALU-bound wherever it runs -- rocprofv3, captured steps @128^3: head conv with the
# epilogue 523 us vs head conv 327 + sampler kernel 210 us (tools/experiments/probe_ccdm_step.py).  A/B switch.
FUSE_POSTERIOR = True
PROLOGUE_FROM_ACC = True            # box convs fold their producers' accumulators themselves where gg_conv_prologue_from_acc says so (A/B switch)
GN_ACC_MAX_ELEMS = 1 << 21          # per sample: only tensors whose norm is launch-bound (latent UNet at batch 1)
GN_ACC_MIN_ELEMS = 1 << 17          # below this the one-launch GroupNorm kernels are as fast (probe_gn_acc_min.py: 2^18 1593, 2^17 1586, 2^16 1590, 2^15 1604 us per forward)
_ARENA_ENTRIES = 1 << 19            # 4 MiB of int64 (the latent UNet at batch 1 uses ~0.4 M entries)
_ARENAS = {}


def stats_begin(device) -> None:
    """Start of a network forward: zero the arena and rewind.  Eager: zeroed is the prefix any forward so far has used (the high-water
    mark, rounded up to 64 Ki entries; entries beyond it have never been written: they are still the zeros of the allocation), so the
    fill (a dependent launch at the head of every forward, and 4 MiB of dirty L2 lines when the whole arena was zeroed) covers only what
    is in use (~1 MiB for the latent UNet).  While a hipGraph is being CAPTURED the whole arena is zeroed instead: the captured memset is
    fixed at capture time, and a forward captured cold (no eager run before it, so the mark still is 0) or one that allocates past the
    mark would otherwise replay onto its own previous sums."""
    if not GN_ACC:
        return
    a = _ARENAS.get(str(device))
    if a is None:
        a = _ARENAS[str(device)] = dict(buf=torch.zeros(_ARENA_ENTRIES, dtype=torch.int64, device=device), off=0, hi=0, active=False)
    else:
        a["hi"] = max(a["hi"], a["off"])
    if torch.cuda.is_current_stream_capturing():
        a["buf"].zero_()
        a["hi"] = _ARENA_ENTRIES                    # every later eager forward zeroes everything a replay may have dirtied
    elif a["hi"]:
        a["buf"][:min(_ARENA_ENTRIES, (a["hi"] + 65535) // 65536 * 65536)].zero_()
    a["off"] = 0
    a["active"] = True


def stats_end(device) -> None:
    a = _ARENAS.get(str(device))
    if a is not None:
        a["hi"] = max(a["hi"], a["off"])
        a["active"] = False


def _stats_alloc(device, N: int, cp: int, stripes: int) -> Optional[torch.Tensor]:
    a = _ARENAS.get(str(device))
    n = N * stripes * cp * 2            # stripes: 1 (box / 160-step kernels, GG_ACC_STRIPES) or 32 (halo-tile kernel)
    if a is None or not a["active"] or a["off"] + n > _ARENA_ENTRIES:
        return None
    v = a["buf"][a["off"]:a["off"] + n].view(N, stripes, cp, 2)
    a["off"] += n
    return v


def conv(src1: CL, weight: torch.Tensor, bias: Optional[torch.Tensor], cout: int, k=(1, 3, 3), stride: int = 1, pad: int = 1,
         upsample: bool = False, src2: Optional[CL] = None, residual: Optional[CL] = None, out_f32: bool = False,
         bias_per_sample: bool = False, prologue: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, prologue_silu: bool = True,
         out: Optional[torch.Tensor] = None, ddim: Optional[tuple] = None, geglu: bool = False, prologue_acc: Optional[tuple] = None,
         want_stats: bool = False, skip: Optional[tuple] = None, post: Optional[dict] = None) -> CL:
    """skip = (x1: CL, x2: CL or None, packed 1x1 weight): K-concatenated skip projection (conv_fuses_skip; `bias` must include its bias);
    prologue_acc = (gamma, beta, eps): GroupNorm prologue computed inside the conv from src1.acc / src2.acc (conv_prologue_from_acc);
    want_stats: leave the output's GroupNorm sums behind whatever its size (the consumer will fold them itself);
    ddim = (x fp32 [M,4], scalars fp32[4] on device, pred_x0 fp32 [M,4] or None, unet_in bf16 [M, stride] or None): the DDIM update
    runs as this (head) conv's epilogue when the kernel supports it (CL.fused_ddim tells); otherwise the caller launches gg_ddim_step;
    post = dict(xt, scalars, K, E, philox_seed, philox_offset, draw, labels_out, onehot_out): the CCDM reverse step (the arguments of
    ccdm_posterior_sample) as this (head) conv's epilogue where gg_conv_fuses_posterior says so (CL.fused_post tells; `out` is then not
    written); otherwise the caller launches gg_ccdm_posterior_sample on the logits."""
    lib = _lib.load()
    t1 = src1.t
    d = _shape_desc(src1, cout, k, stride, pad, upsample, src2)
    N, Do, Ho, Wo, cp = d.N, d.Do, d.Ho, d.Wo, d.Cout_pad
    if is_f32(t1):                                  # fp32 validation path (gg_conv_forward_f32)
        if geglu or prologue is not None or not is_f32(weight) or (residual is not None and not is_f32(residual.t)):
            raise RuntimeError("fp32 validation conv: fp32 weights / residual, no fused prologue or GEGLU (enter ops.fp32_validation() before the first forward)")
        if out is None:
            out = torch.empty((N, Do, Ho, Wo, cp), dtype=torch.float32, device=t1.device)
        d.out_dtype = GG_F32                        # (path_hint comes along from _shape_desc: gg_conv_forward_f32 does not read it)
        d.src1, d.src2 = t1.data_ptr(), (_ptr(src2.t) if src2 is not None else None)
        d.weight, d.bias, d.bias_stride = weight.data_ptr(), _ptr(bias), (cp if bias_per_sample else 0)
        d.residual = _ptr(residual.t) if residual is not None else None
        d.out = out.data_ptr()
        call("gg_conv_forward_f32", C.byref(d), _stream())
        return CL(out, cout)
    if geglu:      # fused GEGLU epilogue (gg_conv_desc.epilogue_geglu): cout = 2 * inner value | gate rows in, inner channels out
        if cout % 32 or out is not None or out_f32 or residual is not None:
            raise ValueError("conv(geglu=True): cout = 2 * inner with inner % 16 == 0, bf16 output, no residual")
        out = torch.empty((N, Do, Ho, Wo, cp // 2), dtype=torch.bfloat16, device=t1.device)
    if out is None:
        out = torch.empty((N, Do, Ho, Wo, cp), dtype=torch.float32 if out_f32 else torch.bfloat16, device=t1.device)
    d.out_dtype = GG_F32 if out.dtype == torch.float32 else GG_BF16
    d.prologue_act = (1 if prologue_silu else 2) if (prologue is not None or prologue_acc is not None) else 0
    if prologue_acc is not None:
        d.pro_gamma, d.pro_beta, d.pro_eps = prologue_acc[0].data_ptr(), prologue_acc[1].data_ptr(), float(prologue_acc[2])
        d.pro_acc1 = src1.acc.data_ptr()
        d.pro_acc2 = src2.acc.data_ptr() if src2 is not None else None
        d.pro_c_logical = src1.C + (src2.C if src2 is not None else 0)
    if skip is not None:
        d.skip_src1, d.skip_C1 = skip[0].t.data_ptr(), skip[0].Cpad
        d.skip_src2, d.skip_C2 = (skip[1].t.data_ptr(), skip[1].Cpad) if skip[1] is not None else (None, 0)
        d.skip_weight = skip[2].data_ptr()
    d.src1 = t1.data_ptr()
    d.src2 = _ptr(src2.t) if src2 is not None else None
    d.weight = weight.data_ptr()
    d.bias = _ptr(bias)
    d.bias_stride = cp if bias_per_sample else 0
    d.residual = _ptr(residual.t) if residual is not None else None
    d.out = out.data_ptr()
    d.gn_scale = _ptr(prologue[0]) if prologue is not None else None
    d.gn_shift = _ptr(prologue[1]) if prologue is not None else None
    d.epilogue_geglu = 1 if geglu else 0
    wsb = lib.gg_conv_workspace_bytes(C.byref(d))
    if wsb > 0:
        ws = torch.empty(wsb // 4, dtype=torch.float32, device=t1.device)
        d.workspace, d.workspace_bytes = ws.data_ptr(), wsb
    acc = None
    if GN_ACC and d.out_dtype == GG_BF16:
        # box / 160-step kernels (1 stripe): only where the norm is launch-bound; halo-tile kernel (32 stripes): always -- there the
        # sums replace a statistics PASS over a 17..805 MB tensor
        stripes = lib.gg_conv_emits_stats(C.byref(d))
        want = want_stats or (PROLOGUE_FROM_ACC and Do * Ho * Wo <= TINY_IMAGE_POSITIONS)
        if stripes == 32 or (stripes and (want or GN_ACC_MIN_ELEMS <= Do * Ho * Wo * cp) and Do * Ho * Wo * cp <= GN_ACC_MAX_ELEMS):
            acc = _stats_alloc(t1.device, N, cp, stripes)
            if acc is not None:
                d.gn_acc = acc.data_ptr()
    fused = False
    if ddim is not None and lib.gg_conv_fuses_ddim(C.byref(d)):
        x, scal, px0, uin = ddim
        d.ddim_x, d.ddim_scalars = x.data_ptr(), scal.data_ptr()
        d.ddim_pred_x0 = _ptr(px0)
        d.ddim_unet_in = _ptr(uin)
        d.ddim_unet_in_stride = uin.shape[-1] if uin is not None else 0
        fused = True
    fused_post = False
    if post is not None and FUSE_POSTERIOR and acc is None and post["K"] == cout and lib.gg_conv_fuses_posterior(C.byref(d)):
        oh = post.get("onehot_out")
        d.post_xt, d.post_labels_out, d.post_scalars = post["xt"].data_ptr(), post["labels_out"].data_ptr(), post["scalars"].data_ptr()
        d.post_E = _ptr(post.get("E"))
        d.post_philox_seed = int(post.get("philox_seed", 0))
        d.post_philox_offset_dev = _ptr(post.get("philox_offset"))
        d.post_draw = 1 if post.get("draw", True) else 0
        d.post_onehot_out, d.post_onehot_stride = _ptr(oh), (oh.shape[-1] if oh is not None else 0)
        seeds = post.get("philox_seeds")
        if seeds is not None:                   # one Philox key per sample (gg_conv_desc.post_philox_seeds)
            d.post_philox_seeds, d.post_rows_per_sample = _seeds_ptr(seeds, N), Do * Ho * Wo
        fused_post = True
    call("gg_conv_forward", C.byref(d), _stream())
    return CL(out, cout // 2 if geglu else cout, acc=acc, fused_ddim=fused, fused_post=fused_post)


# ----------------------------------------------------------------------------------------------- norms / elementwise
def _gn_sources(src1: CL, src2: Optional[CL], padded_first: str = "raise"):
    """What every GroupNorm(cat[src1, src2]) wrapper needs: (N, S, C1, C2, logical channels, pointer of the second source or None).
    The kernels that find channel c >= C1 at c - C1 of the second source need a first source without padding lanes; `padded_first`
    says what happens otherwise: "raise", "ignore", or "none" (None is returned: groupnorm_fused_ok)."""
    if src2 is not None and src1.C != src1.Cpad and padded_first != "ignore":
        if padded_first == "none":
            return None
        raise RuntimeError("two-source GroupNorm needs an unpadded first source")
    if src2 is None:
        return src1.N, src1.S, src1.Cpad, 0, src1.C, None
    return src1.N, src1.S, src1.Cpad, src2.Cpad, src1.C + src2.C, src2.t.data_ptr()


def _gn_out(src1: CL, Ct: int, dtype=torch.bfloat16) -> torch.Tensor:       # a GroupNorm's output: src1's positions, Ct channels
    return torch.empty(tuple(src1.t.shape[:4]) + (Ct,), dtype=dtype, device=src1.t.device)


def _gn_tables(src1: CL, N: int, Ct: int):                                   # per-(n, c) fp32 (scale, shift)
    return tuple(torch.empty((N, Ct), dtype=torch.float32, device=src1.t.device) for _ in range(2))


def groupnorm_stats(src1: CL, gamma: torch.Tensor, beta: torch.Tensor, eps: float, src2: Optional[CL] = None):
    """Returns per-(n, c) fp32 (scale, shift) with y = x*scale + shift == GroupNorm(32, C)(x)."""
    lib = _lib.load()
    N, S, C1, C2, c_log, p2 = _gn_sources(src1, src2)
    ws_bytes = lib.gg_groupnorm_workspace_bytes(N, S, C1 + C2)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=src1.t.device)
    scale, shift = _gn_tables(src1, N, C1 + C2)
    call("gg_groupnorm_stats", src1.t.data_ptr(), C1, p2, C2, N, S, c_log, gamma.data_ptr(), beta.data_ptr(), eps, scale.data_ptr(),
         shift.data_ptr(), ws.data_ptr(), ws_bytes, _stream())
    return scale, shift


def groupnorm_apply(src1: CL, scale: torch.Tensor, shift: torch.Tensor, act: bool, src2: Optional[CL] = None) -> CL:
    N, S, C1, C2, c_log, p2 = _gn_sources(src1, src2, "ignore")       # per-(n, c) tables: padding lanes of the first source have their own rows
    out = _gn_out(src1, C1 + C2)
    call("gg_groupnorm_apply", src1.t.data_ptr(), C1, p2, C2, N, S, scale.data_ptr(), shift.data_ptr(), 1 if act else 0, out.data_ptr(), _stream())
    return CL(out, c_log)


def groupnorm_fused_ok(src1: CL, src2: Optional[CL] = None) -> bool:
    hdr = None if is_f32(src1.t) else _gn_sources(src1, src2, "none")
    return hdr is not None and bool(_lib.load().gg_groupnorm_fused_supported(hdr[1], hdr[2], hdr[3], hdr[4]))


def groupnorm_fused(src1: CL, gamma: torch.Tensor, beta: torch.Tensor, eps: float, act: bool, src2: Optional[CL] = None) -> CL:
    """act(GroupNorm(32)(cat[src1, src2])) in one launch (small tensors: see groupnorm_fused_ok)."""
    N, S, C1, C2, c_log, p2 = _gn_sources(src1, src2, "ignore")       # the caller asked groupnorm_fused_ok
    out = _gn_out(src1, C1 + C2)
    call("gg_groupnorm_fused", src1.t.data_ptr(), C1, p2, C2, N, S, c_log, gamma.data_ptr(), beta.data_ptr(), eps, 1 if act else 0, out.data_ptr(),
         _stream())
    return CL(out, c_log)


def groupnorm_f32(src1: CL, gamma: torch.Tensor, beta: torch.Tensor, eps: float, act: bool, src2: Optional[CL] = None) -> CL:
    """fp32 validation path: act(GroupNorm(32)(cat[src1, src2])) on fp32 CL tensors (fp64 statistics, ATen's fp32 affine order)."""
    N, S, C1, C2, c_log, p2 = _gn_sources(src1, src2)
    out = _gn_out(src1, C1 + C2, torch.float32)
    ws = torch.empty(64 * N, dtype=torch.float32, device=src1.t.device)
    call("gg_groupnorm_f32", src1.t.data_ptr(), C1, p2, C2, N, S, c_log, gamma.data_ptr(), beta.data_ptr(), eps, 1 if act else 0, out.data_ptr(),
         ws.data_ptr(), _stream())
    return CL(out, c_log)


def groupnorm_f32_film(src: CL, gamma: torch.Tensor, beta: torch.Tensor, eps: float, film: torch.Tensor, act: bool) -> CL:
    """fp32 validation path of a FiLM out-norm: act(GroupNorm(32)(src) * (1 + s) + t) in the reference's order, with s = film[n, :C] and
    t = film[n, C:2C] (film fp32 [N, >= 2C], row-strided)."""
    N, S = src.N, src.S
    _check_film(film, N, src.C)
    out = _gn_out(src, src.Cpad, torch.float32)
    ws = torch.empty(64 * N, dtype=torch.float32, device=src.t.device)
    call("gg_groupnorm_f32_film", src.t.data_ptr(), src.Cpad, N, S, src.C, gamma.data_ptr(), beta.data_ptr(), eps, film.data_ptr(), film.stride(0),
         1 if act else 0, out.data_ptr(), ws.data_ptr(), _stream())
    return CL(out, src.C)


def film_fold(scale: torch.Tensor, shift: torch.Tensor, film: torch.Tensor, C: int) -> None:
    """In place: per-(n, c) GroupNorm coefficients [N, Ct] of a FiLM out-norm take the per-sample term *(1 + s) + t, s = film[n, :C],
    t = film[n, C:2C] (gg_film_fold); channels >= C are left as they are."""
    _check_film(film, scale.shape[0], C)
    call("gg_film_fold", scale.data_ptr(), shift.data_ptr(), scale.stride(0), scale.shape[0], C, film.data_ptr(), film.stride(0), _stream())


def _check_film(film: torch.Tensor, N: int, C: int) -> None:
    if film.dtype != torch.float32 or film.dim() != 2 or film.shape[0] != N or film.shape[1] < 2 * C or film.stride(1) != 1:
        raise ValueError(f"film must be fp32 [{N}, >= {2 * C}] rows with unit column stride, got {tuple(film.shape)} {film.dtype}")


def resample2x(src: CL, up: bool, resample_d: bool, prologue: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, act: bool = False) -> CL:
    """Nearest x2 upsample (up) or 2x average pool of a channels-last tensor (bf16, or fp32 in validation mode): H and W, and D too if
    resample_d.  prologue = per-(n, c) fp32 (scale, shift) [N, Cpad]: every input element becomes act(x * scale + shift) first (the h path
    of a down ResBlock in one launch).  The output carries no GroupNorm accumulators."""
    N, D, H, W, cp = src.t.shape
    Do = (D * 2 if up else D // 2) if resample_d else D
    out = torch.empty((N, Do, H * 2 if up else H // 2, W * 2 if up else W // 2, cp), dtype=src.t.dtype, device=src.t.device)
    if prologue is not None and tuple(prologue[0].shape) != (N, cp):
        raise ValueError(f"resample2x: prologue coefficients must be [{N}, {cp}]")
    call("gg_resample2x", src.t.data_ptr(), GG_F32 if is_f32(src.t) else GG_BF16, N, D, H, W, cp, src.C, 1 if resample_d else 0, 0 if up else 1,
         _ptr(prologue[0]) if prologue is not None else None, _ptr(prologue[1]) if prologue is not None else None,
         1 if (act and prologue is not None) else 0, out.data_ptr(), _stream())
    return CL(out, src.C)


def groupnorm_apply_acc(src1: CL, gamma: torch.Tensor, beta: torch.Tensor, eps: float, act: bool, src2: Optional[CL] = None) -> CL:
    """act(GroupNorm(32)(cat[src1, src2])) with the statistics taken from the accumulators the producing convs left in CL.acc."""
    N, S, C1, C2, c_log, p2 = _gn_sources(src1, src2)
    out = _gn_out(src1, C1 + C2)
    call("gg_groupnorm_apply_acc", src1.t.data_ptr(), C1, src1.acc.data_ptr(), p2, C2, src2.acc.data_ptr() if src2 is not None else None, N, S,
         c_log, gamma.data_ptr(), beta.data_ptr(), eps, 1 if act else 0, out.data_ptr(), _stream())
    return CL(out, c_log)


def has_stats(src1: CL, src2: Optional[CL] = None) -> bool:
    """the producing convs (box / 160-step kernels) left their accumulators: gg_groupnorm_apply_acc can normalise without a statistics launch"""
    ok = lambda c: c is None or (c.acc is not None and c.acc.shape[1] != 32)       # box / 160-step producers (GG_ACC_STRIPES), not the halo kernel's 32
    return GN_ACC and src1.acc is not None and ok(src1) and ok(src2) and src1.Cpad + (src2.Cpad if src2 is not None else 0) <= 2048


def has_any_stats(src1: CL, src2: Optional[CL] = None) -> bool:
    """the producing convs left accumulators (any stripe count): gg_groupnorm_scale_shift_acc replaces the statistics pass"""
    return GN_ACC and src1.acc is not None and (src2 is None or src2.acc is not None)


def groupnorm_scale_shift_acc(src1: CL, gamma: torch.Tensor, beta: torch.Tensor, eps: float, src2: Optional[CL] = None):
    """Per-(n, c) fp32 (scale, shift) of GroupNorm(32)(cat[src1, src2]) from the accumulators in CL.acc (no pass over the tensors)."""
    N, S, C1, C2, c_log, p2 = _gn_sources(src1, src2)
    scale, shift = _gn_tables(src1, N, C1 + C2)
    call("gg_groupnorm_scale_shift_acc", src1.acc.data_ptr(), src1.acc.shape[1], C1, src2.acc.data_ptr() if src2 is not None else None,
         src2.acc.shape[1] if src2 is not None else 0, C2, N, S, c_log, gamma.data_ptr(), beta.data_ptr(), eps, scale.data_ptr(), shift.data_ptr(),
         _stream())
    return scale, shift


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    out = torch.empty_like(x)
    call("gg_layernorm", x.data_ptr(), rows, Cc, gamma.data_ptr(), beta.data_ptr(), eps, out.data_ptr(), _stream())
    return out


def geglu(h: torch.Tensor, inner: int) -> torch.Tensor:
    rows = h.numel() // (2 * inner)
    out = torch.empty(tuple(h.shape[:-1]) + (inner,), dtype=torch.bfloat16, device=h.device)
    call("gg_geglu", h.data_ptr(), rows, inner, out.data_ptr(), _stream())
    return out


def add(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(a)
    call("gg_add", a.data_ptr(), b.data_ptr(), a.numel(), out.data_ptr(), _stream())
    return out


# ----------------------------------------------------------------------------------------------- cond stages (gg_cond.hip)
def embed_rows(ids: torch.Tensor, tok: torch.Tensor, pos: Optional[torch.Tensor] = None, bf16: bool = False) -> torch.Tensor:
    """Embedding gather (gg_embed_rows): ids integer [B, T] on the device, tok fp32 [V, D], pos fp32 [P, D] or None ->
    tok[ids] (+ pos[t]) as fp32 [B, T, D], or with bf16=True as channels-last token rows bf16 [B, 1, 1, T, pad32(D)] (pad lanes zero).
    The id range and T <= P are checked on the host first (ValueError naming the values): one sync, outside any captured graph."""
    require_gpu(ids, "embed_rows")
    if ids.dim() != 2 or ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool:
        raise ValueError(f"embed_rows: tokens must be an integer tensor of rank 2 [B, T], got {ids.dtype} {tuple(ids.shape)}")
    for name, t in (("tok", tok), ("pos", pos)):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or t.device != ids.device):
            raise ValueError(f"embed_rows: {name} must be a contiguous fp32 [rows, D] table on {ids.device}")
    B, T = (int(v) for v in ids.shape)
    V, D = (int(v) for v in tok.shape)
    if B < 1 or T < 1:
        raise ValueError(f"embed_rows: empty token tensor {tuple(ids.shape)}")
    P = 0
    if pos is not None:
        P = int(pos.shape[0])
        if pos.shape[1] != D:
            raise ValueError(f"embed_rows: pos has width {pos.shape[1]}, tok has {D}")
        if T > P:
            raise ValueError(f"embed_rows: sequence length {T} exceeds max_seq_len {P}")
    lo, hi = int(ids.min()), int(ids.max())                 # the one host sync of the call
    if lo < 0 or hi >= V:
        raise ValueError(f"embed_rows: token ids span [{lo}, {hi}], outside the table's [0, {V})")
    ids32 = ids.to(torch.int32).contiguous()
    if bf16:
        out = torch.empty((B, 1, 1, T, pad32(D)), dtype=torch.bfloat16, device=ids.device)
    else:
        out = torch.empty((B, T, D), dtype=torch.float32, device=ids.device)
    call("gg_embed_rows", ids32.data_ptr(), B * T, T, tok.data_ptr(), V, D, _ptr(pos), P, out.data_ptr(), GG_BF16 if bf16 else GG_F32, out.shape[-1],
         _stream())
    return out


def bert_embed(ids: torch.Tensor, type_ids: Optional[torch.Tensor], word: torch.Tensor, pos: torch.Tensor, type_tab: torch.Tensor,
               gamma: torch.Tensor, beta: torch.Tensor, eps: float, ids_host: Optional[torch.Tensor] = None,
               type_ids_host: Optional[torch.Tensor] = None) -> torch.Tensor:
    """transformers' BertEmbeddings in one launch (gg_bert_embed): ids int32 [B, T] on the device (type_ids likewise, or None for type 0),
    fp32 tables word [V, D], pos [P, D], type_tab [NT, D], gamma / beta [D] -> LayerNorm(word[ids] + type[tt] + pos[t]) as channels-last
    token rows bf16 [B, 1, 1, T, pad32(D)] (pad lanes zero).  ids_host / type_ids_host: the int32 CPU tensors the device ids were made
    from; the library checks them against the tables before it launches.  Nothing is read back from the device."""
    require_gpu(ids, "bert_embed")
    for name, t in (("ids", ids), ("type_ids", type_ids)):
        if t is not None and (t.dtype != torch.int32 or t.dim() != 2 or not t.is_contiguous() or t.shape != ids.shape or t.device != ids.device):
            raise ValueError(f"bert_embed: {name} must be a contiguous int32 tensor [B, T] on {ids.device}, got {t.dtype} {tuple(t.shape)}")
    for name, t in (("ids_host", ids_host), ("type_ids_host", type_ids_host)):
        if t is not None and (t.dtype != torch.int32 or t.is_cuda or not t.is_contiguous() or t.shape != ids.shape):
            raise ValueError(f"bert_embed: {name} must be a contiguous int32 CPU tensor of shape {tuple(ids.shape)}")
    D = int(word.shape[1])
    for name, t in (("word", word), ("pos", pos), ("type_tab", type_tab), ("gamma", gamma.view(1, -1)), ("beta", beta.view(1, -1))):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != D or not t.is_contiguous() or t.device != ids.device:
            raise ValueError(f"bert_embed: {name} must be a contiguous fp32 table of width {D} on {ids.device}")
    B, T = (int(v) for v in ids.shape)
    out = torch.empty((B, 1, 1, T, pad32(D)), dtype=torch.bfloat16, device=ids.device)
    call("gg_bert_embed", ids.data_ptr(), _ptr(type_ids), B * T, T, word.data_ptr(), int(word.shape[0]), pos.data_ptr(), int(pos.shape[0]),
         type_tab.data_ptr(), int(type_tab.shape[0]), D, gamma.data_ptr(), beta.data_ptr(), float(eps), out.data_ptr(), out.shape[-1],
         _ptr(ids_host), _ptr(type_ids_host), _stream())
    return out


def gelu(x: torch.Tensor) -> torch.Tensor:
    """Elementwise erf-form GELU of a contiguous bf16 tensor (gg_gelu)."""
    require_gpu(x, "gelu")
    if x.dtype != torch.bfloat16 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f"gelu: a non-empty contiguous bf16 tensor, got {x.dtype} {tuple(x.shape)}")
    out = torch.empty_like(x)
    call("gg_gelu", x.data_ptr(), x.numel(), out.data_ptr(), _stream())
    return out


def layernorm_rows(x: CL, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> CL:
    """LayerNorm over the x.C logical channels of channels-last bf16 rows (gg_layernorm_rows; pad lanes of the result are zero).
    `layernorm` normalises whole rows: it serves widths that are a multiple of 32, this one the others."""
    if x.t.dtype != torch.bfloat16 or not x.t.is_contiguous() or gamma.numel() != x.C or beta.numel() != x.C:
        raise ValueError(f"layernorm_rows: contiguous bf16 rows and {x.C} fp32 coefficients, got {x.t.dtype} {tuple(x.t.shape)}")
    out = torch.empty_like(x.t)
    call("gg_layernorm_rows", x.t.data_ptr(), x.t.numel() // x.Cpad, x.C, x.Cpad, gamma.data_ptr(), beta.data_ptr(), eps, out.data_ptr(), _stream())
    return CL(out, x.C)


INTERPOLATE_MODES = {"nearest": 0, "bilinear": 1, "bicubic": 2, "area": 3}


def interpolate_extent(n_in: int, scale_factor: float) -> int:
    """Output extent of F.interpolate(scale_factor=s): floor(in * s), the product in double."""
    import math
    return int(math.floor(float(n_in) * float(scale_factor)))


def interpolate2d(x: torch.Tensor, scale_factor: float, mode: str) -> torch.Tensor:
    """torch.nn.functional.interpolate(x, scale_factor=s, mode=mode) of an fp32 NCHW tensor on the device (gg_interpolate2d_f32;
    align_corners=False, no recompute_scale_factor): the coordinate scale is float(1.0 / s), the output extent floor(in * s)."""
    require_gpu(x, "interpolate2d")
    if mode not in INTERPOLATE_MODES:
        raise NotImplementedError(f"interpolate2d: mode {mode!r} is not supported (nearest, bilinear, bicubic, area)")
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"interpolate2d: an fp32 [N, C, H, W] tensor, got {x.dtype} {tuple(x.shape)}")
    s = float(scale_factor)
    if not s > 0.0:
        raise ValueError(f"interpolate2d: scale_factor = {scale_factor} must be positive")
    N, Cc, H, W = (int(v) for v in x.shape)
    Ho, Wo = interpolate_extent(H, s), interpolate_extent(W, s)
    if min(N, Cc, H, W) < 1 or Ho < 1 or Wo < 1:
        raise ValueError(f"interpolate2d: scale_factor {s} takes {tuple(x.shape)} to an extent of 0 ({Ho} x {Wo})")
    x = x.contiguous()
    out = torch.empty((N, Cc, Ho, Wo), dtype=torch.float32, device=x.device)
    scale = 1.0 / s                                         # ctypes rounds the double to fp32: float(1.0 / s)
    call("gg_interpolate2d_f32", x.data_ptr(), N * Cc, H, W, Ho, Wo, scale, scale, INTERPOLATE_MODES[mode], out.data_ptr(), _stream())
    return out


# ----------------------------------------------------------------------------------------------- attention
def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, N: int, heads: int, head_dim: int, Tq: int,
              Tkv: int, ld_hs_q, ld_hs_k, ld_hs_v, ld_hs_o, scale: float, q_off=0, k_off=0, v_off=0,
              kv_len: Optional[torch.Tensor] = None) -> None:
    """q/k/v/out are bf16 tensors; element (n,t,h,d) at base + off + (n*T+t)*ld + h*hs + d.
    kv_len: int32 device tensor [N]; sample n then attends to keys [0, kv_len[n]) only (gg_attention_forward_kvlen).  It is not read
    back: the caller checks 1 <= kv_len[n] <= Tkv on the host values it built the tensor from."""
    if kv_len is not None and (not isinstance(kv_len, torch.Tensor) or kv_len.dtype != torch.int32 or tuple(kv_len.shape) != (N,)
                               or not kv_len.is_contiguous() or kv_len.device != q.device):
        what = f"{kv_len.dtype} {tuple(kv_len.shape)} on {kv_len.device}" if isinstance(kv_len, torch.Tensor) else type(kv_len).__name__
        raise ValueError(f"attention: kv_len must be a contiguous int32 tensor [{N}] on {q.device}, got {what}")
    d = AttentionDesc()
    d.N, d.heads, d.head_dim, d.Tq, d.Tkv = N, heads, head_dim, Tq, Tkv
    d.ldq, d.hsq = ld_hs_q
    d.ldk, d.hsk = ld_hs_k
    d.ldv, d.hsv = ld_hs_v
    d.ldo, d.hso = ld_hs_o
    d.scale = scale
    esz = q.element_size()
    d.q = q.data_ptr() + esz * q_off
    d.k = k.data_ptr() + esz * k_off
    d.v = v.data_ptr() + esz * v_off
    d.out = out.data_ptr()
    if kv_len is not None:                          # key lengths: the plain kernel, no workspace
        call("gg_attention_forward_kvlen_f32" if is_f32(q) else "gg_attention_forward_kvlen", C.byref(d), kv_len.data_ptr(), _stream())
        return
    if is_f32(q):                                   # fp32 validation path
        call("gg_attention_forward_f32", C.byref(d), _stream())
        return
    wsb = _lib.load().gg_attention_workspace_bytes(C.byref(d))
    if wsb > 0:                                     # under-filled single-head grid (AE mid attention): keys split over workgroups
        ws = torch.empty(wsb // 4, dtype=torch.float32, device=q.device)
        d.workspace, d.workspace_bytes = ws.data_ptr(), wsb
    call("gg_attention_forward", C.byref(d), _stream())


# ----------------------------------------------------------------------------------------------- small fp32 ops
def linear_f32(x: torch.Tensor, W: torch.Tensor, b: Optional[torch.Tensor], act_in: bool = False,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    x = x.contiguous()
    M, I = x.shape
    O = W.shape[0]
    if out is None:
        out = torch.empty((M, O), dtype=torch.float32, device=x.device)
    call("gg_linear_f32", x.data_ptr(), M, I, W.data_ptr(), _ptr(b), O, 1 if act_in else 0, out.data_ptr(), out.stride(0), _stream())
    return out


def timestep_embedding(t: torch.Tensor, dim: int, max_period: float = 10000.0) -> torch.Tensor:
    t = t.float().contiguous()
    out = torch.empty((t.shape[0], dim), dtype=torch.float32, device=t.device)
    call("gg_timestep_embedding", t.data_ptr(), t.shape[0], dim, max_period, out.data_ptr(), _stream())
    return out


# ----------------------------------------------------------------------------------------------- samplers
def ccdm_posterior_sample(head: torch.Tensor, head_is_logits: bool, xt: torch.Tensor, scalars: torch.Tensor, K: int, *,
                          E: Optional[torch.Tensor] = None, philox_seed: int = 0, philox_offset: Optional[torch.Tensor] = None,
                          draw: bool = True, labels_out: Optional[torch.Tensor] = None, probs_out: Optional[torch.Tensor] = None,
                          onehot_out: Optional[torch.Tensor] = None, philox_seeds: Optional[torch.Tensor] = None) -> torch.Tensor:
    """head: fp32 [..., stride] (probs or logits, channels-last); xt int32 [M]; scalars fp32[2] on device.
    philox_seeds: device int64 [N] (bit patterns of the uint64 keys) with M a multiple of N: one Philox key per sample of M / N rows
    (gg_ccdm_posterior_sample_seeds) instead of `philox_seed` for all."""
    stride = head.shape[-1]
    M = head.numel() // stride
    if labels_out is None:
        labels_out = torch.empty(M, dtype=torch.int32, device=head.device)
    oh_stride = _onehot_stride(onehot_out, M, "ccdm_posterior_sample")
    if philox_seeds is not None:
        Ns = philox_seeds.numel()
        rps = _rows_per_sample(M, Ns, "ccdm_posterior_sample")
        call("gg_ccdm_posterior_sample_seeds", head.data_ptr(), stride, 1 if head_is_logits else 0, xt.data_ptr(), _ptr(E),
             _seeds_ptr(philox_seeds, Ns), rps, _ptr(philox_offset), 1 if draw else 0, scalars.data_ptr(), K, M, labels_out.data_ptr(),
             _ptr(probs_out), _ptr(onehot_out), oh_stride, _stream())
        return labels_out
    call("gg_ccdm_posterior_sample", head.data_ptr(), stride, 1 if head_is_logits else 0, xt.data_ptr(), _ptr(E), philox_seed, _ptr(philox_offset),
         1 if draw else 0, scalars.data_ptr(), K, M, labels_out.data_ptr(), _ptr(probs_out), _ptr(onehot_out), oh_stride, _stream())
    return labels_out


def _rows_per_sample(M: int, N: int, what: str) -> int:
    """M rows split into N equal samples: the rows of one."""
    if N < 1 or M % N:
        raise ValueError(f"{what}: {M} rows do not split into {N} samples")
    return M // N


def _onehot_stride(onehot_out: Optional[torch.Tensor], M: int, what: str) -> int:
    """onehot_out is contiguous bf16 rows [M, stride], or None: the stride (0)."""
    if onehot_out is None:
        return 0
    if onehot_out.dtype != torch.bfloat16 or not onehot_out.is_contiguous() or onehot_out.numel() != M * onehot_out.shape[-1]:
        raise ValueError(f"{what}: onehot_out must be contiguous bf16 rows [{M}, stride], got {onehot_out.dtype} {tuple(onehot_out.shape)}")
    return int(onehot_out.shape[-1])


def _seeds_ptr(seeds: torch.Tensor, N: int) -> int:
    if seeds.dtype != torch.int64 or not seeds.is_cuda or not seeds.is_contiguous() or seeds.numel() != N:
        raise ValueError(f"philox_seeds must be a contiguous device int64 tensor of {N} keys")
    return seeds.data_ptr()


def philox_seed_tensor(seeds: Sequence[int], device) -> torch.Tensor:
    """Device int64 tensor holding the uint64 Philox keys `seeds` bit for bit (what `philox_seeds` arguments take)."""
    return torch.tensor([int(s) - (1 << 64) if int(s) >= (1 << 63) else int(s) for s in seeds], dtype=torch.int64, device=device)


def ccdm_draw_tape(M: int, kmax: int, *, philox_seed: int = 0, philox_seeds: Optional[torch.Tensor] = None,
                   philox_offset: Optional[torch.Tensor] = None, bits_in: Optional[torch.Tensor] = None, want_bits: bool = True,
                   want_E: bool = True, device=None) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """The tape of a Philox run (gg_ccdm_draw_tape): (words int32 [M, kmax] holding the uint32 bit patterns, E fp32 [M, kmax]) as
    ccdm_posterior_sample / ccdm_q_sample / the fused head conv draw them for the same philox_seed (or philox_seeds: device int64 [N], M a
    multiple of N) and philox_offset; kmax is 16 for K <= 16 and 32 above.  E[:, :K].contiguous() is the tape `E` of those calls.
    bits_in: device int32 [M, kmax] words to map instead of drawing."""
    if bits_in is not None:
        if bits_in.dtype != torch.int32 or not bits_in.is_cuda or not bits_in.is_contiguous() or bits_in.numel() != M * kmax:
            raise ValueError(f"ccdm_draw_tape: bits_in must be a contiguous device int32 [{M}, {kmax}] tensor")
        device = bits_in.device
    elif philox_seeds is not None:
        device = philox_seeds.device
    elif philox_offset is not None:
        device = philox_offset.device
    if device is None:
        device = torch.device("cuda")
    if not (want_bits or want_E):
        raise ValueError("ccdm_draw_tape: neither the words nor the exponentials are asked for")
    Ns, rps = 0, 0
    if philox_seeds is not None and bits_in is None:
        Ns = philox_seeds.numel()
        rps = _rows_per_sample(M, Ns, "ccdm_draw_tape")
    bits = torch.empty((M, kmax), dtype=torch.int32, device=device) if want_bits else None
    E = torch.empty((M, kmax), dtype=torch.float32, device=device) if want_E else None
    call("gg_ccdm_draw_tape", int(philox_seed) & ((1 << 64) - 1), _seeds_ptr(philox_seeds, Ns) if Ns else None, rps, _ptr(philox_offset), kmax, M,
         _ptr(bits_in), _ptr(bits), _ptr(E), _stream())
    return bits, E


def labels_to_onehot(labels: torch.Tensor, K: int, out: torch.Tensor) -> None:
    if is_f32(out):                                 # fp32 validation path: index scatter (plumbing)
        out[:, :K] = torch.nn.functional.one_hot(labels.long(), K).to(torch.float32)
        return
    call("gg_labels_to_onehot", labels.data_ptr(), labels.numel(), K, out.data_ptr(), out.shape[-1], _stream())


def ddim_step(x: torch.Tensor, eps: torch.Tensor, scalars: torch.Tensor, noise: Optional[torch.Tensor] = None,
              pred_x0_out: Optional[torch.Tensor] = None, unet_in: Optional[torch.Tensor] = None) -> None:
    """x fp32 CL [M, C] (updated in place); eps fp32 CL [M, stride]; scalars fp32[4] on device."""
    Cc = x.shape[-1]
    M = x.numel() // Cc
    call("gg_ddim_step", x.data_ptr(), eps.data_ptr(), eps.shape[-1], _ptr(noise), scalars.data_ptr(), M, Cc, _ptr(pred_x0_out), _ptr(unet_in),
         unet_in.shape[-1] if unet_in is not None else 0, _stream())


def inpaint_blend(x: torch.Tensor, x0: torch.Tensor, mask: torch.Tensor, noise: torch.Tensor, scalars: torch.Tensor,
                  unet_in: Optional[torch.Tensor] = None) -> None:
    """x <- q_sample(x0, t, noise) * mask + (1 - mask) * x in place; x, x0, noise fp32 CL [M, C], mask fp32 CL [M, 1 or C],
    scalars fp32[2] = (sqrt_alphas_cumprod[t], sqrt_one_minus_alphas_cumprod[t]) on device; unet_in channels [0, C) <- bf16(x)."""
    Cc = x.shape[-1]
    M = x.numel() // Cc
    for name, t, c in (("x", x, Cc), ("x0", x0, Cc), ("noise", noise, Cc), ("mask", mask, mask.shape[-1])):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != M * c:
            raise ValueError(f"inpaint_blend: {name} must be contiguous fp32 [{M}, {c}], got {t.dtype} {tuple(t.shape)}")
    call("gg_inpaint_blend", x.data_ptr(), x0.data_ptr(), mask.data_ptr(), mask.shape[-1], noise.data_ptr(), scalars.data_ptr(), M, Cc,
         _ptr(unet_in), unet_in.shape[-1] if unet_in is not None else 0, _stream())


def _codebook(codebook: torch.Tensor, what: str) -> Tuple[int, int]:
    if codebook.dtype != torch.float32 or codebook.dim() != 2 or not codebook.is_contiguous() or not codebook.is_cuda:
        raise ValueError(f"{what}: the codebook must be a contiguous device fp32 [n_embed, C] tensor, got {codebook.dtype} {tuple(codebook.shape)}")
    return int(codebook.shape[0]), int(codebook.shape[1])


def vq_nearest(rows: torch.Tensor, codebook: torch.Tensor, C: Optional[int] = None, *, idx_out: Optional[torch.Tensor] = None,
               st_out: Optional[torch.Tensor] = None, want_st: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Nearest codebook entry of every channels-last row (gg_vq_nearest).  rows fp32 [..., stride] with the channels in [0, C) (C defaults
    to the codebook's width, stride >= C); codebook fp32 [n_embed, C].  Returns (indices int32 [M], straight-through rows fp32 [M, C] =
    z + (E[idx] - z), or None with want_st=False).  st_out may be given (fp32 [M, st_stride >= C], or `rows` itself for in place)."""
    require_gpu(rows, "vq_nearest")
    n_embed, Ce = _codebook(codebook, "vq_nearest")
    C = Ce if C is None else C
    stride = rows.shape[-1]
    if C != Ce or rows.dtype != torch.float32 or not rows.is_contiguous() or stride < C:
        raise ValueError(f"vq_nearest: rows must be contiguous fp32 [..., stride >= {Ce}] for a codebook of width {Ce}, got {rows.dtype} "
                         f"{tuple(rows.shape)} with C={C}")
    M = rows.numel() // stride
    if idx_out is None:
        idx_out = torch.empty(M, dtype=torch.int32, device=rows.device)
    if st_out is None and want_st:
        st_out = torch.empty((M, C), dtype=torch.float32, device=rows.device)
    if idx_out.dtype != torch.int32 or idx_out.numel() != M or not idx_out.is_contiguous():
        raise ValueError(f"vq_nearest: idx_out must be a contiguous int32 tensor of {M} indices")
    st_stride = 0
    if st_out is not None:
        st_stride = st_out.shape[-1]
        if st_out.dtype != torch.float32 or not st_out.is_contiguous() or st_stride < C or st_out.numel() != M * st_stride:
            raise ValueError(f"vq_nearest: st_out must be contiguous fp32 [{M}, stride >= {C}]")
    call("gg_vq_nearest", rows.data_ptr(), stride, codebook.data_ptr(), n_embed, C, M, idx_out.data_ptr(), _ptr(st_out), st_stride, _stream())
    return idx_out, st_out


def ddim_step_vq(x: torch.Tensor, eps: torch.Tensor, scalars: torch.Tensor, codebook: Optional[torch.Tensor],
                 noise: Optional[torch.Tensor] = None, pred_x0_out: Optional[torch.Tensor] = None, unet_in: Optional[torch.Tensor] = None,
                 idx_out: Optional[torch.Tensor] = None, ancestral: bool = False) -> None:
    """One reverse step with the prediction of x_0 quantised (gg_ddim_step_vq).  x fp32 CL [M, C] (updated in place); eps fp32 CL
    [M, stride]; scalars fp32[5] on device: (a_t, a_prev, sigma_t, sqrt(1 - a_t), noise coefficient), or with ancestral=True gg_ddpm_step's
    five; codebook fp32 [n_embed, C], or None for the step without a quantiser; pred_x0_out receives the quantised prediction."""
    Cc = x.shape[-1]
    M = x.numel() // Cc
    n_embed = 0
    if codebook is not None:
        n_embed, Ce = _codebook(codebook, "ddim_step_vq")
        if Ce != Cc:
            raise ValueError(f"ddim_step_vq: the codebook has width {Ce}, the state has {Cc} channels")
    if scalars.numel() < 5 or scalars.dtype != torch.float32 or not scalars.is_contiguous():
        raise ValueError("ddim_step_vq: scalars must be a contiguous fp32[5] device tensor")
    for name, t in (("x", x), ("noise", noise), ("pred_x0_out", pred_x0_out)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != M * Cc):
            raise ValueError(f"ddim_step_vq: {name} must be contiguous fp32 [{M}, {Cc}], got {t.dtype} {tuple(t.shape)}")
    if idx_out is not None and (idx_out.dtype != torch.int32 or idx_out.numel() != M or not idx_out.is_contiguous()):
        raise ValueError(f"ddim_step_vq: idx_out must be a contiguous int32 tensor of {M} indices")
    call("gg_ddim_step_vq", x.data_ptr(), eps.data_ptr(), eps.shape[-1], _ptr(noise), scalars.data_ptr(), 1 if ancestral else 0, _ptr(codebook),
         n_embed, M, Cc, _ptr(idx_out), _ptr(pred_x0_out), _ptr(unet_in), unet_in.shape[-1] if unet_in is not None else 0, _stream())


def unfold_extent(H: int, W: int, kh: int, kw: int, sy: int, sx: int) -> Tuple[int, int]:
    """(Ly, Lx) of torch.nn.Unfold with dilation 1 and padding 0."""
    return (H - kh) // sy + 1, (W - kw) // sx + 1


def _cl_dtype(t: torch.Tensor, what: str) -> int:
    if t.dtype == torch.float32:
        return GG_F32
    if t.dtype == torch.bfloat16:
        return GG_BF16
    raise ValueError(f"{what}: fp32 or bf16 channels-last tensors, got {t.dtype}")


def _rows_dense(t: torch.Tensor) -> bool:
    """A 4-D channels-last tensor (or view) whose pixel rows lie t.stride(2) elements apart with nothing between the lines."""
    return (t.dim() == 4 and (t.stride(3) == 1 or t.shape[3] == 1) and (t.shape[1] == 1 or t.stride(1) == t.shape[2] * t.stride(2))
            and (t.shape[0] == 1 or t.stride(0) == t.shape[1] * t.shape[2] * t.stride(2)) and t.stride(2) >= t.shape[3])


def unfold_cl(src: torch.Tensor, C: int, kh: int, kw: int, sy: int, sx: int, out: Optional[torch.Tensor] = None, c_offset: int = 0) -> torch.Tensor:
    """Crop gather (gg_unfold_cl): src channels-last [N, H, W, stride] (fp32 or bf16; channels [0, C) are read; a view whose rows are
    `stride` elements apart) -> out [L * N, kh, kw, stride_out], channels [c_offset, c_offset + C), crop l of sample n at row l * N + n.
    out defaults to a fresh tensor of src's dtype and C channels; a bf16 out of an fp32 src converts on the way.  Other lanes of out
    are left as they are."""
    require_gpu(src, "unfold_cl")
    if not _rows_dense(src):
        raise ValueError(f"unfold_cl: src must be channels-last [N, H, W, C] with densely packed rows, got {tuple(src.shape)} strides {src.stride()}")
    N, H, W = (int(v) for v in src.shape[:3])
    s_stride = int(src.stride(2))
    if kh > H or kw > W or min(kh, kw, sy, sx) < 1:
        raise ValueError(f"unfold_cl: crop {kh}x{kw} at stride {sy}x{sx} does not fit {H}x{W}")
    Ly, Lx = unfold_extent(H, W, kh, kw, sy, sx)
    if out is None:
        out = torch.empty((Ly * Lx * N, kh, kw, C), dtype=src.dtype, device=src.device)
    if out.dim() != 4 or tuple(out.shape[:3]) != (Ly * Lx * N, kh, kw) or not out.is_contiguous():
        raise ValueError(f"unfold_cl: out must be a contiguous [{Ly * Lx * N}, {kh}, {kw}, stride] tensor, got {tuple(out.shape)}")
    call("gg_unfold_cl", src.data_ptr(), _cl_dtype(src, "unfold_cl"), N, H, W, s_stride, C, out.data_ptr(), _cl_dtype(out, "unfold_cl"),
         out.shape[-1], c_offset, kh, kw, sy, sx, _stream())
    return out


def fold_weighted_cl(crops: torch.Tensor, C: int, weight: torch.Tensor, tie: Optional[torch.Tensor], out: torch.Tensor,
                     kh: int, kw: int, sy: int, sx: int) -> torch.Tensor:
    """Weighted overlap-add (gg_fold_weighted_cl): crops fp32 [L * N, kh, kw, stride] -> out fp32 channels-last [N, H, W, stride_out],
    channels [0, C): sum_l(o[l] * w[l]) / sum_l(w[l]) with w[l][ky, kx] = weight[ky, kx] * tie[l], crops visited in descending l (the
    order of torch's CPU Fold; include/guidegen_hip.h).  weight fp32 [kh, kw], tie fp32 [L] or None.  crops / out may be views whose
    rows are `stride` elements apart."""
    require_gpu(crops, "fold_weighted_cl")
    if out.dtype != torch.float32 or not _rows_dense(out):
        raise ValueError(f"fold_weighted_cl: out must be fp32 channels-last [N, H, W, C] with densely packed rows, got {out.dtype} {tuple(out.shape)}")
    N, H, W = (int(v) for v in out.shape[:3])
    if kh > H or kw > W or min(kh, kw, sy, sx) < 1:
        raise ValueError(f"fold_weighted_cl: crop {kh}x{kw} at stride {sy}x{sx} does not fit {H}x{W}")
    Ly, Lx = unfold_extent(H, W, kh, kw, sy, sx)
    if crops.dtype != torch.float32 or not _rows_dense(crops) or tuple(crops.shape[:3]) != (Ly * Lx * N, kh, kw):
        raise ValueError(f"fold_weighted_cl: crops must be fp32 [{Ly * Lx * N}, {kh}, {kw}, C] with densely packed rows, got {crops.dtype} {tuple(crops.shape)}")
    if weight.dtype != torch.float32 or not weight.is_contiguous() or weight.numel() != kh * kw or weight.device != crops.device:
        raise ValueError(f"fold_weighted_cl: weight must be a contiguous device fp32 [{kh}, {kw}] table")
    if tie is not None and (tie.dtype != torch.float32 or not tie.is_contiguous() or tie.numel() != Ly * Lx or tie.device != crops.device):
        raise ValueError(f"fold_weighted_cl: tie must be a contiguous device fp32 [{Ly * Lx}] table")
    call("gg_fold_weighted_cl", crops.data_ptr(), int(crops.stride(2)), weight.data_ptr(), _ptr(tie), out.data_ptr(), int(out.stride(2)), N, H, W, C,
         kh, kw, sy, sx, _stream())
    return out


def _label_rows(t: torch.Tensor, K: int, what: str) -> torch.Tensor:
    """[S, *spatial] integer labels -> contiguous int32 [S, M] (plumbing; an int64 label is clamped to [-1, K] first, so that no value
    outside int32 can wrap into the valid range)."""
    require_gpu(t, what)
    if t.dim() < 2 or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"{what}: labels must be an integer tensor [S, *spatial], got {t.dtype} {tuple(t.shape)}")
    if t.dtype == torch.int64:
        t = t.clamp(-1, K)
    return t.reshape(t.shape[0], -1).to(torch.int32).contiguous()


def label_confusion(a: torch.Tensor, b: torch.Tensor, K: int) -> torch.Tensor:
    """Pairwise confusion matrices of label volumes (gg_label_confusion): a [Sa, *spatial], b [Sb, *spatial] integer tensors on the device
    -> int64 [Sa, Sb, K, K] with cm[i, j, p, q] = #{voxels m : a[i, m] == p and b[j, m] == q}.  `b is a` scores the self pairs on one
    buffer.  A label outside [0, K) raises ValueError naming the first such pair and its voxel count (ignite's ConfusionMatrix raises on
    such labels too); reading that count back is the one host sync of the call."""
    ra = _label_rows(a, K, "label_confusion")
    rb = ra if b is a else _label_rows(b, K, "label_confusion")
    if ra.shape[1] != rb.shape[1] or ra.device != rb.device:
        raise ValueError(f"label_confusion: volumes of {tuple(a.shape[1:])} and {tuple(b.shape[1:])} voxels (or on two devices)")
    if not 1 <= K <= 32:
        raise ValueError(f"label_confusion: K={K} outside [1, 32]")
    Sa, Sb, M = ra.shape[0], rb.shape[0], ra.shape[1]
    cm = torch.empty((Sa, Sb, K, K), dtype=torch.int64, device=ra.device)
    skipped = torch.empty((Sa, Sb), dtype=torch.int64, device=ra.device)
    call("gg_label_confusion", ra.data_ptr(), Sa, rb.data_ptr(), Sb, M, K, cm.data_ptr(), skipped.data_ptr(), _stream())
    sk = skipped.cpu()
    if int(sk.sum()) != 0:
        i, j = (int(v) for v in torch.nonzero(sk)[0])
        raise ValueError(f"label_confusion: pair ({i}, {j}) has {int(sk[i, j])} voxel(s) with a label outside [0, {K}) "
                         f"({int((sk != 0).sum())} of {Sa * Sb} pairs affected)")
    return cm


# ----------------------------------------------------------------------------------- cleaning label volumes (gg_components.hip)
def _labels_i32(t: torch.Tensor, what: str, name: str, dim: Optional[int] = None) -> None:
    require_gpu(t, what)
    if t.dtype != torch.int32 or not t.is_contiguous() or (dim is not None and t.dim() != dim):
        shape = "" if dim is None else f" with {dim} dimensions"
        raise ValueError(f"{what}: {name} must be a contiguous int32 tensor{shape}, got {t.dtype} {tuple(t.shape)}"
                         f"{'' if t.is_contiguous() else ' (not contiguous)'}")


def _check_classes(what: str, K: int) -> None:
    if not isinstance(K, int) or not 1 <= K <= 32:
        raise ValueError(f"{what}: K={K} outside [1, 32]")


_VOTE_TABLES: dict = {}
_COMPONENT_STATUS: dict = {}


def vote_operands(S: int) -> Tuple["np.ndarray", float, float]:
    """The three fp32 operands of gg_label_vote's entropy, computed in fp64 and rounded once: table[c] = c ln c (c = 0 .. S; table[0] =
    0), ln S, 1 / S.  Returns (numpy fp32 table, ln_s, inv_s), the two scalars as Python floats that hold fp32 values."""
    import math
    import numpy as np
    table = np.array([0.0] + [c * math.log(c) for c in range(1, S + 1)], dtype=np.float64).astype(np.float32)
    return table, float(np.float32(math.log(S))), float(np.float32(1.0 / S))


def component_status(device) -> torch.Tensor:
    """The device status word of the component kernels on `device` (int32 [1], zero unless a loop bound was reached)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"component_status: {device} is not a GPU")
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _COMPONENT_STATUS:
        _COMPONENT_STATUS[key] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", key))
    return _COMPONENT_STATUS[key]


def check_component_status(device) -> None:
    """Reads the status word back (one host sync) and raises if a find or union of gg_label_components reached its bound: the roots it
    wrote are then not to be trusted.  Called wherever the host layer reads component results back."""
    st = component_status(device)
    v = int(st.item())
    if v != 0:
        st.zero_()
        raise RuntimeError(f"label_components: a device loop reached its bound of one volume's voxel count (status {v}: "
                           "1 find, 2 union, 3 flatten); the component roots of this device are invalid")


def label_vote(labels: torch.Tensor, K: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Per-voxel vote of S samples (gg_label_vote): labels int32 [S, M] on the device -> (winner int32 [M], agreement int32 [M], entropy
    fp32 [M] in nats, skipped int64 [1] on the device: votes outside [0, K), which are not cast).  Ties go to the smallest label."""
    _labels_i32(labels, "label_vote", "labels", 2)
    _check_classes("label_vote", K)
    S, M = int(labels.shape[0]), int(labels.shape[1])
    if not 1 <= S <= 64:
        raise ValueError(f"label_vote: S={S} samples outside [1, 64]")
    if not 1 <= M < 2 ** 31:
        raise ValueError(f"label_vote: M={M} voxels outside [1, 2^31)")
    dev = labels.device
    key = (S, dev.index)
    if key not in _VOTE_TABLES:
        table, ln_s, inv_s = vote_operands(S)
        _VOTE_TABLES[key] = (torch.from_numpy(table).to(dev), ln_s, inv_s)
    table, ln_s, inv_s = _VOTE_TABLES[key]
    winner = torch.empty(M, dtype=torch.int32, device=dev)
    agreement = torch.empty(M, dtype=torch.int32, device=dev)
    entropy = torch.empty(M, dtype=torch.float32, device=dev)
    skipped = torch.empty(1, dtype=torch.int64, device=dev)
    call("gg_label_vote", labels.data_ptr(), S, M, K, table.data_ptr(), ln_s, inv_s, winner.data_ptr(), agreement.data_ptr(), entropy.data_ptr(),
         skipped.data_ptr(), _stream())
    return winner, agreement, entropy, skipped


def _check_volumes(what: str, labels: torch.Tensor) -> Tuple[int, int]:
    B = int(labels.shape[0])
    M = 1
    for v in labels.shape[1:]:
        M *= int(v)
    if not 1 <= B <= 65535:
        raise ValueError(f"{what}: B={B} volumes outside [1, 65535]")
    if not 1 <= M < 2 ** 31:
        raise ValueError(f"{what}: {M} voxels per volume outside [1, 2^31)")
    return B, M


def label_components(labels: torch.Tensor, K: int, connectivity: int = 6, background: int = 0) -> torch.Tensor:
    """Connected components (gg_label_components): labels int32 [B, D, H, W] -> root int32 [B, D*H*W], the smallest linear index of the
    voxel's component within its volume, -1 for `background` (-1: none) and for labels outside [0, K).  connectivity 6 or 26."""
    _labels_i32(labels, "label_components", "labels", 4)
    _check_classes("label_components", K)
    if connectivity not in (6, 26):
        raise ValueError(f"label_components: connectivity {connectivity} is neither 6 nor 26")
    if not isinstance(background, int) or not -1 <= background < K:
        raise ValueError(f"label_components: background {background} outside [-1, {K})")
    B, M = _check_volumes("label_components", labels)
    D, H, W = (int(v) for v in labels.shape[1:])
    lib = _lib.load()
    root = torch.empty((B, M), dtype=torch.int32, device=labels.device)
    nbytes = int(lib.gg_label_components_workspace_bytes(B, M))
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=labels.device)
    status = component_status(labels.device)
    call("gg_label_components", labels.data_ptr(), B, D, H, W, K, connectivity, background, root.data_ptr(), ws.data_ptr(), nbytes,
         status.data_ptr(), _stream())
    return root


def _check_root(what: str, labels: torch.Tensor, root: torch.Tensor, B: int, M: int) -> None:
    _labels_i32(root, what, "root", 2)
    if tuple(root.shape) != (B, M) or root.device != labels.device:
        raise ValueError(f"{what}: root must be int32 [{B}, {M}] on {labels.device}, got {tuple(root.shape)} on {root.device}")


def component_stats(labels: torch.Tensor, root: torch.Tensor, K: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """gg_component_stats: labels int32 [B, ...], root int32 [B, M] -> (size int32 [B, M]: the component's voxel count at its root, 0
    elsewhere; stats int64 [B, K, 4] = (components, voxels, size of the largest, root of the largest or -1), ties to the smaller root)."""
    _labels_i32(labels, "component_stats", "labels")
    if labels.dim() < 2:
        raise ValueError(f"component_stats: labels must be [B, *spatial], got {tuple(labels.shape)}")
    _check_classes("component_stats", K)
    B, M = _check_volumes("component_stats", labels)
    _check_root("component_stats", labels, root, B, M)
    size = torch.empty((B, M), dtype=torch.int32, device=labels.device)
    stats = torch.empty((B, K, 4), dtype=torch.int64, device=labels.device)
    call("gg_component_stats", labels.data_ptr(), root.data_ptr(), B, M, K, size.data_ptr(), stats.data_ptr(), _stream())
    return size, stats


def component_filter(labels: torch.Tensor, root: torch.Tensor, size: torch.Tensor, stats: torch.Tensor, K: int, keep_largest: torch.Tensor,
                     min_size: torch.Tensor, background: int = 0, fill: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """gg_component_filter: a voxel keeps its label iff its class is `background`, or (keep_largest[class] == 0 or its component is the
    class's largest) and size >= min_size[class]; otherwise it becomes `fill` (default: the background).  keep_largest, min_size: int32
    [K] on the device.  Returns (cleaned labels, shaped as labels; kept uint8, same shape, 1 where the label was left as it was)."""
    _labels_i32(labels, "component_filter", "labels")
    if labels.dim() < 2:
        raise ValueError(f"component_filter: labels must be [B, *spatial], got {tuple(labels.shape)}")
    _check_classes("component_filter", K)
    B, M = _check_volumes("component_filter", labels)
    _check_root("component_filter", labels, root, B, M)
    _labels_i32(size, "component_filter", "size", 2)
    if tuple(size.shape) != (B, M) or size.device != labels.device:
        raise ValueError(f"component_filter: size must be int32 [{B}, {M}] on {labels.device}, got {tuple(size.shape)}")
    require_gpu(stats, "component_filter")
    if stats.dtype != torch.int64 or tuple(stats.shape) != (B, K, 4) or not stats.is_contiguous() or stats.device != labels.device:
        raise ValueError(f"component_filter: stats must be a contiguous int64 [{B}, {K}, 4] tensor on {labels.device}, "
                         f"got {stats.dtype} {tuple(stats.shape)}")
    for name, t in (("keep_largest", keep_largest), ("min_size", min_size)):
        _labels_i32(t, "component_filter", name, 1)
        if t.numel() != K or t.device != labels.device:
            raise ValueError(f"component_filter: {name} must hold K={K} int32 values on {labels.device}, got {tuple(t.shape)}")
    if not isinstance(background, int) or not -1 <= background < K:
        raise ValueError(f"component_filter: background {background} outside [-1, {K})")
    if fill is None:
        if background < 0:
            raise ValueError("component_filter: fill must be given when there is no background class")
        fill = background
    if not isinstance(fill, int) or not 0 <= fill < K:
        raise ValueError(f"component_filter: fill {fill} outside [0, {K})")
    out = torch.empty_like(labels)
    kept = torch.empty(labels.shape, dtype=torch.uint8, device=labels.device)
    call("gg_component_filter", labels.data_ptr(), root.data_ptr(), size.data_ptr(), stats.data_ptr(), B, M, K, keep_largest.data_ptr(),
         min_size.data_ptr(), background, fill, out.data_ptr(), kept.data_ptr(), _stream())
    return out, kept


# ------------------------------------------------------------------------------------- surface distances (gg_surface.hip)
EDT_MAX_EXTENT = 1024          # the line length gg_edt_squared's LDS tile is sized for (include/guidegen_hip.h)


def _check_border(what: str, labels: torch.Tensor, border: Optional[torch.Tensor]) -> None:
    if border is None:
        return
    require_gpu(border, what)
    if border.dtype != torch.uint8 or not border.is_contiguous() or border.numel() != labels.numel() or border.device != labels.device:
        raise ValueError(f"{what}: border must be a contiguous uint8 tensor of {labels.numel()} voxels on {labels.device}, "
                         f"got {border.dtype} {tuple(border.shape)}")


def _check_f64(what: str, name: str, t: torch.Tensor, numel: int, device) -> None:
    require_gpu(t, what)
    if t.dtype != torch.float64 or not t.is_contiguous() or t.numel() != numel or t.device != device:
        raise ValueError(f"{what}: {name} must be a contiguous float64 tensor of {numel} values on {device}, got {t.dtype} {tuple(t.shape)}")


def label_border(labels: torch.Tensor, K: int, connectivity: int = 1) -> torch.Tensor:
    """Class borders (gg_label_border): labels int32 [B, D, H, W] -> uint8 [B, D*H*W], 1 where the label lies in [0, K) and a neighbour
    under scipy's generate_binary_structure(3, connectivity) carries another label or lies outside the volume."""
    _labels_i32(labels, "label_border", "labels", 4)
    _check_classes("label_border", K)
    if connectivity not in (1, 2, 3):
        raise ValueError(f"label_border: connectivity {connectivity} is none of 1 (faces), 2 (and edges), 3 (and corners)")
    B, M = _check_volumes("label_border", labels)
    D, H, W = (int(v) for v in labels.shape[1:])
    border = torch.empty((B, M), dtype=torch.uint8, device=labels.device)
    call("gg_label_border", labels.data_ptr(), B, D, H, W, K, connectivity, border.data_ptr(), _stream())
    return border


def edt_squared(labels: torch.Tensor, border: Optional[torch.Tensor], cls: int, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Exact squared Euclidean distance transform (gg_edt_squared): labels int32 [B, D, H, W] -> fp64 [B, D*H*W], per voxel the smallest
    (sd dd)^2 + (sh dh)^2 + (sw dw)^2 to a site of its own volume (+inf where the volume has none).  A site carries class `cls` and, with
    `border` (uint8, label_border's), a non-zero border flag.  out / workspace: fp64 tensors of B*D*H*W values to reuse."""
    _labels_i32(labels, "edt_squared", "labels", 4)
    B, M = _check_volumes("edt_squared", labels)
    D, H, W = (int(v) for v in labels.shape[1:])
    if max(D, H, W) > EDT_MAX_EXTENT:
        raise ValueError(f"edt_squared: volume {D}x{H}x{W} has an extent above {EDT_MAX_EXTENT}, the longest line gg_edt_squared stages")
    if not isinstance(cls, int) or isinstance(cls, bool):
        raise ValueError(f"edt_squared: cls={cls!r} must be an integer class")
    _check_border("edt_squared", labels, border)
    import math
    sp = tuple(float(v) for v in spacing)
    if len(sp) != 3 or not all(math.isfinite(v) and v > 0.0 for v in sp):
        raise ValueError(f"edt_squared: spacing {tuple(spacing)} must be three finite values > 0 (d, h, w)")
    if out is None:
        out = torch.empty((B, M), dtype=torch.float64, device=labels.device)
    _check_f64("edt_squared", "out", out, B * M, labels.device)
    nbytes = int(_lib.load().gg_edt_squared_workspace_bytes(B, D, H, W))
    if workspace is None:
        workspace = torch.empty(nbytes // 8, dtype=torch.float64, device=labels.device)
    _check_f64("edt_squared", "workspace", workspace, nbytes // 8, labels.device)
    call("gg_edt_squared", labels.data_ptr(), _ptr(border), cls, B, D, H, W, sp[0], sp[1], sp[2], out.data_ptr(), workspace.data_ptr(), nbytes,
         _stream())
    return out


def surface_reduce(labels_a: torch.Tensor, border_a: Optional[torch.Tensor], sq_b: torch.Tensor, cls: int,
                   out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """gg_surface_reduce: over the voxels of class `cls` of labels_a (int32 [B, ...]) whose border flag is set, (dist2 fp64 [B, M]: sq_b
    there and -1 elsewhere; stats fp64 [B, 3]: their count, the sum of sqrt(sq_b), the maximum of sq_b).  Deterministic to the bit."""
    _labels_i32(labels_a, "surface_reduce", "labels")
    if labels_a.dim() < 2:
        raise ValueError(f"surface_reduce: labels must be [B, *spatial], got {tuple(labels_a.shape)}")
    B, M = _check_volumes("surface_reduce", labels_a)
    if not isinstance(cls, int) or isinstance(cls, bool):
        raise ValueError(f"surface_reduce: cls={cls!r} must be an integer class")
    _check_border("surface_reduce", labels_a, border_a)
    _check_f64("surface_reduce", "sq_b", sq_b, B * M, labels_a.device)
    if out is None:
        out = torch.empty((B, M), dtype=torch.float64, device=labels_a.device)
    _check_f64("surface_reduce", "out", out, B * M, labels_a.device)
    if out.data_ptr() == sq_b.data_ptr():
        raise ValueError("surface_reduce: out must not be sq_b's own memory")
    nbytes = int(_lib.load().gg_surface_reduce_workspace_bytes(B, M))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=labels_a.device)
    stats = torch.empty((B, 3), dtype=torch.float64, device=labels_a.device)
    call("gg_surface_reduce", labels_a.data_ptr(), _ptr(border_a), sq_b.data_ptr(), cls, B, M, out.data_ptr(), stats.data_ptr(), ws.data_ptr(),
         nbytes, _stream())
    return out, stats


# ----------------------------------------------------------------------------------------------- LPIPS (gg_lpips.hip)
def volume_views_cl(x: torch.Tensor, view: int, n0: int, n1: int, shift: torch.Tensor, scale: torch.Tensor, out: torch.Tensor) -> CL:
    """Images [n0, n1) of one axis view of an fp32 volume batch x [B, D, H, W] as channels-last rows (gg_volume_views_cl): view 0 =
    "(b d) 1 h w", 1 = "(b h) 1 d w", 2 = "(b w) 1 d h"; view 3 reads x as [B, 3, H, W] images.  Channels 0..2 = (x - shift_c) /
    scale_c, channels 3..31 zero.  out: contiguous [n1 - n0, 1, hh, ww, 32], bf16 or fp32; shift, scale: device fp32 with 3 values."""
    require_gpu(x, "volume_views_cl")
    if x.dtype != torch.float32 or x.dim() != 4 or not x.is_contiguous():
        raise ValueError(f"volume_views_cl: x must be a contiguous fp32 [B, D, H, W] tensor, got {x.dtype} {tuple(x.shape)}")
    B, D, H, W = (int(v) for v in x.shape)
    if view not in (0, 1, 2, 3) or (view == 3 and D != 3):
        raise ValueError(f"volume_views_cl: view {view} of a {tuple(x.shape)} tensor")
    hh, ww = ((H, W), (D, W), (D, H), (H, W))[view]
    for name, t in (("shift", shift), ("scale", scale)):
        if t.dtype != torch.float32 or t.numel() != 3 or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"volume_views_cl: {name} must be 3 contiguous fp32 values on {x.device}")
    if tuple(out.shape) != (n1 - n0, 1, hh, ww, 32) or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"volume_views_cl: out must be a contiguous {(n1 - n0, 1, hh, ww, 32)} tensor on {x.device}, got {tuple(out.shape)}")
    call("gg_volume_views_cl", x.data_ptr(), B, D, H, W, view, n0, n1, shift.data_ptr(), scale.data_ptr(), out.data_ptr(),
         _cl_dtype(out, "volume_views_cl"), _stream())
    return CL(out, 3)


def relu_cl(x: CL) -> CL:
    """In-place ReLU of a channels-last tensor (gg_relu_cl)."""
    require_gpu(x.t, "relu_cl")
    if not x.t.is_contiguous():
        raise ValueError("relu_cl: a contiguous channels-last tensor")
    call("gg_relu_cl", x.t.data_ptr(), _cl_dtype(x.t, "relu_cl"), x.t.numel(), _stream())
    return x


def lpips_tap(a: torch.Tensor, b: torch.Tensor, lin_w: torch.Tensor, pool: bool = True, tap_out: Optional[torch.Tensor] = None,
              total: Optional[torch.Tensor] = None, accumulate: bool = False):
    """One LPIPS tap (gg_lpips_tap).  a, b: channels-last [n, 1, h, w, C] pre-ReLU conv outputs of the two images (views of one tensor
    are fine as long as each is contiguous); lin_w fp32 [C].  Returns (per-image values fp32 [n], pooled): pooled is
    MaxPool2d(2, 2)(relu(.)) of both as ONE batch [2 n, 1, h // 2, w // 2, C] (a's images first: the next convolution's input), or None
    with pool=False.  total (fp32 [n]) receives the value too, added
    to what it holds with accumulate=True."""
    require_gpu(a, "lpips_tap")
    if a.shape != b.shape or a.dtype != b.dtype or a.dim() != 5 or a.shape[1] != 1 or not a.is_contiguous() or not b.is_contiguous():
        raise ValueError(f"lpips_tap: two contiguous channels-last [n, 1, h, w, C] tensors of one dtype, got {tuple(a.shape)} {a.dtype} and {tuple(b.shape)} {b.dtype}")
    n, _, h, w, Cc = (int(v) for v in a.shape)
    if lin_w.dtype != torch.float32 or lin_w.numel() != Cc or not lin_w.is_contiguous() or lin_w.device != a.device:
        raise ValueError(f"lpips_tap: lin_w must be {Cc} contiguous fp32 weights on {a.device}")
    lib = _lib.load()
    dt = _cl_dtype(a, "lpips_tap")
    wsb = lib.gg_lpips_tap_workspace_bytes(n, h, w, Cc, dt)
    check(min(wsb, 0), "gg_lpips_tap_workspace_bytes")
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=a.device)
    if tap_out is None:
        tap_out = torch.empty(n, dtype=torch.float32, device=a.device)
    for name, t in (("tap_out", tap_out), ("total", total)):
        if t is not None and (t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous() or t.device != a.device):
            raise ValueError(f"lpips_tap: {name} must be {n} contiguous fp32 values on {a.device}")
    pooled = torch.empty((2 * n, 1, h // 2, w // 2, Cc), dtype=a.dtype, device=a.device) if pool else None
    call("gg_lpips_tap", a.data_ptr(), b.data_ptr(), dt, n, h, w, Cc, lin_w.data_ptr(), _ptr(pooled[:n]) if pool else None,
         _ptr(pooled[n:]) if pool else None, tap_out.data_ptr(), _ptr(total), 1 if accumulate else 0, ws.data_ptr(), wsb, _stream())
    return tap_out, pooled


# ----------------------------------------------------------------------------------------------- rendering (gg_render.hip)
def make_grid_extent(B: int, H: int, W: int, nrow: int, padding: int) -> Tuple[int, int]:
    """(Hg, Wg) of torchvision's make_grid for B images of H x W: a single image is returned as it is, without padding."""
    if B == 1:
        return H, W
    xmaps = min(nrow, B)
    ymaps = -(-B // xmaps)
    return ymaps * (H + padding) + padding, xmaps * (W + padding) + padding


def mask_overlay(x: torch.Tensor, colors: Sequence[Sequence[int]], overlay_coef: float = 0.2, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """combine_mask_and_im of the reference on the device (gg_mask_overlay): x fp32 [N, 2, D, H, W] (CT, mask as label / 11) ->
    fp32 [N, D, 3, H, W], bit for bit.  colors: 12 rows of 3 integers.  The range of trunc(x[:, 1] * 11) is the caller's to check
    (render.combine_mask_and_im does); the kernel clamps the table index."""
    if x.dim() != 5 or x.shape[1] != 2 or x.dtype != torch.float32 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f"mask_overlay: x must be a contiguous non-empty fp32 [N, 2, D, H, W] tensor, got {x.dtype} {tuple(x.shape)}")
    table = [int(v) for row in colors for v in row]
    if len(table) != 36 or any(len(row) != 3 for row in colors):
        raise ValueError(f"mask_overlay: colors must be 12 rows of 3 integers, got {len(table)} values")
    require_gpu(x, "mask_overlay")
    N, _, D, H, W = (int(v) for v in x.shape)
    if out is None:
        out = torch.empty((N, D, 3, H, W), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (N, D, 3, H, W) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"mask_overlay: out must be a contiguous fp32 {(N, D, 3, H, W)} tensor on {x.device}, got {out.dtype} {tuple(out.shape)}")
    call("gg_mask_overlay", x.data_ptr(), N, D, H, W, float(overlay_coef), (C.c_int32 * 36)(*table), out.data_ptr(), _stream())
    return out


def make_grid_u8(imgs: torch.Tensor, nrow: int = 8, padding: int = 2, pad_value: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torchvision's make_grid + permute(1, 2, 0) + astype(uint8) on the device (gg_make_grid_u8): imgs fp32 [B, C, H, W], C 1 or 3 ->
    uint8 [Hg, Wg, 3].  The cast truncates toward zero and saturates to [0, 255]."""
    if imgs.dim() != 4 or imgs.shape[1] not in (1, 3) or imgs.dtype != torch.float32 or not imgs.is_contiguous() or imgs.numel() == 0:
        raise ValueError(f"make_grid_u8: imgs must be a contiguous non-empty fp32 [B, 1 or 3, H, W] tensor, got {imgs.dtype} {tuple(imgs.shape)}")
    if int(nrow) < 1 or int(padding) < 0:
        raise ValueError(f"make_grid_u8: nrow={nrow} padding={padding}")
    require_gpu(imgs, "make_grid_u8")
    B, Cc, H, W = (int(v) for v in imgs.shape)
    Hg, Wg = make_grid_extent(B, H, W, int(nrow), int(padding))
    if out is None:
        out = torch.empty((Hg, Wg, 3), dtype=torch.uint8, device=imgs.device)
    elif tuple(out.shape) != (Hg, Wg, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != imgs.device:
        raise ValueError(f"make_grid_u8: out must be a contiguous uint8 {(Hg, Wg, 3)} tensor on {imgs.device}, got {out.dtype} {tuple(out.shape)}")
    call("gg_make_grid_u8", imgs.data_ptr(), B, Cc, H, W, int(nrow), int(padding), float(pad_value), out.data_ptr(), _stream())
    return out


def minmax_normalise(src: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if out is None:
        out = torch.empty_like(src)
    ws = torch.empty(2, dtype=torch.float32, device=src.device)
    call("gg_minmax_normalise", src.data_ptr(), src.numel(), out.data_ptr(), ws.data_ptr(), _stream())
    return out


def mask_to_cond_slice(labels: torch.Tensor, slice_idx: int, D: int, H: int, W: int, prev: Optional[torch.Tensor],
                       cond: torch.Tensor, mask_out: Optional[torch.Tensor] = None) -> None:
    """labels int32 [N,Dm,Hm,Wm] -> cond bf16 CL [N,1,H,W,stride] (ch0 prev slice, ch1 mask/255)."""
    N, Dm, Hm, Wm = labels.shape
    call("gg_mask_to_cond_slice", labels.data_ptr(), N, Dm, Hm, Wm, slice_idx, D, H, W, _ptr(prev), cond.data_ptr(), cond.shape[-1], _ptr(mask_out),
         _stream())


def mask_to_cond_slices(labels: torch.Tensor, D: int, H: int, W: int, schedule: torch.Tensor, it: torch.Tensor, volume: torch.Tensor,
                        cond: torch.Tensor) -> None:
    """Batched glue of independent volumes: sample n's conditioning row from its own schedule row schedule[it[0], n] = (slice, prev,
    active) (device int32 [iterations, N, 3]; `it` device int32[1]); prev read from volume fp32 [D, N, H, W].  cond bf16 CL [N,1,H,W,stride]."""
    N, Dm, Hm, Wm = labels.shape
    _check_schedule(schedule, N, it)
    if tuple(volume.shape) != (D, N, H, W) or volume.dtype != torch.float32 or not volume.is_contiguous():
        raise ValueError(f"mask_to_cond_slices: volume must be contiguous fp32 {(D, N, H, W)}")
    call("gg_mask_to_cond_slices", labels.data_ptr(), N, Dm, Hm, Wm, D, H, W, schedule.data_ptr(), schedule.shape[0], it.data_ptr(),
         volume.data_ptr(), cond.data_ptr(), cond.shape[-1], _stream())


def minmax_normalise_scatter(src: torch.Tensor, schedule: torch.Tensor, it: torch.Tensor, volume: torch.Tensor, advance: bool = True,
                             workspace: Optional[torch.Tensor] = None) -> None:
    """src fp32 [N, ...]: each sample min-max normalised over its own values (bit-equal to minmax_normalise on that sample) and written
    to volume[slice_n, n] (volume fp32 [depth, N, ...]) where its row schedule[it[0], n] is active; advance: then it[0] += 1."""
    N = src.shape[0]
    _check_schedule(schedule, N, it)
    n_per = src.numel() // N
    if volume.dtype != torch.float32 or not volume.is_contiguous() or volume.shape[1] != N or volume[0, 0].numel() != n_per:
        raise ValueError(f"minmax_normalise_scatter: volume must be contiguous fp32 [depth, {N}, ...] of {n_per} values per slice")
    if workspace is None:
        workspace = torch.empty(2 * N, dtype=torch.float32, device=src.device)
    call("gg_minmax_normalise_scatter", src.data_ptr(), N, n_per, workspace.data_ptr(), schedule.data_ptr(), schedule.shape[0], it.data_ptr(),
         1 if advance else 0, volume.shape[0], volume.data_ptr(), _stream())


def _check_edit_volumes(who: str, known: torch.Tensor, keep: torch.Tensor, shape: Tuple[int, ...], device) -> None:
    if tuple(known.shape) != tuple(shape) or known.dtype != torch.float32 or not known.is_contiguous() or known.device != device:
        raise ValueError(f"{who}: known must be a contiguous fp32 {tuple(shape)} tensor on {device}, got {known.dtype} {tuple(known.shape)}")
    if tuple(keep.shape) != tuple(shape) or keep.dtype != torch.uint8 or not keep.is_contiguous() or keep.device != device:
        raise ValueError(f"{who}: keep must be a contiguous uint8 {tuple(shape)} tensor on {device}, got {keep.dtype} {tuple(keep.shape)}")


def ct_edit_glue(known: torch.Tensor, keep: torch.Tensor, schedule: torch.Tensor, it: torch.Tensor, margin: int, image: torch.Tensor,
                 latent_keep: torch.Tensor) -> None:
    """CT editing glue of independent volumes: known fp32 / keep uint8 [D, N, H, W]; sample n at its own slice schedule[it[0], n, 0] ->
    image bf16 CL [N,1,H,W,stride] (channel 0 the known slice, other lanes 0) and latent_keep fp32 [N*lat*lat, 1]: 1 iff every in-image
    pixel of the cell's window, grown by `margin` cells on each side, is kept.  Inactive rows: zero image, mask 0."""
    if known.dim() != 4:
        raise ValueError(f"ct_edit_glue: known must be [D, N, H, W], got {tuple(known.shape)}")
    D, N, H, W = (int(v) for v in known.shape)
    require_gpu(known, "ct_edit_glue")
    _check_edit_volumes("ct_edit_glue", known, keep, (D, N, H, W), known.device)
    _check_schedule(schedule, N, it)
    if image.dtype != torch.bfloat16 or not image.is_contiguous() or tuple(image.shape[:-1]) != (N, 1, H, W) or image.shape[-1] % 8:
        raise ValueError(f"ct_edit_glue: image must be a contiguous bf16 {(N, 1, H, W)} + (stride,) tensor, stride a multiple of 8, got "
                         f"{image.dtype} {tuple(image.shape)}")
    cells = latent_keep.numel() // N
    lat = int(round(cells ** 0.5))
    if latent_keep.dtype != torch.float32 or not latent_keep.is_contiguous() or lat * lat * N != latent_keep.numel() or lat < 1 or H % lat or H != W:
        raise ValueError(f"ct_edit_glue: latent_keep must be a contiguous fp32 tensor of {N} x lat x lat values with lat dividing H = W = {H}, "
                         f"got {latent_keep.dtype} {tuple(latent_keep.shape)}")
    if int(margin) < 0 or (H // lat) * (2 * int(margin) + 1) > H:
        raise ValueError(f"ct_edit_glue: margin = {margin}: the window of {(H // lat) * (2 * int(margin) + 1)} pixels must fit the {H} x {W} slice")
    call("gg_ct_edit_glue", known.data_ptr(), keep.data_ptr(), N, D, H, W, lat, int(margin), schedule.data_ptr(), schedule.shape[0], it.data_ptr(),
         image.data_ptr(), image.shape[-1], latent_keep.data_ptr(), _stream())


def minmax_normalise_keep_scatter(src: torch.Tensor, schedule: torch.Tensor, it: torch.Tensor, known: torch.Tensor, keep: torch.Tensor,
                                  volume: torch.Tensor, advance: bool = True, workspace: Optional[torch.Tensor] = None) -> None:
    """minmax_normalise_scatter with the pixel composite: known fp32 / keep uint8 of volume's shape [depth, N, ...]; of the active row's
    slice, kept pixels receive known bit for bit, the others the normalised value (bit-equal to minmax_normalise on that sample)."""
    N = src.shape[0]
    require_gpu(src, "minmax_normalise_keep_scatter")
    _check_schedule(schedule, N, it)
    n_per = src.numel() // N
    if src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("minmax_normalise_keep_scatter: src must be contiguous fp32")
    if volume.dtype != torch.float32 or not volume.is_contiguous() or volume.shape[1] != N or volume[0, 0].numel() != n_per:
        raise ValueError(f"minmax_normalise_keep_scatter: volume must be contiguous fp32 [depth, {N}, ...] of {n_per} values per slice")
    _check_edit_volumes("minmax_normalise_keep_scatter", known, keep, tuple(volume.shape), volume.device)
    if workspace is None:
        workspace = torch.empty(2 * N, dtype=torch.float32, device=src.device)
    call("gg_minmax_normalise_keep_scatter", src.data_ptr(), N, n_per, workspace.data_ptr(), schedule.data_ptr(), schedule.shape[0], it.data_ptr(),
         1 if advance else 0, volume.shape[0], known.data_ptr(), keep.data_ptr(), volume.data_ptr(), _stream())


def label_keep_volume(old_labels: torch.Tensor, new_labels: torch.Tensor, D: int, H: int, W: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 label volumes [N, Dm, Hm, Wm] -> keep uint8 [D, N, H, W]: 1 where the stage glue's zoomed, rotated label of new_labels equals
    that of old_labels (the index rule and rot90(k=3) of mask_to_cond_slice)."""
    require_gpu(old_labels, "label_keep_volume")
    for name, t in (("old_labels", old_labels), ("new_labels", new_labels)):
        if t.dim() != 4 or t.dtype != torch.int32 or not t.is_contiguous() or t.shape != old_labels.shape or t.device != old_labels.device:
            raise ValueError(f"label_keep_volume: {name} must be a contiguous int32 [N, Dm, Hm, Wm] tensor, both of one shape and device, got "
                             f"{t.dtype} {tuple(t.shape)}")
    N, Dm, Hm, Wm = (int(v) for v in old_labels.shape)
    if out is None:
        out = torch.empty((D, N, H, W), dtype=torch.uint8, device=old_labels.device)
    elif tuple(out.shape) != (D, N, H, W) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != old_labels.device:
        raise ValueError(f"label_keep_volume: out must be a contiguous uint8 {(D, N, H, W)} tensor on {old_labels.device}")
    call("gg_label_keep_volume", old_labels.data_ptr(), new_labels.data_ptr(), N, Dm, Hm, Wm, D, H, W, out.data_ptr(), _stream())
    return out


def _check_schedule(schedule: torch.Tensor, N: int, it: torch.Tensor) -> None:
    if schedule.dtype != torch.int32 or schedule.dim() != 3 or schedule.shape[1:] != (N, 3) or not schedule.is_contiguous():
        raise ValueError(f"schedule must be a contiguous int32 [iterations, {N}, 3] tensor")
    if it.dtype != torch.int32 or it.numel() != 1:
        raise ValueError("the iteration counter must be a device int32[1] tensor")


def zoom0_index(n_in: int, n_out: int) -> torch.Tensor:
    """Host-side index map of scipy.ndimage.zoom(order=0) along one axis (the rule gg_mask_to_cond_slice applies on the device):
    output o reads input floor(o * (n_in-1)/(n_out-1) + 0.5), IEEE double, product and sum rounded separately."""
    zf = (n_in - 1) / (n_out - 1) if n_out > 1 else 1.0
    o = torch.arange(n_out, dtype=torch.float64)
    return torch.clamp(torch.floor(o * zf + 0.5).long(), 0, n_in - 1)


def lincomb4(es, coefs, denom: float, out: torch.Tensor) -> torch.Tensor:
    """out = (sum_i coefs[i] * es[i]) / denom, fp32, left-to-right (PLMS multistep combination)."""
    es = list(es) + [None] * (4 - len(es))
    cs = list(coefs) + [0.0] * (4 - len(coefs))
    call("gg_lincomb4", es[0].data_ptr(), _ptr(es[1]), _ptr(es[2]), _ptr(es[3]), cs[0], cs[1], cs[2], cs[3], denom, out.numel(), out.data_ptr(),
         _stream())
    return out


def ddpm_step(x: torch.Tensor, eps: torch.Tensor, scalars: torch.Tensor, noise: Optional[torch.Tensor] = None,
              unet_in: Optional[torch.Tensor] = None) -> None:
    """Ancestral DDPM update in place; x fp32 CL [M, C], eps fp32 CL [M, stride], scalars fp32[5] on device."""
    Cc = x.shape[-1]
    M = x.numel() // Cc
    call("gg_ddpm_step", x.data_ptr(), eps.data_ptr(), eps.shape[-1], _ptr(noise), scalars.data_ptr(), M, Cc, _ptr(unet_in),
         unet_in.shape[-1] if unet_in is not None else 0, _stream())


DDPM_PREDICTS_X0, DDPM_CLIP = _lib.GG_DDPM_PREDICTS_X0, _lib.GG_DDPM_CLIP        # gg_ddpm_step_x0 flag bits


def ddpm_step_x0(x: torch.Tensor, out: torch.Tensor, scalars: torch.Tensor, noise: Optional[torch.Tensor] = None, *, predicts_x0: bool = False,
                 clip: bool = False, pred_x0_out: Optional[torch.Tensor] = None, unet_in: Optional[torch.Tensor] = None) -> None:
    """Ancestral update with the reference's options, in place (gg_ddpm_step_x0): x fp32 CL [M, C], out fp32 CL [M, stride] (the UNet's
    output: eps, or x_0 with predicts_x0), scalars fp32[5] on device as for ddpm_step; clip clamps the prediction of x_0 to [-1, 1];
    pred_x0_out fp32 [M, C] receives it."""
    Cc = x.shape[-1]
    M = x.numel() // Cc
    flags = (DDPM_PREDICTS_X0 if predicts_x0 else 0) | (DDPM_CLIP if clip else 0)
    call("gg_ddpm_step_x0", x.data_ptr(), out.data_ptr(), out.shape[-1], _ptr(noise), scalars.data_ptr(), flags, M, Cc, _ptr(pred_x0_out),
         _ptr(unet_in), unet_in.shape[-1] if unet_in is not None else 0, _stream())


def dpm_solver_step(x: torch.Tensor, out: torch.Tensor, scalars: torch.Tensor, hist: torch.Tensor, *, predicts_x0: bool = False,
                    clip: bool = False, pred_x0_out: Optional[torch.Tensor] = None, unet_in: Optional[torch.Tensor] = None) -> None:
    """One DPM-Solver++ (2M) reverse step in place (gg_dpm_solver_step): x fp32 CL [M, C], out fp32 CL [M, stride] (the UNet's output:
    eps, or x_0 with predicts_x0), scalars fp32[6] on device = (alpha_s, sigma_s, k_x, k_d, c0, c1), hist fp32 [M, C] the previous step's
    prediction of x_0 (read when c1 != 0 only; this step's is written to it); clip clamps the prediction to [-1, 1]; pred_x0_out fp32
    [M, C] receives it; unet_in channels [0, C) <- bf16(x)."""
    Cc = x.shape[-1]
    M = x.numel() // Cc
    for name, t in (("x", x), ("hist", hist), ("pred_x0_out", pred_x0_out)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != M * Cc):
            raise ValueError(f"dpm_solver_step: {name} must be contiguous fp32 [{M}, {Cc}], got {t.dtype} {tuple(t.shape)}")
    if scalars.dtype != torch.float32 or scalars.numel() < 6:
        raise ValueError(f"dpm_solver_step: scalars must hold six fp32 values, got {scalars.dtype} {tuple(scalars.shape)}")
    flags = (DDPM_PREDICTS_X0 if predicts_x0 else 0) | (DDPM_CLIP if clip else 0)
    call("gg_dpm_solver_step", x.data_ptr(), out.data_ptr(), out.shape[-1], scalars.data_ptr(), flags, M, Cc, hist.data_ptr(),
         _ptr(pred_x0_out), _ptr(unet_in), unet_in.shape[-1] if unet_in is not None else 0, _stream())


def log_rows(state: torch.Tensor, N: int, slot: torch.Tensor) -> None:
    """The fp32 channels-last state [N * S, C] -> slot fp32 [N, C, *sp] (prod(sp) = S), one entry of a pre-allocated log buffer
    (gg_log_rows: from_cl's kernel at a given destination; no allocation, capturable)."""
    Cc = state.shape[-1]
    S = state.numel() // (Cc * N) if N else 0
    if state.dtype != torch.float32 or slot.dtype != torch.float32 or not state.is_contiguous() or not slot.is_contiguous() \
            or slot.numel() != state.numel() or state.numel() != N * S * Cc or (slot.ndim >= 2 and tuple(slot.shape[:2]) != (N, Cc)):
        raise ValueError(f"log_rows: state {tuple(state.shape)} {state.dtype} does not fill a slot {tuple(slot.shape)} {slot.dtype} as "
                         f"[{N}, {Cc}, S]")
    call("gg_log_rows", state.data_ptr(), N, Cc, S, slot.data_ptr(), _stream())


# ----------------------------------------------------------------------------------------------- held-out objectives (gg_loss.hip)
LOSS_MODES = {"l2": _lib.GG_LOSS_L2, "l1": _lib.GG_LOSS_L1, "prior_kl": _lib.GG_LOSS_PRIOR_KL}        # gg_loss_mode


def _f32_dev(t: torch.Tensor, numel: int, what: str) -> torch.Tensor:
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() != numel:
        raise ValueError(f"{what} must be a contiguous device fp32 tensor of {numel} elements, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def _i32_dev(t: torch.Tensor, numel: int, what: str) -> torch.Tensor:
    if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or t.numel() != numel:
        raise ValueError(f"{what} must be a contiguous device int32 tensor of {numel} elements, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def loss_workspace(N: int, rows_per_sample: int, device) -> torch.Tensor:
    """The workspace either reduction of gg_loss.hip needs for N samples of rows_per_sample rows."""
    nbytes = int(_lib.load().gg_loss_workspace_bytes(N, rows_per_sample))
    return torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=device)


def q_sample_rows(x: torch.Tensor, noise: torch.Tensor, scalars: torch.Tensor, out: Optional[torch.Tensor] = None,
                  unet_in: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """x_noisy[n] = s0[n] * x[n] + s1[n] * noise[n] (gg_q_sample_rows): x, noise fp32 NC(D)HW on the device, scalars fp32 [N, 2].
    out: fp32 NC(D)HW; unet_in: channels-last [N, ..., Cpad] bf16 (or fp32 in validation mode), channels [0, C) written."""
    require_gpu(x, "q_sample_rows")
    N, Cc = int(x.shape[0]), int(x.shape[1])
    S = x.numel() // (N * Cc)
    _f32_dev(x, N * Cc * S, "q_sample_rows: x"); _f32_dev(noise, N * Cc * S, "q_sample_rows: noise"); _f32_dev(scalars, 2 * N, "q_sample_rows: scalars")
    if out is None and unet_in is None:
        out = torch.empty_like(x)
    if out is not None:
        _f32_dev(out, N * Cc * S, "q_sample_rows: out")
    dt, stride = GG_BF16, 0
    if unet_in is not None:
        stride = int(unet_in.shape[-1])
        if unet_in.dtype not in (torch.bfloat16, torch.float32) or not unet_in.is_contiguous() or unet_in.numel() != N * S * stride or stride < Cc:
            raise ValueError(f"q_sample_rows: unet_in {unet_in.dtype} {tuple(unet_in.shape)} is not a channels-last buffer of {N * S} rows, >= {Cc} lanes")
        dt = GG_F32 if is_f32(unet_in) else GG_BF16
    call("gg_q_sample_rows", x.data_ptr(), noise.data_ptr(), scalars.data_ptr(), N, Cc, S, _ptr(out), _ptr(unet_in), dt, stride, _stream())
    return out


def loss_rows(mode: str, N: int, C: int, S: int, *, pred: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None,
              x_start: Optional[torch.Tensor] = None, scalars: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
              workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-sample means, fp64 [N] (gg_loss_rows).  "l2" / "l1": pred fp32 channels-last [N * S, stride] (the UNet head's output) against
    target fp32 NC(D)HW; "prior_kl": x_start fp32 NC(D)HW and scalars fp32 [N, 2] = (sqrt_alphas_cumprod[T-1], log_one_minus_alphas_cumprod[T-1])."""
    if mode not in LOSS_MODES:
        raise ValueError(f"loss_rows: unknown mode '{mode}' (one of {sorted(LOSS_MODES)})")
    stride = 0
    if mode == "prior_kl":
        _f32_dev(x_start, N * C * S, "loss_rows: x_start"); _f32_dev(scalars, 2 * N, "loss_rows: scalars")
        dev = x_start.device
    else:
        stride = int(pred.shape[-1])
        _f32_dev(pred, N * S * stride, "loss_rows: pred"); _f32_dev(target, N * C * S, "loss_rows: target")
        dev = pred.device
    if out is None:
        out = torch.empty(N, dtype=torch.float64, device=dev)
    if workspace is None:
        workspace = loss_workspace(N, S, dev)
    call("gg_loss_rows", _ptr(pred), stride, _ptr(target), _ptr(x_start), _ptr(scalars), LOSS_MODES[mode], N, C, S, out.data_ptr(),
         workspace.data_ptr(), workspace.numel() * 8, _stream())
    return out


def ccdm_q_sample(x0: torch.Tensor, mix: torch.Tensor, K: int, *, E: Optional[torch.Tensor] = None,
                  philox_seeds: Optional[torch.Tensor] = None, philox_offset: Optional[torch.Tensor] = None,
                  labels_out: Optional[torch.Tensor] = None, onehot_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q_xt_given_x0(x0, t).sample() on labels (gg_ccdm_q_sample): x0 int32 [M] of N equal samples, mix fp32 [N, 2] = (keep, unif), the
    weights of the one-hot and of the uniform part: (cumalphas[t - 1], 1 - cumalphas[t - 1]), or (1 - betas[t - 1], betas[t - 1]).
    E: fp32 [M, K] exponential tape, or philox_seeds: device int64 [N] keys.  Returns int32 [M]."""
    require_gpu(x0, "ccdm_q_sample")
    M, N = x0.numel(), mix.numel() // 2
    rps = _rows_per_sample(M, N, "ccdm_q_sample")
    _i32_dev(x0, M, "ccdm_q_sample: x0"); _f32_dev(mix, 2 * N, "ccdm_q_sample: mix")
    if (E is None) == (philox_seeds is None):
        raise ValueError("ccdm_q_sample: give either an exponential tape E or philox_seeds")
    if E is not None:
        _f32_dev(E, M * K, "ccdm_q_sample: E")
    if labels_out is None:
        labels_out = torch.empty(M, dtype=torch.int32, device=x0.device)
    _i32_dev(labels_out, M, "ccdm_q_sample: labels_out")
    oh_stride = _onehot_stride(onehot_out, M, "ccdm_q_sample")
    call("gg_ccdm_q_sample", x0.data_ptr(), mix.data_ptr(), rps, K, _ptr(E), _seeds_ptr(philox_seeds, N) if philox_seeds is not None else None,
         _ptr(philox_offset), M, labels_out.data_ptr(), _ptr(onehot_out), oh_stride, _stream())
    return labels_out


PHILOX_POSTERIOR, PHILOX_KNOWN, PHILOX_RENOISE = 0, 1, 2      # `purpose` of a CCDM chain draw (philox_offset_word)


def philox_offset_word(t: int, j: int = 0, purpose: int = PHILOX_POSTERIOR) -> int:
    """The 32-bit Philox offset word of a CCDM chain draw: t | (j << 16) | (purpose << 28), with t the 1-based timestep (< 2^16), j the
    resampling repetition (< 256) and purpose 0 the posterior draw, 1 the known-region noising, 2 the resample re-noise.  At j = 0,
    purpose 0 it is t, the offset of a chain without a mask."""
    if not 0 <= int(t) < (1 << 16):
        raise ValueError(f"philox_offset_word: t={t} does not fit the 16 bits of the offset word (time_steps must be < 65536)")
    if not 0 <= int(j) < 256:
        raise ValueError(f"philox_offset_word: repetition j={j} outside 0..255 (resample must be <= 256)")
    if purpose not in (PHILOX_POSTERIOR, PHILOX_KNOWN, PHILOX_RENOISE):
        raise ValueError(f"philox_offset_word: purpose={purpose} is none of 0 (posterior), 1 (known), 2 (re-noise)")
    return int(t) | (int(j) << 16) | (int(purpose) << 28)


def ccdm_inpaint_blend(labels: torch.Tensor, known: torch.Tensor, keep: torch.Tensor, mix: torch.Tensor, K: int, *,
                       E: Optional[torch.Tensor] = None, philox_seed: int = 0, philox_seeds: Optional[torch.Tensor] = None,
                       philox_offset: Optional[torch.Tensor] = None, onehot_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Mask editing of the CCDM chain state (gg_ccdm_inpaint_blend): labels int32 [M] of N equal samples, in place; rows with keep != 0
    (uint8 [M]) take a draw of q(x_t | x_0 = known) with mix fp32 [N, 2] = (cumalphas[t - 1], 1 - cumalphas[t - 1]), every other row is
    left as it is.  known int32 [M] may be `labels` itself.  E: fp32 [M, K] exponential tape; otherwise Philox with philox_seeds (device
    int64 [N], one key per sample) or the single key philox_seed, at philox_offset (device int64 [1]).  onehot_out: bf16 rows
    [M, stride], channels [0, K) of the kept rows written.  Returns labels."""
    require_gpu(labels, "ccdm_inpaint_blend")
    M, N = labels.numel(), mix.numel() // 2
    rps = _rows_per_sample(M, N, "ccdm_inpaint_blend")
    _i32_dev(labels, M, "ccdm_inpaint_blend: labels"); _i32_dev(known, M, "ccdm_inpaint_blend: known"); _f32_dev(mix, 2 * N, "ccdm_inpaint_blend: mix")
    if keep.dtype != torch.uint8 or not keep.is_cuda or not keep.is_contiguous() or keep.numel() != M:
        raise ValueError(f"ccdm_inpaint_blend: keep must be a contiguous device uint8 tensor of {M} elements, got {keep.dtype} {tuple(keep.shape)} on {keep.device}")
    if E is not None:
        _f32_dev(E, M * K, "ccdm_inpaint_blend: E")
    oh_stride = _onehot_stride(onehot_out, M, "ccdm_inpaint_blend")
    call("gg_ccdm_inpaint_blend", labels.data_ptr(), known.data_ptr(), keep.data_ptr(), mix.data_ptr(), rps, K, _ptr(E),
         int(philox_seed) & ((1 << 64) - 1), _seeds_ptr(philox_seeds, N) if philox_seeds is not None else None, _ptr(philox_offset), M,
         _ptr(onehot_out), oh_stride, _stream())
    return labels


def ccdm_step_loss(logits: torch.Tensor, xt: torch.Tensor, x0: torch.Tensor, scalars: torch.Tensor, class_weights: torch.Tensor, K: int, *,
                   out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp64 [N, 2] per-sample sums of (class-weighted KL, CE) of trainer.py:305-320 (gg_ccdm_step_loss): logits fp32 channels-last
    [M, stride], xt / x0 int32 [M], scalars fp32 [N, 2] per sample, class_weights fp32 [K]."""
    require_gpu(logits, "ccdm_step_loss")
    stride = int(logits.shape[-1])
    M = logits.numel() // stride
    N = scalars.numel() // 2
    rps = _rows_per_sample(M, N, "ccdm_step_loss")
    _f32_dev(logits, M * stride, "ccdm_step_loss: logits"); _i32_dev(xt, M, "ccdm_step_loss: xt"); _i32_dev(x0, M, "ccdm_step_loss: x0")
    _f32_dev(scalars, 2 * N, "ccdm_step_loss: scalars"); _f32_dev(class_weights, K, "ccdm_step_loss: class_weights")
    if out is None:
        out = torch.empty((N, 2), dtype=torch.float64, device=logits.device)
    if workspace is None:
        workspace = loss_workspace(N, rps, logits.device)
    call("gg_ccdm_step_loss", logits.data_ptr(), stride, xt.data_ptr(), x0.data_ptr(), scalars.data_ptr(), rps, class_weights.data_ptr(), K, M,
         out.data_ptr(), workspace.data_ptr(), workspace.numel() * 8, _stream())
    return out


# ----------------------------------------------------------------------------------------------- first-stage objective (gg_patchgan.hip)
def patch_conv_out_extent(in_sp: Sequence[int], kd: int, stride: int) -> Tuple[int, int, int]:
    """Output extent of a kernel-4, padding-2 convolution over (D, H, W); kd == 1: 2-D, D is carried through."""
    D, H, W = in_sp
    return (D if kd == 1 else D // stride + 1, H // stride + 1, W // stride + 1)


def patch_conv(src: CL, weight: torch.Tensor, alpha: Optional[torch.Tensor], beta: torch.Tensor, cout: int, kd: int, stride: int,
               slope: float = 0.2, out_f32: bool = False) -> CL:
    """One PatchGAN convolution (gg_patch_conv_forward, or the fp32 kernel for fp32 inputs): kernel 4, padding 2, then
    y = acc * alpha + beta and LeakyReLU(slope) (slope 1: none).  weight: pack_conv_weight of the OI[D]HW weight; alpha (or None) and
    beta: fp32 [pad32(cout)], the folded conv bias and eval-mode BatchNorm."""
    require_gpu(src.t, "patch_conv")
    N, D, H, W, cin = src.t.shape
    Do, Ho, Wo = patch_conv_out_extent((D, H, W), kd, stride)
    cp = pad32(cout)
    for name, t in (("alpha", alpha), ("beta", beta)):
        if t is not None:
            _f32_dev(t, cp, f"patch_conv: {name}")
    if is_f32(src.t):
        if weight.dtype != torch.float32 or tuple(weight.shape) != (16 * kd, cin, cp):
            raise ValueError(f"patch_conv: fp32 input needs an fp32 weight [{16 * kd}, {cin}, {cp}], got {weight.dtype} {tuple(weight.shape)}")
        out = torch.empty((N, Do, Ho, Wo, cp), dtype=torch.float32, device=src.t.device)
        call("gg_patch_conv_forward_f32", src.t.data_ptr(), weight.data_ptr(), _ptr(alpha), beta.data_ptr(), slope, N, D, H, W, cin, cout, kd,
             stride, Do, Ho, Wo, out.data_ptr(), _stream())
        return CL(out, cout)
    if src.t.dtype != torch.bfloat16 or weight.dtype != torch.bfloat16 or weight.numel() != cp * 16 * kd * cin:
        raise ValueError(f"patch_conv: bf16 input needs a packed bf16 weight of {cp * 16 * kd * cin} elements, got {src.t.dtype} input, "
                         f"{weight.dtype} weight of {weight.numel()}")
    out = torch.empty((N, Do, Ho, Wo, cp), dtype=torch.float32 if out_f32 else torch.bfloat16, device=src.t.device)
    call("gg_patch_conv_forward", src.t.data_ptr(), weight.data_ptr(), _ptr(alpha), beta.data_ptr(), slope, N, D, H, W, cin, cout, kd, stride, Do,
         Ho, Wo, out.data_ptr(), GG_F32 if out_f32 else GG_BF16, _stream())
    return CL(out, cout)


def _moment_rows(moments: torch.Tensor, C: int, what: str) -> Tuple[int, int]:
    stride = int(moments.shape[-1])
    require_gpu(moments, what)
    if moments.dtype != torch.float32 or not moments.is_contiguous() or stride < 2 * C:
        raise ValueError(f"{what}: moments must be contiguous fp32 channels-last rows of >= {2 * C} lanes, got {moments.dtype} {tuple(moments.shape)}")
    N = int(moments.shape[0])
    return N, moments.numel() // (N * stride)


def gauss_kl_rows(moments: torch.Tensor, C: int, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp64 [N] = DiagonalGaussianDistribution.kl() (gg_gauss_kl_rows) of fp32 channels-last moments [N, ..., stride]: mean lanes [0, C),
    logvar lanes [C, 2C)."""
    N, S = _moment_rows(moments, C, "gauss_kl_rows")
    if out is None:
        out = torch.empty(N, dtype=torch.float64, device=moments.device)
    if workspace is None:
        workspace = loss_workspace(N, S, moments.device)
    call("gg_gauss_kl_rows", moments.data_ptr(), int(moments.shape[-1]), N, C, S, out.data_ptr(), workspace.data_ptr(), workspace.numel() * 8,
         _stream())
    return out


def gauss_sample_rows(moments: torch.Tensor, C: int, noise: torch.Tensor, out: Optional[torch.Tensor] = None,
                      z_in: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """z = mean + exp(0.5 * logvar) * noise (gg_gauss_sample_rows): moments as in gauss_kl_rows, noise fp32 [N, C, *spatial].
    out: fp32 like noise; z_in: channels-last [N, ..., Cpad] bf16 (or fp32 in validation mode), channels [0, C) written."""
    N, S = _moment_rows(moments, C, "gauss_sample_rows")
    _f32_dev(noise, N * C * S, "gauss_sample_rows: noise")
    if out is None and z_in is None:
        out = torch.empty_like(noise)
    if out is not None:
        _f32_dev(out, N * C * S, "gauss_sample_rows: out")
    dt, stride = GG_BF16, 0
    if z_in is not None:
        stride = int(z_in.shape[-1])
        if z_in.dtype not in (torch.bfloat16, torch.float32) or not z_in.is_cuda or not z_in.is_contiguous() or z_in.numel() != N * S * stride or stride < C:
            raise ValueError(f"gauss_sample_rows: z_in {z_in.dtype} {tuple(z_in.shape)} is not a channels-last device buffer of {N * S} rows, >= {C} lanes")
        dt = GG_F32 if is_f32(z_in) else GG_BF16
    call("gg_gauss_sample_rows", moments.data_ptr(), int(moments.shape[-1]), noise.data_ptr(), N, C, S, _ptr(out), _ptr(z_in), dt, stride, _stream())
    return out


def logit_stats(logits: torch.Tensor, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp64 [5] = means over all logits l of (l, relu(1 - l), relu(1 + l), softplus(-l), softplus(l)) (gg_logit_stats); logits: lane 0
    of fp32 channels-last rows [..., stride] (a discriminator's last convolution with out_f32)."""
    require_gpu(logits, "logit_stats")
    stride = int(logits.shape[-1])
    M = logits.numel() // stride
    _f32_dev(logits, M * stride, "logit_stats: logits")
    if out is None:
        out = torch.empty(5, dtype=torch.float64, device=logits.device)
    if workspace is None:
        workspace = loss_workspace(3, M, logits.device)
    call("gg_logit_stats", logits.data_ptr(), stride, M, out.data_ptr(), workspace.data_ptr(), workspace.numel() * 8, _stream())
    return out
