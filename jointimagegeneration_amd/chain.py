"""The latent chain's state and what is done to it, written once for the DDIM, PLMS, DPM-Solver (ldm.py, dpm_solver.py) and ancestral
(GaussianDiffusion._ancestral_loop) samplers.

The state is a dict of static channels-last buffers of one chain shape: fp32 `x` and `pred_x0` [N, *sp3, Cx], the bf16 UNet input
`unet_in` [N, *sp3, pad32(Cx + Cc)] with the concat conditioning in channels [Cx, Cx + Cc), the fp32 `eps` the UNet's head writes, the
cross-attention context `ctx`, the per-step tables `table` (time biases) and `scal` (the update's scalars), and by request the patch-wise
evaluator `split`, the inpainting operands `ip_*` and the log buffers `log*`.  The functions below build it, load a call's inputs into
it and make the launches every sampler makes on it.  They take what they need as arguments and decide nothing about caching, graphs or
schedules: those are the samplers'."""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import torch

from . import ops
from .ops import CL, pad32


def nc_to_rows(t: torch.Tensor) -> torch.Tensor:
    """[N, C, *sp] -> [N, *sp, C], the channels-last view (a permutation, no copy)."""
    return t.permute((0,) + tuple(range(2, t.ndim)) + (1,))


def rows_to_nc(t: torch.Tensor) -> torch.Tensor:
    """[N, *sp, C] -> [N, C, *sp], the inverse view."""
    return t.permute((0, t.ndim - 1) + tuple(range(1, t.ndim - 1)))


def split_cond(conditioning, conditioning_key):
    """-> (c_concat, context) of a conditioning: a dict as the reference's apply_model takes it (c_concat's first entry, c_crossattn
    concatenated), or a bare tensor read by the model's conditioning key."""
    c_concat, context = None, None
    if conditioning is not None:
        if isinstance(conditioning, dict):
            c_concat = conditioning.get("c_concat", [None])[0]
            cc = conditioning.get("c_crossattn")
            context = torch.cat(cc, 1) if cc else None
        elif conditioning_key == "concat":
            c_concat = conditioning
        elif conditioning_key == "crossattn":
            context = conditioning
    return c_concat, context


def logged_steps(n: int, log_every_t: int) -> List[int]:
    """The loop values at which the reference's samplers append to their intermediates, in loop order (n - 1 down to 0): the timestep i
    of p_sample_loop / progressive_denoising (ddpm.py:1172,1220), the index of DDIM / PLMS (ddim.py:160, plms.py:166)."""
    k = int(log_every_t)
    if k < 1:
        raise ValueError(f"log_every_t = {log_every_t} must be a positive integer")
    return [i for i in range(n - 1, -1, -1) if i % k == 0 or i == n - 1]


def inpaint_operands(mask, x0, shape, tape=None, steps=0):
    """Host-side validation of the inpainting operands of the samplers (ddim.py:144-148, plms.py:147-150, ddpm.py:1201-1218), run
    before any launch.  Returns None without a mask (x0 alone is ignored, as in the reference); else (x0 fp32 [N, C, *sp],
    mask fp32 [N, Cm, *sp], Cm) as broadcast views, Cm = the mask's channel extent (1 or C).  Bool / integer masks are cast to fp32.
    `tape` (optional): at least `steps` q_sample noises of shape [N, C, *sp].  Anything else raises ValueError naming the shapes."""
    if mask is None:
        return None
    if x0 is None:
        raise ValueError("inpainting: mask= was given without x0= (the latent whose mask = 1 region is kept)")
    if not isinstance(mask, torch.Tensor) or not isinstance(x0, torch.Tensor):
        raise ValueError(f"inpainting: mask and x0 must be tensors, got {type(mask).__name__} and {type(x0).__name__}")
    full = tuple(int(s) for s in shape)
    N, C = full[:2]

    def fits(t):
        try:
            return tuple(torch.broadcast_shapes(tuple(t.shape), full)) == full
        except RuntimeError:
            return False
    if x0.is_complex() or not fits(x0):
        raise ValueError(f"inpainting: x0 of shape {tuple(x0.shape)} ({x0.dtype}) does not broadcast to the latent shape {full}")
    if mask.is_complex() or not fits(mask):
        raise ValueError(f"inpainting: mask of shape {tuple(mask.shape)} ({mask.dtype}) does not broadcast to the latent shape {full}")
    ch = mask.ndim - (len(full) - 1)                  # the mask's channel axis once right-aligned against [N, C, *sp]
    Cm = int(mask.shape[ch]) if ch >= 0 else 1
    m = mask.float().reshape((1,) * (len(full) - mask.ndim) + tuple(mask.shape)).expand((N, Cm) + full[2:])
    if tape is not None:
        if len(tape) < steps:
            raise ValueError(f"inpainting: mask_noise_tape holds {len(tape)} tensors, the schedule has {steps} steps")
        for i in range(steps):
            if tuple(tape[i].shape) != full:
                raise ValueError(f"inpainting: mask_noise_tape[{i}] has shape {tuple(tape[i].shape)}, the latent is {full}")
    return x0.float().expand(full), m, Cm


# ================================================================================================ the UNet on the state
class SplitUNet:
    """The UNet evaluated on overlapping crops (apply_model with split_input_params, ddpm.py:915-997): per call one gg_unfold_cl of the
    fp32 state into the crop batch's UNet input (fp32 -> bf16, channels [0, Cx)), ONE UNet forward at batch L * N (crop l of sample n at
    row l * N + n; every layer is per sample, so this is the reference's loop over crops), one gg_fold_weighted_cl of the head conv's
    fp32 output into the full-size eps.  Concat conditioning is cut into crops once per `bind`, cross-attention context is repeated per
    crop.  All buffers are static, so a chain of calls is capturable."""

    def __init__(self, model, N: int, Cx: int, Cc: int, sp: Sequence[int], device):
        if len(sp) != 2:
            raise NotImplementedError(f"split_input_params: the patch-wise path is 2-D, the latent has spatial shape {tuple(sp)}")
        par = model.split_input_params
        self.plan = model.get_fold_unfold((N, Cx) + tuple(sp), par["ks"], par["stride"])
        self.N, self.Cx, self.Cc, self.device = N, Cx, Cc, device
        self.B = self.plan.L * N
        unet = model.model.diffusion_model
        p = self.plan
        self.eps = torch.empty((self.B, 1, p.kh, p.kw, pad32(unet.out_channels)), dtype=torch.float32, device=device)
        self.inputs: Dict[int, Any] = {}
        self.contexts: Dict[int, Any] = {}

    def bind(self, uin: torch.Tensor, ctx: Optional[CL] = None):
        """(Re)cut the concat conditioning held in channels [Cx, Cx + Cc) of the full-size UNet input `uin` into the crop batch's input
        buffer, and repeat the context per crop.  Outside any graph; the buffers keep their addresses.  One crop buffer is kept per
        distinct `uin` (and one repeated context per distinct `ctx`) for as long as this object lives, so a caller that keeps the
        SplitUNet binds static buffers of its own, never per-call temporaries."""
        p = self.plan
        ent = self.inputs.get(id(uin))
        if ent is None or ent[0] is not uin:
            ent = (uin, torch.zeros((self.B, 1, p.kh, p.kw, uin.shape[-1]), dtype=uin.dtype, device=uin.device))
            self.inputs[id(uin)] = ent
        if self.Cc:
            src = uin.view(self.N, p.H, p.W, uin.shape[-1])[..., self.Cx:self.Cx + self.Cc]
            ops.unfold_cl(src, self.Cc, p.kh, p.kw, p.sy, p.sx, out=ent[1].view(self.B, p.kh, p.kw, -1), c_offset=self.Cx)
        if ctx is not None:
            c = self.contexts.get(id(ctx.t))
            if c is None or c[0] is not ctx.t:
                c = (ctx.t, CL(ctx.t.repeat((p.L,) + (1,) * (ctx.t.dim() - 1)), ctx.C))
                self.contexts[id(ctx.t)] = c
            else:
                c[1].t.copy_(ctx.t.repeat((p.L,) + (1,) * (ctx.t.dim() - 1)))

    def __call__(self, unet, x: torch.Tensor, uin: torch.Tensor, bias_row: torch.Tensor, ctx: Optional[CL], out: torch.Tensor) -> None:
        p = self.plan
        buf = self.inputs[id(uin)][1]
        ops.unfold_cl(x.view(self.N, p.H, p.W, self.Cx), self.Cx, p.kh, p.kw, p.sy, p.sx, out=buf.view(self.B, p.kh, p.kw, -1), c_offset=0)
        unet.forward_cl(CL(buf, self.Cx + self.Cc), bias_row, self.contexts[id(ctx.t)][1] if ctx is not None else None, head_out=self.eps)
        w, t = p.on(self.eps.device)
        ops.fold_weighted_cl(self.eps.view(self.B, p.kh, p.kw, -1), unet.out_channels, w, t, out.view(self.N, p.H, p.W, -1),
                             p.kh, p.kw, p.sy, p.sx)


def unet_eps(st, unet, uin: torch.Tensor, bias_row: torch.Tensor, ctx: Optional[CL], out: torch.Tensor, head_ddim: Optional[tuple] = None) -> Optional[CL]:
    """The one place where the samplers obtain eps: the UNet on the full-size input `uin` (returns the head conv's CL, whose epilogue may
    have applied the DDIM update), or on a "split" state on crops of its fp32 x, folded into `out` (returns None: no fused update)."""
    if "split" not in st:
        return unet.forward_cl(CL(uin, st["Cx"] + st["Cc"]), bias_row, ctx, head_out=out, head_ddim=head_ddim)
    st["split"](unet, st["x"], uin, bias_row, ctx, out)
    return None


# ================================================================================================ the state
LOG_BUFFERS = {"x": "log_x", "pred_x0": "log_p0"}


def new_state(model, N, Cx, Cc, sp, dev, scal, *, ctx_shape=None, inpaint=None, logged=None, log_of=("x", "pred_x0")) -> dict:
    """The static buffers of one chain shape on `model` (its UNet's widths; its split_input_params make the state a patch-wise one).
    scal: the fp32 [S, k] table whose row i step i's update reads.  ctx_shape = (L, C): a cross-attention context [N, L, C] as a static
    channels-last buffer [N, 1, 1, L, pad32(C)], which a captured chain reads in place.  inpaint = (mask_C, ip_scal, n_noise): fp32
    buffers for x0 and a mask of mask_C channels, the [S, 2] q_sample scalar table and, with n_noise > 0, n_noise q_sample noises drawn
    or loaded ahead of the chain.  logged (step indices, `logged_steps`): "log" maps a sampling step to its slot, each of `log_of` gets
    an fp32 log buffer [L, N, Cx, *sp] ("log_x" / "log_p0") that `gg_log_rows` fills in place.  "table": `set_bias_table`."""
    unet = model.model.diffusion_model
    sp = tuple(sp)
    sp3 = (1,) * (3 - len(sp)) + sp
    f32, bf16 = torch.float32, torch.bfloat16
    S = int(scal.shape[0])
    st = dict(N=N, Cx=Cx, Cc=Cc, sp=sp, sp3=sp3, S=S, scal=scal, table=None,
              x=torch.empty((N,) + sp3 + (Cx,), dtype=f32, device=dev), pred_x0=torch.empty((N,) + sp3 + (Cx,), dtype=f32, device=dev),
              unet_in=torch.zeros((N,) + sp3 + (pad32(Cx + Cc),), dtype=bf16, device=dev),
              eps=torch.empty((N,) + sp3 + (pad32(unet.out_channels),), dtype=f32, device=dev),
              ctx=CL(torch.zeros((N, 1, 1, ctx_shape[0], pad32(ctx_shape[1])), dtype=bf16, device=dev), ctx_shape[1]) if ctx_shape is not None else None)
    if getattr(model, "split_input_params", None) is not None:          # patch-wise eps: crop buffers, time-bias rows for L * N
        st["split"] = SplitUNet(model, N, Cx, Cc, sp, dev)
    if inpaint is not None:
        mask_C, ip_scal, n_noise = inpaint
        st.update(ip_x0=torch.empty((N,) + sp3 + (Cx,), dtype=f32, device=dev), ip_mask=torch.empty((N,) + sp3 + (mask_C,), dtype=f32, device=dev),
                  ip_scal=ip_scal)
        if n_noise:
            st["ip_noise"] = torch.empty((n_noise, N) + sp3 + (Cx,), dtype=f32, device=dev)
    if logged is not None:
        st["log"] = {S - 1 - index: j for j, index in enumerate(logged)}
        for name in log_of:
            st[LOG_BUFFERS[name]] = torch.empty((len(logged), N, Cx) + sp, dtype=f32, device=dev)
    return st


def set_bias_table(st, unet, steps: torch.Tensor) -> None:
    """"table": the UNet's time biases of the fp32 timesteps `steps`, one row per sampling step.  The rows of a step are equal for all
    samples, so a "split" state's are repeated per crop."""
    st["table"] = unet.time_bias_table(steps, st["split"].B if "split" in st else st["N"])


def load(st, x_T: torch.Tensor, c_concat: Optional[torch.Tensor], context: Optional[torch.Tensor] = None) -> None:
    """x_T (NC..) -> fp32 CL state + bf16 UNet input; conditioning latent -> channels [Cx, Cx+Cc) of the UNet input; context
    [N, L, C] -> the state's channels-last context buffer."""
    if context is not None:
        ops.to_cl(context.permute(0, 2, 1).contiguous().float(), out=st["ctx"].t, c_offset=0, zero_fill=False)
    st["x"].view((st["N"],) + tuple(x_T.shape[2:]) + (st["Cx"],)).copy_(nc_to_rows(x_T))          # plumbing: layout copy
    ops.to_cl(x_T, out=st["unet_in"], c_offset=0, zero_fill=False)
    if c_concat is not None:
        ops.to_cl(c_concat.float(), out=st["unet_in"], c_offset=st["Cx"], zero_fill=False)
    if "split" in st:
        st["split"].bind(st["unet_in"], st["ctx"] if context is not None else None)


def load_inpaint(st, x0: torch.Tensor, mask: torch.Tensor, mask_noise_tape=None) -> None:
    """x0 [N, C, *sp] and mask [N, Cm, *sp] (inpaint_operands' views) -> the state's static CL buffers; on a state with "ip_noise" its
    q_sample noises from the tape, or from one device randn [S, N, C, *sp].  Outside any graph: a captured chain reads the buffers in
    place."""
    N, Cx = st["N"], st["Cx"]
    dev = st["x"].device
    sp = tuple(x0.shape[2:])
    st["ip_x0"].view((N,) + sp + (Cx,)).copy_(nc_to_rows(x0.to(dev)))              # plumbing: layout copies
    st["ip_mask"].view((N,) + sp + (mask.shape[1],)).copy_(nc_to_rows(mask.to(dev)))
    if "ip_noise" not in st:
        return
    S = st["ip_noise"].shape[0]
    noise = st["ip_noise"].view((S, N) + sp + (Cx,))
    if mask_noise_tape is not None:
        for i in range(S):
            noise[i].copy_(nc_to_rows(mask_noise_tape[i].to(dev).float()))
    else:
        noise.copy_(torch.randn((S, N, Cx) + sp, device=dev).permute((0, 1) + tuple(range(3, len(sp) + 3)) + (2,)))


def rows(st, *buffers):
    """The [M, width] row views the step kernels take, M = N * prod(sp): of state buffers by name, or of channels-last tensors of the
    state's extent (a combined eps, a step's noise).  One view for one argument, else a tuple."""
    M = st["x"].numel() // st["Cx"]
    views = tuple((st[b] if isinstance(b, str) else b).view(M, -1) for b in buffers)
    return views[0] if len(views) == 1 else views


def to_nc(st, name: str) -> torch.Tensor:
    """A state buffer as a fresh [N, C, *sp] tensor."""
    return rows_to_nc(st[name].view((st["N"],) + st["sp"] + (st["Cx"],))).contiguous()


# ================================================================================================ the launches on the state
def blend(st, i, noise=None) -> None:
    """The inpainting blend at step i's timestep (ddim.py:144-148, ddpm.py:1201-1218): x and the UNet input's channels [0, Cx) <-
    q_sample(x0, t_i) * mask + (1 - mask) * x, the q_sample noise being `noise` (channels-last) or the state's pre-drawn one.  No-op (no
    launch) on a mask-free state."""
    if "ip_x0" not in st:
        return
    x, x0, mask, nz, uin = rows(st, "x", "ip_x0", "ip_mask", st["ip_noise"][i] if noise is None else noise, "unet_in")
    ops.inpaint_blend(x, x0, mask, nz, st["ip_scal"][i], unet_in=uin)


def after_step(st, i) -> None:
    """What follows sampling step i: on a logging state the `gg_log_rows` copies into its slot, for every log buffer the state holds
    (launches like any other, so they are captured with the chain); on a state with "callbacks" (callback, img_callback), as the
    DDIM-family samplers set them, callback(i) and img_callback(pred_x0, i) (ddim.py:157-158)."""
    j = st["log"].get(i) if "log" in st else None
    if j is not None:
        for name, buf in LOG_BUFFERS.items():
            if buf in st:
                ops.log_rows(rows(st, name), st["N"], st[buf][j])
    cb = st.get("callbacks")
    if cb is not None:
        if cb[0]:
            cb[0](i)
        if cb[1]:
            p0 = torch.empty((st["N"], st["Cx"]) + st["sp"], dtype=torch.float32, device=st["x"].device)
            ops.log_rows(rows(st, "pred_x0"), st["N"], p0)
            cb[1](p0, i)


def step_noise(st, i, noise_tape, draw: bool, p: float = 0.0, scale: Optional[float] = None):
    """Step i's noise as a channels-last tensor: the tape's [N, C, *sp] tensor, else with `draw` a fresh device randn, else None (a
    deterministic step).  scale multiplies it (the ancestral loop's temperature, ddpm.py:1109), then noise_dropout p (ddim.py:202-203,
    ddpm.py:1110-1111) acts on it, both on the noise as given and only when set."""
    if noise_tape is None and not draw:
        return None
    nz = noise_tape[i].to(st["x"].device).float() if noise_tape is not None else torch.randn_like(st["x"])
    if scale is not None:
        nz = nz * scale
    if p > 0.0:
        nz = torch.nn.functional.dropout(nz, p=p)
    return nc_to_rows(nz).contiguous() if noise_tape is not None else nz
