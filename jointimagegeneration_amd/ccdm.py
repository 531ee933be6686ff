"""CCDM volumetric mask sampler on the HIP engine.

Mirrors (names, signatures, buffers) ccdm/ddpm/models/diffusion_denoising.py:18-227, builder.py:14-53 and the
input conventions of ccdm/ddpm/evaluator.py:127-170.  The reverse chain keeps its state as int32 labels on the
device; one denoising step = UNet forward (channels-last bf16, MFMA) + ONE fused per-voxel kernel
(softmax -> theta_post_prob -> clamp -> renormalise -> exponential-race sample -> one-hot write-back), and the
fixed-shape step is captured in a hipGraph (torch.cuda.CUDAGraph) and replayed with per-step tables.
"""
from __future__ import annotations

import itertools
import math
from typing import Any, Dict, List, Optional, Sequence, Tuple, cast

import numpy as np
import torch
from torch import Tensor, nn

from . import ops
from .chain import nc_to_rows, rows_to_nc
from .ops import CL, pad32
from .unet import create_unet_openai

__all__ = ["DiffusionModel", "DenoisingModel", "build_model", "linear_schedule", "cosine_schedule", "uniform_x_T"]


def linear_schedule(time_steps: int, start=1e-2, end=0.2):
    betas = torch.linspace(start, end, time_steps)
    alphas = 1 - betas
    return betas, alphas, torch.cumprod(alphas, dim=0)


def cosine_schedule(time_steps: int, s: float = 8e-3):
    """Reproduces the reference values bit-for-bit, quirks included (diffusion_denoising.py:25-39):
    `s` is overridden to 0.008, cumalphas is sampled at t=0..T-1 (not a cumprod), betas are capped at 0.999."""
    s = 0.008
    t = torch.arange(0, time_steps)
    cumalphas = torch.cos(((t / time_steps + s) / (1 + s)) * (math.pi / 2)) ** 2
    f = lambda u: math.cos((u + s) / (1.0 + s) * math.pi / 2) ** 2
    betas = torch.tensor([min(1 - f((i + 1) / time_steps) / f(i / time_steps), 0.999) for i in range(time_steps)])
    return betas, 1 - betas, cumalphas


def uniform_x_T(K: int, size: Sequence[int], seeds: Sequence[int], device) -> Tensor:
    """One uniform categorical x_T (evaluator.py:135-136) per seed, each from its own generator: int32 labels [len(seeds), *size]."""
    return torch.cat([torch.randint(0, K, (1,) + tuple(size), generator=torch.Generator(device=device).manual_seed(int(s)), device=device,
                                    dtype=torch.int32) for s in seeds])


class CategoricalBCHW:
    """What q_xt_given_x0 / q_xt_given_xtm1 return (the reference's OneHotCategoricalBCHW, one_hot_categorical.py): the distribution
    keep[b] * x + unif[b] / K around a one-hot x (mix [B, 2] = (keep, unif)).  `.probs` is channels-last [B, *sp, K], normalised as torch's Categorical does
    (torch plumbing); `.sample` is one `gg_ccdm_q_sample` launch on the labels of x."""

    def __init__(self, x: Tensor, mix: Tensor, K: int):
        self.x, self.mix, self.K = x, mix, K

    @property
    def probs(self) -> Tensor:
        nd = self.x.ndim
        k, u = (self.mix[:, i].view((-1,) + (1,) * (nd - 1)) for i in (0, 1))
        p = nc_to_rows(k * self.x + u / self.K)
        return p / p.sum(-1, keepdim=True)

    def sample_labels(self, rng_tape: Optional[Tensor] = None, philox_seeds: Optional[Sequence[int]] = None) -> Tensor:
        """int32 labels [B, *sp].  rng_tape: fp32 [M, K] exponentials (channels-last voxel order); otherwise Philox, one key per sample
        (philox_seeds, default 1024 + b)."""
        x = self.x
        lab = x.argmax(dim=1).to(torch.int32).contiguous()
        if rng_tape is not None:
            out = ops.ccdm_q_sample(lab.view(-1), self.mix, self.K, E=rng_tape.to(x.device).float().contiguous())
        else:
            keys = philox_seeds if philox_seeds is not None else [1024 + b for b in range(x.shape[0])]
            out = ops.ccdm_q_sample(lab.view(-1), self.mix, self.K, philox_seeds=ops.philox_seed_tensor(keys, x.device))
        return out.view(lab.shape)

    def sample(self, rng_tape: Optional[Tensor] = None, philox_seeds: Optional[Sequence[int]] = None) -> Tensor:
        """One-hot NC[D]HW sample in x's dtype (index scatter of the kernel's labels: plumbing)."""
        return rows_to_nc(torch.nn.functional.one_hot(self.sample_labels(rng_tape, philox_seeds).long(), self.K)).to(self.x.dtype)


class DiffusionModel(nn.Module):
    """Schedule buffers `betas/alphas/cumalphas` (diffusion_denoising.py:42-71)."""
    betas: Tensor
    alphas: Tensor
    cumalphas: Tensor

    def __init__(self, schedule: str, time_steps: int, num_classes: int, schedule_params=None, dims=3):
        super().__init__()
        fn = {"linear": linear_schedule, "cosine": cosine_schedule}[schedule]
        betas, alphas, cumalphas = fn(time_steps, **schedule_params) if schedule_params is not None else fn(time_steps)
        self.dims = dims
        self.register_buffer("betas", betas)
        self.register_buffer("alphas", alphas)
        self.register_buffer("cumalphas", cumalphas)
        self.num_classes = num_classes

    @property
    def time_steps(self):
        return len(self.betas)

    def step_scalars(self, t_values: Sequence[int]) -> Tensor:
        """fp32 [S, 2] = (alphas[t-1], cumalphas[t-2]) with the t==1 overrides (a=0, abar=1) of
        theta_post_prob (diffusion_denoising.py:114-122)."""
        al, ca = self.alphas.detach().cpu(), self.cumalphas.detach().cpu()
        rows = [(0.0, 1.0) if t == 1 else (float(al[t - 1]), float(ca[t - 2])) for t in t_values]
        return torch.tensor(rows, dtype=torch.float32)

    def step_scalar_rows(self, t: Tensor) -> Tensor:
        """Per-sample form of `step_scalars`: 1-based t [B] -> fp32 [B, 2] on the schedule's device (index arithmetic only)."""
        t = t.to(self.alphas.device).long()
        if int(t.min()) < 1 or int(t.max()) > self.time_steps:
            raise ValueError(f"t = {t.tolist()} outside 1..{self.time_steps}")
        one = t == 1
        a = torch.where(one, torch.zeros_like(self.alphas[t - 1]), self.alphas[t - 1])
        abar = torch.where(one, torch.ones_like(a), self.cumalphas[(t - 2).clamp(min=0)])
        return torch.stack([a, abar], 1).float().contiguous()

    def known_mix(self, t_values: Sequence[int]) -> Tensor:
        """fp32 [S, 2] = (cumalphas[t-1], 1 - cumalphas[t-1]): the operands of q(x_t | x_0) as `q_xt_given_x0` forms them, one row per step."""
        ca = self.cumalphas[torch.tensor(list(t_values), dtype=torch.long, device=self.cumalphas.device) - 1]
        return torch.stack([ca, 1 - ca], 1).float().contiguous()

    def renoise_mix(self, t_values: Sequence[int]) -> Tensor:
        """fp32 [S, 2] = (1 - betas[t-1], betas[t-1]): the operands of q(x_t | x_{t-1}) as `q_xt_given_xtm1` forms them, one row per step."""
        betas = self.betas[torch.tensor(list(t_values), dtype=torch.long, device=self.betas.device) - 1]
        return torch.stack([1 - betas, betas], 1).float().contiguous()

    def _mix_rows(self, keep: Tensor, unif: Tensor, x: Tensor, who: str) -> "CategoricalBCHW":
        ops.require_gpu(x, who)
        if x.shape[1] != self.num_classes:
            raise ValueError(f"{who}: {x.shape[1]} channels for {self.num_classes} classes")
        return CategoricalBCHW(x, torch.stack([keep, unif], 1).to(x.device).float().contiguous(), self.num_classes)

    def q_xt_given_xtm1(self, xtm1: Tensor, t: Tensor) -> "CategoricalBCHW":
        """q(x_t | x_{t-1}) (diffusion_denoising.py:73-80): one-hot xtm1 NC[D]HW, 1-based t [B]."""
        betas = self.betas[t.to(self.betas.device).long() - 1]
        return self._mix_rows(1 - betas, betas, xtm1, "q_xt_given_xtm1")

    def q_xt_given_x0(self, x0: Tensor, t: Tensor) -> "CategoricalBCHW":
        """q(x_t | x_0) (diffusion_denoising.py:82-89): one-hot x0 NC[D]HW, 1-based t [B]."""
        ca = self.cumalphas[t.to(self.cumalphas.device).long() - 1]
        return self._mix_rows(ca, 1 - ca, x0, "q_xt_given_x0")

    def theta_post(self, xt: Tensor, x0: Tensor, t: Tensor) -> Tensor:
        """q(x_{t-1} | x_t, x_0) for one-hot xt, x0 (diffusion_denoising.py:91-103), evaluated by the posterior kernel with the one-hot x0
        in the place of the predicted distribution: the sum over the predicted x_0 then has one non-zero term.  As theta_post_prob's, the
        values have passed that kernel's clamp (>= 1e-12) and normalisation, so the exact zeros of t == 1 come out as 1e-12."""
        return self.theta_post_prob(xt, x0.float(), t)

    def theta_post_prob(self, xt: Tensor, theta_x0: Tensor, t: Tensor) -> Tensor:
        """Reference signature (NC[D]HW one-hot xt, probs theta_x0, 1-based t [B]); evaluated by the fused HIP kernel
        (one launch per distinct t). Returns the UN-clamped-equivalent normalised posterior (values >= 1e-12)."""
        ops.require_gpu(xt, "theta_post_prob")
        K = self.num_classes
        out = torch.empty_like(nc_to_rows(theta_x0).contiguous())
        for b in range(xt.shape[0]):
            sc = self.step_scalars([int(t[b])]).to(xt.device)[0]
            p0 = nc_to_rows(theta_x0[b:b + 1]).contiguous().float()
            lab = xt[b:b + 1].argmax(dim=1).to(torch.int32).contiguous().view(-1)
            M = lab.numel()
            ops.ccdm_posterior_sample(p0.view(M, K), False, lab, sc, K, draw=False, probs_out=out[b].view(M, K))
        return rows_to_nc(out)


class LabelChain:
    """The state of one `DenoisingModel.sample_labels` call and the launches made on it: the UNet input `xin` (channels-last; channels
    [0, K) the one-hot of the int32 labels `lab` [M], then the condition), the head's `logits`, the posterior `probs` [M, K], the per-step
    tables `table`, `scal`, `kmix`, `rmix`, and the `cur_*` buffers, from which a captured step reads its rows and its Philox offset
    words in place.  `ladder` holds the step graph of `ops.replay_captured`: it lives, as all of this does, for one call."""

    def __init__(self, model: "DenoisingModel", labels: Tensor, condition: Optional[Tensor], tv: Sequence[int],
                 seeds: Optional[Sequence[int]], known_f: Optional[Tensor], keep_f: Optional[Tensor], resample: int):
        dev, unet, diffusion = labels.device, model.unet, model.diffusion
        self.model, self.K, self.M = model, diffusion.num_classes, labels.numel()
        self.masked, self.edit, self.bf16 = known_f is not None, known_f is not None or resample > 1, not ops.FP32
        K, M, N = self.K, self.M, labels.shape[0]
        sp3 = (1,) * (4 - labels.ndim) + tuple(labels.shape[1:])
        self.scal = diffusion.step_scalars(tv).to(dev)
        self.table = unet.time_bias_table(torch.tensor(tv, dtype=torch.float32, device=dev), N)
        self.xin = torch.zeros((N,) + sp3 + (pad32(unet.in_channels),), dtype=torch.bfloat16 if self.bf16 else torch.float32, device=dev)
        self.lab = labels.contiguous().view(-1).clone()
        ops.labels_to_onehot(self.lab, K, self.xin.view(M, -1))       # channels [0,K) one-hot, rest zero
        if condition is not None:                                     # unet.py:774-775: cat([x, input_condition], 1)
            ops.to_cl(condition.to(dev), out=self.xin, c_offset=K, zero_fill=False)
        self.logits = torch.empty((N,) + sp3 + (pad32(K),), dtype=torch.float32, device=dev)
        self.probs = torch.empty((M, K), dtype=torch.float32, device=dev)
        self.cur_bias = torch.empty_like(self.table[0])
        self.cur_scal = torch.empty(2, dtype=torch.float32, device=dev)
        self.cur_off = torch.zeros(1, dtype=torch.int64, device=dev)
        self.xcl = CL(self.xin, unet.in_channels)
        self.seeds = None if seeds is None else ops.philox_seed_tensor(seeds, dev)
        if self.masked:
            self.known, self.keep = known_f.to(dev), keep_f.to(dev)
            self.kmix = diffusion.known_mix(tv).to(dev)
            self.cur_kmix = torch.empty((N, 2), dtype=torch.float32, device=dev)
            self.cur_koff = torch.zeros(1, dtype=torch.int64, device=dev)
        self.rmix = None
        if resample > 1:
            self.rmix = diffusion.renoise_mix(tv).to(dev)
            self.cur_rmix = torch.empty((N, 2), dtype=torch.float32, device=dev)
            self.cur_roff = torch.zeros(1, dtype=torch.int64, device=dev)
            self.rkeys = self.keys()
        self.ladder = dict(warmed=False, graph=None)

    def keys(self) -> Tensor:
        """gg_ccdm_q_sample draws per sample; the single-key stream (key philox_seed, counter = the row of the batch) is its one-sample case."""
        return self.seeds if self.seeds is not None else ops.philox_seed_tensor([self.model.philox_seed], self.lab.device)

    def onehot_out(self, final: bool = False) -> Optional[Tensor]:
        """The launch that changes the labels refreshes the UNet's one-hot input in bf16; `refresh_onehot` does in fp32 validation mode."""
        return self.xin.view(self.M, -1) if (self.bf16 and not final) else None

    def refresh_onehot(self, final: bool = False) -> None:
        if not (self.bf16 or final):                                           # fp32 validation mode: an index scatter
            ops.labels_to_onehot(self.lab, self.K, self.xin.view(self.M, -1))

    def set_step(self, i: int, t: int, j: int) -> None:
        if j == 0:
            self.cur_bias.copy_(self.table[i]); self.cur_scal.copy_(self.scal[i])
            if self.masked:
                self.cur_kmix.copy_(self.kmix[i])
            if self.rmix is not None:
                self.cur_rmix.copy_(self.rmix[i])
        self.t, self.j = t, j                                         # `renoise` fills its own word, immediately before its launch
        self.cur_off.fill_(ops.philox_offset_word(t, j, ops.PHILOX_POSTERIOR) if self.edit else t)
        if self.masked:
            self.cur_koff.fill_(ops.philox_offset_word(t, j, ops.PHILOX_KNOWN))

    def step(self, draw: bool, E=None, want_probs: bool = False) -> None:
        m = self.model
        post = dict(xt=self.lab, scalars=self.cur_scal, K=self.K, E=E, philox_seed=m.philox_seed, philox_offset=self.cur_off, draw=draw,
                    labels_out=self.lab, onehot_out=self.onehot_out(), philox_seeds=self.seeds)
        # softmax + posterior + draw as the head conv's epilogue where the kernel can (ops.conv `post`): the fp32 logits (128 B per
        # voxel) are then never written; steps that return the posterior itself (the last one, traces) take the sampler kernel
        head = m.unet.forward_cl(self.xcl, self.cur_bias, head_out=self.logits, head_post=post if (self.bf16 and not want_probs) else None)
        m.last_step_fused = head.fused_post
        if not head.fused_post:
            ops.ccdm_posterior_sample(self.logits.view(self.M, -1), True, probs_out=self.probs if want_probs else None, **post)
            self.refresh_onehot()

    def blend(self, E=None, final: bool = False) -> None:
        """x_t <- a draw of q(x_t | x_0 = known) where keep != 0, into the labels and the one-hot UNet input (operands (1, 0): known itself)."""
        ops.ccdm_inpaint_blend(self.lab, self.known, self.keep, self.cur_kmix, self.K, E=E, philox_seed=self.model.philox_seed,
                               philox_seeds=self.seeds, philox_offset=self.cur_koff, onehot_out=self.onehot_out(final))
        self.refresh_onehot(final)

    def renoise(self, E=None) -> None:
        """x_t <- a draw of q(x_t | x_{t-1}) on every voxel, in place."""
        self.cur_roff.fill_(ops.philox_offset_word(self.t, self.j, ops.PHILOX_RENOISE))
        mix = self.cur_rmix if (self.seeds is not None or E is not None) else self.cur_rmix[:1]
        ops.ccdm_q_sample(self.lab, mix, self.K, E=E, philox_seeds=None if E is not None else self.rkeys, philox_offset=self.cur_roff,
                          labels_out=self.lab, onehot_out=self.onehot_out())
        self.refresh_onehot()

    def graphed_step(self) -> None:                                   # what `ops.replay_captured` captures
        if self.masked:
            self.blend()
        self.step(True)


class DenoisingModel(nn.Module):
    """`forward(x, condition, ...)` in eval mode runs the whole reverse chain (diffusion_denoising.py:142-227)."""

    def __init__(self, diffusion: DiffusionModel, unet: nn.Module, dataset_file: str, step_T_sample: str = "majority", dims=3):
        super().__init__()
        self.diffusion, self.unet, self.dims = diffusion, unet, dims
        self.dataset_file, self.step_T_sample = dataset_file, step_T_sample
        self.philox_seed = 1024           # RNG of the throughput path (counter-based, in-kernel)
        self.use_graph = True
        self.last_step_fused = False      # whether the last eager step ran as the head conv's epilogue

    @property
    def time_steps(self):
        return self.diffusion.time_steps

    def forward(self, x: Tensor, condition: Tensor, feature_condition: Tensor = None, t: Optional[Tensor] = None,
                label_ref_logits: Optional[Tensor] = None, validation: bool = False, context=None, rng_tapes=None,
                known: Optional[Tensor] = None, keep: Optional[Tensor] = None, resample: int = 1) -> dict:
        if self.training:
            raise RuntimeError("this engine implements sampling only (training is out of scope, SURVEY.md 2.1 row 5)")
        if validation:
            return self.forward_step(x, condition, feature_condition, t, context=context)
        init_t = None if t is None else cast(int, int(t.item()))
        return self.forward_denoising(x, condition, feature_condition, init_t, label_ref_logits, context=context, rng_tapes=rng_tapes,
                                      known=known, keep=keep, resample=resample)

    def forward_step(self, x, condition, feature_condition, t, context=None):
        return self.unet(x, condition, feature_condition=feature_condition, timesteps=t, context=context)

    # -------------------------------------------------------------------------------------------------
    def t_values(self, init_t: Optional[int]) -> List[int]:
        T = self.time_steps
        if init_t is None:
            init_t = T
        if init_t > 10000:                      # "t = 10000+K" sub-sampling (diffusion_denoising.py:190-197)
            K = init_t % 10000
            assert 0 < K <= T
            return list(range(K, 0, -1)) if K == T else [round(v) for v in np.linspace(T, 1, K)]
        return list(range(init_t, 0, -1))

    @torch.no_grad()
    def forward_denoising(self, x: Tensor, condition: Tensor, feature_condition: Tensor = None, init_t: Optional[int] = None,
                          label_ref_logits: Optional[Tensor] = None, context: Tensor = None, rng_tapes=None,
                          known: Optional[Tensor] = None, keep: Optional[Tensor] = None, resample: int = 1) -> dict:
        if label_ref_logits is not None:
            raise NotImplementedError("label_ref_logits guidance is dead code in the reference (undefined guidance_fn)")
        if feature_condition is not None:
            raise NotImplementedError("feature_condition is always None on the shipped path (evaluator.py:169)")
        ops.require_gpu(x, "DenoisingModel.forward_denoising")
        labels = x.argmax(dim=1).to(torch.int32).contiguous()                   # x_T one-hot -> labels (plumbing)
        lab, probs = self.sample_labels(labels, condition, init_t, rng_tapes, known=known, keep=keep, resample=resample)
        K = self.diffusion.num_classes
        if self.step_T_sample is None or self.step_T_sample == "majority":
            out = rows_to_nc(torch.nn.functional.one_hot(lab.long(), K))        # int64 one-hot like max_prob_sample
        elif self.step_T_sample == "confidence":
            out = rows_to_nc(probs.view(*lab.shape, K))
        else:
            raise ValueError(f"step_T_sample={self.step_T_sample}")
        return {"diffusion_out": out}

    def check_edit(self, shape, known: Optional[Tensor], keep: Optional[Tensor], resample: int = 1):
        """The refusals of mask editing, each by name; returns (known int32 [M], keep uint8 [M]) or (None, None) without a mask.  The
        label range is checked where the labels are (one readback for a device tensor)."""
        if isinstance(resample, bool) or not isinstance(resample, int) or resample < 1:
            raise ValueError(f"sample_labels: resample={resample!r} must be an integer >= 1")
        if resample > 256:
            raise ValueError(f"sample_labels: resample={resample} exceeds 256, the repetitions the Philox offset word can number")
        if (known is None) != (keep is None):
            raise ValueError(f"sample_labels: {'keep' if known is None else 'known'} given without {'known' if known is None else 'keep'}; "
                             "mask editing needs both")
        if (known is not None or resample > 1) and self.time_steps >= (1 << 16):
            raise ValueError(f"sample_labels: time_steps={self.time_steps} >= 65536 does not fit the 16 bits the Philox offset word gives t")
        K = self.diffusion.num_classes
        if resample > 1 and K > 16:
            raise NotImplementedError(f"sample_labels: resample > 1 re-noises with gg_ccdm_q_sample, which takes K <= 16 (K = {K})")
        if known is None:
            return None, None
        for name, v in (("known", known), ("keep", keep)):
            if tuple(v.shape) != tuple(shape):
                raise ValueError(f"sample_labels: {name} has shape {tuple(v.shape)}, the labels {tuple(shape)}")
        if known.dtype.is_floating_point or known.dtype == torch.bool:
            raise ValueError(f"sample_labels: known must hold integer labels, got {known.dtype}")
        if keep.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"sample_labels: keep must be bool or uint8, got {keep.dtype}")
        lo, hi = torch.stack([known.min(), known.max()]).tolist()
        if lo < 0 or hi > K - 1:
            raise ValueError(f"sample_labels: known holds labels {lo}..{hi} outside 0..{K - 1}")
        return known.to(torch.int32).contiguous().view(-1), (keep != 0).to(torch.uint8).contiguous().view(-1)

    @torch.no_grad()
    def sample_labels(self, labels: Tensor, condition: Optional[Tensor], init_t: Optional[int] = None, rng_tapes=None,
                      trace: Optional[list] = None, philox_seeds: Optional[Sequence[int]] = None, known: Optional[Tensor] = None,
                      keep: Optional[Tensor] = None, resample: int = 1) -> Tuple[Tensor, Tensor]:
        """labels int32 [N, (D,) H, W] on the GPU -> (final labels int32, final normalised posterior fp32 [M, K]).
        philox_seeds (N keys): sample n draws with its own Philox key and its own voxel index as the counter, so that its chain does not
        depend on its batch slot or its neighbours (independent volumes in one batch); None: `self.philox_seed` over the whole batch.
        known / keep (mask editing): integer labels in 0..K-1 and a bool / uint8 mask, both of labels' shape.  At the top of
        every step the voxels with keep != 0 are replaced by a draw of q(x_t | x_0 = known) (one `gg_ccdm_inpaint_blend` launch in front
        of the UNet), and after the last step they hold known exactly.  resample R: every step runs R times, re-noised one step with
        q(x_t | x_{t-1}) in between (RePaint's resampling, jump length 1).  The Philox offset word is `ops.philox_offset_word(t, j, purpose)`.
        rng_tapes: per (t, j) the blend tape (with a mask), the posterior tape (t > 1), the re-noise tape (j < R - 1), in that order.
        trace entries: t, j, labels, probs and, with a mask, x_in (the labels after the blend, the UNet's input)."""
        known_f, keep_f = self.check_edit(labels.shape, known, keep, resample)
        if philox_seeds is not None and len(philox_seeds) != labels.shape[0]:
            raise ValueError(f"sample_labels: {len(philox_seeds)} philox_seeds for a batch of {labels.shape[0]}")
        tv = self.t_values(init_t)
        S = len(tv)
        st = LabelChain(self, labels, condition, tv, philox_seeds, known_f, keep_f, resample)
        if rng_tapes is not None:
            # per (t, j): the blend tape with a mask, the posterior tape of a DRAWING step (t = 1 takes the argmax), the re-noise tape
            need = sum(resample * (int(st.masked) + int(t > 1)) + (resample - 1) for t in tv)
            if len(rng_tapes) < need:
                what = f"{need} drawing steps (t = {tv[0]} .. 2)" if not st.edit else \
                    f"{S} steps (t = {tv[0]} .. {tv[-1]}) x {resample} repetitions{' with a mask' if st.masked else ''}"
                raise ValueError(f"sample_labels: {what} need {need} rng tapes, got {len(rng_tapes)}")
        tapes = itertools.repeat(None) if rng_tapes is None else (tp.to(labels.device).contiguous() for tp in rng_tapes)   # read in draw order
        use_graph = self.use_graph and rng_tapes is None and trace is None and S > 3 and not ops.FP32
        for i, t in enumerate(tv):
            for j in range(resample):
                st.set_step(i, t, j)
                last, draw = (i == S - 1 and j == resample - 1), (t > 1)
                if use_graph and draw and not last:
                    ops.replay_captured(st.ladder, "graph", st.graphed_step)   # the fixed-shape step: eager once, captured once (hipGraph)
                else:
                    if st.masked:
                        st.blend(next(tapes))
                        x_in = st.lab.clone().view(labels.shape) if trace is not None else None
                    st.step(draw, next(tapes) if draw else None, want_probs=last or trace is not None)
                if trace is not None:
                    entry = dict(t=t, j=j, labels=st.lab.clone().view(labels.shape), probs=st.probs.clone())
                    if st.masked:
                        entry["x_in"] = x_in
                    trace.append(entry)
                if j < resample - 1:                                 # between two repetitions, outside the captured step
                    st.renoise(next(tapes))
        if st.masked:
            # the labels are discrete and kept anatomy must come back unchanged: one more blend with operands (1, 0), whose race has one
            # non-zero class, and the returned posterior rows of the kept voxels are the one-hot of known (an index select: plumbing)
            st.cur_kmix.copy_(torch.tensor([1.0, 0.0], dtype=torch.float32, device=labels.device))
            st.blend(final=True)
            st.probs = torch.where(st.keep.view(-1, 1) != 0, torch.nn.functional.one_hot(st.known.long(), st.K).to(st.probs.dtype), st.probs)
        return st.lab.view(labels.shape), st.probs


def build_model(time_steps: int, schedule: str, schedule_params, input_shapes, cond_encoded_shape, backbone: str,
                backbone_params: Dict[str, Any], dataset_file: str, step_T_sample: str = None, feature_cond_encoder: dict = None,
                dims: int = 3) -> DenoisingModel:
    """Same contract as ccdm/ddpm/models/builder.py:14-53 (in_channels = num_classes + img_channels)."""
    img_shape, label_shape, *_ = input_shapes
    img_channels, num_classes = img_shape[0], label_shape[0]
    diffusion = DiffusionModel(schedule, time_steps, num_classes, schedule_params=schedule_params, dims=dims)
    if backbone != "unet_openai":
        raise NotImplementedError(f"backbone {backbone}")
    fce = feature_cond_encoder if (feature_cond_encoder or {}).get("type", "none") not in ("none", None) else None
    model = create_unet_openai(image_size=min(img_shape[1], img_shape[2]), in_channels=num_classes + img_channels,
                               out_channels=num_classes, num_res_blocks=2, cond_encoded_shape=cond_encoded_shape,
                               feature_cond_encoder=fce, dims=dims, **backbone_params)
    return DenoisingModel(diffusion, model, dataset_file, step_T_sample, dims)
