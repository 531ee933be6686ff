"""DPM-Solver++ in its multistep second-order data-prediction form ("2M": Lu et al. 2022, "DPM-Solver++: Fast Solver for Guided Sampling
of Diffusion Probabilistic Models", Algorithm 2) on the latent chain of ldm.py: a high-order solver of the probability-flow ODE that
DDIM (its first-order member) integrates, meant for 15-25 UNet evaluations where DDIM takes 50.

Symbols, at a DDPM index with cumulative alpha a (the fp32 `alphas_cumprod` value DDIM reads, widened to fp64): alpha = sqrt(a),
sigma = sqrt(1 - a), lambda = log(alpha / sigma) (half the log-SNR).  A step goes from the current point s to the next point t,
h = lambda_t - lambda_s > 0:
    p      = (x - sigma_s * out) / alpha_s                      the prediction of x_0 (out itself on an x0 model; optionally clamped)
    D      = p                                                  first order
             (1 + 1/(2r)) * p - 1/(2r) * p_prev,  r = h_prev / h        second order
    x_next = (sigma_t / sigma_s) * x - alpha_t * expm1(-h) * D
The host computes each step's row {alpha_s, sigma_s, k_x, k_d, c0, c1} in fp64 and rounds it once to fp32 (`dpm_rows`); the step itself
is one `gg_dpm_solver_step` launch on the chain's fp32 state.  The first step is first order; so is the last one when
`lower_order_final` is set and the chain has fewer than 15 steps.  With order = 1 every step is DDIM's at eta 0, algebraically.

Grids (`dpm_timesteps`): "uniform" and "quad" are DDIM's (make_ddim_timesteps) with repeated timesteps dropped, so that h > 0 on every
step; "logsnr", the default here, places the steps uniformly in lambda, which is what the solver's error analysis assumes and where its
gain over DDIM comes from.

`DPMSolverSampler` is a DDIMSampler: it inherits the channels-last state, the captured chain, classifier-free guidance, inpainting, the
step logs and the callbacks, and replaces the scalar table, the state's history buffer and the update launch.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from .chain import rows
from .ldm import DDIMSampler, make_ddim_timesteps

DISCRETIZATIONS = ("uniform", "quad", "logsnr")
LOWER_ORDER_FINAL_BELOW = 15          # steps: a shorter chain ends on a first-order step (lower_order_final)


def half_log_snr(alphas_cumprod) -> np.ndarray:
    """lambda[k] = log(alpha_k / sigma_k) of every DDPM index, fp64 from the fp32 table."""
    a = np.asarray(alphas_cumprod, dtype=np.float32).astype(np.float64)
    return np.log(np.sqrt(a) / np.sqrt(1.0 - a))


def logsnr_timesteps(num_steps: int, alphas_cumprod) -> np.ndarray:
    """The log-SNR-uniform grid: the `num_steps` targets linspace(lambda[T - 1], lambda[0], num_steps + 1)[:-1], each mapped to the DDPM
    index whose lambda is nearest (the lower index on a tie), clamped to >= 1; returns the ascending unique indices (fewer than
    `num_steps` where two targets share an index)."""
    lam = half_log_snr(alphas_cumprod)
    if num_steps < 1 or lam.shape[0] < 2:
        raise ValueError(f"logsnr_timesteps: {num_steps} steps on {lam.shape[0]} DDPM timesteps")
    targets = np.linspace(lam[-1], lam[0], num_steps + 1)[:-1]
    idx = np.abs(lam[None, :] - targets[:, None]).argmin(1)
    return np.unique(np.maximum(idx, 1)).astype(np.int64)


def dpm_timesteps(discretize: str, num_steps: int, alphas_cumprod) -> np.ndarray:
    """Ascending, strictly increasing DDPM indices of the chain's points (the step from index ts[j] goes to ts[j - 1], the last one to
    index 0).  "uniform" / "quad": DDIM's timesteps with repeats dropped ("quad" repeats some at 50 steps and more); "logsnr": above."""
    if discretize == "logsnr":
        return logsnr_timesteps(num_steps, alphas_cumprod)
    if discretize not in DISCRETIZATIONS:
        raise NotImplementedError(f'There is no discretization method called "{discretize}" ({", ".join(DISCRETIZATIONS)})')
    return np.unique(make_ddim_timesteps(discretize, num_steps, len(alphas_cumprod), verbose=False)).astype(np.int64)


def dpm_rows(timesteps, alphas_cumprod, order: int = 2, lower_order_final: bool = True) -> np.ndarray:
    """fp32 [n, 6] rows {alpha_s, sigma_s, k_x, k_d, c0, c1} in SAMPLING order (from timesteps[-1] down; the last step ends at DDPM
    index 0, DDIM's a_prev), computed in fp64 and rounded once."""
    if order not in (1, 2):
        raise ValueError(f"dpm_rows: order = {order!r} is not supported (1 or 2)")
    ts = np.asarray(timesteps, dtype=np.int64)
    a = np.asarray(alphas_cumprod, dtype=np.float32).astype(np.float64)
    n = ts.shape[0]
    a_s = a[ts[::-1]]
    a_t = np.concatenate([a[ts[::-1][1:]], a[:1]])
    alpha_s, sigma_s, alpha_t, sigma_t = np.sqrt(a_s), np.sqrt(1.0 - a_s), np.sqrt(a_t), np.sqrt(1.0 - a_t)
    h = np.log(alpha_t / sigma_t) - np.log(alpha_s / sigma_s)
    if not bool((h > 0).all()):
        raise ValueError(f"dpm_rows: the timesteps {ts.tolist()} do not increase the log-SNR on every step")
    rows = np.zeros((n, 6), dtype=np.float64)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = alpha_s, sigma_s, sigma_t / sigma_s, -alpha_t * np.expm1(-h), 1.0
    for i in range(1, n):
        if order == 2 and not (i == n - 1 and lower_order_final and n < LOWER_ORDER_FINAL_BELOW):
            r = h[i - 1] / h[i]
            rows[i, 4], rows[i, 5] = 1.0 + 1.0 / (2.0 * r), -1.0 / (2.0 * r)
    return rows.astype(np.float32)


class DPMSolverSampler(DDIMSampler):
    """DPM-Solver++ (2M) with DDIMSampler's surface.  order: 2 (the multistep second-order solver) or 1 (DDIM at eta 0 through the same
    kernel).  The sampler is deterministic: eta, temperature, noise_dropout, noise_tape, quantize_x0 and score_corrector are refused by
    name, as are split_input_params models and models on the CPU.  `parameterization="x0"` models are supported (the solver works on
    the prediction of x_0), and `sample(clip_denoised=True)` clamps that prediction to [-1, 1]."""

    parameterizations = ("eps", "x0")
    head_update_is_ddim = False           # the head conv's epilogue is DDIM's update: never asked for here, whatever fuse_ddim says

    def __init__(self, model, order=2, lower_order_final=True, **kwargs):
        if isinstance(order, bool) or order not in (1, 2):
            raise ValueError(f"DPMSolverSampler: order = {order!r} is not supported (1: DDIM at eta 0, 2: DPM-Solver++ 2M)")
        super().__init__(model, **kwargs)
        self.order = int(order)
        self.lower_order_final = bool(lower_order_final)
        self.fuse_ddim = False
        self.clip_denoised = False
        self.ddim_discretize = None

    @property
    def state_tag(self):
        """Joins the key of every chain state: the solver's rows, its history buffer and the clip flag baked into a captured chain."""
        return (("dpm_solver", self.order, self.lower_order_final, bool(self.clip_denoised)),)

    def make_schedule(self, ddim_num_steps, ddim_discretize="logsnr", ddim_eta=0.0, verbose=True):
        """DDIMSampler.make_schedule's tables on the solver's grid (`dpm_timesteps`); the chain's step count is the grid's own."""
        if ddim_eta != 0:
            raise ValueError(f"{type(self).__name__}: eta = {ddim_eta} is not supported (the solver is deterministic; eta must be 0)")
        self._note_schedule(ddim_num_steps, ddim_discretize, ddim_eta)
        ac = self.model.alphas_cumprod.detach().cpu().float()
        assert ac.shape[0] == self.ddpm_num_timesteps, "alphas have to be defined for each timestep"
        ts = dpm_timesteps(ddim_discretize, int(ddim_num_steps), ac.numpy())
        self.ddim_discretize = ddim_discretize
        self.ddim_timesteps = ts
        self.ddim_alphas = ac[ts]
        self.ddim_alphas_prev = torch.as_tensor(np.asarray([float(ac[0])] + ac[ts[:-1]].tolist()))
        self.ddim_sigmas = torch.zeros(ts.shape[0], dtype=torch.float64)
        self.ddim_sqrt_one_minus_alphas = torch.sqrt(1.0 - self.ddim_alphas)

    def step_scalar_table(self) -> torch.Tensor:
        """fp32 [S, 6] rows of `dpm_rows` in SAMPLING order."""
        ac = self.model.alphas_cumprod.detach().cpu().float().numpy()
        return torch.from_numpy(dpm_rows(self.ddim_timesteps, ac, self.order, self.lower_order_final))

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0.0, mask=None, x0=None, temperature=1.0, noise_dropout=0.0, score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=None, unconditional_guidance_scale=1.0,
               unconditional_conditioning=None, noise_tape: Optional[Sequence[torch.Tensor]] = None, ddim_discretize="logsnr",
               mask_noise_tape: Optional[Sequence[torch.Tensor]] = None, clip_denoised=False, **kwargs):
        """DDIMSampler.sample's signature and return values.  `ddim_discretize` defaults to "logsnr"; the chain's step count is the
        grid's own (at most S; the log lists follow it).  `clip_denoised` (this package's addition) clamps each step's prediction of x_0
        to [-1, 1].  Refused on the host, before any launch: eta != 0, temperature != 1, noise_dropout > 0, noise_tape, quantize_x0,
        score_corrector, a model with split_input_params, a model on the CPU."""
        who = f"{type(self).__name__}.sample"
        why = "the solver integrates the deterministic probability-flow ODE"
        if eta != 0:
            raise NotImplementedError(f"{who}: eta = {eta} is not supported ({why}: there is no noise term)")
        if float(temperature) != 1.0:
            raise NotImplementedError(f"{who}: temperature = {temperature} is not supported ({why}: there is no noise to scale)")
        if float(noise_dropout) > 0.0:
            raise NotImplementedError(f"{who}: noise_dropout = {noise_dropout} is not supported ({why}: there is no noise to drop)")
        if noise_tape is not None:
            raise NotImplementedError(f"{who}: noise_tape is not supported ({why}: no step reads a noise)")
        if quantize_x0:
            raise NotImplementedError(f"{who}: quantize_x0 is not supported (the multistep history would mix quantised predictions)")
        if score_corrector is not None:
            raise NotImplementedError(f"{who}: score_corrector is not supported (a user callback inside the step)")
        if getattr(self.model, "split_input_params", None) is not None:
            raise NotImplementedError(f"{who}: split_input_params (patch-wise evaluation) is not supported")
        if self.model.device.type != "cuda":
            raise NotImplementedError(f"{who}: not supported for a model on {self.model.device} (the step kernel is the GPU's; there is "
                                      "no CPU path)")
        keep = self.clip_denoised
        self.clip_denoised = bool(clip_denoised)
        try:
            return super().sample(S, batch_size, shape, conditioning=conditioning, callback=callback, normals_sequence=normals_sequence,
                                  img_callback=img_callback, mask=mask, x0=x0, corrector_kwargs=corrector_kwargs, verbose=verbose, x_T=x_T,
                                  log_every_t=log_every_t, unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, ddim_discretize=ddim_discretize,
                                  mask_noise_tape=mask_noise_tape, **kwargs)
        finally:
            self.clip_denoised = keep

    def prepare_state(self, N, Cx, sp, dev, Cc, ctx_shape=None, *, mask_C=0, vq=None, logged=None):
        """DDIMSampler.prepare_state, with sample()'s refusals of what the solver cannot run for a caller that asks for such a state directly."""
        if vq is not None:
            raise NotImplementedError(f"{type(self).__name__}: quantize_x0 / temperature are not supported")
        if getattr(self.model, "split_input_params", None) is not None:
            raise NotImplementedError(f"{type(self).__name__}: split_input_params (patch-wise evaluation) is not supported")
        return super().prepare_state(N, Cx, sp, dev, Cc, ctx_shape, mask_C=mask_C, logged=logged)

    def extend_state(self, st):
        """"hist": the fp32 CL buffer of the previous step's prediction of x_0.  A captured chain needs no reset of it: its first step is
        first order and does not read it."""
        st["hist"] = torch.empty_like(st["pred_x0"])

    def _update(self, st, eps, scal, noise=None):
        """The solver's update as one launch on the state's buffers (gg_dpm_solver_step); `scal` is a row of the six-column table."""
        if noise is not None:
            raise NotImplementedError(f"{type(self).__name__}: a step with noise (eta != 0 or a noise_tape) is not supported")
        x, out, hist, p0, uin = rows(st, "x", eps, "hist", "pred_x0", "unet_in")
        ops.dpm_solver_step(x, out, scal, hist, predicts_x0=getattr(self.model, "parameterization", "eps") == "x0", clip=bool(self.clip_denoised),
                            pred_x0_out=p0, unet_in=uin)
