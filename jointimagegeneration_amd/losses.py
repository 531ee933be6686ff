"""Held-out objectives of the CCDM mask model, forward only (ccdm/ddpm/trainer.py:298-327).

One call = `gg_ccdm_q_sample` (noise the labels to step t, one-hot straight into the UNet input) -> one `unet.forward_cl` with per-sample
`time_bias_rows(t)` -> `gg_ccdm_step_loss` on the head's fp32 logits, which are written once and read once.  No gradients, no optimizer:
the model stays in eval mode (the LDM counterparts are methods of ldm.DDPM / ldm.LatentDiffusion).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch
from torch import Tensor

from . import ops
from .ops import CL, pad32

__all__ = ["ccdm_step_losses"]


@torch.no_grad()
def ccdm_step_losses(model, x0_labels: Tensor, condition: Optional[Tensor], t: Tensor, class_weights: Optional[Tensor] = None,
                     rng_tape: Optional[Tensor] = None, philox_seeds: Optional[Sequence[int]] = None,
                     feature_condition=None) -> Dict[str, Tensor]:
    """The KL and cross-entropy terms of the reference's train_step for a held-out batch.
    model: ccdm.DenoisingModel on the GPU, eval mode.  x0_labels: integer labels [N, (D,) H, W]; condition: fp32 [N, C_img, (D,) H, W] or
    None; t: 1-based steps [N].  class_weights: [K] (default ones).  The noise of q_xt_given_x0(x0, t).sample() comes from rng_tape (fp32
    [M, K] exponentials) or from Philox with one key per sample (philox_seeds, default 1024 + n), so a sample's terms do not depend on
    its batch slot.  Returns loss_kl, loss_ce, loss (sums / batch size, trainer.py:325-327; fp64 0-d tensors on the device), the
    per-sample fp64 sums `kl_per_sample`, `ce_per_sample` and the drawn `xt` (int32 labels)."""
    if model.training:
        raise RuntimeError("ccdm_step_losses: the model is in training mode; this engine evaluates objectives forward-only (eval mode)")
    if feature_condition is not None:
        raise NotImplementedError("ccdm_step_losses: feature_condition is not supported (always None on the shipped path, evaluator.py:169)")
    unet, diff = model.unet, model.diffusion
    if not getattr(unet, "sofmtax_output", True):
        raise NotImplementedError("ccdm_step_losses: softmax_output=False is not supported (the objective is defined on the softmax head, "
                                  "trainer.py:304-320)")
    dev = diff.alphas.device
    if dev.type != "cuda":
        raise NotImplementedError(f"ccdm_step_losses: not supported for a model on {dev} (the noising and reduction kernels are the GPU's; "
                                  "there is no CPU path)")
    K = diff.num_classes
    N = int(x0_labels.shape[0])
    sp = tuple(x0_labels.shape[1:])
    if len(sp) != diff.dims:
        raise ValueError(f"ccdm_step_losses: labels {tuple(x0_labels.shape)} for a dims = {diff.dims} model")
    t = torch.as_tensor(t).reshape(-1).to(dev).long()
    if t.numel() != N:
        raise ValueError(f"ccdm_step_losses: {t.numel()} timesteps for a batch of {N}")
    sp3 = (1,) * (3 - len(sp)) + sp
    M = x0_labels.numel()
    x0 = x0_labels.to(dev).to(torch.int32).contiguous().view(-1)
    scal = diff.step_scalar_rows(t)                                            # validates t
    ca = diff.cumalphas[t - 1].float()
    keep = torch.stack([ca, 1 - ca], 1).contiguous()                           # (one-hot weight, uniform mass) of q_xt_given_x0
    cw = torch.ones(K, dtype=torch.float32, device=dev) if class_weights is None else class_weights.to(dev).float().contiguous()
    if cw.numel() != K:
        raise ValueError(f"ccdm_step_losses: {cw.numel()} class weights for {K} classes")
    cin = unet.in_channels
    xin = torch.zeros((N,) + sp3 + (pad32(cin),), dtype=torch.float32 if ops.FP32 else torch.bfloat16, device=dev)
    bf16_in = xin.dtype == torch.bfloat16
    if rng_tape is not None:
        xt = ops.ccdm_q_sample(x0, keep, K, E=rng_tape.to(dev).float().contiguous(), onehot_out=xin.view(M, -1) if bf16_in else None)
    else:
        keys = philox_seeds if philox_seeds is not None else [1024 + n for n in range(N)]
        if len(keys) != N:
            raise ValueError(f"ccdm_step_losses: {len(keys)} philox_seeds for a batch of {N}")
        xt = ops.ccdm_q_sample(x0, keep, K, philox_seeds=ops.philox_seed_tensor(keys, dev), onehot_out=xin.view(M, -1) if bf16_in else None)
    if not bf16_in:                                                            # fp32 validation mode: index scatter (plumbing)
        ops.labels_to_onehot(xt, K, xin.view(M, -1))
    if condition is not None:                                                  # unet.py:774-775: cat([x, input_condition], 1)
        ops.to_cl(condition.to(dev), out=xin, c_offset=K, zero_fill=False)
    logits = torch.empty((N,) + sp3 + (pad32(K),), dtype=torch.float32, device=dev)
    unet.forward_cl(CL(xin, cin), unet.time_bias_rows(t.float()), head_out=logits)
    sums = ops.ccdm_step_loss(logits.view(M, -1), xt, x0, scal, cw, K)
    kl, ce = sums[:, 0], sums[:, 1]
    loss_kl, loss_ce = kl.sum() / N, ce.sum() / N
    return {"loss_kl": loss_kl, "loss_ce": loss_ce, "loss": loss_kl + loss_ce, "kl_per_sample": kl, "ce_per_sample": ce,
            "xt": xt.view(x0_labels.shape)}
