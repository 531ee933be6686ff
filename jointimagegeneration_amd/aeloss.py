"""The first stage's held-out objective on the device, forward only: `LPIPSWithDiscriminator` of
ldm/modules/losses/contperceptual.py with its two PatchGAN discriminators, as `AutoencoderKL.validation_step` evaluates it.

The discriminators' convolutions (kernel 4, padding 2, stride 2 / 1, 2-D and 3-D) are `ops.patch_conv` calls with the conv bias and the
eval-mode BatchNorm folded into one multiply-add and LeakyReLU in the epilogue (csrc/gg_patchgan.hip); LPIPS is this package's `LPIPS`;
the pixel term is `gg_loss_rows`, the posterior's KL `gg_gauss_kl_rows`, the logit statistics `gg_logit_stats`.  What is left on the
torch side are combinations of a handful of fp64 numbers that stay on the device: every value of the returned dicts is a 0-dim fp32
device tensor and nothing is read back.

The reference's behaviour is kept, quirks included: `c > 1` is flattened to `(b c) 1 ...` first, so the 2-D nll
sums divide by b * c while kl_loss divides by the posterior's batch b; `forward_2d` always uses |x - y| and ignores gan_feat_weight;
`forward_3d` never uses logvar and averages the broadcast sum of pixel and perceptual terms; d_weight is 0.0, because under
validation's no_grad `autograd.grad` raises and the reference takes its `except` branch.  There are no gradients and no training mode.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from .lpips import LPIPS, MIN_EXTENT

BN_EPS = 1e-5                # nn.SyncBatchNorm's default
LEAKY_SLOPE = 0.2


class _PatchConv(nn.Module):
    """Parameter holder of one kernel-4 convolution."""

    def __init__(self, cin: int, cout: int, dims: int):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros((cout, cin) + (4,) * dims), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)


class _BatchNorm(nn.Module):
    """Parameter / buffer holder of an eval-mode (Sync)BatchNorm: y = (x - running_mean) / sqrt(running_var + eps) * weight + bias."""

    def __init__(self, c: int):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(c), requires_grad=False)
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class _Slot(nn.Module):
    """A parameter-free place in a Sequential (LeakyReLU): keeps the reference's indices."""


def _disc_blocks(input_nc: int, ndf: int, n_layers: int) -> List[Tuple[int, int, int, bool, bool]]:
    """(cin, cout, stride, has_norm, has_act) of the n_layers + 2 blocks (contperceptual.py:305-328)."""
    blocks = [(input_nc, ndf, 2, False, True)]
    nf = ndf
    for _ in range(1, n_layers):
        nf_prev, nf = nf, min(nf * 2, 512)
        blocks.append((nf_prev, nf, 2, True, True))
    nf_prev, nf = nf, min(nf * 2, 512)
    blocks.append((nf_prev, nf, 1, True, True))
    blocks.append((nf, 1, 1, False, False))
    return blocks


class _NLayerDiscriminatorND(nn.Module):
    DIMS = 2

    def __init__(self, input_nc, ndf=64, n_layers=3, norm_layer=None, use_sigmoid=False, getIntermFeat=True, use_actnorm=False):
        super().__init__()
        who = type(self).__name__
        if use_actnorm:
            raise NotImplementedError(f"{who}: use_actnorm=True is not supported (ActNorm is taming's, used by no shipped config)")
        if use_sigmoid:
            raise NotImplementedError(f"{who}: use_sigmoid=True is not supported (the losses take logits)")
        self.getIntermFeat, self.n_layers = getIntermFeat, n_layers
        self.blocks = _disc_blocks(input_nc, ndf, n_layers)
        flat = nn.Module()
        i = 0
        for n, (cin, cout, _, has_norm, has_act) in enumerate(self.blocks):
            seq = nn.Module() if getIntermFeat else flat
            j = 0 if getIntermFeat else i
            seq.add_module(str(j), _PatchConv(cin, cout, self.DIMS))
            if has_norm:
                seq.add_module(str(j + 1), _BatchNorm(cout))
            if has_act:
                seq.add_module(str(j + 1 + has_norm), _Slot())
            i += 1 + has_norm + has_act
            if getIntermFeat:
                self.add_module(f"model{n}", seq)
        if not getIntermFeat:
            self.model = flat
        self._packs = {}

    def _layers(self) -> List[Tuple[_PatchConv, Optional[_BatchNorm]]]:
        out, i = [], 0
        for n, (_, _, _, has_norm, has_act) in enumerate(self.blocks):
            seq = getattr(self, f"model{n}") if self.getIntermFeat else self.model
            j = 0 if self.getIntermFeat else i
            out.append((getattr(seq, str(j)), getattr(seq, str(j + 1)) if has_norm else None))
            i += 1 + has_norm + has_act
        return out

    def _token(self):
        n = v = a = 0
        for t in list(self.parameters()) + list(self.buffers()):
            n, v, a = n + 1, v + t._version, a + t.data_ptr()
        return n, v, a

    def _packed(self):
        """Per precision mode: [(packed weight, alpha or None, beta)] per block; rebuilt when a parameter or a buffer changes.  The fold is
        fp64: alpha = gamma / sqrt(running_var + eps), beta' = (bias - running_mean) * alpha + beta."""
        key = (ops.FP32, self._token())
        hit = self._packs.get(ops.FP32)
        if hit is None or hit[0] != key:
            packs = []
            for (conv, bn), (cin, cout, _, _, _) in zip(self._layers(), self.blocks):
                pw = ops.pack_conv_weight(conv.weight, ops.pad32(cin))
                dev = conv.weight.device
                alpha, beta = None, torch.zeros(ops.pad32(cout), dtype=torch.float32, device=dev)
                if bn is None:
                    beta[:cout] = conv.bias.detach().float()
                else:
                    a64 = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + BN_EPS)
                    alpha = torch.zeros(ops.pad32(cout), dtype=torch.float32, device=dev)
                    alpha[:cout] = a64.float()
                    beta[:cout] = ((conv.bias.detach().double() - bn.running_mean.detach().double()) * a64 + bn.bias.detach().double()).float()
                packs.append((pw, alpha, beta))
            hit = (key, packs)
            self._packs[ops.FP32] = hit
        return hit[1]

    def check_input(self, x: torch.Tensor) -> None:
        who = type(self).__name__
        if self.training:
            raise NotImplementedError(f"{who}: training mode is not supported (BatchNorm runs on its running statistics; call .eval())")
        ops.require_gpu(x, who)
        if x.dim() != 2 + self.DIMS or x.shape[1] != self.blocks[0][0]:
            raise ValueError(f"{who}: input {tuple(x.shape)} is not [N, {self.blocks[0][0]}" + ", *" * self.DIMS + "]")
        if next(self.parameters()).device != x.device:
            raise RuntimeError(f"{who}: the weights are on {next(self.parameters()).device}, the input on {x.device}")

    def run_cl(self, x: ops.CL) -> List[ops.CL]:
        """Every block's output, channels-last; the last one (the logits, lane 0) is fp32."""
        outs, kd = [], (4 if self.DIMS == 3 else 1)
        for n, ((pw, alpha, beta), (_, cout, stride, _, has_act)) in enumerate(zip(self._packed(), self.blocks)):
            x = ops.patch_conv(x, pw, alpha, beta, cout, kd, stride, slope=LEAKY_SLOPE if has_act else 1.0, out_f32=n + 1 == len(self.blocks))
            outs.append(x)
        return outs

    def logits_cl(self, x: torch.Tensor) -> torch.Tensor:
        """NC(D)HW fp32 -> the logits as fp32 channels-last rows (lane 0)."""
        self.check_input(x)
        return self.run_cl(ops.to_cl(x.detach().float()))[-1].t

    @torch.no_grad()
    def forward(self, input: torch.Tensor):
        self.check_input(input)
        outs = [ops.from_cl(o, self.DIMS) for o in self.run_cl(ops.to_cl(input.detach().float()))]
        return (outs[-1], outs) if self.getIntermFeat else outs[-1]


class NLayerDiscriminator(_NLayerDiscriminatorND):
    """contperceptual.py:296-350, eval mode: state_dict names `model.<i>.*` (getIntermFeat False) or `model<n>.<i>.*`."""
    DIMS = 2


class NLayerDiscriminator3D(_NLayerDiscriminatorND):
    """contperceptual.py:353-406, eval mode."""
    DIMS = 3


class LPIPSWithDiscriminator(nn.Module):
    """contperceptual.py:49-293 as validation_step calls it; the constructor's surface equals the reference's key for key."""

    def __init__(self, disc_start, logvar_init=1.0, kl_weight=1.0, pixelloss_weight=1.0, disc_num_layers=3, disc_in_channels=3,
                 disc_factor=1.0, disc_weight=1.0, perceptual_weight=1.0, use_actnorm=False, disc_conditional=False, disc_loss="hinge",
                 pixel_loss="l1", image_gan_weight=0.5, ct_gan_weight=0.5, gan_feat_weight=1.0, dims=2):
        super().__init__()
        if disc_loss not in ("hinge", "vanilla"):
            raise ValueError(f"LPIPSWithDiscriminator: disc_loss '{disc_loss}' (one of 'hinge', 'vanilla')")
        if use_actnorm:
            raise NotImplementedError("LPIPSWithDiscriminator: use_actnorm=True is not supported (ActNorm is taming's, used by no shipped config)")
        if disc_conditional:
            raise NotImplementedError("LPIPSWithDiscriminator: disc_conditional=True is not supported (it concatenates a cond tensor to the "
                                      "discriminator input; no shipped config sets it)")
        self.kl_weight, self.pixel_weight, self.perceptual_weight = kl_weight, pixelloss_weight, perceptual_weight
        self.pixel_loss = "l1" if pixel_loss == "l1" else "l2"                 # anything but "l1" is l2, as in the reference
        self.perceptual_loss = LPIPS().eval()
        self.logvar = nn.Parameter(torch.ones(size=()) * logvar_init, requires_grad=False)
        self.frame_discriminator = NLayerDiscriminator(input_nc=disc_in_channels, n_layers=disc_num_layers, getIntermFeat=dims == 3)
        self.ct_discriminator = NLayerDiscriminator3D(input_nc=disc_in_channels, n_layers=disc_num_layers)
        self.discriminator_iter_start = disc_start
        self.disc_loss = disc_loss
        self.disc_factor, self.discriminator_weight, self.disc_conditional = disc_factor, disc_weight, disc_conditional
        self.image_gan_weight, self.ct_gan_weight, self.gan_feat_weight = image_gan_weight, ct_gan_weight, gan_feat_weight
        self._vgg_checked = None

    # ------------------------------------------------------------------------------------------- refusals, before any launch
    def _check(self, inputs, reconstructions, posteriors, optimizer_idx, cond, weights) -> int:
        who = "LPIPSWithDiscriminator"
        if self.training:
            raise NotImplementedError(f"{who}: training mode is not supported (forward only: no gradients, no adaptive weight; call .eval())")
        if cond is not None or self.disc_conditional:
            raise NotImplementedError(f"{who}: cond / disc_conditional is not supported")
        if weights is not None:
            raise NotImplementedError(f"{who}: weights (per-element nll weights) is not supported")
        if optimizer_idx not in (0, 1):
            raise ValueError(f"{who}: optimizer_idx {optimizer_idx} (0: autoencoder, 1: discriminator)")
        if tuple(inputs.shape) != tuple(reconstructions.shape):
            raise ValueError(f"{who}: {tuple(inputs.shape)} and {tuple(reconstructions.shape)} not match")
        nd = inputs.dim() - 2
        if nd not in (2, 3):
            raise ValueError(f"{who}: [b, c, h, w] or [b, c, h, w, d] inputs, got {tuple(inputs.shape)}")
        if nd == 3:
            if self.gan_feat_weight > 0:
                raise NotImplementedError(f"{who}: dims == 3 with gan_feat_weight = {self.gan_feat_weight} > 0 is not supported: the reference reads "
                                          "disc_factor before it is assigned there (UnboundLocalError, contperceptual.py:247)")
            if self.image_gan_weight <= 0 or self.ct_gan_weight <= 0:
                raise NotImplementedError(f"{who}: dims == 3 with image_gan_weight = {self.image_gan_weight} or ct_gan_weight = {self.ct_gan_weight} "
                                          "<= 0 is not supported: the reference then reads logits it never computed (contperceptual.py:223)")
            if not self.frame_discriminator.getIntermFeat:
                raise ValueError(f"{who}: built with dims = 2 (the frame discriminator returns logits only), called on volumes")
        ops.require_gpu(inputs, who)
        ops.require_gpu(reconstructions, who)
        ops.require_gpu(posteriors.parameters, who)
        if self.logvar.device != inputs.device:
            raise RuntimeError(f"{who}: the loss module is on {self.logvar.device}, the input on {inputs.device}")
        if self.perceptual_weight > 0:
            if min(inputs.shape[-2:]) < MIN_EXTENT:
                raise ValueError(f"{who}: extent {tuple(inputs.shape[-2:])} below {MIN_EXTENT}: LPIPS's fourth max-pool would produce nothing")
            self._check_vgg()
        return nd

    def _check_vgg(self) -> None:
        """Once per set of weights (when LPIPS packs them): a perceptual term on the constructor's zero VGG weights would be a silent 0."""
        token = ops.weights_token(self.perceptual_loss)
        if self._vgg_checked != token:
            w = self.perceptual_loss.net.slice1.get_submodule("0").weight
            if not bool((w != 0).any()):
                raise RuntimeError("LPIPSWithDiscriminator: perceptual_weight > 0 but the VGG16 weights are still the constructor's zeros: load "
                                   "a checkpoint that carries loss.perceptual_loss.*, or the VGG / lin files (weights are never fetched)")
            self._vgg_checked = token

    # ------------------------------------------------------------------------------------------- device side
    def _stats(self, disc, x: torch.Tensor) -> torch.Tensor:
        return ops.logit_stats(disc.logits_cl(x))

    def _d_loss(self, real: torch.Tensor, fake: torch.Tensor) -> torch.Tensor:
        """hinge_d_loss / vanilla_d_loss from two gg_logit_stats rows (fp64)."""
        return 0.5 * (real[1] + fake[2]) if self.disc_loss == "hinge" else 0.5 * (real[3] + fake[4])

    @torch.no_grad()
    def forward(self, inputs, reconstructions, posteriors, optimizer_idx, global_step, last_layer=None, cond=None, split="train",
                weights=None) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
        nd = self._check(inputs, reconstructions, posteriors, optimizer_idx, cond, weights)
        dev = inputs.device
        b, c = int(inputs.shape[0]), int(inputs.shape[1])
        sp = tuple(int(v) for v in inputs.shape[2:])
        n = b * c
        x = inputs.detach().float().contiguous().reshape((n, 1) + sp)              # "b c ... -> (b c) 1 ..."
        y = reconstructions.detach().float().contiguous().reshape((n, 1) + sp)
        S = x[0].numel()
        f32 = lambda v: v.float()
        disc_factor = self.disc_factor if global_step >= self.discriminator_iter_start else 0.0
        fx = x.reshape((n * sp[0], 1) + sp[1:]) if nd == 3 else x                   # "b c h w d -> (b h) c w d" with c == 1
        fy = y.reshape((n * sp[0], 1) + sp[1:]) if nd == 3 else y

        if optimizer_idx == 1:
            fr, ff = self._stats(self.frame_discriminator, fx), self._stats(self.frame_discriminator, fy)
            if nd == 2:
                d_loss = disc_factor * self._d_loss(fr, ff)
                log = {f"{split}/disc_loss": f32(d_loss), f"{split}/logits_real": f32(fr[0]), f"{split}/logits_fake": f32(ff[0])}
                return f32(d_loss), log
            cr, cf = self._stats(self.ct_discriminator, x), self._stats(self.ct_discriminator, y)
            d_loss = disc_factor * (self._d_loss(fr, ff) + self._d_loss(cr, cf)) / 2
            log = {f"{split}/disc_loss": f32(d_loss), f"{split}/logits_frames_real": f32(fr[0]), f"{split}/logits_frames_fake": f32(ff[0]),
                   f"{split}/logits_ct_real": f32(cr[0]), f"{split}/logits_ct_fake": f32(cf[0])}
            return f32(d_loss), log

        # pixel term: per (b c) image / volume mean of |x - y| or (x - y)^2; with one channel the NC(D)HW tensor is its own channels-last form
        pix = ops.loss_rows("l1" if nd == 2 else self.pixel_loss, n, 1, S, pred=y.view(n * S, 1), target=x)               # fp64 [n]
        p = None
        if self.perceptual_weight > 0:
            p = self.perceptual_loss(fx, fy).reshape(-1).double()                                                           # per image / frame
        kl = posteriors.kl_rows().sum() / int(posteriors.parameters.shape[0])
        logvar = self.logvar.detach().double()
        if nd == 2:
            rec = pix + self.perceptual_weight * p if p is not None else pix                    # per image: mean |x - y| + w * p_n
            nll = (S * (rec / torch.exp(logvar) + logvar)).sum() / n
            rec_mean = rec.mean()
            g_loss = -self._stats(self.frame_discriminator, fy)[0]
        else:
            rec_mean = pix.mean() + self.perceptual_weight * p.mean() if p is not None else pix.mean()
            nll = rec_mean
            g_loss = -(self._stats(self.frame_discriminator, fy)[0] + self._stats(self.ct_discriminator, y)[0]) / 2
        d_weight = torch.tensor(0.0, device=dev)        # autograd.grad raises under no_grad: the reference's except branch
        loss = nll + self.kl_weight * kl + d_weight.double() * disc_factor * g_loss
        log = {f"{split}/total_loss": f32(loss), f"{split}/logvar": self.logvar.detach().float(), f"{split}/kl_loss": f32(kl),
               f"{split}/nll_loss": f32(nll), f"{split}/rec_loss": f32(rec_mean), f"{split}/d_weight": d_weight,
               f"{split}/disc_factor": torch.tensor(float(disc_factor), device=dev), f"{split}/g_loss": f32(g_loss)}
        if nd == 3:
            log[f"{split}/gan_feat_loss"] = torch.tensor(0.0, device=dev)        # gan_feat_weight == 0 (checked above)
        return f32(loss), log
