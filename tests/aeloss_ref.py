"""fp64 restatement of the first stage's held-out objective (ldm/modules/losses/contperceptual.py as AutoencoderKL.validation_step calls
it): the PatchGAN convolutions, eval-mode BatchNorm, LeakyReLU, both discriminators, the hinge / vanilla losses, the posterior's KL and
draw, and the two dicts of forward_2d / forward_3d -- and the seed recipe of the weights that tests/golden/aeloss.npz was recorded with.
Test infrastructure: torch on the CPU, in whatever dtype the tensors have (the tests hand it float64)."""
import numpy as np
import torch
import torch.nn.functional as F

import lpips_ref

BN_EPS = 1e-5
SLOPE = 0.2


def disc_blocks(input_nc, n_layers, ndf=64):
    """(cin, cout, stride, has_norm, has_act) per block: n_layers stride-2 convolutions, one stride-1, the 1-channel head."""
    blocks, nf = [(input_nc, ndf, 2, False, True)], ndf
    for _ in range(1, n_layers):
        blocks.append((nf, min(nf * 2, 512), 2, True, True))
        nf = min(nf * 2, 512)
    blocks.append((nf, min(nf * 2, 512), 1, True, True))
    blocks.append((min(nf * 2, 512), 1, 1, False, False))
    return blocks


def disc_names(n_layers, interm):
    """Per block: (prefix of the convolution, prefix of the norm or None) in the discriminator's state_dict."""
    names, i = [], 0
    for n, (_, _, _, has_norm, has_act) in enumerate(disc_blocks(1, n_layers)):
        conv = f"model{n}.0" if interm else f"model.{i}"
        norm = (f"model{n}.1" if interm else f"model.{i + 1}") if has_norm else None
        names.append((conv, norm))
        i += 1 + has_norm + has_act
    return names


def seeded_disc_state_dict(dims, input_nc, n_layers, interm, seed, gain):
    """Convolutions Kaiming-normal (a = 0.2) times `gain`, conv biases N(0, 0.2); BatchNorm weight N(1, 0.2), bias N(0, 0.2), running_mean
    N(0, 0.2), running_var U(0.5, 1.5); drawn in block order from one generator of `seed`.  (The reference's weights_init draws N(0, 0.02):
    every logit is then about 0.03 and the hinge never switches.)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for (cin, cout, _, _, _), (conv, norm) in zip(disc_blocks(input_nc, n_layers), disc_names(n_layers, interm)):
        fan_in = cin * 4 ** dims
        std = gain * np.sqrt(2.0 / (1 + SLOPE ** 2)) / np.sqrt(fan_in)
        sd[conv + ".weight"] = torch.randn((cout, cin) + (4,) * dims, generator=g) * std
        sd[conv + ".bias"] = torch.randn(cout, generator=g) * 0.2
        if norm:
            sd[norm + ".weight"] = 1 + 0.2 * torch.randn(cout, generator=g)
            sd[norm + ".bias"] = 0.2 * torch.randn(cout, generator=g)
            sd[norm + ".running_mean"] = 0.2 * torch.randn(cout, generator=g)
            sd[norm + ".running_var"] = 0.5 + torch.rand(cout, generator=g)
            sd[norm + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.long)
    return sd


def patch_conv(x, w, stride):
    """Kernel 4, zero padding 2 on every spatial axis, one stride: x [N, Cin, *sp], w [Cout, Cin, 4, 4(, 4)]."""
    return (F.conv3d if w.dim() == 5 else F.conv2d)(x, w.to(x), None, stride=stride, padding=2)


def disc_forward(x, sd, n_layers, interm):
    """Every block's output (the last: the logits), in x's dtype."""
    outs = []
    for (_, _, stride, _, has_act), (conv, norm) in zip(disc_blocks(x.shape[1], n_layers), disc_names(n_layers, interm)):
        shape = (1, -1) + (1,) * (x.dim() - 2)
        x = patch_conv(x, sd[conv + ".weight"], stride) + sd[conv + ".bias"].to(x).reshape(shape)
        if norm:
            rm, rv = sd[norm + ".running_mean"].to(x).reshape(shape), sd[norm + ".running_var"].to(x).reshape(shape)
            x = (x - rm) / torch.sqrt(rv + BN_EPS) * sd[norm + ".weight"].to(x).reshape(shape) + sd[norm + ".bias"].to(x).reshape(shape)
        if has_act:
            x = torch.where(x >= 0, x, x * SLOPE)
        outs.append(x)
    return outs


def fold_bn(sd, conv, norm):
    """(alpha, beta) of y = acc * alpha + beta, fp64: conv bias and eval BatchNorm in one multiply-add."""
    b = sd[conv + ".bias"].double()
    if norm is None:
        return None, b
    alpha = sd[norm + ".weight"].double() / torch.sqrt(sd[norm + ".running_var"].double() + BN_EPS)
    return alpha, (b - sd[norm + ".running_mean"].double()) * alpha + sd[norm + ".bias"].double()


def softplus(x):
    return torch.where(x > 20, x, torch.log1p(torch.exp(torch.clamp(x, max=20))))


def logit_stats(l):
    """means of l, relu(1 - l), relu(1 + l), softplus(-l), softplus(l)"""
    return torch.stack([l.mean(), torch.relu(1 - l).mean(), torch.relu(1 + l).mean(), softplus(-l).mean(), softplus(l).mean()])


def d_loss(kind, real, fake):
    return 0.5 * (real[1] + fake[2]) if kind == "hinge" else 0.5 * (real[3] + fake[4])


def gauss_kl(moments):
    """[N, 2C, *sp] -> [N]: 0.5 * sum(mean^2 + var - 1 - logvar), logvar clamped to [-30, 20]."""
    m, lv = torch.chunk(moments, 2, dim=1)
    lv = torch.clamp(lv, -30.0, 20.0)
    return 0.5 * (m ** 2 + torch.exp(lv) - 1.0 - lv).flatten(1).sum(1)


def gauss_sample(moments, noise):
    m, lv = torch.chunk(moments, 2, dim=1)
    return m + torch.exp(0.5 * torch.clamp(lv, -30.0, 20.0)) * noise


def loss_dicts(cfg, x, y, moments, p_images, frame_sd, ct_sd, global_step, split="val"):
    """Both dicts of LPIPSWithDiscriminator.forward(..., optimizer_idx 0 | 1, split) in x's dtype.  cfg: the constructor's arguments that
    matter (dims, disc_start, logvar_init, kl_weight, disc_num_layers, disc_factor, perceptual_weight, disc_loss, pixel_loss); p_images:
    per-image (2-D) / per-frame (3-D) LPIPS values or None.  Returns (dict 0, dict 1, parts): parts holds the intermediate scalars the
    tolerances are taken on."""
    nd = x.dim() - 2
    b, c = x.shape[:2]
    n = b * c
    x, y = x.reshape((n, 1) + tuple(x.shape[2:])), y.reshape((n, 1) + tuple(y.shape[2:]))
    nl, pw = cfg["disc_num_layers"], cfg["perceptual_weight"]
    logvar = torch.tensor(cfg["logvar_init"], dtype=x.dtype)
    disc_factor = cfg["disc_factor"] if global_step >= cfg["disc_start"] else 0.0
    kl = gauss_kl(moments).sum() / moments.shape[0]
    fx = x.reshape((-1, 1) + tuple(x.shape[3:])) if nd == 3 else x
    fy = y.reshape((-1, 1) + tuple(y.shape[3:])) if nd == 3 else y
    interm = nd == 3
    fr = logit_stats(disc_forward(fx, frame_sd, nl, interm)[-1])
    ff = logit_stats(disc_forward(fy, frame_sd, nl, interm)[-1])
    parts = {}
    if nd == 2:
        pix = (x - y).abs().flatten(1).mean(1)
        rec = pix + pw * p_images if pw > 0 else pix
        S = x[0].numel()
        nll = (S * (rec / torch.exp(logvar) + logvar)).sum() / n
        rec_mean = rec.mean()
        g_loss = -ff[0]
        dl = disc_factor * d_loss(cfg["disc_loss"], fr, ff)
        d1 = {f"{split}/disc_loss": dl, f"{split}/logits_real": fr[0], f"{split}/logits_fake": ff[0]}
    else:
        d = x - y
        pix = (d.abs() if cfg["pixel_loss"] == "l1" else d ** 2).flatten(1).mean(1)
        rec_mean = pix.mean() + pw * p_images.mean() if pw > 0 else pix.mean()
        nll = rec_mean
        cr = logit_stats(disc_forward(x, ct_sd, nl, True)[-1])
        cf = logit_stats(disc_forward(y, ct_sd, nl, True)[-1])
        g_loss = -(ff[0] + cf[0]) / 2
        dl = disc_factor * (d_loss(cfg["disc_loss"], fr, ff) + d_loss(cfg["disc_loss"], cr, cf)) / 2
        d1 = {f"{split}/disc_loss": dl, f"{split}/logits_frames_real": fr[0], f"{split}/logits_frames_fake": ff[0],
              f"{split}/logits_ct_real": cr[0], f"{split}/logits_ct_fake": cf[0]}
    zero = torch.zeros((), dtype=x.dtype)
    total = nll + cfg["kl_weight"] * kl + zero * disc_factor * g_loss
    d0 = {f"{split}/total_loss": total, f"{split}/logvar": logvar, f"{split}/kl_loss": kl, f"{split}/nll_loss": nll, f"{split}/rec_loss": rec_mean,
          f"{split}/d_weight": zero, f"{split}/disc_factor": torch.tensor(float(disc_factor), dtype=x.dtype), f"{split}/g_loss": g_loss}
    if nd == 3:
        d0[f"{split}/gan_feat_loss"] = zero
    parts["pixel"] = pix.mean()
    return d0, d1, parts


def lpips_images64(fx, fy, lins):
    """Per-image LPIPS of 1-channel images in fp64 on the seed-recipe VGG weights (lpips_ref)."""
    sd = {k: v.double() for k, v in lpips_ref.seeded_vgg_state_dict().items()}
    return lpips_ref.lpips_images(fx.double(), fy.double(), sd, [torch.as_tensor(w).double() for w in lins])[0]


# which tolerance kind governs each key of the two dicts (tests/golden/aeloss.npz holds tol_<kind>)
KEY_KIND = {"total_loss": "nll", "logvar": "exact", "kl_loss": "kl", "nll_loss": "nll", "rec_loss": "nll", "d_weight": "exact",
            "disc_factor": "exact", "g_loss": "logit", "gan_feat_loss": "exact", "disc_loss": "logit", "logits_real": "logit",
            "logits_fake": "logit", "logits_frames_real": "logit", "logits_frames_fake": "logit", "logits_ct_real": "logit",
            "logits_ct_fake": "logit"}
