"""CPU restatement of the CT editing loop (GuideGenPipeline.sample_ct_volumes with known_ct / keep) for ONE volume, on the
oracle's networks and DDIM functions: oracle.samplers.autoregressive_slices with (a) the visit list minus fully kept slices, (b) the
sampler's inpainting blend before each step of a mixed slice (ddim.py:144-148: img = q_sample(x0, t) * mask + (1 - mask) * img), (c) the
latent keep mask by the window rule, written as a brute-force loop, and (d) the per-pixel composite.  Pure torch, test infrastructure."""
import numpy as np
import torch

from oracle import nets as O
from oracle import samplers as S


def latent_keep_mask(keep2d: torch.Tensor, f: int, r: int) -> torch.Tensor:
    """keep2d bool [H, W] -> fp32 [H / f, W / f]: cell (i, j) is 1 iff every pixel of [f (i - r), f (i + 1 + r)) x [f (j - r), f (j + 1 + r))
    that lies inside the image is kept (pixels outside count as kept).  One pixel at a time."""
    H, W = keep2d.shape
    k = keep2d.bool().tolist()
    out = torch.zeros((H // f, W // f), dtype=torch.float32)
    for i in range(H // f):
        for j in range(W // f):
            ok = True
            for y in range(f * (i - r), f * (i + 1 + r)):
                for x in range(f * (j - r), f * (j + 1 + r)):
                    if 0 <= y < H and 0 <= x < W and not k[y][x]:
                        ok = False
            out[i, j] = 1.0 if ok else 0.0
    return out


def visit_list(window, keep_vol: torch.Tensor):
    """window: the loop values m of the un-edited slice loop (python indexing: -1 is the last slice); keep_vol bool [D, H, W].
    -> (the m that are visited: those whose slice is not kept entirely, in the window's order; per visited m, True if mixed = the slice
    has a kept pixel, False if free)."""
    D = keep_vol.shape[0]
    k = keep_vol.bool().flatten(1)
    visit = [m for m in window if not bool(k[m % D].all())]
    return visit, [bool(k[m % D].any()) for m in visit]


def oracle_window(wholemask: torch.Tensor):
    """The loop values of oracle.samplers.autoregressive_slices for wholemask [1, 1, D, H, W]."""
    nz = torch.where(wholemask.sum((0, 1, 3, 4)))[0]
    return list(range(int(nz[0]) - 1, int(nz[-1]) + 1))


def ddim_sample_blend(eps_model, x_T, alphas_cumprod_f32, steps, x0=None, mask=None, q_noise=None, T=1000):
    """oracle.samplers.ddim_sample at eta = 0 with the blend of ddim.py:144-148 before each step when mask is given: q_sample (ddpm.py:
    q_sample, the fp32 buffers sqrt(alphas_cumprod) / sqrt(1 - alphas_cumprod) made from fp64) with the tape's noise q_noise[i]."""
    sch = S.ddim_schedule(alphas_cumprod_f32, steps, 0.0, T)
    ts = sch["timesteps"]
    total = ts.shape[0]
    ac64 = alphas_cumprod_f32.double().cpu()
    sa, s1 = ac64.sqrt().float(), (1.0 - ac64).sqrt().float()
    img = x_T
    zero = torch.zeros_like(x_T)
    for i, step in enumerate(np.flip(ts)):
        index = total - i - 1
        t = torch.full((img.shape[0],), int(step), dtype=torch.long)
        if mask is not None:
            img_orig = sa[int(step)] * x0 + s1[int(step)] * q_noise[i]
            img = img_orig * mask + (1.0 - mask) * img
        e_t = eps_model(img, t)
        img, _ = S.ddim_step(img, e_t, sch["alphas"][index], sch["alphas_prev"][index], sch["sigmas"][index], sch["sqrt_one_minus_alphas"][index], zero)
    return img


def edited_slices(cond_encode, first_stage_encode_mode, eps_model_for, decode, wholemask, known, keep, x_T_list, q_noise_list,
                  alphas_cumprod_f32, steps, f, r, scale_factor=1.0):
    """The edited slice loop of one volume.  wholemask [1, 1, D, H, W] (label / 255); known fp32, keep bool [D, H, W]; x_T_list: one
    [1, C, h, w] per visited slice; q_noise_list: one [S, 1, C, h, w] per mixed slice; both in loop order.  -> samples [1, 1, D, H, W]."""
    keep = keep.bool()
    samples = torch.where(keep, known.float(), torch.zeros_like(known, dtype=torch.float32))[None, None].clone()
    visit, mixed = visit_list(oracle_window(wholemask), keep)
    xs, qs = iter(x_T_list), iter(q_noise_list)
    for m, mx in zip(visit, mixed):
        concat_cond = torch.cat([samples[:, :, max(0, m - 1)], wholemask[:, :, m]], dim=1)
        c = cond_encode(concat_cond)
        x_T = next(xs).float()
        if mx:
            x0 = scale_factor * first_stage_encode_mode(known[m][None, None].float())
            lm = latent_keep_mask(keep[m], f, r)[None, None]
            z = ddim_sample_blend(eps_model_for(c), x_T, alphas_cumprod_f32, steps, x0, lm, next(qs).float())
        else:
            z = ddim_sample_blend(eps_model_for(c), x_T, alphas_cumprod_f32, steps)
        ds = decode(z)
        samples[:, :, m] = torch.where(keep[m], known[m].float(), S.slice_minmax_normalise(ds)[0, 0])[None, None]
    return samples


def edited_slices_on_state_dict(sd_all, wholemask, known, keep, x_T_list, q_noise_list, steps, alphas_cumprod, model_channels, f, r,
                                head_channels=32, scale_factor=1.0):
    """edited_slices on a LatentDiffusion state_dict, as util.oracle_slice_loop runs the un-edited loop."""
    sd_unet, sd_fs, sd_cs = (O.sub_state_dict(sd_all, p) for p in ("model.diffusion_model.", "first_stage_model.", "cond_stage_model."))
    return edited_slices(lambda cc: O.ae_encode_mode(sd_cs, cc), lambda x: O.ae_encode_mode(sd_fs, x),
                         lambda c: (lambda x, t: O.unet_forward(sd_unet, torch.cat([x, c], 1), t, model_channels=model_channels, head_channels=head_channels)),
                         lambda z: O.ae_decode(sd_fs, z / scale_factor), wholemask, known, keep, x_T_list, q_noise_list, alphas_cumprod, steps,
                         f, r, scale_factor)
