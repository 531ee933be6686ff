"""Generates tests/golden/progressive.npz and progressive_surface.json from the REFERENCE on CPU: the logged lists of its samplers
(ddim.py:134-162, plms.py:134-168, ddpm.py:254-266,1123-1227), the x0 / clip_denoised variants of the ancestral step through DDPM and
LatentDiffusion, the 13 schedule buffers of the cosine / sqrt_linear / sqrt / given_betas schedules, and the timesteps each loop logs.
Models: the small LatentDiffusion of make_golden_inpaint.py ("ldm_pipe." weights, 8x8 latent, N = 2), its 20-timestep twin, and a
20-timestep pixel-space DDPM on the same UNet with 4 input channels ("ddpm_pix." weights).

Run only in the build container (needs the reference tree, like make_golden.py):
    python tests/golden/make_golden_progressive.py [OUT_DIR]
Random draws come from recorded fp16-exact tapes, as in make_golden_inpaint.py: q_sample's randn_like <- q_tape, torch.randn <- step_tape
(DDPM.p_sample_loop draws its x_T through torch.randn too: x_T is put in front of the tape there).

The reference's cosine branch calls np.clip on a torch tensor (util.py:35).  Where this numpy / torch pair refuses that, the cosine betas
are taken from the same formula in fp64 (recorded in `cosine_from_reference` = 0) and handed to the reference's register_schedule as
given_betas, so the 13 buffers are still the reference's arithmetic.
"""
from __future__ import annotations

import contextlib
import io
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402
import make_golden_inpaint as MI  # noqa: E402

from jointimagegeneration_amd.synth import randomize_parameters  # noqa: E402

torch.set_grad_enabled(False)
SEED = MG.SEED
N, C, H, W = MI.N, MI.C, MI.H, MI.W
BUFFERS = ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
           "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_variance",
           "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2")          # + logvar = 13
LOG_T = (1, 2, 5, 20)
LOG_K = (1, 3, 100)
LOG_S = (1, 2, 5, 15, 20)     # DDIM / PLMS on 1000 timesteps: S = 15 does not divide them, and the uniform schedule then holds 16 steps


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def ldm_variant(dm, timesteps, **kw):
    cfg_unet = dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(MG.LDM_SMALL))
    ae = lambda cin: dict(target="ldm.models.autoencoder.AutoencoderKL",
                          params=dict(embed_dim=4, dims=2, ddconfig=dict(MG.AE_SMALL, in_channels=cin, out_ch=cin), lossconfig=dict(target="torch.nn.Identity")))
    with quiet():
        m = dm.LatentDiffusion(first_stage_config=ae(1), cond_stage_config=ae(2), unet_config=cfg_unet, linear_start=0.0015,
                               linear_end=0.0195, timesteps=timesteps, image_size=8, channels=4, dims=2, first_stage_key="image",
                               cond_stage_key="mask", num_timesteps_cond=1, **kw).eval()
    randomize_parameters(m, SEED, "ldm_pipe.")
    return m


def pixel_ddpm(dm, **kw):
    cfg_unet = dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(MG.LDM_SMALL, in_channels=4))
    with quiet():
        m = dm.DDPM(unet_config=cfg_unet, timesteps=20, linear_start=0.0015, linear_end=0.0195, image_size=8, channels=4, log_every_t=10,
                    **kw).eval()
    randomize_parameters(m, SEED, "ddpm_pix.")
    return m


def cosine_betas(n, s=8e-3):
    """util.py:27-35 in fp64, with the clip the reference asks numpy for."""
    t = torch.arange(n + 1, dtype=torch.float64) / n + s
    a = torch.cos(t / (1 + s) * np.pi / 2).pow(2)
    a = a / a[0]
    return np.clip((1 - a[1:] / a[:-1]).numpy(), 0, 0.999)


def schedule_buffers(m, out, tag, **kw):
    m.register_schedule(**kw)
    for b in BUFFERS:
        out[f"sched_{tag}_{b}"] = getattr(m, b).clone()


def stack(lst):
    return torch.stack([t.clone() for t in lst])


def logged_timesteps(m, m1000, di, pl, out):
    """Which loop values each sampler logs: the step functions are replaced by ones that return the timestep / index as the value."""
    shape = (N, C, H, W)

    def p_sample(img, cond, ts, return_x0=False, **kw):
        v = torch.full_like(img, float(ts[0]))
        return (v, v) if return_x0 else v
    m.p_sample = p_sample
    for T in LOG_T:
        for k in LOG_K:
            _, inter = m.p_sample_loop(None, shape, return_intermediates=True, x_T=torch.full(shape, -1.0), verbose=False, timesteps=T,
                                       log_every_t=k)
            out[f"idx_p_sample_loop_{T}_{k}"] = np.asarray([int(t.flatten()[0]) for t in inter], dtype=np.int64)
            _, inter = m.progressive_denoising(None, shape, verbose=False, x_T=torch.full(shape, -1.0), start_T=T, log_every_t=k)
            out[f"idx_progressive_{T}_{k}"] = np.asarray([int(t.flatten()[0]) for t in inter], dtype=np.int64)
    del m.p_sample
    for name, cls, fn in (("ddim", di.DDIMSampler, "p_sample_ddim"), ("plms", pl.PLMSSampler, "p_sample_plms")):
        for S in LOG_S:
            for k in LOG_K:
                s = cls(m1000)

                def step(x, c, t, *a, index=None, **kw):
                    v = torch.full_like(x, float(index))
                    return (v, v) if fn == "p_sample_ddim" else (v, v, v)
                setattr(s, fn, step)
                with quiet():
                    _, inter = s.sample(S=S, batch_size=N, shape=(C, H, W), conditioning=None, verbose=False, x_T=torch.full(shape, -1.0),
                                        log_every_t=k, **(dict(dims=2) if name == "ddim" else {}))
                out[f"idx_{name}_{S}_{k}"] = np.asarray([int(t.flatten()[0]) for t in inter["x_inter"]], dtype=np.int64)


def main(out_dir):
    _om, _at, _mo, _ae, dm, di, ut = MG.import_ldm()
    pl = importlib.import_module("ldm.models.diffusion.plms")
    pl.PLMSSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)
    out = {}

    # ---- schedules: 13 buffers each (logvar is zeros [T]) on a 20-step model
    m20 = ldm_variant(dm, 20)
    try:
        ut.make_beta_schedule("cosine", 20)
        out["cosine_from_reference"] = np.asarray(1)
        schedule_buffers(m20, out, "cosine", beta_schedule="cosine", timesteps=20)
    except Exception as e:                                # np.clip(tensor, a_min=, a_max=) is refused by this numpy / torch pair
        print(f"reference cosine branch failed here ({type(e).__name__}: {e}); cosine betas from the formula")
        out["cosine_from_reference"] = np.asarray(0)
        schedule_buffers(m20, out, "cosine", given_betas=cosine_betas(20))
    schedule_buffers(m20, out, "sqrt_linear", beta_schedule="sqrt_linear", timesteps=20, linear_start=1e-4, linear_end=2e-2)
    schedule_buffers(m20, out, "sqrt", beta_schedule="sqrt", timesteps=20, linear_start=1e-4, linear_end=2e-2)
    given = np.linspace(1e-3, 0.3, 20, dtype=np.float64) ** 1.5
    out["given_betas"] = given
    schedule_buffers(m20, out, "given", given_betas=given)

    # ---- inputs and tapes: those of make_golden_inpaint.py, drawn again in its order and checked against inpaint.npz, which the tests read
    m = ldm_variant(dm, 1000)
    m20 = ldm_variant(dm, 20)
    gen = MG.g(2048)
    concat_cond = torch.rand(N, 2, 32, 32, generator=gen)
    x_T = torch.randn(N, C, H, W, generator=gen)
    c = m.get_learned_conditioning(concat_cond)
    gi = MG.g(777)
    x0 = torch.randn(N, C, H, W, generator=gi)
    torch.rand(N, C, H, W, generator=gi)                                 # the soft mask of inpaint.npz, not used here
    q_tape, step_tape = MI.tape(gi, 20), MI.tape(gi, 20)
    hole = MI.centre_hole()
    have = np.load(os.path.join(MG.OUT, "inpaint.npz"))
    for k, v in (("c", c), ("x_T", x_T), ("x0", x0), ("mask_hole", hole), ("q_tape", q_tape), ("step_tape", step_tape)):
        assert np.array_equal(np.asarray(have[k], dtype=np.float32), v.numpy()), f"inpaint.npz[{k}] is not what this generator drew"
    temps = [0.5 + 0.05 * i for i in range(20)]                         # indexed by the timestep value (ddpm.py:1165)
    out.update(temperature=np.asarray(temps))
    shape = (N, C, H, W)

    # ---- ancestral loops on the 20-step model.  Stored: the lists without their leading x_T (asserted), the final img only where it is
    # not the last list entry (progressive_denoising logs predictions of x_0)
    def keep_loop(tag, z, inter):
        assert torch.equal(inter[0], x_T) and torch.equal(inter[-1], z)
        out[f"inter_{tag}"] = stack(inter[1:])

    def keep_prog(tag, z, inter):
        out.update({f"z_{tag}": z, f"inter_{tag}": stack(inter)})
    with MI.tapes(q_tape[:0], step_tape):
        keep_loop("loop3", *m20.p_sample_loop(c, shape, return_intermediates=True, x_T=x_T, verbose=False, log_every_t=3))
    with MI.tapes(q_tape[:0], step_tape):
        keep_prog("prog3", *m20.progressive_denoising(c, shape, verbose=False, x_T=x_T, log_every_t=3))
    with MI.tapes(q_tape, step_tape):
        keep_prog("prog_temp_mask", *m20.progressive_denoising(c, shape, verbose=False, x_T=x_T, log_every_t=10, temperature=temps, mask=hole, x0=x0))
    m20.clip_denoised = True
    with MI.tapes(q_tape[:0], step_tape):
        keep_prog("prog_clip", *m20.progressive_denoising(c, shape, verbose=False, x_T=x_T, log_every_t=10))
    m20.clip_denoised = False
    mx0 = ldm_variant(dm, 20, parameterization="x0")
    with MI.tapes(q_tape[:0], step_tape):
        keep_prog("prog_x0", *mx0.progressive_denoising(c, shape, verbose=False, x_T=x_T, log_every_t=10))
    mx0.clip_denoised = True
    with MI.tapes(q_tape[:0], step_tape):
        keep_loop("loop_x0_clip", *mx0.p_sample_loop(c, shape, return_intermediates=True, x_T=x_T, verbose=False, log_every_t=10))

    # ---- pixel-space DDPM (clip_denoised=True by default, log_every_t=10), eps and x0; its p_sample_loop draws x_T itself
    for tag, kw in (("eps", {}), ("x0", dict(parameterization="x0"))):
        d = pixel_ddpm(dm, **kw)
        assert d.clip_denoised is True
        with MI.tapes(q_tape[:0], torch.cat([x_T[None], step_tape])):
            keep_loop(f"ddpm_{tag}", *d.p_sample_loop(shape, return_intermediates=True))
        if tag == "eps":
            surf = [[k, list(v.shape)] for k, v in d.state_dict().items()]

    # ---- DDIM eta 0 / eta 1 and PLMS at S = 5 with log_every_t in {1, 2}.  The log_every_t = 2 lists are asserted to be the entries of the
    # log_every_t = 1 lists at index 4, 2, 0 (the same chain), so only the latter are stored
    def sampler_lists(tag, run):
        full = run(1)[1]
        assert torch.equal(full["x_inter"][0], x_T) and torch.equal(full["pred_x0"][0], x_T) and len(full["x_inter"]) == 6
        half = run(2)[1]
        for name in ("x_inter", "pred_x0"):
            assert len(half[name]) == 4 and all(torch.equal(a, b) for a, b in zip(half[name], [full[name][j] for j in (0, 1, 3, 5)]))
        out.update({f"xi_{tag}": stack(full["x_inter"][1:]), f"p0_{tag}": stack(full["pred_x0"][1:])})

    def ddim_run(eta):
        def run(k):
            with MI.tapes(q_tape[:0], step_tape[:5] if eta else None):
                return di.DDIMSampler(m).sample(S=5, batch_size=N, shape=(C, H, W), conditioning=c, verbose=False, x_T=x_T, dims=2,
                                                eta=eta, log_every_t=k)
        return run

    def plms_run(k):
        with MI.tapes(q_tape[:0], None):
            return pl.PLMSSampler(m).sample(S=5, batch_size=N, shape=(C, H, W), conditioning=c, verbose=False, x_T=x_T, log_every_t=k)
    sampler_lists("ddim_eta0", ddim_run(0.0))
    sampler_lists("ddim_eta1", ddim_run(1.0))
    sampler_lists("plms", plms_run)

    logged_timesteps(ldm_variant(dm, 20), m, di, pl, out)

    arrs = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "progressive.npz")
    np.savez_compressed(path, **arrs)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")
    with open(os.path.join(out_dir, "progressive_surface.json"), "w") as f:
        json.dump(dict(ddpm=surf), f)
    print(f"wrote progressive_surface.json ({len(surf)} entries)")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else MG.OUT)
