"""Generates tests/golden/losses.npz from the REFERENCE on CPU: the held-out objectives.

CCDM (ccdm/ddpm/models/diffusion_denoising.py:73-103, one_hot_categorical.py, trainer.py:298-327): q_xt_given_x0 / q_xt_given_xtm1 probs
and the labels their .sample() draws under a seed (the exponential tape is the same draw from a generator of that seed, as in
make_golden.py fx_posterior), theta_post, and the KL / CE sums of train_step written out here over the reference's DiffusionModel --
teacher-forced (softmax of recorded logits) for K = 14, K = 3 (3-D, 5x6x7) and K = 5 (2-D, 9x11), and through the small CCDM UNet
("ccdm_small." weights, K = 6, 8^3), each with unit and with non-uniform class weights.
LDM (ldm/models/diffusion/ddpm.py:160-170,205-215,275-322,883-892,1011-1058): lvlb_weights for eps and x0, q_mean_variance, q_sample,
_prior_bpd, the per-sample means of get_loss, DDPM.p_losses and LatentDiffusion.p_losses dicts for l1 / l2, eps / x0,
original_elbo_weight 0 / 1, learn_logvar off / on with the non-zero logvar of losses_ref.LOGVAR, a cross-attention model, forward() with
cond_stage_trainable, and validation_step's two passes with an EMA that differs from the weights.

Per reduction the fp64 value of tests/losses_ref.py is recorded next to the reference's fp32 one, and their relative distance: the kernels
are held to 4x the largest such distance (`tol_ccdm_step_loss`; `tol_loss_rows` for l1 / l2 and `tol_loss_rows_prior` for the prior
term, whose cancellation sets a scale of its own).  Per race the relative gap of the two best quotients
is recorded, and asserted to exceed 2^-20 on every voxel: no draw of the fixture is undecidable.

The reference's constructor cannot be called with learn_logvar=True (ddpm.py:115 passes `device=` to nn.Parameter); those cases set the
attribute after construction.  Its forward() draws t with torch.randint, which is replaced by the recorded t for that call.

Run only in the build container (needs the reference tree, like make_golden.py):
    python tests/golden/make_golden_losses.py [OUT_DIR]
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import unittest.mock as mock

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

sys.path.insert(0, os.path.join(MG.ROOT, "tests"))
import losses_ref as R  # noqa: E402

from jointimagegeneration_amd.synth import randomize_parameters  # noqa: E402

torch.set_grad_enabled(False)
SEED = MG.SEED
CCDM_CASES = (("k14", 14, 3, (5, 6, 7), (1, 50)), ("k3", 3, 3, (5, 6, 7), (50, 1)), ("k5_2d", 5, 2, (9, 11), (2, 37)))
GRID = [(lt, par, w, lv) for lt in ("l1", "l2") for par in ("eps", "x0") for w in (0.0, 1.0) for lv in (False, True)]
L_SIMPLE = 0.7


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def h(t):
    return t.half().float()


def rel(a, b):
    a, b = R.f64(a), R.f64(b)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def weights(K):
    return h(0.5 + torch.arange(K, dtype=torch.float32) / K)


def cl(x):
    """NC[D]HW -> [N, S, C] numpy."""
    return np.moveaxis(x.numpy(), 1, -1).reshape(x.shape[0], -1, x.shape[1])


def draw(oh, probs_bchw, seed, M, K):
    """The reference's .sample() under a seed, and the exponential tape that is the same draw."""
    torch.manual_seed(seed)
    lab = oh.OneHotCategoricalBCHW(probs=probs_bchw).sample().argmax(dim=1)
    return lab, torch.empty(M, K).exponential_(1, generator=MG.g(seed))


def trainer_sums(dmod, xt, x0, x0pred, t, cw):
    """trainer.py:305-327 on given tensors; per-sample fp32 sums [N, 2] and the three batch values."""
    q_true = dmod.theta_post(xt, x0, t)
    q_pred = dmod.theta_post_prob(xt, x0pred, t)
    mask = cw[x0.argmax(dim=1)]
    kl = torch.nn.functional.kl_div(torch.log(torch.clamp(q_pred, min=1e-12)), q_true, reduction="none").sum(dim=1) * mask
    ce = torch.nn.functional.cross_entropy(x0pred, x0.argmax(1), reduction="none")
    B = x0.shape[0]
    loss_kl, loss_ce = torch.sum(kl) / B, torch.sum(ce) / B
    return torch.stack([kl.flatten(1).sum(1), ce.flatten(1).sum(1)], 1), torch.stack([loss_kl, loss_ce, loss_kl + loss_ce])


def fx_ccdm(dd, oh, un, out):
    worst = 0.0
    for tag, K, dims, sp, tv in CCDM_CASES:
        gen = MG.g(900 + K)
        dmod = dd.DiffusionModel("cosine", R.CCDM_T, K, dims=dims)
        N, M = 2, 2 * int(np.prod(sp))
        t = torch.tensor(tv)
        lab0 = torch.randint(0, K, (N,) + sp, generator=gen)
        x0 = MG.S.one_hot_bchw(lab0, K)
        for name, fn, keep, seed in (("qx0", dmod.q_xt_given_x0, torch.stack([dmod.cumalphas[t - 1], 1 - dmod.cumalphas[t - 1]], 1), 300 + K),
                                     ("qxtm1", dmod.q_xt_given_xtm1, torch.stack([1 - dmod.betas[t - 1], dmod.betas[t - 1]], 1), 400 + K)):
            dist = fn(x0, t)
            lab, E = draw(oh, dist.probs.permute((0, dims + 1) + tuple(range(1, dims + 1))), seed, M, K)
            mine, gap = R.race(R.keep_probs(lab0.numpy(), keep[:, 0], keep[:, 1], K), E)
            assert np.array_equal(mine, R.rows(lab.numpy())), f"{tag} {name}: the race restatement disagrees with the reference's draw"
            assert float(gap.min()) > R.GAP_MIN, f"{tag} {name}: an undecidable race in the fixture (gap {gap.min():.3e})"
            out.update({f"{tag}_{name}_probs": dist.probs.clone(), f"{tag}_{name}_E": E, f"{tag}_{name}_labels": lab.int(),
                        f"{tag}_{name}_gap": gap.astype(np.float32), f"{tag}_{name}_mix": keep.clone()})
        xt_lab = torch.from_numpy(out[f"{tag}_qx0_labels"].numpy().astype(np.int64))
        xt = MG.S.one_hot_bchw(xt_lab, K)
        out[f"{tag}_x0"], out[f"{tag}_t"] = lab0.int(), t
        out[f"{tag}_theta_post"] = dmod.theta_post(xt, x0, t)
        logits = h(2.0 * torch.randn((N, K) + sp, generator=gen))
        out[f"{tag}_logits"] = logits
        scal = R.step_scalars(dmod.alphas, dmod.cumalphas, tv)
        for wtag, cw in (("ones", torch.ones(K)), ("cw", weights(K))):
            per, batch = trainer_sums(dmod, xt, x0, torch.softmax(logits, dim=1), t, cw)
            want = R.ccdm_step_loss(cl(logits), xt_lab.numpy(), lab0.numpy(), scal, cw, K)
            d = rel(per, want)
            worst = max(worst, d)
            print(f"  ccdm {tag} {wtag}: reference fp32 vs fp64 rel {d:.3e}")
            out.update({f"{tag}_{wtag}_sums": per, f"{tag}_{wtag}_sums_f64": want, f"{tag}_{wtag}_batch": batch, f"{tag}_{wtag}_dist": np.asarray(d)})
        out[f"{tag}_class_weights"] = weights(K)
    out["tol_ccdm_step_loss"] = np.asarray(4.0 * worst)
    print(f"  gg_ccdm_step_loss bound: 4 x {worst:.3e} = {4 * worst:.3e}")

    # ---- whole path: the small CCDM UNet, N = 2 with different t, 8^3 voxels, one image channel
    K = R.CCDM_K
    u = un.create_unet_openai(image_size=16, in_channels=K + 1, out_channels=K, num_res_blocks=2, cond_encoded_shape=None, dims=3,
                              **MG.CCDM_SMALL).eval()
    randomize_parameters(u, SEED, "ccdm_small.")
    dmod = dd.DiffusionModel("cosine", R.CCDM_T, K, dims=3)
    gen = MG.g(977)
    t = torch.tensor([1, 33])
    lab0 = torch.randint(0, K, (2, 8, 8, 8), generator=gen)
    cond = h(torch.rand(2, 1, 8, 8, 8, generator=gen))
    x0 = MG.S.one_hot_bchw(lab0, K)
    dist = dmod.q_xt_given_x0(x0, t)
    lab, E = draw(oh, dist.probs.permute(0, 4, 1, 2, 3), 555, 2 * 512, K)
    mine, gap = R.race(R.keep_probs(lab0.numpy(), dmod.cumalphas[t - 1], 1 - dmod.cumalphas[t - 1], K), E)
    assert np.array_equal(mine, R.rows(lab.numpy())) and float(gap.min()) > R.GAP_MIN
    xt = MG.S.one_hot_bchw(lab, K)
    x0pred = u(xt.contiguous(), cond.contiguous(), None, t)["diffusion_out"]
    out.update(net_x0=lab0.int(), net_cond=cond, net_t=t, net_E=E, net_xt=lab.int(), net_x0pred=x0pred, net_class_weights=weights(K))
    for wtag, cw in (("ones", torch.ones(K)), ("cw", weights(K))):
        per, batch = trainer_sums(dmod, xt, x0, x0pred, t, cw)
        out.update({f"net_{wtag}_sums": per, f"net_{wtag}_batch": batch})


def reference_ldm(dm, prefix="ldm_pipe.", unet=None, timesteps=R.LDM_T, **kw):
    cfg_unet = dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(unet or MG.LDM_SMALL))
    ae = lambda cin: dict(target="ldm.models.autoencoder.AutoencoderKL",
                          params=dict(embed_dim=4, dims=2, ddconfig=dict(MG.AE_SMALL, in_channels=cin, out_ch=cin), lossconfig=dict(target="torch.nn.Identity")))
    args = dict(first_stage_config=ae(1), cond_stage_config=ae(2), unet_config=cfg_unet, linear_start=0.0015, linear_end=0.0195,
                timesteps=timesteps, image_size=8, channels=4, dims=2, first_stage_key="image", cond_stage_key="mask", num_timesteps_cond=1)
    args.update(kw)
    with quiet():
        m = dm.LatentDiffusion(**args).eval()
    randomize_parameters(m, SEED, prefix)
    m.logvar.copy_(R.LOGVAR(timesteps))
    return m


def reference_ddpm(dm, **kw):
    cfg_unet = dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(MG.LDM_SMALL, in_channels=4))
    with quiet():
        m = dm.DDPM(unet_config=cfg_unet, timesteps=20, linear_start=0.0015, linear_end=0.0195, image_size=8, channels=4, **kw).eval()
    randomize_parameters(m, SEED, "ddpm_pix.")
    return m


def set_ema(m, prefix="ema_shadow."):
    """losses_ref.set_ema on the reference's LitEma (which has no reset_from)."""
    keep = {k: v.detach().clone() for k, v in m.model.named_parameters()}
    randomize_parameters(m.model, SEED, prefix)
    shadow = dict(m.model_ema.named_buffers())
    for k, p in m.model.named_parameters():
        if p.requires_grad:
            shadow[m.model_ema.m_name2s_name[k]].copy_(p)
        p.copy_(keep[k])


def keep_dict(out, tag, d):
    for k, v in d.items():
        out[f"{tag}|{k}"] = v.detach().clone().reshape(())


def fx_ldm(dm, out):
    gen = MG.g(4242)
    # ---- teacher-forced reductions: N = 3, C = 4, 8x8 and 4x4x4
    d20 = reference_ddpm(dm)
    worst = worst_prior = 0.0
    for tag, sp in (("2d", (8, 8)), ("3d", (4, 4, 4))):
        pred, target = h(torch.randn((3, 4) + sp, generator=gen)), h(torch.randn((3, 4) + sp, generator=gen))
        out.update({f"rows_{tag}_pred": pred, f"rows_{tag}_target": target})
        for lt in ("l1", "l2"):
            d20.loss_type = lt
            per = d20.get_loss(pred, target, mean=False).flatten(1).mean(1)
            if tag == "2d":
                assert torch.equal(per, d20.get_loss(pred, target, mean=False).mean(dim=[1, 2, 3]))
            want = R.loss_rows(lt, pred, target)
            d = rel(per, want)
            worst = max(worst, d)
            print(f"  loss_rows {tag} {lt}: reference fp32 vs fp64 rel {d:.3e}")
            out.update({f"rows_{tag}_{lt}": per, f"rows_{tag}_{lt}_f64": want, f"rows_{tag}_{lt}_dist": np.asarray(d)})
        x = h(1.5 * torch.randn((3, 4) + sp, generator=gen))
        m1000 = reference_ldm(dm)
        bpd = m1000._prior_bpd(x)
        want = R.prior_kl(x, m1000.sqrt_alphas_cumprod[-1], m1000.log_one_minus_alphas_cumprod[-1]) / np.log(2.0)
        d = rel(bpd, want)
        worst_prior = max(worst_prior, d)
        print(f"  _prior_bpd {tag}: reference fp32 vs fp64 rel {d:.3e}")
        out.update({f"rows_{tag}_x": x, f"rows_{tag}_prior_bpd": bpd, f"rows_{tag}_prior_bpd_f64": want, f"rows_{tag}_prior_dist": np.asarray(d)})
    out["tol_loss_rows"], out["tol_loss_rows_prior"] = np.asarray(4.0 * worst), np.asarray(4.0 * worst_prior)
    print(f"  gg_loss_rows bounds: l1 / l2 4 x {worst:.3e} = {4 * worst:.3e}, prior_kl 4 x {worst_prior:.3e} = {4 * worst_prior:.3e}")

    # ---- schedule-side values
    m = reference_ldm(dm)
    mx0 = reference_ldm(dm, parameterization="x0")
    out.update(lvlb_eps_1000=m.lvlb_weights.clone(), lvlb_x0_1000=mx0.lvlb_weights.clone(), lvlb_eps_20=d20.lvlb_weights.clone(),
               lvlb_x0_20=reference_ddpm(dm, parameterization="x0").lvlb_weights.clone())
    assert "lvlb_weights" not in m.state_dict()
    t = torch.tensor([0, 999, 500])
    x = h(torch.randn(3, 4, 8, 8, generator=gen))
    noise = h(torch.randn(3, 4, 8, 8, generator=gen))
    mean, var, logv = m.q_mean_variance(x, t)
    out.update(ldm_x=x, ldm_noise=noise, ldm_t=t, qmv_mean=mean, qmv_var=var.expand(x.shape).clone(), qmv_logvar=logv.expand(x.shape).clone(),
               q_sample=m.q_sample(x, t, noise))
    concat_cond = torch.rand(3, 2, 32, 32, generator=gen)
    c = m.get_learned_conditioning(concat_cond)
    out.update(ldm_concat_cond=concat_cond, ldm_c=c)

    # ---- LatentDiffusion.p_losses: the grid, one model per parameterization (the options are attributes there)
    for par, mm in (("eps", m), ("x0", mx0)):
        mm.l_simple_weight = L_SIMPLE
        model_out = mm.apply_model(mm.q_sample(x, t, noise), t, c)
        out[f"ldm_{par}_out_absmax"] = model_out.abs().max()
        for lt in ("l1", "l2"):
            mm.loss_type = lt
            out[f"ldm_{lt}_{par}_per"] = mm.get_loss(model_out, noise if par == "eps" else x, mean=False).mean([1, 2, 3])
    for lt, par, w, lv in GRID:
        mm = m if par == "eps" else mx0
        mm.loss_type, mm.original_elbo_weight, mm.learn_logvar = lt, w, lv
        loss, d = mm.p_losses(x, c, t, noise=noise)
        assert torch.equal(loss, d["val/loss"]) and (("val/loss_gamma" in d) == lv)
        keep_dict(out, f"ldm_{lt}_{par}_w{int(w)}_lv{int(lv)}", d)
    m.loss_type, m.original_elbo_weight, m.learn_logvar, m.l_simple_weight = "l2", 0.0, False, 1.0

    # ---- forward() with cond_stage_trainable: the raw conditioning goes through the cond stage; t replayed
    m.cond_stage_trainable = True
    with mock.patch.object(dm.torch, "randint", lambda *a, **k: t.clone()):
        _, d = m(x, concat_cond, noise=noise)
    m.cond_stage_trainable = False
    keep_dict(out, "ldm_forward_trainable", d)

    # ---- validation_step's two passes with an EMA that differs from the weights
    set_ema(m)
    _, plain = m.p_losses(x, c, t, noise=noise)
    with m.ema_scope():
        _, ema = m.p_losses(x, c, t, noise=noise)
        mo = m.apply_model(m.q_sample(x, t, noise), t, c)
        out.update(ldm_val_out_absmax_ema=mo.abs().max(), ldm_val_per_ema=m.get_loss(mo, noise, mean=False).mean([1, 2, 3]))
    assert not torch.equal(plain["val/loss"], ema["val/loss"])
    keep_dict(out, "ldm_val", {**plain, **{k + "_ema": v for k, v in ema.items()}})

    # ---- cross-attention conditioning
    ae = dict(target="ldm.models.autoencoder.AutoencoderKL",
              params=dict(embed_dim=4, dims=2, ddconfig=dict(MG.AE_SMALL), lossconfig=dict(target="torch.nn.Identity")))
    cfg_unet = dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel",
                    params=dict(MG.LDM_SMALL, in_channels=4, use_spatial_transformer=True, transformer_depth=1, context_dim=48))
    with quiet():
        mx = dm.LatentDiffusion(first_stage_config=ae, cond_stage_config="__is_first_stage__", unet_config=cfg_unet, linear_start=0.0015,
                                linear_end=0.0195, timesteps=R.LDM_T, image_size=8, channels=4, dims=2, conditioning_key="crossattn",
                                num_timesteps_cond=1).eval()
    randomize_parameters(mx, SEED, "ldm_xattn.")
    ctx = h(torch.randn(3, 5, 48, generator=gen))
    mo = mx.apply_model(mx.q_sample(x, t, noise), t, ctx)
    out.update(xattn_ctx=ctx, xattn_out_absmax=mo.abs().max(), xattn_per=mx.get_loss(mo, noise, mean=False).mean([1, 2, 3]))
    keep_dict(out, "xattn", mx.p_losses(x, ctx, t, noise=noise)[1])

    # ---- DDPM.p_losses on the pixel-space model: l1 / l2, eps / x0, original_elbo_weight 0 / 1
    t20 = torch.tensor([0, 19, 7])
    out["ddpm_t"] = t20
    for par in ("eps", "x0"):
        d = reference_ddpm(dm, parameterization=par, l_simple_weight=L_SIMPLE)
        mo = d.model(d.q_sample(x, t20, noise), t20)
        out[f"ddpm_{par}_out_absmax"] = mo.abs().max()
        for lt in ("l1", "l2"):
            d.loss_type = lt
            out[f"ddpm_{lt}_{par}_per"] = d.get_loss(mo, noise if par == "eps" else x, mean=False).mean(dim=[1, 2, 3])
            for w in (0.0, 1.0):
                d.original_elbo_weight = w
                keep_dict(out, f"ddpm_{lt}_{par}_w{int(w)}", d.p_losses(x, t20, noise=noise)[1])


def main(out_dir):
    dd, oh, un, _unet, _nn = MG.import_ccdm()
    _om, _at, _mo, _ae, dm, _di, _ut = MG.import_ldm()
    out = {}
    fx_ccdm(dd, oh, un, out)
    fx_ldm(dm, out)
    arrs = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "losses.npz")
    np.savez_compressed(path, **arrs)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB, {len(arrs)} arrays)")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else MG.OUT)
