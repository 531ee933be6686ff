"""GPU suite of the held-out objectives (gg_loss.hip, losses.py, the p_losses family of ldm.py) against tests/golden/losses.npz, which
make_golden_losses.py recorded from the REFERENCE on the CPU, and against the fp64 restatement tests/losses_ref.py.

Teacher-forced kernel bounds (inputs fed directly, no network).  The generator measured how far the reference's own fp32 result lies
from the fp64 restatement, per case; a kernel gets 4x the largest distance of its kind (relative, per reduction):
    gg_ccdm_step_loss   reference 9.110e-4 (K = 3, t = 50: the KL of a late step is a small difference of O(1) terms)   bound 3.644e-3
    gg_loss_rows l1/l2  reference 6.901e-8                                                                                bound 2.760e-7
    gg_loss_rows prior  reference 1.732e-4 (-1 - lv + exp(lv) cancels to ~lv^2 / 2 at t = T - 1)                          bound 6.929e-4
Whole-path bounds are derived next to their assertions from what the existing suites allow a network output of that model and mode."""
import json
import os

import numpy as np
import pytest
import torch

import losses_ref as R
from util import CCDM_SMALL, T, gold

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL_CCDM_STEP_LOSS = 3.644e-3
TOL_LOSS_ROWS = 2.760e-7
TOL_LOSS_ROWS_PRIOR = 6.929e-4
# what the existing suites allow the networks' outputs (tests/test_unet_options_gpu.py, tests/test_hip_parity.py)
LDM_EPS_REL = {"bf16": 3e-2, "fp32": 2e-5}           # max |eps - ref| / max |ref|
CCDM_PROBS_ABS_BF16 = 1.5e-2                         # max |p - ref|
# fp32 validation mode of the CCDM path: no bound on the probabilities is stated by the existing suites for this network at these inputs,
# so the deviation of the sums from the fixture was measured (relative, per reduction) and twice that is allowed
CCDM_FP32_MEASURED = 6.812e-7                        # the weighted KL sum of the t = 33 sample (unit weights: 6.198e-7); the other sums lie below 8e-8
CCDM_CASES = (("k14", 14), ("k3", 3), ("k5_2d", 5))
GRID = [(lt, par, w, lv) for lt in ("l1", "l2") for par in ("eps", "x0") for w in (0.0, 1.0) for lv in (False, True)]
L_SIMPLE = 0.7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    f = gold("losses")
    for name, const in (("tol_ccdm_step_loss", TOL_CCDM_STEP_LOSS), ("tol_loss_rows", TOL_LOSS_ROWS), ("tol_loss_rows_prior", TOL_LOSS_ROWS_PRIOR)):
        assert abs(float(f[name]) / const - 1) < 1e-3, f"{name}: the fixture holds {float(f[name]):.4e}, the test states {const:.4e}"
    return f


def cl_rows(x, stride=32, fill=7.0):
    """NC[D]HW fp32 -> channels-last rows [N * S, stride] with a sentinel in the pad lanes."""
    N, C = x.shape[:2]
    rows = x.reshape(N, C, -1).permute(0, 2, 1).reshape(-1, C)
    out = torch.full((rows.shape[0], stride), fill, dtype=torch.float32, device=x.device)
    out[:, :C] = rows
    return out


def fixture_dict(g, tag):
    return {k.split("|", 1)[1]: float(g[k]) for k in g.files if k.startswith(tag + "|")}


# ------------------------------------------------------------------------------------------------ gg_q_sample_rows
@pytest.mark.parametrize("sp", [(8, 8), (4, 4, 4), (5, 6, 7)], ids=["8x8", "4x4x4", "5x6x7"])
def test_q_sample_rows_is_bit_equal_to_q_sample_on_the_cpu(dev, g, sp):
    from jointimagegeneration_amd import ops
    m = R.ldm_loss_model()
    t = T(g["ldm_t"])                                                             # 0, T - 1 and one between
    if sp == (8, 8):
        x, noise, want = T(g["ldm_x"]), T(g["ldm_noise"]), T(g["q_sample"])       # the reference's own q_sample
        assert torch.equal(m.q_sample(x, t, noise), want)
    else:
        gen = torch.Generator().manual_seed(sum(sp))
        x, noise = torch.randn((3, 4) + sp, generator=gen), torch.randn((3, 4) + sp, generator=gen)
        want = m.q_sample(x, t, noise)
    scal = torch.stack([m.sqrt_alphas_cumprod[t], m.sqrt_one_minus_alphas_cumprod[t]], 1).contiguous().to(dev)
    S = int(np.prod(sp))
    want_rows = want.reshape(3, 4, S).permute(0, 2, 1).reshape(-1, 4)
    out = ops.q_sample_rows(x.to(dev), noise.to(dev), scal)
    assert torch.equal(out.cpu(), want)
    for dtype in (torch.bfloat16, torch.float32):
        uin = torch.full((3 * S, 32), 7.0, dtype=dtype, device=dev)
        out2 = torch.empty_like(out)
        ops.q_sample_rows(x.to(dev), noise.to(dev), scal, out=out2, unet_in=uin)
        assert torch.equal(out2, out)
        assert torch.equal(uin[:, :4].cpu(), want_rows.to(dtype)) and bool((uin[:, 4:] == 7.0).all())


# ------------------------------------------------------------------------------------------------ gg_ccdm_q_sample
@pytest.mark.parametrize("tag,K", CCDM_CASES)
@pytest.mark.parametrize("name", ["qx0", "qxtm1"])
def test_ccdm_q_sample_labels_equal_the_reference_on_every_decidable_voxel(dev, g, tag, K, name):
    from jointimagegeneration_amd import ops
    x0 = T(g[f"{tag}_x0"]).to(dev).contiguous()
    mix, E = T(g[f"{tag}_{name}_mix"]).to(dev).contiguous(), T(g[f"{tag}_{name}_E"]).to(dev)
    M = x0.numel()
    oh = torch.full((M, 32), 7.0, dtype=torch.bfloat16, device=dev)
    lab = ops.ccdm_q_sample(x0.view(-1), mix, K, E=E, onehot_out=oh)
    decidable = T(g[f"{tag}_{name}_gap"]).reshape(-1) > R.GAP_MIN
    left_out = int((~decidable).sum())
    assert left_out * 10000 <= M                                                  # at most 1 voxel in 10 000 (the generator left out none)
    want = T(g[f"{tag}_{name}_labels"]).reshape(-1)
    mism = int((lab.cpu()[decidable] != want[decidable]).sum())
    print(f"{tag} {name}: {mism} mismatches on {int(decidable.sum())} decidable voxels, {left_out} left out")
    assert mism == 0
    assert torch.equal(oh[:, :K].float().argmax(1).int(), lab) and bool((oh[:, :K].float().sum(1) == 1).all()) and bool((oh[:, K:] == 7.0).all())


def test_ccdm_q_sample_philox_is_reproducible_and_per_sample(dev, g):
    """One key per sample and the row within the sample as the counter: a sample's draw does not depend on its batch slot."""
    from jointimagegeneration_amd import ops
    K = 14
    x0, mix = T(g["k14_x0"]).to(dev).contiguous(), T(g["k14_qx0_mix"]).to(dev).contiguous()
    keys = ops.philox_seed_tensor([5, (1 << 63) + 9], dev)
    a = ops.ccdm_q_sample(x0.view(-1), mix, K, philox_seeds=keys)
    b = ops.ccdm_q_sample(x0.view(-1), mix, K, philox_seeds=keys)
    assert torch.equal(a, b)
    rows = x0[0].numel()
    second = ops.ccdm_q_sample(x0[1].reshape(-1), mix[1:].contiguous(), K, philox_seeds=keys[1:].contiguous())
    assert torch.equal(second, a[rows:])
    assert float((a[:rows] == x0[0].reshape(-1)).float().mean()) > 0.98          # t = 1 keeps 99.98 % of the mass on x0
    assert 0.5 < float((a[rows:] != x0[1].reshape(-1)).float().mean())           # t = T: uniform, about 13 / 14 move
    off = torch.tensor([3], dtype=torch.int64, device=dev)
    assert not torch.equal(ops.ccdm_q_sample(x0.view(-1), mix, K, philox_seeds=keys, philox_offset=off)[rows:], a[rows:])
    with pytest.raises(ValueError, match="either an exponential tape E or philox_seeds"):
        ops.ccdm_q_sample(x0.view(-1), mix, K)
    with pytest.raises(RuntimeError, match=r"K=17 outside \[2, 16\]"):
        ops.ccdm_q_sample(x0.view(-1), mix, 17, philox_seeds=keys)


# ------------------------------------------------------------------------------------------------ gg_loss_rows
@pytest.mark.parametrize("tag", ["2d", "3d"])
def test_loss_rows_against_the_fp64_restatement(dev, g, tag):
    from jointimagegeneration_amd import ops
    pred, target, x = (T(g[f"rows_{tag}_{k}"]).to(dev) for k in ("pred", "target", "x"))
    N, C = pred.shape[:2]
    S = pred[0, 0].numel()
    rows = cl_rows(pred)
    for lt in ("l1", "l2"):
        got = ops.loss_rows(lt, N, C, S, pred=rows, target=target)
        err = float(np.abs(got.cpu().numpy() / g[f"rows_{tag}_{lt}_f64"] - 1).max())
        print(f"loss_rows {tag} {lt}: rel {err:.3e} vs fp64 (reference fp32: {float(g[f'rows_{tag}_{lt}_dist']):.3e}, bound {TOL_LOSS_ROWS:.3e})")
        assert err <= TOL_LOSS_ROWS
        assert torch.equal(got, ops.loss_rows(lt, N, C, S, pred=rows, target=target))          # two runs: the same bits
    m = R.ldm_loss_model()
    sc = torch.stack([m.sqrt_alphas_cumprod[-1], m.log_one_minus_alphas_cumprod[-1]]).repeat(N, 1).contiguous().to(dev)
    got = ops.loss_rows("prior_kl", N, C, S, x_start=x, scalars=sc)
    err = float(np.abs(got.cpu().numpy() / np.log(2.0) / g[f"rows_{tag}_prior_bpd_f64"] - 1).max())
    print(f"loss_rows {tag} prior_kl: rel {err:.3e} vs fp64 (reference fp32: {float(g[f'rows_{tag}_prior_dist']):.3e}, bound {TOL_LOSS_ROWS_PRIOR:.3e})")
    assert err <= TOL_LOSS_ROWS_PRIOR
    assert torch.equal(got, ops.loss_rows("prior_kl", N, C, S, x_start=x, scalars=sc))
    bpd = m.to(dev)._prior_bpd(x)                                                               # the method: per / log 2, fp32
    assert float(np.abs(bpd.cpu().numpy() / g[f"rows_{tag}_prior_bpd_f64"] - 1).max()) <= TOL_LOSS_ROWS_PRIOR + 2.0 ** -23


def test_loss_rows_over_several_workgroups_with_a_partial_last_one(dev):
    """N = 3, C = 3, S = 5 * 6 * 19 = 570 positions: three workgroups per sample, the last one partial; a stride that is no multiple of 4.
    Every thread still takes one trip of its loop (the grid is capped at 1024 workgroups per sample): the later trips run in
    tests/test_grid_caps_gpu.py::test_loss_rows_exact_integers and ::test_loss_rows_prior_kl."""
    from jointimagegeneration_amd import ops
    gen = torch.Generator().manual_seed(31)
    pred, target = (torch.randn(3, 3, 5, 6, 19, generator=gen).half().float() for _ in range(2))
    rows = cl_rows(pred.to(dev), stride=7)
    for lt in ("l1", "l2"):
        got = ops.loss_rows(lt, 3, 3, 570, pred=rows, target=target.to(dev))
        err = float(np.abs(got.cpu().numpy() / R.loss_rows(lt, pred, target) - 1).max())
        print(f"loss_rows 570 positions {lt}: rel {err:.3e} vs fp64")
        assert err <= TOL_LOSS_ROWS
        assert torch.equal(got, ops.loss_rows(lt, 3, 3, 570, pred=rows, target=target.to(dev)))
    with pytest.raises(RuntimeError, match="workspace"):
        ops.loss_rows("l2", 3, 3, 570, pred=rows, target=target.to(dev), workspace=torch.empty(2, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="unknown mode"):
        ops.loss_rows("huber", 3, 3, 570, pred=rows, target=target.to(dev))


def test_get_loss_mean_is_the_mean_of_the_per_sample_means(dev, g):
    m = R.ldm_loss_model().to(dev)
    pred, target = T(g["rows_2d_pred"]).to(dev), T(g["rows_2d_target"]).to(dev)
    for lt in ("l1", "l2"):
        m.loss_type = lt
        want = float(g[f"rows_2d_{lt}_f64"].mean())
        assert abs(float(m.get_loss(pred, target)) / want - 1) <= TOL_LOSS_ROWS + 2.0 ** -23      # + the fp32 result's own rounding
        assert torch.equal(m.get_loss(pred, target, mean=False), (target - pred).abs() if lt == "l1" else (target - pred) ** 2)


# ------------------------------------------------------------------------------------------------ gg_ccdm_step_loss
@pytest.mark.parametrize("tag,K", CCDM_CASES)
def test_ccdm_step_loss_against_the_fp64_restatement(dev, g, tag, K):
    """N = 2 with different t (t = 1 and t = T in the 3-D cases), 210 voxels per sample (99 in the 2-D case): one partial workgroup each."""
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.ccdm import DiffusionModel
    dims = 2 if tag.endswith("2d") else 3
    dm = DiffusionModel("cosine", R.CCDM_T, K, dims=dims)
    scal = dm.step_scalar_rows(T(g[f"{tag}_t"])).to(dev)
    logits = cl_rows(T(g[f"{tag}_logits"]).to(dev))
    xt, x0 = (T(g[k]).to(dev).contiguous().view(-1) for k in (f"{tag}_qx0_labels", f"{tag}_x0"))
    for wtag, cw in (("ones", torch.ones(K)), ("cw", T(g[f"{tag}_class_weights"]))):
        got = ops.ccdm_step_loss(logits, xt, x0, scal, cw.to(dev), K)
        err = float(np.abs(got.cpu().numpy() / g[f"{tag}_{wtag}_sums_f64"] - 1).max())
        print(f"ccdm_step_loss {tag} {wtag}: rel {err:.3e} vs fp64 (reference fp32: {float(g[f'{tag}_{wtag}_dist']):.3e}, bound {TOL_CCDM_STEP_LOSS:.3e})")
        assert err <= TOL_CCDM_STEP_LOSS
        assert torch.equal(got, ops.ccdm_step_loss(logits, xt, x0, scal, cw.to(dev), K))       # two runs: the same bits


def test_ccdm_step_loss_over_several_workgroups(dev):
    """K = 14, N = 2, 5 * 6 * 19 = 570 voxels per sample (three workgroups, the last partial), t = 1 and t = 27, against the restatement.
    Every thread still takes one trip of its loop: the later trips run in tests/test_grid_caps_gpu.py::test_ccdm_step_loss."""
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.ccdm import DiffusionModel
    K, gen = 14, torch.Generator().manual_seed(57)
    dm = DiffusionModel("cosine", R.CCDM_T, K, dims=3)
    t = torch.tensor([1, 27])
    logits = (2 * torch.randn(2, K, 5, 6, 19, generator=gen)).half().float()
    x0 = torch.randint(0, K, (2, 5, 6, 19), generator=gen)
    xt = x0.clone()
    xt[1] = torch.randint(0, K, (5, 6, 19), generator=gen)
    cw = (0.5 + torch.arange(K) / K).float()
    want = R.ccdm_step_loss(np.moveaxis(logits.numpy(), 1, -1).reshape(2, -1, K), xt.numpy(), x0.numpy(),
                            R.step_scalars(dm.alphas, dm.cumalphas, t.tolist()), cw, K)
    args = (cl_rows(logits.to(dev)), xt.int().to(dev).view(-1), x0.int().to(dev).view(-1), dm.step_scalar_rows(t).to(dev), cw.to(dev), K)
    got = ops.ccdm_step_loss(*args)
    err = float(np.abs(got.cpu().numpy() / want - 1).max())
    print(f"ccdm_step_loss 570 voxels: rel {err:.3e} vs fp64")
    assert err <= TOL_CCDM_STEP_LOSS
    assert torch.equal(got, ops.ccdm_step_loss(*args))


# ------------------------------------------------------------------------------------------------ Python surface of DiffusionModel
@pytest.mark.parametrize("tag,K", CCDM_CASES)
def test_diffusion_model_q_and_theta_post_match_the_reference(dev, g, tag, K):
    from jointimagegeneration_amd.ccdm import DiffusionModel
    dims = 2 if tag.endswith("2d") else 3
    dm = DiffusionModel("cosine", R.CCDM_T, K, dims=dims).to(dev)
    t = T(g[f"{tag}_t"]).to(dev)
    inv = (0, dims + 1) + tuple(range(1, dims + 1))
    x0 = torch.nn.functional.one_hot(T(g[f"{tag}_x0"]).long(), K).permute(inv).float().to(dev)
    for name, fn in (("qx0", dm.q_xt_given_x0), ("qxtm1", dm.q_xt_given_xtm1)):
        dist = fn(x0, t)
        ref = T(g[f"{tag}_{name}_probs"])
        assert tuple(dist.probs.shape) == tuple(ref.shape)
        assert bool(((dist.probs.cpu() - ref).abs() <= (2 * K + 3) * 2.0 ** -24 * ref).all())     # the roundings of the expression
        onehot = dist.sample(rng_tape=T(g[f"{tag}_{name}_E"]))
        assert onehot.dtype == x0.dtype and tuple(onehot.shape) == tuple(x0.shape)
        assert torch.equal(onehot.argmax(1).int().cpu(), T(g[f"{tag}_{name}_labels"]))
        assert torch.equal(dist.sample(), dist.sample()) and tuple(dist.sample().shape) == tuple(x0.shape)   # Philox default keys
    xt = torch.nn.functional.one_hot(T(g[f"{tag}_qx0_labels"]).long(), K).permute(inv).float().to(dev)
    got, ref = dm.theta_post(xt, x0, t).cpu(), T(g[f"{tag}_theta_post"])
    # the posterior kernel clamps at 1e-12 and renormalises; otherwise the roundings of the expression (two K-term sums, products, division)
    assert bool(((got - ref).abs() <= (2 * K + 8) * 2.0 ** -24 * ref + K * 1e-12).all())


# ------------------------------------------------------------------------------------------------ whole path: LDM
def ldm_bound(lt, per, absmax, rel):
    """How far a per-sample mean can move when every element of the network output moves by at most d = rel * max |out_ref| (the form of
    the existing suites' bound on eps): l1: |mean |e + dl| - mean |e|| <= d; l2: mean (2 |e| |dl| + dl^2) <= 2 sqrt(mean e^2) d + d^2
    (Cauchy-Schwarz), with mean e^2 the reference's per-sample value."""
    d = rel * float(absmax)
    per = np.asarray(per, dtype=np.float64)
    return np.full_like(per, d) if lt == "l1" else 2.0 * np.sqrt(per) * d + d * d


def check_dict(got, want, lo, hi, what):
    """Every key of the reference's dict; the bound per key is what the [N]-sized combinations make of the per-sample bounds (they are
    increasing in every per-sample value: hi - lo), plus the fp32 rounding of the reference's own few operations."""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in want:
        bound = (hi[k] - lo[k]) + 4e-6 * max(abs(want[k]), 1e-3)
        err = abs(float(got[k]) - want[k])
        print(f"{what} {k}: got {float(got[k]):.6f} want {want[k]:.6f} |d| {err:.3e} bound {bound:.3e}")
        assert err <= bound, (what, k)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_latent_diffusion_p_losses_match_the_reference_dicts(dev, g, mode):
    """l1 / l2, eps / x0, original_elbo_weight 0 / 1, learn_logvar off / on with a non-zero logvar; concat conditioning; t = 0, T - 1, 500."""
    from jointimagegeneration_amd import ops
    import contextlib
    x, noise, t, c = (T(g[k]).to(dev) for k in ("ldm_x", "ldm_noise", "ldm_t", "ldm_c"))
    models = {par: R.ldm_loss_model(parameterization=par, l_simple_weight=L_SIMPLE).to(dev) for par in ("eps", "x0")}
    with (ops.fp32_validation() if mode == "fp32" else contextlib.nullcontext()):
        for lt, par, w, lv in GRID:
            m = models[par]
            m.loss_type, m.original_elbo_weight, m.learn_logvar = lt, w, lv
            loss, d = m.p_losses(x, c, t, noise=noise)
            assert torch.equal(loss, d["val/loss"])
            per = g[f"ldm_{lt}_{par}_per"].astype(np.float64)
            b = ldm_bound(lt, per, g[f"ldm_{par}_out_absmax"], LDM_EPS_REL[mode])
            args = (g["ldm_t"], m.logvar, m.lvlb_weights, True, L_SIMPLE, w, lv)
            check_dict(d, fixture_dict(g, f"ldm_{lt}_{par}_w{int(w)}_lv{int(lv)}"), R.combine(per, *args), R.combine(per + b, *args),
                       f"{mode} {lt} {par} w{int(w)} lv{int(lv)}")
        # forward(): cond_stage_trainable sends the raw conditioning through the cond stage; t replayed
        m = models["eps"]
        m.loss_type, m.original_elbo_weight, m.learn_logvar, m.l_simple_weight, m.cond_stage_trainable = "l2", 0.0, False, 1.0, True
        _, d = m(x, T(g["ldm_concat_cond"]).to(dev), t=t, noise=noise)
        m.cond_stage_trainable = False
        per = g["ldm_l2_eps_per"].astype(np.float64)
        # the conditioning itself now comes from the engine's cond stage: its deviation is part of what the eps bound of the pipeline tests
        # (same 3e-2 / 2e-5 on the UNet output) covers
        b = ldm_bound("l2", per, g["ldm_eps_out_absmax"], LDM_EPS_REL[mode])
        args = (g["ldm_t"], m.logvar, m.lvlb_weights, True, 1.0, 0.0, False)
        check_dict(d, fixture_dict(g, "ldm_forward_trainable"), R.combine(per, *args), R.combine(per + b, *args), f"{mode} forward trainable")
        # with t=None the draw is the reference's torch.randint on the device: a dict with the same keys, finite values
        _, d = m(x, c, noise=noise)
        assert set(d) == {"val/loss_simple", "val/loss_vlb", "val/loss"} and all(bool(torch.isfinite(v)) for v in d.values())


def test_cross_attention_p_losses_match_the_reference(dev, g):
    """bf16 only: the engine's fp32 validation mode has no SpatialTransformer kernels (LayerNorm, GEGLU and cross-attention are bf16), and
    p_losses refuses that combination by name rather than return what those kernels make of fp32 buffers."""
    from jointimagegeneration_amd import ops
    m = R.xattn_loss_model().to(dev)
    x, noise, t, ctx = (T(g[k]).to(dev) for k in ("ldm_x", "ldm_noise", "ldm_t", "xattn_ctx"))
    _, d = m.p_losses(x, ctx, t, noise=noise)
    per = g["xattn_per"].astype(np.float64)
    b = ldm_bound("l2", per, g["xattn_out_absmax"], LDM_EPS_REL["bf16"])
    args = (g["ldm_t"], m.logvar, m.lvlb_weights, True, 1.0, 0.0, False)
    check_dict(d, fixture_dict(g, "xattn"), R.combine(per, *args), R.combine(per + b, *args), "bf16 crossattn")
    with ops.fp32_validation():
        with pytest.raises(NotImplementedError, match="with a SpatialTransformer UNet is not supported"):
            m.p_losses(x, ctx, t, noise=noise)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_ddpm_p_losses_match_the_reference_dicts(dev, g, mode):
    from jointimagegeneration_amd import ops
    import contextlib
    x, noise, t = (T(g[k]).to(dev) for k in ("ldm_x", "ldm_noise", "ddpm_t"))
    with (ops.fp32_validation() if mode == "fp32" else contextlib.nullcontext()):
        for par in ("eps", "x0"):
            d_ = R.ddpm_loss_model(parameterization=par, l_simple_weight=L_SIMPLE).to(dev)
            for lt in ("l1", "l2"):
                for w in (0.0, 1.0):
                    d_.loss_type, d_.original_elbo_weight = lt, w
                    loss, d = d_(x, t=t, noise=noise)
                    assert torch.equal(loss, d["val/loss"])
                    per = g[f"ddpm_{lt}_{par}_per"].astype(np.float64)
                    b = ldm_bound(lt, per, g[f"ddpm_{par}_out_absmax"], LDM_EPS_REL[mode])
                    args = (g["ddpm_t"], None, d_.lvlb_weights, False, L_SIMPLE, w, False)
                    check_dict(d, fixture_dict(g, f"ddpm_{lt}_{par}_w{int(w)}"), R.combine(per, *args), R.combine(per + b, *args),
                               f"{mode} ddpm {lt} {par} w{int(w)}")


def test_validation_losses_run_the_ema_pass_under_ema_scope(dev, g):
    from jointimagegeneration_amd import ops
    x, noise, t, c = (T(g[k]).to(dev) for k in ("ldm_x", "ldm_noise", "ldm_t", "ldm_c"))
    m = R.set_ema(R.ldm_loss_model(use_ema=True)).to(dev)
    before = {k: v.detach().clone() for k, v in m.model.named_parameters()}
    want = fixture_dict(g, "ldm_val")
    with ops.fp32_validation():
        d = m.validation_losses(x, c, t=t, noise=noise)
    assert set(d) == set(want) == {k + s for k in ("val/loss_simple", "val/loss_vlb", "val/loss") for s in ("", "_ema")}
    assert all(torch.equal(v, before[k]) for k, v in m.model.named_parameters())               # ema_scope restored the weights
    assert float(d["val/loss"]) != float(d["val/loss_ema"])
    # both passes: the fp32-validation bound of the p_losses test, each from its own recorded per-sample values and output range
    args = (g["ldm_t"], m.logvar, m.lvlb_weights, True, 1.0, 0.0, False)
    for sfx, per, absmax in (("", g["ldm_l2_eps_per"], g["ldm_eps_out_absmax"]), ("_ema", g["ldm_val_per_ema"], g["ldm_val_out_absmax_ema"])):
        per = per.astype(np.float64)
        b = ldm_bound("l2", per, absmax, LDM_EPS_REL["fp32"])
        keys = ("val/loss_simple", "val/loss_vlb", "val/loss")
        check_dict({k: d[k + sfx] for k in keys}, {k: want[k + sfx] for k in keys}, R.combine(per, *args), R.combine(per + b, *args),
                   f"validation_losses{sfx}")


# ------------------------------------------------------------------------------------------------ whole path: CCDM
@pytest.fixture(scope="module")
def ccdm(dev):
    return R.ccdm_loss_model().to(dev)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_ccdm_step_losses_match_the_reference(dev, g, ccdm, mode):
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.losses import ccdm_step_losses
    import contextlib
    K = R.CCDM_K
    x0, cond, t, E = (T(g[k]).to(dev) for k in ("net_x0", "net_cond", "net_t", "net_E"))
    scal = R.step_scalars(ccdm.diffusion.alphas, ccdm.diffusion.cumalphas, g["net_t"])
    p_ref = np.moveaxis(g["net_x0pred"], 1, -1).reshape(2, -1, K)
    measured = []
    for wtag, cw in (("ones", None), ("cw", T(g["net_class_weights"]))):
        with (ops.fp32_validation() if mode == "fp32" else contextlib.nullcontext()):
            r = ccdm_step_losses(ccdm, x0, cond, t, class_weights=cw, rng_tape=E)
        assert torch.equal(r["xt"].cpu(), T(g["net_xt"]))                         # every race of the fixture is decidable
        got = torch.stack([r["kl_per_sample"], r["ce_per_sample"]], 1).cpu().numpy()
        want = g[f"net_{wtag}_sums"].astype(np.float64)
        rel = np.abs(got / want - 1)
        print(f"ccdm_step_losses {mode} {wtag}: per-sample (kl, ce) rel {rel.tolist()}")
        batch = g[f"net_{wtag}_batch"].astype(np.float64)
        assert abs(float(r["loss"]) - (float(r["loss_kl"]) + float(r["loss_ce"]))) <= 1e-12 * abs(float(r["loss"]))
        assert abs(float(r["loss_kl"]) - got[:, 0].sum() / 2) <= 1e-12 * abs(float(r["loss_kl"]))
        if mode == "bf16":
            # every probability of the engine's output may lie CCDM_PROBS_ABS_BF16 from the reference's (the bound of the existing suites on
            # this network): losses_ref.ccdm_loss_bound carries that through the posterior, the clamp, the log and the sums
            b = R.ccdm_loss_bound(p_ref, g["net_xt"], g["net_x0"], scal, np.ones(K) if cw is None else g["net_class_weights"], K, CCDM_PROBS_ABS_BF16)
            print(f"  bf16 bound per sample (kl, ce): {b.tolist()}, |d| {np.abs(got - want).tolist()}")
            assert (np.abs(got - want) <= b + 1e-5 * np.abs(want)).all()
            for i, key in enumerate(("loss_kl", "loss_ce")):
                assert abs(float(r[key]) - batch[i]) <= b[:, i].sum() / 2 + 1e-5 * abs(batch[i])
        else:
            measured.append(max(float(rel.max()), *(abs(float(r[key]) / batch[i] - 1) for i, key in enumerate(("loss_kl", "loss_ce", "loss")))))
    if measured:                                                                  # both weightings are printed before either is judged
        print(f"ccdm_step_losses fp32: worst rel {max(measured):.3e} (allowed {2 * CCDM_FP32_MEASURED:.3e})")
        assert max(measured) <= 2 * CCDM_FP32_MEASURED


def test_ccdm_step_losses_philox_terms_do_not_depend_on_the_batch_slot(dev, g, ccdm):
    from jointimagegeneration_amd.losses import ccdm_step_losses
    x0, cond, t = (T(g[k]).to(dev) for k in ("net_x0", "net_cond", "net_t"))
    a = ccdm_step_losses(ccdm, x0, cond, t, philox_seeds=[11, 12])
    b = ccdm_step_losses(ccdm, x0, cond, t, philox_seeds=[11, 12])
    assert all(torch.equal(a[k], b[k]) for k in a)
    one = ccdm_step_losses(ccdm, x0[1:], cond[1:], t[1:], philox_seeds=[12])
    assert torch.equal(one["xt"], a["xt"][1:])
    with pytest.raises(ValueError, match="1 philox_seeds for a batch of 2"):
        ccdm_step_losses(ccdm, x0, cond, t, philox_seeds=[1])


def test_ddpm_eval_loss_block_is_reproducible_and_equals_the_direct_call(dev, tmp_path):
    import yaml
    from jointimagegeneration_amd import ddpm_eval
    from jointimagegeneration_amd.io import write_nifti
    from jointimagegeneration_amd.losses import ccdm_step_losses
    size, K, nvol, ts = (8, 8, 8), 4, 2, (1, 4, 6)
    params = dict(output_path=str(tmp_path), exp_name="t", evaluation_vote_strategy="majority", dataset_file="datasets.ruijin", batch_size=2,
                  dims=3, beta_schedule="cosine", beta_schedule_params=dict(s=0.008), time_steps=6, backbone="unet_openai",
                  feature_cond_encoder=dict(type="none"), unet_openai=dict(CCDM_SMALL))
    pf = tmp_path / "params_eval.yml"
    pf.write_text(yaml.safe_dump(params))
    gt_dir = tmp_path / "gt"
    gt_dir.mkdir()
    rng = np.random.default_rng(21)
    gts = [rng.integers(0, K, size=size).astype(np.uint8) for _ in range(nvol)]
    for vid, gt in enumerate(gts):
        write_nifti(str(gt_dir / f"gt_{vid:04d}.nii.gz"), gt)
    common = [str(pf), "--size", *map(str, size), "--num-classes", str(K), "--num-volumes", str(nvol), "--steps", "2", "--gt", str(gt_dir)]
    docs = []
    for name in ("a", "b"):
        ddpm_eval.main(common[:1] + [name] + common[1:] + ["--loss-t", ",".join(map(str, ts))])
        docs.append(json.loads((tmp_path / name / "metrics.json").read_text()))
    assert docs[0]["loss"] == docs[1]["loss"] and [e["t"] for e in docs[0]["loss"]] == list(ts)
    ddpm_eval.main(common[:1] + ["none"] + common[1:])
    assert "loss" not in json.loads((tmp_path / "none" / "metrics.json").read_text())
    model = ddpm_eval.build_from_params(dict(params), size, K).eval()
    ddpm_eval.load_weights(model, params, log=lambda m: None)
    model = model.to(dev)
    for e in docs[0]["loss"]:
        rs = [ccdm_step_losses(model, torch.from_numpy(gts[v].astype(np.int32))[None].to(dev), torch.zeros((1, 1) + size, device=dev),
                               torch.tensor([e["t"]]), philox_seeds=[ddpm_eval.loss_key(v, e["t"])]) for v in range(nvol)]
        for key in ("loss_kl", "loss_ce", "loss"):
            assert e[key] == float(sum(float(r[key]) for r in rs) / nvol) and np.isfinite(e[key]), (e["t"], key)
        assert e["volumes"] == nvol
    with pytest.raises(ValueError, match="--loss-t needs --gt"):
        ddpm_eval.main([str(pf), "x", "--loss-t", "1"])
    with pytest.raises(ValueError, match=r"steps are 1\.\.6"):
        ddpm_eval.main(common[:1] + ["bad"] + common[1:] + ["--loss-t", "7"])
