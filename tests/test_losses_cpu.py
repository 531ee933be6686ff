"""CPU suite of the held-out objectives: the fp64 restatement (tests/losses_ref.py) against what the REFERENCE recorded
(tests/golden/losses.npz, make_golden_losses.py), lvlb_weights with ==, the unchanged state_dict surfaces, every refusal by name, and the
header / binding / build list of the four new entry points.  Nothing here needs a GPU.

The restatement is fp64 and the fixture fp32, so they are compared at the distance the generator measured between them (`*_dist`, at
most 9.2e-4 for the ill-conditioned KL sums, 1.8e-4 for the prior term) -- the figures the GPU suite's kernel bounds are built from."""
import json
import os

import numpy as np
import pytest
import torch

import losses_ref as R
from util import GOLD, T, gold, surface

torch.set_grad_enabled(False)
CCDM_CASES = (("k14", 14, 3), ("k3", 3, 3), ("k5_2d", 5, 2))
GRID = [(lt, par, w, lv) for lt in ("l1", "l2") for par in ("eps", "x0") for w in (0.0, 1.0) for lv in (False, True)]
L_SIMPLE = 0.7


@pytest.fixture(scope="module")
def g():
    return gold("losses")


def cl(a):
    a = np.asarray(a)
    return np.moveaxis(a, 1, -1).reshape(a.shape[0], -1, a.shape[1])


def fixture_dict(g, tag):
    return {k.split("|", 1)[1]: float(g[k]) for k in g.files if k.startswith(tag + "|")}


# ------------------------------------------------------------------------------------------------ restatement vs fixture
@pytest.mark.parametrize("tag,K,dims", CCDM_CASES)
def test_ccdm_restatement_matches_the_reference(g, tag, K, dims):
    from jointimagegeneration_amd.ccdm import DiffusionModel
    dm = DiffusionModel("cosine", R.CCDM_T, K, dims=dims)
    t = g[f"{tag}_t"]
    x0 = g[f"{tag}_x0"].astype(np.int64)
    # the reference's fp32 values: two products, two K-term sums (at most K - 1 roundings each, worst case) and a division
    ulps = (2 * K + 3) * 2.0 ** -24
    ti = torch.from_numpy(t) - 1
    for name, mix in (("qx0", (dm.cumalphas[ti], 1 - dm.cumalphas[ti])), ("qxtm1", (1 - dm.betas[ti], dm.betas[ti]))):
        assert torch.equal(torch.stack(mix, 1), T(g[f"{tag}_{name}_mix"]))        # the schedule buffers are the reference's
        probs = R.keep_probs(x0, mix[0], mix[1], K)
        ref = g[f"{tag}_{name}_probs"].reshape(probs.shape)
        assert (np.abs(probs - ref) <= ulps * ref).all()
        lab, gap = R.race(probs, g[f"{tag}_{name}_E"])
        assert float(gap.min()) > R.GAP_MIN                                       # the generator left no undecidable draw
        assert np.array_equal(lab, R.rows(g[f"{tag}_{name}_labels"]))
        assert np.allclose(gap, g[f"{tag}_{name}_gap"], rtol=1e-5)
    xt = g[f"{tag}_qx0_labels"].astype(np.int64)
    scal = R.step_scalars(dm.alphas, dm.cumalphas, t)
    assert np.array_equal(scal.astype(np.float32), dm.step_scalar_rows(torch.from_numpy(t)).numpy())
    ref = cl(g[f"{tag}_theta_post"])
    assert (np.abs(R.theta_post(xt, x0, scal, K) - ref) <= ulps * ref).all()
    for wtag, cw in (("ones", np.ones(K)), ("cw", g[f"{tag}_class_weights"])):
        want = R.ccdm_step_loss(cl(g[f"{tag}_logits"]), xt, x0, scal, cw, K)
        assert np.array_equal(want, g[f"{tag}_{wtag}_sums_f64"])
        ref = g[f"{tag}_{wtag}_sums"].astype(np.float64)
        assert np.abs(want - ref).max() <= float(g[f"{tag}_{wtag}_dist"]) * np.abs(want).max() * (1 + 1e-6) + 0.0
        assert float(g[f"{tag}_{wtag}_dist"]) * 4 <= float(g["tol_ccdm_step_loss"])
        batch = np.array([want[:, 0].sum() / 2, want[:, 1].sum() / 2, want.sum() / 2])
        assert np.allclose(batch, g[f"{tag}_{wtag}_batch"], rtol=float(g["tol_ccdm_step_loss"]))


@pytest.mark.parametrize("tag", ["2d", "3d"])
def test_loss_rows_restatement_matches_the_reference(g, tag):
    from jointimagegeneration_amd.ldm import make_beta_schedule
    for lt in ("l1", "l2"):
        want = R.loss_rows(lt, g[f"rows_{tag}_pred"], g[f"rows_{tag}_target"])
        assert np.array_equal(want, g[f"rows_{tag}_{lt}_f64"])
        assert np.abs(want / g[f"rows_{tag}_{lt}"] - 1).max() <= float(g[f"rows_{tag}_{lt}_dist"]) * (1 + 1e-6)
    ac = np.cumprod(1.0 - make_beta_schedule("linear", R.LDM_T, 0.0015, 0.0195))
    s, lv = np.float32(np.sqrt(ac[-1])), np.float32(np.log(1.0 - ac[-1]))
    want = R.prior_kl(g[f"rows_{tag}_x"], s, lv) / np.log(2.0)
    assert np.array_equal(want, g[f"rows_{tag}_prior_bpd_f64"])
    assert np.abs(want / g[f"rows_{tag}_prior_bpd"] - 1).max() <= float(g[f"rows_{tag}_prior_dist"]) * (1 + 1e-6)
    assert float(g["tol_loss_rows"]) >= 4 * max(float(g[f"rows_{tag}_l1_dist"]), float(g[f"rows_{tag}_l2_dist"]))
    assert float(g["tol_loss_rows_prior"]) >= 4 * float(g[f"rows_{tag}_prior_dist"])


def test_combinations_restatement_matches_the_reference_dicts(g):
    """combine() on the reference's per-sample means gives the reference's dicts (fp32 there: 1e-6 relative)."""
    m = {par: R.ldm_loss_model(parameterization=par) for par in ("eps", "x0")}
    t = g["ldm_t"]
    for lt, par, w, lv in GRID:
        want = fixture_dict(g, f"ldm_{lt}_{par}_w{int(w)}_lv{int(lv)}")
        got = R.combine(g[f"ldm_{lt}_{par}_per"], t, m[par].logvar, m[par].lvlb_weights, True, L_SIMPLE, w, lv)
        assert set(got) == set(want), (lt, par, w, lv)
        for k in want:
            assert abs(got[k] - want[k]) <= 2e-6 * max(abs(want[k]), 1e-3), (lt, par, w, lv, k, got[k], want[k])
    for par in ("eps", "x0"):
        d = R.ddpm_loss_model(parameterization=par)
        for lt in ("l1", "l2"):
            for w in (0.0, 1.0):
                want = fixture_dict(g, f"ddpm_{lt}_{par}_w{int(w)}")
                got = R.combine(g[f"ddpm_{lt}_{par}_per"], g["ddpm_t"], None, d.lvlb_weights, False, L_SIMPLE, w, False)
                assert set(got) == set(want)
                for k in want:
                    assert abs(got[k] - want[k]) <= 2e-6 * max(abs(want[k]), 1e-3), (lt, par, w, k)


# ------------------------------------------------------------------------------------------------ schedule-side values
def test_lvlb_weights_equal_the_reference_bit_for_bit(g):
    for par in ("eps", "x0"):
        m = R.ldm_loss_model(parameterization=par)
        assert torch.equal(m.lvlb_weights, T(g[f"lvlb_{par}_1000"])), par
        assert float(m.lvlb_weights[0]) == float(m.lvlb_weights[1]) and not bool(torch.isnan(m.lvlb_weights).any())
        d = R.ddpm_loss_model(parameterization=par)
        assert torch.equal(d.lvlb_weights, T(g[f"lvlb_{par}_20"])), par


def test_q_mean_variance_and_q_sample_equal_the_reference(g):
    m = R.ldm_loss_model()
    x, t = T(g["ldm_x"]), T(g["ldm_t"])
    mean, var, logv = m.q_mean_variance(x, t)
    assert torch.equal(mean, T(g["qmv_mean"])) and torch.equal(var, T(g["qmv_var"])) and torch.equal(logv, T(g["qmv_logvar"]))
    assert torch.equal(m.q_sample(x, t, T(g["ldm_noise"])), T(g["q_sample"]))


def test_state_dict_surfaces_are_unchanged_by_the_new_buffer():
    m = R.ldm_loss_model(learn_logvar=True, loss_type="l1", original_elbo_weight=1.0, l_simple_weight=0.5)
    assert surface(m) == json.loads(str(gold("chains_small")["ldm_pipe_surface"]))
    assert "lvlb_weights" in dict(m.named_buffers()) and "lvlb_weights" not in m.state_dict()
    assert (m.loss_type, m.original_elbo_weight, m.l_simple_weight, m.learn_logvar) == ("l1", 1.0, 0.5, True)
    d = R.ddpm_loss_model(loss_type="l1", original_elbo_weight=0.25, l_simple_weight=0.5, learn_logvar=True)
    want = json.load(open(os.path.join(GOLD, "progressive_surface.json")))["ddpm"]
    assert sorted((k, tuple(s)) for k, s in surface(d)) == sorted((k, tuple(s)) for k, s in want)
    assert (d.loss_type, d.original_elbo_weight, d.l_simple_weight, d.learn_logvar) == ("l1", 0.25, 0.5, True)


# ------------------------------------------------------------------------------------------------ refusals
def test_ldm_refusals_by_name():
    m = R.ldm_loss_model()
    x, c, t = torch.zeros(2, 4, 8, 8), torch.zeros(2, 4, 8, 8), torch.tensor([0, 5])
    with pytest.raises(NotImplementedError, match=r"LatentDiffusion\.p_losses: not supported for a model on cpu"):
        m.p_losses(x, c, t)
    with pytest.raises(NotImplementedError, match="get_input is not supported"):
        m.get_input({"image": x}, "image")
    with pytest.raises(NotImplementedError, match=r"shared_step\(batch\) is not supported"):
        m.shared_step({"image": x})
    m.num_timesteps_cond = 2
    with pytest.raises(NotImplementedError, match=r"LatentDiffusion\.p_losses: num_timesteps_cond = 2"):
        m.p_losses(x, c, t)
    with pytest.raises(NotImplementedError, match=r"LatentDiffusion\.forward: num_timesteps_cond = 2"):
        m(x, c, t=t)
    m.num_timesteps_cond = 1
    m.split_input_params = dict(ks=(4, 4), stride=(2, 2))
    with pytest.raises(NotImplementedError, match="split_input_params .* together with p_losses"):
        m.p_losses(x, c, t)
    del m.split_input_params
    m.train()
    with pytest.raises(RuntimeError, match=r"LatentDiffusion\.p_losses: the model is in training mode"):
        m.p_losses(x, c, t)
    m.eval()
    m.loss_type = "huber"
    with pytest.raises(NotImplementedError, match="unknown loss type 'huber'"):
        m.p_losses(x, c, t)
    with pytest.raises(NotImplementedError, match="unknown loss type 'huber'"):
        m.get_loss(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m._prior_bpd(x)
    d = R.ddpm_loss_model()
    with pytest.raises(NotImplementedError, match=r"DDPM\.p_losses: not supported for a model on cpu"):
        d.p_losses(x, t)
    with pytest.raises(NotImplementedError, match=r"shared_step\(batch\) is not supported"):
        d.shared_step({"image": x})
    d.train()
    with pytest.raises(RuntimeError, match=r"DDPM\.p_losses: the model is in training mode"):
        d(x, t=t)
    d.eval()
    d.model.conditioning_key = "concat"
    with pytest.raises(NotImplementedError, match=r"DDPM\.p_losses: conditioning_key 'concat'"):
        d.p_losses(x, t)


def test_ccdm_refusals_by_name():
    from jointimagegeneration_amd.ccdm import DenoisingModel
    from jointimagegeneration_amd.losses import ccdm_step_losses
    m = R.ccdm_loss_model()
    lab, cond, t = torch.zeros(2, 8, 8, 8, dtype=torch.int64), torch.zeros(2, 1, 8, 8, 8), torch.tensor([1, 7])
    with pytest.raises(NotImplementedError, match="ccdm_step_losses: not supported for a model on cpu"):
        ccdm_step_losses(m, lab, cond, t)
    with pytest.raises(NotImplementedError, match="ccdm_step_losses: feature_condition is not supported"):
        ccdm_step_losses(m, lab, cond, t, feature_condition=torch.zeros(1))
    m.unet.sofmtax_output = False
    with pytest.raises(NotImplementedError, match="ccdm_step_losses: softmax_output=False is not supported"):
        ccdm_step_losses(m, lab, cond, t)
    m.unet.sofmtax_output = True
    m.train()
    with pytest.raises(RuntimeError, match="ccdm_step_losses: the model is in training mode"):
        ccdm_step_losses(m, lab, cond, t)
    with pytest.raises(RuntimeError, match="sampling only"):
        m(torch.zeros(2, R.CCDM_K, 8, 8, 8), cond)                                  # model.train() stays refused by forward
    m.eval()
    x0 = torch.nn.functional.one_hot(lab, R.CCDM_K).permute(0, 4, 1, 2, 3).float()
    for call in (lambda: m.diffusion.q_xt_given_x0(x0, t), lambda: m.diffusion.q_xt_given_xtm1(x0, t), lambda: m.diffusion.theta_post(x0, x0, t)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match=r"outside 1\.\.50"):
        m.diffusion.step_scalar_rows(torch.tensor([0, 3]))
    assert isinstance(m, DenoisingModel)


# ------------------------------------------------------------------------------------------------ header, bindings, build list
ENTRY_POINTS = ("gg_q_sample_rows", "gg_loss_rows", "gg_ccdm_q_sample", "gg_ccdm_step_loss", "gg_loss_workspace_bytes")


def test_library_exports_the_loss_entry_points():
    from util import load_lib
    lib = load_lib()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name)
    assert lib.gg_loss_workspace_bytes(2, 210) == 2 * 1 * 2 * 8 and lib.gg_loss_workspace_bytes(3, 10 ** 7) == 3 * 1024 * 2 * 8
    assert lib.gg_loss_workspace_bytes(0, 5) == 0
    # host-side argument checks run before any launch: callable without a GPU
    assert lib.gg_loss_rows(None, 0, None, None, None, 0, 1, 1, 1, None, None, 0, None) == -1
    assert b"null pointer" in lib.gg_last_error()
    assert lib.gg_ccdm_q_sample(None, None, 1, 14, None, None, None, 1, None, None, 0, None) == -1
