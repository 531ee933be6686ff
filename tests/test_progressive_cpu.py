"""CPU suite for progressive sampling: the cosine / sqrt_linear / sqrt / given_betas schedules bit for bit against the reference's
buffers (tests/golden/progressive.npz, make_golden_progressive.py), the DDPM class and its state_dict surface, the logging rule of the
three loops against what the reference logged, the options refused by name before any launch, and the host-side argument checks of
gg_ddpm_step_x0 and gg_log_rows (their declarations are checked with every other in test_capi_cpu.py)."""
import json
import os

import numpy as np
import pytest
import torch

from progressive_ref import BUFFERS, ddpm_config, ddpm_small, ldm_small, logged, recorded_list
from util import GOLD, gold, surface

SHAPE = (2, 4, 8, 8)


@pytest.fixture(scope="module")
def g():
    return gold("progressive")


@pytest.fixture(scope="module")
def m20():
    return ldm_small(20)


# ------------------------------------------------------------------------------------------------ schedules
def check_buffers(m, g, tag):
    for b in BUFFERS:
        got, want = getattr(m, b).numpy(), g[f"sched_{tag}_{b}"]
        assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape == (20,)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (tag, b)
    assert m.logvar.dtype == torch.float32 and torch.equal(m.logvar, torch.zeros(20))          # the 13th buffer
    assert m.num_timesteps == 20


@pytest.mark.parametrize("schedule", ["cosine", "sqrt_linear", "sqrt"])
def test_schedule_buffers_are_bit_equal_to_the_reference(m20, g, schedule):
    m20.register_schedule(beta_schedule=schedule, timesteps=20, linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3)
    check_buffers(m20, g, schedule)


def test_given_betas_buffers_are_bit_equal_to_the_reference(g):
    m = ldm_small(1000, given_betas=g["given_betas"])              # given_betas decide the number of timesteps (ddpm.py:129-130)
    check_buffers(m, g, "given")
    m.register_schedule(given_betas=torch.from_numpy(g["given_betas"]))
    check_buffers(m, g, "given")


def test_constructor_reaches_the_named_schedule(g):
    check_buffers(ldm_small(20, beta_schedule="sqrt", linear_start=1e-4, linear_end=2e-2), g, "sqrt")


def test_unknown_schedule_raises_the_reference_error():
    from jointimagegeneration_amd.ldm import make_beta_schedule
    with pytest.raises(ValueError, match="schedule 'quadratic' unknown"):
        make_beta_schedule("quadratic", 20)
    with pytest.raises(ValueError, match="unknown"):
        ldm_small(20, beta_schedule="exp")
    assert make_beta_schedule("linear", 7).dtype == np.float64 and make_beta_schedule("cosine", 7).max() <= 0.999


# ------------------------------------------------------------------------------------------------ model surface
def test_ddpm_resolves_and_carries_the_reference_surface():
    from jointimagegeneration_amd.config import get_obj_from_str
    from jointimagegeneration_amd.ldm import DDPM, LatentDiffusion
    assert get_obj_from_str("ldm.models.diffusion.ddpm.DDPM") is DDPM
    d = ddpm_small()
    assert isinstance(d, DDPM) and not isinstance(d, LatentDiffusion)
    want = json.load(open(os.path.join(GOLD, "progressive_surface.json")))["ddpm"]
    got = surface(d)
    assert sorted(map(tuple, map(lambda e: (e[0], tuple(e[1])), got))) == sorted((k, tuple(s)) for k, s in want)
    names = [k for k, _ in got]
    assert any(k.startswith("model.diffusion_model.") for k in names) and any(k.startswith("model_ema.") for k in names)
    assert [k for k in names if not k.startswith(("model.", "model_ema."))] == list(BUFFERS) + ["logvar"]
    assert d.clip_denoised is True and d.log_every_t == 10 and d.parameterization == "eps" and d.num_timesteps == 20
    for name in ("p_sample_loop", "sample", "q_sample", "ema_scope", "init_from_ckpt"):
        assert callable(getattr(d, name))


def test_defaults_of_the_two_classes(m20):
    from jointimagegeneration_amd.config import instantiate_from_config
    cfg = ddpm_config()
    del cfg["params"]["log_every_t"]
    d = instantiate_from_config(cfg)
    assert d.clip_denoised is True and d.log_every_t == 100
    assert m20.clip_denoised is False and m20.log_every_t == 100 and m20.num_timesteps_cond == 1 and m20.parameterization == "eps"
    m = ldm_small(20, parameterization="x0", log_every_t=7, num_timesteps_cond=3)
    assert (m.parameterization, m.log_every_t, m.num_timesteps_cond, m.clip_denoised) == ("x0", 7, 3, False)
    with pytest.raises(ValueError, match="parameterization"):
        ldm_small(20, parameterization="v")
    # the training-only constructor arguments of the reference are accepted
    instantiate_from_config(ddpm_config(loss_type="l1", monitor=None, original_elbo_weight=0.1, l_simple_weight=0.5, scheduler_config=None,
                                        use_positional_encodings=False, learn_logvar=False, logvar_init=0.0, load_only_unet=False,
                                        conditioning_key=None, v_posterior=0.0, use_ema=False, given_betas=None, cosine_s=8e-3,
                                        beta_schedule="linear", first_stage_key="image", ignore_keys=[], ckpt_path=None))


def test_ddpm_q_sample_and_ema_scope():
    d = ddpm_small()
    x, n = torch.randn(SHAPE), torch.randn(SHAPE)
    t = torch.tensor([3, 17])
    want = d.sqrt_alphas_cumprod[t].view(2, 1, 1, 1) * x + d.sqrt_one_minus_alphas_cumprod[t].view(2, 1, 1, 1) * n
    assert torch.equal(d.q_sample(x, t, n), want)
    p = next(d.model.parameters())
    before = p.detach().clone()
    d.model_ema.reset_from(d.model)
    with torch.no_grad():
        p.add_(1.0)
    with d.ema_scope():
        assert torch.equal(p, before)                  # the EMA shadow holds the values it was reset from
    assert torch.equal(p, before + 1.0)


# ------------------------------------------------------------------------------------------------ logging rule
@pytest.mark.parametrize("loop", ["p_sample_loop", "progressive", "ddim", "plms"])
@pytest.mark.parametrize("n", [1, 2, 5, 20])
@pytest.mark.parametrize("k", [1, 3, 100])
def test_logged_indices_match_what_the_reference_logged(g, loop, n, k):
    from jointimagegeneration_amd.ldm import logged_steps
    want = g[f"idx_{loop}_{n}_{k}"].tolist()
    assert recorded_list(loop, n, k) == want
    assert logged_steps(n, k) == logged(n, k) == [v for v in want if v >= 0]


@pytest.mark.parametrize("loop", ["ddim", "plms"])
@pytest.mark.parametrize("k", [1, 3, 100])
def test_logged_indices_count_the_schedules_own_steps(g, loop, k):
    """S = 15 does not divide 1000 timesteps: the uniform schedule holds 16 steps and the reference's indices run from 15 (ddim.py:136,160)."""
    from jointimagegeneration_amd.ldm import logged_steps, make_ddim_timesteps
    steps = make_ddim_timesteps("uniform", 15, 1000).shape[0]
    assert steps == 16
    assert [-1] + logged_steps(steps, k) == recorded_list(loop, steps, k) == g[f"idx_{loop}_15_{k}"].tolist()


def test_logged_steps_refuses_a_non_positive_interval():
    from jointimagegeneration_amd.ldm import logged_steps
    with pytest.raises(ValueError, match="log_every_t"):
        logged_steps(5, 0)


# ------------------------------------------------------------------------------------------------ refusals, by name, before any launch
def test_ddim_and_plms_refuse_an_x0_model():
    from jointimagegeneration_amd.ldm import DDIMSampler, PLMSSampler
    m = ldm_small(20, parameterization="x0")
    for cls in (DDIMSampler, PLMSSampler):
        with pytest.raises(NotImplementedError, match="parameterization 'x0'"):
            cls(m).sample(S=5, batch_size=2, shape=(4, 8, 8), verbose=False)


def test_num_timesteps_cond_is_refused_in_the_ancestral_loops():
    m = ldm_small(20, num_timesteps_cond=2)
    with pytest.raises(NotImplementedError, match="num_timesteps_cond"):
        m.p_sample_loop(None, SHAPE, verbose=False)
    with pytest.raises(NotImplementedError, match="num_timesteps_cond"):
        m.progressive_denoising(None, SHAPE, verbose=False)
    with pytest.raises(NotImplementedError, match="num_timesteps_cond"):
        m.sample(None, batch_size=2, shape=SHAPE)


def test_cpu_models_and_score_corrector_are_refused(m20):
    with pytest.raises(NotImplementedError, match=r"progressive_denoising: not supported for a model on cpu"):
        m20.progressive_denoising(None, SHAPE, verbose=False)
    with pytest.raises(NotImplementedError, match="score_corrector"):
        m20.progressive_denoising(None, SHAPE, verbose=False, score_corrector=object())
    d = ddpm_small()
    with pytest.raises(NotImplementedError, match=r"DDPM.p_sample_loop: not supported for a model on cpu"):
        d.p_sample_loop(SHAPE)
    with pytest.raises(NotImplementedError, match=r"DDPM.p_sample_loop: not supported for a model on cpu"):
        d.sample(batch_size=2, return_intermediates=True)


# ------------------------------------------------------------------------------------------------ C-ABI
@pytest.fixture(scope="module")
def lib():
    from util import load_lib
    return load_lib()


def test_gg_ddpm_step_x0_rejects_bad_arguments_on_the_host(lib):
    """Every check runs before a launch, so the codes are observable without a GPU (the fake pointers are never read)."""
    p, bad_shape, unsupported = 0x1000, -1, -3
    step = lib.gg_ddpm_step_x0
    for i in (0, 1, 4):                                                                        # null x, out, scalars
        a = [p, p, 32, p, p]
        a[i] = None
        assert step(*a, 0, 16, 4, p, p, 32, None) == bad_shape, i
        assert b"null" in lib.gg_last_error()
    assert step(p, p, 3, p, p, 0, 16, 4, None, None, 0, None) == bad_shape                       # out_stride < C
    assert b"out_stride" in lib.gg_last_error()
    assert step(p, p, 32, p, p, 0, 16, 4, None, p, 3, None) == bad_shape                         # unet_in_stride < C
    assert b"unet_in_stride" in lib.gg_last_error()
    for flags in (4, 8, 7, -1):
        assert step(p, p, 32, p, p, flags, 16, 4, None, None, 0, None) == unsupported, flags    # unknown flag bits
        assert b"flag" in lib.gg_last_error()
    for flags in (0, 1, 2, 3):                                                                  # M = 0: nothing to do, no launch
        assert step(p, p, 32, None, p, flags, 0, 4, None, p, 32, None) == 0
        assert step(p, p, 3, p, p, flags, 0, 3, p, None, 0, None) == 0


def test_gg_log_rows_rejects_bad_arguments_on_the_host(lib):
    p, bad_shape = 0x1000, -1
    assert lib.gg_log_rows(None, 2, 4, 64, p, None) == bad_shape
    assert lib.gg_log_rows(p, 2, 4, 64, None, None) == bad_shape
    assert lib.gg_log_rows(p, 2, 0, 64, p, None) == bad_shape
    assert lib.gg_log_rows(p, -1, 4, 64, p, None) == bad_shape
    assert lib.gg_log_rows(p, 2, 4, -5, p, None) == bad_shape
    assert lib.gg_log_rows(p, 0, 4, 64, p, None) == 0                                          # empty: no launch
    assert lib.gg_log_rows(p, 2, 4, 0, p, None) == 0


# ------------------------------------------------------------------------------------------------ entry point
def test_sample_diffusion_flags_go_together():
    from jointimagegeneration_amd import sample_diffusion as sd
    opt = sd.get_parser().parse_args(["-v", "--progress-png", "--log-every-t", "5"])
    assert opt.progress_png and opt.log_every_t == 5 and opt.vanilla_sample
    assert sd.get_parser().parse_args([]).progress_png is False and sd.get_parser().parse_args([]).log_every_t is None
    with pytest.raises(SystemExit, match="--progress-png goes with -v"):
        sd.main(["--config", "none.yaml", "--progress-png"])
    with pytest.raises(SystemExit, match="--log-every-t goes with --progress-png"):
        sd.main(["--config", "none.yaml", "-v", "--log-every-t", "5"])
