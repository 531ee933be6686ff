"""CPU suite of the DPM-Solver++ (2M) sampler: the step grids and the coefficient rows of dpm_solver.py against the fp64 restatement of
tests/dpm_ref.py, first order as DDIM (an fp64 identity), the Gaussian toy problem on which the exact probability-flow solution is a
closed form, the host-side refusals, and the entry points.  Nothing here needs a GPU."""
import types

import numpy as np
import pytest
import torch

import dpm_ref as R

GRIDS = ("uniform", "quad", "logsnr")
STEPS = (5, 10, 20, 50)


def stub(ac, **kw):
    """What the sampler's host side reads of a model."""
    return types.SimpleNamespace(num_timesteps=len(ac), alphas_cumprod=torch.from_numpy(np.asarray(ac)), device=torch.device("cpu"),
                                 parameterization="eps", **kw)


@pytest.fixture(scope="module")
def tables():
    return [R.alphas_cumprod(*s) for s in R.SCHEDULES]


# ------------------------------------------------------------------------------------------------ grids and rows
@pytest.mark.parametrize("grid", GRIDS)
def test_grid_and_rows_equal_the_restatement(tables, grid):
    from jointimagegeneration_amd import dpm_solver as D
    for ac in tables:
        for S in STEPS:
            ts = D.dpm_timesteps(grid, S, ac)
            want_ts = R.grid(grid, S, ac)
            assert ts.tolist() == want_ts.tolist(), (grid, S)
            assert len(ts) <= (S + 1 if grid == "uniform" else S) and ts[0] >= 1 and ts[-1] <= len(ac) - 1 and bool((np.diff(ts) > 0).all())
            if grid == "logsnr":
                assert ts[-1] == len(ac) - 1                        # the first target is lambda[T - 1] itself
            for order in (1, 2):
                for lof in (True, False):
                    sampler = D.DPMSolverSampler(stub(ac), order=order, lower_order_final=lof)
                    sampler.make_schedule(S, ddim_discretize=grid, verbose=False)
                    got = sampler.step_scalar_table()
                    want, h = R.rows(want_ts, ac, order, lof)
                    assert bool((h > 0).all()), (grid, S, h.min())
                    assert got.dtype == torch.float32 and tuple(got.shape) == (len(want_ts), 6)
                    assert np.array_equal(got.numpy(), want.astype(np.float32)), (grid, S, order, lof)
                    second = got[:, 5] != 0
                    n = len(want_ts)
                    assert not bool(second[0]) and bool((got[~second, 4] == 1).all())
                    assert int(second.sum()) == (0 if order == 1 else n - 1 - (1 if (lof and n < 15 and n > 1) else 0))


def test_quad_at_50_steps_repeats_before_the_dedupe(tables):
    from jointimagegeneration_amd import dpm_solver as D
    raw = R.ddim_timesteps("quad", 50)
    assert len(set(raw.tolist())) < 50
    ts = D.dpm_timesteps("quad", 50, tables[0])
    assert len(ts) == len(set(raw.tolist())) and bool((np.diff(ts) > 0).all())
    sampler = D.DPMSolverSampler(stub(tables[0]))
    sampler.make_schedule(50, ddim_discretize="quad")
    assert sampler.ddim_timesteps.shape[0] == len(ts) == sampler.step_scalar_table().shape[0]
    with pytest.raises(NotImplementedError, match="no discretization method"):
        D.dpm_timesteps("cosine", 10, tables[0])


def test_schedule_tables_are_ddims_on_the_shared_grids(tables):
    """On "uniform" (no repeats) the (a_t, a_prev) pairs are DDIMSampler.make_schedule's."""
    from jointimagegeneration_amd import dpm_solver as D
    from jointimagegeneration_amd.ldm import DDIMSampler
    m = stub(tables[0])
    a, b = D.DPMSolverSampler(m), DDIMSampler(m)
    for S in STEPS:
        a.make_schedule(S, ddim_discretize="uniform")
        b.make_schedule(S, ddim_discretize="uniform", verbose=False)
        assert a.ddim_timesteps.tolist() == b.ddim_timesteps.tolist()
        assert torch.equal(a.ddim_alphas, b.ddim_alphas) and torch.equal(a.ddim_alphas_prev, b.ddim_alphas_prev)
        assert torch.equal(a.ddim_sqrt_one_minus_alphas, b.ddim_sqrt_one_minus_alphas) and not bool(a.ddim_sigmas.any())


@pytest.mark.parametrize("grid", GRIDS)
def test_first_order_is_ddim_at_eta_0(tables, grid):
    """k_x x + k_d p == sqrt(a_prev) p + sqrt(1 - a_prev) e with e = (x - alpha_s p) / sigma_s: a pure fp64 identity, held to a relative
    1e-10 (the slack covers the cancellation in sigma_t alpha_s / sigma_s)."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for ac in tables:
        for S in STEPS:
            ts = R.grid(grid, S, ac)
            want, _ = R.rows(ts, ac, 1, True)
            for (a_s, a_prev), row in zip(R.point_pairs(ts, ac), want):
                x, p = rng.standard_normal(64), rng.standard_normal(64)
                e = (x - np.sqrt(a_s) * p) / np.sqrt(1.0 - a_s)
                ddim = np.sqrt(a_prev) * p + np.sqrt(1.0 - a_prev) * e
                mine = row[2] * x + row[3] * p
                assert row[4] == 1.0 and row[5] == 0.0
                worst = max(worst, float(np.abs(mine - ddim).max() / np.abs(ddim).max()))
    print(f"first order vs DDIM on {grid}: worst relative difference {worst:.3e}")
    assert worst <= 1e-10


# ------------------------------------------------------------------------------------------------ the Gaussian toy
@pytest.mark.parametrize("s", [0.1, 0.5, 1.0])
@pytest.mark.parametrize("sched", range(3))
def test_gaussian_toy_2m_on_the_logsnr_grid_beats_ddim(tables, sched, s):
    """(a) 2M / logsnr at 20 steps has at most half the error of first order / uniform at 50 steps; (b) it has less error than first
    order / logsnr at 20 steps.  The error is the max abs difference from the closed-form probability-flow solution at alphas_cumprod[0]."""
    ac = tables[sched]
    x_T = np.random.default_rng(0).standard_normal(64)
    e_2m = R.toy_error("logsnr", 20, 2, ac, s, x_T)
    e_ddim50 = R.toy_error("uniform", 50, 1, ac, s, x_T)
    e_1_20 = R.toy_error("logsnr", 20, 1, ac, s, x_T)
    print(f"schedule {R.SCHEDULES[sched]} s = {s}: 2M/logsnr/20 {e_2m:.3e}  DDIM/uniform/50 {e_ddim50:.3e} (ratio {e_ddim50 / e_2m:.2f})  "
          f"first order/logsnr/20 {e_1_20:.3e}")
    assert 2.0 * e_2m <= e_ddim50
    assert e_2m < e_1_20


def test_product_rows_drive_the_same_toy_chain(tables):
    """The product's fp32 rows, run in fp64 as the kernel runs them (p, D, x_next), follow the restated solver to fp32 rounding: the
    row table and the order rule are the solver's, not merely self-consistent."""
    from jointimagegeneration_amd import dpm_solver as D
    ac, s = tables[0], 0.5
    eps = R.toy_eps(s)
    x_T = np.random.default_rng(0).standard_normal(64)
    for grid, S in (("logsnr", 20), ("logsnr", 10), ("uniform", 10), ("quad", 20)):
        ts = D.dpm_timesteps(grid, S, ac)
        tab = D.dpm_rows(ts, ac, 2, True).astype(np.float64)
        x, hist = x_T.copy(), None
        for i, row in enumerate(tab):
            p = (x - row[1] * eps(x, float(ac[ts[len(ts) - 1 - i]]))) / row[0]
            Dv = p if row[5] == 0 else row[4] * p + row[5] * hist
            x, hist = row[2] * x + row[3] * Dv, p
        want = R.chain(eps, x_T.copy(), R.grid(grid, S, ac), ac, 2, True)
        assert float(np.abs(x - want).max()) < 20 * len(tab) * 2.0 ** -24 * max(1.0, float(np.abs(want).max())), (grid, S)


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_fires_by_name_on_the_host(tables):
    from jointimagegeneration_amd import dpm_solver as D
    ac = tables[0]
    for bad in (0, 3, "2", None, True):
        with pytest.raises(ValueError, match="order"):
            D.DPMSolverSampler(stub(ac), order=bad)
    with pytest.raises(ValueError, match="order"):
        D.dpm_rows([1, 2], ac, 3)
    sampler = D.DPMSolverSampler(stub(ac))
    shape = (4, 8, 8)
    cases = [(dict(eta=0.5), r"DPMSolverSampler\.sample: eta = 0\.5"), (dict(temperature=0.7), "temperature = 0.7"),
             (dict(noise_dropout=0.1), "noise_dropout = 0.1"), (dict(noise_tape=[torch.zeros(2, 4, 8, 8)] * 10), "noise_tape"),
             (dict(quantize_x0=True), "quantize_x0"), (dict(score_corrector=object()), "score_corrector"),
             (dict(), r"not supported for a model on cpu")]
    for kw, pattern in cases:
        with pytest.raises(NotImplementedError, match=pattern):
            sampler.sample(10, 2, shape, verbose=False, **kw)
    split = D.DPMSolverSampler(stub(ac, split_input_params=dict(ks=(4, 4), stride=(2, 2))))
    with pytest.raises(NotImplementedError, match="split_input_params"):
        split.sample(10, 2, shape, verbose=False)
    with pytest.raises(NotImplementedError, match="split_input_params"):
        split.prepare_state(2, 4, (8, 8), torch.device("cpu"), 4)
    with pytest.raises(ValueError, match="eta = 0.3"):
        sampler.make_schedule(10, ddim_eta=0.3)
    with pytest.raises(NotImplementedError, match="a step with noise"):
        sampler._update({}, None, None, noise=torch.zeros(1))
    with pytest.raises(NotImplementedError, match="quantize_x0 / temperature"):
        sampler.prepare_state(2, 4, (8, 8), torch.device("cpu"), 4, vq=(None, 0.5))


def test_ddim_and_plms_still_refuse_x0_models_and_the_solver_takes_them(tables):
    from jointimagegeneration_amd import dpm_solver as D
    from jointimagegeneration_amd.ldm import DDIMSampler, PLMSSampler
    m = stub(tables[0])
    m.parameterization = "x0"
    for cls in (DDIMSampler, PLMSSampler):
        assert cls.parameterizations == ("eps",) and cls.state_tag == ()
        with pytest.raises(NotImplementedError, match=r"%s\.sample: parameterization 'x0' is not supported" % cls.__name__):
            cls(m).sample(10, 2, (4, 8, 8), verbose=False)
    with pytest.raises(NotImplementedError, match="not supported for a model on cpu"):          # past the parameterization check
        D.DPMSolverSampler(m).sample(10, 2, (4, 8, 8), verbose=False)
    a, b = D.DPMSolverSampler(m), D.DPMSolverSampler(m, order=1)
    assert a.state_tag != b.state_tag and a.state_tag[0][0] == "dpm_solver" and a.fuse_ddim is False


# ------------------------------------------------------------------------------------------------ entry points
def test_the_reference_path_resolves_to_the_sampler():
    from jointimagegeneration_amd import config, dpm_solver
    assert config.get_obj_from_str("ldm.models.diffusion.dpm_solver.DPMSolverSampler") is dpm_solver.DPMSolverSampler


def test_sample_diffusion_options():
    from jointimagegeneration_amd import sample_diffusion as sd
    parse = sd.get_parser().parse_args
    assert sd.sampler_from_options(parse([])) == ("ddim", None) and sd.sampler_from_options(parse(["--plms"])) == ("plms", None)
    assert sd.sampler_from_options(parse(["--plms", "--sampler", "plms", "--discretize", "quad"])) == ("plms", "quad")
    assert sd.sampler_from_options(parse(["--sampler", "dpmpp_2m", "-c", "20"])) == ("dpmpp_2m", None)
    assert sd.sampler_from_options(parse(["--sampler", "dpmpp_2m", "--discretize", "uniform"])) == ("dpmpp_2m", "uniform")
    for argv, msg in ((["--plms", "--sampler", "ddim"], "--plms contradicts --sampler ddim"),
                      (["--plms", "--sampler", "dpmpp_2m"], "--plms contradicts --sampler dpmpp_2m"),
                      (["--sampler", "dpmpp_2m", "-e", "0.5"], r"--sampler dpmpp_2m: eta = 0\.5"),
                      (["--sampler", "dpmpp_2m", "-v"], "contradicts -v"),
                      (["--sampler", "ddim", "--discretize", "logsnr"], "not a grid of the ddim sampler"),
                      (["--plms", "--discretize", "logsnr"], "not a grid of the plms sampler")):
        with pytest.raises(SystemExit, match=msg):
            sd.main(["--config", "none.yaml"] + argv)
    with pytest.raises(SystemExit):
        parse(["--sampler", "euler"])
    from jointimagegeneration_amd.dpm_solver import DPMSolverSampler
    from jointimagegeneration_amd.ldm import DDIMSampler, PLMSSampler
    m = stub(R.alphas_cumprod(*R.SCHEDULES[0]))
    assert [type(sd.make_sampler(m, n)) for n in ("ddim", "plms", "dpmpp_2m")] == [DDIMSampler, PLMSSampler, DPMSolverSampler]


def test_pipeline_options(capsys):
    from jointimagegeneration_amd import pipeline as P
    P.check_sampler_options("ddim", None)
    P.check_sampler_options("dpmpp_2m", "logsnr")
    with pytest.raises(ValueError, match="sampler = 'plms' is not one of ddim, dpmpp_2m"):
        P.check_sampler_options("plms", None)
    with pytest.raises(ValueError, match="discretize = 'logsnr' is not a grid of the ddim sampler"):
        P.check_sampler_options("ddim", "logsnr")
    with pytest.raises(SystemExit):
        P.main(["--volumes", "1", "--sampler", "ddim", "--discretize", "logsnr"])
    assert "not a grid of the ddim sampler" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        P.main(["--volumes", "1", "--sampler", "plms"])


def test_pipeline_builds_the_chosen_sampler_and_defaults_to_ddim():
    from jointimagegeneration_amd.dpm_solver import DPMSolverSampler
    from jointimagegeneration_amd.ldm import DDIMSampler
    from jointimagegeneration_amd.pipeline import GuideGenPipeline
    from util import small_ldm
    m = small_ldm()
    pipe = GuideGenPipeline(None, m, ddim_steps=8)
    assert type(pipe.sampler) is DDIMSampler and (pipe.sampler_name, pipe.discretize, pipe.steps) == ("ddim", "uniform", 8)
    fast = GuideGenPipeline(None, m, ddim_steps=8, sampler="dpmpp_2m")
    assert type(fast.sampler) is DPMSolverSampler and (fast.sampler_name, fast.discretize) == ("dpmpp_2m", "logsnr") and 1 < fast.steps <= 8
    assert fast.sampler.ddim_timesteps.tolist() == R.grid("logsnr", 8, m.alphas_cumprod.float().numpy()).tolist()
    quad = GuideGenPipeline(None, m, ddim_steps=8, sampler="dpmpp_2m", discretize="quad")
    assert quad.discretize == "quad" and quad.sampler.ddim_timesteps.tolist() == R.grid("quad", 8, m.alphas_cumprod.float().numpy()).tolist()
    with pytest.raises(ValueError, match="sampler = 'euler'"):
        GuideGenPipeline(None, m, sampler="euler")
    with pytest.raises(NotImplementedError, match="CT editing runs the DDIM sampler"):
        fast._check_edit(1, 4, 32, torch.zeros(1, 4, 32, 32), torch.zeros(1, 4, 32, 32, dtype=torch.bool), 0, None)


# ------------------------------------------------------------------------------------------------ C-ABI
def test_gg_dpm_solver_step_rejects_bad_arguments_on_the_host():
    """Every check runs before a launch, so the codes are observable without a GPU (the fake pointers are never read)."""
    from util import load_lib
    lib = load_lib()
    p, bad_shape, unsupported = 0x1000, -1, -3
    step = lib.gg_dpm_solver_step
    # (x, out, out_stride, scalars, flags, M, C, hist, pred_x0_out, unet_in, unet_in_stride, stream)
    good = [p, p, 32, p, 0, 16, 4, p, p, p, 32, None]
    for i in (0, 1, 3, 7):                                                                     # null x, out, scalars, hist
        a = list(good)
        a[i] = None
        assert step(*a) == bad_shape, i
        assert b"null" in lib.gg_last_error()
    assert step(p, p, 3, p, 0, 16, 4, p, None, None, 0, None) == bad_shape and b"out_stride" in lib.gg_last_error()
    assert step(p, p, 32, p, 0, 16, 4, p, None, p, 3, None) == bad_shape and b"unet_in_stride" in lib.gg_last_error()
    assert step(p, p, 32, p, 0, 16, 0, p, None, None, 0, None) == bad_shape
    assert step(p, p, 32, p, 0, -1, 4, p, None, None, 0, None) == bad_shape
    for flags in (4, 8, 7, -1):
        assert step(p, p, 32, p, flags, 16, 4, p, None, None, 0, None) == unsupported, flags
        assert b"flag" in lib.gg_last_error()
    for flags in (0, 1, 2, 3):                                                                  # M = 0: nothing to do, no launch
        assert step(p, p, 32, p, flags, 0, 4, p, None, p, 32, None) == 0
        assert step(p, p, 3, p, flags, 0, 3, p, p, None, 0, None) == 0
    # one unit per lane on an exact grid: more than 2^31 - 1 workgroups of 256 is refused, for rows (aligned C = 4) and for elements
    cap = (2 ** 31 - 1) * 256
    assert step(p, p, 32, p, 0, cap + 1, 4, p, None, None, 0, None) == unsupported and b"exceed the grid" in lib.gg_last_error()
    assert step(p, p, 32, p, 0, cap // 3 + 1, 3, p, None, None, 0, None) == unsupported
    assert step(p + 4, p, 32, p, 0, cap // 4 + 1, 4, p, None, None, 0, None) == unsupported          # misaligned x: per element
