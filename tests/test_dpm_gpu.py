"""GPU suite of the DPM-Solver++ (2M) sampler: gg_dpm_solver_step bit for bit against its expression as separate fp32 torch ops
(tests/dpm_ref.py: torch_step) on both kernel shapes, the chain's arithmetic bit for bit and teacher-forced (every logged x from the
logged x before it, the logged predictions of x_0 and the row table), the captured chain against the eager one, the state keys, and the
pipeline's slice loop on the new sampler.  Everything is exact: there is no tolerance in this file."""
import pytest
import torch

import dpm_ref as R
from util import synth_labels

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
SHAPE = (4, 8, 8)
N, S = 2, 10
FIRST = [0.6234898, 0.7818315, 0.9127341, 0.1532907, 1.0, 0.0]           # {alpha_s, sigma_s, k_x, k_d, c0, c1}; alpha^2 + sigma^2 = 1
SECOND = FIRST[:4] + [1.4142135, -0.4142135]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def small(dev):
    from util import small_ldm
    return small_ldm().to(dev)


@pytest.fixture(scope="module")
def small_x0(dev):
    from progressive_ref import ldm_small
    return ldm_small(1000, parameterization="x0", use_ema=False).to(dev)          # the weights of `small`, the output read as x_0


@pytest.fixture(scope="module")
def operands(dev):
    g = torch.Generator(device=dev).manual_seed(5)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    mask = torch.ones((N, 1) + SHAPE[1:], device=dev)
    mask[:, :, 2:6, 3:7] = 0.0
    mask[:, :, 0, 0] = 0.25                                              # a soft value
    return dict(c=r(N, *SHAPE), c2=r(N, *SHAPE), uc=torch.zeros((N,) + SHAPE, device=dev), x_T=r(N, *SHAPE), x_T2=r(N, *SHAPE),
                x0=r(N, *SHAPE), mask=mask, q=[r(N, *SHAPE) for _ in range(S)])


# ------------------------------------------------------------------------------------------------ kernel
def step_case(dev, M, C, stride, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(M, C, device=dev, generator=g) * 1.5               # |p| crosses 1 on a good share of the elements
    out = torch.randn(M, stride, device=dev, generator=g)
    hist = torch.randn(M, C, device=dev, generator=g)
    return x, out, hist


@pytest.mark.parametrize("M,C,stride,vector", [(1030, 4, 32, True), (1030, 4, 6, False), (257, 3, 5, False), (1, 8, 8, False)],
                         ids=["C4_rows_M1030", "C4_unaligned_out_stride", "C3_M257", "C8_M1"])
@pytest.mark.parametrize("flags", [0, 1, 2, 3], ids=["eps", "x0", "eps_clip", "x0_clip"])
def test_step_kernel_is_bit_equal_to_the_torch_expression(dev, M, C, stride, vector, flags):
    from jointimagegeneration_amd import ops
    x0_, out, hist0 = step_case(dev, M, C, stride, M * 13 + C * 5 + flags)
    assert (C == 4 and x0_.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and stride % 4 == 0) == vector
    out_before = out.clone()
    for row in (FIRST, SECOND):
        sc = torch.tensor(row, device=dev)
        want_x, want_p = R.torch_step(x0_, out[:, :C], hist0, sc, flags)
        if flags & 2 and M > 1:
            assert bool((want_p.abs() == 1.0).any()) and bool((want_p.abs() < 1.0).any())
        for with_p0 in (True, False):
            for with_uin in (True, False):
                x, hist = x0_.clone(), hist0.clone()
                p0 = torch.full((M, C), 9.0, device=dev) if with_p0 else None
                uin = torch.full((M, 32), 7.0, dtype=torch.bfloat16, device=dev) if with_uin else None      # pad lanes: a sentinel that must survive
                ops.dpm_solver_step(x, out, sc, hist, predicts_x0=bool(flags & 1), clip=bool(flags & 2), pred_x0_out=p0, unet_in=uin)
                torch.cuda.synchronize()
                tag = (row[5], with_p0, with_uin)
                assert torch.equal(x, want_x), tag
                assert torch.equal(hist, want_p), tag
                if with_p0:
                    assert torch.equal(p0, want_p), tag
                if with_uin:
                    assert torch.equal(uin[:, :C], want_x.bfloat16()) and bool((uin[:, C:] == 7.0).all()), tag
                assert torch.equal(out, out_before), tag                 # channels >= C of the UNet's output included


@pytest.mark.parametrize("C,stride", [(4, 32), (3, 5)], ids=["rows", "elements"])
def test_first_order_step_does_not_read_the_history(dev, C, stride):
    """c1 == 0 with hist full of NaN: the result is finite and is the first-order expression; hist then holds p."""
    from jointimagegeneration_amd import ops
    M = 1030
    x0_, out, _ = step_case(dev, M, C, stride, 99 + C)
    sc = torch.tensor(FIRST, device=dev)
    want_x, want_p = R.torch_step(x0_, out[:, :C], None, sc, 0)
    x, hist = x0_.clone(), torch.full((M, C), float("nan"), device=dev)
    uin = torch.zeros((M, 32), dtype=torch.bfloat16, device=dev)
    ops.dpm_solver_step(x, out, sc, hist, unet_in=uin)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and torch.equal(x, want_x) and torch.equal(hist, want_p) and torch.equal(uin[:, :C], want_x.bfloat16())


def test_misaligned_rows_take_the_element_kernel(dev):
    """C = 4 rows at a one-float offset and a unet_in stride that is no multiple of 4: the same bits, and nothing in front of the views."""
    from jointimagegeneration_amd import ops
    M = 1030
    g = torch.Generator(device=dev).manual_seed(77)
    flat = torch.randn(3, M * 4 + 1, device=dev, generator=g)
    col0 = flat[:, 0].clone()
    x, hist, p0 = (flat[i, 1:].view(M, 4) for i in range(3))
    assert x.data_ptr() % 16 != 0 and x.is_contiguous()
    out = torch.randn(M, 4, device=dev, generator=g)
    sc = torch.tensor(SECOND, device=dev)
    want_x, want_p = R.torch_step(x.clone(), out, hist.clone(), sc, 2)
    uin = torch.full((M, 6), -3.0, dtype=torch.bfloat16, device=dev)
    ops.dpm_solver_step(x, out, sc, hist, clip=True, pred_x0_out=p0, unet_in=uin)
    torch.cuda.synchronize()
    assert torch.equal(x, want_x) and torch.equal(p0, want_p) and torch.equal(hist, want_p)
    assert torch.equal(uin[:, :4], want_x.bfloat16()) and bool((uin[:, 4:] == -3.0).all()) and torch.equal(flat[:, 0], col0)


def test_empty_step_launches_nothing_and_the_error_codes(dev):
    from jointimagegeneration_amd import _lib, ops
    lib = _lib.load()
    x, out, hist = step_case(dev, 16, 4, 32, 3)
    sc = torch.tensor(SECOND, device=dev)
    keep = [t.clone() for t in (x, out, hist)]
    args = lambda M, flags=0, C=4, stride=32: (x.data_ptr(), out.data_ptr(), stride, sc.data_ptr(), flags, M, C, hist.data_ptr(), None, None, 0, None)
    assert lib.gg_dpm_solver_step(*args(0)) == 0                          # M == 0: GG_OK, no launch
    assert lib.gg_dpm_solver_step(*args(16, flags=4)) == _lib.GG_ERR_UNSUPPORTED
    assert lib.gg_dpm_solver_step(*args(16, stride=3)) == _lib.GG_ERR_BAD_SHAPE
    assert lib.gg_dpm_solver_step(x.data_ptr(), out.data_ptr(), 32, sc.data_ptr(), 0, 16, 4, None, None, None, 0, None) == _lib.GG_ERR_BAD_SHAPE
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((x, out, hist), keep))
    with pytest.raises(ValueError, match="hist must be contiguous fp32"):
        ops.dpm_solver_step(x, out, sc, hist[:8])
    with pytest.raises(ValueError, match="six fp32 values"):
        ops.dpm_solver_step(x, out, sc[:4], hist)


# ------------------------------------------------------------------------------------------------ chain arithmetic, teacher-forced
def blend(x, x0, noise, mask, a, b):
    """gg_inpaint_blend's expression as separate fp32 torch ops."""
    t1 = a * x0
    t2 = b * noise
    o = t1 + t2
    p = o * mask
    q = (1.0 - mask) * x
    return p + q


def check_teacher_forced(sampler, z, logs, x_T, dev, inpaint=None):
    """Every logged x after step i == k_x * (x before it, blended first under inpainting) + k_d * D, D from the logged predictions of
    steps i and i - 1 and row i of the table, as separate fp32 torch ops.  Returns the number of second-order steps."""
    tab = sampler.step_scalar_table().to(dev)
    xs, ps = logs["x_inter"], logs["pred_x0"]
    n = tab.shape[0]
    assert n == sampler.ddim_timesteps.shape[0] and len(xs) == len(ps) == n + 1, (n, len(xs), len(ps))
    assert torch.equal(xs[0], x_T) and torch.equal(xs[-1], z)
    q_scal = sampler.q_sample_scalar_table().to(dev) if inpaint is not None else None
    for i in range(n):
        x = xs[i]
        if inpaint is not None:
            x = blend(x, inpaint["x0"], inpaint["q"][i], inpaint["mask"], q_scal[i, 0], q_scal[i, 1])
        want, _ = R.torch_step(x, ps[i + 1], ps[i], tab[i], 1)              # flag 1: the logged prediction is p itself
        assert torch.equal(xs[i + 1], want), f"step {i} of {n}: {int((xs[i + 1] != want).sum())} elements differ"
    return int((tab[:, 5] != 0).sum())


def run_logged(sampler, c, x_T, **kw):
    return sampler.sample(S, N, tuple(x_T.shape[1:]), conditioning=c, x_T=x_T, log_every_t=1, verbose=False, **kw)


def test_chain_is_the_solver_bit_for_bit(dev, small, operands):
    from jointimagegeneration_amd.dpm_solver import DPMSolverSampler
    sampler = DPMSolverSampler(small)
    z, logs = run_logged(sampler, operands["c"], operands["x_T"])
    second = check_teacher_forced(sampler, z, logs, operands["x_T"], dev)
    n = sampler.ddim_timesteps.shape[0]
    assert 3 <= n <= S and second == n - 2                                # first and (fewer than 15 steps) last step are first order
    assert sampler.ddim_timesteps.tolist() == R.grid("logsnr", S, small.alphas_cumprod.float().cpu().numpy()).tolist()
    assert sampler.last_step_fused is False
    # the default lists: two entries, the same final tensors
    z2, two = sampler.sample(S, N, SHAPE, conditioning=operands["c"], x_T=operands["x_T"], verbose=False)
    assert torch.equal(z2, z) and len(two["x_inter"]) == 2 and torch.equal(two["pred_x0"][1], logs["pred_x0"][-1])
    # order 1 and the other grids run the same kernel
    for kw, grid in ((dict(order=1), "logsnr"), (dict(lower_order_final=False), "uniform"), (dict(), "quad")):
        s1 = DPMSolverSampler(small, **kw)
        z1, l1 = run_logged(s1, operands["c"], operands["x_T"], ddim_discretize=grid)
        n1 = s1.ddim_timesteps.shape[0]
        assert check_teacher_forced(s1, z1, l1, operands["x_T"], dev) == (0 if "order" in kw else n1 - 1 if "lower_order_final" in kw else n1 - 2)


def test_chain_with_guidance_inpainting_and_callbacks(dev, small, operands):
    from jointimagegeneration_amd.dpm_solver import DPMSolverSampler
    sampler = DPMSolverSampler(small)
    z, logs = run_logged(sampler, operands["c"], operands["x_T"], unconditional_conditioning=operands["uc"], unconditional_guidance_scale=2.0)
    assert check_teacher_forced(sampler, z, logs, operands["x_T"], dev) >= 1
    plain, _ = run_logged(sampler, operands["c"], operands["x_T"])
    assert not torch.equal(plain, z)                                       # the guidance did something
    ip = dict(x0=operands["x0"], mask=operands["mask"], q=operands["q"])
    z, logs = run_logged(sampler, operands["c"], operands["x_T"], mask=operands["mask"], x0=operands["x0"], mask_noise_tape=operands["q"])
    assert check_teacher_forced(sampler, z, logs, operands["x_T"], dev, inpaint=ip) >= 1
    z_g, logs_g = run_logged(sampler, operands["c"], operands["x_T"], mask=operands["mask"], x0=operands["x0"], mask_noise_tape=operands["q"],
                             unconditional_conditioning=operands["uc"], unconditional_guidance_scale=2.0)
    assert check_teacher_forced(sampler, z_g, logs_g, operands["x_T"], dev, inpaint=ip) >= 1
    # clip_denoised: every prediction inside [-1, 1], some on the border, and the same arithmetic
    z_c, logs_c = run_logged(sampler, operands["c"], operands["x_T"] * 3.0, clip_denoised=True)
    check_teacher_forced(sampler, z_c, logs_c, operands["x_T"] * 3.0, dev)
    allp = torch.stack(logs_c["pred_x0"][1:])
    assert float(allp.abs().max()) == 1.0 and sampler.clip_denoised is False
    # callbacks: called after every step, the chain runs eagerly with the same bits
    seen, imgs = [], []
    z_cb, _ = run_logged(sampler, operands["c"], operands["x_T"], callback=seen.append, img_callback=lambda p, i: imgs.append(p.clone()))
    n = sampler.ddim_timesteps.shape[0]
    assert seen == list(range(n)) and len(imgs) == n and torch.equal(z_cb, plain)
    # log_every_t: the reference's rule on the chain's own step count
    from jointimagegeneration_amd.ldm import logged_steps
    _, l3 = sampler.sample(S, N, SHAPE, conditioning=operands["c"], x_T=operands["x_T"], log_every_t=3, verbose=False)
    assert len(l3["x_inter"]) == 1 + len(logged_steps(n, 3))


def test_chain_on_an_x0_model(dev, small, small_x0, operands):
    from jointimagegeneration_amd.dpm_solver import DPMSolverSampler
    from jointimagegeneration_amd.ldm import DDIMSampler
    sampler = DPMSolverSampler(small_x0)
    z, logs = run_logged(sampler, operands["c"], operands["x_T"])
    assert check_teacher_forced(sampler, z, logs, operands["x_T"], dev) >= 1
    # the first prediction is the UNet's output itself.  The eps model of the `small` fixture has the same weights, so its first step
    # saw the same output `out` and logged p = (x_T - sigma_s out) / alpha_s: out = (x_T - alpha_s p) / sigma_s up to the roundings of
    # these few fp32 operations (a few ulp of the terms, |alpha_s p| <= |x_T| + |out|): held to 1e-5 of the largest value
    _, logs_eps = run_logged(DPMSolverSampler(small), operands["c"], operands["x_T"])
    tab = sampler.step_scalar_table().to(dev)
    out = (operands["x_T"] - tab[0, 0] * logs_eps["pred_x0"][1]) / tab[0, 1]
    diff = float((out - logs["pred_x0"][1]).abs().max())
    print(f"x0 model: first prediction vs the eps model's output, max abs {diff:.3e} of {float(out.abs().max()):.3e}")
    assert diff <= 1e-5 * max(float(out.abs().max()), float(operands["x_T"].abs().max()))
    with pytest.raises(NotImplementedError, match="parameterization 'x0'"):
        DDIMSampler(small_x0).sample(S, N, SHAPE, conditioning=operands["c"], verbose=False)


def test_chain_on_a_3d_latent(dev):
    from jointimagegeneration_amd.dpm_solver import DPMSolverSampler
    from jointimagegeneration_amd.ldm import LatentDiffusion
    from util import seeded
    ae = dict(target="ldm.models.autoencoder.AutoencoderKL",
              params=dict(embed_dim=4, dims=3, lossconfig=dict(target="torch.nn.Identity"),
                          ddconfig=dict(double_z=True, z_channels=4, resolution=8, in_channels=1, out_ch=1, ch=32, ch_mult=[1, 2], num_res_blocks=1,
                                        dropout=0.0, dims=3, attn_resolutions=[4])))
    unet = dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel",
                params=dict(image_size=8, in_channels=8, out_channels=4, model_channels=32, attention_resolutions=[2], num_res_blocks=1,
                            channel_mult=[1, 2], num_head_channels=32, dims=3))
    m = seeded(LatentDiffusion(first_stage_config=ae, cond_stage_config=ae, unet_config=unet, linear_start=0.0015, linear_end=0.0195, timesteps=300,
                               image_size=8, channels=4, dims=3, first_stage_key="image", cond_stage_key="mask", num_timesteps_cond=1,
                               conditioning_key="concat"), "ldm3d.").to(dev)
    g = torch.Generator(device=dev).manual_seed(8)
    shape = (N, 4, 4, 8, 8)
    c, x_T = torch.randn(shape, device=dev, generator=g), torch.randn(shape, device=dev, generator=g)
    sampler = DPMSolverSampler(m)
    z, logs = run_logged(sampler, c, x_T)
    assert tuple(z.shape) == shape and check_teacher_forced(sampler, z, logs, x_T, dev) >= 1


# ------------------------------------------------------------------------------------------------ graph and state
def test_captured_chain_equals_the_eager_one_and_is_replayed(dev, small, operands):
    from jointimagegeneration_amd.dpm_solver import DPMSolverSampler
    from jointimagegeneration_amd.ldm import DDIMSampler
    eager = DPMSolverSampler(small)
    eager.use_graph = False
    want = [eager.sample(S, N, SHAPE, conditioning=c, x_T=x, verbose=False) for c, x in ((operands["c"], operands["x_T"]), (operands["c2"], operands["x_T2"]))]
    assert all(st["graph"] is None for st in eager._graphs.values())
    sampler = DPMSolverSampler(small)
    for k in range(3):                                                     # eager warm-up, capture + replay, replay
        z, d = sampler.sample(S, N, SHAPE, conditioning=operands["c"], x_T=operands["x_T"], verbose=False)
        assert torch.equal(z, want[0][0]) and torch.equal(d["pred_x0"][1], want[0][1]["pred_x0"][1]), k
    assert len(sampler._graphs) == 1
    st = next(iter(sampler._graphs.values()))
    graph = st["graph"]
    assert graph is not None and "hist" in st and tuple(st["scal"].shape) == (sampler.ddim_timesteps.shape[0], 6)
    z, d = sampler.sample(S, N, SHAPE, conditioning=operands["c2"], x_T=operands["x_T2"], verbose=False)      # new operands, the same graph
    assert torch.equal(z, want[1][0]) and torch.equal(d["pred_x0"][1], want[1][1]["pred_x0"][1])
    assert len(sampler._graphs) == 1 and st["graph"] is graph
    # a logged chain is a state (and a graph) of its own and replays to the same bits
    for k in range(3):
        zl, dl = run_logged(sampler, operands["c"], operands["x_T"])
        assert torch.equal(zl, want[0][0]) and check_teacher_forced(sampler, zl, dl, operands["x_T"], dev) >= 1
    assert len(sampler._graphs) == 2 and all(s["graph"] is not None for s in sampler._graphs.values())
    # clip_denoised is baked into a captured chain: a key of its own
    sampler.sample(S, N, SHAPE, conditioning=operands["c"], x_T=operands["x_T"], verbose=False, clip_denoised=True)
    assert len(sampler._graphs) == 3
    # a DDIM sampler on the same model shares nothing with it
    ddim = DDIMSampler(small)
    zd, _ = ddim.sample(S, N, SHAPE, conditioning=operands["c"], x_T=operands["x_T"], verbose=False)
    assert not torch.equal(zd, want[0][0]) and ddim._graphs is not sampler._graphs and not (set(ddim._graphs) & set(sampler._graphs))
    assert all("hist" not in s and s["scal"].shape[1] == 4 for s in ddim._graphs.values())
    assert all(s["x"].data_ptr() != st["x"].data_ptr() for s in ddim._graphs.values())


def test_first_order_chain_is_close_to_ddim(dev, small, operands):
    """order = 1 on DDIM's own grid is DDIM at eta 0 algebraically: the fp32 chains differ by rounding through a bf16 UNet only.  The
    bound is the one the existing chain tests hold DDIM itself to against the reference on this network (max 2e-2, rms 1.5e-2)."""
    from jointimagegeneration_amd.dpm_solver import DPMSolverSampler
    from jointimagegeneration_amd.ldm import DDIMSampler
    from util import rel_err, rms_err
    a, la = run_logged(DPMSolverSampler(small, order=1), operands["c"], operands["x_T"], ddim_discretize="uniform")
    b, lb = run_logged(DDIMSampler(small), operands["c"], operands["x_T"])
    print(f"first order vs DDIM, {S} uniform steps: max {rel_err(a, b):.3e} rms {rms_err(a, b):.3e}")
    assert rel_err(a, b) < 2e-2 and rms_err(a, b) < 1.5e-2
    # the first step sees the same x_T, so the same eps bits: the two predictions of x_0 are the same expression with alpha_s, sigma_s
    # rounded from fp64 on one side and fp32 roots on the other, an ulp apart at most: held to 1e-5
    first = rel_err(la["pred_x0"][1], lb["pred_x0"][1])
    print(f"first prediction of x_0, solver vs DDIM: max rel {first:.3e}")
    assert first < 1e-5


def test_batch_elements_are_independent(dev, small, operands):
    from jointimagegeneration_amd.dpm_solver import DPMSolverSampler
    sampler = DPMSolverSampler(small)
    z, _ = sampler.sample(S, N, SHAPE, conditioning=operands["c"], x_T=operands["x_T"], verbose=False)
    c, x = operands["c"].clone(), operands["x_T"].clone()
    c[1], x[1] = operands["c2"][1], operands["x_T2"][1] * 2.0
    for k in range(2):                                                     # eager, then captured
        z2, _ = sampler.sample(S, N, SHAPE, conditioning=c, x_T=x, verbose=False)
        assert torch.equal(z2[0], z[0]) and not torch.equal(z2[1], z[1]), k


# ------------------------------------------------------------------------------------------------ pipeline
def pipeline_labels(dev):
    lab = synth_labels((5, 16, 16), 12, seed=2)
    lab[0, 3:9, 4:12] = 7
    lab[3:] = 0
    return torch.from_numpy(lab).int()[None].to(dev)


def test_pipeline_slice_loop_on_the_solver_graph_equals_eager(dev, small):
    from jointimagegeneration_amd.dpm_solver import DPMSolverSampler
    from jointimagegeneration_amd.pipeline import GuideGenPipeline
    labels = pipeline_labels(dev)
    depth, hw, seed = 7, 32, 4242
    out, vol = {}, {}
    for use_graph in (True, False):
        pipe = GuideGenPipeline(None, small, ddim_steps=8, sampler="dpmpp_2m")
        assert type(pipe.sampler) is DPMSolverSampler and pipe.discretize == "logsnr" and 3 <= pipe.steps <= 8
        pipe.use_graph = pipe.sampler.use_graph = use_graph
        out[use_graph] = pipe.sample_ct(labels, depth, hw, seed)
        vol[use_graph] = pipe.sample_ct_volumes(labels, depth, hw, [seed])
        if use_graph:      # slices after the first are ONE captured graph each: cond-encode + all solver steps + decode
            assert pipe._slice_graphs and all(sg["slice"] is not None for sg in pipe._slice_graphs.values())
            assert pipe._volume_graphs and all(ve["graph"] is not None for ve in pipe._volume_graphs.values())
            stages = pipe.time_slice_stages(N=1, hw=hw)
            assert set(stages) == {"encode_ms", "ddim_step_ms", "decode_ms"} and stages["ddim_step_ms"] > 0
    assert torch.equal(out[True], out[False]) and float(out[True].abs().max()) > 0
    assert torch.equal(vol[True], vol[False])
    # the batched loop at B = 1 runs the same chain; its normalise + scatter is another kernel (the bound of test_volumes_gpu's
    # batched-against-solo comparison)
    assert float((vol[True] - out[True]).abs().max()) < 2e-2
    with pytest.raises(NotImplementedError, match="CT editing runs the DDIM sampler"):
        pipe.sample_ct_volumes(labels, depth, hw, [seed], known_ct=torch.zeros(1, depth, hw, hw, device=dev),
                               keep=torch.zeros(1, depth, hw, hw, dtype=torch.bool, device=dev))


def test_default_pipeline_is_unchanged_ddim(dev, small):
    """Built without the new keywords and with them at their defaults: a DDIMSampler either way, the same bits, the fused head."""
    from jointimagegeneration_amd.ldm import DDIMSampler
    from jointimagegeneration_amd.pipeline import GuideGenPipeline
    labels = pipeline_labels(dev)
    a = GuideGenPipeline(None, small, ddim_steps=5)
    b = GuideGenPipeline(None, small, ddim_steps=5, sampler="ddim", discretize=None)
    assert type(a.sampler) is DDIMSampler and type(b.sampler) is DDIMSampler and a.sampler.state_tag == () and a.steps == b.steps == 5
    assert a.sampler.ddim_timesteps.tolist() == b.sampler.ddim_timesteps.tolist() == [1, 201, 401, 601, 801]
    ct_a, ct_b = a.sample_ct(labels, 7, 32, 4242), b.sample_ct(labels, 7, 32, 4242)
    assert torch.equal(ct_a, ct_b) and a.sampler.last_step_fused == b.sampler.last_step_fused
    assert all("hist" not in st and st["scal"].shape[1] == 4 for st in a.sampler._graphs.values())
    fast = GuideGenPipeline(None, small, ddim_steps=5, sampler="dpmpp_2m")
    assert not torch.equal(fast.sample_ct(labels, 7, 32, 4242), ct_a)


def test_the_head_conv_is_never_asked_for_the_ddim_update(dev, small, operands):
    """fuse_ddim set to True on the solver changes nothing: the head conv's epilogue is DDIM's update, which the class never asks for."""
    from jointimagegeneration_amd.dpm_solver import DPMSolverSampler
    from jointimagegeneration_amd.ldm import DDIMSampler
    unet = small.model.diffusion_model
    asked = []
    unet.forward_cl = lambda *a, **k: (asked.append(k.get("head_ddim")), type(unet).forward_cl(unet, *a, **k))[1]
    try:
        want, _ = DPMSolverSampler(small).sample(S, N, SHAPE, conditioning=operands["c"], x_T=operands["x_T"], verbose=False)
        sampler = DPMSolverSampler(small)
        sampler.fuse_ddim = True
        for k in range(3):                                                 # eager warm-up, capture + replay, replay
            z, _ = sampler.sample(S, N, SHAPE, conditioning=operands["c"], x_T=operands["x_T"], verbose=False)
            assert torch.equal(z, want) and sampler.last_step_fused is False, k
        assert len(asked) >= 3 * sampler.ddim_timesteps.shape[0] and all(h is None for h in asked)
        assert DPMSolverSampler.head_update_is_ddim is False and DDIMSampler.head_update_is_ddim is True
        del asked[:]
        DDIMSampler(small).sample(S, N, SHAPE, conditioning=operands["c"], x_T=operands["x_T"], verbose=False)
        assert asked and all(h is not None for h in asked)                 # the wrapper does see DDIM's request
    finally:
        del unet.forward_cl
