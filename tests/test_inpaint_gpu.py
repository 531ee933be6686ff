"""GPU suite for latent inpainting (mask= / x0=): the gg_inpaint_blend kernel bit for bit against the separate-op torch expression, the
DDIM / guided DDIM / PLMS / ancestral samplers against what the REFERENCE samplers produced from the same tapes (tests/golden/inpaint.npz,
make_golden_inpaint.py), the engine's bit-exact invariants (captured == eager, graph reuse with new operands, all-zero mask == no mask,
no state leaking into mask-free calls), encode_first_stage, and the full-size latent UNet.

Tolerances are those of the existing chain tests (tests/test_hip_parity.py): bf16 networks inside 5 to 20 step chains."""
import numpy as np
import pytest
import torch

from util import AE_SMALL, LDM_FULL, LDM_SMALL, SEED, T, gold, rel_err, rms_err, seeded

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def ldm_small(dev, timesteps=1000):
    """The LatentDiffusion of make_golden_inpaint.py (= make_golden.py fx_ddim_options), "ldm_pipe." weights."""
    from jointimagegeneration_amd.ldm import LatentDiffusion
    cfg_unet = dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(LDM_SMALL))
    ae = lambda cin: dict(target="ldm.models.autoencoder.AutoencoderKL",
                          params=dict(embed_dim=4, dims=2, ddconfig=dict(AE_SMALL, in_channels=cin, out_ch=cin), lossconfig=dict(target="torch.nn.Identity")))
    m = LatentDiffusion(first_stage_config=ae(1), cond_stage_config=ae(2), unet_config=cfg_unet, linear_start=0.0015, linear_end=0.0195,
                        timesteps=timesteps, image_size=8, channels=4, dims=2, first_stage_key="image", cond_stage_key="mask",
                        num_timesteps_cond=1)
    return seeded(m, "ldm_pipe.").to(dev)


@pytest.fixture(scope="module")
def small(dev):
    return ldm_small(dev)


@pytest.fixture(scope="module")
def g():
    return gold("inpaint")


def tape(g, name, n, dev):
    return list(T(g[name]).float()[:n].to(dev))


# ------------------------------------------------------------------------------------------------ kernel
def torch_blend(x, x0, mask, noise, sc):
    """The reference's expression (ddpm.py:275-278 + ddim.py:147-148) as separate fp32 torch ops on the GPU."""
    t1 = sc[0] * x0
    t2 = sc[1] * noise
    o = t1 + t2
    p = o * mask
    q = (1.0 - mask) * x
    return p + q


@pytest.mark.parametrize("M", [1000, 2 ** 20 + 3], ids=["M1000", "M2^20+3"])
@pytest.mark.parametrize("C,mask_C", [(4, 1), (4, 4), (3, 1), (3, 3)])
@pytest.mark.parametrize("with_unet_in", [False, True], ids=["x_only", "unet_in"])
def test_blend_kernel_is_bit_equal_to_the_torch_expression(dev, M, C, mask_C, with_unet_in):
    from jointimagegeneration_amd import ops
    gen = torch.Generator(device=dev).manual_seed(M * 31 + C * 7 + mask_C)
    x = torch.randn(M, C, device=dev, generator=gen)
    x0 = torch.randn(M, C, device=dev, generator=gen)
    noise = torch.randn(M, C, device=dev, generator=gen)
    mask = torch.rand(M, mask_C, device=dev, generator=gen)                     # soft values in [0, 1)
    mask[: M // 4] = (mask[: M // 4] > 0.5).float()                              # and hard 0 / 1 rows
    sc = torch.tensor([0.7834521, 0.6214398], device=dev)
    want = torch_blend(x, x0, mask, noise, sc)
    uin = None
    if with_unet_in:
        uin = torch.full((M, 32), 7.0, dtype=torch.bfloat16, device=dev)        # pad lanes hold a sentinel that must survive
    ops.inpaint_blend(x, x0, mask, noise, sc, unet_in=uin)
    torch.cuda.synchronize()
    assert torch.equal(x, want)
    if with_unet_in:
        assert torch.equal(uin[:, :C], want.bfloat16())
        assert bool((uin[:, C:] == 7.0).all())


def test_blend_kernel_unaligned_rows_take_the_scalar_path(dev):
    """C = 4 rows that are not 16-byte aligned (a view at a 1-float offset) and a unet_in stride that is not a multiple of 4."""
    from jointimagegeneration_amd import ops
    M, C = 4099, 4
    gen = torch.Generator(device=dev).manual_seed(5)
    buf = torch.randn(4, M * C + 1, device=dev, generator=gen)
    x, x0, noise = (buf[i, 1:].view(M, C) for i in range(3))
    mask = torch.rand(M, 1, device=dev, generator=gen)
    sc = torch.tensor([0.25, 0.9682458], device=dev)
    want = torch_blend(x.clone(), x0, mask, noise, sc)
    uin = torch.full((M, 6), -3.0, dtype=torch.bfloat16, device=dev)
    ops.inpaint_blend(x, x0, mask, noise, sc, unet_in=uin)
    torch.cuda.synchronize()
    assert torch.equal(x, want) and torch.equal(uin[:, :C], want.bfloat16()) and bool((uin[:, C:] == -3.0).all())


# ------------------------------------------------------------------------------------------------ parity with the reference samplers
def test_ddim_inpainting_matches_reference_fixture(dev, small, g):
    from jointimagegeneration_amd.ldm import DDIMSampler
    c, uc, x_T, x0 = (T(g[k]).to(dev) for k in ("c", "uc", "x_T", "x0"))
    hole, soft = T(g["mask_hole"]).to(dev), T(g["mask_soft"]).to(dev)
    s = DDIMSampler(small)
    z, _ = s.sample(S=5, batch_size=2, shape=(4, 8, 8), conditioning=c, verbose=False, x_T=x_T, dims=2, mask=hole, x0=x0,
                    mask_noise_tape=tape(g, "q_tape", 5, dev))
    assert np.array_equal(s.ddim_timesteps, g["ddim5_timesteps"])
    e, r = rel_err(z, T(g["z_ddim_hole"])), rms_err(z, T(g["z_ddim_hole"]))
    print(f"DDIM 5 steps, centre hole: max {e:.3e} rms {r:.3e}")
    assert e < 2e-2 and r < 1.5e-2
    z, _ = s.sample(S=5, batch_size=2, shape=(4, 8, 8), conditioning=c, verbose=False, x_T=x_T, dims=2, eta=0.5, mask=soft, x0=x0,
                    noise_tape=tape(g, "step_tape", 5, dev), mask_noise_tape=tape(g, "q_tape", 5, dev))
    e, r = rel_err(z, T(g["z_ddim_soft_eta"])), rms_err(z, T(g["z_ddim_soft_eta"]))
    print(f"DDIM 5 steps, eta 0.5, soft per-channel mask: max {e:.3e} rms {r:.3e}")
    assert e < 2e-2 and r < 1.5e-2
    z, _ = s.sample(S=5, batch_size=2, shape=(4, 8, 8), conditioning=c, verbose=False, x_T=x_T, dims=2, mask=hole, x0=x0,
                    unconditional_guidance_scale=3.0, unconditional_conditioning=uc, mask_noise_tape=tape(g, "q_tape", 5, dev))
    e, r = rel_err(z, T(g["z_ddim_cfg"])), rms_err(z, T(g["z_ddim_cfg"]))
    print(f"DDIM 5 steps, guidance scale 3, centre hole: max {e:.3e} rms {r:.3e}")
    assert e < 6e-2 and r < 3e-2


def test_plms_inpainting_matches_reference_fixture(dev, small, g):
    from jointimagegeneration_amd.ldm import PLMSSampler
    c, x_T, x0, hole = (T(g[k]).to(dev) for k in ("c", "x_T", "x0", "mask_hole"))
    z, _ = PLMSSampler(small).sample(S=10, batch_size=2, shape=(4, 8, 8), conditioning=c, verbose=False, x_T=x_T, mask=hole, x0=x0,
                                     mask_noise_tape=tape(g, "q_tape", 10, dev))
    e, r = rel_err(z, T(g["z_plms_hole"])), rms_err(z, T(g["z_plms_hole"]))
    print(f"PLMS 10 steps, centre hole: max {e:.3e} rms {r:.3e}")
    assert e < 1.5e-2 and r < 1e-2


def test_ancestral_inpainting_matches_reference_fixture(dev, g):
    m20 = ldm_small(dev, 20)
    c, x_T, x0, hole = (T(g[k]).to(dev) for k in ("c", "x_T", "x0", "mask_hole"))
    q = tape(g, "q_tape", 20, dev)
    z = m20.p_sample_loop(c, (2, 4, 8, 8), x_T=x_T, verbose=False, mask=hole, x0=x0, noise_tape=tape(g, "step_tape", 20, dev), mask_noise_tape=q)
    e, r = rel_err(z, T(g["z_vanilla_hole"])), rms_err(z, T(g["z_vanilla_hole"]))
    known = (m20.sqrt_alphas_cumprod[0] * x0 + m20.sqrt_one_minus_alphas_cumprod[0] * q[19])
    err_known = float(((z - known) * hole).abs().max())
    print(f"ancestral 20 steps, centre hole: max {e:.3e} rms {r:.3e}; known region vs q_sample(x0, 0): {err_known:.2e}")
    assert e < 1.5e-2 and r < 1e-2
    assert err_known <= 1e-6
    # sample() / sample_log(ddim=False) are the same loop (ddpm.py:1231-1260)
    z2, inter = m20.sample_log(c, 2, False, None, x_T=x_T, mask=hole, x0=x0, noise_tape=tape(g, "step_tape", 20, dev), mask_noise_tape=q)
    assert torch.equal(z2, z) and len(inter) == 2


# ------------------------------------------------------------------------------------------------ engine invariants (bit for bit)
def _ddim(s, c, x_T, **kw):
    z, _ = s.sample(S=5, batch_size=2, shape=(4, 8, 8), conditioning=c, verbose=False, x_T=x_T, dims=2, **kw)
    return z


def test_captured_chain_equals_eager_and_reuses_its_graph_with_new_operands(dev, small, g):
    from jointimagegeneration_amd.ldm import DDIMSampler
    c, x_T, x0, hole = (T(g[k]).to(dev) for k in ("c", "x_T", "x0", "mask_hole"))
    gen = torch.Generator(device=dev).manual_seed(9)
    cases = [(x0, hole, tape(g, "q_tape", 5, dev))]
    for _ in range(2):
        cases.append((torch.randn(2, 4, 8, 8, device=dev, generator=gen), (torch.rand(2, 1, 8, 8, device=dev, generator=gen) > 0.4).float(),
                      [torch.randn(2, 4, 8, 8, device=dev, generator=gen) for _ in range(5)]))
    sg = DDIMSampler(small)
    for k, (x0_, m_, q_) in enumerate([cases[0]] + cases):          # call 1 eager (warm-up), 2 captures, 3 and 4 replay new operands
        got = _ddim(sg, c, x_T, mask=m_, x0=x0_, mask_noise_tape=q_)
        se = DDIMSampler(small)
        se.use_graph = False
        want = _ddim(se, c, x_T, mask=m_, x0=x0_, mask_noise_tape=q_)
        assert torch.equal(got, want), k
    st = [v for key, v in sg._graphs.items() if ("inpaint", 1) in key]
    assert len(st) == 1 and st[0]["graph"] is not None
    f = DDIMSampler(small)
    _ddim(f, c, x_T)
    assert sg.last_step_fused == f.last_step_fused                   # the blend leaves the head conv's fused DDIM epilogue as it was
    # a soft 4-channel mask gets its own state (the key holds the mask's channel extent) and its own graph
    soft = T(g["mask_soft"]).to(dev)
    for _ in range(3):
        got = _ddim(sg, c, x_T, mask=soft, x0=x0, mask_noise_tape=cases[1][2])
    se = DDIMSampler(small)
    se.use_graph = False
    assert torch.equal(got, _ddim(se, c, x_T, mask=soft, x0=x0, mask_noise_tape=cases[1][2]))
    assert sum(1 for key in sg._graphs if ("inpaint", 4) in key) == 1


def test_zero_mask_equals_no_mask_and_no_state_leaks(dev, small, g):
    from jointimagegeneration_amd.ldm import DDIMSampler, PLMSSampler
    c, x_T, x0 = (T(g[k]).to(dev) for k in ("c", "x_T", "x0"))
    zero = torch.zeros(2, 1, 8, 8, device=dev)
    fresh = DDIMSampler(small)
    ref = [_ddim(fresh, c, x_T) for _ in range(3)]                  # eager, capture, replay
    s = DDIMSampler(small)
    for k in range(3):
        assert torch.equal(_ddim(s, c, x_T, mask=zero, x0=x0), ref[k]), k                              # random q noise: multiplied by 0
        assert torch.equal(_ddim(s, c, x_T, mask=zero.bool(), x0=x0, eta=0.0), ref[k]), k
    for k in range(3):                                               # mask-free after masked calls: its own untouched state
        assert torch.equal(_ddim(s, c, x_T), ref[k]), k
    assert all("ip_x0" not in st for key, st in s._graphs.items() if not any(isinstance(e, tuple) and e[0] == "inpaint" for e in key))
    zp, _ = PLMSSampler(small).sample(S=10, batch_size=2, shape=(4, 8, 8), conditioning=c, verbose=False, x_T=x_T)
    zpm, _ = PLMSSampler(small).sample(S=10, batch_size=2, shape=(4, 8, 8), conditioning=c, verbose=False, x_T=x_T, mask=zero, x0=x0)
    assert torch.equal(zp, zpm)


def test_ancestral_all_ones_mask_returns_q_sample_of_x0(dev, g):
    m20 = ldm_small(dev, 20)
    c, x_T, x0 = (T(g[k]).to(dev) for k in ("c", "x_T", "x0"))
    q = tape(g, "q_tape", 20, dev)
    z = m20.p_sample_loop(c, (2, 4, 8, 8), x_T=x_T, verbose=False, mask=torch.ones(2, 4, 8, 8, device=dev), x0=x0, mask_noise_tape=q)
    assert torch.equal(z, m20.q_sample(x0, torch.zeros(2, dtype=torch.long, device=dev), q[19]))
    zf = m20.p_sample_loop(c, (2, 4, 8, 8), x_T=x_T, verbose=False, noise_tape=tape(g, "step_tape", 20, dev))
    zm = m20.p_sample_loop(c, (2, 4, 8, 8), x_T=x_T, verbose=False, noise_tape=tape(g, "step_tape", 20, dev),
                           mask=torch.zeros(2, 1, 8, 8, device=dev), x0=x0)
    assert torch.equal(zf, zm)


def test_encode_first_stage_matches_reference_fixture(dev, small, g):
    from jointimagegeneration_amd.ldm import DiagonalGaussianDistribution
    post = small.encode_first_stage(T(g["enc_img"]).to(dev))
    assert isinstance(post, DiagonalGaussianDistribution)
    em, rm = rel_err(post.mean, T(g["enc_mean"])), rms_err(post.mean, T(g["enc_mean"]))
    el, rl = rel_err(post.logvar, T(g["enc_logvar"])), rms_err(post.logvar, T(g["enc_logvar"]))
    print(f"encode_first_stage 32x32: mean max {em:.3e} rms {rm:.3e}; logvar max {el:.3e} rms {rl:.3e}")
    assert em < 4e-2 and rm < 2e-2 and el < 4e-2 and rl < 2e-2
    assert torch.equal(small.get_first_stage_encoding(post.mean), small.scale_factor * post.mean)


# ------------------------------------------------------------------------------------------------ full size
@pytest.fixture(scope="module")
def full(dev):
    from jointimagegeneration_amd.ldm import LatentDiffusion
    from jointimagegeneration_amd.synth import randomize_parameters
    m = LatentDiffusion(first_stage_config="__is_no_first_stage__", cond_stage_config=dict(target="ldm.modules.encoders.modules.IdentityEncoder"),
                        unet_config=dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(LDM_FULL)),
                        linear_start=0.0015, linear_end=0.0195, timesteps=1000, image_size=64, channels=4, dims=2, use_ema=False,
                        first_stage_key="image", cond_stage_key="mask", num_timesteps_cond=1).eval()
    randomize_parameters(m.model.diffusion_model, SEED, "ldm.")
    return m.to(dev)


@pytest.mark.parametrize("N", [1, 2])
def test_full_size_50_step_inpainting(dev, full, N):
    """LDM_FULL, 64x64 latent of a 512^2 slice, 50 DDIM steps.  Known region: the last step blends at t = 1 and then takes one DDIM step
    to a_prev = alphas_cumprod[0] with the model's eps e, so  x_out - x0 = (sqrt(a_prev) - 1) x0 + sqrt(a_prev / a_1) s1 (n - e)
    + sqrt(1 - a_prev) e  (s1 = sqrt(1 - a_1), n the last q noise), and |x_out - x0| is bounded by the same terms in absolute value.
    e is recovered from the returned latent and pred_x0 of that step."""
    from jointimagegeneration_amd.ldm import DDIMSampler
    gen = torch.Generator().manual_seed(600 + N)
    c = torch.randn(N, 4, 64, 64, generator=gen).to(dev)
    x_T = torch.randn(N, 4, 64, 64, generator=gen).to(dev)
    x_T2 = torch.randn(N, 4, 64, 64, generator=gen).to(dev)
    q = [torch.randn(N, 4, 64, 64, generator=gen).to(dev) for _ in range(50)]

    def run(s, **kw):
        return s.sample(S=50, batch_size=N, shape=(4, 64, 64), conditioning=c, verbose=False, dims=2, **kw)
    s = DDIMSampler(full)
    x0, _ = run(s, x_T=x_T)                                          # a previously sampled latent
    hole = torch.ones(N, 1, 64, 64, device=dev)
    hole[:, :, 16:48, 16:48] = 0.0
    runs = [run(s, x_T=x_T2, mask=hole, x0=x0, mask_noise_tape=q) for _ in range(3)]      # eager, capture, replay
    se = DDIMSampler(full)
    se.use_graph = False
    z_e, inter_e = run(se, x_T=x_T2, mask=hole, x0=x0, mask_noise_tape=q)
    for z, _ in runs:
        assert torch.equal(z, z_e)
    free = [run(s, x_T=x_T2)[0] for _ in range(2)]
    zero = [run(s, x_T=x_T2, mask=torch.zeros_like(hole), x0=x0)[0] for _ in range(3)]
    for z in zero + free[1:]:
        assert torch.equal(z, free[0])
    # known region within the stated bound of x0
    ac = full.alphas_cumprod
    a1, a_prev = ac[1], ac[0]
    p0 = inter_e["pred_x0"][1]
    e = (z_e - a_prev.sqrt() * p0) / (1.0 - a_prev).sqrt()
    s1 = (1.0 - a1).sqrt()
    bound = (1.0 - a_prev.sqrt()) * x0.abs() + (a_prev / a1).sqrt() * s1 * (q[-1].abs() + e.abs()) + (1.0 - a_prev).sqrt() * e.abs()
    bound = bound + 1e-4 * (1.0 + x0.abs() + q[-1].abs() + e.abs())                        # fp32 rounding of the few operations
    err = (z_e - x0).abs()
    keep = hole.expand_as(err) > 0
    ratio = float((err[keep] / bound[keep]).max())
    rms_keep = float(err[keep].pow(2).mean().sqrt())
    rms_hole = float(err[~keep].pow(2).mean().sqrt())
    print(f"full size N={N}: known region |x_out - x0| rms {rms_keep:.3e} (worst err / bound {ratio:.3f}); hole rms {rms_hole:.3e}")
    assert ratio <= 1.0
    assert rms_keep < rms_hole
