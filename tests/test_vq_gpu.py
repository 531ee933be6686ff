"""GPU suite for the VQ first stage and quantised sampling (gg_vq.hip): gg_vq_nearest bit for bit against the fp64 restatement on inputs
whose fp32 arithmetic is exact, and on random inputs outside near-ties; gg_ddim_step_vq and gg_ddim_step against the same step as separate fp32 torch ops;
the quantised DDIM chain teacher-forced, captured and eager; VQModelInterface against the reference fixture (tests/golden/vq.npz,
make_golden_vq.py); temperature and noise_dropout.

Near-tie rule (random inputs): a row may be left out of a comparison only if the fp64 gap between its two smallest distances is below
1e-4 * (1 + d_min); at most 2 % of the rows of a case may be left out."""
import numpy as np
import pytest
import torch

import vq_ref
from util import AE_SMALL, LDM_SMALL, SEED, T, gold, rel_err, rms_err, seeded

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
LOSS = dict(target="torch.nn.Identity")
CAP = 0.02


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def vq_first_stage(n_embed=64):
    return dict(target="ldm.models.autoencoder.VQModelInterface",
                params=dict(embed_dim=4, n_embed=n_embed, dims=2, ddconfig=dict(AE_SMALL), lossconfig=LOSS))


@pytest.fixture(scope="module")
def vqldm(dev):
    """The small latent config of the inpainting tests (UNet LDM_SMALL, 8x8 latent of 4 channels, AE_SMALL cond stage, "ldm_pipe."
    weights) with a VQModelInterface first stage of 256 codes; the codebook is N(0, 1/4) from the seed recipe."""
    from jointimagegeneration_amd.ldm import LatentDiffusion
    ae2 = dict(target="ldm.models.autoencoder.AutoencoderKL", params=dict(embed_dim=4, dims=2, ddconfig=dict(AE_SMALL, in_channels=2, out_ch=2), lossconfig=LOSS))
    m = LatentDiffusion(first_stage_config=vq_first_stage(256), cond_stage_config=ae2,
                        unet_config=dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(LDM_SMALL)),
                        linear_start=0.0015, linear_end=0.0195, timesteps=1000, image_size=8, channels=4, dims=2, first_stage_key="image",
                        cond_stage_key="mask", num_timesteps_cond=1)
    return seeded(m, "ldm_pipe.").to(dev)


@pytest.fixture(scope="module")
def operands(dev):
    gen = torch.Generator().manual_seed(2048)
    return dict(c=torch.randn(2, 4, 8, 8, generator=gen).to(dev), uc=torch.randn(2, 4, 8, 8, generator=gen).to(dev),
                x_T=torch.randn(2, 4, 8, 8, generator=gen).to(dev), x0=torch.randn(2, 4, 8, 8, generator=gen).to(dev),
                tape=[torch.randn(2, 4, 8, 8, generator=gen).to(dev) for _ in range(20)],
                qtape=[torch.randn(2, 4, 8, 8, generator=gen).to(dev) for _ in range(20)])


def ddim(s, ops_, **kw):
    kw.setdefault("x_T", ops_["x_T"])
    return s.sample(S=5, batch_size=2, shape=(4, 8, 8), conditioning=ops_["c"], verbose=False, dims=2, **kw)


# ------------------------------------------------------------------------------------------------ 1. exact arithmetic, zero exclusions
def exact_case(C, n_embed, M, stride, dev, seed):
    """Multiples of 1/8 in [-2, 2]: every fp32 product and sum of the distance is exact.  Duplicate codes are planted, and rows equal to
    duplicated codes, so that exact ties occur at distance 0 and elsewhere."""
    gen = torch.Generator().manual_seed(seed)
    E = torch.randint(-16, 17, (n_embed, C), generator=gen).float() / 8.0
    if n_embed > 1:
        src = torch.randint(0, n_embed, (max(1, n_embed // 8),), generator=gen)
        dst = torch.randint(0, n_embed, (max(1, n_embed // 8),), generator=gen)
        E[dst] = E[src].clone()
    rows = torch.full((M, stride), 99.0)                      # the pad lanes hold a sentinel that must not be read
    rows[:, :C] = torch.randint(-16, 17, (M, C), generator=gen).float() / 8.0
    pick = torch.randint(0, n_embed, (M,), generator=gen)
    rows[::3, :C] = E[pick[::3]]
    return rows.to(dev), E.to(dev)


@pytest.mark.parametrize("M", [1, 63, 4101])
@pytest.mark.parametrize("n_embed", [1, 37, 1000, 8192])
@pytest.mark.parametrize("C", [1, 3, 4, 8])
def test_nearest_exact_arithmetic_bit_for_bit(dev, C, n_embed, M):
    from jointimagegeneration_amd import ops
    rows, E = exact_case(C, n_embed, M, C, dev, 1000 * C + n_embed + M)
    want, _ = vq_ref.quantise(rows, E)
    idx, st = ops.vq_nearest(rows, E)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (M,) and tuple(st.shape) == (M, C)
    assert torch.equal(idx.long(), want)
    assert torch.equal(st, vq_ref.straight_through(rows.double(), E.double(), want).float())
    if n_embed >= 37 and M >= 63:                              # the planted ties were exercised: some chosen code has a duplicate
        dup = (E[None, :, :] == E[want[:63], None, :]).all(2)
        assert bool((dup.sum(1) > 1).any())


@pytest.mark.parametrize("C,stride", [(3, 4), (4, 32), (1, 2), (8, 11)])
def test_nearest_padded_rows_and_in_place(dev, C, stride):
    from jointimagegeneration_amd import ops
    M, n_embed = 1030, 1500
    rows, E = exact_case(C, n_embed, M, stride, dev, 77 + stride)
    want, _ = vq_ref.quantise(rows[:, :C].contiguous(), E)
    idx, st = ops.vq_nearest(rows, E, C)
    assert torch.equal(idx.long(), want) and torch.equal(st, E[want])
    idx2, _ = ops.vq_nearest(rows, E, C, want_st=False)                    # indices alone
    assert torch.equal(idx2, idx)
    ops.vq_nearest(rows, E, C, st_out=rows)                                # in place, into the padded rows
    assert torch.equal(rows[:, :C], E[want]) and bool((rows[:, C:] == 99.0).all())


# ------------------------------------------------------------------------------------------------ 2. random inputs
# (C, n_embed, M, seed): share of rows inside the near-tie margin, measured on the CPU with the fp64 restatement alone before committing:
#   (4, 1000, 4101, 11): 0.12 %     (3, 8192, 2050, 12): 1.41 %     (8, 37, 4101, 13): 0.00 %     (1, 16, 1030, 14): 0.68 %
# (C = 1 with 1000 N(0, 1) codes puts 93 % of the rows inside the margin -- a dense line of codes -- so that case has 16 codes.)
# The step cases of test 3: (4, 1000, 4101): 0.05 %, (3, 300, 1030): 0.00 %, ancestral (4, 300, 1030): 0.10 %.
RANDOM_CASES = [(4, 1000, 4101, 11), (3, 8192, 2050, 12), (8, 37, 4101, 13), (1, 16, 1030, 14)]


def random_case(C, n_embed, M, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(M, C, generator=gen), torch.randn(n_embed, C, generator=gen)      # N(0, 1) codebook, not uniform(+-1/n_embed)


@pytest.mark.parametrize("C,n_embed,M,seed", RANDOM_CASES)
def test_nearest_random_inputs(dev, C, n_embed, M, seed):
    from jointimagegeneration_amd import ops
    rows, E = random_case(C, n_embed, M, seed)
    rows, E = rows.to(dev), E.to(dev)
    want, amb = vq_ref.quantise(rows, E)
    share = float(amb.float().mean())
    idx, st = ops.vq_nearest(rows, E)
    keep = ~amb
    wrong = int((idx.long() != want)[keep].sum())
    print(f"C={C} n_embed={n_embed} M={M}: {100 * share:.2f} % of the rows inside the near-tie margin; {wrong} compared rows differ; "
          f"{int((idx.long() != want).sum())} rows differ in all")
    assert share <= CAP
    assert wrong == 0
    assert torch.equal(st[keep], vq_ref.straight_through(rows, E, want)[keep])
    assert torch.equal(st, vq_ref.straight_through(rows, E, idx.long()))              # every row is the straight-through of ITS index


# ------------------------------------------------------------------------------------------------ 3. the step
@pytest.mark.parametrize("temperature", [1.0, 0.7])
@pytest.mark.parametrize("eta", [0.0, 0.6])
@pytest.mark.parametrize("C,n_embed,M", [(4, 1000, 4101), (3, 300, 1030)])
def test_ddim_step_vq_equals_the_separate_torch_ops(dev, C, n_embed, M, eta, temperature):
    from jointimagegeneration_amd import ops
    gen = torch.Generator().manual_seed(31 * M + C)
    x, e, nz = (torch.randn(M, C, generator=gen).to(dev) for _ in range(3))
    E = torch.randn(n_embed, C, generator=gen).to(dev)
    eps = torch.full((M, 32), 55.0, device=dev)
    eps[:, :C] = e
    a_t, a_prev = 0.6132, 0.6811
    sigma = eta * float(np.sqrt((1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)))
    sc = torch.tensor([a_t, a_prev, sigma, float(np.sqrt(1 - a_t))], dtype=torch.float32)
    sc = torch.cat([sc, sc[2:3] * torch.tensor(temperature, dtype=torch.float32)]).to(dev)
    noise = nz if eta > 0 else None
    want_x, want_q, want_idx, amb, _ = vq_ref.ddim_step_vq(x, e, sc, E, noise)
    xs, p0 = x.clone(), torch.empty_like(x)
    uin = torch.full((M, 32), 7.0, dtype=torch.bfloat16, device=dev)
    idx = torch.empty(M, dtype=torch.int32, device=dev)
    ops.ddim_step_vq(xs, eps, sc, E, noise=noise, pred_x0_out=p0, unet_in=uin, idx_out=idx)
    torch.cuda.synchronize()
    keep = ~amb
    share = float(amb.float().mean())
    ulp = lambda a, b: int((a.view(torch.int32).long() - b.view(torch.int32).long()).abs().max()) if a.numel() else 0
    print(f"C={C} eta={eta} T={temperature}: near-tie share {100 * share:.2f} %; index mismatches on compared rows "
          f"{int((idx.long() != want_idx)[keep].sum())}; max ulp pred_x0 {ulp(p0[keep], want_q[keep])}, x {ulp(xs[keep], want_x[keep])}")
    assert share <= CAP
    assert torch.equal(idx.long()[keep], want_idx[keep])
    assert torch.equal(p0[keep], want_q[keep])
    assert torch.equal(xs[keep], want_x[keep])
    assert torch.equal(uin[:, :C][keep], want_x.bfloat16()[keep])
    assert bool((uin[:, C:] == 7.0).all())
    # without a codebook the entry is the plain step with its own noise coefficient
    xs2, p2 = x.clone(), torch.empty_like(x)
    ops.ddim_step_vq(xs2, eps, sc, None, noise=noise, pred_x0_out=p2)
    w_x, w_p, _, _, _ = vq_ref.ddim_step_vq(x, e, sc, None, noise)
    assert torch.equal(xs2, w_x) and torch.equal(p2, w_p)
    if temperature == 1.0:                                      # and then it is gg_ddim_step
        xs3, p3 = x.clone(), torch.empty_like(x)
        ops.ddim_step(xs3, eps, sc[:4].contiguous(), noise=noise, pred_x0_out=p3)
        assert torch.equal(xs3, xs2) and torch.equal(p3, p2)


def test_ancestral_step_vq_equals_the_separate_torch_ops(dev):
    from jointimagegeneration_amd import ops
    M, C, n_embed = 1030, 4, 300
    gen = torch.Generator().manual_seed(5)
    x, e, nz = (torch.randn(M, C, generator=gen).to(dev) for _ in range(3))
    E = torch.randn(n_embed, C, generator=gen).to(dev)
    sc = torch.tensor([1.2771, 0.7943, 0.0312, 0.9654, 0.0871], dtype=torch.float32, device=dev)
    want_x, want_q, want_idx, amb, _ = vq_ref.ddim_step_vq(x, e, sc, E, nz, ancestral=True)
    xs, p0, idx = x.clone(), torch.empty_like(x), torch.empty(M, dtype=torch.int32, device=dev)
    ops.ddim_step_vq(xs, e.contiguous(), sc, E, noise=nz, pred_x0_out=p0, idx_out=idx, ancestral=True)
    keep = ~amb
    assert float(amb.float().mean()) <= CAP
    assert torch.equal(idx.long()[keep], want_idx[keep]) and torch.equal(p0[keep], want_q[keep]) and torch.equal(xs[keep], want_x[keep])
    xs2 = x.clone()
    ops.ddim_step_vq(xs2, e.contiguous(), sc, None, noise=nz, ancestral=True)             # no codebook: gg_ddpm_step
    xs3 = x.clone()
    ops.ddpm_step(xs3, e.contiguous(), sc, noise=nz)
    assert torch.equal(xs2, xs3)


def ddim_scalars(eta, dev):
    """The scalar row of test_ddim_step_vq_equals_the_separate_torch_ops (vq_ref is written around these roots), fp32[4]."""
    a_t, a_prev = 0.6132, 0.6811
    sigma = eta * float(np.sqrt((1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)))
    return torch.tensor([a_t, a_prev, sigma, float(np.sqrt(1 - a_t))], dtype=torch.float32).to(dev)


def ddim_want(x, e, sc, noise):
    """gg_ddim_step's result as separate torch ops: the step of vq_ref without a codebook, its noise coefficient sigma_t."""
    want_x, want_p, _, _, _ = vq_ref.ddim_step_vq(x, e, torch.cat([sc, sc[2:3]]), None, noise)
    return want_x, want_p


@pytest.mark.parametrize("eta", [0.0, 0.6])
@pytest.mark.parametrize("C", [4, 3], ids=["C4", "C3"])
@pytest.mark.parametrize("M", [1000, 4099])
def test_ddim_step_is_bit_equal_to_the_torch_expression(dev, M, C, eta):
    from jointimagegeneration_amd import ops
    gen = torch.Generator().manual_seed(17 * M + C)
    x0_, e, nz = (torch.randn(M, C, generator=gen).to(dev) for _ in range(3))
    eps = torch.full((M, 32), 55.0, device=dev)
    eps[:, :C] = e
    sc = ddim_scalars(eta, dev)
    for with_noise in (True, False):
        want_x, want_p = ddim_want(x0_, e, sc, nz if with_noise else None)
        for with_p0 in (True, False):
            for with_uin in (True, False):
                x = x0_.clone()
                p0 = torch.full((M, C), 9.0, device=dev) if with_p0 else None
                uin = torch.full((M, 32), 7.0, dtype=torch.bfloat16, device=dev) if with_uin else None      # pad lanes: a sentinel that must survive
                ops.ddim_step(x, eps, sc, noise=nz if with_noise else None, pred_x0_out=p0, unet_in=uin)
                torch.cuda.synchronize()
                tag = (with_noise, with_p0, with_uin)
                assert torch.equal(x, want_x), tag
                if with_p0:
                    assert torch.equal(p0, want_p), tag
                if with_uin:
                    assert torch.equal(uin[:, :C], want_x.bfloat16()) and bool((uin[:, C:] == 7.0).all()), tag


def test_ddim_step_misaligned_rows_give_the_same_bits(dev):
    """gg_ddim_step has no path that depends on alignment, and this pins it: the two misaligned views of the gg_ddpm_step_x0 suite
    (tests/test_progressive_gpu.py), x one row into a C = 3 buffer (12 bytes off any 16-byte boundary) and C = 4 rows one float in with a
    unet_in stride that is no multiple of 4, give the bits of the torch expression and touch nothing in front of the views."""
    from jointimagegeneration_amd import ops
    sc = ddim_scalars(0.6, dev)
    gen = torch.Generator(device=dev).manual_seed(78)
    M = 4099
    buf = torch.randn(M + 1, 3, device=dev, generator=gen)
    x, row0 = buf[1:], buf[0].clone()
    assert x.data_ptr() % 16 != 0 and x.is_contiguous()
    eps, noise = torch.randn(M, 5, device=dev, generator=gen), torch.randn(M, 3, device=dev, generator=gen)
    want_x, want_p = ddim_want(x.clone(), eps[:, :3].contiguous(), sc, noise)
    p0, uin = torch.empty(M, 3, device=dev), torch.full((M, 6), -3.0, dtype=torch.bfloat16, device=dev)
    ops.ddim_step(x, eps, sc, noise=noise, pred_x0_out=p0, unet_in=uin)
    torch.cuda.synchronize()
    assert torch.equal(x, want_x) and torch.equal(p0, want_p) and torch.equal(uin[:, :3], want_x.bfloat16()) and bool((uin[:, 3:] == -3.0).all())
    assert torch.equal(buf[0], row0)                         # the row in front of the view is not touched
    flat = torch.randn(3, M * 4 + 1, device=dev, generator=gen)
    col0 = flat[:, 0].clone()
    x, noise, p0 = (flat[i, 1:].view(M, 4) for i in range(3))
    eps = torch.randn(M, 4, device=dev, generator=gen)
    want_x, want_p = ddim_want(x.clone(), eps, sc, noise.clone())
    uin = torch.full((M, 6), -3.0, dtype=torch.bfloat16, device=dev)
    ops.ddim_step(x, eps, sc, noise=noise, pred_x0_out=p0, unet_in=uin)
    torch.cuda.synchronize()
    assert torch.equal(x, want_x) and torch.equal(p0, want_p) and torch.equal(uin[:, :4], want_x.bfloat16()) and bool((uin[:, 4:] == -3.0).all())
    assert torch.equal(flat[:, 0], col0)


# ------------------------------------------------------------------------------------------------ 4. chains
def test_quantised_chain_teacher_forced_in_fp32_validation(dev, vqldm, operands):
    """5 DDIM steps with quantize_x0 on the sampler's own state.  Each step's eps comes from the engine's UNet in ops.fp32_validation()
    (evaluated on the engine's current x), and the SAME eps goes to the torch restatement of the step; outputs compared as in test 3.
    The final pred_x0 holds codebook rows up to the straight-through rounding: |q - e| <= 2^-23 (|e - p| + |e|) per element (the
    rounding of t = e - p is at most 2^-24 |t|, that of p + t at most 2^-24 |p + t|, and |p + t| <= |e| (1 + 2^-23))."""
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.ldm import DDIMSampler, first_stage_codebook
    unet = vqldm.model.diffusion_model
    s = DDIMSampler(vqldm)
    s.make_schedule(5, ddim_eta=0.0, verbose=False)
    E = first_stage_codebook(vqldm, "test", 4)
    st = s.prepare_state(2, 4, (8, 8), dev, 4, vq=(E, 1.0))
    assert tuple(st["scal"].shape) == (5, 5) and st["vq"] is E
    assert torch.equal(st["scal"][:, 4], st["scal"][:, 2])                     # temperature 1: the noise coefficient is sigma_t
    s.load_state(st, operands["x_T"], operands["c"])
    ts = np.flip(s.ddim_timesteps).copy()
    cl = lambda t: t.permute(0, 2, 3, 1).reshape(-1, 4)
    for i in range(5):
        x_nchw = st["x"].view(2, 8, 8, 4).permute(0, 3, 1, 2).contiguous()
        with ops.fp32_validation():
            eps = unet(torch.cat([x_nchw, operands["c"]], 1), torch.full((2,), int(ts[i]), device=dev))
        st["eps"].view(-1, st["eps"].shape[-1])[:, :4] = cl(eps)
        x_before = st["x"].view(-1, 4).clone()
        s._update(st, st["eps"], st["scal"][i])
        want_x, want_q, want_idx, amb, p = vq_ref.ddim_step_vq(x_before, cl(eps).contiguous(), st["scal"][i], E)
        keep = ~amb
        assert float(amb.float().mean()) <= CAP, i
        assert torch.equal(st["pred_x0"].view(-1, 4)[keep], want_q[keep]), i
        assert torch.equal(st["x"].view(-1, 4)[keep], want_x[keep]), i
        assert torch.equal(st["unet_in"].view(-1, st["unet_in"].shape[-1])[:, :4][keep], want_x.bfloat16()[keep]), i
    q = st["pred_x0"].view(-1, 4)
    idx, _ = ops.vq_nearest(q.contiguous(), E, want_st=False)
    e = E[idx.long()]
    pk = p.clone()
    pk[~keep] = q[~keep]                                                        # a near-tie row is compared against its own code
    bound = 2.0 ** -23 * ((e - pk).abs() + e.abs())
    assert bool(((q - e).abs() <= bound)[keep].all())
    assert bool(((q - e).abs() <= 2.0 ** -22 * (1.0 + e.abs())).all())


def test_quantised_bf16_chain_is_one_graph_and_equals_eager(dev, vqldm, operands):
    from jointimagegeneration_amd.ldm import DDIMSampler
    sg = DDIMSampler(vqldm)
    runs = [ddim(sg, operands, quantize_x0=True) for _ in range(3)]             # eager warm-up, capture, replay
    se = DDIMSampler(vqldm)
    se.use_graph = False
    z_e, inter_e = ddim(se, operands, quantize_x0=True)
    for z, inter in runs:
        assert torch.equal(z, z_e) and torch.equal(inter["pred_x0"][1], inter_e["pred_x0"][1])
    states = [v for k, v in sg._graphs.items() if k[-1] == ("vq", True)]
    assert len(states) == 1 and states[0]["graph"] is not None and not sg.last_step_fused
    z_plain, _ = ddim(DDIMSampler(vqldm), operands)
    assert float((z_plain - z_e).abs().max()) > 1e-3                            # the quantiser changed the chain


def test_quantisation_with_guidance_mask_eta_plms_and_ancestral(dev, vqldm, operands):
    """quantize_x0 / quantize_denoised in every sampler variant: the returned pred_x0 holds codebook rows, and the ancestral loop with
    quantize_denoised is the plain loop with the quantised x_recon (one step, checked against the restatement)."""
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.ldm import DDIMSampler, PLMSSampler, first_stage_codebook
    E = first_stage_codebook(vqldm, "test", 4)
    hole = torch.ones(2, 1, 8, 8, device=dev)
    hole[:, :, 2:6, 2:6] = 0.0

    def codebook_valued(p0):
        q = p0.permute(0, 2, 3, 1).reshape(-1, 4).contiguous()
        idx, _ = ops.vq_nearest(q, E, want_st=False)
        return bool(((q - E[idx.long()]).abs() <= 2.0 ** -22 * (1.0 + E[idx.long()].abs())).all())
    cases = [dict(unconditional_guidance_scale=3.0, unconditional_conditioning=operands["uc"]),
             dict(mask=hole, x0=operands["x0"], mask_noise_tape=operands["qtape"][:5]),
             dict(eta=0.5, noise_tape=operands["tape"][:5]),
             dict(eta=0.5, noise_tape=operands["tape"][:5], temperature=0.7, noise_dropout=0.25, mask=hole, x0=operands["x0"],
                  mask_noise_tape=operands["qtape"][:5])]
    for kw in cases:
        z, inter = ddim(DDIMSampler(vqldm), operands, quantize_x0=True, **kw)
        assert bool(torch.isfinite(z).all()) and codebook_valued(inter["pred_x0"][1]), sorted(kw)
    z, inter = PLMSSampler(vqldm).sample(S=6, batch_size=2, shape=(4, 8, 8), conditioning=operands["c"], verbose=False, x_T=operands["x_T"],
                                         quantize_x0=True)
    assert bool(torch.isfinite(z).all()) and codebook_valued(inter["pred_x0"][1])
    zp, _ = PLMSSampler(vqldm).sample(S=6, batch_size=2, shape=(4, 8, 8), conditioning=operands["c"], verbose=False, x_T=operands["x_T"])
    assert float((zp - z).abs().max()) > 1e-3
    kw = dict(x_T=operands["x_T"], verbose=False, timesteps=4, noise_tape=operands["tape"][:4])
    zq = vqldm.p_sample_loop(operands["c"], (2, 4, 8, 8), quantize_denoised=True, **kw)
    zf = vqldm.p_sample_loop(operands["c"], (2, 4, 8, 8), **kw)
    assert bool(torch.isfinite(zq).all()) and float((zq - zf).abs().max()) > 1e-3
    z2, _ = vqldm.sample_log(operands["c"], 2, False, None, quantize_denoised=True, shape=(2, 4, 8, 8), **kw)
    assert torch.equal(z2, zq)


# ------------------------------------------------------------------------------------------------ 5. the first stage
def test_vqmodelinterface_against_the_reference_fixture(dev):
    """Tolerances: those of the AutoencoderKL module tests (tests/test_hip_parity.py, AE decode / encode vs the reference fixture):
    max < 4e-2, rms < 2e-2 (bf16 networks)."""
    from jointimagegeneration_amd.config import instantiate_from_config
    g = gold("vq")
    m = seeded(instantiate_from_config(vq_first_stage(64)), "vq_small.").to(dev)
    h, img = T(g["h"]).to(dev), T(g["img"]).to(dev)
    quant, loss, (perp, enc1h, ind) = m.quantize(h)
    assert loss is None and perp is None and enc1h is None
    assert ind.dtype == torch.int64 and tuple(ind.shape) == (64, 1) and torch.equal(ind.view(-1).cpu(), T(g["idx"]).long())
    assert torch.equal(quant.cpu(), T(g["quant"]))
    dec = m.decode(h)
    assert torch.equal(dec, m.decode(quant, force_not_quantize=True))
    dec_nq = m.decode(h, force_not_quantize=True)
    enc = m.encode(img)
    for name, got, want in (("decode", dec, g["dec"]), ("decode, force_not_quantize", dec_nq, g["dec_nq"]), ("encode (pre-quantisation)", enc, g["enc"])):
        e, r = rel_err(got, T(want)), rms_err(got, T(want))
        print(f"VQModelInterface {name}: max {e:.3e} rms {r:.3e}")
        assert e < 4e-2 and r < 2e-2, name
    assert isinstance(enc, torch.Tensor) and tuple(enc.shape) == (1, 4, 8, 8)
    assert torch.equal(m.encode_to_prequant(img), enc)
    # VQModel.encode quantises what the interface's encode returns; decode_code decodes codebook rows
    from jointimagegeneration_amd.ldm import VQModel
    q2, _, (_, _, i2) = VQModel.encode(m, img)
    qi, _, (_, _, ii) = m.quantize(enc)
    assert torch.equal(q2, qi) and torch.equal(i2, ii)
    assert torch.equal(m.decode_code(i2.view(1, 8, 8)), m.decode(m.quantize.embed_code(i2.view(1, 8, 8)), force_not_quantize=True))


def test_decode_first_stage_passes_force_not_quantize(dev, vqldm):
    gen = torch.Generator().manual_seed(3)
    z = 0.5 * torch.randn(1, 4, 8, 8, generator=gen).to(dev)
    fs = vqldm.first_stage_model
    assert torch.equal(vqldm.decode_first_stage(z), fs.decode(z))
    assert torch.equal(vqldm.decode_first_stage(z, force_not_quantize=True), fs.decode(z, force_not_quantize=True))
    assert not torch.equal(fs.decode(z), fs.decode(z, force_not_quantize=True))
    img = torch.rand(1, 1, 32, 32, generator=gen).to(dev)
    enc = vqldm.encode_first_stage(img)
    assert isinstance(enc, torch.Tensor) and torch.equal(vqldm.get_first_stage_encoding(enc), vqldm.scale_factor * enc)


# ------------------------------------------------------------------------------------------------ 6. temperature, noise_dropout, defaults
def test_temperature_equals_a_premultiplied_tape(dev, vqldm, operands):
    """temperature sits in the scalar table: x += (sigma * t) * noise.  With t = 0.5, a power of two, (sigma * t) * n and
    sigma * (t * n) are the same fp32 number, so the run equals the run on the pre-multiplied tape bit for bit."""
    from jointimagegeneration_amd.ldm import DDIMSampler
    tape = operands["tape"][:5]
    for extra in (dict(), dict(quantize_x0=True)):
        z_t, _ = ddim(DDIMSampler(vqldm), operands, eta=0.8, noise_tape=tape, temperature=0.5, **extra)
        z_m, _ = ddim(DDIMSampler(vqldm), operands, eta=0.8, noise_tape=[0.5 * n for n in tape], **extra)
        z_1, _ = ddim(DDIMSampler(vqldm), operands, eta=0.8, noise_tape=tape, **extra)
        assert torch.equal(z_t, z_m) and not torch.equal(z_t, z_1), sorted(extra)
    s = DDIMSampler(vqldm)
    ddim(s, operands, eta=0.8, noise_tape=tape, temperature=0.3)
    z_07, _ = ddim(s, operands, eta=0.8, noise_tape=tape, temperature=0.7)             # temperatures share one state; column 5 is rewritten
    assert torch.equal(z_07, ddim(DDIMSampler(vqldm), operands, eta=0.8, noise_tape=tape, temperature=0.7)[0])
    hot = [v for k, v in s._graphs.items() if k[-1] == ("vq", False)]
    assert len(hot) == 1 and hot[0]["vq"] is None and tuple(hot[0]["scal"].shape) == (5, 5)
    plain = s.step_scalar_table().to(dev)
    assert torch.equal(hot[0]["scal"][:, :4], plain) and float(plain[:, 2].min()) > 0.0        # dir_xt keeps sigma_t unscaled
    assert torch.equal(hot[0]["scal"][:, 4], plain[:, 2] * torch.tensor(0.7, dtype=torch.float32, device=dev))
    z_det, _ = ddim(s, operands, temperature=0.7)                                       # eta = 0: no effect, the plain state
    assert torch.equal(z_det, ddim(DDIMSampler(vqldm), operands)[0])
    assert sum(1 for k in s._graphs if isinstance(k[-1], tuple) and k[-1] and k[-1][0] == "vq") == 1


def test_noise_dropout_equals_the_same_dropout_on_the_tape(dev, vqldm, operands):
    from jointimagegeneration_amd.ldm import DDIMSampler
    tape = operands["tape"][:5]
    torch.cuda.manual_seed(1234)
    z_d, _ = ddim(DDIMSampler(vqldm), operands, eta=0.8, noise_tape=tape, noise_dropout=0.3)
    torch.cuda.manual_seed(1234)
    dropped = [torch.nn.functional.dropout(n, p=0.3) for n in tape]
    assert all(bool((d == 0).any()) for d in dropped)
    z_m, _ = ddim(DDIMSampler(vqldm), operands, eta=0.8, noise_tape=dropped)
    z_1, _ = ddim(DDIMSampler(vqldm), operands, eta=0.8, noise_tape=tape)
    assert torch.equal(z_d, z_m) and not torch.equal(z_d, z_1)


def test_default_call_keeps_its_state_graph_and_launches(dev, vqldm, operands, monkeypatch):
    """A call with all defaults after calls that used the new options: the same `_graphs` key as before them (the key a sampler without
    the options builds), the same state object and captured graph, and the same launches."""
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.ldm import DDIMSampler
    s = DDIMSampler(vqldm)
    ref = [ddim(s, operands)[0] for _ in range(3)]                              # eager, capture, replay
    keys_before = list(s._graphs)
    assert keys_before == [(2, 4, (1, 8, 8), 4, str(dev), None)]
    st = s._graphs[keys_before[0]]
    graph = st["graph"]
    assert graph is not None and "vq" not in st and tuple(st["scal"].shape) == (5, 4)
    ddim(s, operands, quantize_x0=True)
    ddim(s, operands, eta=0.5, noise_tape=operands["tape"][:5], temperature=0.7, noise_dropout=0.2)
    assert torch.equal(ddim(s, operands)[0], ref[2])
    assert s._graphs[keys_before[0]] is st and st["graph"] is graph
    assert [k for k in s._graphs if k[-1] != ("vq", True)][0] == keys_before[0]
    # launches of an eager default chain: counted through the ops entry points, before and after the options were used
    def count(sampler):
        n = {"ddim_step": 0, "ddim_step_vq": 0, "vq_nearest": 0, "inpaint_blend": 0, "lincomb4": 0, "capture_graph": 0}
        with monkeypatch.context() as mp:
            for name in n:
                real = getattr(ops, name)
                mp.setattr(ops, name, (lambda real, name: lambda *a, **k: (n.__setitem__(name, n[name] + 1), real(*a, **k))[1])(real, name))
            ddim(sampler, operands)
        return n
    fresh = DDIMSampler(vqldm)
    fresh.use_graph = False
    a = count(fresh)
    ddim(fresh, operands, quantize_x0=True)
    b = count(fresh)
    assert a == b and a["ddim_step_vq"] == 0 and a["vq_nearest"] == 0
    with monkeypatch.context() as mp:
        calls = []
        real = ops.ddim_step_vq
        mp.setattr(ops, "ddim_step_vq", lambda *a_, **k: (calls.append(1), real(*a_, **k))[1])
        ddim(fresh, operands, quantize_x0=True)
    assert len(calls) == 5
