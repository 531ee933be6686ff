"""GPU suite for the volumetric (dims = 3) first stage and 3-D latent sampling, against what the REFERENCE computed on the CPU
(tests/golden/ae3d.npz, make_golden_ae3d.py): AutoencoderKL and VQModel in fp32 validation mode and on the bf16 path, the two conv
geometries only a 3-D autoencoder reaches (stride 2 with a trailing pad on D, H and W; x2 upsample of D, H and W) bit for bit against
fp64, the attention launch of AttnBlock3d bit for bit, 3-step DDIM chains on [2, 4, 4, 6, 6] latents, and the shape round trip.

Tolerances (none is new):
  fp32 validation   max abs / max |ref| < 2e-5: FP32_REL of tests/test_unet_options_gpu.py (fp32 validation blocks and networks against
                    reference fixtures).  The reference's own fp32-vs-fp64 spread on this fixture is at most 2.0e-6
                    (ae3d_surface.json), so the bound is ten times the reference's rounding, not a looser one than the project has.
  bf16 first stage  max < 4e-2, rms < 2e-2: the AE decode / encode bound of tests/test_hip_parity.py and tests/test_vq_gpu.py.
  VQ indices (bf16) may differ from the reference only on rows whose two smallest fp64 distances differ by less than
                    4e-2 * (1 + d_min) (tests/vq_ref.py's near-tie form with the bf16 tolerance); at most 2 % of the rows.
  chains            max 2e-2 / rms 1.5e-2, guided max 6e-2 / rms 3e-2: tests/test_inpaint_gpu.py's 2-D DDIM chains.
"""
import json
import os

import numpy as np
import pytest
import torch

import attn_exact as A
import conv_exact as X
import test_conv_exact_gpu as TX          # run_exact: the launcher + comparator of the exact conv cases (conv_exact.py holds the data side only);
                                         # reused as it is, with its module-level cache of prepared references, rather than copied
import vq_ref
from util import GOLD, T, gold, rel_err, rms_err, seeded

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
LOSS = dict(target="torch.nn.Identity")
FP32_REL = 2e-5
CAP = 0.02

with open(os.path.join(GOLD, "ae3d_surface.json")) as _f:
    META = json.load(_f)
AE3D, UNET3D = META["ae3d"], META["unet3d"]
LAT = (2, 4, 4, 6, 6)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    return gold("ae3d")


@pytest.fixture(scope="module")
def kl(dev):
    from jointimagegeneration_amd.ldm import AutoencoderKL
    return seeded(AutoencoderKL(ddconfig=dict(AE3D), lossconfig=LOSS, embed_dim=4, dims=3), "ae3d_kl.").to(dev)


@pytest.fixture(scope="module")
def vq(dev):
    from jointimagegeneration_amd.ldm import VQModel
    m = seeded(VQModel(ddconfig=dict(AE3D), lossconfig=LOSS, n_embed=META["n_embed"], embed_dim=4, dims=3), "ae3d_vq.")
    m.quantize.embedding.weight.mul_(META["code_scale"])
    return m.to(dev)


def first_stage_cfg(vq_interface=False):
    if vq_interface:
        return dict(target="ldm.models.autoencoder.VQModelInterface",
                    params=dict(embed_dim=4, n_embed=META["n_embed"], dims=3, ddconfig=dict(AE3D), lossconfig=LOSS))
    return dict(target="ldm.models.autoencoder.AutoencoderKL", params=dict(embed_dim=4, dims=3, ddconfig=dict(AE3D), lossconfig=LOSS))


def build_ldm(dev, vq_interface=False):
    """The LatentDiffusion of make_golden_ae3d.py ("ldm3d." weights): dims = 3 UNetModel, concat conditioning, 300 timesteps."""
    from jointimagegeneration_amd.ldm import LatentDiffusion
    m = LatentDiffusion(first_stage_config=first_stage_cfg(vq_interface), cond_stage_config=first_stage_cfg(),
                        unet_config=dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(UNET3D)),
                        linear_start=0.0015, linear_end=0.0195, timesteps=META["timesteps"], image_size=6, channels=4, dims=3,
                        first_stage_key="image", cond_stage_key="mask", num_timesteps_cond=1, conditioning_key="concat")
    return seeded(m, "ldm3d.").to(dev)


@pytest.fixture(scope="module")
def ldm(dev):
    return build_ldm(dev)


@pytest.fixture(scope="module")
def op(dev, g):
    f = lambda k: T(g[k]).float().to(dev)
    return dict(c=f("c"), uc=f("uc"), x_T=f("x_T"), x0=f("x0"), hole=f("mask_hole"), q=list(f("q_tape")), step=list(f("step_tape")))


def report(name, got, want):
    e, r = rel_err(got, want), rms_err(got, want)
    print(f"{name}: max {e:.3e} rms {r:.3e}")
    return e, r


# ------------------------------------------------------------------------------------------------ 1. first stage against the reference
def test_first_stage_fp32_validation_matches_the_reference(dev, kl, vq, g):
    from jointimagegeneration_amd import ops
    img = T(g["img"]).to(dev)
    with ops.fp32_validation():
        post = kl.encode(img)
        dec = kl.decode(T(g["kl_z"]).to(dev))
        quant, _, (_, _, idx) = vq.encode(img)
        prequant = vq.encode_to_prequant(img)
        vq_dec = vq.decode(T(g["vq_quant"]).to(dev))
    assert tuple(post.mean.shape) == (1, 4, 3, 4, 5) and tuple(dec.shape) == (1, 1, 6, 8, 10)
    errs = {name: report("fp32 validation " + name, got, T(g[key]))[0]
            for name, got, key in (("KL mean", post.mean, "kl_mean"), ("KL logvar", post.logvar, "kl_logvar"), ("KL decode", dec, "kl_dec"),
                                   ("VQ prequant", prequant, "vq_prequant"), ("VQ quant", quant, "vq_quant"), ("VQ decode", vq_dec, "vq_dec"))}
    same = int((idx.view(-1).cpu() == T(g["vq_idx"]).long()).sum())
    print(f"fp32 validation VQ indices: {same} of {idx.numel()} equal the reference's")
    assert all(e < FP32_REL for e in errs.values()), errs
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (60, 1) and same == 60


def test_first_stage_bf16_matches_the_reference(dev, kl, vq, g):
    img = T(g["img"]).to(dev)
    post = kl.encode(img)
    dec = kl.decode(T(g["kl_z"]).to(dev))
    prequant = vq.encode_to_prequant(img)
    quant, _, (_, _, idx) = vq.encode(img)
    vq_dec = vq.decode(T(g["vq_quant"]).to(dev))
    res = [report("bf16 " + name, got, T(g[key]))
           for name, got, key in (("KL mean", post.mean, "kl_mean"), ("KL logvar", post.logvar, "kl_logvar"), ("KL decode", dec, "kl_dec"),
                                  ("VQ prequant", prequant, "vq_prequant"), ("VQ decode", vq_dec, "vq_dec"))]
    # indices: only rows inside the reference's near-tie margin may differ
    rows = T(g["vq_prequant"]).permute(0, 2, 3, 4, 1).reshape(-1, 4)
    E = vq.quantize.codebook().cpu()
    two = torch.topk(vq_ref.distances(rows, E), 2, dim=1, largest=False).values
    near = (two[:, 1] - two[:, 0]) < META["bf16_tol"] * (1.0 + two[:, 0])
    differ = idx.view(-1).cpu() != T(g["vq_idx"]).long()
    print(f"bf16 VQ indices: {int(differ.sum())} of {differ.numel()} differ from the reference's, {int((differ & ~near).sum())} of them outside "
          f"the near-tie margin; {int(near.sum())} rows ({100 * float(near.float().mean()):.2f} %) are inside it")
    assert all(e < 4e-2 and r < 2e-2 for e, r in res), res
    assert float(near.float().mean()) <= CAP
    assert int((differ & ~near).sum()) == 0
    # every quantised row is the straight-through value of ITS index on the engine's own pre-quantisation rows
    own = prequant.permute(0, 2, 3, 4, 1).reshape(-1, 4)
    assert torch.equal(quant.permute(0, 2, 3, 4, 1).reshape(-1, 4), vq_ref.straight_through(own, E.to(dev), idx.view(-1)))
    assert torch.equal(vq.decode_code(idx.view(1, 3, 4, 5)), vq.decode(vq.quantize.embed_code(idx.view(1, 3, 4, 5))))


def test_every_conv_of_the_autoencoder_runs_on_the_tiny_or_gather_kernel(dev, kl, g):
    """DESIGN.md 7e's table: at the fixture's sizes the 3 x 4 x 5 level (M = 60) runs on the tiny-M kernel, the 6 x 8 x 10 level
    (M = 480) on the gather kernel; no launch carries a fused GroupNorm prologue or leaves GroupNorm sums."""
    from jointimagegeneration_amd import _lib
    lib = _lib.load()
    sink = []
    with X.captured_descs(sink):
        kl.decode(kl.encode(T(g["img"]).to(dev)).mode())
    paths = [(d.N * d.Do * d.Ho * d.Wo, X.kernel_path(lib, d), d.prologue_act, bool(d.gn_acc)) for d in sink]
    for d, p in zip(sink, paths):
        print(f"conv {d.C1}->{d.Cout} k{d.kd}{d.kh}{d.kw} s{d.stride} p{d.pad} up{d.upsample} in {d.D}x{d.H}x{d.W}: M = {p[0]} {p[1]}")
    assert len(sink) == 40                                                     # 17 convs in the encoder path, 23 in the decoder path
    assert all(p == (60, "tiny", 0, False) or p == (480, "gather", 0, False) for p in paths), paths
    s2 = [d for d in sink if d.stride == 2]
    up = [d for d in sink if d.upsample]
    assert len(s2) == 1 and (s2[0].kd, s2[0].pad, s2[0].D, s2[0].Do, s2[0].Ho, s2[0].Wo) == (3, 0, 6, 3, 4, 5)
    assert len(up) == 1 and (up[0].kd, up[0].D, up[0].Do, up[0].Ho, up[0].Wo) == (3, 3, 6, 8, 10)


# ------------------------------------------------------------------------------------------------ 2. exact arithmetic
DOWN = dict(stride=2, pad=0)
EXACT_CONVS = [
    X.c3("ae3d_down_5x6x7", "tiny", 1, 32, 0, 32, (5, 6, 7), splitk=False, **DOWN),                 # 2 x 3 x 3 outputs: D and W end on the pad
    X.c3("ae3d_down_5x6x7_splitk", "tiny", 2, 64, 0, 64, (5, 6, 7), splitk=True, residual=True, **DOWN),
    X.c3("ae3d_down_5x6x7_n8", "gather", 8, 32, 0, 32, (5, 6, 7), splitk=True, bias="per_sample", **DOWN),      # M = 144: the gather kernel
    X.c3("ae3d_down_5x6x7_f32", "f32", 2, 15, 0, 40, (5, 6, 7), out_f32=True, **DOWN),               # the fp32 validation conv
    X.c3("ae3d_up_3x4x5", "gather", 1, 64, 0, 64, (3, 4, 5), up=True, splitk=True),
    X.c3("ae3d_up_3x4x5_n2", "gather", 2, 32, 0, 32, (3, 4, 5), up=True, splitk=True, residual=True),
    X.c3("ae3d_up_3x4x5_f32", "f32", 1, 15, 0, 33, (3, 4, 5), up=True, out_f32=True),
]


@pytest.mark.parametrize("cr", [(c, r) for c in EXACT_CONVS for r in (("D",) if c.path == "f32" else ("D", "S"))], ids=X.case_id)
def test_trailing_pad_downsample_and_d_doubling_upsample_bit_for_bit(dev, cr, monkeypatch):
    """Stride 2 with leading pad 0 / trailing pad 1 on D, H and W at 5 x 6 x 7 (odd and even extents), and the x2 upsample of D, H and W
    at 3 x 4 x 5, against fp64 with no tolerance (tests/conv_exact.py).  The dispatch fuses a GroupNorm prologue into neither (asserted:
    only the halo-tile and box kernels take one, and they take neither shape), so there is no prologue variant to run."""
    from jointimagegeneration_amd import _lib
    case, regime = cr
    assert case.out_sp == ((2, 3, 3) if case.stride == 2 else (6, 8, 10))
    if case.path != "f32":
        assert _lib.load().gg_conv_fuses_prologue(X.C.byref(X.case_desc(case, "P"))) == 0
    TX.run_exact(case, regime, dev, monkeypatch)


ATTN_CASES = [A.Case("ae3d_attn_t64", "plain", 64, 64, 64, layout="ae"), A.Case("ae3d_attn_t60", "plain", 64, 60, 60, layout="ae")]


@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: c.name)
def test_attnblock3d_attention_launch_bit_for_bit(dev, case):
    """The attention launch of AttnBlock3d (one head of 64 channels, q | k | v blocks in one row) at T = 4^3 = 64 and T = 3 * 4 * 5 = 60
    tokens -- one full 64-key tile, and a ragged one -- in the three exact regimes of tests/attn_exact.py."""
    A.assert_path(case)
    for regime in case.regimes():
        inp = A.build(case, regime)
        A.check_reference(regime, inp, A.reference(inp, dev))
        p = A.pack(case, inp).to(dev)
        A.launch(case, p, inp.scale)
        torch.cuda.synchronize()
        msg = A.check_output(case, inp, p.out)
        assert not msg, f"{case.name}/{regime}: {msg}"


@pytest.mark.parametrize("sp", [(4, 4, 4), (3, 4, 5)], ids=["T64", "T60"])
def test_attnblock3d_launches_that_attention_and_matches_fp32_validation(dev, sp, monkeypatch):
    """AttnBlock3d.run: GroupNorm -> fused q|k|v 1x1x1 conv -> ONE attention launch (N, 1 head of C, T = D * H * W, scale C^-1/2, q / k /
    v at channel offsets 0 / C / 2C of one row) -> proj_out + x.  Against the same block in fp32 validation mode at rel 3e-2, the bf16
    block bound of tests/test_unet_options_gpu.py."""
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.blocks import AttnBlock3d
    blk = seeded(AttnBlock3d(64), "ae3d_attn.").to(dev)
    assert [tuple(m.weight.shape) for m in (blk.q, blk.k, blk.v, blk.proj_out)] == [(64, 64, 1, 1, 1)] * 4
    x = torch.randn((2, 64) + sp, generator=torch.Generator().manual_seed(sum(sp))).to(dev)
    calls = []
    real = ops.attention
    monkeypatch.setattr(ops, "attention", lambda *a, **k: (calls.append((a[4:13], a[13], k)), real(*a, **k))[1])
    y = ops.from_cl(blk.run(ops.to_cl(x)), 3)
    Tn = sp[0] * sp[1] * sp[2]
    assert calls == [((2, 1, 64, Tn, Tn, (192, 64), (192, 64), (192, 64), (64, 64)), 64 ** -0.5, dict(q_off=0, k_off=64, v_off=128))]
    with ops.fp32_validation():
        ref = ops.from_cl(blk.run(ops.to_cl(x)), 3)
    err = rel_err(y, ref)
    print(f"AttnBlock3d T = {Tn}: rel {err:.3e} vs fp32 validation")
    assert tuple(y.shape) == tuple(x.shape) and err < 3e-2


# ------------------------------------------------------------------------------------------------ 3. sampling
def ddim(s, op, **kw):
    return s.sample(S=META["steps"], batch_size=2, shape=LAT[1:], conditioning=op["c"], verbose=False, x_T=op["x_T"], dims=3, **kw)


def test_ddim_chains_match_the_reference(dev, ldm, op, g):
    from jointimagegeneration_amd.ldm import DDIMSampler
    s = DDIMSampler(ldm)
    guided = dict(unconditional_guidance_scale=META["guidance_scale"], unconditional_conditioning=op["uc"])
    inpaint = dict(mask=op["hole"], x0=op["x0"], mask_noise_tape=op["q"])
    cases = [("z_plain_eta0", dict(), (2e-2, 1.5e-2)),
             ("z_mask_eta1", dict(eta=1.0, noise_tape=op["step"], **inpaint), (2e-2, 1.5e-2)),
             ("z_cfg_mask_eta0", dict(**inpaint, **guided), (6e-2, 3e-2)),
             ("z_cfg_mask_eta1", dict(eta=1.0, noise_tape=op["step"], **inpaint, **guided), (6e-2, 3e-2))]
    res = []
    for key, kw, bound in cases:
        z, inter = ddim(s, op, **kw)
        assert tuple(z.shape) == LAT and tuple(inter["pred_x0"][1].shape) == LAT
        res.append(report(f"3-D DDIM {key}", z, T(g[key])) + bound)
    assert np.array_equal(s.ddim_timesteps, g["ddim_timesteps"])
    assert all(e < be and r < br for e, r, be, br in res), res


def test_captured_chain_equals_eager_and_samples_are_independent(dev, ldm, op):
    """The eta = 0 chain is one captured graph and equals the eager chain bit for bit (also with the inpainting blend inside).  Sample 0
    is bit-equal whatever its neighbour holds, and bit-equal to the same sample run alone (batch 1): every kernel of this chain adds a
    sample's fp32 partial sums in an order that does not depend on the batch -- the tiny-M conv's split is a function of the channel
    counts alone, the gather conv's split-K is capped by the k-steps (KS / 8) at both grid sizes, GroupNorm and attention work per
    sample."""
    from jointimagegeneration_amd.ldm import DDIMSampler
    sg, se = DDIMSampler(ldm), DDIMSampler(ldm)
    se.use_graph = False
    for kw in (dict(), dict(mask=op["hole"], x0=op["x0"], mask_noise_tape=op["q"])):
        runs = [ddim(sg, op, **kw) for _ in range(3)]                          # eager warm-up, capture, replay
        z_e, inter_e = ddim(se, op, **kw)
        for z, inter in runs:
            assert torch.equal(z, z_e) and torch.equal(inter["pred_x0"][1], inter_e["pred_x0"][1])
    assert len(sg._graphs) == 2 and all(st["graph"] is not None for st in sg._graphs.values())
    assert all(st["graph"] is None for st in se._graphs.values())
    run = lambda x, c: se.sample(S=3, batch_size=x.shape[0], shape=LAT[1:], conditioning=c, verbose=False, x_T=x, dims=3)[0]
    both = run(op["x_T"], op["c"])
    other = run(torch.cat([op["x_T"][:1], op["x_T"][1:] * -1.5]), torch.cat([op["c"][:1], op["c"][1:].flip(-1)]))
    assert torch.equal(both[0], other[0]) and not torch.equal(both[1], other[1])
    solo = run(op["x_T"][:1], op["c"][:1])
    report("3-D DDIM sample 0: batch of 2 vs alone", both[:1], solo)
    assert torch.equal(both[:1], solo)


def plms_restatement(ldm, sampler, c, x_T, mask, x0, q_tape):
    """The reference's plms_sampling / p_sample_plms (plms.py:113-236) written out in fp32 torch ops on [N, C, D, H, W] tensors, eta = 0:
    the blend before each step, pseudo improved Euler first, then Adams-Bashforth of order 2, 3, 4.  eps comes from the engine's own
    eager apply_model; the schedule tables are the sampler's (the 2-D tests pin them to the reference)."""
    S = sampler.ddim_timesteps.shape[0]
    steps = np.flip(sampler.ddim_timesteps)
    dev = x_T.device
    a, ap, s1 = (t.to(dev).float() for t in (sampler.ddim_alphas, sampler.ddim_alphas_prev, sampler.ddim_sqrt_one_minus_alphas))
    eps = lambda x, t: ldm.apply_model(x, torch.full((x.shape[0],), int(t), device=dev), c)

    def update(x, e, index):
        pred = (x - s1[index] * e) / a[index].sqrt()
        return ap[index].sqrt() * pred + (1.0 - ap[index]).sqrt() * e

    img, old = x_T, []
    for i, step in enumerate(steps):
        index = S - i - 1
        t = torch.full((img.shape[0],), int(step), device=dev)
        img = ldm.q_sample(x0, t, noise=q_tape[i]) * mask + (1.0 - mask) * img
        e_t = eps(img, step)
        if len(old) == 0:
            e_next = eps(update(img, e_t, index), steps[min(i + 1, S - 1)])
            e_p = (e_t + e_next) / 2
        elif len(old) == 1:
            e_p = (3 * e_t - old[-1]) / 2
        elif len(old) == 2:
            e_p = (23 * e_t - 16 * old[-1] + 5 * old[-2]) / 12
        else:
            e_p = (55 * e_t - 59 * old[-1] + 37 * old[-2] - 9 * old[-3]) / 24
        img = update(img, e_p, index)
        old = (old + [e_t])[-3:]
    return img


def test_plms_and_ancestral_chains_on_volumes(dev, ldm, op, g):
    """The reference's PLMSSampler is 2-D only (plms.py:93 unpacks C, H, W; :201-204 builds [b, 1, 1, 1] scalars), so the 3-D PLMS chain
    is held to the restatement above, 5 steps (all four multistep orders) with the inpainting blend, at the PLMS bound of
    tests/test_inpaint_gpu.py (max 1.5e-2, rms 1e-2): both sides evaluate the same bf16 UNet, on states that differ by fp32 rounding.
    The ancestral loop has a reference fixture (3 timesteps, mask, both tapes) and that file's ancestral bound (max 1.5e-2, rms 1e-2);
    its known region is q_sample(x0, 0) with the last blend noise."""
    from jointimagegeneration_amd.ldm import PLMSSampler
    gen = torch.Generator().manual_seed(77)
    q5 = [torch.randn(LAT, generator=gen).to(dev) for _ in range(5)]
    s = PLMSSampler(ldm)
    z, _ = s.sample(S=5, batch_size=2, shape=LAT[1:], conditioning=op["c"], verbose=False, x_T=op["x_T"], dims=3,
                    mask=op["hole"], x0=op["x0"], mask_noise_tape=q5)
    want = plms_restatement(ldm, s, op["c"], op["x_T"], op["hole"], op["x0"], q5)
    e, r = report("3-D PLMS 5 steps with mask vs the torch restatement", z, want)
    free, _ = s.sample(S=5, batch_size=2, shape=LAT[1:], conditioning=op["c"], verbose=False, x_T=op["x_T"], dims=3)
    assert tuple(z.shape) == LAT and e < 1.5e-2 and r < 1e-2
    assert float((free - z).abs().max()) > 1e-2                                # the blend changed the chain
    za = ldm.p_sample_loop(op["c"], LAT, x_T=op["x_T"], verbose=False, timesteps=3, noise_tape=op["step"], mask=op["hole"], x0=op["x0"],
                           mask_noise_tape=op["q"])
    ea, ra = report("3-D ancestral 3 timesteps with mask", za, T(g["z_ancestral_mask"]))
    known = ldm.sqrt_alphas_cumprod[0] * op["x0"] + ldm.sqrt_one_minus_alphas_cumprod[0] * op["q"][2]
    err_known = float(((za - known) * op["hole"]).abs().max())
    print(f"known region vs q_sample(x0, 0): {err_known:.2e}")
    assert ea < 1.5e-2 and ra < 1e-2 and err_known <= 1e-6


def test_quantize_x0_and_the_eager_model_carry_volumes(dev, ldm, op):
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.ldm import DDIMSampler, first_stage_codebook
    # eager apply_model: cat on dim 1, UNetModel.forward on [N, C, D, H, W]
    t = torch.full((2,), 201, device=dev)
    eps = ldm.apply_model(op["x_T"], t, op["c"])
    assert tuple(eps.shape) == LAT
    assert torch.equal(eps, ldm.model.diffusion_model(torch.cat([op["x_T"], op["c"]], 1), t))
    with ops.fp32_validation():
        ref = ldm.apply_model(op["x_T"], t, op["c"])
    e, r = report("3-D apply_model bf16 vs fp32 validation", eps, ref)
    assert e < 3e-2 and r < 2e-2                                               # the small LDM UNet forward bound of tests/test_hip_parity.py
    # quantize_x0 with a volumetric VQModelInterface first stage: pred_x0 holds codebook rows
    vqldm = build_ldm(dev, vq_interface=True)
    E = first_stage_codebook(vqldm, "test", 4)
    for kw in (dict(), dict(eta=1.0, noise_tape=op["step"])):
        zq, inter = ddim(DDIMSampler(vqldm), op, quantize_x0=True, **kw)
        q = inter["pred_x0"][1].permute(0, 2, 3, 4, 1).reshape(-1, 4).contiguous()
        idx, _ = ops.vq_nearest(q, E, want_st=False)
        assert bool(torch.isfinite(zq).all()) and bool(((q - E[idx.long()]).abs() <= 2.0 ** -22 * (1.0 + E[idx.long()].abs())).all())
    h = torch.randn(1, 4, 3, 4, 5, generator=torch.Generator().manual_seed(9)).to(dev)
    fs = vqldm.first_stage_model
    assert torch.equal(vqldm.decode_first_stage(h), fs.decode(h)) and not torch.equal(fs.decode(h), fs.decode(h, force_not_quantize=True))


# ------------------------------------------------------------------------------------------------ 4. round trip
def test_first_stage_round_trip_returns_the_input_shape(dev, ldm, g):
    from jointimagegeneration_amd.ldm import DiagonalGaussianDistribution
    img = T(g["img"]).to(dev)
    post = ldm.encode_first_stage(img)
    assert isinstance(post, DiagonalGaussianDistribution)
    z = ldm.get_first_stage_encoding(post.mode())
    assert tuple(z.shape) == (1, 4, 3, 4, 5) and torch.equal(z, ldm.scale_factor * post.mean)
    out = ldm.decode_first_stage(z)
    assert tuple(out.shape) == tuple(img.shape) and bool(torch.isfinite(out).all())
    assert tuple(ldm.get_first_stage_encoding(post).shape) == (1, 4, 3, 4, 5)          # a posterior sample
    c = ldm.get_learned_conditioning(img)                                              # the cond stage: a second autoencoder with weights of its own
    assert tuple(c.shape) == (1, 4, 3, 4, 5) and torch.equal(c, ldm.cond_stage_model.encode(img).mode()) and not torch.equal(c, post.mean)
