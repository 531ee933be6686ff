"""GPU suite (-m gpu): every ops.* kernel call of the production networks, at its real shape, batch size and plan, against an fp64
reference of that call (tests/shadow.py), at batch sizes 1, 2 and 8.

Eager runs only (no graph capture), distinct seeded inputs per sample.  Each test asserts that every shadowed call is inside the bound
of tests/shadow.py, that every sample of every conv / GroupNorm / attention call was checked, and that the kernel plans this suite is
meant to cover still occur (from the host predicates recorded per call).  It prints one line per op family: worst err / bound, number
of calls, number of distinct plans."""
import gc

import pytest
import torch

from shadow import shadow_ops
from util import CCDM_FULL, CCDM_SMALL, LDM_SMALL, SEED, seeded, synth_labels

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    torch.cuda.reset_peak_memory_stats()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ldm(dev):
    from jointimagegeneration_amd.pipeline import build_ldm
    return build_ldm(SEED, dev)


@pytest.fixture(scope="module")
def ccdm(dev):
    from jointimagegeneration_amd.synth import randomize_parameters
    from jointimagegeneration_amd.unet import create_unet_openai
    u = create_unet_openai(image_size=128, in_channels=15, out_channels=14, num_res_blocks=2, cond_encoded_shape=None, dims=3,
                           **CCDM_FULL).eval()
    randomize_parameters(u, SEED, "ccdm.")
    return u.to(dev)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def free():
    gc.collect()
    torch.cuda.empty_cache()


def report(sh, title, N):
    print()
    print(sh.summary(f"{title} N={N}"))
    print(f"{title} N={N}: peak GPU memory so far {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    sh.assert_within_bounds(N)


def convs(sh, sp, k, cout=None):
    """conv records whose input extent is sp, kernel k, stride 1, no upsample, bf16 output (and Cout == cout)"""
    out = []
    for r in sh.records:
        p = dict(r.plan)
        if r.family == "conv" and r.shape[1:4] == sp and r.shape[6:] == k and p["stride"] == 1 and not p["upsample"] \
                and not p["out_f32"] and (cout is None or r.shape[5] == cout):
            out.append(p)
    return out


def test_ldm_c5_latent_unet_ddim_step(dev, ldm):
    """C5 latent UNet (4 latent + 4 concat channels at 64 x 64, 160 base channels): one deterministic DDIM step with the update fused
    into the head conv, at N = 1, 2, 8.  At N = 8 the 64 x 64 3x3 convs run on the halo-tile kernel with 32-stripe statistics, at N = 1
    on the box kernel; the tiny-M path (M <= 128, no prologue) occurs at N = 1."""
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.ldm import DDIMSampler
    for N in (1, 2, 8):
        with shadow_ops() as sh:
            ops.invalidate_caches(ldm)
            sampler = DDIMSampler(ldm)
            sampler.use_graph = False
            sampler.make_schedule(50, ddim_eta=0.0, verbose=False)
            g = gen(SEED + N)
            x_T = torch.randn(N, 4, 64, 64, generator=g).to(dev)
            cc = torch.randn(N, 4, 64, 64, generator=g).to(dev)
            st = sampler.prepare_state(N, 4, (64, 64), dev, 4)
            sampler.load_state(st, x_T, cc)
            sampler._step(st, None, st["table"][0], st["scal"][0], None)
            assert sampler.last_step_fused, "the DDIM update no longer runs as the head conv's epilogue"
            if N == 2:                          # the next step with the update as its own launch (gg_ddim_step)
                sampler.fuse_ddim = False
                sampler._step(st, None, st["table"][1], st["scal"][1], None)
            torch.cuda.synchronize()
        report(sh, "LDM C5 DDIM step", N)
        assert any(r.family == "conv.ddim" for r in sh.records)
        assert N != 2 or any(r.family == "ddim_step" for r in sh.records)
        c64 = convs(sh, (1, 64, 64), (1, 3, 3), 160)
        halo = [p for p in c64 if p["halo"] and p["stats"] == 32]
        print(f"LDM C5 N={N}: {len(halo)} of {len(c64)} 64x64 3x3 160-channel convs on the halo-tile kernel with 32-stripe statistics")
        assert c64, "no 64x64 3x3 conv of 160 channels was recorded"
        if N == 8:
            plain = [p for p in c64 if not p["skip"]]
            assert plain and all(p["halo"] and p["stats"] == 32 for p in plain), \
                "plan no longer occurs: LDM 64x64 3x3 convs at N = 8 on the halo-tile kernel with 32-stripe statistics"
        if N == 1:
            assert not any(p["halo"] for p in c64), "plan changed: LDM 64x64 3x3 convs at N = 1 are no longer on the box kernel"
            tiny = [r for r in sh.records if r.family == "conv" and dict(r.plan)["tiny_m"]]
            print(f"LDM C5 N=1: {len(tiny)} tiny-M convs (M <= 128, no prologue)")
            assert tiny, "plan no longer occurs: the tiny-M conv path (M <= 128, no prologue)"
        del sampler, st, sh
        free()


def test_autoencoders_encode_and_decode(dev, ldm):
    """Cond-stage encode of a 512 x 512 two-channel mask slice and first-stage decode of a 64 x 64 latent, at N = 1 and 8."""
    from jointimagegeneration_amd import ops
    for N in (1, 8):
        g = gen(SEED + 100 + N)
        lab = torch.stack([torch.from_numpy(synth_labels((1, 512, 512), 12, seed=n))[0] for n in range(N)]).float()
        cond = torch.stack([torch.rand(N, 512, 512, generator=g) * 2 - 1, lab / 255.0], 1).to(dev)
        z = torch.randn(N, 4, 64, 64, generator=g).to(dev)
        with shadow_ops() as sh:
            ops.invalidate_caches(ldm)
            ldm.cond_stage_model.encode_moments_cl(ops.to_cl(cond))
            ldm.first_stage_model.decode_cl(ops.to_cl(z))
            torch.cuda.synchronize()
        report(sh, "AE encode + decode", N)
        assert any(r.family == "attention" for r in sh.records)
        del sh, cond, z
        free()


def test_ccdm_128_unet_forward(dev, ccdm):
    """One plain forward of the full 128^3 CCDM UNet (K = 14) at N = 1, 2, 8; at N = 8 the top up path concatenates 64 + 64 channels
    into [8, 128, 128, 128, 128] = 2^31 elements.  The 16^3 convs of 256 channels take a split-K workspace at N = 1 and the halo-tile
    kernel at N >= 2."""
    from jointimagegeneration_amd import ops
    from oracle import samplers as S
    K, R = 14, 128
    for N in (1, 2, 8):
        lab = torch.stack([torch.from_numpy(synth_labels((R, R, R), K, seed=11 + n)) for n in range(N)])
        x = S.one_hot_bchw(lab, K).to(dev)
        cond = torch.zeros(N, 1, R, R, R, device=dev)
        t = torch.tensor([17.0 + 40 * n for n in range(N)], device=dev)          # distinct per-sample time-bias rows
        del lab
        with shadow_ops() as sh:
            ops.invalidate_caches(ccdm)
            out = ccdm(x, cond, None, t)["diffusion_out"]
            torch.cuda.synchronize()
        report(sh, "CCDM 128^3 forward", N)
        c16 = convs(sh, (16, 16, 16), (3, 3, 3), 256)
        print(f"CCDM N={N}: 16^3 3x3x3 256-channel convs: {sum(1 for p in c16 if p['ws'] > 0)} with a split-K workspace, "
              f"{sum(1 for p in c16 if p['halo'])} on the halo-tile kernel, of {len(c16)}")
        assert c16, "no 16^3 3x3x3 conv of 256 channels was recorded"
        if N == 1:
            assert any(p["ws"] > 0 and not p["halo"] for p in c16) and not any(p["halo"] for p in c16), \
                "plan no longer occurs: CCDM 16^3 convs at N = 1 with a split-K workspace"
        else:
            plain = [p for p in c16 if not p["skip"]]
            assert plain and all(p["halo"] for p in plain), "plan no longer occurs: CCDM 16^3 convs at N >= 2 on the halo-tile kernel"
        if N == 8:
            big = [r for r in sh.records if r.family == "conv" and r.shape[1:5] == (R, R, R, 128)]
            print(f"CCDM N=8: {len(big)} convs read a {N} x 128^3 x 128 (2^31-element) concat")
            assert big, "the 2^31-element concat of the top up path was not shadowed"
        del x, cond, out, sh
        free()


@pytest.mark.usefixtures("halo_hint")
def test_small_and_option_networks(dev, monkeypatch):
    """CCDM_SMALL, LDM_SMALL, the option-bearing networks of test_unet_options_gpu.py and an LDM_SMALL with a cross-attention
    SpatialTransformer (fused and separate GEGLU) under the halo_hint path hints, N = 2."""
    from jointimagegeneration_amd import blocks
    from jointimagegeneration_amd.unet import CCDMUNetModel, UNetModel
    N = 2
    ON = dict(use_scale_shift_norm=True, resblock_updown=True, use_new_attention_order=True)
    ST = dict(use_spatial_transformer=True, context_dim=64)
    cfg = dict(CCDM_SMALL)
    base = cfg.pop("base_channels")
    g = gen(SEED + 7)
    lab = torch.randint(0, 6, (N, 16, 16, 16), generator=g)
    xc = torch.nn.functional.one_hot(lab, 6).permute(0, 4, 1, 2, 3).float().to(dev)
    cc = torch.randn(N, 1, 16, 16, 16, generator=g).to(dev)
    tc = torch.tensor([5.0, 90.0], device=dev)
    xl = torch.randn(N, 8, 16, 16, generator=g).to(dev)
    tl = torch.tensor([981.0, 21.0], device=dev)
    ctx = torch.randn(N, 7, 64, generator=g).to(dev)
    nets = (("ccdm_small", {}), ("ccdm_opt", ON), ("ccdm_nc", dict(conv_resample=False)), ("ldm_small", {}), ("ldm_opt", ON),
            ("ldm_st", ST), ("ldm_st_geglu", ST))
    for name, opts in nets:
        monkeypatch.setattr(blocks, "FUSE_GEGLU", name != "ldm_st_geglu")
        with shadow_ops() as sh:
            if name.startswith("ccdm"):
                u = seeded(CCDMUNetModel(in_channels=7, model_channels=base, out_channels=6, num_res_blocks=2, cond_encoded_shape=None,
                                         dims=3, **cfg, **opts), name + ".").to(dev)
                u(xc, cc, None, tc)
            else:
                u = seeded(UNetModel(**LDM_SMALL, **opts), name + ".").to(dev)
                u(xl, tl, ctx if "context_dim" in opts else None)
            torch.cuda.synchronize()
        report(sh, name, N)
        fams = {r.family for r in sh.records}
        if opts.get("use_scale_shift_norm"):
            assert "film_fold" in fams
        if opts.get("resblock_updown") or opts.get("conv_resample") is False:
            assert "resample2x" in fams
        if "context_dim" in opts:
            assert "layernorm" in fams and ("geglu" in fams) == (name == "ldm_st_geglu")
            assert any(dict(r.plan)["geglu"] for r in sh.records if r.family == "conv") == (name == "ldm_st")
        if name.startswith("ccdm"):
            assert any(dict(r.plan)["halo"] for r in sh.records if r.family == "conv"), "no conv ran on the halo-tile kernel"
        del u, sh
        free()
