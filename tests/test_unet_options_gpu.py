"""GPU suite: the UNet constructor options use_scale_shift_norm (FiLM), resblock_updown, use_new_attention_order and conv_resample=False
against what the REFERENCE modules computed (tests/golden/unet_options.npz, make_golden_unet_options.py), on the bf16 path and under
ops.fp32_validation(); per-sample FiLM independence; captured graphs of option-bearing networks equal their eager runs; the resample
kernel against torch.

The fixture shapes are small, so their convs run on the box / gather kernels.  The halo-tile conv (whose fused prologue takes the FiLM
coefficients at production sizes) needs outputs of at least 4 x 8 x 16 positions; there the 3-D blocks are compared with this engine's
fp32 validation mode, which the fixtures pin to the reference at 2e-5.

Tolerances: bf16 blocks rel 3e-2 (the bound of test_blocks_match_reference_fixtures); fp32 validation blocks rel 2e-5 of the output
scale (measured on one MI355X: worst 7.7e-7), fp32 CCDM network probabilities abs 2e-5 (measured 1.5e-6); networks as the networks_small
fixtures (CCDM probabilities abs 1.5e-2, measured 1.1e-2; LDM eps rel 3e-2 / rms 2e-2, measured 1.3e-2 / 1.0e-2); halo-shaped blocks
vs fp32 validation rel 3e-2 (measured <= 4.9e-3).  Measured values are printed."""
import pytest
import torch
import torch.nn.functional as F

from util import CCDM_SMALL, LDM_SMALL, T, gold, rel_err, rms_err, seeded

pytestmark = pytest.mark.gpu

ON = dict(use_scale_shift_norm=True, resblock_updown=True, use_new_attention_order=True)
FP32_REL = 2e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _resblocks(name, dims):
    from jointimagegeneration_amd import blocks as B
    return {
        "rbf3a": lambda: B.ResBlock(64, 128, 0.0, out_channels=96, dims=3, use_scale_shift_norm=True),
        "rbf3b": lambda: B.ResBlock(64, 128, 0.0, out_channels=64, dims=3, use_scale_shift_norm=True),
        "rbd3": lambda: B.ResBlock(64, 128, 0.0, dims=3, down=True),
        "rbu3": lambda: B.ResBlock(64, 128, 0.0, dims=3, up=True),
        "rbdf3": lambda: B.ResBlock(64, 128, 0.0, dims=3, down=True, use_scale_shift_norm=True),
        "rbuf3": lambda: B.ResBlock(64, 128, 0.0, dims=3, up=True, use_scale_shift_norm=True),
        "rbf2a": lambda: B.ResBlock(64, 128, 0.0, out_channels=96, dims=2, use_scale_shift_norm=True),
        "rbf2b": lambda: B.ResBlock(64, 128, 0.0, out_channels=64, dims=2, use_scale_shift_norm=True),
        "rbd2": lambda: B.ResBlock(64, 128, 0.0, dims=2, down=True),
        "rbu2": lambda: B.ResBlock(64, 128, 0.0, dims=2, up=True),
    }[name]()


def _run_resblock(dev, g, name, dims):
    from jointimagegeneration_amd import ops
    rb = seeded(_resblocks(name, dims), name + ".").to(dev)
    x, emb = T(g[name + "_x"]), T(g[name + "_emb"])
    tb = torch.zeros(x.shape[0], rb.time_bias_width, device=dev)
    rb.time_bias(emb.to(dev), tb)
    return ops.from_cl(rb.run(ops.to_cl(x.to(dev)), tb.view(-1)), dims)


def _run_attention(dev, g, name, dims):
    from jointimagegeneration_amd import blocks as B
    from jointimagegeneration_amd import ops
    ab = B.AttentionBlock(64, num_head_channels=32, use_new_attention_order=True) if name == "abn3" else \
        B.AttentionBlock(96, num_heads=-1, num_head_channels=32, use_new_attention_order=True)
    assert ab.num_heads >= 2
    ab = seeded(ab, name + ".").to(dev)
    return ops.from_cl(ab.run(ops.to_cl(T(g[name + "_x"]).to(dev))), dims)


def _run_resample(dev, g, name, dims, up):
    from jointimagegeneration_amd import blocks as B
    from jointimagegeneration_amd import ops
    m = (B.Upsample if up else B.Downsample)(48, False, dims=dims)
    return ops.from_cl(m.run(ops.to_cl(T(g[name + "_x"]).to(dev))), dims)


CONV_3D = ["rbf3a", "rbf3b", "rbd3", "rbu3", "rbdf3", "rbuf3"]
CONV_2D = ["rbf2a", "rbf2b", "rbd2", "rbu2"]


@pytest.mark.parametrize("name", CONV_3D)
def test_3d_resblocks_with_options_match_the_reference_bf16(dev, name):
    g = gold("unet_options")
    y = _run_resblock(dev, g, name, 3)
    err = rel_err(y, T(g[name + "_y"]))
    print(f"{name}: rel {err:.3e}")
    assert err < 3e-2


# input extents whose conv outputs are 4 x 8 x 16 (the smallest 3-D halo-tile shape)
HALO_IN = {"rbf3a": (4, 8, 16), "rbf3b": (4, 8, 16), "rbd3": (8, 16, 32), "rbdf3": (8, 16, 32), "rbu3": (2, 4, 8), "rbuf3": (2, 4, 8)}


@pytest.mark.parametrize("name", CONV_3D)
def test_3d_resblocks_on_the_halo_kernel_match_fp32_validation(dev, name, halo_hint):
    """The 3-D blocks at shapes the halo-tile conv takes (under the test path hints), inside a network forward's GroupNorm-sum arena:
    FiLM coefficients then come from the halo producer's sums (gg_groupnorm_scale_shift_acc), go through gg_film_fold and into the
    halo conv's fused prologue, as at 128^3.  Reference: the same block in fp32 validation mode."""
    from jointimagegeneration_amd import ops
    rb = seeded(_resblocks(name, 3), name + ".").to(dev)
    gen = torch.Generator().manual_seed(len(name))
    x = torch.randn((2, 64) + HALO_IN[name], generator=gen).bfloat16().float().to(dev)
    emb = torch.randn(2, 128, generator=gen).to(dev)
    cout = rb.out_channels
    h1 = ops.CL(torch.empty((2, 4, 8, 16, ops.pad32(cout)), dtype=torch.bfloat16, device=dev), cout)
    assert ops.conv_runs_halo_tile(h1, cout, k=(3, 3, 3)) and ops.conv_fuses_prologue(h1, cout, k=(3, 3, 3))      # conv2 + its norm

    def run():
        tb = torch.zeros(2, rb.time_bias_width, device=dev)
        rb.time_bias(emb, tb)
        ops.stats_begin(dev)
        try:
            return ops.from_cl(rb.run(ops.to_cl(x), tb.view(-1)), 3)
        finally:
            ops.stats_end(dev)

    y = run()
    with ops.fp32_validation():
        ref = run()
    err = rel_err(y, ref)
    print(f"{name} @ halo shape: rel {err:.3e} vs fp32 validation")
    assert err < 3e-2


def test_2d_blocks_attention_and_resampling_match_the_reference_bf16(dev):
    g = gold("unet_options")
    for name in CONV_2D + ["rbf3a", "rbd3", "rbu3"]:            # + production dispatch of the 3-D blocks
        err = rel_err(_run_resblock(dev, g, name, 2 if name in CONV_2D else 3), T(g[name + "_y"]))
        print(f"{name}: rel {err:.3e}")
        assert err < 3e-2, name
    for name, dims in (("abn3", 3), ("abn2", 2)):
        err = rel_err(_run_attention(dev, g, name, dims), T(g[name + "_y"]))
        print(f"{name}: rel {err:.3e}")
        assert err < 3e-2, name
    for name, dims in (("rs3", 3), ("rs2", 2)):
        up, dn = _run_resample(dev, g, name, dims, True), _run_resample(dev, g, name, dims, False)
        # the input is rounded to bf16 once; nearest copies it, the pool rounds its fp32 mean once
        assert torch.equal(up.cpu(), F.interpolate(T(g[name + "_x"]).bfloat16().float(), scale_factor=2, mode="nearest"))
        assert rel_err(up, T(g[name + "_up"])) < 1e-2 and rel_err(dn, T(g[name + "_dn"])) < 1e-2


def test_blocks_with_options_match_the_reference_fp32_validation(dev):
    from jointimagegeneration_amd import ops
    g = gold("unet_options")
    worst = 0.0
    with ops.fp32_validation():
        for name in CONV_3D + CONV_2D:
            err = rel_err(_run_resblock(dev, g, name, 2 if name in CONV_2D else 3), T(g[name + "_y"]))
            print(f"fp32 {name}: rel {err:.3e}")
            worst = max(worst, err)
            assert err < FP32_REL, name
        for name, dims in (("abn3", 3), ("abn2", 2)):
            err = rel_err(_run_attention(dev, g, name, dims), T(g[name + "_y"]))
            print(f"fp32 {name}: rel {err:.3e}")
            assert err < FP32_REL, name
        for name, dims in (("rs3", 3), ("rs2", 2)):
            assert rel_err(_run_resample(dev, g, name, dims, True), T(g[name + "_up"])) == 0.0
            assert rel_err(_run_resample(dev, g, name, dims, False), T(g[name + "_dn"])) < 1e-6
    print(f"fp32 validation blocks: worst rel {worst:.3e}")


def _ccdm(name, **opts):
    from jointimagegeneration_amd.unet import CCDMUNetModel
    cfg = dict(CCDM_SMALL)
    base = cfg.pop("base_channels")
    return seeded(CCDMUNetModel(in_channels=7, model_channels=base, out_channels=6, num_res_blocks=2, cond_encoded_shape=None, dims=3,
                                **cfg, **opts), name + ".")


def _ccdm_inputs(g, dev):
    from oracle import samplers as S
    return S.one_hot_bchw(T(g["ccdm_labels"]).long(), 6).to(dev), T(g["ccdm_cond"]).to(dev), T(g["ccdm_t"]).to(dev)


@pytest.mark.parametrize("hint", [0, 1], ids=["production_dispatch", "halo_hint_box512"])
def test_option_networks_match_the_reference(dev, hint, monkeypatch):
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.unet import UNetModel
    monkeypatch.setattr(ops, "PATH_HINT", hint)
    g = gold("unet_options")
    xt, cond, t = _ccdm_inputs(g, dev)
    for name, opts in (("ccdm_opt", ON), ("ccdm_nc", dict(conv_resample=False))):
        out = _ccdm(name, **opts).to(dev)(xt, cond, None, t)["diffusion_out"]
        err = float((out.cpu() - T(g[name + "_probs"])).abs().max())
        print(f"{name}: probabilities max abs {err:.3e}")
        assert err < 1.5e-2
    u = seeded(UNetModel(**LDM_SMALL, **ON), "ldm_opt.").to(dev)
    e = u(T(g["ldm_x"]).to(dev), T(g["ldm_t"]).to(dev))
    r, m = rel_err(e, T(g["ldm_opt_eps"])), rms_err(e, T(g["ldm_opt_eps"]))
    print(f"ldm_opt: eps rel {r:.3e} rms {m:.3e}")
    assert r < 3e-2 and m < 2e-2


def test_option_networks_fp32_validation(dev):
    from jointimagegeneration_amd import ops
    g = gold("unet_options")
    xt, cond, t = _ccdm_inputs(g, dev)
    with ops.fp32_validation():
        out = _ccdm("ccdm_opt", **ON).to(dev)(xt, cond, None, t)["diffusion_out"]
    err = float((out.cpu() - T(g["ccdm_opt_probs"])).abs().max())
    print(f"fp32 ccdm_opt: probabilities max abs {err:.3e}")
    assert err < 2e-5


def test_film_coefficients_follow_their_own_sample(dev):
    """Sample 0's output is bit-identical whatever sample 1's input and timestep are (FiLM rows indexed by the right sample)."""
    g = gold("unet_options")
    u = _ccdm("ccdm_opt", **ON).to(dev)
    xt, cond, t = _ccdm_inputs(g, dev)
    a = u(xt, cond, None, t)["diffusion_out"]
    xt2, cond2 = xt.clone(), cond.clone()
    xt2[1] = xt[1].roll(1, 0)
    cond2[1] = -cond[1]
    b = u(xt2, cond2, None, torch.tensor([t[0].item(), 3.0], device=dev))["diffusion_out"]
    assert torch.equal(a[0], b[0])
    assert not torch.equal(a[1], b[1])


def test_option_networks_captured_graphs_equal_eager(dev):
    from jointimagegeneration_amd.ccdm import DenoisingModel, DiffusionModel
    g = gold("unet_options")
    u = _ccdm("ccdm_opt", **ON).to(dev)
    model = DenoisingModel(DiffusionModel("cosine", 8, 6, dims=3), u, "none", "majority", dims=3).eval().to(dev)
    labels = T(g["ccdm_labels"]).int().to(dev)
    cond = T(g["ccdm_cond"]).to(dev)
    a, pa = model.sample_labels(labels, cond)                  # warm-up eager, then one captured reverse step replayed
    model.use_graph = False
    b, pb = model.sample_labels(labels, cond)
    assert torch.equal(a, b) and torch.equal(pa, pb)
    # DDIM chain graph on an option-bearing LDM UNet
    from jointimagegeneration_amd.ldm import DDIMSampler, LatentDiffusion
    from util import AE_SMALL
    cfg_unet = dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(LDM_SMALL, **ON))
    cfg_ae = dict(target="ldm.models.autoencoder.AutoencoderKL", params=dict(embed_dim=4, dims=2, ddconfig=dict(AE_SMALL), lossconfig=dict(target="torch.nn.Identity")))
    cfg_cond = dict(target="ldm.models.autoencoder.AutoencoderKL", params=dict(embed_dim=4, dims=2, ddconfig=dict(AE_SMALL, in_channels=2, out_ch=2), lossconfig=dict(target="torch.nn.Identity")))
    m = seeded(LatentDiffusion(first_stage_config=cfg_ae, cond_stage_config=cfg_cond, unet_config=cfg_unet, linear_start=0.0015,
                               linear_end=0.0195, timesteps=1000, image_size=8, channels=4, dims=2, first_stage_key="image",
                               cond_stage_key="mask", num_timesteps_cond=1), "ldm_opt_pipe.").to(dev)
    gen = torch.Generator().manual_seed(5)
    c = torch.randn(2, 4, 8, 8, generator=gen).to(dev)
    x_T = torch.randn(2, 4, 8, 8, generator=gen).to(dev)
    s_graph = DDIMSampler(m)
    za, _ = s_graph.sample(S=5, batch_size=2, shape=(4, 8, 8), conditioning=c, verbose=False, x_T=x_T, dims=2)
    zc, _ = s_graph.sample(S=5, batch_size=2, shape=(4, 8, 8), conditioning=c, verbose=False, x_T=x_T, dims=2)
    assert next(iter(s_graph._graphs.values()))["graph"] is not None
    s_eager = DDIMSampler(m)
    s_eager.use_graph = False
    zb, _ = s_eager.sample(S=5, batch_size=2, shape=(4, 8, 8), conditioning=c, verbose=False, x_T=x_T, dims=2)
    assert torch.equal(za, zb) and torch.equal(zc, zb)


def _ulps(got, ref):
    """|got - ref| in bf16 ulps of the larger magnitude (both bf16-representable)."""
    mag = torch.maximum(got.abs(), ref.abs()).clamp_min(2.0 ** -126)
    _, e = torch.frexp(mag)
    return (got - ref).abs() / torch.ldexp(torch.ones_like(mag), e - 8)


@pytest.mark.parametrize("dims", [2, 3])
def test_resample_kernel_vs_torch(dev, dims):
    from jointimagegeneration_amd import ops
    gen = torch.Generator().manual_seed(11 + dims)
    N, C, sp = 2, 40, ((4, 6, 10) if dims == 3 else (6, 10))
    x = torch.randn((N, C) + sp, generator=gen).bfloat16().float()
    xcl = ops.to_cl(x.to(dev))
    pool = F.avg_pool3d if dims == 3 else F.avg_pool2d
    up = ops.resample2x(xcl, True, dims == 3)
    assert torch.equal(ops.from_cl(up, dims).cpu(), F.interpolate(x, scale_factor=2, mode="nearest"))
    assert float(up.t[..., C:].abs().max()) == 0.0
    dn = ops.resample2x(xcl, False, dims == 3)
    assert float(_ulps(ops.from_cl(dn, dims).cpu(), pool(x, 2).bfloat16().float()).max()) <= 1.0
    sc, sh = torch.zeros(N, 64), torch.zeros(N, 64)
    sc[:, :C] = 1 + 0.3 * torch.randn(N, C, generator=gen)
    sh[:, :C] = 0.5 * torch.randn(N, C, generator=gen)
    bshape = (N, C) + (1,) * dims
    y = F.silu(x * sc[:, :C].reshape(bshape) + sh[:, :C].reshape(bshape))
    dp = ops.resample2x(xcl, False, dims == 3, prologue=(sc.to(dev), sh.to(dev)), act=True)
    assert float(_ulps(ops.from_cl(dp, dims).cpu(), pool(y, 2).bfloat16().float()).max()) <= 1.0
    assert float(dp.t[..., C:].abs().max()) == 0.0 and dp.acc is None
    odd = ops.to_cl(torch.randn((1, 32) + ((2, 5, 4) if dims == 3 else (5, 4)), generator=gen).to(dev))
    with pytest.raises(RuntimeError, match="gg_status -3"):
        ops.resample2x(odd, False, dims == 3)
