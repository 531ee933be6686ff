"""GPU suite (-m gpu): every ops.* kernel call of the text, 3-D, GAN and LPIPS networks, at the shape, stride and offset the network
itself passes, against the fp64 reference of that call (tests/shadow.py): TransformerEmbedder / BERTEmbedder, FrozenBERTEmbedder's
BertModel under per-sample key lengths, SpatialRescaler, the volumetric AutoencoderKL / VQModel, the PatchGAN discriminators and the
three-view LPIPS.

Eager runs on the bf16 path, inside shadow_ops(), on the small configs and seeded weights the networks' own test files build.  Each
test asserts that every shadowed call is inside its bound (a `contract` record, ratio inf, fails the same way), that the families and
plans it is meant to cover did occur, and prints one line per op family: worst err / bound, calls, plans."""
import json
import os

import pytest
import torch

import bert_ref
import lpips_ref
from shadow import shadow_ops
from test_aeloss_cpu import disc_sd
from test_bert_cpu import tiny_cfg
from test_cond_cpu import embedder
from util import GOLD, T, gold, seeded

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
LOSS = dict(target="torch.nn.Identity")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def report(sh, title, N):
    print()
    print(sh.summary(f"{title} N={N}"))
    sh.assert_within_bounds(N)
    return {r.family for r in sh.records}


def plans(sh, family):
    return [dict(r.plan) for r in sh.records if r.family == family]


# ------------------------------------------------------------------------------------------------ text
@pytest.mark.parametrize("name", ["te", "bert"])
def test_token_embedders(dev, name):
    """TransformerEmbedder and BERTEmbedder (width 48: padded rows, so gg_layernorm_rows; q, k and v read out of one packed projection)
    on the cond fixture's [2, 20] tokens, 20 being max_seq_len."""
    from jointimagegeneration_amd import ops
    m, _ = embedder(name)
    m = m.to(dev)
    tok = T(gold("cond")[f"{name}_2x20_tokens"]).to(dev)
    with shadow_ops() as sh:
        ops.invalidate_caches(m)
        z = m.encode(tok)
        torch.cuda.synchronize()
    fams = report(sh, name, 2)
    assert tuple(z.shape) == (2, 20, 48)
    assert {"embed_rows", "attention", "conv"} <= fams and fams & {"layernorm", "layernorm_rows"} and fams & {"gelu", "geglu"}
    assert "layernorm_rows" in fams, "width 48 no longer runs on gg_layernorm_rows"
    assert any(p["residual"] for p in plans(sh, "conv"))


def bert_model(cfg, prefix, dev):
    from jointimagegeneration_amd import cond
    m = cond.BertModel(cfg)
    m.load_state_dict(bert_ref.seeded_state_dict(cfg, prefix))
    return m.eval().to(dev)


def run_bert(m, cfg, lengths, T_len, seed):
    from jointimagegeneration_amd import ops
    N = len(lengths)
    ids = torch.randint(0, cfg["vocab_size"], (N, T_len), generator=gen(seed)).int()
    ids[0, 0], ids[-1, 1 % T_len] = cfg["vocab_size"] - 1, 0
    with shadow_ops() as sh:
        ops.invalidate_caches(m)
        out = m.run(ids.to(m.embeddings.word_embeddings.weight.device), lengths, ids_host=ids.contiguous())
        torch.cuda.synchronize()
    fams = report(sh, f"BertModel {cfg['hidden_size']} lengths {lengths}", N)
    assert tuple(out.shape) == (N, T_len, cfg["hidden_size"]) and bool(torch.isfinite(out).all())
    assert {"bert_embed", "attention", "attention.kvlen", "conv", "gelu"} <= fams
    assert any(p["residual"] for p in plans(sh, "conv")), "no conv with a residual in the plan"
    kv = plans(sh, "attention.kvlen")
    assert len(kv) == cfg["num_hidden_layers"] and all(p["kvlen"] and p["lengths"] == tuple(lengths) for p in kv)
    assert all(p["kvlen"] for p in plans(sh, "attention"))
    return sh


@pytest.mark.parametrize("lengths", [[16, 1], [3, 16]], ids=lambda v: "-".join(map(str, v)))
def test_bert_tiny_key_lengths(dev, lengths):
    """2 layers x 64 (2 heads of 32), T = 16; length 1 is the clamp's edge."""
    cfg = tiny_cfg()
    run_bert(bert_model(cfg, "bert_tiny.", dev), cfg, lengths, 16, 5)


@pytest.fixture(scope="module")
def bert_base2(dev):
    cfg = dict(bert_ref.BASE, num_hidden_layers=2)
    return cfg, bert_model(cfg, "bert_base.", dev)


@pytest.mark.parametrize("lengths", [[128, 37], [5, 128, 64]], ids=lambda v: "-".join(map(str, v)))
def test_bert_base_width_key_lengths(dev, bert_base2, lengths):
    """bert_ref.BASE cut to 2 layers: 768 wide, 12 heads of 64 at packed q / k / v offsets 0 / 768 / 1536, T = 128.  With three samples
    of three lengths a sample that attended to a neighbour's key length cannot pass."""
    cfg, m = bert_base2
    run_bert(m, cfg, lengths, 128, 12)


# ------------------------------------------------------------------------------------------------ SpatialRescaler
@pytest.mark.parametrize("multiplier", [0.5, 2])
@pytest.mark.parametrize("n_stages", [1, 2])
@pytest.mark.parametrize("method", ["nearest", "bilinear", "bicubic", "area"])
def test_spatial_rescaler(dev, method, n_stages, multiplier):
    """[2, 3, 17, 20] (odd and even extents) through n_stages interpolations and the 1x1 channel mapper (3 -> 5, with bias)."""
    from jointimagegeneration_amd import cond, ops
    m = seeded(cond.SpatialRescaler(n_stages=n_stages, method=method, multiplier=multiplier, in_channels=3, out_channels=5, bias=True),
               f"cond_rs_{method}_b1.").to(dev)
    x = torch.randn(2, 3, 17, 20, generator=gen(31)).to(dev)
    with shadow_ops() as sh:
        ops.invalidate_caches(m)
        y = m.encode(x)
        torch.cuda.synchronize()
    fams = report(sh, f"SpatialRescaler {method} x{multiplier} stages={n_stages}", 2)
    ext = lambda n: ops.interpolate_extent(ops.interpolate_extent(n, multiplier), multiplier) if n_stages == 2 else ops.interpolate_extent(n, multiplier)
    assert tuple(y.shape) == (2, 5, ext(17), ext(20))
    assert {"interpolate2d", "conv"} <= fams and len(plans(sh, "interpolate2d")) == n_stages
    assert all(p["mode"] == method and p["scale_factor"] == multiplier for p in plans(sh, "interpolate2d"))


# ------------------------------------------------------------------------------------------------ 3-D first stage
with open(os.path.join(GOLD, "ae3d_surface.json")) as _f:
    META3D = json.load(_f)
AE3D = META3D["ae3d"]
assert min(AE3D["attn_resolutions"]) * 2 ** (len(AE3D["ch_mult"]) - 1) == AE3D["resolution"], "AE3D no longer has attention at its lowest level"
GN_FAMILIES = {"groupnorm.apply", "groupnorm.coeffs", "conv.stats"}


def volumes(N, dev):
    """The fixture volume [1, 1, 6, 8, 10] and, at N = 2, a second one with other content (mirrored, rescaled, shifted)."""
    img = T(gold("ae3d")["img"])
    if N == 2:
        img = torch.cat([img, 0.8 * img.flip(-1).flip(-2) - 0.1])
    return img.to(dev)


def check_first_stage(sh, fams, quantised):
    convs = [(r.shape, dict(r.plan)) for r in sh.records if r.family == "conv"]
    assert any(s[6:] == (3, 3, 3) and p["stride"] == 2 for s, p in convs), "no stride-2 3x3x3 conv (Downsample over D, H and W)"
    assert any(s[6:] == (3, 3, 3) and p["upsample"] for s, p in convs), "no x2-upsample 3x3x3 conv"
    att = [r for r in sh.records if r.family == "attention"]
    assert att and all(r.shape[3] == r.shape[4] and r.shape[3] > 1 for r in att), "AttnBlock's attention over D*H*W tokens did not occur"
    assert fams & GN_FAMILIES, "no GroupNorm family was recorded"
    assert ("vq_nearest" in fams) == quantised


@pytest.mark.parametrize("N", [1, 2])
def test_autoencoder_kl_3d(dev, N):
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.ldm import AutoencoderKL
    m = seeded(AutoencoderKL(ddconfig=dict(AE3D), lossconfig=LOSS, embed_dim=4, dims=3), "ae3d_kl.").to(dev)
    img = volumes(N, dev)
    with shadow_ops() as sh:
        ops.invalidate_caches(m)
        z = m.encode(img).mode()
        dec = m.decode(z)
        torch.cuda.synchronize()
    fams = report(sh, "AutoencoderKL(dims=3)", N)
    assert tuple(z.shape) == (N, 4, 3, 4, 5) and tuple(dec.shape) == tuple(img.shape)
    check_first_stage(sh, fams, False)


@pytest.mark.parametrize("N", [1, 2])
def test_vq_model_3d(dev, N):
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.ldm import VQModel
    m = seeded(VQModel(ddconfig=dict(AE3D), lossconfig=LOSS, n_embed=META3D["n_embed"], embed_dim=4, dims=3), "ae3d_vq.")
    m.quantize.embedding.weight.mul_(META3D["code_scale"])
    m = m.to(dev)
    img = volumes(N, dev)
    with shadow_ops() as sh:
        ops.invalidate_caches(m)
        quant = m.encode(img)[0]
        dec = m.decode(quant)
        torch.cuda.synchronize()
    fams = report(sh, "VQModel(dims=3)", N)
    assert tuple(quant.shape) == (N, 4, 3, 4, 5) and tuple(dec.shape) == tuple(img.shape)
    check_first_stage(sh, fams, True)
    for p in plans(sh, "vq_nearest"):
        print(f"VQModel(dims=3) N={N}: near-tie share {p['near_tie_share']:.4f}")


# ------------------------------------------------------------------------------------------------ PatchGAN discriminators
@pytest.mark.parametrize("dims, nl", [(2, 2), (2, 3), (3, 3)])
def test_patchgan_discriminators(dev, dims, nl):
    """NLayerDiscriminator (2-D, [2, 1, 17, 20]) and NLayerDiscriminator3D ([2, 1, 9, 17, 20]) on the bf16 path: kernel-4 padding-2 convs
    at strides 2 and 1 over odd extents, folded BatchNorm, the fp32 logits."""
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.aeloss import NLayerDiscriminator, NLayerDiscriminator3D
    with open(os.path.join(GOLD, "aeloss_surface.json")) as f:
        meta = json.load(f)
    which = "ct" if dims == 3 else "frame"
    disc = (NLayerDiscriminator3D if dims == 3 else NLayerDiscriminator)(1, n_layers=nl, getIntermFeat=dims == 3).eval()
    disc.load_state_dict(disc_sd(meta, dims, which, nl))
    disc = disc.to(dev)
    x = torch.randn((2, 1) + ((9, 17, 20) if dims == 3 else (17, 20)), generator=gen(40 + dims)).to(dev)
    with shadow_ops() as sh:
        ops.invalidate_caches(disc)
        out = disc(x)
        torch.cuda.synchronize()
    fams = report(sh, f"NLayerDiscriminator{'3D' if dims == 3 else ''} n_layers={nl}", 2)
    logits = out[0] if dims == 3 else out
    assert bool(torch.isfinite(logits).all())
    pc = plans(sh, "patch_conv")
    assert fams == {"patch_conv"} and len(pc) == nl + 2
    assert {p["stride"] for p in pc} == {1, 2} and {p["kd"] for p in pc} == {4 if dims == 3 else 1}
    assert [p["out_f32"] for p in pc] == [0] * (nl + 1) + [1] and any(p["alpha"] for p in pc) and not pc[0]["alpha"]


# ------------------------------------------------------------------------------------------------ LPIPS
@pytest.fixture(scope="module")
def lpips_model(dev, tmp_path_factory):
    from jointimagegeneration_amd.lpips import LPIPS
    g = gold("lpips")
    d = tmp_path_factory.mktemp("lpips_weights")
    torch.save(lpips_ref.seeded_vgg_state_dict(), d / "vgg.pth")
    torch.save({f"lin{k}.model.1.weight": T(g[f"lin{k}"]).reshape(1, -1, 1, 1) for k in range(5)}, d / "lin.pth")
    return LPIPS.load(str(d / "vgg.pth"), str(d / "lin.pth")).to(dev)


def test_lpips_three_views_and_images(dev, lpips_model):
    """The lpips.npz volumes cut to 16 x 17 x 18 (three unequal extents, the smallest the fourth max-pool allows), three of them under
    batch_per_segment = 2 (a last segment of one volume) and 12 images per chunk (a partial last chunk in every view), then the
    3-channel images through LPIPS.forward.  The network cuts its batch itself, so no one batch size is required of the calls."""
    from jointimagegeneration_amd import lpips, ops
    g = gold("lpips")
    pred, gt = T(g["pred"])[..., :17, :18], T(g["gt"])[..., :17, :18]
    pred = torch.cat([pred, 0.5 * (pred[:1] + gt[1:])]).contiguous().to(dev)
    gt = torch.cat([gt, gt[:1]]).contiguous().to(dev)
    x4, y4 = T(g["x4"])[..., :17, :18].contiguous().to(dev), T(g["y4"])[..., :17, :18].contiguous().to(dev)
    m = lpips_model
    m.chunk_images = 12
    try:
        with shadow_ops() as sh:
            ops.invalidate_caches(m)
            score = lpips.lpips_3view(pred, gt, batch_per_segment=2, model=m)
            per_image = m(x4, y4)
            torch.cuda.synchronize()
    finally:
        m.chunk_images = None
    fams = report(sh, "LPIPS 3 views + 3-channel images", None)
    assert score > 0.0 and tuple(per_image.shape) == (2, 1, 1, 1)
    assert {"volume_views_cl", "conv", "relu_cl", "lpips_tap"} <= fams
    assert {p["view"] for p in plans(sh, "volume_views_cl")} == {0, 1, 2, 3}
    assert {p["pool"] for p in plans(sh, "lpips_tap")} == {0, 1} and {p["accumulate"] for p in plans(sh, "lpips_tap")} == {0, 1}
    sizes = {p["n1"] - p["n0"] for p in plans(sh, "volume_views_cl")}
    assert 12 in sizes and sizes - {12, 2}, f"no partial last chunk: chunk sizes {sorted(sizes)}"
