"""CPU suite of the first stage's held-out objective (jointimagegeneration_amd/aeloss.py, csrc/gg_patchgan.hip, ae_eval): the fp64
restatement (tests/aeloss_ref.py) against the reference's recorded values (tests/golden/aeloss.npz, make_golden_aeloss.py), the state_dict
surfaces, every refusal, the host-side argument checks of the new C-ABI functions and ae_eval's argument errors.  Nothing here launches."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aeloss_ref as A  # noqa: E402
from util import AE_SMALL, GOLD, surface  # noqa: E402

REF = os.environ.get("GG_REFERENCE", "/root/reference")
SLACK = 1 + 1e-6            # the fp64 restatement may reassociate between machines: parts in 1e15 against recorded distances of parts in 1e8
LOSS = "ldm.modules.losses.LPIPSWithDiscriminator"


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "aeloss.npz")))


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLD, "aeloss_surface.json")) as f:
        return json.load(f)


def disc_sd(meta, dims, which, nl):
    interm = dims == 3 or which == "ct"
    return A.seeded_disc_state_dict(3 if which == "ct" else 2, 1, nl, interm, 1000 * dims + 100 * (which == "ct") + nl,
                                    meta["gains"][f"dims{dims}_{which}_layers{nl}"])


def frames(t, dims):
    n = t.shape[0] * t.shape[1]
    t = t.reshape((n, 1) + tuple(t.shape[2:]))
    return t.reshape((-1, 1) + tuple(t.shape[3:])) if dims == 3 else t


# ------------------------------------------------------------------------------------------------ restatement against the recording
def test_restatement_reproduces_every_recorded_dict_value(gold, meta):
    lins = [gold[f"lin{k}"] for k in range(5)]
    p64 = {}
    for case in meta["cases"]:
        dims, cfg, name = case["dims"], case["cfg"], case["name"]
        x, y, mom = (torch.from_numpy(gold[f"{k}{dims}"]).double() for k in ("x", "y", "mom"))
        if dims not in p64:
            p64[dims] = A.lpips_images64(frames(x, dims), frames(y, dims), lins)
            assert np.abs(p64[dims].numpy() - gold[f"p{dims}_f64"]).max() <= 1e-12 * np.abs(gold[f"p{dims}_f64"]).max()
        nl = cfg["disc_num_layers"]
        d0, d1, _ = A.loss_dicts(dict(cfg, dims=dims), x, y, mom, p64[dims] if cfg["perceptual_weight"] > 0 else None,
                                 disc_sd(meta, dims, "frame", nl), disc_sd(meta, dims, "ct", nl) if dims == 3 else None, case["step"])
        assert list(d0) == case["keys0"] and list(d1) == case["keys1"]
        for tag, d in (("0", d0), ("1", d1)):
            for (k, v), ref in zip(d.items(), gold[f"{name}_ref{tag}"]):
                kind = A.KEY_KIND[k.split("/")[1]]
                want = float(v)
                if kind == "exact":
                    assert np.float32(want) == ref, (name, k)
                else:
                    dist = abs(float(ref) - want) / abs(want) if want else abs(float(ref))
                    assert dist <= float(gold[f"tol_{kind}"]) * SLACK, (name, k, dist)


def test_restatement_reproduces_posterior_and_block_samples(gold, meta):
    for dims in (2, 3):
        mom, noise = torch.from_numpy(gold[f"mom{dims}"]).double(), torch.from_numpy(gold[f"noise{dims}"]).double()
        assert float((mom[:, 4:] < -30).sum()) >= 1 and float((mom[:, 4:] > 20).sum()) >= 1          # both clamp edges occur
        z = A.gauss_sample(mom, noise).numpy()
        assert np.abs(gold[f"z{dims}"] - z).max() / np.abs(z).max() <= float(gold["tol_sample"]) * SLACK
        kl = A.gauss_kl(mom).sum().item()
        assert abs(float(gold[f"kl{dims}"].astype(np.float64).sum()) - kl) / kl <= float(gold["tol_kl"]) * SLACK
    for key in [k[:-len("_logits")] for k in gold if k.endswith("_logits")]:
        dims, which, nl = int(key[4]), key.split("_")[1], int(key[-1])
        y = frames(torch.from_numpy(gold[f"y{dims}"]).double(), dims if which == "frame" else 2)
        interm = dims == 3 or which == "ct"
        outs = A.disc_forward(y, disc_sd(meta, dims, which, nl), nl, interm)
        tol = float(gold["tol_block"]) * SLACK
        assert np.abs(gold[f"{key}_logits"] - outs[-1].numpy()).max() / np.abs(outs[-1].numpy()).max() <= tol
        l = gold[f"{key}_logits"].reshape(-1)
        assert min((l < -1).mean(), (np.abs(l) <= 1).mean(), (l > 1).mean()) >= 0.05          # the hinge switches both ways
        for i, o in enumerate(outs if interm else []):
            rec = gold[f"{key}_block{i}"]
            flat = o.reshape(-1).numpy()
            got = flat[::max(1, flat.size // 2048)]
            assert got.shape == rec.shape and np.abs(rec - got).max() / np.abs(flat).max() <= tol, (key, i)


# ------------------------------------------------------------------------------------------------ surfaces
@pytest.mark.parametrize("dims,nl", [(2, 3), (2, 2), (3, 3), (3, 2)])
def test_loss_surface_equals_the_reference(meta, dims, nl):
    from jointimagegeneration_amd.aeloss import LPIPSWithDiscriminator
    with torch.device("meta"):
        m = LPIPSWithDiscriminator(disc_start=5, disc_in_channels=1, disc_num_layers=nl, gan_feat_weight=0.0, dims=dims)
    assert surface(m) == meta["surfaces"][f"dims{dims}_layers{nl}"]


def test_discriminator_classes_keep_the_reference_names():
    from jointimagegeneration_amd.aeloss import NLayerDiscriminator, NLayerDiscriminator3D
    d = NLayerDiscriminator(1, getIntermFeat=False)
    assert [k for k, _ in surface(d)][:4] == ["model.0.weight", "model.0.bias", "model.2.weight", "model.2.bias"]
    assert dict((k, s) for k, s in surface(d))["model.11.weight"] == [1, 512, 4, 4]
    d3 = NLayerDiscriminator3D(1, n_layers=2)
    assert [k for k, _ in surface(d3)][-2:] == ["model3.0.weight", "model3.0.bias"] and tuple(d3.model1.get_submodule("0").weight.shape) == (128, 64, 4, 4, 4)
    for kw in (dict(use_actnorm=True), dict(use_sigmoid=True)):
        with pytest.raises(NotImplementedError, match=list(kw)[0]):
            NLayerDiscriminator(1, **kw)
    with pytest.raises(NotImplementedError, match="training mode"):
        NLayerDiscriminator(1).train()(torch.zeros(1, 1, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        NLayerDiscriminator3D(1).eval()(torch.zeros(1, 1, 4, 16, 16))


def ae(lossconfig, dims=2, **dd):
    from jointimagegeneration_amd.ldm import AutoencoderKL
    return AutoencoderKL(ddconfig=dict(AE_SMALL, dims=dims, **dd), lossconfig=lossconfig, embed_dim=4, dims=dims)


def test_identity_or_absent_lossconfig_is_unchanged():
    plain = surface(ae(None))
    for cfg in (None, dict(target="torch.nn.Identity"), dict(target="some.other.Loss", params=dict(a=1))):
        m = ae(cfg)
        assert type(m.loss) is torch.nn.Identity and surface(m) == plain and not any(k.startswith("loss.") for k, _ in plain)
    assert m.global_step == 0


def test_lossconfig_builds_the_loss_after_the_decoder(meta):
    from jointimagegeneration_amd.aeloss import LPIPSWithDiscriminator
    from jointimagegeneration_amd.config import TARGET_ALIASES
    for target in (LOSS, "ldm.modules.losses.contperceptual.LPIPSWithDiscriminator"):
        assert TARGET_ALIASES[target] == "jointimagegeneration_amd.aeloss.LPIPSWithDiscriminator"
        m = ae(dict(target=target, params=dict(disc_start=5, disc_in_channels=1, gan_feat_weight=0)))
        assert isinstance(m.loss, LPIPSWithDiscriminator)
        assert [n for n, _ in m.named_children()][:3] == ["encoder", "decoder", "loss"]
        assert [[k[5:], s] for k, s in surface(m) if k.startswith("loss.")] == meta["surfaces"]["dims2_layers3"]


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is only present in the build container")
def test_shipped_autoencoder_yaml_builds_unedited_with_the_loss_surface(meta):
    from jointimagegeneration_amd.config import instantiate_from_config, load_yaml
    cfg = load_yaml(os.path.join(REF, "latentdiffusion", "configs", "autoencoder", "ruijin-pimage_and_mask_autoencoder_kl.yaml"))
    with torch.device("meta"):
        m = instantiate_from_config(cfg["model"])
    assert [[k[5:], s] for k, s in surface(m) if k.startswith("loss.")] == meta["surfaces"]["dims2_layers3"]
    assert m.loss.kl_weight == 1e-6 and m.loss.discriminator_iter_start == 50001 and m.loss.gan_feat_weight == 0 and m.image_key == "mask"


# ------------------------------------------------------------------------------------------------ refusals, by name
class FakePosterior:
    parameters = torch.zeros(1, 8, 4, 4)


def test_loss_refusals():
    from jointimagegeneration_amd.aeloss import LPIPSWithDiscriminator as L
    for kw, pat in ((dict(use_actnorm=True), "use_actnorm"), (dict(disc_conditional=True), "disc_conditional")):
        with pytest.raises(NotImplementedError, match=pat):
            L(disc_start=1, **kw)
    with pytest.raises(ValueError, match="disc_loss"):
        L(disc_start=1, disc_loss="wasserstein")
    x2, x3 = torch.zeros(1, 1, 16, 16), torch.zeros(1, 1, 4, 16, 16)
    m = L(disc_start=1, disc_in_channels=1)
    assert m.training
    with pytest.raises(NotImplementedError, match="training mode"):
        m(x2, x2, FakePosterior(), 0, 0)
    m.eval()
    with pytest.raises(NotImplementedError, match="cond"):
        m(x2, x2, FakePosterior(), 0, 0, cond=x2)
    with pytest.raises(NotImplementedError, match="weights"):
        m(x2, x2, FakePosterior(), 0, 0, weights=x2)
    with pytest.raises(ValueError, match="not match"):
        m(x2, x3, FakePosterior(), 0, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x2, x2, FakePosterior(), 0, 0)
    for kw, pat in ((dict(gan_feat_weight=1.0), "gan_feat_weight"), (dict(gan_feat_weight=0, image_gan_weight=0.0), "image_gan_weight"),
                    (dict(gan_feat_weight=0, ct_gan_weight=0.0), "ct_gan_weight")):
        m3 = L(disc_start=1, disc_in_channels=1, dims=3, **kw).eval()
        with pytest.raises(NotImplementedError, match=pat):
            m3(x3, x3, FakePosterior(), 0, 0)
    with pytest.raises(ValueError, match="built with dims = 2"):
        L(disc_start=1, disc_in_channels=1, gan_feat_weight=0).eval()(x3, x3, FakePosterior(), 0, 0)
    m3 = L(disc_start=1, disc_in_channels=1, dims=3, gan_feat_weight=1.0).eval()
    assert m3.gan_feat_weight == 1.0 and L(disc_start=1, dims=2, gan_feat_weight=1.0).gan_feat_weight == 1.0      # accepted at construction; 2-D ignores it


def test_zero_vgg_weights_are_refused_when_the_perceptual_term_is_on():
    from jointimagegeneration_amd.aeloss import LPIPSWithDiscriminator as L
    m = L(disc_start=1, disc_in_channels=1).eval()
    with pytest.raises(RuntimeError, match="VGG16 weights are still the constructor's zeros"):
        m._check_vgg()
    m.perceptual_loss.net.slice1.get_submodule("0").weight.data.fill_(0.5)
    m._check_vgg()
    L(disc_start=1, perceptual_weight=0.0)            # nothing to check when the term is off


def test_autoencoder_refusals_and_get_input():
    m = ae(None).eval()
    with pytest.raises(NotImplementedError, match="loss is nn.Identity"):
        m.validation_losses(torch.zeros(1, 1, 32, 32))
    m = ae(dict(target=LOSS, params=dict(disc_start=1, disc_in_channels=1)))
    m.train()
    with pytest.raises(NotImplementedError, match="training mode"):
        m.validation_losses(torch.zeros(1, 1, 32, 32))
    m.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.validation_losses(torch.zeros(1, 1, 32, 32))
    with pytest.raises(NotImplementedError, match="conditional"):
        from jointimagegeneration_amd.ldm import AutoencoderKL
        AutoencoderKL(ddconfig=dict(AE_SMALL), lossconfig=None, embed_dim=4, dims=2, conditional=True, cond_key="x")
    b = dict(image=torch.arange(2 * 4 * 6 * 3, dtype=torch.float64).reshape(2, 4, 6, 3), flat=torch.zeros(2, 4, 6))
    assert tuple(m.get_input(b, "image").shape) == (2, 3, 4, 6) and m.get_input(b, "image").dtype == torch.float32
    assert torch.equal(m.get_input(b, "image")[1, 2], b["image"][1, :, :, 2].float()) and tuple(m.get_input(b, "flat").shape) == (2, 1, 4, 6)
    assert m.latent_shape((3, 1, 32, 36)) == (3, 4, 8, 9)
    m3 = ae(None, dims=3)
    assert tuple(m3.get_input(dict(v=torch.zeros(2, 4, 6, 8)), "v").shape) == (2, 1, 4, 6, 8)


def test_posterior_kl_refusals_and_cpu_sample():
    from jointimagegeneration_amd.ldm import DiagonalGaussianDistribution
    p = DiagonalGaussianDistribution(torch.zeros(2, 8, 4, 4))
    with pytest.raises(NotImplementedError, match=r"kl\(other\)"):
        p.kl(p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        p.kl()
    assert not hasattr(p, "nll")
    e = torch.randn(2, 4, 4, 4)
    assert torch.equal(p.sample(e), e) and tuple(p.sample().shape) == (2, 4, 4, 4)           # host tensors keep the torch path


# ------------------------------------------------------------------------------------------------ C-ABI: host-side argument checks
@pytest.fixture(scope="module")
def lib():
    from util import load_lib
    return load_lib()


def test_new_entry_points_reject_bad_arguments_on_the_host(lib):
    P = 0x1000                                            # a non-null pointer that is never dereferenced: every call below fails before a launch
    BAD_SHAPE, BAD_DTYPE, UNSUPPORTED, WS = -1, -2, -3, -4

    def conv(src=P, w=P, alpha=None, beta=P, N=1, D=1, H=16, W=20, cin=32, cout=64, kd=1, stride=2, Do=1, Ho=9, Wo=11, out=P, dt=0):
        return lib.gg_patch_conv_forward(src, w, alpha, beta, 0.2, N, D, H, W, cin, cout, kd, stride, Do, Ho, Wo, out, dt, None)

    def conv32(src=P, beta=P, cin=32, stride=2, Ho=9, kd=1, Do=1):
        return lib.gg_patch_conv_forward_f32(src, P, None, beta, 0.2, 1, 1, 16, 20, cin, 64, kd, stride, Do, Ho, 11, P, None)

    assert conv(cin=48) == BAD_SHAPE and b"multiple of 32" in lib.gg_last_error()
    assert conv(stride=3) == UNSUPPORTED and b"stride" in lib.gg_last_error()
    assert conv(Ho=8) == BAD_SHAPE and b"output extent" in lib.gg_last_error()
    assert conv(kd=4, D=4, Do=2) == BAD_SHAPE and conv(kd=3) == UNSUPPORTED                  # 4 / 2 + 1 = 3 slices, not 2
    assert conv(stride=1, Ho=17, Wo=21, H=0) == BAD_SHAPE
    for kw in (dict(src=None), dict(w=None), dict(beta=None), dict(out=None)):
        assert conv(**kw) == BAD_SHAPE and b"null pointer" in lib.gg_last_error()
    assert conv(dt=7) == BAD_DTYPE
    assert conv(N=1 << 20, H=2047, W=2047, Ho=1024, Wo=1024) == UNSUPPORTED and b"32-bit" in lib.gg_last_error()
    assert conv32(cin=16) == BAD_SHAPE and conv32(stride=3) == UNSUPPORTED and conv32(Ho=10) == BAD_SHAPE
    assert conv32(src=None) == BAD_SHAPE and conv32(beta=None) == BAD_SHAPE and conv32(kd=2) == UNSUPPORTED
    # reductions: null pointers, strides, workspace
    need = lib.gg_loss_workspace_bytes(3, 4096)
    assert need == 3 * 16 * 2 * 8
    assert lib.gg_gauss_kl_rows(None, 32, 3, 4, 4096, P, P, need, None) == BAD_SHAPE and b"null pointer" in lib.gg_last_error()
    assert lib.gg_gauss_kl_rows(P, 7, 3, 4, 4096, P, P, need, None) == BAD_SHAPE and b"stride" in lib.gg_last_error()
    assert lib.gg_gauss_kl_rows(P, 32, 3, 4, 4096, P, P, 3 * 16 * 8 - 1, None) == WS
    assert lib.gg_gauss_kl_rows(P, 32, 0, 4, 4096, P, P, need, None) == BAD_SHAPE
    assert lib.gg_gauss_sample_rows(P, 32, None, 3, 4, 35, P, None, 0, 0, None) == BAD_SHAPE
    assert lib.gg_gauss_sample_rows(P, 32, P, 3, 4, 35, None, None, 0, 0, None) == BAD_SHAPE and b"no output" in lib.gg_last_error()
    assert lib.gg_gauss_sample_rows(P, 32, P, 3, 4, 35, None, P, 0, 3, None) == BAD_SHAPE
    assert lib.gg_gauss_sample_rows(P, 32, P, 3, 4, 35, None, P, 5, 32, None) == BAD_DTYPE
    assert lib.gg_logit_stats(None, 32, 100, P, P, 4096, None) == BAD_SHAPE
    assert lib.gg_logit_stats(P, 32, 0, P, P, 4096, None) == BAD_SHAPE
    assert lib.gg_logit_stats(P, 32, 1000, P, P, 4 * 5 * 8 - 1, None) == WS and b"workspace" in lib.gg_last_error()


def test_ops_wrappers_refuse_host_tensors():
    from jointimagegeneration_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gauss_kl_rows(torch.zeros(1, 4, 4, 32), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.logit_stats(torch.zeros(1, 4, 4, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.patch_conv(ops.CL(torch.zeros(1, 1, 16, 16, 32, dtype=torch.bfloat16), 1), torch.zeros(1), None, torch.zeros(64), 64, 1, 2)
    assert ops.patch_conv_out_extent((1, 16, 20), 1, 2) == (1, 9, 11) and ops.patch_conv_out_extent((4, 17, 21), 4, 2) == (3, 9, 11)
    assert ops.patch_conv_out_extent((2, 3, 4), 4, 1) == (3, 4, 5)


# ------------------------------------------------------------------------------------------------ ae_eval: argument errors
def test_ae_eval_argument_errors(tmp_path):
    import yaml
    from jointimagegeneration_amd import ae_eval
    from jointimagegeneration_amd.io import write_nifti
    base = ["--config", str(tmp_path / "ae.yaml"), "--ckpt", str(tmp_path / "ae.ckpt"), "--ct", str(tmp_path / "ct"), "--out", str(tmp_path / "m.json")]
    with pytest.raises(SystemExit):
        ae_eval.main(["--config", "x"])
    with pytest.raises(ValueError, match="--every"):
        ae_eval.main(base + ["--every", "0"])
    with pytest.raises(ValueError, match="go together"):
        ae_eval.main(base + ["--lpips-vgg", "v.pth"])
    with pytest.raises(FileNotFoundError, match="not a file"):
        ae_eval.main(base)
    params = dict(embed_dim=4, dims=2, image_key="mask", ddconfig=dict(AE_SMALL, in_channels=2, out_ch=2),
                  lossconfig=dict(target="torch.nn.Identity"))
    (tmp_path / "ae.yaml").write_text(yaml.safe_dump(dict(model=dict(target="ldm.models.autoencoder.AutoencoderKL", params=params))))
    torch.save(dict(state_dict={}), tmp_path / "ae.ckpt")
    with pytest.raises(FileNotFoundError, match="no \\*.nii"):
        ae_eval.main(base)
    (tmp_path / "ct").mkdir()
    write_nifti(str(tmp_path / "ct" / "v0.nii.gz"), np.zeros((4, 32, 32), dtype=np.float32))
    with pytest.raises(ValueError, match="names no objective"):
        ae_eval.main(base)
    params["lossconfig"] = dict(target=LOSS, params=dict(disc_start=3, disc_in_channels=1, gan_feat_weight=0))
    (tmp_path / "ae.yaml").write_text(yaml.safe_dump(dict(model=dict(target="ldm.models.autoencoder.AutoencoderKL", params=params))))
    with pytest.raises(KeyError, match="missing keys"):
        ae_eval.main(base)
    from jointimagegeneration_amd.config import instantiate_from_config
    m = instantiate_from_config(dict(target="ldm.models.autoencoder.AutoencoderKL", params=params))
    torch.save(dict(state_dict={k: v for k, v in m.state_dict().items() if not k.startswith("loss.perceptual_loss.")}, global_step=7), tmp_path / "ae.ckpt")
    with pytest.raises(KeyError, match="--lpips-vgg"):
        ae_eval.main(base)
    torch.save(dict(state_dict=m.state_dict(), global_step=7), tmp_path / "ae.ckpt")
    with pytest.raises(ValueError, match="--seg"):
        ae_eval.main(base)
    # the inputs of one volume: 'image' slices, 'mask' = [previous CT slice (zeros first), label slice], every K-th
    ct, seg = np.arange(4 * 2 * 3, dtype=np.float32).reshape(4, 2, 3), -np.arange(4 * 2 * 3, dtype=np.float32).reshape(4, 2, 3)
    b = ae_eval.batches(ct, seg, "mask", 2, 2)
    assert len(b) == 2 and tuple(b[1].shape) == (1, 2, 2, 3) and float(b[0][0, 0].abs().max()) == 0
    assert np.array_equal(b[1][0, 0].numpy(), ct[1]) and np.array_equal(b[1][0, 1].numpy(), seg[2])
    assert [tuple(t.shape) for t in ae_eval.batches(ct, None, "image", 2, 3)] == [(1, 1, 2, 3)] * 2
    assert tuple(ae_eval.batches(ct, None, "image", 3, 1)[0].shape) == (1, 1, 4, 2, 3)
