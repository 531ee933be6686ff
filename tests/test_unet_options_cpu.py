"""CPU suite: the UNet constructor options use_scale_shift_norm (FiLM), resblock_updown, use_new_attention_order and conv_resample=False
build in both UNets and in the blocks, with the reference's state_dict names and shapes for every option combination
(sha256 digests in tests/golden/unet_options_surfaces.json, captured from the reference constructors by make_golden_unet_options.py);
the options that stay out of scope still raise; option-bearing copies of the shipped YAML files build through the ddpm_eval / sample_diffusion paths."""
import hashlib
import itertools
import json
import os

import pytest
import torch
import yaml

from util import CCDM_SMALL, GOLD, LDM_SMALL

REF = os.environ.get("GG_REFERENCE", "/root/reference")
OPTIONS = ("use_scale_shift_norm", "resblock_updown", "use_new_attention_order", "conv_resample")
COMBOS = list(itertools.product((False, True), repeat=4))


def _surfaces():
    with open(os.path.join(GOLD, "unet_options_surfaces.json")) as f:
        return json.load(f)


def surface(m):
    """sha256 of [[name, shape], ...] as compact JSON, as the fixture generator digests the reference modules."""
    s = json.dumps([[k, list(v.shape)] for k, v in m.state_dict().items()], separators=(",", ":"))
    return hashlib.sha256(s.encode()).hexdigest()


def _opts(bits):
    return dict(zip(OPTIONS[:3], bits[:3]), conv_resample=not bits[3])


def _tag(bits):
    return "".join("1" if b else "0" for b in bits)


def _ccdm(**opts):
    from jointimagegeneration_amd.unet import CCDMUNetModel
    cfg = dict(CCDM_SMALL)
    base = cfg.pop("base_channels")
    return CCDMUNetModel(in_channels=7, model_channels=base, out_channels=6, num_res_blocks=2, cond_encoded_shape=None, dims=3, **cfg, **opts)


@pytest.mark.parametrize("bits", COMBOS, ids=[_tag(b) for b in COMBOS])
def test_unet_surfaces_match_the_reference_for_every_option_combination(bits):
    from jointimagegeneration_amd.unet import UNetModel
    surf = _surfaces()
    with torch.device("meta"):
        assert surface(_ccdm(**_opts(bits))) == surf[f"ccdm_{_tag(bits)}"]
        assert surface(UNetModel(**LDM_SMALL, **_opts(bits))) == surf[f"ldm_{_tag(bits)}"]


def test_option_networks_of_the_fixture_have_the_reference_surface():
    from jointimagegeneration_amd.unet import UNetModel
    surf = _surfaces()
    on = dict(use_scale_shift_norm=True, resblock_updown=True, use_new_attention_order=True)
    with torch.device("meta"):
        assert surface(_ccdm(**on)) == surf["ccdm_opt"]
        assert surface(_ccdm(conv_resample=False)) == surf["ccdm_nc"]
        u = UNetModel(**LDM_SMALL, **on)
    assert surface(u) == surf["ldm_opt"]
    # FiLM: emb_layers.1 projects to 2C; up / down ResBlocks between levels, h_upd / x_upd without parameters
    sd = u.state_dict()
    assert list(sd["input_blocks.1.0.emb_layers.1.weight"].shape) == [64, 128]
    rb = u.input_blocks[3][0]
    assert rb.down and not rb.up and not any(k.startswith("input_blocks.3.0.h_upd") or k.startswith("input_blocks.3.0.x_upd") for k in sd)


def test_blocks_construct_with_each_option_and_match_the_reference_surface():
    from jointimagegeneration_amd import blocks as B
    surf = _surfaces()
    with torch.device("meta"):
        built = {
            "rbf3a": B.ResBlock(64, 128, 0.0, out_channels=96, dims=3, use_scale_shift_norm=True),
            "rbf3b": B.ResBlock(64, 128, 0.0, out_channels=64, dims=3, use_scale_shift_norm=True),
            "rbf2a": B.ResBlock(64, 128, 0.0, out_channels=96, dims=2, use_scale_shift_norm=True),
            "rbf2b": B.ResBlock(64, 128, 0.0, out_channels=64, dims=2, use_scale_shift_norm=True),
            "rbd3": B.ResBlock(64, 128, 0.0, dims=3, down=True), "rbu3": B.ResBlock(64, 128, 0.0, dims=3, up=True),
            "rbdf3": B.ResBlock(64, 128, 0.0, dims=3, down=True, use_scale_shift_norm=True),
            "rbuf3": B.ResBlock(64, 128, 0.0, dims=3, up=True, use_scale_shift_norm=True),
            "rbd2": B.ResBlock(64, 128, 0.0, dims=2, down=True), "rbu2": B.ResBlock(64, 128, 0.0, dims=2, up=True),
            "abn3": B.AttentionBlock(64, num_head_channels=32, use_new_attention_order=True),
            "abn2": B.AttentionBlock(96, num_heads=-1, num_head_channels=32, use_new_attention_order=True),
            "rs3_up": B.Upsample(48, False, dims=3), "rs3_dn": B.Downsample(48, False, dims=3),
            "rs2_up": B.Upsample(48, False, dims=2), "rs2_dn": B.Downsample(48, False, dims=2),
        }
    for name, m in built.items():
        assert surface(m) == surf[name], name
    assert built["rbf3a"].time_bias_width == 2 * 96 and built["rbd3"].time_bias_width == 64


def test_out_of_scope_options_still_raise():
    from jointimagegeneration_amd.unet import UNetModel
    with torch.device("meta"):
        for kw in (dict(ce_head=True), dict(num_classes=3), dict(use_spatial_transformer=True, context_dim=8)):
            with pytest.raises(NotImplementedError, match="option outside the shipped CCDM configuration"):
                _ccdm(**kw)
        with pytest.raises(NotImplementedError, match="feature_cond_encoder"):
            _ccdm(feature_cond_encoder={"type": "dino"})
        for kw in (dict(num_classes=3), dict(n_embed=16)):
            with pytest.raises(NotImplementedError, match="option outside the shipped LDM configurations"):
                UNetModel(**LDM_SMALL, **kw)


@pytest.mark.skipif(not os.path.isdir(REF), reason="the shipped YAML files are only present in the build container")
def test_option_bearing_copies_of_the_shipped_yamls_build(tmp_path):
    from jointimagegeneration_amd import ddpm_eval
    from jointimagegeneration_amd.blocks import AttentionBlock, ResBlock
    from jointimagegeneration_amd.config import instantiate_from_config, load_yaml
    from jointimagegeneration_amd.sample_diffusion import strip_ckpt_paths
    on = dict(use_scale_shift_norm=True, resblock_updown=True, use_new_attention_order=True)

    def check(unet, C0):
        rbs = [m for m in unet.modules() if isinstance(m, ResBlock)]
        assert rbs and all(rb.use_scale_shift_norm for rb in rbs) and any(rb.down for rb in rbs) and any(rb.up for rb in rbs)
        assert all(a.new_order for a in unet.modules() if isinstance(a, AttentionBlock))
        assert unet.input_blocks[1][0].emb_layers[1].weight.shape[0] == 2 * C0

    with open(os.path.join(REF, "ccdm", "params_eval.yml")) as f:
        params = yaml.safe_load(f)
    params["unet_openai"].update(on)
    path = tmp_path / "params_eval.yml"
    path.write_text(yaml.safe_dump(params))
    with torch.device("meta"):
        model = ddpm_eval.build_from_params(yaml.safe_load(path.read_text()), (128, 128, 128), 14)
    check(model.unet, params["unet_openai"]["base_channels"])
    for name in ("ruijin-ldm_from_controlnet_ae.yaml", "ruijin-ldm_from_controlnet.yaml"):
        cfg = load_yaml(os.path.join(REF, "latentdiffusion", "configs", "latent-diffusion", name))
        cfg["model"]["params"]["unet_config"]["params"].update(on)
        path = tmp_path / name
        path.write_text(yaml.safe_dump(cfg))
        with torch.device("meta"):
            m = instantiate_from_config(strip_ckpt_paths(load_yaml(str(path)))["model"])
        check(m.model.diffusion_model, cfg["model"]["params"]["unet_config"]["params"]["model_channels"])


def test_pack_cache_misses_for_new_parameters_on_reused_storage():
    """Blocks built, run and freed one after another (as the option tests do) can hand a new module the freed module's id() and its
    parameters' storage at the same version counter: the repack cache must not return the freed module's repack."""
    from jointimagegeneration_amd.blocks import _Packed
    cache = _Packed()
    p = torch.nn.Parameter(torch.ones(4))
    assert cache.get(("conv", 1), [p, None], lambda: "old") == "old"
    assert cache.get(("conv", 1), [p, None], lambda: "rebuilt") == "old"
    q = torch.nn.Parameter(p.detach())                  # another tensor object on the same storage, same version
    assert q.data_ptr() == p.data_ptr() and q._version == p._version
    assert cache.get(("conv", 1), [q], lambda: "new") == "new"
