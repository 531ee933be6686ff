"""CPU suite for the VQ first stage and quantised sampling: the state-dict surface of VQModelInterface against the reference's
(tests/golden/vq_surface.json, make_golden_vq.py), config instantiation through the reference's dotted paths, the options that stay refused,
host-side validation before any launch, the C-ABI of the two new entries, and the torch restatement of the quantiser (tests/vq_ref.py)
against a hand-computed case."""
import ctypes as C
import json
import os
import re

import pytest
import torch

import vq_ref
from util import AE_SMALL, GOLD, LDM_SMALL, small_ldm, surface

LOSS = dict(target="torch.nn.Identity")


def vq_cfg(target="ldm.models.autoencoder.VQModelInterface", **kw):
    return dict(target=target, params=dict(dict(embed_dim=4, n_embed=64, dims=2, ddconfig=dict(AE_SMALL), lossconfig=LOSS), **kw))


def vq_ldm(first_stage):
    from jointimagegeneration_amd.ldm import LatentDiffusion
    ae2 = dict(target="ldm.models.autoencoder.AutoencoderKL", params=dict(embed_dim=4, dims=2, ddconfig=dict(AE_SMALL, in_channels=2, out_ch=2), lossconfig=LOSS))
    return LatentDiffusion(first_stage_config=first_stage, cond_stage_config=ae2,
                           unet_config=dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(LDM_SMALL)),
                           linear_start=0.0015, linear_end=0.0195, timesteps=1000, image_size=8, channels=4, dims=2, first_stage_key="image",
                           cond_stage_key="mask", num_timesteps_cond=1, use_ema=False).eval()


# ------------------------------------------------------------------------------------------------ surface and configs
def test_vqmodelinterface_surface_equals_the_reference():
    from jointimagegeneration_amd.config import instantiate_from_config
    from jointimagegeneration_amd.ldm import VQModelInterface
    with open(os.path.join(GOLD, "vq_surface.json")) as f:
        want = json.load(f)
    m = instantiate_from_config(vq_cfg(n_embed=want["n_embed"], embed_dim=want["embed_dim"]))
    assert isinstance(m, VQModelInterface)
    assert surface(m) == want["surface"]
    names = dict((k, s) for k, s in want["surface"])
    assert names["quantize.embedding.weight"] == [want["n_embed"], want["embed_dim"]]
    assert names["quant_conv.weight"] == [want["embed_dim"], 2 * AE_SMALL["z_channels"], 1, 1]          # the fork's 2 * z_channels
    assert names["post_quant_conv.weight"] == [AE_SMALL["z_channels"], want["embed_dim"], 1, 1]


def test_reference_dotted_paths_instantiate():
    from jointimagegeneration_amd import ldm
    from jointimagegeneration_amd.config import instantiate_from_config
    assert type(instantiate_from_config(vq_cfg("ldm.models.autoencoder.VQModel"))) is ldm.VQModel
    ident = instantiate_from_config(dict(target="ldm.models.autoencoder.IdentityFirstStage", params=dict(vq_interface=True)))
    assert isinstance(ident, ldm.IdentityFirstStage)
    x = torch.randn(1, 4, 2, 2)
    assert ident.encode(x) is x and ident.decode(x) is x and ident(x) is x
    q, loss, info = ident.quantize(x)
    assert q is x and loss is None and list(info) == [None, None, None]
    assert ldm.IdentityFirstStage().quantize(x) is x
    vq = instantiate_from_config(dict(target="taming.modules.vqvae.quantize.VectorQuantizer", params=dict(n_e=7, e_dim=3, beta=0.25)))
    assert isinstance(vq, ldm.VectorQuantizer) and tuple(vq.embedding.weight.shape) == (7, 3)
    assert float(vq.embedding.weight.detach().abs().max()) <= 1.0 / 7
    m = vq_ldm(vq_cfg())
    assert isinstance(m.first_stage_model, ldm.VQModelInterface)
    assert "first_stage_model.quantize.embedding.weight" in m.state_dict()
    # index lookups are host-side plumbing: they run without a GPU
    w = m.first_stage_model.quantize.embedding.weight
    idx = torch.tensor([[[3, 5], [0, 63]]])
    e = m.first_stage_model.quantize.embed_code(idx)
    assert tuple(e.shape) == (1, 4, 2, 2) and torch.equal(e[0, :, 1, 1], w[63]) and torch.equal(e[0, :, 0, 1], w[5])
    assert torch.equal(m.first_stage_model.quantize.get_codebook_entry(idx.reshape(-1), (1, 2, 2, 4)), e)
    assert torch.equal(m.first_stage_model.quantize.get_codebook_entry(idx.reshape(-1), None), w[idx.reshape(-1)])


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_their_option():
    from jointimagegeneration_amd.config import instantiate_from_config
    from jointimagegeneration_amd.ldm import DDIMSampler, PLMSSampler
    from jointimagegeneration_amd.unet import UNetModel
    m = vq_ldm(vq_cfg())
    with pytest.raises(NotImplementedError, match="predict_cids"):
        m.decode_first_stage(torch.zeros(1, 4, 8, 8), predict_cids=True)
    with torch.device("meta"):
        with pytest.raises(NotImplementedError, match="n_embed"):
            UNetModel(**LDM_SMALL, n_embed=64)
    for cls in (DDIMSampler, PLMSSampler):
        with pytest.raises(NotImplementedError, match="score_corrector"):
            cls(m).sample(S=5, batch_size=2, shape=(4, 8, 8), verbose=False, quantize_x0=True, score_corrector=object())
    for kw, name in ((dict(remap="x.npy"), "remap"), (dict(sane_index_shape=True), "sane_index_shape"),
                     (dict(batch_resize_range=(16, 32)), "batch_resize_range"), (dict(use_ema=True), "use_ema")):
        with pytest.raises(NotImplementedError, match=name):
            instantiate_from_config(vq_cfg(**kw))
    with pytest.raises(NotImplementedError, match=re.escape("the shipped AE configs are 2-D")):      # AutoencoderKL's message
        instantiate_from_config(vq_cfg(dims=3, ddconfig=dict((k, v) for k, v in AE_SMALL.items() if k != "dims")))


def test_quantisation_without_a_codebook_is_refused_before_any_launch():
    """CPU tensors, no GPU here: the errors come from host code."""
    from jointimagegeneration_amd.ldm import DDIMSampler, LatentDiffusion, PLMSSampler
    kl = small_ldm()                                          # AutoencoderKL first stage: no `quantize`
    for cls in (DDIMSampler, PLMSSampler):
        with pytest.raises(NotImplementedError, match="quantize_x0.*AutoencoderKL"):
            cls(kl).sample(S=5, batch_size=2, shape=(4, 8, 8), verbose=False, quantize_x0=True)
    with pytest.raises(NotImplementedError, match="quantize_denoised.*AutoencoderKL"):
        kl.p_sample_loop(None, (2, 4, 8, 8), quantize_denoised=True)
    with pytest.raises(NotImplementedError, match="quantize_denoised"):
        kl.sample(None, batch_size=2, shape=(2, 4, 8, 8), quantize_denoised=True)
    none = LatentDiffusion(first_stage_config="__is_no_first_stage__", cond_stage_config="__is_unconditional__",
                           unet_config=dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(LDM_SMALL)),
                           timesteps=20, image_size=8, channels=8, dims=2, use_ema=False)
    with pytest.raises(NotImplementedError, match="quantize_x0"):
        DDIMSampler(none).sample(S=5, batch_size=1, shape=(8, 8, 8), verbose=False, quantize_x0=True)
    wide = vq_ldm(vq_cfg(embed_dim=3))                        # codebook width 3, latent of 4 channels
    with pytest.raises(ValueError, match="e_dim = 3"):
        DDIMSampler(wide).sample(S=5, batch_size=2, shape=(4, 8, 8), verbose=False, quantize_x0=True)
    with pytest.raises(ValueError, match="noise_dropout"):
        DDIMSampler(kl).sample(S=5, batch_size=2, shape=(4, 8, 8), verbose=False, noise_dropout=1.0)


# ------------------------------------------------------------------------------------------------ C-ABI
def test_entries_reject_bad_arguments_on_the_host():
    from jointimagegeneration_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    unsupported, bad_shape = -3, -1
    assert _lib.GG_ERR_BAD_SHAPE == -1 and _lib.GG_ERR_UNSUPPORTED == -3
    for Cc in (0, 9, 16):
        assert lib.gg_vq_nearest(p, 32, p, 8, Cc, 4, p, p, 32, None) == unsupported
        assert b"C=" in lib.gg_last_error()
        assert lib.gg_ddim_step_vq(p, p, 32, None, p, 0, p, 8, 4, Cc, None, None, None, 0, None) == unsupported
    assert lib.gg_vq_nearest(None, 4, p, 8, 4, 4, p, p, 4, None) == bad_shape
    assert lib.gg_vq_nearest(p, 4, None, 8, 4, 4, p, p, 4, None) == bad_shape
    assert lib.gg_vq_nearest(p, 4, p, 8, 4, 4, None, None, 0, None) == bad_shape            # no output at all
    assert lib.gg_vq_nearest(p, 3, p, 8, 4, 4, p, None, 0, None) == bad_shape               # row stride < C
    assert lib.gg_vq_nearest(p, 4, p, 8, 4, 4, p, p, 3, None) == bad_shape                  # output stride < C
    assert lib.gg_vq_nearest(p, 4, p, 0, 4, 4, p, p, 4, None) == bad_shape                  # empty codebook
    assert lib.gg_vq_nearest(p, 4, p, 8, 4, 0, p, p, 4, None) == 0                          # M = 0: nothing to do, no launch
    assert lib.gg_ddim_step_vq(None, p, 32, None, p, 0, p, 8, 4, 4, None, None, None, 0, None) == bad_shape
    assert lib.gg_ddim_step_vq(p, p, 3, None, p, 0, p, 8, 4, 4, None, None, None, 0, None) == bad_shape       # eps stride < C
    assert lib.gg_ddim_step_vq(p, p, 32, None, p, 0, p, 8, 4, 4, None, None, p, 3, None) == bad_shape         # unet_in stride < C
    assert lib.gg_ddim_step_vq(p, p, 32, None, p, 0, None, 8, 4, 4, None, None, None, 0, None) == bad_shape   # n_embed without a codebook
    assert lib.gg_ddim_step_vq(p, p, 32, None, p, 0, None, 0, 4, 4, p, None, None, 0, None) == bad_shape      # indices without a codebook
    assert lib.gg_ddim_step_vq(p, p, 32, None, p, 1, p, 8, 0, 4, None, None, None, 0, None) == 0


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_restatement_against_a_hand_computed_case():
    """E = [(0,0), (1,0), (1,0), (0,2)] (codes 1 and 2 are duplicates).
    row (0.75, 0):   d = 0.5625, 0.0625, 0.0625, 4.5625     -> tie between 1 and 2: the first, 1
    row (0.5, 1):    d = 1.25, 1.25, 1.25, 1.25             -> four-way tie: 0
    row (-1, 1.5):   d = 3.25, 6.25, 6.25, 1.25             -> 3"""
    E = torch.tensor([[0.0, 0.0], [1.0, 0.0], [1.0, 0.0], [0.0, 2.0]])
    rows = torch.tensor([[0.75, 0.0], [0.5, 1.0], [-1.0, 1.5]])
    d = vq_ref.distances(rows, E)
    assert torch.equal(d, torch.tensor([[0.5625, 0.0625, 0.0625, 4.5625], [1.25, 1.25, 1.25, 1.25], [3.25, 6.25, 6.25, 1.25]], dtype=torch.float64))
    idx, amb = vq_ref.quantise(rows, E)
    assert idx.tolist() == [1, 0, 3]
    assert amb.tolist() == [True, True, False]                  # exact ties are "ambiguous" for inexact arithmetic; exact inputs ignore the flag
    assert torch.equal(vq_ref.straight_through(rows, E, idx), E[idx])
    q, loss, (perp, enc, ind) = vq_ref.RefVectorQuantizer(4, 2)(torch.zeros(1, 2, 1, 3))
    assert loss is None and perp is None and enc is None and tuple(ind.shape) == (3, 1) and ind.dtype == torch.int64
    # the straight-through expression is not z_q: one rounding apart for inexact values
    z = torch.tensor([[0.1, 0.3]])
    E2 = torch.tensor([[1.0 / 3.0, 0.7]])
    st = vq_ref.straight_through(z, E2, torch.tensor([0]))
    assert torch.allclose(st, E2, rtol=0, atol=2 ** -23) and tuple(st.shape) == (1, 2)
