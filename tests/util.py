"""Shared test helpers (tests may import both the product package and the oracle)."""
import json
import os

import numpy as np
import torch

from jointimagegeneration_amd.synth import randomize_parameters

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 1024

CCDM_SMALL = dict(base_channels=32, channel_mult=[1, 2, 2], attention_resolutions=[2, 4], num_heads=1,
                  num_head_channels=32, softmax_output=True)
LDM_SMALL = dict(image_size=16, in_channels=8, out_channels=4, model_channels=32, attention_resolutions=[2, 4],
                 num_res_blocks=2, channel_mult=[1, 2, 2], num_head_channels=32, dims=2)
AE_SMALL = dict(double_z=True, z_channels=4, resolution=32, in_channels=1, out_ch=1, ch=32, ch_mult=[1, 2, 2],
                num_res_blocks=1, dropout=0.0, dims=2, attn_resolutions=[])
CCDM_FULL = dict(base_channels=64, channel_mult=[1, 2, 2, 4, 5], attention_resolutions=[32, 16, 8], num_heads=1,
                 num_head_channels=32, softmax_output=True)
LDM_FULL = dict(dims=2, image_size=512, in_channels=8, out_channels=4, model_channels=160, attention_resolutions=[8, 4, 2],
                num_res_blocks=2, channel_mult=[1, 2, 4, 4, 5], num_head_channels=32)
AE_FULL = dict(double_z=True, z_channels=4, resolution=512, in_channels=1, out_ch=1, ch=128, ch_mult=[1, 2, 4, 4],
               num_res_blocks=2, dropout=0.0, dims=2, attn_resolutions=[16, 8])


def load_lib():
    """The loaded C-ABI library (ctypes), built first where this checkout has not been built yet."""
    import __graft_entry__ as ge
    from jointimagegeneration_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)


def T(a):
    return torch.from_numpy(np.asarray(a))


def surface(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


def sd_cpu(m):
    return {k: v.detach().float().cpu().clone() for k, v in m.state_dict().items()}


def seeded(mod, prefix):
    randomize_parameters(mod, SEED, prefix)
    return mod.eval()


def rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def rms_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float(torch.sqrt(((a - b) ** 2).mean()) / (torch.sqrt((b ** 2).mean()) + 1e-30))


def synth_labels(shape, n_labels=12, seed=0):
    """Deterministic nested-ellipsoid label volume [D, H, W] int64 (labels 0..n_labels-1) used by the stage-glue fixtures and
    the pipeline tests; pure integer / float64 numpy so that it is identical in the build container and on the GPU box."""
    D, H, W = shape
    z, y, x = np.meshgrid(np.arange(D, dtype=np.float64), np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    lab = np.zeros(shape, dtype=np.int64)
    rs = np.random.RandomState(seed)
    for k in range(1, n_labels):
        c = (rs.uniform(0.3, 0.7) * D, rs.uniform(0.3, 0.7) * H, rs.uniform(0.3, 0.7) * W)
        r = (rs.uniform(0.08, 0.3) * D + 1, rs.uniform(0.08, 0.3) * H + 1, rs.uniform(0.08, 0.3) * W + 1)
        lab[((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 <= 1.0] = k
    return lab


def small_ldm(prefix="ldm_pipe.", use_ema=False):
    """The small LatentDiffusion (UNet LDM_SMALL, first/cond stage AE_SMALL with 1 / 2 input channels) that the chain and
    slice-loop fixtures were captured on (tests/golden/make_golden.py fx_chains / fx_autoreg), with the seed-recipe weights."""
    from jointimagegeneration_amd.ldm import LatentDiffusion
    cfg_unet = dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(LDM_SMALL))
    ae = lambda cin: dict(target="ldm.models.autoencoder.AutoencoderKL",
                          params=dict(embed_dim=4, dims=2, ddconfig=dict(AE_SMALL, in_channels=cin, out_ch=cin), lossconfig=dict(target="torch.nn.Identity")))
    m = LatentDiffusion(first_stage_config=ae(1), cond_stage_config=ae(2), unet_config=cfg_unet, linear_start=0.0015, linear_end=0.0195,
                        timesteps=1000, image_size=8, channels=4, dims=2, first_stage_key="image", cond_stage_key="mask",
                        num_timesteps_cond=1, use_ema=use_ema)
    return seeded(m, prefix)


def oracle_slice_loop(sd_all, wholemask, x_T_list, ddim_steps, alphas_cumprod, model_channels, head_channels=32, n_samples=1):
    """oracle.samplers.autoregressive_slices (sample_diffusion.py:196-224) on a LatentDiffusion state_dict, eta = 0: the x_T of
    every slice comes from `x_T_list`, the per-step noises (multiplied by sigma = 0) are zeros."""
    from oracle import nets as O
    from oracle import samplers as S
    sd_unet, sd_fs, sd_cs = (O.sub_state_dict(sd_all, p) for p in ("model.diffusion_model.", "first_stage_model.", "cond_stage_model."))
    shape = tuple(x_T_list[0].shape[1:])
    draws = []
    for x in x_T_list:
        draws += [x.float()] + [torch.zeros_like(x, dtype=torch.float32)] * ddim_steps
    it = iter(draws)
    return S.autoregressive_slices(lambda cc: O.ae_encode_mode(sd_cs, cc),
                                   lambda c: (lambda x, t: O.unet_forward(sd_unet, torch.cat([x, c], 1), t, model_channels=model_channels, head_channels=head_channels)),
                                   lambda z: O.ae_decode(sd_fs, z), wholemask, n_samples, shape, lambda shp: next(it), alphas_cumprod, ddim_steps)
