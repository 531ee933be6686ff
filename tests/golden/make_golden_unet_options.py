"""Generates tests/golden/unet_options.npz and unet_options_surfaces.json from the REFERENCE modules on CPU: the UNet constructor
options use_scale_shift_norm (FiLM), resblock_updown, use_new_attention_order and conv_resample=False, which the oracle restatement
does not cover.

Run only in the build container (needs the reference tree, like make_golden.py):
    python tests/golden/make_golden_unet_options.py [OUT_DIR]
Weights come from jointimagegeneration_amd.synth (name, shape, seed) on both sides; the fixtures hold inputs (bf16-representable
values, so that both engine paths read them exactly), fp32 outputs and sha256 digests of the state_dict surfaces.
"""
from __future__ import annotations

import hashlib
import itertools
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

from jointimagegeneration_amd.synth import randomize_parameters  # noqa: E402

SEED = MG.SEED
OPTIONS = ("use_scale_shift_norm", "resblock_updown", "use_new_attention_order", "conv_resample")
CCDM_SMALL = dict(MG.CCDM_SMALL)
LDM_SMALL = dict(MG.LDM_SMALL)
ALL_ON = dict(use_scale_shift_norm=True, resblock_updown=True, use_new_attention_order=True)


def surface(m):
    """sha256 of the state_dict names and shapes, [[name, shape], ...] as compact JSON (tests/test_unet_options_cpu.py hashes alike)."""
    s = json.dumps([[k, list(v.shape)] for k, v in m.state_dict().items()], separators=(",", ":"))
    return hashlib.sha256(s.encode()).hexdigest()


def rnd(gen, *shape):
    return torch.randn(*shape, generator=gen).bfloat16().float()


def ccdm_unet(unet_mod, K, **opts):
    """The reference CCDM UNetModel as create_unet_openai builds it (unet_openai/__init__.py), plus conv_resample."""
    cfg = dict(CCDM_SMALL)
    base = cfg.pop("base_channels")
    return unet_mod.UNetModel(in_channels=K + 1, model_channels=base, out_channels=K, num_res_blocks=2, cond_encoded_shape=None,
                              num_classes=None, dims=3, **cfg, **opts)


def fx_blocks(unet_ccdm, om, out, surf):
    gen = MG.g(31)

    def rb(name, mod, x_shape, prefix):
        m = mod.eval()
        randomize_parameters(m, SEED, prefix)
        x = rnd(gen, *x_shape)
        emb = torch.randn(x_shape[0], 128, generator=gen)
        out.update({f"{name}_x": x, f"{name}_emb": emb, f"{name}_y": m(x, emb)})
        surf[name] = surface(m)

    # FiLM ResBlocks at N = 2 (a different emb per sample): 64 -> 96 with the 1x1 skip, and same-channel
    rb("rbf3a", unet_ccdm.ResBlock(64, 128, 0.0, out_channels=96, dims=3, use_scale_shift_norm=True), (2, 64, 2, 4, 4), "rbf3a.")
    rb("rbf3b", unet_ccdm.ResBlock(64, 128, 0.0, out_channels=64, dims=3, use_scale_shift_norm=True), (2, 64, 2, 4, 4), "rbf3b.")
    rb("rbf2a", om.ResBlock(64, 128, 0.0, out_channels=96, dims=2, use_scale_shift_norm=True), (2, 64, 4, 8), "rbf2a.")
    rb("rbf2b", om.ResBlock(64, 128, 0.0, out_channels=64, dims=2, use_scale_shift_norm=True), (2, 64, 4, 8), "rbf2b.")
    # up / down ResBlocks (resblock_updown), plain and with FiLM
    rb("rbd3", unet_ccdm.ResBlock(64, 128, 0.0, dims=3, down=True), (2, 64, 2, 4, 4), "rbd3.")
    rb("rbu3", unet_ccdm.ResBlock(64, 128, 0.0, dims=3, up=True), (2, 64, 1, 2, 2), "rbu3.")
    rb("rbdf3", unet_ccdm.ResBlock(64, 128, 0.0, dims=3, down=True, use_scale_shift_norm=True), (2, 64, 2, 4, 4), "rbdf3.")
    rb("rbuf3", unet_ccdm.ResBlock(64, 128, 0.0, dims=3, up=True, use_scale_shift_norm=True), (2, 64, 1, 2, 2), "rbuf3.")
    rb("rbd2", om.ResBlock(64, 128, 0.0, dims=2, down=True), (2, 64, 4, 8), "rbd2.")
    rb("rbu2", om.ResBlock(64, 128, 0.0, dims=2, up=True), (2, 64, 2, 4), "rbu2.")
    # new-order attention with 2 / 3 heads (one head would not see the order)
    for name, mod, shape in (("abn3", unet_ccdm.AttentionBlock(64, num_head_channels=32, use_new_attention_order=True), (2, 64, 2, 2, 4)),
                             ("abn2", om.AttentionBlock(96, num_heads=-1, num_head_channels=32, use_new_attention_order=True), (2, 96, 4, 4))):
        m = mod.eval()
        randomize_parameters(m, SEED, name + ".")
        x = rnd(gen, *shape)
        out.update({f"{name}_x": x, f"{name}_y": m(x)})
        surf[name] = surface(m)
    # conv-free Upsample / Downsample (48 channels: the pad lanes of a 64-lane tensor)
    for name, ref, dims, shape in (("rs3", unet_ccdm, 3, (2, 48, 2, 2, 4)), ("rs2", om, 2, (2, 48, 4, 4))):
        x = rnd(gen, *shape)
        up, dn = ref.Upsample(48, False, dims=dims).eval(), ref.Downsample(48, False, dims=dims).eval()
        out.update({f"{name}_x": x, f"{name}_up": up(x), f"{name}_dn": dn(x)})
        surf[name + "_up"], surf[name + "_dn"] = surface(up), surface(dn)


def fx_networks(unet_ccdm, om, out, surf):
    gen = MG.g(37)
    K = 6
    lab = torch.randint(0, K, (2, 8, 8, 8), generator=gen)
    from oracle import samplers as S
    xt = S.one_hot_bchw(lab, K)
    cond = rnd(gen, 2, 1, 8, 8, 8)
    t = torch.tensor([17.0, 143.0])
    out.update(ccdm_labels=lab.int(), ccdm_cond=cond, ccdm_t=t)
    for name, opts in (("ccdm_opt", ALL_ON), ("ccdm_nc", dict(conv_resample=False))):
        u = ccdm_unet(unet_ccdm, K, **opts).eval()
        randomize_parameters(u, SEED, name + ".")
        out[name + "_probs"] = u(xt, cond, None, t)["diffusion_out"]
        surf[name] = surface(u)
    u2 = om.UNetModel(**LDM_SMALL, **ALL_ON).eval()
    randomize_parameters(u2, SEED, "ldm_opt.")
    x = rnd(gen, 2, 8, 16, 16)
    t2 = torch.tensor([981, 500])
    out.update(ldm_x=x, ldm_t=t2, ldm_opt_eps=u2(x, t2))
    surf["ldm_opt"] = surface(u2)


def fx_surfaces(unet_ccdm, om, surf):
    """state_dict surfaces of both small UNets for every combination of the four options."""
    for bits in itertools.product((False, True), repeat=4):
        opts = dict(zip(OPTIONS[:3], bits[:3]), conv_resample=not bits[3])
        tag = "".join("1" if b else "0" for b in bits)
        surf[f"ccdm_{tag}"] = surface(ccdm_unet(unet_ccdm, 6, **opts))
        surf[f"ldm_{tag}"] = surface(om.UNetModel(**LDM_SMALL, **opts))


def main(out_dir):
    torch.manual_seed(0)
    _, _, _, unet_ccdm, _ = MG.import_ccdm()
    om = MG.import_ldm()[0]
    out, surf = {}, {}
    fx_blocks(unet_ccdm, om, out, surf)
    fx_networks(unet_ccdm, om, out, surf)
    fx_surfaces(unet_ccdm, om, surf)
    arrs = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "unet_options.npz")
    np.savez_compressed(path, **arrs)
    with open(os.path.join(out_dir, "unet_options_surfaces.json"), "w") as f:
        json.dump(surf, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB) and unet_options_surfaces.json ({len(surf)} surfaces)")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else MG.OUT)
