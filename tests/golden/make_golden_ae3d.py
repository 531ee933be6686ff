"""Generates tests/golden/ae3d.npz and tests/golden/ae3d_surface.json from the REFERENCE on CPU: the volumetric (dims = 3) first stages
(ldm/models/autoencoder.py AutoencoderKL and VQModel over ldm/modules/diffusionmodules/model.py Encoder / Decoder with Conv3d,
AttnBlock3d, the (0,1,0,1,0,1) pad in front of the stride-2 conv) and 3-step DDIM chains of a tiny dims = 3 UNetModel on
[2, 4, 4, 6, 6] latents with concat conditioning (ldm/models/diffusion/ddim.py; free-running from x_T with recorded noise tapes, not
teacher-forced) plus one ancestral chain over 3 timesteps (ddpm.py p_sample_loop), imported with the stubs of make_golden.py.  taming's
VectorQuantizer is stood in for by tests/vq_ref.py:RefVectorQuantizer with a forward that takes any number of spatial axes.

Run only in the build container (needs the reference tree, like make_golden.py):
    python tests/golden/make_golden_ae3d.py [OUT_DIR]
Weights come from the seed recipe (jointimagegeneration_amd.synth; prefixes "ae3d_kl.", "ae3d_vq.", "ldm3d."; the VQ codebook is the
recipe's times CODE_SCALE), so the .npz holds inputs and reference outputs only.  A row of the pre-quantisation tensor is a near-tie at
the bf16 margin if its two smallest fp64 distances differ by less than BF16_TOL * (1 + d_min), the form of tests/vq_ref.py with the bf16
first-stage tolerance in place of 1e-4; the fixture's share of such rows is asserted below the 2 % cap here, on the CPU.
ae3d_surface.json holds the state_dict surfaces, the reference's conv output extents for sizes 5..8, its dims precedence, and its own fp32-vs-fp64 spread on the fixture (the same modules run in double on the same inputs).
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys
import unittest.mock as mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import vq_ref  # noqa: E402

from jointimagegeneration_amd.synth import randomize_parameters  # noqa: E402

torch.set_grad_enabled(False)
LOSS = dict(target="torch.nn.Identity")
AE3D = dict(double_z=True, z_channels=4, resolution=8, in_channels=1, out_ch=1, ch=32, ch_mult=[1, 2], num_res_blocks=1, dropout=0.0,
            dims=3, attn_resolutions=[4])
UNET3D = dict(image_size=6, in_channels=8, out_channels=4, model_channels=32, attention_resolutions=[2], num_res_blocks=1,
              channel_mult=[1, 2], num_head_channels=32, dims=3)
N_EMBED, EMBED_DIM = 16, 4
CODE_SCALE = 2.0                           # the seed recipe's N(0, 1/4) codebook times 2: codes about as far apart as the pre-quantisation rows spread
IMG_SEED = 3036                            # searched (3030..3129 x n_embed 16 / 32 / 64 x scale 1 / 2): the one draw with at most one of the
                                           # 60 rows inside the bf16 near-tie margin
IMG = (1, 1, 6, 8, 10)                     # non-cubic: the odd 3 x 4 x 5 level is reached through the trailing-pad downsample of D = 6 -> 3
LAT = (2, 4, 4, 6, 6)
S, SCALE = 3, 2.0
TIMESTEPS = 300                            # a multiple of S: the uniform DDIM schedule of 3 steps indexes past the end of a 1000-step one
BF16_TOL = 4e-2                            # the bf16 first-stage bound of tests/test_hip_parity.py; also the near-tie margin of the VQ indices
CAP = 0.02


class RefVectorQuantizerNd(vq_ref.RefVectorQuantizer):
    """RefVectorQuantizer on [N, C, *sp]: rows are the channels-last flattening (taming's class permutes (0, 2, 3, 1); same rule)."""

    def forward(self, z):
        nd = z.ndim - 2
        zc = z.permute((0,) + tuple(range(2, nd + 2)) + (1,)).contiguous()
        rows = zc.view(-1, self.e_dim)
        idx, _ = vq_ref.quantise(rows, self.embedding.weight, rows.dtype)
        q = vq_ref.straight_through(rows, self.embedding.weight, idx).view(zc.shape).permute((0, nd + 1) + tuple(range(1, nd + 1))).contiguous()
        return q, None, (None, None, idx.view(-1, 1))


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def near_tie(rows, E, tol):
    """bool [M]: the two smallest fp64 distances of a row differ by less than tol * (1 + d_min)"""
    two = torch.topk(vq_ref.distances(rows, E), 2, dim=1, largest=False).values
    return (two[:, 1] - two[:, 0]) < tol * (1.0 + two[:, 0])


@contextlib.contextmanager
def tapes(q_tape, step_tape, shape):
    """q_sample's randn_like <- q_tape rows in order; the step noise (torch.randn) <- step_tape rows, or zeros when None (eta = 0: the
    reference still draws, and multiplies the draw by sigma = 0)."""
    q_it = iter(q_tape)
    s_it = iter(step_tape) if step_tape is not None else None

    def randn_like(x, *a, **k):
        v = next(q_it)
        assert v.shape == x.shape, (v.shape, x.shape)
        return v.clone()

    def randn(*a, **k):
        return next(s_it).clone() if s_it is not None else torch.zeros(shape)
    with mock.patch.object(torch, "randn_like", randn_like), mock.patch.object(torch, "randn", randn), quiet(), \
            contextlib.redirect_stderr(io.StringIO()):
        yield
    assert next(q_it, None) is None, "q_sample drew fewer noises than the tape holds"
    assert s_it is None or next(s_it, None) is None, "the sampler drew fewer step noises than the tape holds"


def spread(a32, a64):
    """max |fp32 - fp64| relative to max |fp64|: the reference's own rounding on the fixture"""
    return float((a32.double() - a64).abs().max() / a64.abs().max())


def extents(mo):
    """The reference's Downsample / Upsample output extents for input sizes 5..8 (a one-channel module: the extents are what is recorded)."""
    dn, up = mo.Downsample(1, True, dims=3), mo.Upsample(1, True, dims=3)
    out = {}
    for s in (5, 6, 7, 8):
        x = torch.zeros(1, 1, s, s, s)
        out[str(s)] = dict(down=int(dn(x).shape[-1]), up=int(up(x).shape[-1]))
    mixed = torch.zeros(1, 1, 5, 6, 7)
    out["5x6x7"] = dict(down=list(dn(mixed).shape[2:]), up=list(up(mixed).shape[2:]))
    return out


def precedence(ae, mo):
    """What the reference builds for each (ddconfig dims, model dims): the kernel rank of encoder.conv_in and of quant_conv."""
    out = []
    for dd, md in ((None, None), (None, 2), (2, 2), (3, None), (3, 3), (2, 3), (3, 2)):
        cfg = dict((k, v) for k, v in AE3D.items() if k != "dims")
        if dd is not None:
            cfg["dims"] = dd
        kw = {} if md is None else dict(dims=md)
        with quiet():
            m = ae.AutoencoderKL(ddconfig=cfg, lossconfig=LOSS, embed_dim=4, **kw)
        out.append(dict(ddconfig_dims=dd, model_dims=md, encoder_rank=m.encoder.conv_in.weight.ndim - 2, quant_conv_rank=m.quant_conv.weight.ndim - 2))
    return out


def main(out_dir):
    _om, _at, mo, ae, dm, di, _ut = MG.import_ldm()
    ae.VectorQuantizer = RefVectorQuantizerNd
    with quiet():
        kl = ae.AutoencoderKL(ddconfig=dict(AE3D), lossconfig=LOSS, embed_dim=EMBED_DIM, dims=3).eval()
        vq = ae.VQModel(ddconfig=dict(AE3D), lossconfig=LOSS, n_embed=N_EMBED, embed_dim=EMBED_DIM, dims=3).eval()
    randomize_parameters(kl, MG.SEED, "ae3d_kl.")
    randomize_parameters(vq, MG.SEED, "ae3d_vq.")
    vq.quantize.embedding.weight.mul_(CODE_SCALE)
    gen = MG.g(IMG_SEED)
    img = torch.rand(IMG, generator=gen) * 2.0 - 1.0
    post = kl.encode(img)
    z = post.mode()
    assert tuple(z.shape) == (1, 4, 3, 4, 5)
    dec = kl.decode(z)
    assert tuple(dec.shape) == IMG
    quant, _, (_, _, idx) = vq.encode(img)
    prequant = vq.encode_to_prequant(img)
    vq_dec = vq.decode(quant)
    rows = prequant.permute(0, 2, 3, 4, 1).reshape(-1, EMBED_DIM)
    E = vq.quantize.embedding.weight
    i64, amb = vq_ref.quantise(rows, E)
    assert not bool(amb.any()) and torch.equal(i64, idx.view(-1)), "pick another seed: the pre-quantisation tensor has an fp32-level near-tie"
    share = float(near_tie(rows, E, BF16_TOL).float().mean())
    assert share < CAP, f"near-tie share {share:.3f} at the bf16 margin is not below the cap"
    assert len(torch.unique(idx)) >= 6                                  # the codes in use are not a handful

    # the reference's own fp32-vs-fp64 spread on the fixture
    kl64, vq64 = kl.double(), vq.double()
    p64 = kl64.encode(img.double())
    sp = dict(kl_mean=spread(post.mean, p64.mean), kl_logvar=spread(post.logvar, p64.logvar), kl_decode=spread(dec, kl64.decode(z.double())),
              vq_prequant=spread(prequant, vq64.encode_to_prequant(img.double())), vq_decode=spread(vq_dec, vq64.decode(quant.double())))
    kl.float(), vq.float()

    # ---- 3-step DDIM chains of a dims = 3 latent diffusion model with concat conditioning
    cfg_unet = dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(UNET3D))
    cfg_ae = dict(target="ldm.models.autoencoder.AutoencoderKL", params=dict(embed_dim=4, dims=3, ddconfig=dict(AE3D), lossconfig=LOSS))
    with quiet():
        m = dm.LatentDiffusion(first_stage_config=cfg_ae, cond_stage_config=cfg_ae, unet_config=cfg_unet, linear_start=0.0015,
                               linear_end=0.0195, timesteps=TIMESTEPS, image_size=6, channels=4, dims=3, first_stage_key="image",
                               cond_stage_key="mask", num_timesteps_cond=1, conditioning_key="concat").eval()
    randomize_parameters(m, MG.SEED, "ldm3d.")
    gc = MG.g(3131)
    half = lambda t: t.half().float()                                   # fp16-representable: stored as fp16, read back exactly
    c, uc, x_T, x0 = (half(torch.randn(LAT, generator=gc)) for _ in range(4))
    q_tape, step_tape = half(torch.randn((S,) + LAT, generator=gc)), half(torch.randn((S,) + LAT, generator=gc))
    hole = torch.ones(LAT[0], 1, *LAT[2:])
    hole[:, :, 1:3, 2:5, 1:4] = 0.0                                     # zeros are generated
    ddim = di.DDIMSampler(m)
    run = lambda **kw: ddim.sample(S=S, batch_size=LAT[0], shape=LAT[1:], conditioning=c, verbose=False, x_T=x_T, dims=3, **kw)[0]
    out = dict(img=img, kl_mean=post.mean, kl_logvar=post.logvar, kl_z=z, kl_dec=dec, vq_quant=quant, vq_idx=idx.view(-1).int(),
               vq_prequant=prequant, vq_dec=vq_dec, c=c.half(), uc=uc.half(), x_T=x_T.half(), x0=x0.half(), mask_hole=hole,
               q_tape=q_tape.half(), step_tape=step_tape.half())
    with tapes(q_tape[:0], None, LAT):
        out["z_plain_eta0"] = run()
    with tapes(q_tape, step_tape, LAT):
        out["z_mask_eta1"] = run(eta=1.0, mask=hole, x0=x0)
    with tapes(q_tape, None, LAT):
        out["z_cfg_mask_eta0"] = run(mask=hole, x0=x0, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc)
    with tapes(q_tape, step_tape, LAT):
        out["z_cfg_mask_eta1"] = run(eta=1.0, mask=hole, x0=x0, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc)
    out["ddim_timesteps"] = ddim.ddim_timesteps
    # the ancestral loop (ddpm.py:1179-1227) over 3 timesteps with the same mask, x0 and tapes.  (The reference's PLMSSampler is 2-D only:
    # plms.py:93 unpacks C, H, W and :201-204 builds [b, 1, 1, 1] scalars, so there is no reference PLMS chain on volumes.)
    with tapes(q_tape, step_tape, LAT):
        out["z_ancestral_mask"] = m.p_sample_loop(c, LAT, x_T=x_T, verbose=False, timesteps=S, mask=hole, x0=x0)
    zs = [out[k] for k in ("z_plain_eta0", "z_mask_eta1", "z_cfg_mask_eta0", "z_cfg_mask_eta1", "z_ancestral_mask")]
    assert all(tuple(v.shape) == LAT and bool(torch.isfinite(v).all()) for v in zs)
    assert all(float((a - b).abs().max()) > 1e-2 for i, a in enumerate(zs) for b in zs[i + 1:])      # every option changed the chain

    arrs = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "ae3d.npz")
    np.savez_compressed(path, **arrs)
    surf = lambda mod: [[k, list(v.shape)] for k, v in mod.state_dict().items()]
    meta = dict(ae3d=AE3D, unet3d=UNET3D, n_embed=N_EMBED, embed_dim=EMBED_DIM, code_scale=CODE_SCALE, bf16_tol=BF16_TOL, steps=S, timesteps=TIMESTEPS, guidance_scale=SCALE,
                near_tie_share_at_bf16_margin=share, fp32_vs_fp64_spread=sp, extents=extents(mo), precedence=precedence(ae, mo))
    with open(os.path.join(out_dir, "ae3d_surface.json"), "w") as f:
        f.write("{" + ",\n".join('"%s": %s' % (k, json.dumps(v)) for k, v in meta.items()))
        for name, mod in (("surface_kl", kl), ("surface_vq", vq)):
            f.write(',\n"%s": [\n' % name + ",\n".join(json.dumps(e) for e in surf(mod)) + "\n]")
        f.write("}\n")
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB) and ae3d_surface.json; near-tie share {share:.4f}; fp32-vs-fp64 spread {sp}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else MG.OUT)
