"""Score a first-stage checkpoint on held-out volumes: the reference's `AutoencoderKL.validation_step` (autoencoder.py:401-416) over a
directory, on the device.

    python -m jointimagegeneration_amd.ae_eval --config AE.yaml --ckpt AE.ckpt --ct DIR [--seg DIR] [--every K] [--seed S]
                                               [--lpips-vgg PATH --lpips-lin PATH] --out metrics.json

Volumes are read with `io.read_nifti` and used as they are: CT already in the model's value range (as `sample_diffusion` writes it),
labels already scaled as `gg_mask_to_cond_slice` scales them; nothing is windowed or resampled.  `image_key: image` feeds the CT slice,
`image_key: mask` feeds [previous CT slice (zeros for the first), label slice] -- the dataset's `control` -- from the same-named volume
of --seg.  A `dims: 3` model gets whole volumes.  Each batch is one `validation_losses` call whose posterior noise comes from
`torch.Generator().manual_seed(S + index)` on the host, so reruns agree; metrics.json holds the mean of every key over the batches, in
order, and the `global_step` used (the checkpoint's: it decides disc_factor against disc_start).  --lpips-vgg / --lpips-lin load the
VGG16 / lin weights where the checkpoint does not carry `loss.perceptual_loss.*`.  Local files only; nothing is fetched.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys
from typing import List, Optional

import numpy as np
import torch

from .config import instantiate_from_config, load_yaml
from .io import load_checkpoint, read_nifti
from .lpips import map_lin_state_dict, map_vgg_state_dict
from .sample_diffusion import strip_ckpt_paths


def volume_files(d: str) -> List[str]:
    files = sorted(f for f in glob.glob(os.path.join(d, "*.nii*")) if f.endswith((".nii", ".nii.gz")))
    if not files:
        raise FileNotFoundError(f"{d}: no *.nii / *.nii.gz volumes")
    return files


def batches(ct: np.ndarray, seg: Optional[np.ndarray], image_key: str, dims: int, every: int) -> List[torch.Tensor]:
    """The model inputs of one volume [D, H, W], as host fp32 tensors [1, C, ...]."""
    ct_t = torch.from_numpy(np.array(ct, dtype=np.float32))                 # a copy: read_nifti's array may be read-only
    if dims == 3:
        if image_key != "image":
            raise NotImplementedError(f"ae_eval: image_key '{image_key}' with a dims = 3 model (whole volumes are fed as 'image')")
        return [ct_t[None, None]]
    if image_key == "image":
        return [ct_t[d][None, None] for d in range(0, ct_t.shape[0], every)]
    if image_key != "mask":
        raise NotImplementedError(f"ae_eval: image_key '{image_key}' (one of 'image', 'mask')")
    seg_t = torch.from_numpy(np.array(seg, dtype=np.float32))
    out = []
    for d in range(0, ct_t.shape[0], every):
        prev = ct_t[d - 1] if d > 0 else torch.zeros_like(ct_t[0])
        out.append(torch.stack([prev, seg_t[d]])[None])
    return out


def load_model(config: str, ckpt: str, lpips_vgg: Optional[str], lpips_lin: Optional[str]):
    """(model on the host in eval mode, the checkpoint's global_step).  Every file is checked before the device is touched."""
    cfg = strip_ckpt_paths(load_yaml(config))
    model = instantiate_from_config(cfg["model"]).eval()
    if isinstance(model.loss, torch.nn.Identity):
        raise ValueError(f"{config}: the model's lossconfig names no objective this engine scores (ldm.modules.losses.LPIPSWithDiscriminator)")
    ck = load_checkpoint(ckpt)
    sd = ck["state_dict"] if "state_dict" in ck else ck
    missing, unexpected = model.load_state_dict(sd, strict=False)
    own = [k for k in missing if not k.startswith("loss.perceptual_loss.")]
    if own or unexpected:
        raise KeyError(f"{ckpt}: missing keys {own[:8]}{'...' if len(own) > 8 else ''}, unexpected keys {list(unexpected)[:8]}")
    lp_missing = [k for k in missing if k.startswith("loss.perceptual_loss.") and ".scaling_layer." not in k]
    if lp_missing:
        if not lpips_vgg or not lpips_lin:
            raise KeyError(f"{ckpt}: carries no loss.perceptual_loss.* weights ({len(lp_missing)} missing): give --lpips-vgg and --lpips-lin")
        lp = dict(map_vgg_state_dict(load_checkpoint(lpips_vgg), lpips_vgg))
        lp.update(map_lin_state_dict(load_checkpoint(lpips_lin), lpips_lin))
        model.loss.perceptual_loss.load_state_dict(lp, strict=False)
    return model, int(ck.get("global_step", 0)) if isinstance(ck, dict) else 0


def evaluate(model, ct_files: List[str], seg_dir: Optional[str], every: int, seed: int, device):
    """({key: mean over the batches of all volumes, in file then slice order}, number of batches)."""
    sums, count = None, 0
    for path in ct_files:
        seg = None
        if model.image_key == "mask":
            sp = os.path.join(seg_dir, os.path.basename(path))
            if not os.path.isfile(sp):
                raise FileNotFoundError(f"no label volume {sp} for {path}")
            seg = read_nifti(sp)
        ct = read_nifti(path)
        if seg is not None and seg.shape != ct.shape:
            raise ValueError(f"{path}: CT {ct.shape} and labels {seg.shape} differ in shape")
        for x in batches(ct, seg, model.image_key, model.dims, every):
            x = x.to(device)
            noise = torch.randn(model.latent_shape(x.shape), generator=torch.Generator().manual_seed(seed + count)).to(device)
            log = model.validation_losses(x, noise=noise)
            keys = list(log)
            vals = torch.stack([v.double() for v in log.values()])
            sums = vals if sums is None else sums + vals
            count += 1
    means = (sums / count).cpu().tolist()                  # the one readback of the run
    return dict(zip(keys, means)), count


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description="held-out losses of an AutoencoderKL checkpoint (val/rec_loss and the rest of validation_step)")
    ap.add_argument("--config", required=True, help="the autoencoder's yaml (model: target / params)")
    ap.add_argument("--ckpt", required=True, help="checkpoint with state_dict (and global_step)")
    ap.add_argument("--ct", required=True, help="directory of CT volumes, *.nii / *.nii.gz, already in the model's value range")
    ap.add_argument("--seg", default=None, help="directory of same-named label volumes (image_key: mask)")
    ap.add_argument("--every", type=int, default=1, help="score every K-th slice (2-D models)")
    ap.add_argument("--seed", type=int, default=1024, help="batch i draws its posterior noise from seed + i")
    ap.add_argument("--lpips-vgg", default=None, help="VGG16 feature state dict, when the checkpoint has no loss.perceptual_loss.*")
    ap.add_argument("--lpips-lin", default=None, help="lpips checkpoint with linK.model.1.weight")
    ap.add_argument("--out", required=True, help="metrics.json path")
    args = ap.parse_args(argv)
    if args.every < 1:
        raise ValueError(f"--every {args.every}: at least 1")
    if bool(args.lpips_vgg) != bool(args.lpips_lin):
        raise ValueError("--lpips-vgg and --lpips-lin go together")
    for p in (args.config, args.ckpt, args.lpips_vgg, args.lpips_lin):
        if p and not os.path.isfile(p):
            raise FileNotFoundError(f"{p!r} is not a file (local files only: nothing is fetched)")
    files = volume_files(args.ct)
    model, step = load_model(args.config, args.ckpt, args.lpips_vgg, args.lpips_lin)
    if model.image_key == "mask" and not args.seg:
        raise ValueError("image_key 'mask' needs --seg DIR: the input is [previous CT slice, label slice]")
    assert torch.cuda.is_available(), "the GuideGen engine needs an MI355X (no CPU fallback)"
    dev = torch.device("cuda", 0)
    model = model.to(dev)
    model.global_step = step
    means, count = evaluate(model, files, args.seg, args.every, args.seed, dev)
    doc = dict(config=os.path.basename(args.config), ckpt=os.path.basename(args.ckpt), global_step=step, batches=count, seed=args.seed,
               every=args.every, volumes=[os.path.basename(f) for f in files], **means)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(f"val/rec_loss {doc['val/rec_loss']:.6f} over {count} batch(es) -> {args.out}", file=sys.stderr)
    return doc


if __name__ == "__main__":
    main(sys.argv[1:])
