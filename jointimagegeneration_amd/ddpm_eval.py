"""CCDM mask sampling entry point: `python -m jointimagegeneration_amd.ddpm_eval params_eval.yml [exp_name]`.

Re-creates the CLI/config/checkpoint surface of ccdm/ddpm_eval.py:16-57 + ccdm/ddpm/evaluator.py:127-170,215-237,326-393
without ignite or datasets (out of scope, SURVEY.md 2.1 rows 4,7): seeds, flat yaml dict,
`build_model(..., backbone, params[params["backbone"]], ...)`, ignite-style checkpoint {"model", "average_model"} holding the
UNet's state_dict, x_T ~ uniform one-hot, condition image = zeros, output label = argmax.  Inputs are synthetic (the
hospital dataset is private): the volume extent comes from --size or the yaml key `input_size`.

Scores (evaluator.py:188-190, ddpm/utils.py:190-236; metrics.py): `--gt DIR` holds `gt_{vid:04d}.nii.gz` label volumes of the run's size;
the run then accumulates the [K, K] confusion matrix on the device and rank 0 writes `metrics.json` (the integer matrix, Dice per class
with `--ignore-class` removed, its mean).  `--samples S` (the yaml comment "samples: 12  # For GED calculation") samples S masks per
volume as one batch, written as `pred_{vid:04d}_s{j:02d}.nii.gz`; with --gt each volume then also gets its GED, the two diversities and
the Hungarian-matched IoU.  Without these options the run writes exactly what it wrote before they existed.

Objectives (trainer.py:298-327; losses.py): `--gt DIR --loss-t T1,T2,...` adds a `loss` block to metrics.json: per listed step t the
KL, cross-entropy and their sum of the ground-truth volumes noised to t, averaged over the volumes.  The noise of volume v at step t
comes from the Philox key (1024 + v) + (t << 32), so reruns agree and a volume's terms do not depend on the rank that scored it.

Mask editing (DenoisingModel.sample_labels known / keep / resample): `--known DIR` holds `known_{vid:04d}.nii.gz` label volumes of the
run's size, and exactly one of `--keep-classes a,b,c` (keep the voxels whose known label is listed) and `--keep-mask DIR`
(`keep_{vid:04d}.nii.gz`, non-zero = keep) says which voxels come back unchanged; `--resample R` repeats every step R times.  With
--samples S the S masks of a volume share one known / keep pair.  metrics.json (written with or without --gt) then holds an `edit`
block: per volume the kept fraction and the count of kept voxels that differ from known, which is 0.

Cleaning (postprocess.py; no counterpart in the reference): `--consensus` (with --samples S > 1) writes the per-voxel vote of a volume's
S masks as `consensus_{vid:04d}.nii.gz` and its entropy in nats as `entropy_{vid:04d}.nii.gz`, and adds a `consensus` block to
metrics.json.  `--largest-component all|a,b,c`, `--min-component V` and `--connectivity 6|26` clean the mask -- the consensus, or the
single sample at --samples 1 -- into `clean_{vid:04d}.nii.gz` and add a `components` block: per volume and class the components, voxels
and largest component before and after.  With --gt, `dice_consensus` / `dice_clean` (and their means) score the two new masks.  The
existing keys and files are untouched (--keep-mask / --keep-classes belong to mask editing, hence the new names).

Surface distances (metrics.surface_distances; medpy.metric.binary's hd / hd95 / asd / assd, the module evaluator.py takes dc, precision
and recall from): `--gt DIR --surface [--spacing d,h,w] [--surface-connectivity 1|2|3]` adds a `surface` block to metrics.json: the five
scores per class, their class means and `absent` (the classes missing from the prediction or the ground truth, which have no surface
distance: null), per volume and averaged over the run; with --samples S a volume's scores are the mean over its S masks.  With the
cleaning options `hd95_consensus` / `hd95_clean` stand beside `dice_consensus` / `dice_clean`.  --gt alone now also reports `precision`
and `recall` per class beside Dice.  Without --surface none of the surface kernels is launched.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch
import yaml

from . import distributed as ggd
from . import metrics
from . import postprocess
from .ccdm import build_model, uniform_x_T
from .encoder import build_feature_cond_encoder
from .io import load_checkpoint, read_nifti, write_nifti
from .losses import ccdm_step_losses
from .synth import randomize_parameters


def set_seeds(seed: int):
    random.seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)
    np.random.seed(seed % 2 ** 32)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


def build_from_params(params: dict, size, num_classes: int):
    input_shapes = [(1,) + tuple(size), (num_classes,) + tuple(size)]
    return build_model(time_steps=params["time_steps"], schedule=params["beta_schedule"], schedule_params=params.get("beta_schedule_params"),
                       input_shapes=input_shapes, cond_encoded_shape=None, backbone=params["backbone"],
                       backbone_params=params[params["backbone"]], dataset_file=params.get("dataset_file", "synthetic"),
                       step_T_sample=params.get("evaluation_vote_strategy"), feature_cond_encoder=params.get("feature_cond_encoder"),
                       dims=params.get("dims", 3))


def load_weights(model, params: dict, log=print) -> str:
    path = params.get("load_from")
    if path and os.path.exists(path):
        ckpt = load_checkpoint(path)
        sd = ckpt.get("average_model", ckpt.get("model", ckpt))        # Polyak average is what evaluator.predict uses
        missing, unexpected = model.unet.load_state_dict(sd, strict=False)
        log(f"loaded {path}: {len(missing)} missing / {len(unexpected)} unexpected keys")
        return path
    log(f"checkpoint {path!r} not found: using random-init weights from the seed recipe (synthetic run)")
    randomize_parameters(model.unet, 1024, "ccdm.")
    return "random-init"


def loss_key(vid: int, t: int) -> int:
    """The Philox key of volume `vid` at step `t` of the --loss-t block."""
    return (1024 + vid) + (t << 32)


def load_edit(args, vids, size, K: int):
    """{vid: (known int32 [D, H, W], keep uint8 [D, H, W])} of --known with --keep-classes or --keep-mask; None without --known.
    Host-side: a bad option or volume ends the run before any sampling."""
    if args.known is None:
        if args.keep_classes is not None or args.keep_mask is not None or args.resample != 1:
            raise ValueError("--keep-classes / --keep-mask / --resample edit a known mask: give --known DIR")
        return None
    if (args.keep_classes is None) == (args.keep_mask is None):
        raise ValueError("--known needs exactly one of --keep-classes a,b,c and --keep-mask DIR")
    classes = None
    if args.keep_classes is not None:
        classes = [int(v) for v in args.keep_classes.split(",") if v.strip()]
        if not classes or any(c < 0 or c >= K for c in classes):
            raise ValueError(f"--keep-classes {args.keep_classes}: classes are 0..{K - 1}")
    known = metrics.load_gt(args.known, vids, size, K, prefix="known")
    out = {}
    for vid in vids:
        if classes is not None:
            keep = np.isin(known[vid], classes)
        else:
            path = os.path.join(args.keep_mask, f"keep_{vid:04d}.nii.gz")
            if not os.path.exists(path):
                raise FileNotFoundError(f"{path}: no keep mask for volume {vid}")
            keep = read_nifti(path) != 0
            if tuple(keep.shape) != tuple(size):
                raise ValueError(f"{path}: shape {tuple(keep.shape)}, the run samples {tuple(size)}")
        out[vid] = (known[vid], np.ascontiguousarray(keep.astype(np.uint8)))
    return out


def score_volume(labels: torch.Tensor, gt: torch.Tensor, K: int, ignore, surf):
    """The scores of one volume's S masks against its ground truth: (confusion matrix, ensemble scores or None, the volume's surface
    document -- metrics.case_surface -- or None without --surface).  A seam for the tests: main's only scoring call, so that a test
    without a device can show that no surface op is reached when `surf` is None."""
    cm, scores = metrics.score_case(labels, gt, K)
    return cm, scores, (metrics.case_surface(labels, gt, K, surf, ignore) if surf is not None else None)


def pack_surface(doc: dict) -> torch.Tensor:
    """The five [K] rows of a surface document as fp64 bit patterns (int64 [5 K]); None travels as NaN."""
    rows = [[float("nan") if v is None else v for v in doc[name]] for name in metrics.SURFACE_SCORES]
    return torch.tensor(rows, dtype=torch.float64).reshape(-1).view(torch.int64)


def unpack_surface(bits: torch.Tensor, K: int, classes) -> dict:
    vals = bits.contiguous().view(torch.float64).reshape(len(metrics.SURFACE_SCORES), K).tolist()
    rows = {name: [None if v != v else v for v in row] for name, row in zip(metrics.SURFACE_SCORES, vals)}
    return metrics.mean_surface([rows], classes)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("params_file", nargs="?", default="params_eval.yml")
    ap.add_argument("exp_name", nargs="?", default="local_test")
    ap.add_argument("--size", type=int, nargs=3, default=None, help="D H W of the mask volume (default: yaml input_size or 64 128 128)")
    ap.add_argument("--num-classes", type=int, default=None)
    ap.add_argument("--num-volumes", type=int, default=None, help="volumes to sample (default: yaml batch_size, reference forces 2)")
    ap.add_argument("--steps", type=int, default=None, help="run K evenly spaced reverse steps (reference convention t = 10000+K)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples", type=int, default=1, help="masks per volume, sampled as one batch (pred_VVVV_sJJ.nii.gz; GED / HM-IoU with --gt)")
    ap.add_argument("--gt", default=None, help="directory of gt_{vid:04d}.nii.gz label volumes: score the run into metrics.json")
    ap.add_argument("--ignore-class", type=int, default=None, help="class left out of Dice (default: yaml ignore_class, else 0)")
    ap.add_argument("--loss-t", default=None, help="comma-separated steps t (1..time_steps): KL / CE / loss of the --gt volumes noised to t, into metrics.json")
    ap.add_argument("--known", default=None, help="directory of known_{vid:04d}.nii.gz label volumes: mask editing, with one of the two keep options")
    ap.add_argument("--keep-classes", default=None, help="comma-separated classes: keep the voxels whose known label is listed")
    ap.add_argument("--keep-mask", default=None, help="directory of keep_{vid:04d}.nii.gz volumes, non-zero = keep the known label")
    ap.add_argument("--resample", type=int, default=1, help="repetitions of every step of an edited chain (re-noised one step in between)")
    ap.add_argument("--consensus", action="store_true", help="with --samples S > 1: write the per-voxel vote of the S masks and its entropy")
    postprocess.add_cleanup_arguments(ap)
    metrics.add_surface_arguments(ap)
    args = ap.parse_args(argv)
    if args.resample < 1:
        raise ValueError(f"--resample {args.resample}: at least one repetition per step")
    if args.samples < 1:
        raise ValueError(f"--samples {args.samples}: at least one mask per volume")
    loss_ts = [int(v) for v in args.loss_t.split(",") if v.strip()] if args.loss_t else []
    if loss_ts and not args.gt:
        raise ValueError("--loss-t needs --gt DIR: the objectives are evaluated on the ground-truth volumes")
    set_seeds(1024)
    with open(args.params_file, "r") as f:
        params = yaml.safe_load(f)
    params["batch_size"] = 2 if args.num_volumes is None else args.num_volumes        # ddpm_eval.py:51
    size = tuple(args.size or params.get("input_size") or (64, 128, 128))
    K = args.num_classes or params.get("num_classes", 12)
    rank, local, world = ggd.env_rank_world()
    vids = ggd.shard(params["batch_size"], rank, world)
    S = args.samples
    ignore = args.ignore_class if args.ignore_class is not None else params.get("ignore_class", 0)      # ruijin's get_ignore_class: 0
    gts = metrics.load_gt(args.gt, vids, size, K) if args.gt else None           # a bad ground truth ends the run before any sampling
    edits = load_edit(args, vids, size, K)
    if args.consensus and not 2 <= S <= 64:
        raise ValueError(f"--consensus votes over the masks of a volume: give --samples S with 2 <= S <= 64, got {S}")
    clean_opts = postprocess.cleanup_options(args, K)
    if clean_opts is not None and S > 1 and not args.consensus:
        raise ValueError("--largest-component / --min-component clean ONE mask per volume: with --samples S > 1 give --consensus")
    surf = metrics.surface_options(args)
    if surf is not None and not args.gt:
        raise ValueError("--surface needs --gt DIR: surface distances are measured against the ground-truth volumes")
    if surf is not None and (len(size) != 3 or max(size) > metrics.ops.EDT_MAX_EXTENT):
        raise ValueError(f"--surface: volume {size} has an extent above {metrics.ops.EDT_MAX_EXTENT}, the longest line of the distance transform")
    if any(t < 1 or t > params["time_steps"] for t in loss_ts):
        raise ValueError(f"--loss-t {args.loss_t}: steps are 1..{params['time_steps']}")
    assert torch.cuda.is_available(), "the GuideGen engine needs an MI355X (no CPU fallback)"
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    ggd.init("nccl", dev)
    model = build_from_params(params, size, K).eval()
    load_weights(model, params, log=lambda m: print(f"[rank {rank}] {m}", file=sys.stderr))
    model = model.to(dev)
    # text conditioning (evaluator.py:166-169): the 'selfattn' feature encoder runs over the cached BERT features of the volume;
    # synthetic features here (the hospital reports are private).  The shipped UNet has no SpatialTransformer and ignores the
    # resulting context, exactly as in the reference.
    fce = build_feature_cond_encoder(params)
    if fce is not None:
        path = params.get("load_from")
        sd_fce = None
        if path and os.path.exists(path):
            ck = load_checkpoint(path)
            sd_fce = ck.get("average_feature_cond_encoder", ck.get("feature_cond_encoder"))
        try:
            if sd_fce is not None:      # a DDP / DataParallel-wrapped encoder saves its keys as `module.*` (condition_encoder.py:91-97)
                fce.load_state_dict({(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd_fce.items()})
            else:
                randomize_parameters(fce, 1024, "fce.")
            fce = fce.eval().to(dev)
            feats = torch.randn((1, fce.embed_dim, int(params.get("context_length", 512))), generator=torch.Generator(device=dev).manual_seed(7), device=dev)
            context = fce(feats)        # computed as evaluator.py:166-169 does; the shipped UNet takes no context and ignores it
            print(f"[rank {rank}] feature_cond_encoder context {tuple(context.shape)} (not consumed by the shipped UNet)", file=sys.stderr)
        except RuntimeError as e:       # load_state_dict mismatch (the reference's load would raise, ccdm/ddpm/trainer.py:444-463)
            if getattr(model.unet, "context_dim", None) is not None:
                raise                   # a UNet that consumes the context must not silently run unconditioned
            # the shipped UNet takes no context: the eval does not need the encoder, say so and go on
            print(f"[rank {rank}] WARNING: feature_cond_encoder skipped ({type(e).__name__}: {e})", file=sys.stderr)
    out_dir = args.out or os.path.join(params.get("output_path", "."), args.exp_name)
    os.makedirs(out_dir, exist_ok=True)
    init_t = None if args.steps is None else 10000 + args.steps
    t0 = time.time()
    # scores travel as ONE int64 buffer: the [K, K] counts, then 4 fp64 scores per volume stored as their bit patterns (a volume belongs
    # to one rank and the other ranks hold zeros there, so the integer sum over ranks reproduces the bits)
    n_vol = params["batch_size"]
    L = len(loss_ts)
    loss_at = K * K + 4 * n_vol                                                       # then 3 fp64 (kl, ce, loss) per (volume, listed t)
    score_buf = torch.zeros(loss_at + 3 * L * n_vol, dtype=torch.int64, device=dev) if gts is not None else None
    edit_buf = torch.zeros((n_vol, 2), dtype=torch.int64, device=dev) if edits is not None else None   # (kept voxels, kept voxels != known)
    # the cleaning blocks travel the same way: per volume 3 fp64 consensus means as bit patterns and the two [K, 4] component tables,
    # then the [K, K] counts of the consensus and of the cleaned mask against the ground truth
    post_vol = 3 + 8 * K
    post_buf = torch.zeros(post_vol * n_vol + 2 * K * K, dtype=torch.int64, device=dev) if (args.consensus or clean_opts is not None) else None
    # the surface block travels the same way: per volume the five [K] rows of its scores, then the hd95 rows of the consensus and of the
    # cleaned mask, all as fp64 bit patterns (NaN: no surface distance)
    surf_buf = torch.zeros((n_vol, 7 * K), dtype=torch.int64, device=dev) if surf is not None else None
    for vid in vids:                                                                  # volumes are independent units
        ed = {}
        if edits is not None:                                                         # the S masks of a volume share one known / keep pair
            known, keep = (torch.from_numpy(a).to(dev)[None].expand((S,) + size).contiguous() for a in edits[vid])
            ed = dict(known=known, keep=keep, resample=args.resample)
        if S == 1:
            x_T = uniform_x_T(K, size, [1024 + vid], dev)
            model.philox_seed = 1024 + vid
            labels, _ = model.sample_labels(x_T, torch.zeros((1, 1) + size, device=dev), init_t, **ed)
            write_nifti(os.path.join(out_dir, f"pred_{vid:04d}.nii.gz"), labels[0].to(torch.uint8).cpu().numpy())
        else:                                                                         # the S masks of a volume: one batch, S independent chains
            seeds = [1024 + vid * S + j for j in range(S)]
            x_T = uniform_x_T(K, size, seeds, dev)
            labels, _ = model.sample_labels(x_T, torch.zeros((S, 1) + size, device=dev), init_t, philox_seeds=seeds, **ed)
            host = labels.to(torch.uint8).cpu().numpy()
            for j in range(S):
                write_nifti(os.path.join(out_dir, f"pred_{vid:04d}_s{j:02d}.nii.gz"), host[j])
        if edits is not None:
            kept = ed["keep"] != 0
            edit_buf[vid, 0] = kept[0].sum()
            edit_buf[vid, 1] = (kept & (labels != ed["known"])).sum()
        if post_buf is not None:
            mask = labels[0]
            at = post_vol * vid
            if args.consensus:
                mask, agreement, entropy = postprocess.consensus(labels, K)
                cs = postprocess.consensus_summary(agreement, entropy, S)
                post_buf[at:at + 3] = torch.tensor([cs["mean_entropy"], cs["mean_agreement"], cs["unanimous_fraction"]],
                                                   dtype=torch.float64).view(torch.int64).to(dev)
                write_nifti(os.path.join(out_dir, f"consensus_{vid:04d}.nii.gz"), mask.to(torch.uint8).cpu().numpy())
                write_nifti(os.path.join(out_dir, f"entropy_{vid:04d}.nii.gz"), entropy.cpu().numpy())
                if gts is not None:
                    post_buf[post_vol * n_vol:post_vol * n_vol + K * K] += metrics.confusion_matrix(
                        torch.from_numpy(gts[vid]).to(dev), mask, K).reshape(-1)
                    if surf is not None:
                        sd = metrics.case_surface(mask[None], torch.from_numpy(gts[vid]).to(dev), K, surf, ignore)
                        surf_buf[vid, 5 * K:6 * K] = pack_surface(sd)[K:2 * K].to(dev)
            if clean_opts is not None:
                cleaned, _ = postprocess.clean(mask, K, scores=False, **clean_opts)[:2]
                tables = torch.stack([postprocess.components(m, K, clean_opts["connectivity"])[2][0] for m in (mask, cleaned)])
                post_buf[at + 3:at + post_vol] = tables.reshape(-1)
                write_nifti(os.path.join(out_dir, f"clean_{vid:04d}.nii.gz"), cleaned.to(torch.uint8).cpu().numpy())
                if gts is not None:
                    post_buf[post_vol * n_vol + K * K:] += metrics.confusion_matrix(torch.from_numpy(gts[vid]).to(dev), cleaned, K).reshape(-1)
                    if surf is not None:
                        sd = metrics.case_surface(cleaned[None], torch.from_numpy(gts[vid]).to(dev), K, surf, ignore)
                        surf_buf[vid, 6 * K:] = pack_surface(sd)[K:2 * K].to(dev)
        if gts is not None:
            cm, scores, sd = score_volume(labels, torch.from_numpy(gts[vid]).to(dev), K, ignore, surf)
            score_buf[:K * K] += cm.reshape(-1)
            if sd is not None:
                surf_buf[vid, :5 * K] = pack_surface(sd).to(dev)
            if scores is not None:
                vals = torch.tensor([scores["ged"], scores["diversity_pred"], scores["diversity_gt"], scores["hm_iou"]], dtype=torch.float64)
                score_buf[K * K + 4 * vid:K * K + 4 * vid + 4] = vals.view(torch.int64).to(dev)
            for j, t in enumerate(loss_ts):
                r = ccdm_step_losses(model, torch.from_numpy(gts[vid])[None].to(dev), torch.zeros((1, 1) + size, device=dev), torch.tensor([t]),
                                     philox_seeds=[loss_key(vid, t)])
                at = loss_at + 3 * (vid * L + j)
                score_buf[at:at + 3] = torch.stack([r["loss_kl"], r["loss_ce"], r["loss"]]).view(torch.int64)
    torch.cuda.synchronize()
    print(f"[rank {rank}] sampled {len(vids)} volume(s) of {size} in {time.time() - t0:.1f}s -> {out_dir}", file=sys.stderr)
    post_doc = {}
    if post_buf is not None:
        from .ops import check_component_status
        check_component_status(dev)
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(post_buf)                                    # a volume belongs to one rank, the others hold zeros
        host = post_buf.cpu()
        per_vol = host[:post_vol * n_vol].reshape(n_vol, post_vol)
        voxels = int(np.prod(size))
        if args.consensus:
            means = per_vol[:, :3].contiguous().view(torch.float64)
            post_doc["consensus"] = dict(samples=S, mean_entropy=float(means[:, 0].sum() / n_vol), mean_agreement=float(means[:, 1].sum() / n_vol),
                                         unanimous_fraction=float(means[:, 2].sum() / n_vol),
                                         volumes=[dict(id=v, mean_entropy=float(means[v, 0]), mean_agreement=float(means[v, 1]),
                                                       unanimous_fraction=float(means[v, 2])) for v in range(n_vol)])
        if clean_opts is not None:
            tables = per_vol[:, 3:].reshape(n_vol, 2, K, 4).numpy()
            post_doc["components"] = dict(largest=clean_opts["largest"], min_size=clean_opts["min_size"], connectivity=clean_opts["connectivity"],
                                          volumes=[dict(id=v, before=postprocess.scores_from_stats(tables[v, :1], voxels)[0],
                                                        after=postprocess.scores_from_stats(tables[v, 1:], voxels)[0]) for v in range(n_vol)])
        if gts is not None:
            for j, (name, on) in enumerate((("consensus", args.consensus), ("clean", clean_opts is not None))):
                if on:
                    dice = metrics.dice_coefficient(host[post_vol * n_vol + j * K * K:post_vol * n_vol + (j + 1) * K * K].reshape(K, K), ignore)
                    post_doc[f"dice_{name}"] = [float(v) for v in dice.tolist()]
                    post_doc[f"mean_dice_{name}"] = float(dice.mean())
        if rank == 0 and score_buf is None and edit_buf is None:
            with open(os.path.join(out_dir, "metrics.json"), "w") as f:
                json.dump(post_doc, f, indent=1)
    edit_doc = None
    if edit_buf is not None:
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(edit_buf)                                    # a volume belongs to one rank, the others hold zeros
        voxels = int(np.prod(size))
        edit_doc = dict(resample=args.resample, keep_classes=args.keep_classes, keep_mask=args.keep_mask,
                        volumes=[dict(id=v, kept_fraction=k / voxels, kept_differing=d) for v, (k, d) in enumerate(edit_buf.cpu().tolist())])
        if rank == 0 and score_buf is None:
            with open(os.path.join(out_dir, "metrics.json"), "w") as f:
                json.dump(dict(edit=edit_doc, **post_doc), f, indent=1)
    surf_host = None
    if surf_buf is not None:
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(surf_buf)                                    # a volume belongs to one rank, the others hold zeros
        surf_host = surf_buf.cpu()
    if score_buf is not None:
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(score_buf)                                   # once, after the sampling loop: off the data path
        if rank == 0:
            host = score_buf.cpu()
            per = host[K * K:loss_at].view(torch.float64).reshape(n_vol, 4).tolist()
            volumes = [dict(id=v, samples=S, **(dict(zip(("ged", "diversity_pred", "diversity_gt", "hm_iou"), per[v])) if S > 1 else {}))
                       for v in range(n_vol)]
            doc = metrics.summarise(host[:K * K].reshape(K, K), volumes, K, ignore)
            if L:
                lv = host[loss_at:].view(torch.float64).reshape(n_vol, L, 3)
                mean = lv.sum(0) / n_vol                                              # volume order: the same bits on every run
                doc["loss"] = [dict(t=t, loss_kl=float(mean[j, 0]), loss_ce=float(mean[j, 1]), loss=float(mean[j, 2]), volumes=n_vol)
                               for j, t in enumerate(loss_ts)]
            if edit_doc is not None:
                doc["edit"] = edit_doc
            doc.update(post_doc)
            if surf_host is not None:
                classes = doc["dice_classes"]
                doc["surface"] = metrics.surface_block({v: unpack_surface(surf_host[v, :5 * K], K, classes) for v in range(n_vol)}, K, surf, ignore)
                for j, (name, on) in enumerate((("consensus", args.consensus), ("clean", clean_opts is not None))):
                    if on:                                                        # per class the mean over the volumes that have it (NaN: none)
                        per = surf_host[:, (5 + j) * K:(6 + j) * K].contiguous().view(torch.float64).numpy()
                        hd95 = [[float(v) for v in per[:, c] if v == v] for c in classes]
                        doc[f"hd95_{name}"] = [float(np.mean(v)) if v else None for v in hd95]
                        scored = [v for v in doc[f"hd95_{name}"] if v is not None]
                        doc[f"mean_hd95_{name}"] = float(np.mean(scored)) if scored else None
            with open(os.path.join(out_dir, "metrics.json"), "w") as f:
                json.dump(doc, f, indent=1)
            print(f"[rank 0] {metrics.summary_line(doc)} -> {os.path.join(out_dir, 'metrics.json')}", file=sys.stderr)
    ggd.finalize()


if __name__ == "__main__":
    main(sys.argv[1:])
