"""Scores of sampled masks: confusion matrix, Dice, generalised energy distance (GED) and Hungarian-matched IoU (HM-IoU).

What the reference's evaluation run reports besides the volumes: ccdm/ddpm/evaluator.py:188-190 attaches ignite's `ConfusionMatrix` and
`DiceCoefficient(cm, ignore_index=ignore_class)`; ccdm/ddpm/utils.py:190-236 holds the ensemble scores (`iou`, `batched_distance`,
`calc_batched_generalised_energy_distance`, `batched_hungarian_matching`).  Every one of them is a function of pairwise K x K confusion
matrices, which are exact integer counts: `ops.label_confusion` (gg_label_confusion, one HIP kernel) takes them in one pass over labels
that are already on the device, and the rest is fp64 arithmetic on tiny tensors, on whatever device the counts are on.  The reference's
own form builds a boolean [B, S0, S1, M, K] array (about 4 GB for 12 x 12 samples of a 128^3, 14-class mask).

    python -m jointimagegeneration_amd.metrics --pred DIR --gt DIR --num-classes K [--ignore-class C] [--out FILE]
                                              [--surface [--spacing d,h,w] [--surface-connectivity 1|2|3]]

scores `pred_{vid:04d}.nii.gz` / `pred_{vid:04d}_s{j:02d}.nii.gz` against `gt_{vid:04d}.nii.gz`, as `ddpm_eval --gt` does while it samples.

Surface distances: `surface_distances` gives Hausdorff distance, its 95th percentile and the average (symmetric) surface
distances per volume and class, by the definitions of `medpy.metric.binary` (hd, hd95, asd, assd) -- the module the reference's
evaluator imports dc / precision / recall from (ccdm/ddpm/evaluator.py).  Borders, the exact distance transform and the per-volume
count / sum / maximum are HIP kernels (`ops.label_border`, `ops.edt_squared`, `ops.surface_reduce`); `--surface` adds them to the document.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import re
import sys
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import ops
from .io import read_nifti


# ------------------------------------------------------------------------------------------------ counts (device)
def confusion_matrix(y: torch.Tensor, y_pred: torch.Tensor, K: int) -> torch.Tensor:
    """int64 [K, K], rows = ground truth, columns = prediction, summed over the batch (ignite's ConfusionMatrix convention).
    y, y_pred: integer label tensors of one shape [B, *spatial] on the device (labels, not class scores)."""
    if tuple(y.shape) != tuple(y_pred.shape):
        raise ValueError(f"confusion_matrix: y {tuple(y.shape)} and y_pred {tuple(y_pred.shape)} differ in shape")
    return ops.label_confusion(y.reshape(1, -1), y_pred.reshape(1, -1), K)[0, 0]


# ------------------------------------------------------------------------------------------------ fp64 formulas (any device)
def dice_coefficient(cm: torch.Tensor, ignore_index: Optional[int] = None) -> torch.Tensor:
    """Per-class Dice 2 * diag / (cm.sum(1) + cm.sum(0) + 1e-15) in fp64, with the `ignore_index` entry removed: ignite's
    `DiceCoefficient` as its source defines it.  (ignite is not a dependency: the tests check this against the same formula in numpy,
    not against an ignite run.)"""
    if cm.dim() != 2 or cm.shape[0] != cm.shape[1]:
        raise ValueError(f"dice_coefficient: a [K, K] confusion matrix, got {tuple(cm.shape)}")
    K = cm.shape[0]
    if ignore_index is not None and not (isinstance(ignore_index, int) and 0 <= ignore_index < K):
        raise ValueError(f"dice_coefficient: ignore_index={ignore_index!r} must be an integer in [0, {K})")
    c = cm.to(torch.float64)
    dice = 2.0 * c.diagonal() / (c.sum(1) + c.sum(0) + 1e-15)
    if ignore_index is None:
        return dice
    return torch.cat([dice[:ignore_index], dice[ignore_index + 1:]])


def precision_recall(cm: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-class (precision, recall) in fp64 from a [K, K] confusion matrix with rows = ground truth and columns = prediction:
    tp / (tp + fp) and tp / (tp + fn), medpy.metric.binary's `precision` / `recall` of the mask of each class, 0.0 where the
    denominator is 0 (medpy's ZeroDivisionError branch)."""
    if cm.dim() != 2 or cm.shape[0] != cm.shape[1]:
        raise ValueError(f"precision_recall: a [K, K] confusion matrix, got {tuple(cm.shape)}")
    c = cm.to(torch.float64)
    tp = c.diagonal()
    predicted, actual = c.sum(0), c.sum(1)
    zero = torch.zeros_like(tp)
    return (torch.where(predicted > 0, tp / predicted.clamp(min=1.0), zero), torch.where(actual > 0, tp / actual.clamp(min=1.0), zero))


def iou_distance(cm_pairs: torch.Tensor) -> torch.Tensor:
    """[..., K, K] confusion matrices -> [...] distances 1 - mean over classes 1..K-1 of the per-class IoU, class 0 left out and
    0 / 0 -> 1 (a class absent from both volumes agrees): `batched_distance` of ccdm/ddpm/utils.py:190-203."""
    c = cm_pairs.to(torch.float64)
    inter = c.diagonal(dim1=-2, dim2=-1)
    union = c.sum(-1) + c.sum(-2) - inter
    iou = torch.where(union == 0, torch.ones_like(inter), inter / union)
    return 1.0 - iou[..., 1:].mean(-1)


def energy_distance_from_confusion(cm_01: torch.Tensor, cm_00: torch.Tensor, cm_11: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(ged, diversity_0, diversity_1) from the cross [S0, S1, K, K] and the two self [S, S, K, K] confusion matrices:
    ged = 2 mean(d01) - mean(d00) - mean(d11), means over all pairs, the diagonal included (ccdm/ddpm/utils.py:206-218)."""
    cross = iou_distance(cm_01).mean()
    d0 = iou_distance(cm_00).mean()
    d1 = iou_distance(cm_11).mean()
    return 2.0 * cross - d0 - d1, d0, d1


def hungarian_iou_from_confusion(cm_01: torch.Tensor) -> float:
    """Mean of 1 - cost over the optimal assignment of the cost matrix iou_distance(cm_01) (ccdm/ddpm/utils.py:221-236).  The matched
    mean is unique even where the assignment is not."""
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError as e:
        raise ImportError("hungarian_iou needs scipy (scipy.optimize.linear_sum_assignment), which is not installed") from e
    cost = iou_distance(cm_01).cpu().numpy()
    rows, cols = linear_sum_assignment(cost)
    return float((1.0 - cost)[rows, cols].mean())


# ------------------------------------------------------------------------------------------------ ensemble scores (device)
def generalised_energy_distance(labels_0: torch.Tensor, labels_1: torch.Tensor, K: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(ged, diversity_0, diversity_1) of two sets of label volumes [S0, *spatial] and [S1, *spatial] of one case, fp64 scalars on the
    device: three label_confusion calls (cross and the two self sets), then energy_distance_from_confusion."""
    return energy_distance_from_confusion(ops.label_confusion(labels_0, labels_1, K), ops.label_confusion(labels_0, labels_0, K),
                                          ops.label_confusion(labels_1, labels_1, K))


def hungarian_iou(labels_0: torch.Tensor, labels_1: torch.Tensor, K: int) -> float:
    """HM-IoU of two sets of label volumes of one case (batched_hungarian_matching for that case)."""
    return hungarian_iou_from_confusion(ops.label_confusion(labels_0, labels_1, K))


# ------------------------------------------------------------------------------------------------ surface distances (device)
SURFACE_SCORES = ("hd", "hd95", "asd_pred_to_gt", "asd_gt_to_pred", "assd")


def _surface_labels(t: torch.Tensor, K: int, name: str) -> torch.Tensor:
    ops.require_gpu(t, "surface_distances")
    if t.dim() != 4 or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"surface_distances: {name} must be an integer label tensor [B, D, H, W], got {t.dtype} {tuple(t.shape)}")
    if t.dtype == torch.int64:
        t = t.clamp(-1, K)                                         # no value outside int32 can wrap into the valid range
    return t.to(torch.int32).contiguous()


def percentile_of_sorted_squares(read, n: int, q: float = 95.0) -> float:
    """np.percentile(sqrt(values), q) with numpy's default linear interpolation, from the ascending SQUARED values: `read(i)` returns
    the i-th of the n.  The two neighbouring order statistics are read, rooted and interpolated in fp64 on the host, in numpy's own
    arithmetic (virtual index (n - 1) * (q / 100); a + (b - a) * t, taken from b's side once t >= 0.5)."""
    virtual = (n - 1) * (q / 100.0)
    lo = int(np.floor(virtual))
    t = virtual - lo
    lo = min(max(lo, 0), n - 1)
    hi = min(lo + 1, n - 1)
    a, b = float(np.sqrt(read(lo))), float(np.sqrt(read(hi)))
    diff = b - a
    return b - diff * (1.0 - t) if t >= 0.5 else a + diff * t


def surface_distances(pred: torch.Tensor, gt: torch.Tensor, K: int, spacing=(1.0, 1.0, 1.0), connectivity: int = 1,
                      ignore_index: Optional[int] = None) -> dict:
    """Surface distances of label volumes pred, gt [B, D, H, W] on the device, per volume and class, by medpy.metric.binary's definitions.
    With sds(a, b) = edt(~border_b)[border_a], the distances from a's surface voxels to b's surface under `spacing` (d, h, w):
        hd = max(max sds(pred, gt), max sds(gt, pred)),      hd95 = np.percentile(hstack(sds(pred, gt), sds(gt, pred)), 95),
        asd_pred_to_gt = mean sds(pred, gt),  asd_gt_to_pred = mean sds(gt, pred),  assd = their mean.
    Returns {classes, hd, hd95, asd_pred_to_gt, asd_gt_to_pred, assd: [B][K] floats, None for a class absent from either volume (medpy
    raises there) and for `ignore_index`; absent: [B] lists of such classes (ignore_index not among them); mean: [B] dicts of the class
    means over the scored classes (None when there is none)}.
    One class and one direction at a time: two fp64 volumes (the transform and its workspace) and dist2 are alive, not K of them."""
    K = int(K)
    if not 1 <= K <= 32:
        raise ValueError(f"surface_distances: K={K} outside [1, 32]")
    if ignore_index is not None and not (isinstance(ignore_index, int) and 0 <= ignore_index < K):
        raise ValueError(f"surface_distances: ignore_index={ignore_index!r} must be an integer in [0, {K})")
    if tuple(pred.shape) != tuple(gt.shape) or pred.device != gt.device:
        raise ValueError(f"surface_distances: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape (or lie on two devices)")
    vols = {"pred": _surface_labels(pred, K, "pred"), "gt": _surface_labels(gt, K, "gt")}
    B, M = int(pred.shape[0]), int(pred[0].numel())
    borders = {name: ops.label_border(v, K, connectivity) for name, v in vols.items()}
    dev = vols["pred"].device
    sq = torch.empty((B, M), dtype=torch.float64, device=dev)
    ws = torch.empty((B, M), dtype=torch.float64, device=dev)
    dist2 = torch.empty((B, M), dtype=torch.float64, device=dev)
    classes = [c for c in range(K) if c != ignore_index]
    out = {name: [[None] * K for _ in range(B)] for name in SURFACE_SCORES}
    absent: List[List[int]] = [[] for _ in range(B)]
    for c in classes:
        members, stats = {}, {}
        for a, b in (("pred", "gt"), ("gt", "pred")):              # the surface voxels of a, their distances to the surface of b
            ops.edt_squared(vols[b], borders[b], c, spacing, out=sq, workspace=ws)
            _, st = ops.surface_reduce(vols[a], borders[a], sq, c, out=dist2)
            stats[a] = st.cpu()
            members[a] = dist2[dist2 >= 0].split([int(n) for n in stats[a][:, 0].tolist()])
        for v in range(B):
            (n_p, sum_p, max_p), (n_g, sum_g, max_g) = stats["pred"][v].tolist(), stats["gt"][v].tolist()
            if n_p == 0 or n_g == 0:                               # a class has a border voxel wherever it has a voxel
                absent[v].append(c)
                continue
            pooled = torch.sort(torch.cat([members["pred"][v], members["gt"][v]])).values
            out["hd"][v][c] = float(np.sqrt(max(max_p, max_g)))
            out["hd95"][v][c] = percentile_of_sorted_squares(lambda i: float(pooled[i]), int(pooled.numel()))
            out["asd_pred_to_gt"][v][c] = sum_p / n_p
            out["asd_gt_to_pred"][v][c] = sum_g / n_g
            out["assd"][v][c] = float(np.mean((sum_p / n_p, sum_g / n_g)))
    mean = []
    for v in range(B):
        scored = [c for c in classes if c not in absent[v]]
        mean.append({name: (float(np.mean([out[name][v][c] for c in scored])) if scored else None) for name in SURFACE_SCORES})
    return dict(classes=classes, absent=absent, mean=mean, **out)


def surface_options(args) -> Optional[dict]:
    """The keyword arguments of surface_distances from --surface / --spacing / --surface-connectivity; None without --surface.  A bad
    value is a ValueError on the host, before anything is sampled or launched."""
    if not args.surface:
        if args.spacing is not None or args.surface_connectivity is not None:
            raise ValueError("--spacing / --surface-connectivity belong to the surface distances: give --surface")
        return None
    spacing = (1.0, 1.0, 1.0)
    if args.spacing is not None:
        try:
            spacing = tuple(float(v) for v in args.spacing.split(","))
        except ValueError:
            spacing = ()
        if len(spacing) != 3 or not all(np.isfinite(v) and v > 0 for v in spacing):
            raise ValueError(f"--spacing {args.spacing}: three comma-separated values > 0 (d,h,w)")
    conn = 1 if args.surface_connectivity is None else args.surface_connectivity
    if conn not in (1, 2, 3):
        raise ValueError(f"--surface-connectivity {conn}: 1 (faces), 2 (and edges) or 3 (and corners)")
    return dict(spacing=spacing, connectivity=conn)


def add_surface_arguments(ap: argparse.ArgumentParser) -> None:
    ap.add_argument("--surface", action="store_true", help="with --gt: HD, HD95 and the average surface distances per class (a `surface` block)")
    ap.add_argument("--spacing", default=None, help="voxel spacing d,h,w of the surface distances (default 1,1,1: voxel units)")
    ap.add_argument("--surface-connectivity", type=int, default=None, help="1 (faces, default), 2 (and edges), 3 (and corners): what makes a border voxel")


def mean_surface(rows: List[dict], classes: List[int]) -> dict:
    """The mean of several {score: [K] values or None} rows (the S samples of a case, or the volumes of a run): per score and class the
    mean over the rows that have it, None where none has; `absent`: the classes of `classes` that no row scores; `mean`: the class
    means of the per-class values."""
    K = len(rows[0]["hd"])
    doc = {}
    for name in SURFACE_SCORES:
        vals = [[r[name][c] for r in rows if r[name][c] is not None] for c in range(K)]
        doc[name] = [float(np.mean(v)) if v else None for v in vals]
    scored = [c for c in classes if doc["hd"][c] is not None]
    doc["absent"] = [c for c in classes if c not in scored]
    doc["mean"] = {name: (float(np.mean([doc[name][c] for c in scored])) if scored else None) for name in SURFACE_SCORES}
    return doc


def surface_block(per_volume: Dict[int, dict], K: int, options: dict, ignore_class: Optional[int]) -> dict:
    """The `surface` block of metrics.json from the mean_surface document of every volume id: the five scores per class and the class
    means over the run, `absent`, the options, and the per-volume documents."""
    classes = [c for c in range(K) if c != ignore_class]
    return dict(spacing=list(options["spacing"]), connectivity=options["connectivity"], classes=classes,
                **mean_surface([per_volume[v] for v in sorted(per_volume)], classes),
                volumes=[dict(id=v, **per_volume[v]) for v in sorted(per_volume)])


# ------------------------------------------------------------------------------------------------ what the entry points report
def load_gt(gt_dir: str, vids, size, K: int, prefix: str = "gt") -> Dict[int, np.ndarray]:
    """gt_{vid:04d}.nii.gz of every volume id -> int32 [D, H, W].  A volume of another shape, or with a label outside [0, K), is a
    ValueError (host-side: nothing has been sampled yet).  prefix: the file stem of another set of label volumes ("known")."""
    out = {}
    for vid in vids:
        path = os.path.join(gt_dir, f"{prefix}_{vid:04d}.nii.gz")
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path}: no {'ground truth' if prefix == 'gt' else prefix + ' label volume'} for volume {vid}")
        arr = read_nifti(path)
        if size is not None and tuple(arr.shape) != tuple(size):
            raise ValueError(f"{path}: shape {tuple(arr.shape)}, the run samples {tuple(size)}")
        if arr.dtype.kind not in "iu":
            if not np.array_equal(arr, np.round(arr)):
                raise ValueError(f"{path}: not a label volume ({arr.dtype} with fractional values)")
        lo, hi = int(arr.min()), int(arr.max())
        if lo < 0 or hi >= K:
            raise ValueError(f"{path}: labels in [{lo}, {hi}], the run has {K} classes (labels must lie in [0, {K}))")
        out[vid] = np.ascontiguousarray(arr.astype(np.int32))
    return out


def score_case(pred: torch.Tensor, gt: torch.Tensor, K: int) -> Tuple[torch.Tensor, Optional[dict]]:
    """pred int [S, *spatial], gt int [*spatial] on the device -> (int64 [K, K] confusion matrix, rows = ground truth, summed over the S
    samples; with S > 1 the case's ensemble scores {ged, diversity_pred, diversity_gt, hm_iou} against the one ground truth)."""
    gt1 = gt.reshape((1,) + tuple(pred.shape[1:]))
    cross = ops.label_confusion(gt1, pred, K)                      # [1, S, K, K]: rows = ground truth
    cm = cross[0].sum(0)
    if pred.shape[0] < 2:
        return cm, None
    cm_01 = cross.permute(1, 0, 3, 2).contiguous()                 # [S, 1, K, K] samples x ground truth (the scores are symmetric anyway)
    ged, d0, d1 = energy_distance_from_confusion(cm_01, ops.label_confusion(pred, pred, K), ops.label_confusion(gt1, gt1, K))
    return cm, dict(ged=float(ged), diversity_pred=float(d0), diversity_gt=float(d1), hm_iou=hungarian_iou_from_confusion(cm_01))


def case_surface(pred: torch.Tensor, gt: torch.Tensor, K: int, options: dict, ignore_class: Optional[int]) -> dict:
    """pred int [S, D, H, W], gt int [D, H, W] on the device -> the mean_surface document of the case: every sample against the one
    ground truth, one sample at a time (the memory of one volume), then the mean over the S samples."""
    if pred.dim() != 4 or gt.dim() != 3:
        raise ValueError(f"surface distances need volumes [D, H, W]: prediction {tuple(pred.shape[1:])}, ground truth {tuple(gt.shape)}")
    rows = []
    for j in range(pred.shape[0]):
        r = surface_distances(pred[j:j + 1], gt[None], K, ignore_index=ignore_class, **options)
        rows.append({name: r[name][0] for name in SURFACE_SCORES})
    return mean_surface(rows, [c for c in range(K) if c != ignore_class])


def summarise(cm: torch.Tensor, volumes: List[dict], K: int, ignore_class: Optional[int]) -> dict:
    """The metrics.json document: the raw integer matrix, Dice per class (the ignored class removed) and its mean, precision and recall
    per class (the same classes), per-volume scores."""
    dice = dice_coefficient(cm, ignore_class)
    precision, recall = (torch.cat([v[:ignore_class], v[ignore_class + 1:]]) if ignore_class is not None else v for v in precision_recall(cm))
    return dict(num_classes=K, ignore_class=ignore_class, confusion_matrix=[[int(v) for v in row] for row in cm.cpu().tolist()],
                dice_classes=[c for c in range(K) if c != ignore_class], dice=[float(v) for v in dice.cpu().tolist()],
                mean_dice=float(dice.mean()), precision=[float(v) for v in precision.cpu().tolist()],
                recall=[float(v) for v in recall.cpu().tolist()], volumes=volumes)


def summary_line(doc: dict) -> str:
    s = f"mean Dice {doc['mean_dice']:.4f} over {len(doc['dice'])} classes (ignore_class={doc['ignore_class']})"
    vols = [v for v in doc["volumes"] if "ged" in v]
    if vols:
        s += f", GED {np.mean([v['ged'] for v in vols]):.4f}, HM-IoU {np.mean([v['hm_iou'] for v in vols]):.4f} over {len(vols)} volume(s)"
    return s


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description="score pred_*.nii.gz against gt_*.nii.gz: confusion matrix, Dice, GED, HM-IoU")
    ap.add_argument("--pred", required=True, help="directory of pred_{vid:04d}.nii.gz or pred_{vid:04d}_s{j:02d}.nii.gz")
    ap.add_argument("--gt", required=True, help="directory of gt_{vid:04d}.nii.gz")
    ap.add_argument("--num-classes", type=int, required=True)
    ap.add_argument("--ignore-class", type=int, default=0)
    ap.add_argument("--out", default=None, help="metrics.json path (default: PRED/metrics.json)")
    add_surface_arguments(ap)
    args = ap.parse_args(argv)
    K = args.num_classes
    surf = surface_options(args)
    cases: Dict[int, List[str]] = {}
    for path in sorted(glob.glob(os.path.join(args.pred, "pred_*.nii.gz"))):
        m = re.fullmatch(r"pred_(\d{4,})(?:_s(\d{2,}))?\.nii\.gz", os.path.basename(path))
        if m:
            cases.setdefault(int(m.group(1)), []).append(path)
    if not cases:
        raise FileNotFoundError(f"{args.pred}: no pred_*.nii.gz volumes")
    gts = {}
    for vid in sorted(cases):                                      # every ground truth is checked before the first launch
        gts.update(load_gt(args.gt, [vid], None, K))
    assert torch.cuda.is_available(), "the GuideGen engine needs an MI355X (no CPU fallback)"
    dev = torch.device("cuda", 0)
    cm = torch.zeros((K, K), dtype=torch.int64, device=dev)
    volumes = []
    surfaces = {}
    for vid in sorted(cases):
        pred = np.stack([read_nifti(p) for p in cases[vid]])
        if tuple(pred.shape[1:]) != tuple(gts[vid].shape):
            raise ValueError(f"volume {vid}: prediction {tuple(pred.shape[1:])} and ground truth {tuple(gts[vid].shape)} differ in shape")
        pred_dev, gt_dev = torch.from_numpy(pred.astype(np.int32)).to(dev), torch.from_numpy(gts[vid]).to(dev)
        c, scores = score_case(pred_dev, gt_dev, K)
        cm += c
        volumes.append(dict(id=vid, samples=len(cases[vid]), **(scores or {})))
        if surf is not None:
            surfaces[vid] = case_surface(pred_dev, gt_dev, K, surf, args.ignore_class)
    doc = summarise(cm, volumes, K, args.ignore_class)
    if surf is not None:
        doc["surface"] = surface_block(surfaces, K, surf, args.ignore_class)
    out = args.out or os.path.join(args.pred, "metrics.json")
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(f"{summary_line(doc)} -> {out}", file=sys.stderr)
    return doc


if __name__ == "__main__":
    main(sys.argv[1:])
