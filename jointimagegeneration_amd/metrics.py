"""Scores of sampled masks: confusion matrix, Dice, generalised energy distance (GED) and Hungarian-matched IoU (HM-IoU).

What the reference's evaluation run reports besides the volumes: ccdm/ddpm/evaluator.py:188-190 attaches ignite's `ConfusionMatrix` and
`DiceCoefficient(cm, ignore_index=ignore_class)`; ccdm/ddpm/utils.py:190-236 holds the ensemble scores (`iou`, `batched_distance`,
`calc_batched_generalised_energy_distance`, `batched_hungarian_matching`).  Every one of them is a function of pairwise K x K confusion
matrices, which are exact integer counts: `ops.label_confusion` (gg_label_confusion, one HIP kernel) takes them in one pass over labels
that are already on the device, and the rest is fp64 arithmetic on tiny tensors, on whatever device the counts are on.  The reference's
own form builds a boolean [B, S0, S1, M, K] array (about 4 GB for 12 x 12 samples of a 128^3, 14-class mask).

    python -m jointimagegeneration_amd.metrics --pred DIR --gt DIR --num-classes K [--ignore-class C] [--out FILE]

scores `pred_{vid:04d}.nii.gz` / `pred_{vid:04d}_s{j:02d}.nii.gz` against `gt_{vid:04d}.nii.gz`, as `ddpm_eval --gt` does while it samples.
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


def summarise(cm: torch.Tensor, volumes: List[dict], K: int, ignore_class: Optional[int]) -> dict:
    """The metrics.json document: the raw integer matrix, Dice per class (the ignored class removed) and its mean, per-volume scores."""
    dice = dice_coefficient(cm, ignore_class)
    return dict(num_classes=K, ignore_class=ignore_class, confusion_matrix=[[int(v) for v in row] for row in cm.cpu().tolist()],
                dice_classes=[c for c in range(K) if c != ignore_class], dice=[float(v) for v in dice.cpu().tolist()],
                mean_dice=float(dice.mean()), volumes=volumes)


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
    args = ap.parse_args(argv)
    K = args.num_classes
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
    for vid in sorted(cases):
        pred = np.stack([read_nifti(p) for p in cases[vid]])
        if tuple(pred.shape[1:]) != tuple(gts[vid].shape):
            raise ValueError(f"volume {vid}: prediction {tuple(pred.shape[1:])} and ground truth {tuple(gts[vid].shape)} differ in shape")
        c, scores = score_case(torch.from_numpy(pred.astype(np.int32)).to(dev), torch.from_numpy(gts[vid]).to(dev), K)
        cm += c
        volumes.append(dict(id=vid, samples=len(cases[vid]), **(scores or {})))
    doc = summarise(cm, volumes, K, args.ignore_class)
    out = args.out or os.path.join(args.pred, "metrics.json")
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(f"{summary_line(doc)} -> {out}", file=sys.stderr)
    return doc


if __name__ == "__main__":
    main(sys.argv[1:])
