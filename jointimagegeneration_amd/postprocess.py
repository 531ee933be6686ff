"""Cleaning sampled masks on the device: the consensus of S samples, connected components, and the keep-largest /
minimum-size filter that stands between the mask stage (S raw samples per volume) and the CT stage (one label volume per patient).

    consensus(labels[S, ...], K)          -> winner, agreement, entropy (nats)
    components(labels, K, ...)            -> root, size, stats (ops.label_components + ops.component_stats)
    component_scores(...)                 -> per class: components, voxels, largest, largest_fraction; stray_voxels / stray_fraction
    clean(labels, K, largest=, min_size=) -> cleaned labels, kept, scores before and after

`python -m jointimagegeneration_amd.postprocess --pred DIR --num-classes K [--samples S] [--largest-component all|a,b,c]
[--min-component V] [--connectivity 6|26] --out DIR` works on the `pred_VVVV[.nii.gz | _sJJ.nii.gz]` volumes ddpm_eval writes.

Every kernel is in gg_components.hip; this module only shapes arguments and reads the small per-class table back.  There is no CPU path.
No counterpart in the reference, which hands a raw sample to the CT stage.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import re
import sys
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from . import ops

CLEAN_OPTIONS = ("largest", "min_size", "connectivity", "background", "fill")


def _volumes(labels: torch.Tensor, K: int, what: str) -> Tuple[torch.Tensor, bool]:
    """[D, H, W] or [B, D, H, W] integer labels on the device -> contiguous int32 [B, D, H, W] (plumbing) and whether a batch axis was
    added.  An int64 label is clamped to [-1, K] first so that no value outside int32 can wrap into the valid range."""
    ops.require_gpu(labels, what)
    if labels.dim() not in (3, 4) or labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
        raise ValueError(f"{what}: labels must be an integer tensor [D, H, W] or [B, D, H, W], got {labels.dtype} {tuple(labels.shape)}")
    single = labels.dim() == 3
    if single:
        labels = labels[None]
    if labels.dtype == torch.int64:
        labels = labels.clamp(-1, K)
    return labels.to(torch.int32).contiguous(), single


def consensus(labels: torch.Tensor, K: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """labels [S, *spatial] on the device -> (winner int32, agreement int32, entropy fp32), each [*spatial]: the most-voted label per
    voxel (ties to the smallest label), its votes, and the entropy in nats of the vote distribution.  A label outside [0, K) raises
    ValueError with its count (reading that count back is the one host sync of the call)."""
    rows = ops._label_rows(labels, K, "consensus")
    winner, agreement, entropy, skipped = ops.label_vote(rows, K)
    n = int(skipped.item())
    if n:
        raise ValueError(f"consensus: {n} vote(s) with a label outside [0, {K})")
    shape = tuple(labels.shape[1:])
    return winner.reshape(shape), agreement.reshape(shape), entropy.reshape(shape)


def consensus_summary(agreement: torch.Tensor, entropy: torch.Tensor, S: int) -> dict:
    """The `consensus` block of metrics.json: samples, mean entropy in nats, mean agreement (votes / S), unanimous fraction; the means
    in fp64 (torch's reductions on the device: plumbing over two small sums)."""
    n = agreement.numel()
    return dict(samples=S, mean_entropy=float(entropy.double().sum()) / n, mean_agreement=float(agreement.double().sum()) / (n * S),
                unanimous_fraction=float((agreement == S).sum()) / n)


def components(labels: torch.Tensor, K: int, connectivity: int = 6, background: int = 0):
    """labels [D, H, W] or [B, D, H, W] -> (root int32 [B, M], size int32 [B, M], stats int64 [B, K, 4]) on the device; see
    ops.label_components and ops.component_stats.  No host sync."""
    vol, _ = _volumes(labels, K, "components")
    root = ops.label_components(vol, K, connectivity, background)
    size, stats = ops.component_stats(vol, root, K)
    return root, size, stats


def scores_from_stats(stats: np.ndarray, voxels: int) -> List[dict]:
    """Per volume of an int64 [B, K, 4] stats table (host): the per-class rows and the volume's stray voxels -- those outside their
    class's largest component -- with the fractions in fp64."""
    out = []
    for vol in np.asarray(stats, dtype=np.int64):
        classes, stray, fg = [], 0, 0
        for c, (n, vox, largest, _root) in enumerate(vol.tolist()):
            classes.append(dict(label=c, components=n, voxels=vox, largest=largest, largest_fraction=(largest / vox) if vox else 1.0))
            stray += vox - largest
            fg += vox
        out.append(dict(classes=classes, stray_voxels=stray, stray_fraction=(stray / fg) if fg else 0.0, foreground_voxels=fg,
                        voxels=int(voxels)))
    return out


def component_scores(labels: torch.Tensor, K: int, connectivity: int = 6, background: int = 0) -> Union[dict, List[dict]]:
    """Scores of a sampled mask that need no ground truth: per class the number of components, its voxels, the largest component and
    its share; per volume the voxels outside their class's largest component (`stray_voxels`, `stray_fraction` of the foreground).
    One dict for [D, H, W] labels, a list for a batch.  Reads the [B, K, 4] table back (the host sync) and checks the status word."""
    vol, single = _volumes(labels, K, "component_scores")
    _, _, stats = components(vol, K, connectivity, background)
    host = stats.cpu().numpy()
    ops.check_component_status(vol.device)
    res = scores_from_stats(host, vol[0].numel())
    return res[0] if single else res


def _policy(K: int, largest, min_size, background: int) -> Tuple[List[int], List[int]]:
    if largest is None:
        keep = []
    elif isinstance(largest, str):
        if largest != "all":
            raise ValueError(f"clean: largest={largest!r}: 'all', a list of classes or None")
        keep = [c for c in range(K) if c != background]
    else:
        keep = [int(c) for c in largest]
        if any(c < 0 or c >= K for c in keep):
            raise ValueError(f"clean: largest={list(largest)}: classes are 0..{K - 1}")
    keep_largest = [1 if c in keep else 0 for c in range(K)]
    if isinstance(min_size, dict):
        if any(int(c) < 0 or int(c) >= K for c in min_size):
            raise ValueError(f"clean: min_size classes {sorted(min_size)}: classes are 0..{K - 1}")
        sizes = [int(min_size.get(c, 0)) for c in range(K)]
    else:
        sizes = [int(min_size)] * K
    if any(v < 0 or v >= 2 ** 31 for v in sizes):
        raise ValueError(f"clean: min_size {min_size}: sizes are 0 .. 2^31 - 1 voxels")
    return keep_largest, sizes


def clean(labels: torch.Tensor, K: int, largest="all", min_size=0, connectivity: int = 6, background: int = 0, fill: Optional[int] = None,
          scores: bool = True):
    """Remove what is not the largest component of a class (`largest`: "all" = every class but the background, a list of classes, or
    None) and every component below `min_size` voxels (an int, or {class: int}); removed voxels become `fill` (default: the
    background).  Returns (cleaned labels int32, kept uint8, scores before, scores after), the first two shaped as `labels`; with
    scores=False the last two are None and nothing is read back (the status word is then the caller's to check)."""
    vol, single = _volumes(labels, K, "clean")
    keep_largest, sizes = _policy(K, largest, min_size, background)
    root, size, stats = components(vol, K, connectivity, background)
    dev = vol.device
    out, kept = ops.component_filter(vol, root, size, stats, K, torch.tensor(keep_largest, dtype=torch.int32).to(dev),
                                     torch.tensor(sizes, dtype=torch.int32).to(dev), background, fill)
    before = after = None
    if scores:
        _, _, stats_after = components(out, K, connectivity, background)
        host = torch.stack([stats, stats_after]).cpu().numpy()
        ops.check_component_status(dev)
        before, after = scores_from_stats(host[0], vol[0].numel()), scores_from_stats(host[1], vol[0].numel())
        if single:
            before, after = before[0], after[0]
    if single:
        out, kept = out[0], kept[0]
    return out, kept, before, after


# ---------------------------------------------------------------------------------------------------------------- command line
def parse_largest(text: Optional[str], K: int):
    """--largest-component: None, "all" or a comma-separated class list -> the `largest` argument of clean()."""
    if text is None:
        return None
    if text.strip() == "all":
        return "all"
    try:
        classes = [int(v) for v in text.split(",") if v.strip()]
    except ValueError:
        raise ValueError(f"--largest-component {text}: 'all' or comma-separated classes") from None
    if not classes or any(c < 0 or c >= K for c in classes):
        raise ValueError(f"--largest-component {text}: classes are 0..{K - 1}")
    return classes


def add_cleanup_arguments(ap: argparse.ArgumentParser) -> None:
    ap.add_argument("--largest-component", default=None, help="'all' or comma-separated classes: keep only the largest component of these classes")
    ap.add_argument("--min-component", type=int, default=None, help="remove every component below this many voxels")
    ap.add_argument("--connectivity", type=int, default=None, help="6 (faces, the default) or 26 (faces, edges, corners)")


def cleanup_options(args, K: int) -> Optional[dict]:
    """The clean() options of the three command-line flags, or None when none of them asks for a cleanup."""
    if args.connectivity is not None and args.connectivity not in (6, 26):
        raise ValueError(f"--connectivity {args.connectivity}: 6 or 26")
    if args.min_component is not None and args.min_component < 0:
        raise ValueError(f"--min-component {args.min_component}: a voxel count")
    if args.largest_component is None and args.min_component is None:
        if args.connectivity is not None:
            raise ValueError("--connectivity needs --largest-component or --min-component")
        return None
    return dict(largest=parse_largest(args.largest_component, K), min_size=args.min_component or 0, connectivity=args.connectivity or 6)


def find_predictions(pred_dir: str, samples: int) -> Dict[int, List[str]]:
    """{vid: [paths]} of pred_VVVV.nii.gz (samples == 1) or pred_VVVV_sJJ.nii.gz, J = 0 .. samples - 1."""
    pat = re.compile(r"pred_(\d{4})\.nii(\.gz)?$" if samples == 1 else r"pred_(\d{4})_s(\d{2})\.nii(\.gz)?$")
    found: Dict[int, Dict[int, str]] = {}
    for path in sorted(glob.glob(os.path.join(pred_dir, "pred_*.nii*"))):
        m = pat.search(os.path.basename(path))
        if m:
            found.setdefault(int(m.group(1)), {})[0 if samples == 1 else int(m.group(2))] = path
    if not found:
        raise FileNotFoundError(f"{pred_dir}: no pred_VVVV{'' if samples == 1 else '_sJJ'}.nii.gz volumes")
    out = {}
    for vid, by in sorted(found.items()):
        if sorted(by) != list(range(samples)):
            raise FileNotFoundError(f"{pred_dir}: volume {vid} has samples {sorted(by)}, --samples {samples} needs 0..{samples - 1}")
        out[vid] = [by[j] for j in range(samples)]
    return out


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--pred", required=True, help="directory of pred_VVVV.nii.gz (or pred_VVVV_sJJ.nii.gz with --samples S) label volumes")
    ap.add_argument("--num-classes", type=int, required=True)
    ap.add_argument("--samples", type=int, default=1, help="masks per volume: their consensus is formed first (consensus_VVVV, entropy_VVVV)")
    add_cleanup_arguments(ap)
    ap.add_argument("--out", required=True)
    return ap


def main(argv=None) -> dict:
    from .io import read_nifti, write_nifti
    args = build_parser().parse_args(argv)
    K, S = args.num_classes, args.samples
    if not 1 <= K <= 32:
        raise ValueError(f"--num-classes {K}: 1..32")
    if not 1 <= S <= 64:
        raise ValueError(f"--samples {S}: 1..64")
    opts = cleanup_options(args, K)
    if opts is None and S == 1:
        raise ValueError("nothing to do: give --samples S > 1 (consensus) and/or --largest-component / --min-component")
    preds = find_predictions(args.pred, S)
    assert torch.cuda.is_available(), "the GuideGen engine needs an MI355X (no CPU fallback)"
    dev = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(args.out, exist_ok=True)
    doc: dict = dict(num_classes=K, samples=S, volumes=[])
    for vid, paths in preds.items():
        vols = [read_nifti(p) for p in paths]
        if any(v.shape != vols[0].shape for v in vols):
            raise ValueError(f"volume {vid}: its samples differ in shape")
        labels = torch.from_numpy(np.stack(vols).astype(np.int32)).to(dev)
        entry: dict = dict(id=vid)
        mask = labels[0]
        if S > 1:
            mask, agreement, entropy = consensus(labels, K)
            entry["consensus"] = consensus_summary(agreement, entropy, S)
            write_nifti(os.path.join(args.out, f"consensus_{vid:04d}.nii.gz"), mask.to(torch.uint8).cpu().numpy())
            write_nifti(os.path.join(args.out, f"entropy_{vid:04d}.nii.gz"), entropy.cpu().numpy())
        if opts is not None:
            cleaned, kept, before, after = clean(mask, K, **opts)
            entry["components"] = dict(before=before, after=after, removed_voxels=int((kept == 0).sum()), **_json_options(opts))
            write_nifti(os.path.join(args.out, f"clean_{vid:04d}.nii.gz"), cleaned.to(torch.uint8).cpu().numpy())
        else:
            entry["components"] = dict(before=component_scores(mask, K))
        doc["volumes"].append(entry)
    with open(os.path.join(args.out, "postprocess.json"), "w") as f:
        json.dump(doc, f, indent=1)
    print(f"postprocess: {len(preds)} volume(s) -> {args.out}", file=sys.stderr)
    return doc


def _json_options(opts: dict) -> dict:
    return dict(largest=opts.get("largest", "all"), min_size=opts.get("min_size", 0), connectivity=opts.get("connectivity", 6))


if __name__ == "__main__":
    main(sys.argv[1:])
