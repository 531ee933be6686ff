"""Cost of CCDM mask editing on the full-size chain: the shipped CCDM UNet, 128^3 voxels, K = 14, 250 reverse steps, Philox mode with the
captured step, with and without a mask (known = a synthetic organ volume, keep = about half of its classes).

    python tools/bench_ccdm_edit.py [--steps 250] [--size 128] [--rounds 3]

After a warm-up of both configurations (weight repack, short chains) whole chains ALTERNATE for --rounds rounds, each timed alone with
device events around the whole `sample_labels` call (DESIGN.md section 5 times chains the same way; the call includes its own graph
capture).  Prints one JSON line: median, min and max per configuration, the median per-round difference per step, and the count of kept
voxels that differ from known (0).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from jointimagegeneration_amd.pipeline import build_ccdm  # noqa: E402


def organ_volume(n: int, K: int) -> np.ndarray:
    """Nested ellipsoids, labels 0..K-1 (integer / fp64 numpy only)."""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    lab = np.zeros((n, n, n), dtype=np.int32)
    rs = np.random.RandomState(0)
    for k in range(1, K):
        c = rs.uniform(0.3, 0.7, 3) * n
        r = rs.uniform(0.08, 0.3, 3) * n + 1
        lab[((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 <= 1.0] = k
    return lab


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    K, n = 14, args.size
    m = build_ccdm(K, args.steps, 1024, dev)
    size = (n, n, n)
    x_T = torch.randint(0, K, (1,) + size, generator=torch.Generator(device=dev).manual_seed(7), device=dev, dtype=torch.int32)
    cond = torch.zeros((1, 1) + size, device=dev)
    known = torch.from_numpy(organ_volume(n, K))[None].to(dev)
    keep = (known % 2 == 0)                                      # the background and every second organ
    edit = dict(known=known, keep=keep)

    def chain(init_t=None, **kw):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        lab, _ = m.sample_labels(x_T, cond, init_t, **kw)
        b.record()
        b.synchronize()
        return a.elapsed_time(b), lab

    for kw in ({}, edit):                                         # warm-up: repack, allocator, a short captured chain each
        chain(10005, **kw)
    t = {"mask_free": [], "masked": []}
    differing = None
    for r in range(args.rounds):
        for name in (("mask_free", "masked") if r % 2 == 0 else ("masked", "mask_free")):
            ms, lab = chain(None, **(edit if name == "masked" else {}))
            t[name].append(ms)
            if name == "masked":
                differing = int((keep & (lab != known)).sum())
    diff = [b - a for a, b in zip(t["mask_free"], t["masked"])]
    res = {"size": n, "steps": args.steps, "rounds": args.rounds, "kept_fraction": round(float(keep.float().mean()), 4),
           "kept_differing": differing}
    for name, v in t.items():
        res[name] = {"median_ms": round(statistics.median(v), 1), "min_ms": round(min(v), 1), "max_ms": round(max(v), 1)}
    res["overhead_median_ms"] = round(statistics.median(diff), 1)
    res["overhead_per_step_us"] = round(1000.0 * statistics.median(diff) / args.steps, 1)
    res["overhead_fraction"] = round(statistics.median(diff) / statistics.median(t["mask_free"]), 5)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
