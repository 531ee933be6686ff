"""Cost of rendering a sampled (CT, mask) volume: organ overlay (gg_mask_overlay) plus slice grid (gg_make_grid_u8) on the device,
against the host restatement tests/render_ref.py (numpy / torch on the CPU, the work a user would otherwise do after copying the
volume back), in the same process.

    python tools/bench_render.py [--sizes 64x512x512 256x512x512] [--rounds 15] [--inner 5] [--host-repeats 1]

Input: synth.synth_mask_volume's nested ellipsoids (labels 0..11, mostly uniform tiles, as an organ mask is) and a random CT.  The
device side is warmed up, then timed between device events, `--inner` calls per window, `--rounds` windows; the two kernels are also
timed apart.  The host side is timed with a wall clock, `--host-repeats` times (it takes seconds to minutes).  The two pictures are
checked equal byte for byte before anything is timed.  `min_bytes` is what any implementation must move: 8 B read and 12 B written per
voxel by the overlay, 12 B read per voxel and 3 B written per pixel by the grid.  Prints one JSON line per size.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import render_ref as R  # noqa: E402
from jointimagegeneration_amd import ops  # noqa: E402
from jointimagegeneration_amd.synth import synth_mask_volume  # noqa: E402


def timed_ms(fn, calls: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", nargs="+", default=["64x512x512", "256x512x512"])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_render measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    for size in args.sizes:
        D, H, W = (int(v) for v in size.split("x"))
        lab = synth_mask_volume(D, H, W)
        ct = torch.rand((D, H, W), generator=torch.Generator().manual_seed(1))
        x = torch.stack([ct, lab.float() / 11]).contiguous()
        xd = x[None].to(dev)
        over = torch.empty((1, D, 3, H, W), dtype=torch.float32, device=dev)
        Hg, Wg = ops.make_grid_extent(D, H, W, 8, 5)
        pic = torch.empty((Hg, Wg, 3), dtype=torch.uint8, device=dev)

        def overlay():
            ops.mask_overlay(xd, R.COLORS, 0.2, out=over)

        def grid():
            ops.make_grid_u8(over[0], nrow=8, padding=5, out=pic)

        def both():
            overlay()
            grid()

        host_s = []
        for _ in range(args.host_repeats):
            t0 = time.perf_counter()
            want = R.volume_image(x)
            host_s.append(time.perf_counter() - t0)
        for _ in range(3):                                   # warm-up, and the check
            both()
        torch.cuda.synchronize()
        assert np.array_equal(pic.cpu().numpy(), want), f"{size}: the device picture differs from the host restatement"
        t = {"overlay": [], "grid": [], "both": []}
        fns = {"overlay": overlay, "grid": grid, "both": both}
        keys = list(fns)
        for r in range(args.rounds):
            for key in (keys if r % 2 == 0 else keys[::-1]):
                t[key].append(timed_ms(fns[key], args.inner))
        vox = D * H * W
        res = {"size": size, "voxels": vox, "picture": [Hg, Wg], "rounds": args.rounds, "inner": args.inner,
               "background_fraction": round(float((lab == 0).float().mean()), 4)}
        for key, v in t.items():
            res[f"device_{key}_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        res["host_render_ref_s"] = {"median": round(statistics.median(host_s), 3), "min": round(min(host_s), 3), "repeats": len(host_s)}
        res["host_over_device"] = round(statistics.median(host_s) * 1e3 / statistics.median(t["both"]), 1)
        res["min_bytes"] = {"overlay": 20 * vox, "grid": 12 * vox + 3 * Hg * Wg}
        res["overlay_TBps"] = round(20 * vox / (statistics.median(t["overlay"]) * 1e-3) / 1e12, 3)
        res["grid_TBps"] = round((12 * vox + 3 * Hg * Wg) / (statistics.median(t["grid"]) * 1e-3) / 1e12, 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
