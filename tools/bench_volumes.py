"""Timed throughput of whole C5 volumes, B independent volumes per batch (GuideGenPipeline.run_volumes) against B = 1, in one process.

    python tools/bench_volumes.py [--batch 8] [--ccdm-steps 250] [--ddim-steps 50] [--depth 256] [--hw 512]

Each batch size gets one untimed warm-up batch on the same shapes (5 CCDM steps, 3 slices: weight repacks, graph capture), then one
timed batch of whole volumes (128^3 mask, the full CCDM chain, every slice of the window x S DDIM steps), synchronised at the end.
voxels/s counts, per volume, the mask (D*H*W) and the CT volume (depth*hw*hw), as bench.py does.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from jointimagegeneration_amd.pipeline import GuideGenPipeline, build_ccdm, build_ldm  # noqa: E402


def timed_batch(pipe: GuideGenPipeline, B: int, args) -> dict:
    seeds = [args.seed + 1000 * i for i in range(B)]
    size = tuple(args.mask_size)
    pipe.run_volumes(seeds, size, args.depth, args.hw, ccdm_init_t=10005, max_slices=3)            # warm-up batch
    torch.cuda.synchronize()
    t0 = time.time()
    pipe.run_volumes(seeds, size, args.depth, args.hw)
    torch.cuda.synchronize()
    dt = time.time() - t0
    vox = B * (size[0] * size[1] * size[2] + args.depth * args.hw * args.hw)
    return {"volumes": B, "seconds": round(dt, 2), "voxels_per_s": round(vox / dt, 1), "ccdm_s": round(pipe.stats["ccdm_s"], 2),
            "ldm_s": round(pipe.stats["ldm_s"], 2), "wasted_slot_fraction": round(pipe.stats["wasted_slot_fraction"], 4)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--mask-size", type=int, nargs=3, default=(128, 128, 128))
    ap.add_argument("--depth", type=int, default=256)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--ccdm-steps", type=int, default=250)
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1024)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_volumes needs an MI355X"
    dev = torch.device("cuda", 0)
    pipe = GuideGenPipeline(build_ccdm(14, args.ccdm_steps, 1024, dev), build_ldm(1024, dev), ddim_steps=args.ddim_steps)
    one = timed_batch(pipe, 1, args)
    many = timed_batch(pipe, args.batch, args)
    print(json.dumps({"metric": f"whole-volume voxels/s, B = {args.batch} independent volumes per batch vs B = 1",
                      "b1": one, f"b{args.batch}": many, "ratio": round(many["voxels_per_s"] / one["voxels_per_s"], 3),
                      "config": {"mask_size": list(args.mask_size), "ccdm_steps": args.ccdm_steps, "depth": args.depth, "hw": args.hw,
                                 "ddim_steps": args.ddim_steps, "weights": "random-init (seed recipe)"}}), flush=True)


if __name__ == "__main__":
    main()
