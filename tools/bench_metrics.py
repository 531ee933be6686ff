"""Cost of the pairwise confusion matrices behind GED / HM-IoU at the workload's shape: Sa = Sb = 12 sampled masks of 128^3 voxels,
K = 14 classes (gg_label_confusion), against a loop of torch.bincount(a[i] * K + b[j], minlength=K * K) over the 144 pairs on the same
device, in the same process.

    python tools/bench_metrics.py [--samples 12] [--classes 14] [--size 128 128 128] [--rounds 15] [--inner 20]

Two inputs: a mostly-background mask (synth.synth_mask_volume, each sample rolled by a few voxels so that the pairs differ) and
uniform-random labels.  Three configurations alternate for --rounds rounds, each timed alone with device events: the kernel, the kernel
without its wave-uniform path (GG_CONFUSION_UNIFORM=0) and the bincount loop.  The raw C entry is timed (ops.label_confusion adds one
host read-back of the skipped counts).  Reports medians, the ratio, and the kernel's bytes/s: `volume_bytes` counts each of the 24
volumes once (what any implementation must read), `read_bytes` what the kernel's pair tiles read (each volume once per tile row or
column it belongs to); compare with the stream-copy peak of `bench.py --full`.  The counts of the three are checked equal first.
Prints one JSON line per input.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from jointimagegeneration_amd import _lib  # noqa: E402
from jointimagegeneration_amd.synth import synth_mask_volume  # noqa: E402


def timed_ms(fn, calls: int = 1) -> float:
    """Time per call of `calls` back-to-back calls, between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, default=12)
    ap.add_argument("--classes", type=int, default=14)
    ap.add_argument("--size", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20, help="kernel calls per timed window (the bincount loop is 288 launches already)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    S, K = args.samples, args.classes
    D, H, W = args.size
    M = D * H * W
    base = synth_mask_volume(D, H, W, n_labels=K).to(torch.int32)
    gen = torch.Generator().manual_seed(1)
    inputs = {
        "synth_mask": tuple(torch.stack([torch.roll(base, shifts=(s + o, 2 * s, -s), dims=(0, 1, 2)) for s in range(S)]).reshape(S, M).to(dev)
                            for o in (0, 3)),
        "uniform_random": tuple(torch.randint(0, K, (S, M), generator=gen, dtype=torch.int32).to(dev) for _ in range(2)),
    }
    cm = torch.empty((S, S, K, K), dtype=torch.int64, device=dev)
    sk = torch.empty((S, S), dtype=torch.int64, device=dev)
    cm_ref = torch.empty((S, S, K * K), dtype=torch.int64, device=dev)
    T = 6
    while T > 1 and T * T * K * K * 4 > 40 * 1024:                   # the tile rule of gg_metrics.hip
        T -= 1
    tiles = -(-S // T)
    for name, (a, b) in inputs.items():
        def kernel():
            _lib.check(lib.gg_label_confusion(a.data_ptr(), S, b.data_ptr(), S, M, K, cm.data_ptr(), sk.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "gg_label_confusion")

        def kernel_plain():
            os.environ["GG_CONFUSION_UNIFORM"] = "0"
            try:
                kernel()
            finally:
                del os.environ["GG_CONFUSION_UNIFORM"]

        def bincount_loop():
            for i in range(S):
                for j in range(S):
                    cm_ref[i, j] = torch.bincount(a[i] * K + b[j], minlength=K * K)

        configs = {"kernel": kernel, "kernel_no_uniform_path": kernel_plain, "bincount_loop": bincount_loop}
        bincount_loop()
        for key in ("kernel", "kernel_no_uniform_path"):              # also the warm-up
            configs[key]()
            torch.cuda.synchronize()
            assert torch.equal(cm.view(S, S, K * K), cm_ref) and int(sk.sum()) == 0, f"{name}: {key} differs from the bincount loop"
        t = {key: [] for key in configs}
        keys = list(configs)
        for r in range(args.rounds):
            for key in (keys if r % 2 == 0 else keys[::-1]):
                t[key].append(timed_ms(configs[key], 1 if key == "bincount_loop" else args.inner))
        res = {"input": name, "samples": S, "classes": K, "voxels": M, "rounds": args.rounds, "tile": T,
               "background_fraction": round(float((a == 0).float().mean()), 4)}
        for key, v in t.items():
            res[key] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        med = statistics.median(t["kernel"])
        res["bincount_over_kernel"] = round(statistics.median(t["bincount_loop"]) / med, 2)
        res["no_uniform_over_kernel"] = round(statistics.median(t["kernel_no_uniform_path"]) / med, 3)
        res["volume_bytes"] = 2 * S * M * 4
        res["read_bytes"] = tiles * tiles * 2 * min(T, S) * M * 4 if S % T == 0 else None
        res["volume_TBps"] = round(res["volume_bytes"] / (med * 1e-3) / 1e12, 3)
        if res["read_bytes"]:
            res["read_TBps"] = round(res["read_bytes"] / (med * 1e-3) / 1e12, 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
