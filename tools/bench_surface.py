"""Cost of the surface distances on the device (gg_surface.hip) at two sizes: the 128^3 mask the CCDM samples and the
256 x 512 x 512 mask the stage glue hands to the CT stage, K = 14.

    python tools/bench_surface.py [--classes 14] [--sizes 128,128,128 256,512,512] [--rounds 7] [--inner 5] [--speckle 0.005]

Input: synth.synth_mask_volume (nested ellipsoid shells) as the prediction; the ground truth is the same volume displaced by (2, 3, -3)
voxels with `--speckle` of its voxels redrawn (seeded).  Timed per size, after a warm-up of every call:
  border    gg_label_border, connectivity 1                                    (device events, --inner calls per window)
  edt       ONE gg_edt_squared from the border sites of the class --edt-class  (device events, --inner calls per window)
  scores    the whole metrics.surface_distances for all K classes              (host clock around a call that ends in read-backs)
and the stream-copy rate of the same run (gg_ubench_stream_copy) with the bytes a call must move: border 5 M (labels in, flags out),
edt 5 M + 4 x 8 M (labels and flags in; three fp64 passes, the first of which only writes).  Medians over --rounds windows.  Prints
one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from jointimagegeneration_amd import _lib, metrics  # noqa: E402
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
    ap.add_argument("--classes", type=int, default=14)
    ap.add_argument("--sizes", nargs="+", default=["128,128,128", "256,512,512"])
    ap.add_argument("--edt-class", type=int, default=7)
    ap.add_argument("--speckle", type=float, default=0.005)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    K = args.classes
    st = torch.cuda.current_stream().cuda_stream
    nbytes = 256 << 20
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def copy():
        _lib.check(lib.gg_ubench_stream_copy(src.data_ptr(), dst.data_ptr(), nbytes, st), "gg_ubench_stream_copy")
    copy()
    torch.cuda.synchronize()
    copy_ms = statistics.median(timed_ms(copy, args.inner) for _ in range(args.rounds))
    copy_Bps = 2 * nbytes / (copy_ms * 1e-3)
    res = {"classes": K, "speckle": args.speckle, "rounds": args.rounds, "inner": args.inner, "edt_class": args.edt_class,
           "stream_copy_TBps": round(copy_Bps / 1e12, 3), "sizes": {}}
    for size in args.sizes:
        D, H, W = (int(v) for v in size.split(","))
        M = D * H * W
        pred = synth_mask_volume(D, H, W, n_labels=K).to(torch.int32)
        g = torch.Generator().manual_seed(17)
        gt = torch.roll(pred, (2, 3, -3), (0, 1, 2))
        flip = torch.rand((D, H, W), generator=g) < args.speckle
        gt = torch.where(flip, torch.randint(0, K, (D, H, W), generator=g, dtype=torch.int32), gt)
        pred, gt = pred[None].contiguous().to(dev), gt[None].contiguous().to(dev)
        border = torch.empty((1, M), dtype=torch.uint8, device=dev)
        sq = torch.empty((1, M), dtype=torch.float64, device=dev)
        ws = torch.empty((1, M), dtype=torch.float64, device=dev)

        def f_border():
            _lib.check(lib.gg_label_border(gt.data_ptr(), 1, D, H, W, K, 1, border.data_ptr(), st), "gg_label_border")

        def f_edt():
            _lib.check(lib.gg_edt_squared(gt.data_ptr(), border.data_ptr(), args.edt_class, 1, D, H, W, 1.0, 1.0, 1.0, sq.data_ptr(), ws.data_ptr(),
                                          8 * M, st), "gg_edt_squared")

        def f_scores():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = metrics.surface_distances(pred, gt, K)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out
        f_border(); f_edt()
        ms, scores = f_scores()                                       # warm-up of every call, and the scores this input gets
        print(f"{size}: warm-up done, first surface_distances {ms:.0f} ms", file=sys.stderr, flush=True)
        t = {"border": [], "edt": [], "scores": []}
        for _ in range(args.rounds):
            t["border"].append(timed_ms(f_border, args.inner))
            t["edt"].append(timed_ms(f_edt, args.inner))
        for _ in range(3):
            t["scores"].append(f_scores()[0])
            print(f"{size}: surface_distances {t['scores'][-1]:.0f} ms", file=sys.stderr, flush=True)
        floors = {"border": 5 * M, "edt": 5 * M + 4 * 8 * M}
        res["sizes"][size] = {"voxels": M, "border_voxels": int(border.sum()), "edt_sites": int(((gt.reshape(1, M) == args.edt_class) & (border != 0)).sum()),
                              "median_ms": {k: round(statistics.median(v), 4) for k, v in t.items()},
                              "min_ms": {k: round(min(v), 4) for k, v in t.items()},
                              "floor_ms": {k: round(v / copy_Bps * 1e3, 4) for k, v in floors.items()},
                              "mean_hd": scores["mean"][0]["hd"], "mean_hd95": scores["mean"][0]["hd95"], "mean_assd": scores["mean"][0]["assd"],
                              "absent": scores["absent"][0]}
        del pred, gt, border, sq, ws
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
