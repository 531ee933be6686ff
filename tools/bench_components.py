"""Cost of cleaning a sampled mask on the device at the workload's shape: the vote of S = 8 masks of 128^3 voxels, K = 14, then connected
components, their stats and the filter on the consensus (gg_components.hip), against the bytes each step must move at the stream-copy
rate measured in the same run (gg_ubench_stream_copy).

    python tools/bench_components.py [--samples 8] [--classes 14] [--size 128 128 128] [--speckle 0.02] [--rounds 15] [--inner 10]

Input: synth.synth_mask_volume with seeded speckles (each sample flips `--speckle` of its voxels to a random class: the isolated voxels
and small islands a categorical chain leaves).  The raw C entries are timed between stream-ordered events after a warm-up, --inner calls
per window, the median over --rounds windows.  Byte floors (4-byte labels): vote (S + 3) M, components 2 M (labels in, roots out; the
parent array's traffic comes on top), stats 3 M (labels and roots in, sizes out), filter 4.25 M (labels, roots, sizes in; labels and kept
out).  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from jointimagegeneration_amd import _lib, ops  # noqa: E402
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
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--classes", type=int, default=14)
    ap.add_argument("--size", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--speckle", type=float, default=0.02)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    S, K = args.samples, args.classes
    D, H, W = args.size
    M = D * H * W
    st = torch.cuda.current_stream().cuda_stream
    base = synth_mask_volume(D, H, W, n_labels=K).to(torch.int32)
    samples = []
    for s in range(S):
        g = torch.Generator().manual_seed(100 + s)
        flip = torch.rand((D, H, W), generator=g) < args.speckle
        samples.append(torch.where(flip, torch.randint(0, K, (D, H, W), generator=g, dtype=torch.int32), base))
    labels = torch.stack(samples).reshape(S, M).to(dev)
    one = labels[0].reshape(1, D, H, W).contiguous()                 # a raw sample: what the filter is for

    table, ln_s, inv_s = ops.vote_operands(S)
    table = torch.from_numpy(table).to(dev)
    winner = torch.empty(M, dtype=torch.int32, device=dev)
    agreement = torch.empty(M, dtype=torch.int32, device=dev)
    entropy = torch.empty(M, dtype=torch.float32, device=dev)
    skipped = torch.empty(1, dtype=torch.int64, device=dev)
    root = torch.empty((1, M), dtype=torch.int32, device=dev)
    ws = torch.empty(M, dtype=torch.int32, device=dev)
    status = ops.component_status(dev)
    size = torch.empty((1, M), dtype=torch.int32, device=dev)
    stats = torch.empty((1, K, 4), dtype=torch.int64, device=dev)
    keep_largest = torch.tensor([0] + [1] * (K - 1), dtype=torch.int32, device=dev)
    min_size = torch.zeros(K, dtype=torch.int32, device=dev)
    out = torch.empty(M, dtype=torch.int32, device=dev)
    kept = torch.empty(M, dtype=torch.uint8, device=dev)

    def vote():
        _lib.check(lib.gg_label_vote(labels.data_ptr(), S, M, K, table.data_ptr(), ln_s, inv_s, winner.data_ptr(), agreement.data_ptr(),
                                     entropy.data_ptr(), skipped.data_ptr(), st), "gg_label_vote")

    def make(src):
        def components(conn=6):
            _lib.check(lib.gg_label_components(src.data_ptr(), 1, D, H, W, K, conn, 0, root.data_ptr(), ws.data_ptr(), 4 * M, status.data_ptr(),
                                               st), "gg_label_components")

        def cstats():
            _lib.check(lib.gg_component_stats(src.data_ptr(), root.data_ptr(), 1, M, K, size.data_ptr(), stats.data_ptr(), st), "gg_component_stats")

        def cfilter():
            _lib.check(lib.gg_component_filter(src.data_ptr(), root.data_ptr(), size.data_ptr(), stats.data_ptr(), 1, M, K, keep_largest.data_ptr(),
                                               min_size.data_ptr(), 0, 0, out.data_ptr(), kept.data_ptr(), st), "gg_component_filter")
        return components, cstats, cfilter

    comp_w, stats_w, filter_w = make(winner)
    comp_1, stats_1, filter_1 = make(one)

    def chain():
        vote(); comp_w(); stats_w(); filter_w()

    nbytes = 256 << 20
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def copy():
        _lib.check(lib.gg_ubench_stream_copy(src.data_ptr(), dst.data_ptr(), nbytes, st), "gg_ubench_stream_copy")

    configs = {"vote": vote, "components6_consensus": comp_w, "components26_consensus": lambda: comp_w(26), "stats_consensus": stats_w,
               "filter_consensus": filter_w, "chain_consensus": chain, "components6_raw_sample": comp_1, "components26_raw_sample": lambda: comp_1(26),
               "stats_raw_sample": stats_1, "filter_raw_sample": filter_1, "stream_copy": copy}
    for fn in (copy, chain, comp_1, stats_1, filter_1):               # warm-up, and the buffers every step reads exist
        fn()
    torch.cuda.synchronize()
    ops.check_component_status(dev)
    raw_stats = stats.cpu()
    chain()
    torch.cuda.synchronize()
    t = {key: [] for key in configs}
    keys = list(configs)
    for r in range(args.rounds):
        for key in (keys if r % 2 == 0 else keys[::-1]):
            if key.endswith("raw_sample"):
                comp_1()                                              # roots of the raw sample for its stats / filter windows
            elif key.endswith("consensus") and key != "chain_consensus":
                comp_w()
            t[key].append(timed_ms(configs[key], args.inner))
    ops.check_component_status(dev)
    med = {key: statistics.median(v) for key, v in t.items()}
    copy_Bps = 2 * nbytes / (med["stream_copy"] * 1e-3)
    floors = {"vote": (S + 3) * M * 4, "components": 2 * M * 4, "stats": 3 * M * 4, "filter": 4 * M * 4 + M}
    floors["chain"] = sum(floors.values())
    res = {"samples": S, "classes": K, "voxels": M, "speckle": args.speckle, "rounds": args.rounds, "inner": args.inner,
           "stream_copy_TBps": round(copy_Bps / 1e12, 3), "raw_sample_components": int(raw_stats[0, :, 0].sum()),
           "raw_sample_stray_voxels": int((raw_stats[0, :, 1] - raw_stats[0, :, 2]).sum()),
           "median_ms": {k: round(v, 4) for k, v in med.items()}, "min_ms": {k: round(min(v), 4) for k, v in t.items()}}
    res["floor_bytes"] = floors
    res["floor_ms"] = {k: round(v / copy_Bps * 1e3, 4) for k, v in floors.items()}
    res["time_over_floor"] = {k: round(med[k] / (floors[k.split("_")[0].rstrip("626")] / copy_Bps * 1e3), 1) for k in med if k != "stream_copy"}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
