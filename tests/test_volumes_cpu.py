"""CPU suite: the host side of batches of independent volumes (GuideGenPipeline.run_volumes): the per-volume slice windows and the
(slice, previous slice, active) schedule, and the `--volumes-per-gpu` grouping of the sharded CLI on two gloo ranks."""
import os
import socket
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _solo_visits(labels_np, depth, max_slices=None):
    """What sample_ct does for ONE volume, restated with numpy: scipy's order-0 zoom index rule along depth, `any` over the volume's
    own upsampled slices, loop m = start - 1 .. end (python indexing, an empty mask gives start, end = 1, 0), and per visit the slice
    written (m % depth) and the previous slice read (max(0, m - 1) % depth)."""
    Dm = labels_np.shape[0]
    zf = (Dm - 1) / (depth - 1) if depth > 1 else 1.0
    src = np.clip(np.floor(np.arange(depth, dtype=np.float64) * zf + 0.5).astype(np.int64), 0, Dm - 1)
    nz = (labels_np != 0).reshape(Dm, -1).any(-1)[src]
    idx = np.nonzero(nz)[0]
    start, end = (int(idx[0]), int(idx[-1])) if idx.size else (1, 0)
    ms = list(range(start - 1, end + 1))
    if max_slices is not None:
        ms = ms[:max_slices]
    return [(m % depth, max(0, m - 1) % depth) for m in ms]


def _mask(Dm, HW, lo, hi, seed):
    """Label volume that is non-empty exactly on the mask slices [lo, hi) (empty if lo >= hi)."""
    g = torch.Generator().manual_seed(seed)
    lab = torch.zeros((Dm, HW, HW), dtype=torch.int32)
    if hi > lo:
        lab[lo:hi] = torch.randint(0, 14, (hi - lo, HW, HW), generator=g, dtype=torch.int32)
        lab[lo:hi, 0, 0] = 3                               # at least one voxel per slice
    return lab


def test_schedule_equals_the_solo_slice_loops():
    from jointimagegeneration_amd.pipeline import slice_window, volume_schedule
    g = torch.Generator().manual_seed(5)
    cases = [
        (16, 64, [(3, 9), (0, 16), (5, 6), (0, 0), (0, 1), (15, 16)]),          # different lengths, full, one slice, EMPTY, slice 0, last
        (32, 256, [(0, 4), (10, 31), (7, 7)]),                                   # wrap-around m = -1 at the C5 depth ratio; empty
        (8, 8, [(2, 5), (0, 8)]),                                                # depth == mask depth
    ]
    for Dm, depth, wins in cases:
        vols = [_mask(Dm, 4, lo, hi, seed=i) for i, (lo, hi) in enumerate(wins)]
        for _ in range(3):                                                      # random masks too
            vols.append(torch.randint(0, 2, (Dm, 4, 4), generator=g, dtype=torch.int32) * (torch.rand(Dm, 1, 1, generator=g) < 0.4))
        labels = torch.stack(vols)
        for max_slices in (None, 3):
            windows = [slice_window(labels[i], depth, max_slices) for i in range(len(vols))]
            sched, wasted = volume_schedule(windows, depth)
            solo = [_solo_visits(v.numpy(), depth, max_slices) for v in vols]
            lens = [len(s) for s in solo]
            assert sched.dtype == torch.int32 and tuple(sched.shape) == (max(lens), len(vols), 3)
            for i, visits in enumerate(solo):
                act = sched[:, i, 2]
                assert act.tolist() == [1] * len(visits) + [0] * (sched.shape[0] - len(visits))
                got = [(int(sched[it, i, 0]), int(sched[it, i, 1])) for it in range(len(visits))]
                assert got == visits, (Dm, depth, i)
            assert abs(wasted - (1.0 - sum(lens) / (len(vols) * max(lens)))) < 1e-12
    # the edge cases explicitly: an empty mask visits slice 0 only (previous 0); a mask non-empty on slice 0 starts at m = -1
    assert _solo_visits(np.zeros((4, 2, 2), np.int32), 16) == [(0, 0)]
    assert slice_window(torch.zeros((1, 4, 2, 2), dtype=torch.int32), 16) == [0]
    lab0 = _mask(4, 2, 0, 1, seed=1)
    assert slice_window(lab0, 16)[0] == -1
    sched, _ = volume_schedule([slice_window(lab0, 16)], 16)
    assert sched[0, 0].tolist() == [15, 0, 1] and sched[1, 0].tolist() == [0, 0, 1]


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def test_pipeline_cli_groups_volumes_per_gpu_on_two_gloo_ranks(tmp_path):
    """`--volumes 7 --volumes-per-gpu 3` under two ranks (GG_PIPELINE_DRY=1): every volume id exactly once, on rank id mod 2, with the
    seed of B = 1; each rank's shard split into groups of at most 3 in shard order."""
    port = _free_port()
    out = tmp_path / "vols"
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), GG_PIPELINE_DRY="1",
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        procs.append(subprocess.Popen([sys.executable, "-m", "jointimagegeneration_amd.pipeline", "--volumes", "7", "--volumes-per-gpu", "3",
                                       "--out", str(out)], env=env, cwd=ROOT))
    assert [p.wait(timeout=180) for p in procs] == [0, 0]
    got = {f: (out / f).read_text().split() for f in sorted(os.listdir(out))}
    assert sorted(got) == [f"ct_{v:04d}.txt" for v in range(7)]
    groups = {}
    for v in range(7):
        words = got[f"ct_{v:04d}.txt"]                 # "rank R world W seed S group G volumes a,b,c"
        assert int(words[1]) == v % 2 and int(words[3]) == 2 and int(words[5]) == 1024 + 1000 * v
        assert words[6] == "group" and words[8] == "volumes"
        members = [int(x) for x in words[9].split(",")]
        assert v in members
        groups.setdefault((int(words[1]), int(words[7])), members)
        assert groups[(int(words[1]), int(words[7]))] == members
    assert groups == {(0, 0): [0, 2, 4], (0, 1): [6], (1, 0): [1, 3, 5]}
