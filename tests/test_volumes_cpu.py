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


def _batch_window(labels_np, depth, max_slices=None):
    """The reference's rule for a batch [N, Dm, H, W] (sample_diffusion.py:202 on N masks): slices whose order-0 zoomed mask is non-empty
    in ANY batch element, from one before the first to the last, python-indexed; an empty batch gives start, end = 1, 0."""
    Dm = labels_np.shape[1]
    zf = (Dm - 1) / (depth - 1) if depth > 1 else 1.0
    src = np.clip(np.floor(np.arange(depth, dtype=np.float64) * zf + 0.5).astype(np.int64), 0, Dm - 1)
    zoomed = labels_np[:, src]                                                  # [N, depth, H, W]
    nz = np.array([any((zoomed[n, d] != 0).any() for n in range(zoomed.shape[0])) for d in range(depth)])
    idx = np.nonzero(nz)[0]
    start, end = (int(idx[0]), int(idx[-1])) if idx.size else (1, 0)
    ms = list(range(start - 1, end + 1))
    return ms[:max_slices] if max_slices is not None else ms


def test_slice_window_of_a_batch_is_the_any_over_the_batch_rule():
    from jointimagegeneration_amd.pipeline import slice_window
    cases = {                                      # name: (Dm, depth, non-empty mask slices [lo, hi) of the two elements, the window)
        "empty": (6, 6, [(0, 0), (0, 0)], [0]),
        "slice 0 (wraps to -1)": (6, 6, [(0, 2), (0, 0)], [-1, 0, 1]),
        "last slice only": (6, 6, [(0, 0), (5, 6)], [4, 5]),
        "5 into 7": (5, 7, [(1, 2), (3, 4)], [0, 1, 2, 3, 4, 5]),       # zoom index 0 1 1 2 3 3 4: mask slices 1 and 3 are slices 1, 2, 4, 5
        "union wider than either": (6, 6, [(1, 3), (3, 5)], [0, 1, 2, 3, 4]),
    }
    for name, (Dm, depth, wins, want) in cases.items():
        labels = torch.stack([_mask(Dm, 4, lo, hi, seed=7 + i) for i, (lo, hi) in enumerate(wins)])
        assert labels.shape == (2, Dm, 4, 4)
        for max_slices in (None, 2):
            ref = _batch_window(labels.numpy(), depth, max_slices)
            assert ref == (want if max_slices is None else want[:2]), name
            assert slice_window(labels, depth, max_slices) == ref, name
    a, b = (slice_window(_mask(6, 4, lo, hi, seed=7 + i), 6) for i, (lo, hi) in enumerate(cases["union wider than either"][2]))
    assert a == [0, 1, 2] and b == [2, 3, 4]                                    # each element alone is narrower than the union


def test_ct_edit_plan_visits_counters_start_volume_and_tape_refusals():
    """plan_ct_edit on three volumes with the window 0 .. 4 of 6 slices: volume 0's window is kept whole, volume 1 keeps slices 0, 2, 4 and
    parts of 1 and 3 (two mixed slices), volume 2 keeps nothing."""
    import pytest
    from jointimagegeneration_amd.pipeline import plan_ct_edit
    depth, hw, q_shape = 6, 4, (5, 1, 4, 1, 1)
    g = torch.Generator().manual_seed(9)
    labels = torch.stack([_mask(depth, hw, 1, 5, seed=i) for i in range(3)])
    known = torch.rand((depth, 3, hw, hw), generator=g)                         # slice-major, as the loop holds it
    keep = torch.ones((depth, 3, hw, hw), dtype=torch.bool)
    keep[5, 0, 0, 0] = False                                                    # volume 0: one un-kept pixel, outside its window
    keep[1, 1, :2] = False
    keep[3, 1, 2, 3] = False
    keep[5, 1, 0, :3] = False
    keep[:, 2] = False
    windows, mixed, counters, start = plan_ct_edit(labels, depth, None, known, keep, q_shape)
    assert windows == [[], [1, 3], [0, 1, 2, 3, 4]]
    assert mixed == [[], [True, True], [False] * 5]
    assert counters == dict(slices_visited=7, slices_skipped_kept=5 + 3, slices_mixed=2, unkept_outside_window=1 + 3 + hw * hw)
    assert torch.equal(start, torch.where(keep, known, torch.zeros(())))
    # max_slices truncates the window before the kept slices leave it
    windows, mixed, counters, _ = plan_ct_edit(labels, depth, 2, known, keep, q_shape)
    assert windows == [[], [1], [0, 1]] and mixed == [[], [True], [False, False]]
    assert (counters["slices_visited"], counters["slices_skipped_kept"], counters["slices_mixed"]) == (3, 2 + 1, 1)
    # nothing to visit: every window kept whole
    keep_all = torch.ones_like(keep)
    windows, _, counters, start = plan_ct_edit(labels, depth, None, known, keep_all, q_shape)
    assert not any(windows) and counters["slices_visited"] == 0 and counters["slices_skipped_kept"] == 15 and torch.equal(start, known)
    # tapes that fit, then each refusal by its text
    x_ok = [[], [torch.zeros(1, 4, 1, 1)] * 2, [torch.zeros(1, 4, 1, 1)] * 5]
    q_ok = [[], [torch.zeros(q_shape)] * 2, []]
    assert plan_ct_edit(labels, depth, None, known, keep, q_shape, x_ok, q_ok)[0] == [[], [1, 3], [0, 1, 2, 3, 4]]
    with pytest.raises(ValueError, match=r"sample_ct_volumes: x_T_tapes\[1\] holds 1 tensors, volume 1 visits 2 slices"):
        plan_ct_edit(labels, depth, None, known, keep, q_shape, [[], x_ok[1][:1], x_ok[2]], q_ok)
    with pytest.raises(ValueError, match=r"sample_ct_volumes: q_noise_tapes\[1\] holds 0 tensors, volume 1 has 2 mixed slices"):
        plan_ct_edit(labels, depth, None, known, keep, q_shape, x_ok, [[], [], []])
    with pytest.raises(ValueError, match=r"sample_ct_volumes: q_noise_tapes\[2\] holds 1 tensors, volume 2 has 0 mixed slices"):
        plan_ct_edit(labels, depth, None, known, keep, q_shape, None, [[], q_ok[1], [torch.zeros(q_shape)]])
    with pytest.raises(ValueError, match=r"sample_ct_volumes: q_noise_tapes\[1\]\[1\] has shape \(5, 4, 1, 1\), a mixed slice takes \(5, 1, 4, 1, 1\)"):
        plan_ct_edit(labels, depth, None, known, keep, q_shape, None, [[], [torch.zeros(q_shape), torch.zeros(5, 4, 1, 1)], []])


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
