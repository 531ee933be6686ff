"""CPU suite for the mask-cleaning feature (gg_components.hip, ops.label_vote / label_components / component_stats / component_filter,
postprocess.py): the numpy reference of tests/components_ref.py against the scipy fixture (tests/golden/components.npz), the host
refusals by name, the command-line handling, and that run_volumes without `clean` calls none of the new ops."""
import hashlib
import os

import numpy as np
import pytest
import torch

import components_ref as R
from util import GOLD


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "components.npz"), allow_pickle=False)


def test_reference_equals_the_scipy_fixture_on_every_case(gold):
    cases = R.fixture_cases()
    assert len(cases) >= 40
    for name, (labels, K) in cases.items():
        for conn in (6, 26):
            got = R.roots(labels, K, conn)
            assert got.dtype == np.int32 and np.array_equal(got, gold[f"{name}__root{conn}"]), (name, conn)
    # the properties the patterns were built for, read off the fixture itself
    serp = gold["serpentine_33x17x9__root6"]
    assert (serp[serp >= 0] == 0).all() and int((serp >= 0).sum()) > 1000                # ONE component rooted at voxel 0
    cb6, cb26 = gold["checkerboard_5x6x7__root6"][0], gold["checkerboard_5x6x7__root26"][0]
    assert np.array_equal(cb6, np.arange(210)) and sorted(set(cb26.tolist())) == [0, 1]  # singletons; one component per colour
    ce6, ce26 = gold["corner_and_edge__root6"][0], gold["corner_and_edge__root26"][0]
    assert len(set(ce6[ce6 >= 0].tolist())) == 4 and len(set(ce26[ce26 >= 0].tolist())) == 2
    for conn in (6, 26):                                                                  # adjacent in memory, not in space
        w = gold[f"wrap_traps__root{conn}"][0]
        assert np.array_equal(w[w >= 0], np.nonzero(w >= 0)[0]), conn
    b3 = gold["batch3_5x6x7__root6"]
    assert 0 <= b3[0, -1] <= 209 and 0 <= b3[1, -1] <= 209                                # the last voxels are foreground, rooted in their volume
    assert b3[1, 0] == 0 and b3[2, 0] == 0                                                # a new volume starts its own components
    oob = gold["out_of_range__root6"][0]
    assert oob[0] == -1 and oob[1] == -1 and oob[(2 * 6 + 3) * 7 + 4] == -1 and oob[-1] == -1


def test_reference_equals_scipy_on_the_random_64_cube(gold):
    big = R.random_labels((1, 64, 64, 64), 2, 64)
    for conn in (6, 26):
        root = R.roots(big, 2, conn)
        assert np.array_equal(np.frombuffer(hashlib.sha256(root.tobytes()).digest(), dtype=np.uint8), gold[f"random64__sha{conn}"])
        assert np.array_equal(R.sizes_and_stats(big, root, 2)[1], gold[f"random64__stats{conn}"])
    st = gold["random64__stats6"][0, 1]
    assert st[0] > 10000 and st[2] > 10000            # thousands of islands and one tortuous cluster that crosses the volume


def test_reference_stats_filter_and_vote():
    labels, K = R.fixture_cases()["tie"]
    root = R.roots(labels, K)
    size, stats = R.sizes_and_stats(labels, root, K)
    assert stats[0, 1].tolist() == [3, 10, 4, 0] and stats[0, 2].tolist() == [3, 6, 3, (1 * 6 + 3) * 7] and stats[0, 0].tolist() == [0, 0, 0, -1]
    assert size[0, 0] == 4 and size[0, 1] == 0 and int(size.sum()) == 16
    out, kept = R.filter_labels(labels, root, size, stats, K, [0, 1, 0], [0, 0, 2])
    assert int((out == 1).sum()) == 4 and out[0, 0, 0, 0] == 1 and out[0, 4, 5, 6] == 0   # the tie goes to the smaller root
    assert int((out == 2).sum()) == 5 and out[0, 4, 0, 0] == 0                            # size == min_size stays, min_size - 1 goes
    assert np.array_equal(kept, (out == labels).astype(np.uint8))
    lab = np.array([[1, 1, 0, 3, -1], [1, 2, 0, 3, 9], [2, 2, 1, 0, 9]], dtype=np.int32)
    w, a, h, sk = R.vote(lab, 4)
    assert w.tolist() == [1, 2, 0, 3, 0] and a.tolist() == [2, 2, 2, 2, 0] and sk == 3
    assert h[4] == 0.0 and h[0] == h[1] and abs(float(h[0]) - (np.log(3) - 2 * np.log(2) / 3)) < 1e-6 and h.dtype == np.float32
    w1, a1, h1, _ = R.vote(lab[:1].clip(0, 3), 4)
    assert w1.tolist() == lab[0].clip(0, 3).tolist() and (a1 == 1).all() and (h1 == 0).all()


def test_host_refusals_are_named(monkeypatch):
    from jointimagegeneration_amd import ops, postprocess
    vol = torch.zeros((1, 2, 3, 4), dtype=torch.int32)
    rows = torch.zeros((2, 24), dtype=torch.int32)
    for call in (lambda: ops.label_vote(rows, 4), lambda: ops.label_components(vol, 4), lambda: ops.component_stats(vol, rows[:1], 4),
                 lambda: ops.component_filter(vol, rows[:1], rows[:1], torch.zeros(1, 4, 4, dtype=torch.int64), 4, rows[0, :4], rows[0, :4]),
                 lambda: postprocess.consensus(vol, 4), lambda: postprocess.clean(vol, 4), lambda: postprocess.component_scores(vol, 4)):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call()
    monkeypatch.setattr(ops, "require_gpu", lambda t, what: None)
    monkeypatch.setattr(ops._lib, "load", lambda: pytest.fail("a refused call must not reach the library"))
    root = torch.zeros((1, 24), dtype=torch.int32)
    stats = torch.zeros((1, 4, 4), dtype=torch.int64)
    pol = torch.zeros(4, dtype=torch.int32)
    refusals = [
        (lambda: ops.label_vote(rows.long(), 4), "label_vote: labels must be a contiguous int32"),
        (lambda: ops.label_vote(rows.t(), 4), "not contiguous"),
        (lambda: ops.label_vote(rows[0], 4), "with 2 dimensions"),
        (lambda: ops.label_vote(rows, 33), "label_vote: K=33"),
        (lambda: ops.label_vote(rows, 0), "label_vote: K=0"),
        (lambda: ops.label_vote(torch.zeros((65, 3), dtype=torch.int32), 4), "S=65"),
        (lambda: ops.label_vote(torch.zeros((2, 0), dtype=torch.int32), 4), "M=0"),
        (lambda: ops.label_components(vol[0], 4), "label_components: labels must be a contiguous int32 tensor with 4 dimensions"),
        (lambda: ops.label_components(vol.to(torch.uint8), 4), "label_components: labels must be a contiguous int32"),
        (lambda: ops.label_components(vol, 4, connectivity=18), "connectivity 18 is neither 6 nor 26"),
        (lambda: ops.label_components(vol, 4, background=4), "background 4 outside"),
        (lambda: ops.label_components(vol, 40), "label_components: K=40"),
        (lambda: ops.component_stats(vol, root[:, :23], 4), "component_stats: root must be int32 \\[1, 24\\]"),
        (lambda: ops.component_stats(vol, root.long(), 4), "component_stats: root must be a contiguous int32"),
        (lambda: ops.component_filter(vol, root, root[:, :5], stats, 4, pol, pol), "component_filter: size must be int32"),
        (lambda: ops.component_filter(vol, root, root, stats.int(), 4, pol, pol), "component_filter: stats must be a contiguous int64"),
        (lambda: ops.component_filter(vol, root, root, stats, 4, pol[:3], pol), "component_filter: keep_largest must hold K=4"),
        (lambda: ops.component_filter(vol, root, root, stats, 4, pol, pol.long()), "component_filter: min_size must be a contiguous int32"),
        (lambda: ops.component_filter(vol, root, root, stats, 4, pol, pol, fill=4), "fill 4 outside"),
        (lambda: ops.component_filter(vol, root, root, stats, 4, pol, pol, background=-1), "fill must be given"),
        (lambda: postprocess.clean(vol, 4, largest="some"), "largest='some'"),
        (lambda: postprocess.clean(vol, 4, largest=[4]), "classes are 0..3"),
        (lambda: postprocess.clean(vol, 4, min_size={7: 2}), "min_size classes"),
        (lambda: postprocess.clean(vol, 4, min_size=-1), "min_size -1"),
        (lambda: postprocess.clean(vol.float(), 4), "clean: labels must be an integer tensor"),
        (lambda: postprocess.consensus(rows.float(), 4), "consensus: labels must be an integer tensor"),
    ]
    for call, match in refusals:
        with pytest.raises(ValueError, match=match):
            call()


def test_policy_and_scores_from_stats():
    from jointimagegeneration_amd import postprocess
    assert postprocess._policy(4, "all", 0, 0) == ([0, 1, 1, 1], [0, 0, 0, 0])
    assert postprocess._policy(4, "all", 5, -1) == ([1, 1, 1, 1], [5, 5, 5, 5])
    assert postprocess._policy(4, [3], {1: 2}, 0) == ([0, 0, 0, 1], [0, 2, 0, 0])
    assert postprocess._policy(4, None, 0, 0) == ([0, 0, 0, 0], [0, 0, 0, 0])
    labels, K = R.fixture_cases()["tie"]
    _, stats = R.sizes_and_stats(labels, R.roots(labels, K), K)
    s = postprocess.scores_from_stats(stats, 210)[0]
    assert s["stray_voxels"] == 6 + 3 and s["stray_fraction"] == 9 / 16 and s["foreground_voxels"] == 16 and s["voxels"] == 210
    assert s["classes"][1] == dict(label=1, components=3, voxels=10, largest=4, largest_fraction=0.4)
    assert s["classes"][0]["largest_fraction"] == 1.0 and s["classes"][0]["components"] == 0


def test_command_line_handling(tmp_path):
    import yaml
    from jointimagegeneration_amd import ddpm_eval, postprocess, sample_diffusion
    from jointimagegeneration_amd.io import write_nifti
    ap = postprocess.build_parser()
    a = ap.parse_args(["--pred", "p", "--num-classes", "6", "--out", "o", "--largest-component", "1,3", "--min-component", "9", "--connectivity", "26"])
    assert postprocess.cleanup_options(a, 6) == dict(largest=[1, 3], min_size=9, connectivity=26)
    a = ap.parse_args(["--pred", "p", "--num-classes", "6", "--out", "o", "--largest-component", "all"])
    assert postprocess.cleanup_options(a, 6) == dict(largest="all", min_size=0, connectivity=6)
    a = ap.parse_args(["--pred", "p", "--num-classes", "6", "--out", "o", "--min-component", "4"])
    assert postprocess.cleanup_options(a, 6) == dict(largest=None, min_size=4, connectivity=6)
    assert postprocess.cleanup_options(ap.parse_args(["--pred", "p", "--num-classes", "6", "--out", "o"]), 6) is None
    for extra, match in ((["--connectivity", "18", "--min-component", "2"], "--connectivity 18"), (["--connectivity", "26"], "--connectivity needs"),
                         (["--largest-component", "6"], "classes are 0..5"), (["--largest-component", "a,b"], "comma-separated"),
                         (["--min-component", "-3"], "--min-component -3")):
        with pytest.raises(ValueError, match=match):
            postprocess.cleanup_options(ap.parse_args(["--pred", "p", "--num-classes", "6", "--out", "o"] + extra), 6)
    with pytest.raises(SystemExit):
        ap.parse_args(["--num-classes", "6", "--out", "o"])                              # --pred is required
    # the prediction files of a run: all samples of every volume, or a named refusal
    pred = tmp_path / "pred"
    pred.mkdir()
    with pytest.raises(FileNotFoundError, match="no pred_"):
        postprocess.find_predictions(str(pred), 1)
    for v in range(2):
        for j in range(3):
            write_nifti(str(pred / f"pred_{v:04d}_s{j:02d}.nii.gz"), np.zeros((2, 3, 4), np.uint8))
    found = postprocess.find_predictions(str(pred), 3)
    assert sorted(found) == [0, 1] and [os.path.basename(p) for p in found[1]] == [f"pred_0001_s{j:02d}.nii.gz" for j in range(3)]
    with pytest.raises(FileNotFoundError, match="needs 0..3"):
        postprocess.find_predictions(str(pred), 4)
    with pytest.raises(ValueError, match="nothing to do"):
        postprocess.main(["--pred", str(pred), "--num-classes", "4", "--out", str(tmp_path / "o")])
    with pytest.raises(ValueError, match="--samples 65"):
        postprocess.main(["--pred", str(pred), "--num-classes", "4", "--samples", "65", "--out", str(tmp_path / "o")])
    # ddpm_eval refuses the new flags before it samples (and before it needs a GPU)
    pf = tmp_path / "params_eval.yml"
    pf.write_text(yaml.safe_dump(dict(time_steps=4, batch_size=1)))
    base = [str(pf), "t", "--size", "4", "4", "4", "--num-classes", "4", "--num-volumes", "1", "--out", str(tmp_path / "e")]
    for extra, match in ((["--consensus"], "--consensus votes over the masks"), (["--samples", "3", "--largest-component", "all"], "give --consensus"),
                         (["--connectivity", "26"], "--connectivity needs"), (["--largest-component", "4"], "classes are 0..3")):
        with pytest.raises(ValueError, match=match):
            ddpm_eval.main(base + extra)
    # sample_diffusion: the three options belong to --inputs
    opt = sample_diffusion.get_parser().parse_args(["--largest-component", "all", "--min-component", "5"])
    with pytest.raises(SystemExit, match="--inputs DIR"):
        sample_diffusion.cleanup_from_options(opt)
    opt = sample_diffusion.get_parser().parse_args(["--inputs", "d", "--largest-component", "1,2", "--connectivity", "26"])
    assert sample_diffusion.cleanup_from_options(opt) == dict(largest=[1, 2], min_size=0, connectivity=26)
    assert sample_diffusion.cleanup_from_options(sample_diffusion.get_parser().parse_args(["--inputs", "d"])) is None
    with pytest.raises(SystemExit, match="--connectivity 7"):
        sample_diffusion.cleanup_from_options(sample_diffusion.get_parser().parse_args(["--inputs", "d", "--connectivity", "7", "--min-component", "1"]))


def test_run_volumes_without_clean_calls_none_of_the_new_ops(monkeypatch):
    from jointimagegeneration_amd import ops, pipeline, postprocess
    calls = {name: 0 for name in ("label_vote", "label_components", "component_stats", "component_filter")}
    for name in calls:
        def counted(*a, _n=name, **k):
            calls[_n] += 1
            raise AssertionError(f"ops.{_n} launched")
        monkeypatch.setattr(ops, name, counted)
    cleaned = {"n": 0}

    def fake_clean(labels, K, **kw):
        cleaned["n"] += 1
        cleaned["kw"] = (K, kw)
        return labels + 1, torch.ones_like(labels, dtype=torch.uint8), dict(stray_voxels=3), dict(stray_voxels=0)
    monkeypatch.setattr(postprocess, "clean", fake_clean)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    pipe = pipeline.GuideGenPipeline.__new__(pipeline.GuideGenPipeline)
    pipe.stats = {"wasted_slot_fraction": 0.0}

    class _Diffusion:
        num_classes = 6

    class _Ccdm:
        diffusion = _Diffusion()
    pipe.ccdm = _Ccdm()
    labels = torch.arange(2 * 2 * 3 * 4, dtype=torch.int32).reshape(2, 2, 3, 4) % 6
    seen = {}
    pipe.sample_masks = lambda seeds, size, init_t: labels.clone()

    def fake_ct(lab, depth, hw, seeds, max_slices):
        seen["labels"] = lab
        return torch.zeros((lab.shape[0], depth, hw, hw))
    pipe.sample_ct_volumes = fake_ct
    got, _ = pipe.run_volumes([1, 2], mask_size=(2, 3, 4), depth=2, hw=4)
    assert torch.equal(got, labels) and torch.equal(seen["labels"], labels)
    assert cleaned["n"] == 0 and all(v == 0 for v in calls.values()) and "mask_cleanup" not in pipe.stats
    got, _ = pipe.run_volumes([1, 2], mask_size=(2, 3, 4), depth=2, hw=4, clean=dict(largest=[2], min_size=5))
    assert cleaned["n"] == 1 and cleaned["kw"] == (6, dict(largest=[2], min_size=5, connectivity=6, background=0, fill=None))
    assert torch.equal(got, labels + 1) and torch.equal(seen["labels"], labels + 1)       # the slice loop sees the cleaned masks
    assert pipe.stats["mask_cleanup"] == dict(before=dict(stray_voxels=3), after=dict(stray_voxels=0))
    with pytest.raises(ValueError, match="clean options \\['smallest'\\]"):
        pipe.run_volumes([1, 2], mask_size=(2, 3, 4), depth=2, hw=4, clean=dict(smallest=1))
