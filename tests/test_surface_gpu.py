"""GPU suite for gg_surface.hip (class borders, exact squared distance transform, per-volume reduction) and the layers above it
(ops, metrics.surface_distances, ddpm_eval --surface), against the scipy fixture tests/golden/surface.npz on the cases of
tests/surface_ref.py.  The comparisons are the ones the feature was specified with:

    border                                                        == the fixture at connectivity 1, 2 and 3
    sq, dist2, count, maximum at spacing (1, 1, 1), (2.5, .75, .75)  == the fixture (every product and sum is exact in fp64)
    hd at those two spacings                                      == the fixture
    sq at spacing (3.0, 0.7, 0.7)                                 within relative 1e-14 (five roundings of 2^-53 a side, ties aside)
    asd, assd, hd95                                               within relative 1e-12 (the bound of the fp64 formulas of this suite)
    stats and dist2 of two runs on one input                      identical bits

No test here imports scipy or reads anything but the fixture."""
import json
import os

import numpy as np
import pytest
import torch

import surface_ref as R
from util import CCDM_SMALL, GOLD

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

CASES = R.cases()
SMALL = sorted(n for n in CASES if not R.is_big(CASES[n]))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "surface.npz"), allow_pickle=False)


def on(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("name", sorted(CASES))
def test_borders_equal_the_fixture(dev, gold, name):
    from jointimagegeneration_amd import ops
    case = CASES[name]
    for conn in (1, 2, 3):
        for side in ("pred", "gt"):
            got = ops.label_border(on(dev, case[side]), case["K"], conn)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (case[side].shape[0], case[side][0].size)
            assert np.array_equal(R.held(got.cpu().numpy(), R.is_big(case)), gold[f"{name}__border{conn}_{side}"]), (conn, side)


@pytest.mark.parametrize("name", sorted(CASES))
def test_squared_distances_and_the_reduction_equal_the_fixture(dev, gold, name):
    """sq of either volume's border sites, then dist2 / count / sum / maximum over the OTHER volume's border voxels, per class."""
    from jointimagegeneration_amd import ops
    case = CASES[name]
    big, K = R.is_big(case), case["K"]
    lab = {s: on(dev, case[s]) for s in ("pred", "gt")}
    brd = {s: ops.label_border(lab[s], K, 1) for s in lab}
    for tag, spacing in R.SPACINGS.items():
        for c in ([1] if big else range(K)):
            for side, other in (("gt", "pred"), ("pred", "gt")):
                if big and tag not in R.EXACT:
                    continue                                        # the fixture holds a big case's sq as a hash of exact values only
                sq_dev = ops.edt_squared(lab[side], brd[side], c, spacing)
                sq = sq_dev.cpu().numpy()
                want = gold[f"{name}__sq_{tag}_c{c}_{side}"]
                if big:
                    if tag == "unit":
                        assert np.isfinite(sq).all() and np.array_equal(sq, np.rint(sq)), (tag, c, side)     # integers, so the cast loses nothing
                        assert np.array_equal(R.sha(sq.astype(np.int64)), want), (tag, c, side)
                    elif tag == "dyadic":
                        assert np.array_equal(R.sha(sq), want), (tag, c, side)
                elif tag in R.EXACT:
                    assert np.array_equal(sq, want), (tag, c, side)
                else:
                    fin = np.isfinite(want)
                    err = float((np.abs(sq[fin] - want[fin]) / want[fin].clip(min=1e-300)).max()) if fin.any() else 0.0
                    print(f"{name} {tag} class {c} {side}: max relative error of sq {err:.3e}")
                    assert np.array_equal(np.isfinite(sq), fin) and err <= 1e-14, (tag, c, side, err)
                if tag not in R.EXACT:
                    continue
                dist2, stats = ops.surface_reduce(lab[other], brd[other], sq_dev, c)
                if big:                                             # hashes only in the fixture: the device's sq (held to its hash above)
                    want_d2, want_st = R.reduce(case[other], brd[other].cpu().numpy(), sq, c)       # and border (held in the border test)
                else:
                    want_d2, want_st = R.reduce(case[other], gold[f"{name}__border1_{other}"], want, c)
                got_d2, got_st = dist2.cpu().numpy(), stats.cpu().numpy()
                assert np.array_equal(got_d2, want_d2), (tag, c, other)
                assert np.array_equal(got_st[:, 0], want_st[:, 0]) and np.array_equal(got_st[:, 2], want_st[:, 2]), (tag, c, other)
                with np.errstate(invalid="ignore"):
                    ok = np.isfinite(want_st[:, 1])
                    assert np.array_equal(got_st[~ok, 1], want_st[~ok, 1]) and (np.abs(got_st[ok, 1] - want_st[ok, 1]) <= 1e-12 * want_st[ok, 1]).all()
                again_d2, again_st = ops.surface_reduce(lab[other], brd[other], sq_dev, c)
                assert torch.equal(again_d2.view(torch.int64), dist2.view(torch.int64)) and torch.equal(again_st.view(torch.int64), stats.view(torch.int64))
    if not big:                                                     # the general-purpose form: every voxel of the class is a site
        full = ops.edt_squared(lab["gt"], None, 1).cpu().numpy()
        assert np.array_equal(full, gold[f"{name}__sqfull_unit_c1_gt"])


def test_the_transform_reuses_the_callers_buffers_and_keeps_volumes_apart(dev, gold):
    from jointimagegeneration_amd import ops
    case = CASES["batch3_5x6x7"]
    lab = on(dev, case["gt"])
    brd = ops.label_border(lab, 3, 1)
    out = torch.full((3, 210), -7.0, dtype=torch.float64, device=dev)
    ws = torch.empty(3 * 210, dtype=torch.float64, device=dev)
    got = ops.edt_squared(lab, brd, 1, out=out, workspace=ws)
    assert got is out and np.array_equal(out.cpu().numpy(), gold["batch3_5x6x7__sq_unit_c1_gt"])
    assert torch.isinf(out[1]).all() and torch.isfinite(out[0]).all()                   # the middle volume has no site: +inf, untouched by its neighbours
    dist2, stats = ops.surface_reduce(on(dev, case["pred"]), None, out, 2)              # border None: every voxel of the class
    n = (case["pred"] == 2).reshape(3, -1).sum(1)
    assert stats[:, 0].tolist() == n.tolist() and int((dist2 >= 0).sum()) == int(n.sum())
    none = ops.surface_reduce(on(dev, case["pred"]), None, out, 9)[1]
    assert none.tolist() == [[0.0, 0.0, -1.0]] * 3


@pytest.mark.parametrize("name", sorted(CASES))
def test_scores_equal_the_fixture(dev, gold, name):
    from jointimagegeneration_amd import metrics
    case = CASES[name]
    K = case["K"]
    pred, gt = on(dev, case["pred"]), on(dev, case["gt"])
    for tag, conn in [(t, 1) for t in R.SPACINGS] + ([] if R.is_big(case) else [("unit", 2), ("unit", 3)]):
        got = metrics.surface_distances(pred, gt, K, spacing=R.SPACINGS[tag], connectivity=conn)
        assert got["classes"] == list(range(K))
        for score in R.SCORES:
            want = gold[f"{name}__{score}_{tag}_conn{conn}"]
            for v in range(pred.shape[0]):
                for c in range(K):
                    g, w = got[score][v][c], float(want[v, c])
                    if np.isnan(w):
                        assert g is None and c in got["absent"][v], (score, tag, conn, v, c)
                        continue
                    assert g is not None and c not in got["absent"][v]
                    if score == "hd" and tag in R.EXACT:
                        assert g == w, (tag, conn, v, c, g, w)
                    else:
                        print(f"{name} {score} {tag} conn {conn} volume {v} class {c}: got {g!r} want {w!r}")
                        assert abs(g - w) <= 1e-12 * abs(w), (score, tag, conn, v, c, g, w)
        for v in range(pred.shape[0]):
            scored = [c for c in range(K) if c not in got["absent"][v]]
            for score in R.SCORES:
                m = got["mean"][v][score]
                assert (m is None) == (not scored) and (m is None or abs(m - np.mean([got[score][v][c] for c in scored])) <= 1e-12 * m)
    ign = metrics.surface_distances(pred, gt.long(), K, ignore_index=0)                 # int64 labels are plumbing; the ignored class is None
    assert ign["classes"] == list(range(1, K)) and all(row[0] is None for row in ign["hd"]) and all(0 not in a for a in ign["absent"])
    assert [row[1:] for row in ign["hd"]] == [row[1:] for row in metrics.surface_distances(pred, gt, K)["hd"]]


def test_an_extent_above_the_limit_is_refused_by_name(dev):
    from jointimagegeneration_amd import _lib, ops
    lib = _lib.load()
    for shape in ((1, 1, 1, 1025), (1, 1025, 1, 2)):
        lab = torch.ones(shape, dtype=torch.int32, device=dev)
        assert ops.label_border(lab, 2).sum() == lab.numel()                            # the border has no such limit
        with pytest.raises(ValueError, match="edt_squared: volume .* has an extent above 1024"):
            ops.edt_squared(lab, None, 1)
        out = torch.full((lab.numel(),), -3.0, dtype=torch.float64, device=dev)
        rc = lib.gg_edt_squared(lab.data_ptr(), None, 1, 1, shape[1], shape[2], shape[3], 1.0, 1.0, 1.0, out.data_ptr(), out.data_ptr(), 1 << 30, None)
        assert rc == _lib.GG_ERR_UNSUPPORTED and b"an extent above 1024" in lib.gg_last_error()
        torch.cuda.synchronize()
        assert (out == -3.0).all()                                                      # refused before any launch
    lab = torch.ones((1, 1, 2, 1024), dtype=torch.int32, device=dev)                    # the limit itself runs
    lab[0, 0, 1, 1000] = 0
    sq = ops.edt_squared(lab, None, 0).reshape(2, 1024)
    w = torch.arange(1024, device=dev, dtype=torch.float64)
    assert torch.equal(sq[1], (w - 1000) ** 2) and torch.equal(sq[0], (w - 1000) ** 2 + 1)


def test_ddpm_eval_reports_the_surface_block_and_stays_as_it_was_without_the_flag(dev, tmp_path, monkeypatch):
    """A small synthetic run: the `surface` block is the score of the written files, recomputed here; hd95_consensus / hd95_clean stand
    beside the Dice of the two masks; the stand-alone scorer reports the same block; without --surface the run launches none of the
    three ops and writes the document of a run with the flag minus the new keys."""
    import yaml
    from jointimagegeneration_amd import ddpm_eval, metrics, ops
    from jointimagegeneration_amd.io import read_nifti, write_nifti
    size, K, S, nvol = (8, 16, 16), 4, 2, 2
    params = dict(output_path=str(tmp_path), exp_name="t", evaluation_vote_strategy="majority", dataset_file="datasets.ruijin", batch_size=2,
                  dims=3, beta_schedule="cosine", beta_schedule_params=dict(s=0.008), time_steps=6, backbone="unet_openai",
                  feature_cond_encoder=dict(type="none"), unet_openai=dict(CCDM_SMALL))
    pf = tmp_path / "params_eval.yml"
    pf.write_text(yaml.safe_dump(params))
    gt_dir = tmp_path / "gt"
    gt_dir.mkdir()
    gts = [R.random_blobs(size, K, 70 + v, noise=0.02).astype(np.uint8) for v in range(nvol)]
    gts[1][gts[1] == 3] = 0                                                             # class 3 is absent from the second ground truth
    for vid, g in enumerate(gts):
        write_nifti(str(gt_dir / f"gt_{vid:04d}.nii.gz"), g)
    calls = {name: 0 for name in ("label_border", "edt_squared", "surface_reduce")}
    for name in calls:
        def counted(*a, _n=name, _f=getattr(ops, name), **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, counted)
    common = [str(pf), "--size", *map(str, size), "--num-classes", str(K), "--num-volumes", str(nvol), "--steps", "3", "--gt", str(gt_dir),
              "--samples", str(S), "--consensus", "--min-component", "3"]

    ddpm_eval.main(common[:1] + ["plain"] + common[1:])
    assert calls == dict(label_border=0, edt_squared=0, surface_reduce=0)
    plain = json.loads((tmp_path / "plain" / "metrics.json").read_text())
    assert "surface" not in plain and "hd95_clean" not in plain and len(plain["precision"]) == len(plain["recall"]) == K - 1

    ddpm_eval.main(common[:1] + ["surf"] + common[1:] + ["--surface", "--spacing", "2.5,0.75,0.75", "--surface-connectivity", "2"])
    assert min(calls.values()) > 0
    out = tmp_path / "surf"
    doc = json.loads((out / "metrics.json").read_text())
    new_keys = {"surface", "hd95_consensus", "mean_hd95_consensus", "hd95_clean", "mean_hd95_clean"}
    assert set(doc) - set(plain) == new_keys and {k: v for k, v in doc.items() if k not in new_keys} == plain
    block = doc["surface"]
    assert block["spacing"] == [2.5, 0.75, 0.75] and block["connectivity"] == 2 and block["classes"] == [1, 2, 3]
    opts = dict(spacing=(2.5, 0.75, 0.75), connectivity=2, ignore_index=0)
    for v in range(nvol):
        gt = on(dev, gts[v].astype(np.int32))[None]
        per = [metrics.surface_distances(on(dev, read_nifti(str(out / f"pred_{v:04d}_s{j:02d}.nii.gz")).astype(np.int32))[None], gt, K, **opts)
               for j in range(S)]
        vol = block["volumes"][v]
        assert vol["id"] == v and vol["hd"][0] is None
        for score in R.SCORES:
            for c in range(1, K):
                vals = [p[score][0][c] for p in per if p[score][0][c] is not None]
                want = float(np.mean(vals)) if vals else None
                assert (vol[score][c] is None) == (want is None) and (want is None or abs(vol[score][c] - want) <= 1e-12 * want), (v, score, c)
        assert vol["absent"] == [c for c in range(1, K) if vol["hd"][c] is None]
        for kind in ("consensus", "clean"):
            mask = on(dev, read_nifti(str(out / f"{kind}_{v:04d}.nii.gz")).astype(np.int32))[None]
            vol[f"hd95_{kind}"] = metrics.surface_distances(mask, gt, K, **opts)["hd95"][0]
    assert 3 in block["volumes"][1]["absent"]                                           # absent from the ground truth: null, not a number
    for score in R.SCORES:
        for c in range(1, K):
            vals = [vol[score][c] for vol in block["volumes"] if vol[score][c] is not None]
            assert (block[score][c] is None) == (not vals) and (not vals or abs(block[score][c] - np.mean(vals)) <= 1e-12 * np.mean(vals))
    for kind in ("consensus", "clean"):
        for i, c in enumerate(range(1, K)):
            vals = [vol[f"hd95_{kind}"][c] for vol in block["volumes"] if vol[f"hd95_{kind}"][c] is not None]
            got = doc[f"hd95_{kind}"][i]
            assert (got is None) == (not vals) and (not vals or abs(got - np.mean(vals)) <= 1e-12 * np.mean(vals)), (kind, c)
    again = metrics.main(["--pred", str(out), "--gt", str(gt_dir), "--num-classes", str(K), "--out", str(tmp_path / "again.json"), "--surface",
                          "--spacing", "2.5,0.75,0.75", "--surface-connectivity", "2"])
    for vol in block["volumes"]:
        for kind in ("consensus", "clean"):
            del vol[f"hd95_{kind}"]
    assert json.loads(json.dumps(again["surface"])) == block and again["precision"] == doc["precision"]
