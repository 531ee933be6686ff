"""CPU suite for the mask scores (jointimagegeneration_amd/metrics.py): the fp64 formulas on confusion matrices taken with np.bincount
from the labels of tests/golden/metrics.npz, against what the reference's calc_batched_generalised_energy_distance and
batched_hungarian_matching returned for those labels (make_golden_metrics.py); Dice against its formula in numpy; the C-ABI of
gg_label_confusion; the host-side refusals of ops.label_confusion, metrics.load_gt and ddpm_eval."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from util import GOLD


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "metrics.npz"))


def pair_cm(a, b, K):
    """np.bincount confusion matrices of label sets a [Sa, ...], b [Sb, ...] -> int64 [Sa, Sb, K, K]."""
    a, b = a.reshape(a.shape[0], -1).astype(np.int64), b.reshape(b.shape[0], -1).astype(np.int64)
    return np.stack([np.stack([np.bincount(x * K + y, minlength=K * K).reshape(K, K) for y in b]) for x in a])


# GED, the diversities and HM-IoU lie in [0, 2] and are sums of at most a few thousand fp64 terms in an order other than numpy's
TOL = 1e-12


@pytest.mark.parametrize("name", ["k4", "k14"])
def test_energy_distance_and_hungarian_iou_equal_the_reference(gold, name):
    from jointimagegeneration_amd import metrics
    K = int(gold[f"{name}_K"])
    a, b = gold[f"{name}_a"], gold[f"{name}_b"]
    assert a.shape == (2, 3, 4, 6, 5) and b.shape == (2, 4, 4, 6, 5)
    for c in range(a.shape[0]):
        cm01, cm00, cm11 = (torch.from_numpy(pair_cm(x, y, K)) for x, y in ((a[c], b[c]), (a[c], a[c]), (b[c], b[c])))
        ged, d0, d1 = metrics.energy_distance_from_confusion(cm01, cm00, cm11)
        assert ged.dtype == torch.float64
        got = dict(ged=float(ged), div0=float(d0), div1=float(d1), hm=metrics.hungarian_iou_from_confusion(cm01))
        for key, v in got.items():
            want = float(gold[f"{name}_{key}"][c])
            print(f"{name} case {c} {key}: got {v!r} want {want!r} diff {abs(v - want):.3e}")
            assert abs(v - want) <= TOL, (name, c, key, v, want)


def test_fixture_runs_the_branches_it_is_there_for(gold):
    from jointimagegeneration_amd import metrics
    a, b = gold["k14_a"], gold["k14_b"]
    absent = set(range(14)) - set(np.unique(a).tolist()) - set(np.unique(b).tolist())
    assert len(absent - {0}) >= 3                                     # 0 / 0 -> 1 for these classes in every pair
    d = metrics.iou_distance(torch.from_numpy(pair_cm(a[0], b[0], 14)))
    assert torch.isfinite(d).all() and tuple(d.shape) == (3, 4)
    a4, b4 = gold["k4_a"], gold["k4_b"]
    assert np.array_equal(a4[1, 0], b4[1, 2])                         # a sample equals a ground truth: distance exactly 0
    d4 = metrics.iou_distance(torch.from_numpy(pair_cm(a4[1], b4[1], 4)))
    assert float(d4[0, 2]) == 0.0 and float(d4.max()) > 0.0
    # the diagonal of a self set is zero and is part of the mean
    d00 = metrics.iou_distance(torch.from_numpy(pair_cm(a4[0], a4[0], 4)))
    assert torch.equal(d00.diagonal(), torch.zeros(3, dtype=torch.float64)) and torch.equal(d00, d00.T)


def test_iou_distance_by_hand():
    """K = 3, one pair: class 1: inter 2, union 2 + 1 + 0 = 3 -> 2/3; class 2: absent from both -> 1; distance 1 - (2/3 + 1)/2 = 1/6."""
    from jointimagegeneration_amd import metrics
    cm = torch.tensor([[5, 1, 0], [0, 2, 0], [0, 0, 0]])
    assert abs(float(metrics.iou_distance(cm)) - 1.0 / 6.0) < 1e-15
    assert tuple(metrics.iou_distance(cm.expand(2, 5, 3, 3)).shape) == (2, 5)


def test_dice_is_the_formula_and_ignore_index_removes_exactly_that_entry(gold):
    from jointimagegeneration_amd import metrics
    K = 14
    cm = pair_cm(gold["k14_a"][0], gold["k14_b"][0], K).sum((0, 1))
    c = cm.astype(np.float64)
    want = 2.0 * np.diag(c) / (c.sum(1) + c.sum(0) + 1e-15)
    got = metrics.dice_coefficient(torch.from_numpy(cm))
    assert got.dtype == torch.float64 and tuple(got.shape) == (K,)
    assert np.abs(got.numpy() - want).max() <= 1e-15
    assert float(got[3]) == 0.0                                       # a class absent from both: 0 / 1e-15, not NaN
    for ig in (0, 5, K - 1):
        g = metrics.dice_coefficient(torch.from_numpy(cm), ignore_index=ig).numpy()
        assert g.shape == (K - 1,) and np.abs(g - np.delete(want, ig)).max() <= 1e-15
    for bad in (-1, K, 1.0):
        with pytest.raises(ValueError, match="ignore_index"):
            metrics.dice_coefficient(torch.from_numpy(cm), ignore_index=bad)
    with pytest.raises(ValueError, match=r"\[K, K\]"):
        metrics.dice_coefficient(torch.zeros(3, 4))
    doc = metrics.summarise(torch.from_numpy(cm), [], K, 0)
    assert doc["confusion_matrix"] == cm.tolist() and doc["dice_classes"] == list(range(1, K))
    assert np.abs(np.array(doc["dice"]) - want[1:]).max() <= 1e-15 and abs(doc["mean_dice"] - want[1:].mean()) <= 1e-15


# ------------------------------------------------------------------------------------------------ C-ABI
def test_entry_rejects_bad_arguments_on_the_host():
    """No device here: every refusal comes from host code, before any launch."""
    from jointimagegeneration_amd import _lib
    lib = _lib.load()
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    bad = -1
    assert _lib.GG_ERR_BAD_SHAPE == -1
    f = lib.gg_label_confusion
    assert f(None, 1, p, 1, 8, 4, p, p, None) == bad and b"null" in lib.gg_last_error()
    assert f(p, 1, None, 1, 8, 4, p, p, None) == bad
    assert f(p, 1, p, 1, 8, 4, None, p, None) == bad
    for Sa, Sb, M in ((0, 1, 8), (1, 0, 8), (-3, 1, 8), (1, 1, 0), (1, 1, -1)):
        assert f(p, Sa, p, Sb, M, 4, p, p, None) == bad, (Sa, Sb, M)
    for K in (0, -1, 33, 256):
        assert f(p, 1, p, 1, 8, K, p, p, None) == bad, K
        assert b"K=" in lib.gg_last_error()


# ------------------------------------------------------------------------------------------------ Python refusals
def test_label_confusion_refuses_cpu_tensors():
    from jointimagegeneration_amd import metrics, ops
    a = torch.zeros(2, 4, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.label_confusion(a, a, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.generalised_energy_distance(a, a, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.confusion_matrix(a, a, 4)


def _params(tmp_path):
    import yaml
    from util import CCDM_SMALL
    params = dict(output_path=str(tmp_path), exp_name="t", evaluation_vote_strategy="majority", dataset_file="datasets.ruijin", batch_size=2,
                  dims=3, beta_schedule="cosine", beta_schedule_params=dict(s=0.008), time_steps=6, backbone="unet_openai",
                  feature_cond_encoder=dict(type="none"), unet_openai=dict(CCDM_SMALL))
    pf = tmp_path / "params_eval.yml"
    pf.write_text(yaml.safe_dump(params))
    return str(pf)


def test_ddpm_eval_refuses_a_bad_ground_truth_on_the_host(tmp_path):
    """A gt of another shape, or with a label >= K, is a ValueError before any sampling: it is raised here, where there is no device
    (a run that got past the check would stop at the entry point's own `needs an MI355X` assertion instead)."""
    from jointimagegeneration_amd import ddpm_eval, metrics
    from jointimagegeneration_amd.io import write_nifti
    size, K = (8, 16, 16), 4
    good = (np.arange(8 * 16 * 16).reshape(size) % K).astype(np.uint8)
    pf = _params(tmp_path)
    argv = [pf, "exp", "--size", *map(str, size), "--num-classes", str(K), "--num-volumes", "2", "--steps", "3"]

    shape_dir = tmp_path / "gt_shape"
    shape_dir.mkdir()
    write_nifti(str(shape_dir / "gt_0000.nii.gz"), good)
    write_nifti(str(shape_dir / "gt_0001.nii.gz"), good[:, :8])
    with pytest.raises(ValueError, match=r"gt_0001.*shape \(8, 8, 16\)"):
        ddpm_eval.main(argv + ["--gt", str(shape_dir)])

    range_dir = tmp_path / "gt_range"
    range_dir.mkdir()
    high = good.copy()
    high[3, 5, 7] = K
    write_nifti(str(range_dir / "gt_0000.nii.gz"), high)
    write_nifti(str(range_dir / "gt_0001.nii.gz"), good)
    with pytest.raises(ValueError, match=r"gt_0000.*labels in \[0, 4\]"):
        ddpm_eval.main(argv + ["--gt", str(range_dir)])
    with pytest.raises(ValueError, match="--samples"):
        ddpm_eval.main(argv + ["--samples", "0"])
    assert not (tmp_path / "exp").exists()                            # nothing was written

    got = metrics.load_gt(str(shape_dir), [0], size, K)
    assert got[0].dtype == np.int32 and np.array_equal(got[0], good)
    with pytest.raises(FileNotFoundError, match="gt_0007"):
        metrics.load_gt(str(shape_dir), [7], size, K)
    neg = tmp_path / "gt_neg"
    neg.mkdir()
    write_nifti(str(neg / "gt_0000.nii.gz"), good.astype(np.int16) - 1)
    with pytest.raises(ValueError, match=r"labels in \[-1, 2\]"):
        metrics.load_gt(str(neg), [0], size, K)
