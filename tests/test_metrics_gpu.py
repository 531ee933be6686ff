"""GPU suite for gg_label_confusion (gg_metrics.hip) and the scores built on it.  Every count is compared with `==` against
np.bincount(a * K + b, minlength=K * K) in int64: integer adds commute, so no tolerance applies below the fp64 formulas; those are held
to 1e-12 against the reference's numbers (tests/golden/metrics.npz) and Dice to 1e-15 against its formula."""
import gzip
import json
import os

import numpy as np
import pytest
import torch

from util import CCDM_SMALL, GOLD

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def bincount_cm(a, b, K):
    """Expectation: int64 [Sa, Sb, K, K] and [Sa, Sb] skipped counts; a voxel with either label outside [0, K) is left out of cm."""
    a, b = a.astype(np.int64), b.astype(np.int64)
    cm = np.zeros((a.shape[0], b.shape[0], K, K), dtype=np.int64)
    sk = np.zeros((a.shape[0], b.shape[0]), dtype=np.int64)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            ok = (x >= 0) & (x < K) & (y >= 0) & (y < K)
            cm[i, j] = np.bincount(x[ok] * K + y[ok], minlength=K * K).reshape(K, K)
            sk[i, j] = int((~ok).sum())
    return cm, sk


def raw_call(dev, a, b, K, cm=None, sk=None, same=False):
    """gg_label_confusion through _lib (no range check): numpy int32 [S, M] in, numpy (cm, skipped) out."""
    from jointimagegeneration_amd import _lib
    lib = _lib.load()
    ta = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    tb = ta if same else torch.from_numpy(np.ascontiguousarray(b, dtype=np.int32)).to(dev)
    Sa, Sb, M = ta.shape[0], tb.shape[0], ta.shape[1]
    if cm is None:
        cm = torch.full((Sa, Sb, K, K), -7, dtype=torch.int64, device=dev)       # the call zeroes its outputs itself
        sk = torch.full((Sa, Sb), -7, dtype=torch.int64, device=dev)
    _lib.check(lib.gg_label_confusion(ta.data_ptr(), Sa, tb.data_ptr(), Sb, M, K, cm.data_ptr(), sk.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream), "gg_label_confusion")
    torch.cuda.synchronize()
    return cm.cpu().numpy(), sk.cpu().numpy()


def mixed_labels(rng, S, M, K):
    """Mostly background, runs of one class of 1..300 voxels, and a sprinkle of random voxels: waves that are uniform in both rows, in
    one row, and in neither."""
    out = np.zeros((S, M), dtype=np.int32)
    for s in range(S):
        pos = 0
        while pos < M:
            run = int(rng.integers(1, 300))
            out[s, pos:pos + run] = rng.integers(0, K) if rng.random() < 0.4 else 0
            pos += run
        noise = rng.random(M) < 0.02
        out[s, noise] = rng.integers(0, K, size=int(noise.sum()))
    return out


@pytest.mark.parametrize("pairs", [(1, 1), (3, 5)], ids=["1x1", "3x5"])
@pytest.mark.parametrize("K", [1, 2, 14, 32])
def test_counts_equal_bincount_at_partial_waves_and_chunks(dev, K, pairs):
    rng = np.random.default_rng(100 * K + pairs[1])
    for M in (1, 63, 64, 65, 4099):                                   # partial wave, one wave, one more lane, more than one chunk
        a, b = mixed_labels(rng, pairs[0], M, K), rng.integers(0, K, size=(pairs[1], M)).astype(np.int32)
        want, _ = bincount_cm(a, b, K)
        cm, sk = raw_call(dev, a, b, K)
        assert (cm == want).all(), (K, pairs, M)
        assert (sk == 0).all() and cm.sum() == pairs[0] * pairs[1] * M


@pytest.mark.parametrize("K", [14, 32])
def test_twelve_by_twelve_pairs_cross_tile_edges(dev, K):
    """More pairs than one tile holds at either K (6 x 6 at K = 14, 3 x 3 at K = 32), over many workgroups."""
    rng = np.random.default_rng(K)
    M = 64 ** 3
    a, b = mixed_labels(rng, 12, M, K), mixed_labels(rng, 12, M, K)
    b[5] = rng.integers(0, K, size=M)
    want, _ = bincount_cm(a, b, K)
    cm, sk = raw_call(dev, a, b, K)
    assert (cm == want).all() and (sk == 0).all()


def test_label_patterns(dev):
    K, M = 14, 4099
    rng = np.random.default_rng(7)
    m = np.arange(M)
    runs = lambda S, shift: np.stack([((m + 27) // 64 + shift * s) % K for s in range(S)]).astype(np.int32)   # changes at 37, 101, ...
    last = lambda S: np.concatenate([np.zeros((S, M - 1), np.int32), np.arange(1, S + 1, dtype=np.int32)[:, None]], 1)
    cases = {"background": (np.zeros((3, M), np.int32), np.zeros((5, M), np.int32)),
             "uniform random": (rng.integers(0, K, (3, M)).astype(np.int32), rng.integers(0, K, (5, M)).astype(np.int32)),
             "runs of 64 changing mid-wave": (runs(3, 1), runs(5, 3)),
             "background but the last voxel": (last(3), last(5))}
    assert runs(1, 0)[0, 36] != runs(1, 0)[0, 37] and runs(1, 0)[0, 37] == runs(1, 0)[0, 100]
    for name, (a, b) in cases.items():
        want, _ = bincount_cm(a, b, K)
        cm, sk = raw_call(dev, a, b, K)
        assert (cm == want).all() and (sk == 0).all(), name
    cm, _ = raw_call(dev, *cases["background"], K)
    assert cm[2, 4, 0, 0] == M and cm.sum() == 15 * M


def test_self_pairs_on_one_buffer(dev):
    K, M = 14, 4099
    a = mixed_labels(np.random.default_rng(11), 4, M, K)
    cm, sk = raw_call(dev, a, None, K, same=True)
    want, _ = bincount_cm(a, a, K)
    assert (cm == want).all() and (sk == 0).all()
    for i in range(4):
        d = cm[i, i]
        assert d.sum() == M and (d == np.diag(np.diag(d))).all()
        assert (cm[i] == np.swapaxes(cm[:, i], -1, -2)).all()          # pair (i, j) is the transpose of pair (j, i)


def test_out_of_range_labels_are_skipped_and_refused(dev):
    from jointimagegeneration_amd import ops
    K, M = 14, 4099
    rng = np.random.default_rng(3)
    a, b = mixed_labels(rng, 3, M, K), rng.integers(0, K, size=(5, M)).astype(np.int32)
    a[0, 5], a[1, 100], a[1, 4098], a[2, 64] = -1, K, 255, -2 ** 31
    b[2, 5], b[2, 4098], b[4, 63] = -1, 255, K                        # (0, 2) voxel 5 and (1, 2) voxel 4098: both labels bad, counted once
    want, want_sk = bincount_cm(a, b, K)
    assert want_sk[0, 2] == 2 and want_sk[1, 2] == 3 and want_sk[0, 0] == 1 and want_sk[2, 4] == 2 and want_sk[0, 1] == 1
    cm, sk = raw_call(dev, a, b, K)
    assert (sk == want_sk).all()
    assert (cm == want).all()
    assert (cm.sum((2, 3)) + sk == M).all()
    with pytest.raises(ValueError, match=r"pair \(0, 0\) has 1 voxel"):
        ops.label_confusion(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), K)
    u8 = torch.zeros(2, 8, 8, dtype=torch.uint8, device=dev)
    u8[1, 7, 7] = 255
    with pytest.raises(ValueError, match=r"pair \(0, 1\) has 1 voxel"):
        ops.label_confusion(u8, u8, K)
    big = torch.zeros(1, 64, dtype=torch.int64, device=dev)
    big[0, 3] = 2 ** 32                                               # would wrap to 0 in int32
    with pytest.raises(ValueError, match="outside"):
        ops.label_confusion(big, big, K)


def test_second_call_into_the_same_buffers_and_python_plumbing(dev):
    from jointimagegeneration_amd import metrics, ops
    K = 14
    rng = np.random.default_rng(5)
    a, b = mixed_labels(rng, 3, 4099, K), mixed_labels(rng, 5, 4099, K)
    cm_t = torch.empty((3, 5, K, K), dtype=torch.int64, device=dev)
    sk_t = torch.empty((3, 5), dtype=torch.int64, device=dev)
    first = raw_call(dev, a, b, K, cm_t, sk_t)
    second = raw_call(dev, a, b, K, cm_t, sk_t)
    want, _ = bincount_cm(a, b, K)
    assert (first[0] == want).all() and (second[0] == want).all() and (second[1] == 0).all()
    # [S, *spatial] tensors of any integer dtype, non-contiguous included
    vol = torch.from_numpy(a[:, :4096].reshape(3, 16, 16, 16)).to(dev)
    ref, _ = bincount_cm(a[:, :4096], a[:, :4096], K)
    for t in (vol, vol.long(), vol.to(torch.uint8), vol.to(torch.int16)):
        got = ops.label_confusion(t, t, K)
        assert got.dtype == torch.int64 and tuple(got.shape) == (3, 3, K, K) and (got.cpu().numpy() == ref).all()
    tr = vol.transpose(1, 3)
    want_tr, _ = bincount_cm(tr.cpu().numpy().reshape(3, -1), a[:, :4096], K)
    assert (ops.label_confusion(tr, vol, K).cpu().numpy() == want_tr).all()
    assert (metrics.confusion_matrix(vol, vol.flip(0), K).cpu().numpy() == sum(ref[i, 2 - i] for i in range(3))).all()
    with pytest.raises(ValueError, match="voxels"):
        ops.label_confusion(vol, vol[:, :8], K)
    with pytest.raises(ValueError, match="K=33"):
        ops.label_confusion(vol, vol, 33)
    with pytest.raises(ValueError, match="integer"):
        ops.label_confusion(vol.float(), vol, K)


@pytest.mark.parametrize("name", ["k4", "k14"])
def test_energy_distance_and_hungarian_iou_on_the_device_equal_the_reference(dev, name):
    from jointimagegeneration_amd import metrics
    gold = np.load(os.path.join(GOLD, "metrics.npz"))
    K = int(gold[f"{name}_K"])
    for c in range(2):
        a, b = torch.from_numpy(gold[f"{name}_a"][c]).to(dev), torch.from_numpy(gold[f"{name}_b"][c]).to(dev)
        ged, d0, d1 = metrics.generalised_energy_distance(a, b, K)
        assert ged.is_cuda and ged.dtype == torch.float64
        got = dict(ged=float(ged), div0=float(d0), div1=float(d1), hm=metrics.hungarian_iou(a, b, K))
        for key, v in got.items():
            want = float(gold[f"{name}_{key}"][c])
            print(f"{name} case {c} {key}: got {v!r} want {want!r} diff {abs(v - want):.3e}")
            assert abs(v - want) <= 1e-12, (name, c, key, v, want)


def _payload(path):
    """The NIfTI bytes of a .nii.gz (the gzip header carries the time of writing, so the compressed files are compared unpacked)."""
    with open(path, "rb") as f:
        return gzip.decompress(f.read())


def test_ddpm_eval_scores_its_run_and_stays_as_it_was_without_the_options(dev, tmp_path):
    import yaml
    from jointimagegeneration_amd import ddpm_eval, metrics
    from jointimagegeneration_amd.io import read_nifti, write_nifti
    size, K, S, nvol = (8, 16, 16), 4, 3, 2
    params = dict(output_path=str(tmp_path), exp_name="t", evaluation_vote_strategy="majority", dataset_file="datasets.ruijin", batch_size=2,
                  dims=3, beta_schedule="cosine", beta_schedule_params=dict(s=0.008), time_steps=6, backbone="unet_openai",
                  feature_cond_encoder=dict(type="none"), unet_openai=dict(CCDM_SMALL))
    pf = tmp_path / "params_eval.yml"
    pf.write_text(yaml.safe_dump(params))
    gt_dir = tmp_path / "gt"
    gt_dir.mkdir()
    rng = np.random.default_rng(9)
    gts = [mixed_labels(rng, 1, 8 * 16 * 16, K).reshape(size).astype(np.uint8) for _ in range(nvol)]
    for vid, g in enumerate(gts):
        write_nifti(str(gt_dir / f"gt_{vid:04d}.nii.gz"), g)
    common = [str(pf), "--size", *map(str, size), "--num-classes", str(K), "--num-volumes", str(nvol), "--steps", "3"]

    ddpm_eval.main(common[:1] + ["scored"] + common[1:] + ["--samples", str(S), "--gt", str(gt_dir)])
    out = tmp_path / "scored"
    assert sorted(os.listdir(out)) == sorted([f"pred_{v:04d}_s{j:02d}.nii.gz" for v in range(nvol) for j in range(S)] + ["metrics.json"])
    doc = json.loads((out / "metrics.json").read_text())
    want = np.zeros((K, K), dtype=np.int64)
    preds = {}
    for v in range(nvol):
        preds[v] = np.stack([read_nifti(str(out / f"pred_{v:04d}_s{j:02d}.nii.gz")) for j in range(S)])
        for p in preds[v]:
            want += np.bincount(gts[v].reshape(-1).astype(np.int64) * K + p.reshape(-1), minlength=K * K).reshape(K, K)
    assert not np.array_equal(preds[0][0], preds[0][1]) and not np.array_equal(preds[0][0], preds[1][0])      # independent chains
    assert doc["confusion_matrix"] == want.tolist() and want.sum() == nvol * S * 8 * 16 * 16
    c = want.astype(np.float64)
    dice = 2.0 * np.diag(c) / (c.sum(1) + c.sum(0) + 1e-15)
    assert doc["ignore_class"] == 0 and doc["dice_classes"] == [1, 2, 3]
    assert np.abs(np.array(doc["dice"]) - dice[1:]).max() <= 1e-15 and abs(doc["mean_dice"] - dice[1:].mean()) <= 1e-15
    assert [v["id"] for v in doc["volumes"]] == [0, 1]
    for v in doc["volumes"]:                                           # the per-volume scores are those of the files, recomputed here
        p, g = torch.from_numpy(preds[v["id"]].astype(np.int32)).to(dev), torch.from_numpy(gts[v["id"]].astype(np.int32)).to(dev)[None]
        ged, d0, d1 = metrics.generalised_energy_distance(p, g, K)
        assert v["samples"] == S and abs(v["ged"] - float(ged)) <= 1e-12 and abs(v["diversity_pred"] - float(d0)) <= 1e-12
        assert v["diversity_gt"] == 0.0 == float(d1) and abs(v["hm_iou"] - metrics.hungarian_iou(p, g, K)) <= 1e-12
    # the stand-alone scorer reads the same files and reports the same document
    again = metrics.main(["--pred", str(out), "--gt", str(gt_dir), "--num-classes", str(K), "--out", str(tmp_path / "again.json")])
    assert again["confusion_matrix"] == doc["confusion_matrix"] and again["dice"] == doc["dice"]
    for v, w in zip(again["volumes"], doc["volumes"]):
        assert abs(v["ged"] - w["ged"]) <= 1e-12 and abs(v["hm_iou"] - w["hm_iou"]) <= 1e-12

    # without the options: the files, names and voxels of a run before they existed (one chain per volume, seeds 1024 + vid)
    ddpm_eval.main(common[:1] + ["plain"] + common[1:])
    plain = tmp_path / "plain"
    assert sorted(os.listdir(plain)) == [f"pred_{v:04d}.nii.gz" for v in range(nvol)]
    model = ddpm_eval.build_from_params(dict(params), size, K).eval()
    ddpm_eval.load_weights(model, params, log=lambda m: None)
    model = model.to(dev)
    for vid in range(nvol):
        g = torch.Generator(device=dev).manual_seed(1024 + vid)
        x_T = torch.randint(0, K, (1,) + size, generator=g, device=dev, dtype=torch.int32)
        model.philox_seed = 1024 + vid
        labels, _ = model.sample_labels(x_T, torch.zeros((1, 1) + size, device=dev), 10003)
        ref = tmp_path / f"ref_{vid:04d}.nii.gz"
        write_nifti(str(ref), labels[0].to(torch.uint8).cpu().numpy())
        assert _payload(str(plain / f"pred_{vid:04d}.nii.gz")) == _payload(str(ref)), vid
    # --gt alone scores the single chain: Dice only, no ensemble scores
    ddpm_eval.main(common[:1] + ["single"] + common[1:] + ["--gt", str(gt_dir), "--ignore-class", "2"])
    single = json.loads((tmp_path / "single" / "metrics.json").read_text())
    w1 = sum(np.bincount(gts[v].reshape(-1).astype(np.int64) * K + read_nifti(str(tmp_path / "single" / f"pred_{v:04d}.nii.gz")).reshape(-1),
                         minlength=K * K).reshape(K, K) for v in range(nvol))
    assert single["confusion_matrix"] == w1.tolist() and single["dice_classes"] == [0, 1, 3] and "ged" not in single["volumes"][0]
    for vid in range(nvol):
        assert _payload(str(tmp_path / "single" / f"pred_{vid:04d}.nii.gz")) == _payload(str(plain / f"pred_{vid:04d}.nii.gz"))
