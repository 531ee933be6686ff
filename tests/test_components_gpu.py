"""GPU suite for gg_components.hip (vote, connected components, stats, filter) and the layers above it (ops, postprocess, ddpm_eval).
Every comparison is exact: integer outputs with `==` against tests/components_ref.py and the scipy fixture (tests/golden/
components.npz), the vote's fp32 entropy bit for bit against the same recipe in numpy fp32.  There is no tolerance anywhere below.
The device status word of the component kernels is read after every test and must be 0."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import components_ref as R
from util import CCDM_SMALL, GOLD

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "components.npz"), allow_pickle=False)


@pytest.fixture(autouse=True)
def status_stays_zero(dev):
    yield
    from jointimagegeneration_amd import ops
    torch.cuda.synchronize()
    ops.check_component_status(dev)                    # raises if a find / union / flatten loop reached its bound


def gpu_components(dev, labels, K, conn, background=0):
    """(root, size, stats) as numpy through the ops layer."""
    from jointimagegeneration_amd import ops
    t = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(dev)
    root = ops.label_components(t, K, conn, background)
    size, stats = ops.component_stats(t, root, K)
    return root.cpu().numpy(), size.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize("conn", [6, 26])
def test_roots_sizes_and_stats_equal_scipy_on_every_fixture_case(dev, gold, conn):
    """Shapes (1,1,1), (1,1,70), (5,6,7), (3,4,130), (33,17,9), (16,16,16) x background / one class / random K = 2 and 14 at density
    0.32 / checkerboard; the serpentine, combs, U shapes, corner-only and edge-only contacts, row-wrap traps, the two equal largest
    components, B = 3 with equal classes across the volume boundary, labels outside [0, K)."""
    for name, (labels, K) in R.fixture_cases().items():
        want = gold[f"{name}__root{conn}"]
        root, size, stats = gpu_components(dev, labels, K, conn)
        assert root.dtype == np.int32 and np.array_equal(root, want), (name, conn)
        want_size, want_stats = R.sizes_and_stats(np.where((labels >= 0) & (labels < K), labels, 0), want, K)
        assert np.array_equal(size, want_size) and np.array_equal(stats, want_stats), (name, conn)
    labels, K = R.fixture_cases()["tie"]
    assert gpu_components(dev, labels, K, 6)[2][0, 1].tolist() == [3, 10, 4, 0]            # equal sizes: the smaller root


@pytest.mark.parametrize("conn", [6, 26])
def test_random_64_cube_equals_scipy(dev, gold, conn):
    """Density 0.32 at 64^3: thousands of islands and one tortuous cluster through the whole grid of workgroups."""
    big = R.random_labels((1, 64, 64, 64), 2, 64)
    root, size, stats = gpu_components(dev, big, 2, conn)
    assert np.array_equal(stats, gold[f"random64__stats{conn}"])
    assert np.array_equal(np.frombuffer(hashlib.sha256(root.tobytes()).digest(), dtype=np.uint8), gold[f"random64__sha{conn}"])
    assert int(size.sum()) == int((big == 1).sum()) and int((size > 0).sum()) == int(stats[0, 1, 0])


def test_no_background_class_and_other_background(dev):
    labels, K = R.fixture_cases()["random_k14_5x6x7"]
    for background in (-1, 3):
        for conn in (6, 26):
            want = R.roots(labels, K, conn, background)
            root, size, stats = gpu_components(dev, labels, K, conn, background)
            assert np.array_equal(root, want)
            want_size, want_stats = R.sizes_and_stats(labels, want, K)
            assert np.array_equal(size, want_size) and np.array_equal(stats, want_stats)
    assert (R.roots(labels, K, 6, -1) >= 0).all()


def _filter(dev, labels, K, keep_largest, min_size, conn=6, background=0, fill=None):
    from jointimagegeneration_amd import ops
    t = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(dev)
    root = ops.label_components(t, K, conn, background)
    size, stats = ops.component_stats(t, root, K)
    out, kept = ops.component_filter(t, root, size, stats, K, torch.tensor(keep_largest, dtype=torch.int32, device=dev),
                                     torch.tensor(min_size, dtype=torch.int32, device=dev), background, fill)
    assert out.shape == t.shape and kept.shape == t.shape and kept.dtype == torch.uint8 and out.dtype == torch.int32
    want = R.filter_labels(labels, root.cpu().numpy(), size.cpu().numpy(), stats.cpu().numpy(), K, keep_largest, min_size, background, fill)
    return out.cpu().numpy(), kept.cpu().numpy(), want


def test_filter_thresholds_policies_fill_and_kept(dev):
    labels, K = R.fixture_cases()["tie"]                                                  # class 1: sizes 4, 4, 2; class 2: 3, 2, 1
    out, kept, want = _filter(dev, labels, K, [0, 1, 0], [0, 0, 2])
    assert np.array_equal(out, want[0]) and np.array_equal(kept, want[1])
    assert int((out == 1).sum()) == 4 and out[0, 0, 0, 0] == 1 and out[0, 4, 5, 6] == 0   # the tie goes to the smaller root
    assert int((out == 2).sum()) == 5 and out[0, 3, 0, 5] == 2 and out[0, 4, 0, 0] == 0   # size == min_size stays, min_size - 1 goes
    assert np.array_equal(kept, (out == labels).astype(np.uint8))
    out, kept, want = _filter(dev, labels, K, [0, 0, 0], [0, 5, 3], fill=2)               # fill with a class: nothing of class 1 survives
    assert np.array_equal(out, want[0]) and np.array_equal(kept, want[1]) and int((out == 1).sum()) == 0 and int((out == 2).sum()) == 16
    assert int(kept.sum()) == 210 - 16 + 3                                                # a class-2 voxel filled with 2 is not 'kept'
    out, kept, want = _filter(dev, labels, K, [0, 0, 0], [0, 0, 0])                       # no policy: the input, every voxel kept
    assert np.array_equal(out, labels) and kept.all()
    for name in ("random_k14_33x17x9", "batch3_16x16x16", "batch3_5x6x7", "out_of_range", "checkerboard_5x6x7"):
        labels, K = R.fixture_cases()[name]
        rng = np.random.default_rng(K)
        keep_largest, min_size = rng.integers(0, 2, K).tolist(), rng.integers(0, 4, K).tolist()
        for conn in (6, 26):
            out, kept, want = _filter(dev, labels, K, keep_largest, min_size, conn)
            assert np.array_equal(out, want[0]) and np.array_equal(kept, want[1]), (name, conn)
    labels, K = R.fixture_cases()["out_of_range"]
    out, kept, _ = _filter(dev, labels, K, [0] * K, [0] * K)
    assert out[0, 0, 0, 0] == 0 and out[0, 0, 0, 1] == 0 and kept[0, 0, 0, 0] == 0 and out.min() >= 0 and out.max() < K


def test_clean_leaves_one_component_per_class_and_is_idempotent(dev):
    from jointimagegeneration_amd import postprocess
    for name in ("random_k14_16x16x16", "batch3_16x16x16", "u_shapes_16x16x16", "comb_3x4x130"):
        labels, K = R.fixture_cases()[name]
        t = torch.from_numpy(labels).to(dev)
        for conn in (6, 26):
            out, kept, before, after = postprocess.clean(t, K, largest="all", connectivity=conn)
            root = R.roots(labels, K, conn)
            size, stats = R.sizes_and_stats(labels, root, K)
            want, want_kept = R.filter_labels(labels, root, size, stats, K, [0] + [1] * (K - 1), [0] * K)
            assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(kept.cpu().numpy(), want_kept)
            for b in range(labels.shape[0]):
                assert all(c["components"] <= 1 for c in after[b]["classes"]) and after[b]["stray_voxels"] == 0
                assert before[b]["stray_voxels"] == int((want_kept[b] == 0).sum()) == int((stats[b, :, 1] - stats[b, :, 2]).sum())
                assert [c["components"] for c in before[b]["classes"]] == stats[b, :, 0].tolist()
            again, kept2, b2, a2 = postprocess.clean(out, K, largest="all", connectivity=conn)
            assert torch.equal(again, out) and bool(kept2.all()) and b2 == after and a2 == after
    # a single [D, H, W] volume, other integer dtypes, per-class minimum sizes
    labels, K = R.fixture_cases()["tie"]
    out, kept, before, after = postprocess.clean(torch.from_numpy(labels[0]).to(dev).to(torch.uint8), K, largest=[1], min_size={2: 2})
    assert tuple(out.shape) == (5, 6, 7) and isinstance(before, dict) and before["classes"][1]["components"] == 3
    assert after["classes"][1] == dict(label=1, components=1, voxels=4, largest=4, largest_fraction=1.0) and after["classes"][2]["components"] == 2
    assert postprocess.component_scores(out, K) == after


@pytest.mark.parametrize("K", [2, 14, 32])
@pytest.mark.parametrize("S", [1, 2, 5, 64])
def test_vote_equals_reference_bit_for_bit(dev, S, K):
    from jointimagegeneration_amd import ops
    rng = np.random.default_rng(1000 * S + K)
    for M in (1, 63, 64, 65, 4097):
        lab = rng.integers(0, K, size=(S, M)).astype(np.int32)
        if M >= 63:
            lab[:, 3] = np.arange(S) % 2 * (K - 1)                       # a tie between the first and the last class (S even)
            lab[:, 5] = K - 1                                            # unanimous
            lab[:, 7] = rng.integers(0, min(K, 3), size=S)               # few classes: large counts
            lab[:, 11] = -1 if S > 1 else K                              # no valid vote
            lab[0, 13], lab[S - 1, 17] = K, -2 ** 31                     # single bad votes
        want_w, want_a, want_h, want_sk = R.vote(lab, K)
        w, a, h, sk = ops.label_vote(torch.from_numpy(lab).to(dev), K)
        assert w.dtype == torch.int32 and a.dtype == torch.int32 and h.dtype == torch.float32 and sk.dtype == torch.int64
        assert np.array_equal(w.cpu().numpy(), want_w) and np.array_equal(a.cpu().numpy(), want_a), (S, K, M)
        assert np.array_equal(h.cpu().numpy().view(np.uint32), want_h.view(np.uint32)), (S, K, M)
        assert int(sk.item()) == want_sk
        if M >= 63:
            assert w[11] == 0 and a[11] == 0 and h[11] == 0.0
            if S % 2 == 0:
                assert w[3] == 0 and a[3] == S // 2
        if S == 1:
            ok = (lab[0] >= 0) & (lab[0] < K)
            assert np.array_equal(w.cpu().numpy()[ok], lab[0][ok]) and bool((h == 0).all())


def test_consensus_refuses_bad_labels_and_shapes_its_outputs(dev):
    from jointimagegeneration_amd import postprocess
    lab = torch.from_numpy(R.random_labels((5, 5, 6, 7), 4, 3)).to(dev)
    w, a, h = postprocess.consensus(lab.long(), 4)
    ww, wa, wh, _ = R.vote(lab.cpu().numpy().reshape(5, -1), 4)
    assert tuple(w.shape) == (5, 6, 7) and np.array_equal(w.cpu().numpy().reshape(-1), ww) and np.array_equal(a.cpu().numpy().reshape(-1), wa)
    assert np.array_equal(h.cpu().numpy().reshape(-1).view(np.uint32), wh.view(np.uint32))
    s = postprocess.consensus_summary(a, h, 5)
    assert s["samples"] == 5 and abs(s["mean_entropy"] - wh.astype(np.float64).mean()) < 1e-12
    assert abs(s["mean_agreement"] - wa.mean() / 5) < 1e-12 and s["unanimous_fraction"] == float((wa == 5).mean())
    lab[2, 1, 1, 1] = 9
    with pytest.raises(ValueError, match="1 vote"):
        postprocess.consensus(lab, 4)


def test_vote_components_stats_filter_captured_once_and_replayed(dev):
    from jointimagegeneration_amd import ops
    S, K, shape = 5, 6, (1, 9, 10, 11)
    M = int(np.prod(shape))
    rng = np.random.default_rng(21)

    def draw():                                                          # correlated samples: a base mask and per-sample noise
        base = R.random_labels(shape, K, int(rng.integers(1 << 30)), density=0.6).reshape(-1)
        lab = np.repeat(base[None], S, 0)
        noise = rng.random((S, M)) < 0.3
        lab[noise] = rng.integers(0, K, size=int(noise.sum()))
        return lab.astype(np.int32)

    keep_largest = torch.tensor([0, 1, 1, 0, 1, 1], dtype=torch.int32, device=dev)
    min_size = torch.tensor([0, 0, 2, 3, 0, 1], dtype=torch.int32, device=dev)
    static = torch.from_numpy(draw()).to(dev)

    def chain():
        w, a, h, sk = ops.label_vote(static, K)
        vol = w.reshape(shape)
        root = ops.label_components(vol, K, 26)
        size, stats = ops.component_stats(vol, root, K)
        out, kept = ops.component_filter(vol, root, size, stats, K, keep_largest, min_size)
        return w, a, h, sk, root, size, stats, out, kept

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                          # warm-up: the vote table and the status word exist before capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = chain()
    for _ in range(2):                                                   # new contents of the same buffer
        static.copy_(torch.from_numpy(draw()).to(dev))
        g.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in captured]
        eager = chain()
        for x, y in zip(got, eager):
            assert torch.equal(x.view(torch.uint8) if x.dtype == torch.float32 else x, y.view(torch.uint8) if y.dtype == torch.float32 else y)
        lab = static.cpu().numpy()
        ww, wa, wh, _ = R.vote(lab, K)
        assert np.array_equal(got[0].cpu().numpy(), ww) and np.array_equal(got[2].cpu().numpy().view(np.uint32), wh.view(np.uint32))
        assert np.array_equal(got[4].cpu().numpy(), R.roots(ww.reshape(shape), K, 26))


def test_sampled_masks_to_consensus_to_clean_and_ddpm_eval_blocks(dev, tmp_path):
    """End to end with the small CCDM: S = 4 masks -> consensus -> clean through the pipeline object, then ddpm_eval with the new flags:
    the new files exist, and the metrics.json blocks are the scores of those files read back."""
    import yaml
    from jointimagegeneration_amd import ddpm_eval, postprocess
    from jointimagegeneration_amd.io import read_nifti, write_nifti
    from jointimagegeneration_amd.pipeline import GuideGenPipeline
    from test_full_size_configs import _small_ccdm
    pipe = GuideGenPipeline.__new__(GuideGenPipeline)                    # the mask stage alone: no LDM is built
    pipe.ccdm, pipe.stats = _small_ccdm(dev, T_steps=6, K=6), {}
    masks = pipe.sample_masks([11, 12, 13, 14], (8, 16, 16), None)
    winner, agreement, entropy = postprocess.consensus(masks, 6)
    ww, wa, wh, _ = R.vote(masks.cpu().numpy().reshape(4, -1), 6)
    assert np.array_equal(winner.cpu().numpy().reshape(-1), ww) and np.array_equal(entropy.cpu().numpy().reshape(-1).view(np.uint32), wh.view(np.uint32))
    out, kept, before, after = pipe.clean_masks(winner[None], largest="all", min_size=2)
    lab = ww.reshape(1, 8, 16, 16)
    root = R.roots(lab, 6)
    size, stats = R.sizes_and_stats(lab, root, 6)
    want, want_kept = R.filter_labels(lab, root, size, stats, 6, [0, 1, 1, 1, 1, 1], [2] * 6)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(kept.cpu().numpy(), want_kept) and kept.shape == masks[:1].shape
    assert pipe.stats["mask_cleanup"] == dict(before=before, after=after) and after[0]["stray_voxels"] == 0

    size3, K, S, nvol = (8, 16, 16), 4, 4, 2
    params = dict(output_path=str(tmp_path), exp_name="t", evaluation_vote_strategy="majority", dataset_file="datasets.ruijin", batch_size=2,
                  dims=3, beta_schedule="cosine", beta_schedule_params=dict(s=0.008), time_steps=6, backbone="unet_openai",
                  feature_cond_encoder=dict(type="none"), unet_openai=dict(CCDM_SMALL))
    pf = tmp_path / "params_eval.yml"
    pf.write_text(yaml.safe_dump(params))
    gt_dir = tmp_path / "gt"
    gt_dir.mkdir()
    gts = [R.random_labels(size3, K, 30 + v, density=0.5).astype(np.uint8) for v in range(nvol)]
    for vid, g in enumerate(gts):
        write_nifti(str(gt_dir / f"gt_{vid:04d}.nii.gz"), g)
    ddpm_eval.main([str(pf), "run", "--size", *map(str, size3), "--num-classes", str(K), "--num-volumes", str(nvol), "--steps", "3",
                    "--samples", str(S), "--gt", str(gt_dir), "--consensus", "--largest-component", "all", "--min-component", "2",
                    "--connectivity", "26"])
    run = tmp_path / "run"
    names = [f"pred_{v:04d}_s{j:02d}.nii.gz" for v in range(nvol) for j in range(S)]
    names += [f"{kind}_{v:04d}.nii.gz" for v in range(nvol) for kind in ("consensus", "entropy", "clean")] + ["metrics.json"]
    assert sorted(os.listdir(run)) == sorted(names)
    doc = json.loads((run / "metrics.json").read_text())
    assert {"confusion_matrix", "dice", "mean_dice", "volumes"} <= set(doc)          # the existing keys are still there
    assert doc["components"]["largest"] == "all" and doc["components"]["min_size"] == 2 and doc["components"]["connectivity"] == 26
    cm_cons, cm_clean = np.zeros((K, K), np.int64), np.zeros((K, K), np.int64)
    ent_means, agr_means, unan = [], [], []
    for v in range(nvol):
        preds = np.stack([read_nifti(str(run / f"pred_{v:04d}_s{j:02d}.nii.gz")) for j in range(S)]).astype(np.int32)
        ww, wa, wh, _ = R.vote(preds.reshape(S, -1), K)
        cons, ent, cl = (read_nifti(str(run / f"{kind}_{v:04d}.nii.gz")) for kind in ("consensus", "entropy", "clean"))
        assert np.array_equal(cons.reshape(-1), ww) and ent.dtype == np.float32 and np.array_equal(ent.reshape(-1).view(np.uint32), wh.view(np.uint32))
        lab = cons.astype(np.int32)[None]
        root = R.roots(lab, K, 26)
        sz, st = R.sizes_and_stats(lab, root, K)
        want, _ = R.filter_labels(lab, root, sz, st, K, [0, 1, 1, 1], [2] * K)
        assert np.array_equal(cl.astype(np.int32)[None], want)
        block = doc["components"]["volumes"][v]
        assert block["id"] == v
        assert block["before"] == postprocess.component_scores(torch.from_numpy(cons.astype(np.int32)).to(dev), K, 26)
        assert block["after"] == postprocess.component_scores(torch.from_numpy(cl.astype(np.int32)).to(dev), K, 26)
        assert all(c["components"] <= 1 for c in block["after"]["classes"])
        cv = doc["consensus"]["volumes"][v]
        assert abs(cv["mean_entropy"] - wh.astype(np.float64).mean()) < 1e-12 and abs(cv["mean_agreement"] - wa.mean() / S) < 1e-12
        assert cv["unanimous_fraction"] == float((wa == S).mean())
        ent_means.append(cv["mean_entropy"]); agr_means.append(cv["mean_agreement"]); unan.append(cv["unanimous_fraction"])
        g = gts[v].reshape(-1).astype(np.int64)
        cm_cons += np.bincount(g * K + cons.reshape(-1), minlength=K * K).reshape(K, K)
        cm_clean += np.bincount(g * K + cl.reshape(-1), minlength=K * K).reshape(K, K)
    c = doc["consensus"]
    assert c["samples"] == S and abs(c["mean_entropy"] - np.mean(ent_means)) < 1e-12 and abs(c["mean_agreement"] - np.mean(agr_means)) < 1e-12
    assert abs(c["unanimous_fraction"] - np.mean(unan)) < 1e-12
    for key, cm in (("consensus", cm_cons), ("clean", cm_clean)):
        cf = cm.astype(np.float64)
        dice = 2.0 * np.diag(cf) / (cf.sum(1) + cf.sum(0) + 1e-15)
        assert np.abs(np.array(doc[f"dice_{key}"]) - dice[1:]).max() <= 1e-15 and abs(doc[f"mean_dice_{key}"] - dice[1:].mean()) <= 1e-15
    # the stand-alone tool on the same prediction files writes the same masks
    pdoc = postprocess.main(["--pred", str(run), "--num-classes", str(K), "--samples", str(S), "--largest-component", "all", "--min-component", "2",
                             "--connectivity", "26", "--out", str(tmp_path / "post")])
    for v in range(nvol):
        for kind in ("consensus", "entropy", "clean"):
            assert np.array_equal(read_nifti(str(tmp_path / "post" / f"{kind}_{v:04d}.nii.gz")), read_nifti(str(run / f"{kind}_{v:04d}.nii.gz")))
        assert pdoc["volumes"][v]["components"]["after"] == doc["components"]["volumes"][v]["after"]


def test_sample_diffusion_inputs_are_cleaned_before_the_slice_loop(dev, tmp_path, monkeypatch):
    """`sample_diffusion --inputs DIR --largest-component ... --min-component V`, the sampler stubbed (sampling is covered elsewhere):
    the slice loop is conditioned on the cleaned stage-1 mask, and metrics.json records the cleanup.  Without the options the
    conditioning is that of the raw mask and no metrics.json is written."""
    from jointimagegeneration_amd import sample_diffusion as sd
    from jointimagegeneration_amd.io import write_nifti
    (tmp_path / "m.yaml").write_text("model:\n  target: none\n")
    labels, K = R.fixture_cases()["tie"]
    inputs = tmp_path / "stage1"
    inputs.mkdir()
    write_nifti(str(inputs / "pred_0000.nii.gz"), labels[0].astype(np.uint8))
    seen = {}

    def fake_sample_cond(model, instance, n_samples=1, **kw):
        seen["wholemask"] = instance["wholemask"][0, ..., 0].clone()
        return torch.stack([torch.zeros_like(seen["wholemask"]), seen["wholemask"]])[None].to(dev)
    monkeypatch.setattr(sd, "load_model", lambda config, ckpt: (object(), 3))
    monkeypatch.setattr(sd, "sample_cond", fake_sample_cond)
    monkeypatch.chdir(tmp_path)
    common = ["--config", str(tmp_path / "m.yaml"), "--inputs", str(inputs), "--slices", "5", "--size", "12"]
    sd.main(common)
    raw = seen["wholemask"].cpu()
    out = tmp_path / "samples" / "00000003"
    assert sorted(os.listdir(out)) == ["pred_0000_0000.nii.gz"]
    sd.main(common + ["--largest-component", "1", "--min-component", "2"])
    assert sorted(os.listdir(out)) == ["metrics.json", "pred_0000_0000.nii.gz"]
    root = R.roots(labels, K)
    size, stats = R.sizes_and_stats(labels, root, K)
    want, want_kept = R.filter_labels(labels, root, size, stats, K, [0, 1, 0], [2, 2, 2])
    assert torch.equal(seen["wholemask"].cpu(), sd.stage1_mask_to_wholemask(want[0].astype(np.uint8), 5, 12).cpu())
    assert torch.equal(raw, sd.stage1_mask_to_wholemask(labels[0].astype(np.uint8), 5, 12).cpu()) and not torch.equal(raw, seen["wholemask"].cpu())
    doc = json.loads((out / "metrics.json").read_text())["mask_cleanup"]
    assert doc["largest"] == [1] and doc["min_size"] == 2 and doc["connectivity"] == 6 and len(doc["volumes"]) == 1
    v = doc["volumes"][0]
    assert v["volume"] == "pred_0000" and v["num_classes"] == 3 and v["removed_voxels"] == int((want_kept == 0).sum()) == 7
    assert [c["components"] for c in v["before"]["classes"]] == [0, 3, 3] and [c["components"] for c in v["after"]["classes"]] == [0, 1, 2]
