"""GPU suite of the three-view LPIPS (csrc/gg_lpips.hip, jointimagegeneration_amd/lpips.py).

gg_volume_views_cl, gg_relu_cl and the pooled outputs of gg_lpips_tap round nothing beyond one cast: compared with torch.equal.  The
distances of gg_lpips_tap are held to 2e-5 (the project's fp32-validation bound; the rule is written once, as LPIPS_TAP_RTOL of
tests/shadow.py, which applies it to every tap call of the network) relative to an fp64 restatement on the same inputs; end
to end under ops.fp32_validation() every recorded value of the reference (tests/golden/lpips.npz) is held to the same 2e-5.  The bf16
path has no bound that can be derived in advance; BF16_BOUND below is twice the largest deviation measured."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_ref as R  # noqa: E402
from shadow import LPIPS_TAP_RTOL  # noqa: E402

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = LPIPS_TAP_RTOL     # 2e-5
BF16_BOUND = 2.26e-3     # 2 x 1.128e-3, the largest entry of the bf16 table in DESIGN.md 7g (the factor 2: kernel path selection may differ between boxes)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "lpips.npz")))


@pytest.fixture(scope="module")
def weight_files(gold, tmp_path_factory):
    d = tmp_path_factory.mktemp("lpips_weights")
    torch.save(R.seeded_vgg_state_dict(), d / "vgg.pth")
    torch.save({f"lin{k}.model.1.weight": torch.from_numpy(gold[f"lin{k}"]).reshape(1, -1, 1, 1) for k in range(5)}, d / "lin.pth")
    return str(d / "vgg.pth"), str(d / "lin.pth")


@pytest.fixture(scope="module")
def model(dev, weight_files):
    from jointimagegeneration_amd.lpips import LPIPS
    return LPIPS.load(*weight_files).to(dev)


@pytest.fixture(scope="module")
def vols(dev, gold):
    return torch.from_numpy(gold["pred"]).to(dev), torch.from_numpy(gold["gt"]).to(dev)


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want) / np.abs(want)))


# ------------------------------------------------------------------------------------------------ gg_volume_views_cl
SHIFT = torch.tensor(R.SHIFT, dtype=torch.float32)
SCALE = torch.tensor(R.SCALE, dtype=torch.float32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("view,n0,n1", [(0, 0, 32), (1, 0, 40), (2, 0, 80), (0, 13, 19), (1, 17, 26), (2, 30, 67), (2, 79, 80)])
def test_views_equal_torch_bit_for_bit(dev, view, n0, n1, dtype):
    """b = 2, D = 16, H = 20, W = 40: three unequal extents, so a swapped axis changes the answer; the partial ranges start and end
    mid-volume, straddle the two volumes, and (view 2) cut the 32-image tiles of the LDS kernel."""
    from jointimagegeneration_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 16, 20, 40, generator=g) * 1.5 - 0.25
    imgs = R.views(x[:, None])[view][n0:n1]                                  # [n, 1, hh, ww]: the reference's rearrange
    want = ((imgs - SHIFT[None, :, None, None]) / SCALE[None, :, None, None]).permute(0, 2, 3, 1)      # fp32 on the CPU: IEEE
    n, hh, ww = want.shape[:3]
    out = torch.full((n, 1, hh, ww, 32), 7.0, dtype=dtype, device=dev)
    cl = ops.volume_views_cl(x.to(dev), view, n0, n1, SHIFT.to(dev), SCALE.to(dev), out)
    assert cl.C == 3 and cl.t.data_ptr() == out.data_ptr()
    got = out.cpu()[:, 0]
    assert torch.equal(got[..., :3], want.to(dtype))
    assert torch.equal(got[..., 3:], torch.zeros_like(got[..., 3:]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_three_channel_images_are_scaled_per_channel(dev, dtype):
    from jointimagegeneration_amd import ops
    x = torch.rand(3, 3, 5, 7, generator=torch.Generator().manual_seed(4))
    want = R.scaling(x).permute(0, 2, 3, 1)[1:3]
    out = torch.full((2, 1, 5, 7, 32), 7.0, dtype=dtype, device=dev)
    ops.volume_views_cl(x.to(dev), 3, 1, 3, SHIFT.to(dev), SCALE.to(dev), out)
    assert torch.equal(out.cpu()[:, 0, :, :, :3], want.to(dtype)) and float(out[..., 3:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ gg_relu_cl
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 32), (3, 1, 5, 3, 64), (2, 1, 20, 40, 512)])
def test_relu_equals_torch(dev, shape, dtype):
    from jointimagegeneration_amd import ops
    x = torch.randn(shape, generator=torch.Generator().manual_seed(5)).to(dtype).to(dev)
    want = F.relu(x)
    got = ops.relu_cl(ops.CL(x, shape[-1]))
    assert got.t.data_ptr() == x.data_ptr() and torch.equal(x, want) and float(x.min()) == 0.0


# ------------------------------------------------------------------------------------------------ gg_lpips_tap
def tap_inputs(dev, n, h, w, C, dtype, seed):
    """Pre-ReLU rows with the row cases in them (where the image has room): pixel 0 all zero in a, pixel 1 all zero in both, pixel 2 all
    negative in both, pixel 3 all negative in b only."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, 1, h, w, C, generator=g) + 0.3
    b = a + 0.5 * torch.randn(n, 1, h, w, C, generator=g)
    fa, fb = a.view(n, h * w, C), b.view(n, h * w, C)
    if h * w >= 8:
        fa[:, 0] = 0.0
        fa[:, 1] = 0.0
        fb[:, 1] = 0.0
        fa[:, 2] = -fa[:, 2].abs() - 0.1
        fb[:, 2] = -fb[:, 2].abs() - 0.1
        fb[:, 3] = -fb[:, 3].abs() - 0.1
    return a.to(dtype).to(dev), b.to(dtype).to(dev), (torch.rand(C, generator=g) + 0.05).to(dev)


def tap_f64(a, b, w):
    """fp64 restatement on the same (already rounded) inputs: [n, 1, h, w, C] -> [n]."""
    A, B = F.relu(a.double())[:, 0].permute(0, 3, 1, 2), F.relu(b.double())[:, 0].permute(0, 3, 1, 2)
    return R.tap_distance(A, B, w.double())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h,w", [(1, 1), (5, 3), (20, 40)])
@pytest.mark.parametrize("C", [64, 512])
def test_tap_distance_pool_and_determinism(dev, C, h, w, n, dtype):
    from jointimagegeneration_amd import ops
    a, b, lw = tap_inputs(dev, n, h, w, C, dtype, seed=C + h)
    want = tap_f64(a, b, lw).cpu().numpy()
    total = torch.full((n,), 2.0, device=dev)
    got, pooled = ops.lpips_tap(a, b, lw, pool=True, total=total, accumulate=True)
    err = rel(got.cpu().numpy(), want)
    print(f"tap C={C} {h}x{w} n={n} {dtype}: max rel err vs fp64 {err:.3e}")
    assert err <= RTOL
    assert torch.equal(total, 2.0 + got)
    assert pooled.shape == (2 * n, 1, h // 2, w // 2, C)
    if h >= 2 and w >= 2:                                   # odd extents drop the last line / column, as MaxPool2d(2, 2) does
        for src, dst in ((a, pooled[:n]), (b, pooled[n:])):
            ref = F.max_pool2d(F.relu(src[:, 0].permute(0, 3, 1, 2).float()), 2).permute(0, 2, 3, 1).to(dtype)
            assert torch.equal(dst[:, 0], ref)
    again, pooled2 = ops.lpips_tap(a, b, lw, pool=True)
    assert torch.equal(again, got) and torch.equal(pooled2, pooled)          # equal bits: no floating-point atomics
    nopool, none = ops.lpips_tap(a, b, lw, pool=False)
    assert none is None and torch.equal(nopool, got)
    if n == 3:                                              # an image's value does not depend on the batch it is in
        alone, _ = ops.lpips_tap(a[1:2].contiguous(), b[1:2].contiguous(), lw, pool=False)
        assert torch.equal(alone, got[1:2])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_zero_rows_contribute_exactly_zero(dev, dtype):
    """Rows that are zero, or negative before the ReLU, in BOTH inputs: 0 / (0 + 1e-10) = 0, so the image scores exactly 0; one live
    pixel out of 15 then gives that pixel's term / 15."""
    from jointimagegeneration_amd import ops
    g = torch.Generator().manual_seed(9)
    a = -torch.rand(2, 1, 5, 3, 64, generator=g)
    b = -torch.rand(2, 1, 5, 3, 64, generator=g)
    a[0, 0, :, :, ::2] = 0.0
    lw = (torch.rand(64, generator=g) + 0.05).to(dev)
    a[1, 0, 4, 2] = torch.rand(64, generator=g)
    b[1, 0, 4, 2] = torch.rand(64, generator=g)
    a, b = a.to(dtype).to(dev), b.to(dtype).to(dev)
    got, pooled = ops.lpips_tap(a, b, lw)
    assert float(got[0]) == 0.0
    assert rel(got[1:].cpu().numpy(), tap_f64(a, b, lw)[1:].cpu().numpy()) <= RTOL and float(got[1]) > 0.0
    assert float(pooled.abs().max()) == 0.0                 # the live pixel sits in the dropped odd line and column


# ------------------------------------------------------------------------------------------------ end to end
def test_fp32_validation_reproduces_every_recorded_value(dev, gold, model, vols):
    from jointimagegeneration_amd import lpips, ops
    pred, gt = vols
    errs = {}
    with ops.fp32_validation():
        means = []
        for v in range(3):
            total, taps = model.score_view(pred[:, 0].contiguous(), gt[:, 0].contiguous(), v)
            errs[f"taps_view{v}"] = rel(taps.cpu().numpy(), gold[f"taps_view{v}"])
            errs[f"images_view{v}"] = rel(total.cpu().numpy(), gold[f"images_view{v}"])
            means.append(float(total.double().cpu().mean()))
        errs["view_means"] = rel(model.view_means(pred, gt), gold["view_means"])
        assert means == model.view_means(pred, gt)
        errs["score"] = rel(lpips.lpips_3view(pred, gt, model=model), gold["score"])
        errs["score_bps1"] = rel(lpips.lpips_3view(pred, gt, 1, model=model), gold["score_bps1"])
        errs["score_bps3"] = rel(lpips.lpips_3view(pred, gt, 3, model=model), gold["score_bps3"])
        out4 = model(torch.from_numpy(gold["x4"]).to(dev), torch.from_numpy(gold["y4"]).to(dev))
        assert out4.shape == (2, 1, 1, 1) and out4.dtype == torch.float32
        errs["out4"] = rel(out4.cpu().numpy(), gold["out4"])
        assert lpips.compute_metrics(pred, gt, ["lpips"], model=model) == {"lpips": lpips.lpips_3view(pred, gt, model=model)}
    print("fp32 validation, max rel err vs the reference:", json.dumps(errs))
    assert all(e <= RTOL for e in errs.values()), errs


def test_bf16_path_stays_within_the_measured_bound_and_keeps_the_view_order(dev, gold, model, vols):
    from jointimagegeneration_amd import lpips
    pred, gt = vols
    means = model.view_means(pred, gt)
    errs = {f"view_mean{v}": rel(means[v], gold["view_means"][v]) for v in range(3)}
    errs["score"] = rel(lpips.lpips_3view(pred, gt, model=model), gold["score"])
    errs["score_bps1"] = rel(lpips.lpips_3view(pred, gt, 1, model=model), gold["score_bps1"])
    errs["score_bps3"] = rel(lpips.lpips_3view(pred, gt, 3, model=model), gold["score_bps3"])
    out4 = model(torch.from_numpy(gold["x4"]).to(dev), torch.from_numpy(gold["y4"]).to(dev))
    errs["out4"] = rel(out4.cpu().numpy(), gold["out4"])
    print("bf16 path, |score - reference| / reference:", json.dumps(errs))
    assert list(np.argsort(means)) == list(np.argsort(gold["view_means"]))
    assert max(errs.values()) <= BF16_BOUND, errs            # twice the largest value of the table in DESIGN.md 7g


def test_chunks_of_three_images_give_the_same_bits(dev, model, vols):
    """Chunks only partition the images: 32, 40 and 80 images in chunks of 3 (a short last chunk each time) against one chunk."""
    from jointimagegeneration_amd import ops
    pred, gt = vols
    p, g = pred[:, 0].contiguous(), gt[:, 0].contiguous()
    with ops.fp32_validation():
        assert model.chunk_size(20, 40) >= 80               # the rule gives one chunk at this size
        one = [model.score_view(p, g, v) for v in range(3)]
        m1 = model.view_means(pred, gt)
        model.chunk_images = 3
        try:
            three = [model.score_view(p, g, v) for v in range(3)]
            m3 = model.view_means(pred, gt)
        finally:
            model.chunk_images = None
    for (t1, k1), (t3, k3) in zip(one, three):
        assert torch.equal(t1, t3) and torch.equal(k1, k3)
    assert m1 == m3


def test_the_chunk_rule_bounds_the_64_channel_activation():
    from jointimagegeneration_amd import lpips, ops
    m = lpips.LPIPS()
    assert m.chunk_size(512, 512) == 8 and 2 * 8 * 512 * 512 * 64 * 2 == lpips.CHUNK_BYTES       # a 512-image view runs in 64 chunks
    with ops.fp32_validation():
        assert m.chunk_size(512, 512) == 4
    assert m.chunk_size(4096, 4096) == 1


def test_two_calls_leave_no_memory_behind(dev, model, vols):
    from jointimagegeneration_amd import lpips
    pred, gt = vols
    model.prepare()                                         # the weight packs are the module's, not the call's
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    a = lpips.lpips_3view(pred, gt, model=model)
    b = lpips.lpips_3view(pred, gt, model=model)
    torch.cuda.synchronize()
    assert a == b and torch.cuda.memory_allocated() == before


def test_sample_diffusion_scores_its_samples(dev, gold, weight_files, vols, tmp_path, monkeypatch):
    """The sampler is stubbed with the fixture's volumes (sampling itself is covered elsewhere): main() writes metrics.json next to the
    samples with the three-view score of each, and nothing else changes."""
    from jointimagegeneration_amd import sample_diffusion as sd
    from jointimagegeneration_amd.io import write_nifti
    pred, gt = vols
    (tmp_path / "m.yaml").write_text("model:\n  target: none\n")
    gt_dir = tmp_path / "gt"
    gt_dir.mkdir()
    for i in range(2):
        write_nifti(str(gt_dir / f"sample_{i:04d}.nii.gz"), gold["gt"][i, 0])
    monkeypatch.setattr(sd, "load_model", lambda config, ckpt: (object(), 3))
    monkeypatch.setattr(sd, "synth_mask_volume", lambda d, h, w: torch.zeros(d, h, w, dtype=torch.long))
    monkeypatch.setattr(sd, "sample_cond", lambda model, instance, n_samples=1, **kw: torch.cat([pred, torch.zeros_like(pred)], 1))
    monkeypatch.chdir(tmp_path)
    common = ["--config", str(tmp_path / "m.yaml"), "-n", "2", "--slices", "16", "--size", "8"]
    sd.main(common + ["--gt", str(gt_dir), "--lpips-vgg", weight_files[0], "--lpips-lin", weight_files[1]])
    out = tmp_path / "samples" / "00000003"
    assert sorted(os.listdir(out)) == ["metrics.json", "sample_0000.nii.gz", "sample_0001.nii.gz"]
    doc = json.load(open(out / "metrics.json"))
    assert [v["name"] for v in doc["volumes"]] == ["sample_0000.nii.gz", "sample_0001.nii.gz"] and doc["volumes"][0]["shape"] == [16, 20, 40]
    # the mean over the two volumes, each scored alone, is compute_metrics with batch_per_segment = 1
    assert abs(doc["mean_lpips"] - float(gold["score_bps1"])) <= BF16_BOUND * float(gold["score_bps1"])
    from jointimagegeneration_amd import lpips
    again = lpips.main(["--pred", str(out), "--gt", str(gt_dir), "--vgg", weight_files[0], "--lin", weight_files[1], "--out", str(tmp_path / "again.json")])
    assert again == doc
