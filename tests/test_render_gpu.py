"""GPU suite of the volume rendering (csrc/gg_render.hip, jointimagegeneration_amd/render.py).

Everything is exact: gg_mask_overlay against tests/render_ref.py (which tests/test_render_cpu.py holds to the reference's recorded
output) with torch.equal on the fp32 tensor, gg_make_grid_u8 byte for byte.  There is no tolerance in this feature."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as R  # noqa: E402
from test_render_cpu import VOLUMES, decode_png  # noqa: E402

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTENTS = [(1, 1, 1), (1, 5, 7), (2, 3, 70), (9, 17, 33), (16, 64, 65)]          # none a multiple of the 8 x 8 x 64 tile


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "render.npz")))


def generated(shape, seed, noise=0.05):
    """(CT, label / 11) fp32 [2, D, H, W]: blocky labels 0..11 with label noise, a CT that leaves [0, 1] on both sides."""
    g = torch.Generator().manual_seed(seed)
    D, H, W = shape
    coarse = torch.randint(0, 12, (-(-D // 3), -(-H // 4), -(-W // 5)), generator=g)
    lab = coarse.repeat_interleave(3, 0).repeat_interleave(4, 1).repeat_interleave(5, 2)[:D, :H, :W].clone()
    flip = torch.rand(shape, generator=g) < noise
    lab[flip] = torch.randint(0, 12, (int(flip.sum()),), generator=g)
    ct = torch.rand(shape, generator=g) * 1.2 - 0.1
    return torch.stack([ct, lab.float() / 11]).contiguous()


_REF = {}


def reference(key, x, coef=0.2):
    """render_ref's overlay of x [2, D, H, W], computed once per key and never modified."""
    if key not in _REF:
        _REF[key] = R.combine_mask_and_im(x.clone(), overlay_coef=coef)
    return _REF[key]


def overlay(x, dev, coef=0.2, **kw):
    from jointimagegeneration_amd import ops
    return ops.mask_overlay(x.to(dev), R.COLORS, coef, **kw).cpu()


# ------------------------------------------------------------------------------------------------ gg_mask_overlay
@pytest.mark.parametrize("name", VOLUMES)
def test_overlay_equals_the_reference_on_the_fixture(dev, gold, name):
    x = torch.from_numpy(gold[f"x_{name}"])
    got = overlay(x[None], dev)[0]
    assert torch.equal(got, reference(name, x))
    assert np.array_equal(got.numpy(), gold[f"out_{name}"])                  # and so the recorded output itself


def test_overlay_at_another_coefficient(dev, gold):
    x, coef = torch.from_numpy(gold["x_faces"]), float(gold["coef_other"])
    got = overlay(x[None], dev, coef)[0]
    assert torch.equal(got, reference("faces_other", x, coef)) and np.array_equal(got.numpy(), gold[f"out_faces_coef{coef}"])


@pytest.mark.parametrize("shape", EXTENTS)
def test_overlay_on_extents_off_the_tile(dev, shape):
    x = generated(shape, seed=sum(shape))
    assert torch.equal(overlay(x[None], dev)[0], reference(shape, x))


def test_overlay_batch_and_poisoned_output(dev):
    """N = 2 with two different volumes (a batch mix-up changes bits), written into a NaN-filled buffer with guard bands on both sides:
    every output element is written, nothing beside the output is."""
    from jointimagegeneration_amd import ops
    shape = (9, 17, 33)
    xs = [generated(shape, seed=59), generated(shape, seed=60, noise=0.2)]
    want = torch.stack([reference(shape, xs[0]), reference((shape, "b"), xs[1])])
    assert not torch.equal(want[0], want[1])
    n, guard = want.numel(), 4096
    buf = torch.full((n + 2 * guard,), float("nan"), device=dev)
    out = buf[guard:guard + n].view(want.shape)
    got = ops.mask_overlay(torch.stack(xs).to(dev), R.COLORS, 0.2, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got.cpu(), want)
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all())
    with pytest.raises(ValueError, match="out must be"):
        ops.mask_overlay(torch.stack(xs).to(dev), R.COLORS, 0.2, out=out[:1])


def test_overlay_uniform_tiles_and_a_foreign_voxel_on_a_tile_edge(dev):
    """24 x 24 x 192 = 3 x 3 x 3 tiles: the middle tile's halo lies inside the volume, so in a uniform volume it holds one value and skips
    the stencil.  One foreign voxel on that tile's first corner, or one just outside it (inside its halo only), must switch the
    stencil back on for every tile that can see it."""
    shape = (24, 24, 192)
    ct = torch.rand(shape, generator=torch.Generator().manual_seed(8))
    for key, spots in (("uniform", ()), ("corner", ((8, 8, 64),)), ("halo", ((7, 8, 64), (16, 15, 128)))):
        lab = torch.full(shape, 3.0)
        for s in spots:
            lab[s] = 1.0                                                       # the lower class: its boundary wins around the voxel
        x = torch.stack([ct, lab / 11])
        want = reference((shape, key), x)
        assert torch.equal(overlay(x[None], dev)[0], want)
        painted = int(((want[:, 0] == 0) & (want[:, 1] == 80) & (want[:, 2] == 100)).sum())     # class 1's colour, found in no blend here
        assert (painted >= 26 * len(spots)) if spots else painted == 0


def test_overlay_on_a_side_stream(dev, gold):
    from jointimagegeneration_amd import ops
    x = torch.from_numpy(gold["x_noisy"])[None].to(dev)
    t = (torch.arange(2 * 3 * 5 * 7, dtype=torch.float32) * 1.37 % 256).reshape(2, 3, 5, 7).to(dev)
    want_grid = ops.make_grid_u8(t, nrow=8, padding=5).cpu()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = ops.mask_overlay(x, R.COLORS, 0.2)
        grid = ops.make_grid_u8(t, nrow=8, padding=5)
    s.synchronize()
    assert torch.equal(got.cpu()[0], reference("noisy", torch.from_numpy(gold["x_noisy"]))) and torch.equal(grid.cpu(), want_grid)


def test_combine_mask_and_im_shapes_and_range(dev, gold):
    from jointimagegeneration_amd import render
    x = torch.from_numpy(gold["x_fractional"])
    want = reference("fractional", x)
    assert torch.equal(render.combine_mask_and_im(x.to(dev)).cpu(), want)
    both = render.combine_mask_and_im(torch.stack([x, x.flip(1)]).to(dev)).cpu()
    assert torch.equal(both[0], want) and torch.equal(both[1], reference("fractional_flipped", x.flip(1).contiguous()))
    bad = x.clone()
    bad[1, 1, 2, 3] = 12 / 11
    with pytest.raises(ValueError, match=r"0\.\.11"):
        render.combine_mask_and_im(bad.to(dev))
    bad[1, 1, 2, 3] = -1.5 / 11
    with pytest.raises(ValueError, match=r"0\.\.11"):
        render.combine_mask_and_im(bad.to(dev))


# ------------------------------------------------------------------------------------------------ gg_make_grid_u8
def edge_values(B, C_, H, W):
    """Integers k and k - 2^-17 (fp32 holds the latter up to k = 128), and values in between."""
    n = B * C_ * H * W
    k = (torch.arange(n) * 7 % 255 + 1).float()
    kind = torch.arange(n) % 3
    frac = torch.rand(n, generator=torch.Generator().manual_seed(n))
    return torch.where(kind == 0, k, torch.where(kind == 1, k - 2.0 ** -17, (k - frac).clamp(min=0))).reshape(B, C_, H, W)


@pytest.mark.parametrize("padding", [0, 5])
@pytest.mark.parametrize("C_", [1, 3])
@pytest.mark.parametrize("B", [1, 2, 9])
def test_make_grid_u8_equals_the_reference(dev, B, C_, padding):
    from jointimagegeneration_amd import ops
    t = edge_values(B, C_, 5, 7)
    assert (t == t.floor()).any() and (t.floor() != (t + 2.0 ** -16).floor()).any()
    got = ops.make_grid_u8(t.to(dev), nrow=8, padding=padding).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, R.to_u8(R.make_grid(t, nrow=8, padding=padding)))
    got = ops.make_grid_u8(t.to(dev), nrow=2, padding=padding, pad_value=37.9).cpu().numpy()
    assert np.array_equal(got, R.to_u8(R.make_grid(t, nrow=2, padding=padding, pad_value=37.9)))


def test_make_grid_u8_wide_rows_poisoned_output_and_saturation(dev):
    from jointimagegeneration_amd import ops
    t = edge_values(3, 1, 3, 300)                                             # rows wider than one workgroup
    want = R.to_u8(R.make_grid(t, nrow=2, padding=3))
    n, guard = want.size, 1024
    buf = torch.full((n + 2 * guard,), 0xAB, dtype=torch.uint8, device=dev)
    out = buf[guard:guard + n].view(want.shape)
    ops.make_grid_u8(t.to(dev), nrow=2, padding=3, out=out)
    assert np.array_equal(out.cpu().numpy(), want)
    assert bool((buf[:guard] == 0xAB).all()) and bool((buf[guard + n:] == 0xAB).all())
    s = torch.tensor([-3.5, -0.25, 0.0, 0.999, 254.999, 255.0, 255.5, 300.0, 1e30, float("nan")]).reshape(1, 1, 2, 5)
    got = ops.make_grid_u8(s.to(dev)).cpu()
    assert got[..., 0].reshape(-1).tolist() == [0, 0, 0, 0, 254, 255, 255, 255, 255, 0]
    assert torch.equal(got[..., 0], got[..., 1]) and torch.equal(got[..., 0], got[..., 2])


# ------------------------------------------------------------------------------------------------ end to end
def test_volume_png_end_to_end(dev, gold, tmp_path):
    from jointimagegeneration_amd import render
    x = torch.from_numpy(gold["x_noisy"])
    assert render.volume_png(x.to(dev), str(tmp_path / "two.png")) == str(tmp_path / "two.png")
    img = decode_png((tmp_path / "two.png").read_bytes())
    assert np.array_equal(img, R.volume_image(x)) and np.array_equal(img, gold["grid_noisy"])
    grey = x[:1].clamp(0, 1)
    render.volume_png(grey.to(dev), str(tmp_path / "one.png"))
    assert np.array_equal(decode_png((tmp_path / "one.png").read_bytes()), R.volume_image(grey))
    assert render.volume_png(torch.zeros(1, 101, 2, 2, device=dev), str(tmp_path / "long.png")) is None
    assert not (tmp_path / "long.png").exists()
    assert render.volume_image(torch.zeros(2, 101, 2, 2, device=dev)).shape == (13 * 7 + 5, 8 * 7 + 5, 3)      # with a mask: always rendered


def test_render_cli_and_sample_diffusion_png(dev, tmp_path, monkeypatch):
    """`sample_diffusion --png` on the synthetic mask, the sampler stubbed with a random CT (sampling itself is covered elsewhere): the
    PNG's pixels are render_ref's for (CT, label / 11).  `python -m ...render` on the written volumes gives the same picture."""
    from jointimagegeneration_amd import render, sample_diffusion as sd
    from jointimagegeneration_amd.io import write_nifti
    from jointimagegeneration_amd.synth import synth_mask_volume
    (tmp_path / "m.yaml").write_text("model:\n  target: none\n")
    ct = torch.rand(6, 24, 24, generator=torch.Generator().manual_seed(9))
    monkeypatch.setattr(sd, "load_model", lambda config, ckpt: (object(), 3))
    monkeypatch.setattr(sd, "sample_cond", lambda model, instance, n_samples=1, **kw:
                        torch.stack([ct, instance["wholemask"][0, ..., 0]])[None].to(dev))
    monkeypatch.chdir(tmp_path)
    sd.main(["--config", str(tmp_path / "m.yaml"), "--slices", "6", "--size", "24", "--png"])
    out = tmp_path / "samples" / "00000003"
    assert sorted(os.listdir(out)) == ["sample_0000.nii.gz", "sample_0000.png"]
    lab = synth_mask_volume(6, 24, 24)
    assert lab.max() >= 5 and lab.min() == 0                                 # several organs and background
    want = R.volume_image(torch.stack([ct, lab.float() / 11]))
    assert np.array_equal(decode_png((out / "sample_0000.png").read_bytes()), want)
    write_nifti(str(tmp_path / "lab.nii.gz"), lab.numpy().astype(np.uint8))
    render.main(["--ct", str(out / "sample_0000.nii.gz"), "--mask", str(tmp_path / "lab.nii.gz"), "--out", str(tmp_path / "cli.png")])
    assert np.array_equal(decode_png((tmp_path / "cli.png").read_bytes()), want)
