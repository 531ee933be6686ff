"""CPU suite of the volume rendering (csrc/gg_render.hip, jointimagegeneration_amd/render.py): the host restatement tests/render_ref.py
against what the reference's combine_mask_and_im gave (tests/golden/render.npz, recorded by tests/golden/make_golden_render.py), bit for
bit; make_grid's shapes and offsets; io.write_png; every refusal, raised before any device call; the C declarations; sample_diffusion's
file list with and without --png."""
import ctypes as C
import os
import re
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOLUMES = ("noisy", "faces", "flat_d", "flat_h", "flat_w", "fractional", "label255")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "render.npz")))


# ------------------------------------------------------------------------------------------------ restatement == reference
def test_fixture_holds_the_cases_that_matter(gold):
    assert gold["count_rule_vs_shortcut"] > 0 and gold["count_two_claims"] > 0 and gold["count_fractional"] > 0
    assert {tuple(gold[f"x_{n}"].shape[1:]) for n in ("flat_d", "flat_h", "flat_w")} == {(1, 6, 7), (5, 1, 7), (5, 6, 1)}
    assert (gold["x_label255"][1] * np.float32(11) == 255).sum() == 18
    m = gold["x_fractional"][1] * np.float32(11)
    assert ((m > 0) & (m < 1)).any() and (m != np.trunc(m)).any()
    assert gold["x_faces"][1].min() > 0                                  # organs on every face
    assert gold["x_noisy"][0].min() < 0 and gold["x_noisy"][0].max() > 1  # the clamp works on something


@pytest.mark.parametrize("name", VOLUMES)
def test_restatement_equals_the_reference_bit_for_bit(gold, name):
    x = torch.from_numpy(gold[f"x_{name}"])
    got = R.combine_mask_and_im(x.clone())
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), gold[f"out_{name}"])
    if f"grid_{name}" in gold:
        img = R.volume_image(x)
        assert img.dtype == np.uint8 and np.array_equal(img, gold[f"grid_{name}"])


def test_restatement_equals_the_reference_at_another_coefficient(gold):
    coef = float(gold["coef_other"])
    assert coef != 0.2
    got = R.combine_mask_and_im(torch.from_numpy(gold["x_faces"]), overlay_coef=coef)
    assert np.array_equal(got.numpy(), gold[f"out_faces_coef{coef}"])
    assert not np.array_equal(got.numpy(), gold["out_faces"])


def test_boundary_rule_is_the_integer_response_not_a_neighbour_test():
    """sobel_nonzero against the 27-tap sum written out voxel by voxel, on a noisy volume; and a neighbourhood in which the class is
    present on both sides of every axis with equal smoothed weight, so that all three responses cancel although neighbours differ."""
    rng = np.random.default_rng(1)
    e = rng.random((4, 5, 6)) < 0.4
    e[:, :, 3:] = False                                   # an empty half: voxels with nothing in reach
    p = np.pad(e.astype(np.int64), 1)
    want = np.zeros(e.shape, dtype=bool)
    dv, sm = (-1, 0, 1), (1, 2, 1)
    for z in range(4):
        for y in range(5):
            for x in range(6):
                resp = [0, 0, 0]
                for a in range(3):
                    for b in range(3):
                        for c in range(3):
                            v = int(p[z + a, y + b, x + c])
                            resp[0] += dv[a] * sm[b] * sm[c] * v
                            resp[1] += sm[a] * dv[b] * sm[c] * v
                            resp[2] += sm[a] * sm[b] * dv[c] * v
                want[z, y, x] = any(resp)
    assert np.array_equal(R.sobel_nonzero(e), want) and want.any() and not want.all()
    sym = np.zeros((3, 3, 3), dtype=bool)
    sym[0, 0, 0] = sym[2, 2, 2] = sym[0, 2, 2] = sym[2, 0, 0] = sym[0, 0, 2] = sym[2, 2, 0] = sym[0, 2, 0] = sym[2, 0, 2] = True   # the eight corners
    assert not R.sobel_nonzero(sym)[1, 1, 1] and not sym[1, 1, 1]


# ------------------------------------------------------------------------------------------------ make_grid
@pytest.mark.parametrize("B", [1, 2, 8, 9, 17])
@pytest.mark.parametrize("C_", [1, 3])
def test_make_grid_shapes_and_offsets(B, C_):
    from jointimagegeneration_amd import ops
    H, W, pad = 3, 4, 5
    t = (torch.arange(B * C_ * H * W, dtype=torch.float32).reshape(B, C_, H, W) % 251) + 1          # never 0: the padding is 0
    g = R.make_grid(t, nrow=8, padding=pad)
    xmaps = min(8, B)
    ymaps = -(-B // xmaps)
    want = (H, W) if B == 1 else (ymaps * (H + pad) + pad, xmaps * (W + pad) + pad)
    assert tuple(g.shape) == (3,) + want == (3,) + R.grid_extent(B, H, W, 8, pad) == (3,) + ops.make_grid_extent(B, H, W, 8, pad)
    covered = torch.zeros(want, dtype=torch.bool)
    for k in range(B):
        y, x = R.grid_offset(k, B, H, W, 8, pad)
        assert (y, x) == ((0, 0) if B == 1 else (k // xmaps * (H + pad) + pad, k % xmaps * (W + pad) + pad))
        for c in range(3):
            assert torch.equal(g[c, y:y + H, x:x + W], t[k, c if C_ == 3 else 0])
        covered[y:y + H, x:x + W] = True
    assert (g[:, ~covered] == 0).all() and int(covered.sum()) == B * H * W
    assert R.make_grid(t, nrow=8, padding=pad, pad_value=7.0)[:, ~covered].eq(7).all()


def test_to_u8_truncates_toward_zero():
    k = torch.arange(1, 256, dtype=torch.float32)
    t = torch.stack([k - 2.0 ** -17, k]).reshape(2, 1, 1, 255)
    img = R.to_u8(R.make_grid(t, nrow=1, padding=0))
    # fp32 holds k - 2^-17 up to k = 128 (above, the difference is half an ulp and the subtraction gives k back)
    assert np.array_equal(img[0, :128, 0], np.arange(0, 128)) and np.array_equal(img[0, 128:, 1], np.arange(129, 256))
    assert np.array_equal(img[1, :, 2], np.arange(1, 256))


# ------------------------------------------------------------------------------------------------ write_png
def decode_png(raw: bytes) -> np.ndarray:
    """A minimal decoder: 8-bit RGB, no interlace, filter type 0 on every scanline; every chunk's CRC is checked."""
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(raw):
        n, tag = struct.unpack(">I4s", raw[at:at + 8])
        data = raw[at + 8:at + 8 + n]
        assert struct.unpack(">I", raw[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF, tag
        chunks.append((tag, data))
        at += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, flt, lace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(b"".join(d for t, d in chunks if t == b"IDAT")), dtype=np.uint8).reshape(H, 1 + 3 * W)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(H, W, 3)


def test_write_png_round_trip(tmp_path):
    from jointimagegeneration_amd.io import write_png
    img = np.random.default_rng(3).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    for name, a in (("a.png", img), ("b.png", img[:1, :1]), ("c.png", img[:, ::2])):        # c: a non-contiguous view
        write_png(str(tmp_path / name), a)
        assert np.array_equal(decode_png((tmp_path / name).read_bytes()), a)
    for bad in (img.astype(np.float32), img[..., 0], img[..., :2], np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError, match="write_png"):
            write_png(str(tmp_path / "bad.png"), bad)
    assert not (tmp_path / "bad.png").exists()
    src = open(os.path.join(ROOT, "jointimagegeneration_amd", "io.py")).read()
    assert not re.search(r"^\s*(import|from)\s+PIL", src, flags=re.M)


def test_write_png_is_read_by_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from jointimagegeneration_amd.io import write_png
    img = np.random.default_rng(4).integers(0, 256, (19, 23, 3), dtype=np.uint8)
    write_png(str(tmp_path / "a.png"), img)
    with Image.open(str(tmp_path / "a.png")) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), img)


# ------------------------------------------------------------------------------------------------ refusals
def test_organ_classes_are_the_reference_table():
    from jointimagegeneration_amd import render
    assert render.COLORS == R.COLORS and len(render.ORGAN_CLASSES) == 12
    assert [c.totalseg_id for c in render.ORGAN_CLASSES] == [0, 1, 2, 3, 5, 6, 10, 55, 56, 57, 104, 255]
    assert render.ORGAN_CLASSES[4].label_name == "liver" and render.ORGAN_CLASSES[11].color == (0, 255, 0)


def test_cpu_tensors_are_refused():
    from jointimagegeneration_amd import ops, render
    x = torch.zeros(2, 3, 4, 5)
    for call in (lambda: ops.mask_overlay(x[None], R.COLORS), lambda: ops.make_grid_u8(torch.zeros(2, 1, 4, 5)),
                 lambda: render.combine_mask_and_im(x), lambda: render.make_grid(torch.zeros(2, 3, 4, 5)),
                 lambda: render.volume_image(x), lambda: render.volume_image(x[:1]), lambda: render.volume_png(x, "never.png")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert not os.path.exists("never.png")


def test_bad_arguments_are_refused_before_any_device_call():
    from jointimagegeneration_amd import ops, render
    with pytest.raises(ValueError, match=r"\[N, 2, D, H, W\]"):
        ops.mask_overlay(torch.zeros(2, 3, 4, 5), R.COLORS)
    with pytest.raises(ValueError, match="fp32"):
        ops.mask_overlay(torch.zeros(1, 2, 3, 4, 5, dtype=torch.float64), R.COLORS)
    with pytest.raises(ValueError, match="contiguous"):
        ops.mask_overlay(torch.zeros(1, 2, 3, 4, 10)[..., ::2], R.COLORS)
    with pytest.raises(ValueError, match="12 rows of 3"):
        ops.mask_overlay(torch.zeros(1, 2, 3, 4, 5), R.COLORS[:11])
    with pytest.raises(ValueError, match="1 or 3"):
        ops.make_grid_u8(torch.zeros(2, 2, 4, 5))
    with pytest.raises(ValueError, match="1 or 3"):
        ops.make_grid_u8(torch.zeros(3, 4, 5))
    with pytest.raises(ValueError, match="nrow=0"):
        ops.make_grid_u8(torch.zeros(2, 1, 4, 5), nrow=0)
    with pytest.raises(ValueError, match="padding=-1"):
        ops.make_grid_u8(torch.zeros(2, 1, 4, 5), padding=-1)
    with pytest.raises(ValueError, match=r"\[2, D, H, W\]"):
        render.combine_mask_and_im(torch.zeros(3, 3, 4, 5))
    with pytest.raises(ValueError, match="1 or 2"):
        render.volume_image(torch.zeros(3, 3, 4, 5))
    for kw in ({"normalize": True}, {"value_range": (0, 1)}, {"scale_each": True}):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            render.make_grid(torch.zeros(2, 1, 4, 5), **kw)


def test_mask_range_is_refused_by_name(monkeypatch):
    """The range check reads the tensor, so it runs after the device check; that check and the kernel call are switched off here."""
    from jointimagegeneration_amd import ops, render
    monkeypatch.setattr(ops, "require_gpu", lambda t, what: None)
    monkeypatch.setattr(ops, "mask_overlay", lambda xb, colors, coef: torch.zeros(xb.shape[0], xb.shape[2], 3, xb.shape[3], xb.shape[4]))
    x = torch.zeros(2, 2, 3, 4)
    for bad in (12 / 11, -1 / 11, 254 / 11, float("nan")):
        x[1, 0, 0, 0] = bad
        with pytest.raises(ValueError, match=r"0\.\.11"):
            render.combine_mask_and_im(x)
    for fine in (255 / 11, 11.9 / 11, -0.5 / 11, 1.0):
        x[1, 0, 0, 0] = fine
        assert tuple(render.combine_mask_and_im(x).shape) == (2, 3, 3, 4)
    assert tuple(render.combine_mask_and_im(x[None].repeat(3, 1, 1, 1, 1)).shape) == (3, 2, 3, 3, 4)


# ------------------------------------------------------------------------------------------------ C-ABI
def test_entries_reject_bad_arguments_on_the_host():
    """No device here: every refusal comes from host code, before any launch."""
    from jointimagegeneration_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    colors = (C.c_int32 * 36)()
    shape = -1
    f = lib.gg_mask_overlay
    assert f(None, 1, 2, 2, 2, 0.2, colors, p, None) == shape and b"null" in lib.gg_last_error()
    assert f(p, 1, 2, 2, 2, 0.2, colors, None, None) == shape and f(p, 1, 2, 2, 2, 0.2, None, p, None) == shape
    for dims in ((0, 2, 2, 2), (1, 0, 2, 2), (1, 2, 0, 2), (1, 2, 2, -1)):
        assert f(p, *dims, 0.2, colors, p, None) == shape, dims
    g = lib.gg_make_grid_u8
    assert g(None, 2, 1, 2, 2, 8, 5, 0.0, p, None) == shape and g(p, 2, 1, 2, 2, 8, 5, 0.0, None, None) == shape
    assert g(p, 2, 2, 2, 2, 8, 5, 0.0, p, None) == shape and b"C=2" in lib.gg_last_error()
    for args in ((0, 1, 2, 2, 8, 5), (2, 1, 0, 2, 8, 5), (2, 1, 2, 0, 8, 5), (2, 1, 2, 2, 0, 5), (2, 1, 2, 2, 8, -1)):
        assert g(p, *args, 0.0, p, None) == shape, args


# ------------------------------------------------------------------------------------------------ sample_diffusion
def test_sample_diffusion_writes_the_pngs_only_with_the_option(tmp_path, monkeypatch):
    """The sampler, the model and the device rendering are stubbed (no device here); what is checked is main()'s own file list and what
    it hands to the renderer: (CT, label / 11), not the reference's (CT, label / 255)."""
    from jointimagegeneration_amd import sample_diffusion as sd
    from jointimagegeneration_amd.io import write_png
    (tmp_path / "m.yaml").write_text("model:\n  target: none\n")
    lab = torch.randint(0, 12, (4, 8, 8), generator=torch.Generator().manual_seed(5))
    ct = torch.rand(4, 8, 8, generator=torch.Generator().manual_seed(6))
    seen = []

    def fake_volume_png(x, path):
        seen.append(x.clone())
        write_png(path, R.volume_image(x))
        return path
    monkeypatch.setattr(sd, "load_model", lambda config, ckpt: (object(), 7))
    monkeypatch.setattr(sd, "synth_mask_volume", lambda d, h, w: lab)
    monkeypatch.setattr(sd, "sample_cond", lambda model, instance, n_samples=1, **kw:
                        torch.stack([ct, instance["wholemask"][0, ..., 0]])[None].repeat(n_samples, 1, 1, 1, 1))
    monkeypatch.setattr(sd, "volume_png", fake_volume_png)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.chdir(tmp_path)
    args = ["--config", str(tmp_path / "m.yaml"), "-n", "2", "--slices", "4", "--size", "8"]
    sd.main(args)
    out = tmp_path / "samples" / "00000007"
    assert sorted(os.listdir(out)) == ["sample_0000.nii.gz", "sample_0001.nii.gz"] and not seen
    sd.main(args + ["--png"])
    assert sorted(os.listdir(out)) == ["sample_0000.nii.gz", "sample_0000.png", "sample_0001.nii.gz", "sample_0001.png"]
    want = torch.stack([ct, lab.float() / 11])
    assert len(seen) == 2 and all(torch.equal(x, want) for x in seen)
    assert np.array_equal(decode_png((out / "sample_0001.png").read_bytes()), R.volume_image(want))
    assert (R.combine_mask_and_im(want) != R.combine_mask_and_im(torch.stack([ct, lab.float() / 255]))).any()     # the reference's call paints nothing
    assert "label / 11" in sd.get_parser().format_help().replace("\n", " ").replace("  ", " ")
