"""Records tests/golden/render.npz from the REFERENCE's combine_mask_and_im (latentdiffusion/sample_diffusion.py:23-58), on the CPU, with
scipy's sobel as the reference calls it.  Only data is written.

    python tests/golden/make_golden_render.py <path to the reference's latentdiffusion directory>

The reference module imports nibabel, omegaconf, torchvision, its own ldm / models packages and more at its top; none of that is used
by the function, so empty stubs stand in for whatever is missing.  torchvision's make_grid is among the missing: the uint8 grids in the
fixture are tiled by the plain loop below, written from make_grid's rule independently of tests/render_ref.py.

The generator asserts that the fixture holds what makes it worth having: voxels where the integer Sobel rule and the shortcut "some
neighbour along the axis differs, dilated over the other two axes" disagree, voxels that two classes claim (the lower must win), and
voxels with 0 < m < 1.  The counts are stored.
"""
import importlib.machinery
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def import_reference(ref_root):
    class _Any(types.ModuleType):
        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            return object

    missing = {}
    for name in ("nibabel", "omegaconf", "yaml", "PIL", "PIL.Image", "torchvision", "torchvision.utils", "ldm", "ldm.models",
                 "ldm.models.diffusion", "ldm.models.diffusion.ddim", "models", "models.util", "SimpleITK"):
        top = name.split(".")[0]
        if top not in missing:                            # decided once per package, before its stub lands in sys.modules
            missing[top] = top in ("ldm", "models") or importlib.util.find_spec(top) is None
        if missing[top]:
            m = _Any(name)
            m.__spec__ = importlib.machinery.ModuleSpec(name, None)
            m.__path__ = []
            sys.modules[name] = m
    spec = importlib.util.spec_from_file_location("reference_sample_diffusion", os.path.join(ref_root, "sample_diffusion.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    R.tqdm = lambda it=None, **k: it                      # no progress bars
    return R


def blocky_labels(g, shape, block, noise):
    """Labels 0..11 constant on blocks, with a fraction `noise` of the voxels redrawn."""
    D, H, W = shape
    coarse = torch.randint(0, 12, tuple(-(-n // b) for n, b in zip(shape, block)), generator=g)
    lab = coarse.repeat_interleave(block[0], 0).repeat_interleave(block[1], 1).repeat_interleave(block[2], 2)[:D, :H, :W].clone()
    flip = torch.rand(shape, generator=g) < noise
    lab[flip] = torch.randint(0, 12, (int(flip.sum()),), generator=g)
    return lab


def volumes():
    g = torch.Generator().manual_seed(20)
    v = {}

    def pair(lab_or_mask, is_label=True):
        ct = torch.rand(lab_or_mask.shape, generator=g) * 1.2 - 0.1            # some values outside [0, 1]: the clamp
        mask = lab_or_mask.float() / 11 if is_label else lab_or_mask
        return torch.stack([ct, mask]).contiguous()

    lab = blocky_labels(g, (12, 20, 24), (4, 5, 6), 0.05)
    lab[:, :, :3][lab[:, :, :3] > 6] = 0                                     # some background
    v["noisy"] = pair(lab)
    v["faces"] = pair(blocky_labels(g, (5, 6, 7), (3, 3, 4), 0.0).clamp(min=1))   # no background: organs on every face
    v["flat_d"] = pair(blocky_labels(g, (1, 6, 7), (1, 3, 3), 0.1))
    v["flat_h"] = pair(blocky_labels(g, (5, 1, 7), (2, 1, 3), 0.1))
    v["flat_w"] = pair(blocky_labels(g, (5, 6, 1), (2, 3, 1), 0.1))
    frac = blocky_labels(g, (4, 6, 8), (2, 3, 4), 0.1).float() / 11
    soft = torch.rand(frac.shape, generator=g) < 0.4
    frac[soft] = torch.rand(int(soft.sum()), generator=g) * (11.9 / 11)       # fractional m in [0, 11.9): a colour, but no class
    v["fractional"] = pair(frac, is_label=False)
    l255 = blocky_labels(g, (4, 5, 6), (2, 2, 3), 0.1).float() / 11
    l255[1:3, 1:4, 2:5] = 255 / 11                                            # rounded to fp32 by the assignment
    v["label255"] = pair(l255, is_label=False)
    return v


def tile(imgs, nrow, padding):
    """make_grid's rule as a plain loop; imgs fp32 [B, 3, H, W] -> uint8 [Hg, Wg, 3]."""
    B, C, H, W = imgs.shape
    if B == 1:
        return imgs[0].transpose(1, 2, 0).astype(np.uint8)
    xmaps = min(nrow, B)
    ymaps = (B + xmaps - 1) // xmaps
    canvas = np.zeros((3, ymaps * (H + padding) + padding, xmaps * (W + padding) + padding), dtype=np.float32)
    k = 0
    for yy in range(ymaps):
        for xx in range(xmaps):
            if k >= B:
                break
            top, left = yy * (H + padding) + padding, xx * (W + padding) + padding
            canvas[:, top:top + H, left:left + W] = imgs[k]
            k += 1
    return canvas.transpose(1, 2, 0).astype(np.uint8)


def census(x):
    """(voxels where the integer rule and the dilation shortcut disagree for some class, voxels claimed by two classes, 0 < m < 1)."""
    from scipy.ndimage import maximum_filter, sobel
    m = (x[1] * 11).numpy()
    m[m == 255] = 11
    disagree = np.zeros(m.shape, dtype=bool)
    claims = np.zeros(m.shape, dtype=np.int32)
    for i in range(1, 12):
        e = m == i
        exact = np.zeros(m.shape, dtype=bool)
        short = np.zeros(m.shape, dtype=bool)
        p = np.pad(e, 1)
        for axis in range(3):
            exact |= sobel(e, axis=axis, mode="constant")
            n = p.shape[axis]
            differs = np.take(p, range(2, n), axis) != np.take(p, range(0, n - 2), axis)
            size = [3, 3, 3]
            size[axis] = 1
            grown = maximum_filter(differs, size=size, mode="constant")
            inner = [slice(1, -1)] * 3
            inner[axis] = slice(None)
            short |= grown[tuple(inner)]
        disagree |= exact != short
        claims += exact
    return int(disagree.sum()), int((claims >= 2).sum()), int(((m > 0) & (m < 1)).sum())


def main(ref_root):
    R = import_reference(ref_root)
    out, totals = {}, np.zeros(3, dtype=np.int64)
    for name, x in volumes().items():
        for coef in ((0.2, 0.35) if name == "faces" else (0.2,)):
            y = R.combine_mask_and_im(x.clone(), overlay_coef=coef)
            assert y.dtype == torch.float32 and tuple(y.shape) == (x.shape[1], 3, x.shape[2], x.shape[3])
            key = name if coef == 0.2 else f"{name}_coef{coef}"
            out[f"out_{key}"] = y.numpy()
            if name in ("noisy", "faces", "flat_d") and coef == 0.2:       # 12, 5 and 1 slices: two rows, one row, the single image
                out[f"grid_{key}"] = tile(y.numpy(), 8, 5)
        out[f"x_{name}"] = x.numpy()
        c = census(x)
        print(name, tuple(x.shape), "rule != shortcut, two claims, 0 < m < 1:", c)
        totals += c
    m255 = out["x_label255"][1] * np.float32(11)
    assert (m255 == 255).sum() == 18, "255 / 11 must give exactly 255 after the fp32 multiply"
    assert (totals > 0).all(), totals
    assert census(torch.from_numpy(out["x_noisy"]))[0] > 0 and census(torch.from_numpy(out["x_noisy"]))[1] > 0
    out["count_rule_vs_shortcut"], out["count_two_claims"], out["count_fractional"] = (np.int64(t) for t in totals)
    out["coef_other"] = np.float64(0.35)
    path = os.path.join(HERE, "render.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; counts", totals)


if __name__ == "__main__":
    main(sys.argv[1])
