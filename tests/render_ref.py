"""Host restatement of the reference's rendering (latentdiffusion/sample_diffusion.py:23-58, 241-261) in torch / numpy on the CPU, without
scipy or torchvision: what tests/golden/render.npz was recorded from, and what the device kernels are compared with bit for bit.

combine_mask_and_im: every arithmetic step is the reference's own fp32 torch operation in its own order.  The boundary rule is the exact
integer Sobel response of the bool volume `m == i` with zeros outside the volume ([-1, 0, 1] along one axis, [1, 2, 1] along the other
two): scipy.ndimage.sobel(mode='constant') on a bool array stores that response modulo 256 in a bool byte, so it is non-zero exactly
when the integer response is (|response| <= 16).  make_grid restates torchvision.utils.make_grid.
"""
import numpy as np
import torch

COLORS = ((0, 0, 0), (0, 80, 100), (119, 11, 32), (119, 11, 32), (250, 170, 30), (220, 220, 0), (107, 142, 35), (255, 0, 0),
          (70, 130, 180), (0, 0, 255), (0, 255, 255), (0, 255, 0))


def _along(a, axis, lo, hi):
    idx = [slice(None)] * a.ndim
    idx[axis] = slice(lo, hi)
    return a[tuple(idx)]


def sobel_nonzero(e: np.ndarray) -> np.ndarray:
    """e: bool [D, H, W].  True where one of the three integer Sobel responses of e (zero padding) is non-zero."""
    p = np.pad(e.astype(np.int32), 1)
    hit = np.zeros(e.shape, dtype=bool)
    for axis in range(3):
        r = p
        for ax in range(3):
            n = r.shape[ax]
            if ax == axis:
                r = _along(r, ax, 2, n) - _along(r, ax, 0, n - 2)
            else:
                r = _along(r, ax, 0, n - 2) + 2 * _along(r, ax, 1, n - 1) + _along(r, ax, 2, n)
        hit |= r != 0
    return hit


def boundaries(m: torch.Tensor) -> torch.Tensor:
    """m fp32 [D, H, W] (mask * 11 after the 255 rule) -> int64 [D, H, W]: the lowest class i in 1..11 of which the voxel is a boundary
    voxel, 0 where there is none."""
    b = np.zeros(tuple(m.shape), dtype=np.int64)
    mn = m.numpy()
    for i in range(1, 12):
        hit = sobel_nonzero(mn == i)
        b = np.where((b == 0) & hit, i, b)
    return torch.from_numpy(b)


def combine_mask_and_im(x: torch.Tensor, overlay_coef: float = 0.2) -> torch.Tensor:
    """x fp32 [2, D, H, W] on the CPU -> fp32 [D, 3, H, W]."""
    assert x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] == 2 and not x.is_cuda
    colors = torch.tensor(COLORS, dtype=torch.float32)
    image = (255 * x[0].clamp(0, 1))[..., None].repeat(1, 1, 1, 3)
    m = x[1] * 11
    m[m == 255] = 11
    pos, zero = (m > 0)[..., None].float(), (m == 0)[..., None].float()
    colored = colors[m.long()] * pos + image * zero
    im = colored * overlay_coef + image * (1 - overlay_coef)
    b = boundaries(m)
    on, off = (b > 0)[..., None].float(), (b == 0)[..., None].float()
    im = colors[b] * on + im * off
    return im.permute(0, 3, 1, 2).contiguous()


def grid_extent(B, H, W, nrow, padding):
    if B == 1:
        return H, W
    xmaps = min(nrow, B)
    ymaps = -(-B // xmaps)
    return ymaps * (H + padding) + padding, xmaps * (W + padding) + padding


def grid_offset(k, B, H, W, nrow, padding):
    """Top-left corner of image k in the grid."""
    if B == 1:
        return 0, 0
    xmaps = min(nrow, B)
    return k // xmaps * (H + padding) + padding, k % xmaps * (W + padding) + padding


def make_grid(t: torch.Tensor, nrow: int = 8, padding: int = 2, pad_value: float = 0.0) -> torch.Tensor:
    """t fp32 [B, C, H, W], C 1 or 3 -> fp32 [3, Hg, Wg] (torchvision.utils.make_grid without normalisation)."""
    assert t.dim() == 4 and t.shape[1] in (1, 3)
    if t.shape[1] == 1:
        t = torch.cat((t, t, t), 1)
    B, _, H, W = t.shape
    if B == 1:
        return t[0]
    Hg, Wg = grid_extent(B, H, W, nrow, padding)
    grid = t.new_full((3, Hg, Wg), pad_value)
    for k in range(B):
        y, x = grid_offset(k, B, H, W, nrow, padding)
        grid[:, y:y + H, x:x + W] = t[k]
    return grid


def to_u8(grid: torch.Tensor) -> np.ndarray:
    """The caller's `.permute(1, 2, 0).numpy().astype(np.uint8)`: truncation toward zero (values in [0, 256) only)."""
    return grid.permute(1, 2, 0).numpy().astype(np.uint8)


def volume_image(x: torch.Tensor) -> np.ndarray:
    """The picture of one sampled volume [c, D, H, W] (sample_diffusion.py:243-261): uint8 [Hg, Wg, 3]."""
    if x.shape[0] == 2:
        return to_u8(make_grid(combine_mask_and_im(x), nrow=8, padding=5))
    return to_u8(make_grid(255.0 * x.permute(1, 0, 2, 3), nrow=8, padding=5))
