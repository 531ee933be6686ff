"""Restatement of the patch-wise path's weighted fold for the split tests: the evaluation order gg_fold_weighted_cl is held to, written
as a plain fp32 loop over the crops in DESCENDING index, plus the torch.nn.Fold expression of the reference (ddpm.py:990-993) to pin it."""
import torch
import torch.nn.functional as F


def extent(H, W, kh, kw, sy, sx):
    return (H - kh) // sy + 1, (W - kw) // sx + 1


def weight_tables(kh, kw, Ly, Lx, tie, seed=0):
    """Random positive stand-ins for the border tables (the kernel takes any tables): W fp32 [kh, kw], T fp32 [L] or None."""
    g = torch.Generator().manual_seed(seed)
    W = torch.rand(kh, kw, generator=g) * 0.49 + 0.01
    T = (torch.rand(Ly * Lx, generator=g) * 0.49 + 0.01) if tie else None
    return W, T


def fold_descending(crops, W, T, N, H, Wd, kh, kw, sy, sx):
    """crops fp32 [L * N, kh, kw, C] (row l * N + n) -> fp32 [N, H, Wd, C]: num and den start from 0.0, crops are visited in descending
    l, each product rounded before it is added, w[l] = W * T[l] rounded first, one fp32 division at the end."""
    Ly, Lx = extent(H, Wd, kh, kw, sy, sx)
    C = crops.shape[-1]
    num = torch.zeros(N, H, Wd, C, dtype=torch.float32, device=crops.device)
    den = torch.zeros(H, Wd, dtype=torch.float32, device=crops.device)
    for l in range(Ly * Lx - 1, -1, -1):
        y0, x0 = (l // Lx) * sy, (l % Lx) * sx
        w = W if T is None else W * T[l]
        num[:, y0:y0 + kh, x0:x0 + kw] += crops[l * N:(l + 1) * N] * w[None, :, :, None]
        den[y0:y0 + kh, x0:x0 + kw] += w
    return num / den[None, :, :, None]


def fold_reference(crops, W, T, N, H, Wd, kh, kw, sy, sx):
    """The reference's expression on CPU: o [N, C, kh, kw, L] * weighting [1, 1, kh, kw, L] -> Fold -> / Fold(weighting)."""
    Ly, Lx = extent(H, Wd, kh, kw, sy, sx)
    L, C = Ly * Lx, crops.shape[-1]
    weighting = W.reshape(1, kh * kw, 1).repeat(1, 1, L)
    if T is not None:
        weighting = weighting * T.view(1, 1, L)
    normalization = F.fold(weighting, (H, Wd), (kh, kw), stride=(sy, sx)).view(1, 1, H, Wd)
    o = crops.view(L, N, kh, kw, C).permute(1, 4, 2, 3, 0)                      # [N, C, kh, kw, L]
    o = o * weighting.view(1, 1, kh, kw, L)
    out = F.fold(o.reshape(N, C * kh * kw, L), (H, Wd), (kh, kw), stride=(sy, sx)) / normalization
    return out.permute(0, 2, 3, 1).contiguous()


def unfold_reference(x_nchw, kh, kw, sy, sx):
    """torch.nn.Unfold crops of [N, C, H, W] as channels-last rows [L * N, kh, kw, C] (row l * N + n)."""
    N, C = x_nchw.shape[:2]
    u = F.unfold(x_nchw, (kh, kw), stride=(sy, sx))                            # [N, C * kh * kw, L]
    L = u.shape[-1]
    return u.view(N, C, kh, kw, L).permute(4, 0, 2, 3, 1).reshape(L * N, kh, kw, C).contiguous()
