"""Plain numpy reference for gg_components.hip (test infrastructure): breadth-first component labelling for 6- and 26-connectivity in
canonical form (root = smallest linear index of the component within its volume), sizes, the per-class table with its tie rule, the
keep-largest / minimum-size filter, and the vote with the fp32 entropy recipe of include/guidegen_hip.h restated in numpy fp32 in the
same order.  Also the fixture volumes shared by tests/golden/make_golden_components.py and the two test files."""
import math
from collections import deque

import numpy as np


def offsets(connectivity):
    assert connectivity in (6, 26)
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                n = abs(dz) + abs(dy) + abs(dx)
                if n and (connectivity == 26 or n == 1):
                    out.append((dz, dy, dx))
    return out


def roots_one(vol, K, connectivity=6, background=0):
    """int32 [D*H*W]: the smallest linear index of the voxel's component, -1 for background / labels outside [0, K)."""
    D, H, W = vol.shape
    flat = vol.reshape(-1)
    root = np.full(flat.size, -1, dtype=np.int32)
    offs = offsets(connectivity)
    for start in range(flat.size):                   # ascending: the first voxel met of a component is its smallest index
        c = int(flat[start])
        if root[start] >= 0 or c < 0 or c >= K or c == background:
            continue
        root[start] = start
        queue = deque([start])
        while queue:
            i = queue.popleft()
            z, r = divmod(i, H * W)
            y, x = divmod(r, W)
            for dz, dy, dx in offs:
                zz, yy, xx = z + dz, y + dy, x + dx
                if 0 <= zz < D and 0 <= yy < H and 0 <= xx < W:      # rows never wrap
                    j = (zz * H + yy) * W + xx
                    if root[j] < 0 and flat[j] == c:
                        root[j] = start
                        queue.append(j)
    return root


def roots(labels, K, connectivity=6, background=0):
    """labels [B, D, H, W] -> int32 [B, M]; volumes never join."""
    return np.stack([roots_one(v, K, connectivity, background) for v in labels])


def sizes_and_stats(labels, root, K):
    """size int32 [B, M] (count at the root position, 0 elsewhere); stats int64 [B, K, 4] = (components, voxels, largest, root of the
    largest or -1); equal sizes tie to the smaller root."""
    B = labels.shape[0]
    flat = labels.reshape(B, -1)
    size = np.zeros(root.shape, dtype=np.int32)
    stats = np.zeros((B, K, 4), dtype=np.int64)
    stats[:, :, 3] = -1
    for b in range(B):
        r = root[b]
        np.add.at(size[b], r[r >= 0], 1)
        for i in np.nonzero(r == np.arange(r.size))[0]:        # ascending roots: a strict > keeps the smaller root on a tie
            c, s = int(flat[b, i]), int(size[b, i])
            stats[b, c, 0] += 1
            stats[b, c, 1] += s
            if s > stats[b, c, 2]:
                stats[b, c, 2], stats[b, c, 3] = s, i
    return size, stats


def filter_labels(labels, root, size, stats, K, keep_largest, min_size, background=0, fill=None):
    """(cleaned labels, kept uint8), shaped as labels."""
    fill = background if fill is None else fill
    B = labels.shape[0]
    flat = labels.reshape(B, -1)
    out = np.empty_like(flat)
    kept = np.zeros(flat.shape, dtype=np.uint8)
    for b in range(B):
        for i, c in enumerate(flat[b].tolist()):
            if c == background:
                keep = True
            elif c < 0 or c >= K:
                keep = False
            else:
                r = int(root[b, i])
                keep = (keep_largest[c] == 0 or r == stats[b, c, 3]) and size[b, r] >= min_size[c]
            out[b, i] = c if keep else fill
            kept[b, i] = 1 if keep else 0
    return out.reshape(labels.shape), kept.reshape(labels.shape)


def vote_operands(S):
    """The host's three fp32 operands, formed in fp64 and rounded once."""
    table = np.array([0.0] + [c * math.log(c) for c in range(1, S + 1)], dtype=np.float64).astype(np.float32)
    return table, np.float32(math.log(S)), np.float32(1.0 / S)


def vote(labels, K):
    """labels [S, M] -> winner int32 [M], agreement int32 [M], entropy fp32 [M], skipped (int)."""
    S, M = labels.shape
    table, ln_s, inv_s = vote_operands(S)
    ok = (labels >= 0) & (labels < K)
    counts = np.zeros((M, K), dtype=np.int64)
    for s in range(S):
        m = np.nonzero(ok[s])[0]
        np.add.at(counts, (m, labels[s, m]), 1)
    winner = counts.argmax(1).astype(np.int32)                 # first maximum = smallest label among the most voted
    agreement = counts.max(1).astype(np.int32)
    acc = np.zeros(M, dtype=np.float32)
    for k in range(K):                                         # ascending k, every add rounded to fp32
        acc = (acc + table[counts[:, k]]).astype(np.float32)
    entropy = (ln_s - (acc * inv_s).astype(np.float32)).astype(np.float32)
    entropy[agreement == 0] = np.float32(0.0)
    return winner, agreement, entropy, int((~ok).sum())


# ------------------------------------------------------------------------------------------------------------------ fixtures
def serpentine(D, H, W, c=1):
    """A one-voxel-wide path through the whole volume: every second row in y, joined at alternating ends, every second slice in z,
    joined at alternating corners.  One component whose root (voxel 0) is far from its end."""
    v = np.zeros((D, H, W), dtype=np.int32)
    flip_z = False
    for z in range(0, D, 2):
        ys = list(range(0, H, 2))
        right = False
        for n, y in enumerate(ys):
            v[z, y, :] = c
            if n + 1 < len(ys):
                v[z, y + 1, W - 1 if not right else 0] = c
                right = not right
        end_y = ys[-1]
        end_x = (W - 1) if (len(ys) % 2 == 1) else 0         # where the last row of this slice ends
        if z + 2 < D:
            # this slice is traversed from (y=0, x=0) to (end_y, end_x) or back; join to the next slice at alternating ends
            if not flip_z:
                v[z + 1, end_y, end_x] = c
            else:
                v[z + 1, 0, 0] = c
            flip_z = not flip_z
    return v


def comb(D, H, W, c=2):
    """Teeth along x that meet only in the last row: arms whose provisional roots differ until the far end joins them."""
    v = np.zeros((D, H, W), dtype=np.int32)
    v[:, :, ::2] = c
    v[:, :H - 1, 1::2] = 0
    v[:, H - 1, :] = c
    v[1::2] = 0
    return v


def u_shapes(D, H, W):
    v = np.zeros((D, H, W), dtype=np.int32)
    v[0, :, 0] = 1
    v[0, :, W - 1] = 1
    v[0, H - 1, :] = 1                                         # a U open at y = 0
    if D > 2:
        v[2, 0, :] = 2
        v[2, :, 0] = 2
        v[2, :, W - 1] = 2                                     # a U open at y = H - 1: the arms meet at the START
        v[D - 1, :, W // 2] = 1                                # a second component of class 1
    return v


def checkerboard(D, H, W):
    z, y, x = np.indices((D, H, W))
    return (1 + (z + y + x) % 2).astype(np.int32)              # classes 1 and 2, no background


def corner_and_edge():
    v = np.zeros((4, 4, 6), dtype=np.int32)
    v[0, 0, 0] = v[1, 1, 1] = 1                                # touch at a corner only
    v[3, 0, 3] = v[3, 1, 4] = 2                                # touch at an edge only
    return v


def wrap_traps():
    """Equal labels at the end of one row / slice and the start of the next: adjacent in memory, not in space."""
    v = np.zeros((3, 4, 5), dtype=np.int32)
    v[0, 0, 4] = v[0, 1, 0] = 1                                # x = W-1 | x = 0 of the next row
    v[0, 3, 2] = v[1, 0, 2] = 2                                # y = H-1 | y = 0 of the next slice
    v[1, 3, 4] = v[2, 0, 0] = 3                                # last voxel of a slice | first of the next
    v[2, 3, 4] = 4
    return v


def random_labels(shape, K, seed, density=0.32):
    rng = np.random.default_rng(seed)
    fg = rng.random(shape) < density
    return np.where(fg, rng.integers(1, K, size=shape), 0).astype(np.int32)


def tie_volume():
    """Two equal largest components of class 1 (4 voxels each; the smaller root wins) and a smaller third; class 2 has sizes 3, 2, 1."""
    v = np.zeros((5, 6, 7), dtype=np.int32)
    v[0, 0, 0:4] = 1
    v[4, 5, 3:7] = 1
    v[2, 2, 2:4] = 1
    v[1, 3, 0:3] = 2
    v[3, 0, 5:7] = 2
    v[4, 0, 0] = 2
    return v


def fixture_cases():
    """{name: (labels int32 [B, D, H, W], K)}: the small volumes of the golden file and of both test files."""
    cases = {}
    for shape in ((1, 1, 1), (1, 1, 70), (5, 6, 7), (3, 4, 130), (33, 17, 9), (16, 16, 16)):
        tag = "x".join(map(str, shape))
        cases[f"background_{tag}"] = (np.zeros((1,) + shape, np.int32), 2)
        cases[f"one_class_{tag}"] = (np.ones((1,) + shape, np.int32), 2)
        cases[f"random_k2_{tag}"] = (random_labels((1,) + shape, 2, 11), 2)
        cases[f"random_k14_{tag}"] = (random_labels((1,) + shape, 14, 12), 14)
        cases[f"checkerboard_{tag}"] = (checkerboard(*shape)[None], 3)
    cases["serpentine_33x17x9"] = (serpentine(33, 17, 9)[None], 2)
    cases["comb_5x6x7"] = (comb(5, 6, 7)[None], 3)
    cases["comb_3x4x130"] = (comb(3, 4, 130)[None], 3)
    cases["u_shapes_5x6x7"] = (u_shapes(5, 6, 7)[None], 3)
    cases["u_shapes_16x16x16"] = (u_shapes(16, 16, 16)[None], 3)
    cases["corner_and_edge"] = (corner_and_edge()[None], 3)
    cases["wrap_traps"] = (wrap_traps()[None], 5)
    cases["tie"] = (tie_volume()[None], 3)
    # B = 3: the last voxel of one volume and the first of the next carry the same class
    b3 = random_labels((3, 5, 6, 7), 4, 13)
    b3[0, -1, -1, -1] = b3[1, 0, 0, 0] = 2
    b3[1, -1, -1, -1] = b3[2, 0, 0, 0] = 3
    cases["batch3_5x6x7"] = (b3, 4)
    b3b = np.stack([serpentine(16, 16, 16), random_labels((16, 16, 16), 14, 14), np.ones((16, 16, 16), np.int32)])
    b3b[0, -1, -1, -1] = b3b[1, 0, 0, 0] = 1
    cases["batch3_16x16x16"] = (b3b, 14)
    oob = random_labels((1, 5, 6, 7), 4, 15)
    oob[0, 0, 0, 0], oob[0, 0, 0, 1], oob[0, 2, 3, 4], oob[0, 4, 5, 6] = -1, 4, 255, -2 ** 31
    cases["out_of_range"] = (oob, 4)
    return cases
