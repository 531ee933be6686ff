"""Plain numpy reference for gg_surface.hip and metrics.surface_distances (test infrastructure; no scipy): class borders by shifted
comparisons, the squared Euclidean distance transform by brute force -- over all sites (edt_all_sites) and as three brute-force
min-plus passes (edt_separable, the only form that is affordable at 10^5 voxels; the CPU suite holds the two against each other on
the small cases) -- and medpy.metric.binary's hd / hd95 / asd / assd written out.  Every term is formed as (s * delta) * (s * delta)
and added W first, then H, then D, which is the order the header states.  Also the case builders shared by
tests/golden/make_golden_surface.py and the two test files."""
import hashlib

import numpy as np

SPACINGS = {"unit": (1.0, 1.0, 1.0), "dyadic": (2.5, 0.75, 0.75), "odd": (3.0, 0.7, 0.7)}
EXACT = ("unit", "dyadic")                     # every product and sum is exact in fp64: `==`
SCORES = ("hd", "hd95", "asd_pred_to_gt", "asd_gt_to_pred", "assd")
BIG = 20000                                    # voxels per case above which the fixture holds a SHA-256, not the array


def structure_offsets(connectivity):
    """The offsets of scipy's generate_binary_structure(3, connectivity) without the centre."""
    assert connectivity in (1, 2, 3)
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if 1 <= abs(dz) + abs(dy) + abs(dx) <= connectivity]


def borders(labels, K, connectivity=1):
    """labels [B, D, H, W] -> uint8 [B, M]: 1 where the label lies in [0, K) and a neighbour differs or lies outside the volume."""
    B, D, H, W = labels.shape
    lab = np.zeros((B, D + 2, H + 2, W + 2), dtype=labels.dtype)
    inside = np.zeros(lab.shape, dtype=bool)
    lab[:, 1:-1, 1:-1, 1:-1] = labels
    inside[:, 1:-1, 1:-1, 1:-1] = True
    edge = np.zeros(labels.shape, dtype=bool)
    for dz, dy, dx in structure_offsets(connectivity):
        sl = (slice(None), slice(1 + dz, 1 + dz + D), slice(1 + dy, 1 + dy + H), slice(1 + dx, 1 + dx + W))
        edge |= ~inside[sl] | (lab[sl] != labels)
    return (edge & (labels >= 0) & (labels < K)).astype(np.uint8).reshape(B, -1)


def site_mask(labels, border, cls):
    """bool [B, D, H, W]: the sites of gg_edt_squared (border None: every voxel of the class)."""
    m = labels == cls
    return m if border is None else m & (border.reshape(labels.shape) != 0)


def edt_all_sites(sites, spacing):
    """sites bool [D, H, W] -> float64 [D, H, W]: min over ALL sites of (sw dw)^2 + (sh dh)^2 + (sd dd)^2; +inf without a site."""
    sd, sh, sw = (np.float64(v) for v in spacing)
    D, H, W = sites.shape
    out = np.full(sites.size, np.inf)
    pts = np.argwhere(sites).astype(np.float64)
    if len(pts) == 0:
        return out.reshape(sites.shape)
    vox = np.argwhere(np.ones(sites.shape, dtype=bool)).astype(np.float64)
    step = max(1, (1 << 22) // len(pts))
    for i in range(0, len(vox), step):
        v = vox[i:i + step, None, :]
        dd, dh, dw = (sd * (v[..., 0] - pts[:, 0])), (sh * (v[..., 1] - pts[:, 1])), (sw * (v[..., 2] - pts[:, 2]))
        out[i:i + step] = ((dw * dw + dh * dh) + dd * dd).min(1)
    return out.reshape(sites.shape)


def _min_plus(g, axis, s):
    """out[.., l, ..] = min over l' of g[.., l', ..] + (s (l - l'))^2 along `axis`, by brute force."""
    g = np.ascontiguousarray(np.moveaxis(g, axis, -1))          # contiguous: the reshapes below are views
    L = g.shape[-1]
    k = np.float64(s) * (np.arange(L, dtype=np.float64)[:, None] - np.arange(L, dtype=np.float64)[None, :])
    cost = k * k                                                   # [l, l']
    out = np.empty_like(g)
    flat_in, flat_out = g.reshape(-1, L), out.reshape(-1, L)
    step = max(1, (1 << 22) // (L * L))
    for i in range(0, flat_in.shape[0], step):
        flat_out[i:i + step] = (flat_in[i:i + step, None, :] + cost[None]).min(-1)
    return np.moveaxis(out, -1, axis)


def edt_separable(sites, spacing):
    """The same minimum as three brute-force passes, W, H, D (exact: the minimum of a sum of per-axis terms separates)."""
    g = np.where(sites, 0.0, np.inf)
    for axis, s in ((2, spacing[2]), (1, spacing[1]), (0, spacing[0])):
        g = _min_plus(np.ascontiguousarray(g), axis, s)
    return g


def edt_squared(labels, border, cls, spacing, separable=True):
    """labels [B, D, H, W] -> float64 [B, M]; volumes never mix."""
    f = edt_separable if separable else edt_all_sites
    return np.stack([f(m, spacing) for m in site_mask(labels, border, cls)]).reshape(labels.shape[0], -1)


def reduce(labels_a, border_a, sq_b, cls):
    """(dist2 float64 [B, M], stats float64 [B, 3] = count, sum of sqrt, max; (0, 0, -1) for none)."""
    B = labels_a.shape[0]
    member = site_mask(labels_a, border_a, cls).reshape(B, -1)
    dist2 = np.where(member, sq_b.reshape(B, -1), -1.0)
    stats = np.array([[m.sum(), np.sqrt(d[m]).sum(), d[m].max() if m.any() else -1.0] for m, d in zip(member, dist2)], dtype=np.float64)
    return dist2, stats


def scores(pred, gt, K, spacing, connectivity=1):
    """{score: float64 [B, K]} by medpy's formulas, NaN for a class absent from either volume."""
    B = pred.shape[0]
    out = {name: np.full((B, K), np.nan) for name in SCORES}
    bp, bg = borders(pred, K, connectivity), borders(gt, K, connectivity)
    for c in range(K):
        to_gt = np.sqrt(edt_squared(gt, bg, c, spacing))
        to_pred = np.sqrt(edt_squared(pred, bp, c, spacing))
        mp, mg = site_mask(pred, bp, c).reshape(B, -1), site_mask(gt, bg, c).reshape(B, -1)
        for v in range(B):
            if not mp[v].any() or not mg[v].any():
                continue
            s_pg, s_gp = to_gt[v][mp[v]], to_pred[v][mg[v]]
            out["hd"][v, c] = max(s_pg.max(), s_gp.max())
            out["hd95"][v, c] = np.percentile(np.hstack((s_pg, s_gp)), 95)
            out["asd_pred_to_gt"][v, c] = s_pg.mean()
            out["asd_gt_to_pred"][v, c] = s_gp.mean()
            out["assd"][v, c] = np.mean((s_pg.mean(), s_gp.mean()))
    return out


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def held(a, big):
    """What the fixture holds of an array: the array, or its SHA-256 for a big case."""
    return sha(a) if big else a


# ------------------------------------------------------------------------------------------------------------------ cases
def _boxes(shape, lo, hi, inner=None):
    v = np.zeros(shape, dtype=np.int32)
    v[tuple(slice(a, b) for a, b in zip(lo, hi))] = 1
    if inner is not None:
        v[tuple(slice(a, b) for a, b in inner)] = 2
    return v


def _shift(v, by):
    """v displaced by `by` voxels, zeros moving in (no wrap)."""
    out = np.zeros_like(v)
    src = tuple(slice(max(0, -b), v.shape[i] - max(0, b)) for i, b in enumerate(by))
    dst = tuple(slice(max(0, b), v.shape[i] - max(0, -b)) for i, b in enumerate(by))
    out[dst] = v[src]
    return out


def random_blobs(shape, K, seed, noise=0.01):
    """Spherical blobs of classes 1..K-1 and `noise` of the voxels redrawn uniformly from [0, K)."""
    rng = np.random.default_rng(seed)
    z, y, x = np.indices(shape)
    v = np.zeros(shape, dtype=np.int32)
    for c in range(1, K):
        for _ in range(2):
            ctr = [rng.integers(0, n) for n in shape]
            r = rng.integers(5, 12)
            v[(z - ctr[0]) ** 2 + (y - ctr[1]) ** 2 + (x - ctr[2]) ** 2 <= r * r] = c
    flip = rng.random(shape) < noise
    return np.where(flip, rng.integers(0, K, size=shape), v).astype(np.int32)


def cases():
    """{name: dict(pred, gt int32 [B, D, H, W], K)}: the case list of the issue, smallest shapes at which the kernels can go wrong."""
    out = {}

    def add(name, pred, gt, K):
        pred, gt = (np.ascontiguousarray(v if v.ndim == 4 else v[None], dtype=np.int32) for v in (pred, gt))
        assert pred.shape == gt.shape
        out[name] = dict(pred=pred, gt=gt, K=K)
    nested = _boxes((5, 6, 7), (0, 1, 1), (4, 5, 6), inner=((1, 3), (2, 4), (2, 5)))
    add("odd_5x6x7", nested, _shift(nested, (1, 1, -1)), 3)                                # two nested boxes and a displaced copy
    flat = _boxes((1, 9, 11), (0, 2, 1), (1, 8, 9), inner=((0, 1), (4, 6), (3, 7)))
    add("slice_1x9x11", flat, _shift(flat, (0, -2, 2)), 3)                                 # an axis of extent 1
    full = np.ones((4, 5, 6), dtype=np.int32)
    dent = full.copy()
    dent[3, 3:, 4:] = 0
    add("full_volume_4x5x6", full, dent, 2)                                                # the border is the volume's shell
    near, far = np.zeros((3, 4, 300), np.int32), np.zeros((3, 4, 300), np.int32)
    near[0, 0, 0] = far[2, 3, 299] = 1
    add("far_corner_3x4x300", near, far, 2)                                                # the largest distance; a 300-long line
    z, y, x = np.indices((4, 5, 6))
    add("checkerboard_4x5x6", 1 + (z + y + x) % 2, 1 + (z + y + x + 1) % 2, 3)
    mid, pair = np.zeros((3, 3, 9), np.int32), np.zeros((3, 3, 9), np.int32)
    mid[1, 1, 4] = 1
    pair[1, 1, 2] = pair[1, 1, 6] = 1
    add("equidistant_3x3x9", mid, pair, 2)                                                 # two sites at equal distance on either side
    inner, ends = np.zeros((2, 3, 8), np.int32), np.zeros((2, 3, 8), np.int32)
    inner[:, 1, 3] = 1
    ends[0, 0, 0] = ends[1, 2, 7] = ends[0, 1, 7] = ends[1, 1, 0] = 1
    add("line_ends_2x3x8", inner, ends, 2)                                                 # a site at each end of a line
    add("empty_4x5x6", _boxes((4, 5, 6), (1, 1, 1), (3, 4, 5)), np.zeros((4, 5, 6), np.int32), 3)
    b3p = np.stack([nested, _shift(nested, (0, 0, 1)), _shift(nested, (1, 0, 0))])
    b3g = np.stack([_shift(nested, (0, 1, 0)), np.where(nested == 1, 0, nested), nested])  # the middle volume has no voxel of class 1
    add("batch3_5x6x7", b3p, b3g, 3)
    lab = _boxes((3, 4, 5), (0, 0, 0), (3, 4, 5))
    lab[1, 1, 2], lab[1, 2, 2], lab[0, 0, 0] = 7, -1, 3                                    # labels outside [0, 3): never sites
    add("border_by_label_3x4x5", lab, _boxes((3, 4, 5), (0, 0, 0), (3, 4, 4)), 3)
    blk = _boxes((7, 7, 7), (1, 1, 1), (6, 6, 6))
    blk[1, 1, 1] = blk[1, 1, 3] = 0                                                        # a missing corner and a missing edge voxel
    add("connectivity_7x7x7", blk, _boxes((7, 7, 7), (1, 1, 1), (6, 6, 6)), 2)
    add("long_line_2x3x600", _boxes((2, 3, 600), (0, 0, 5), (1, 2, 9)), _boxes((2, 3, 600), (1, 1, 590), (2, 3, 597)), 2)
    for name, shape, lo, hi, by in (("many_w_257x256x2", (257, 256, 2), (100, 80, 0), (160, 200, 2), (-30, 20, 0)),
                                    ("many_h_257x2x256", (257, 2, 256), (100, 0, 80), (160, 2, 200), (40, 0, -25)),
                                    ("many_d_2x257x256", (2, 257, 256), (0, 100, 80), (2, 160, 200), (0, -35, 30))):
        box = _boxes(shape, lo, hi)                                                        # more than 65535 lines along one axis
        add(name, box, _shift(box, by), 2)
    add("random_48x56x64", random_blobs((48, 56, 64), 5, 31), random_blobs((48, 56, 64), 5, 32), 5)
    return out


def is_big(case):
    return case["pred"][0].size > BIG
