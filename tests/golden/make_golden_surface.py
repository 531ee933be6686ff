"""Writes tests/golden/surface.npz: the cases of tests/surface_ref.py scored with scipy.ndimage -- generate_binary_structure,
binary_erosion and distance_transform_edt -- and medpy.metric.binary's formulas written out (medpy itself is not needed):

    border  = m ^ binary_erosion(m, structure=generate_binary_structure(3, connectivity), iterations=1),  m = labels == c
    sds(a, b) = distance_transform_edt(~border_b, sampling=spacing)[border_a]
    hd = max(sds(a, b).max(), sds(b, a).max());  hd95 = np.percentile(np.hstack((sds(a, b), sds(b, a))), 95)
    asd(a, b) = sds(a, b).mean();  assd = np.mean((asd(a, b), asd(b, a)))

The squared distances are formed from the nearest-site indices scipy returns, as (sw dw)^2 + (sh dh)^2 + (sd dd)^2 in that order, so
that they are exact integers (or exact dyadic values) where the spacing allows.  Arrays of the cases above surface_ref.BIG voxels are
held as SHA-256 (of the int64 squared distances at unit spacing).  Needs scipy (1.15.3 when the file was written); the tests do not.

    python tests/golden/make_golden_surface.py
"""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import surface_ref as R  # noqa: E402


def class_border(labels, c, connectivity):
    m = labels == c
    return m ^ ndimage.binary_erosion(m, structure=ndimage.generate_binary_structure(3, connectivity), iterations=1)


def scipy_borders(labels, K, connectivity):
    out = np.zeros(labels.shape, dtype=bool)
    for b, vol in enumerate(labels):
        for c in range(K):
            out[b] |= class_border(vol, c, connectivity)
    return out.astype(np.uint8).reshape(labels.shape[0], -1)


def scipy_sq(sites, spacing):
    """sites bool [B, D, H, W] -> float64 [B, M] squared distances to the nearest site scipy finds; +inf in a volume without sites."""
    sd, sh, sw = (np.float64(v) for v in spacing)
    out = np.full(sites.shape, np.inf)
    for b, s in enumerate(sites):
        if not s.any():
            continue
        idx = ndimage.distance_transform_edt(~s, sampling=spacing, return_distances=False, return_indices=True)
        z, y, x = np.indices(s.shape)
        dd, dh, dw = sd * (z - idx[0]).astype(np.float64), sh * (y - idx[1]).astype(np.float64), sw * (x - idx[2]).astype(np.float64)
        out[b] = (dw * dw + dh * dh) + dd * dd
    return out.reshape(sites.shape[0], -1)


def sds(a, b, c, spacing, connectivity):
    """medpy's __surface_distances for the masks a == c, b == c of one volume."""
    a_border, b_border = class_border(a, c, connectivity), class_border(b, c, connectivity)
    return ndimage.distance_transform_edt(~b_border, sampling=spacing)[a_border]


def scipy_scores(pred, gt, K, spacing, connectivity):
    out = {name: np.full((pred.shape[0], K), np.nan) for name in R.SCORES}
    for v in range(pred.shape[0]):
        for c in range(K):
            if not (pred[v] == c).any() or not (gt[v] == c).any():          # medpy raises: "does not contain any binary object"
                continue
            s_pg, s_gp = sds(pred[v], gt[v], c, spacing, connectivity), sds(gt[v], pred[v], c, spacing, connectivity)
            out["hd"][v, c] = max(s_pg.max(), s_gp.max())
            out["hd95"][v, c] = np.percentile(np.hstack((s_pg, s_gp)), 95)
            out["asd_pred_to_gt"][v, c] = s_pg.mean()
            out["asd_gt_to_pred"][v, c] = s_gp.mean()
            out["assd"][v, c] = np.mean((s_pg.mean(), s_gp.mean()))
    return out


def main():
    doc = {}
    for name, case in R.cases().items():
        big = R.is_big(case)
        K = case["K"]
        bord = {}
        for conn in (1, 2, 3):
            for side in ("pred", "gt"):
                bord[conn, side] = scipy_borders(case[side], K, conn)
                doc[f"{name}__border{conn}_{side}"] = R.held(bord[conn, side], big)
        for tag, spacing in R.SPACINGS.items():
            for c in ([1] if big else range(K)):
                for side in ("pred", "gt"):
                    sq = scipy_sq(R.site_mask(case[side], bord[1, side], c), spacing)
                    if big and tag == "unit":
                        assert np.isfinite(sq).all() and (sq == np.rint(sq)).all()
                        sq = sq.astype(np.int64)
                    doc[f"{name}__sq_{tag}_c{c}_{side}"] = R.held(sq, big)
            for conn in ((1, 2, 3) if tag == "unit" else (1,)):
                for score, arr in scipy_scores(case["pred"], case["gt"], K, spacing, conn).items():
                    doc[f"{name}__{score}_{tag}_conn{conn}"] = arr
        if not big:
            doc[f"{name}__sqfull_unit_c1_gt"] = scipy_sq(case["gt"] == 1, R.SPACINGS["unit"])
    np.savez_compressed(os.path.join(HERE, "surface.npz"), **doc)
    size = os.path.getsize(os.path.join(HERE, "surface.npz"))
    print(f"wrote {os.path.join(HERE, 'surface.npz')}: {len(doc)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
