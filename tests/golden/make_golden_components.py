"""Writes tests/golden/components.npz: the fixture volumes of tests/components_ref.py labelled with scipy.ndimage.label, per class, with
generate_binary_structure(3, 1) (6-connectivity) and (3, 3) (26-connectivity), in the canonical form of gg_label_components (root =
smallest linear index of the component within its volume, -1 for background and labels outside [0, K)).  The 64^3 random volume is
stored as its per-class table and the SHA-256 of its roots.  Needs scipy (1.15.3 when the file was written); the tests do not.

    python tests/golden/make_golden_components.py
"""
import hashlib
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import components_ref as R  # noqa: E402


def scipy_roots(labels, K, connectivity, background=0):
    structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    out = np.full((labels.shape[0], labels[0].size), -1, dtype=np.int32)
    for b, vol in enumerate(labels):
        for c in range(K):
            if c == background:
                continue
            lab, n = ndimage.label(vol == c, structure=structure)
            if n == 0:
                continue
            flat = lab.reshape(-1)
            idx = np.nonzero(flat)[0]
            first = np.full(n + 1, flat.size, dtype=np.int64)
            np.minimum.at(first, flat[idx], idx)
            out[b, idx] = first[flat[idx]]
    return out


def table(labels, root, K):
    return R.sizes_and_stats(labels, root, K)[1]


def main():
    doc = {}
    for name, (labels, K) in R.fixture_cases().items():
        for conn in (6, 26):
            doc[f"{name}__root{conn}"] = scipy_roots(labels, K, conn)
    serp = doc["serpentine_33x17x9__root6"]
    assert (serp[serp >= 0] == 0).all() and (serp >= 0).sum() > 33 * 17 * 9 // 5, "the serpentine is one 6-connected component"
    big = R.random_labels((1, 64, 64, 64), 2, 64)
    for conn in (6, 26):
        root = scipy_roots(big, 2, conn)
        st = table(big, root, 2)
        doc[f"random64__stats{conn}"] = st
        doc[f"random64__sha{conn}"] = np.frombuffer(hashlib.sha256(root.tobytes()).digest(), dtype=np.uint8)
        print(f"random 64^3, density 0.32, K = 2, connectivity {conn}: {int(st[0, 1, 0])} components, largest {int(st[0, 1, 2])} voxels")
    np.savez_compressed(os.path.join(HERE, "components.npz"), **doc)
    print(f"wrote {os.path.join(HERE, 'components.npz')}: {len(doc)} arrays")


if __name__ == "__main__":
    main()
