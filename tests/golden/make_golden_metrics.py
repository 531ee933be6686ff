"""Generates tests/golden/metrics.npz from the REFERENCE's ensemble scores (ccdm/ddpm/utils.py:190-236:
calc_batched_generalised_energy_distance and batched_hungarian_matching), imported from the reference tree with a stub for torchvision
(not installed; utils.py only draws with it) and with `np.bool = bool` set before the call (utils.py:212 uses the alias numpy dropped).

Run only in the build container (needs the reference tree, like make_golden.py):
    python tests/golden/make_golden_metrics.py [OUT_DIR]
The fixture holds data only: small label arrays and the numbers the two functions return for them.
  k4:  K = 4,  B = 2 cases, S0 = 3 samples against S1 = 4, spatial 4 x 6 x 5; in case 1 sample 0 of set 0 EQUALS sample 2 of set 1
  k14: K = 14 with classes 3, 7, 8, 11 and 13 absent from every sample (the 0 / 0 -> 1 branch of `iou`), same extents
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402

B, S0, S1, SP = 2, 3, 4, (4, 6, 5)


def import_utils():
    if "torchvision" not in sys.modules:
        tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
        tr.ToPILImage = object
        tv.transforms = tr
        sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr
    spec = importlib.util.spec_from_file_location("ccdm_ddpm_utils", os.path.join(MG.REF, "ccdm", "ddpm", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def labels(rng, K, present):
    """Blocky label volumes (runs of one class, so that the IoUs are not all near zero) over the classes in `present`."""
    present = np.asarray(present)

    def one(S):
        coarse = present[rng.integers(0, len(present), size=(B, S, 2, 3, 5))]
        vol = np.repeat(np.repeat(coarse, 2, axis=2), 2, axis=3)
        noise = rng.random(vol.shape) < 0.15
        return np.where(noise, present[rng.integers(0, len(present), size=vol.shape)], vol).astype(np.int64)

    a, b = one(S0), one(S1)
    assert a.shape == (B, S0) + SP and b.shape == (B, S1) + SP and a.max() < K
    return a, b


def main(out_dir):
    U = import_utils()
    if not hasattr(np, "bool"):
        np.bool = bool
    rng = np.random.default_rng(20240607)
    out = {}
    for name, K, present in (("k4", 4, range(4)), ("k14", 14, [0, 1, 2, 4, 5, 6, 9, 10, 12])):
        a, b = labels(rng, K, present)
        if name == "k4":
            a[1, 0] = b[1, 2]                                       # one sample equals a ground truth
        with np.errstate(invalid="ignore", divide="ignore"):        # 0 / 0 is the reference's own route to "absent from both"
            ged, d0, d1 = U.calc_batched_generalised_energy_distance(a, b, K)
            hm = np.asarray(U.batched_hungarian_matching(a, b, K), dtype=np.float64)
        assert ged.shape == (B,) and hm.shape == (B,) and np.isfinite(ged).all() and np.isfinite(hm).all()
        if name == "k14":
            absent = sorted(set(range(K)) - set(np.unique(a)) - set(np.unique(b)))
            assert len(absent) >= 3, absent
        out.update({f"{name}_K": np.int64(K), f"{name}_a": a.astype(np.int32), f"{name}_b": b.astype(np.int32),
                    f"{name}_ged": ged.astype(np.float64), f"{name}_div0": d0.astype(np.float64), f"{name}_div1": d1.astype(np.float64),
                    f"{name}_hm": hm})
        print(name, "ged", ged, "div0", d0, "div1", d1, "hm", hm)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "metrics.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else MG.OUT)
