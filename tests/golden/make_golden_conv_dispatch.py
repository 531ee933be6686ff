"""Generates tests/golden/conv_dispatch.json: what the host-side conv dispatch predicates of libguidegen_hip.so answer for a sweep of
descriptors.  The predicates read no pointers and launch nothing (dry runs return before any HIP call), so this needs no GPU.

Run it on a library built from the commit whose dispatch is to be pinned (the PARENT of a refactor, never the code under test):
    python tests/golden/make_golden_conv_dispatch.py PATH/TO/libguidegen_hip.so [OUT_DIR]

The sweep is the full product of the axes below, thinned to every STRIDE-th case (STRIDE is prime to every axis length, so every value
of every axis, and every pair of values of the faster axes, stays in), plus every head conv unthinned (64 channels to 4 or 14 fp32 couts,
3-tap kernels, stride 1): the fused DDIM and CCDM epilogues exist only there, and the thinned product alone would meet them a few times.
Every descriptor field that is set is written out, so the test rebuilds each descriptor from the fixture alone.
"""
from __future__ import annotations

import ctypes as C
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from jointimagegeneration_amd import _lib  # noqa: E402
from jointimagegeneration_amd.ops import conv_out_extent, pad32  # noqa: E402

BATCH = (1, 2, 8)
EXTENT = [(1, s, s) for s in (4, 8, 16, 32, 64, 128, 256, 512)] + [(s, s, s) for s in (8, 16, 32, 64, 128)]
CHANNELS = ((32, 0), (64, 0), (128, 0), (160, 0), (320, 320), (640, 320), (1280, 1280))
COUT = (4, 14, 64, 128, 320, 640, 1280)
KERNEL = ((1, 1, 1), (1, 3, 3), (3, 3, 3))
STRIDE_UP = ((1, 0), (2, 0), (1, 1))              # (stride, upsample); an upsampling conv has stride 1
OUT_DTYPE = (_lib.GG_BF16, _lib.GG_F32)
ACT = (0, 1, 2)
SKIP = (0, 1)                                     # skip_C1 = 0 / C1
HINT = (0, 1)
STRIDE = 131

FIELDS = ["N", "D", "H", "W", "C1", "C2", "Cout", "Cout_pad", "kd", "kh", "kw", "stride", "pad", "upsample", "Do", "Ho", "Wo", "out_dtype",
          "prologue_act", "pro_c_logical", "skip_C1", "path_hint"]
PREDICATES = ["gg_conv_runs_halo_tile", "gg_conv_fuses_prologue", "gg_conv_prologue_from_acc", "gg_conv_fuses_skip", "gg_conv_fuses_ddim",
              "gg_conv_fuses_posterior", "gg_conv_emits_stats", "gg_conv_workspace_bytes"]


def cases():
    axes = (BATCH, EXTENT, CHANNELS, COUT, KERNEL, STRIDE_UP, OUT_DTYPE, ACT, SKIP, HINT)
    for a in axes:
        assert STRIDE % len(a), "STRIDE must be prime to every axis length"
    heads = (BATCH, EXTENT, ((64, 0),), (4, 14), KERNEL[1:], ((1, 0),), (_lib.GG_F32,), ACT, (0,), HINT)
    picked = [c for i, c in enumerate(itertools.product(*axes)) if i % STRIDE == 0]
    thinned = set(picked)
    picked += [c for c in itertools.product(*heads) if c not in thinned]
    for n, sp, (c1, c2), cout, k, (stride, up), dt, act, skip, hint in picked:
        pad = 0 if k == (1, 1, 1) else 1
        do, ho, wo = conv_out_extent(sp, k, stride, pad, bool(up))
        yield [n, *sp, c1, c2, cout, pad32(cout), *k, stride, pad, up, do, ho, wo, dt, act, c1 + c2, c1 if skip else 0, hint]


def main(lib_path, out_dir):
    lib = C.CDLL(lib_path)
    for name in PREDICATES:
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    rows = []
    for row in cases():
        d = _lib.ConvDesc()
        for f, v in zip(FIELDS, row):
            setattr(d, f, v)
        rows.append(row + [int(getattr(lib, name)(C.byref(d))) for name in PREDICATES])
    for j, f in enumerate(FIELDS + PREDICATES):
        print(f"{f}: {len(set(r[j] for r in rows))} distinct values, {sum(1 for r in rows if r[j])} non-zero")
    path = os.path.join(out_dir, "conv_dispatch.json")
    with open(path, "w") as fh:
        fh.write('{"fields": %s,\n "predicates": %s,\n "cases": [\n' % (json.dumps(FIELDS), json.dumps(PREDICATES)))
        fh.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
        fh.write("\n]}\n")
    print(f"wrote {path}: {len(rows)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else HERE)
