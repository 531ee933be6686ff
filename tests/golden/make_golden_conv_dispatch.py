"""Generates tests/golden/conv_dispatch.json and tests/golden/conv_dispatch_routes.json: what the host-side conv dispatch predicates of
libguidegen_hip.so answer for two sweeps of descriptors.  The predicates read no pointers and launch nothing (a dispatch walk that does not launch makes no HIP call), so this needs no GPU.

Run it on a library built from the commit whose dispatch is to be pinned (the PARENT of a refactor, never the code under test):
    python tests/golden/make_golden_conv_dispatch.py PATH/TO/libguidegen_hip.so [OUT_DIR]

The sweep is the full product of the axes below, thinned to every STRIDE-th case (STRIDE is prime to every axis length, so every value
of every axis, and every pair of values of the faster axes, stays in), plus every head conv unthinned (64 channels to 4 or 14 fp32 couts,
3-tap kernels, stride 1): the fused DDIM and CCDM epilogues exist only there, and the thinned product alone would meet them a few times.
Every descriptor field that is set is written out, so the test rebuilds each descriptor from the fixture alone.

The second table, conv_dispatch_routes.json, pins all eleven predicates, so that one row fixes a whole route through gg_conv_forward's
kernel ladder: gg_conv_runs_tile, gg_conv_runs_halo_split and gg_conv_runs_tile_s2 decide on 3-D grids of 64 to 512 channels under the
hints 12 to 15, which the first sweep does not hold.  Its product is thinned by the same rule (ROUTE_STRIDE); the production shapes that
tests/test_conv_tile_cpu.py, test_conv_tile_s2_cpu.py and test_halo_split_cpu.py name come unthinned under every hint, and ROUTE_EXTRA
holds one 2-D box or head conv for each predicate that 3-D grids of 64 couts and more cannot move (fused DDIM / CCDM epilogue, skip
projection, prologue from accumulators).
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
ROUTE_BATCH = (1, 2)
ROUTE_EXTENT = [(s, s, s) for s in (8, 16, 32, 64, 128)] + [(8, 16, 16)]
ROUTE_CHANNELS = ((64, 0), (128, 0), (64, 64), (128, 64), (128, 128), (160, 0), (256, 0), (256, 256), (512, 0))
ROUTE_COUT = (64, 128, 256)
ROUTE_KERNEL = ((1, 1, 1), (3, 3, 3))
ROUTE_STRIDE_UP = ((1, 0), (2, 0))
ROUTE_ACT = (0, 1)
ROUTE_HINT = (0, 12, 13, 14, 15)
ROUTE_STRIDE = 11
# (cube, C1, C2, Cout, kernel extent, stride) of the CCDM UNet: the streaming 1x1 skip projections, the five 3x3x3 shapes of the 16^3 level
# (batch 1, batch 2, and batch 2 at half the depth) and the Downsample convs
ROUTE_PRODUCTION = ([(1, (c,) * 3, c1, c2, co, 1, 1) for c, c1, c2, co in ((128, 128, 64, 64), (128, 64, 64, 64), (64, 128, 128, 128), (64, 128, 64, 128), (64, 64, 0, 128))]
                    + [(n, sp, c1, c2, 256, 3, 1) for n, sp in ((1, (16, 16, 16)), (2, (16, 16, 16)), (2, (8, 16, 16)))
                       for c1, c2 in ((128, 0), (256, 0), (320, 256), (256, 256), (256, 128))]
                    + [(1, (c,) * 3, ch, 0, ch, 3, 2) for c, ch in ((128, 64), (64, 128), (32, 128), (16, 256), (8, 320))])
# (N, extent, C1, Cout, kernel, out dtype, prologue_act, skip): latent-UNet head and ResBlock convs on the box kernel, the CCDM head @128^3
ROUTE_EXTRA = ((1, (1, 64, 64), 320, 4, (1, 3, 3), _lib.GG_F32, 1, 0), (1, (1, 32, 32), 640, 640, (1, 3, 3), _lib.GG_BF16, 1, 1),
               (1, (1, 16, 16), 1280, 1280, (1, 3, 3), _lib.GG_BF16, 0, 1), (1, (128, 128, 128), 64, 14, (3, 3, 3), _lib.GG_F32, 1, 0))

PREDICATES = ["gg_conv_runs_halo_tile", "gg_conv_fuses_prologue", "gg_conv_prologue_from_acc", "gg_conv_fuses_skip", "gg_conv_fuses_ddim",
              "gg_conv_fuses_posterior", "gg_conv_emits_stats", "gg_conv_workspace_bytes"]
ROUTE_PREDICATES = PREDICATES + ["gg_conv_runs_tile", "gg_conv_runs_halo_split", "gg_conv_runs_tile_s2"]


def cases():
    axes = (BATCH, EXTENT, CHANNELS, COUT, KERNEL, STRIDE_UP, OUT_DTYPE, ACT, SKIP, HINT)
    for a in axes:
        assert STRIDE % len(a), "STRIDE must be prime to every axis length"
    heads = (BATCH, EXTENT, ((64, 0),), (4, 14), KERNEL[1:], ((1, 0),), (_lib.GG_F32,), ACT, (0,), HINT)
    picked = [c for i, c in enumerate(itertools.product(*axes)) if i % STRIDE == 0]
    thinned = set(picked)
    picked += [c for c in itertools.product(*heads) if c not in thinned]
    yield from rows_of(picked)


def route_cases():
    axes = (ROUTE_BATCH, ROUTE_EXTENT, ROUTE_CHANNELS, ROUTE_COUT, ROUTE_KERNEL, ROUTE_STRIDE_UP, OUT_DTYPE, ROUTE_ACT, ROUTE_HINT)
    for a in axes:
        assert ROUTE_STRIDE % len(a), "ROUTE_STRIDE must be prime to every axis length"
    picked = [(*c[:-1], 0, c[-1]) for i, c in enumerate(itertools.product(*axes)) if i % ROUTE_STRIDE == 0]          # (no skip projection)
    production = [(n, sp, (c1, c2), cout, (k,) * 3, (stride, 0), _lib.GG_BF16, 0, 0, hint)
                  for n, sp, c1, c2, cout, k, stride in ROUTE_PRODUCTION for hint in ROUTE_HINT]
    thinned = set(picked)
    picked += [c for c in production if c not in thinned]
    picked += [(n, sp, (c1, 0), cout, k, (1, 0), dt, act, skip, 0) for n, sp, c1, cout, k, dt, act, skip in ROUTE_EXTRA]
    yield from rows_of(picked)


def rows_of(picked):
    for n, sp, (c1, c2), cout, k, (stride, up), dt, act, skip, hint in picked:
        pad = 0 if k == (1, 1, 1) else 1
        do, ho, wo = conv_out_extent(sp, k, stride, pad, bool(up))
        yield [n, *sp, c1, c2, cout, pad32(cout), *k, stride, pad, up, do, ho, wo, dt, act, c1 + c2, c1 if skip else 0, hint]


def write_table(lib, out_dir, fname, descs, predicates):
    rows = []
    for row in descs:
        d = _lib.ConvDesc()
        for f, v in zip(FIELDS, row):
            setattr(d, f, v)
        rows.append(row + [int(getattr(lib, name)(C.byref(d))) for name in predicates])
    for j, f in enumerate(FIELDS + predicates):
        print(f"{f}: {len(set(r[j] for r in rows))} distinct values, {sum(1 for r in rows if r[j])} non-zero")
    path = os.path.join(out_dir, fname)
    with open(path, "w") as fh:
        fh.write('{"fields": %s,\n "predicates": %s,\n "cases": [\n' % (json.dumps(FIELDS), json.dumps(predicates)))
        fh.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
        fh.write("\n]}\n")
    print(f"wrote {path}: {len(rows)} cases, {os.path.getsize(path)} bytes")
    return rows


def main(lib_path, out_dir):
    lib = C.CDLL(lib_path)
    for name in ROUTE_PREDICATES:
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    first = write_table(lib, out_dir, "conv_dispatch.json", cases(), PREDICATES)
    routes = write_table(lib, out_dir, "conv_dispatch_routes.json", route_cases(), ROUTE_PREDICATES)
    assert len(routes) <= len(first), "the routes table stays the smaller one"
    for j, name in enumerate(ROUTE_PREDICATES):
        assert len({r[len(FIELDS) + j] for r in routes}) >= 2, f"{name} gives one answer only in the routes table"


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else HERE)
