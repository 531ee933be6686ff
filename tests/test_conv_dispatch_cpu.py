"""CPU suite: the conv dispatch predicates of the C-ABI answer exactly what tests/golden/conv_dispatch.json recorded
(tests/golden/make_golden_conv_dispatch.py: the sweep and how the fixture is made).  They are host logic -- no pointer is read, dry runs
return before any HIP call -- so which kernel a convolution runs on is pinned without a GPU."""
import ctypes as C
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_dispatch_answer_equals_the_recorded_one():
    from jointimagegeneration_amd import _lib, ops
    from util import load_lib
    lib = load_lib()
    with open(os.path.join(ROOT, "tests", "golden", "conv_dispatch.json")) as fh:
        gold = json.load(fh)
    fields, preds, cases = gold["fields"], gold["predicates"], gold["cases"]
    assert preds == ["gg_conv_runs_halo_tile", "gg_conv_fuses_prologue", "gg_conv_prologue_from_acc", "gg_conv_fuses_skip",
                     "gg_conv_fuses_ddim", "gg_conv_fuses_posterior", "gg_conv_emits_stats", "gg_conv_workspace_bytes"]
    assert len(cases) >= 4000
    wrong = []
    for row in cases:
        assert len(row) == len(fields) + len(preds)
        d = _lib.ConvDesc()
        for f, v in zip(fields, row):
            setattr(d, f, v)
        # the recorded output extents are the ones ops.conv() would ask for
        assert (d.Do, d.Ho, d.Wo) == ops.conv_out_extent((d.D, d.H, d.W), (d.kd, d.kh, d.kw), d.stride, d.pad, bool(d.upsample))
        for name, want in zip(preds, row[len(fields):]):
            got = int(getattr(lib, name)(C.byref(d)))
            if got != want:
                wrong.append((name, dict(zip(fields, row)), want, got))
    for j, name in enumerate(preds):           # the fixture exercises both answers of every predicate
        assert len({row[len(fields) + j] for row in cases}) >= 2, name
    assert not wrong, f"{len(wrong)} answers differ from the fixture, the first: {wrong[0]}"


ROUTE_PREDS = ["gg_conv_runs_halo_tile", "gg_conv_fuses_prologue", "gg_conv_prologue_from_acc", "gg_conv_fuses_skip", "gg_conv_fuses_ddim",
               "gg_conv_fuses_posterior", "gg_conv_emits_stats", "gg_conv_workspace_bytes", "gg_conv_runs_tile", "gg_conv_runs_halo_split",
               "gg_conv_runs_tile_s2"]


def _descriptors(*fixtures):
    """(fields, row, descriptor) of every case of the named fixtures"""
    from jointimagegeneration_amd import _lib
    for name in fixtures:
        with open(os.path.join(ROOT, "tests", "golden", name)) as fh:
            gold = json.load(fh)
        for row in gold["cases"]:
            d = _lib.ConvDesc()
            for f, v in zip(gold["fields"], row):
                setattr(d, f, v)
            yield gold, row, d


def test_every_route_equals_the_recorded_one():
    """conv_dispatch_routes.json: all eleven predicates, so that one row fixes a whole route through gg_conv_forward's kernel ladder
    (3-D grids of 64 to 512 channels under the hints 0 and 12 to 15, the CCDM production shapes under every hint)."""
    from jointimagegeneration_amd import ops
    from util import load_lib
    lib = load_lib()
    wrong, n, answers = [], 0, [set() for _ in ROUTE_PREDS]
    for gold, row, d in _descriptors("conv_dispatch_routes.json"):
        fields = gold["fields"]
        assert gold["predicates"] == ROUTE_PREDS and len(row) == len(fields) + len(ROUTE_PREDS)
        assert (d.Do, d.Ho, d.Wo) == ops.conv_out_extent((d.D, d.H, d.W), (d.kd, d.kh, d.kw), d.stride, d.pad, bool(d.upsample))
        for j, (name, want) in enumerate(zip(ROUTE_PREDS, row[len(fields):])):
            got = int(getattr(lib, name)(C.byref(d)))
            answers[j].add(want)
            if got != want:
                wrong.append((name, dict(zip(fields, row)), want, got))
        n += 1
    assert 2000 <= n <= 4077                     # no larger than the first fixture
    for name, seen in zip(ROUTE_PREDS, answers):
        assert len(seen) >= 2, name
    assert not wrong, f"{len(wrong)} answers differ from the fixture, the first: {wrong[0]}"


def test_the_answers_of_one_descriptor_agree():
    """What the predicates say about ONE descriptor describes one route (answers computed live, over the descriptors of both fixtures)."""
    from jointimagegeneration_amd._lib import GG_BF16
    from util import load_lib
    lib = load_lib()
    n = 0
    for gold, row, d in _descriptors("conv_dispatch.json", "conv_dispatch_routes.json"):
        a = {name: int(getattr(lib, name)(C.byref(d))) for name in ROUTE_PREDS}
        what = (dict(zip(gold["fields"], row)), a)
        halo, split = a["gg_conv_runs_halo_tile"], a["gg_conv_runs_halo_split"]
        # (a) one kernel runs the conv
        assert sum(1 for v in (halo, a["gg_conv_runs_tile"], a["gg_conv_runs_tile_s2"], split) if v) <= 1, what
        # (b) the split halo path's slabs are the workspace
        if split > 0:
            assert a["gg_conv_workspace_bytes"] == split * d.N * d.Do * d.Ho * d.Wo * d.Cout_pad * 4, what
        # (c) 32 stripes of GroupNorm statistics: the halo-tile kernel, and only it
        if d.out_dtype == GG_BF16 and not d.epilogue_geglu and d.C1 > 0 and d.C1 % 32 == 0 and d.C2 % 32 == 0 and d.Cout_pad % 32 == 0:
            assert (a["gg_conv_emits_stats"] == 32) == (halo == 1), what
        # (d) the box kernel's fusions are not the halo-tile kernel's
        if a["gg_conv_fuses_skip"] or a["gg_conv_fuses_ddim"] or a["gg_conv_prologue_from_acc"]:
            assert halo == 0, what
        n += 1
    assert n >= 6000
