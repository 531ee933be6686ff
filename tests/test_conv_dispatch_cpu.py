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
