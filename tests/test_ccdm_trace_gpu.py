"""GPU suite: the launches and results of every label-chain case of tests/ccdm_trace.py against the fingerprints recorded at the parent
commit of the label chain's restructuring (tests/golden/ccdm_launch_traces.json, written by tests/golden/make_golden_ccdm_traces.py).
Per case and per call the entries are compared in order, each by a digest over every operand and scalar argument, and the returned
tensors by their SHA-1 digests.  The step graph lives for one call, so the three calls of a case are equal to each other.  Each planted
defect must fail against the fixture, named by case and by the entry it touches."""
import json
import os

import pytest
import torch

import ccdm_trace as LT
import chain_trace as CT
from util import GOLD

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLD, "ccdm_launch_traces.json")) as f:
    FIXTURE = json.load(f)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def test_the_fixture_holds_every_case_and_every_wrapped_name():
    assert sorted(FIXTURE) == LT.case_names()
    names_of = lambda call: {e.split(":")[0] for e in call.split()}
    assert set().union(*(names_of(call) for t in FIXTURE.values() for call in t["calls"])) == set(LT.OPS) | set(LT.UNET)
    for name, t in FIXTURE.items():
        assert len(t["calls"]) == len(t["results"]) == CT.CALLS, name
        assert len(set(t["calls"])) == 1 and len(set(t["results"])) == 1, name    # the graph is per call: every call is the first
    graphed = {name for name, t in FIXTURE.items() if "capture_graph" in names_of(t["calls"][0])}
    assert graphed == {n for n in FIXTURE if "tape" not in n and n not in ("philox-graph-off", "subsampled-3")}, graphed
    # eager and graph, and a mask that keeps nothing, return the bits of the plain chain
    for same in ("philox-graph-off", "masked-keep-none"):
        assert FIXTURE[same]["results"] == FIXTURE["philox"]["results"], same


@pytest.mark.parametrize("name", LT.case_names())
def test_launches_and_results_equal_the_parent_commits(dev, name):
    diff = CT.compare(LT.trace(name, dev), FIXTURE[name])
    assert not diff, "\n".join(diff)


def first(trace, op, nth=0):
    """Index of the nth `op` entry of the first call."""
    return [i for i, e in enumerate(trace["calls"][0]) if e["op"] == op][nth]


# (defect, case, the entry of the first call that must be named: op and which of its occurrences)
PLANTED = [
    ("blend_after_step", "masked-philox", ("ccdm_inpaint_blend", 0)),
    ("blend_after_step", "masked-tape-trace", ("ccdm_inpaint_blend", 0)),
    ("stale_onehot", "philox", ("ccdm_posterior_sample", 0)),
    ("bias_row", "philox-graph-off", ("forward_cl", 1)),
]


@pytest.mark.parametrize("defect, name, entry", PLANTED, ids=[f"{p[0]}-{p[1]}" for p in PLANTED])
def test_planted_defects_fail_by_case_and_entry(dev, defect, name, entry):
    clean, bad = LT.trace(name, dev), LT.trace(name, dev, defect)
    assert not CT.compare(clean, FIXTURE[name])
    diff = "\n".join(CT.compare(bad, FIXTURE[name]))
    i = first(clean, *entry)
    assert f"call 0 entry {i}" in diff, (i, diff)
    assert "call 0: returned tensors" in diff, diff                              # the defect also moves what the call returns
