"""GPU suite: the launches and results of every sampler case of tests/chain_trace.py against the fingerprints recorded at the parent
commit of the chain restructuring (tests/golden/chain_launch_traces.json, written by tests/golden/make_golden_chain_traces.py).  Per
case and per call (eager, capture + replay, replay) the entries are compared in order, each by a digest over every operand and scalar
argument, and the returned tensors by their SHA-1 digests.  Each planted defect must fail against the fixture, named by case and by the
entry it touches."""
import json
import os

import pytest
import torch

import chain_trace as CT
from util import GOLD

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLD, "chain_launch_traces.json")) as f:
    FIXTURE = json.load(f)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def test_the_fixture_holds_every_case_and_every_wrapped_name():
    assert sorted(FIXTURE) == CT.case_names()
    names = {e.split(":")[0] for t in FIXTURE.values() for call in t["calls"] for e in call.split()}
    assert names == set(CT.OPS) | set(CT.UNET) - {"context_cl"}, names          # context_cl: the ancestral context path, in no listed case
    for name, t in FIXTURE.items():
        assert len(t["calls"]) == len(t["results"]) == CT.CALLS and len(set(t["results"])) == 1, name        # graph == eager, bit for bit
        names_of = lambda call: {e.split(":")[0] for e in call.split()}
        if "capture_graph" in names_of(t["calls"][1]):
            assert not {"forward_cl", "capture_graph"} & names_of(t["calls"][2]), name          # a replay records nothing of the chain


@pytest.mark.parametrize("name", CT.case_names())
def test_launches_and_results_equal_the_parent_commits(dev, name):
    diff = CT.compare(CT.trace(name, dev), FIXTURE[name])
    assert not diff, "\n".join(diff)


def first(trace, op, nth=0):
    """Index of the nth `op` entry of the first (eager) call."""
    return [i for i, e in enumerate(trace["calls"][0]) if e["op"] == op][nth]


# (defect, case, the entry of the eager call that must be named: op and which of its occurrences)
PLANTED = [
    ("blend_after_step", "ddim-inpaint-mask1-tape", ("inpaint_blend", 0)),       # fused head: the blend follows forward_cl
    ("blend_after_step", "ddim-inpaint-maskC-draw", ("inpaint_blend", 0)),
    ("plms_bias_row", "plms", ("forward_cl", 1)),
    ("plms_bias_row", "plms-inpaint", ("forward_cl", 1)),
    ("log_slot", "ddim-log_every_t2", ("log_rows", 0)),
    ("log_slot", "anc-log_every_t2", ("log_rows", 0)),
]


@pytest.mark.parametrize("defect, name, entry", PLANTED, ids=[f"{p[0]}-{p[1]}" for p in PLANTED])
def test_planted_defects_fail_by_case_and_entry(dev, defect, name, entry):
    clean, bad = CT.trace(name, dev), CT.trace(name, dev, defect)
    assert not CT.compare(clean, FIXTURE[name])
    diff = "\n".join(CT.compare(bad, FIXTURE[name]))
    i = first(clean, *entry)
    assert f"call 0 entry {i}" in diff, (i, diff)
    assert "call 0: returned tensors" in diff, diff                              # the defect also moves what the call returns
