"""CPU suite: the ops launches of every network block against the fingerprints recorded at the parent commit of the network-layer
refactor (tests/golden/block_launch_traces.json, written by tests/golden/make_golden_block_traces.py; the recorder and the cases are
tests/block_trace.py).  Launches are compared in order, each by a digest over every operand's provenance and every scalar argument,
pack events as a set, and a second run of a module packs nothing.  Each planted defect must fail against the fixture at the launch it
touches, and against the clean trace by the name of the argument."""
import json
import os

import pytest

import block_trace as BT
from util import GOLD

with open(os.path.join(GOLD, "block_launch_traces.json")) as f:
    FIXTURE = json.load(f)


def test_the_cases_cover_every_op_and_conv_feature_under_both_settings():
    assert sorted(FIXTURE) == sorted(f"{name}/{label}" for name in BT.case_names() for label, _ in BT.settings())
    launches = [e for t in BT.record_all().values() for e in t["launches"]]
    assert len(launches) == sum(len(t["launches"].split()) for t in FIXTURE.values())
    assert {"conv", "attention", "layernorm", "layernorm_rows", "gelu", "geglu", "groupnorm_stats", "groupnorm_apply",
            "groupnorm_scale_shift_acc", "groupnorm_f32", "groupnorm_f32_film", "film_fold", "resample2x", "embed_rows", "bert_embed",
            "interpolate2d"} <= {e["op"] for e in launches}
    convs = [e for e in launches if e["op"] == "conv"]
    for kw in ("skip", "prologue", "prologue_acc", "geglu", "upsample", "bias_per_sample", "residual", "out_f32", "want_stats", "src2", "ddim", "post"):
        assert any(kw in e for e in convs), kw                      # both arms of the skip fusion, every conv feature the blocks use
    assert any(e["op"] == "attention" and "kv_len" in e for e in launches)


@pytest.mark.parametrize("label, answer", BT.settings())
@pytest.mark.parametrize("name", BT.case_names())
def test_launches_equal_the_parent_commits(name, label, answer):
    diff = BT.compare(BT.trace(name, answer), FIXTURE[f"{name}/{label}"])
    assert not diff, "\n".join(diff)


# (defect, case, what fails against the fixture, the arguments named against the clean trace)
PLANTED = [
    ("swap_kv_offset", "AttentionBlock-new_order", ["launch 3 attention:"], ["attention.k_off: got 128, want 64", "attention.v_off: got 64, want 128"]),
    ("swap_kv_offset", "BertModel", ["attention:"], ["attention.k_off", "attention.v_off"]),
    ("legacy_stride", "AttentionBlock-new_order", ["launch 3 attention:"], ["attention.ld_hs_q: got [192, 96], want [192, 32]", "attention.ld_hs_k", "attention.ld_hs_v"]),
    ("legacy_stride", "SpatialTransformer-context1-geglu1", ["attention:"], ["attention.ld_hs_q", "attention.ld_hs_k"]),
    ("wrong_pad", "ResBlock-skip3x3", ["launch 0 conv:"], ["conv.pad"]),
    ("wrong_pad", "AttnBlock2d", ["conv:"], ["conv.pad"]),
    ("wrong_cin_pad", "ResBlock-src2", ["conv:", "pack event not in the fixture", '"cin_pad": 128', "of the fixture missing"],
     ["conv.weight: got 'pack:in_layers.2/128/", "pack event added", "pack event missing"]),
    ("wrong_cin_pad", "TransformerWrapper-dim48", ["conv:", "of the fixture missing"], ["conv.weight"]),
]


@pytest.mark.parametrize("defect, name, at, named", PLANTED, ids=[f"{p[0]}-{p[1]}" for p in PLANTED])
def test_planted_defects_fail_by_name(defect, name, at, named):
    assert defect in BT.DEFECTS
    clean, bad = BT.trace(name, False), BT.trace(name, False, defect)
    assert not BT.compare(clean, FIXTURE[f"{name}/all_false"])
    against_fixture = "\n".join(BT.compare(bad, FIXTURE[f"{name}/all_false"]))
    by_argument = "\n".join(BT.diff_traces(bad, clean))
    for what in at:
        assert what in against_fixture, (what, against_fixture)
    for what in named:
        assert what in by_argument, (what, by_argument)
