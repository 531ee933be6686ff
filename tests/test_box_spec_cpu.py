"""CPU suite: the shape table of the specialised box convs (gg_conv_box_specs.inc) is well formed and consistent with the conv
arithmetic, and build.sh compiles its translation unit and rebuilds it when the table or the shared kernel header change.  (That the
table holds exactly the configurations the C5 latent UNet reaches at batch 1 is checked against the library's own trace on the GPU:
tests/test_box_spec_gpu.py.)"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jointimagegeneration_amd", "csrc")
FIELDS = ("H W C1 C2 Cout Cout_pad Ho Wo K3 UP TWI MT CT NS nstage nch_stage gn_bytes q_major skip_C1 skip_C2 nstage_s nch_stage_s "
          "pro acc bias res stats out_f32 ddim ddim_px0 ddim_uin").split()


def entries():
    out = []
    for ln in open(os.path.join(CSRC, "gg_conv_box_specs.inc")):
        if ln.startswith("GG_BOX_SPEC("):
            m = re.fullmatch(r"GG_BOX_SPEC\(([-0-9, ]+)\)", ln.strip())
            assert m, ln
            vals = [int(v) for v in m.group(1).split(",")]
            assert len(vals) == len(FIELDS), ln
            out.append(dict(zip(FIELDS, vals)))
    return out


def test_table_entries_are_consistent():
    es = entries()
    assert len(es) >= 20                                   # the latent UNet runs ~40 distinct box configurations at batch 1
    keys = [tuple(e.values()) for e in es]
    assert len(keys) == len(set(keys))
    for e in es:
        nchunk = (e["C1"] + e["C2"]) // 32
        assert e["C1"] % 32 == 0 and e["C2"] % 32 == 0 and e["Cout_pad"] % 32 == 0 and 0 < e["Cout"] <= e["Cout_pad"], e
        assert e["UP"] in (0, 1, 2) and e["K3"] in (0, 1) and (e["K3"] or e["UP"] == 0), e
        ext = {0: e["H"], 1: 2 * e["H"], 2: e["H"] // 2}[e["UP"]]
        assert e["Ho"] == ext and e["Wo"] == {0: e["W"], 1: 2 * e["W"], 2: e["W"] // 2}[e["UP"]], e
        assert e["TWI"] in (16, 8, 4) and e["Wo"] % e["TWI"] == 0 and e["CT"] in (1, 2) and e["NS"] in (1, 2, 4), e
        assert e["nstage"] >= 1 and (e["nstage"] - 1) * e["nch_stage"] < nchunk <= e["nstage"] * e["nch_stage"], e
        nsk = (e["skip_C1"] + e["skip_C2"]) // 32
        assert (nsk == 0) == (e["nstage_s"] == 0), e
        if nsk:
            assert e["K3"] and e["UP"] == 0 and (e["nstage_s"] - 1) * e["nch_stage_s"] < nsk <= e["nstage_s"] * e["nch_stage_s"], e
        assert e["pro"] in (0, 1, 2) and (e["pro"] or not e["acc"]) and (e["pro"] == 0) == (e["gn_bytes"] == 0), e
        assert all(e[k] in (0, 1) for k in ("acc", "bias", "res", "stats", "out_f32", "ddim", "ddim_px0", "ddim_uin")), e
        assert e["ddim"] or not (e["ddim_px0"] or e["ddim_uin"]), e
        assert not (e["ddim"] and not e["out_f32"]) and not (e["stats"] and e["out_f32"]), e


def test_build_compiles_the_table_and_tracks_its_dependencies():
    sh = open(os.path.join(CSRC, "build.sh")).read()
    assert re.search(r"for f in [^;]*\bgg_conv_box_spec\b", sh)
    # every object depends on every *.h / *.inc of csrc/ (a loop, not a list that a new header can be missing from): these two are such files
    assert re.search(r'for dep in \$1\.hip \./\*\.h \./\*\.inc [^;]*guidegen_hip\.h; do\s+if \[ "\$dep" -nt \$1\.o \]; then return 0; fi', sh)
    assert re.search(r"if stale \$f; then\s+echo \"hipcc \$f\.hip\"", sh)
    for dep in ("gg_conv_box_kernel.h", "gg_conv_box_specs.inc"):
        assert os.path.isfile(os.path.join(CSRC, dep)), dep
