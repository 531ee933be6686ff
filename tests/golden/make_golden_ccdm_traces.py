"""Generates tests/golden/ccdm_launch_traces.json: per label-chain case of tests/ccdm_trace.py and per call a fingerprint of the launch
trace (chain_trace.fingerprint: one digest per entry, which holds every operand's shape, dtype, strides, offset and buffer number and
every scalar argument) and the digests of the tensors the call returned.  Needs the GPU.

Run it at the commit whose launches and results are to be pinned (the PARENT of a restructuring of the label chain, never the code
under test), twice: the two files must be equal byte for byte, else a case is not reproducible and is a finding of its own.
    python tests/golden/make_golden_ccdm_traces.py [OUT_DIR]

The committed fixture was generated at commit f5752cf ("Latent samplers: one chain state for DDIM, PLMS, DPM-Solver, ancestral"), the
parent of the change that introduced ccdm.LabelChain, and is committed unchanged."""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import torch  # noqa: E402

import ccdm_trace  # noqa: E402
from chain_trace import fingerprint  # noqa: E402


def main(out_dir):
    from jointimagegeneration_amd import _lib
    _lib.load()
    dev = torch.device("cuda:0")
    names = ccdm_trace.case_names()
    path = os.path.join(out_dir, "ccdm_launch_traces.json")
    entries = 0
    with open(path, "w") as f:
        f.write("{\n")
        for i, name in enumerate(names):
            t = ccdm_trace.trace(name, dev)
            fp = fingerprint(t)
            entries += sum(len(c) for c in t["calls"])
            if len(set(fp["calls"])) != 1 or len(set(fp["results"])) != 1:
                print(f"NOTE {name}: the three calls differ: {fp}")
            f.write(f" {json.dumps(name)}: {json.dumps(fp)}" + (",\n" if i + 1 < len(names) else "\n"))
            print(f"{name}: {[len(c) for c in t['calls']]} entries", flush=True)
        f.write("}\n")
    print(f"wrote {path}: {len(names)} cases, {entries} entries, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
