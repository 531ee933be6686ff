"""Generates tests/golden/block_launch_traces.json: a fingerprint (block_trace.fingerprint: one digest per launch entry, which holds
the operands by provenance and every scalar and keyword argument, and one per pack event) of every block configuration in
tests/block_trace.py, under the dispatch predicates pinned all False and all True.  The launching functions are replaced by
recorders, so this needs neither a GPU nor the library.

Run it at the commit whose launches are to be pinned (the PARENT of a refactor of the network layer, never the code under test):
    python tests/golden/make_golden_block_traces.py [OUT_DIR]

The committed fixture was generated at commit 24abcb1 ("Conv host layer: one walk of the kernel ladder, predicates read it"), the parent
of the change that introduced blocks.conv_of / blocks.qkv_attention / blocks.layernorm_cl, and is committed unchanged."""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import block_trace  # noqa: E402


def main(out_dir):
    traces = block_trace.record_all()
    path = os.path.join(out_dir, "block_launch_traces.json")
    with open(path, "w") as f:
        f.write("{\n")
        for i, (name, t) in enumerate(sorted(traces.items())):
            assert not t["rerun"]["packs"] and t["rerun"]["same_launches"], name
            f.write(f" {json.dumps(name)}: {json.dumps(block_trace.fingerprint(t))}" + (",\n" if i + 1 < len(traces) else "\n"))
        f.write("}\n")
    launches = sum(len(t["launches"]) for t in traces.values())
    print(f"wrote {path}: {len(traces)} traces, {launches} launches, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
