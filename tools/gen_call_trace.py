#!/usr/bin/env python3
"""Writes tests/golden/call_trace_b4_t24_m64_l2.json: the C-ABI call sequence of one eager train step (tests/call_trace.py: every entry
point with its scalar arguments, null-ness of its pointers and stream ordinals) under the four settings of tests/test_gpu_call_trace.py,
and the node counts of the captured step.  Needs the GPU.  Goes through the public surface only (train.initialize_model, train.train_step,
GraphedTrainStep, config, utils, portable), so it runs unchanged on any commit whose call sequence is to become the yardstick."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import call_trace as CT  # noqa: E402


def main():
    out = {}
    for name, settings in CT.VARIANTS.items():
        with pytest.MonkeyPatch.context() as mp:
            out[name] = dict(settings=settings, records=CT.record_step(mp, settings))
        if name in CT.GRAPHED:
            with pytest.MonkeyPatch.context() as mp:
                info = CT.captured_counts(mp, settings)
            out[name]["graph"] = {k: info[k] for k in CT.GRAPH_KEYS + ("cross_stream_edges", "streams")}
        print(name, len(out[name]["records"]), "records", out[name].get("graph"))
    path = os.path.join(ROOT, "tests", "golden", CT.FIXTURE)
    with open(path, "w") as f:                       # one record per line: a changed launch shows as a changed line
        f.write("{\n")
        for i, (name, v) in enumerate(out.items()):
            f.write('"%s": {"settings": %s, "graph": %s, "records": [\n' % (name, json.dumps(v["settings"]), json.dumps(v.get("graph"))))
            f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in v["records"]))
            f.write("\n]}%s\n" % ("," if i + 1 < len(out) else ""))
        f.write("}\n")
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
