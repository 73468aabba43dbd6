"""The C-ABI call sequence of one eager train step, and the node counts of the captured step, against the fixture written by
tools/gen_call_trace.py (tests/call_trace.py records; parity mode off, so every drop_p, seed and RNG stream id is in the trace).
With config.JOINT_GEN on the sequence must equal the fixture's exactly; with it off -- the single-call path, on which a sub-layer's backward
may issue its independent launches in another order -- as a multiset."""
import json
import os

import pytest

from tests import call_trace as CT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture(golden_dir):
    with open(os.path.join(golden_dir, CT.FIXTURE)) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CT.VARIANTS))
def test_train_step_issues_the_recorded_calls(name, fixture, monkeypatch):
    from unast_amd import ops
    settings, want = CT.VARIANTS[name], fixture[name]
    assert want["settings"] == settings
    panel, fused = list(ops.PANEL_LAUNCHES), ops.LNBWD_FUSED[0]
    with monkeypatch.context() as mp:
        got = CT.record_step(mp, settings)
    if settings["PANEL_MIN_ROWS"] == 1:     # both panel kernels and the fused LayerNorm backward served the small shape
        assert ops.PANEL_LAUNCHES[0] > panel[0] and ops.PANEL_LAUNCHES[1] > panel[1] and ops.LNBWD_FUSED[0] > fused
    else:
        assert ops.PANEL_LAUNCHES == panel and ops.LNBWD_FUSED[0] == fused
    want = want["records"]
    print(name, len(got), "records, fixture", len(want))
    if settings["JOINT_GEN"]:
        diff = CT.first_difference(got, want)
        assert diff is None, "first differing record at index %d:\n got  %r\n want %r" % diff
    else:
        assert len(got) == len(want), (len(got), len(want))
        diff = CT.first_difference(CT.as_multiset(got), CT.as_multiset(want))
        assert diff is None, "first differing record of the sorted lists at index %d:\n got  %s\n want %s" % diff


@pytest.mark.parametrize("name", CT.GRAPHED)
def test_captured_step_has_the_recorded_node_counts(name, fixture, monkeypatch):
    with monkeypatch.context() as mp:
        info = CT.captured_counts(mp, CT.VARIANTS[name])
    print(name, info, "fixture", fixture[name]["graph"])
    assert {k: info[k] for k in CT.GRAPH_KEYS} == {k: fixture[name]["graph"][k] for k in CT.GRAPH_KEYS}
