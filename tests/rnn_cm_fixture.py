"""Reading tests/golden/rnn_cm_{luong,lsa}.npz (tools/gen_golden_rnn_cm.py): the reference's cross-model sub-step and optimizer step on the cases of
tests/rnn_cm_mirror.CM_FIXTURE.  The bounds are tests/rnn_step_fixture.py's, applied to this fixture's own e32 figures.

The encoder-side gradients carry a flat 1e-3 bar with no e32 term, and here the re-encoders read GENERATED sequences: how close a correct fp32
implementation comes to that bar is set by the fixture's conditioning (the reference's own fp32 run is 3.3e-4 off on lsa case a's
query_layer.weight, where the kernels measure 0.78 of the bar), not by the kernels' order of sums alone.  A later kernel change that trips this
bar by a small factor should first be weighed against the fixture's e32."""
import json
import os

import numpy as np

from tests import rnn_step_fixture as SF

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("a", "b", "a_eps")
LOSS_KEYS = ("s_cm", "t_cm", "d_cm")
FRAME_MARGIN = 16.0                                   # frames and stop logits: 16 x e32 (5h's bound)
_FX = {}


def fixture(attn):
    if attn not in _FX:
        _FX[attn] = np.load(os.path.join(HERE, "golden", "rnn_cm_%s.npz" % attn))
    return _FX[attn]


def meta(attn):
    return json.loads(str(fixture(attn)["meta"]))


def grads(attn, case):
    """(grad samples, grad norms, e32s) of the sub-step, each {key: ...}."""
    fx = fixture(attn)
    g = SF.group(fx, "%s/g" % case)
    keys = list(g)
    return g, dict(zip(keys, fx["%s/gnorm" % case].tolist())), dict(zip(keys, fx["e32/%s/grad" % case].tolist()))


def running(attn, case):
    """({key: sample}, {key: e32}) of the running statistics after the sub-step."""
    fx = fixture(attn)
    g = SF.group(fx, "%s/running" % case)
    return g, dict(zip(g, fx["e32/%s/running" % case].tolist()))


def running_bound(want, e32):
    return max(SF.BUF_TOL * max(1.0, float(np.abs(want).max())), SF.GRAD_MARGIN * e32)
