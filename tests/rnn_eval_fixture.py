"""What the tests of unast_amd.eval_rnn share: reading tests/golden/rnn_eval_{luong,lsa}.npz (tools/gen_golden_rnn_eval.py: the reference's own
evaluate() in fp64, and its fp32 run's error `e32`), the seeded weights and batches of its cases, and the bounds.

Bounds.  Tokens, lengths, JSON content and d_score: exact (the fixtures' decisions keep a margin of 1e-2 of the largest logit).  Losses:
rnn_step_fixture.LOSS_TOL x max(1, |ref|), the bound the step tests hold.  Frames and stop logits: 16 x their own e32 (DESIGN 5m's rule), e32
floored at the fp32 unit roundoff of the largest value."""
import json
import os

import numpy as np
import torch

from tests import rnn_cm_mirror as CM
from tests import rnn_step_fixture as SF

HERE = os.path.dirname(os.path.abspath(__file__))
ATTNS = ("luong", "lsa")
CASES = ("a", "b")
LOSS_TOL, MARGIN32 = SF.LOSS_TOL, 16.0
KEYS_D = ("t_ae", "s_ae", "d_ae", "asr", "tts", "d_sp", "s_cm", "t_cm", "d_cm", "dis")       # evaluate()'s keys in the order it fills them
KEYS_PLAIN = ("t_ae", "s_ae", "asr", "tts", "s_cm", "t_cm")
_FX = {}


def fixture(attn):
    if attn not in _FX:
        _FX[attn] = np.load(os.path.join(HERE, "golden", "rnn_eval_%s.npz" % attn))
    return _FX[attn]


def meta(attn):
    return json.loads(str(fixture(attn)["meta"]))


def setup(attn, case):
    return meta(attn)["setups"][case]


DISC_GAIN = 6.0         # on the discriminator's weight matrices: with the portable draw as it is, its logits barely respond to their input, and
                        # the d_* losses could not tell a wrong encoder output or a wrong length from a right one (tests/test_cpu_rnn_eval.py)


def with_disc_gain(sd, gain):
    return {k: (v * gain if k.startswith("discriminator.") and "weight" in k and v.is_floating_point() else v) for k, v in sd.items()}


def state_dict(attn, case):
    fx, m = setup(attn, case), SF.meta(attn)
    return with_disc_gain(CM.state_dict(m["keys"], m["shapes"], fx["weight_seed"], CM.gains(fx["eos_bias"], fx["stop_bias"])), fx["disc_gain"])


def batch(attn, case):
    text, mel, tl, ml = CM.fixture_batch(setup(attn, case))
    return text, mel, torch.tensor(tl), torch.tensor(ml)


def frame_bound(fx, name, ref):
    scale = float(np.abs(ref).max())
    return MARGIN32 * max(float(fx["e32/" + name]), 2.0 ** -24 * scale)
