"""CPU-side checks of RNN encoder training (unast_amd.train_rnn): the fp64 mirror (tests/rnn_train_mirror.py) against the reference's
fixture (tests/golden/rnn_encoder_train.npz, tools/gen_golden_rnn_encoder_train.py), the C ABI's new symbols, the refusals that need no
GPU, and the gradient metric of tests/test_gpu_rnn_train_model.py against two planted faults."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import dropout_mirror as DM
from tests import rnn_train_mirror as TM
from tests import rnn_weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRAD_CAP, GRAD_MARGIN = 1e-3, 16.0          # tests/test_gpu_vocoder_train.py
SIDES = [("text", "text", "text_len"), ("speech", "mel", "mel_len")]


@functools.lru_cache(maxsize=None)
def _fixture():
    z = np.load(os.path.join(GOLDEN, "rnn_encoder_train.npz"))
    return {k: z[k] for k in z.files}


def _inputs(side):
    fx = _fixture()
    sd = rnn_weights.fixture_state_dicts(fx)[0 if side == "text" else 1]
    xk, lk = ("text", "text_len") if side == "text" else ("mel", "mel_len")
    x = torch.from_numpy(fx[xk])
    cot = TM.cotangents(rnn_weights.meta_of(fx)["cot_seed"], x.shape[0], x.shape[1])
    return sd, x, fx[lk], cot


@functools.lru_cache(maxsize=None)
def _plain(side):
    sd, x, lens, cot = _inputs(side)
    return TM.run(side, sd, x, lens, cot)


@pytest.mark.parametrize("side", ["text", "speech"])
def test_mirror_reproduces_the_reference_fixture(side):
    fx, r = _fixture(), _plain(side)
    rel = lambda got, ref: np.abs(got - ref).max() / np.abs(ref).max()                           # noqa: E731
    worst = max(rel(r["h"].numpy(), fx[side + "/h"]), rel(r["c"].numpy(), fx[side + "/c"]),
                rel(TM.sample(r["enc_output"].numpy()), fx[side + "/enc_output"]))
    if side == "speech":
        worst = max(worst, rel(TM.sample(r["d_mel"].numpy()), fx["speech/d_mel"]))
    for k, v in r.items():
        if "running_" in k:
            worst = max(worst, rel(v.numpy(), fx[side + "/" + k]))
    keys = TM.trained_keys(dict(zip(rnn_weights.meta_of(fx)[side + "_keys"], rnn_weights.meta_of(fx)[side + "_keys"])))
    assert sorted(keys) == sorted(r["grads"])
    for k in keys:
        g = r["grads"][k]
        if k in TM.DEGENERATE:                                   # mathematically zero: rounding noise on both sides
            assert g.abs().max().item() <= 1e-12 and np.abs(fx["%s/gsample/%s" % (side, k)]).max() <= 1e-12
            continue
        gn = float(fx["%s/gnorm/%s" % (side, k)])
        worst = max(worst, rel(TM.sample(g.numpy()), fx["%s/gsample/%s" % (side, k)]), abs(g.norm().item() - gn) / gn)
    print("%s mirror against the reference fixture: %.2e" % (side, worst))
    assert worst <= 1e-9
    assert r["grads"]["prenet.embed.weight"][0].abs().max().item() == 0.0 if side == "text" else True


def test_header_declares_the_train_entry_points():
    from unast_amd import _lib
    protos = _lib.parse_header()
    assert "unast_lstm_seq_fwd_train" in protos and "unast_lstm_seq_bwd" in protos
    assert len(protos["unast_lstm_seq_fwd_train"][1]) == 15 and len(protos["unast_lstm_seq_bwd"][1]) == 12


def _cpu_models():
    from unast_amd.network import TextRNN, SpeechRNN
    return TextRNN(rnn_weights.rnn_args("luong")), SpeechRNN(rnn_weights.rnn_args("luong"))


def test_train_rnn_refusals_without_a_gpu():
    from unast_amd import train_rnn
    tm, sm = _cpu_models()
    text, mel = torch.ones(2, 5, dtype=torch.int64), torch.zeros(2, 6, 80)
    with pytest.raises(RuntimeError, match="train"):
        train_rnn.encoder_forward(tm.eval(), text, [5, 3])
    with pytest.raises(RuntimeError, match="train"):
        train_rnn.encoder_forward(sm.eval(), mel, [6, 3])
    tm.train(), sm.train()
    with pytest.raises(ValueError, match="max\\(lens\\)"):
        train_rnn.encoder_forward(tm, text, [4, 3])
    with pytest.raises(ValueError, match="max\\(lens\\)"):
        train_rnn.encoder_forward(sm, mel, [5, 6, 6])
    with pytest.raises(ValueError, match="CUDA"):
        train_rnn.encoder_forward(tm, text, [5, 3])
    with pytest.raises(ValueError, match="CUDA"):
        train_rnn.encoder_forward(sm, mel, [6, 3])
    with pytest.raises(TypeError):
        train_rnn.encoder_forward(torch.nn.Linear(2, 2), text, [5, 3])
    with pytest.raises(TypeError):
        train_rnn.encoder_backward(object())
    # the existing interface still refuses train mode
    with pytest.raises(NotImplementedError):
        tm.encode(text, [5, 3])


def _masks(side, B, T, seed=11):
    """Masks at the configs' probabilities on the fixture's shapes, from the kernels' RNG mirror (any masks would do for this check)."""
    N = B * T
    f = lambda stream, cols, p: torch.from_numpy(DM.drop_factor(seed, stream, N, cols, p))       # noqa: E731
    noise = torch.from_numpy(DM.row_keep(seed, 2, N, TM.NOISE_P).astype(np.float64))
    if side == "text":
        m = {"emb_dropout": f(1, 256, 0.5), "noise": noise, "dropout1": f(3, 256, 0.5), "dropout2": f(4, 256, 0.5), "dropout3": f(5, 256, 0.5)}
    else:
        m = {"noise": noise, "dropout2": f(3, 256, 0.5)}
    m["e_drop0"] = f(6, 512, 0.5)
    return m


@pytest.mark.parametrize("fault", TM.FAULTS)
@pytest.mark.parametrize("side", ["text", "speech"])
def test_the_gradient_metric_sees_the_planted_faults(side, fault):
    """Each planted fault moves some gradient by at least 10 x the bound the GPU test applies, on the fixture's shapes."""
    fx = _fixture()
    sd, x, lens, cot = _inputs(side)
    masks = _masks(side, x.shape[0], x.shape[1])
    good = TM.run(side, sd, x, lens, cot, masks=masks)
    bad = TM.run(side, sd, x, lens, cot, masks=masks, fault=fault)
    assert torch.equal(good["enc_output"], bad["enc_output"]) and torch.equal(good["h"], bad["h"])      # the forward is untouched
    names = [k for k in good["grads"] if k not in TM.DEGENERATE]
    e32 = max(float(fx["e32/%s/grad/%s" % (side, k)]) for k in names)
    bound = min(GRAD_CAP, GRAD_MARGIN * e32)
    errs = {k: TM.normerr(bad["grads"][k], good["grads"][k]) for k in names}
    worst = max(errs, key=errs.get)
    print("%s %s: bound %.2e, worst %s %.2e (%.0f x the bound)" % (side, fault, bound, worst, errs[worst], errs[worst] / bound))
    assert errs[worst] >= 10 * bound
