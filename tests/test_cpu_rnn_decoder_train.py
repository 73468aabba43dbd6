"""CPU-side checks of SpeechRNN decoder training (unast_amd.train_rnn.decoder_forward / decoder_backward): the fp64 mirror
(tests/rnn_decoder_mirror.py) against the reference's fixtures (tests/golden/rnn_decoder_train_{luong,lsa}.npz,
tools/gen_golden_rnn_decoder_train.py), the C ABI's new symbols, the refusals that need no GPU, and the gradient metric of
tests/test_gpu_rnn_decoder_train.py against two planted faults."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import dropout_mirror as DM
from tests import rnn_decoder_mirror as RD
from tests import rnn_train_mirror as TM
from tests import rnn_weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRAD_CAP, GRAD_MARGIN = 1e-3, 16.0
ATTNS = ["luong", "lsa"]


@functools.lru_cache(maxsize=None)
def fixture(attn):
    z = np.load(os.path.join(GOLDEN, "rnn_decoder_train_%s.npz" % attn))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _sd(attn):
    m = rnn_weights.meta_of(fixture(attn))
    return rnn_weights.state_dict("speech", m["speech_keys"], m["speech_shapes"], m["seed"], m["gains"])


def case_a(attn):
    fx = fixture(attn)
    tgt = torch.from_numpy(fx["a_target"])
    cot = RD.cotangents(rnn_weights.meta_of(fx)["cot_seed"], tgt.shape[0], tgt.shape[1], tgt.shape[2])
    return tgt, torch.from_numpy(fx["a_enc_output"]), torch.from_numpy(fx["a_h"]), torch.from_numpy(fx["a_c"]), fx["a_lens_k"], cot


def case_b(attn):
    fx = fixture(attn)
    mel = torch.from_numpy(fx["b_mel"])
    return mel, fx["b_mel_len"], RD.cotangents(rnn_weights.meta_of(fx)["cot_seed"] + 1, mel.shape[0], mel.shape[1], mel.shape[2])


@functools.lru_cache(maxsize=None)
def mirror_a(attn):
    tgt, enc, h, c, lens_k, cot = case_a(attn)
    return RD.run(_sd(attn), attn, tgt, enc, h, c, lens_k, cot)


@functools.lru_cache(maxsize=None)
def mirror_b(attn):
    mel, lens, cot = case_b(attn)
    return RD.autoencoder(_sd(attn), attn, mel, lens, cot)


def grad_bounds(fx, case, names):
    """tests/rnn_decoder_mirror.grad_bounds over the fixture's e32 figures of one case."""
    return RD.grad_bounds({k: float(fx["e32/%s/grad/%s" % (case, k)]) for k in names}, GRAD_CAP, GRAD_MARGIN)


def _rel(got, ref):
    return np.abs(np.asarray(got) - ref).max() / max(np.abs(ref).max(), 1e-300)


def _check_grads_fp64(fx, case, grads, stride):
    worst = 0.0
    for k, g in grads.items():
        key = "%s/gsample/%s" % (case, k)
        if k in RD.DEGENERATE:
            assert g.abs().max().item() <= 1e-11 and float(fx["%s/gnorm/%s" % (case, k)]) <= 1e-11
            continue
        gn = float(fx["%s/gnorm/%s" % (case, k)])
        worst = max(worst, abs(g.norm().item() - gn) / gn)
        if key in fx:
            worst = max(worst, _rel(TM.sample(g.numpy())[::stride], fx[key]))
    return worst


@pytest.mark.parametrize("attn", ATTNS)
def test_mirror_reproduces_the_reference_fixture_decoder_alone(attn):
    fx, r = fixture(attn), mirror_a(attn)
    assert sorted(r["grads"]) == sorted(RD.trained_keys(_sd(attn)))
    worst = max(_rel(r[k].numpy(), fx["a/" + k]) for k in ("pre", "post", "stop", "d_h", "d_c"))
    worst = max(worst, _rel(TM.sample(r["d_enc_output"].numpy()), fx["a/d_enc_output"]))
    for k, v in r.items():
        if "running_" in k:
            worst = max(worst, _rel(v.numpy(), fx["a/" + k]))
    worst = max(worst, _check_grads_fp64(fx, "a", r["grads"], 1))
    print("%s decoder mirror against the reference fixture: %.2e" % (attn, worst))
    assert worst <= 1e-9
    lens_k = fx["a_lens_k"]
    for b in range(len(lens_k)):
        assert r["d_enc_output"][b, int(lens_k[b]):].abs().sum().item() == 0.0


@pytest.mark.parametrize("attn", ATTNS)
def test_mirror_reproduces_the_reference_fixture_autoencoder(attn):
    fx, r = fixture(attn), mirror_b(attn)
    worst = max(_rel(r[k].numpy(), fx["b/" + k]) for k in ("pre", "post", "stop", "h", "c"))
    worst = max(worst, _rel(TM.sample(r["enc_output"].numpy()), fx["b/enc_output"]), _rel(TM.sample(r["d_mel"].numpy()), fx["b/d_mel"]))
    for k, v in r.items():
        if "running_" in k:
            worst = max(worst, _rel(v.numpy(), fx["b/" + k]))
    assert sorted(r["grads"]) == sorted(k[len("b/gnorm/"):] for k in fx if k.startswith("b/gnorm/"))
    worst = max(worst, _check_grads_fp64(fx, "b", r["grads"], 2))
    print("%s autoencoder mirror against the reference fixture: %.2e" % (attn, worst))
    assert worst <= 1e-9


def test_fixtures_fit_the_size_limit():
    for attn in ATTNS:
        assert os.path.getsize(os.path.join(GOLDEN, "rnn_decoder_train_%s.npz" % attn)) <= 900000


def test_header_declares_the_decoder_train_entry_points():
    from unast_amd import _lib
    protos = _lib.parse_header()
    want = {"unast_rnn_attn_step_train": 22, "unast_rnn_attn_step_bwd": 36, "unast_rnn_attn_step_bwd_ws_floats": 3, "unast_lstm_cell_train": 15,
            "unast_lstm_cell_bwd": 19, "unast_tanh_bwd": 7}
    for name, nargs in want.items():
        assert name in protos and len(protos[name][1]) == nargs, name
    # the eval entry points keep their signatures
    assert len(protos["unast_rnn_attn_step"][1]) == 18 and len(protos["unast_lstm_cell"][1]) == 9


def test_decoder_refusals_without_a_gpu():
    from unast_amd import train_rnn
    from unast_amd.network import TextRNN, SpeechRNN
    tm, sm = TextRNN(rnn_weights.rnn_args("luong")), SpeechRNN(rnn_weights.rnn_args("lsa"))
    mel = torch.zeros(2, 6, 80)
    enc_outputs = ((torch.zeros(2, 2, 256), torch.zeros(2, 2, 256)), torch.zeros(2, 5, 512))
    with pytest.raises(NotImplementedError, match="TextPrenet"):
        train_rnn.decoder_forward(tm.train(), mel, enc_outputs, [5, 3])
    with pytest.raises(TypeError):
        train_rnn.decoder_forward(torch.nn.Linear(2, 2), mel, enc_outputs, [5, 3])
    with pytest.raises(RuntimeError, match="train"):
        train_rnn.decoder_forward(sm.eval(), mel, enc_outputs, [5, 3])
    sm.train()
    with pytest.raises(ValueError, match="CUDA"):
        train_rnn.decoder_forward(sm, mel, enc_outputs, [5, 3])
    with pytest.raises(ValueError):
        train_rnn.decoder_forward(sm, torch.zeros(2, 6, 79), enc_outputs, [5, 3])
    with pytest.raises(TypeError):
        train_rnn.decoder_backward(object())
    with pytest.raises(TypeError):
        train_rnn.decoder_backward(train_rnn.Tape())                     # an encoder tape
    with pytest.raises(TypeError):
        train_rnn.encoder_backward(train_rnn.DecoderTape())
    used = train_rnn.DecoderTape()
    used.used = True
    with pytest.raises(RuntimeError, match="used"):
        train_rnn.decoder_backward(used)
    # the existing interface still refuses train mode
    with pytest.raises(NotImplementedError):
        sm.decode_sequence(mel, [6, 6], enc_outputs, None)
    assert train_rnn.S_DPRE > train_rnn.S_EDROP + 1 and len({train_rnn.S_DPRE, train_rnn.S_DDROP, train_rnn.S_DOUT, train_rnn.S_POST}) == 4


def masks_for(B, T, seed=11, p_pre=0.5, p_dec=0.3, p_post=0.1):
    """Masks at the configs' probabilities on a case's shapes, from the kernels' RNG mirror (any masks would do for this check)."""
    f = lambda stream, rows, p: torch.from_numpy(DM.drop_factor(seed, stream, rows, 256, p))     # noqa: E731
    m = {"d_prenet_dropout": f(8, B * T, p_pre), "d_drop0": f(9, B * T, p_dec), "d_dropout1": f(10, B * T, p_dec)}
    for k in range(4):
        m["post_dropout%d" % k] = f(11 + k, B * (T + 1), p_post)
    return m


@pytest.mark.parametrize("attn,fault", [("luong", "query_after_lstm"), ("lsa", "query_after_lstm"), ("lsa", "lsa_cum_dropped")])
def test_the_gradient_metric_sees_the_planted_faults(attn, fault):
    """Each planted fault moves some gradient by orders of magnitude beyond the bound the GPU test applies (at least 100 x), on case a's shapes."""
    fx = fixture(attn)
    tgt, enc, h, c, lens_k, cot = case_a(attn)
    masks = masks_for(tgt.shape[0], tgt.shape[1])
    good = RD.run(_sd(attn), attn, tgt, enc, h, c, lens_k, cot, masks=masks)
    bad = RD.run(_sd(attn), attn, tgt, enc, h, c, lens_k, cot, masks=masks, fault=fault)
    assert torch.equal(good["pre"], bad["pre"]) and torch.equal(good["post"], bad["post"]) and torch.equal(good["stop"], bad["stop"])
    names = [k for k in good["grads"] if k not in RD.DEGENERATE]
    bounds, _ = grad_bounds(fx, "a", names)
    ratio = {k: TM.normerr(bad["grads"][k], good["grads"][k]) / bounds[k] for k in names}
    for k in ("d_enc_output", "d_h", "d_c"):
        ratio[k] = TM.normerr(bad[k], good[k]) / min(GRAD_CAP, GRAD_MARGIN * float(fx["e32/a/rel/" + k]))
    worst = max(ratio, key=ratio.get)
    print("%s %s: worst %s at %.0f x its bound" % (attn, fault, worst, ratio[worst]))
    assert ratio[worst] >= 100
