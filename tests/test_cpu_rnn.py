"""The RNN model family without a GPU: TextRNN / SpeechRNN speak the reference's state_dict, refuse what is not built, and the fp64 mirror
(tests/rnn_mirror.py) that the GPU tests lean on reproduces the reference's own fp64 results (tests/golden/rnn_values_*.npz) and loses them
under every planted fault."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import rnn_mirror as M
from tests import rnn_weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ATTNS = ["luong", "lsa"]
TRAJ_ATTNS = ["luong", "lsa"]  # one trajectory fixture per attention type (tools/gen_golden_rnn.py TRAJ_SETUP)
PARITY = 1e-3                  # the bound the GPU model tests apply (x max|ref|)


@functools.lru_cache(maxsize=None)
def _fixture(attn):
    z = np.load(os.path.join(GOLDEN, "rnn_values_%s.npz" % attn))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _mirror_outputs(attn, fault=None):
    fx = _fixture(attn)
    t_sd, s_sd = rnn_weights.fixture_state_dicts(fx)
    return M.value_outputs(t_sd, s_sd, attn, *[torch.from_numpy(fx[k]) for k in ("text", "text_len", "mel", "mel_len")], fault=fault)


def _rel_errors(attn, fault=None):
    fx = _fixture(attn)
    return {k: np.abs(v.numpy() - fx[k]).max() / np.abs(fx[k]).max() for k, v in _mirror_outputs(attn, fault).items()}


@pytest.mark.parametrize("attn", ATTNS)
def test_state_dict_keys_shapes_and_order_equal_the_references(attn):
    from unast_amd.network import TextRNN, SpeechRNN
    meta = rnn_weights.meta_of(_fixture(attn))
    for side, cls in (("text", TextRNN), ("speech", SpeechRNN)):
        sd = cls(rnn_weights.rnn_args(attn)).state_dict()
        assert list(sd.keys()) == meta[side + "_keys"]
        assert [list(v.shape) for v in sd.values()] == meta[side + "_shapes"]


@pytest.mark.parametrize("change", [dict(hidden=128, e_in=128, t_emb_dim=128, s_pre_hid=128, attn_dim=64), dict(hidden=128), dict(d_attn=None), dict(e_bi=False),
                                    dict(num_layers=1), dict(num_layers=3), dict(attn_dim=30), dict(attn_dim=128), dict(num_mels=82)])
def test_other_configurations_are_refused(change):
    from unast_amd.network import TextRNN, SpeechRNN
    args = rnn_weights.rnn_args("lsa")
    for k, v in change.items():
        setattr(args, k, v)
    for cls in (TextRNN, SpeechRNN):
        with pytest.raises(NotImplementedError, match="hidden = e_in = t_emb_dim = s_pre_hid = 256"):
            cls(args)


def test_train_mode_autograd_noise_and_teacher_ratio_are_refused():
    from unast_amd.network import TextRNN, SpeechRNN
    tm, sm = TextRNN(rnn_weights.rnn_args("luong")), SpeechRNN(rnn_weights.rnn_args("luong"))
    text, lens = torch.full((2, 5), 7, dtype=torch.int64), torch.tensor([5, 5])
    mel = torch.zeros(2, 5, 80)
    enc = ((torch.zeros(2, 2, 256), torch.zeros(2, 2, 256)), torch.zeros(2, 5, 512))
    mask = torch.zeros(2, 5, dtype=torch.bool)
    for m, x in ((tm, text), (sm, mel)):
        m.train()
        with torch.no_grad(), pytest.raises(NotImplementedError, match=r"train\(\) mode"):
            m.encode(x, lens)
        with torch.no_grad(), pytest.raises(NotImplementedError, match=r"train\(\) mode"):
            m(x, lens)
        m.eval()
        with pytest.raises(NotImplementedError, match="autograd"):
            m.encode(x, lens)
        with pytest.raises(NotImplementedError, match="autograd"):
            m.infer_sequence(enc, mask, max_len=4)
        with torch.no_grad(), pytest.raises(NotImplementedError, match="noise_in"):
            m.encode(x, lens, noise_in=True)
        with torch.no_grad(), pytest.raises(NotImplementedError, match="noise_in"):
            m(x, lens, noise_in=True)
        with torch.no_grad(), pytest.raises(NotImplementedError, match="teacher_ratio"):
            m.decode_sequence(x, lens, enc, mask, teacher_ratio=0.5)


def test_encode_needs_the_longest_sequence_to_fill_the_batch():
    """pad_packed_sequence without total_length (src/module.py:317): the reference only works when max(lens) == T."""
    from unast_amd.network import TextRNN, SpeechRNN
    tm, sm = TextRNN(rnn_weights.rnn_args("lsa")).eval(), SpeechRNN(rnn_weights.rnn_args("lsa")).eval()
    with torch.no_grad():
        for lens in ([4, 3], [6, 2], [5, 0], [5]):
            with pytest.raises(ValueError, match=r"max\(lens\) == T"):
                tm.encode(torch.full((2, 5), 7, dtype=torch.int64), torch.tensor(lens))
            with pytest.raises(ValueError, match=r"max\(lens\) == T"):
                sm.encode(torch.zeros(2, 5, 80), torch.tensor(lens))


def test_initialize_model_and_the_discriminator_batch_still_refuse_rnn():
    from unast_amd import train
    with pytest.raises(NotImplementedError):
        train.initialize_model(SimpleNamespace(model_type="rnn"))
    with pytest.raises(NotImplementedError):
        train.discriminator_shuffle_batch(torch.zeros(2, 3, 256), torch.tensor([3, 3]), torch.zeros(2, 4, 256), torch.tensor([4, 4]), "rnn")


@pytest.mark.parametrize("attn", ATTNS)
def test_mirror_reproduces_every_value_fixture_tensor(attn):
    fx = _fixture(attn)
    errs = _rel_errors(attn)
    recorded = {k for k in fx if "e32/" + k in fx}
    assert set(errs) == recorded, (sorted(recorded - set(errs)), sorted(set(errs) - recorded))
    assert max(errs.values()) <= 1e-9, errs


@pytest.mark.parametrize("attn", TRAJ_ATTNS)
def test_mirror_reproduces_the_trajectory_fixtures_exactly(attn):
    z = np.load(os.path.join(GOLDEN, "rnn_traj_%s.npz" % attn))
    fx = {k: z[k] for k in z.files}
    meta = rnn_weights.meta_of(fx)
    t_sd, s_sd = rnn_weights.fixture_state_dicts(fx)
    tm, sm = M.RNNModel("text", t_sd, attn), M.RNNModel("speech", s_sd, attn)
    text, text_len, mel, mel_len = [torch.from_numpy(fx[k]) for k in ("text", "text_len", "mel", "mel_len")]
    with torch.no_grad():
        t_eo, t_mask = tm.encode(text, text_len)
        s_eo, s_mask = sm.encode(mel, mel_len)
        tokens, tok_lens = tm.infer_sequence(s_eo, s_mask, meta["max_text"])
        pre, post, stop, stop_lens = sm.infer_sequence(t_eo, t_mask, meta["max_speech"])
    assert np.array_equal(tokens.numpy(), fx["tokens"]) and np.array_equal(tok_lens.numpy(), fx["text_lens"])
    assert np.array_equal(stop_lens.numpy(), fx["stop_lens"])
    for name, got in (("pre", pre), ("post", post), ("stop", stop)):
        assert np.abs(got.numpy() - fx[name]).max() <= 1e-9 * np.abs(fx[name]).max(), name
    # what the GPU test relies on: an early EOS and a run to max_len, several tokens, unequal stop lengths
    assert (fx["text_lens"] < meta["max_text"]).any() and (fx["text_lens"] == meta["max_text"]).any() and len(set(fx["tokens"].ravel())) >= 4
    assert len(set(fx["stop_lens"])) > 1 and (fx["stop_lens"] >= 8).any() and (fx["stop_lens"] == meta["max_speech"]).any()
    assert meta["margins"]["gap"] >= 1e-2 and meta["margins"]["stop_margin"] >= 1e-2


def test_mirror_lstm_direction_is_torchs_packed_lstm():
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    torch.manual_seed(0)
    lstm = torch.nn.LSTM(8, 16, bidirectional=True, batch_first=True).double()
    x, lens = torch.randn(3, 6, 8, dtype=M.F64), torch.tensor([6, 1, 4])
    with torch.no_grad():
        out, (hn, cn) = lstm(pack_padded_sequence(x, lens, batch_first=True, enforce_sorted=False))
        y, _ = pad_packed_sequence(out, batch_first=True, total_length=6)
        for d, sfx in enumerate(("", "_reverse")):
            g = lambda n: getattr(lstm, n + "_l0" + sfx)                       # noqa: E731
            yy, h, c = M.lstm_direction(x, lens, g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh"), reverse=bool(d))
            assert (yy - y[..., 16 * d:16 * d + 16]).abs().max() < 1e-12 and (h - hn[d]).abs().max() < 1e-12 and (c - cn[d]).abs().max() < 1e-12


@pytest.mark.parametrize("attn,fault", [(a, f) for a in ATTNS for f in M.FAULTS if a == "lsa" or f not in ("no_cum", "conv_shift")])
def test_the_parity_bound_sees_planted_faults(attn, fault):
    """Each fault moves at least one recorded tensor by 10 x the bound the GPU tests apply; otherwise the fixture would be too forgiving."""
    errs = _rel_errors(attn, fault)
    worst = max(errs, key=errs.get)
    print(fault, worst, errs[worst])
    assert errs[worst] >= 10 * PARITY, (fault, worst, errs[worst])
