"""TextRNN / SpeechRNN (unast_amd.network, unast_amd.rnn) on the GPU against the reference's own fp64 results (tests/golden/rnn_values_*.npz,
written by tools/gen_golden_rnn.py; weights rebuilt by tests/rnn_weights.py).  Bound: 1e-3 x max|ref| per tensor, the project's parity bar
(SURVEY.md section 8); each tensor's error is also printed as a multiple of the reference's own fp32-vs-fp64 error (e32)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import rnn_weights

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARITY = 1e-3
ATTNS = ["luong", "lsa"]
TRAJ_ATTNS = ["luong", "lsa"]  # one trajectory fixture per attention type (tools/gen_golden_rnn.py TRAJ_SETUP)


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _fixture(attn, kind="values"):
    z = np.load(os.path.join(GOLDEN, "rnn_%s_%s.npz" % (kind, attn)))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _models(attn, kind="values"):
    from unast_amd.network import TextRNN, SpeechRNN, UNAST
    fx = _fixture(attn, kind)
    t_sd, s_sd = rnn_weights.fixture_state_dicts(fx)
    tm, sm = TextRNN(rnn_weights.rnn_args(attn)), SpeechRNN(rnn_weights.rnn_args(attn))
    tm.load_state_dict(t_sd)
    sm.load_state_dict(s_sd)
    tm, sm = tm.to(_dev()).eval(), sm.to(_dev()).eval()
    return tm, sm, UNAST(tm, sm).eval()


def _batch(attn):
    fx, dev = _fixture(attn), _dev()
    return (torch.from_numpy(fx["text"]).to(dev), torch.from_numpy(fx["text_len"]), torch.from_numpy(fx["mel"]).to(dev), torch.from_numpy(fx["mel_len"]))


def _close(fx, name, got, report):
    ref = fx[name]
    got = got.detach().cpu().double().numpy()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err, mx = np.abs(got - ref).max(), np.abs(ref).max()
    report.append("%-22s err %.3g = %.3g of max|ref| = %.1f x e32" % (name, err, err / mx, err / float(fx["e32/" + name])))
    print(report[-1])
    return err <= PARITY * mx


@pytest.mark.parametrize("attn", ATTNS)
def test_value_fixtures_within_the_parity_bar(attn):
    fx = _fixture(attn)
    tm, sm, model = _models(attn)
    text, text_len, mel, mel_len = _batch(attn)
    rep, ok = [], []
    with torch.no_grad():
        ((h, c), eo), mask = tm.encode(text, text_len)
        assert mask.dtype == torch.bool and torch.equal(mask, text.eq(0))
        ok += [_close(fx, "text_enc_out", eo, rep), _close(fx, "text_h", h, rep), _close(fx, "text_c", c, rep)]
        for b in range(text.shape[0]):
            assert torch.equal(eo[b, int(text_len[b]):], torch.zeros_like(eo[b, int(text_len[b]):]))
        ((h, c), eo), mask = sm.encode(mel, mel_len)
        assert torch.equal(mask.cpu(), torch.arange(mel.shape[1])[None, :] >= mel_len[:, None])
        ok += [_close(fx, "speech_enc_out", eo, rep), _close(fx, "speech_h", h, rep), _close(fx, "speech_c", c, rep)]
        ok.append(_close(fx, "text_forward", tm(text, text_len), rep))
        pre, post, stop = sm(mel, mel_len)
        ok += [_close(fx, "speech_forward_pre", pre, rep), _close(fx, "speech_forward_post", post, rep), _close(fx, "speech_forward_stop", stop, rep)]
        pre, post, stop, lens = model.tts(text, text_len, mel, mel_len, infer=False)
        assert lens is mel_len
        ok += [_close(fx, "tts_pre", pre, rep), _close(fx, "tts_post", post, rep), _close(fx, "tts_stop", stop, rep)]
        ok.append(_close(fx, "asr", model.asr(text, text_len, mel, mel_len, infer=False), rep))
    assert all(ok), "\n".join(rep)


@pytest.mark.parametrize("attn", ATTNS)
def test_text_prenet_window_for_prefix_lengths_1_to_9_in_both_conventions(attn):
    """The last position of TextPrenet over a prefix, recomputed from a 7-token window: generation prefixes [SOS, c0, ...] and the
    teacher-forced ones ([SOS], then target[:, :i] without SOS)."""
    from unast_amd import rnn
    fx = _fixture(attn)
    tm, _, _ = _models(attn)
    text, _, _, _ = _batch(attn)
    dev = _dev()
    B = text.shape[0]
    with torch.no_grad():
        P = tm._pack()
        bufs = rnn.window_bufs(P, B, dev)
        gen_tokens = torch.cat([torch.full((B, 1), 1, dtype=torch.int64, device=dev), text[:, :9]], dim=1).contiguous()
        rep, ok = [], []
        for L in range(1, 10):
            pos = torch.tensor([L - 1], dtype=torch.int64, device=dev)
            got = rnn.text_prenet_last(P, gen_tokens, pos, False, bufs).clone()
            sub = {"x": fx["prenet_infer"][L - 1], "e32/x": fx["e32/prenet_infer"]}
            ok.append(_close(sub, "x", got, rep))
            pos = torch.tensor([L], dtype=torch.int64, device=dev)
            got = rnn.text_prenet_last(P, text.contiguous(), pos, True, bufs).clone()
            sub = {"x": fx["prenet_tf"][L - 1], "e32/x": fx["e32/prenet_tf"]}
            ok.append(_close(sub, "x", got, rep))
        got = rnn.text_prenet_last(P, text.contiguous(), torch.zeros(1, dtype=torch.int64, device=dev), True, bufs).clone()       # step 0: [SOS]
        ok.append(_close({"x": fx["prenet_infer"][0], "e32/x": fx["e32/prenet_infer"]}, "x", got, rep))
    assert all(ok), "\n".join(rep)


@pytest.mark.parametrize("attn", ATTNS)
def test_prenet_rows_the_teacher_forced_text_steps_feed(attn):
    """Step i of TextRNN.decode_sequence feeds the prenet's last position over [SOS] (i = 0) or target[:, :i] (no SOS in front)."""
    from unast_amd import rnn
    fx = _fixture(attn)
    tm, _, _ = _models(attn)
    text, _, _, _ = _batch(attn)
    dev = _dev()
    B, T = text.shape
    with torch.no_grad():
        P = tm._pack()
        bufs = rnn.window_bufs(P, B, dev)
        got = torch.stack([rnn.text_prenet_last(P, text.contiguous(), torch.tensor([i], dtype=torch.int64, device=dev), True, bufs).clone() for i in range(T)])
    rep = []
    assert _close(fx, "text_forward_prenet", got, rep), rep


@pytest.mark.parametrize("attn", TRAJ_ATTNS)
def test_greedy_trajectories_equal_the_references(attn):
    """infer_sequence at max_len 16 (text; 2 x SYNC_EVERY, so the replayed path runs) and 24 (speech) with the fixture's scaled weights: tokens and
    lengths exactly (the generator asserts every decision's margin), frames and stop logits within 16 x the reference's own fp32-vs-fp64 error.

    Measured on an MI355X: lsa `pre` 4.6, `post` 4.7, stop logits 6.9 x e32; luong 1.1, 1.1, 1.2 x e32.  The path keeps fp32-level products for this: unast_rnn_linear in the step, the
    three-launch split form around the GEMMs and convs (with three-term split-bf16 products alone the frames sat at 51-66 x e32)."""
    fx = _fixture(attn, "traj")
    meta = rnn_weights.meta_of(fx)
    tm, sm, model = _models(attn, "traj")
    text, text_len, mel, mel_len = _batch(attn)
    with torch.no_grad():
        t_eo, t_mask = tm.encode(text, text_len)
        s_eo, s_mask = sm.encode(mel, mel_len)
        tokens, tok_lens = tm.infer_sequence(s_eo, s_mask, max_len=meta["max_text"])
        pre, post, stop, stop_lens = sm.infer_sequence(t_eo, t_mask, max_len=meta["max_speech"])
    print("tokens", tokens.tolist(), tok_lens.tolist(), stop_lens.tolist())
    assert np.array_equal(tok_lens.cpu().numpy(), fx["text_lens"]) and np.array_equal(tokens.cpu().numpy(), fx["tokens"])
    assert np.array_equal(stop_lens.cpu().numpy(), fx["stop_lens"])
    errs = {}
    for name, got in (("pre", pre), ("post", post), ("stop", stop)):
        errs[name] = np.abs(got.cpu().double().numpy() - fx[name]).max() / float(fx["e32/" + name])
        print("%-5s err = %.3g x e32 (e32 = %.3g)" % (name, errs[name], float(fx["e32/" + name])))
    assert max(errs.values()) <= 16, errs


def test_five_consecutive_lsa_weight_vectors():
    """Attention weights of the speech auto-encoder's first five teacher-forced decoder steps (Tk = 40 > the conv's 31 taps)."""
    from unast_amd import rnn
    fx = _fixture("lsa")
    _, sm, _ = _models("lsa")
    _, _, mel, mel_len = _batch("lsa")
    with torch.no_grad():
        enc_outputs, mask = sm.encode(mel, mel_len)
        g = rnn.speech_generation(sm._pack(), enc_outputs, mel_len.to(_dev(), torch.int32), mel.shape[1], target=mel)
        got = []
        for _ in range(5):
            g.step(None)
            got.append(g.core.prev.clone())
    rep = []
    assert _close(fx, "lsa_weights", torch.stack(got), rep), rep


@pytest.mark.parametrize("attn", ATTNS)
def test_replayed_decoding_equals_the_eager_one_to_the_bit(attn, monkeypatch):
    from unast_amd import config
    tm, sm, model = _models(attn)
    text, text_len, mel, mel_len = _batch(attn)
    res = {}
    for graph in (True, False):
        monkeypatch.setattr(config, "DECODE_GRAPH", graph)
        with torch.no_grad():
            s_eo, s_mask = sm.encode(mel, mel_len)
            t_eo, t_mask = tm.encode(text, text_len)
            res[graph] = list(sm.decode_sequence(mel, mel_len, t_eo, t_mask)[:3]) + list(tm.infer_sequence(s_eo, s_mask, max_len=16)) \
                + list(sm.infer_sequence(t_eo, t_mask, max_len=24))
    for a, b in zip(res[True], res[False]):
        assert a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize("attn", ATTNS)
def test_unast_tts_and_asr_equal_the_direct_calls(attn):
    tm, sm, model = _models(attn)
    text, text_len, mel, mel_len = _batch(attn)
    with torch.no_grad():
        t_eo, t_mask = tm.encode(text, text_len)
        s_eo, s_mask = sm.encode(mel, mel_len)
        for infer in (False, True):
            got = model.tts(text, text_len, mel, mel_len, infer=infer)
            want = sm.infer_sequence(t_eo, t_mask) if infer else sm.decode_sequence(mel, mel_len, t_eo, t_mask)
            for a, b in zip(got, want):
                assert torch.equal(a, b) if torch.is_tensor(a) else a is b
            got = model.asr(text, text_len, mel, mel_len, infer=infer)
            want = tm.infer_sequence(s_eo, s_mask) if infer else tm.decode_sequence(text, text_len, s_eo, s_mask)
            if infer:
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            else:
                assert torch.equal(got, want)


def test_single_step_decode_matches_the_first_teacher_forced_step():
    """TextRNN.decode / SpeechRNN.decode on the step-0 inputs give position 0 of decode_sequence."""
    tm, sm, model = _models("luong")
    text, text_len, mel, mel_len = _batch("luong")
    with torch.no_grad():
        (hc, eo), mask = tm.encode(text, text_len)
        sos = torch.full((text.shape[0], 1), 1, dtype=torch.int64, device=_dev())
        logits, (h, c) = tm.decode(sos, hc, eo, mask)
        full = tm.decode_sequence(text, text_len, (hc, eo), mask)
        assert torch.equal(logits[:, 0], full[:, 0]) and h.shape == hc[0].shape
        (frame, stop), _ = sm.decode(torch.zeros(mel.shape[0], 1, mel.shape[2], device=_dev()), hc, eo, mask)
        pre, _, stops, _ = sm.decode_sequence(mel, mel_len, (hc, eo), mask)
        assert torch.equal(frame[:, 0], pre[:, 0]) and torch.equal(stop[:, 0, 0], stops[:, 0])


def test_a_second_call_follows_an_in_place_weight_edit():
    """The kernels read derived copies (folded BatchNorm, fragment-ordered W_hh, the joined head): they must refresh when a weight moves."""
    from unast_amd.network import TextRNN
    fx = _fixture("luong")
    t_sd, _ = rnn_weights.fixture_state_dicts(fx)
    tm = TextRNN(rnn_weights.rnn_args("luong"))
    tm.load_state_dict(t_sd)
    tm = tm.to(_dev()).eval()
    text, text_len, _, _ = _batch("luong")
    with torch.no_grad():
        a = tm(text, text_len).clone()
        tm.encoder.rnn.weight_hh_l0.mul_(0.5)
        tm.prenet.batch_norm1.running_var.mul_(2.0)
        b = tm(text, text_len).clone()
        tm.encoder.rnn.weight_hh_l0.mul_(2.0)
        tm.prenet.batch_norm1.running_var.mul_(0.5)
        c = tm(text, text_len)
    assert not torch.equal(a, b) and (a - b).abs().max().item() > 1e-4
    assert torch.equal(a, c)


def test_token_ids_outside_the_embedding_table_are_refused():
    """The window kernel indexes the embedding table with the given ids; a teacher-forced target or a decode() prefix out of range is an error."""
    tm, _, _ = _models("luong")
    text, text_len, _, _ = _batch("luong")
    vocab = tm.prenet.embed.weight.shape[0]
    with torch.no_grad():
        enc_outputs, mask = tm.encode(text, text_len)
        for bad in (vocab, -1):
            t = text.clone()
            t[1, 3] = bad
            with pytest.raises(ValueError, match="token ids"):
                tm.decode_sequence(t, text_len, enc_outputs, mask)
            with pytest.raises(ValueError, match="token ids"):
                tm.decode(t[:, :5], enc_outputs[0], enc_outputs[1], mask)


def test_a_sequence_call_resets_the_stand_alone_lsa_state():
    """decode() continues from the previous decode()'s attention weights; decode_sequence / infer_sequence end that, as the reference's clear_memory does."""
    _, sm, _ = _models("lsa")
    _, _, mel, mel_len = _batch("lsa")
    with torch.no_grad():
        (hc, eo), mask = sm.encode(mel, mel_len)
        go = torch.zeros(mel.shape[0], 1, mel.shape[2], device=_dev())
        sm.clear_memory()
        (first, _), _ = sm.decode(go, hc, eo, mask)
        (second, _), _ = sm.decode(go, hc, eo, mask)            # same inputs, but prev / cum moved
        assert not torch.equal(first, second)
        sm.decode_sequence(mel, mel_len, (hc, eo), mask)
        (again, _), _ = sm.decode(go, hc, eo, mask)
        assert torch.equal(first, again)
        sm.decode(go, hc, eo, mask)
        sm.infer_sequence((hc, eo), mask, max_len=2)
        (again, _), _ = sm.decode(go, hc, eo, mask)
        assert torch.equal(first, again)
        sm.clear_memory()
