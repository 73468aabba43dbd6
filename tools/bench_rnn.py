#!/usr/bin/env python3
"""Times the RNN model family's eval path on the GPU (HIP events, warm-up, medians): unast_lstm_seq_fwd per recurrent step, both encoders,
one decoded position eager and replayed for both models and both attention types, and a whole tts(infer) cut to --frames frames (the text
encoder plus SpeechRNN.infer_sequence(max_len=frames); UNAST.tts itself always decodes up to infer_sequence's default of 815).
Sizes: B = 32, T_text = 180, T_mel = 800.  --train: the encoder-training mode instead -- unast_lstm_seq_fwd_train next to unast_lstm_seq_fwd,
unast_lstm_seq_bwd per recurrent step, and train_rnn.encoder_forward + encoder_backward of both models (dropout and noise on).
Usage: python tools/bench_rnn.py [--reps 7] [--frames 800] [--train]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import rnn_weights  # noqa: E402
from unast_amd import ops, rnn  # noqa: E402
from unast_amd.inference import _capture  # noqa: E402
from unast_amd.network import TextRNN, SpeechRNN  # noqa: E402
from unast_amd.portable import synth_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--frames", type=int, default=800)
ap.add_argument("--train", action="store_true")
a = ap.parse_args()
D = torch.device("cuda:0")
B, TT, TM = 32, 180, 800


def median_ms(fn, reps=a.reps, inner=1):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return statistics.median(out)


def models(attn):
    tm, sm = TextRNN(rnn_weights.rnn_args(attn)), SpeechRNN(rnn_weights.rnn_args(attn))
    for side, m in (("text", tm), ("speech", sm)):
        sd = m.state_dict()
        m.load_state_dict(rnn_weights.state_dict(side, list(sd), [list(v.shape) for v in sd.values()], 1234))
    return tm.to(D).eval(), sm.to(D).eval()


def train_mode():
    from unast_amd import train_rnn
    g = torch.Generator().manual_seed(0)
    for T in (TM, TT):
        xproj = torch.randn(B, T, 2048, generator=g).to(D)
        whh = (torch.randn(2, 1024, 256, generator=g) / 16).to(D)
        wfrag, wfrag_t = ops.lstm_whh_fragments(whh), ops.lstm_whh_fragments_bwd(whh)
        bias = torch.zeros(2048, device=D)
        lens = torch.full((B,), T, dtype=torch.int32, device=D)
        y, hn, cn = torch.empty(B, T, 512, device=D), torch.empty(B, 512, device=D), torch.empty(B, 512, device=D)
        saved, hprev = torch.empty(B, T, 2, 5, 256, device=D), torch.empty(B, T, 512, device=D)
        dy, dfin, dxproj = torch.randn(B, T, 512, generator=g).to(D), torch.randn(B, 512, generator=g).to(D), torch.empty(B, T, 2048, device=D)
        ev = median_ms(lambda: ops.lstm_seq_fwd(xproj, wfrag, bias, bias, lens, y, hn, cn))
        tr = median_ms(lambda: ops.lstm_seq_fwd_train(xproj, wfrag, bias, bias, lens, y, hn, cn, saved, hprev))
        bw = median_ms(lambda: ops.lstm_seq_bwd(dy, wfrag_t, saved, lens, dxproj, dhfinal=dfin, dcfinal=dfin))
        print("B=%d T=%d ndir=2: lstm_seq_fwd %.2f ms (%.2f us/step), lstm_seq_fwd_train %.2f ms (%.2f us/step, x %.3f), lstm_seq_bwd %.2f ms "
              "(%.2f us/step, x %.2f of the forward)" % (B, T, ev, ev * 1e3 / T, tr, tr * 1e3 / T, tr / ev, bw, bw * 1e3 / T, bw / ev))
    text, mel, text_len, mel_len = (torch.from_numpy(x) for x in synth_batch(B, TT, TM, seed=3))
    text, mel = text.to(D), mel.to(D)
    tm, sm = models("luong")
    tm.train(), sm.train()
    for name, m, x, ln, T in (("text", tm, text, text_len, TT), ("speech", sm, mel, mel_len, TM)):
        ln = ln.clone()
        ln[0] = T                                                      # encode's rule: max(lens) == T
        cot = (torch.randn(B, T, 512, device=D), torch.randn(2, B, 256, device=D), torch.randn(2, B, 256, device=D))
        tapes = []
        fw = median_ms(lambda: tapes.append(train_rnn.encoder_forward(m, x, ln, noise_in=True, seed=len(tapes))))

        def both():
            train_rnn.encoder_backward(train_rnn.encoder_forward(m, x, ln, noise_in=True, seed=1), *cot)
        del tapes[:]
        fb = median_ms(both)
        print("%s encoder, B=%d T=%d, dropout and noise on: encoder_forward %.2f ms, encoder_forward + encoder_backward %.2f ms" % (name, B, T, fw, fb))


if a.train:
    train_mode()
    sys.exit(0)

with torch.no_grad():
    # the recurrence alone
    g = torch.Generator().manual_seed(0)
    for T, Bb in ((TM, B), (TT, B), (TM, 16)):
        xproj = torch.randn(Bb, T, 2048, generator=g).to(D)
        wfrag = ops.lstm_whh_fragments((torch.randn(2, 1024, 256, generator=g) / 16).to(D))
        bias = torch.zeros(2048, device=D)
        lens = torch.full((Bb,), T, dtype=torch.int32, device=D)
        y, hn, cn = torch.empty(Bb, T, 512, device=D), torch.empty(Bb, 512, device=D), torch.empty(Bb, 512, device=D)
        ms = median_ms(lambda: ops.lstm_seq_fwd(xproj, wfrag, bias, bias, lens, y, hn, cn))
        print("lstm_seq_fwd B=%d T=%d ndir=2: %.2f ms = %.2f us per recurrent step" % (Bb, T, ms, ms * 1e3 / T))

    text, mel, text_len, mel_len = (torch.from_numpy(x) for x in synth_batch(B, TT, TM, seed=3))
    text, mel = text.to(D), mel.to(D)
    for attn in ("luong", "lsa"):
        tm, sm = models(attn)
        print("[%s] text encoder %.2f ms, speech encoder %.2f ms" % (attn, median_ms(lambda: tm.encode(text, text_len)), median_ms(lambda: sm.encode(mel, mel_len))))
        t_eo, t_mask = tm.encode(text, text_len)
        s_eo, s_mask = sm.encode(mel, mel_len)
        for name, gen in (("text over speech memory", tm.generation(s_eo, s_mask, 300)), ("speech over text memory", sm.generation(t_eo, t_mask, 815))):
            gen.step(None)
            gen.reset()
            eager = median_ms(lambda: gen.step(None), inner=20)
            gen.reset()
            graph = _capture(lambda: gen.step(None))
            gen.reset()
            replay = median_ms(graph.replay, inner=20)
            print("[%s] one decoded position, %s: eager %.3f ms, replayed %.3f ms" % (attn, name, eager, replay))
        sm.postnet.stop_linear.bias.fill_(-30.0)                     # never stops: all frames are decoded

        def tts():                                                   # UNAST.tts(infer=True), whose infer_sequence runs at its default max_len of 815
            t_enc, t_pad = tm.encode(text, text_len)
            out = sm.infer_sequence(t_enc, t_pad, max_len=a.frames)
            assert out[0].shape[1] == a.frames
            return out
        ms = median_ms(tts, reps=3)
        print("[%s] tts: text encoder + infer_sequence of %d frames, B=%d, T_text=%d: %.1f ms" % (attn, a.frames, B, TT, ms))
