#!/usr/bin/env python3
"""Golden vectors of the RNN model family's eval path (TextRNN / SpeechRNN, src/network.py:279-402, 503-624).

Runs ONLY in the build container: imports the reference (tools/gen_golden.import_reference), loads seeded weights by name
(tests/rnn_weights.py), runs the reference's own methods on the CPU in fp64 and once more in fp32, and writes data-only fixtures:

  tests/golden/rnn_values_<attn>.npz   plain portable weights: encoders, teacher-forced forward / tts / asr, the text-prenet last-position
                                       rows of prefix lengths 1..9 in both prefix conventions, the prenet rows the teacher-forced text steps feed, five consecutive LSA weight vectors
  tests/golden/rnn_traj_<attn>.npz     scaled weights (meta 'gains'): infer_sequence at max_len 16 (text) / 24 (speech)

Each output tensor `x` comes with `e32/x` = max |fp32 run - fp64 run|.  Weights are not stored: key names, shapes, seed and gains are.
Usage: python tools/gen_golden_rnn.py [--out tests/golden]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from gen_golden import import_reference, REF_SRC  # noqa: E402
from tests import rnn_weights  # noqa: E402
from unast_amd.portable import synth_batch  # noqa: E402

B, T_TEXT, T_MEL = 3, 12, 40
TEXT_LEN, MEL_LEN = (12, 7, 1), (40, 33, 1)
TRAJ_GAINS = [[".rnn.weight_", "scale", 5.0], ["attention_layer", "scale", 5.0], ["linear_projection.linear_layer.weight", "scale", 5.0],
              ["embed.weight", "scale", 5.0], ["text_m.postnet.fc1.weight", "scale", 40.0], ["stop_linear.weight", "scale", 12.0],
              ["stop_linear.bias", "fill", -0.5], ["linear_project.weight", "scale", 4.0]]
MAX_TEXT, MAX_SPEECH = 16, 24


def batch():
    text, mel, _, _ = synth_batch(B, T_TEXT, T_MEL, seed=5)
    text_len, mel_len = np.array(TEXT_LEN, np.int64), np.array(MEL_LEN, np.int64)
    for b in range(B):
        text[b, text_len[b] - 1] = 2
        text[b, text_len[b]:] = 0
        mel[b, mel_len[b]:] = 0.0
    return text, mel, text_len, mel_len


def build(network, attn, dtype, seed, gains):
    cfg = json.load(open(os.path.join(REF_SRC, "configs", "rnn_d_lsa.json")))
    args = SimpleNamespace(**cfg)
    args.d_attn = attn
    torch.set_default_dtype(dtype)                      # LSA's init_memory creates default-dtype tensors
    tm, sm = network.TextRNN(args), network.SpeechRNN(args)
    spec = {}
    for side, m in (("text", tm), ("speech", sm)):
        sd = m.state_dict()
        keys, shapes = list(sd.keys()), [list(v.shape) for v in sd.values()]
        new = rnn_weights.state_dict(side, keys, shapes, seed, gains)
        m.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in new.items()})
        m.eval()
        spec[side + "_keys"], spec[side + "_shapes"] = keys, shapes
    return tm, sm, network.UNAST(tm, sm), spec


def run_values(network, attn, dtype, seed, inputs):
    tm, sm, model, spec = build(network, attn, dtype, seed, [])
    text, mel, text_len, mel_len = (torch.from_numpy(inputs[k]) for k in ("text", "mel", "text_len", "mel_len"))
    mel = mel.to(dtype)
    out = {}
    lsa_w = []
    if attn == "lsa":
        def grab(mod, inp, res):
            if grab.on and len(lsa_w) < 5:
                lsa_w.append(mod.attention_weights.detach().clone())
        grab.on = False
        sm.decoder.attention_layer.register_forward_hook(grab)
    with torch.no_grad():
        (hc, eo), _ = tm.encode(text, text_len)
        out["text_enc_out"], out["text_h"], out["text_c"] = eo, hc[0], hc[1]
        (hc, eo), _ = sm.encode(mel, mel_len)
        out["speech_enc_out"], out["speech_h"], out["speech_c"] = eo, hc[0], hc[1]
        rows = []
        hook = tm.prenet.register_forward_hook(lambda mod, inp, res: rows.append(res[:, -1].detach().clone()))   # TextRNN.decode's prenet rows
        out["text_forward"] = tm.forward(text, text_len)
        hook.remove()
        out["text_forward_prenet"] = torch.stack(rows)                                      # [T, B, 256]: what each teacher-forced step feeds
        if attn == "lsa":
            grab.on = True
        out["speech_forward_pre"], out["speech_forward_post"], out["speech_forward_stop"] = sm.forward(mel, mel_len)
        if attn == "lsa":
            grab.on = False
            out["lsa_weights"] = torch.stack(lsa_w)                                      # speech auto-encoder (Tk = 40), decoder steps 0..4
        out["tts_pre"], out["tts_post"], out["tts_stop"], _ = model.tts(text, text_len, mel, mel_len, infer=False)
        out["asr"] = model.asr(text, text_len, mel, mel_len, infer=False)
        sos = torch.full((B, 1), 1, dtype=torch.long)
        out["prenet_infer"] = torch.stack([tm.prenet(torch.cat([sos, text[:, :L - 1]], dim=1))[:, -1] for L in range(1, 10)])
        out["prenet_tf"] = torch.stack([tm.prenet(text[:, :L])[:, -1] for L in range(1, 10)])
    return {k: v.double().numpy() for k, v in out.items()}, spec


def run_traj(network, attn, dtype, seed, gains, inputs, eos_bias=None):
    tm, sm, model, spec = build(network, attn, dtype, seed, gains + ([["text_m.postnet.fc1.bias", "eos", eos_bias]] if eos_bias is not None else []))
    text, mel, text_len, mel_len = (torch.from_numpy(inputs[k]) for k in ("text", "mel", "text_len", "mel_len"))
    mel = mel.to(dtype)
    logits, stops = [], []
    t_dec, s_dec = tm.decode, sm.decode

    def t_wrap(*a):
        o, h = t_dec(*a)
        logits.append(o[:, 0].detach().clone())
        return o, h

    def s_wrap(*a):
        (o, s), h = s_dec(*a)
        stops.append(s[:, 0, 0].detach().clone())
        return (o, s), h
    tm.decode, sm.decode = t_wrap, s_wrap
    with torch.no_grad():
        t_eo, t_mask = tm.encode(text, text_len)
        s_eo, s_mask = sm.encode(mel, mel_len)
        tokens, tok_lens = tm.infer_sequence(s_eo, s_mask, max_len=MAX_TEXT)                # asr direction
        pre, post, stop, stop_lens = sm.infer_sequence(t_eo, t_mask, max_len=MAX_SPEECH)   # tts direction
    lg, sl = torch.stack(logits, 1).double(), torch.stack(stops, 1).double()               # [B, steps, V], [B, steps]
    top2 = lg.topk(2, dim=-1).values
    live_t = torch.arange(lg.shape[1])[None, :] < tok_lens[:, None]                        # choices up to and including the EOS
    gap = ((top2[..., 0] - top2[..., 1])[live_t]).min().item() / lg.abs().max().item()
    live_s = torch.arange(sl.shape[1])[None, :] < stop_lens[:, None]
    smargin = sl.abs()[live_s].min().item() / sl.abs().max().item()
    out = dict(tokens=tokens, text_lens=tok_lens, pre=pre, post=post, stop=stop, stop_lens=stop_lens)
    return {k: v.double().numpy() for k, v in out.items()}, spec, dict(gap=gap, stop_margin=smargin)


def save(path, inputs, out64, out32, meta, int_keys=()):
    arrs = dict(inputs)
    for k, v in out64.items():
        arrs[k] = v.astype(np.int64) if k in int_keys else v
        if k not in int_keys:
            arrs["e32/" + k] = np.float64(np.abs(out32[k] - v).max())
    arrs["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    assert size <= 1000000, (path, size)
    print("wrote", path, size, "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    _, network, _, _ = import_reference()
    text, mel, text_len, mel_len = batch()                  # drawn once, under the float32 default dtype
    inputs = dict(text=text, mel=mel, text_len=text_len, mel_len=mel_len)
    for attn in ("luong", "lsa"):
        if "traj" != a.only:
            o64, spec = run_values(network, attn, torch.float64, 1234, inputs)
            o32, _ = run_values(network, attn, torch.float32, 1234, inputs)
            meta = dict(spec, seed=1234, gains=[], attn=attn, attn_dim=32)
            save(os.path.join(a.out, "rnn_values_%s.npz" % attn), inputs, o64, o32, meta)
            for k in o64:
                print("  %-22s max|ref| %.4g  e32 %.3g (%.3g of max)" % (k, np.abs(o64[k]).max(), np.abs(o32[k] - o64[k]).max(),
                                                                        np.abs(o32[k] - o64[k]).max() / max(np.abs(o64[k]).max(), 1e-30)))
        if "values" != a.only:
            seed, gains, eos_bias = TRAJ_SETUP[attn]
            o64, spec, margins = run_traj(network, attn, torch.float64, seed, gains, inputs, eos_bias)
            o32, _, _ = run_traj(network, attn, torch.float32, seed, gains, inputs, eos_bias)
            gains = gains + ([["text_m.postnet.fc1.bias", "eos", eos_bias]] if eos_bias is not None else [])
            ints = ("tokens", "text_lens", "stop_lens")
            print(attn, "text lens", o64["text_lens"], "stop lens", o64["stop_lens"], "tokens", sorted(set(o64["tokens"].astype(int).ravel())), margins)
            tl, sl = o64["text_lens"].astype(int), o64["stop_lens"].astype(int)
            # what tests/test_gpu_rnn_model.py relies on
            assert (tl < MAX_TEXT).any() and (tl == MAX_TEXT).any(), tl
            assert len(set(o64["tokens"].astype(int).ravel())) >= 4
            assert len(set(sl)) > 1 and (sl >= 8).any() and (sl == MAX_SPEECH).any(), sl
            assert margins["gap"] >= 1e-2 and margins["stop_margin"] >= 1e-2, margins
            for k in ints:
                assert np.array_equal(o64[k], o32[k]), k                                   # the fp32 reference run decides identically
            meta = dict(spec, seed=seed, gains=gains, attn=attn, attn_dim=32, max_text=MAX_TEXT, max_speech=MAX_SPEECH, margins=margins)
            save(os.path.join(a.out, "rnn_traj_%s.npz" % attn), inputs, o64, o32, meta, int_keys=ints)
    torch.set_default_dtype(torch.float32)


# (seed, gains, EOS bias) per attention type, found by trying seeds until the asserted conditions hold (the outcome of a greedy decode with
# random weights is a property of the draw).  LSA: portable seed 1236 with the stop bias at -4.  Luong: the same seed with the stop bias at -8 and
# +60 on the EOS logit's bias (without it no Luong draw emits an early EOS).
def _with_stop_bias(v):
    return [[p, op, (v if p == "stop_linear.bias" else val)] for p, op, val in TRAJ_GAINS]


TRAJ_SETUP = {"lsa": (1236, _with_stop_bias(-4.0), None), "luong": (1236, _with_stop_bias(-8.0), 60.0)}

if __name__ == "__main__":
    main()
