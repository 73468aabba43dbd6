#!/usr/bin/env python3
"""Golden vectors of SpeechRNN's teacher-forced train-mode decoder and its backward (decode_sequence / forward under model.train(),
src/network.py:352-402) -- the fixtures of unast_amd.train_rnn.decoder_forward / decoder_backward.

Runs ONLY in the build container: imports the reference (tools/gen_golden.import_reference), loads seeded weights by name
(tests/rnn_weights.py), sets every dropout probability to 0 (batch-statistics BatchNorm stays on), and runs on the CPU in fp64 and once
more in fp32, per attention type, two cases of L = <pre, R1> + <post, R2> + <stop, R3>:

  a   the decoder alone over a text-shaped memory: B = 3, T = 9, Tk = 12, lens_k (12, 1, 7), random enc_output with zero rows past
      lens_k and random (h, c) (tests/rnn_decoder_mirror.memory), all three with requires_grad;
  b   the autoencoder, SpeechRNN.forward's encode + decode_sequence on B = 3, T_mel = 10, lengths (10, 1, 6): every gradient including the
      shared prenet's, and d_mel through the encoder (the teacher-forcing frames enter detached: they are data).

Writes data-only fixtures tests/golden/rnn_decoder_train_{luong,lsa}.npz: inputs, lengths, seeds; per case pre / post / stop, the
post-net's running statistics after the call, d_h, d_c, strided samples of d_enc_output (and d_mel); per parameter the gradient's L2 norm
and a strided sample of at most 2048 elements (tests/rnn_train_mirror.sample; case b keeps every second element of that sample for the
decoder's parameters and the shared prenet, and norms only for the encoder's, whose mirror tests/golden/rnn_encoder_train.npz pins -- two
full sets would not fit the size limit); `e32/...` = the fp32 run's error
against the fp64 run (max |.| for forward tensors, relative L2 norm for gradients).

Weights are not stored: key names, shapes and the seed are.  Usage: python tools/gen_golden_rnn_decoder_train.py [--out tests/golden]
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
from tests import rnn_weights, rnn_train_mirror as TM, rnn_decoder_mirror as DM  # noqa: E402
from unast_amd.portable import synth_batch  # noqa: E402

B = 3
T_A, TK_A, LENS_K_A = 9, 12, (12, 1, 7)
T_B, LENS_B = 10, (10, 1, 6)
SEED, COT_SEED, MEM_SEED = 1234, 4321, 97
MAX_BYTES = 900000           # what tools/gen_golden_rnn_encoder_train.py asserts of its fixture


def inputs():
    _, mel, _, _ = synth_batch(B, 12, T_B, seed=5)
    mel_b = mel[:, :T_B].copy()
    for b in range(B):
        mel_b[b, LENS_B[b]:] = 0.0
    _, mel2, _, _ = synth_batch(B, 12, T_A, seed=6)
    enc, h, c = DM.memory(MEM_SEED, B, TK_A, LENS_K_A)
    return dict(a_target=mel2[:, :T_A].copy(), a_enc_output=enc, a_h=h, a_c=c, a_lens_k=np.array(LENS_K_A, np.int64),
                b_mel=mel_b, b_mel_len=np.array(LENS_B, np.int64))


def model_of(network, attn, dtype):
    cfg = json.load(open(os.path.join(REF_SRC, "configs", "rnn_d_%s.json" % attn)))
    args = SimpleNamespace(**cfg)
    args.s_pre_drop = args.s_post_drop = args.e_drop = args.d_drop = 0.0
    m = network.SpeechRNN(args)
    sd = m.state_dict()
    keys, shapes = list(sd.keys()), [list(v.shape) for v in sd.values()]
    new = rnn_weights.state_dict("speech", keys, shapes, SEED, [])
    m.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in new.items()})
    return m.train(), keys, shapes


def collect(m, pre, post, stop, extra):
    o = {"pre": pre.detach(), "post": post.detach(), "stop": stop.detach()}
    o.update({k: v.detach() for k, v in extra.items()})
    for k, v in m.state_dict().items():
        if k.startswith("postnet.") and k.endswith(("running_mean", "running_var")):
            o[k] = v.detach().clone()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    return o, grads


def run(network, attn, dtype, inp):
    torch.set_default_dtype(dtype)
    out = {}
    t = lambda a: torch.from_numpy(a).to(dtype)                                                  # noqa: E731
    # case a: the decoder alone
    m, keys, shapes = model_of(network, attn, dtype)
    enc, h, c = (t(inp[k]).requires_grad_(True) for k in ("a_enc_output", "a_h", "a_c"))
    lens_k = torch.from_numpy(inp["a_lens_k"])
    mask = torch.arange(TK_A)[None, :] >= lens_k[:, None]
    target = t(inp["a_target"])
    pre, post, stop, _ = m.decode_sequence(target, None, ((h, c), enc), mask)
    r1, r2, r3 = (x.to(dtype) for x in DM.cotangents(COT_SEED, B, T_A, target.shape[2]))
    ((pre * r1).sum() + (post * r2).sum() + (stop * r3).sum()).backward()
    out["a"] = collect(m, pre, post, stop, dict(d_enc_output=enc.grad, d_h=h.grad, d_c=c.grad))
    assert sorted(out["a"][1]) == sorted(DM.trained_keys(m.state_dict()))
    assert all(float(enc.grad[b, int(lens_k[b]):].abs().max()) == 0.0 for b in range(B) if int(lens_k[b]) < TK_A)
    # case b: encode + decode_sequence (SpeechRNN.forward with the teacher-forcing frames as data)
    m, _, _ = model_of(network, attn, dtype)
    mel = t(inp["b_mel"]).requires_grad_(True)
    mel_len = torch.from_numpy(inp["b_mel_len"])
    enc_outputs, pad_mask = m.encode(mel, mel_len)
    pre, post, stop, _ = m.decode_sequence(mel.detach(), mel_len, enc_outputs, pad_mask)
    r1, r2, r3 = (x.to(dtype) for x in DM.cotangents(COT_SEED + 1, B, T_B, mel.shape[2]))
    ((pre * r1).sum() + (post * r2).sum() + (stop * r3).sum()).backward()
    (hh, cc), eo = enc_outputs
    out["b"] = collect(m, pre, post, stop, dict(d_mel=mel.grad, enc_output=eo, h=hh, c=cc))
    torch.set_default_dtype(torch.float32)
    return out, dict(speech_keys=keys, speech_shapes=shapes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    _, network, _, _ = import_reference()
    inp = inputs()
    for attn in ("luong", "lsa"):
        r64, spec = run(network, attn, torch.float64, inp)
        r32, _ = run(network, attn, torch.float32, inp)
        arrs = dict(inp)
        for case in ("a", "b"):
            (o64, g64), (o32, g32) = r64[case], r32[case]
            for k, v in o64.items():
                full = v.double().numpy()
                arrs["%s/%s" % (case, k)] = TM.sample(full) if k in ("d_enc_output", "d_mel", "enc_output") else full
                arrs["e32/%s/%s" % (case, k)] = np.float64(np.abs(o32[k].double().numpy() - full).max())
                arrs["max/%s/%s" % (case, k)] = np.float64(np.abs(full).max())
            for k in ("d_enc_output", "d_h", "d_c", "d_mel"):
                if k in o64:
                    arrs["e32/%s/rel/%s" % (case, k)] = np.float64(TM.normerr(o32[k], o64[k]))
            for k, g in g64.items():
                arrs["%s/gnorm/%s" % (case, k)] = np.float64(g.double().norm().item())
                if case == "a":
                    arrs["a/gsample/%s" % k] = TM.sample(g.double().numpy())
                elif not k.startswith("encoder."):
                    arrs["b/gsample/%s" % k] = TM.sample(g.double().numpy())[::2]
                arrs["e32/%s/grad/%s" % (case, k)] = np.float64(TM.normerr(g32[k], g))
                print("  %-5s %s %-62s |g| %.4g  e32 %.3g" % (attn, case, k, arrs["%s/gnorm/%s" % (case, k)], arrs["e32/%s/grad/%s" % (case, k)]))
        arrs["meta"] = np.array(json.dumps(dict(spec, seed=SEED, gains=[], cot_seed=COT_SEED, attn=attn)))
        path = os.path.join(a.out, "rnn_decoder_train_%s.npz" % attn)
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        assert size <= MAX_BYTES, (path, size)
        print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
