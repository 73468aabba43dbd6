#!/usr/bin/env python3
"""Golden vectors of TextRNN's teacher-forced train-mode decoder and its backward (decode_sequence / forward under model.train(),
src/network.py:495-575) -- the fixtures of unast_amd.train_rnn.text_decoder_forward / text_decoder_backward.

Runs ONLY in the build container: imports the reference (tools/gen_golden.import_reference), loads seeded weights by name
(tests/rnn_weights.py), sets every dropout probability to 0 (batch-statistics BatchNorm stays on), and runs on the CPU in fp64 and once
more in fp32, per attention type, three cases of L = <logits, R>:

  a      the decoder alone over a random memory: B = 3, T = 9, Tk = 12, lens_k (12, 1, 7), random enc_output with zero rows past lens_k and
         random (h, c) (tests/rnn_decoder_mirror.memory), all three with requires_grad; PAD tokens in the second half of target row 1;
  a_eps  the same with eps = 0.1 on the three prenet BatchNorms (position 0's prefix is [SOS] in every sequence: zero variance, rstd =
         eps^-1/2; at eps = 1e-5 three gradients are ill-conditioned in fp32 -- see e32 -- and this case is the well-conditioned twin);
  b      the autoencoder, TextRNN.forward's encode + decode_sequence (shared prenet) on B = 3, T = 10, lengths (10, 1, 6).

Writes data-only fixtures tests/golden/text_rnn_decoder_train_{luong,lsa}.npz: inputs, lengths, seeds; per case the logits, the prenet
BatchNorms' running statistics and num_batches_tracked after the call, d_h, d_c, a strided sample of d_enc_output; per parameter the
gradient's L2 norm and a strided sample of at most 2048 elements (tests/rnn_train_mirror.sample; cases a_eps and b keep every second element
of it, and case b norms only for the encoder's parameters, whose mirror tests/golden/rnn_encoder_train.npz pins);
`e32/...` = the fp32 run's error against the fp64 run (max |.| for forward tensors, relative L2 norm for gradients).

Weights are not stored: key names, shapes and the seed are.  Usage: python tools/gen_golden_text_rnn_decoder_train.py [--out tests/golden]
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
from tests import rnn_weights, rnn_train_mirror as TM, text_decoder_mirror as XM  # noqa: E402

B = 3
T_A, TK_A, LENS_K_A = 9, 12, (12, 1, 7)
T_B, LENS_B = 10, (10, 1, 6)
SEED, COT_SEED, MEM_SEED, TOK_SEED = 1234, 4321, 97, 11
EPS_COND = 0.1
MAX_BYTES = 900000           # what tools/gen_golden_rnn_encoder_train.py asserts of its fixture
CASES = ("a", "a_eps", "b")


def inputs():
    enc, h, c = XM.memory(MEM_SEED, B, TK_A, LENS_K_A)
    return dict(a_target=XM.tokens(TOK_SEED, B, T_A, pad_rows=(1,)), a_enc_output=enc, a_h=h, a_c=c, a_lens_k=np.array(LENS_K_A, np.int64),
                b_text=XM.tokens(TOK_SEED + 1, B, T_B, lens=LENS_B), b_text_len=np.array(LENS_B, np.int64))


def model_of(network, attn, dtype, eps=None):
    cfg = json.load(open(os.path.join(REF_SRC, "configs", "rnn_d_%s.json" % attn)))
    args = SimpleNamespace(**cfg)
    args.t_pre_drop = args.t_post_drop = args.e_drop = args.d_drop = 0.0
    m = network.TextRNN(args)
    sd = m.state_dict()
    keys, shapes = list(sd.keys()), [list(v.shape) for v in sd.values()]
    new = rnn_weights.state_dict("text", keys, shapes, SEED, [])
    m.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in new.items()})
    if eps is not None:
        for bn in (m.prenet.batch_norm1, m.prenet.batch_norm2, m.prenet.batch_norm3):
            bn.eps = eps
    return m.train(), keys, shapes


def collect(m, logits, extra):
    o = {"logits": logits.detach()}
    o.update({k: v.detach() for k, v in extra.items()})
    for k, v in m.state_dict().items():
        if k.startswith("prenet.") and k.endswith(XM.BUFFERS):
            o[k] = v.detach().clone()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    return o, grads


def run(network, attn, dtype, inp):
    torch.set_default_dtype(dtype)
    out = {}
    t = lambda a: torch.from_numpy(a).to(dtype)                                                  # noqa: E731
    V = None
    for case, eps in (("a", None), ("a_eps", EPS_COND)):
        m, keys, shapes = model_of(network, attn, dtype, eps)
        enc, h, c = (t(inp[k]).requires_grad_(True) for k in ("a_enc_output", "a_h", "a_c"))
        lens_k = torch.from_numpy(inp["a_lens_k"])
        mask = torch.arange(TK_A)[None, :] >= lens_k[:, None]
        logits = m.decode_sequence(torch.from_numpy(inp["a_target"]), None, ((h, c), enc), mask)
        V = logits.shape[2]
        (logits * XM.cotangent(COT_SEED, B, T_A, V).to(dtype)).sum().backward()
        out[case] = collect(m, logits, dict(d_enc_output=enc.grad, d_h=h.grad, d_c=c.grad))
        assert sorted(out[case][1]) == sorted(XM.trained_keys(m.state_dict()))
        assert all(float(enc.grad[b, int(lens_k[b]):].abs().max()) == 0.0 for b in range(B) if int(lens_k[b]) < TK_A)
    # case b: encode + decode_sequence (TextRNN.forward)
    m, _, _ = model_of(network, attn, dtype)
    text, text_len = torch.from_numpy(inp["b_text"]), torch.from_numpy(inp["b_text_len"])
    enc_outputs, pad_mask = m.encode(text, text_len)
    logits = m.decode_sequence(text, text_len, enc_outputs, pad_mask)
    (logits * XM.cotangent(COT_SEED + 1, B, T_B, V).to(dtype)).sum().backward()
    (hh, cc), eo = enc_outputs
    out["b"] = collect(m, logits, dict(enc_output=eo, h=hh, c=cc))
    torch.set_default_dtype(torch.float32)
    return out, dict(text_keys=keys, text_shapes=shapes)


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
        for case in CASES:
            (o64, g64), (o32, g32) = r64[case], r32[case]
            for k, v in o64.items():
                if k.endswith("num_batches_tracked"):
                    arrs["%s/%s" % (case, k)] = np.int64(int(v))
                    continue
                full = v.double().numpy()
                arrs["%s/%s" % (case, k)] = TM.sample(full) if k in ("d_enc_output", "enc_output") else full
                arrs["e32/%s/%s" % (case, k)] = np.float64(np.abs(o32[k].double().numpy() - full).max())
                arrs["max/%s/%s" % (case, k)] = np.float64(np.abs(full).max())
            for k in ("d_enc_output", "d_h", "d_c"):
                if k in o64:
                    arrs["e32/%s/rel/%s" % (case, k)] = np.float64(TM.normerr(o32[k], o64[k]))
            for k, g in g64.items():
                arrs["%s/gnorm/%s" % (case, k)] = np.float64(g.double().norm().item())
                if case == "a":
                    arrs["a/gsample/%s" % k] = TM.sample(g.double().numpy())
                elif not k.startswith("encoder."):
                    arrs["%s/gsample/%s" % (case, k)] = TM.sample(g.double().numpy())[::2]
                arrs["e32/%s/grad/%s" % (case, k)] = np.float64(TM.normerr(g32[k], g))
                print("  %-5s %-5s %-62s |g| %.4g  e32 %.3g" % (attn, case, k, arrs["%s/gnorm/%s" % (case, k)], arrs["e32/%s/grad/%s" % (case, k)]))
        arrs["meta"] = np.array(json.dumps(dict(spec, seed=SEED, gains=[], cot_seed=COT_SEED, attn=attn, eps_cond=EPS_COND)))
        path = os.path.join(a.out, "text_rnn_decoder_train_%s.npz" % attn)
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        assert size <= MAX_BYTES, (path, size)
        print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
