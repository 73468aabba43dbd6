#!/usr/bin/env python3
"""Golden vectors of the RNN family's cross-model (back-translation) sub-step (src/train.py:261-294, 418-444; UNAST.cm_speech_in / cm_text_in,
src/network.py:103-123; train-mode infer_sequence, src/network.py:312-349, 586-617): the fixtures of unast_amd.train_rnn_step.train_cm_step.

Runs ONLY in the build container: imports the reference (tools/gen_golden.import_reference), builds UNAST(TextRNN, SpeechRNN, LSTMDiscriminator)
from the reference's rnn_d_{luong,lsa} config, loads seeded weights by name with 5h's trajectory gains (tests/rnn_cm_mirror.state_dict: stop
bias, EOS bias, scaled recurrent / attention / head weights, so that greedy decisions have margins), sets every dropout probability to 0,
patches torch.randperm to the identity and infer_sequence's default max_len to small values, and runs on the CPU in fp64 and once more in fp32,
with accum_steps = 1, grad_clip = 1.0 and torch.optim.AdamW at the config's lr and weight_decay, the reference's own entry points:

    freeze(D); train_cm_step; optimizer_step

per attention type on three cases (tests/rnn_cm_mirror.CM_FIXTURE):

  a      B = 3, T_text = 7, T_mel = 12, max_len 7 (text) / 12 (speech): generated lengths that differ, one EOS at position 1, one sequence stopped
         while another runs on;
  b      B = 2, T_text = 6, T_mel = 10, max_len 6 / 10: one sequence never stops;
  a_eps  case a with eps = 0.1 on the text prenet's three BatchNorms (the conditioned twin).

It ASSERTS: every argmax top-2 gap and every stop margin of a live decision >= 1e-2 of the largest logit (tools/gen_golden_rnn.py's thresholds),
that the fp32 and fp64 runs agree on every token and length, and that no PAD id lies inside a generated sentence's length.

Writes data-only fixtures tests/golden/rnn_cm_{luong,lsa}.npz: inputs; per case the generated tokens, frames (post-net output), stop logits and
lengths; the three losses; the names of the parameters that have a gradient (the reference leaves the others None), each one's L2 norm and a
strided sample of at most 128 elements; a strided sample of at most 32 elements of every parameter and BatchNorm buffer after the step
(num_batches_tracked whole) and of the running statistics after the sub-step; `e32/...` = the fp32 run's error against the fp64 run.
Weights are not stored: key names, shapes, seed and gains are.  Usage: python tools/gen_golden_rnn_cm.py [--out tests/golden]
"""
import argparse
import json
import os
import sys
from collections import defaultdict
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from gen_golden import import_reference, REF_SRC  # noqa: E402
from gen_golden_rnn_step import sample, pack, normerr  # noqa: E402
from tests import rnn_cm_mirror as CM  # noqa: E402

EPS_COND = 0.1
G_SAMPLE, P_SAMPLE = 128, 32
MAX_BYTES = 900000
LOSS_KEYS = ("s_cm", "t_cm", "d_cm")
MARGIN = 1e-2


def make_args(attn):
    cfg = json.load(open(os.path.join(REF_SRC, "configs", "rnn_d_%s.json" % attn)))
    args = SimpleNamespace(**cfg)
    args.t_pre_drop = args.t_post_drop = args.s_pre_drop = args.s_post_drop = args.e_drop = args.d_drop = 0.0
    args.load_path = None
    args.ae_steps, args.sp_steps, args.cm_steps, args.d_steps = 0, 0, 1, 0
    args.grad_clip = 1.0
    assert args.optim_type == "adamw" and args.use_discriminator
    return args


def run(mods, attn, case, dtype, inputs):
    module, network, utils, train = mods
    fx = CM.CM_FIXTURE[attn]["a" if case == "a_eps" else case]
    torch.set_default_dtype(dtype)
    train.DEVICE = torch.device("cpu")
    train.WRITER = None
    real_randperm = torch.randperm
    torch.randperm = lambda n, *a, **k: torch.arange(n)
    t_def, s_def = network.TextRNN.infer_sequence.__defaults__, network.SpeechRNN.infer_sequence.__defaults__
    network.TextRNN.infer_sequence.__defaults__ = (fx["max_text"],)
    network.SpeechRNN.infer_sequence.__defaults__ = (fx["max_speech"],)
    try:
        args = make_args(attn)
        _, _, model, optimizer, _ = train.initialize_model(args)
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
            if isinstance(m, torch.nn.LSTM):
                m.dropout = 0.0
        sd = model.state_dict()
        keys, shapes = list(sd.keys()), [list(v.shape) for v in sd.values()]
        new = CM.fixture_state_dict(attn, case, keys, shapes)
        model.load_state_dict({k: v.to(dtype if sd[k].is_floating_point() else sd[k].dtype) for k, v in new.items()})
        if case == "a_eps":
            for bn in (model.text_m.prenet.batch_norm1, model.text_m.prenet.batch_norm2, model.text_m.prenet.batch_norm3):
                bn.eps = EPS_COND
        model.train()
        text, mel, tl, ml = inputs
        batch = (text, mel.to(dtype), torch.tensor(tl), torch.tensor(ml))
        # what the two generations decided and returned
        gen = dict(logits=[], stops=[])
        t_dec, s_dec, t_inf, s_inf = model.text_m.decode, model.speech_m.decode, model.text_m.infer_sequence, model.speech_m.infer_sequence
        live = dict(t=False, s=False)

        def t_wrap(*a):
            o, h = t_dec(*a)
            if live["t"]:
                gen["logits"].append(o[:, 0].detach().clone())
            return o, h

        def s_wrap(*a):
            (o, s), h = s_dec(*a)
            if live["s"]:
                gen["stops"].append(s[:, 0, 0].detach().clone())
            return (o, s), h

        def t_infer(*a, **k):
            live["t"] = True
            r = t_inf(*a, **k)
            live["t"] = False
            gen["tokens"], gen["text_lens"] = r[0].detach().clone(), r[1].detach().clone()
            return r

        def s_infer(*a, **k):
            live["s"] = True
            r = s_inf(*a, **k)
            live["s"] = False
            gen["pre"], gen["post"], gen["stop"], gen["speech_lens"] = (x.detach().clone() for x in r)
            return r
        model.text_m.decode, model.speech_m.decode, model.text_m.infer_sequence, model.speech_m.infer_sequence = t_wrap, s_wrap, t_infer, s_infer
        losses = defaultdict(list)
        train.freeze_model_parameters(model.discriminator)
        train.train_cm_step(losses, model, batch, 0, 1, args)
        out = dict(gen=gen)
        out["sub_state"] = {k: v.detach().clone() for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
        out["grads"] = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        out["norm"] = float(torch.nn.utils.clip_grad_norm_(model.parameters(), 1e30))
        train.optimizer_step(model, optimizer, args)
        out["state"] = {k: v.detach().clone() for k, v in model.state_dict().items()}
        out["losses"] = {k: float(losses[k][0]) for k in LOSS_KEYS}
        # the margins of every live decision
        lg, sl = torch.stack(gen["logits"], 1).double(), torch.stack(gen["stops"], 1).double()
        top2 = lg.topk(2, dim=-1).values
        live_t = torch.arange(lg.shape[1])[None, :] < gen["text_lens"][:, None]
        live_s = torch.arange(sl.shape[1])[None, :] < gen["speech_lens"][:, None]
        out["gap"] = ((top2[..., 0] - top2[..., 1])[live_t]).min().item() / lg.abs().max().item()
        out["stop_margin"] = sl.abs()[live_s].min().item() / sl.abs().max().item()
        out["live_pad"] = int(((gen["tokens"] == 0) & live_t[:, :gen["tokens"].shape[1]]).sum())
        return out, dict(keys=keys, shapes=shapes, lr=args.lr, weight_decay=args.weight_decay)
    finally:
        torch.randperm = real_randperm
        network.TextRNN.infer_sequence.__defaults__, network.SpeechRNN.infer_sequence.__defaults__ = t_def, s_def
        torch.set_default_dtype(torch.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--attn", default="luong,lsa")
    a = ap.parse_args()
    mods = import_reference()
    for attn in a.attn.split(","):
        arrs, spec = {}, None
        for case in ("a", "b", "a_eps"):
            fx = CM.CM_FIXTURE[attn]["a" if case == "a_eps" else case]
            inputs = CM.fixture_batch(fx)                                                        # drawn under the float32 default dtype, as the tests draw it
            r64, spec = run(mods, attn, case, torch.float64, inputs)
            r32, _ = run(mods, attn, case, torch.float32, inputs)
            g64, g32 = r64["gen"], r32["gen"]
            tl, sl = g64["text_lens"].tolist(), g64["speech_lens"].tolist()
            print("%s %s: text lens %s gap %.3g live PAD %d; speech lens %s stop margin %.3g; losses %s" % (attn, case, tl, r64["gap"], r64["live_pad"], sl,
                                                                                                        r64["stop_margin"], r64["losses"]))
            assert r64["gap"] >= MARGIN and r64["stop_margin"] >= MARGIN and r32["gap"] >= MARGIN and r32["stop_margin"] >= MARGIN, (attn, case)
            assert r64["live_pad"] == 0, "a PAD id inside a generated sentence"
            for k in ("tokens", "text_lens", "speech_lens"):
                assert torch.equal(g64[k], g32[k]), (attn, case, k)                                  # the fp32 reference run decides identically
            if case == "a":
                assert len(set(tl)) > 1 and 1 in tl and len(set(sl)) > 1, (tl, sl)
            elif case == "b":
                assert fx["max_text"] in tl and min(tl) < fx["max_text"] and fx["max_speech"] in sl and min(sl) < fx["max_speech"], (tl, sl)
            for k in ("tokens", "text_lens", "speech_lens"):
                arrs["%s/gen/%s" % (case, k)] = g64[k].numpy().astype(np.int64)
            for k in ("pre", "post", "stop"):
                arrs["%s/gen/%s" % (case, k)] = g64[k].numpy()
                arrs["e32/%s/gen/%s" % (case, k)] = np.float64((g32[k].double() - g64[k]).abs().max().item())
            for k in LOSS_KEYS:
                arrs["%s/loss/%s" % (case, k)] = np.float64(r64["losses"][k])
                arrs["e32/%s/loss/%s" % (case, k)] = np.float64(abs(r32["losses"][k] - r64["losses"][k]))
            arrs["%s/norm" % case] = np.float64(r64["norm"])
            assert sorted(r64["grads"]) == sorted(r32["grads"])
            gkeys = list(r64["grads"])
            pack(arrs, "%s/g" % case, gkeys, [sample(r64["grads"][k].numpy(), G_SAMPLE) for k in gkeys])
            arrs["%s/gnorm" % case] = np.array([r64["grads"][k].norm().item() for k in gkeys])
            arrs["e32/%s/grad" % case] = np.array([normerr(r32["grads"][k], r64["grads"][k]) for k in gkeys])
            st, s32 = r64["state"], r32["state"]
            nbt = {k: int(v) for k, v in st.items() if k.endswith("num_batches_tracked")}
            skeys = [k for k in st if k not in nbt]
            pack(arrs, "%s/state" % case, skeys, [sample(st[k].numpy(), P_SAMPLE) for k in skeys])
            arrs["e32/%s/state" % case] = np.array([np.abs(sample(s32[k].double().numpy(), P_SAMPLE) - sample(st[k].numpy(), P_SAMPLE)).max() for k in skeys])
            arrs["%s/num_batches_tracked" % case] = np.array(json.dumps(nbt))
            rkeys = [k for k in r64["sub_state"] if not k.endswith("num_batches_tracked")]
            pack(arrs, "%s/running" % case, rkeys, [sample(r64["sub_state"][k].numpy(), P_SAMPLE) for k in rkeys])
            arrs["e32/%s/running" % case] = np.array([np.abs(sample(r32["sub_state"][k].double().numpy(), P_SAMPLE) - sample(r64["sub_state"][k].numpy(), P_SAMPLE)).max()
                                                     for k in rkeys])
            arrs["%s/margins" % case] = np.array([r64["gap"], r64["stop_margin"]])
        arrs["meta"] = np.array(json.dumps(dict(keys=spec["keys"], shapes=spec["shapes"], attn=attn, eps_cond=EPS_COND, lr=spec["lr"], weight_decay=spec["weight_decay"],
                                                accum_steps=1, grad_clip=1.0, g_sample=G_SAMPLE, p_sample=P_SAMPLE, setups=CM.CM_FIXTURE[attn])))
        path = os.path.join(a.out, "rnn_cm_%s.npz" % attn)
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        assert size <= MAX_BYTES, (path, size)
        print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
