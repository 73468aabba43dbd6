#!/usr/bin/env python3
"""Golden vectors of the RNN family's train steps (src/train.py:199-259, 296-363, 365-416, 446-463): the fixtures of unast_amd.train_rnn_step.

Runs ONLY in the build container: imports the reference (tools/gen_golden.import_reference), builds UNAST(TextRNN, SpeechRNN,
LSTMDiscriminator(512, 64, bidirectional, 2 layers)) from the reference's rnn_d_{luong,lsa} config, loads seeded weights by name
(unast_amd.portable.portable_tensor), sets every dropout probability to 0, patches noise_fn, specaugment and torch.randperm to the identity,
and runs on the CPU in fp64 and once more in fp32, with accum_steps = 2, grad_clip = 1.0 and torch.optim.AdamW at the config's lr and
weight_decay, the reference's own entry points in this order:

    freeze(D); train_ae_step; train_sp_step; optimizer_step; unfreeze(D); train_discriminator_step; optimizer_step

per attention type on three cases:

  a      B = 3, T_text = 7, T_mel = 12, lengths (7, 3, 5) / (12, 5, 9);
  b      B = 2, T_text = 9, T_mel = 6, lengths (9, 4) / (6, 2): the text rows are the long ones (the gather pads the speech side);
  a_eps  case a with eps = 0.1 on the text prenet's three BatchNorms (the conditioned twin).

Writes data-only fixtures tests/golden/rnn_step_{luong,lsa}.npz: inputs; per case the seven losses, the two pre-clip gradient norms, per
optimizer step ('gen', 'disc') the names of the parameters that have a gradient (the reference leaves the others None), each one's L2 norm
and a strided sample of at most 128 elements, and a strided sample of at most 32 elements of every parameter and BatchNorm buffer after
the step (after 'disc': of those it moved; num_batches_tracked whole), packed per group (see pack);
`e32/...` = the fp32 run's error against the fp64 run (absolute for losses and norms, relative L2 norm for gradients, largest absolute
error over the sample for the post-step state).  Also writes
tests/golden/rnn_configs.json: the hyper-parameters of the reference's RNN configs (settings only).

Weights are not stored: key names, shapes and the seed are.  Usage: python tools/gen_golden_rnn_step.py [--out tests/golden]
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
from unast_amd.portable import portable_tensor  # noqa: E402

SEED = 1234
EPS_COND = 0.1
G_SAMPLE, P_SAMPLE = 128, 32
MAX_BYTES = 900000
CASES = {"a": dict(B=3, Tt=7, Tm=12, tl=(7, 3, 5), ml=(12, 5, 9), tok_seed=21, mel_seed=22),
         "b": dict(B=2, Tt=9, Tm=6, tl=(9, 4), ml=(6, 2), tok_seed=23, mel_seed=24)}
CASES["a_eps"] = CASES["a"]
RNN_CONFIGS = ("rnn_d", "rnn_d_b16", "rnn_d_lsa", "rnn_d_luong", "rnn_d_test", "rnn_lsa", "rnn_luong", "rnn_no_discrim", "rnn_small_no_discrim")
LOSS_KEYS = ("t_ae", "s_ae", "d_ae", "asr_", "tts_", "sp_d", "d")


def sample(v, n):
    flat = np.asarray(v, dtype=np.float64).reshape(-1)
    return flat[::max(1, -(-flat.size // n))]


def pack(arrs, name, keys, vecs):
    """One entry per group instead of one per tensor (an .npz member costs more than a 32-element sample): name/keys (JSON), name/off [n + 1],
    name/data = the samples back to back."""
    arrs[name + "/keys"] = np.array(json.dumps(list(keys)))
    arrs[name + "/off"] = np.cumsum([0] + [len(v) for v in vecs]).astype(np.int64)
    arrs[name + "/data"] = np.concatenate(vecs) if vecs else np.zeros(0)


def inputs(case):
    c = CASES[case]
    text = np.random.RandomState(c["tok_seed"]).randint(3, 46, size=(c["B"], c["Tt"])).astype(np.int64)
    mel = np.random.RandomState(c["mel_seed"]).standard_normal((c["B"], c["Tm"], 80))
    for b in range(c["B"]):
        text[b, c["tl"][b] - 1] = 2                                                               # EOS closes every sequence
        text[b, c["tl"][b]:] = 0
        mel[b, c["ml"][b]:] = 0.0
    return text, mel, np.array(c["tl"], np.int64), np.array(c["ml"], np.int64)


def make_args(attn):
    cfg = json.load(open(os.path.join(REF_SRC, "configs", "rnn_d_%s.json" % attn)))
    args = SimpleNamespace(**cfg)
    args.t_pre_drop = args.t_post_drop = args.s_pre_drop = args.s_post_drop = args.e_drop = args.d_drop = 0.0
    args.load_path = None
    args.ae_steps, args.sp_steps, args.cm_steps, args.d_steps = 1, 1, 0, 1
    args.grad_clip = 1.0
    assert args.optim_type == "adamw" and args.disc_hid == 64 and args.disc_bidirectional and args.disc_num_layers == 2
    return args


def run(mods, attn, case, dtype):
    module, network, utils, train = mods
    torch.set_default_dtype(dtype)
    train.DEVICE = torch.device("cpu")
    train.WRITER = None
    network.noise_fn = lambda x, *a, **k: x
    train.specaugment = lambda mel, mel_len, *a, **k: mel
    real_randperm = torch.randperm
    torch.randperm = lambda n, *a, **k: torch.arange(n)
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
        model.load_state_dict({k: torch.from_numpy(np.asarray(portable_tensor(k, s, SEED))).to(dtype if sd[k].is_floating_point() else sd[k].dtype)
                               for k, s in zip(keys, shapes)})
        if case == "a_eps":
            for bn in (model.text_m.prenet.batch_norm1, model.text_m.prenet.batch_norm2, model.text_m.prenet.batch_norm3):
                bn.eps = EPS_COND
        model.train()
        text, mel, tl, ml = inputs(case)
        batch = lambda: (torch.from_numpy(text), torch.from_numpy(mel).to(dtype), torch.from_numpy(tl), torch.from_numpy(ml))   # noqa: E731
        losses = defaultdict(list)
        out = dict(grads={}, norm={}, state={})

        def step(tag):
            out["grads"][tag] = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
            out["norm"][tag] = float(torch.nn.utils.clip_grad_norm_(model.parameters(), 1e30))      # the pre-clip norm (nothing is scaled)
            train.optimizer_step(model, optimizer, args)
            out["state"][tag] = {k: v.detach().clone() for k, v in model.state_dict().items()}
            assert all(p.grad is None for p in model.parameters())

        train.freeze_model_parameters(model.discriminator)
        train.train_ae_step(losses, model, batch(), 0, 2, args)
        train.train_sp_step(losses, model, batch(), 0, 2, args)
        step("gen")
        train.unfreeze_model_parameters(model.discriminator)
        train.train_discriminator_step(losses, model, batch(), 0, 1, args)
        step("disc")
        out["losses"] = {k: float(losses[k][0]) for k in LOSS_KEYS}
        out["opt_steps"] = {k: int(optimizer.state[p]["step"]) if p in optimizer.state and "step" in optimizer.state[p] else 0 for k, p in model.named_parameters()}
        return out, dict(keys=keys, shapes=shapes, lr=args.lr, weight_decay=args.weight_decay)
    finally:
        torch.randperm = real_randperm
        torch.set_default_dtype(torch.float32)


def normerr(got, ref):
    ref = ref.double()
    return ((got.double() - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    mods = import_reference()
    cfgs = {}
    for name in RNN_CONFIGS:
        cfg = json.load(open(os.path.join(REF_SRC, "configs", name + ".json")))
        cfgs[name] = {k: v for k, v in cfg.items() if not k.endswith("_path")}
    with open(os.path.join(a.out, "rnn_configs.json"), "w") as f:
        json.dump(cfgs, f, indent=1, sort_keys=True)
        f.write("\n")
    for attn in ("luong", "lsa"):
        arrs, spec = {}, None
        for case in ("a", "b", "a_eps"):
            r64, spec = run(mods, attn, case, torch.float64)
            r32, _ = run(mods, attn, case, torch.float32)
            if case != "a_eps":
                text, mel, tl, ml = inputs(case)
                arrs.update({case + "/text": text, case + "/mel": mel, case + "/text_len": tl, case + "/mel_len": ml})
            for k in LOSS_KEYS:
                arrs["%s/loss/%s" % (case, k)] = np.float64(r64["losses"][k])
                arrs["e32/%s/loss/%s" % (case, k)] = np.float64(abs(r32["losses"][k] - r64["losses"][k]))
            for tag in ("gen", "disc"):
                arrs["%s/%s/norm" % (case, tag)] = np.float64(r64["norm"][tag])
                arrs["e32/%s/%s/norm" % (case, tag)] = np.float64(abs(r32["norm"][tag] - r64["norm"][tag]))
                assert sorted(r64["grads"][tag]) == sorted(r32["grads"][tag])
                g64, g32 = r64["grads"][tag], r32["grads"][tag]
                gkeys = list(g64)
                pack(arrs, "%s/%s/g" % (case, tag), gkeys, [sample(g64[k].numpy(), G_SAMPLE) for k in gkeys])
                arrs["%s/%s/gnorm" % (case, tag)] = np.array([g64[k].norm().item() for k in gkeys])
                arrs["e32/%s/%s/grad" % (case, tag)] = np.array([normerr(g32[k], g64[k]) for k in gkeys])
                prev = r64["state"]["gen"] if tag == "disc" else None
                st = r64["state"][tag]
                nbt = {k: int(v) for k, v in st.items() if k.endswith("num_batches_tracked")}
                moved = [k for k, v in st.items() if k not in nbt and (prev is None or not torch.equal(prev[k], v))]      # the D phase records what it moved
                pack(arrs, "%s/%s/state" % (case, tag), moved, [sample(st[k].numpy(), P_SAMPLE) for k in moved])
                arrs["%s/%s/num_batches_tracked" % (case, tag)] = np.array(json.dumps(nbt))
                s32 = r32["state"][tag]
                arrs["e32/%s/%s/state" % (case, tag)] = np.array([np.abs(sample(s32[k].double().numpy(), P_SAMPLE) - sample(st[k].numpy(), P_SAMPLE)).max() for k in moved])
            arrs["%s/opt_steps" % case] = np.array(json.dumps(r64["opt_steps"]))
            worst = max(zip(arrs["e32/%s/gen/grad" % case].tolist(), json.loads(str(arrs["%s/gen/g/keys" % case]))))
            print("%s %s: losses %s  norms %.6g %.6g  worst gen e32 %.3g (%s)" % (attn, case, {k: round(v, 6) for k, v in r64["losses"].items()},
                                                                                  r64["norm"]["gen"], r64["norm"]["disc"], worst[0], worst[1]))
        arrs["meta"] = np.array(json.dumps(dict(keys=spec["keys"], shapes=spec["shapes"], seed=SEED, attn=attn, eps_cond=EPS_COND, lr=spec["lr"],
                                                weight_decay=spec["weight_decay"], accum_steps=2, grad_clip=1.0, disc_hid=64, g_sample=G_SAMPLE, p_sample=P_SAMPLE)))
        path = os.path.join(a.out, "rnn_step_%s.npz" % attn)
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        assert size <= MAX_BYTES, (path, size)
        print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
