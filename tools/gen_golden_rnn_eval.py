#!/usr/bin/env python3
"""Golden vectors of the RNN family's evaluate() (src/train.py:474-565): the fixtures of unast_amd.eval_rnn.

Runs ONLY in the build container: imports the reference (tools/gen_golden.import_reference), builds UNAST(TextRNN, SpeechRNN, LSTMDiscriminator)
from the reference's rnn_d_{luong,lsa} config, loads seeded weights by name with 5m's gains (tests/rnn_cm_mirror.state_dict) and a gain of
rnn_eval_fixture.DISC_GAIN on the discriminator's weight matrices (so that the d_* losses respond to what they are fed), and runs the
reference's OWN evaluate() on the CPU in fp64 and once more in fp32, once plain and once with is_test, per attention type on two one-batch
loaders (CASES below: the batches of tests/rnn_cm_mirror.CM_FIXTURE, weights seeded per case):

  a   B = 3, T_text = 7, T_mel = 12, infer_sequence caps 7 (text) / 12 (speech);
  b   B = 2, T_text = 6, T_mel = 10, caps 6 / 10, with one sequence of each generation that never stops.

Patched, and nothing else: noise_fn and specaugment to the identity, torch.randperm to the identity, infer_sequence's default caps, compute_per by
a recorder (jiwer is not installed), compare_outputs and the TensorBoard logger to no-ops, tqdm to the identity.

It ASSERTS: every live argmax top-2 gap and stop margin of every generation evaluate() runs >= 1e-2 of the largest logit, that the fp32 and
fp64 runs agree on every token and length, and that no PAD id lies inside a generated sentence's length.

Writes data-only fixtures tests/golden/rnn_eval_{luong,lsa}.npz: per case the losses, the tokens and lengths evaluate() hands compute_per, the
is_test run's d_score, JSON content, TTS stop_lens and a strided sample of the saved frames, and `e32/...` = the fp32 run's error against the
fp64 run of each quantity.  Weights are not stored: seeds and gains are.  Usage: python tools/gen_golden_rnn_eval.py [--out tests/golden] [--scan N]
"""
import argparse
import json
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from gen_golden import import_reference, REF_SRC  # noqa: E402
from tests import rnn_cm_mirror as CM  # noqa: E402
from tests import rnn_eval_fixture as EF  # noqa: E402
from tests import rnn_step_fixture as SF  # noqa: E402

MARGIN = 1e-2
FRAME_SAMPLE = 256
MAX_BYTES = 900000
# weight seeds chosen on the reference side alone (--scan): the first seed from 1234 on whose fp64 and fp32 runs keep MARGIN, decide alike,
# generate no live PAD and give the case's lengths their shape (a: lengths that differ; b: one sequence of each generation never stops)
CASES = {"luong": {"a": dict(weight_seed=1236, eos_bias=50.0, stop_bias=-6.0), "b": dict(weight_seed=1237, eos_bias=60.0, stop_bias=-4.0)},
         "lsa": {"a": dict(weight_seed=1235, eos_bias=50.0, stop_bias=-6.0), "b": dict(weight_seed=1239, eos_bias=40.0, stop_bias=-3.0)}}
LOSS_KEYS = ("t_ae", "s_ae", "d_ae", "asr", "tts", "d_sp", "s_cm", "t_cm", "d_cm", "dis")


def case_spec(attn, case):
    fx = dict(CM.CM_FIXTURE[attn][case])
    fx.update(CASES[attn][case], disc_gain=EF.DISC_GAIN)
    return fx


def make_args(attn, out_dir, B):
    cfg = json.load(open(os.path.join(REF_SRC, "configs", "rnn_d_%s.json" % attn)))
    args = SimpleNamespace(**cfg)
    args.load_path = None
    args.out_test_dir = out_dir
    args.eval_batch_size = B
    assert args.use_discriminator
    return args


def run(mods, attn, fx, dtype, inputs, is_test):
    module, network, utils, train = mods
    torch.set_default_dtype(dtype)
    train.DEVICE = torch.device("cpu")
    train.WRITER = None
    saved = dict(randperm=torch.randperm, t_def=network.TextRNN.infer_sequence.__defaults__, s_def=network.SpeechRNN.infer_sequence.__defaults__,
                 noise=network.noise_fn, spec=train.specaugment, per=train.compute_per, cmp=train.compare_outputs, tb=train.log_tb_discrim_out,
                 tqdm=getattr(train, "tqdm", None))
    torch.randperm = lambda n, *a, **k: torch.arange(n)
    network.TextRNN.infer_sequence.__defaults__ = (fx["max_text"],)
    network.SpeechRNN.infer_sequence.__defaults__ = (fx["max_speech"],)
    network.noise_fn = lambda x, *a, **k: x
    train.specaugment = lambda mel, *a, **k: mel
    rec = dict(per=[], logits=[], stops=[], gens=[])
    train.compute_per = lambda gt, hyp, gl, hl: rec["per"].append(tuple(torch.as_tensor(x).detach().clone() for x in (gt, hyp, gl, hl))) or 0.0
    train.compare_outputs = lambda *a, **k: None
    train.log_tb_discrim_out = lambda *a, **k: None
    train.tqdm = lambda x, *a, **k: x
    out_dir = tempfile.mkdtemp()
    try:
        args = make_args(attn, out_dir, fx["B"])
        _, _, model, _, _ = train.initialize_model(args)
        sd = model.state_dict()
        keys, shapes = list(sd.keys()), [list(v.shape) for v in sd.values()]
        new = EF.with_disc_gain(CM.state_dict(keys, shapes, fx["weight_seed"], CM.gains(fx["eos_bias"], fx["stop_bias"])), fx["disc_gain"])
        model.load_state_dict({k: v.to(dtype if sd[k].is_floating_point() else sd[k].dtype) for k, v in new.items()})
        t_dec, s_dec, t_inf, s_inf = model.text_m.decode, model.speech_m.decode, model.text_m.infer_sequence, model.speech_m.infer_sequence
        live = dict(t=None, s=None)

        def t_wrap(*a):
            o, h = t_dec(*a)
            if live["t"] is not None:
                live["t"].append(o[:, 0].detach().clone())
            return o, h

        def s_wrap(*a):
            (o, s), h = s_dec(*a)
            if live["s"] is not None:
                live["s"].append(s[:, 0, 0].detach().clone())
            return (o, s), h

        def t_infer(*a, **k):
            live["t"] = []
            r = t_inf(*a, **k)
            lg, live["t"] = torch.stack(live["t"], 1).double(), None
            top2 = lg.topk(2, dim=-1).values
            on = torch.arange(lg.shape[1])[None, :] < r[1][:, None]
            rec["gens"].append(dict(kind="text", tokens=r[0].detach().clone(), lens=r[1].detach().clone(),
                                    margin=((top2[..., 0] - top2[..., 1])[on]).min().item() / lg.abs().max().item(),
                                    live_pad=int(((r[0] == 0) & on[:, :r[0].shape[1]]).sum())))
            return r

        def s_infer(*a, **k):
            live["s"] = []
            r = s_inf(*a, **k)
            sl, live["s"] = torch.stack(live["s"], 1).double(), None
            on = torch.arange(sl.shape[1])[None, :] < r[3][:, None]
            rec["gens"].append(dict(kind="speech", post=r[1].detach().clone(), stop=r[2].detach().clone(), lens=r[3].detach().clone(),
                                    margin=sl.abs()[on].min().item() / sl.abs().max().item(), live_pad=0))
            return r
        model.text_m.decode, model.speech_m.decode, model.text_m.infer_sequence, model.speech_m.infer_sequence = t_wrap, s_wrap, t_infer, s_infer
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        text, mel, tl, ml = inputs
        batch = (text, mel.to(dtype), torch.tensor(tl), torch.tensor(ml))
        fnames = ["utt%d" % b for b in range(fx["B"])]
        loader = [(batch, fnames)] if is_test else [batch]
        res = train.evaluate(model, loader, 0, args, is_test=is_test)
        after = model.state_dict()
        assert all(torch.equal(before[k], after[k]) for k in before), "the reference's evaluate() moved the state"
        out = dict(losses={k: float(res[1][k][0]) for k in LOSS_KEYS}, per=rec["per"], gens=rec["gens"])
        if is_test:
            out["d_score"] = float(res[2])
            out["json"] = json.load(open(os.path.join(out_dir, "text_preds.json")))
            out["mels"] = [np.load(os.path.join(out_dir, "mels", f + ".pt.npy")) for f in fnames]
        return out
    finally:
        torch.randperm = saved["randperm"]
        network.TextRNN.infer_sequence.__defaults__, network.SpeechRNN.infer_sequence.__defaults__ = saved["t_def"], saved["s_def"]
        network.noise_fn, train.specaugment, train.compute_per, train.compare_outputs = saved["noise"], saved["spec"], saved["per"], saved["cmp"]
        train.log_tb_discrim_out = saved["tb"]
        if saved["tqdm"] is not None:
            train.tqdm = saved["tqdm"]
        torch.set_default_dtype(torch.float32)


def qualifies(case, fx, r64, r32):
    """None if the pair of runs can serve as a fixture, else why not."""
    for r in (r64, r32):
        for g in r["gens"]:
            if g["margin"] < MARGIN:
                return "%s margin %.3g" % (g["kind"], g["margin"])
            if g["live_pad"]:
                return "live PAD"
    if len(r64["gens"]) != len(r32["gens"]):
        return "different generations"
    for a, b in zip(r64["gens"], r32["gens"]):
        if not torch.equal(a["lens"], b["lens"]) or (a["kind"] == "text" and not torch.equal(a["tokens"], b["tokens"])):
            return "fp32 decides differently"
    tl = [g["lens"].tolist() for g in r64["gens"] if g["kind"] == "text"]
    sl = [g["lens"].tolist() for g in r64["gens"] if g["kind"] == "speech"]
    if case == "a":
        if not all(len(set(x)) > 1 for x in tl + sl):
            return "lengths alike %s %s" % (tl, sl)
    elif not all(fx["max_text"] in x and min(x) < fx["max_text"] for x in tl) or not all(fx["max_speech"] in x and min(x) < fx["max_speech"] for x in sl):
        return "no sequence that never stops next to one that does %s %s" % (tl, sl)
    return None


def sample(v, limit):
    return SF.sample(v, limit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--attn", default="luong,lsa")
    ap.add_argument("--scan", type=int, default=0, help="try this many weight seeds from 1234 on per case and print the ones that qualify")
    a = ap.parse_args()
    mods = import_reference()
    for attn in a.attn.split(","):
        arrs, setups = {}, {}
        for case in ("a", "b"):
            fx = case_spec(attn, case)
            inputs = CM.fixture_batch(fx)
            if a.scan:
                for seed in range(1234, 1234 + a.scan):
                    f2 = dict(fx, weight_seed=seed)
                    why = qualifies(case, f2, run(mods, attn, f2, torch.float64, inputs, False), run(mods, attn, f2, torch.float32, inputs, False))
                    print(attn, case, seed, why or "QUALIFIES", flush=True)
                    if why is None:
                        break
                continue
            r64, r32 = run(mods, attn, fx, torch.float64, inputs, False), run(mods, attn, fx, torch.float32, inputs, False)
            t64, t32 = run(mods, attn, fx, torch.float64, inputs, True), run(mods, attn, fx, torch.float32, inputs, True)
            for x64, x32 in ((r64, r32), (t64, t32)):
                why = qualifies(case, fx, x64, x32)
                assert why is None, (attn, case, why)
            print("%s %s: losses %s" % (attn, case, {k: round(v, 5) for k, v in r64["losses"].items()}))
            print("   generations:", [(g["kind"], g["lens"].tolist(), "%.3g" % g["margin"]) for g in t64["gens"]], "d_score", t64["d_score"])
            assert r64["losses"] == t64["losses"], "is_test changes no loss"
            for k in LOSS_KEYS:
                arrs["%s/loss/%s" % (case, k)] = np.float64(r64["losses"][k])
                arrs["e32/%s/loss/%s" % (case, k)] = np.float64(abs(r32["losses"][k] - r64["losses"][k]))
            (gt, hyp, gl, hl), = r64["per"]
            arrs["%s/asr/tokens" % case], arrs["%s/asr/lens" % case] = hyp.numpy().astype(np.int64), hl.numpy().astype(np.int64)
            assert torch.equal(hyp, r32["per"][0][1]) and torch.equal(hl, r32["per"][0][3])
            # the generations in evaluate()'s order: cm text, cm speech, asr[, tts]
            kinds = [g["kind"] for g in t64["gens"]]
            assert kinds == ["text", "speech", "text", "speech"], kinds
            cm_t, cm_s, _, tts = t64["gens"]
            cm_s32, tts32 = t32["gens"][1], t32["gens"][3]
            arrs["%s/cm/tokens" % case], arrs["%s/cm/text_lens" % case] = cm_t["tokens"].numpy().astype(np.int64), cm_t["lens"].numpy().astype(np.int64)
            arrs["%s/cm/speech_lens" % case] = cm_s["lens"].numpy().astype(np.int64)
            arrs["%s/cm/post" % case], arrs["%s/cm/stop" % case] = cm_s["post"].numpy(), cm_s["stop"].numpy()
            arrs["e32/%s/cm/post" % case] = np.float64((cm_s32["post"].double() - cm_s["post"]).abs().max().item())
            arrs["e32/%s/cm/stop" % case] = np.float64((cm_s32["stop"].double() - cm_s["stop"]).abs().max().item())
            arrs["%s/tts/stop_lens" % case] = tts["lens"].numpy().astype(np.int64)
            arrs["%s/tts/stop" % case] = tts["stop"].numpy()
            arrs["e32/%s/tts/stop" % case] = np.float64((tts32["stop"].double() - tts["stop"]).abs().max().item())
            arrs["%s/d_score" % case] = np.float64(t64["d_score"])
            assert abs(t64["d_score"] - t32["d_score"]) < 1e-6
            arrs["%s/json" % case] = np.array(json.dumps(t64["json"], sort_keys=True))
            assert t64["json"] == t32["json"]
            for b, (m64, m32) in enumerate(zip(t64["mels"], t32["mels"])):
                assert m64.shape == m32.shape == (int(tts["lens"][b]), m64.shape[1])
                arrs["%s/mels/%d" % (case, b)] = sample(m64, FRAME_SAMPLE)
            arrs["e32/%s/mels" % case] = np.float64(max(np.abs(m32.astype(np.float64) - m64).max() for m64, m32 in zip(t64["mels"], t32["mels"])))
            arrs["%s/margins" % case] = np.array([g["margin"] for g in t64["gens"]])
            setups[case] = fx
        if a.scan:
            continue
        arrs["meta"] = np.array(json.dumps(dict(attn=attn, setups=setups, frame_sample=FRAME_SAMPLE, loss_keys=LOSS_KEYS)))
        path = os.path.join(a.out, "rnn_eval_%s.npz" % attn)
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        assert size <= MAX_BYTES, (path, size)
        print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
