#!/usr/bin/env python3
"""One evaluate() batch of the RNN family at the configs' eval shape (B = 128, T_text = 180, T_mel = 800) per attention type, split into the
loss passes, the generations behind PER and the metric itself, and compute_per_device against utils.compute_per on the same tokens.

Times: HIP events around each part on the current stream (ms, median of --reps after one warm-up of the same shapes); the host metric with
time.perf_counter around the host function, its inputs already on the host.  The metric pair is also timed at a long-hypothesis shape
(--per-tokens ids per side), where greedy decoding with these seeded weights gives short sentences.  Usage (on the GPU machine):
    python tools/bench_rnn_eval.py [--reps 3] > profiles/rnn_eval_bench.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    """(median ms by HIP events, result of the last call); one warm-up call first."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), out


def host_timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), out


def metric_pair(name, gt, hyp, gl, hl, reps):
    from unast_amd import utils
    dev_ms, dev_per = timed(lambda: utils.compute_per_device(gt, hyp, gl, hl), reps)
    host = tuple(x.cpu() for x in (gt, hyp, gl, hl))
    host_ms, host_per = host_timed(lambda: utils.compute_per(*host), max(1, min(reps, 2)))
    assert dev_per == host_per, (dev_per, host_per)
    print("%s: truth %d ids, hypothesis %d ids: compute_per_device %.3f ms (one kernel + 8-byte read-back), utils.compute_per %.3f ms on the host, "
          "ratio %.1f, PER %.4f (equal)" % (name, int(gl.sum()), int(hl.sum()), dev_ms, host_ms, host_ms / dev_ms, dev_per), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T-text", type=int, default=180)
    ap.add_argument("--T-mel", type=int, default=800)
    ap.add_argument("--per-tokens", type=int, default=23040, help="ids per side of the long metric shape (128 x 180)")
    a = ap.parse_args()
    from tests import rnn_cm_mirror as CM
    from tests import rnn_step_fixture as SF
    from unast_amd import eval_rnn, train, utils
    from unast_amd.portable import synth_batch
    dev = torch.device("cuda:0")
    train.DEVICE = dev
    print("device:", torch.cuda.get_device_name(0), "| B %d T_text %d T_mel %d | reps %d" % (a.B, a.T_text, a.T_mel, a.reps), flush=True)
    rng = np.random.RandomState(0)
    tl = rng.randint(a.T_text // 2, a.T_text + 1, size=a.B)
    ml = rng.randint(a.T_mel // 2, a.T_mel + 1, size=a.B)
    tl[0], ml[0] = a.T_text, a.T_mel
    text, mel, _, _ = synth_batch(a.B, a.T_text, a.T_mel, seed=1)
    for b in range(a.B):
        text[b, tl[b] - 1], text[b, tl[b]:], mel[b, ml[b]:] = utils.EOS_IDX, utils.PAD_IDX, 0.0
    batch = (torch.from_numpy(text), torch.from_numpy(mel), torch.from_numpy(tl), torch.from_numpy(ml))
    for attn in ("luong", "lsa"):
        utils.set_seed(0)
        args = SF.args_of(attn, None, eval_batch_size=a.B)
        _, _, model, _, _ = train.initialize_model(args)
        m = SF.meta(attn)
        model.load_state_dict(CM.state_dict(m["keys"], m["shapes"], 1234, CM.gains(40.0, -3.0)))
        parts = {}
        for name, fn in (("autoencoder_losses", eval_rnn.autoencoder_losses), ("supervised_losses", eval_rnn.supervised_losses),
                         ("crossmodel_losses (two generations inside)", eval_rnn.crossmodel_losses), ("discriminator_eval", eval_rnn.discriminator_eval)):
            parts[name], _ = timed(lambda fn=fn: [x.item() for x in fn(model, batch, args) if torch.is_tensor(x)], a.reps)      # one .item() per loss, as evaluate() takes them
        text_d, mel_d, tl_l, ml_l, tl_d, ml_d = eval_rnn._process(batch)

        def asr():
            s_mem, s_mask, _ = eval_rnn._encode(model.speech_m, mel_d, ml_l)
            return model.text_m.generation(s_mem, s_mask, eval_rnn.TEXT_MAX_LEN).run()
        with torch.no_grad():
            parts["ASR generation behind PER (cap %d)" % eval_rnn.TEXT_MAX_LEN], (pred, pred_len) = timed(asr, a.reps)
        whole, _ = timed(lambda: eval_rnn.evaluate(model, [batch], 0, args), max(1, a.reps - 1))
        for k, v in parts.items():
            print("%s %-48s %10.2f ms" % (attn, k, v))
        print("%s %-48s %10.2f ms (generated lengths %d..%d)" % (attn, "evaluate(), one batch, whole", whole, int(pred_len.min()), int(pred_len.max())), flush=True)
        metric_pair(attn + " PER of this batch", text_d, pred, tl_d, pred_len, a.reps)
    # the metric at the length evaluate() sees once a model emits full sentences: B rows of T_text ids on both sides, ~20 % edits
    n = a.per_tokens // a.B
    ref = rng.randint(3, 45, size=(a.B, n))
    hyp = np.where(rng.rand(a.B, n) < 0.2, rng.randint(3, 45, size=(a.B, n)), ref)
    gl = torch.full((a.B,), n, dtype=torch.int32, device=dev)
    hl = torch.from_numpy(rng.randint(int(0.8 * n), n + 1, size=a.B).astype(np.int32)).to(dev)
    metric_pair("full-length sentences (%d x %d)" % (a.B, n), torch.from_numpy(ref).to(dev), torch.from_numpy(hyp).to(dev), gl, hl, a.reps)
    n2 = 300
    ref2 = rng.randint(3, 45, size=(a.B, n2))
    metric_pair("at the text cap (%d x %d)" % (a.B, n2), torch.from_numpy(ref2).to(dev), torch.from_numpy(rng.randint(3, 45, size=(a.B, n2))).to(dev),
                torch.full((a.B,), n2, dtype=torch.int32, device=dev), torch.full((a.B,), n2, dtype=torch.int32, device=dev), a.reps)


if __name__ == "__main__":
    main()
