#!/usr/bin/env python3
"""One training step of the CBHG vocoder (unast_amd.train_vocoder: vocoder_step + FlatAdamW.step) at B=32, T=800 on one GPU: median of 20
timed steps after 3 warm-up ones (HIP events around each step, single stream), then a per-family split from HIP events around every
wrapper call of further steps (the step is one stream, so the events serialise nothing, but each pair adds its own few microseconds: the
split is normalised by its own sum, not by the end-to-end figure; torch's layout copies and zero fills fall between the pairs).
Prints one JSON line.  No speed target is claimed for this path; the figures are recorded in DESIGN.md section 5g.
Usage: python tools/bench_vocoder_train.py [--batch 32] [--frames 800] [--warmup 3] [--iters 20] [--split-iters 3] [--loss l1]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unast_amd import ops  # noqa: E402
from unast_amd.network import Vocoder  # noqa: E402
from unast_amd.portable import portable_tensor  # noqa: E402
from unast_amd.train_vocoder import FlatAdamW, vocoder_step  # noqa: E402


def gemm_family(a_mode, b_mode, A, lda, B, ldb, C, ldc, M, N, K, **kw):
    if a_mode == ops.OP_RC:
        return "linear / GRU weight gradients"
    if b_mode == ops.OP_RC:
        return "linear / GRU input gradients"
    return {512: "highway GEMMs", 768: "GRU input GEMMs", 256: "pre-projection"}.get(N, "post-projection")


FAMILIES = {
    "gemm": gemm_family,
    "conv_taps_fwd": lambda x3d, *a, **k: "projection 1 conv (fwd)" if x3d.shape[2] > 256 else "bank + projection 2 convs (fwd)",
    "conv_taps_dgrad": lambda *a, **k: "conv input gradients",
    "conv_taps_wgrad": lambda *a, **k: "conv weight gradients",
    "bn_fwd": lambda *a, **k: "BatchNorm (fwd)",
    "bn_bwd": lambda *a, **k: "BatchNorm (bwd)",
    "gru_fwd_train": lambda *a, **k: "GRU recurrence (fwd)",
    "gru_bwd": lambda *a, **k: "GRU recurrence (bwd)",
    "maxpool_prev": lambda *a, **k: "max pool, ReLU gates, highway combine, loss",
    "maxpool_prev_bwd": lambda *a, **k: "max pool, ReLU gates, highway combine, loss",
    "relu_bwd": lambda *a, **k: "max pool, ReLU gates, highway combine, loss",
    "highway_combine": lambda *a, **k: "max pool, ReLU gates, highway combine, loss",
    "highway_combine_bwd": lambda *a, **k: "max pool, ReLU gates, highway combine, loss",
    "sum_loss": lambda *a, **k: "max pool, ReLU gates, highway combine, loss",
    "add_inplace": lambda *a, **k: "max pool, ReLU gates, highway combine, loss",
    "sumsq": lambda *a, **k: "optimizer (sumsq + adamw)",
    "adamw": lambda *a, **k: "optimizer (sumsq + adamw)",
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--split-iters", type=int, default=3)
    ap.add_argument("--loss", default="l1", choices=["l1", "l2"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vocoder_train.py measures on a GPU; none found")
    dev = torch.device("cuda:0")
    model = Vocoder(80, 256, 2048)
    model.load_state_dict({k: torch.from_numpy(portable_tensor(k, tuple(v.shape), 1234)) for k, v in model.state_dict().items()})
    model = model.to(dev).train()
    opt = FlatAdamW(model, lr=1e-4, weight_decay=1e-2)
    g = torch.Generator().manual_seed(0)
    mel = torch.rand(a.batch, a.frames, 80, generator=g).to(dev)
    mag = torch.rand(a.batch, a.frames, 1025, generator=g).to(dev)

    def step():
        loss, _ = vocoder_step(model, mel, mag, a.loss)
        opt.step(max_norm=1.0)
        return loss

    times, fb_times = [], []
    torch.cuda.reset_peak_memory_stats()
    for i in range(a.warmup + a.iters):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        loss, _ = vocoder_step(model, mel, mag, a.loss)
        e1.record()
        opt.step(max_norm=1.0)
        e2.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            times.append(e0.elapsed_time(e2))
            fb_times.append(e0.elapsed_time(e1))
    peak_gib = torch.cuda.max_memory_allocated() / 2 ** 30
    records = []

    def timed(fn, family):
        def wrapper(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*args, **kw)
            e1.record()
            records.append((family(*args, **kw), e0, e1))
            return r
        return wrapper
    saved = {n: getattr(ops, n) for n in FAMILIES}
    for n, fam in FAMILIES.items():
        setattr(ops, n, timed(saved[n], fam))
    try:
        for _ in range(a.split_iters):
            step()
        torch.cuda.synchronize()
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)
    split = {}
    for fam, e0, e1 in records:
        split[fam] = split.get(fam, 0.0) + e0.elapsed_time(e1) / a.split_iters
    med = statistics.median(times)
    print(json.dumps({"workload": "vocoder training step (forward, loss, backward, clip + AdamW)", "batch": a.batch, "frames": a.frames,
                      "loss_type": a.loss, "median_ms": round(med, 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3),
                      "forward_backward_median_ms": round(statistics.median(fb_times), 3), "iters": a.iters, "warmup": a.warmup,
                      "frames_per_s": round(a.batch * a.frames / (med / 1e3)), "last_loss": round(float(loss.item()), 3),
                      "peak_memory_gib": round(peak_gib, 2), "launches_per_step": len(records) // a.split_iters,
                      "split_ms": {k: round(v, 3) for k, v in sorted(split.items(), key=lambda kv: -kv[1])},
                      "split_sum_ms": round(sum(split.values()), 3)}))


if __name__ == "__main__":
    main()
