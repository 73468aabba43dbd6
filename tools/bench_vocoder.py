#!/usr/bin/env python3
"""Eval forward of the CBHG vocoder (unast_amd.network.Vocoder) at B=32, T=800 on one GPU: median of 20 timed launches after 5 warm-up
ones (HIP events around each forward, single stream), then a per-family split from HIP events around every kernel launch of further
forwards (the events serialise nothing -- the forward is one stream -- but each pair adds its own few microseconds, so the split is
normalised by its own sum, not by the end-to-end figure).  Prints one JSON line.

Algorithmic work: 2 FLOP per multiply-add of every contraction, counted from the shapes (about 27.3 MFLOP per frame).  peak_fraction sets
the whole forward's rate against PEAK_TFLOPS: the chip's dense bf16 MFMA rate (16 x the 157.3 TFLOP/s fp32 rate) over the three MFMAs a
split-bf16 product takes -- an end-to-end figure (recurrence, pooling and launch gaps included), not a kernel's share of peak.
Usage: python tools/bench_vocoder.py [--batch 32] [--frames 800] [--warmup 5] [--iters 20] [--split-iters 5]
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


PEAK_TFLOPS = 16 * 157.3 / 3


def flop_per_frame(num_mels=80, C=256, K=16, bins=1025):
    macs = num_mels * C + sum(k * C * C for k in range(1, K + 1)) + 3 * K * C * C + 3 * C * C + 4 * 2 * C * C + 2 * 3 * C * C + bins * C
    gru = 2 * 2 * 3 * (C // 2) * (C // 2)               # recurrent multiply-adds: 2 layers x 2 directions x 384 x 128
    return 2 * (macs + gru)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--split-iters", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vocoder.py measures on a GPU; none found")
    dev = torch.device("cuda:0")
    model = Vocoder(80, 256, 2048)
    model.load_state_dict({k: torch.from_numpy(portable_tensor(k, tuple(v.shape), 1234)) for k, v in model.state_dict().items()})
    model = model.to(dev).eval()
    mel = torch.rand(a.batch, a.frames, 80, generator=torch.Generator().manual_seed(0)).to(dev)
    times = []
    with torch.no_grad():
        for i in range(a.warmup + a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            model(mel)
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times.append(e0.elapsed_time(e1))
        # ---- per-family split: events around every launch ----
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

        def conv_family(x3d, Wp, bias, out, pad_left, act=0, R=None):
            return "projection 1" if x3d.shape[2] > 256 else "projection 2" if R is not None else "bank convs"

        def gemm_family(a_mode, b_mode, A, lda, B, ldb, C, ldc, M, N, K, **kw):
            return {512: "highway", 768: "GRU input GEMMs", 256: "pre-projection"}.get(N, "post-projection")
        saved = {n: getattr(ops, n) for n in ("conv_taps_fwd", "gemm", "gru_fwd", "maxpool_prev", "highway_combine")}
        ops.conv_taps_fwd = timed(saved["conv_taps_fwd"], conv_family)
        ops.gemm = timed(saved["gemm"], gemm_family)
        ops.gru_fwd = timed(saved["gru_fwd"], lambda *x, **k: "GRU recurrence")
        ops.maxpool_prev = timed(saved["maxpool_prev"], lambda *x, **k: "max pool")
        ops.highway_combine = timed(saved["highway_combine"], lambda *x, **k: "highway")
        try:
            for _ in range(a.split_iters):
                model(mel)
            torch.cuda.synchronize()
        finally:
            for n, f in saved.items():
                setattr(ops, n, f)
    split = {}
    for fam, e0, e1 in records:
        split[fam] = split.get(fam, 0.0) + e0.elapsed_time(e1) / a.split_iters
    med = statistics.median(times)
    flop = flop_per_frame() * a.batch * a.frames
    gru_ms = split.get("GRU recurrence", 0.0)
    print(json.dumps({"workload": "vocoder eval forward", "batch": a.batch, "frames": a.frames, "median_ms": round(med, 3),
                      "min_ms": round(min(times), 3), "max_ms": round(max(times), 3), "iters": a.iters, "warmup": a.warmup,
                      "algorithmic_tflop": round(flop / 1e12, 4), "achieved_tflops": round(flop / 1e12 / (med / 1e3), 2),
                      "peak_fraction": round(flop / 1e12 / (med / 1e3) / PEAK_TFLOPS, 4),
                      "split_ms": {k: round(v, 3) for k, v in sorted(split.items(), key=lambda kv: -kv[1])},
                      "split_sum_ms": round(sum(split.values()), 3),
                      "gru_us_per_step": round(gru_ms * 1e3 / (2 * a.frames), 3)}))


if __name__ == "__main__":
    main()
