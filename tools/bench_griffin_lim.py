#!/usr/bin/env python3
"""Waveform synthesis (unast_amd.audio.spectrogram2wav_batch, csrc/audio.hip) at B=32, T=800 and B=1, T=800 on one GPU: the whole call
(de-normalisation, 60 Griffin-Lim iterations, de-preemphasis, trim; median of --iters calls, HIP events on one stream), one Griffin-Lim
iteration (the three launches, median over a run of iterations) and its split by kernel (events around every launch, normalised by their own
sum).  Baseline: the same definitions through torch.stft / torch.istft in float32 on the CPU with --threads threads (the only baseline there
is: the parent commit has no synthesis, and the reference runs librosa on one core per utterance), timed over --cpu-iters iterations.

Bytes per iteration: what the three kernels must move when every re-read of a frame's samples hits a cache -- spectra read and written
(2 x 8 bytes x bins), the windowed frames written and read (2 x 4 x win), the magnitude read (4 x bins), the signal written and read
(2 x 4 x hop) per frame; set against HBM_PEAK = 8 TB/s.  Prints one JSON line per batch size.
Usage: python tools/bench_griffin_lim.py [--frames 800] [--warmup 2] [--iters 7] [--cpu-iters 3] [--threads 16] [--no-cpu]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unast_amd import audio, ops  # noqa: E402

HBM_PEAK = 8.0e12


def bytes_per_iteration(B, T, p):
    return B * T * (2 * 8 * p.bins + 2 * 4 * p.win + 4 * p.bins + 2 * 4 * p.hop)


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def cpu_iteration_ms(M, p, iters, threads):
    """One Griffin-Lim iteration of the float32 CPU path, batched: istft then stft with the phase update."""
    torch.set_num_threads(threads)
    w = torch.from_numpy((0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(p.win) / p.win)).astype(np.float32))
    Mt = M.transpose(1, 2).contiguous()                        # torch's layout [B, bins, T]
    X = Mt.to(torch.complex64)
    n = p.hop * (M.shape[1] - 1)
    times = []
    for _ in range(iters + 1):
        t0 = time.perf_counter()
        y = torch.istft(X, p.n_fft, hop_length=p.hop, win_length=p.win, window=w, center=True, length=n)
        e = torch.stft(y, p.n_fft, hop_length=p.hop, win_length=p.win, window=w, center=True, pad_mode="reflect", return_complex=True)
        X = Mt * e / torch.clamp(e.abs(), min=1e-8)
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times[1:])


def run(B, T, a):
    dev = torch.device("cuda:0")
    p = audio.AudioParams()
    g = torch.Generator().manual_seed(B)
    mags = (0.35 + 0.5 * torch.rand(B, T, p.bins, generator=g)).to(dev)
    lens = [T] * B
    total = []
    for i in range(a.warmup + a.iters):
        e0, e1 = events()
        e0.record()
        wavs = audio.spectrogram2wav_batch(mags, lens, p)
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            total.append(e0.elapsed_time(e1))
    # ---- the iteration alone: 60 iterations between two events, and events around every launch of a further run ----
    M = torch.empty(B, T, p.bins, device=dev)
    ops.gl_prepare(mags, p.max_db, p.ref_db, p.power, M)
    loop = []
    for i in range(a.warmup + a.iters):
        e0, e1 = events()
        e0.record()
        audio.griffin_lim(M, lens, p)
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            loop.append(e0.elapsed_time(e1) / (p.n_iter + 0.5))   # 60 iterations and a closing istft (two of an iteration's three launches)
    records = []

    def timed(fn, name):
        def wrapper(*args, **kw):
            e0, e1 = events()
            e0.record()
            r = fn(*args, **kw)
            e1.record()
            records.append((name, e0, e1))
            return r
        return wrapper
    saved = {n: getattr(ops, n) for n in ("istft_frames", "overlap_add", "stft")}
    for n, f in saved.items():
        setattr(ops, n, timed(f, n))
    try:
        audio.griffin_lim(M, lens, p)
        torch.cuda.synchronize()
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)
    split = {}
    for name, e0, e1 in records:
        split.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
    it_us = statistics.median(loop) * 1e3
    nbytes = bytes_per_iteration(B, T, p)
    out = {"workload": "spectrogram2wav_batch", "batch": B, "frames": T, "n_iter": p.n_iter, "samples_out": int(sum(len(w) for w in wavs)),
           "total_ms_median": round(statistics.median(total), 3), "total_ms_min": round(min(total), 3), "total_ms_max": round(max(total), 3),
           "iteration_us_median": round(it_us, 1), "iteration_us_min": round(min(loop) * 1e3, 1), "iteration_us_max": round(max(loop) * 1e3, 1),
           "kernel_us_median": {k: round(statistics.median(v), 1) for k, v in split.items()},
           "bytes_per_iteration": nbytes, "tb_per_s": round(nbytes / (it_us * 1e-6) / 1e12, 3), "hbm_peak_fraction": round(nbytes / (it_us * 1e-6) / HBM_PEAK, 3),
           "iters": a.iters, "warmup": a.warmup}
    if not a.no_cpu:
        cpu_ms = cpu_iteration_ms(M.cpu(), p, a.cpu_iters, a.threads)
        out.update({"cpu_float32_iteration_ms": round(cpu_ms, 2), "cpu_threads": a.threads, "cpu_iters": a.cpu_iters,
                    "cpu_float32_60_iterations_ms_extrapolated": round(cpu_ms * (p.n_iter + 0.5), 1),
                    "iteration_speedup_vs_cpu": round(cpu_ms * 1e3 / it_us, 1)})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--cpu-iters", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_griffin_lim.py measures on a GPU; none found")
    for B in (32, 1):
        run(B, a.frames, a)


if __name__ == "__main__":
    main()
