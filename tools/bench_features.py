#!/usr/bin/env python3
"""Feature extraction (unast_amd.audio.get_spectrograms_batch, the features kernel of csrc/audio.hip) at B=32 utterances of 6.5 s (143 325
samples, 522 frames at the defaults) on one GPU: the whole call with trimming (trim bounds, their read-back, the features launch) and the
features launch alone (trim=False), medians of --iters calls, HIP events on one stream.  Baseline: the same definitions in float32 on the CPU
with --threads threads (preemphasis in numpy, torch.stft, a float32 matmul with the mel basis, torch.log10), the only baseline there is: the
parent commit has no feature extraction, and the reference runs librosa on one core per utterance.

Bytes: what the features launch must move when every re-read of a frame's samples hits a cache -- the samples once (4 x hop per frame) and
the two normalised rows written (4 x (bins + n_mels)); set against HBM_PEAK = 8 TB/s.  Prints one JSON line.
Usage: python tools/bench_features.py [--batch 32] [--seconds 6.5] [--warmup 3] [--iters 15] [--cpu-iters 3] [--threads 16] [--no-cpu]
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
from unast_amd import audio  # noqa: E402

HBM_PEAK = 8.0e12


def speech_like(B, n, sr, seed=0):
    """Harmonics of a moving pitch under a slow envelope plus weak noise, 0.5 peak: nothing for trim to cut, every frame is computed."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    out = np.empty((B, n), dtype=np.float32)
    for b in range(B):
        f0 = 120.0 + 3.0 * b + 30.0 * np.sin(2 * np.pi * 1.3 * t + b)
        ph = 2 * np.pi * np.cumsum(f0) / sr
        x = sum(np.sin(h * ph + 0.3 * h) / h for h in range(1, 13)) * (0.6 + 0.4 * np.sin(2 * np.pi * 2.1 * t + 0.3 * b))
        x += 0.01 * rng.standard_normal(n)
        out[b] = 0.5 * x / np.abs(x).max()
    return out


def timed(fn, warmup, iters):
    ms = []
    for i in range(warmup + iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return ms


def cpu_ms(y, p, iters, threads):
    """The float32 CPU path for the whole batch (no trimming: there is nothing to trim in this input)."""
    torch.set_num_threads(threads)
    w = torch.from_numpy((0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(p.win) / p.win)).astype(np.float32))
    W = torch.from_numpy(audio.mel_basis(p)[0].copy())
    times = []
    for _ in range(iters + 1):
        t0 = time.perf_counter()
        e = np.concatenate([y[:, :1], y[:, 1:] - np.float32(p.preemphasis) * y[:, :-1]], axis=1)
        S = torch.stft(torch.from_numpy(e), p.n_fft, hop_length=p.hop, win_length=p.win, window=w, center=True, pad_mode="reflect", return_complex=True)
        A = S.abs().transpose(1, 2)

        def norm(x):
            return torch.clamp((20.0 * torch.log10(torch.clamp(x, min=1e-5)) - p.ref_db + p.max_db) / p.max_db, 1e-8, 1.0)
        mel, mag = norm(A @ W.t()), norm(A)
        times.append((time.perf_counter() - t0) * 1e3)
    assert mel.shape[2] == p.n_mels and mag.shape[2] == p.bins
    return statistics.median(times[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=6.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--cpu-iters", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_features.py measures on a GPU; none found")
    p = audio.AudioParams()
    B, n = a.batch, int(round(a.seconds * p.sr))
    y_host = speech_like(B, n, p.sr)
    y = torch.from_numpy(y_host).to("cuda:0")
    lens = [n] * B
    mel, mag, frames = audio.get_spectrograms_batch(y, lens, p)
    whole = timed(lambda: audio.get_spectrograms_batch(y, lens, p), a.warmup, a.iters)
    launch = timed(lambda: audio.get_spectrograms_batch(y, lens, p, trim=False), a.warmup, a.iters)
    T = sum(frames)
    nbytes = 4 * n * B + 4 * T * (p.bins + p.n_mels)
    us = statistics.median(launch) * 1e3
    out = {"workload": "get_spectrograms_batch", "batch": B, "samples": n, "seconds": a.seconds, "frames": frames[0], "frames_total": T,
           "whole_call_ms_median": round(statistics.median(whole), 3), "whole_call_ms_min": round(min(whole), 3), "whole_call_ms_max": round(max(whole), 3),
           "untrimmed_call_ms_median": round(statistics.median(launch), 3), "untrimmed_call_ms_min": round(min(launch), 3),
           "untrimmed_call_ms_max": round(max(launch), 3), "us_per_frame": round(us / T, 4),
           "bytes": nbytes, "tb_per_s": round(nbytes / (us * 1e-6) / 1e12, 3), "hbm_peak_fraction": round(nbytes / (us * 1e-6) / HBM_PEAK, 4),
           "audio_seconds_per_second": round(B * a.seconds / (statistics.median(whole) * 1e-3), 0), "iters": a.iters, "warmup": a.warmup}
    if not a.no_cpu:
        c = cpu_ms(y_host, p, a.cpu_iters, a.threads)
        out.update({"cpu_float32_ms": round(c, 1), "cpu_threads": a.threads, "cpu_iters": a.cpu_iters,
                    "speedup_vs_cpu_untrimmed": round(c / statistics.median(launch), 1)})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
