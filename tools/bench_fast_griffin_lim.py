#!/usr/bin/env python3
"""Fast Griffin-Lim (unast_amd.audio.griffinlim, method='librosa' of spectrogram2wav_batch) against the deterministic
path at B=32, T=800 and B=1, T=800 on one GPU, by tools/bench_griffin_lim.py's convention (HIP events on one stream, --warmup calls, medians of
--iters): the whole spectrogram2wav_batch call with method='librosa' (32 iterations) and method='reference' (60), one momentum iteration
against one plain iteration (a run of iterations between two events, divided by iterations + 0.5 for the closing inverse transform), the
momentum forward-transform launch against the plain one (events around every launch of a further run) and the random-phase launch.
Bytes per frame: the plain iteration's as tools/bench_griffin_lim.py counts them, plus tprev read and written (2 x 8 bytes x bins).
Prints one JSON line per batch size.  Usage: python tools/bench_fast_griffin_lim.py [--frames 800] [--warmup 2] [--iters 7]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unast_amd import audio, ops  # noqa: E402


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed_ms(fn, a):
    out = []
    for i in range(a.warmup + a.iters):
        e0, e1 = events()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            out.append(e0.elapsed_time(e1))
    return out


def launch_split(fn, names):
    """Median microseconds per launch of the ops named, over one run of fn with events around each of them."""
    records = []

    def timed(f, name):
        def wrapper(*args, **kw):
            e0, e1 = events()
            e0.record()
            r = f(*args, **kw)
            e1.record()
            records.append((name, e0, e1))
            return r
        return wrapper
    saved = {n: getattr(ops, n) for n in names}
    for n, f in saved.items():
        setattr(ops, n, timed(f, n))
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)
    split = {}
    for name, e0, e1 in records:
        split.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
    return {k: round(statistics.median(v), 1) for k, v in split.items()}


def run(B, T, a):
    dev = torch.device("cuda:0")
    p = audio.AudioParams()
    g = torch.Generator().manual_seed(B)
    mags = (0.35 + 0.5 * torch.rand(B, T, p.bins, generator=g)).to(dev)
    lens = [T] * B
    total = {m: timed_ms(lambda m=m: audio.spectrogram2wav_batch(mags, lens, p, method=m), a) for m in audio.GL_METHODS}
    M = torch.empty(B, T, p.bins, device=dev)
    ops.gl_prepare(mags, p.max_db, p.ref_db, p.power, M)
    n_fast = audio.LIBROSA_N_ITER
    plain = [t / (p.n_iter + 0.5) * 1e3 for t in timed_ms(lambda: audio.griffin_lim(M, lens, p), a)]
    # init=None: the loop alone, without the random-phase launch (timed on its own below)
    fast = [t / (n_fast + 0.5) * 1e3 for t in timed_ms(lambda: audio.griffinlim(M, lens, p, init=None), a)]
    names = ("istft_frames", "overlap_add", "stft", "stft_momentum")
    split_plain = launch_split(lambda: audio.griffin_lim(M, lens, p), names)
    split_fast = launch_split(lambda: audio.griffinlim(M, lens, p, init=None), names)
    X = torch.empty(B, T, p.bins, dtype=torch.complex64, device=dev)
    frames_dev = audio._i32(lens, dev)
    phase = [t * 1e3 for t in timed_ms(lambda: audio._random_phase(M, X, frames_dev, list(range(B)), 0, p), a)]
    per_frame_plain = 2 * 8 * p.bins + 2 * 4 * p.win + 4 * p.bins + 2 * 4 * p.hop
    per_frame_fast = per_frame_plain + 2 * 8 * p.bins
    med = statistics.median
    out = {"workload": "spectrogram2wav_batch librosa vs reference", "batch": B, "frames": T, "n_iter": {"librosa": n_fast, "reference": p.n_iter},
           "total_ms_median": {m: round(med(v), 3) for m, v in total.items()},
           "total_ms_min_max": {m: [round(min(v), 3), round(max(v), 3)] for m, v in total.items()},
           "iteration_us_median": {"momentum": round(med(fast), 1), "plain": round(med(plain), 1)},
           "iteration_us_min_max": {"momentum": [round(min(fast), 1), round(max(fast), 1)], "plain": [round(min(plain), 1), round(max(plain), 1)]},
           "iteration_ratio": round(med(fast) / med(plain), 3),
           "kernel_us_median": {"momentum": split_fast, "plain": split_plain},
           "gl_random_phase_us_median": round(med(phase), 1), "gl_random_phase_us_min_max": [round(min(phase), 1), round(max(phase), 1)],
           "bytes_per_frame": {"momentum": per_frame_fast, "plain": per_frame_plain}, "bytes_ratio": round(per_frame_fast / per_frame_plain, 3),
           "iters": a.iters, "warmup": a.warmup}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fast_griffin_lim.py measures on a GPU; none found")
    for B in (32, 1):
        run(B, a.frames, a)


if __name__ == "__main__":
    main()
