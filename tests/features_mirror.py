"""The float64 statement of the feature-extraction definitions (src/utils.py:235-278, get_spectrograms) that the features
kernel of csrc/audio.hip is held to, on top of tests/griffin_lim_mirror.py (its stft, trim_bounds, signal and K): numpy's float32 preemphasis,
librosa.filters.mel at its defaults written out, |S|, the mel projection, dB, normalise, clip.  Also the float32 CPU path (torch.stft in
float32, a float32 matmul with the basis, torch.log10) whose distance from this mirror is the yardstick of the GPU bounds, the cases and the
metric.  No test functions.

Spectrograms are frame-major: mel [T, n_mels], mag [T, 1 + n_fft/2]."""
from dataclasses import dataclass

import numpy as np
import torch

from tests import griffin_lim_mirror as G

K = G.K
LOW = float(np.float32(1e-8))            # the lower clip as the device stores it


@dataclass(frozen=True)
class P(G.P):
    n_mels: int = 80


DEFAULT = P()
SMALL = P(n_fft=256, hop=64, win=200, n_mels=20)
SMALL80 = P(n_fft=256, hop=64, win=200, n_mels=80)       # two empty filters
PARAMS = {"default": DEFAULT, "small": SMALL}


def floor_(p):
    """What a relative magnitude error of eps32 * log2(n_fft) moves a normalised value by: d/dx of 20 log10(x) / max_db is 20 / (max_db ln 10 x)."""
    return 20.0 / (p.max_db * np.log(10.0)) * G.EPS32 * np.log2(p.n_fft)


def rms(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.sqrt(np.mean((a - b) ** 2)))


def frames_of(n, p):
    return 1 + n // p.hop


# ---- the definitions ------------------------------------------------------------------------------------------------------------------
def preemphasis(y, coef=0.97):
    """src/utils.py:251 on a float32 array, exactly as numpy does it: one float32 multiply, one float32 subtract."""
    y = np.asarray(y, dtype=np.float32)
    return np.append(y[0], y[1:] - np.float32(coef) * y[:-1]).astype(np.float32)


def hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f < 1000.0, f / (200.0 / 3.0), 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0))


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m < 15.0, m * (200.0 / 3.0), 1000.0 * np.exp((m - 15.0) * (np.log(6.4) / 27.0)))


def mel_edges(p):
    return mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(p.sr / 2.0), p.n_mels + 2))


def mel_basis64(p):
    """librosa.filters.mel(sr, n_fft, n_mels) at its defaults (fmin 0, fmax sr/2, Slaney scale and norm) in float64, [n_mels, 1 + n_fft/2]."""
    f = np.arange(p.n_fft // 2 + 1, dtype=np.float64) * p.sr / p.n_fft
    m = mel_edges(p)
    W = np.zeros((p.n_mels, f.shape[0]))
    for i in range(p.n_mels):
        lower = (f - m[i]) / (m[i + 1] - m[i])
        upper = (m[i + 2] - f) / (m[i + 2] - m[i + 1])
        W[i] = np.maximum(0.0, np.minimum(lower, upper)) * 2.0 / (m[i + 2] - m[i])
    return W


def ranges_of(W):
    """int32 [n_mels, 2]: [lo, hi) of each row's nonzeros, (0, 0) for an empty row."""
    r = np.zeros((W.shape[0], 2), dtype=np.int32)
    for i, row in enumerate(W):
        nz = np.flatnonzero(row)
        if nz.size:
            r[i] = (nz[0], nz[-1] + 1)
    return r


def mel_basis(p):
    """(W float32 [n_mels, bins], ranges int32 [n_mels, 2]): the float64 basis rounded once."""
    def make():
        W = mel_basis64(p).astype(np.float32)
        return W, ranges_of(W)
    return G.cached(("mel_basis", p), make)


def normalise(x, p):
    return np.clip((20.0 * np.log10(np.maximum(1e-5, x)) - p.ref_db + p.max_db) / p.max_db, 1e-8, 1.0)


def features(y, p=DEFAULT):
    """(mel [T, n_mels], mag [T, bins], |S| [T, bins]) in float64 for an already trimmed float32 waveform y."""
    e = preemphasis(y, p.preemphasis).astype(np.float64)
    A = np.abs(G.stft(e, p))
    W, _ = mel_basis(p)
    return normalise(A @ W.astype(np.float64).T, p), normalise(A, p), A


def f32_features(y, p=DEFAULT):
    """The float32 CPU path: (mel, mag) float32 numpy."""
    e = torch.from_numpy(preemphasis(y, p.preemphasis))
    A = G.torch_stft(e, p).abs()
    W, _ = mel_basis(p)

    def norm(x):
        return torch.clamp((20.0 * torch.log10(torch.clamp(x, min=1e-5)) - p.ref_db + p.max_db) / p.max_db, 1e-8, 1.0)
    return norm(A @ torch.tensor(W).t()).numpy(), norm(A).numpy()


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def counts(p):
    """The smallest legal count, n % hop == 0, n % hop == hop - 1, a long odd count."""
    return (p.n_fft // 2 + 1, p.hop * 8, p.hop * 9 - 1, p.hop * 39 + 17)


# name: (scale of G.signal, amplitude of a 5 kHz tone added to it).  "plain": nothing clipped; "quiet": mel and mag reach the lower clip;
# "tone": mag reaches the upper clip; "loud": mel reaches the upper clip as well (a waveform far beyond [-1, 1]: the arithmetic does not care).
SIGNALS = {"plain": (1.0, 0.0), "quiet": (0.02, 0.0), "tone": (1.0, 0.4), "loud": (50.0, 0.0)}
# Under the small parameter set the quiet signal leaves 64 .. 79 % of the mel entries on the lower clip, and a filter there sums at most 0.0116 of
# weight, so mel reaches the upper clip only at scales (about 1000) that put 95 % of mag on it: neither is an accuracy case
# (tests/test_cpu_features.py checks that every case listed here keeps at least half of its entries strictly inside the clips).
SKIP = {("small", "quiet"), ("small", "loud")}


def make_signal(name, n, p, seed):
    scale, tone = SIGNALS[name]
    y = scale * G.signal(n, seed=seed, sr=p.sr)
    if tone:
        y = y + tone * np.sin(2.0 * np.pi * 5000.0 * np.arange(n) / p.sr)
    return y.astype(np.float32)


def accuracy_cases(pn):
    """[(signal name, [float32 waveforms, one per count])] for a parameter set."""
    p = PARAMS[pn]
    return G.cached(("feat_cases", pn), lambda: tuple(
        (name, tuple(make_signal(name, n, p, seed=11 + i) for i, n in enumerate(counts(p)))) for name in SIGNALS if (pn, name) not in SKIP))


def reference(pn, name, i):
    """(mirror mel, mirror mag, float32 CPU mel, float32 CPU mag) of accuracy case (pn, name, i), computed once."""
    def make():
        y = dict(accuracy_cases(pn))[name][i]
        mel, mag, _ = features(y, PARAMS[pn])
        fm, fg = f32_features(y, PARAMS[pn])
        return mel, mag, fm, fg
    return G.cached(("feat_ref", pn, name, i), make)


def inside(v):
    """The share of entries strictly inside (1e-8, 1)."""
    return float(np.mean((v > 1e-8) & (v < 1.0)))


def trim_batch():
    """G.trim_cases() as float32: (names, [waveforms])."""
    cases = G.trim_cases()
    return list(cases), [cases[k].astype(np.float32) for k in cases]
