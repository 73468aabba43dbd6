"""The float64 statement of the waveform-synthesis definitions (src/utils.py:281-328) that csrc/audio.hip is held to:
librosa's stft / istft at the reference's settings written out with numpy.fft, the Griffin-Lim iteration, scipy's lfilter for the
de-preemphasis and librosa.effects.trim in plain numpy.  Also the float32 CPU path (the same definitions through torch.stft / torch.istft in
float32) whose distance from this mirror is the yardstick of the GPU bounds, the test signal, and the metric.  No test functions.

Spectra are frame-major [T, 1 + n_fft/2]."""
from dataclasses import dataclass

import numpy as np
import torch
from scipy.signal import lfilter

EPS32 = float(np.finfo(np.float32).eps)
K = 8.0                                  # a GPU bound is K times the float32 CPU path's error on the same input


@dataclass(frozen=True)
class P:
    n_fft: int = 2048
    hop: int = 275
    win: int = 1102
    preemphasis: float = 0.97
    power: float = 1.2
    max_db: float = 100.0
    ref_db: float = 20.0
    n_iter: int = 60
    sr: int = 22050


DEFAULT = P()
SMALL = P(n_fft=256, hop=64, win=200)
MID = (P(n_fft=512, hop=128, win=400), P(n_fft=1024, hop=200, win=1024))     # the other two transform sizes; win = n_fft leaves no padding of the window
RAGGED = (5, 9, 40)                      # frame counts of the ragged batch; 5 is the reflection edge at the defaults (1100 samples, 1024 of padding)


def rel(a, b):
    """||a - b||_2 / ||b||_2 over one whole utterance."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def floor_(p):
    return EPS32 * np.log2(p.n_fft)


def window(p):
    """The periodic Hann window in float64 rounded to float32 (what the kernels read), as float64."""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(p.win, dtype=np.float64) / p.win)
    return w.astype(np.float32).astype(np.float64)


def padded_window(p):
    wp = np.zeros(p.n_fft)
    lpad = (p.n_fft - p.win) // 2
    wp[lpad:lpad + p.win] = window(p)
    return wp


def stft(y, p=DEFAULT):
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    assert n > p.n_fft // 2
    yp = np.pad(y, p.n_fft // 2, mode="reflect")
    T = 1 + n // p.hop
    wp = padded_window(p)
    frames = np.stack([wp * yp[t * p.hop:t * p.hop + p.n_fft] for t in range(T)])
    return np.fft.rfft(frames, axis=1)


def istft(S, p=DEFAULT):
    S = np.asarray(S, dtype=np.complex128)
    T = S.shape[0]
    wp = padded_window(p)
    f = wp[None, :] * np.fft.irfft(S, p.n_fft, axis=1)
    total = p.n_fft + p.hop * (T - 1)
    num, den = np.zeros(total), np.zeros(total)
    for t in range(T):
        num[t * p.hop:t * p.hop + p.n_fft] += f[t]
        den[t * p.hop:t * p.hop + p.n_fft] += wp * wp
    ok = den > np.finfo(np.float32).tiny
    num[ok] /= den[ok]
    return num[p.n_fft // 2:total - p.n_fft // 2]


def gl_step(X, M, p=DEFAULT):
    e = stft(istft(X, p), p)
    return M * e / np.maximum(1e-8, np.abs(e))


def griffin_lim(M, p=DEFAULT, n_iter=None, X0=None, return_state=False):
    M = np.asarray(M, dtype=np.float64)
    X = M.astype(np.complex128) if X0 is None else np.asarray(X0, dtype=np.complex128)
    for _ in range(p.n_iter if n_iter is None else n_iter):
        X = gl_step(X, M, p)
    return (istft(X, p), X) if return_state else istft(X, p)


def gl_prepare(mag, p=DEFAULT):
    mag = np.asarray(mag, dtype=np.float64)
    return (10.0 ** (0.05 * (np.clip(mag, 0, 1) * p.max_db - p.max_db + p.ref_db))) ** p.power


def deemphasis(y, coef=0.97):
    return lfilter([1.0], [1.0, -coef], np.asarray(y, dtype=np.float64))


def frame_db(y, frame_length=2048, hop_length=512, pad_mode="reflect"):
    """Per centred frame: 10 log10(max(1e-10, mean square)) relative to the loudest frame's."""
    y = np.asarray(y, dtype=np.float64)
    yp = np.pad(y, frame_length // 2, mode=pad_mode)
    nf = 1 + y.shape[0] // hop_length
    pw = np.array([np.mean(yp[i * hop_length:i * hop_length + frame_length] ** 2) for i in range(nf)])
    return 10.0 * np.log10(np.maximum(1e-10, pw)) - 10.0 * np.log10(np.maximum(1e-10, pw.max()))


def trim_bounds(y, top_db=60.0, frame_length=2048, hop_length=512, pad_mode="reflect"):
    db = frame_db(y, frame_length, hop_length, pad_mode)
    keep = np.flatnonzero(db > -top_db)
    if keep.size == 0:
        return 0, 0
    return int(keep[0]) * hop_length, min(len(y), (int(keep[-1]) + 1) * hop_length)


def spectrogram2wav(mag, p=DEFAULT, trim=True, pad_mode="reflect"):
    """(waveform float64 before the cast, (start, end))."""
    y = deemphasis(griffin_lim(gl_prepare(mag, p), p), p.preemphasis)
    s, e = trim_bounds(y, pad_mode=pad_mode) if trim else (0, len(y))
    return y[s:e], (s, e)


# ---- the float32 CPU path: the same definitions through torch's transforms in float32 -----------------------------------------------
def _twin(p, dtype):
    return torch.from_numpy(window(p)).to(dtype)


def torch_stft(y, p=DEFAULT, dtype=torch.float32):
    S = torch.stft(torch.as_tensor(y).to(dtype), p.n_fft, hop_length=p.hop, win_length=p.win, window=_twin(p, dtype), center=True,
                   pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    return S.transpose(0, 1)


def torch_istft(S, p=DEFAULT, dtype=torch.float32):
    cd = torch.complex64 if dtype == torch.float32 else torch.complex128
    S = torch.as_tensor(S).to(cd).transpose(0, 1)
    return torch.istft(S, p.n_fft, hop_length=p.hop, win_length=p.win, window=_twin(p, dtype), center=True, normalized=False, onesided=True,
                       length=p.hop * (S.shape[1] - 1))


def f32_gl_step(X, M, p=DEFAULT):
    e = torch_stft(torch_istft(X, p), p)
    return M * e / torch.clamp(e.abs(), min=1e-8)


def f32_griffin_lim(M, p=DEFAULT, n_iter=None, X0=None):
    M = M.to(torch.float32) if torch.is_tensor(M) else torch.from_numpy(np.array(M, dtype=np.float32))
    X = M.to(torch.complex64) if X0 is None else torch.from_numpy(np.array(X0, dtype=np.complex64))
    for _ in range(p.n_iter if n_iter is None else n_iter):
        X = f32_gl_step(X, M, p)
    return torch_istft(X, p)


def f32_spectrogram2wav(mag, p=DEFAULT):
    """The untrimmed float32 CPU waveform: de-normalisation and recurrence in float32 as well."""
    mag = torch.as_tensor(np.asarray(mag, dtype=np.float32))
    M = torch.pow(torch.pow(torch.tensor(10.0), 0.05 * (torch.clamp(mag, 0, 1) * p.max_db - p.max_db + p.ref_db)), p.power)
    y = f32_griffin_lim(M, p).numpy()
    return lfilter(np.array([1.0], dtype=np.float32), np.array([1.0, -p.preemphasis], dtype=np.float32), y).astype(np.float32)


# ---- test signals --------------------------------------------------------------------------------------------------------------------
def signal(n, seed=0, sr=22050, lead=0, tail=0):
    """A harmonic source with moving pitch under a slow envelope plus weak noise, 0.5 peak, with `lead` / `tail` silent samples inside n."""
    rng = np.random.default_rng(seed)
    m = n - lead - tail
    t = np.arange(m) / sr
    f0 = 140.0 + 40.0 * np.sin(2 * np.pi * 1.7 * t + seed) + 15.0 * np.sin(2 * np.pi * 0.45 * t)
    phase = 2 * np.pi * np.cumsum(f0) / sr
    x = sum(np.sin(h * phase + 0.3 * h) / h for h in range(1, 13))
    x *= 0.55 + 0.45 * np.sin(2 * np.pi * 2.3 * t + 0.5)
    x += 0.01 * rng.standard_normal(m)
    x *= 0.5 / np.abs(x).max()
    return np.concatenate([np.zeros(lead), x, np.zeros(tail)])


def utterance(T, p=DEFAULT, seed=0):
    """(signal of hop (T - 1) samples, its magnitude |stft| [T, bins])."""
    y = signal(p.hop * (T - 1), seed=seed, sr=p.sr)
    return y, np.abs(stft(y, p))


def normalised_mag(T, p=DEFAULT, seed=0):
    """A normalised magnitude in [0, 1] as the vocoder emits it (src/utils.py:272 applied to a real spectrum), float32 [T, bins], with a few
    entries pushed outside [0, 1] so that the clip matters."""
    _, M = utterance(T, p, seed)
    db = 20.0 * np.log10(np.maximum(1e-5, M / M.max() * 10.0))
    mag = (db - p.ref_db + p.max_db) / p.max_db
    mag[0, :4] = -0.25
    mag[-1, -4:] = 1.5
    return mag.astype(np.float32)


_CACHE = {}


def cached(key, fn):
    """Compute a reference once per session and share it (kept read-only)."""
    if key not in _CACHE:
        v = fn()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def trim_cases():
    """{name: signal}: silent margins of different lengths, silence on one side only, no silence, all silent (then every frame sits at the
    loudest frame's level and nothing is trimmed)."""
    return cached("trim_cases", lambda: {
        "margins": signal(12000, seed=3, lead=3000, tail=2500),
        "long_lead": signal(10725, seed=4, lead=5200, tail=700),
        "tail_only": signal(9000, seed=5, lead=0, tail=4000),
        "no_silence": signal(8000, seed=6),
        "all_silent": np.zeros(6000),
    })


def ragged_batch(p=DEFAULT):
    """[(signal, |stft|)] for the frame counts RAGGED."""
    return cached(("ragged", p), lambda: tuple(utterance(T, p, seed=T) for T in RAGGED))


def pad_mode_case():
    """A signal on which trim's two padding modes decide differently: a burst in the first 8 samples is mirrored into the frames that reach
    the left padding under 'reflect' (15 loud samples in the loudest frame) and not under 'constant' (8); the background lies 60 dB below a
    frame of 11 loud samples, 1.3 dB on either side of the threshold (the two modes differ by 10 log10(15 / 8) = 2.7 dB at most, so no such
    case can keep 3 dB; a float32 mean of 2048 squares errs by less than 2048 eps = 2.4e-4 relative, 1e-3 dB)."""
    z = np.full(4096, np.sqrt(1e-6 * 11 / 2048))
    z[:8] = 1.0
    return z
