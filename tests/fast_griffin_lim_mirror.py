"""The float64 statement of fast Griffin-Lim (librosa.griffinlim as src/gl_vocoder.py:26 calls it) that
unast_stft_momentum and unast_gl_random_phase of csrc/audio.hip are held to, on top of tests/griffin_lim_mirror.py's stft / istft:

    alpha = float32(momentum / (1 + momentum));  ang = angles0;  tprev = 0
    n_iter times:  e = stft(istft(M * ang));  c = e - alpha * tprev;  tprev = e;  ang = c / (|c| + 1e-16)
    result = istft(M * ang)

Also the float32 CPU path (the same loop through G.torch_stft / G.torch_istft, alpha as float32) whose distance from the mirror is the
yardstick of the GPU bounds, the numpy restatement of the kernels' phase draw

    m = pcg(k + pcg(t + pcg(key + pcg(seed)))) & (n_fft - 1),   angles0[t, k] = tw[m],  tw[m] = complex64(exp(-2 pi i m / n_fft))

and the weighted metric of the new iterate.  No test functions.  Spectra are frame-major [T, 1 + n_fft/2]."""
import numpy as np
import torch

from tests import griffin_lim_mirror as G
from tests.dropout_mirror import pcg_hash

N_ITER, MOMENTUM = 32, 0.99              # librosa.griffinlim's defaults
TINY = 1e-16


def alpha_of(momentum):
    """momentum / (1 + momentum) in double, rounded to float32, as a Python float."""
    return float(np.float32(momentum / (1.0 + momentum)))


def step(X, tprev, M, alpha, p=G.DEFAULT):
    """One iteration from the iterate X = M * ang and the previous rebuilt spectrum: (new X, e, c)."""
    e = G.stft(G.istft(X, p), p)
    c = e - alpha * np.asarray(tprev, dtype=np.complex128)
    return M * (c / (np.abs(c) + TINY)), e, c


def griffinlim(M, p=G.DEFAULT, n_iter=N_ITER, momentum=MOMENTUM, angles0=None, return_state=False):
    """angles0 None: all phases zero.  return_state: (waveform, X, tprev, c) with c the last iteration's e - alpha tprev (None without one)."""
    M = np.asarray(M, dtype=np.float64)
    alpha = alpha_of(momentum)
    X = M.astype(np.complex128) if angles0 is None else M * np.asarray(angles0, dtype=np.complex128)
    tprev, c = np.zeros_like(X), None
    for _ in range(n_iter):
        X, tprev, c = step(X, tprev, M, alpha, p)
    y = G.istft(X, p)
    return (y, X, tprev, c) if return_state else y


# ---- the float32 CPU path ------------------------------------------------------------------------------------------------------------
def f32_step(X, tprev, M, alpha, p=G.DEFAULT):
    """X, tprev complex64 tensors, M float32 tensor, alpha a Python float holding a float32 value: (new X, e)."""
    e = G.torch_stft(G.torch_istft(X, p), p)
    c = e - torch.tensor(alpha, dtype=torch.float32) * tprev
    return M * (c / (c.abs() + torch.tensor(TINY, dtype=torch.float32))), e


def f32_griffinlim(M, p=G.DEFAULT, n_iter=N_ITER, momentum=MOMENTUM, angles0=None):
    M = torch.from_numpy(np.array(M, dtype=np.float32))
    alpha = alpha_of(momentum)
    X = M.to(torch.complex64) if angles0 is None else M * torch.from_numpy(np.array(angles0, dtype=np.complex64))
    tprev = torch.zeros_like(X)
    for _ in range(n_iter):
        X, tprev = f32_step(X, tprev, M, alpha, p)
    return G.torch_istft(X, p)


def f32_spread(M, angles0, p=G.DEFAULT, runs=3):
    """The float32 CPU path from X0 = M * angles0 and from `runs` copies of X0 with every component moved by -1, 0 or +1 ulp: (smallest,
    largest) distance of the 32-iteration waveforms from the mirror's.  Their ratio is how far rounding alone moves a float32 result."""
    y = griffinlim(M, p, N_ITER, MOMENTUM, angles0)
    Mf = np.asarray(M, dtype=np.float32)
    a0 = np.asarray(angles0, dtype=np.complex64)
    X0 = np.empty(a0.shape, dtype=np.complex64)
    X0.real, X0.imag = Mf * a0.real, Mf * a0.imag
    alpha, errs = alpha_of(MOMENTUM), []
    for r in range(runs + 1):
        v = X0.view(np.float32).copy()
        if r:
            d = np.random.default_rng(r - 1).integers(-1, 2, v.shape)
            v = np.where(d > 0, np.nextafter(v, np.float32(np.inf)), np.where(d < 0, np.nextafter(v, np.float32(-np.inf)), v)).astype(np.float32)
        X = torch.from_numpy(v.view(np.complex64))
        tprev = torch.zeros_like(X)
        for _ in range(N_ITER):
            X, tprev = f32_step(X, tprev, torch.from_numpy(Mf), alpha, p)
        errs.append(G.rel(G.torch_istft(X, p).numpy(), y))
    return min(errs), max(errs)


# ---- the random phase ----------------------------------------------------------------------------------------------------------------
def phase_hash(seed, key, t, k):
    """h(seed, key, t, k) of csrc/audio.hip (gl_phase_hash) in uint32 arithmetic; the arguments broadcast."""
    u = np.uint64
    m32 = u(0xFFFFFFFF)
    a = pcg_hash(np.asarray(seed, dtype=u))
    a = pcg_hash((np.asarray(key, dtype=u) + a) & m32)
    a = pcg_hash((np.asarray(t, dtype=u) + a) & m32)
    return pcg_hash((np.asarray(k, dtype=u) + a) & m32)


def phase_index(seed, key, T, n_fft):
    """m [T, 1 + n_fft/2] int64 in 0..n_fft-1."""
    t = np.arange(T, dtype=np.uint64)[:, None]
    k = np.arange(n_fft // 2 + 1, dtype=np.uint64)[None, :]
    return (phase_hash(seed, key, t, k) & np.uint64(n_fft - 1)).astype(np.int64)


def twiddle(n_fft):
    """exp(-2 pi i m / n_fft) in float64 rounded once to complex64: the table the kernels read (unast_amd.audio._tables)."""
    ang = -2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft
    return (np.cos(ang) + 1j * np.sin(ang)).astype(np.complex64)


def random_angles(seed, key, T, p=G.DEFAULT):
    """angles0 [T, bins] complex64."""
    return twiddle(p.n_fft)[phase_index(seed, key, T, p.n_fft)]


# ---- metrics -------------------------------------------------------------------------------------------------------------------------
def weight(c):
    """w = min(1, |c| / median |c|): a phase c / |c| is ill-conditioned in any float32 arithmetic where c nearly cancels."""
    a = np.abs(c)
    return np.minimum(1.0, a / np.median(a))


def wrel(a, b, w):
    """||(a - b) w|| / ||b w|| over one whole utterance; no bin is left out."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape == w.shape, (a.shape, b.shape, w.shape)
    return float(np.linalg.norm(((a - b) * w).ravel()) / np.linalg.norm((b * w).ravel()))


def spectral_convergence(y, M, p=G.DEFAULT):
    """||abs(stft(y)) - M|| / ||M||."""
    return float(np.linalg.norm(np.abs(G.stft(np.asarray(y, dtype=np.float64), p)) - M) / np.linalg.norm(M))


# ---- shared references ---------------------------------------------------------------------------------------------------------------
PARAM_SETS = {"default": G.DEFAULT, "small": G.SMALL, "512": G.MID[0], "1024": G.MID[1]}
# Seeds of the angles0 the arithmetic tests start from (an utterance's key is its frame count) and of the end-to-end tests (SEEDED_KEYS).
# A 32-iteration run can be held to the K rule only from a start on which float32 itself is stable: where one bin's c nearly cancels, its
# phase is decided by rounding, and the float32 CPU path started one ulp away ends up to 90 times
# further from the mirror (seed 7, defaults, T = 40: 1.0e-5 .. 9.3e-4 over four such runs).  f32_spread measures that; each seed below is the
# first of 0, 1, 2, ... whose spread stays below K at all six utterances (6: at most 4.5; 1: at most 3.5; tests/test_cpu_fast_griffin_lim.py).
ANGLE_SEED, SEED = 6, 1
SEEDED_KEYS = (11, 0, 4000000000)        # the keys of the ragged batch's utterances in the end-to-end tests


def magnitude(T, p):
    """The generator's utterance of T frames, its magnitude rounded to float32 (what the device reads), as float64."""
    return G.cached(("fgl_M", T, p), lambda: G.utterance(T, p, seed=T)[1].astype(np.float32).astype(np.float64))


def state10(T, p):
    """The mirror after 10 iterations from the restated random phases (seed ANGLE_SEED, key T): (M, X, tprev) with X and tprev rounded to
    complex64, and one further mirror iteration from exactly that state: (X', e', c')."""
    def make():
        M = magnitude(T, p)
        _, X, tprev, _ = griffinlim(M, p, 10, MOMENTUM, random_angles(ANGLE_SEED, T, T, p), return_state=True)
        X, tprev = X.astype(np.complex64), tprev.astype(np.complex64)
        return (M, X, tprev) + step(X, tprev, M, alpha_of(MOMENTUM), p)
    return G.cached(("fgl_state10", T, p), make)


def run32(T, p, seed=ANGLE_SEED, key=None):
    """(M, angles0 complex64, the mirror's 32-iteration waveform) from the restated phases of (seed, key); key defaults to T."""
    key = T if key is None else key

    def make():
        M = magnitude(T, p)
        a0 = random_angles(seed, key, T, p)
        return M, a0, griffinlim(M, p, N_ITER, MOMENTUM, a0)
    return G.cached(("fgl_run32", T, p, seed, key), make)
