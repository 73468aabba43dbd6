"""What fast Griffin-Lim (unast_amd.audio.griffinlim, unast_stft_momentum / unast_gl_random_phase of csrc/audio.hip) rests on, checked without
a GPU: the float64 mirror (tests/fast_griffin_lim_mirror.py) equals an independent statement through torch's float64 transforms and, without
momentum, the plain mirror; on the mirror the algorithm gets closer to the target magnitude than 60 plain iterations; the restated phase draw is
uniform and its four arguments all matter; the float32 CPU yardsticks of the GPU bounds; header, ops and the documents agree; every refusal
raises with its reason before anything is launched."""
import os
import re

import numpy as np
import pytest
import torch

from tests import fast_griffin_lim_mirror as F
from tests import griffin_lim_mirror as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"unast_stft_momentum": 15, "unast_gl_random_phase": 10}
CONVERGENCE_SEEDS = (0, 1, 2, 3, 4, 5)       # measured 0.067 0.078 0.095 0.081 0.068 0.059 against 0.118: at least 19 % to spare


def independent_griffinlim(M, p, n_iter, momentum, angles0):
    """librosa 0.8's loop written again, on torch.stft / torch.istft in float64 and torch's own complex arithmetic."""
    M = torch.from_numpy(np.array(M, dtype=np.float64))
    angles = torch.from_numpy(np.asarray(angles0, dtype=np.complex128))
    alpha = torch.tensor(np.float64(np.float32(momentum / (1 + momentum))))
    tprev = torch.zeros_like(angles)
    for _ in range(n_iter):
        rebuilt = G.torch_stft(G.torch_istft(M * angles, p, torch.float64), p, torch.float64)
        angles = rebuilt - alpha * tprev
        angles = angles / (angles.abs() + 1e-16)
        tprev = rebuilt
    return G.torch_istft(M * angles, p, torch.float64).numpy()


@pytest.mark.parametrize("pn", ["default", "small"])
@pytest.mark.parametrize("T", [5, 9, 40])
def test_mirror_equals_an_independent_float64_statement(pn, T):
    p = F.PARAM_SETS[pn]
    M = F.magnitude(T, p)
    a0 = F.random_angles(F.ANGLE_SEED, T, T, p)
    y = F.griffinlim(M, p, F.N_ITER, F.MOMENTUM, a0)
    ref = independent_griffinlim(M, p, F.N_ITER, F.MOMENTUM, a0)
    err = G.rel(y, ref)
    print("mirror against torch float64, %s T=%d, 32 iterations: rel %.3g" % (pn, T, err))
    assert y.shape == (p.hop * (T - 1),) and np.isfinite(y).all()
    assert err <= 1e-10


@pytest.mark.parametrize("T", [9, 40])
def test_mirror_without_momentum_is_the_plain_mirror(T):
    """momentum = 0 and angles0 = 1: the two normalisations, e / max(1e-8, |e|) and e / (|e| + 1e-16), differ only where |e| < 1e-8."""
    p = G.SMALL
    M = G.utterance(T, p, seed=T)[1]
    X, tprev, low = M.astype(np.complex128), np.zeros(M.shape, dtype=np.complex128), []
    for _ in range(8):
        X, tprev, _ = F.step(X, tprev, M, 0.0, p)
        low.append(np.abs(tprev).min())
    y = F.griffinlim(M, p, 8, 0.0, None)
    err = G.rel(y, G.griffin_lim(M, p, 8))
    print("momentum 0 against the plain mirror, small T=%d: rel %.3g, min |e| %.3g" % (T, err, min(low)))
    assert min(low) >= 1e-6
    assert err <= 1e-12
    assert np.array_equal(y, G.istft(X, p)) and F.alpha_of(0.0) == 0.0


def test_momentum_converges_below_sixty_plain_iterations():
    """Defaults, T = 40: 32 momentum iterations from the restated random phases against the 60 plain iterations of src/utils.py:309-320."""
    p = G.DEFAULT
    _, M = G.utterance(40, p, seed=40)
    plain60 = F.spectral_convergence(G.griffin_lim(M, p), M, p)
    plain32 = F.spectral_convergence(G.griffin_lim(M, p, 32), M, p)
    print("spectral convergence, mirror: plain 60 iterations %.4f, plain 32 iterations %.4f" % (plain60, plain32))
    assert abs(plain60 - 0.1180) < 5e-4
    for seed in CONVERGENCE_SEEDS:
        sc = F.spectral_convergence(F.griffinlim(M, p, F.N_ITER, F.MOMENTUM, F.random_angles(seed, 0, 40, p)), M, p)
        print("    momentum 32 iterations, seed %d: %.4f (%.1f %% below)" % (seed, sc, 100 * (1 - sc / plain60)))
        assert sc <= 0.95 * plain60


def resultant(d, n_fft):
    return float(np.abs(np.exp(2j * np.pi * np.asarray(d, dtype=np.float64) / n_fft).mean()))


@pytest.mark.parametrize("seed,key", [(0, 0), (1, 0), (F.SEED, 2), (12345, 4000000000)])
def test_phase_table_is_uniform_and_every_argument_matters(seed, key):
    """The mean resultant length of n uniform phases exceeds 4 / sqrt(n) with probability about exp(-16)."""
    T, n_fft = 40, 2048
    m = F.phase_index(seed, key, T, n_fft)
    assert m.shape == (T, 1025) and m.min() >= 0 and m.max() < n_fft
    figures = {"table": resultant(m, n_fft),
               "neighbouring bins": resultant(m[:, 1:] - m[:, :-1], n_fft),
               "neighbouring frames": resultant(m[1:] - m[:-1], n_fft),
               "seed + 1": resultant(F.phase_index(seed + 1, key, T, n_fft) - m, n_fft),
               "key + 1": resultant(F.phase_index(seed, (key + 1) & 0xFFFFFFFF, T, n_fft) - m, n_fft)}
    for name, r in figures.items():
        n = m.size if name in ("table", "seed + 1", "key + 1") else (m[:, 1:].size if name == "neighbouring bins" else m[1:].size)
        print("phase table seed %d key %d, %s: resultant %.4f, bound %.4f" % (seed, key, name, r, 4 / np.sqrt(n)))
        assert r <= 4 / np.sqrt(n), name
    assert len(np.unique(m)) == n_fft, "every level occurs among 41 000 draws"
    a0 = F.random_angles(seed, key, T, G.DEFAULT)
    assert a0.dtype == np.complex64 and np.abs(np.abs(a0) - 1).max() <= 2 * G.EPS32


def test_phase_hash_known_values():
    """h written out by hand for a few arguments, from dropout_mirror's pcg_hash (whose literal values test_cpu_dropout_mirror.py pins)."""
    from tests.dropout_mirror import pcg_hash
    for seed, key, t, k in ((0, 0, 0, 0), (3, 2, 39, 1024), (0xFFFFFFFF, 0xFFFFFFFF, 7, 5)):
        want = int(pcg_hash((k + int(pcg_hash((t + int(pcg_hash((key + int(pcg_hash(seed))) % 2**32))) % 2**32))) % 2**32))
        assert int(F.phase_hash(seed, key, t, k)) == want
        assert int(F.phase_index(seed, key, t + 1, 2048)[t, k]) == want % 2048
    tw = F.twiddle(2048)
    assert tw[0] == 1 and tw[512].imag == -1 and tw[1024].real == -1 and tw[1].imag < 0, "exp(-2 pi i m / n_fft)"


def test_yardsticks():
    """The float32 CPU path against the mirror in the cases the GPU tests use: the figures their bounds are multiples of."""
    alpha = F.alpha_of(F.MOMENTUM)
    assert alpha == float(np.float32(0.99 / 1.99)) and 0.497 < alpha < 0.498
    for pn, Ts in (("default", G.RAGGED), ("small", G.RAGGED), ("512", (9,)), ("1024", (9,))):
        p = F.PARAM_SETS[pn]
        for T in Ts:
            M, X, tprev, X1, e1, c1 = F.state10(T, p)
            Xf, ef = F.f32_step(torch.from_numpy(X.copy()), torch.from_numpy(tprev.copy()), torch.from_numpy(M.astype(np.float32)), alpha, p)
            y_e, y_x, y_w = G.rel(ef.numpy(), e1), G.rel(Xf.numpy(), X1), F.wrel(Xf.numpy(), X1, F.weight(c1))
            print("one momentum pass %s T=%d, float32 CPU: rebuilt spectrum %.3g, new iterate %.3g plain / %.3g weighted" % (pn, T, y_e, y_x, y_w))
            assert y_e < 10 * 1.5e-7 and y_w < 10 * 2.2e-7
    for pn in ("default", "small"):
        p = F.PARAM_SETS[pn]
        for T in G.RAGGED:
            M, a0, y32 = F.run32(T, p)
            yard = G.rel(F.f32_griffinlim(M, p, F.N_ITER, F.MOMENTUM, a0).numpy(), y32)
            print("32 iterations %s T=%d, float32 CPU: %.3g" % (pn, T, yard))
            # the growth of a rounding error through 32 iterations depends on the start: 5e-6 to 1.3e-3 over the starts tried (a bin whose c
            # nearly cancels in some iteration turns its phase); float32 must still follow the mirror to a percent
            assert yard < 1e-2 and np.isfinite(y32).all() and np.abs(y32).max() > 0.01


@pytest.mark.parametrize("which", ["given angles0", "seeded"])
def test_the_thirty_two_iteration_starts_are_stable_in_float32(which):
    """The input condition of the GPU tests of whole runs: from the chosen starts the float32 CPU path moved by one ulp stays within K of
    itself, so that K times one such run is a bound a float32 implementation can be held to (seed 7 would not do: 89 at the defaults, T = 40)."""
    for pn in ("default", "small"):
        p = F.PARAM_SETS[pn]
        for T, key in zip(G.RAGGED, F.SEEDED_KEYS):
            seed, key = (F.ANGLE_SEED, T) if which == "given angles0" else (F.SEED, key)
            lo, hi = F.f32_spread(F.magnitude(T, p), F.random_angles(seed, key, T, p), p)
            print("float32 CPU, %s, %s T=%d seed %d key %d: %.3g .. %.3g from the mirror over 4 runs one ulp apart, ratio %.1f" % (which, pn, T, seed, key, lo, hi, hi / lo))
            assert hi <= G.K * lo


def test_header_ops_and_documents_agree():
    from unast_amd import audio, ops, utils
    from unast_amd._lib import parse_header
    protos = parse_header()
    assert {k: len(protos[k][1]) for k in ENTRIES} == ENTRIES
    src = open(os.path.join(ROOT, "unast_amd", "csrc", "audio.hip")).read()
    for k in ENTRIES:
        assert re.search(r'extern "C" int %s\(' % k, src), k
    for name in ("stft_momentum", "gl_random_phase"):
        assert callable(getattr(ops, name))
    assert len(re.findall(r"void stft_kernel\(", src)) == 1 and "stft_kernel<true>" in src and "stft_kernel<false>" in src, "one kernel body, two epilogues"
    n = len(protos)
    for doc, pat in (("README.md", r"the C ABI \((\d+) entry points\)"), ("INTEGRATION.md", r"for every entry point \((\d+)\)")):
        m = re.search(pat, open(os.path.join(ROOT, doc)).read())
        assert m and int(m.group(1)) == n, (doc, m and m.group(1), n)
    assert utils.griffinlim is audio.griffinlim
    assert (audio.LIBROSA_N_ITER, audio.LIBROSA_MOMENTUM) == (F.N_ITER, F.MOMENTUM) == (32, 0.99)
    assert audio._alpha(0.99) == F.alpha_of(0.99) and audio._alpha(0.0) == 0.0
    for doc in ("DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "not pinnable" not in text and "no test could pin" not in text, doc
    assert "is not built" not in audio.__doc__.split("feature extraction")[0]


def test_refusals_come_before_any_launch():
    """On CPU tensors: each refusal names its reason (a launch would have raised TypeError for the device first)."""
    from unast_amd import audio
    A = audio.AudioParams
    ok = torch.zeros(2, 6, 1025)
    for m in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="momentum must lie in \\[0, 1\\)"):
            audio.griffinlim(ok, momentum=m)
    with pytest.raises(ValueError, match="init is 'random' or None"):
        audio.griffinlim(ok, init="zeros")
    with pytest.raises(ValueError, match="n_iter"):
        audio.griffinlim(ok, n_iter=-1)
    with pytest.raises(ValueError, match="seed must fit 32 bits"):
        audio.griffinlim(ok, seed=1 << 32)
    with pytest.raises(ValueError, match="2 utterances, 3 keys"):
        audio.griffinlim(ok, keys=[0, 1, 2])
    with pytest.raises(ValueError, match="key must fit 32 bits"):
        audio.griffinlim(ok, keys=[0, -1])
    with pytest.raises(ValueError, match="angles0 and S differ in shape"):
        audio.griffinlim(ok, angles0=torch.zeros(2, 5, 1025, dtype=torch.complex64))
    with pytest.raises(TypeError, match="complex64 tensor is needed"):
        audio.griffinlim(ok, angles0=torch.zeros(2, 6, 1025))
    with pytest.raises(TypeError, match="float32 tensor is needed"):
        audio.griffinlim(ok.to(torch.complex64))
    # everything griffin_lim refuses
    with pytest.raises(ValueError, match="last dimension"):
        audio.griffinlim(torch.zeros(6, 1024))
    with pytest.raises(ValueError, match="too short"):
        audio.griffinlim(torch.zeros(4, 1025))
    with pytest.raises(ValueError, match="beyond the 6 frames"):
        audio.griffinlim(ok, [6, 7])
    with pytest.raises(ValueError, match="2 utterances, 1 lengths"):
        audio.griffinlim(ok, [6])
    with pytest.raises(ValueError, match="n_fft must be one of"):
        audio.griffinlim(torch.zeros(40, 151), None, A(n_fft=300, hop=32, win=100))
    with pytest.raises(ValueError, match="win must not exceed n_fft"):
        audio.griffinlim(torch.zeros(40, 129), None, A(n_fft=256, hop=64, win=300))
    # the callers
    for call in (lambda **kw: audio.spectrogram2wav_batch(ok, [6, 6], **kw),
                 lambda **kw: audio.spectrogram2wav(np.zeros((6, 1025), np.float32), **kw),
                 lambda **kw: audio.mel2wav(None, None, [6], **kw),
                 lambda **kw: audio.vocode([], "/nonexistent", "/nonexistent", **kw)):
        with pytest.raises(ValueError, match="method is 'reference'.*or 'librosa'"):
            call(method="fast")
        with pytest.raises(ValueError, match="seed must fit 32 bits"):
            call(method="librosa", seed=-1)
    with pytest.raises(ValueError, match="2 utterances, 1 keys"):
        audio.spectrogram2wav_batch(ok, [6, 6], method="librosa", keys=[5])


def test_nothing_runs_without_a_gpu():
    from unast_amd import audio, ops
    ok = torch.zeros(2, 6, 1025)
    for kw in ({}, {"init": None}, {"angles0": torch.ones(2, 6, 1025, dtype=torch.complex64)}, {"n_iter": 0}):
        with pytest.raises(TypeError, match="CUDA"):
            audio.griffinlim(ok, **kw)
    with pytest.raises(TypeError, match="CUDA"):
        audio.spectrogram2wav_batch(ok, [6, 5], method="librosa")
    i32, c64 = torch.zeros(1, dtype=torch.int32), torch.zeros(1, 6, 1025, dtype=torch.complex64)
    w, tw = torch.zeros(1102), torch.zeros(2048, dtype=torch.complex64)
    for call in (lambda: ops.stft_momentum(torch.zeros(1, 1375), i32, 6, 2048, 275, 1102, w, tw, c64, torch.zeros(1, 6, 1025), 0.25, c64.clone()),
                 lambda: ops.gl_random_phase(torch.zeros(1, 6, 1025), i32, i32, 0, 2048, tw, c64)):
        with pytest.raises(TypeError, match="CUDA"):
            call()
    with pytest.raises(ValueError, match="n_fft must be one of"):
        ops.stft_momentum(torch.zeros(1, 1375), i32, 6, 300, 275, 200, w, tw, c64, torch.zeros(1, 6, 1025), 0.25, c64.clone())
