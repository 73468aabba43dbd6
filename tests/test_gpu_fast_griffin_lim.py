"""GPU tests of fast Griffin-Lim (unast_amd.audio.griffinlim; unast_stft_momentum and unast_gl_random_phase of csrc/audio.hip) against the
float64 mirror (tests/fast_griffin_lim_mirror.py).  Bounds follow DESIGN.md section 5q's rule: K = 8 times the float32 CPU path's error on the
same input (the same loop through torch.stft / torch.istft in float32), floored at eps32 * log2(n_fft).  The new iterate is compared under the
weighted metric ||(a - b) w|| / ||b w||, w = min(1, |c| / median |c|) from the mirror: where c = e - alpha tprev nearly cancels, its phase is
ill-conditioned in any float32 arithmetic; no bin is left out.  Every figure is printed before it is asserted; DESIGN.md section 5s records them."""
import os
import wave

import numpy as np
import pytest
import torch

from tests import fast_griffin_lim_mirror as F
from tests import griffin_lim_mirror as G

pytestmark = pytest.mark.gpu

ALPHA = F.alpha_of(F.MOMENTUM)
ONE_PASS = {"default": G.RAGGED, "small": G.RAGGED, "512": (9,), "1024": (9,)}


def dev():
    return torch.device("cuda:0")


def ap(p):
    from unast_amd.audio import AudioParams
    return AudioParams(n_fft=p.n_fft, hop=p.hop, win=p.win, preemphasis=p.preemphasis, power=p.power, max_db=p.max_db, ref_db=p.ref_db, n_iter=p.n_iter, sr=p.sr)


def bound(yard, p):
    return G.K * max(yard, G.floor_(p))


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))


def c64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.complex64)))


def batch_of(arrays, dtype, fill):
    """[B, T_max, bins] on the device from per-utterance [T, bins] arrays, `fill` in the frames behind each utterance."""
    T_max, bins = max(a.shape[0] for a in arrays), arrays[0].shape[1]
    out = np.full((len(arrays), T_max, bins), fill, dtype=dtype)
    for b, a in enumerate(arrays):
        out[b, :a.shape[0]] = a
    return torch.from_numpy(out).to(dev())


def one_pass(pn):
    """One momentum pass on the device from the mirror's state after 10 iterations, the utterances of ONE_PASS[pn] as one ragged batch with NaN
    behind each utterance: (device X, device tprev, frame counts), shared by the tests of the pass."""
    def make():
        from unast_amd import audio, ops
        p = F.PARAM_SETS[pn]
        A = ap(p)
        Ts = list(ONE_PASS[pn])
        states = [F.state10(T, p) for T in Ts]
        M = batch_of([s[0] for s in states], np.float32, np.nan)
        X = batch_of([s[1] for s in states], np.complex64, np.nan + 0j)
        tprev = batch_of([s[2] for s in states], np.complex64, np.nan + 0j)
        frames = audio._i32(Ts, dev())
        window, tw = audio._tables(A, dev())
        T_max = max(Ts)
        y = torch.zeros(len(Ts), p.hop * (T_max - 1), device=dev())
        fr = torch.empty(len(Ts), T_max, p.win, device=dev())
        audio._istft_into(X, frames, A, window, tw, fr, y)
        ops.stft_momentum(y, frames, T_max, p.n_fft, p.hop, p.win, window, tw, X, M, ALPHA, tprev)
        return X.cpu().numpy(), tprev.cpu().numpy(), Ts
    return G.cached(("fgl_one_pass", pn), make)


def f32_pass(T, p):
    """The float32 CPU path's pass from the same state: (X, e) as numpy."""
    def make():
        M, X, tprev = F.state10(T, p)[:3]
        Xf, ef = F.f32_step(torch.from_numpy(X.copy()), torch.from_numpy(tprev.copy()), f32(M), ALPHA, p)
        return Xf.numpy(), ef.numpy()
    return G.cached(("fgl_f32_pass", T, p), make)


@pytest.mark.parametrize("pn", ONE_PASS)
def test_one_momentum_pass_rebuilt_spectrum(pn):
    """tprev <- e: the rebuilt spectrum against the mirror's, plain rel."""
    p = F.PARAM_SETS[pn]
    X, tprev, Ts = one_pass(pn)
    for b, T in enumerate(Ts):
        e1 = F.state10(T, p)[4]
        yard = G.rel(f32_pass(T, p)[1], e1)
        err = G.rel(tprev[b, :T], e1)
        print("momentum pass %s T=%d, rebuilt spectrum: rel %.3g, float32 CPU %.3g, ratio to yardstick %.2f, bound %.3g"
              % (pn, T, err, yard, err / max(yard, G.floor_(p)), bound(yard, p)))
        assert err <= bound(yard, p)
        assert np.isnan(tprev[b, T:]).all() and np.isnan(X[b, T:]).all(), "frames behind the utterance's length are not written"


@pytest.mark.parametrize("pn", ONE_PASS)
def test_one_momentum_pass_new_iterate(pn):
    """spec <- M c / (|c| + 1e-16) against the mirror's under the weighted metric; every bin's magnitude is M's."""
    p = F.PARAM_SETS[pn]
    X, _, Ts = one_pass(pn)
    for b, T in enumerate(Ts):
        M, _, _, X1, _, c1 = F.state10(T, p)
        w = F.weight(c1)
        yard = F.wrel(f32_pass(T, p)[0], X1, w)
        err = F.wrel(X[b, :T], X1, w)
        print("momentum pass %s T=%d, new iterate: weighted rel %.3g (plain %.3g), float32 CPU %.3g (plain %.3g), ratio to yardstick %.2f, bound %.3g"
              % (pn, T, err, G.rel(X[b, :T], X1), yard, G.rel(f32_pass(T, p)[0], X1), err / max(yard, G.floor_(p)), bound(yard, p)))
        assert err <= bound(yard, p)
        pos = M > 0
        mag_err = np.abs(np.abs(X[b, :T].astype(np.complex128))[pos] / M[pos] - 1).max()
        print("    magnitude: max relative error %.3g = %.2f eps32 over %d bins, %d of them with M = 0" % (mag_err, mag_err / G.EPS32, M.size, (~pos).sum()))
        assert mag_err <= 4 * G.EPS32
        assert not X[b, :T][~pos].any()


def ragged32(pn):
    """32 device iterations from the given angles0 for the ragged batch (NaN behind each utterance): the waveforms [3, n_max] as numpy."""
    def make():
        from unast_amd import audio
        p = F.PARAM_SETS[pn]
        runs = [F.run32(T, p) for T in G.RAGGED]
        M = batch_of([r[0] for r in runs], np.float32, np.nan)
        a0 = batch_of([r[1] for r in runs], np.complex64, np.nan + 0j)
        return audio.griffinlim(M, list(G.RAGGED), ap(p), angles0=a0).cpu().numpy()
    return G.cached(("fgl_ragged32", pn), make)


@pytest.mark.parametrize("pn", ["default", "small"])
def test_thirty_two_iterations_from_given_angles(pn):
    """Rounding grows through the iteration, so the waveform's allowance is K times what the float32 CPU run of the same loop shows.  The
    start is one on which float32 is stable (F.ANGLE_SEED; the condition is asserted in tests/test_cpu_fast_griffin_lim.py): from a start on
    which one bin's c nearly cancels, float32 runs one ulp apart end up to 89 times apart and no float32 implementation can be held to K times
    one of them (DESIGN.md section 5s has the record of such a start)."""
    from unast_amd import audio
    p = F.PARAM_SETS[pn]
    y = ragged32(pn)
    assert y.shape == (3, p.hop * 39) and y.dtype == np.float32
    for b, T in enumerate(G.RAGGED):
        n = p.hop * (T - 1)
        M, a0, y32 = F.run32(T, p)
        yard = G.rel(F.f32_griffinlim(M, p, F.N_ITER, F.MOMENTUM, a0).numpy(), y32)
        err = G.rel(y[b, :n], y32)
        print("32 iterations %s T=%d: rel %.3g, float32 CPU %.3g, ratio %.2f, bound %.3g" % (pn, T, err, yard, err / max(yard, G.floor_(p)), bound(yard, p)))
        assert np.isfinite(y[b, :n]).all() and not y[b, n:].any()
        assert err <= bound(yard, p)
    if pn == "default":                                                                     # T = 40 alone, a 2-D magnitude
        M, a0, _ = F.run32(40, p)
        alone = audio.griffinlim(f32(M).to(dev()), None, ap(p), angles0=torch.from_numpy(a0.copy()).to(dev()))
        assert tuple(alone.shape) == (p.hop * 39,) and np.array_equal(alone.cpu().numpy(), y[2])


@pytest.mark.parametrize("T", [9, 40])
def test_without_momentum_it_is_griffin_lim_to_the_bit(T):
    """momentum = 0, init = None: |e| + 1e-16 rounds to |e| and max(1e-8, |e|) is |e| where |e| >= 1e-8 (the mirror keeps min |e| >= 7.8e-6 on
    these inputs, tests/test_cpu_fast_griffin_lim.py), and the two epilogues share their expression order."""
    from unast_amd import audio
    p = G.SMALL
    M = f32(G.utterance(T, p, seed=T)[1]).to(dev())
    y, X, tprev = audio.griffinlim(M, None, ap(p), n_iter=8, momentum=0.0, init=None, return_state=True)
    y0, X0 = audio.griffin_lim(M, None, ap(p), n_iter=8, return_state=True)
    assert torch.equal(y, y0) and torch.equal(torch.view_as_real(X), torch.view_as_real(X0))
    assert float(tprev.abs().min()) >= 1e-6


def read_index(X0, n_fft):
    """The table index of every entry of a complex64 array of twiddle values, checked to reproduce it exactly."""
    tw = F.twiddle(n_fft)
    m = np.rint(-np.angle(X0.astype(np.complex128)) * n_fft / (2 * np.pi)).astype(np.int64) % n_fft
    assert np.array_equal(tw[m].view(np.float32), X0.view(np.float32)), "every entry is a table entry, to the bit"
    return m


@pytest.mark.parametrize("pn", ["default", "small"])
def test_random_phase_is_the_restated_draw(pn):
    from unast_amd import audio, ops
    p = F.PARAM_SETS[pn]
    A = ap(p)
    bins = p.n_fft // 2 + 1
    keys = [5, 0, 4000000000]
    frames = audio._i32(list(G.RAGGED), dev())
    _, tw = audio._tables(A, dev())
    assert np.array_equal(tw.cpu().numpy().view(np.float32), F.twiddle(p.n_fft).view(np.float32))
    X0 = torch.full((3, 40, bins), float("nan") + 0j, dtype=torch.complex64, device=dev())
    ops.gl_random_phase(torch.ones(3, 40, bins, device=dev()), frames, audio._keys_dev(keys, dev()), F.SEED, p.n_fft, tw, X0)
    X0 = X0.cpu().numpy()
    real = [f32(F.magnitude(T, p)).numpy() for T in G.RAGGED]
    XM = torch.full((3, 40, bins), float("nan") + 0j, dtype=torch.complex64, device=dev())
    ops.gl_random_phase(batch_of(real, np.float32, np.nan), frames, audio._keys_dev(keys, dev()), F.SEED, p.n_fft, tw, XM)
    XM = XM.cpu().numpy()
    for b, T in enumerate(G.RAGGED):
        want = F.phase_index(F.SEED, keys[b], T, p.n_fft)
        assert np.array_equal(read_index(X0[b, :T], p.n_fft), want), "utterance %d" % b
        t = F.twiddle(p.n_fft)[want]
        prod = np.empty(t.shape, dtype=np.complex64)
        prod.real, prod.imag = real[b] * t.real, real[b] * t.imag                           # float32 products, one rounding each
        assert np.array_equal(XM[b, :T].view(np.float32), prod.view(np.float32)), "M * tw[m] in float32, utterance %d" % b
        assert np.isnan(X0[b, T:]).all() and np.isnan(XM[b, T:]).all(), "frames behind the utterance's length are untouched"


def seeded(pn):
    """griffinlim(M, seed, keys) on the ragged batch with NaN behind each utterance: (waveforms as a device tensor, M, keys)."""
    def make():
        from unast_amd import audio
        p = F.PARAM_SETS[pn]
        keys = list(F.SEEDED_KEYS)
        M = batch_of([f32(F.magnitude(T, p)).numpy() for T in G.RAGGED], np.float32, np.nan)
        return audio.griffinlim(M, list(G.RAGGED), ap(p), seed=F.SEED, keys=keys), M, keys
    return G.cached(("fgl_seeded", pn), make)


@pytest.mark.parametrize("pn", ["default", "small"])
def test_seeded_run_equals_the_mirror_from_the_restated_phases(pn):
    """griffinlim(M, seed, keys) against the mirror run from the restated phases, under the K rule; F.SEED and F.SEEDED_KEYS give starts on
    which float32 is stable, as in test_thirty_two_iterations_from_given_angles."""
    p = F.PARAM_SETS[pn]
    y, _, keys = seeded(pn)
    y = y.cpu().numpy()
    for b, T in enumerate(G.RAGGED):
        n = p.hop * (T - 1)
        M, a0, y32 = F.run32(T, p, F.SEED, keys[b])
        yard = G.rel(F.f32_griffinlim(M, p, F.N_ITER, F.MOMENTUM, a0).numpy(), y32)
        err = G.rel(y[b, :n], y32)
        print("seeded 32 iterations %s T=%d key %d: rel %.3g, float32 CPU %.3g, ratio %.2f, bound %.3g"
              % (pn, T, keys[b], err, yard, err / max(yard, G.floor_(p)), bound(yard, p)))
        assert err <= bound(yard, p)


@pytest.mark.parametrize("pn", ["default", "small"])
def test_seeded_run_is_repeatable_and_independent_of_the_batch(pn):
    """Two runs are bit-equal; each utterance of the ragged batch (NaN in the padding, the whole tprev workspace pre-filled with NaN: the first
    iteration must not read it) equals to the bit the same utterance run alone with its key; another seed or key gives another waveform."""
    from unast_amd import audio
    p = F.PARAM_SETS[pn]
    A = ap(p)
    y, M, keys = seeded(pn)
    lens = list(G.RAGGED)
    assert torch.equal(y, audio.griffinlim(M, lens, A, seed=F.SEED, keys=keys)) and not torch.isnan(y).any()
    frames = audio._i32(lens, dev())
    X = torch.full(tuple(M.shape), float("nan") + 0j, dtype=torch.complex64, device=dev())
    tprev = torch.full_like(X, float("nan") + 0j)
    audio._random_phase(M, X, frames, keys, F.SEED, A)
    y2 = torch.zeros_like(y)
    audio._fast_griffin_lim(M, X, tprev, frames, A, F.N_ITER, ALPHA, y2)
    assert torch.equal(y, y2), "a workspace of NaN changes nothing"
    for b, T in enumerate(lens):
        assert torch.isnan(tprev[b, T:].real).all() and not torch.isnan(tprev[b, :T].real).any()
    for b, T in enumerate(lens):
        n = p.hop * (T - 1)
        alone = audio.griffinlim(M[b, :T].clone(), None, A, seed=F.SEED, keys=[keys[b]])
        assert torch.equal(y[b, :n], alone), "utterance %d" % b
    b, T = 1, 9
    n = p.hop * (T - 1)
    other_seed = audio.griffinlim(M[b, :T].clone(), None, A, seed=F.SEED + 1, keys=[keys[b]])
    other_key = audio.griffinlim(M[b, :T].clone(), None, A, seed=F.SEED, keys=[keys[b] + 1])
    default_key = audio.griffinlim(M[b, :T].clone(), None, A, seed=F.SEED)
    assert not torch.equal(other_seed, y[b, :n]) and not torch.equal(other_key, y[b, :n]) and not torch.equal(other_seed, other_key)
    assert torch.equal(default_key, y[b, :n]), "keys default to the utterance's index: key 0 for a single utterance"


def test_spectral_convergence_on_the_device():
    """Defaults, T = 40, 32 iterations from the restated phases: the device's spectral convergence against the mirror's from the same phases,
    and against the 60 plain iterations'."""
    from unast_amd import audio
    p = G.DEFAULT
    M, a0, y32 = F.run32(40, p)
    y = ragged32("default")[2]
    sc_dev, sc_ref = F.spectral_convergence(y, M, p), F.spectral_convergence(y32, M, p)
    plain = audio.griffin_lim(f32(M).to(dev()), None, ap(p)).cpu().numpy()
    sc_plain = F.spectral_convergence(plain, M, p)
    print("spectral convergence, T=40: momentum 32 iterations %.6g on the device, %.6g on the mirror (relative difference %.3g); plain 60 iterations on the device %.6g"
          % (sc_dev, sc_ref, abs(sc_dev / sc_ref - 1), sc_plain))
    assert abs(sc_dev / sc_ref - 1) <= 1e-3


def test_callers_with_method_librosa(tmp_path):
    from unast_amd import audio, ops
    p = G.DEFAULT
    A = ap(p)
    lens = list(G.RAGGED)
    mags = batch_of([G.normalised_mag(T, p, T) for T in lens], np.float32, np.nan)
    keys = [7, 8, 9]
    wavs = audio.spectrogram2wav_batch(mags, lens, A, method="librosa", seed=F.SEED, keys=keys)
    M = torch.empty_like(mags)
    ops.gl_prepare(mags, p.max_db, p.ref_db, p.power, M)
    y = audio.griffinlim(M, lens, A, seed=F.SEED, keys=keys)
    y = audio.deemphasis(y, [p.hop * (T - 1) for T in lens], p.preemphasis)
    bounds = audio.trim_bounds(y, [p.hop * (T - 1) for T in lens]).tolist()
    for b, (s, e) in enumerate(bounds):
        assert wavs[b].dim() == 1 and wavs[b].dtype == torch.float32 and 0 < len(wavs[b]) <= p.hop * (lens[b] - 1)
        assert torch.equal(wavs[b], y[b, s:e]), "utterance %d" % b
    # the default method is untouched
    short = audio.AudioParams(n_iter=3)
    ref = audio.spectrogram2wav_batch(mags, lens, short)
    kw = audio.spectrogram2wav_batch(mags, lens, short, method="reference", seed=5, keys=keys)
    assert all(torch.equal(a, b) for a, b in zip(ref, kw))
    one = audio.spectrogram2wav(G.normalised_mag(9, p, 9), method="librosa", seed=F.SEED)
    alone = audio.spectrogram2wav_batch(mags[1:2, :9].contiguous(), [9], A, method="librosa", seed=F.SEED)[0]
    assert one.dtype == np.float32 and np.array_equal(one, alone.cpu().numpy())
    # vocode: the same files at any batch size
    names = ["u5", "u9", "u6"]
    for n, T in zip(names, (5, 9, 6)):
        np.save(str(tmp_path / ("%s.mag.npy" % n)), G.normalised_mag(T, p, T))
    out1 = audio.vocode(names, str(tmp_path), str(tmp_path / "b1"), A, batch=1, method="librosa", seed=F.SEED)
    out3 = audio.vocode(names, str(tmp_path), str(tmp_path / "b3"), A, batch=3, method="librosa", seed=F.SEED)
    for a, b in zip(out1, out3):
        with wave.open(a, "rb") as fa, wave.open(b, "rb") as fb:
            assert fa.getnframes() == fb.getnframes() > 0 and fa.readframes(fa.getnframes()) == fb.readframes(fb.getnframes()), os.path.basename(a)
    with wave.open(out3[1], "rb") as f9:
        pcm = np.frombuffer(f9.readframes(f9.getnframes()), dtype="<i2")
    by_key = audio.spectrogram2wav_batch(mags[1:2, :9].contiguous(), [9], A, method="librosa", seed=F.SEED, keys=[1])[0].cpu().numpy()
    assert np.array_equal(pcm, np.round(np.clip(by_key.astype(np.float64), -1, 1) * 32767).astype("<i2")), "an utterance is keyed by its index in names"


def test_mel2wav_with_method_librosa_is_the_composition(golden_dir):
    from unast_amd import audio
    from unast_amd.network import Vocoder
    from unast_amd.portable import portable_tensor
    fx = np.load(os.path.join(golden_dir, "vocoder_b2_t37.npz"))
    model = Vocoder(80, 256, 2048)
    model.load_state_dict({k: torch.from_numpy(portable_tensor(k, tuple(v.shape), int(fx["meta"][2]))) for k, v in model.state_dict().items()})
    model = model.to(dev()).eval()
    mel = torch.from_numpy(fx["mel"]).to(dev())
    lens = [37, 21]
    got = audio.mel2wav(model, mel, lens, method="librosa", seed=F.SEED)
    with torch.no_grad():
        mags = model(mel)
    want = audio.spectrogram2wav_batch(mags, lens, method="librosa", seed=F.SEED)
    assert len(got) == 2 and all(torch.equal(a, b) for a, b in zip(got, want))
    assert all(torch.isfinite(w).all() and 0 < len(w) <= 275 * (n - 1) for w, n in zip(got, lens))


def test_c_entry_points_refuse_before_any_launch():
    """The C ABI itself: the package's error code and a message, nothing written."""
    from unast_amd import audio
    from unast_amd._lib import lib
    L = lib()
    d = dev()
    frames = torch.tensor([6], dtype=torch.int32, device=d)
    keys = torch.tensor([0], dtype=torch.int32, device=d)
    y = torch.zeros(1, 1375, device=d)
    w, tw = audio._tables(audio.AudioParams(), d)
    mag = torch.ones(1, 6, 1025, device=d)
    spec = torch.full((1, 6, 1025), 7.0 + 0j, dtype=torch.complex64, device=d)
    tprev = torch.full((1, 6, 1025), 3.0 + 0j, dtype=torch.complex64, device=d)
    p_ = lambda t: t.data_ptr()                                                            # noqa: E731

    def mom(y_=y, ld=1375, T=6, n_fft=2048, win=1102, mag_=mag, alpha=0.25, tprev_=tprev, spec_=spec):
        q_ = lambda t: None if t is None else t.data_ptr()                                 # noqa: E731
        return L.unast_stft_momentum(p_(y_), ld, p_(frames), 1, T, n_fft, 275, win, p_(w), p_(tw), q_(mag_), alpha, q_(tprev_), q_(spec_), None)
    calls = {
        "mag and tprev": lambda: mom(tprev_=None),
        "mag and tprev are needed": lambda: mom(mag_=None),
        "alpha": lambda: mom(alpha=0.5),
        "[0, 0.5)": lambda: mom(alpha=-0.01),
        "must lie in": lambda: mom(alpha=float("nan")),
        "is not spec": lambda: mom(tprev_=spec),
        "n_fft": lambda: mom(n_fft=300, win=200),
        "win": lambda: mom(win=2049),
        "frames": lambda: mom(T=4),
        "row stride": lambda: mom(ld=1000),
        "null": lambda: mom(spec_=None),
        "unast_gl_random_phase: null": lambda: L.unast_gl_random_phase(p_(mag), p_(frames), None, 0, 1, 6, 2048, p_(tw), p_(spec), None),
        "unast_gl_random_phase: n_fft": lambda: L.unast_gl_random_phase(p_(mag), p_(frames), p_(keys), 0, 1, 6, 1000, p_(tw), p_(spec), None),
        "alignment": lambda: L.unast_gl_random_phase(p_(mag), p_(frames), p_(keys), 0, 1, 6, 2048, p_(tw), p_(spec) + 4, None),
        "B <= 65535": lambda: L.unast_gl_random_phase(p_(mag), p_(frames), p_(keys), 0, 0, 6, 2048, p_(tw), p_(spec), None),
    }
    for word, call in calls.items():
        assert call() == -1, word
        assert word in L.unast_last_error().decode(), (word, L.unast_last_error().decode())
    torch.cuda.synchronize()
    assert bool((spec == 7.0 + 0j).all()) and bool((tprev == 3.0 + 0j).all()) and not y.any()
