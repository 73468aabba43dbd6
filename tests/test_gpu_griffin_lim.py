"""GPU tests of the waveform synthesis (unast_amd/audio.py, csrc/audio.hip) against the float64 mirror (tests/griffin_lim_mirror.py) with
rel(a, b) = ||a - b|| / ||b|| over whole utterances.  A bound "K times the yardstick" takes the float32 CPU path's error on the same input
(torch.stft / torch.istft in float32), floored at eps32 * log2(n_fft), times K = 8: pocketfft is about as accurate as a float32 FFT gets, a
Stockham radix-4 transform with exact table twiddles should land within about 3 times of it, and an indexing or twiddle mistake costs 1e-2
or more.  Every figure is printed before it is asserted; the measured ratios are recorded in DESIGN.md section 5q."""
import os
import wave

import numpy as np
import pytest
import torch
from scipy.signal import lfilter

from tests import griffin_lim_mirror as G

pytestmark = pytest.mark.gpu

PARAMS = {"default": G.DEFAULT, "small": G.SMALL}


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


def signal_batch(p, fill=0.0):
    """(y [3, n_max] float32 with `fill` behind each utterance, frame counts, the float32-rounded signals as float64)."""
    utts = G.ragged_batch(p)
    n_max = p.hop * (max(G.RAGGED) - 1)
    y = np.full((len(utts), n_max), fill, dtype=np.float32)
    sigs = []
    for b, (s, _) in enumerate(utts):
        y[b, :len(s)] = s
        sigs.append(y[b, :len(s)].astype(np.float64))
    return torch.from_numpy(y).to(dev()), list(G.RAGGED), sigs


def spectra_batch(p, fill=0.0):
    """Random complex spectra (imaginary DC / Nyquist bins included) [3, 40, bins] complex64 with `fill` in the frames behind each utterance."""
    F = p.n_fft // 2 + 1
    S = np.full((len(G.RAGGED), max(G.RAGGED), F), fill, dtype=np.complex64)
    for b, T in enumerate(G.RAGGED):
        rng = np.random.default_rng(100 + T)
        S[b, :T] = rng.standard_normal((T, F)) + 1j * rng.standard_normal((T, F))
    return S


@pytest.mark.parametrize("pn", PARAMS)
def test_stft_ragged_batch_and_alone(pn):
    from unast_amd import audio
    p = PARAMS[pn]
    y, frames, sigs = signal_batch(p)
    S = audio.stft(y, frames, ap(p)).cpu().numpy()
    assert S.shape == (3, 40, p.n_fft // 2 + 1) and S.dtype == np.complex64
    for b, T in enumerate(frames):
        ref = G.stft(sigs[b], p)
        yard = G.rel(G.torch_stft(sigs[b], p).numpy(), ref)
        err = G.rel(S[b, :T], ref)
        print("stft %s T=%d: rel %.3g, float32 CPU %.3g, ratio to yardstick %.2f, bound %.3g" % (pn, T, err, yard, err / max(yard, G.floor_(p)), bound(yard, p)))
        assert err <= bound(yard, p)
        assert not S[b, T:].any(), "frames behind the utterance's length are not written"
    one = audio.stft(f32(sigs[1]).to(dev()), None, ap(p))                                  # B = 1, a 1-D signal
    assert tuple(one.shape) == (9, p.n_fft // 2 + 1) and np.array_equal(one.cpu().numpy(), S[1, :9])


@pytest.mark.parametrize("pn", PARAMS)
def test_istft_ragged_batch_and_alone(pn):
    from unast_amd import audio
    p = PARAMS[pn]
    S = spectra_batch(p)
    y = audio.istft(torch.from_numpy(S).to(dev()), list(G.RAGGED), ap(p)).cpu().numpy()
    assert y.shape == (3, p.hop * 39) and y.dtype == np.float32
    for b, T in enumerate(G.RAGGED):
        n = p.hop * (T - 1)
        ref = G.istft(S[b, :T], p)
        yard = G.rel(G.torch_istft(S[b, :T], p).numpy(), ref)
        err = G.rel(y[b, :n], ref)
        print("istft %s T=%d: rel %.3g, float32 CPU %.3g, ratio to yardstick %.2f, bound %.3g" % (pn, T, err, yard, err / max(yard, G.floor_(p)), bound(yard, p)))
        assert err <= bound(yard, p)
        assert not y[b, n:].any()
    one = audio.istft(torch.from_numpy(S[1, :9].copy()).to(dev()), None, ap(p))
    assert tuple(one.shape) == (p.hop * 8,) and np.array_equal(one.cpu().numpy(), y[1, :p.hop * 8])
    # the imaginary parts of the DC and Nyquist bins are ignored
    S0 = S[1, :9].copy()
    S0[:, 0], S0[:, -1] = S0[:, 0].real, S0[:, -1].real
    assert torch.equal(audio.istft(torch.from_numpy(S0).to(dev()), None, ap(p)), one)


@pytest.mark.parametrize("pn", PARAMS)
def test_round_trip(pn):
    from unast_amd import audio
    p = PARAMS[pn]
    y, frames, sigs = signal_batch(p)
    back = audio.istft(audio.stft(y, frames, ap(p)), frames, ap(p)).cpu().numpy()
    for b, T in enumerate(frames):
        n = p.hop * (T - 1)
        yard = G.rel(G.torch_istft(G.torch_stft(sigs[b], p), p).numpy(), sigs[b])
        err = G.rel(back[b, :n], sigs[b])
        print("round trip %s T=%d: rel %.3g, float32 CPU %.3g, bound %.3g" % (pn, T, err, yard, bound(yard, p)))
        assert err <= bound(yard, p)


@pytest.mark.parametrize("pn", PARAMS)
def test_utterances_do_not_depend_on_their_batch(pn):
    """Each utterance of the ragged batch, with NaN in the batch's padding samples and frames, equals to the bit the same utterance run alone;
    two runs of one call are bit-equal."""
    from unast_amd import audio
    p = PARAMS[pn]
    A = ap(p)
    y, frames, _ = signal_batch(p, fill=np.nan)
    S = audio.stft(y, frames, A)
    assert torch.equal(S, audio.stft(y, frames, A)) and not torch.isnan(S.real).any()
    Sr = torch.from_numpy(spectra_batch(p, fill=np.nan + 0j)).to(dev())
    w = audio.istft(Sr, frames, A)
    assert torch.equal(w, audio.istft(Sr, frames, A)) and not torch.isnan(w).any()
    M = torch.full((3, 40, p.n_fft // 2 + 1), float("nan"), device=dev())
    for b, (_, mag) in enumerate(G.ragged_batch(p)):
        M[b, :frames[b]] = f32(mag).to(dev())
    g = audio.griffin_lim(M, frames, A, n_iter=3)
    assert torch.equal(g, audio.griffin_lim(M, frames, A, n_iter=3)) and not torch.isnan(g).any()
    for b, T in enumerate(frames):
        n = p.hop * (T - 1)
        assert torch.equal(S[b, :T], audio.stft(y[b, :n].clone(), None, A)), "stft, utterance %d" % b
        assert torch.equal(w[b, :n], audio.istft(Sr[b, :T].clone(), None, A)), "istft, utterance %d" % b
        assert torch.equal(g[b, :n], audio.griffin_lim(M[b, :T].clone(), None, A, n_iter=3)), "griffin_lim, utterance %d" % b


@pytest.mark.parametrize("p", G.MID, ids=["512", "1024"])
def test_the_other_transform_sizes(p):
    """n_fft 512 (radix-4 passes and the closing radix-2 pass) and 1024 (radix-4 only), the latter with win = n_fft: both transforms and the
    round trip at T = 9."""
    from unast_amd import audio
    y, _ = G.utterance(9, p, seed=9)
    y = y.astype(np.float32).astype(np.float64)
    ref = G.stft(y, p)
    S = audio.stft(f32(y).to(dev()), None, ap(p))
    yard = G.rel(G.torch_stft(y, p).numpy(), ref)
    err = G.rel(S.cpu().numpy(), ref)
    rng = np.random.default_rng(p.n_fft)
    R = (rng.standard_normal(ref.shape) + 1j * rng.standard_normal(ref.shape)).astype(np.complex64)
    refi = G.istft(R, p)
    yardi = G.rel(G.torch_istft(R, p).numpy(), refi)
    erri = G.rel(audio.istft(torch.from_numpy(R).to(dev()), None, ap(p)).cpu().numpy(), refi)
    back = G.rel(audio.istft(S, None, ap(p)).cpu().numpy(), y)
    print("n_fft %d: stft rel %.3g (float32 CPU %.3g), istft rel %.3g (float32 CPU %.3g), round trip %.3g; bounds %.3g / %.3g"
          % (p.n_fft, err, yard, erri, yardi, back, bound(yard, p), bound(yardi, p)))
    assert err <= bound(yard, p) and erri <= bound(yardi, p) and back <= bound(0.0, p)


def test_c_entry_points_refuse_before_any_launch():
    """The C ABI itself: the package's error code and a message, nothing written."""
    from unast_amd import audio
    from unast_amd._lib import lib
    L = lib()
    d = dev()
    frames = torch.tensor([6], dtype=torch.int32, device=d)
    y = torch.zeros(1, 1375, device=d)
    w, tw = audio._tables(audio.AudioParams(), d)
    spec = torch.full((1, 6, 1025), 7.0 + 0j, dtype=torch.complex64, device=d)
    fr = torch.full((1, 6, 1102), 7.0, device=d)
    out = torch.full((1, 2), -5, dtype=torch.int32, device=d)
    p_ = lambda t: t.data_ptr()                                                            # noqa: E731
    calls = {
        "n_fft": lambda: L.unast_stft(p_(y), 1375, p_(frames), 1, 6, 300, 275, 200, p_(w), p_(tw), None, p_(spec), None),
        "win": lambda: L.unast_istft_frames(p_(spec), p_(frames), 1, 6, 2048, 2049, p_(w), p_(tw), p_(fr), None),
        "frames": lambda: L.unast_stft(p_(y), 1375, p_(frames), 1, 4, 2048, 275, 1102, p_(w), p_(tw), None, p_(spec), None),
        "row stride": lambda: L.unast_overlap_add(p_(fr), p_(frames), 1, 6, 2048, 275, 1102, p_(w), p_(y), 1000, None),
        "null": lambda: L.unast_gl_prepare(None, 1025, 6, 1025, 100.0, 20.0, 1.2, p_(fr), None, None),
        "coef": lambda: L.unast_deemphasis(p_(y), 1375, p_(y), 1375, p_(frames), 1, 1.5, None),
        "pad_mode": lambda: L.unast_trim_bounds(p_(y), 1375, p_(frames), 1, 1375, 60.0, 2048, 512, 2, p_(fr), 6612, p_(out), None),
        "workspace": lambda: L.unast_trim_bounds(p_(y), 1375, p_(frames), 1, 1375, 60.0, 2048, 512, 0, p_(fr), 2, p_(out), None),
    }
    for word, call in calls.items():
        assert call() == -1, word
        assert word in L.unast_last_error().decode(), (word, L.unast_last_error().decode())
    torch.cuda.synchronize()
    assert bool((spec == 7.0 + 0j).all()) and bool((fr == 7.0).all()) and bool((out == -5).all()) and not y.any()


def _t40():
    """T = 40 at the defaults: (M float32 as float64, state after 30 mirror iterations as complex64, the mirror's 60-iteration waveform)."""
    def make():
        p = G.DEFAULT
        _, M = G.utterance(40, p, seed=40)
        M = M.astype(np.float32).astype(np.float64)
        _, X30 = G.griffin_lim(M, p, 30, return_state=True)
        return M, X30.astype(np.complex64), G.griffin_lim(M, p)
    return G.cached("t40", make)


def test_one_iteration_from_a_common_state():
    from unast_amd import audio
    p = G.DEFAULT
    M, X30, _ = _t40()
    ref = G.gl_step(X30, M, p)
    yard = G.rel(G.f32_gl_step(torch.from_numpy(X30.copy()), f32(M), p).numpy(), ref)
    _, X = audio.griffin_lim(f32(M).to(dev()), None, ap(p), n_iter=1, X0=torch.from_numpy(X30.copy()).to(dev()), return_state=True)
    err = G.rel(X.cpu().numpy(), ref)
    print("one iteration: rel %.3g, float32 CPU %.3g, ratio to yardstick %.2f, bound %.3g" % (err, yard, err / max(yard, G.floor_(p)), bound(yard, p)))
    assert err <= bound(yard, p)


def test_sixty_iterations():
    """Rounding grows through the iteration, so the waveform's allowance is K times what the float32 CPU run of the same map shows; the
    spectral convergence must agree with the mirror's to 1e-4 relative."""
    from unast_amd import audio
    p = G.DEFAULT
    M, _, y60 = _t40()
    yard = G.rel(G.f32_griffin_lim(M, p).numpy(), y60)
    y = audio.griffin_lim(f32(M).to(dev()), None, ap(p)).cpu().numpy()
    err = G.rel(y, y60)

    def sc(w):
        return np.linalg.norm(np.abs(G.stft(np.asarray(w, dtype=np.float64), p)) - M) / np.linalg.norm(M)
    sc_dev, sc_ref = sc(y), sc(y60)
    print("60 iterations: rel %.3g, float32 CPU %.3g, ratio %.2f, bound %.3g; spectral convergence %.8g (mirror %.8g, relative difference %.3g)"
          % (err, yard, err / max(yard, G.floor_(p)), bound(yard, p), sc_dev, sc_ref, abs(sc_dev / sc_ref - 1)))
    assert np.isfinite(y).all()
    assert err <= bound(yard, p)
    assert abs(sc_dev / sc_ref - 1) <= 1e-4


def test_zero_magnitude_and_gl_prepare():
    from unast_amd import audio, ops
    p = G.DEFAULT
    z = audio.griffin_lim(torch.zeros(2, 6, 1025, device=dev()), [6, 5], ap(p), n_iter=4)
    assert tuple(z.shape) == (2, 275 * 5) and not z.any() and not torch.isnan(z).any()
    # the lowest normalised magnitude, clip(mag) = 0, is a small positive M: finite as well
    w = audio.spectrogram2wav_batch(torch.zeros(1, 6, 1025, device=dev()), [6], ap(p), trim=False)[0]
    assert torch.isfinite(w).all()
    mag = np.concatenate([G.normalised_mag(9, p, 9), np.linspace(-0.5, 1.5, 2 * 1025, dtype=np.float32).reshape(2, 1025)])
    ref = G.gl_prepare(mag, p)
    buf = torch.full((11, 1028), float("nan"), device=dev())                                # rows of 1028 floats, as Vocoder.forward's output
    buf[:, :1025] = torch.from_numpy(mag).to(dev())
    for src in (torch.from_numpy(mag).to(dev()), buf[:, :1025]):
        M = torch.empty(11, 1025, device=dev())
        X = torch.empty(11, 1025, dtype=torch.complex64, device=dev())
        ops.gl_prepare(src, p.max_db, p.ref_db, p.power, M, X)
        err = np.abs(M.cpu().numpy() / ref - 1).max()
        print("gl_prepare: max relative error %.3g = %.2f eps32" % (err, err / G.EPS32))
        assert err <= 32 * G.EPS32
        assert torch.equal(X.real, M) and not X.imag.any()


def test_deemphasis_against_lfilter():
    """max |y - lfilter| <= 64 eps32 * peak of lfilter's output: the recurrence sums about 1 / (1 - 0.97) = 33 terms of weight, each rounded at the
    output's scale, and the reference accumulates in float64.  Lengths: 1, around the per-thread chunk and the workgroup tile, 1100, 10725."""
    from unast_amd import audio, ops
    c, t = ops.DEEMPH_CHUNK, ops.DEEMPH_TILE
    lens = [1, c - 1, c, c + 1, t - 1, t, t + 1, 2 * t + c + 3, 1100, 10725]
    n_max = max(lens)
    x = np.full((len(lens), n_max), np.nan, dtype=np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = G.signal(max(n, 64), seed=b)[:n] + 0.2                                   # an offset: the carries between chunks matter
    y = audio.deemphasis(torch.from_numpy(x).to(dev()), lens, 0.97).cpu().numpy()
    for b, n in enumerate(lens):
        ref = lfilter([1.0], [1.0, -0.97], x[b, :n].astype(np.float64))
        err = np.abs(y[b, :n] - ref).max() / np.abs(ref).max()
        print("deemphasis n=%d: max error / peak %.3g = %.2f eps32" % (n, err, err / G.EPS32))
        assert err <= 64 * G.EPS32
        assert not y[b, n:].any(), "samples behind the length are not written"
    xd = torch.from_numpy(x[-1:, :10725].copy()).to(dev())
    assert torch.equal(ops.deemphasis(xd, torch.tensor([10725], dtype=torch.int32, device=dev()), 0.97, xd)[0], torch.from_numpy(y[-1, :10725]).to(dev())), "in place"


def test_trim_bounds():
    from unast_amd import audio
    cases = G.trim_cases()
    names = list(cases)
    lens = [len(cases[k]) for k in names]
    y = np.full((len(names), max(lens)), np.nan, dtype=np.float32)
    for b, k in enumerate(names):
        y[b, :lens[b]] = cases[k]
    yd = torch.from_numpy(y).to(dev())
    for mode in ("reflect", "constant"):
        got = audio.trim_bounds(yd, lens, pad_mode=mode).cpu().tolist()
        for b, k in enumerate(names):
            ref = G.trim_bounds(y[b, :lens[b]].astype(np.float64), pad_mode=mode)
            print("trim %s %s: %s (mirror %s)" % (k, mode, tuple(got[b]), ref))
            assert tuple(got[b]) == ref
        alone = audio.trim_bounds(yd[0, :lens[0]].clone(), pad_mode=mode).cpu().tolist()
        assert alone == got[0]
    z = G.pad_mode_case()
    zd = f32(z).to(dev())
    r, c = audio.trim_bounds(zd, pad_mode="reflect").tolist(), audio.trim_bounds(zd, pad_mode="constant").tolist()
    print("trim pad-mode case: reflect %s constant %s" % (r, c))
    assert tuple(r) == G.trim_bounds(z, pad_mode="reflect") == (0, 1536) and tuple(c) == G.trim_bounds(z, pad_mode="constant") == (0, 4096)


def test_spectrogram2wav_batch_end_to_end():
    from unast_amd import audio
    p = G.DEFAULT
    mags = [G.normalised_mag(T, p, T) for T in G.RAGGED]
    batch = np.full((3, 40, 1025), np.nan, dtype=np.float32)
    for b, m in enumerate(mags):
        batch[b, :len(m)] = m
    wavs = audio.spectrogram2wav_batch(torch.from_numpy(batch).to(dev()), list(G.RAGGED), ap(p))
    for b, T in enumerate(G.RAGGED):
        full, _ = G.cached(("s2w", T), lambda: G.spectrogram2wav(mags[b], p, trim=False))
        s, e = G.trim_bounds(full)
        got = wavs[b].cpu().numpy()
        assert wavs[b].dtype == torch.float32 and wavs[b].dim() == 1 and wavs[b].is_cuda
        yard = G.rel(G.f32_spectrogram2wav(mags[b], p)[s:e], full[s:e])
        print("spectrogram2wav T=%d: %d samples (mirror %d..%d)" % (T, len(got), s, e))
        assert len(got) == e - s
        err = G.rel(got, full[s:e])
        print("    rel %.3g, float32 CPU %.3g, ratio %.2f, bound %.3g" % (err, yard, err / max(yard, G.floor_(p)), bound(yard, p)))
        assert err <= bound(yard, p)
    one = audio.spectrogram2wav(mags[1])
    assert isinstance(one, np.ndarray) and one.dtype == np.float32 and np.array_equal(one, wavs[1].cpu().numpy())
    from unast_amd import utils
    assert np.array_equal(utils.spectrogram2wav(mags[1]), one)
    untrimmed = audio.spectrogram2wav_batch(torch.from_numpy(batch).to(dev()), list(G.RAGGED), ap(p), trim=False)
    assert [len(w) for w in untrimmed] == [275 * (T - 1) for T in G.RAGGED]


def test_mel2wav_is_the_composition(golden_dir):
    from unast_amd import audio
    from unast_amd.network import Vocoder
    from unast_amd.portable import portable_tensor
    fx = np.load(os.path.join(golden_dir, "vocoder_b2_t37.npz"))
    model = Vocoder(80, 256, 2048)
    model.load_state_dict({k: torch.from_numpy(portable_tensor(k, tuple(v.shape), int(fx["meta"][2]))) for k, v in model.state_dict().items()})
    model = model.to(dev()).eval()
    mel = torch.from_numpy(fx["mel"]).to(dev())
    lens = [37, 21]
    short = audio.AudioParams(n_iter=3)
    got = audio.mel2wav(model, mel, lens, short)
    with torch.no_grad():
        mags = model(mel)
    want = audio.spectrogram2wav_batch(mags, lens, short)
    assert len(got) == 2 and all(torch.equal(a, b) for a, b in zip(got, want))
    assert all(torch.isfinite(w).all() and 0 < len(w) <= 275 * (n - 1) for w, n in zip(got, lens))


def test_write_wav_round_trip(tmp_path):
    from unast_amd import audio
    x = (0.8 * G.signal(3000, seed=1)).astype(np.float32)
    x[:3] = (1.5, -1.5, 0.0)                                                                # clipped
    path = audio.write_wav(str(tmp_path / "a.wav"), torch.from_numpy(x).to(dev()), 22050)
    with wave.open(path, "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 22050, 3000)
        pcm = np.frombuffer(f.readframes(3000), dtype="<i2")
    assert pcm[0] == 32767 and pcm[1] == -32767 and pcm[2] == 0
    assert np.abs(pcm / 32767.0 - np.clip(x, -1, 1)).max() <= 0.5 / 32767 + 1e-7
    # vocode: <name>.mag.npy in, <name>.wav out
    mag = G.normalised_mag(6, G.DEFAULT, 6)
    np.save(str(tmp_path / "u1.mag.npy"), mag)
    out = audio.vocode(["u1"], str(tmp_path), str(tmp_path / "wavs"), audio.AudioParams(n_iter=2))
    with wave.open(out[0], "rb") as f:
        assert f.getframerate() == 22050 and 0 < f.getnframes() <= 275 * 5
