"""GPU tests of the feature extraction (unast_amd/audio.py: get_spectrograms_batch, preemphasis, prepare_data; the features kernel of
csrc/audio.hip) against the float64 mirror (tests/features_mirror.py).  Metric: rms(a - ref) over an utterance's valid frames, in normalised
units, separately for mel and mag.  Bound: K = 8 (the project's own, tests/griffin_lim_mirror.py) times the larger of the float32 CPU path's
rms on the same input and floor = 20 / (max_db ln 10) * eps32 * log2(n_fft) (1.14e-7 at the defaults), the sensitivity of a normalised value
to a relative magnitude error of eps32 * log2(n_fft).  Every figure is printed before it is asserted; the max-abs is printed and not asserted
(it is decided by the few bins near 1e-4, where two correct FFTs differ by chance).  The measured ratios are recorded in DESIGN.md section 5r."""
import os
import wave

import numpy as np
import pytest
import torch

from tests import features_mirror as F
from tests import griffin_lim_mirror as G

pytestmark = pytest.mark.gpu

LOW = np.float32(1e-8)


def dev():
    return torch.device("cuda:0")


def ap(p, **kw):
    from unast_amd.audio import AudioParams
    return AudioParams(n_fft=p.n_fft, hop=p.hop, win=p.win, preemphasis=p.preemphasis, power=p.power, max_db=p.max_db, ref_db=p.ref_db, n_iter=p.n_iter,
                       sr=p.sr, n_mels=p.n_mels, **kw)


def bits(t):
    """The float32 words of a float32 or complex64 tensor, for comparisons to the bit."""
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def batch_of(wavs, fill=0.0, starts=None, extra=0):
    """y float32 [B, n_max + extra] on the device with utterance b at starts[b] (default 0) and `fill` everywhere else."""
    starts = [0] * len(wavs) if starts is None else starts
    y = np.full((len(wavs), max(len(w) for w in wavs) + extra), fill, dtype=np.float32)
    for b, w in enumerate(wavs):
        y[b, starts[b]:starts[b] + len(w)] = w
    return torch.from_numpy(y).to(dev())


def check_accuracy(tag, p, got, ref, f32, cols=None):
    """One utterance, one of mel / mag: got (device), ref (mirror), f32 (float32 CPU), optionally over some columns only."""
    if cols is not None:
        got, ref, f32 = got[:, cols], ref[:, cols], f32[:, cols]
    yard = F.rms(f32, ref)
    err = F.rms(got, ref)
    bound = F.K * max(yard, F.floor_(p))
    print("%s: rms %.3g, max-abs %.3g, float32 CPU rms %.3g, ratio to max(yardstick, floor) %.2f, bound %.3g"
          % (tag, err, float(np.abs(got - ref).max()), yard, err / max(yard, F.floor_(p)), bound))
    assert np.isfinite(got).all()
    assert err <= bound, tag


def test_preemphasis_equals_numpy_to_the_bit():
    """A ragged batch (a row of length 1 among them) through audio.preemphasis, and the same utterances at non-zero starts through the op."""
    from unast_amd import audio, ops
    rng = np.random.default_rng(7)
    lens = [1, 2, 255, 256, 257, 5000]
    wavs = [(rng.standard_normal(n) * 0.3).astype(np.float32) for n in lens]
    wavs[3][:4] = (0.0, -0.0, 1e-38, 3.0e38)                                                # zeros, a subnormal product, a huge value
    out = audio.preemphasis(batch_of(wavs, fill=np.nan), lens).cpu().numpy()
    for b, w in enumerate(wavs):
        want = F.preemphasis(w)
        assert want.dtype == np.float32 and np.array_equal(out[b, :lens[b]].view(np.int32), want.view(np.int32)), "row %d" % b
        assert not out[b, lens[b]:].any(), "samples behind the length are not written"
    one = audio.preemphasis(torch.tensor(wavs[5]).to(dev()))
    assert np.array_equal(one.cpu().numpy().view(np.int32), F.preemphasis(wavs[5]).view(np.int32))
    starts = [3, 0, 700, 1, 256, 29]
    x = batch_of(wavs, fill=1e30, starts=starts, extra=800)
    y = torch.full_like(x, -7.0)
    ops.preemphasis(x, torch.tensor(lens, dtype=torch.int32, device=dev()), 0.97, y, start=torch.tensor(starts, dtype=torch.int32, device=dev()))
    y = y.cpu().numpy()
    for b, w in enumerate(wavs):
        s, n = starts[b], lens[b]
        assert np.array_equal(y[b, s:s + n].view(np.int32), F.preemphasis(w).view(np.int32)), "row %d at start %d" % (b, s)
        assert (y[b, :s] == -7.0).all() and (y[b, s + n:] == -7.0).all(), "nothing outside the utterance is written"


@pytest.mark.parametrize("pn", F.PARAMS)
def test_spectrum_equals_the_stft_kernels_to_the_bit(pn):
    """Utterances of exactly hop * (T - 1) samples: the features kernel's complex output is unast_stft's of the emphasised signal, and placing
    each utterance at a non-zero start in a row that holds 1e30 elsewhere changes nothing: nothing outside [start, start + n) is read."""
    from unast_amd import audio
    p = F.PARAMS[pn]
    A = ap(p)
    wavs = [G.signal(p.hop * (T - 1), seed=T, sr=p.sr).astype(np.float32) for T in G.RAGGED]
    lens = [len(w) for w in wavs]
    y = batch_of(wavs)
    mel, mag, frames, S = audio.get_spectrograms_batch(y, lens, A, trim=False, return_spec=True)
    assert frames == list(G.RAGGED)
    want = audio.stft(audio.preemphasis(y, lens), frames, A)
    for b, T in enumerate(frames):
        assert same_bits(S[b, :T], want[b, :T]), "utterance %d" % b
        assert not S[b, T:].abs().any()
    assert float(S.abs().max()) > 1.0
    starts = [37, 1, 64]
    y2 = batch_of(wavs, fill=1e30, starts=starts, extra=101)
    mel2, mag2, frames2, S2 = audio.get_spectrograms_batch(y2, lens, A, trim=False, starts=starts, return_spec=True)
    assert frames2 == frames and same_bits(S2, S) and same_bits(mel2, mel) and same_bits(mag2, mag)


CASES = [(pn, name) for pn in F.PARAMS for name in F.SIGNALS if (pn, name) not in F.SKIP]


@pytest.mark.parametrize("pn,name", CASES, ids=["%s-%s" % c for c in CASES])
def test_accuracy_against_the_mirror(pn, name):
    """The four sample counts as one ragged batch (NaN behind each utterance) and each utterance alone."""
    from unast_amd import audio
    p = F.PARAMS[pn]
    A = ap(p)
    wavs = dict(F.accuracy_cases(pn))[name]
    lens = [len(w) for w in wavs]
    assert tuple(lens) == F.counts(p)
    y = batch_of(wavs, fill=np.nan)
    mel, mag, frames = audio.get_spectrograms_batch(y, lens, A, trim=False)
    assert frames == [F.frames_of(n, p) for n in lens]
    assert tuple(mel.shape) == (4, max(frames), p.n_mels) and tuple(mag.shape) == (4, max(frames), p.n_fft // 2 + 1)
    assert mel.dtype == torch.float32 and mag.dtype == torch.float32
    again = audio.get_spectrograms_batch(y, lens, A, trim=False)
    assert same_bits(again[0], mel) and same_bits(again[1], mag), "two runs"
    for b, T in enumerate(frames):
        rmel, rmag, fmel, fmag = F.reference(pn, name, b)
        check_accuracy("%s %s n=%d mel" % (pn, name, lens[b], ), p, mel[b, :T].cpu().numpy(), rmel, fmel)
        check_accuracy("%s %s n=%d mag" % (pn, name, lens[b], ), p, mag[b, :T].cpu().numpy(), rmag, fmag)
        assert not mel[b, T:].any() and not mag[b, T:].any(), "rows at or behind frames[b] are zero"
        m1, g1, f1 = audio.get_spectrograms_batch(torch.tensor(wavs[b]).to(dev()).unsqueeze(0), [lens[b]], A, trim=False)
        assert f1 == [T] and same_bits(m1[0], mel[b, :T]) and same_bits(g1[0], mag[b, :T]), "utterance %d alone" % b


@pytest.mark.parametrize("mode", ["reflect", "constant"])
def test_trim_path(mode):
    from unast_amd import audio
    p = F.DEFAULT
    A = ap(p)
    names, wavs = F.trim_batch()
    lens = [len(w) for w in wavs]
    mel, mag, frames = audio.get_spectrograms_batch(batch_of(wavs, fill=np.nan), lens, A, trim=True, pad_mode=mode)
    bounds = [G.trim_bounds(w.astype(np.float64), pad_mode=mode) for w in wavs]
    print("trim %s: %s, frames %s" % (mode, dict(zip(names, bounds)), frames))
    assert [e - s for s, e in bounds] == [8704, 6117, 6144, 8000, 6000]
    assert frames == [1 + (e - s) // p.hop for s, e in bounds]
    cut = [w[s:e] for w, (s, e) in zip(wavs, bounds)]
    mel2, mag2, frames2 = audio.get_spectrograms_batch(batch_of(cut), [len(c) for c in cut], A, trim=False)
    assert frames2 == frames and same_bits(mel2, mel) and same_bits(mag2, mag)
    b = names.index("all_silent")
    T = frames[b]
    assert (mel[b, :T].cpu().numpy() == LOW).all() and (mag[b, :T].cpu().numpy() == LOW).all(), "silence is the lower clip exactly"
    rmel, rmag, _ = F.features(cut[0], p)
    fmel, fmag = F.f32_features(cut[0], p)
    check_accuracy("trimmed %s mel" % names[0], p, mel[0, :frames[0]].cpu().numpy(), rmel, fmel)
    check_accuracy("trimmed %s mag" % names[0], p, mag[0, :frames[0]].cpu().numpy(), rmag, fmag)


def test_empty_filters():
    """n_fft 256 with 80 filters: two of them hold no bin; their columns are the lower clip exactly, the others meet the accuracy bound."""
    from unast_amd import audio
    p = F.SMALL80
    W, ranges = audio.mel_basis(ap(p))
    empty = np.flatnonzero(ranges[:, 1] == ranges[:, 0])
    full = np.flatnonzero(ranges[:, 1] > ranges[:, 0])
    assert len(empty) == 2
    w = F.make_signal("plain", F.counts(p)[3], p, seed=14)
    mel, mag, frames = audio.get_spectrograms_batch(torch.tensor(w).to(dev()).unsqueeze(0), [len(w)], ap(p), trim=False)
    mel, mag = mel[0].cpu().numpy(), mag[0].cpu().numpy()
    assert mel.shape == (frames[0], 80) and (mel[:, empty] == LOW).all()
    rmel, rmag, _ = F.features(w, p)
    fmel, fmag = F.f32_features(w, p)
    check_accuracy("empty filters mel", p, mel, rmel, fmel, cols=full)
    check_accuracy("empty filters mag", p, mag, rmag, fmag)


def test_prepare_data_writes_what_the_loaders_read(tmp_path):
    from unast_amd import audio, utils
    from unast_amd.data import NpyFeatureDataset
    sigs = {"u1": G.signal(9000, seed=21, lead=1500, tail=1200), "u2": G.signal(7000, seed=22), "u3": G.signal(12000, seed=23, lead=0, tail=3000)}
    wav_dir = tmp_path / "wavs"
    wav_dir.mkdir()
    for k, v in sigs.items():
        audio.write_wav(str(wav_dir / ("%s.wav" % k)), v.astype(np.float32))
    out = audio.prepare_data(list(sigs), str(wav_dir), batch=2)
    assert [os.path.basename(a) for a, _ in out] == ["u1.pt.npy", "u2.pt.npy", "u3.pt.npy"] and all(os.path.dirname(a) == str(wav_dir) for a, _ in out)
    for k, (pm, pg) in zip(sigs, out):
        mel, mag = np.load(pm), np.load(pg)
        assert mel.dtype == np.float32 and mag.dtype == np.float32
        assert mel.ndim == 2 and mel.shape[1] == 80 and mag.shape == (mel.shape[0], 1025) and mel.shape[0] >= 5
        m1, g1 = audio.get_spectrograms(str(wav_dir / ("%s.wav" % k)))
        assert np.array_equal(m1, mel) and np.array_equal(g1, mag)
        y = audio.load_wav(str(wav_dir / ("%s.wav" % k)))
        s, e = G.trim_bounds(y.astype(np.float64))
        assert mel.shape[0] == 1 + (e - s) // 275
        assert mel.min() >= LOW and mel.max() <= 1.0 and 0.2 < mel.mean() < 0.9
    assert utils.get_spectrograms is audio.get_spectrograms
    other = audio.prepare_data(["u2"], str(wav_dir), str(tmp_path / "feats"))
    assert other == [(str(tmp_path / "feats" / "u2.pt.npy"), str(tmp_path / "feats" / "u2.mag.npy"))]
    assert np.array_equal(np.load(other[0][0]), np.load(out[1][0]))
    # unast_amd.data reads the .pt.npy where an .ids.npy is present
    np.save(str(wav_dir / "u1.ids.npy"), np.array([5, 9, 2, 7], dtype=np.int32))
    meta = tmp_path / "meta.csv"
    meta.write_text("u1|some text|some text\n")
    sample = NpyFeatureDataset(str(meta), str(wav_dir))[0]
    assert np.array_equal(sample["mel"], np.load(out[0][0])) and sample["mel_length"] == sample["mel"].shape[0] and sample["text_length"] == 4
    # audio.vocode reads the .mag.npy
    wavs = audio.vocode(["u1"], str(wav_dir), str(tmp_path / "synth"), audio.AudioParams(n_iter=2))
    with wave.open(wavs[0], "rb") as f:
        assert f.getframerate() == 22050 and 0 < f.getnframes() <= 275 * (sample["mel_length"] - 1)


def test_c_entry_points_refuse_before_any_launch():
    """The C ABI itself: the package's error code and a message, nothing written."""
    from unast_amd import audio
    from unast_amd._lib import lib
    L = lib()
    d = dev()
    A = audio.AudioParams()
    one = torch.tensor([2200], dtype=torch.int32, device=d)
    zero = torch.zeros(1, dtype=torch.int32, device=d)
    y = torch.zeros(1, 2200, device=d)
    w, tw = audio._tables(A, d)
    W, ranges = audio.mel_basis(A, d)
    mel = torch.full((1, 9, 80), 7.0, device=d)
    mag = torch.full((1, 9, 1025), 7.0, device=d)
    out = torch.full((1, 2200), 7.0, device=d)
    p_ = lambda t: t.data_ptr()                                                            # noqa: E731

    def feat(n_fft=2048, hop=275, win=1102, n_mels=80, T_max=9, n_max=2200, ld=2200, max_db=100.0, basis=p_(W)):
        return L.unast_features(p_(y), ld, n_max, p_(zero), p_(one), 1, T_max, n_fft, hop, win, 0.97, p_(w), p_(tw), basis, p_(ranges), n_mels, 20.0, max_db,
                                p_(mel), p_(mag), None, None)
    calls = {
        "n_fft": lambda: feat(n_fft=300),
        "win": lambda: feat(win=2049),
        "hop >= 1": lambda: feat(hop=0),
        "hop must not exceed win": lambda: feat(hop=1103),
        "n_mels": lambda: feat(n_mels=0),
        "T_max": lambda: feat(T_max=3),
        "row stride": lambda: feat(ld=2000),
        "n_max": lambda: feat(n_max=1024, ld=1024),
        "max_db": lambda: feat(max_db=0.0),
        "null": lambda: feat(basis=None),
        "in place": lambda: L.unast_preemphasis(p_(y), 2200, p_(y), 2200, 2200, None, p_(one), 1, 0.97, None),
        "row strides": lambda: L.unast_preemphasis(p_(y), 2200, p_(out), 2000, 2200, None, p_(one), 1, 0.97, None),
        "B=0": lambda: L.unast_preemphasis(p_(y), 2200, p_(out), 2200, 2200, None, p_(one), 0, 0.97, None),
    }
    for word, call in calls.items():
        assert call() == -1, word
        assert word in L.unast_last_error().decode(), (word, L.unast_last_error().decode())
    torch.cuda.synchronize()
    assert bool((mel == 7.0).all()) and bool((mag == 7.0).all()) and bool((out == 7.0).all())
    assert feat() == 0                                                                     # the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert bool((mel == float(LOW)).all()) and bool((mag == float(LOW)).all())
