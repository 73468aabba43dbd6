"""What the feature extraction (unast_amd/audio.py: get_spectrograms and its batch form; the features kernel of csrc/audio.hip) rests on, checked
without a GPU: the mel basis meets the check values of a float64 prototype of its definition; header, ops, audio, utils and the documents
agree; load_wav reads what write_wav wrote and refuses what is not built; every refusal comes before any launch; the input conditions the
GPU test builds its bounds on hold for the mirror alone."""
import os
import re
import wave

import numpy as np
import pytest
import torch

from tests import features_mirror as F
from tests import griffin_lim_mirror as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"unast_features": 22, "unast_preemphasis": 10, "unast_stft": 13}


def _ap(p):
    from unast_amd.audio import AudioParams
    return AudioParams(n_fft=p.n_fft, hop=p.hop, win=p.win, sr=p.sr, n_mels=p.n_mels)


def test_mel_basis_meets_the_check_values():
    from unast_amd import audio
    W, r = audio.mel_basis(audio.AudioParams())
    assert W.dtype == np.float32 and W.shape == (80, 1025) and r.dtype == np.int32 and r.shape == (80, 2)
    assert int((W != 0).sum()) == 2001 and (r[:, 1] > r[:, 0]).all()
    assert int((r[:, 1] - r[:, 0]).max()) == 83
    assert tuple(r[0]) == (1, 8) and tuple(r[79]) == (941, 1024)
    assert abs(float(W.max()) - 0.0241469014) <= 1e-9
    total = float(W.astype(np.float64).sum())
    assert abs(total - 7.42989098) <= 1e-7 and abs(total * 22050 / 2048 - 80.0) < 0.05          # 80.0: area 1 per filter, sampled at the bins
    assert abs(float(F.mel_edges(F.DEFAULT)[1]) - 41.078679) <= 1e-6
    W2, r2 = audio.mel_basis(_ap(F.SMALL80))
    assert int((W2 != 0).sum()) == 249 and int((r2[:, 1] == r2[:, 0]).sum()) == 2 and (r2[r2[:, 1] == r2[:, 0]] == 0).all()
    W3, r3 = audio.mel_basis(_ap(F.SMALL))
    assert int((W3 != 0).sum()) == 234 and int((r3[:, 1] - r3[:, 0]).max()) == 35
    for p, (Wa, ra) in ((F.DEFAULT, (W, r)), (F.SMALL80, (W2, r2)), (F.SMALL, (W3, r3))):
        Wm, rm = F.mel_basis(p)                                                            # the mirror's own statement of the definition
        assert np.array_equal(Wa, Wm) and np.array_equal(ra, rm)
        assert (Wa >= 0).all()
        for i in range(Wa.shape[0]):                                                       # each row's nonzeros are contiguous and are the range
            nz = np.flatnonzero(Wa[i])
            assert (nz.size == 0 and tuple(ra[i]) == (0, 0)) or (nz[0] == ra[i, 0] and nz[-1] + 1 == ra[i, 1] and nz.size == ra[i, 1] - ra[i, 0])
    assert audio.mel_basis(audio.AudioParams())[0] is W, "cached"
    with pytest.raises(ValueError):
        W[0, 0] = 1.0                                                                      # read-only
    with pytest.raises(ValueError, match="n_mels"):
        audio.mel_basis(audio.AudioParams(n_mels=0))


def test_mirror_preemphasis_is_the_reference_line():
    y = (G.signal(500, seed=2) * 0.9).astype(np.float32)
    want = np.append(y[0], y[1:] - 0.97 * y[:-1])                                           # src/utils.py:251 as written
    assert want.dtype == np.float32 and np.array_equal(F.preemphasis(y).view(np.int32), want.view(np.int32))
    assert np.array_equal(F.preemphasis(y[:1]), y[:1])


def test_header_ops_and_documents_agree():
    from unast_amd import audio, ops, utils
    from unast_amd._lib import parse_header
    protos = parse_header()
    assert {k: len(protos[k][1]) for k in ENTRIES} == ENTRIES
    for name in ("features", "preemphasis"):
        assert callable(getattr(ops, name))
    n = len(protos)
    for doc, pat in (("README.md", r"the C ABI \((\d+) entry points\)"), ("INTEGRATION.md", r"for every entry point \((\d+)\)")):
        m = re.search(pat, open(os.path.join(ROOT, doc)).read())
        assert m and int(m.group(1)) == n, (doc, m and m.group(1), n)
    src = open(os.path.join(ROOT, "unast_amd", "csrc", "audio.hip")).read()
    for k in ("unast_features", "unast_preemphasis"):
        assert re.search(r'extern "C" int %s\(' % k, src), k
    assert utils.get_spectrograms is audio.get_spectrograms
    for name in ("mel_basis", "preemphasis", "get_spectrograms_batch", "load_wav", "get_spectrograms", "prepare_data"):
        assert callable(getattr(audio, name))
    ap = audio.AudioParams()
    assert ap.n_mels == 80 and list(ap.__dataclass_fields__)[-1] == "n_mels"
    assert audio.AudioParams(n_fft=256, hop=64, win=200).n_mels == 80                       # existing keyword constructions keep working
    assert all(getattr(ap, f) == getattr(F.DEFAULT, f) for f in ("n_fft", "hop", "win", "preemphasis", "max_db", "ref_db", "sr", "n_mels"))
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "get_spectrograms" in open(os.path.join(ROOT, doc)).read(), doc
    assert "bench_features.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert "## 5r." in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_load_wav_round_trip_and_refusals(tmp_path):
    from unast_amd import audio
    x = (0.8 * G.signal(3000, seed=1)).astype(np.float32)
    path = audio.write_wav(str(tmp_path / "a.wav"), x, 22050)
    y = audio.load_wav(path)
    assert y.dtype == np.float32 and y.shape == (3000,)
    assert np.abs(y - x).max() <= 1.0 / 32768 + 1e-7, "within one 16-bit step"
    with wave.open(path, "rb") as f:
        pcm = np.frombuffer(f.readframes(3000), dtype="<i2")
    assert np.array_equal(y, pcm.astype(np.float32) / np.float32(32768))                   # int / 2^15, as librosa.load reads it

    def write(name, data, channels, width, rate):
        with wave.open(str(tmp_path / name), "wb") as f:
            f.setnchannels(channels)
            f.setsampwidth(width)
            f.setframerate(rate)
            f.writeframes(data)
        return str(tmp_path / name)
    stereo = np.stack([pcm, -pcm // 2], axis=1).astype("<i2")
    ys = audio.load_wav(write("s.wav", stereo.tobytes(), 2, 2, 22050))
    assert ys.shape == (3000,) and np.abs(ys - stereo.astype(np.float64).mean(axis=1) / 32768).max() <= 1e-7
    with pytest.raises(ValueError, match="44100 Hz.*resampling is not built"):
        audio.load_wav(write("r.wav", pcm.tobytes(), 1, 2, 44100))
    with pytest.raises(ValueError, match="8-bit"):
        audio.load_wav(write("b.wav", bytes(3000), 1, 1, 22050))
    with pytest.raises(ValueError, match="resampling is not built"):
        audio.get_spectrograms(write("r2.wav", pcm.tobytes(), 1, 2, 16000))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="CUDA"):
            audio.get_spectrograms(path)


def test_refusals_come_before_any_launch():
    """On CPU tensors: each refusal names its reason (a launch would have raised TypeError for the device first)."""
    from unast_amd import audio, ops
    A = audio.AudioParams
    ok = torch.zeros(2, 3000)
    with pytest.raises(ValueError, match="utterance 1 has 1024 samples, too short.*n_fft / 2 = 1024"):
        audio.get_spectrograms_batch(ok, [3000, 1024])
    with pytest.raises(ValueError, match="utterance 0 has 128 samples"):
        audio.get_spectrograms_batch(torch.zeros(1, 500), [128], A(n_fft=256, hop=64, win=200, n_mels=20), trim=False)
    with pytest.raises(ValueError, match="pad_mode"):
        audio.get_spectrograms_batch(ok, [3000, 3000], pad_mode="edge")
    for n_fft in (128, 300, 4096):
        with pytest.raises(ValueError, match="n_fft must be one of"):
            audio.get_spectrograms_batch(ok, [3000, 3000], A(n_fft=n_fft, hop=32, win=100))
    with pytest.raises(ValueError, match="win must not exceed n_fft"):
        audio.get_spectrograms_batch(ok, [3000, 3000], A(n_fft=256, hop=64, win=300))
    with pytest.raises(ValueError, match="hop must be in 1..win"):
        audio.get_spectrograms_batch(ok, [3000, 3000], A(hop=0))
    with pytest.raises(ValueError, match="n_mels must be positive"):
        audio.get_spectrograms_batch(ok, [3000, 3000], A(n_mels=0))
    with pytest.raises(ValueError, match="2 rows, 1 lengths"):
        audio.get_spectrograms_batch(ok, [3000])
    with pytest.raises(ValueError, match="outside its row"):
        audio.get_spectrograms_batch(ok, [3000, 3001])
    with pytest.raises(ValueError, match="outside its row"):
        audio.get_spectrograms_batch(ok, [2500, 2500], trim=False, starts=[0, 501])
    with pytest.raises(ValueError, match="without trim"):
        audio.get_spectrograms_batch(ok, [2500, 2500], starts=[0, 5])
    with pytest.raises(ValueError, match=r"\[B, n_max\]"):
        audio.get_spectrograms_batch(torch.zeros(3000), [3000])
    # nothing runs without a GPU
    with pytest.raises(TypeError, match="CUDA"):
        audio.get_spectrograms_batch(ok, [3000, 2000])
    with pytest.raises(TypeError, match="CUDA"):
        audio.preemphasis(torch.zeros(100))
    i32 = torch.zeros(1, dtype=torch.int32)
    w, tw = torch.zeros(1102), torch.zeros(2048, dtype=torch.complex64)
    for call in (lambda: ops.preemphasis(torch.zeros(1, 10), i32, 0.97, torch.zeros(1, 10)),
                 lambda: ops.features(torch.zeros(1, 2200), None, i32, 9, 2048, 275, 1102, 0.97, w, tw, torch.zeros(80, 1025), torch.zeros(80, 2, dtype=torch.int32),
                                      20.0, 100.0, torch.zeros(1, 9, 80), torch.zeros(1, 9, 1025))):
        with pytest.raises(TypeError, match="CUDA"):
            call()


def test_trim_cases_keep_clear_of_the_threshold():
    """The trim decisions of the GPU test's batch, on the float32 signals it feeds, in both pad modes."""
    names, wavs = F.trim_batch()
    for name, w in zip(names, wavs):
        for mode in ("reflect", "constant"):
            margin = np.abs(G.frame_db(w.astype(np.float64), pad_mode=mode) + 60.0).min()
            print(name, mode, G.trim_bounds(w.astype(np.float64), pad_mode=mode), "margin %.1f dB" % margin)
            assert margin >= 3.0
    for mode in ("reflect", "constant"):
        assert [e - s for s, e in (G.trim_bounds(w.astype(np.float64), pad_mode=mode) for w in wavs)] == [8704, 6117, 6144, 8000, 6000]


def test_accuracy_cases_are_mostly_unclipped_and_reach_the_clips():
    """In every accuracy case at least half of the mirror's mel entries and half of its mag entries lie strictly inside (1e-8, 1); over the
    cases, mag reaches both clips and mel both as well; the yardsticks lie where the GPU test's docstring says."""
    hit = {"mel_lo": 0, "mel_hi": 0, "mag_lo": 0, "mag_hi": 0}
    for pn in F.PARAMS:
        p = F.PARAMS[pn]
        for name, wavs in F.accuracy_cases(pn):
            for i, w in enumerate(wavs):
                assert len(w) == F.counts(p)[i] and w.dtype == np.float32
                mel, mag, fmel, fmag = F.reference(pn, name, i)
                assert mel.shape == (F.frames_of(len(w), p), p.n_mels) and mag.shape == (F.frames_of(len(w), p), p.n_fft // 2 + 1)
                print("%s %s n=%d: inside mel %.2f mag %.2f; float32 CPU rms mel %.3g mag %.3g" % (pn, name, len(w), F.inside(mel), F.inside(mag),
                                                                                                   F.rms(fmel, mel), F.rms(fmag, mag)))
                assert F.inside(mel) >= 0.5 and F.inside(mag) >= 0.5, (pn, name, i)
                assert F.rms(fmel, mel) <= 2e-6 and F.rms(fmag, mag) <= 2e-5
                hit["mel_lo"] += int((mel <= 1e-8).sum())
                hit["mel_hi"] += int((mel >= 1.0).sum())
                hit["mag_lo"] += int((mag <= 1e-8).sum())
                hit["mag_hi"] += int((mag >= 1.0).sum())
    print(hit)
    assert all(v > 0 for v in hit.values()), hit
    assert abs(F.floor_(F.DEFAULT) - 1.14e-7) <= 1e-9
    # silence and an empty filter are the lower clip; float32(1e-8) is what the device stores for it
    mel, mag, _ = F.features(np.zeros(2200, dtype=np.float32), F.DEFAULT)
    assert (mel == 1e-8).all() and (mag == 1e-8).all() and abs(F.LOW - 1e-8) < 1e-15
