"""What the waveform synthesis (unast_amd/audio.py, csrc/audio.hip) rests on, checked without a GPU: the float64 mirror's transforms equal
torch's in float64; its de-preemphasis is lfilter's recurrence; trim on hand-made signals; the float32 CPU yardsticks and input conditions the GPU
test builds its bounds on; header, ops and the documents agree; the kernel file keeps its constraints; every refusal raises with its reason
and nothing runs without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests import griffin_lim_mirror as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"unast_stft": 13, "unast_istft_frames": 10, "unast_overlap_add": 11, "unast_gl_prepare": 10, "unast_deemphasis": 8, "unast_trim_bounds": 13}


@pytest.mark.parametrize("p", [G.DEFAULT, G.SMALL], ids=["default", "small"])
@pytest.mark.parametrize("T", [5, 6, 9, 40])
def test_mirror_transforms_equal_torch_float64(p, T):
    y, _ = G.utterance(T, p, seed=T)
    S = G.stft(y, p)
    assert S.shape == (T, p.n_fft // 2 + 1)
    St = G.torch_stft(y, p, torch.float64).numpy()
    rng = np.random.default_rng(T)
    R = rng.standard_normal(S.shape) + 1j * rng.standard_normal(S.shape)          # not a consistent spectrogram; imaginary DC / Nyquist bins too
    yi, yt = G.istft(R, p), G.torch_istft(R, p, torch.float64).numpy()
    assert yi.shape == (p.hop * (T - 1),)
    print("stft", np.abs(S - St).max(), "istft", np.abs(yi - yt).max(), "round trip", G.rel(G.istft(S, p), y))
    assert np.abs(S - St).max() <= 1e-12 and np.abs(yi - yt).max() <= 1e-12
    assert G.rel(G.istft(S, p), y) <= 1e-12
    R0 = R.copy()
    R0[:, 0], R0[:, -1] = R0[:, 0].real, R0[:, -1].real
    assert np.array_equal(G.istft(R0, p), yi), "irfft ignores the imaginary parts of the DC and Nyquist bins"


def test_mirror_deemphasis_is_the_recurrence():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(300)
    y = np.zeros(300)
    for k in range(300):
        y[k] = x[k] + (0.97 * y[k - 1] if k else 0.0)
    assert np.abs(G.deemphasis(x) - y).max() <= 1e-13


def test_trim_on_hand_made_signals():
    y = np.zeros(8192)
    y[3000:5000] = 0.5
    # frames of 2048 centred at 512 i: frame i holds samples [512 i - 1024, 512 i + 1024); the first with a loud sample is i = 4, the last i = 11
    for mode in ("reflect", "constant"):
        assert G.trim_bounds(y, pad_mode=mode) == (4 * 512, 12 * 512)
    # a burst in the first 8 samples: reflect padding mirrors 7 of them into the frames that reach the padding (15 loud samples in the loudest
    # frame), zero padding does not (8).  A background 60 dB below a frame of 11 loud samples is then silent under 'reflect' and kept under 'constant'.
    z = np.full(4096, np.sqrt(1e-6 * 11 / 2048))
    z[:8] = 1.0
    assert G.trim_bounds(z, pad_mode="reflect") == (0, 3 * 512)
    assert G.trim_bounds(z, pad_mode="constant") == (0, 4096)
    assert G.trim_bounds(np.zeros(3000)) == (0, 3000), "all frames of a silent signal sit at the loudest frame's level"
    assert G.trim_bounds(np.full(3000, 0.1)) == (0, 3000)


def test_yardsticks_and_input_conditions():
    """The float32 CPU path against the mirror on the generator's signal: the figures the GPU bounds are multiples of."""
    p = G.DEFAULT
    y, M = G.utterance(40, p, seed=40)
    S = G.stft(y, p)
    rng = np.random.default_rng(40)
    R = rng.standard_normal(S.shape) + 1j * rng.standard_normal(S.shape)
    e_stft = G.rel(G.torch_stft(y, p).numpy(), S)
    e_istft = G.rel(G.torch_istft(R, p).numpy(), G.istft(R, p))
    _, X30 = G.griffin_lim(M, p, 30, return_state=True)
    e_one = G.rel(G.f32_gl_step(torch.from_numpy(X30.astype(np.complex64)), torch.from_numpy(M.astype(np.float32)), p).numpy(),
                  G.gl_step(X30.astype(np.complex64), M.astype(np.float32), p))
    y60 = G.griffin_lim(M.astype(np.float32), p)
    e_60 = G.rel(G.f32_griffin_lim(M, p).numpy(), y60)
    print("float32 CPU vs mirror: stft %.3g istft %.3g one iteration %.3g sixty iterations %.3g" % (e_stft, e_istft, e_one, e_60))
    assert e_stft < 10 * 1.4e-7 and e_istft < 10 * 9e-8 and e_one < 10 * 4e-7 and e_60 < 10 * 4e-4
    assert np.isfinite(y60).all() and np.abs(y60).max() > 0.05


def test_trim_cases_keep_clear_of_the_threshold():
    for name, y in G.trim_cases().items():
        for mode in ("reflect", "constant"):
            margin = np.abs(G.frame_db(y, pad_mode=mode) + 60.0).min()
            print(name, mode, G.trim_bounds(y, pad_mode=mode), "margin %.1f dB" % margin)
            assert margin >= 3.0
    # the end-to-end utterances: float32 must not be able to flip a decision there either
    for T in G.RAGGED:
        w, _ = G.cached(("s2w", T), lambda: G.spectrogram2wav(G.normalised_mag(T, G.DEFAULT, T), G.DEFAULT, trim=False))
        for mode in ("reflect", "constant"):
            assert np.abs(G.frame_db(w, pad_mode=mode) + 60.0).min() >= 3.0


def test_header_ops_and_documents_agree():
    from unast_amd import audio, ops, utils
    from unast_amd._lib import parse_header
    protos = parse_header()
    assert {k: len(protos[k][1]) for k in ENTRIES} == ENTRIES
    for name in ("stft", "istft_frames", "overlap_add", "gl_prepare", "deemphasis", "trim_bounds"):
        assert callable(getattr(ops, name))
    n = len(protos)
    for doc, pat in (("README.md", r"the C ABI \((\d+) entry points\)"), ("INTEGRATION.md", r"for every entry point \((\d+)\)")):
        m = re.search(pat, open(os.path.join(ROOT, doc)).read())
        assert m and int(m.group(1)) == n, (doc, m and m.group(1), n)
    for name in ("spectrogram2wav", "griffin_lim", "invert_spectrogram"):
        assert getattr(utils, name) is getattr(audio, name)
    ap = audio.AudioParams()
    assert (ap.n_fft, ap.hop, ap.win, ap.preemphasis, ap.power, ap.max_db, ap.ref_db, ap.n_iter, ap.sr) == (2048, 275, 1102, 0.97, 1.2, 100, 20, 60, 22050)
    assert ap.bins == 1025 and ap.min_frames == 5
    with pytest.raises(Exception):
        ap.n_fft = 1024                                   # frozen
    mp = G.DEFAULT
    assert all(getattr(ap, f) == getattr(mp, f) for f in ("n_fft", "hop", "win", "preemphasis", "power", "max_db", "ref_db", "n_iter", "sr"))


def test_kernel_file_keeps_its_constraints():
    from unast_amd import ops
    src = open(os.path.join(ROOT, "unast_amd", "csrc", "audio.hip")).read()
    for k in ENTRIES:
        assert re.search(r'extern "C" int %s\(' % k, src), k
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code.lower()
    for word in ("hipfft", "rocfft", "cufft", "sincosf", "__sinf", "__cosf", "sinf(", "cosf("):
        assert word not in code.lower(), word
    for py in ("audio.py", "ops.py"):
        assert "torch.fft" not in open(os.path.join(ROOT, "unast_amd", py)).read()
    consts = {name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) for name in ("DEEMPH_THREADS", "DEEMPH_CHUNK", "FFT_MAX")}
    assert consts["DEEMPH_CHUNK"] == ops.DEEMPH_CHUNK and consts["DEEMPH_THREADS"] * consts["DEEMPH_CHUNK"] == ops.DEEMPH_TILE
    assert consts["FFT_MAX"] == max(ops.STFT_SIZES) and ops.STFT_SIZES == (256, 512, 1024, 2048)


def test_refusals_come_before_any_launch():
    """On CPU tensors: each refusal names its reason (a launch would have raised TypeError for the device first)."""
    from unast_amd import audio
    A = audio.AudioParams
    ok = torch.zeros(2, 6, 1025)
    with pytest.raises(ValueError, match="too short.*5 frames"):
        audio.spectrogram2wav_batch(torch.zeros(1, 4, 1025), [4])
    with pytest.raises(ValueError, match="too short"):
        audio.spectrogram2wav_batch(ok, [6, 4])
    with pytest.raises(ValueError, match="too short"):
        audio.spectrogram2wav(np.zeros((4, 1025), np.float32))
    with pytest.raises(ValueError, match="too short"):
        audio.stft(torch.zeros(275 * 3))
    for n_fft in (128, 300, 4096):
        with pytest.raises(ValueError, match="n_fft must be one of"):
            audio.spectrogram2wav_batch(torch.zeros(1, 40, n_fft // 2 + 1), [40], A(n_fft=n_fft, hop=32, win=100))
    with pytest.raises(ValueError, match="win must not exceed n_fft"):
        audio.spectrogram2wav_batch(torch.zeros(1, 40, 129), [40], A(n_fft=256, hop=64, win=300))
    with pytest.raises(ValueError, match="win must not exceed n_fft"):
        audio.istft(torch.zeros(40, 129, dtype=torch.complex64), None, A(n_fft=256, hop=64, win=300))
    with pytest.raises(ValueError, match="last dimension must be 1 \\+ n_fft/2 = 1025"):
        audio.spectrogram2wav_batch(torch.zeros(1, 6, 1024), [6])
    with pytest.raises(ValueError, match="last dimension"):
        audio.griffin_lim(torch.zeros(6, 1024))
    with pytest.raises(ValueError, match="last dimension"):
        audio.spectrogram2wav(np.zeros((6, 1024), np.float32))
    with pytest.raises(ValueError, match="beyond the 6 frames"):
        audio.spectrogram2wav_batch(ok, [6, 7])
    with pytest.raises(ValueError, match="beyond"):
        audio.istft(torch.zeros(2, 6, 1025, dtype=torch.complex64), [7, 6])
    with pytest.raises(ValueError, match="pad_mode"):
        audio.spectrogram2wav_batch(ok, [6, 6], pad_mode="edge")
    with pytest.raises(ValueError, match="2 utterances, 1 lengths"):
        audio.spectrogram2wav_batch(ok, [6])


def test_nothing_runs_without_a_gpu():
    from unast_amd import audio, ops
    from unast_amd.network import Vocoder
    with pytest.raises(TypeError, match="CUDA"):
        audio.spectrogram2wav_batch(torch.zeros(2, 6, 1025), [6, 5])
    with pytest.raises(TypeError, match="CUDA"):
        audio.stft(torch.zeros(275 * 5))
    with pytest.raises(TypeError, match="CUDA"):
        audio.istft(torch.zeros(6, 1025, dtype=torch.complex64))
    with pytest.raises(TypeError, match="CUDA"):
        audio.griffin_lim(torch.zeros(6, 1025))
    with pytest.raises(TypeError, match="CUDA"):
        audio.deemphasis(torch.zeros(100))
    with pytest.raises(TypeError, match="CUDA"):
        audio.trim_bounds(torch.zeros(3000))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="CUDA"):
            audio.spectrogram2wav(np.zeros((6, 1025), np.float32))
    voc = Vocoder(80, 256, 2048).eval()
    with pytest.raises(ValueError, match="CUDA"):
        audio.mel2wav(voc, torch.zeros(1, 6, 80), [6])
    i32, c64 = torch.zeros(1, dtype=torch.int32), torch.zeros(1, 6, 1025, dtype=torch.complex64)
    w, tw = torch.zeros(1102), torch.zeros(2048, dtype=torch.complex64)
    for call in (lambda: ops.stft(torch.zeros(1, 1375), i32, 6, 2048, 275, 1102, w, tw, c64),
                 lambda: ops.istft_frames(c64, i32, 2048, 1102, w, tw, torch.zeros(1, 6, 1102)),
                 lambda: ops.overlap_add(torch.zeros(1, 6, 1102), i32, 2048, 275, w, torch.zeros(1, 1375)),
                 lambda: ops.gl_prepare(torch.zeros(1, 6, 1025), 100.0, 20.0, 1.2, torch.zeros(1, 6, 1025)),
                 lambda: ops.deemphasis(torch.zeros(1, 10), i32, 0.97, torch.zeros(1, 10)),
                 lambda: ops.trim_bounds(torch.zeros(1, 3000), i32, 60.0, 2048, 512, "reflect")):
        with pytest.raises(TypeError, match="CUDA"):
            call()
