"""Waveform synthesis on HIP: the reference's spectrogram2wav (src/utils.py:281-328 -- de-normalise, Griffin-Lim with istft / stft, de-preemphasis,
trim) for whole batches, every arithmetic step a kernel of csrc/audio.hip.  DESIGN.md section 5q states the definitions: librosa's stft / istft
at the reference's settings written out (centred frames, reflect padding, a periodic Hann window of `win` samples centred in n_fft, overlap-add
divided by the window's sum of squares, hop * (T - 1) samples for T frames), scipy's lfilter for the de-preemphasis, and librosa.effects.trim
with its one version-dependent choice, the padding mode of the frame RMS, as an argument.

Spectra are frame-major [frames, 1 + n_fft/2], the layout Vocoder.forward produces, so the reference's transposes do not occur.  One
Griffin-Lim iteration is three launches (inverse transforms, overlap-add gather, forward transforms with the phase update in their epilogue);
the utterances of a batch run side by side and each one's result is bit-identical to running it alone.

`librosa.griffinlim` as gl_vocoder.py calls it (fast Griffin-Lim: 32 iterations, momentum 0.99, random initial phase) is `griffinlim`, and
method='librosa' of spectrogram2wav_batch / spectrogram2wav / mel2wav / vocode: the momentum update is a second
epilogue of the forward transform, the random phase a seeded counter-based draw over the n_fft levels of the twiddle table, so that a run
can be repeated and tested; the deterministic path stays the default.

The other direction, feature extraction: the reference's get_spectrograms (src/utils.py:235-278 -- load, trim, preemphasis, stft, |S|, mel
basis, dB, normalise, clip) and prepare_data.py's loop over a folder of wavs, a batch of utterances per launch.  The mel
basis is librosa.filters.mel at its defaults written out; resampling is not built, so a file at another rate than sr is refused."""
import os
import wave
from dataclasses import dataclass

import numpy as np
import torch

from . import ops

_F32 = torch.float32


@dataclass(frozen=True)
class AudioParams:
    """The reference's audio settings (src/audio_parameters.py: n_fft :4, sr :5, preemphasis :8, hop_length = int(sr * 0.0125) :9-11,
    win_length = int(sr * 0.05) :10-12, power :14, max_db :17, ref_db :18, n_iter :19, n_mels :13)."""
    n_fft: int = 2048
    hop: int = 275
    win: int = 1102
    preemphasis: float = 0.97
    power: float = 1.2
    max_db: float = 100.0
    ref_db: float = 20.0
    n_iter: int = 60
    sr: int = 22050
    n_mels: int = 80

    @property
    def bins(self):
        return self.n_fft // 2 + 1

    @property
    def min_frames(self):
        """The signal of an utterance, hop * (frames - 1) samples, must be longer than the reflect padding n_fft / 2."""
        return self.n_fft // (2 * self.hop) + 2


def _check_params(who, p):
    if p.n_fft not in ops.STFT_SIZES:
        raise ValueError("%s: n_fft must be one of %s (got %r)" % (who, ops.STFT_SIZES, p.n_fft))
    if not 1 <= p.win <= p.n_fft:
        raise ValueError("%s: win must not exceed n_fft (win=%r, n_fft=%d): a longer window has no centred padding" % (who, p.win, p.n_fft))
    if p.hop < 1 or p.hop > p.win:
        raise ValueError("%s: hop must be in 1..win (got %r): a larger hop leaves samples no frame covers" % (who, p.hop))
    if p.n_iter < 0:
        raise ValueError("%s: n_iter must not be negative" % who)


def _check_lens(who, lens, T, p):
    """lens as a list of ints, each within min_frames..T."""
    lens = [int(n) for n in (lens.tolist() if hasattr(lens, "tolist") else lens)]
    if not lens:
        raise ValueError("%s: empty batch" % who)
    for n in lens:
        if n > T:
            raise ValueError("%s: a length of %d frames lies beyond the %d frames given" % (who, n, T))
        if n < p.min_frames:
            raise ValueError("%s: an utterance of %d frames is too short: n_fft // (2 * hop) + 2 = %d frames are needed for the signal to be longer "
                             "than the reflect padding of %d samples" % (who, n, p.min_frames, p.n_fft // 2))
    return lens


def _need_cuda(who, t, name):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise TypeError("%s: %s must be a CUDA tensor: the transforms are HIP kernels and have no CPU path" % (who, name))


_TABLES = {}


def _tables(p, device):
    """(window float32 [win], twiddle complex64 [n_fft]) on the device, computed in float64 and rounded once."""
    key = (p.n_fft, p.win, str(device))
    if key not in _TABLES:
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(p.win, dtype=np.float64) / p.win)           # periodic Hann
        ang = -2.0 * np.pi * np.arange(p.n_fft, dtype=np.float64) / p.n_fft
        tw = (np.cos(ang) + 1j * np.sin(ang)).astype(np.complex64)
        _TABLES[key] = (torch.from_numpy(w.astype(np.float32)).to(device), torch.from_numpy(tw).to(device))
    return _TABLES[key]


def _i32(values, device):
    return torch.tensor(values, dtype=torch.int32, device=device)


def stft(y, frames=None, params=AudioParams()):
    """librosa.stft(y, n_fft, hop, win_length=win) frame-major: y [n] or [B, n_max] float32 -> complex64 [T, bins] or [B, T_max, bins].
    frames (ints, optional): utterance b has hop * (frames[b] - 1) valid samples; by default every row is taken whole, and n_max must then be
    a multiple of hop.  Rows of the result at or behind frames[b] are left unwritten (zero here)."""
    p = params
    _check_params("stft", p)
    single = torch.is_tensor(y) and y.dim() == 1
    y2 = y.unsqueeze(0) if single else y
    if not torch.is_tensor(y2) or y2.dim() != 2:
        raise ValueError("stft: y must be [n] or [B, n]")
    B, n_max = y2.shape
    if frames is None:
        if n_max % p.hop != 0:
            raise ValueError("stft: %d samples are no multiple of hop = %d; give frames" % (n_max, p.hop))
        frames = [1 + n_max // p.hop] * B
    T = 1 + n_max // p.hop
    frames = _check_lens("stft", frames, T, p)
    if len(frames) != B:
        raise ValueError("stft: %d rows, %d frame counts" % (B, len(frames)))
    _need_cuda("stft", y2, "y")
    T_max = max(frames)
    window, tw = _tables(p, y2.device)
    spec = torch.zeros(B, T_max, p.bins, dtype=torch.complex64, device=y2.device)
    ops.stft(y2 if y2.stride(1) == 1 else y2.contiguous(), _i32(frames, y2.device), T_max, p.n_fft, p.hop, p.win, window, tw, spec)
    return spec[0] if single else spec


def _istft_into(spec, frames_dev, p, window, tw, fr, y):
    ops.istft_frames(spec, frames_dev, p.n_fft, p.win, window, tw, fr)
    return ops.overlap_add(fr, frames_dev, p.n_fft, p.hop, window, y)


def _check_spec(who, S, p, complex_):
    if not torch.is_tensor(S) or S.dim() not in (2, 3):
        raise ValueError("%s: a [T, %d] or [B, T, %d] tensor is needed" % (who, p.bins, p.bins))
    if S.shape[-1] != p.bins:
        raise ValueError("%s: the last dimension must be 1 + n_fft/2 = %d (got %d)" % (who, p.bins, S.shape[-1]))
    if S.is_complex() != complex_:
        raise TypeError("%s: a %s tensor is needed (got %s)" % (who, "complex64" if complex_ else "float32", S.dtype))
    single = S.dim() == 2
    return (S.unsqueeze(0) if single else S), single


def istft(S, lens=None, params=AudioParams()):
    """librosa.istft(S, hop, win_length=win) for frame-major complex64 S [T, bins] or [B, T, bins] -> float32 [hop (T-1)] or [B, hop (T_max-1)];
    lens (frames per utterance, optional): samples behind hop * (lens[b] - 1) are left unwritten (zero here)."""
    p = params
    _check_params("istft", p)
    S3, single = _check_spec("istft", S, p, True)
    B, T = S3.shape[0], S3.shape[1]
    lens = _check_lens("istft", [T] * B if lens is None else lens, T, p)
    if len(lens) != B:
        raise ValueError("istft: %d utterances, %d lengths" % (B, len(lens)))
    _need_cuda("istft", S3, "S")
    dev = S3.device
    window, tw = _tables(p, dev)
    fr = torch.empty(B, T, p.win, dtype=_F32, device=dev)
    y = torch.zeros(B, p.hop * (T - 1), dtype=_F32, device=dev)
    _istft_into(S3.contiguous(), _i32(lens, dev), p, window, tw, fr, y)
    return y[0] if single else y


def _griffin_lim(M, X, frames_dev, p, n_iter, y):
    """The iteration of src/utils.py:309-320 on M float32 / X complex64 [B,T,bins] (X = M on entry; overwritten) into y [B, hop (T-1)]."""
    B, T = M.shape[0], M.shape[1]
    window, tw = _tables(p, M.device)
    fr = torch.empty(B, T, p.win, dtype=_F32, device=M.device)
    for _ in range(n_iter):
        _istft_into(X, frames_dev, p, window, tw, fr, y)
        ops.stft(y, frames_dev, T, p.n_fft, p.hop, p.win, window, tw, X, mag=M)
    return _istft_into(X, frames_dev, p, window, tw, fr, y)


def griffin_lim(M, lens=None, params=AudioParams(), n_iter=None, X0=None, return_state=False):
    """src/utils.py:309-320 for a frame-major magnitude M (float32, non-negative, [T, bins] or [B, T, bins]): X = M; n_iter times
    X = M * e / max(1e-8, |e|) with e = stft(istft(X)); returns istft(X), float32 [hop (T-1)] or [B, hop (T_max-1)].
    X0 (complex64, same shape; optional) replaces the initial X = M: a single iteration from a given state.  return_state: (waveform, X), X the
    complex64 spectrum of the last iterate."""
    p = params
    _check_params("griffin_lim", p)
    M3, single = _check_spec("griffin_lim", M, p, False)
    B, T = M3.shape[0], M3.shape[1]
    lens = _check_lens("griffin_lim", [T] * B if lens is None else lens, T, p)
    if len(lens) != B:
        raise ValueError("griffin_lim: %d utterances, %d lengths" % (B, len(lens)))
    _need_cuda("griffin_lim", M3, "M")
    dev = M3.device
    M3 = M3.contiguous()
    if X0 is None:
        X = torch.complex(M3, torch.zeros_like(M3))
    else:
        X3, _ = _check_spec("griffin_lim", X0, p, True)
        if X3.shape != M3.shape:
            raise ValueError("griffin_lim: X0 and M differ in shape")
        X = X3.contiguous().clone()
    y = torch.zeros(B, p.hop * (T - 1), dtype=_F32, device=dev)
    _griffin_lim(M3, X, _i32(lens, dev), p, p.n_iter if n_iter is None else n_iter, y)
    if return_state:
        return (y[0], X[0]) if single else (y, X)
    return y[0] if single else y


GL_METHODS = ("reference", "librosa")
LIBROSA_N_ITER, LIBROSA_MOMENTUM = 32, 0.99          # librosa.griffinlim's defaults, what src/gl_vocoder.py:26 runs with


def _alpha(momentum):
    """momentum / (1 + momentum) in double, rounded to the float32 the kernel multiplies by."""
    return float(np.float32(momentum / (1.0 + momentum)))


def _check_seed(who, seed):
    if not 0 <= int(seed) < 1 << 32:
        raise ValueError("%s: seed must fit 32 bits (got %r)" % (who, seed))


def _check_method(who, method, seed):
    if method not in GL_METHODS:
        raise ValueError("%s: method is 'reference' (src/utils.py:309-320) or 'librosa' (librosa.griffinlim, src/gl_vocoder.py:26), got %r" % (who, method))
    _check_seed(who, seed)


def _check_keys(who, keys, B):
    """keys as a list of B uint32 values; by default an utterance's index in the batch."""
    keys = list(range(B)) if keys is None else [int(k) for k in (keys.tolist() if hasattr(keys, "tolist") else keys)]
    if len(keys) != B:
        raise ValueError("%s: %d utterances, %d keys" % (who, B, len(keys)))
    if any(not 0 <= k < 1 << 32 for k in keys):
        raise ValueError("%s: a key must fit 32 bits (got %s)" % (who, keys))
    return keys


def _keys_dev(keys, device):
    return torch.from_numpy(np.array(keys, dtype=np.uint32).view(np.int32)).to(device)


def _random_phase(M, X, frames_dev, keys, seed, p):
    """X = M * exp(i phase), the phase drawn per (seed, key, frame, bin) from the n_fft levels of the twiddle table."""
    _, tw = _tables(p, M.device)
    return ops.gl_random_phase(M, frames_dev, _keys_dev(keys, M.device), seed, p.n_fft, tw, X)


def _fast_griffin_lim(M, X, tprev, frames_dev, p, n_iter, alpha, y):
    """librosa.griffinlim's loop on M float32 / X = M * angles0 complex64 [B,T,bins] (overwritten) into y [B, hop (T-1)].  tprev complex64
    [B,T,bins] is workspace: the first iteration runs with alpha = 0 (tprev = 0 by definition) and does not read it, so it may be fresh memory."""
    B, T = M.shape[0], M.shape[1]
    window, tw = _tables(p, M.device)
    fr = torch.empty(B, T, p.win, dtype=_F32, device=M.device)
    for i in range(n_iter):
        _istft_into(X, frames_dev, p, window, tw, fr, y)
        ops.stft_momentum(y, frames_dev, T, p.n_fft, p.hop, p.win, window, tw, X, M, alpha if i else 0.0, tprev)
    return _istft_into(X, frames_dev, p, window, tw, fr, y)


def griffinlim(S, lens=None, params=AudioParams(), n_iter=LIBROSA_N_ITER, momentum=LIBROSA_MOMENTUM, init="random", seed=0, keys=None, angles0=None,
               return_state=False):
    """librosa.griffinlim(S, n_iter, hop_length=hop, win_length=win, momentum=momentum) (src/gl_vocoder.py:26; fast Griffin-Lim, Perraudin et
    al.) for a frame-major magnitude S (float32, non-negative, [T, bins] or [B, T, bins]): ang = angles0, tprev = 0; n_iter times e =
    stft(istft(S * ang)), c = e - momentum / (1 + momentum) * tprev, tprev = e, ang = c / (|c| + 1e-16); returns istft(S * ang), float32
    [hop (T-1)] or [B, hop (T_max-1)].  init: 'random' -- a phase per (seed, key, frame, bin) uniform over n_fft levels, keys one uint32 per
    utterance (default: its index), so that a draw does not depend on the batch (librosa draws a continuous phase from an unseeded generator) --
    or None, all phases zero.  angles0 (complex64, S's shape) overrides init.  return_state: (waveform, X, tprev), the last iterate S * ang and
    the last rebuilt spectrum."""
    who = "griffinlim"
    p = params
    _check_params(who, p)
    if int(n_iter) != n_iter or n_iter < 0:
        raise ValueError("%s: n_iter must be a non-negative integer (got %r)" % (who, n_iter))
    if not 0.0 <= momentum < 1.0:
        raise ValueError("%s: momentum must lie in [0, 1) (got %r)" % (who, momentum))
    if angles0 is None and init not in (None, "random"):
        raise ValueError("%s: init is 'random' or None (got %r)" % (who, init))
    _check_seed(who, seed)
    S3, single = _check_spec(who, S, p, False)
    B, T = S3.shape[0], S3.shape[1]
    lens = _check_lens(who, [T] * B if lens is None else lens, T, p)
    if len(lens) != B:
        raise ValueError("%s: %d utterances, %d lengths" % (who, B, len(lens)))
    keys = _check_keys(who, keys, B)
    if angles0 is not None:
        A3, _ = _check_spec(who, angles0, p, True)
        if A3.shape != S3.shape:
            raise ValueError("%s: angles0 and S differ in shape" % who)
    _need_cuda(who, S3, "S")
    dev = S3.device
    M = S3.contiguous()
    frames_dev = _i32(lens, dev)
    if angles0 is not None:
        _need_cuda(who, A3, "angles0")
        X = (M * A3).contiguous()
    elif init is None:
        X = torch.complex(M, torch.zeros_like(M))
    else:
        X = _random_phase(M, torch.zeros(B, T, p.bins, dtype=torch.complex64, device=dev), frames_dev, keys, seed, p)
    tprev = torch.zeros_like(X)
    y = torch.zeros(B, p.hop * (T - 1), dtype=_F32, device=dev)
    _fast_griffin_lim(M, X, tprev, frames_dev, p, int(n_iter), _alpha(momentum), y)
    if return_state:
        return (y[0], X[0], tprev[0]) if single else (y, X, tprev)
    return y[0] if single else y


def invert_spectrogram(S, params=AudioParams()):
    """src/utils.py:323-328 (frame-major)."""
    return istft(S, None, params)


def deemphasis(y, lens=None, coef=AudioParams.preemphasis):
    """scipy.signal.lfilter([1], [1, -coef], y) (src/utils.py:301) for y [n] or [B, n]; lens: samples per row (default: all)."""
    _need_cuda("deemphasis", y, "y")
    single = y.dim() == 1
    y2 = (y.unsqueeze(0) if single else y).contiguous()
    lens = [y2.shape[1]] * y2.shape[0] if lens is None else [int(n) for n in lens]
    if any(n < 0 or n > y2.shape[1] for n in lens):
        raise ValueError("deemphasis: a length lies outside 0..%d" % y2.shape[1])
    out = ops.deemphasis(y2, _i32(lens, y2.device), float(coef), torch.zeros_like(y2))
    return out[0] if single else out


def trim_bounds(y, lens=None, top_db=60.0, frame_length=2048, hop_length=512, pad_mode="reflect"):
    """(start, end) per utterance of librosa.effects.trim (src/utils.py:304), int32 [B, 2] on the device ([2] for a 1-D y)."""
    if pad_mode not in ("reflect", "constant"):
        raise ValueError("trim_bounds: pad_mode is 'reflect' (librosa 0.8) or 'constant' (later versions), got %r" % (pad_mode,))
    _need_cuda("trim_bounds", y, "y")
    single = y.dim() == 1
    y2 = (y.unsqueeze(0) if single else y).contiguous()
    lens = [y2.shape[1]] * y2.shape[0] if lens is None else [int(n) for n in lens]
    if any(n < 1 or n > y2.shape[1] for n in lens):
        raise ValueError("trim_bounds: a length lies outside 1..%d" % y2.shape[1])
    out = ops.trim_bounds(y2, _i32(lens, y2.device), float(top_db), int(frame_length), int(hop_length), pad_mode)
    return out[0] if single else out


def spectrogram2wav_batch(mags, lens, params=AudioParams(), trim=True, pad_mode="reflect", method="reference", seed=0, keys=None):
    """src/utils.py:281-306 for a batch: mags float32 [B, T, bins] normalised magnitudes (Vocoder.forward's output as it is), lens frames per
    utterance -> a list of 1-D float32 device tensors, utterance b with at most hop * (lens[b] - 1) samples (fewer after trimming).
    method 'reference': the deterministic iteration of src/utils.py:309-320, params.n_iter times.  method 'librosa': what src/gl_vocoder.py:26
    runs in its place, griffinlim with 32 iterations, momentum 0.99 and the random phase of (seed, keys) (keys: one uint32 per utterance,
    default its index in the batch)."""
    p = params
    _check_params("spectrogram2wav_batch", p)
    _check_method("spectrogram2wav_batch", method, seed)
    if pad_mode not in ("reflect", "constant"):
        raise ValueError("spectrogram2wav_batch: pad_mode is 'reflect' (librosa 0.8) or 'constant' (later versions), got %r" % (pad_mode,))
    if not torch.is_tensor(mags) or mags.dim() != 3:
        raise ValueError("spectrogram2wav_batch: mags must be [B, T, %d]" % p.bins)
    if mags.shape[2] != p.bins:
        raise ValueError("spectrogram2wav_batch: the last dimension must be 1 + n_fft/2 = %d (got %d)" % (p.bins, mags.shape[2]))
    B, T = mags.shape[0], mags.shape[1]
    lens = _check_lens("spectrogram2wav_batch", lens, T, p)
    if len(lens) != B:
        raise ValueError("spectrogram2wav_batch: %d utterances, %d lengths" % (B, len(lens)))
    if method == "librosa":
        keys = _check_keys("spectrogram2wav_batch", keys, B)
    _need_cuda("spectrogram2wav_batch", mags, "mags")
    dev = mags.device
    with torch.no_grad():
        T_max = T                                            # frames behind an utterance's length are skipped by every kernel
        M = torch.empty(B, T_max, p.bins, dtype=_F32, device=dev)
        X = torch.empty(B, T_max, p.bins, dtype=torch.complex64, device=dev)
        frames_dev = _i32(lens, dev)
        y = torch.zeros(B, p.hop * (T_max - 1), dtype=_F32, device=dev)
        if method == "librosa":
            ops.gl_prepare(mags, p.max_db, p.ref_db, p.power, M)
            _random_phase(M, X, frames_dev, keys, seed, p)
            _fast_griffin_lim(M, X, torch.empty_like(X), frames_dev, p, LIBROSA_N_ITER, _alpha(LIBROSA_MOMENTUM), y)
        else:
            ops.gl_prepare(mags, p.max_db, p.ref_db, p.power, M, X)
            _griffin_lim(M, X, frames_dev, p, p.n_iter, y)
        samples = [p.hop * (n - 1) for n in lens]
        samples_dev = _i32(samples, dev)
        ops.deemphasis(y, samples_dev, p.preemphasis, y)
        if trim:
            bounds = ops.trim_bounds(y, samples_dev, 60.0, 2048, 512, pad_mode).tolist()
        else:
            bounds = [(0, n) for n in samples]
        return [y[b, s:e] for b, (s, e) in enumerate(bounds)]


def spectrogram2wav(mag, params=AudioParams(), pad_mode="reflect", device="cuda", method="reference", seed=0):
    """The reference's signature (src/utils.py:281-306): a numpy magnitude [T, 1 + n_fft/2] -> a 1-D float32 numpy waveform; method and seed
    as in spectrogram2wav_batch (the utterance's key is 0)."""
    m = torch.as_tensor(np.asarray(mag, dtype=np.float32))
    if m.dim() != 2:
        raise ValueError("spectrogram2wav: mag must be [T, %d]" % params.bins)
    _check_params("spectrogram2wav", params)
    if m.shape[1] != params.bins:
        raise ValueError("spectrogram2wav: the last dimension must be 1 + n_fft/2 = %d (got %d)" % (params.bins, m.shape[1]))
    _check_lens("spectrogram2wav", [m.shape[0]], m.shape[0], params)
    _check_method("spectrogram2wav", method, seed)
    if not torch.cuda.is_available():
        raise RuntimeError("spectrogram2wav: needs a CUDA (ROCm) device: the transforms are HIP kernels and have no CPU path")
    return spectrogram2wav_batch(m.to(device).unsqueeze(0), [m.shape[0]], params, True, pad_mode, method, seed)[0].cpu().numpy()


def mel2wav(vocoder, mel, mel_lens, params=AudioParams(), trim=True, pad_mode="reflect", method="reference", seed=0, keys=None):
    """mel [B, T, num_mels] -> waveforms: Vocoder.forward under no_grad (src/inf_vocoder.py:56-64), then spectrogram2wav_batch (gl_vocoder.py's
    loop over the stored magnitudes: by default with the deterministic Griffin-Lim of src/utils.py, with method='librosa' with its own
    librosa.griffinlim)."""
    _check_method("mel2wav", method, seed)
    with torch.no_grad():
        mags = vocoder.forward(mel)
    return spectrogram2wav_batch(mags, mel_lens, params, trim, pad_mode, method, seed, keys)


def write_wav(path, wav, sr=AudioParams.sr):
    """16-bit PCM mono through the standard library: samples clipped to [-1, 1] and scaled by 32767."""
    x = wav.detach().cpu().numpy() if torch.is_tensor(wav) else np.asarray(wav)
    if x.ndim != 1:
        raise ValueError("write_wav: a 1-D waveform is needed")
    pcm = np.round(np.clip(x.astype(np.float64), -1.0, 1.0) * 32767.0).astype("<i2")
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(int(sr))
        f.writeframes(pcm.tobytes())
    return path


def vocode(names, mags_dir, out_dir, params=AudioParams(), pad_mode="reflect", device="cuda", batch=32, method="reference", seed=0):
    """gl_vocoder.py's loop: reads <mags_dir>/<name>.mag.npy (what make_mags' caller stores, [T, bins] each), synthesises `batch` utterances at a
    time and writes <out_dir>/<name>.wav.  Returns the paths written.  method='librosa' runs gl_vocoder.py's own algorithm (griffinlim); an
    utterance's random phase is keyed by its index in names, so one list gives the same files at any `batch`."""
    _check_method("vocode", method, seed)
    os.makedirs(out_dir, exist_ok=True)
    names = list(names)
    out = []
    for i in range(0, len(names), batch):
        part = names[i:i + batch]
        mags = [np.load(os.path.join(mags_dir, "%s.mag.npy" % n)).astype(np.float32) for n in part]
        lens = [m.shape[0] for m in mags]
        padded = np.zeros((len(mags), max(lens), params.bins), dtype=np.float32)
        for b, m in enumerate(mags):
            padded[b, :lens[b]] = m
        wavs = spectrogram2wav_batch(torch.from_numpy(padded).to(device), lens, params, True, pad_mode, method, seed, list(range(i, i + len(part))))
        for n, w in zip(part, wavs):
            out.append(write_wav(os.path.join(out_dir, "%s.wav" % n), w, params.sr))
    return out


# ---- feature extraction (src/utils.py:235-278, src/prepare_data.py) ------------------------------------------------------------------
_MEL = {}


def _mel_basis_host(p):
    """librosa.filters.mel(sr, n_fft, n_mels) at its defaults (fmin 0, fmax sr / 2, Slaney scale, Slaney norm), float64 rounded once."""
    key = (p.sr, p.n_fft, p.n_mels)
    if key not in _MEL:
        step, knee, logstep = 200.0 / 3.0, 1000.0, np.log(6.4) / 27.0

        def to_mel(f):
            return f / step if f < knee else knee / step + np.log(f / knee) / logstep
        pts = np.linspace(to_mel(0.0), to_mel(p.sr / 2.0), p.n_mels + 2)
        m = np.where(pts < knee / step, pts * step, knee * np.exp((pts - knee / step) * logstep))          # the filters' edges in Hz
        f = np.arange(p.bins, dtype=np.float64) * p.sr / p.n_fft
        W = np.zeros((p.n_mels, p.bins))
        for i in range(p.n_mels):
            tri = np.minimum((f - m[i]) / (m[i + 1] - m[i]), (m[i + 2] - f) / (m[i + 2] - m[i + 1]))
            W[i] = np.maximum(0.0, tri) * 2.0 / (m[i + 2] - m[i])
        W = W.astype(np.float32)
        ranges = np.zeros((p.n_mels, 2), dtype=np.int32)
        for i in range(p.n_mels):
            nz = np.flatnonzero(W[i])
            if nz.size:                                      # contiguous: a triangle; a filter narrower than a bin's spacing may hold none
                ranges[i] = (nz[0], nz[-1] + 1)
        W.setflags(write=False)
        ranges.setflags(write=False)
        _MEL[key] = (W, ranges)
    return _MEL[key]


def mel_basis(params=AudioParams(), device=None):
    """(W float32 [n_mels, bins], ranges int32 [n_mels, 2]): the mel filterbank and each filter's [lo, hi) of nonzero bins ((0, 0) for an empty
    filter), read-only numpy arrays; with a device, the same two as tensors there (cached per device, like the window and twiddle tables)."""
    p = params
    if p.n_mels < 1:
        raise ValueError("mel_basis: n_mels must be positive (got %r)" % (p.n_mels,))
    if p.n_fft < 2 or p.n_fft % 2 or p.sr <= 0:
        raise ValueError("mel_basis: n_fft must be even and sr positive (got n_fft=%r, sr=%r)" % (p.n_fft, p.sr))
    W, ranges = _mel_basis_host(p)
    if device is None:
        return W, ranges
    key = (p.sr, p.n_fft, p.n_mels, str(device))
    if key not in _MEL:
        _MEL[key] = (torch.from_numpy(W.copy()).to(device), torch.from_numpy(ranges.copy()).to(device))
    return _MEL[key]


def preemphasis(y, lens=None, coef=AudioParams.preemphasis):
    """np.append(y[0], y[1:] - coef * y[:-1]) (src/utils.py:251) in float32, numpy's bits, for y [n] or [B, n]; lens: samples per row (default:
    all); samples behind a row's length are left unwritten (zero here)."""
    _need_cuda("preemphasis", y, "y")
    single = y.dim() == 1
    y2 = (y.unsqueeze(0) if single else y).contiguous()
    lens = [y2.shape[1]] * y2.shape[0] if lens is None else [int(n) for n in lens]
    if len(lens) != y2.shape[0] or any(n < 0 or n > y2.shape[1] for n in lens):
        raise ValueError("preemphasis: one length per row is needed, each within 0..%d" % y2.shape[1])
    out = ops.preemphasis(y2, _i32(lens, y2.device), float(coef), torch.zeros_like(y2))
    return out[0] if single else out


def get_spectrograms_batch(y, lens, params=AudioParams(), trim=True, pad_mode="reflect", starts=None, return_spec=False):
    """src/utils.py:248-276 for a batch: y float32 [B, n_max] on the device, lens samples per row -> (mel [B, T_max, n_mels], mag [B, T_max, bins],
    frames): normalised, frame-major, frames[b] = 1 + n_b // hop with n_b the samples left after trimming; rows at or behind frames[b] are zero.
    trim: librosa.effects.trim at its defaults first (one read-back of the bounds); starts (without trim): utterance b begins at starts[b] of
    its row.  return_spec: the complex64 spectrum of the emphasised signal as a fourth result.  One launch for the whole batch; an utterance's
    result is bit-identical to running it alone."""
    who = "get_spectrograms_batch"
    p = params
    _check_params(who, p)
    if p.n_mels < 1:
        raise ValueError("%s: n_mels must be positive (got %r)" % (who, p.n_mels))
    if pad_mode not in ("reflect", "constant"):
        raise ValueError("%s: pad_mode is 'reflect' (librosa 0.8) or 'constant' (later versions), got %r" % (who, pad_mode))
    if not torch.is_tensor(y) or y.dim() != 2:
        raise ValueError("%s: y must be [B, n_max]" % who)
    B, n_max = y.shape
    lens = [int(n) for n in (lens.tolist() if hasattr(lens, "tolist") else lens)]
    if len(lens) != B or B < 1:
        raise ValueError("%s: %d rows, %d lengths" % (who, B, len(lens)))
    if trim and starts is not None:
        raise ValueError("%s: starts are given without trim (trim finds them)" % who)
    starts = [0] * B if starts is None else [int(v) for v in starts]
    if len(starts) != B or any(s < 0 or n < 1 or s + n > n_max for s, n in zip(starts, lens)):
        raise ValueError("%s: an utterance lies outside its row of %d samples (starts %s, lengths %s)" % (who, n_max, starts, lens))

    def long_enough(counts, when):
        for b, n in enumerate(counts):
            if n <= p.n_fft // 2:
                raise ValueError("%s: utterance %d has %d samples%s, too short: more than n_fft / 2 = %d are needed for the signal to be longer than "
                                 "the reflect padding" % (who, b, n, when, p.n_fft // 2))
    long_enough(lens, "")
    _need_cuda(who, y, "y")
    if y.dtype != _F32:
        raise TypeError("%s: y must be float32 (got %s)" % (who, y.dtype))
    dev = y.device
    with torch.no_grad():
        y = y if y.stride(1) == 1 else y.contiguous()
        if trim:
            bounds = ops.trim_bounds(y, _i32(lens, dev), 60.0, 2048, 512, pad_mode).tolist()
            starts, samples = [s for s, _ in bounds], [e - s for s, e in bounds]
            long_enough(samples, " after trimming")
        else:
            samples = lens
        frames = [1 + n // p.hop for n in samples]
        T_max = max(frames)
        window, tw = _tables(p, dev)
        W, ranges = mel_basis(p, dev)
        mel = torch.zeros(B, T_max, p.n_mels, dtype=_F32, device=dev)
        mag = torch.zeros(B, T_max, p.bins, dtype=_F32, device=dev)
        spec = torch.zeros(B, T_max, p.bins, dtype=torch.complex64, device=dev) if return_spec else None
        ops.features(y, _i32(starts, dev), _i32(samples, dev), T_max, p.n_fft, p.hop, p.win, float(p.preemphasis), window, tw, W, ranges,
                     float(p.ref_db), float(p.max_db), mel, mag, spec)
    return (mel, mag, frames, spec) if return_spec else (mel, mag, frames)


def load_wav(path, sr=AudioParams.sr):
    """librosa.load(path, sr=sr) (src/utils.py:245) for what the reference feeds it, through the standard library's wave: 16-bit PCM read as
    int / 32768, channels averaged, float32 [n].  Resampling is not built: a file at another rate is refused, as is another sample width."""
    with wave.open(path, "rb") as f:
        ch, width, rate, n = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
        raw = f.readframes(n)
    if width != 2:
        raise ValueError("load_wav: %s holds %d-bit samples; only 16-bit PCM is read" % (path, 8 * width))
    if rate != int(sr):
        raise ValueError("load_wav: %s is sampled at %d Hz, not %d: resampling is not built, convert the file first" % (path, rate, int(sr)))
    x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / np.float32(32768.0)
    return x.reshape(-1, ch).mean(axis=1, dtype=np.float32) if ch > 1 else x


def _features_of(wavs, p, pad_mode, device):
    """[(mel [T, n_mels], mag [T, bins])] float32 numpy for a list of 1-D float32 numpy waveforms: one batch."""
    lens = [len(w) for w in wavs]
    padded = np.zeros((len(wavs), max(lens)), dtype=np.float32)
    for b, w in enumerate(wavs):
        padded[b, :lens[b]] = w
    mel, mag, frames = get_spectrograms_batch(torch.from_numpy(padded).to(device), lens, p, True, pad_mode)
    mel, mag = mel.cpu().numpy(), mag.cpu().numpy()
    return [(mel[b, :T].copy(), mag[b, :T].copy()) for b, T in enumerate(frames)]


def get_spectrograms(fpath, params=AudioParams(), pad_mode="reflect", device="cuda"):
    """The reference's signature (src/utils.py:235-278): a wav file -> (mel [T, n_mels], mag [T, 1 + n_fft/2]) float32 numpy, normalised."""
    y = load_wav(fpath, params.sr)
    if not torch.cuda.is_available():
        raise RuntimeError("get_spectrograms: needs a CUDA (ROCm) device: the transforms are HIP kernels and have no CPU path")
    return _features_of([y], params, pad_mode, device)[0]


def prepare_data(names, wav_dir, out_dir=None, params=AudioParams(), pad_mode="reflect", device="cuda", batch=32):
    """src/prepare_data.py's loop, `batch` files per launch: reads <wav_dir>/<name>.wav and writes <name>.pt.npy (mel, what unast_amd.data and
    train_vocoder.py read) and <name>.mag.npy (what train_vocoder.py and vocode read) next to the wavs, or under out_dir.  Returns the
    (mel path, mag path) pairs written."""
    out_dir = wav_dir if out_dir is None else out_dir
    os.makedirs(out_dir, exist_ok=True)
    names = list(names)
    out = []
    for i in range(0, len(names), batch):
        part = names[i:i + batch]
        feats = _features_of([load_wav(os.path.join(wav_dir, "%s.wav" % n), params.sr) for n in part], params, pad_mode, device)
        for n, (mel, mag) in zip(part, feats):
            paths = (os.path.join(out_dir, "%s.pt.npy" % n), os.path.join(out_dir, "%s.mag.npy" % n))
            np.save(paths[0], mel)
            np.save(paths[1], mag)
            out.append(paths)
    return out
