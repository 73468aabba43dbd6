"""Waveform synthesis on HIP: the reference's spectrogram2wav (src/utils.py:281-328 -- de-normalise, Griffin-Lim with istft / stft, de-preemphasis,
trim) for whole batches, every arithmetic step a kernel of csrc/audio.hip.  DESIGN.md section 5q states the definitions: librosa's stft / istft
at the reference's settings written out (centred frames, reflect padding, a periodic Hann window of `win` samples centred in n_fft, overlap-add
divided by the window's sum of squares, hop * (T - 1) samples for T frames), scipy's lfilter for the de-preemphasis, and librosa.effects.trim
with its one version-dependent choice, the padding mode of the frame RMS, as an argument.

Spectra are frame-major [frames, 1 + n_fft/2], the layout Vocoder.forward produces, so the reference's transposes do not occur.  One
Griffin-Lim iteration is three launches (inverse transforms, overlap-add gather, forward transforms with the phase update in their epilogue);
the utterances of a batch run side by side and each one's result is bit-identical to running it alone.

`librosa.griffinlim` as gl_vocoder.py calls it (random initial phase, momentum) is not this path and is not built."""
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
    win_length = int(sr * 0.05) :10-12, power :14, max_db :17, ref_db :18, n_iter :19)."""
    n_fft: int = 2048
    hop: int = 275
    win: int = 1102
    preemphasis: float = 0.97
    power: float = 1.2
    max_db: float = 100.0
    ref_db: float = 20.0
    n_iter: int = 60
    sr: int = 22050

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


def spectrogram2wav_batch(mags, lens, params=AudioParams(), trim=True, pad_mode="reflect"):
    """src/utils.py:281-306 for a batch: mags float32 [B, T, bins] normalised magnitudes (Vocoder.forward's output as it is), lens frames per
    utterance -> a list of 1-D float32 device tensors, utterance b with at most hop * (lens[b] - 1) samples (fewer after trimming)."""
    p = params
    _check_params("spectrogram2wav_batch", p)
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
    _need_cuda("spectrogram2wav_batch", mags, "mags")
    dev = mags.device
    with torch.no_grad():
        T_max = T                                            # frames behind an utterance's length are skipped by every kernel
        M = torch.empty(B, T_max, p.bins, dtype=_F32, device=dev)
        X = torch.empty(B, T_max, p.bins, dtype=torch.complex64, device=dev)
        ops.gl_prepare(mags, p.max_db, p.ref_db, p.power, M, X)
        frames_dev = _i32(lens, dev)
        y = torch.zeros(B, p.hop * (T_max - 1), dtype=_F32, device=dev)
        _griffin_lim(M, X, frames_dev, p, p.n_iter, y)
        samples = [p.hop * (n - 1) for n in lens]
        samples_dev = _i32(samples, dev)
        ops.deemphasis(y, samples_dev, p.preemphasis, y)
        if trim:
            bounds = ops.trim_bounds(y, samples_dev, 60.0, 2048, 512, pad_mode).tolist()
        else:
            bounds = [(0, n) for n in samples]
        return [y[b, s:e] for b, (s, e) in enumerate(bounds)]


def spectrogram2wav(mag, params=AudioParams(), pad_mode="reflect", device="cuda"):
    """The reference's signature (src/utils.py:281-306): a numpy magnitude [T, 1 + n_fft/2] -> a 1-D float32 numpy waveform."""
    m = torch.as_tensor(np.asarray(mag, dtype=np.float32))
    if m.dim() != 2:
        raise ValueError("spectrogram2wav: mag must be [T, %d]" % params.bins)
    _check_params("spectrogram2wav", params)
    if m.shape[1] != params.bins:
        raise ValueError("spectrogram2wav: the last dimension must be 1 + n_fft/2 = %d (got %d)" % (params.bins, m.shape[1]))
    _check_lens("spectrogram2wav", [m.shape[0]], m.shape[0], params)
    if not torch.cuda.is_available():
        raise RuntimeError("spectrogram2wav: needs a CUDA (ROCm) device: the transforms are HIP kernels and have no CPU path")
    return spectrogram2wav_batch(m.to(device).unsqueeze(0), [m.shape[0]], params, True, pad_mode)[0].cpu().numpy()


def mel2wav(vocoder, mel, mel_lens, params=AudioParams(), trim=True, pad_mode="reflect"):
    """mel [B, T, num_mels] -> waveforms: Vocoder.forward under no_grad (src/inf_vocoder.py:56-64), then spectrogram2wav_batch (gl_vocoder.py's
    loop over the stored magnitudes, with the deterministic Griffin-Lim of src/utils.py)."""
    with torch.no_grad():
        mags = vocoder.forward(mel)
    return spectrogram2wav_batch(mags, mel_lens, params, trim, pad_mode)


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


def vocode(names, mags_dir, out_dir, params=AudioParams(), pad_mode="reflect", device="cuda", batch=32):
    """gl_vocoder.py's loop: reads <mags_dir>/<name>.mag.npy (what make_mags' caller stores, [T, bins] each), synthesises `batch` utterances at a
    time and writes <out_dir>/<name>.wav.  Returns the paths written."""
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
        wavs = spectrogram2wav_batch(torch.from_numpy(padded).to(device), lens, params, True, pad_mode)
        for n, w in zip(part, wavs):
            out.append(write_wav(os.path.join(out_dir, "%s.wav" % n), w, params.sr))
    return out
