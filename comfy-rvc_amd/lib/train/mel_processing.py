"""Spectrogram and mel functions of the training chain on the device (mirror of the reference's lib/train/mel_processing.py).

`spectrogram_torch`, `spec_to_mel_torch` and `mel_spectrogram_torch` keep the reference's signatures; device tensors go in and come out.  The STFT is
the LDS FFT of csrc/spectrogram.hip (rvc_spectrogram_batch), the projection its banded filterbank kernel (rvc_spec_to_mel_batch); this module is host
plumbing only.  `spectrogram_batch` is the ragged entry the spectrogram cache uses: any number of clips of any lengths, one launch.
`spectrogram_torch` and `mel_spectrogram_torch` send n_fft 1024 / 2048 with hop <= n_fft through rvc_spectrogram_batch and every other geometry (n_fft
256 .. 4096, also hop > n_fft, where the reference's negative padding crops) through rvc_spectrogram_batch_ms.

`mel_spectrogram_vjp` is the backward of `mel_spectrogram_torch` with respect to the waveform (rvc_mel_spectrogram_vjp: the forward FFT redone in LDS, the
filterbank's transpose, the inverse FFT, an overlap-add gather; 2 launches): what torch.autograd.grad sends into y_hat from a cotangent on its log-mel.

Differences from the reference: `center=True` raises (the reference never passes it); n_fft 256 .. 4096 with win_size == n_fft; spectrogram_torch
does not print the reference's out-of-range warnings (they would cost a device round trip; the clamp to +-1.05 itself is applied); `mel_filterbank`
restates librosa.filters.mel and is PARITY-UNPINNED (see its docstring).
"""
import functools

import numpy as np
import torch

from ... import _lib

MAX_WAV_VALUE = 32768.0
FRAME_ALIGN = 16          # a clip's first output column is a multiple of the kernel's frames per workgroup: its 64-byte stores stay aligned


# ----------------------------------------------------------------------------------------------------------------- filterbank (host, float64)
def _hz_to_mel_slaney(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp = 200.0 / 3.0
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz_slaney(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp = 200.0 / 3.0
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_center_frequencies(sr, n_mels, fmin, fmax):
    """The n_mels + 2 band edges / centres in Hz: equally spaced on the Slaney mel scale between fmin and fmax (None: sr / 2)."""
    fmax = float(sr) / 2.0 if fmax is None else float(fmax)
    return _mel_to_hz_slaney(np.linspace(_hz_to_mel_slaney(float(fmin)), _hz_to_mel_slaney(fmax), n_mels + 2))


@functools.lru_cache(None)
def mel_filterbank(sr, n_fft, n_mels, fmin, fmax):
    """float32 [n_mels, n_fft / 2 + 1]: this project's float64 restatement of librosa.filters.mel(sr=, n_fft=, n_mels=, fmin=, fmax=) with its
    defaults - Slaney mel scale (htk=False), triangles between neighbouring centres, Slaney area normalisation 2 / (f[m + 2] - f[m]) - rounded once to
    float32 as librosa does.  PARITY-UNPINNED: librosa is not available where this project is built and tested, so no test compares these numbers with
    librosa's; the tests pin the properties (shape, sign, contiguous support, peak at the centre, banded round trip) and the kernels against THIS matrix.
    (oracle/ref_shim.librosa_mel is the HTK-scale bank of RMVPE and a different function.)"""
    freqs = np.arange(n_fft // 2 + 1, dtype=np.float64) * (float(sr) / n_fft)
    f = mel_center_frequencies(sr, n_mels, fmin, fmax)
    fdiff = np.diff(f)
    ramps = f[:, None] - freqs[None, :]
    w = np.zeros((n_mels, freqs.shape[0]), dtype=np.float64)
    for m in range(n_mels):
        lower = -ramps[m] / fdiff[m]
        upper = ramps[m + 2] / fdiff[m + 1]
        w[m] = np.maximum(0.0, np.minimum(lower, upper))
    w *= (2.0 / (f[2:n_mels + 2] - f[:n_mels]))[:, None]
    w = w.astype(np.float32)
    w.setflags(write=False)
    return w


def band_filterbank(w):
    """Dense [n_mels, n_bins] -> (first int32 [n_mels], count int32 [n_mels], weights float32 [sum count]): per row the span from its first to its last
    non-zero bin (zeros inside a span, which librosa's triangles do not have, would be kept as weights)."""
    w = np.asarray(w, dtype=np.float32)
    first = np.zeros(w.shape[0], dtype=np.int32)
    count = np.zeros(w.shape[0], dtype=np.int32)
    parts = []
    for m in range(w.shape[0]):
        nz = np.flatnonzero(w[m])
        if nz.size:
            first[m], count[m] = nz[0], nz[-1] - nz[0] + 1
            parts.append(w[m, nz[0]:nz[-1] + 1])
    weights = np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)
    return first, count, np.ascontiguousarray(weights, dtype=np.float32)


def unband_filterbank(first, count, weights, n_bins):
    """The dense matrix of a banded filterbank."""
    w = np.zeros((len(first), n_bins), dtype=np.float32)
    o = 0
    for m, (a, c) in enumerate(zip(first, count)):
        w[m, a:a + c] = weights[o:o + c]
        o += c
    return w


# ----------------------------------------------------------------------------------------------------------------- device calls
def _dev_index(t):
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def frames_of(n_samples, hop_size):
    return int(n_samples) // int(hop_size)


def spectrogram_packed(audio, table, n_fft, hop_size, eps, clamp, out):
    """One rvc_spectrogram_batch: audio = 1-D float32 device tensor, table = int64 [n, 3] numpy (sample offset, samples, first column), out = 2-D float32
    device tensor [n_fft / 2 + 1, pitch] whose other columns stay as they are."""
    table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 3)
    assert audio.is_cuda and out.is_cuda and audio.dtype == torch.float32 and out.dtype == torch.float32 and audio.is_contiguous() and out.is_contiguous()
    assert out.dim() == 2 and out.shape[0] == n_fft // 2 + 1
    with torch.cuda.device(audio.device):
        _lib.check(_lib.lib.rvc_spectrogram_batch(_lib.get_ctx(_dev_index(audio)), _lib.current_stream(), _lib.ptr(audio), audio.numel(), _lib.ptr(table),
                                                  table.shape[0], int(n_fft), int(hop_size), float(eps), int(bool(clamp)), _lib.ptr(out), out.shape[1]))
    return out


def spectrogram_packed_ms(audio, table, n_fft, hop_size, eps, clamp, out):
    """spectrogram_packed through rvc_spectrogram_batch_ms: n_fft 256, 512, 1024, 2048 or 4096 and any hop with n_fft - hop even, also hop > n_fft."""
    table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 3)
    assert audio.is_cuda and out.is_cuda and audio.dtype == torch.float32 and out.dtype == torch.float32 and audio.is_contiguous() and out.is_contiguous()
    assert out.dim() == 2 and out.shape[0] == n_fft // 2 + 1
    with torch.cuda.device(audio.device):
        _lib.check(_lib.lib.rvc_spectrogram_batch_ms(_lib.get_ctx(_dev_index(audio)), _lib.current_stream(), _lib.ptr(audio), audio.numel(), _lib.ptr(table),
                                                     table.shape[0], int(n_fft), int(hop_size), float(eps), int(bool(clamp)), _lib.ptr(out), out.shape[1]))
    return out


def _check_geometry(n_fft, win_size, center):
    if center:
        raise NotImplementedError("center=True is not implemented (the reference never passes it)")
    if win_size != n_fft:
        raise NotImplementedError(f"win_size {win_size} != n_fft {n_fft}: the kernel windows whole frames")


def spectrogram_batch(clips, n_fft, hop_size, win_size, center=False, eps=1e-8, clamp=True, device="cuda:0"):
    """Ragged batch: clips = 1-D float32 tensors / arrays of any lengths -> (packed [n_fft / 2 + 1, pitch] device tensor, int64 [n, 2] (first column,
    frames)); clip i's spectrogram - what spectrogram_torch(clip[None]) returns - is packed[:, col:col + frames].  One launch for the whole batch."""
    _check_geometry(n_fft, win_size, center)
    ts = [c if torch.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)) for c in clips]
    ts = [t.reshape(-1).float() for t in ts]
    dev = next((t.device for t in ts if t.is_cuda), torch.device(device))
    pad = (n_fft - hop_size) // 2
    table = np.zeros((len(ts), 3), dtype=np.int64)
    off = col = 0
    for i, t in enumerate(ts):
        if t.numel() <= pad:
            raise ValueError(f"clip {i} has {t.numel()} samples: the reflect padding of ({n_fft} - {hop_size}) / 2 needs more than {pad}")
        table[i] = (off, t.numel(), col)
        off += t.numel()
        col += -(-frames_of(t.numel(), hop_size) // FRAME_ALIGN) * FRAME_ALIGN
    audio = torch.cat([t.to(dev, non_blocking=True) for t in ts]) if len(ts) != 1 else ts[0].to(dev).contiguous()
    out = torch.empty(n_fft // 2 + 1, max(col, 1), device=dev, dtype=torch.float32)
    spectrogram_packed(audio, table, n_fft, hop_size, eps, clamp, out)
    cols = np.stack([table[:, 2], table[:, 1] // hop_size], axis=1) if len(ts) else np.zeros((0, 2), dtype=np.int64)
    return out, cols


def min_samples(n_fft, hop_size):
    """The shortest signal the reference accepts: one more than the reflect padding, or - hop > n_fft, where it crops instead - one hop."""
    return (n_fft - hop_size) // 2 + 1 if hop_size <= n_fft else hop_size


def rows_spectrogram_packed(y, n_fft, hop_size, eps, clamp, align=True):
    """y [R, T] on the device -> (packed [n_fft / 2 + 1, R * nfa], frames nf, columns per row nfa): row r fills columns [r nfa, r nfa + nf).  (1024 | 2048,
    hop <= n_fft) run through rvc_spectrogram_batch, everything else through rvc_spectrogram_batch_ms.  One launch."""
    R, T = y.shape
    if T < min_samples(n_fft, hop_size):
        raise ValueError(f"{T} samples: n_fft {n_fft} at hop {hop_size} needs at least {min_samples(n_fft, hop_size)}")
    nf = frames_of(T, hop_size)
    nfa = -(-nf // FRAME_ALIGN) * FRAME_ALIGN if align else nf
    table = np.array([(r * T, T, r * nfa) for r in range(R)], dtype=np.int64).reshape(-1, 3)
    x = y.detach().float().contiguous().reshape(-1)
    out = torch.empty(n_fft // 2 + 1, max(R * nfa, 1), device=y.device, dtype=torch.float32)
    first = n_fft in (1024, 2048) and hop_size <= n_fft
    (spectrogram_packed if first else spectrogram_packed_ms)(x, table, n_fft, hop_size, eps, clamp, out)
    return out, nf, nfa


def _rows_spectrogram(y, n_fft, hop_size, eps, clamp):
    """y [B, T] on the device -> [B, n_fft / 2 + 1, T // hop] (contiguous)."""
    B = y.shape[0]
    out, nf, nfa = rows_spectrogram_packed(y, n_fft, hop_size, eps, clamp, align=B != 1)
    if B == 1:
        return out[:, :nf].reshape(1, n_fft // 2 + 1, nf)
    return out.view(n_fft // 2 + 1, B, nfa)[:, :, :nf].permute(1, 0, 2).contiguous()


def spectrogram_torch(y, n_fft, hop_size, win_size, center=False):
    """Waveforms y [B, T] (device tensor) -> linear-frequency linear-amplitude spectrogram [B, n_fft / 2 + 1, T // hop_size] in y's dtype:
    clamp to +-1.05, reflect padding of (n_fft - hop_size) / 2, periodic Hann window, sqrt(re^2 + im^2 + 1e-8) (lib/train/mel_processing.py:47-87)."""
    _check_geometry(n_fft, win_size, center)
    if not y.is_cuda:
        raise ValueError("spectrogram_torch runs on the device: pass a CUDA tensor (there is no CPU path)")
    return _rows_spectrogram(y, n_fft, hop_size, 1e-8, True).to(dtype=y.dtype)


_bank_on_device = {}      # (device index, n_fft, n_mels) -> (sr, fmin, fmax) of the bank the context holds


def ensure_bank(dev_index, n_fft, n_mels, sr, fmin, fmax):
    """The context's filterbank of (n_fft, n_mels) is the one of (sr, fmin, fmax): uploaded only when it is not."""
    _ensure_bank(dev_index, n_fft, n_mels, sr, fmin, fmax)


def _ensure_bank(dev_index, n_fft, n_mels, sr, fmin, fmax):
    key, want = (dev_index, n_fft, n_mels), (sr, fmin, fmax)
    if _bank_on_device.get(key) != want:
        first, count, weights = band_filterbank(mel_filterbank(sr, n_fft, n_mels, fmin, fmax))
        _lib.check(_lib.lib.rvc_mel_filterbank_set(_lib.get_ctx(dev_index), int(n_fft), int(n_mels), _lib.ptr(first), _lib.ptr(count), _lib.ptr(weights)))
        _bank_on_device[key] = want


def mel_packed(spec, cols, n_fft, n_mels, sampling_rate, fmin, fmax, out=None):
    """One rvc_spec_to_mel_batch: spec [n_fft / 2 + 1, pitch] float32 device tensor, cols int64 [n, 2] (first column, frames) -> mel [n_mels, pitch]
    (other columns untouched / uninitialised)."""
    cols = np.ascontiguousarray(cols, dtype=np.int64).reshape(-1, 2)
    assert spec.is_cuda and spec.dtype == torch.float32 and spec.is_contiguous() and spec.dim() == 2 and spec.shape[0] == n_fft // 2 + 1
    if out is None:
        out = torch.empty(n_mels, spec.shape[1], device=spec.device, dtype=torch.float32)
    with torch.cuda.device(spec.device):
        _ensure_bank(_dev_index(spec), n_fft, n_mels, sampling_rate, fmin, fmax)
        _lib.check(_lib.lib.rvc_spec_to_mel_batch(_lib.get_ctx(_dev_index(spec)), _lib.current_stream(), _lib.ptr(spec), spec.shape[1], _lib.ptr(cols),
                                                  cols.shape[0], int(n_fft), int(n_mels), _lib.ptr(out), out.shape[1]))
    return out


def _rows_mel(spec3, n_fft, n_mels, sampling_rate, fmin, fmax):
    """spec3 [B, F, T] float32 device -> [B, n_mels, T]."""
    B, F, T = spec3.shape
    flat = spec3[0] if B == 1 else spec3.permute(1, 0, 2).reshape(F, B * T)
    mel = mel_packed(flat.contiguous(), np.array([(0, B * T)], dtype=np.int64), n_fft, n_mels, sampling_rate, fmin, fmax)
    if B == 1:
        return mel.reshape(1, n_mels, T)
    return mel.view(n_mels, B, T).permute(1, 0, 2).contiguous()


def spec_to_mel_torch(spec, n_fft, num_mels, sampling_rate, fmin, fmax):
    """Linear spectrogram [B, n_fft / 2 + 1, T] (or [n_fft / 2 + 1, T]) -> log-mel [B, num_mels, T]: log(clamp(mel_basis @ spec, min=1e-5))
    (lib/train/mel_processing.py:89-96)."""
    if not spec.is_cuda:
        raise ValueError("spec_to_mel_torch runs on the device: pass a CUDA tensor (there is no CPU path)")
    s3 = spec if spec.dim() == 3 else spec[None]
    mel = _rows_mel(s3.detach().float(), n_fft, num_mels, sampling_rate, fmin, fmax).to(dtype=spec.dtype)
    return mel if spec.dim() == 3 else mel[0]


def mel_spectrogram_torch(wav, n_fft, n_mels, sampling_rate, hop_length, window_length, fmin, fmax, center=False):
    """wav [B, C, T] (device tensor) -> log-mel [B * C, n_mels, T // hop_length] of torch.abs(torch.stft(...)) - no clamp, no epsilon under the root
    (lib/train/mel_processing.py:117-150)."""
    _check_geometry(n_fft, window_length, center)
    if not wav.is_cuda:
        raise ValueError("mel_spectrogram_torch runs on the device: pass a CUDA tensor (there is no CPU path)")
    B, Cn, T = wav.shape
    spec = _rows_spectrogram(wav.reshape(-1, T), n_fft, hop_length, 0.0, False)
    return _rows_mel(spec, n_fft, n_mels, sampling_rate, fmin, fmax).to(dtype=wav.dtype)


def mel_vjp_packed(audio, table, cot, n_fft, hop_size, eps, clamp, n_mels, sampling_rate, fmin, fmax, out=None):
    """One rvc_mel_spectrogram_vjp (2 launches): audio = 1-D float32 device tensor, table = int64 [n, 3] numpy (sample offset, samples, first cotangent column),
    cot = [n_mels, pitch] float32 device tensor on the log-mel -> d_audio in audio's shape; every sample of every listed clip is written."""
    table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 3)
    assert audio.is_cuda and cot.is_cuda and audio.dtype == torch.float32 and cot.dtype == torch.float32 and audio.is_contiguous() and cot.is_contiguous()
    assert cot.dim() == 2 and cot.shape[0] == n_mels
    if out is None:
        out = torch.empty_like(audio)
    with torch.cuda.device(audio.device):
        _ensure_bank(_dev_index(audio), n_fft, n_mels, sampling_rate, fmin, fmax)
        _lib.check(_lib.lib.rvc_mel_spectrogram_vjp(_lib.get_ctx(_dev_index(audio)), _lib.current_stream(), _lib.ptr(audio), audio.numel(), _lib.ptr(table),
                                                    table.shape[0], int(n_fft), int(hop_size), float(eps), int(bool(clamp)), int(n_mels), _lib.ptr(cot), cot.shape[1],
                                                    _lib.ptr(out)))
    return out


def rows_mel_vjp(y, cot, nfa, n_fft, hop_size, eps, clamp, n_mels, sampling_rate, fmin, fmax):
    """y [R, T] on the device, cot [n_mels, >= R * nfa] with row r's frames from column r * nfa -> the gradient [R, T]."""
    R, T = y.shape
    if T < min_samples(n_fft, hop_size):
        raise ValueError(f"{T} samples: n_fft {n_fft} at hop {hop_size} needs at least {min_samples(n_fft, hop_size)}")
    table = np.array([(r * T, T, r * nfa) for r in range(R)], dtype=np.int64).reshape(-1, 3)
    x = y.detach().float().contiguous().reshape(-1)
    return mel_vjp_packed(x, table, cot, n_fft, hop_size, eps, clamp, n_mels, sampling_rate, fmin, fmax).view(R, T)


def mel_spectrogram_vjp(wav, cot_mel, n_fft, n_mels, sampling_rate, hop_length, window_length, fmin, fmax, center=False):
    """The vector-Jacobian product of mel_spectrogram_torch: wav [B, C, T] (device tensor), cot_mel [B * C, n_mels, T // hop_length] on its log-mel ->
    d <cot_mel, mel_spectrogram_torch(wav, ...)> / d wav, [B, C, T] in wav's dtype.  2 launches behind one re-layout of the cotangent."""
    _check_geometry(n_fft, window_length, center)
    if not wav.is_cuda or not cot_mel.is_cuda:
        raise ValueError("mel_spectrogram_vjp runs on the device: pass CUDA tensors (there is no CPU path)")
    B, Cn, T = wav.shape
    nf = frames_of(T, hop_length)
    if tuple(cot_mel.shape) != (B * Cn, n_mels, nf):
        raise ValueError(f"mel_spectrogram_vjp: cot_mel must be [{B * Cn}, {n_mels}, {nf}]: got {tuple(cot_mel.shape)}")
    if nf == 0:
        return torch.zeros_like(wav)
    cot = cot_mel.detach().float().permute(1, 0, 2).reshape(n_mels, B * Cn * nf).contiguous()
    g = rows_mel_vjp(wav.reshape(-1, T), cot, nf, n_fft, hop_length, 0.0, False, n_mels, sampling_rate, fmin, fmax)
    return g.view(B, Cn, T).to(dtype=wav.dtype)
