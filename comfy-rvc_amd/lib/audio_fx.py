"""Audio effects of the audio nodes on the device (csrc/audio_fx.hip): the silence gate, click removal, peak normalisation, the track merge and the
segment energy behind AudioBatchValueNode.

The reference computes these on the host (lib/karafan/audio_utils.py::Silent / Normalize, lib/audio.py::AudioProcessor, custom_nodes/audio_nodes.py)
with scipy, librosa and numpy over whole songs.  Here a signal goes to the device once and every step is a fixed number of launches; the functions
take float32 CUDA tensors (kept on the device, so that steps chain without a copy) or numpy arrays (uploaded to `device`) and return CUDA tensors.
The parts that are plain arithmetic over a short list (window levels, the range scan, array_split bounds) are host functions of their own so that
they can be checked against the reference's values without a device.
"""
import ctypes as C

import numpy as np

MERGE_MODES = {"mean": 0, "median": 1, "min": 2, "max": 3}
MAX_KERNEL_SIZE = 31
LAUNCHES = {"gate": 2, "declick_median": 4, "declick_interpolation": 11, "normalize": 3, "merge": 1, "peak_limit": 2, "segment_energy": 1}


def to_device(x, device="cuda:0", dtype=None):
    """numpy array or tensor -> contiguous 1-D CUDA tensor (float32 unless `dtype` says otherwise)."""
    import torch   # noqa: PLC0415
    dtype = torch.float32 if dtype is None else dtype
    if not hasattr(x, "is_cuda"):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x).reshape(-1)))
    if x.dtype != dtype:
        x = x.to(dtype)
    if not x.is_cuda:
        x = x.to(device)
    return x.reshape(-1).contiguous()


# ---------------------------------------------------------------------------------------------- silence gate
def gate_params(sample_rate):
    """(window, min_size, fade) in samples (reference lib/karafan/audio_utils.py:119-121)."""
    return int(0.500 * sample_rate), int(1.000 * sample_rate), int(0.300 * sample_rate)


def window_levels(ss, n, win):
    """ss [n_windows][2] sums of squares (rvc_gate_levels) -> the level of every window in dB: the maximum over the window's frames of
    20 log10(max(1e-5, rms)), rms = sqrt(sum / win) - amplitude_to_db(amin=1e-5, ref=1) of librosa.feature.rms; the top_db clip cannot lower a maximum."""
    ss = np.asarray(ss, dtype=np.float64).reshape(-1, 2)
    nw = ss.shape[0]
    lens = np.minimum(win, n - win * np.arange(nw))
    frames = 1 + (lens + 2 * (win // 2) - win) // win
    rms = np.sqrt(ss / float(win))
    rms[:, 1] = np.where(frames > 1, rms[:, 1], 0.0)
    return 20.0 * np.log10(np.maximum(1e-5, rms.max(axis=1)))


def gate_ranges(levels, n, win, min_size, fade, threshold_db):
    """The reference's loop over the window levels as an int64 array [n_ranges, 3] of (begin, end, kind), kind 0 fade-out, 1 zero, 2 fade-in
    (host; rvc_gate_ranges)."""
    from .. import _lib   # noqa: PLC0415
    levels = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
    ranges = np.zeros((3 * levels.size + 3, 3), dtype=np.int64)
    nr = C.c_int64(0)
    _lib.check(_lib.lib.rvc_gate_ranges(_lib.ptr(levels), levels.size, int(n), int(win), int(min_size), int(fade), float(threshold_db),
                                        _lib.ptr(ranges), ranges.shape[0], C.byref(nr)))
    return ranges[:nr.value].copy()


def gate_levels(x, win):
    """float32 CUDA tensor [n] -> float64 numpy [n_windows][2]: the frame sums of squares of every window (one launch, one small download)."""
    import torch   # noqa: PLC0415
    from .. import _lib   # noqa: PLC0415
    n = x.numel()
    nw = (n + win - 1) // win
    ss = torch.empty(nw, 2, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib.rvc_gate_levels(_lib.current_stream(), _lib.ptr(x), n, int(win), _lib.ptr(ss), nw))
    return ss.cpu().numpy()


def gate_apply(x, ranges, fade):
    """x with the (begin, end, kind) ranges applied -> a new float32 CUDA tensor (one launch)."""
    import torch   # noqa: PLC0415
    from .. import _lib   # noqa: PLC0415
    ranges = np.ascontiguousarray(ranges, dtype=np.int64).reshape(-1, 3)
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        rd = torch.from_numpy(ranges).to(x.device) if ranges.shape[0] else None
        _lib.check(_lib.lib.rvc_gate_apply(_lib.current_stream(), _lib.ptr(x), _lib.ptr(y), x.numel(), _lib.ptr(rd), ranges.shape[0], int(fade)))
    return y


def silence_gate(x, sample_rate, threshold_db=-50, device="cuda:0", return_ranges=False):
    """Silent() of the reference on a mono signal: float32 CUDA tensor [n]."""
    x = to_device(x, device)
    win, min_size, fade = gate_params(sample_rate)
    if win < 1 or fade < 2:
        raise ValueError(f"sample rate {sample_rate} is too low for the silence gate")
    levels = window_levels(gate_levels(x, win), x.numel(), win)
    ranges = gate_ranges(levels, x.numel(), win, min_size, fade, threshold_db)
    y = gate_apply(x, ranges, fade)
    return (y, ranges, levels) if return_ranges else y


# ---------------------------------------------------------------------------------------------- click removal
def declick(x, multiplier=2., sample_size=16000, method="median", kernel_size=5, device="cuda:0", return_mask=False, clicks=None):
    """AudioProcessor.dynamic_thresholding on the device -> float32 CUDA tensor [n] (and the uint8 click mask).  `clicks`: a caller's mask [n]
    (replace_clicks) - detection is skipped, sample_size and multiplier are not used."""
    import torch   # noqa: PLC0415
    from .. import _lib   # noqa: PLC0415
    if method not in ("median", "interpolation"):
        raise ValueError("Method must be 'median' or 'interpolation'")
    x = to_device(x, device)
    n, size, kernel_size = x.numel(), (int(sample_size) if clicks is None else 1), int(kernel_size)
    if size < 1 or n < size or n < kernel_size:
        raise ValueError(f"the signal ({n} samples) must be at least as long as sample_size ({size}) and kernel_size ({kernel_size})")
    y = torch.empty_like(x)
    if clicks is None:
        mask = torch.empty(n, dtype=torch.uint8, device=x.device)
    else:
        mask = to_device(np.asarray(clicks.cpu() if hasattr(clicks, "is_cuda") else clicks).astype(bool).astype(np.uint8), x.device, dtype=torch.uint8)
        if mask.numel() != n:
            raise ValueError("the click mask must have one entry per sample")
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib.rvc_declick(_lib.current_stream(), _lib.ptr(x), n, size, float(multiplier), int(method == "interpolation"), kernel_size,
                                        int(clicks is None), _lib.ptr(y), _lib.ptr(mask)))
    return (y, mask) if return_mask else y


# ---------------------------------------------------------------------------------------------- normalise, limit
def peak_normalize(x, threshold_db=-1.0, device="cuda:0"):
    """Normalize() of the reference: DC removed, peak at 10^(threshold_db / 20) -> float32 CUDA tensor."""
    import torch   # noqa: PLC0415
    from .. import _lib   # noqa: PLC0415
    x = to_device(x, device)
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib.rvc_peak_normalize(_lib.current_stream(), _lib.ptr(x), x.numel(), float(np.float32(10 ** (threshold_db / 20))), _lib.ptr(y)))
    return y


def peak_limit_(x, max_volume=.95):
    """remix_audio's limiter, in place on a float32 CUDA tensor."""
    import torch   # noqa: PLC0415
    from .. import _lib   # noqa: PLC0415
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib.rvc_peak_limit(_lib.current_stream(), _lib.ptr(x), x.numel(), float(max_volume)))
    return x


# ---------------------------------------------------------------------------------------------- merge
def merge_tracks(tracks, merge_type="median", device="cuda:0"):
    """Two to four mono tracks of any lengths -> float32 CUDA tensor [longest]: pad_audio + get_merge_func(merge_type)(..., axis=0) in one launch
    (an unknown merge_type means the mean, as get_merge_func has it)."""
    import torch   # noqa: PLC0415
    from .. import _lib   # noqa: PLC0415
    tracks = [to_device(t, device) for t in tracks if t is not None]
    if not 2 <= len(tracks) <= 4:
        raise ValueError(f"merge_tracks takes two to four tracks, got {len(tracks)}")
    n_out = max(t.numel() for t in tracks)
    if n_out == 0:
        raise ValueError("merge_tracks: every track is empty")
    dev = tracks[0].device
    out = torch.empty(n_out, dtype=torch.float32, device=dev)
    ptrs = (C.c_void_p * len(tracks))(*[t.data_ptr() if t.numel() else None for t in tracks])
    lens = (C.c_int64 * len(tracks))(*[t.numel() for t in tracks])
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.rvc_merge_tracks(_lib.current_stream(), ptrs, lens, len(tracks), MERGE_MODES.get(merge_type, 0), _lib.ptr(out), n_out))
    return out


# ---------------------------------------------------------------------------------------------- segment energy
def split_bounds(n, k):
    """[k + 1] boundaries of np.array_split(range(n), k): the first n % k segments hold n // k + 1 samples."""
    q, r = divmod(int(n), int(k))
    return np.concatenate([[0], np.cumsum([q + 1] * r + [q] * (k - r))]).astype(np.int64)


def segment_energy(x_i16, num_segments, device="cuda:0"):
    """int16 samples -> int64 numpy [num_segments]: the exact sum of squares of every np.array_split segment (one launch)."""
    import torch   # noqa: PLC0415
    from .. import _lib   # noqa: PLC0415
    x = to_device(x_i16, device, dtype=torch.int16)
    k = int(num_segments)
    if k < 1 or x.numel() < k:
        raise ValueError(f"{x.numel()} samples cannot be split into {k} non-empty segments")
    out = torch.empty(k, dtype=torch.int64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib.rvc_segment_energy(_lib.current_stream(), _lib.ptr(x), x.numel(), k, _lib.ptr(out)))
    return out.cpu().numpy()
