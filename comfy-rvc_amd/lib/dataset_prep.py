"""Training-set slicing on the device (mirror of reference lib/slicer2.py::Slicer plus the window arithmetic of preprocessing_utils.py:52-71).

The reference filters, scans and cuts a recording on the CPU and resamples every window on its own.  Here the recording goes to the device once:
rvc_lfilter_hp (the slicer's forward 48 Hz high-pass), rvc_frame_rms (its framed RMS), rvc_slice_tags (the silence scan, host C++ over the RMS
list) and rvc_cut_windows (every window as float32 and as its peak-limited 16 kHz version) - a fixed number of launches per recording.  The parts
that are plain integer arithmetic (slicer parameters, chunk bounds, window plan) are host functions of their own so that they can be checked
against the reference's values without a device.
"""
import ctypes as C
import functools
import math

import numpy as np


def slicer_params(sr, threshold=-50., min_length=1500, min_interval=400, hop_size=15, max_sil_kept=500):
    """Slicer.__init__'s derived values (reference lib/slicer2.py:48-62; the defaults are the ones Preprocess passes): the linear threshold, hop and
    window in samples, min_length / min_interval / max_sil_kept in frames."""
    if not min_length >= min_interval >= hop_size:
        raise ValueError("The following condition must be satisfied: min_length >= min_interval >= hop_size")
    if not max_sil_kept >= hop_size:
        raise ValueError("The following condition must be satisfied: max_sil_kept >= hop_size")
    interval = sr * min_interval / 1000
    hop = round(sr * hop_size / 1000)
    return dict(threshold=10 ** (threshold / 20.0), hop_size=hop, win_size=min(round(interval), 4 * hop),
                min_length=round(sr * min_length / 1000 / hop), min_interval=round(interval / hop),
                max_sil_kept=round(sr * max_sil_kept / 1000 / hop))


@functools.lru_cache(maxsize=8)
def highpass_sos(sr):
    """butter(5, 48, "high", fs=sr) as three second-order sections [3, 6] (a0 = 1): the form rvc_lfilter_hp evaluates."""
    from scipy import signal   # noqa: PLC0415
    sos = np.ascontiguousarray(signal.butter(N=5, Wn=48, btype="high", fs=sr, output="sos"), dtype=np.float64)
    assert sos.shape == (3, 6) and np.all(sos[:, 3] == 1.0)
    return sos


def n_frames(n, win, hop):
    return (n + 2 * (win // 2) - win) // hop + 1


def lfilter_hp(x, sr):
    """x: float32 / float64 CUDA tensor [n] -> float64 CUDA tensor [n] = scipy.signal.lfilter(bh, ah, x) of the slicer's high-pass."""
    import torch   # noqa: PLC0415
    from .. import _lib   # noqa: PLC0415
    assert x.is_cuda and x.dim() == 1 and x.is_contiguous() and x.dtype in (torch.float32, torch.float64) and x.numel() > 0
    y = torch.empty(x.numel(), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib.rvc_lfilter_hp(_lib.current_stream(), _lib.ptr(x), int(x.dtype == torch.float64), x.numel(), _lib.ptr(highpass_sos(int(sr))),
                                           _lib.ptr(y)))
    return y


def frame_rms(y, win, hop):
    """float64 CUDA tensor [n] -> float64 CUDA tensor [n_frames]: get_rms(y, frame_length=win, hop_length=hop) of the reference."""
    import torch   # noqa: PLC0415
    from .. import _lib   # noqa: PLC0415
    assert y.is_cuda and y.dim() == 1 and y.is_contiguous() and y.dtype == torch.float64
    nf = n_frames(y.numel(), win, hop)
    rms = torch.empty(max(nf, 0), dtype=torch.float64, device=y.device)
    if nf > 0:
        with torch.cuda.device(y.device):
            _lib.check(_lib.lib.rvc_frame_rms(_lib.current_stream(), _lib.ptr(y), y.numel(), int(win), int(hop), _lib.ptr(rms), nf))
    return rms


def slice_tags(rms, n_samples, params):
    """The silences Slicer.slice drops, as an int64 array [n_tags, 2] of (begin, end) frames (host; rvc_slice_tags)."""
    from .. import _lib   # noqa: PLC0415
    rms = np.ascontiguousarray(rms, dtype=np.float64).reshape(-1)
    tags = np.zeros((rms.size + 1, 2), dtype=np.int64)
    nt = C.c_int64(0)
    _lib.check(_lib.lib.rvc_slice_tags(_lib.ptr(rms), rms.size, int(n_samples), float(params["threshold"]), int(params["min_length"]),
                                       int(params["min_interval"]), int(params["max_sil_kept"]), _lib.ptr(tags), tags.shape[0], C.byref(nt)))
    return tags[:nt.value].copy()


def chunk_bounds(tags, total_frames, hop, n):
    """(begin, end) in samples of the clips between the dropped silences (reference lib/slicer2.py:168-183); no tags: the whole recording."""
    tags = [(int(b), int(e)) for b, e in tags]
    if not tags:
        return [(0, n)]
    spans = []
    if tags[0][0] > 0:
        spans.append((0, tags[0][0]))
    spans += [(tags[i][1], tags[i + 1][0]) for i in range(len(tags) - 1)]
    if tags[-1][1] < total_frames:
        spans.append((tags[-1][1], total_frames))
    out = []
    for b, e in spans:                       # numpy slicing of [b * hop : min(n, e * hop)]: an inverted span is empty
        b, e = min(b * hop, n), min(n, e * hop)
        out.append((b, max(b, e)))
    return out


def plan_windows(chunks, sr, period=3.0, overlap=.3):
    """[(start, length, idx1, written)] in the order Preprocess.pipeline reaches norm_write (reference preprocessing_utils.py:45-71): windows of
    `period` s every period - overlap s while more than period + overlap s remain, then the remainder; a window is written only if longer than
    2 * overlap s.  idx1 is incremented BEFORE the remainder is written and not after, so the first window of the next chunk reuses (overwrites)
    the remainder's number - the reference's numbering, kept because trained-model tooling lists these names."""
    tail = period + overlap
    plan, idx1 = [], 0
    for cb, ce in chunks:
        clen, i = ce - cb, 0
        while True:
            start = int(sr * (period - overlap) * i)
            i += 1
            rem = max(0, clen - start)
            if rem > tail * sr:
                length = min(int(period * sr), rem)
                plan.append((cb + start, length, idx1, int(length > overlap * sr * 2)))
                idx1 += 1
            else:
                idx1 += 1
                plan.append((cb + min(start, clen), rem, idx1, int(rem > overlap * sr * 2)))
                break
    return plan


def cut_windows(filt, windows, sr, max_volume=.95, target_sr=16000):
    """filt: float64 CUDA tensor [n]; windows: [(start, length), ...] -> (gt, y16): lists of float32 numpy arrays, one per window - the window
    itself and its peak-limited target_sr version (what remix_audio((window, sr), target_sr=target_sr, max_volume=max_volume) returns)."""
    import torch   # noqa: PLC0415
    from .. import _lib   # noqa: PLC0415
    from .audio import design_resample_filter   # noqa: PLC0415
    if int(sr) == int(target_sr):
        raise ValueError("cut_windows resamples: the recording must not already be at the target rate")
    win = np.ascontiguousarray(np.asarray(windows, dtype=np.int64).reshape(-1, 2))
    if win.shape[0] == 0:
        return [], []
    n = filt.numel()
    assert filt.is_cuda and filt.dtype == torch.float64 and filt.is_contiguous()
    assert (win[:, 1] >= 0).all() and (win[:, 0] >= 0).all() and (win[:, 0] + win[:, 1] <= n).all(), "window outside the recording"
    len16 = np.array([int(math.ceil(int(l) * float(target_sr) / float(sr))) for l in win[:, 1]], dtype=np.int64)
    off_gt, off_16 = np.concatenate([[0], np.cumsum(win[:, 1])]), np.concatenate([[0], np.cumsum(len16)])
    taps, half, up, down = design_resample_filter(int(sr), int(target_sr))
    dev = filt.device
    with torch.cuda.device(dev):
        h = torch.from_numpy(taps).to(dev)
        wd = torch.from_numpy(win).to(dev)
        gt = torch.empty(int(off_gt[-1]), dtype=torch.float32, device=dev)
        y16 = torch.empty(int(off_16[-1]), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib.rvc_cut_windows(_lib.current_stream(), _lib.ptr(filt), n, _lib.ptr(wd), win.shape[0], int(sr), int(target_sr), _lib.ptr(h),
                                            half, up, down, float(max_volume), _lib.ptr(gt), gt.numel(), _lib.ptr(y16), y16.numel()))
        gt, y16 = gt.cpu().numpy(), y16.cpu().numpy()
    return ([gt[off_gt[i]:off_gt[i + 1]] for i in range(win.shape[0])], [y16[off_16[i]:off_16[i + 1]] for i in range(win.shape[0])])
