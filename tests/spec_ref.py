"""Shared by the training-input tests: the float64 restatement of the reference's spectrogram_torch, the error metric, and the case tables."""
import numpy as np

GEOMETRIES = ((1024, 320, 32000), (2048, 400, 40000), (2048, 480, 48000))        # (n_fft, hop, model rate) of the training configurations
FRAMES_PER_WG = 16                                                               # kSpecFrames of csrc/spectrogram.hip


def spec_f64(x, n_fft, hop, eps=1e-8, clamp=True):
    """float64 [n_fft / 2 + 1, len(x) // hop]: clamp to the float32 +-1.05, reflect padding of (n_fft - hop) / 2, periodic Hann window, rfft of the frames
    every hop, sqrt(re^2 + im^2 + eps) - lib/train/mel_processing.py:47-87 of the reference evaluated in float64."""
    x = np.asarray(x, dtype=np.float32)
    if clamp:
        x = np.clip(x, np.float32(-1.05), np.float32(1.05))
    x = x.astype(np.float64)
    pad = (n_fft - hop) // 2
    y = np.pad(x, (pad, pad), mode="reflect")
    nf = (y.shape[0] - n_fft) // hop + 1
    assert nf == x.shape[0] // hop
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)
    frames = np.stack([y[f * hop:f * hop + n_fft] for f in range(nf)], axis=0) * win[None, :] if nf else np.zeros((0, n_fft))
    z = np.fft.rfft(frames, axis=1)
    return np.sqrt(z.real ** 2 + z.imag ** 2 + float(eps)).T


def frame_peak_err(got, ref64):
    """max over frames of max_bin |got - ref| / (that frame's peak in ref)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    if ref64.shape[1] == 0:
        return 0.0
    return float((np.abs(got - ref64).max(axis=0) / ref64.max(axis=0)).max())


def torch_spec_f32(x, n_fft, hop, eps=1e-8, clamp=True):
    """The reference's steps with torch on the CPU in float32 (for cases without a golden)."""
    import torch
    y = torch.from_numpy(np.asarray(x, dtype=np.float32))[None]
    if clamp:
        y = y.clamp(min=-1.05, max=1.05)
    pad = (n_fft - hop) // 2
    y = torch.nn.functional.pad(y.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    z = torch.view_as_real(torch.stft(y, n_fft, hop_length=hop, win_length=n_fft, window=torch.hann_window(n_fft), center=False, normalized=False,
                                      onesided=True, return_complex=True))
    return torch.sqrt(z.pow(2).sum(-1) + eps)[0].numpy()


def clip_cases(g):
    """name -> (samples, seed or None for the all-zero clip) of geometry g: the shortest legal clip (the reflect index reaches sample 0 and sample
    N - 1), 3 hops, 7 hops + 123, one frame more than a workgroup's block, all zeros.  `min` and `l7` are the cases of tests/golden/spec_cases.npz."""
    n_fft, hop, _ = GEOMETRIES[g]
    return {"min": ((n_fft - hop) // 2 + 1, 10 + g), "l3": (3 * hop, 30 + g), "l7": (7 * hop + 123, 20 + g),
            "l17": ((FRAMES_PER_WG + 1) * hop + 5, 40 + g), "zero": (4 * hop + 10, None)}


def clip_signal(g, name):
    from comfy_rvc_amd import synthetic as S
    n, seed = clip_cases(g)[name]
    return np.zeros(n, dtype=np.float32) if seed is None else S.spec_test_signal(GEOMETRIES[g][2], n, seed)
