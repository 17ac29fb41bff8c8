"""CPU restatement of the multi-scale mel loss and of the HPSS / TSI auxiliary losses (comfy_rvc_amd.lib.train.losses), in float64 or float32, shared
by the host and the GPU tests.  Written from the definitions (what each quantity IS), not from the reference's text; tests/golden/aux_loss_cases.npz
holds what the reference itself returns.  The filterbank is the project's float32 mel_filterbank in every precision, as on the device."""
import numpy as np
import torch

HPSS_SIZES = (3, 7, 13, 19, 29)
DEFAULT_N_MELS = (20, 64, 80, 128, 160, 256)


def window_length(n_mels):
    """Largest power of two not above 16 n_mels (8 n_mels / (rate / 2) seconds, whatever the rate)."""
    return 1 << ((16 * n_mels).bit_length() - 1)


def frames(x, n_fft, hop):
    """x [R, T] -> [R, T // hop, n_fft]: reflect padding of (n_fft - hop) / 2 on both sides, or for hop > n_fft the middle n_fft samples of every hop."""
    R, T = x.shape
    pad = (n_fft - hop) // 2
    if pad >= 0:
        left = x[:, 1:pad + 1].flip(1)
        right = x[:, T - 1 - pad:T - 1].flip(1)
        x, start = torch.cat([left, x, right], dim=1), 0
    else:
        start = -pad
    nf = T // hop
    idx = start + hop * torch.arange(nf)[:, None] + torch.arange(n_fft)[None, :]
    return x[:, idx]


def stft_mag(x, n_fft, hop, dtype=torch.float64):
    """|rfft(periodic Hann window * frame)| -> [R, n_fft / 2 + 1, T // hop] (no epsilon, no clamp: torch.abs(torch.stft))."""
    x = torch.as_tensor(x).to(dtype)
    win = torch.hann_window(n_fft, periodic=True, dtype=torch.float32).to(dtype)      # a float32 table in every precision, as in the reference and on the device
    return torch.fft.rfft(frames(x, n_fft, hop) * win, dim=-1).abs().transpose(1, 2)


def log_mel(x, n_fft, n_mels, sr, hop, fmin, fmax, dtype=torch.float64):
    from comfy_rvc_amd.lib.train.mel_processing import mel_filterbank
    w = torch.from_numpy(np.array(mel_filterbank(sr, n_fft, n_mels, fmin, fmax))).to(dtype)
    return torch.log(torch.clamp(w @ stft_mag(x, n_fft, hop, dtype), min=1e-5))


def pointwise(kind, a, b):
    d = a - b
    if kind == "l1":
        return d.abs().mean()
    if kind == "l2":
        return (d * d).mean()
    assert kind == "smoothl1"
    return torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5).mean()


def multiscale(x, y, sr, n_mels=DEFAULT_N_MELS, fmin=50.0, fmax=None, loss="l1", log_weight=1.0, mag_weight=0.0, dtype=torch.float64):
    """x, y [B, T] -> (per-scale losses, their mean).  Scale i: n_mels sorted, the window of the i-th n_mels AS GIVEN, band (fmin[i], fmax[i])."""
    K = len(n_mels)
    windows = [window_length(m) for m in n_mels]
    fmin = [fmin] * K if np.isscalar(fmin) else list(fmin)
    fmax = [sr // 2 if fmax is None else fmax] * K if (fmax is None or np.isscalar(fmax)) else list(fmax)
    out = []
    for m, w, lo, hi in zip(sorted(n_mels), windows, fmin, fmax):
        a, b = (log_mel(torch.as_tensor(v), w, m, sr, sr // 100, lo, hi, dtype) for v in (x, y))
        s = torch.zeros((), dtype=dtype)
        if log_weight > 0:
            s = s + log_weight * pointwise(loss, a, b)
        if mag_weight > 0:
            s = s + mag_weight * pointwise(loss, a.exp(), b.exp())
        out.append(float(s))
    return out, float(np.sum(np.array(out, dtype=np.float64 if dtype == torch.float64 else np.float32)) / K)


def median_along(S, k, axis):
    """Median over k neighbours along axis, the edge sample repeated at the boundary (d c b a | a b c d | d c b a); k odd: one of the inputs."""
    S = torch.as_tensor(S)
    h = k // 2
    S = S.movedim(axis, -1)
    ext = torch.cat([S[..., :h].flip(-1), S, S[..., S.shape[-1] - h:].flip(-1)], dim=-1)
    med = ext.unfold(-1, k, 1).sort(dim=-1).values[..., h]
    return med.movedim(-1, axis)


def soft_masks(mh, mp):
    """Power-2 masks of the two medians with margin 1: mh^2 / (mh^2 + mp^2) after dividing both by the larger; 0.5 each where both vanish."""
    z = torch.maximum(mh, mp)
    tiny = torch.finfo(mh.dtype).tiny
    dead = z < tiny
    z = torch.where(dead, torch.ones_like(z), z)
    a, b = (mh / z) ** 2, (mp / z) ** 2
    s = torch.where(dead, torch.ones_like(a), a + b)
    half = torch.full_like(a, 0.5)
    return torch.where(dead, half, a / s), torch.where(dead, half, b / s)


def hpss_parts(mag, dtype=torch.float64):
    """mag [B, F, T] -> (harmonic, percussive) [B, F, 5 T] before scaling (the medians themselves are exact in every precision)."""
    S = torch.as_tensor(mag).to(dtype).abs()
    H, P = [], []
    for k in HPSS_SIZES:
        a, b = soft_masks(median_along(S, k, -1), median_along(S, k, -2))
        H.append(S * a)
        P.append(S * b)
    return torch.cat(H, dim=-1), torch.cat(P, dim=-1)


def minmax(t, eps):
    return ((t - t.min()) / (t.max() - t.min() + eps)).nan_to_num(eps)


def harmonics(mag, eps, dtype=torch.float64):
    h, p = hpss_parts(mag, dtype)
    return minmax(h, eps), minmax(p, eps)


def harmonic_loss(org_mag, gen_mag, eps, dtype=torch.float64):
    (oh, op), (gh, gp) = harmonics(org_mag, eps, dtype), harmonics(gen_mag, eps, dtype)
    return float((gh - oh).abs().mean() + (gp - op).abs().mean())


def envelope(mag, dim, eps, dtype=torch.float64):
    """Unit L2 norm along dim (norm floored at eps), running maximum over t - 1 .. t + 1 along the LAST axis, sum along dim."""
    x = torch.as_tensor(mag).to(dtype)
    x = x / x.pow(2).sum(dim, keepdim=True).sqrt().clamp_min(eps)
    inf = torch.full_like(x[..., :1], -np.inf)
    e = torch.cat([inf, x, inf], dim=-1)
    m = torch.maximum(torch.maximum(e[..., :-2], e[..., 1:-1]), e[..., 2:])
    return m.nan_to_num(eps).sum(dim)


def tsi_term(org_mag, gen_mag, dim, eps, dtype=torch.float64):
    a, b = envelope(org_mag, dim, eps, dtype), envelope(gen_mag, dim, eps, dtype)
    a, b = a - a.mean(-1, keepdim=True), b - b.mean(-1, keepdim=True)
    sa, sb = ((a * a).sum(-1) + eps).sqrt(), ((b * b).sum(-1) + eps).sqrt()
    corr = (a * b).sum(-1) / (sa * sb + eps)
    return float((1 - corr).mean())


def tsi_loss(org_mag, gen_mag, eps, dtype=torch.float64):
    return tsi_term(org_mag, gen_mag, -1, eps, dtype) + tsi_term(org_mag, gen_mag, -2, eps, dtype)


def aux_mags(org, gen, n_mels, sr, n_fft, hop, fmin, fmax, dtype=torch.float64):
    """org, gen [B, T] -> their log-mels [B, n_mels, T // hop]."""
    return log_mel(org, n_fft, n_mels, sr, hop, fmin, fmax, dtype), log_mel(gen, n_fft, n_mels, sr, hop, fmin, fmax, dtype)


def wave_pair(sr, B, T, seed):
    """A seeded (wave, generated wave) pair [B, T] float32: harmonics of a gliding fundamental plus clicks, and a detuned, noisier copy."""
    g = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64) / sr
    out = []
    for det, noise in ((1.0, 0.01), (1.03, 0.05)):
        rows = []
        for b in range(B):
            f0 = (110.0 + 40.0 * b) * det * (1.0 + 0.2 * t * sr / max(T, 1))
            ph = 2 * np.pi * np.cumsum(f0) / sr
            x = sum(np.sin(h * ph + 0.3 * h) / h for h in range(1, 12)) * 0.2
            clicks = np.zeros(T)
            clicks[g.integers(0, T, size=max(T // 2000, 2))] = g.uniform(-0.8, 0.8, size=max(T // 2000, 2))
            rows.append(x + clicks + noise * g.standard_normal(T))
        out.append(np.stack(rows).astype(np.float32))
    return out[0], out[1]
