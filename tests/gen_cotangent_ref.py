"""CPU restatement, differentiable through torch autograd, of what the generator-side losses compute from a waveform: the log-mel spectrogram (frames as
aux_loss_ref.frames, the project's float32 mel_filterbank in every precision), the two mel losses of the trainer (F.l1_loss on the log-mels; the
multi-scale loss) and kl_loss.  float64 unless a dtype is given.  Written from the definitions, shared by the host and the GPU tests; what the reference
itself returns is in tests/golden/gen_cotangent_cases.npz."""
import numpy as np
import torch

import aux_loss_ref as R


def log_mel(x, n_fft, n_mels, sr, hop, fmin, fmax, dtype=torch.float64, eps=0.0, clamp=False):
    """x [R, T] tensor (may require grad) -> [R, n_mels, T // hop]: log(max(W sqrt(|rfft(window * frame)|^2 + eps), 1e-5)); clamp: samples limited to +-1.05."""
    from comfy_rvc_amd.lib.train.mel_processing import mel_filterbank
    x = x.to(dtype)
    if clamp:
        x = x.clamp(-1.05, 1.05)
    win = torch.hann_window(n_fft, periodic=True, dtype=torch.float32).to(dtype)
    X = torch.fft.rfft(R.frames(x, n_fft, hop) * win, dim=-1)
    p = X.real ** 2 + X.imag ** 2 + eps
    mag = torch.where(p > 0, p.clamp_min(torch.finfo(dtype).tiny).sqrt(), torch.zeros_like(p)).transpose(1, 2)       # the root's slope at an exact zero is taken as 0
    w = torch.from_numpy(np.array(mel_filterbank(sr, n_fft, n_mels, fmin, fmax))).to(dtype)
    return torch.log(torch.clamp(w @ mag, min=1e-5))


def vjp(x, cot, n_fft, n_mels, sr, hop, fmin, fmax, dtype=torch.float64, eps=0.0, clamp=False):
    """d <cot, log_mel(x)> / dx for x [R, T], cot [R, n_mels, T // hop] (numpy or tensors) -> tensor [R, T] of dtype."""
    x = torch.as_tensor(x).to(dtype).clone().requires_grad_(True)
    mel = log_mel(x, n_fft, n_mels, sr, hop, fmin, fmax, dtype, eps, clamp)
    return torch.autograd.grad((mel * torch.as_tensor(cot).to(dtype)).sum(), x)[0]


def mel_l1(y_mel, y_hat, n_fft, n_mels, sr, hop, fmin, fmax, dtype=torch.float64):
    """F.l1_loss(y_mel, log-mel of y_hat [R, T])"""
    return (torch.as_tensor(y_mel).to(dtype) - log_mel(y_hat, n_fft, n_mels, sr, hop, fmin, fmax, dtype)).abs().mean()


def multiscale(x, y, sr, n_mels=R.DEFAULT_N_MELS, fmin=50.0, fmax=None, loss="l1", log_weight=1.0, mag_weight=0.0, dtype=torch.float64):
    """aux_loss_ref.multiscale as one differentiable tensor: x, y [B, T] tensors -> the mean over the scales."""
    K = len(n_mels)
    windows = [R.window_length(m) for m in n_mels]
    fmin = [fmin] * K if np.isscalar(fmin) else list(fmin)
    fmax = [sr // 2 if fmax is None else fmax] * K if (fmax is None or np.isscalar(fmax)) else list(fmax)
    total = torch.zeros((), dtype=dtype)
    for m, w, lo, hi in zip(sorted(n_mels), windows, fmin, fmax):
        a, b = (log_mel(v, w, m, sr, sr // 100, lo, hi, dtype) for v in (x, y))
        if log_weight > 0:
            total = total + log_weight * R.pointwise(loss, a, b)
        if mag_weight > 0:
            total = total + mag_weight * R.pointwise(loss, a.exp(), b.exp())
    return total / K


def pointwise_slope(kind, d):
    """d loss(d) / dd of aux_loss_ref.pointwise's element: sign (0 at 0) | 2 d | d inside (-1, 1), sign outside"""
    if kind == "l1":
        return torch.sign(d)
    if kind == "l2":
        return 2 * d
    return torch.where(d.abs() < 1, d, torch.sign(d))


def mel_loss_cotangent(kind, a, b, log_weight, mag_weight, scale):
    """scale d(log_weight sum loss(a, b) + mag_weight sum loss(exp a, exp b)) / da in float64 from the given log-mels (any shape)"""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    g = torch.zeros_like(a)
    if log_weight > 0:
        g = g + log_weight * pointwise_slope(kind, a - b)
    if mag_weight > 0:
        g = g + mag_weight * pointwise_slope(kind, a.exp() - b.exp()) * a.exp()
    return scale * g


def kl_loss(z_p, logs_q, m_p, logs_p, z_mask):
    """sum over the mask of logs_p - logs_q - 0.5 + 0.5 (z_p - m_p)^2 exp(-2 logs_p), over the mask's sum"""
    kl = logs_p - logs_q - 0.5 + 0.5 * (z_p - m_p) ** 2 * torch.exp(-2.0 * logs_p)
    return (kl * z_mask).sum() / z_mask.sum()


def kl_grads(z_p, logs_q, m_p, logs_p, z_mask, scale=1.0, dtype=torch.float64):
    """{name: d (scale kl_loss) / d tensor} by autograd, tensors of dtype"""
    names = ("z_p", "logs_q", "m_p", "logs_p")
    ts = [torch.as_tensor(t).to(dtype).clone().requires_grad_(True) for t in (z_p, logs_q, m_p, logs_p)]
    loss = scale * kl_loss(*ts, torch.as_tensor(z_mask).to(dtype))
    return dict(zip(names, torch.autograd.grad(loss, ts)))


def balancer_norm(g):
    """per-item 2-norm, mean over the batch, in float64"""
    g = torch.as_tensor(g).double()
    return float(g.reshape(g.shape[0], -1).square().sum(-1).sqrt().mean())
