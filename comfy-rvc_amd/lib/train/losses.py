"""The two reconstruction losses of the trainer on device tensors (reference lib/train/losses.py:596-611 kl_loss; F.l1_loss as training_cli.py:570 uses
it): each is one fixed-order float64 reduction on the device (rvc_kl_loss per item, rvc_l1_sum) and returns a 0-dim float32 tensor.  No backward pass."""
import torch

from ... import _lib


def _dev(t):
    if not t.is_cuda:
        raise ValueError("the losses run on the device: pass CUDA tensors (there is no CPU path)")
    return t.detach().to(torch.float32).contiguous()


def kl_loss(z_p, logs_q, m_p, logs_p, z_mask):
    """z_p, logs_q, m_p, logs_p [B, C, T]; z_mask [B, 1, T], a sequence mask (ones up to each item's length): sum over the unmasked elements of
    logs_p - logs_q - 0.5 + 0.5 (z_p - m_p)^2 exp(-2 logs_p), divided by sum(z_mask)."""
    z_p, logs_q, m_p, logs_p = (_dev(t) for t in (z_p, logs_q, m_p, logs_p))
    B, C, T = z_p.shape
    mask = z_mask.detach().reshape(B, -1).to("cpu")
    lengths = mask.sum(dim=1).to(torch.int64)
    if not torch.equal(mask, (torch.arange(mask.shape[1])[None, :] < lengths[:, None]).to(mask.dtype)):
        raise ValueError("z_mask must be a sequence mask (ones up to each length, zeros behind)")
    sums = torch.zeros(B, 2, dtype=torch.float64, device=z_p.device)
    with torch.cuda.device(z_p.device):
        st = _lib.current_stream()
        for b in range(B):
            if int(lengths[b]) > 0:
                _lib.check(_lib.lib.rvc_kl_loss(st, _lib.ptr(z_p[b]), _lib.ptr(logs_q[b]), _lib.ptr(m_p[b]), _lib.ptr(logs_p[b]), C, T, int(lengths[b]),
                                                _lib.ptr(sums[b])))
    tot = sums.sum(dim=0)
    return (tot[0] / tot[1]).to(torch.float32)


def l1_loss(a, b):
    """mean |a - b| over tensors of one shape."""
    a, b = _dev(a), _dev(b)
    if a.shape != b.shape:
        raise ValueError(f"l1_loss: shapes differ: {tuple(a.shape)} and {tuple(b.shape)}")
    out = torch.zeros(1, dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib.rvc_l1_sum(_lib.current_stream(), _lib.ptr(a), _lib.ptr(b), a.numel(), _lib.ptr(out)))
    return (out[0] / a.numel()).to(torch.float32)
