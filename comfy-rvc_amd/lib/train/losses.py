"""The trainer's losses on device tensors, forward only: the two reconstruction losses (reference lib/train/losses.py:596-611 kl_loss; F.l1_loss as
training_cli.py:570 uses it) and the three GAN losses (:564-593 feature_loss, discriminator_loss, generator_loss).  Each is a fixed-order float64
reduction on the device (rvc_kl_loss per item, rvc_l1_sum; rvc_sqerr_sums / rvc_l1_sums: one segmented reduction over all tensors of a loss) and
returns 0-dim float32 tensors.  No backward pass."""
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


# ------------------------------------------------------------------------------------------------- GAN losses (reference lib/train/losses.py:564-593)
def _segments(tensors):
    ts = [_dev(t) for t in tensors]
    if not ts:
        raise ValueError("no tensors")
    if len(ts) > 64:
        raise ValueError("at most 64 tensors per loss")
    n = (_lib.c_int64 * len(ts))(*[t.numel() for t in ts])
    return ts, (_lib.c_void_p * len(ts))(*[t.data_ptr() for t in ts]), n


def _sqerr_means(tensors, consts):
    """mean (c - x)^2 of every tensor: ONE segmented float64 reduction (rvc_sqerr_sums), float64 [K] on the device."""
    ts, ptrs, n = _segments(tensors)
    c = (_lib.c_float * len(ts))(*consts)
    out = torch.zeros(len(ts), dtype=torch.float64, device=ts[0].device)
    with torch.cuda.device(ts[0].device):
        _lib.check(_lib.lib.rvc_sqerr_sums(_lib.current_stream(), ptrs, n, c, len(ts), _lib.ptr(out)))
    return out / torch.tensor([t.numel() for t in ts], dtype=torch.float64, device=out.device)


def feature_loss(fmap_r, fmap_g):
    """sum over every (real, generated) feature-map pair of mean |r - g| (one segmented reduction, rvc_l1_sums); 0-dim float32."""
    rs, gs = [t for d in fmap_r for t in d], [t for d in fmap_g for t in d]
    if len(rs) != len(gs) or any(r.shape != g.shape for r, g in zip(rs, gs)):
        raise ValueError("feature_loss: the two lists of feature maps differ in structure")
    rs, pr, n = _segments(rs)
    gs, pg, _ = _segments(gs)
    out = torch.zeros(len(rs), dtype=torch.float64, device=rs[0].device)
    with torch.cuda.device(rs[0].device):
        _lib.check(_lib.lib.rvc_l1_sums(_lib.current_stream(), pr, pg, n, len(rs), _lib.ptr(out)))
    means = out / torch.tensor([t.numel() for t in rs], dtype=torch.float64, device=out.device)
    return means.sum().to(torch.float32)


def discriminator_loss(disc_real_outputs, disc_generated_outputs):
    """(sum_i L_i, [L_i]) with L_i = mean (1 - dr_i)^2 + mean dg_i^2; 0-dim float32 tensors."""
    K = len(disc_real_outputs)
    if K != len(disc_generated_outputs):
        raise ValueError("discriminator_loss: lists of different lengths")
    m = _sqerr_means(list(disc_real_outputs) + list(disc_generated_outputs), [1.0] * K + [0.0] * K)
    per = (m[:K] + m[K:]).to(torch.float32)
    return per.sum(), [per[i] for i in range(K)]


def generator_loss(disc_outputs):
    """(sum_i L_i, [L_i]) with L_i = mean (1 - dg_i)^2; 0-dim float32 tensors."""
    per = _sqerr_means(list(disc_outputs), [1.0] * len(disc_outputs)).to(torch.float32)
    return per.sum(), [per[i] for i in range(len(disc_outputs))]
