"""Restatement of the discriminators' input-gradient pass in plain torch (float64) for the tests: the vector-Jacobian product from cotangents on the taps
to the waveform, with the leaky ReLU's masks taken from GIVEN feature maps (tap > 0 ? 1 : 0.1, torch's slope at exactly 0) - so fed the device's own
feature maps it is the exact linear map the device has to apply.  Nothing from the product; the forward stays in tests/disc_ref.py.  Also the cotangents of
the three GAN losses and the two scalars the trainer forms from an input gradient (gradient_norm_loss, reference lib/train/losses.py:401-426;
LossBalancer.calculate_gradients, :76-92)."""
import numpy as np
import torch
from torch.nn import grad as G

import disc_ref as R


def _t(x):
    return None if x is None else torch.as_tensor(np.asarray(x.detach().cpu()) if torch.is_tensor(x) else np.asarray(x)).to(torch.float64)


def mask(tap):
    """the leaky ReLU's derivative from its OUTPUT, float64: 1 where tap > 0, the slope elsewhere (torch takes the slope at exactly 0)"""
    one = torch.ones((), dtype=torch.float64)
    return torch.where(tap > 0, one, one * R.LRELU_SLOPE)


def _layers(i, period):
    """[(prefix, stride, padding, groups)] of sub-discriminator i, conv_post last"""
    pre = f"discriminators.{i}"
    if period:
        return [(f"{pre}.convs.{l}", s, 2, 1) for l, s in enumerate(R.P_STRIDES)] + [(f"{pre}.conv_post", 1, 1, 1)]
    return [(f"{pre}.convs.{l}", s, p, g) for l, (s, p, g) in enumerate(R.S_LAYERS)] + [(f"{pre}.conv_post", 1, 1, 1)]


def _conv_input(period, shape, w, delta, stride, padding, groups):
    if period:
        return G.conv2d_input(shape, w, delta, stride=(stride, 1), padding=(padding, 0), groups=groups)
    return G.conv1d_input(shape, w, delta, stride=stride, padding=padding, groups=groups)


def input_grad(W, version, fmaps, cotangents, T):
    """W: disc_ref.folded(sd, torch.float64); fmaps[i][l]: tap l of sub-discriminator i, [B,C,H,p] ([B,C,T'] for DiscriminatorS); cotangents[i][l]: its
    cotangent or None.  -> (dsignal [B,1,T], deltas[i][l] = dL / d(pre-activation of layer l)), float64."""
    B = int(fmaps[0][0].shape[0])
    total = torch.zeros(B, 1, T, dtype=torch.float64)
    deltas = []
    for i, period in enumerate((0,) + R.PERIODS[version]):
        taps = [_t(a) for a in fmaps[i]]
        cots = [_t(c) for c in cotangents[i]]
        layers = _layers(i, period)
        nl = len(layers)
        assert len(taps) == nl and len(cots) == nl
        d = [None] * nl
        d[nl - 1] = cots[nl - 1] if cots[nl - 1] is not None else torch.zeros_like(taps[nl - 1])
        for l in range(nl - 1, 0, -1):
            name, stride, padding, groups = layers[l]
            g = _conv_input(period, taps[l - 1].shape, W[name][0], d[l], stride, padding, groups)
            if cots[l - 1] is not None:
                g = g + cots[l - 1]
            d[l - 1] = g * mask(taps[l - 1])
        name, stride, padding, groups = layers[0]
        if period:
            Tp = -(-T // period) * period
            dA = _conv_input(period, (B, 1, Tp // period, period), W[name][0], d[0], stride, padding, groups).reshape(B, 1, Tp)
            dsig = dA[..., :T].clone()
            for q in range(T, Tp):                      # F.pad(..., "reflect") on the right: position q >= T holds sig[2 (T - 1) - q]
                dsig[..., 2 * (T - 1) - q] += dA[..., q]
        else:
            dsig = _conv_input(period, (B, 1, T), W[name][0], d[0], stride, padding, groups)
        total = total + dsig
        deltas.append(d)
    return total, deltas


def none_like(fmaps):
    return [[None] * len(d) for d in fmaps]


def cot_discriminator_generated(scores):
    """d sum_i mean(s_i^2) / d s_i: the generated half of discriminator_loss (the real half has no path to the generated input)"""
    return [2.0 * _t(s) / s.numel() for s in scores]


def cot_generator(scores):
    """d sum_i mean((1 - s_i)^2) / d s_i"""
    return [-2.0 * (1.0 - _t(s)) / s.numel() for s in scores]


def cot_feature(fmap_r, fmap_g):
    """d sum mean|r - g| / d g, sign(0) = 0"""
    return [[torch.sign(_t(g) - _t(r)) / g.numel() for r, g in zip(dr, dg)] for dr, dg in zip(fmap_r, fmap_g)]


def with_scores(fmaps, score_cots, base=None):
    """cotangent lists with the given ones on the last taps (in the tap's shape)"""
    out = none_like(fmaps) if base is None else [list(d) for d in base]
    for i, c in enumerate(score_cots):
        c = c.reshape(fmaps[i][-1].shape)
        out[i][-1] = c if out[i][-1] is None else out[i][-1] + c
    return out


def item_norms(g):
    g = _t(g)
    return g.reshape(g.shape[0], -1).square().sum(-1).sqrt()


def penalty(g):
    """gradient_norm_loss's value from the gradient: mean_b (||g_b||_2 - 1)^2"""
    return float(((item_norms(g) - 1.0) ** 2).mean())


def balancer_norm(g):
    """LossBalancer.calculate_gradients' norm: per-item 2-norm, mean over the batch"""
    return float(item_norms(g).mean())


def interpolate(alpha, y, y_hat):
    """alpha * y + (1 - alpha) * y_hat in float32 with torch's own roundings (what the reference computes)"""
    a, y, y_hat = (torch.as_tensor(np.asarray(v), dtype=torch.float32) for v in (alpha, y, y_hat))
    return (a * y + (1 - a) * y_hat).numpy()
