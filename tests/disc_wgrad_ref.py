"""Restatement of the discriminators' weight-gradient pass in plain torch (float64) for the tests: from GIVEN feature maps, deltas (dL / d pre-activation of
every layer, what the input-gradient pass leaves) and the signal,
    dW_l = conv_weight(X_l, delta_l),   db_l = sum of delta_l over items and positions,
with X_0 the signal after DiscriminatorP's reflect pad and [H][p] view and X_l = tap[l - 1] otherwise, then torch's weight_norm(dim=0) backward:
    grad_g[m] = <dW[m], v[m]> / |v[m]|,   grad_v[m] = (g[m] / |v[m]|) (dW[m] - (<dW[m], v[m]> / |v[m]|^2) v[m]).
Given the maps and deltas the pass is linear, so fed the device's own buffers it is the exact map the device has to apply.  Nothing from the product.  Also
the trainer's clip_grad_value_ in closed form (reference lib/infer_pack/commons.py:257-272)."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F
from torch.nn import grad as G

import disc_ref as R
from disc_grad_ref import _layers, _t


def layer_input(period, x, T):
    """the first layer's input: the signal [S,1,T] itself (DiscriminatorS) or reflect-padded on the right to a multiple of the period and viewed [S,1,H,p]"""
    if not period:
        return x
    if T % period:
        x = F.pad(x, (0, period - T % period), "reflect")
    return x.view(x.shape[0], 1, -1, period)


def conv_weight(period, x, shape, delta, stride, padding, groups):
    if period:
        return G.conv2d_weight(x, shape, delta, stride=(stride, 1), padding=(padding, 0), groups=groups)
    return G.conv1d_weight(x, shape, delta, stride=stride, padding=padding, groups=groups)


def weight_norm_backward(dW, v, g):
    """(grad_g, grad_v) of w = g v / |v| (norm over every dimension but the first), float64"""
    rows = v.shape[0]
    n = v.reshape(rows, -1).norm(dim=1)
    d = (dW * v).reshape(rows, -1).sum(dim=1)
    bc = [-1] + [1] * (v.dim() - 1)
    grad_g = (d / n).reshape(g.shape)
    grad_v = (g.reshape(bc) / n.reshape(bc)) * (dW - (d / n ** 2).reshape(bc) * v)
    return grad_g, grad_v


def weight_grad(sd, version, x, fmaps, deltas, only=None):
    """sd: the state dict (numpy or torch; weight_g / weight_v, or plain weight); x [S,1,T]; fmaps[i][l], deltas[i][l] as the device (or disc_grad_ref) gives
    them.  only: the sub-discriminators to compute (None: all).  -> OrderedDict name -> float64 gradient in the parameter's shape, per layer in the state
    dict's order (bias, weight_g, weight_v; or weight, bias)."""
    x = _t(x)
    T = int(x.shape[-1])
    out = OrderedDict()
    for i, period in enumerate((0,) + R.PERIODS[version]):
        if only is not None and i not in only:
            continue
        inp = layer_input(period, x, T)
        for l, (name, stride, padding, groups) in enumerate(_layers(i, period)):
            delta = _t(deltas[i][l])
            plain = name + ".weight" in sd
            v = _t(sd[name + (".weight" if plain else ".weight_v")])
            dW = conv_weight(period, inp, v.shape, delta, stride, padding, groups)
            db = delta.sum(dim=[d for d in range(delta.dim()) if d != 1])
            if plain:
                out[name + ".weight"] = dW
                out[name + ".bias"] = db
            else:
                out[name + ".bias"] = db
                out[name + ".weight_g"], out[name + ".weight_v"] = weight_norm_backward(dW, v, _t(sd[name + ".weight_g"]))
            inp = _t(fmaps[i][l])
    return out


def clip_grad_value(grads, clip_value, norm_type=2, batch_size=1):
    """(total norm, clamped copies) in float64: (sum_k (|g_k|_norm_type / batch_size)^norm_type)^(1 / norm_type), the norm of the UNCLIPPED gradients"""
    gs = [_t(g) for g in grads]
    total = sum(float(g.norm(float(norm_type)) / batch_size) ** float(norm_type) for g in gs) ** (1.0 / float(norm_type))
    return total, [g if clip_value is None else g.clamp(-float(clip_value), float(clip_value)) for g in gs]
