"""Float64 restatement of the decoder's weight and bias gradients (GeneratorNSF / Generator, reference lib/infer_pack/models.py:460-566; ResBlock1,
lib/infer_pack/modules.py:295-308) GIVEN the activations and deltas of tests/gen_grad_ref.py under the tape's names: every dec.* parameter's gradient, summed
over the items, the chain through weight norm (dim 0) included.  The leaky ReLUs are applied to the activations handed in, so on the device's own tape this is
the exact map the device computes.  No tests in here (tests/test_gen_wgrad_host.py pins it against float64 autograd)."""
from collections import OrderedDict

import torch

from gen_grad_ref import SLOPE, noise_geometry


def lrelu(x, slope=SLOPE):
    return torch.where(x > 0, x, x * slope)


def gather(G, n_out, cstride, off):
    """Y[c][n] = G[c][cstride n + off] for n < n_out, zero where the index leaves [0, G.shape[1])"""
    idx = torch.arange(n_out) * cstride + off
    ok = (idx >= 0) & (idx < G.shape[1])
    Y = torch.zeros(G.shape[0], n_out, dtype=G.dtype)
    Y[:, ok] = G[:, idx[ok]]
    return Y


def correlate(P, G, k, cstride, tstep, off0):
    """out[r][c][t] = sum_n P[r][n] G[c][cstride n + tstep t + off0]: a Conv1d's weight gradient with (1, dilation, -pad), P the delta and G the input; a
    ConvTranspose1d's with (stride, 1, -pad), P the input and G the delta"""
    return torch.stack([P @ gather(G, P.shape[1], cstride, tstep * t + off0).t() for t in range(k)], dim=2)


def weight_norm_chain(dW, v, g):
    """(grad_g, grad_v) from dW = d loss / d(g v / |v|), rows = dim 0"""
    flat_v, flat_w = v.reshape(v.shape[0], -1), dW.reshape(v.shape[0], -1)
    n = flat_v.norm(dim=1)
    d = (flat_w * flat_v).sum(dim=1)
    gg = d / n
    gv = (g.reshape(-1) / n)[:, None] * (flat_w - (d / n ** 2)[:, None] * flat_v)
    return gg.reshape(g.shape), gv.reshape(v.shape)


def weight_grads(sd, config, items, f0=True):
    """sd: the state dict (weight_v / weight_g as stored); items: one dict per item with "acts" and "deltas" (name -> [rows, cols] under the tape's names, d.cond
    [up_init] among the deltas), "g" [gin] and, for the f0 family, "sine" [seg*upp].  Returns an OrderedDict name -> float64 gradient in the state dict's dec.*
    order and shapes."""
    rb_k, rb_d, up_rates, up_k = config[10], config[11], config[12], config[14]
    nu = len(up_rates)
    f64 = lambda t: torch.as_tensor(t).double()
    A = [{k: f64(v) for k, v in it["acts"].items()} for it in items]
    D = [{k: f64(v).reshape(-1) if k in ("d.cond", "d.g", "d.har") else f64(v) for k, v in it["deltas"].items()} for it in items]
    total = lambda f: sum(f(a, d, it) for a, d, it in zip(A, D, items))
    raw = {}

    def dense(prefix, fn, bias):
        """a weight-normed layer: fn(a, d) -> one item's dW, bias(a, d) -> the delta whose row sums are db"""
        v, g = f64(sd[prefix + ".weight_v"]), f64(sd[prefix + ".weight_g"])
        dW = total(lambda a, d, it: fn(a, d))
        raw[prefix + ".bias"] = total(lambda a, d, it: bias(a, d).sum(dim=1))
        raw[prefix + ".weight_g"], raw[prefix + ".weight_v"] = weight_norm_chain(dW, v, g)

    for i in range(nu):
        u, k = up_rates[i], up_k[i]
        prev = f"out{i - 1}" if i > 0 else "pre"
        dense(f"dec.ups.{i}", lambda a, d, i=i, u=u, k=k, prev=prev: correlate(lrelu(a[prev]), d[f"d.up{i}"], k, u, 1, -((k - u) // 2)), lambda a, d, i=i: d[f"d.up{i}"])
        if f0:
            nk, ns, npad = noise_geometry(config, i)
            raw[f"dec.noise_convs.{i}.weight"] = total(lambda a, d, it, i=i: correlate(d[f"d.up{i}"], a["har"], nk, ns, 1, -npad))
            raw[f"dec.noise_convs.{i}.bias"] = total(lambda a, d, it, i=i: d[f"d.up{i}"].sum(dim=1))
        for j in range(3):
            kk = rb_k[j]
            for m in range(3):
                dil = rb_d[j][m]
                p = f"dec.resblocks.{i * 3 + j}."
                y = f"rb{i}.{j}.y{m}" if m > 0 else f"up{i}"
                t = f"rb{i}.{j}.t{m}"
                dy = f"d.rb{i}.{j}.y{m + 1}" if m < 2 else f"d.out{i}"
                dense(p + f"convs1.{m}", lambda a, d, y=y, t=t, kk=kk, dil=dil: correlate(d["d." + t], lrelu(a[y]), kk, 1, dil, -((kk * dil - dil) // 2)),
                      lambda a, d, t=t: d["d." + t])
                dense(p + f"convs2.{m}", lambda a, d, t=t, dy=dy, kk=kk: correlate(d[dy], lrelu(a[t]), kk, 1, 1, -((kk - 1) // 2)), lambda a, d, dy=dy: d[dy])
    raw["dec.conv_pre.weight"] = total(lambda a, d, it: correlate(d["d.pre"], a["z"], 7, 1, 1, -3))
    raw["dec.conv_pre.bias"] = total(lambda a, d, it: d["d.cond"])
    raw["dec.cond.weight"] = total(lambda a, d, it: torch.outer(d["d.cond"], f64(it["g"]).reshape(-1)))[:, :, None]
    raw["dec.cond.bias"] = total(lambda a, d, it: d["d.cond"])
    raw["dec.conv_post.weight"] = total(lambda a, d, it: correlate(d["d.post"], lrelu(a[f"out{nu - 1}"], 0.01), 7, 1, 1, -3))
    if f0:
        e = lambda a, d: d["d.har"] * (1 - a["har"].reshape(-1) ** 2)
        raw["dec.m_source.l_linear.weight"] = total(lambda a, d, it: (e(a, d) * f64(it["sine"]).reshape(-1)).sum()).reshape(1, 1)
        raw["dec.m_source.l_linear.bias"] = total(lambda a, d, it: e(a, d).sum()).reshape(1)
    return OrderedDict((k, raw[k].reshape(tuple(sd[k].shape))) for k in sd if k.startswith("dec."))
