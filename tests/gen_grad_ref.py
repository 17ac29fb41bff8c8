"""Float64 restatement of the decoder (GeneratorNSF / Generator, reference lib/infer_pack/models.py:542-564; ResBlock1, lib/infer_pack/modules.py:295-308) layer
by layer, returning every tensor the device's tape holds under the tape's names, and of its vector-Jacobian product GIVEN a set of activations: the masks of
the leaky ReLUs are read from the activations handed in, so on the device's own taped activations the VJP is the exact linear map the device computes.
No tests in here (tests/test_gen_grad_host.py pins it against float64 autograd through oracle.nets.generator_forward)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import nets

SLOPE = 0.1


def weights(sd, config, f0=True, dtype=torch.float64):
    """The decoder's folded weights in `dtype`: dict name -> tensor."""
    sd = {k: v.to(dtype) for k, v in nets.tensors({k: v for k, v in sd.items() if k.startswith("dec.")}).items()}
    rb_k, up_rates = config[10], config[12]
    w = {"pre.w": sd["dec.conv_pre.weight"], "pre.b": sd["dec.conv_pre.bias"], "cond.w": sd["dec.cond.weight"], "cond.b": sd["dec.cond.bias"],
         "post.w": sd["dec.conv_post.weight"]}
    for i in range(len(up_rates)):
        w[f"up{i}.w"] = nets.weight_norm_fold(sd[f"dec.ups.{i}.weight_v"], sd[f"dec.ups.{i}.weight_g"])
        w[f"up{i}.b"] = sd[f"dec.ups.{i}.bias"]
        if f0:
            w[f"noise{i}.w"], w[f"noise{i}.b"] = sd[f"dec.noise_convs.{i}.weight"], sd[f"dec.noise_convs.{i}.bias"]
        for j in range(len(rb_k)):
            p = f"dec.resblocks.{i * len(rb_k) + j}."
            for m in range(3):
                for c in (1, 2):
                    w[f"rb{i}.{j}.c{c}.{m}.w"] = nets.weight_norm_fold(sd[p + f"convs{c}.{m}.weight_v"], sd[p + f"convs{c}.{m}.weight_g"])
                    w[f"rb{i}.{j}.c{c}.{m}.b"] = sd[p + f"convs{c}.{m}.bias"]
    return w


def noise_geometry(config, i):
    up_rates = config[12]
    if i + 1 < len(up_rates):
        s = int(np.prod(up_rates[i + 1:]))
        return 2 * s, s, s // 2
    return 1, 1, 0


def forward(w, config, z, har, g):
    """z [1,inter,seg], har [1,1,seg*upp] or None (no-f0 family), g [1,gin,1] -> dict name -> [rows, cols] tensor: z, har, pre, up{i}, rb{i}.{j}.y{m} (m = 1, 2),
    rb{i}.{j}.t{m}, out{i}, y_hat."""
    rb_k, rb_d, up_rates, up_k = config[10], config[11], config[12], config[14]
    a = {"z": z[0]}
    if har is not None:
        a["har"] = har[0]
    x = F.conv1d(z, w["pre.w"], w["pre.b"], padding=3) + F.conv1d(g, w["cond.w"], w["cond.b"])
    a["pre"] = x[0]
    for i, (u, k) in enumerate(zip(up_rates, up_k)):
        x = F.conv_transpose1d(F.leaky_relu(x, SLOPE), w[f"up{i}.w"], w[f"up{i}.b"], stride=u, padding=(k - u) // 2)
        if har is not None:
            nk, ns, npad = noise_geometry(config, i)
            x = x + F.conv1d(har, w[f"noise{i}.w"], w[f"noise{i}.b"], stride=ns, padding=npad)
        a[f"up{i}"] = x[0]
        xs = None
        for j in range(3):
            y = x
            for m in range(3):
                d = rb_d[j][m]
                if m > 0:
                    a[f"rb{i}.{j}.y{m}"] = y[0]
                t = F.conv1d(F.leaky_relu(y, SLOPE), w[f"rb{i}.{j}.c1.{m}.w"], w[f"rb{i}.{j}.c1.{m}.b"], padding=(rb_k[j] * d - d) // 2, dilation=d)
                a[f"rb{i}.{j}.t{m}"] = t[0]
                y = F.conv1d(F.leaky_relu(t, SLOPE), w[f"rb{i}.{j}.c2.{m}.w"], w[f"rb{i}.{j}.c2.{m}.b"], padding=(rb_k[j] - 1) // 2) + y
            xs = y if xs is None else xs + y
        x = xs / 3
        a[f"out{i}"] = x[0]
    a["y_hat"] = torch.tanh(F.conv1d(F.leaky_relu(x), w["post.w"], None, padding=3))[0]
    return a


def _mask(a, slope):
    return torch.where(a > 0, torch.ones_like(a), torch.full_like(a, slope))


def vjp(w, config, acts, dy, f0=True):
    """dy [1,1,seg*upp] and the activations `acts` (name -> [rows, cols], any float dtype; converted to dy's) -> dict: dz [inter,seg], dg [gin], dcond [up_init],
    dhar [seg*upp] (f0) and every delta under the tape's names (d.post, d.out{i}, d.rb{i}.{j}.t{m}, d.rb{i}.{j}.y{m}, d.up{i}, d.pre)."""
    rb_k, rb_d, up_rates, up_k = config[10], config[11], config[12], config[14]
    A = {k: v.to(dy.dtype)[None] for k, v in acts.items()}
    nu = len(up_rates)
    out = {}
    d = dy * (1 - A["y_hat"] ** 2)
    out["d.post"] = d[0]
    # conv_post: the data gradient of a Conv1d is the transposed convolution with the same weight; F.leaky_relu's default slope in front of it; the stage mean's 1 / 3
    D3 = F.conv_transpose1d(d, w["post.w"], padding=3) * _mask(A[f"out{nu - 1}"], 0.01) / 3
    dhar_terms = {}
    for i in range(nu - 1, -1, -1):
        out[f"d.out{i}"] = D3[0]
        dup = None
        for j in range(3):
            D = D3
            for m in (2, 1, 0):
                dil, k = rb_d[j][m], rb_k[j]
                dt = F.conv_transpose1d(D, w[f"rb{i}.{j}.c2.{m}.w"], padding=(k - 1) // 2) * _mask(A[f"rb{i}.{j}.t{m}"], SLOPE)
                ym = A[f"rb{i}.{j}.y{m}"] if m > 0 else A[f"up{i}"]
                D = D + F.conv_transpose1d(dt, w[f"rb{i}.{j}.c1.{m}.w"], padding=(k * dil - dil) // 2, dilation=dil) * _mask(ym, SLOPE)
                out[f"d.rb{i}.{j}.t{m}"] = dt[0]
                if m > 0:
                    out[f"d.rb{i}.{j}.y{m}"] = D[0]
            dup = D if dup is None else dup + D
        out[f"d.up{i}"] = dup[0]
        if f0:
            nk, ns, npad = noise_geometry(config, i)
            dhar_terms[i] = F.conv_transpose1d(dup, w[f"noise{i}.w"], stride=ns, padding=npad)
        # ConvTranspose1d(Cin, Cout, k, u, p): its data gradient is the stride-u convolution with the same [Cin][Cout][k] weight read as a Conv1d's [out][in][k]
        u, k = up_rates[i], up_k[i]
        prev = A[f"out{i - 1}"] if i > 0 else A["pre"]
        dprev = F.conv1d(dup, w[f"up{i}.w"], stride=u, padding=(k - u) // 2) * _mask(prev, SLOPE)
        D3 = dprev / 3
    out["d.pre"] = dprev[0]
    out["dz"] = F.conv_transpose1d(dprev, w["pre.w"], padding=3)[0]
    out["dcond"] = dprev[0].sum(dim=1)
    out["dg"] = w["cond.w"][:, :, 0].t() @ out["dcond"]
    if f0:
        dh = dhar_terms[0]
        for i in range(1, nu):
            dh = dh + dhar_terms[i]
        out["dhar"] = dh[0, 0]
    return out
