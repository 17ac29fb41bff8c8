"""Float64 restatement of the flow's 100 parameter gradients (ResidualCouplingBlock, reference lib/infer_pack/models.py:150-196; WN of modules.py:130-209) GIVEN
the tensors a trainable net's tape holds, for one or more items each at its own length, weight norm included; the flow's forward and vector-Jacobian product of
tests/flow_grad_ref.py restated WITH the four tensors the parameter gradients additionally need (flow{f}.xin, flow{f}.out, d.flow{f}.x1 / x2, d.flow{f}.skip);
and the raw cases of the ragged, gated weight-gradient GEMM (csrc/conv_flow_wgrad.hip, rvc_gated_conv1d_weight_grad) with their float64 references and the hi /
lo emulation of the kernel's product, the gate computed in float32 (tests/gather_gemm_ref.py).
No tests in here (tests/test_flow_wgrad_host.py pins the restatement against float64 autograd through flow_grad_ref.forward)."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import flow_grad_ref as FR
import gather_gemm_ref as G

F64 = torch.float64
N_FLOWS, N_LAYERS, KERNEL = FR.N_FLOWS, FR.N_LAYERS, FR.KERNEL


# ---------------------------------------------------------------------------------------------------------------- names
def prefix(f):
    return f"flow.flows.{2 * f}."


def parameter_names():
    """the reference module's state-dict order: per coupling pre, enc.in_layers.*, enc.res_skip_layers.*, enc.cond_layer (bias, weight_g, weight_v), post"""
    out = []
    for f in range(N_FLOWS):
        p = prefix(f)
        out += [p + "pre.weight", p + "pre.bias"]
        for m in ("in_layers", "res_skip_layers"):
            for i in range(N_LAYERS):
                out += [p + f"enc.{m}.{i}.{s}" for s in ("bias", "weight_g", "weight_v")]
        out += [p + f"enc.cond_layer.{s}" for s in ("bias", "weight_g", "weight_v")]
        out += [p + "post.weight", p + "post.bias"]
    return out


def fold(v, g):
    """weight norm over dim 0: w[m] = g[m] v[m] / |v[m]|"""
    return g.view(-1, 1, 1) * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)


def folded_weights(sd):
    """flow_grad_ref.weights from a dict of torch tensors in any dtype, differentiable: the fold is applied here explicitly"""
    out = []
    for f in range(N_FLOWS):
        p = prefix(f)
        w = {"pre.w": sd[p + "pre.weight"], "pre.b": sd[p + "pre.bias"], "post.w": sd[p + "post.weight"], "post.b": sd[p + "post.bias"],
             "cond.w": fold(sd[p + "enc.cond_layer.weight_v"], sd[p + "enc.cond_layer.weight_g"]), "cond.b": sd[p + "enc.cond_layer.bias"]}
        for i in range(N_LAYERS):
            for n, m in (("in", "in_layers"), ("rs", "res_skip_layers")):
                w[f"{n}{i}.w"] = fold(sd[p + f"enc.{m}.{i}.weight_v"], sd[p + f"enc.{m}.{i}.weight_g"])
                w[f"{n}{i}.b"] = sd[p + f"enc.{m}.{i}.bias"]
        out.append(w)
    return out


def random_state_dict(inter, hidden, gin, seed):
    """a tiny net's flow.* tensors in float64: flow_grad_ref.random_weights as weight_v, a positive weight_g of its own"""
    ws = FR.random_weights(inter, hidden, gin, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    sd = OrderedDict()
    for f, w in enumerate(ws):
        p = prefix(f)
        sd[p + "pre.weight"], sd[p + "pre.bias"] = w["pre.w"], w["pre.b"]
        for n, m in (("in", "in_layers"), ("rs", "res_skip_layers")):
            for i in range(N_LAYERS):
                v = w[f"{n}{i}.w"]
                sd[p + f"enc.{m}.{i}.bias"] = w[f"{n}{i}.b"]
                sd[p + f"enc.{m}.{i}.weight_g"] = (0.5 + torch.rand(v.shape[0], 1, 1, generator=gen, dtype=F64)) * v.flatten(1).norm(dim=1).view(-1, 1, 1)
                sd[p + f"enc.{m}.{i}.weight_v"] = v
        v = w["cond.w"]
        sd[p + "enc.cond_layer.bias"] = w["cond.b"]
        sd[p + "enc.cond_layer.weight_g"] = (0.5 + torch.rand(v.shape[0], 1, 1, generator=gen, dtype=F64)) * v.flatten(1).norm(dim=1).view(-1, 1, 1)
        sd[p + "enc.cond_layer.weight_v"] = v
        sd[p + "post.weight"], sd[p + "post.bias"] = w["post.w"], w["post.b"]
    assert list(sd) == parameter_names()
    return sd


# ---------------------------------------------------------------------------------------------------------------- the flow with the four additional tensors
def forward(ws, z, mask, g):
    """flow_grad_ref.forward, its dict extended by flow{f}.xin [B,inter/2,T] (pre's input) and flow{f}.out [B,H,T] (the summed skip output, post's input)"""
    a = {}
    x = z
    half = z.shape[1] // 2
    for f, w in enumerate(ws):
        H = w["pre.w"].shape[0]
        x0, x1 = x[:, :half], x[:, half:]
        a[f"flow{f}.xin"] = x0
        h0 = F.conv1d(x0, w["pre.w"], w["pre.b"]) * mask
        a[f"flow{f}.h0"] = h0
        gc = F.conv1d(g, w["cond.w"], w["cond.b"])
        h, out = h0, 0
        for i in range(N_LAYERS):
            a[f"flow{f}.x{i}"] = h
            pre = F.conv1d(h, w[f"in{i}.w"], w[f"in{i}.b"], padding=KERNEL // 2) + gc[:, 2 * H * i:2 * H * (i + 1)]
            a[f"flow{f}.a{i}"] = pre
            acts = torch.tanh(pre[:, :H]) * torch.sigmoid(pre[:, H:])
            rs = F.conv1d(acts, w[f"rs{i}.w"], w[f"rs{i}.b"])
            if i < N_LAYERS - 1:
                h = (h + rs[:, :H]) * mask
                out = out + rs[:, H:]
            else:
                out = out + rs
        a[f"flow{f}.out"] = out * mask
        m = F.conv1d(out * mask, w["post.w"], w["post.b"]) * mask
        x = torch.cat([x0, m + x1 * mask], 1)
        x = torch.flip(x, [1])
    return x, a


def vjp(ws, acts, d_zp, mask):
    """flow_grad_ref.vjp, its dict extended by d.flow{f}.skip (post^T d m, the skip cotangent of every layer) and d.flow{f}.x1 / x2 (the masked x-chain cotangent
    at the input of layers 1 and 2: the residual half of res_skip_layers[0]'s and [1]'s output cotangent)"""
    out = {}
    d = d_zp
    half = d.shape[1] // 2
    dg = 0
    for f in range(N_FLOWS - 1, -1, -1):
        w = ws[f]
        H = w["pre.w"].shape[0]
        d = torch.flip(d, [1])
        dx0, dx1 = d[:, :half], d[:, half:]
        dm = dx1 * mask
        out[f"d.flow{f}.m"] = dm
        dh = torch.einsum("oc,bot->bct", w["post.w"][:, :, 0], dm) * mask
        out[f"d.flow{f}.skip"] = dh
        dx = torch.zeros_like(dh)
        dgc = []
        for i in range(N_LAYERS - 1, -1, -1):
            if i < N_LAYERS - 1:
                out[f"d.flow{f}.x{i + 1}"] = dx * mask
            drs = dh if i == N_LAYERS - 1 else torch.cat([dx * mask, dh], 1)
            dacts = torch.einsum("oc,bot->bct", w[f"rs{i}.w"][:, :, 0], drs)
            pre = acts[f"flow{f}.a{i}"]
            t, s = torch.tanh(pre[:, :H]), torch.sigmoid(pre[:, H:])
            da = torch.cat([dacts * s * (1 - t * t), dacts * t * s * (1 - s)], 1)
            out[f"d.flow{f}.a{i}"] = da
            dx = (dx * mask if i < N_LAYERS - 1 else 0) + F.conv1d(da, w[f"in{i}.w"].transpose(0, 1).flip(2), padding=KERNEL // 2)
            dgc.insert(0, da.sum(2))
        dh0 = dx * mask
        out[f"d.flow{f}.h0"] = dh0
        out[f"d.flow{f}.gc"] = torch.cat(dgc, 1)
        dg = dg + torch.einsum("og,bo->bg", w["cond.w"][:, :, 0], out[f"d.flow{f}.gc"])
        d = torch.cat([dx0 + torch.einsum("oc,bot->bct", w["pre.w"][:, :, 0], dh0), dx1 * mask], 1)
    out["dz"], out["dg"], out["d.flow.g"] = d, dg, dg
    return out


WGRAD_ACTIVATIONS = [f"flow{f}.{n}" for f in range(N_FLOWS) for n in ["xin", "out"] + [f"x{i}" for i in range(N_LAYERS)] + [f"a{i}" for i in range(N_LAYERS)]]
WGRAD_DELTAS = [f"d.flow{f}.{n}" for f in range(N_FLOWS) for n in ["m", "h0", "x1", "x2", "skip"] + [f"a{i}" for i in range(N_LAYERS)]]


# ---------------------------------------------------------------------------------------------------------------- the 100 gradients given the tape's tensors
def weight_norm_chain(dw, v, g):
    """(grad_g, grad_v) of w = g v / |v| (dim 0) from dW"""
    n = v.flatten(1).norm(dim=1).view(-1, 1, 1)
    d = (dw * v).flatten(1).sum(1).view(-1, 1, 1)
    return d / n, g.view(-1, 1, 1) / n * (dw - d / (n * n) * v)


def gradients(sd, items, gs):
    """sd: the flow.* tensors (float64, weight_v / weight_g raw); items: one dict per item, name -> float64 [rows][T_item] of WGRAD_ACTIVATIONS and WGRAD_DELTAS;
    gs: one [gin] float64 speaker row per item.  Returns the OrderedDict name -> gradient in parameter_names() order, summed over the items."""
    out = OrderedDict((n, None) for n in parameter_names())
    K = KERNEL
    for f in range(N_FLOWS):
        p = prefix(f)
        H = sd[p + "pre.weight"].shape[0]
        dw = {k: 0 for k in ["pre", "post", "cond"] + [f"in{i}" for i in range(N_LAYERS)] + [f"rs{i}" for i in range(N_LAYERS)]}
        db = dict(dw)
        for t, g in zip(items, gs):
            dh0, dm = t[f"d.flow{f}.h0"], t[f"d.flow{f}.m"]
            dw["pre"] = dw["pre"] + (dh0 @ t[f"flow{f}.xin"].T)[:, :, None]
            db["pre"] = db["pre"] + dh0.sum(1)
            dw["post"] = dw["post"] + (dm @ t[f"flow{f}.out"].T)[:, :, None]
            db["post"] = db["post"] + dm.sum(1)
            dgc = []
            for i in range(N_LAYERS):
                da, x, a = t[f"d.flow{f}.a{i}"], t[f"flow{f}.x{i}"], t[f"flow{f}.a{i}"]
                T = x.shape[1]
                xp = F.pad(x, (K // 2, K // 2))
                dw[f"in{i}"] = dw[f"in{i}"] + torch.stack([da @ xp[:, k:k + T].T for k in range(K)], 2)
                db[f"in{i}"] = db[f"in{i}"] + da.sum(1)
                dgc.append(da.sum(1))
                acts = torch.tanh(a[:H]) * torch.sigmoid(a[H:])
                P = t[f"d.flow{f}.skip"] if i == N_LAYERS - 1 else torch.cat([t[f"d.flow{f}.x{i + 1}"], t[f"d.flow{f}.skip"]], 0)
                dw[f"rs{i}"] = dw[f"rs{i}"] + (P @ acts.T)[:, :, None]
                db[f"rs{i}"] = db[f"rs{i}"] + P.sum(1)
            dgc = torch.cat(dgc)
            dw["cond"] = dw["cond"] + (dgc[:, None] * g.view(1, -1))[:, :, None]
            db["cond"] = db["cond"] + dgc
        out[p + "pre.weight"], out[p + "pre.bias"] = dw["pre"], db["pre"]
        out[p + "post.weight"], out[p + "post.bias"] = dw["post"], db["post"]
        for key, name in [(f"in{i}", f"enc.in_layers.{i}") for i in range(N_LAYERS)] + [(f"rs{i}", f"enc.res_skip_layers.{i}") for i in range(N_LAYERS)] + [("cond", "enc.cond_layer")]:
            gg, gv = weight_norm_chain(dw[key], sd[p + name + ".weight_v"], sd[p + name + ".weight_g"])
            out[p + name + ".bias"], out[p + name + ".weight_g"], out[p + name + ".weight_v"] = db[key], gg, gv
    return out


# ---------------------------------------------------------------------------------------------------------------- conv_flow_wgrad_kernel<WM, AM, GATE>: the raw cases
# out[r][c k + t] = sum_item sum_{n < N[item]} P[item][r][n] act(G[item])[c][n + t - (k - 1) / 2].  bm = 128 for R % 128 == 0, 64 for R % 64 == 0, 32 otherwise (R =
# 16, 48 leave the last 32-row tile half empty; 96 is post's).  C k = 65: a ragged last column tile and tap runs that cross it; 96: a tile and a half (bm 128 / 64);
# 960: in_layers' own.  Lengths: one frame, exactly a stage, one frame past it, three ragged items, two short ones, sixteen of 3 .. 40 frames, and two long ones
# whose 35 stages are cut into 18 splits of 2 - more splits than items, split 10 holding item 0's last stage and item 1's first.
SIXTEEN = [3 + (7 * j) % 38 for j in range(16)]
RAW = G._rows(
    ("R", "C", "k", "lengths", "gate", "adv", "bm"),
    [(16, 13, 5, [1], 0, 0, 32),                   # a single stage in all, one frame: every tap but the centre is out of range
     (48, 96, 1, [128], 1, 0, 32),                 # a single full stage, gated
     (64, 13, 5, [129], 1, 0, 64),
     (64, 96, 1, [127, 130, 5], 0, 0, 64),
     (96, 192, 5, [11, 13], 0, 0, 32),
     (96, 96, 1, [129, 128], 1, 0, 32),
     (128, 13, 5, [127, 130, 5], 1, 0, 128),
     (384, 192, 5, [11, 13], 0, 0, 128),           # in_layers
     (384, 96, 1, SIXTEEN, 1, 0, 128),             # sixteen items
     (16, 13, 5, [2600, 1700], 1, 0, 32),          # 21 + 14 stages in 18 splits of 2
     (64, 13, 5, [43, 129], 0, 1, 64)])            # adv: operands whose lo is hardest to round (gather_gemm_ref.worst_lo)


class Raw:
    name, table = "gated_conv1d_weight_grad", RAW

    @staticmethod
    def label(c):
        n = "x".join(str(v) for v in c["lengths"]) if len(c["lengths"]) <= 3 else f"{len(c['lengths'])}items"
        return "R{R}_C{C}_k{k}_g{gate}_n".format(**c) + n + ("_adv" if c["adv"] else "")

    @staticmethod
    def inputs(c, seed):
        """per item P [R][N] and G [C or 2 C][N] (float32)"""
        g = G._gen(seed)
        f = G.worst_lo if c["adv"] else (lambda t: t)
        rows = c["C"] * (2 if c["gate"] else 1)
        return {"p": [f(torch.randn(c["R"], n, generator=g)) for n in c["lengths"]], "g": [f(torch.randn(rows, n, generator=g)) for n in c["lengths"]]}

    @staticmethod
    def padded(ts):
        n = max(t.shape[1] for t in ts)
        return torch.stack([F.pad(t, (0, n - t.shape[1])) for t in ts])      # zero behind an item's length: what the kernel reads there

    @staticmethod
    def act(c, g):
        C = c["C"]
        return torch.tanh(g[:, :C]) * torch.sigmoid(g[:, C:]) if c["gate"] else g

    @staticmethod
    def operands(c, i):
        """the two fp32 operands the kernel splits: the delta, and the gated input with the gate computed in float32"""
        return Raw.padded(i["p"]), Raw.act(c, Raw.padded(i["g"]))

    @staticmethod
    def gemm(c, d, h):
        w0 = torch.zeros(c["R"], c["C"], c["k"], dtype=F64, requires_grad=True)
        with torch.enable_grad():
            y = F.conv1d(h, w0, None, padding=(c["k"] - 1) // 2)
            return torch.autograd.grad(y, w0, d)[0].detach()

    @staticmethod
    def reference(c, i):
        """float64 autograd of the forward operation conv1d(act(G), W), the gate in float64"""
        return Raw.gemm(c, Raw.padded(i["p"]).double(), Raw.act(c, Raw.padded(i["g"]).double()))


def raw_cases():
    return [(c, 7000 + n) for n, c in enumerate(RAW)]


def calibrate(c, seed):
    """(gate, three-term error, two-term error) of a raw case on its own inputs, on the CPU: the project's 2e-5 where the three-term emulation lies below 1e-5
    and the two-term one above 2e-4; a GATED case whose emulation cannot stay below 1e-5 because of the float32 gate gets twice its emulation error."""
    i = Raw.inputs(c, seed)
    a, b = Raw.operands(c, i)
    want = Raw.reference(c, i)
    gemm = lambda u, v: Raw.gemm(c, u, v)      # noqa: E731
    e3, e2 = G.rel_err(G.emulate(gemm, a, b, 3), want), G.rel_err(G.emulate(gemm, a, b, 2), want)
    gate = G.GATE if (e3 < G.GATE / 2 or not c["gate"]) else 2 * e3
    return gate, e3, e2


INFO = G.INFO


def plan(c, **over):
    """the planner's pure query (no device): the info of include/rvc_hip.h as a dict, or None where the planner declines"""
    import ctypes as C
    from comfy_rvc_amd import _lib
    c = dict(c, **over)
    info = (C.c_int * 8)()
    n = (C.c_int64 * max(1, len(c["lengths"])))(*c["lengths"])
    rc = _lib.lib.rvc_gated_conv1d_weight_grad_plan(c.get("B", len(c["lengths"])), c["R"], c["C"], c["k"], n, c.get("off0", -((c["k"] - 1) // 2)), c["gate"], info)
    if rc < 0:
        return None
    out = dict(zip(INFO, list(info)))
    assert rc == out["splits"]
    return out
