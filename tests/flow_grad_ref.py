"""Float64 restatement of the flow (ResidualCouplingBlock, reference lib/infer_pack/models.py:150-196; ResidualCouplingLayer, WN and Flip of
lib/infer_pack/modules.py) in the training direction, returning every tensor the device's tape holds under the tape's names, and of its vector-Jacobian product
GIVEN a set of activations: the gate's derivative is read from the pre-gate activations handed in, so on the device's own taped activations the VJP is the exact
linear map the device computes.  mean_only couplings, no dropout, WN with kernel 5, dilation 1 and 3 layers.
No tests in here (tests/test_flow_grad_host.py pins it against float64 autograd through its own forward)."""
import torch
import torch.nn.functional as F

from oracle import nets

N_FLOWS, N_LAYERS, KERNEL = 4, 3, 5


def weights(sd, dtype=torch.float64):
    """The four couplings' folded weights in `dtype`: a list of dicts pre.w/b, post.w/b, in{i}.w/b, rs{i}.w/b, cond.w/b."""
    sd = {k: v.to(dtype) for k, v in nets.tensors({k: v for k, v in sd.items() if k.startswith("flow.")}).items()}
    out = []
    for f in range(N_FLOWS):
        p = f"flow.flows.{2 * f}."
        w = {"pre.w": sd[p + "pre.weight"], "pre.b": sd[p + "pre.bias"], "post.w": sd[p + "post.weight"], "post.b": sd[p + "post.bias"],
             "cond.w": nets.weight_norm_fold(sd[p + "enc.cond_layer.weight_v"], sd[p + "enc.cond_layer.weight_g"]), "cond.b": sd[p + "enc.cond_layer.bias"]}
        for i in range(N_LAYERS):
            for n, m in (("in", "in_layers"), ("rs", "res_skip_layers")):
                w[f"{n}{i}.w"] = nets.weight_norm_fold(sd[p + f"enc.{m}.{i}.weight_v"], sd[p + f"enc.{m}.{i}.weight_g"])
                w[f"{n}{i}.b"] = sd[p + f"enc.{m}.{i}.bias"]
        out.append(w)
    return out


def random_weights(inter, hidden, gin, seed, dtype=torch.float64):
    """Weights of a net of any size (the tiny one of the host test), drawn at a scale that keeps the gates away from saturation."""
    gen = torch.Generator().manual_seed(seed)
    half, H = inter // 2, hidden

    def draw(*shape):
        fan = max(1, int(torch.tensor(shape[1:]).prod())) if len(shape) > 1 else 1
        return (torch.randn(*shape, generator=gen, dtype=torch.float64) / fan ** 0.5).to(dtype)
    out = []
    for _ in range(N_FLOWS):
        w = {"pre.w": draw(H, half, 1), "pre.b": 0.1 * draw(H), "post.w": draw(half, H, 1), "post.b": 0.1 * draw(half),
             "cond.w": draw(2 * H * N_LAYERS, gin, 1), "cond.b": 0.1 * draw(2 * H * N_LAYERS)}
        for i in range(N_LAYERS):
            w[f"in{i}.w"], w[f"in{i}.b"] = draw(2 * H, H, KERNEL), 0.1 * draw(2 * H)
            rows = 2 * H if i < N_LAYERS - 1 else H
            w[f"rs{i}.w"], w[f"rs{i}.b"] = draw(rows, H, 1), 0.1 * draw(rows)
        out.append(w)
    return out


def forward(ws, z, mask, g):
    """z [B,inter,T], mask [B,1,T], g [B,gin,1] -> (z_p [B,inter,T], dict name -> [B,rows,T]: flow{f}.h0, flow{f}.x{i}, flow{f}.a{i})."""
    a = {}
    x = z
    half = z.shape[1] // 2
    for f, w in enumerate(ws):
        H = w["pre.w"].shape[0]
        x0, x1 = x[:, :half], x[:, half:]
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
        m = F.conv1d(out * mask, w["post.w"], w["post.b"]) * mask
        x = torch.cat([x0, m + x1 * mask], 1)
        x = torch.flip(x, [1])
    return x, a


def vjp(ws, acts, d_zp, mask):
    """The cotangent d_zp [B,inter,T] at z_p carried back on the given pre-gate activations acts["flow{f}.a{i}"] [B,2H,T]: dict with dz [B,inter,T], dg [B,gin]
    and the per-layer deltas d.flow{f}.a{i}, d.flow{f}.m, d.flow{f}.h0 ([B,rows,T]), d.flow{f}.gc [B,6H], d.flow.g (= dg)."""
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
        dh = torch.einsum("oc,bot->bct", w["post.w"][:, :, 0], dm) * mask      # the skip cotangent of every layer
        dx = torch.zeros_like(dh)
        dgc = []
        for i in range(N_LAYERS - 1, -1, -1):
            drs = dh if i == N_LAYERS - 1 else torch.cat([dx * mask, dh], 1)
            dacts = torch.einsum("oc,bot->bct", w[f"rs{i}.w"][:, :, 0], drs)
            pre = acts[f"flow{f}.a{i}"]
            t, s = torch.tanh(pre[:, :H]), torch.sigmoid(pre[:, H:])
            da = torch.cat([dacts * s * (1 - t * t), dacts * t * s * (1 - s)], 1)
            out[f"d.flow{f}.a{i}"] = da
            # in_layers[i] transposed: a k = 5 convolution with flipped taps, 2H -> H
            dx = (dx * mask if i < N_LAYERS - 1 else 0) + F.conv1d(da, w[f"in{i}.w"].transpose(0, 1).flip(2), padding=KERNEL // 2)
            dgc.insert(0, da.sum(2))
        dh0 = dx * mask
        out[f"d.flow{f}.h0"] = dh0
        out[f"d.flow{f}.gc"] = torch.cat(dgc, 1)
        dg = dg + torch.einsum("og,bo->bg", w["cond.w"][:, :, 0], out[f"d.flow{f}.gc"])
        d = torch.cat([dx0 + torch.einsum("oc,bot->bct", w["pre.w"][:, :, 0], dh0), dx1 * mask], 1)
    out["dz"], out["dg"], out["d.flow.g"] = d, dg, dg
    return out
