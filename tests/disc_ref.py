"""Restatement of the trainer's discriminators and GAN losses in plain torch (float64 by default) for the tests: functional conv1d / conv2d on weights with the
weight norm folded, nothing from the product.  Reference lib/infer_pack/models.py:1024-1145 and lib/train/losses.py:564-593;
tools/gen_golden_discriminator.py compares it with the real reference over the full tensors of both golden cases and stores the measured error."""
import numpy as np
import torch
import torch.nn.functional as F

PERIODS = {"v1": (2, 3, 5, 7, 11, 17), "v2": (2, 3, 5, 7, 11, 17, 23, 37)}
LRELU_SLOPE = 0.1
S_LAYERS = [(1, 7, 1), (4, 20, 4), (4, 20, 16), (4, 20, 64), (4, 20, 256), (1, 2, 1)]     # (stride, padding, groups) of DiscriminatorS.convs
P_STRIDES = [3, 3, 3, 3, 1]


def fold_weight_norm(v, g):
    """weight_norm(dim=0): w = v g / ||v||, the norm over every dimension but the first."""
    v = torch.as_tensor(np.asarray(v), dtype=torch.float64)
    g = torch.as_tensor(np.asarray(g), dtype=torch.float64)
    norm = v.reshape(v.shape[0], -1).norm(dim=1).reshape([-1] + [1] * (v.dim() - 1))
    return v * (g.reshape(norm.shape) / norm)


def folded(sd, dtype=torch.float64):
    """state dict (weight_g / weight_v or plain weight) -> {layer prefix: (weight, bias)} in `dtype`."""
    out = {}
    for name in sd:
        if name.endswith(".bias"):
            pre = name[:-5]
            w = fold_weight_norm(sd[pre + ".weight_v"], sd[pre + ".weight_g"]) if pre + ".weight_v" in sd else torch.as_tensor(np.asarray(sd[pre + ".weight"]), dtype=torch.float64)
            out[pre] = (w.to(dtype), torch.as_tensor(np.asarray(sd[name])).to(dtype))
    return out


def disc_s(W, i, x):
    fmap = []
    for l, (stride, pad, groups) in enumerate(S_LAYERS):
        w, b = W[f"discriminators.{i}.convs.{l}"]
        x = F.leaky_relu(F.conv1d(x, w, b, stride=stride, padding=pad, groups=groups), LRELU_SLOPE)
        fmap.append(x)
    w, b = W[f"discriminators.{i}.conv_post"]
    x = F.conv1d(x, w, b, padding=1)
    fmap.append(x)
    return torch.flatten(x, 1, -1), fmap


def disc_p(W, i, period, x):
    fmap = []
    b_, c, t = x.shape
    if t % period != 0:
        n_pad = period - (t % period)
        x = F.pad(x, (0, n_pad), "reflect")
        t = t + n_pad
    x = x.view(b_, c, t // period, period)
    for l, stride in enumerate(P_STRIDES):
        w, b = W[f"discriminators.{i}.convs.{l}"]
        x = F.leaky_relu(F.conv2d(x, w, b, stride=(stride, 1), padding=(2, 0)), LRELU_SLOPE)
        fmap.append(x)
    w, b = W[f"discriminators.{i}.conv_post"]
    x = F.conv2d(x, w, b, padding=(1, 0))
    fmap.append(x)
    return torch.flatten(x, 1, -1), fmap


def forward(sd, version, y, y_hat, dtype=torch.float64, W=None):
    """(y_d_rs, y_d_gs, fmap_rs, fmap_gs) like MultiPeriodDiscriminator[V2].forward; y, y_hat [B,1,T] (numpy or torch); W: folded(sd, dtype) made beforehand."""
    W = folded(sd, dtype) if W is None else W
    y = torch.as_tensor(np.asarray(y)).to(dtype)
    y_hat = torch.as_tensor(np.asarray(y_hat)).to(dtype)
    res = ([], [], [], [])
    with torch.no_grad():
        for i, period in enumerate((0,) + PERIODS[version]):
            for k, x in enumerate((y, y_hat)):
                score, fmap = disc_p(W, i, period, x) if period else disc_s(W, i, x)
                res[k].append(score)
                res[2 + k].append(fmap)
    return res


def feature_loss(fmap_r, fmap_g):
    loss = 0
    for dr, dg in zip(fmap_r, fmap_g):
        for rl, gl in zip(dr, dg):
            loss = loss + torch.mean(torch.abs(rl - gl))
    return loss


def discriminator_loss(disc_real_outputs, disc_generated_outputs):
    losses = [torch.mean((1 - dr) ** 2) + torch.mean(dg ** 2) for dr, dg in zip(disc_real_outputs, disc_generated_outputs)]
    return sum(losses), losses


def generator_loss(disc_outputs):
    losses = [torch.mean((1 - dg) ** 2) for dg in disc_outputs]
    return sum(losses), losses


def losses(res):
    """{"loss_disc", "loss_gen", "loss_fm"} (floats) of a forward result."""
    y_d_rs, y_d_gs, fmap_rs, fmap_gs = res
    return {"loss_disc": float(discriminator_loss(y_d_rs, y_d_gs)[0]), "loss_gen": float(generator_loss(y_d_gs)[0]), "loss_fm": float(feature_loss(fmap_rs, fmap_gs))}


def sample_positions(numel, seed, name, count=256):
    """The seeded flat positions at which a golden keeps a feature map (all of them when it is smaller)."""
    import hashlib
    h = hashlib.sha256(f"{seed}:{name}".encode()).digest()
    rng = np.random.Generator(np.random.PCG64(int.from_bytes(h[:16], "little")))
    return np.sort(rng.choice(numel, size=min(count, numel), replace=False)).astype(np.int64)
