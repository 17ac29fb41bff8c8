"""CPU: the restatement of the discriminators' weight-gradient pass (tests/disc_wgrad_ref.py) against torch float64 autograd through the weight-normed conv
stacks of tests/disc_ref.py, clip_grad_value_ on host tensors against the closed form and against the reference's numbers
(tools/gen_golden_disc_wgrad.py).  The GPU tests (test_hip_disc_wgrad.py) compare the device with this restatement fed the device's own buffers."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden
from comfy_rvc_amd import synthetic as S
import disc_ref as R
import disc_grad_ref as GR
import disc_wgrad_ref as WR
from test_disc_grad_host import forward_with_grad, random_cotangents

# T = 47: every period pads (2: 47 -> 48, H = 24 and H' = 8, 3, 1 ...; 3: H = 16, not a multiple of 3 either); T = 210: case A of the goldens
CASES = [("v1", 47, 2, 5), ("v2", 210, 1, 11)]


def wgrad_case():
    g = golden("disc_wgrad_B_v2.npz")
    y, y_hat = S.disc_waves(int(g["B"]), int(g["T"]), int(g["wave_seed"]))
    return g, y, y_hat


def normed_weights(sd):
    """(leaf parameters {name: float64 tensor requiring grad}, {layer prefix: (w = g v / |v|, bias)}) built from them"""
    leaves = {k: torch.as_tensor(np.asarray(v), dtype=torch.float64).clone().requires_grad_(True) for k, v in sd.items()}
    W = {}
    for k in sd:
        if k.endswith(".bias"):
            pre = k[:-5]
            if pre + ".weight_v" in sd:
                v, g = leaves[pre + ".weight_v"], leaves[pre + ".weight_g"]
                w = v * (g / v.reshape(v.shape[0], -1).norm(dim=1).reshape(g.shape))
            else:
                w = leaves[pre + ".weight"]
            W[pre] = (w, leaves[k])
    return leaves, W


@pytest.mark.parametrize("version,T,B,seed", CASES)
def test_restatement_equals_autograd(version, T, B, seed):
    """cotangents on every tap: every weight_g, weight_v and bias gradient to 1e-11 relative (per tensor, max-norm)"""
    sd = S.disc_state_dict(version, 0)
    leaves, W = normed_weights(sd)
    _, y_hat = S.disc_waves(B, T, seed)
    x = torch.from_numpy(y_hat).to(torch.float64)
    fmaps = forward_with_grad(W, version, x)
    cots = random_cotangents(fmaps, 300 + T)
    sum((c * t).sum() for dc, dt in zip(cots, fmaps) for c, t in zip(dc, dt)).backward()
    taps = [[t.detach() for t in d] for d in fmaps]
    _, deltas = GR.input_grad(R.folded(sd), version, taps, cots, T)
    got = WR.weight_grad(sd, version, x, taps, deltas)
    assert list(got) == list(sd)
    for name, g in got.items():
        want = leaves[name].grad
        assert tuple(g.shape) == tuple(want.shape), name
        e = float((g - want).abs().max() / want.abs().max())
        assert e < 1e-11, (name, e)


def test_plain_weights_and_restriction():
    """a plain-weight state dict gets dW itself; `only` computes the chosen sub-discriminators alone, with the same values"""
    version, T, B = "v1", 47, 1
    sd = S.disc_state_dict(version, 0)
    folded = R.folded(sd)
    plain = {}
    for pre, (w, b) in folded.items():
        plain[pre + ".weight"], plain[pre + ".bias"] = w.numpy(), b.numpy()
    leaves, W = normed_weights(plain)
    _, y_hat = S.disc_waves(B, T, 5)
    x = torch.from_numpy(y_hat).to(torch.float64)
    fmaps = forward_with_grad(W, version, x)
    cots = random_cotangents(fmaps, 9)
    sum((c * t).sum() for dc, dt in zip(cots, fmaps) for c, t in zip(dc, dt)).backward()
    taps = [[t.detach() for t in d] for d in fmaps]
    _, deltas = GR.input_grad(folded, version, taps, cots, T)
    got = WR.weight_grad(plain, version, x, taps, deltas)
    assert set(got) == set(plain)
    for name, g in got.items():
        want = leaves[name].grad
        assert float((g - want).abs().max() / want.abs().max()) < 1e-11, name
    some = WR.weight_grad(plain, version, x, taps, deltas, only=(0, 6))
    assert set(some) == {k for k in plain if k.startswith(("discriminators.0.", "discriminators.6."))}
    assert all(torch.equal(some[k], got[k]) for k in some)


def test_clip_grad_value_closed_form():
    """host tensors: the norm is that of the unclipped gradients divided by batch_size per tensor, the clamp is in place; objects with .grad and bare
    gradient tensors give the same; norm types 1 and 2"""
    from comfy_rvc_amd.lib.infer_pack.commons import clip_grad_value_
    rng = np.random.default_rng(3)
    arrays = [rng.standard_normal(s).astype(np.float32) * sc for s, sc in (((7,), 1.0), ((3, 4, 5), 0.1), ((1,), 5.0), ((16, 1, 1), 2.0))]
    for norm_type in (2, 1):
        for bs in (1, 4):
            want = sum((np.linalg.norm(a.astype(np.float64).ravel(), norm_type) / bs) ** norm_type for a in arrays) ** (1.0 / norm_type)
            ref, _ = WR.clip_grad_value(arrays, None, norm_type, bs)
            grads = [torch.from_numpy(a.copy()) for a in arrays]
            got = clip_grad_value_(grads, None, norm_type, bs)
            assert isinstance(got, float) and abs(got - want) <= 1e-6 * want and abs(ref - want) <= 1e-12 * want
            assert all(np.array_equal(g.numpy(), a) for g, a in zip(grads, arrays)), "clip_value=None must not touch the gradients"
            got = clip_grad_value_(grads, 0.25, norm_type, bs)
            assert abs(got - want) <= 1e-6 * want, "the returned norm is the unclipped one"
            assert all(np.array_equal(g.numpy(), np.clip(a, -0.25, 0.25)) for g, a in zip(grads, arrays))

    class P:
        def __init__(self, g):
            self.grad = g
    params = [P(torch.from_numpy(a.copy())) for a in arrays] + [P(None)]
    assert clip_grad_value_(params, None, 2, 4) == clip_grad_value_([torch.from_numpy(a) for a in arrays], None, 2, 4)
    assert clip_grad_value_(torch.from_numpy(arrays[0]), None) == pytest.approx(float(np.linalg.norm(arrays[0].astype(np.float64))), rel=1e-6)
    assert clip_grad_value_([], None) == 0.0


def test_golden_loads_and_its_numbers_are_consistent():
    """the golden is small, holds one norm per parameter in the state dict's order, and grad_norm_d is clip_grad_value_'s number for those norms"""
    from comfy_rvc_amd.lib.infer_pack.commons import clip_grad_value_
    assert os.path.getsize(os.path.join(GOLDEN, "disc_wgrad_B_v2.npz")) <= 1_000_000
    g, y, y_hat = wgrad_case()
    B = int(g["B"])
    names = [str(n) for n in g["names"]]
    assert names == list(S.disc_spec("v2")) and g["norms"].shape == (len(names),)
    want = float(np.sqrt(np.sum((g["norms"] / B) ** 2)))
    # the reference takes each norm in float32 (Tensor.norm over up to 5.2 M elements), the stored norms are float64: 1e-4 relative covers that rounding
    assert abs(want - float(g["grad_norm_d"])) <= 1e-4 * want
    assert 0 < float(g["grad_norm_d_tol"]) < 0.05 * float(g["grad_norm_d"])
    stored = {n: g["grad." + n] for n in names if "grad." + n in g}
    assert set(stored) == {n for n in names if n.endswith(".bias") or ".conv_post." in n}
    for n, a in stored.items():
        assert tuple(a.shape) == tuple(S.disc_spec("v2")[n])
        assert abs(float(np.linalg.norm(a.astype(np.float64))) - float(g["norms"][names.index(n)])) <= 1e-5 * float(g["norms"][names.index(n)]) + 1e-12
    # the stored full gradients alone, through clip_grad_value_ on host tensors
    part = clip_grad_value_([torch.from_numpy(a) for a in stored.values()], None, batch_size=B)
    want = float(np.sqrt(sum((np.linalg.norm(a.astype(np.float64)) / B) ** 2 for a in stored.values())))
    assert abs(part - want) <= 1e-6 * want


def test_restatement_matches_reference_golden():
    """float64 restatement of the whole discriminator step on case B (forward, loss cotangents, deltas, weight gradients): loss_disc, grad_norm_d within the
    golden's tolerance, per-parameter norms printed"""
    g, y, y_hat = wgrad_case()
    B, T = int(g["B"]), int(g["T"])
    sd = S.disc_state_dict("v2", 0)
    W = R.folded(sd)
    x = torch.from_numpy(np.concatenate([y, y_hat])).to(torch.float64)
    with torch.no_grad():
        fmaps = [(R.disc_p(W, i, p, x) if p else R.disc_s(W, i, x))[1] for i, p in enumerate((0,) + R.PERIODS["v2"])]
    cots = GR.none_like(fmaps)
    loss = 0.0
    for i, d in enumerate(fmaps):
        s = d[-1]
        n = s[:B].numel()
        loss += float(((1 - s[:B]) ** 2).mean() + (s[B:] ** 2).mean())
        cots[i][-1] = torch.cat([-2.0 * (1.0 - s[:B]) / n, 2.0 * s[B:] / n])
    _, deltas = GR.input_grad(W, "v2", fmaps, cots, T)
    grads = WR.weight_grad(sd, "v2", x, fmaps, deltas)
    norm, _ = WR.clip_grad_value(list(grads.values()), None, 2, B)
    print("loss_disc", loss, float(g["loss_disc"]), "grad_norm_d", norm, float(g["grad_norm_d"]), "tolerance", float(g["grad_norm_d_tol"]))
    assert abs(loss - float(g["loss_disc"])) <= 1e-5 * float(g["loss_disc"])
    assert abs(norm - float(g["grad_norm_d"])) <= float(g["grad_norm_d_tol"])
