"""CPU: the restatement of the discriminators' input-gradient pass (tests/disc_grad_ref.py) against torch autograd through tests/disc_ref.py, and its gradient
penalty and loss-balancer norms against the reference's goldens (tools/gen_golden_disc_grad.py).  The GPU tests (test_hip_disc_grad.py) compare the device
with this restatement fed the device's own feature maps."""
import numpy as np
import pytest
import torch

from conftest import golden
from comfy_rvc_amd import synthetic as S
import disc_ref as R
import disc_grad_ref as GR

CASES = [("v2", 210, 1, 11), ("v1", 210, 1, 11), ("v2", 997, 2, 12)]      # case A (v1 and V2) and case B of the forward's goldens


def grad_case():
    g = golden("disc_grad_B_v2.npz")
    y, y_hat = S.disc_waves(int(g["B"]), int(g["T"]), int(g["wave_seed"]))
    return g, y, y_hat


def forward_with_grad(W, version, x):
    """disc_ref's sub-discriminators on x (requires grad), every tap keeping its gradient: [[tap...] per sub-discriminator]"""
    fmaps = []
    for i, period in enumerate((0,) + R.PERIODS[version]):
        _, fmap = R.disc_p(W, i, period, x) if period else R.disc_s(W, i, x)
        for t in fmap:
            t.retain_grad()
        fmaps.append(fmap)
    return fmaps


def random_cotangents(fmaps, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(t.shape, generator=g, dtype=torch.float64) * (scale / np.sqrt(t[0].numel())) for t in d] for d in fmaps]


@pytest.mark.parametrize("version,T,B,seed", CASES)
def test_restatement_equals_autograd(version, T, B, seed):
    """cotangents on every tap: the signal gradient, and every delta_l (autograd's gradient of tap l times the mask), to 1e-12 relative"""
    W = R.folded(S.disc_state_dict(version, 0))
    _, y_hat = S.disc_waves(B, T, seed)
    x = torch.from_numpy(y_hat).to(torch.float64).requires_grad_(True)
    fmaps = forward_with_grad(W, version, x)
    cots = random_cotangents(fmaps, 100 + T)
    sum((c * t).sum() for dc, dt in zip(cots, fmaps) for c, t in zip(dc, dt)).backward()
    got, deltas = GR.input_grad(W, version, [[t.detach() for t in d] for d in fmaps], cots, T)
    assert tuple(got.shape) == (B, 1, T)
    e = float((got - x.grad).abs().max() / x.grad.abs().max())
    print(version, T, "signal gradient", e)
    assert e < 1e-12
    for i, d in enumerate(fmaps):
        for l, t in enumerate(d):
            mask = 1.0 if l + 1 == len(d) else GR.mask(t.detach())
            want = t.grad * mask
            e = float((deltas[i][l] - want).abs().max() / want.abs().max())
            assert e < 1e-12, (i, l, e)


def test_scores_only_and_single_tap_equal_autograd():
    """null cotangents: only the scores, then only one inner tap"""
    version, T, B = "v2", 210, 1
    W = R.folded(S.disc_state_dict(version, 0))
    _, y_hat = S.disc_waves(B, T, 11)
    for pick in ("scores", (3, 2)):
        x = torch.from_numpy(y_hat).to(torch.float64).requires_grad_(True)
        fmaps = forward_with_grad(W, version, x)
        full = random_cotangents(fmaps, 5)
        cots = GR.none_like(fmaps)
        if pick == "scores":
            for i in range(len(fmaps)):
                cots[i][-1] = full[i][-1]
        else:
            cots[pick[0]][pick[1]] = full[pick[0]][pick[1]]
        sum((c * t).sum() for dc, dt in zip(cots, fmaps) for c, t in zip(dc, dt) if c is not None).backward()
        got, _ = GR.input_grad(W, version, [[t.detach() for t in d] for d in fmaps], cots, T)
        assert float((got - x.grad).abs().max() / x.grad.abs().max()) < 1e-12


def test_loss_cotangents_equal_autograd():
    """the three GAN losses' cotangents through the restatement equal autograd of disc_ref's losses"""
    g, y, y_hat = grad_case()
    T = int(g["T"])
    W = R.folded(S.disc_state_dict("v2", 0))
    real = R.forward(None, "v2", y, y_hat, W=W)
    for name in ("disc", "gen", "fm"):
        x = torch.from_numpy(y_hat).to(torch.float64).requires_grad_(True)
        fmaps = forward_with_grad(W, "v2", x)
        scores = [torch.flatten(d[-1], 1, -1) for d in fmaps]
        if name == "disc":
            loss = sum(torch.mean(s ** 2) for s in scores)
            cots = GR.with_scores(fmaps, GR.cot_discriminator_generated([s.detach() for s in scores]))
        elif name == "gen":
            loss = R.generator_loss(scores)[0]
            cots = GR.with_scores(fmaps, GR.cot_generator([s.detach() for s in scores]))
        else:
            loss = R.feature_loss(real[2], fmaps)
            cots = GR.cot_feature(real[2], [[t.detach() for t in d] for d in fmaps])
        loss.backward()
        got, _ = GR.input_grad(W, "v2", [[t.detach() for t in d] for d in fmaps], cots, T)
        e = float((got - x.grad).abs().max() / x.grad.abs().max())
        print(name, e)
        assert e < 1e-12


def test_penalty_and_norms_match_reference():
    """with the recorded alpha the restatement's penalty and balancer norms lie within the stored tolerances of the reference's"""
    g, y, y_hat = grad_case()
    T = int(g["T"])
    W = R.folded(S.disc_state_dict("v2", 0))
    x = GR.interpolate(g["alpha"], y, y_hat)
    with torch.no_grad():
        res = R.forward(None, "v2", y, x, W=W)
    grad, _ = GR.input_grad(W, "v2", res[3], GR.with_scores(res[3], GR.cot_discriminator_generated(res[1])), T)
    got = {"penalty": GR.penalty(grad)}
    with torch.no_grad():
        res = R.forward(None, "v2", y, y_hat, W=W)
    got["norm_gen"] = GR.balancer_norm(GR.input_grad(W, "v2", res[3], GR.with_scores(res[3], GR.cot_generator(res[1])), T)[0])
    got["norm_fm"] = GR.balancer_norm(GR.input_grad(W, "v2", res[3], GR.cot_feature(res[2], res[3]), T)[0])
    for k, v in got.items():
        d, tol = abs(v - float(g[k])), float(g[k + "_tol"])
        print(k, v, "reference", float(g[k]), "delta", d, "tolerance", tol)
        assert d <= tol
    assert abs(GR.penalty(g["grad_pen"]) - float(g["penalty"])) <= 1e-5 * float(g["penalty"])      # the stored gradient is the penalty's
