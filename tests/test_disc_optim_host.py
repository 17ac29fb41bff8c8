"""CPU: the float64 restatement of AdamW (tests/adamw_ref.py) against torch's, torch's float32 kernel inside the device test's gates, ExponentialLR against
torch's, and the optimizer's state-dict conversion through a real torch.optim.AdamW."""
import collections
import copy

import numpy as np
import pytest
import torch

import adamw_ref as A
from comfy_rvc_amd.lib.train import optim as O

LR = 1e-4


def torch_steps(params, grads_per_step, dtype, preset_step, m0=None, v0=None, lr=LR, clip=None):
    """torch.optim.AdamW on the CPU: the parameters after the steps, with its state; preset_step > 0 starts from a loaded state"""
    ps = [torch.nn.Parameter(torch.tensor(p, dtype=dtype)) for p in params]
    opt = torch.optim.AdamW(ps, lr, betas=A.BETAS, eps=A.EPS, weight_decay=A.WD)
    if preset_step > 0:
        sd = opt.state_dict()
        sd["state"] = {k: {"step": torch.tensor(float(preset_step)), "exp_avg": torch.tensor(m0[k], dtype=dtype), "exp_avg_sq": torch.tensor(v0[k], dtype=dtype)}
                       for k in range(len(ps))}
        opt.load_state_dict(sd)
    for grads in grads_per_step:
        for p, g in zip(ps, grads):
            p.grad = torch.tensor(g, dtype=dtype)
            if clip is not None:
                p.grad.clamp_(-clip, clip)
        opt.step()
    return ps, opt


# ------------------------------------------------------------------------------------------------- H1
@pytest.mark.parametrize("preset", [0, 1, 999])
def test_restatement_equals_torch_float64(preset):
    """3 steps with the clamp, from a preset step count of 0, 1 and 999: 1e-14 relative"""
    rng = np.random.default_rng(preset)
    sizes = (1, 17, 300)
    p = [rng.standard_normal(n) for n in sizes]
    m = [0.1 * rng.standard_normal(n) * (preset > 0) for n in sizes]
    v = [0.01 * rng.random(n) * (preset > 0) for n in sizes]
    grads = [[A.gradients(rng, n).astype(np.float64) for n in sizes] for _ in range(3)]
    ps, opt = torch_steps(p, grads, torch.float64, preset, m, v, clip=A.CLIP)
    for k in range(len(sizes)):
        pk, mk, vk = p[k], m[k], v[k]
        for s in range(3):
            pk, mk, vk = A.step64(pk, grads[s][k], mk, vk, LR, A.BETAS, A.EPS, A.WD, preset + s + 1, A.CLIP)
        st = opt.state[ps[k]]
        assert float(st["step"]) == preset + 3
        for mine, theirs in ((pk, ps[k]), (mk, st["exp_avg"]), (vk, st["exp_avg_sq"])):
            theirs = theirs.detach().numpy()
            assert np.max(np.abs(mine - theirs)) <= 1e-14 * max(np.max(np.abs(theirs)), 1e-300)


# ------------------------------------------------------------------------------------------------- H2
@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("lr", [1e-4, 1e-2])
def test_torch_float32_lies_inside_the_device_gates(step, lr):
    """torch's own float32 CPU kernel on the very inputs of the device test G1 passes G1's staged gates"""
    tensors = A.case(step)
    ps, opt = torch_steps([t[0] for t in tensors], [[t[1] for t in tensors]], torch.float32, step - 1, [t[2] for t in tensors], [t[3] for t in tensors], lr=lr,
                          clip=A.CLIP)
    worst = np.zeros(3)
    for (p, g, m, v), q in zip(tensors, ps):
        st = opt.state[q]
        worst = np.maximum(worst, A.gate_units(p, g, m, v, q.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), lr, A.BETAS, A.EPS, A.WD, step, A.CLIP))
    print("torch float32 in gate units (m, v, p)", step, lr, worst)
    assert np.all(worst <= 1.0), worst


# ------------------------------------------------------------------------------------------------- H3
class _Groups:
    def __init__(self, lr):
        self.param_groups = [{"lr": lr}]


@pytest.mark.parametrize("last_epoch", [-1, 0, 5])
def test_exponential_lr_gives_torchs_floats(last_epoch):
    gamma = 0.999875
    p = torch.nn.Parameter(torch.zeros(2))
    theirs_opt, mine_opt = torch.optim.AdamW([p], LR, betas=A.BETAS, eps=A.EPS), _Groups(LR)
    if last_epoch >= 0:
        with pytest.raises(KeyError):
            O.ExponentialLR(_Groups(LR), gamma, last_epoch=last_epoch)
        theirs_opt.param_groups[0]["initial_lr"] = mine_opt.param_groups[0]["initial_lr"] = LR
    theirs = torch.optim.lr_scheduler.ExponentialLR(theirs_opt, gamma, last_epoch=last_epoch)
    mine = O.ExponentialLR(mine_opt, gamma, last_epoch=last_epoch)
    for _ in range(10):
        assert mine_opt.param_groups[0]["lr"] == theirs_opt.param_groups[0]["lr"] and mine.get_last_lr() == theirs.get_last_lr()
        assert mine.last_epoch == theirs.last_epoch and mine_opt.param_groups[0]["initial_lr"] == theirs_opt.param_groups[0]["initial_lr"]
        theirs_opt.step()
        theirs.step()
        mine.step()
    assert mine_opt.param_groups[0]["lr"] == theirs_opt.param_groups[0]["lr"] != LR
    sd = mine.state_dict()
    assert {k: sd[k] for k in ("gamma", "last_epoch", "base_lrs", "_last_lr")} == {k: theirs.state_dict()[k] for k in ("gamma", "last_epoch", "base_lrs", "_last_lr")}


# ------------------------------------------------------------------------------------------------- H4
def test_state_conversion_round_trip_through_torch():
    """our state dict loads into torch.optim.AdamW; one torch step equals one restated step; torch's state converts back to the flat buffers"""
    rng = np.random.default_rng(5)
    shapes = collections.OrderedDict([("a.bias", (4,)), ("a.weight_g", (4, 1, 1)), ("a.weight_v", (4, 3, 5)), ("b.bias", (1,))])
    sizes = [int(np.prod(s)) for s in shapes.values()]
    total = sum(sizes)
    p = rng.standard_normal(total)
    m, v, step = (0.1 * rng.standard_normal(total)).astype(np.float32), (0.01 * rng.random(total)).astype(np.float32), 7
    group = O.torch_group_defaults()
    group.update(lr=LR, betas=A.BETAS, eps=A.EPS, weight_decay=A.WD, params=list(range(len(shapes))))
    ours = {"state": O.state_from_flat(step, torch.from_numpy(m), torch.from_numpy(v), shapes), "param_groups": [group]}
    offs = np.concatenate([[0], np.cumsum(sizes)])
    ps = [torch.nn.Parameter(torch.tensor(p[offs[k]:offs[k + 1]].reshape(s), dtype=torch.float64)) for k, s in enumerate(shapes.values())]
    opt = torch.optim.AdamW(ps, 1.0)
    assert set(opt.state_dict()["param_groups"][0]) == set(group)
    opt.load_state_dict(copy.deepcopy(ours))              # torch keeps the step tensors it is given and counts on in them
    assert opt.param_groups[0]["lr"] == LR and tuple(opt.param_groups[0]["betas"]) == A.BETAS
    g = rng.standard_normal(total)
    for k, q in enumerate(ps):
        q.grad = torch.tensor(g[offs[k]:offs[k + 1]].reshape(q.shape), dtype=torch.float64)
    opt.step()
    p1, m1, v1 = A.step64(p, g, m, v, LR, A.BETAS, A.EPS, A.WD, step + 1)
    got = np.concatenate([q.detach().numpy().reshape(-1) for q in ps])
    assert np.max(np.abs(got - p1)) <= 1e-14 * np.max(np.abs(p1))
    back_step, bm, bv = O.state_to_flat(opt.state_dict()["state"], shapes)
    assert back_step == step + 1 and bm.dtype == torch.float32
    assert np.max(np.abs(bm.numpy() - m1)) <= 2 * A.U * np.max(np.abs(m1)) and np.max(np.abs(bv.numpy() - v1)) <= 2 * A.U * np.max(np.abs(v1))
    # the conversion itself loses nothing
    s2, m2, v2 = O.state_to_flat(ours["state"], shapes)
    assert s2 == step and torch.equal(m2, torch.from_numpy(m)) and torch.equal(v2, torch.from_numpy(v))
    assert O.state_from_flat(0, m2, v2, shapes) == {} and O.state_to_flat({}, shapes)[0] == 0
    bad = dict(ours["state"])
    bad[1] = dict(bad[1], step=torch.tensor(3.0))
    with pytest.raises(ValueError):
        O.state_to_flat(bad, shapes)
    with pytest.raises(ValueError):
        O.state_to_flat({0: ours["state"][0]}, shapes)
