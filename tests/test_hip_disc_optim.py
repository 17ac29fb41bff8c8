"""GPU: the optimizer step on the device.  G1 rvc_adamw_step alone against the staged float64 gates of tests/adamw_ref.py; G2 rvc_disc_adamw_step on v1, V2 and
the plain-weight net under the same gates; G3 the re-folded weights and re-made images bit for bit the host's (a fresh net loaded from state_dict()); G4 K
trainer steps against the reference's golden (tools/gen_golden_disc_step.py); G5 guard rails; G6 the checkpoint round trip.  Measured values are kept by
conftest.record_parity under "disc_optim.*"; profiles/disc_optim_parity.json is a copy of those entries."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import golden, record_parity
from comfy_rvc_amd import synthetic as S
import adamw_ref as A
import disc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 12345.0
LR2 = 1e-2                                   # G2 / G3: large enough that two steps move every weight by many ulps


def record(name, value, gate):
    record_parity(f"disc_optim.{name}", {"measured": float(value), "gate": None if gate is None else float(gate)})


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def carve_misaligned(sizes, fill, gap=259):
    """one device pool filled with `fill`; a block per size, each starting ONE float past a 16-byte boundary, with untouched elements around the blocks"""
    offs, o = [], gap
    for n in sizes:
        o += (1 - o) % 4
        offs.append(o)
        o += n + gap
    pool = torch.full((o,), fill, dtype=torch.float32, device=DEV)
    assert pool.data_ptr() % 16 == 0
    inside = torch.zeros(o, dtype=torch.bool, device=DEV)
    views = []
    for a, n in zip(offs, sizes):
        views.append(pool[a:a + n])
        inside[a:a + n] = True
        assert views[-1].data_ptr() % 16 == 4
    return pool, views, inside


def hyper(lr, step, clip):
    from comfy_rvc_amd import _lib
    return _lib.AdamwHyper(lr, A.BETAS[0], A.BETAS[1], A.EPS, A.WD, step, int(clip is not None), 0.0 if clip is None else clip)


def raw_step(ps, gs, ms, vs, h):
    from comfy_rvc_amd import _lib
    K = len(ps)
    arr = lambda ts: (C.c_void_p * K)(*[t.data_ptr() for t in ts])
    n = (_lib.c_int64 * K)(*[t.numel() for t in ps])
    return _lib.lib.rvc_adamw_step(_lib.current_stream(), arr(ps), arr(gs), arr(ms), arr(vs), n, K, C.byref(h))


def gate_units_t(p_prev, g, m_prev, v_prev, p, m, v, lr, step, clip):
    """adamw_ref.gate_units on device tensors (float64 on the device: the nets hold 4e7 parameters)"""
    p_prev, g, m_prev, v_prev, p, m, v = (t.double() for t in (p_prev, g, m_prev, v_prev, p, m, v))
    decay, step_size, sbc2 = A.scalars(lr, A.BETAS[0], A.BETAS[1], A.WD, step)
    gc = g if clip is None else g.clamp(-clip, clip)
    m64 = m_prev + (gc - m_prev) * (1 - A.BETAS[0])
    v64 = v_prev * A.BETAS[1] + (1 - A.BETAS[1]) * gc * gc
    delta64 = step_size * (m / (v.sqrt() / sbc2 + A.EPS))
    p64 = p_prev * decay - delta64

    def worst(err, scale):
        err, scale = err.abs(), 4 * A.U * scale
        if bool(((scale == 0) & (err != 0)).any()):
            return float("inf")
        return float(torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.zeros_like(err)).max())
    return (worst(m - m64, m_prev.abs() + gc.abs()), worst(v - v64, v_prev + gc * gc), worst(p - p64, p_prev.abs() + p64.abs() + delta64.abs()))


def dev_gradients(n, seed, clip=A.CLIP):
    """adamw_ref.gradients drawn on the device"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda: torch.rand(n, generator=gen, device=DEV, dtype=torch.float64)
    lo, hi = math.log(1e-14), math.log(clip)
    mag = torch.exp(lo + rnd() * (hi - lo))
    mag = torch.where(rnd() < 0.1, clip * (1.001 + 3.0 * rnd()), mag)
    g = (mag * torch.where(rnd() < 0.5, -1.0, 1.0)).float()
    g[::7] = 0.0
    assert not bool(((g != 0) & (g.abs() < 1e-15)).any())
    return g


# ------------------------------------------------------------------------------------------------- G1
@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("lr", [1e-4, 1e-2])
def test_adamw_kernel_alone(step, lr):
    """K = 10 tensors of 1 .. 4099 elements in one call, every pointer one float past 16-byte alignment, g in a NaN-filled pool, p / m / v in sentinel-filled
    pools; the staged gates, sentinels intact, g unchanged, two calls from the same state the same bits"""
    tensors = A.case(step)
    sizes = [t[0].size for t in tensors]
    assert tuple(sizes) == A.SIZES
    gpool, gs, _ = carve_misaligned(sizes, float("nan"))
    pools = [carve_misaligned(sizes, SENTINEL) for _ in range(3)]
    results = []
    for _ in range(2):
        for k, t in enumerate(tensors):
            gs[k].copy_(dev(t[1]))
            for role in range(3):
                pools[role][1][k].copy_(dev(t[(0, 2, 3)[role]]))
        assert raw_step(pools[0][1], gs, pools[1][1], pools[2][1], hyper(lr, step, A.CLIP)) == 0
        torch.cuda.synchronize()
        results.append([pool.clone() for pool, _, _ in pools])
    assert all(torch.equal(a, b) for a, b in zip(*results)), "two calls from the same state differ"
    for pool, _, inside in pools:
        assert bool((pool[~inside] == SENTINEL).all()), "the kernel wrote outside a tensor"
        assert bool(torch.isfinite(pool).all())
    assert all(np.array_equal(gs[k].cpu().numpy(), t[1]) for k, t in enumerate(tensors)), "the gradient was changed"
    worst, worst_t = np.zeros(3), np.zeros(3)
    for k, (p, g, m, v) in enumerate(tensors):
        out = [pools[role][1][k] for role in range(3)]
        worst = np.maximum(worst, A.gate_units(p, g, m, v, out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy(), lr, A.BETAS, A.EPS, A.WD, step, A.CLIP))
        worst_t = np.maximum(worst_t, gate_units_t(dev(p), dev(g), dev(m), dev(v), out[0], out[1], out[2], lr, step, A.CLIP))
        assert bool((out[0] != dev(p)).any()) or p.size < 3
    print("gate units (m, v, p)", step, lr, worst)
    for name, w in zip("mvp", worst):
        record(f"G1.step{step}.lr{lr}.{name}", w, 1.0)
    assert np.allclose(worst, worst_t, rtol=1e-6), "the device-side gate evaluation disagrees with adamw_ref's"
    assert np.all(worst <= 1.0), worst


def test_adamw_kernel_tensor_count():
    """K = 64 works (and touches nothing else); K = 65 is refused and nothing is launched"""
    from comfy_rvc_amd import _lib
    rng = np.random.default_rng(3)
    for K in (64, 65):
        sizes = [5 + (k % 7) for k in range(K)]
        pools = [carve_misaligned(sizes, SENTINEL, gap=8) for _ in range(4)]
        init = []
        for k, n in enumerate(sizes):
            vals = (rng.standard_normal(n).astype(np.float32), A.gradients(rng, n), np.zeros(n, np.float32), np.zeros(n, np.float32))
            for role in range(4):
                pools[role][1][k].copy_(dev(vals[role]))
            init.append(vals)
        before = [pool.clone() for pool, _, _ in pools]
        if K == 64:
            assert raw_step(pools[0][1], pools[1][1], pools[2][1], pools[3][1], hyper(1e-2, 1, A.CLIP)) == 0
        else:
            # K = 65 needs arrays of 65 entries: the binding's own types take them
            arr = lambda ts: (C.c_void_p * K)(*[t.data_ptr() for t in ts])
            n = (_lib.c_int64 * K)(*sizes)
            h = hyper(1e-2, 1, A.CLIP)
            assert _lib.lib.rvc_adamw_step(_lib.current_stream(), arr(pools[0][1]), arr(pools[1][1]), arr(pools[2][1]), arr(pools[3][1]), n, K, C.byref(h)) != 0
            assert b"64" in _lib.lib.rvc_last_error()
        torch.cuda.synchronize()
        if K == 65:
            assert all(torch.equal(a, pool) for a, (pool, _, _) in zip(before, pools)), "a refused call wrote something"
            continue
        assert torch.equal(before[1], pools[1][0])
        for role in (0, 2, 3):
            pool, views, inside = pools[role]
            assert bool((pool[~inside] == SENTINEL).all())
        for k, (p, g, m, v) in enumerate(init):
            w = A.gate_units(p, g, m, v, *[pools[role][1][k].cpu().numpy() for role in (0, 2, 3)], 1e-2, A.BETAS, A.EPS, A.WD, 1, A.CLIP)
            assert max(w) <= 1.0, (k, w)


def test_clip_none_equals_a_clip_above_every_gradient():
    """has_clip = 0 and a clip value beyond max |g| give the same bits; a biting clip does not"""
    tensors = A.case(2, seed=7, sizes=(4099,))
    outs = []
    for clip in (None, 1e3, A.CLIP):
        bufs = [dev(t).clone() for t in tensors[0]]
        assert raw_step([bufs[0]], [bufs[1]], [bufs[2]], [bufs[3]], hyper(1e-2, 2, clip)) == 0
        outs.append(bufs)
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    assert not torch.equal(outs[0][0], outs[2][0]) and not torch.equal(outs[0][3], outs[2][3])


# ------------------------------------------------------------------------------------------------- G2, G3
def plain_state_dict(sd):
    """the same net with the weight norm folded: plain .weight tensors in the module's shapes (float32)"""
    out = {}
    for pre, (w, b) in R.folded(sd).items():
        out[pre + ".weight"] = w.to(torch.float32).numpy()
        out[pre + ".bias"] = b.to(torch.float32).numpy()
    return out


def build(variant, sd=None, trainable=True):
    from comfy_rvc_amd.lib.infer_pack.models import MultiPeriodDiscriminator, MultiPeriodDiscriminatorV2
    if sd is None:
        sd = S.disc_state_dict(variant[:2], 0)
        if variant.endswith(".plain"):
            sd = plain_state_dict(sd)
    cls = MultiPeriodDiscriminatorV2 if variant.startswith("v2") else MultiPeriodDiscriminator
    return cls(device=DEV, trainable=trainable).load_state_dict(sd)


_stepped = {}


@pytest.fixture(scope="module", autouse=True)
def _release_stepped_nets():
    """the stepped nets are shared by the tests of this file and released with it"""
    yield
    _stepped.clear()
    torch.cuda.empty_cache()


def stepped(variant):
    """the net after two steps from random flat gradients, with what the steps were measured against; made once per variant"""
    if variant in _stepped:
        return _stepped[variant]
    net = build(variant)
    n = net.parameter_count()
    out = {"net": net, "units": [], "count": net.adamw_step_launch_count()}
    p0 = net.get_parameters()
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for step in (1, 2):
        g = dev_gradients(n, 100 * step + len(variant))
        kept = g.clone()
        p_prev, m_prev, v_prev = net.get_parameters(), m.clone(), v.clone()
        net.adamw_step(g, m, v, LR2, A.BETAS, A.EPS, A.WD, step, A.CLIP)
        assert torch.equal(g, kept), "the gradient buffer was changed"
        p = net.get_parameters()
        out["units"].append(gate_units_t(p_prev, g, m_prev, v_prev, p, m, v, LR2, step, A.CLIP))
        if step == 1:                                                  # again from the same state: the same bits
            first = (p.clone(), m.clone(), v.clone(), net.forward_single(probe(210))[1][4].clone())
            net.load_parameters(p0)
            m.zero_()
            v.zero_()
            net.adamw_step(g, m, v, LR2, A.BETAS, A.EPS, A.WD, step, A.CLIP)
            out["same"] = all(torch.equal(a, b) for a, b in zip(first, (net.get_parameters(), m, v, net.forward_single(probe(210))[1][4])))
            out["moved"] = float((p.double() - p0.double()).abs().mean())
        del g, kept, p_prev, m_prev, v_prev
    _stepped[variant] = out
    return out


def probe(T):
    B = 1 if T == 210 else 2
    return dev(np.concatenate(S.disc_waves(B, T, 11 if T == 210 else 12)))


VARIANTS = ["v1", "v2", "v1.plain"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_disc_step_under_the_kernel_gates(variant):
    """two steps of rvc_disc_adamw_step from a random flat gradient: every parameter (through rvc_disc_get_parameters), exp_avg and exp_avg_sq inside G1's gates;
    the launch count a small constant; two runs from the same state the same bits"""
    r = stepped(variant)
    net = r["net"]
    for step, units in enumerate(r["units"], 1):
        print(variant, "step", step, "gate units (m, v, p)", units)
        for name, w in zip("mvp", units):
            record(f"G2.{variant}.step{step}.{name}", w, 1.0)
    assert all(max(u) <= 1.0 for u in r["units"]), r["units"]
    layers = 7 + 6 * (len(net.periods))
    assert r["count"] == net.adamw_step_launch_count() == (2 if variant.endswith(".plain") else 3) <= 2 * layers
    assert r["same"], "two runs from the same state differ"
    assert r["moved"] > 1e-3, "the step did not move the parameters"


@pytest.mark.parametrize("variant", VARIANTS)
def test_refold_is_the_hosts_fold_bit_for_bit(variant):
    """state_dict() of the stepped net loaded into a fresh frozen net (rvc_disc_finalize's host path) and a fresh trainable one: every tap of forward_single,
    dsignals and every delta of input_grad (all phase images) and weight_grad's buffer are torch.equal; load_parameters(get_parameters()) changes no bit"""
    from test_hip_disc_grad import random_cotangents, to_dev
    net = stepped(variant)["net"]
    sd = net.state_dict()
    assert list(sd) == list(net.parameter_shapes()) and all(t.dtype == torch.float32 and not t.is_cuda and tuple(t.shape) == s
                                                             for t, s in zip(sd.values(), net.parameter_shapes().values()))
    frozen, fresh = build(variant, sd, trainable=False), build(variant, sd, trainable=True)
    assert torch.equal(fresh.get_parameters(), net.get_parameters())
    with pytest.raises(ValueError):
        frozen.state_dict()

    def passes(n, x, weight):
        fmaps = n.forward_single(x)
        dsig, deltas = n.input_grad(fmaps, to_dev(random_cotangents(fmaps, 77)), return_deltas=True)
        flat = [t for d in fmaps for t in d] + [dsig] + [t for d in deltas for t in d]
        return flat + ([n.weight_grad(x, fmaps, deltas).flat] if weight else [])

    for T in (210, 997):
        x = probe(T)
        mine = passes(net, x, True)
        for other, weight in ((frozen, False), (fresh, True)):
            theirs = passes(other, x, weight)
            bad = [i for i, (a, b) in enumerate(zip(mine, theirs)) if not torch.equal(a, b)]
            assert not bad, (variant, T, "frozen" if other is frozen else "fresh", bad[:8], len(mine))
        if T == 210:
            net.load_parameters(net.get_parameters())
            assert all(torch.equal(a, b) for a, b in zip(mine, passes(net, x, True))), "load_parameters(get_parameters()) changed a bit"
    assert stepped(variant)["moved"] > 1e-3                # the comparison above is not one of untouched buffers


# ------------------------------------------------------------------------------------------------- G4
def test_trainer_steps_against_the_reference():
    """K calls of train_discriminator_step on the golden's waves: every loss_disc[k] and grad_norm_d[k] inside its stored tolerance, the last loss farther than
    its tolerance from the frozen net's; the parameter-delta norms are recorded next to the reference's, not gated"""
    from comfy_rvc_amd.lib.train.optim import AdamW
    from comfy_rvc_amd.lib.train.train_step import train_discriminator_step
    g = golden("disc_step_B_v2.npz")
    B, T, K = int(g["B"]), int(g["T"]), int(g["K"])
    sd0 = S.disc_state_dict("v2", int(g["weight_seed"]))
    net = build("v2", sd0)
    opt = AdamW(net, float(g["lr"]), betas=(float(g["beta1"]), float(g["beta2"])), eps=float(g["eps"]), weight_decay=float(g["weight_decay"]))
    losses, norms = [], []
    for k in range(K):
        y, y_hat = S.disc_waves(B, T, int(g["wave_seed0"]) + k)
        loss, norm = train_discriminator_step(net, opt, dev(y), dev(y_hat), float(g["clip_value"]), B)
        assert loss.dim() == 0 and loss.dtype == torch.float32 and isinstance(norm, float)
        losses.append(float(loss))
        norms.append(norm)
    bad = []
    for k in range(K):
        dl, dn = abs(losses[k] - float(g["loss_disc"][k])), abs(norms[k] - float(g["grad_norm_d"][k]))
        print(f"step {k}: loss_disc {losses[k]} reference {float(g['loss_disc'][k])} delta {dl} tolerance {float(g['loss_disc_tol'][k])};  "
              f"grad_norm_d {norms[k]} reference {float(g['grad_norm_d'][k])} delta {dn} tolerance {float(g['grad_norm_d_tol'][k])}")
        record(f"G4.loss_disc.{k}", dl, g["loss_disc_tol"][k])
        record(f"G4.grad_norm_d.{k}", dn, g["grad_norm_d_tol"][k])
        if not (dl <= float(g["loss_disc_tol"][k]) and dn <= float(g["grad_norm_d_tol"][k])):
            bad.append(k)
    gap = abs(losses[-1] - float(g["loss_disc_frozen"][-1]))
    record("G4.gap_to_frozen", gap, g["loss_disc_tol"][-1])
    after = net.state_dict()
    assert list(after) == [str(n) for n in g["names"]]
    for k, name in enumerate(after):
        mine = float((after[name].double() - torch.from_numpy(sd0[name]).double()).norm())
        record(f"G4.delta_norm.{name}", mine, None)
        record(f"G4.delta_norm_reference.{name}", float(g["delta_norms"][k]), None)
    assert opt.state_dict()["state"][0]["step"] == K
    assert not bad, bad
    assert gap > float(g["loss_disc_tol"][-1]), "the stepped net cannot be told from the frozen one"


# ------------------------------------------------------------------------------------------------- G5, G6
def test_guard_rails():
    """step on a net without trainable=True raises (Python and C entry); anything that is not weight_grad's result raises; a frozen net's forward gives the same
    bits before and after another net is stepped"""
    from comfy_rvc_amd import _lib
    from comfy_rvc_amd.lib.train.optim import AdamW
    from comfy_rvc_amd.lib.train.train_step import train_discriminator_step
    frozen = build("v1", trainable=False)
    x = probe(210)
    before = [t.clone() for d in frozen.forward_single(x) for t in d]
    y, y_hat = (dev(w) for w in S.disc_waves(1, 210, 11))
    with pytest.raises(ValueError):
        train_discriminator_step(frozen, AdamW(frozen, 1e-4), y, y_hat, None, 1)
    n = sum(int(np.prod(s)) for s in frozen.parameter_shapes().values())
    bufs = [torch.zeros(n, device=DEV) for _ in range(3)]
    h = hyper(1e-4, 1, None)
    assert _lib.lib.rvc_disc_adamw_step(frozen._h, _lib.current_stream(), _lib.ptr(bufs[0]), _lib.ptr(bufs[1]), _lib.ptr(bufs[2]), C.byref(h)) != 0
    assert b"keep_parameters" in _lib.lib.rvc_last_error()
    assert _lib.lib.rvc_disc_adamw_step_launch_count(frozen._h) == -1
    with pytest.raises(ValueError):
        frozen.get_parameters()
    net = build("v1")                                                     # another net, stepped while the frozen one exists
    opt = AdamW(net, 1e-4, betas=A.BETAS, eps=A.EPS)
    loss, _ = train_discriminator_step(net, opt, y, y_hat, A.CLIP, 1)
    assert opt._step == 1 and float(train_discriminator_step(net, opt, y, y_hat, A.CLIP, 1)[0]) != float(loss)
    for wrong in ({"a": bufs[0]}, bufs[0], None):
        with pytest.raises(ValueError):
            opt.step(wrong)

    class Short(dict):
        flat = bufs[0][:-1]
    with pytest.raises(ValueError):
        opt.step(Short())
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(NotImplementedError):
        opt.step(Short())
    with pytest.raises(NotImplementedError):
        AdamW(net, 1e-4).load_state_dict(opt.state_dict())
    h0 = hyper(1e-4, 0, None)
    assert _lib.lib.rvc_disc_adamw_step(net._h, _lib.current_stream(), _lib.ptr(bufs[0]), _lib.ptr(bufs[1]), _lib.ptr(bufs[2]), C.byref(h0)) != 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, [t for d in frozen.forward_single(x) for t in d]))


def test_checkpoint_round_trip(tmp_path):
    """save_checkpoint writes the reference's keys and torch.optim.AdamW's optimizer format; after load_checkpoint into a new net and optimizer the next step
    gives the bits of continuing without the round trip"""
    from comfy_rvc_amd.lib.train.optim import AdamW, ExponentialLR
    from comfy_rvc_amd.lib.train.train_step import train_discriminator_step
    from comfy_rvc_amd.lib.train.utils import latest_checkpoint_path, load_checkpoint, save_checkpoint
    T, B = 997, 1
    waves = [tuple(dev(w) for w in S.disc_waves(B, T, 20 + k)) for k in range(2)]
    net = build("v1")
    opt = AdamW(net, 1e-4, betas=A.BETAS, eps=A.EPS)
    sched = ExponentialLR(opt, 0.999875)
    train_discriminator_step(net, opt, *waves[0], A.CLIP, B)
    sched.step()
    save_checkpoint(net, opt, opt.param_groups[0]["lr"], 3, str(tmp_path / "D_3.pth"), note="x")
    (tmp_path / "D_12.pth").write_bytes(b"")
    assert latest_checkpoint_path(str(tmp_path), "D_*.pth").endswith("D_12.pth")
    ck = torch.load(str(tmp_path / "D_3.pth"), map_location="cpu")
    assert set(ck) == {"model", "iteration", "optimizer", "learning_rate", "kwargs"} and ck["iteration"] == 3 and ck["kwargs"] == {"note": "x"}
    assert list(ck["model"]) == list(net.parameter_shapes())
    assert set(ck["optimizer"]) == {"state", "param_groups"} and sorted(ck["optimizer"]["state"]) == list(range(len(ck["model"])))
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} and float(s["step"]) == 1.0 for s in ck["optimizer"]["state"].values())
    theirs = torch.optim.AdamW([torch.nn.Parameter(t.clone()) for t in ck["model"].values()], 1.0)      # the real class takes the state as it is
    theirs.load_state_dict(ck["optimizer"])
    group = theirs.param_groups[0]
    assert group["lr"] == ck["learning_rate"] == opt.param_groups[0]["lr"] and group["initial_lr"] == 1e-4 and tuple(group["betas"]) == A.BETAS
    del theirs
    net2 = build("v1")
    opt2 = AdamW(net2, 1.0)
    _, _, lr, iteration, kwargs = load_checkpoint(str(tmp_path / "D_3.pth"), net2, opt2)
    assert (lr, iteration, kwargs) == (ck["learning_rate"], 3, {"note": "x"})
    assert torch.equal(net2.get_parameters(), net.get_parameters())
    a = train_discriminator_step(net, opt, *waves[1], A.CLIP, B)
    b = train_discriminator_step(net2, opt2, *waves[1], A.CLIP, B)
    assert torch.equal(a[0], b[0]) and a[1] == b[1]
    assert torch.equal(net2.get_parameters(), net.get_parameters()) and torch.equal(opt2._m, opt._m) and torch.equal(opt2._v, opt._v)
    assert ExponentialLR(opt2, 0.999875, last_epoch=0).get_last_lr() == sched.get_last_lr()
