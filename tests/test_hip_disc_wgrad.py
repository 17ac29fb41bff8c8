"""GPU: the discriminators' weight-gradient pass on the device (rvc_disc_weight_grad: models.*.weight_grad), losses.discriminator_grads and
commons.clip_grad_value_, against the float64 restatement (tests/disc_wgrad_ref.py) fed the DEVICE'S OWN feature maps and deltas, and against the
reference's golden (tools/gen_golden_disc_wgrad.py) for the scalars.  Given the maps and deltas the pass is linear, so the restatement is the exact map the
device has to apply; gate: conftest.rel_err < 1e-3 per tensor, the project's fp32 gate.  Every measured value is kept by conftest.record_parity under
"disc_wgrad.*"; profiles/disc_wgrad_parity.json is a copy of those entries."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import record_parity, rel_err
from comfy_rvc_amd import synthetic as S
import disc_ref as R
import disc_wgrad_ref as WR
from test_disc_wgrad_host import wgrad_case
from test_hip_disc_grad import SENTINEL, SHAPES, carve, dev, random_cotangents, to_dev

pytestmark = pytest.mark.gpu
GATE = 1e-3
DEV = "cuda:0"


def record(name, value, gate):
    record_parity(f"disc_wgrad.{name}", {"measured": float(value), "gate": None if gate is None else float(gate)})


def plain_state_dict(sd):
    """the same net with the weight norm folded: plain .weight tensors in the module's shapes (float32)"""
    out = {}
    for pre, (w, b) in R.folded(sd).items():
        out[pre + ".weight"] = w.to(torch.float32).numpy()
        out[pre + ".bias"] = b.to(torch.float32).numpy()
    return out


@pytest.fixture(scope="module")
def nets():
    from comfy_rvc_amd.lib.infer_pack.models import MultiPeriodDiscriminator, MultiPeriodDiscriminatorV2
    sd = {v: S.disc_state_dict(v, 0) for v in ("v1", "v2")}
    plain = plain_state_dict(sd["v1"])
    return {"v2": (MultiPeriodDiscriminatorV2(False, device=DEV, trainable=True).load_state_dict(sd["v2"]), sd["v2"]),
            "v1": (MultiPeriodDiscriminator(device=DEV, trainable=True).load_state_dict(sd["v1"]), sd["v1"]),
            "v1.plain": (MultiPeriodDiscriminator(device=DEV, trainable=True).load_state_dict(plain), plain),
            "v2.frozen": (MultiPeriodDiscriminatorV2(False, device=DEV).load_state_dict(sd["v2"]), sd["v2"])}


def device_pass(net, x, seed):
    """forward, input gradient with cotangents on every tap, weight gradient: (fmaps, deltas, grads)"""
    fmaps = net.forward_single(x)
    _, deltas = net.input_grad(fmaps, to_dev(random_cotangents(fmaps, seed)), return_deltas=True)
    return fmaps, deltas, net.weight_grad(x, fmaps, deltas)


def check(net, sd, version, x, tag, seed, only=None):
    fmaps, deltas, grads = device_pass(net, x, seed)
    want = WR.weight_grad(sd, version, x, fmaps, deltas, only=only)
    assert list(grads) == list(sd) if "discriminators.0.convs.0.weight_v" in sd else set(grads) == set(sd)
    assert grads.flat.is_contiguous() and grads.flat.numel() == sum(t.numel() for t in grads.values())
    o = 0
    for t in grads.values():                              # views of one buffer, in order
        assert t.dtype == torch.float32 and t.data_ptr() == grads.flat.data_ptr() + 4 * o
        o += t.numel()
    worst = 0.0
    for name, w in want.items():
        g = grads[name]
        assert tuple(g.shape) == tuple(w.shape) == tuple(np.shape(sd[name])), name
        e = rel_err(g.cpu().numpy(), w.numpy())
        record(f"{tag}.{name}", e, GATE)
        if not e < GATE:
            print(tag, name, e)
        worst = max(worst, e)
    print(tag, "largest error over", len(want), "parameter tensors", worst)
    bad = [n for n, w in want.items() if not rel_err(grads[n].cpu().numpy(), w.numpy()) < GATE]
    assert not bad, (tag, bad)
    return worst


# ------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("case,version", [("A", "v2"), ("A", "v1"), ("B", "v2"), ("B", "v1"), ("A", "v1.plain")])
def test_every_gradient_matches_restatement_on_the_devices_buffers(case, version, nets):
    """S = 2 B signals (y, then y_hat).  Case A reaches H = 1 planes (reductions of 2 .. 74 columns), case B has ragged tile edges; the plain-weight net checks
    dW itself."""
    net, sd = nets[version]
    T, B, seed = SHAPES[case]
    x = dev(np.concatenate(S.disc_waves(B, T, seed)))
    check(net, sd, version[:2], x, f"{case}.{version}", 2000 + T)


# ------------------------------------------------------------------------------------------------- 2
def test_trainer_size(nets):
    """T = 12800 (the trainer's segment), B = 1 (S = 2): DiscriminatorS, period 2 (the longest reductions and the most splits) and period 37"""
    net, sd = nets["v2"]
    x = dev(np.concatenate(S.disc_waves(1, 12800, 13)))
    check(net, sd, "v2", x, "T12800.v2", 78, only=(0, 1, 8))


# ------------------------------------------------------------------------------------------------- 3
def test_determinism_and_launch_count(nets):
    net, _ = nets["v2"]
    T, B, seed = SHAPES["B"]
    x = dev(np.concatenate(S.disc_waves(B, T, seed)))
    fmaps, deltas, a = device_pass(net, x, 9)
    before = [t.clone() for d in fmaps + deltas for t in d]
    b = net.weight_grad(x, fmaps, deltas)
    assert torch.equal(a.flat, b.flat), "two calls differ"
    assert all(torch.equal(p, q) for p, q in zip(before, [t for d in fmaps + deltas for t in d])), "the pass changed one of its inputs"
    for v, subs in (("v2", 9), ("v1", 7)):
        n = nets[v][0]
        counts = [n.weight_grad_launch_count(S_, T_) for S_, T_ in ((2, 210), (8, 12800), (1, 997))]
        print("weight-gradient launches", v, counts)
        assert len(set(counts)) == 1 and counts[0] <= 2 * n.launch_count(2, 997) == 2 * (7 + 6 * (subs - 1))


# ------------------------------------------------------------------------------------------------- 4
def test_nothing_is_read_or_written_out_of_range(nets):
    """Signal, feature maps and deltas lie inside NaN-filled device pools; every gradient buffer lies inside a sentinel-filled pool with gaps.  Afterwards the
    sentinels outside are intact, every output is finite and fully written: no tap reached another plane's rows, the pad of the signal or a buffer's outside."""
    from comfy_rvc_amd import _lib
    net, _ = nets["v2"]
    for case in ("A", "B"):
        T, B, seed = SHAPES[case]
        S_ = 2 * B
        x = dev(np.concatenate(S.disc_waves(B, T, seed)))
        fmaps, deltas, want = device_pass(net, x, 5)
        flat_f, flat_d = [t for d in fmaps for t in d], [t for d in deltas for t in d]
        shapes = [tuple(t.shape) for t in flat_f]
        _, fin, _ = carve(shapes, float("nan"))
        _, din, _ = carve(shapes, float("nan"))
        _, sin, _ = carve([(S_, 1, T)], float("nan"))
        for dst, src in zip(fin + din + sin, flat_f + flat_d + [x]):
            dst.copy_(src)
        pool, outs, inside = carve([tuple(t.shape) for t in want.values()], SENTINEL)
        n = len(flat_f)
        arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        _lib.check(_lib.lib.rvc_disc_weight_grad(net._h, _lib.current_stream(), _lib.ptr(sin[0]), S_, T, arr(fin), arr(din), arr(outs)))
        torch.cuda.synchronize()
        assert n == 55
        assert bool((pool[~inside] == SENTINEL).all()), "a kernel wrote outside its buffer"
        assert bool(torch.isfinite(pool).all()), "an out-of-range read reached an output"
        assert not bool((pool[inside] == SENTINEL).any()), "an output is not fully written"
        assert all(torch.equal(o, w) for o, w in zip(outs, want.values()))


# ------------------------------------------------------------------------------------------------- 5
def test_discriminator_grads_and_grad_norm(nets):
    """loss_disc bit-equal to discriminator_loss of the same scores; the trainer's grad_norm_d within the golden's tolerance; clipping clamps in place and
    returns the unclipped norm.  Per-parameter norms and the pointwise difference to the reference's float32 autograd gradients are RECORDED, not gated
    (the forward's rounding flips leaky-ReLU masks: the 0.25 - 0.44 % effect recorded for the input gradient)."""
    from comfy_rvc_amd.lib.infer_pack.commons import clip_grad_value_
    from comfy_rvc_amd.lib.train.losses import discriminator_grads, discriminator_loss
    net, sd = nets["v2"]
    g, y, y_hat = wgrad_case()
    B = int(g["B"])
    loss, grads = discriminator_grads(net, dev(y), dev(y_hat))
    d_r, d_g, _, _ = net(dev(y), dev(y_hat))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and torch.equal(loss, discriminator_loss(d_r, d_g)[0])
    assert abs(float(loss) - float(g["loss_disc"])) <= 1e-3 * float(g["loss_disc"])
    assert list(grads) == [str(n) for n in g["names"]]
    norm = clip_grad_value_(grads.values(), None, batch_size=B)
    delta, tol = abs(norm - float(g["grad_norm_d"])), float(g["grad_norm_d_tol"])
    print("grad_norm_d", norm, "reference", float(g["grad_norm_d"]), "delta", delta, "tolerance", tol)
    record("B.grad_norm_d", delta, tol)
    for k, name in enumerate(grads):
        mine = float(grads[name].double().norm())
        record(f"B.norm.{name}", abs(mine - float(g["norms"][k])) / max(float(g["norms"][k]), 1e-30), None)
        if "grad." + name in g:
            record(f"B.end_to_end.{name}", rel_err(grads[name].cpu().numpy(), g["grad." + name]), None)
    assert delta <= tol
    assert norm == clip_grad_value_(grads.values(), None, batch_size=B), "two calls differ"
    host = WR.clip_grad_value([t.cpu() for t in grads.values()], None, 2, B)[0]
    assert abs(norm - host) <= 1e-9 * host
    clip = 0.5 * float(max(t.abs().max() for t in grads.values()))
    kept = grads.flat.clone()
    assert clip_grad_value_(grads.values(), clip, batch_size=B) == norm, "the returned norm is the unclipped one"
    assert float(grads.flat.abs().max()) <= clip and bool((grads.flat != kept).any())
    assert torch.equal(grads.flat, kept.clamp(-clip, clip))


def test_adversarial_losses_grad_norm(nets):
    """adversarial_losses(..., grad_norm=True) adds the trainer's logged number (batch_size = hps.train.batch_size, no clipping) and changes nothing else;
    with c_gp > 0 the request raises; load_discriminator(trainable=True) builds a net that can form it"""
    from comfy_rvc_amd.lib.infer_pack.commons import clip_grad_value_
    from comfy_rvc_amd.lib.train.evaluate import adversarial_losses, load_discriminator
    from comfy_rvc_amd.lib.train.losses import discriminator_grads
    from comfy_rvc_amd.lib.train.utils import HParams
    net, sd = nets["v2"]
    g, y, y_hat = wgrad_case()
    B = int(g["B"])
    hp = HParams(train={"batch_size": B}, data={"hop_length": 400})
    plain = adversarial_losses(net, dev(y), dev(y_hat), hps=hp)
    out = adversarial_losses(net, dev(y), dev(y_hat), hps=hp, grad_norm=True)
    assert set(out) == set(plain) | {"grad_norm_d"} and all(torch.equal(out[k], plain[k]) for k in plain)
    assert isinstance(out["grad_norm_d"], float)
    assert out["grad_norm_d"] == clip_grad_value_(discriminator_grads(net, dev(y), dev(y_hat))[1].values(), None, batch_size=B)
    assert abs(out["grad_norm_d"] - float(g["grad_norm_d"])) <= float(g["grad_norm_d_tol"])
    with pytest.raises(NotImplementedError):
        adversarial_losses(net, dev(y), dev(y_hat), hps=HParams(train={"batch_size": B, "c_gp": 0.5}, data={"hop_length": 400}), grad_norm=True)
    loaded = load_discriminator({"model": {k: torch.from_numpy(v) for k, v in sd.items()}}, "v2", DEV, trainable=True)
    assert loaded.trainable and adversarial_losses(loaded, dev(y), dev(y_hat), hps=hp, grad_norm=True)["grad_norm_d"] == out["grad_norm_d"]


def test_evaluate_checkpoint_with_grad_norm(tmp_path, nets):
    """grad_norm=True adds grad_norm_d per batch and as their mean; every other number is what it was"""
    from comfy_rvc_amd.lib.train.evaluate import evaluate_checkpoint, load_generator
    from conftest import golden
    from test_hip_train_forward import hps
    e = golden("train_eval_cases.npz")
    filelist = S.write_train_filelist(str(tmp_path), feat_dim=768, spec_bins=1025)
    net_g = load_generator({"model": {k: torch.from_numpy(v) for k, v in S.synth_train_state_dict(S.CONFIG_40K_V2).items()}}, hps())
    kw = dict(seed=int(e["walk_seed"]), batch_size=int(e["walk_batch_size"]), boundaries=[int(x) for x in e["walk_boundaries"]], ckpt_d=nets["v2"][0])
    without = evaluate_checkpoint(net_g, filelist, hps(), **kw)
    with_n = evaluate_checkpoint(net_g, filelist, hps(), grad_norm=True, **kw)
    assert set(with_n) == set(without) | {"grad_norm_d"} and all(with_n[k] == without[k] for k in without if k != "batches")
    norms = [r["grad_norm_d"] for r in with_n["batches"]]
    print("grad_norm_d", with_n["grad_norm_d"], norms)
    assert all(np.isfinite(n) and n > 0 for n in norms) and with_n["grad_norm_d"] == float(np.mean(norms))
    assert all({k: v for k, v in a.items() if k not in ("grad_norm_d", "ids_slice")} == {k: v for k, v in b.items() if k != "ids_slice"}
               for a, b in zip(with_n["batches"], without["batches"]))


# ------------------------------------------------------------------------------------------------- 6
def test_errors(nets):
    """a net loaded without trainable, CPU tensors, wrong shapes and c_gp > 0 each raise; the C entry refuses the frozen net before anything is launched"""
    from comfy_rvc_amd import _lib
    from comfy_rvc_amd.lib.train.losses import discriminator_grads
    net, _ = nets["v2"]
    frozen, _ = nets["v2.frozen"]
    T, B, seed = SHAPES["A"]
    x = dev(np.concatenate(S.disc_waves(B, T, seed)))
    fmaps, deltas, _ = device_pass(net, x, 3)
    with pytest.raises(ValueError):
        frozen.weight_grad(x, fmaps, deltas)
    with pytest.raises(_lib.RvcHipError):
        frozen.weight_grad_launch_count(2, T)
    with pytest.raises(ValueError):
        net.weight_grad(x.cpu(), fmaps, deltas)
    with pytest.raises(ValueError):
        net.weight_grad(x, [[t.cpu() for t in d] for d in fmaps], deltas)
    with pytest.raises(ValueError):
        net.weight_grad(x, fmaps, [[t.cpu() for t in d] for d in deltas])
    with pytest.raises(ValueError):
        net.weight_grad(x[:1], fmaps, deltas)                                     # the maps belong to two signals
    with pytest.raises(ValueError):
        net.weight_grad(x[:, 0], fmaps, deltas)
    with pytest.raises(ValueError):
        net.weight_grad(x, fmaps[:-1], deltas[:-1])
    short = [list(d) for d in deltas]
    short[4][3] = short[4][3][..., :1]
    with pytest.raises(ValueError):
        net.weight_grad(x, fmaps, short)
    half = [list(d) for d in deltas]
    half[2][1] = half[2][1].double()
    with pytest.raises(ValueError):
        net.weight_grad(x, fmaps, half)
    with pytest.raises(NotImplementedError):
        discriminator_grads(net, x[:B], x[B:], c_gp=0.5)
    with pytest.raises(ValueError):
        discriminator_grads(net, x[:B].cpu(), x[B:].cpu())
    with pytest.raises(ValueError):
        discriminator_grads(frozen, x[:B], x[B:])
    # the C entry itself on the frozen net and with a NULL gradient pointer: an error, nothing written
    flat_f, flat_d = [t for d in fmaps for t in d], [t for d in deltas for t in d]
    shapes = net.parameter_shapes()
    outs = [torch.full(s, SENTINEL, device=DEV) for s in shapes.values()]
    arr = lambda ts: (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
    st = _lib.current_stream()
    assert _lib.lib.rvc_disc_weight_grad(frozen._h, st, _lib.ptr(x), 2 * B, T, arr(flat_f), arr(flat_d), arr(outs)) != 0
    assert b"keep_parameters" in _lib.lib.rvc_last_error()
    assert _lib.lib.rvc_disc_weight_grad(net._h, st, _lib.ptr(x), 2 * B, T, arr(flat_f), arr(flat_d), arr(outs[:-1] + [None])) != 0
    assert _lib.lib.rvc_disc_weight_grad(net._h, st, _lib.ptr(x), 2 * B, T, arr(flat_f), arr(flat_d[:-1] + [None]), arr(outs)) != 0
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs)
    assert frozen.parameter_shapes() == shapes == S.disc_spec("v2")
