"""GPU: the discriminators' input-gradient pass on the device (rvc_disc_input_grad: models.*.input_grad), gradient_norm_loss, adversarial_input_grads and the
checkpoint evaluation with hps.train.c_gp, against the float64 restatement (tests/disc_grad_ref.py) fed the DEVICE'S OWN feature maps, and against the
reference's goldens (tools/gen_golden_disc_grad.py) for the scalars.  Given the feature maps the pass is linear, so the restatement is the exact map the
device has to apply; gate: conftest.rel_err < 1e-3, the project's fp32 gate.  Every measured value is kept by conftest.record_parity under "disc_grad.*";
profiles/disc_grad_parity.json is a copy of those entries."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import record_parity, rel_err
from comfy_rvc_amd import synthetic as S
import disc_ref as R
import disc_grad_ref as GR
from test_disc_grad_host import grad_case

pytestmark = pytest.mark.gpu
GATE = 1e-3
DEV = "cuda:0"
SHAPES = {"A": (210, 1, 11), "B": (997, 2, 12)}            # T, B, disc_waves seed: the forward's two golden cases


def record(name, value, gate):
    record_parity(f"disc_grad.{name}", {"measured": float(value), "gate": None if gate is None else float(gate)})


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(scope="module")
def nets():
    from comfy_rvc_amd.lib.infer_pack.models import MultiPeriodDiscriminator, MultiPeriodDiscriminatorV2
    sd = {v: S.disc_state_dict(v, 0) for v in ("v1", "v2")}
    return {"v2": (MultiPeriodDiscriminatorV2(False, device=DEV).load_state_dict(sd["v2"]), R.folded(sd["v2"])),
            "v1": (MultiPeriodDiscriminator(device=DEV).load_state_dict({k: torch.from_numpy(v) for k, v in sd["v1"].items()}), R.folded(sd["v1"]))}


def random_cotangents(fmaps, seed):
    """float32 numpy cotangents of every tap, about unit 2-norm per item"""
    rng = np.random.default_rng(seed)
    return [[(rng.standard_normal(tuple(t.shape)) / np.sqrt(t[0].numel())).astype(np.float32) for t in d] for d in fmaps]


def to_dev(cots):
    return [[None if c is None else dev(c) for c in d] for d in cots]


def check_vjp(net, W, version, fmaps, cots, T, tag, deltas=True):
    """device against the restatement on the same feature maps and cotangents; returns the largest error"""
    out = net.input_grad(fmaps, to_dev(cots), return_deltas=True)
    want, want_d = GR.input_grad(W, version, fmaps, cots, T)
    assert out[0].dtype == torch.float32 and tuple(out[0].shape) == tuple(want.shape)
    worst = rel_err(out[0].cpu().numpy(), want.numpy())
    record(f"{tag}.dsignals", worst, GATE)
    print(tag, "dsignals", worst)
    assert worst < GATE, (tag, worst)
    if deltas:
        for i, d in enumerate(want_d):
            for l, w in enumerate(d):
                e = rel_err(out[1][i][l].cpu().numpy(), w.numpy())
                record(f"{tag}.d{i}.delta{l}", e, GATE)
                assert e < GATE, (tag, i, l, e)
                worst = max(worst, e)
        print(tag, "largest error over dsignals and every delta", worst)
    return worst


# ------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("case,version", [("A", "v2"), ("A", "v1"), ("B", "v2"), ("B", "v1")])
def test_vjp_matches_restatement_on_the_devices_feature_maps(case, version, nets):
    """cotangents on every tap, on the scores only (every other pointer NULL), on a single inner tap only"""
    net, W = nets[version]
    T, B, seed = SHAPES[case]
    _, y_hat = S.disc_waves(B, T, seed)
    fmaps = net.forward_single(dev(y_hat))
    full = random_cotangents(fmaps, 1000 + T)
    check_vjp(net, W, version, fmaps, full, T, f"{case}.{version}.all")
    scores = GR.none_like(fmaps)
    for i in range(len(fmaps)):
        scores[i][-1] = full[i][-1]
    check_vjp(net, W, version, fmaps, scores, T, f"{case}.{version}.scores")
    for (i, l) in ((3, 2), (0, 4)):                      # a stride-3 GEMM layer's output in a DiscriminatorP; the last grouped layer of DiscriminatorS
        one = GR.none_like(fmaps)
        one[i][l] = full[i][l]
        check_vjp(net, W, version, fmaps, one, T, f"{case}.{version}.tap{i}_{l}")


# ------------------------------------------------------------------------------------------------- 2
def test_trainer_size(nets):
    """T = 12800 (the trainer's segment), B = 1: many column tiles per phase; the signal gradient only"""
    net, W = nets["v2"]
    _, y_hat = S.disc_waves(1, 12800, 13)
    fmaps = net.forward_single(dev(y_hat))
    check_vjp(net, W, "v2", fmaps, random_cotangents(fmaps, 77), 12800, "T12800.v2.all", deltas=False)


# ------------------------------------------------------------------------------------------------- 3
SENTINEL = 12345.0


def carve(shapes, fill, gap=1024):
    """one device pool filled with `fill`; a contiguous block per shape with `gap` untouched elements in front of, between and behind the blocks"""
    sizes = [int(np.prod(s)) for s in shapes]
    pool = torch.full((gap + sum(n + gap for n in sizes),), fill, dtype=torch.float32, device=DEV)
    views, inside, o = [], torch.zeros(pool.numel(), dtype=torch.bool, device=DEV), gap
    for s, n in zip(shapes, sizes):
        views.append(pool[o:o + n].view(*s))
        inside[o:o + n] = True
        o += n + gap
    return pool, views, inside


def test_nothing_is_read_or_written_out_of_range(nets):
    """Every input (feature maps, cotangents) lies inside a NaN-filled device buffer; dsignals and every work buffer lie inside a sentinel-filled one larger
    than their extent.  Afterwards the sentinels are intact and every output is finite: no tap reached another plane's rows or a buffer's outside."""
    from comfy_rvc_amd import _lib
    net, _ = nets["v2"]
    for case in ("A", "B"):
        T, B, seed = SHAPES[case]
        _, y_hat = S.disc_waves(B, T, seed)
        grouped = net.forward_single(dev(y_hat))
        fmaps = [t for d in grouped for t in d]
        shapes = [tuple(t.shape) for t in fmaps]
        cots = [dev(c) for c in random_cotangents([fmaps], 5)[0]]
        _, fin, _ = carve(shapes, float("nan"))
        _, cin, _ = carve(shapes, float("nan"))
        for dst, src in zip(fin + cin, fmaps + cots):
            dst.copy_(src)
        pool, outs, inside = carve(shapes + [(B, 1, T)], SENTINEL)
        n = len(fmaps)
        arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        _lib.check(_lib.lib.rvc_disc_input_grad(net._h, _lib.current_stream(), B, T, arr(fin), arr(cin), arr(outs[:n]), _lib.ptr(outs[n])))
        torch.cuda.synchronize()
        assert bool((pool[~inside] == SENTINEL).all()), "a kernel wrote outside its buffer"
        assert bool(torch.isfinite(pool).all()), "an out-of-range read reached an output"
        assert not bool((pool[inside] == SENTINEL).any()), "an output is not fully written"
        it = iter(cots)
        assert torch.equal(outs[n], net.input_grad(grouped, [[next(it) for _ in d] for d in grouped]))


# ------------------------------------------------------------------------------------------------- 4
def test_gradient_norm_loss_and_balancer_norms_match_reference(nets):
    """gradient_norm_loss with the recorded alpha, and adversarial_input_grads' two norms, within the golden's tolerances; the penalty recomputed on the host
    in float64 from the device's own gradient agrees with the returned value to 1e-6 relative; alpha=None with a seeded generator is reproducible."""
    from comfy_rvc_amd.lib.train.losses import adversarial_input_grads, gradient_norm_loss
    net, _ = nets["v2"]
    g, y, y_hat = grad_case()
    loss, grad = gradient_norm_loss(dev(y), dev(y_hat), net, alpha=torch.from_numpy(g["alpha"]), return_gradient=True)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and tuple(grad.shape) == y.shape
    assert torch.equal(loss, gradient_norm_loss(dev(y), dev(y_hat), net, alpha=torch.from_numpy(g["alpha"])))
    host = GR.penalty(grad)
    print("penalty", float(loss), "host float64 from the device gradient", host, "reference", float(g["penalty"]), "tolerance", float(g["penalty_tol"]))
    record("B.penalty", abs(float(loss) - float(g["penalty"])), float(g["penalty_tol"]))
    record("B.penalty_vs_host", abs(float(loss) - host) / host, 1e-6)
    assert abs(float(loss) - float(g["penalty"])) <= float(g["penalty_tol"])
    assert abs(float(loss) - host) <= 1e-6 * host
    grads, norms = adversarial_input_grads(net, dev(y), dev(y_hat))
    assert set(grads) == set(norms) == {"loss_gen", "loss_fm"}
    for k, name in (("loss_gen", "norm_gen"), ("loss_fm", "norm_fm")):
        assert tuple(grads[k].shape) == y.shape and norms[k].dim() == 0 and norms[k].dtype == torch.float32
        d, tol = abs(float(norms[k]) - float(g[name])), float(g[name + "_tol"])
        print(name, float(norms[k]), "reference", float(g[name]), "delta", d, "tolerance", tol)
        record(f"B.{name}", d, tol)
        assert d <= tol
        assert abs(float(norms[k]) - GR.balancer_norm(grads[k])) <= 1e-6 * float(norms[k])
    a = gradient_norm_loss(dev(y), dev(y_hat), net, generator=torch.Generator().manual_seed(5))
    b = gradient_norm_loss(dev(y), dev(y_hat), net, generator=torch.Generator().manual_seed(5))
    c = gradient_norm_loss(dev(y), dev(y_hat), net, generator=torch.Generator().manual_seed(6))
    assert torch.equal(a, b) and not torch.equal(a, c)


# ------------------------------------------------------------------------------------------------- 5
def test_end_to_end_difference_is_recorded(nets):
    """The device gradients against the golden's float32 autograd gradients of the reference's own forward: max-norm and relative L2, RECORDED, NOT GATED.
    The pointwise gradient is ill conditioned in the forward's rounding: noise of 3e-6 of each layer's peak on the pre-activations (the bf16x3 error of one
    layer) moves it by 1.6 - 3.1 % in max-norm, because one flipped unit beside a short score layer (period 37 runs at H = 1) moves the whole field.  The
    scalars formed from it are well conditioned and are gated above; the linear map itself is gated against the restatement."""
    from comfy_rvc_amd.lib.train.losses import adversarial_input_grads, gradient_norm_loss
    net, _ = nets["v2"]
    g, y, y_hat = grad_case()
    _, pen = gradient_norm_loss(dev(y), dev(y_hat), net, alpha=torch.from_numpy(g["alpha"]), return_gradient=True)
    grads, _ = adversarial_input_grads(net, dev(y), dev(y_hat))
    for name, got in (("grad_pen", pen), ("grad_gen", grads["loss_gen"]), ("grad_fm", grads["loss_fm"])):
        a, b = got.cpu().numpy().astype(np.float64), g[name].astype(np.float64)
        assert np.isfinite(a).all() and a.shape == b.shape
        mx, l2 = rel_err(a, b), float(np.linalg.norm(a - b) / np.linalg.norm(b))
        print("end to end", name, "max-norm", mx, "relative L2", l2)
        record(f"B.end_to_end.{name}.max", mx, None)
        record(f"B.end_to_end.{name}.l2", l2, None)


# ------------------------------------------------------------------------------------------------- 6
def test_isolation_determinism_and_launch_count(nets):
    net, _ = nets["v2"]
    T, B, seed = SHAPES["B"]
    _, y_hat = S.disc_waves(B, T, seed)
    _, other = S.disc_waves(B, T, 777)
    fm = net.forward_single(dev(y_hat))
    before = [t.clone() for d in fm for t in d]
    cots = to_dev(random_cotangents(fm, 9))
    a, da = net.input_grad(fm, cots, return_deltas=True)
    b, db = net.input_grad(fm, cots, return_deltas=True)
    assert torch.equal(a, b) and all(torch.equal(p, q) for dp, dq in zip(da, db) for p, q in zip(dp, dq)), "two calls differ"
    assert all(torch.equal(p, q) for p, q in zip(before, [t for d in fm for t in d])), "the backward pass changed a feature map"
    again = net.forward_single(dev(y_hat))
    assert all(torch.equal(p, q) for p, q in zip(before, [t for d in again for t in d])), "the forward changed after a backward call"
    # other data in item 1 (signal and cotangents) leaves item 0's gradient bit-identical
    yh2 = y_hat.copy()
    yh2[1] = -2.0 * other[1]
    fm2 = net.forward_single(dev(yh2))
    cots2 = [[torch.cat([c[:1], 3.0 * c[1:]]) for c in d] for d in cots]
    c2 = net.input_grad(fm2, cots2)
    assert torch.equal(a[0], c2[0]) and not torch.equal(a[1], c2[1])
    for v, subs in (("v2", 9), ("v1", 7)):
        counts = [nets[v][0].backward_launch_count(S_, T_) for S_ in (1, 4) for T_ in (997, 12800)]
        print("backward launches", v, counts)
        assert len(set(counts)) == 1 and counts[0] == 7 + 6 * (subs - 1) == nets[v][0].launch_count(2, 997)


# ------------------------------------------------------------------------------------------------- 7
def test_evaluate_checkpoint_with_c_gp(tmp_path, nets):
    from comfy_rvc_amd.lib.train.evaluate import evaluate_checkpoint, load_generator
    from comfy_rvc_amd.lib.train.utils import HParams
    from conftest import golden
    from test_hip_train_forward import HPS_40K, hps
    e = golden("train_eval_cases.npz")
    filelist = S.write_train_filelist(str(tmp_path), feat_dim=768, spec_bins=1025)
    net_g = load_generator({"model": {k: torch.from_numpy(v) for k, v in S.synth_train_state_dict(S.CONFIG_40K_V2).items()}}, hps())
    net_d = nets["v2"][0]
    kw = dict(seed=int(e["walk_seed"]), batch_size=int(e["walk_batch_size"]), boundaries=[int(x) for x in e["walk_boundaries"]])
    hp = HParams(**{**HPS_40K, "train": {**HPS_40K["train"], "c_gp": 0.5}})
    with_gp = evaluate_checkpoint(net_g, filelist, hp, ckpt_d=net_d, **kw)
    again = evaluate_checkpoint(net_g, filelist, hp, ckpt_d=net_d, **kw)
    without = evaluate_checkpoint(net_g, filelist, hps(), ckpt_d=net_d, **kw)
    zero = evaluate_checkpoint(net_g, filelist, HParams(**{**HPS_40K, "train": {**HPS_40K["train"], "c_gp": 0.0}}), ckpt_d=net_d, **kw)
    assert set(without) == set(zero) == {"loss_mel", "loss_kl", "loss_disc", "loss_gen", "loss_fm", "batches"}
    assert set(with_gp) == set(without) | {"gradient_penalty"}
    assert all(set(r) == {"loss_mel", "loss_kl", "loss_disc", "loss_gen", "loss_fm", "ids_slice", "gradient_penalty"} for r in with_gp["batches"])
    gp = with_gp["gradient_penalty"]
    print("gradient_penalty", gp, [r["gradient_penalty"] for r in with_gp["batches"]])
    assert np.isfinite(gp) and gp > 0 and gp == float(np.mean([r["gradient_penalty"] for r in with_gp["batches"]])) and gp == again["gradient_penalty"]
    first = with_gp["batches"][0]                  # the first batch's other numbers do not move (alpha is drawn after the batch's own draws)
    assert all(first[k] == without["batches"][0][k] == zero["batches"][0][k] for k in ("loss_mel", "loss_kl", "loss_disc", "loss_gen", "loss_fm"))
    assert all(zero[k] == without[k] for k in ("loss_mel", "loss_kl", "loss_disc", "loss_gen", "loss_fm"))


# ------------------------------------------------------------------------------------------------- 8
def test_errors(nets):
    """CPU tensors, mismatched shapes, a NULL feature map and a T too short for period 37's pad each raise; nothing is launched (the output stays untouched)"""
    from comfy_rvc_amd import _lib
    from comfy_rvc_amd.lib.train.losses import gradient_norm_loss
    net, _ = nets["v2"]
    T, B, seed = SHAPES["A"]
    _, y_hat = S.disc_waves(B, T, seed)
    fm = net.forward_single(dev(y_hat))
    none = GR.none_like(fm)
    with pytest.raises(ValueError):
        net.input_grad([[t.cpu() for t in d] for d in fm], none)
    cpu_cot = GR.none_like(fm)
    cpu_cot[2][1] = torch.zeros(fm[2][1].shape)
    with pytest.raises(ValueError):
        net.input_grad(fm, cpu_cot)
    bad = GR.none_like(fm)
    bad[2][1] = torch.zeros(fm[2][1].shape, device=DEV)[..., :1]
    with pytest.raises(ValueError):
        net.input_grad(fm, bad)
    short = [list(d) for d in fm]
    short[4][3] = short[4][3][:, :, :0]
    with pytest.raises(ValueError):
        net.input_grad(short, none)
    with pytest.raises(ValueError):
        net.input_grad(fm[:-1], none[:-1])
    missing = [list(d) for d in fm]
    missing[1][0] = None
    with pytest.raises(ValueError):
        net.input_grad(missing, none)
    with pytest.raises(ValueError):
        gradient_norm_loss(torch.zeros(1, 1, 210), torch.zeros(1, 1, 210), net)
    with pytest.raises(ValueError):
        gradient_norm_loss(torch.zeros(1, 1, 210, device=DEV), torch.zeros(1, 1, 211, device=DEV), net)
    with pytest.raises(ValueError):
        gradient_norm_loss(torch.zeros(1, 1, 18, device=DEV), torch.zeros(1, 1, 18, device=DEV), net)          # period 37 would pad 19 >= 18 samples
    with pytest.raises(_lib.RvcHipError):
        net.backward_launch_count(1, 18)
    # the C entry itself: a NULL feature map, a NULL work buffer and a short T fail before anything is launched
    flat = [t for d in fm for t in d]
    n = len(flat)
    work = [torch.empty_like(t) for t in flat]
    out = torch.full((B, 1, T), SENTINEL, device=DEV)
    arr = lambda ts: (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])
    st = _lib.current_stream()
    for f, w, T_ in (([None] + flat[1:], work, T), (flat, work[:-1] + [None], T), (flat, work, 18)):
        assert _lib.lib.rvc_disc_input_grad(net._h, st, B, T_, arr(f), arr([None] * n), arr(w), _lib.ptr(out)) != 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
