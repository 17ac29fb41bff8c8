"""GPU: MultiPeriodDiscriminator / MultiPeriodDiscriminatorV2 on the device (rvc_disc_forward), the GAN losses' segmented reductions and the checkpoint
evaluation with a discriminator, against the reference's goldens (tools/gen_golden_discriminator.py) and the float64 restatement (tests/disc_ref.py).
Gate: conftest.rel_err < 1e-3, the project's fp32 gate.  Every measured error is kept by conftest.record_parity under "disc.*";
profiles/disc_parity.json is a copy of those entries."""
import numpy as np
import pytest
import torch

from conftest import golden, record_parity, rel_err
from comfy_rvc_amd import synthetic as S
import disc_ref as R
from test_disc_host import case_a, case_b, check_case_a, check_case_b

pytestmark = pytest.mark.gpu
GATE = 1e-3
DEV = "cuda:0"


def record(name, value, gate):
    record_parity(f"disc.{name}", {"measured": float(value), "gate": None if gate is None else float(gate)})


@pytest.fixture(scope="module")
def sd2():
    return S.disc_state_dict("v2", 0)


@pytest.fixture(scope="module")
def net2(sd2):
    from comfy_rvc_amd.lib.infer_pack.models import MultiPeriodDiscriminatorV2
    return MultiPeriodDiscriminatorV2(False, device=DEV).load_state_dict(sd2)


@pytest.fixture(scope="module")
def net1():
    from comfy_rvc_amd.lib.infer_pack.models import MultiPeriodDiscriminator
    return MultiPeriodDiscriminator(device=DEV).load_state_dict({k: torch.from_numpy(v) for k, v in S.disc_state_dict("v1", 0).items()})


@pytest.fixture(scope="module")
def ref_b(sd2):
    """case B through the restatement, computed once"""
    g, y, y_hat = case_b()
    return R.forward(sd2, "v2", y, y_hat)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def device_losses(res):
    from comfy_rvc_amd.lib.train.losses import discriminator_loss, feature_loss, generator_loss
    ld, per_d = discriminator_loss(res[0], res[1])
    lg, per_g = generator_loss(res[1])
    return {"loss_disc": ld, "loss_gen": lg, "loss_fm": feature_loss(res[2], res[3])}, per_d, per_g


def against_restatement(res, ref, tag):
    """every score and every feature map in full"""
    worst = 0.0
    for k, side in ((0, "r"), (1, "g")):
        for i, (a, b) in enumerate(zip(res[k], ref[k])):
            assert tuple(a.shape) == tuple(b.shape) and a.dtype == torch.float32
            e = rel_err(a.cpu().numpy(), b.numpy())
            record(f"{tag}.ref.d{i}.{side}.score", e, GATE)
            assert e < GATE, (tag, i, side, e)
            worst = max(worst, e)
        for i, (da, db) in enumerate(zip(res[2 + k], ref[2 + k])):
            assert len(da) == len(db)
            for l, (a, b) in enumerate(zip(da, db)):
                assert tuple(a.shape) == tuple(b.shape) and a.dtype == torch.float32
                e = rel_err(a.cpu().numpy(), b.numpy())
                record(f"{tag}.ref.d{i}.{side}.fmap{l}", e, GATE)
                assert e < GATE, (tag, i, side, l, e)
                worst = max(worst, e)
    print(tag, "largest error against the restatement", worst)
    return worst


# ------------------------------------------------------------------------------------------------- (a), (b)
@pytest.mark.parametrize("version", ["v2", "v1"])
def test_case_a_matches_reference_golden_and_restatement(version, net1, net2, sd2):
    m, y, y_hat = case_a()
    net = net2 if version == "v2" else net1
    res = net(dev(y), dev(y_hat))
    assert len(res[0]) == len(res[1]) == len(res[2]) == len(res[3]) == len(R.PERIODS[version]) + 1
    print("case A", version, "largest error against the golden", check_case_a(res, version, GATE, record, f32=True))
    against_restatement(res, R.forward(sd2 if version == "v2" else S.disc_state_dict("v1", 0), version, y, y_hat), f"A.{version}")


def test_case_b_matches_reference_golden_and_restatement(net2, ref_b):
    g, y, y_hat = case_b()
    res = net2(dev(y), dev(y_hat))
    print("case B largest error against the golden", check_case_b(res, g, GATE, record))
    against_restatement(res, ref_b, "B")


# ------------------------------------------------------------------------------------------------- (c)
def test_losses_match_reference(net2):
    g, y, y_hat = case_b()
    losses, per_d, per_g = device_losses(net2(dev(y), dev(y_hat)))
    assert len(per_d) == int(g["n_losses_disc"]) and len(per_g) == int(g["n_losses_gen"])
    for k, v in losses.items():
        assert v.dtype == torch.float32 and v.dim() == 0 and v.is_cuda
        d, tol = abs(float(v) - float(g[k])), float(g[k + "_tol"])
        print(k, float(v), "reference", float(g[k]), "delta", d, "tolerance", tol)
        record(f"B.{k}", d, tol)
        assert d <= tol
    assert abs(float(sum(per_d)) - float(losses["loss_disc"])) < 1e-4 and abs(float(sum(per_g)) - float(losses["loss_gen"])) < 1e-4


# ------------------------------------------------------------------------------------------------- (d)
def test_trainer_size_against_restatement(net2, sd2):
    """T = 12800 (the trainer's segment), B = 1: many column tiles of the GEMM per signal.  Scores at the gate.  Losses: a score within the gate is off by at
    most d = 1e-3 max|x|, which moves mean (c - x)^2 by at most 2 mean|c - x| d + d^2; a feature map within the gate moves mean |r - g| by at most
    1e-3 (max|r| + max|g|).  The tolerance of each loss is the sum of those bounds over its terms, computed from the restatement's tensors."""
    y, y_hat = S.disc_waves(1, 12800, 13)
    ref = R.forward(sd2, "v2", y, y_hat)
    res = net2(dev(y), dev(y_hat))
    for k, side in ((0, "r"), (1, "g")):
        for i, (a, b) in enumerate(zip(res[k], ref[k])):
            assert tuple(a.shape) == tuple(b.shape)
            e = rel_err(a.cpu().numpy(), b.numpy())
            print("T=12800 score", i, side, e)
            record(f"T12800.d{i}.{side}.score", e, GATE)
            assert e < GATE

    def sq_bound(x, c):
        d = GATE * float(x.abs().max())
        return 2 * float((c - x).abs().mean()) * d + d * d
    tol = {"loss_disc": sum(sq_bound(r, 1.0) + sq_bound(g, 0.0) for r, g in zip(ref[0], ref[1])),
           "loss_gen": sum(sq_bound(g, 1.0) for g in ref[1]),
           "loss_fm": sum(GATE * (float(r.abs().max()) + float(g.abs().max())) for dr, dg in zip(ref[2], ref[3]) for r, g in zip(dr, dg))}
    want = R.losses(ref)
    got, _, _ = device_losses(res)
    for k in want:
        d = abs(float(got[k]) - want[k])
        print("T=12800", k, float(got[k]), "restatement", want[k], "delta", d, "tolerance", tol[k])
        record(f"T12800.{k}", d, tol[k])
        assert d <= tol[k]


# ------------------------------------------------------------------------------------------------- (e)
def flat(res):
    return [t for t in res[0]] + [t for t in res[1]] + [t for d in res[2] for t in d] + [t for d in res[3] for t in d]


def test_items_and_halves_are_isolated(net2):
    """No tap of one signal reads another signal's rows: other data in item 1 of y and y_hat leaves every output of item 0 bit-identical; other data in all of
    y_hat leaves the real half bit-identical, and other data in all of y the generated half."""
    g, y, y_hat = case_b()
    oy, oy_hat = S.disc_waves(2, int(g["T"]), 777)
    base = net2(dev(y), dev(y_hat))
    y2, yh2 = y.copy(), y_hat.copy()
    y2[1], yh2[1] = 3.0 * oy[1], -2.0 * oy_hat[1]
    other = net2(dev(y2), dev(yh2))
    for a, b in zip(flat(base), flat(other)):
        assert torch.equal(a[0], b[0])
        assert not torch.equal(a[1], b[1])
    gen_changed = net2(dev(y), dev(5.0 * oy_hat))
    real_changed = net2(dev(-4.0 * oy), dev(y_hat))
    for a, b in zip(base[0] + [t for d in base[2] for t in d], gen_changed[0] + [t for d in gen_changed[2] for t in d]):
        assert torch.equal(a, b)
    for a, b in zip(base[1] + [t for d in base[3] for t in d], real_changed[1] + [t for d in real_changed[3] for t in d]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- (f)
def test_two_calls_give_the_same_bits(net2):
    g, y, y_hat = case_b()
    a, b = net2(dev(y), dev(y_hat)), net2(dev(y), dev(y_hat))
    assert all(torch.equal(p, q) for p, q in zip(flat(a), flat(b)))
    la, lb = device_losses(a), device_losses(b)
    assert all(torch.equal(la[0][k], lb[0][k]) for k in la[0])
    assert all(torch.equal(p, q) for p, q in zip(la[1] + la[2], lb[1] + lb[2]))


@pytest.mark.parametrize("n", [1, 63, 1000, 300001])
def test_segmented_reductions(n):
    """rvc_sqerr_sums / rvc_l1_sums on segments of unequal lengths against float64 numpy; two calls give the same bits"""
    from comfy_rvc_amd.lib.train import losses as L
    rng = np.random.default_rng(n)
    lens = [n, 1, 7 * n + 3, 257]
    a = [rng.standard_normal(m).astype(np.float32) for m in lens]
    b = [rng.standard_normal(m).astype(np.float32) for m in lens]
    got = [L._sqerr_means([dev(x) for x in a], [1.0, 0.0, 1.0, 0.5]) for _ in range(2)]
    assert torch.equal(got[0], got[1])
    want = [np.mean((np.float32(c) - x).astype(np.float64) ** 2) for x, c in zip(a, (1.0, 0.0, 1.0, 0.5))]
    assert np.allclose(got[0].cpu().numpy(), want, rtol=1e-12, atol=0)
    fm = [L.feature_loss([[dev(x) for x in a[:2]], [dev(x) for x in a[2:]]], [[dev(x) for x in b[:2]], [dev(x) for x in b[2:]]]) for _ in range(2)]
    assert torch.equal(fm[0], fm[1])
    want = sum(np.mean(np.abs((x - z).astype(np.float64))) for x, z in zip(a, b))
    assert abs(float(fm[0]) - want) <= 2.0 ** -22 * want


# ------------------------------------------------------------------------------------------------- (g)
def test_launch_count(net1, net2):
    for net, budget, subs in ((net2, 63, 9), (net1, 49, 7)):
        counts = [net.launch_count(S_, T) for S_ in (2, 8) for T in (997, 12800)]
        print("launches", counts)
        assert len(set(counts)) == 1 and counts[0] <= budget and counts[0] <= 7 * subs
        assert counts[0] == 7 + 6 * (subs - 1)


# ------------------------------------------------------------------------------------------------- (h)
def test_evaluate_checkpoint_with_a_discriminator(tmp_path, sd2):
    from comfy_rvc_amd.lib.train import data_utils
    from comfy_rvc_amd.lib.train.evaluate import adversarial_losses, evaluate_checkpoint, load_discriminator, load_generator, reconstruction_losses
    from test_hip_train_forward import hps
    e = golden("train_eval_cases.npz")
    filelist = S.write_train_filelist(str(tmp_path), feat_dim=768, spec_bins=1025)
    net_g = load_generator({"model": {k: torch.from_numpy(v) for k, v in S.synth_train_state_dict(S.CONFIG_40K_V2).items()}}, hps())
    ckpt_d = str(tmp_path / "D_0.pth")
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd2.items()}, "iteration": 0, "learning_rate": 1e-4}, ckpt_d)
    net_d = load_discriminator(ckpt_d, "v2")
    kw = dict(seed=int(e["walk_seed"]), batch_size=int(e["walk_batch_size"]), boundaries=[int(x) for x in e["walk_boundaries"]])
    with_d = evaluate_checkpoint(net_g, filelist, hps(), ckpt_d=net_d, **kw)
    without = evaluate_checkpoint(net_g, filelist, hps(), **kw)
    assert set(without) == {"loss_mel", "loss_kl", "batches"} and all(set(r) == {"loss_mel", "loss_kl", "ids_slice"} for r in without["batches"])
    assert set(with_d) == {"loss_mel", "loss_kl", "loss_disc", "loss_gen", "loss_fm", "batches"}
    for k in ("loss_mel", "loss_kl"):
        assert with_d[k] == without[k] and abs(without[k] - float(e[f"walk_{k}"])) <= float(e[f"walk_{k}_tol"])
    assert len(with_d["batches"]) == len(without["batches"]) == 2
    for k in ("loss_disc", "loss_gen", "loss_fm"):
        assert np.isfinite(with_d[k]) and with_d[k] > 0 and with_d[k] == float(np.mean([r[k] for r in with_d["batches"]]))
    # the first batch again, piece by piece: the three numbers are the restatement's on the same waves, the real ones sliced at ids_slice * hop_length
    ds = data_utils.TextAudioLoaderMultiNSFsid(filelist, hps().data)
    idx = next(iter(data_utils.BucketSampler(ds, kw["batch_size"], kw["boundaries"], shuffle=False)))
    batch = data_utils.TextAudioCollateMultiNSFsid()([ds[i] for i in idx])
    r = reconstruction_losses(net_g, batch, hps(), torch.Generator().manual_seed(kw["seed"]), return_y_hat=True)
    adv = adversarial_losses(net_d, batch[6], r["y_hat"], r["ids_slice"], hps())
    ids = r["ids_slice"].cpu().numpy()
    assert np.array_equal(ids, with_d["batches"][0]["ids_slice"])
    wave = np.stack([batch[6][i, :, int(s) * 400:int(s) * 400 + 12800].numpy() for i, s in enumerate(ids)])
    want = R.losses(R.forward(sd2, "v2", wave, r["y_hat"].cpu().numpy()))
    for k in want:
        assert float(adv[k]) == with_d["batches"][0][k]
        d = abs(float(adv[k]) - want[k]) / want[k]
        print("evaluate", k, float(adv[k]), "restatement", want[k], "relative", d)
        record(f"evaluate.batch0.{k}", d, GATE)
        assert d < GATE


# ------------------------------------------------------------------------------------------------- (i)
def test_errors(net1, net2):
    from comfy_rvc_amd import _lib
    from comfy_rvc_amd.lib.infer_pack.models import MultiPeriodDiscriminatorV2
    with pytest.raises(NotImplementedError):
        MultiPeriodDiscriminatorV2(use_spectral_norm=True)
    for net, T in ((net2, 10), (net2, 18), (net1, 8)):          # the pad of the largest period (27, 19, 9 samples) is not shorter than the signal
        with pytest.raises(ValueError):
            net(torch.zeros(1, 1, T, device=DEV), torch.zeros(1, 1, T, device=DEV))
        with pytest.raises(_lib.RvcHipError):
            net.launch_count(2, T)
    net2(torch.zeros(1, 1, 19, device=DEV), torch.zeros(1, 1, 19, device=DEV))      # pad 18 < 19: the shortest signal V2 takes
    with pytest.raises(ValueError):
        net2(torch.zeros(2, 1, 210, device=DEV), torch.zeros(2, 1, 211, device=DEV))
    with pytest.raises(ValueError):
        net2(torch.zeros(2, 1, 210, device=DEV), torch.zeros(1, 1, 210, device=DEV))
    with pytest.raises(ValueError):
        net2(torch.zeros(1, 210, device=DEV), torch.zeros(1, 210, device=DEV))
    with pytest.raises(ValueError):
        net2(torch.zeros(1, 1, 210), torch.zeros(1, 1, 210))
    with pytest.raises(ValueError):
        net2(torch.zeros(1, 1, 210, device=DEV), torch.zeros(1, 1, 210))
    from comfy_rvc_amd.lib.train.losses import feature_loss, generator_loss
    with pytest.raises(ValueError):
        generator_loss([torch.zeros(3)])
    with pytest.raises(ValueError):
        feature_loss([[torch.zeros(3, device=DEV)]], [[torch.zeros(4, device=DEV)]])
    # a state dict with spectral-norm tensors, or one that misses a tensor, does not finalize
    from comfy_rvc_amd.lib.infer_pack.models import MultiPeriodDiscriminator
    bad = {k: v for k, v in S.disc_state_dict("v1", 0).items() if not k.startswith("discriminators.6.conv_post")}
    with pytest.raises(_lib.RvcHipError):
        MultiPeriodDiscriminator(device=DEV).load_state_dict(bad)
