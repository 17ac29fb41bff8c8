"""GPU: SynthesizerTrnMs{256,768}NSFsid[_nono].forward on the device (rvc_synth_forward), the two loss reductions and the checkpoint evaluation, against
the reference's goldens (tools/gen_golden_train_forward.py) and the CPU restatement (tests/train_forward_ref.py).  Gate: conftest.rel_err < 1e-3, the
gate of test_hip_models.py.  Every measured error is kept by conftest.record_parity; profiles/train_forward_parity.json is a copy of those entries."""
import numpy as np
import pytest
import torch

from conftest import golden, record_parity, rel_err
from comfy_rvc_amd import synthetic as S
import train_forward_ref as R
from test_train_forward_host import CASES, TAPS, case_inputs

pytestmark = pytest.mark.gpu
GATE = 1e-3
HPS_40K = dict(data=dict(filter_length=2048, hop_length=400, win_length=2048, n_mel_channels=125, sampling_rate=40000, mel_fmin=0.0, mel_fmax=None,
                         max_wav_value=32768.0),
               train=dict(segment_size=12800),
               model=dict(inter_channels=192, hidden_channels=192, filter_channels=768, n_heads=2, n_layers=6, kernel_size=3, p_dropout=0, resblock="1",
                          resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, upsample_rates=[10, 10, 2, 2],
                          upsample_initial_channel=512, upsample_kernel_sizes=[16, 16, 4, 4], spk_embed_dim=109, gin_channels=256))


def record(name, value, gate):
    """Keeps a measured error next to its gate through the suite's parity record (conftest.record_parity), under "train_forward.<name>"."""
    record_parity(f"train_forward.{name}", {"measured": float(value), "gate": None if gate is None else float(gate)})


def make_net(tag, train=True, delete_enc_q=False):
    from comfy_rvc_amd.lib.infer_pack import models
    config, version, f0 = CASES[tag]
    cls = getattr(models, f"SynthesizerTrnMs{768 if version == 'v2' else 256}NSFsid" + ("" if f0 else "_nono"))
    net = cls(*config, is_half=False) if f0 else cls(*config)
    if delete_enc_q:
        del net.enc_q
    seed = int(golden(f"train_forward_{tag}.npz")["weight_seed"])
    net.load_state_dict(S.synth_train_state_dict(config, version, seed, f0=f0) if train else S.synth_state_dict(config, version, seed, f0=f0))
    return net


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = make_net(tag)
        return cache[tag]
    return get


def call(net, f0, b, noise=None, ids=None):
    t = {k: (None if v is None else torch.from_numpy(np.asarray(v))) for k, v in b.items()}
    if f0:
        return net(t["phone"], t["lengths"], t["pitch"], t["pitchf"], t["spec"], t["lengths"], t["sid"], noise=noise, ids_slice=ids)
    return net(t["phone"], t["lengths"], t["spec"], t["lengths"], t["sid"], noise=noise, ids_slice=ids)


def check_against(tag, name, res, want, lengths, ids):
    o, ids_out, x_mask, y_mask, taps = res
    T = int(max(lengths))
    assert np.array_equal(ids_out.cpu().numpy(), np.asarray(ids)) and ids_out.dtype == torch.int64
    mask = (np.arange(T)[None, :] < np.asarray(lengths)[:, None]).astype(np.float32)[:, None, :]
    assert tuple(x_mask.shape) == tuple(y_mask.shape) == (len(lengths), 1, T)
    assert np.array_equal(x_mask.cpu().numpy(), mask) and np.array_equal(y_mask.cpu().numpy(), mask)
    for b, L in enumerate(lengths):
        for k, t in zip(TAPS, taps):
            got = t[b].cpu().numpy()
            e = rel_err(got[:, :L], want[k][b][:, :L])
            print(name, "item", b, k, e)
            record(f"{name}.item{b}.{k}", e, GATE)
            assert e < GATE, (name, b, k, e)
            assert not np.any(got[:, L:]), (name, b, k, "nonzero beyond the length")
        e = rel_err(o[b].cpu().numpy(), want["o"][b])
        print(name, "item", b, "o", e)
        record(f"{name}.item{b}.o", e, GATE)
        assert e < GATE, (name, b, "o", e)


@pytest.mark.parametrize("tag", list(CASES))
def test_forward_matches_reference_golden(tag, nets):
    config, sd, b, noise_q, noise_src, g = case_inputs(tag)
    f0 = CASES[tag][2]
    res = call(nets(tag), f0, b, noise=(noise_q, noise_src) if f0 else noise_q, ids=torch.from_numpy(g["ids_slice"]))
    assert tuple(res[0].shape) == tuple(g["o"].shape)
    check_against(tag, f"golden_{tag}", res, g, [int(x) for x in g["lengths"]], g["ids_slice"])


def test_plain_fp32_graph_forward_and_losses_match_reference_golden():
    """The training forward built at rvc_set_conv_precision(0) (the plain fp32 graph: no split-resident branch of synth_forward is taken): taps and wave against
    train_forward_40k_v2 at the gate above, both losses against the reference's values within the tolerances stored in the golden."""
    from comfy_rvc_amd import _lib as L
    from comfy_rvc_amd.lib.train.evaluate import reconstruction_losses
    L.check(L.lib.rvc_set_conv_precision(0))
    try:
        net = make_net("40k_v2")
    finally:
        L.check(L.lib.rvc_set_conv_precision(1))
    config, sd, b, noise_q, noise_src, g = case_inputs("40k_v2")
    res = call(net, True, b, noise=(noise_q, noise_src), ids=torch.from_numpy(g["ids_slice"]))
    assert tuple(res[0].shape) == tuple(g["o"].shape)
    check_against("40k_v2", "plain_fp32_40k_v2", res, g, [int(x) for x in g["lengths"]], g["ids_slice"])
    e = golden("train_eval_cases.npz")
    t = {k: torch.from_numpy(np.asarray(v)) for k, v in b.items()}
    batch = (t["phone"], t["lengths"], t["pitch"], t["pitchf"], t["spec"], t["lengths"], None, None, t["sid"])
    r = reconstruction_losses(net, batch, hps(), None, noise=(noise_q, noise_src), ids_slice=torch.from_numpy(g["ids_slice"]))
    for k in ("loss_mel", "loss_kl"):
        d, tol = abs(float(r[k]) - float(e[f"batch_{k}"])), float(e[f"{k}_tol"])
        print("plain fp32", k, float(r[k]), "reference", float(e[f"batch_{k}"]), "delta", d, "tolerance", tol)
        record(f"plain_fp32_batch.{k}", d, tol)
    for k in ("loss_mel", "loss_kl"):
        assert abs(float(r[k]) - float(e[f"batch_{k}"])) <= float(e[f"{k}_tol"]), k


def test_forward_fresh_seeds_against_restatement(nets):
    """Lengths 47 / 32 and starts 13 / 0: shapes the golden does not hold."""
    config, version, f0 = CASES["40k_v2"]
    lengths, ids = [47, 32], np.array([13, 0], dtype=np.int64)
    b = S.synth_train_batch(config, version, lengths, seed=77)
    gen = torch.Generator().manual_seed(99)
    noise_q, noise_src = torch.randn(2, 192, 47, generator=gen), torch.randn(2, 32 * 400, 1, generator=gen)
    sd = S.synth_train_state_dict(config, version, int(golden("train_forward_40k_v2.npz")["weight_seed"]))
    want = R.forward(sd, config, b["phone"], b["lengths"], b["pitch"], b["pitchf"], b["spec"], b["sid"], noise_q, noise_src, ids)
    res = call(nets("40k_v2"), True, b, noise=(noise_q, noise_src), ids=torch.from_numpy(ids))
    check_against("40k_v2", "fresh_40k_v2", res, want, lengths, ids)


def test_slice_is_a_sequence_of_its_own(nets):
    """o of item 0 is the generator run on z[:, 7:39] and pitchf[7:39] as a 32-frame sequence (zero padding at both cut edges, the source's phase starting at
    the slice): the CPU generator on the DEVICE's own z tap reproduces it; the generator run on the whole item and cut to the same frames does not."""
    config, sd, b, noise_q, noise_src, g = case_inputs("40k_v2")
    res = call(nets("40k_v2"), True, b, noise=(noise_q, noise_src), ids=torch.from_numpy(g["ids_slice"]))
    from oracle import nets as N
    tsd = N.tensors(sd)
    L, start, seg, upp = int(g["lengths"][0]), int(g["ids_slice"][0]), config[1], 400
    z = res[4][0][0:1, :, :L].cpu()
    gv = tsd["emb_g.weight"][int(b["sid"][0])].view(1, -1, 1)
    pf = torch.from_numpy(b["pitchf"][0:1, :L])
    with torch.no_grad():
        own = R.generator_slice(tsd, config, z, pf, gv, noise_src[0:1], start).numpy()
        pad = torch.zeros(1, L * upp, 1)
        pad[:, start * upp:(start + seg) * upp] = noise_src[0:1]
        whole = N.generator_forward(tsd, config, z, pf, gv, pad).numpy()[:, :, start * upp:(start + seg) * upp]
    o = res[0][0:1].cpu().numpy()
    e_own, e_whole = rel_err(o, own), rel_err(o, whole)
    print("slice as its own sequence", e_own, "cut from the whole item", e_whole)
    record("slice_own_sequence.o", e_own, GATE)
    assert e_own < GATE
    assert e_whole > 10 * GATE


def test_default_draws_follow_the_reference_order(nets):
    config, version, f0 = CASES["40k_v2"]
    lengths = [41, 33, 32]
    b = S.synth_train_batch(config, version, lengths, seed=5)
    torch.manual_seed(321)
    res = call(nets("40k_v2"), True, b)
    torch.manual_seed(321)
    noise_q = torch.randn(3, 192, 41)
    ids = R.slice_starts(torch.rand([3]), lengths, 32)
    torch.rand(3, 1)
    noise_src = torch.randn(3, 32 * 400, 1)
    res2 = call(nets("40k_v2"), True, b, noise=(noise_q, noise_src), ids=ids)
    assert torch.equal(res[1].cpu(), ids)
    assert torch.equal(res[0], res2[0]) and all(torch.equal(a, c) for a, c in zip(res[4], res2[4]))
    # the no-f0 family: one randn_like, then the slice's rand
    bn = S.synth_train_batch(config, version, [40, 35], seed=7, f0=False)
    torch.manual_seed(11)
    rn = call(nets("40k_v2_nono"), False, bn)
    torch.manual_seed(11)
    nq = torch.randn(2, 192, 40)
    idn = R.slice_starts(torch.rand([2]), [40, 35], 32)
    rn2 = call(nets("40k_v2_nono"), False, bn, noise=nq, ids=idn)
    assert torch.equal(rn[1].cpu(), idn) and torch.equal(rn[0], rn2[0])


@pytest.mark.parametrize("C_,T,L", [(192, 41, 41), (192, 47, 33), (7, 1100, 1031), (3, 5, 1)])
def test_kl_loss_reduction(C_, T, L):
    from comfy_rvc_amd import _lib
    rng = np.random.default_rng(C_ * 1000 + T)
    z_p, m_p = (rng.standard_normal((C_, T)).astype(np.float32) * 2 for _ in range(2))
    logs_q, logs_p = (rng.uniform(-2.5, 2.5, (C_, T)).astype(np.float32) for _ in range(2))
    dev = [torch.from_numpy(a).cuda() for a in (z_p, logs_q, m_p, logs_p)]
    outs = []
    for _ in range(2):
        out = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
        _lib.check(_lib.lib.rvc_kl_loss(_lib.current_stream(), *[_lib.ptr(t) for t in dev], C_, T, L, _lib.ptr(out)))
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    a = [x[:, :L].astype(np.float64) for x in (z_p, logs_q, m_p, logs_p)]
    term = a[3] - a[1] - 0.5 + 0.5 * (a[0] - a[2]) ** 2 * np.exp(-2.0 * a[3])
    gate = 1e-5 * float(np.mean(np.abs(term)))
    d = abs(outs[0][0] / term.size - float(np.mean(term)))
    print("kl", C_, T, L, d, gate)
    record(f"kl_loss.{C_}x{T}_len{L}", d, gate)
    assert outs[0][1] == L and d <= gate


@pytest.mark.parametrize("n", [1, 63, 1000, 125 * 32 * 3 + 5])
def test_l1_sum_reduction(n):
    from comfy_rvc_amd import _lib
    rng = np.random.default_rng(n)
    a, b = (rng.standard_normal(n).astype(np.float32) * 3 for _ in range(2))
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    outs = []
    for _ in range(2):
        out = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
        _lib.check(_lib.lib.rvc_l1_sum(_lib.current_stream(), _lib.ptr(da), _lib.ptr(db), n, _lib.ptr(out)))
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    term = np.abs(a.astype(np.float64) - b.astype(np.float64))
    gate = 1e-5 * float(np.mean(term))
    d = abs(outs[0][0] / n - float(np.mean(term)))
    print("l1", n, d, gate)
    record(f"l1_sum.{n}", d, gate)
    assert d <= gate


def hps():
    from comfy_rvc_amd.lib.train.utils import HParams
    return HParams(**HPS_40K)


def test_reconstruction_losses_on_the_golden_batch(nets):
    from comfy_rvc_amd.lib.train.evaluate import reconstruction_losses
    config, sd, b, noise_q, noise_src, g = case_inputs("40k_v2")
    e = golden("train_eval_cases.npz")
    t = {k: torch.from_numpy(np.asarray(v)) for k, v in b.items()}
    batch = (t["phone"], t["lengths"], t["pitch"], t["pitchf"], t["spec"], t["lengths"], None, None, t["sid"])
    r = reconstruction_losses(nets("40k_v2"), batch, hps(), None, noise=(noise_q, noise_src), ids_slice=torch.from_numpy(g["ids_slice"]))
    assert r["loss_mel"].dim() == 0 and r["loss_mel"].dtype == torch.float32 and r["loss_kl"].dim() == 0 and r["loss_mel"].is_cuda
    for k in ("loss_mel", "loss_kl"):
        d, tol = abs(float(r[k]) - float(e[f"batch_{k}"])), float(e[f"{k}_tol"])
        print(k, float(r[k]), "reference", float(e[f"batch_{k}"]), "delta", d, "tolerance", tol)
        record(f"golden_batch.{k}", d, tol)
    for k in ("loss_mel", "loss_kl"):
        assert abs(float(r[k]) - float(e[f"batch_{k}"])) <= float(e[f"{k}_tol"]), k
    # draws from a generator: the same seed gives the same bits, another seed another slice
    runs = [reconstruction_losses(nets("40k_v2"), batch, hps(), torch.Generator().manual_seed(s)) for s in (1337, 1337, 4)]
    assert torch.equal(runs[0]["loss_mel"], runs[1]["loss_mel"]) and torch.equal(runs[0]["loss_kl"], runs[1]["loss_kl"])
    assert torch.equal(runs[0]["ids_slice"], runs[1]["ids_slice"]) and not torch.equal(runs[0]["ids_slice"], runs[2]["ids_slice"])


def test_evaluate_checkpoint_on_the_synthetic_filelist(tmp_path):
    """The unshuffled two-batch walk the reference's loader, collate and sampler make of the synthetic file list: per-batch and mean losses within the stored
    tolerances of the reference's values, the slice starts equal."""
    from comfy_rvc_amd.lib.train.evaluate import evaluate_checkpoint
    e = golden("train_eval_cases.npz")
    filelist = S.write_train_filelist(str(tmp_path), feat_dim=768, spec_bins=1025)
    ckpt = str(tmp_path / "G_0.pth")
    torch.save({"model": {k: torch.from_numpy(v) for k, v in S.synth_train_state_dict(S.CONFIG_40K_V2).items()}, "iteration": 0, "learning_rate": 1e-4},
               ckpt)
    kw = dict(batch_size=int(e["walk_batch_size"]), boundaries=[int(x) for x in e["walk_boundaries"]])
    runs = [evaluate_checkpoint(ckpt, filelist, hps(), seed=s, **kw) for s in (int(e["walk_seed"]), int(e["walk_seed"]), 4)]
    r = runs[0]
    assert len(r["batches"]) == len(e["walk_batches"]) == 2
    for k in ("loss_mel", "loss_kl"):
        d, tol = abs(r[k] - float(e[f"walk_{k}"])), float(e[f"walk_{k}_tol"])
        print("walk", k, r[k], "reference", float(e[f"walk_{k}"]), "delta", d, "tolerance", tol)
        record(f"evaluate_checkpoint.{k}", d, tol)
        for i, row in enumerate(r["batches"]):
            db, tolb = abs(row[k] - float(e[f"walk_batch_{k}"][i])), float(e[f"walk_batch_{k}_tol"])
            print("walk batch", i, k, row[k], "delta", db, "tolerance", tolb)
            record(f"evaluate_checkpoint.batch{i}.{k}", db, tolb)
    for i, row in enumerate(r["batches"]):
        assert np.array_equal(row["ids_slice"], e["walk_ids_slice"][i])
    for k in ("loss_mel", "loss_kl"):
        assert abs(r[k] - float(e[f"walk_{k}"])) <= float(e[f"walk_{k}_tol"]), k
        for i, row in enumerate(r["batches"]):
            assert abs(row[k] - float(e[f"walk_batch_{k}"][i])) <= float(e[f"walk_batch_{k}_tol"]), (k, i)
    assert runs[0]["loss_mel"] == runs[1]["loss_mel"] and runs[0]["loss_kl"] == runs[1]["loss_kl"]
    assert any(not np.array_equal(a["ids_slice"], c["ids_slice"]) for a, c in zip(runs[0]["batches"], runs[2]["batches"]))


def test_errors(nets):
    from comfy_rvc_amd import _lib
    config, version, f0 = CASES["40k_v2"]
    b = S.synth_train_batch(config, version, [41, 33, 32], seed=5)
    for net in (make_net("40k_v2", train=False), make_net("40k_v2", delete_enc_q=True)):      # an inference state dict; `del net.enc_q` before loading
        assert not _lib.lib.rvc_synth_has_posterior(net._h)
        with pytest.raises(RuntimeError):
            call(net, True, b)
    net = nets("40k_v2")
    assert _lib.lib.rvc_synth_has_posterior(net._h)
    short = S.synth_train_batch(config, version, [41, 31], seed=5)
    with pytest.raises(ValueError):
        call(net, True, short)
    with pytest.raises(_lib.RvcHipError, match="slice start"):
        call(net, True, b, ids=torch.tensor([7, 2, 0]))                  # 33 frames leave the starts 0 and 1
    with pytest.raises(_lib.RvcHipError, match="slice start"):
        call(net, True, b, ids=torch.tensor([-1, 0, 0]))
    t = {k: torch.from_numpy(np.asarray(v)) for k, v in b.items()}
    with pytest.raises(ValueError):
        net(t["phone"], t["lengths"], t["pitch"], t["pitchf"], t["spec"], t["lengths"] - 1, t["sid"])
    nono = nets("40k_v2_nono")
    with pytest.raises(ValueError):
        nono(t["phone"], t["lengths"], t["pitch"], t["pitchf"], t["spec"], t["lengths"], t["sid"])
    from comfy_rvc_amd.lib.infer_pack import models
    cfg_do = list(config)
    cfg_do[8] = 0.1                                                     # p_dropout: only the dropout-free arithmetic exists
    net_do = models.SynthesizerTrnMs768NSFsid(*cfg_do, is_half=False)
    net_do.load_state_dict(S.synth_train_state_dict(config, version, 0))
    with pytest.raises(ValueError, match="p_dropout"):
        call(net_do, True, b)
    # the C entry point itself: T below the segment, pitch arguments to a no-f0 model
    x = torch.zeros(1025 * 64, device="cuda")
    out = torch.zeros(12800, device="cuda")
    st = _lib.current_stream()
    assert _lib.lib.rvc_synth_forward(net._h, st, _lib.ptr(x), 0, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), 0, _lib.ptr(x), _lib.ptr(x), 31, 0, _lib.ptr(out),
                                      None) != 0
    assert b"segment" in _lib.lib.rvc_last_error()
    assert _lib.lib.rvc_synth_forward(nono._h, st, _lib.ptr(x), 0, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), 0, _lib.ptr(x), _lib.ptr(x), 40, 0, _lib.ptr(out),
                                      None) != 0
    assert b"no-f0" in _lib.lib.rvc_last_error()
    # the model is intact afterwards
    res = call(net, True, b, ids=torch.tensor([7, 1, 0]))
    assert torch.isfinite(res[0]).all()
