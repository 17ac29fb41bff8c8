"""GPU: the generator loss's cotangents on the device - rvc_mel_spectrogram_vjp (mel_processing.mel_vjp_packed / mel_spectrogram_vjp), rvc_mel_loss_cotangents,
rvc_kl_loss_grad, losses.mel_loss_grad, MultiScaleMelSpectrogramLoss.forward_and_grad, LossBalancer's device norms and train_step.generator_loss_cotangents -
against the float64 restatement (tests/gen_cotangent_ref.py) and the reference's goldens (tools/gen_golden_gen_cotangent.py).

Gate of every gradient through the STFT: max |device - float64| / max |float64| <= 8 x the same figure of torch's float32 CPU autograd on the same input and
cotangent (the project's STFT rule; both figures are measured here and printed).  Where a loss decides the cotangent's sign, the float64 restatement is
given the cotangent formed from the DEVICE'S OWN log-mels, so a sign that rounding flipped does not enter (the discriminator tests' rule).  Element-wise
kernels: 4 u |value| with u = 2^-24.  With GEN_COT_PARITY_DUMP=<file.json> every figure is also written there (profiles/gen_cotangent_parity.json)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden
from comfy_rvc_amd import synthetic as S
import aux_loss_ref as R
import gen_cotangent_ref as G
from test_gen_cotangent_host import AUX, MSML, case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
GATE = 8.0
SR = 40000
N_MELS = {256: 20, 512: 40, 1024: 80, 2048: 125, 4096: 256}
GEOMETRIES = [(256, 400), (512, 400), (1024, 320), (2048, 400), (2048, 480), (4096, 400)]


def dump(key, value):
    print(key, value)
    path = os.environ.get("GEN_COT_PARITY_DUMP")
    if not path:
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        data = json.load(open(path)) if os.path.isfile(path) else {}
        data[key] = value
        with open(path, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
    except OSError:
        pass


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def peak_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def vjp_device(clips, cots, n_fft, hop, n_mels, eps=0.0, clamp=False, sr=SR):
    """clips: 1-D float32 arrays, cots: [n_mels, frames] float32 arrays -> the device gradients per clip (one call; every clip's columns start at a multiple of 16).
    The audio buffer is NaN-filled between and behind the clips: the call must leave that alone."""
    from comfy_rvc_amd.lib.train import mel_processing as MP
    gap = 7
    table, off, col = [], gap, 0
    for c in clips:
        table.append((off, len(c), col))
        off += len(c) + gap
        col += -(-(len(c) // hop) // 16) * 16 + 16
    audio = np.full(off, np.nan, dtype=np.float32)
    cot = np.full((n_mels, col), np.nan, dtype=np.float32)
    for (o, n, cl), c, ct in zip(table, clips, cots):
        audio[o:o + n] = c
        cot[:, cl:cl + n // hop] = ct
    out = torch.full((off,), 777.0, device=DEV)
    a, ct = dev(audio), dev(cot)
    MP.mel_vjp_packed(a, np.array(table, dtype=np.int64), ct, n_fft, hop, eps, clamp, n_mels, sr, 0.0, None, out=out)
    again = torch.full((off,), 555.0, device=DEV)
    MP.mel_vjp_packed(a, np.array(table, dtype=np.int64), ct, n_fft, hop, eps, clamp, n_mels, sr, 0.0, None, out=again)
    out, again = out.cpu().numpy(), again.cpu().numpy()
    inside = np.zeros(off, dtype=bool)
    for o, n, _ in table:
        inside[o:o + n] = True
    assert (out[~inside] == 777.0).all() and (again[~inside] == 555.0).all(), "a sample outside every clip was written"
    assert np.array_equal(out[inside], again[inside]), "two calls differ"
    assert np.isfinite(out[inside]).all()
    return [out[o:o + n] for o, n, _ in table]


def vjp_ref(clip, cot, n_fft, hop, n_mels, dtype, eps=0.0, clamp=False, sr=SR):
    return G.vjp(clip[None], cot[None], n_fft, n_mels, sr, hop, 0.0, None, dtype=dtype, eps=eps, clamp=clamp)[0].numpy()


def gated(tag, got, f64, f32):
    e, base = peak_err(got, f64), peak_err(f32, f64)
    dump(tag, {"device": e, "torch_float32": base, "gate": GATE * base})
    assert e <= GATE * base, (tag, e, base)


# ------------------------------------------------------------------------------------------------- 1: the vector-Jacobian product, given cotangent
@pytest.mark.parametrize("n_fft,hop", GEOMETRIES)
def test_vjp_matches_float64_with_a_given_cotangent(n_fft, hop):
    """two clips in one call: 19 frames + 5 samples (no multiple of 16, 8 or 4 frames, several workgroups) and 7 frames + 3 samples"""
    n_mels, sr = N_MELS[n_fft], (32000 if hop == 320 else SR)
    rng = np.random.default_rng(n_fft + hop)
    clips = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in (19 * hop + 5, 7 * hop + 3)]
    cots = [rng.standard_normal((n_mels, len(c) // hop)).astype(np.float32) for c in clips]
    got = vjp_device(clips, cots, n_fft, hop, n_mels, sr=sr)
    f64 = [vjp_ref(c, ct, n_fft, hop, n_mels, torch.float64, sr=sr) for c, ct in zip(clips, cots)]
    f32 = [vjp_ref(c, ct, n_fft, hop, n_mels, torch.float32, sr=sr) for c, ct in zip(clips, cots)]
    gated(f"vjp.{n_fft}_{hop}", np.concatenate(got), np.concatenate(f64), np.concatenate(f32))
    from comfy_rvc_amd import _lib
    assert _lib.lib.rvc_mel_spectrogram_vjp_launch_count() == 2


def test_vjp_with_epsilon_and_clamp_matches_float64():
    """the spectrogram cache's switches (eps 1e-8 under the root, samples clamped to +-1.05): samples set to +-1.2 get exactly 0"""
    n_fft, hop, n_mels = 1024, 320, 80
    rng = np.random.default_rng(5)
    clip = (0.3 * rng.standard_normal(19 * hop + 5)).astype(np.float32)
    hot = rng.choice(len(clip), 40, replace=False)
    clip[hot] = np.where(rng.random(40) < 0.5, -1.2, 1.2).astype(np.float32)
    cot = rng.standard_normal((n_mels, 19)).astype(np.float32)
    got = vjp_device([clip], [cot], n_fft, hop, n_mels, eps=1e-8, clamp=True)[0]
    cut = np.abs(clip) > 1.05                                # the 40 planted samples and whatever the normal draw itself put beyond the clamp
    assert cut[hot].all() and (got[cut] == 0.0).all() and np.count_nonzero(got[~cut]) == (~cut).sum()
    gated("vjp.eps_clamp", got, vjp_ref(clip, cot, n_fft, hop, n_mels, torch.float64, 1e-8, True), vjp_ref(clip, cot, n_fft, hop, n_mels, torch.float32, 1e-8, True))


# ------------------------------------------------------------------------------------------------- 2: edges
def test_shortest_clip_is_all_fold_back():
    """4096 / 400 pads 1848 samples: the shortest legal clip has 1849, four frames, and every padded position is a mirror image"""
    n_fft, hop, n_mels = 4096, 400, 256
    rng = np.random.default_rng(6)
    clip = (0.3 * rng.standard_normal(1849)).astype(np.float32)
    cot = rng.standard_normal((n_mels, 4)).astype(np.float32)
    got = vjp_device([clip], [cot], n_fft, hop, n_mels)[0]
    gated("vjp.shortest_4096", got, vjp_ref(clip, cot, n_fft, hop, n_mels, torch.float64), vjp_ref(clip, cot, n_fft, hop, n_mels, torch.float32))


def test_crop_leaves_exact_zeros_between_the_frames():
    n_fft, hop, n_mels = 256, 400, 20
    rng = np.random.default_rng(7)
    clip = (0.3 * rng.standard_normal(19 * hop + 5)).astype(np.float32)
    cot = rng.standard_normal((n_mels, 19)).astype(np.float32)
    got = vjp_device([clip], [cot], n_fft, hop, n_mels)[0]
    pos = np.arange(len(clip))
    covered = (pos % hop >= 72) & (pos % hop < 72 + 256) & (pos < 19 * hop)
    assert (got[~covered] == 0.0).all() and np.count_nonzero(got[covered]) > 0.99 * covered.sum()


def test_silent_half_gives_a_finite_gradient_and_silent_frames_nothing():
    """eps = 0: |X| = 0 in the frames inside the silence, where the root has no slope; those frames contribute exactly 0"""
    n_fft, hop, n_mels = 512, 400, 40
    rng = np.random.default_rng(8)
    n = 20 * hop
    clip = (0.3 * rng.standard_normal(n)).astype(np.float32)
    clip[n // 2:] = 0.0
    cot = rng.standard_normal((n_mels, 20)).astype(np.float32)
    got = vjp_device([clip], [cot], n_fft, hop, n_mels)[0]
    first_silent = -(-(n // 2 + 56) // hop)                  # frame f reads samples f hop - 56 .. f hop + 455
    last_touched = (first_silent - 1) * hop - 56 + 512      # one past the last sample a frame with signal reads
    assert np.isfinite(got).all() and (got[last_touched:] == 0.0).all() and np.count_nonzero(got[:n // 2]) > 0.99 * (n // 2)
    gated("vjp.silent_half", got, vjp_ref(clip, cot, n_fft, hop, n_mels, torch.float64), vjp_ref(clip, cot, n_fft, hop, n_mels, torch.float32))


def test_one_cotangent_entry_touches_one_frame_and_its_mirror_images():
    n_fft, hop, n_mels = 1024, 320, 80
    rng = np.random.default_rng(9)
    clip = (0.3 * rng.standard_normal(19 * hop + 5)).astype(np.float32)
    pad = (n_fft - hop) // 2
    for frame in (0, 9, 18):
        cot = np.zeros((n_mels, 19), dtype=np.float32)
        cot[37, frame] = 1.0
        got = vjp_device([clip], [cot], n_fft, hop, n_mels)[0]
        p = frame * hop - pad + np.arange(n_fft)              # the frame's positions; mirrored where they leave the clip
        p = np.where(p < 0, -p, p)
        p = np.where(p >= len(clip), 2 * (len(clip) - 1) - p, p)
        touched = np.zeros(len(clip), dtype=bool)
        touched[p] = True
        assert (got[~touched] == 0.0).all() and np.count_nonzero(got[touched]) > 0.9 * touched.sum(), frame


# ------------------------------------------------------------------------------------------------- 3: the element-wise kernels
def within_4u(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool((np.abs(got - want) <= 4 * U * np.abs(want)).all())


@pytest.mark.parametrize("kind,lw,mw", [("l1", 1.0, 0.0), ("l2", 1.0, 0.5), ("smoothl1", 1.0, 0.5), ("l1", 0.0, 2.0)])
def test_mel_loss_cotangents_against_float64(kind, lw, mw):
    from comfy_rvc_amd.lib.train.losses import _mel_cotangents
    rng = np.random.default_rng(11)
    shapes = [(20, 35), (64, 35), (80, 35), (128, 35), (160, 35), (256, 35), (125, 7), (3, 1)]      # K = 8, the most one launch takes
    a = [(rng.standard_normal(s) * 2.0 - 3.0).astype(np.float32) for s in shapes]
    b = [(x + rng.standard_normal(x.shape) * 1.5).astype(np.float32) for x in a]
    for x, y in zip(a, b):
        y.reshape(-1)[::5] = x.reshape(-1)[::5]                 # exact ties: sign(0) = 0
    scales = [1.0 / (len(shapes) * x.size) for x in a]
    got = _mel_cotangents(kind, [dev(x) for x in a], [dev(y) for y in b], lw, mw, scales)
    for x, y, s, o in zip(a, b, scales, got):
        want = G.mel_loss_cotangent(kind, x, y, lw, mw, float(np.float32(s))).numpy()
        assert o.dtype == torch.float32 and tuple(o.shape) == x.shape and within_4u(o.cpu().numpy(), want)
        assert (o.cpu().numpy().reshape(-1)[::5] == 0.0).all()


def test_kl_loss_grad_against_float64():
    from comfy_rvc_amd.lib.train.losses import kl_loss_grads
    t = golden("train_forward_40k_v2.npz")
    taps = [t[k] for k in ("z_p", "logs_q", "m_p", "logs_p")]
    for scale in (1.0, 1.75):
        got = kl_loss_grads(*[dev(x) for x in taps], dev(t["y_mask"]), scale=scale)
        eff = float(np.float32(scale / float(t["y_mask"].sum())))      # the factor as the kernel receives it
        want = G.kl_grads(*taps, t["y_mask"], scale=eff * float(t["y_mask"].sum()))
        dead = np.broadcast_to(t["y_mask"] == 0, taps[0].shape)
        assert dead.any()
        for k in ("z_p", "logs_q", "m_p", "logs_p"):
            o = got[k].cpu().numpy()
            assert got[k].dtype == torch.float32 and o.shape == taps[0].shape and within_4u(o, want[k].numpy()), k
            assert (o[dead] == 0.0).all(), k


# ------------------------------------------------------------------------------------------------- 4: losses with gradient
def rows_vjp_ref(gen, cot_rows, n_fft, hop, n_mels, sr, fmin, fmax, dtype):
    """gen [B, T], cot_rows [B, n_mels, frames] -> the restatement's gradient [B, T]"""
    return G.vjp(gen, cot_rows, n_fft, n_mels, sr, hop, fmin, fmax, dtype=dtype).numpy()


@pytest.mark.parametrize("r", [40, 32])
def test_mel_loss_grad(r):
    from comfy_rvc_amd.lib.train import mel_processing as MP
    from comfy_rvc_amd.lib.train.losses import LossBalancer, l1_loss, mel_loss_grad
    g = golden("gen_cotangent_cases.npz")
    sr, wave, gen = case(g, r)
    a = AUX[r]
    args = (a["n_fft"], a["n_mels"], sr, a["hop"], a["n_fft"], 0.0, None)
    y_mel, y_hat = dev(g[f"c{r}_y_mel"]), dev(gen[:, None])
    loss, grad, mel = mel_loss_grad(y_mel, y_hat, *args, return_mel=True)
    assert torch.equal(loss, l1_loss(y_mel, MP.mel_spectrogram_torch(y_hat, *args))) and torch.equal(mel, MP.mel_spectrogram_torch(y_hat, *args))
    assert grad.dtype == torch.float32 and tuple(grad.shape) == tuple(y_hat.shape)
    assert torch.equal(grad, mel_loss_grad(y_mel, y_hat, *args)[1])
    cot = G.mel_loss_cotangent("l1", mel.cpu().numpy(), g[f"c{r}_y_mel"], 1.0, 0.0, 1.0 / mel.numel()).numpy()
    got = grad.cpu().numpy()[:, 0]
    gated(f"mel_loss_grad.{r}", got, rows_vjp_ref(gen, cot, a["n_fft"], a["hop"], a["n_mels"], sr, 0.0, None, torch.float64),
          rows_vjp_ref(gen, cot, a["n_fft"], a["hop"], a["n_mels"], sr, 0.0, None, torch.float32))
    check_norm_and_record(g, f"c{r}_mel", grad, LossBalancer)


def check_norm_and_record(g, key, grad, LossBalancer):
    """the balancer's norm of the device gradient (formed on the device, weight 1) inside the golden's tolerance; the pointwise difference is recorded only"""
    bal = LossBalancer(None, initial_weights={"loss_mel": 1.0}, historical_losses={}, ema_weights={}, use_norm=True)
    norm = float(bal.calculate_gradients("loss_mel", torch.tensor(1.0), 1.0, grad))
    want, tol = float(g[key + "_norm"]), float(g[key + "_norm_tol"])
    dump(f"norm.{key}", {"device": norm, "reference": want, "tolerance": tol})
    assert abs(norm - want) <= tol, (key, norm, want, tol)
    assert abs(norm - G.balancer_norm(grad.cpu())) <= 1e-6 * norm
    dump(f"end_to_end.{key}", {"max": peak_err(grad.cpu().numpy(), g[key + "_grad32"]), "gate": None})


@pytest.mark.parametrize("r", [40, 32])
@pytest.mark.parametrize("name", ["msml_l1", "msml_sl1"])
def test_multiscale_forward_and_grad(r, name):
    from comfy_rvc_amd.lib.train.losses import LossBalancer, MultiScaleMelSpectrogramLoss
    g = golden("gen_cotangent_cases.npz")
    sr, wave, gen = case(g, r)
    kw = MSML[name]
    x, y = dev(gen[:, None]), dev(wave[:, None])
    loss, grad, mels = MultiScaleMelSpectrogramLoss(sr, **kw).forward_and_grad(x, y, return_mels=True)
    assert torch.equal(loss, MultiScaleMelSpectrogramLoss(sr, **kw).forward(x, y))
    assert grad.dtype == torch.float32 and tuple(grad.shape) == tuple(x.shape)
    assert torch.equal(grad, MultiScaleMelSpectrogramLoss(sr, **kw).forward_and_grad(x, y)[1])
    hop, K = sr // 100, len(R.DEFAULT_N_MELS)
    want = {torch.float64: 0.0, torch.float32: 0.0}
    for n_mels, (a, b) in zip(sorted(R.DEFAULT_N_MELS), mels):
        a, b = a.permute(1, 0, 2).cpu().numpy(), b.permute(1, 0, 2).cpu().numpy()       # [B, n_mels, frames]
        assert a.shape == (gen.shape[0], n_mels, gen.shape[1] // hop)
        cot = G.mel_loss_cotangent(kw["loss"], a, b, kw["log_weight"], kw["mag_weight"], 1.0 / (K * a.size)).numpy()
        for dt in want:
            want[dt] = want[dt] + rows_vjp_ref(gen, cot, R.window_length(n_mels), hop, n_mels, sr, 50.0, sr // 2, dt).astype(np.float64)
    gated(f"forward_and_grad.{r}.{name}", grad.cpu().numpy()[:, 0], want[torch.float64], want[torch.float32])
    check_norm_and_record(g, f"c{r}_{name}", grad, LossBalancer)


def test_forward_and_grad_adjusts_the_bands_after_the_gradient():
    from comfy_rvc_amd.lib.train.losses import MultiScaleMelSpectrogramLoss
    g = golden("gen_cotangent_cases.npz")
    sr, wave, gen = case(g, 40)
    x, y = dev(gen[:, None]), dev(wave[:, None])
    fixed, moving, twin = (MultiScaleMelSpectrogramLoss(sr, adjustment_factor=f) for f in (0.0, 0.05, 0.05))
    l0, g0 = fixed.forward_and_grad(x, y)
    l1, g1 = moving.forward_and_grad(x, y)
    assert torch.equal(l0, l1) and torch.equal(g0, g1), "the first call's gradient belongs to the bands its loss used"
    assert torch.equal(twin.forward(x, y), l1) and (moving.mel_fmin, moving.mel_fmax) == (twin.mel_fmin, twin.mel_fmax) != (fixed.mel_fmin, fixed.mel_fmax)
    assert torch.equal(moving.forward_and_grad(x, y)[0], twin.forward(x, y))


# ------------------------------------------------------------------------------------------------- 5: the generator's loss and its cotangents
class CountingNet:
    """net_d with a counter on its forward"""

    def __init__(self, net):
        self.net, self.calls = net, 0

    def __call__(self, *a):
        self.calls += 1
        return self.net(*a)

    def __getattr__(self, name):
        return getattr(self.net, name)


def test_generator_loss_cotangents():
    from comfy_rvc_amd.lib.infer_pack.models import MultiPeriodDiscriminatorV2
    from comfy_rvc_amd.lib.train.losses import LossBalancer, adversarial_input_grads, kl_loss_grads, mel_loss_grad
    from comfy_rvc_amd.lib.train.train_step import GEN_LOSS_KEYS, generator_loss_cotangents
    from comfy_rvc_amd.lib.train.utils import HParams
    from test_hip_train_forward import HPS_40K
    g, t = golden("gen_cotangent_cases.npz"), golden("train_forward_40k_v2.npz")
    sr, wave, gen = case(g, 40)
    net = CountingNet(MultiPeriodDiscriminatorV2(False, device=DEV).load_state_dict(S.disc_state_dict("v2", 0)))
    wave_d, y_hat, y_mel = dev(wave[:, None]), dev(gen[:, None]), dev(g["c40_y_mel"])
    taps = [dev(t[k][:2]) for k in ("z_p", "logs_q", "m_p", "logs_p")]
    mask = dev(t["y_mask"][:2])
    hps = HParams(**HPS_40K)
    initial = dict(zip(GEN_LOSS_KEYS, (1., 2., 45., 1., 0., 0., 0.)))
    settings = dict(epsilon=1e-8, weights_decay=.75, loss_decay=.8, active=True, use_pareto=True, use_norm=True)
    bal = LossBalancer(None, initial_weights=dict(initial), historical_losses={}, ema_weights={}, **settings)
    host = LossBalancer(None, initial_weights=dict(initial), historical_losses={}, ema_weights={}, **settings)
    a = AUX[40]
    for step in range(2):                                     # the second batch meets moving averages
        net.calls = 0
        total, terms, d_y_hat, kl_cot = generator_loss_cotangents(net, bal, wave_d, y_hat, y_mel, taps, mask, hps)
        assert net.calls == 1, "the discriminators ran more than once"
        assert tuple(terms) == GEN_LOSS_KEYS and total.dim() == 0 and total.is_cuda and d_y_hat.dtype == torch.float32 and tuple(d_y_hat.shape) == tuple(y_hat.shape)
        w = bal.last_weights
        assert set(w) == {"loss_gen", "loss_fm", "loss_mel", "loss_kl"}
        grads, _ = adversarial_input_grads(net.net, wave_d, y_hat)
        grads["loss_mel"] = mel_loss_grad(y_mel, y_hat, a["n_fft"], a["n_mels"], sr, a["hop"], a["n_fft"], 0.0, None)[1]
        want = sum(w[k] * grads[k].double().cpu().numpy() for k in grads)
        assert within_4u(d_y_hat.cpu().numpy(), want)
        sep = kl_loss_grads(*taps, mask, scale=w["loss_kl"])
        assert all(torch.equal(kl_cot[k], sep[k]) for k in sep)
        norms = {k: float(LossBalancer(None, epsilon=1e-8).calculate_gradients(k, torch.tensor(1.0), initial[k], v)) for k, v in grads.items()}
        ref_total = host.on_train_batch_start({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in terms.items()}, grad_norms=norms)
        dump(f"generator_loss_cotangents.step{step}", {"loss_gen_all": float(total), "host": float(ref_total), "weights": w, "norms": norms})
        assert abs(float(total) - float(ref_total)) <= 1e-6 * abs(float(ref_total))
        assert all(abs(w[k] - host.last_weights[k]) <= 1e-6 * abs(host.last_weights[k]) for k in w)
    with pytest.raises(NotImplementedError):
        generator_loss_cotangents(net, bal, wave_d, y_hat, y_mel, taps, mask, HParams(**{**HPS_40K, "train": {**HPS_40K["train"], "c_tsi": 1.0}}))
