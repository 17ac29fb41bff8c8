"""GPU: the STFT at the multi-scale geometries (rvc_spectrogram_batch_ms), MultiScaleMelSpectrogramLoss, the HPSS / TSI auxiliary losses and the
evaluation that follows the trainer's switches (csrc/spectrogram.hip, csrc/aux_losses.hip, lib/train/losses.py, lib/train/evaluate.py).

Gates.
  STFT: err = max |x - f64| / (that frame's peak in f64) against a float64 DFT of the same fp32 frames; err_dev <= 8 err_ref, err_ref the same figure of
    torch.stft in fp32 on the CPU for that input (the rule of test_hip_spectrogram.py).
  HPSS: the medians bit-equal to scipy.ndimage.median_filter(mode="reflect"); the masked parts within 4 x the largest error of the float32 restatement
    (tests/aux_loss_ref.py) against its float64 self over the same tensor.
  Losses: inside the tolerance stored with the reference's value (tests/golden/aux_loss_cases.npz), and within 8 x the float32 restatement's own error
    of the float64 restatement.  A single loss is one number, and the float32 error of one number is one draw of a rounding error that is as likely tiny
    as typical; "the float32 restatement's own error" is therefore taken per QUANTITY as the largest relative |f32 - f64| / |f64| that quantity shows
    over the four golden cases (A, B at 40 and 32 kHz; for the multi-scale loss over all scales, loss types and cases), times the value at hand.
Every figure is printed (-s); with AUX_PARITY_DUMP=<file.json> in the environment they are also written there (profiles/aux_loss_parity.json)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden
from spec_ref import frame_peak_err, torch_spec_f32
import aux_loss_ref as R
from test_aux_loss_host import AUX, F32_EPS, SAVED, case_waves, msml_args, msml_keys

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ("A40", "B40", "A32", "B32")


def _mp():
    from comfy_rvc_amd.lib.train import mel_processing as MP
    return MP


def _losses():
    from comfy_rvc_amd.lib.train import losses as L
    return L


def _record(key, value):
    path = os.environ.get("AUX_PARITY_DUMP")
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


# ----------------------------------------------------------------------------------------------------------------- STFT
STFT_GEOMETRIES = ((256, 400, 40000), (512, 400, 40000), (4096, 400, 40000), (256, 480, 48000), (4096, 320, 32000))
FRAMES = 19                                   # not a multiple of 16 or 8 frames per workgroup, more than one workgroup at every size


def _signal(sr, n, seed):
    from comfy_rvc_amd import synthetic as S
    return S.spec_test_signal(sr, n, seed)


def _ms(x, n_fft, hop, eps=1e-8, clamp=True):
    MP = _mp()
    out = torch.empty(n_fft // 2 + 1, max(x.shape[0] // hop, 1), device=DEV)
    MP.spectrogram_packed_ms(torch.from_numpy(x).to(DEV), np.array([[0, x.shape[0], 0]], dtype=np.int64), n_fft, hop, eps, clamp, out)
    return out[:, :x.shape[0] // hop].cpu().numpy()


def _f64(x, n_fft, hop, eps=1e-8):
    """float64 DFT of the fp32 frames: clamp, frames (reflected or cropped), the Hann window in float64, sqrt(re^2 + im^2 + eps)."""
    x = torch.from_numpy(np.clip(x, np.float32(-1.05), np.float32(1.05)).astype(np.float64))[None]
    win = 0.5 - 0.5 * torch.cos(2.0 * np.pi * torch.arange(n_fft, dtype=torch.float64) / n_fft)
    z = torch.fft.rfft(R.frames(x, n_fft, hop) * win, dim=-1)[0]
    return torch.sqrt(z.real ** 2 + z.imag ** 2 + eps).numpy().T


@pytest.mark.parametrize("n_fft,hop,sr", STFT_GEOMETRIES)
def test_stft_accuracy(n_fft, hop, sr):
    x = _signal(sr, FRAMES * hop + 5, 60 + n_fft // 256)
    dev, ref64 = _ms(x, n_fft, hop), _f64(x, n_fft, hop)
    assert dev.shape == (n_fft // 2 + 1, FRAMES) and dev.dtype == np.float32
    err_dev, err_ref = frame_peak_err(dev, ref64), frame_peak_err(torch_spec_f32(x, n_fft, hop), ref64)
    print(f"stft {n_fft}/{hop}: err_dev {err_dev:.3e} err_ref {err_ref:.3e}")
    _record(f"stft_{n_fft}_{hop}", {"err_dev": err_dev, "err_ref": err_ref, "reference": "torch.stft cpu fp32"})
    assert err_dev <= 8 * err_ref
    assert np.array_equal(dev, _ms(x, n_fft, hop))


def test_stft_shortest_clip_at_4096():
    from comfy_rvc_amd import _lib
    n_fft, hop = 4096, 400
    pad = (n_fft - hop) // 2
    x = _signal(40000, pad + 1, 71)
    assert x.shape[0] == 1849
    dev, ref64 = _ms(x, n_fft, hop), _f64(x, n_fft, hop)
    err_dev, err_ref = frame_peak_err(dev, ref64), frame_peak_err(torch_spec_f32(x, n_fft, hop), ref64)
    print(f"stft 4096/400 shortest: err_dev {err_dev:.3e} err_ref {err_ref:.3e}")
    _record("stft_4096_400_shortest", {"err_dev": err_dev, "err_ref": err_ref})
    assert dev.shape[1] == 4 and err_dev <= 8 * err_ref
    with pytest.raises(_lib.RvcHipError):
        _ms(x[:-1], n_fft, hop)
    with pytest.raises(ValueError):
        _mp().mel_spectrogram_torch(torch.from_numpy(x[:-1]).to(DEV)[None, None], n_fft, 80, 40000, hop, n_fft, 0.0, None)


def test_stft_crop_starts_at_sample_72():
    """hop 400 > n_fft 256: nothing is reflected, frame f is samples [400 f + 72, 400 f + 328); one hop is enough for one frame."""
    n_fft, hop = 256, 400
    x = _signal(40000, 3 * hop + 7, 72)
    dev = _ms(x, n_fft, hop, eps=0.0, clamp=False)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    for f in range(3):
        want = np.abs(np.fft.rfft(x[hop * f + 72:hop * f + 72 + n_fft].astype(np.float64) * win))
        assert np.abs(dev[:, f] - want).max() <= 1e-5 * want.max(), f
    shifted = x.copy()
    shifted[:72] = 0.5                         # samples before the first frame do not matter
    assert np.array_equal(_ms(shifted, n_fft, hop, eps=0.0, clamp=False), dev)
    assert _ms(x[:hop], n_fft, hop).shape == (129, 1)
    from comfy_rvc_amd import _lib
    with pytest.raises(_lib.RvcHipError):
        _ms(x[:hop - 1], n_fft, hop)


@pytest.mark.parametrize("n_fft,hop", [(256, 400), (4096, 400)])
def test_stft_ragged_batch_leaves_gaps(n_fft, hop):
    MP = _mp()
    xs = [_signal(40000, n, 80 + i) for i, n in enumerate((max(17 * hop + 3, 1849), 1849 if n_fft == 4096 else hop, 9 * hop + 399))]
    table, off, col = [], 0, 0
    for x in xs:
        col += 5
        table.append((off, x.shape[0], col))
        off += x.shape[0]
        col += x.shape[0] // hop
    out = torch.full((n_fft // 2 + 1, col + 5), float("nan"), device=DEV)
    MP.spectrogram_packed_ms(torch.from_numpy(np.concatenate(xs)).to(DEV), np.array(table, dtype=np.int64), n_fft, hop, 1e-8, True, out)
    whole = out.cpu().numpy()
    used = np.zeros(whole.shape[1], dtype=bool)
    for (o, n, c), x in zip(table, xs):
        assert np.array_equal(whole[:, c:c + n // hop], _ms(x, n_fft, hop))
        used[c:c + n // hop] = True
    assert np.all(np.isnan(whole[:, ~used])) and not np.any(np.isnan(whole[:, used]))


def test_stft_refused_calls_leave_the_output_untouched():
    from comfy_rvc_amd import _lib
    MP = _mp()
    x = torch.from_numpy(_signal(40000, 4000, 90)).to(DEV)

    def attempt(n_fft, hop, samples):
        out = torch.full((n_fft // 2 + 1, 64), float("nan"), device=DEV)
        with pytest.raises(_lib.RvcHipError):
            MP.spectrogram_packed_ms(x, np.array([[0, 4000, 0], [0, samples, 16]], dtype=np.int64), n_fft, hop, 1e-8, True, out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), (n_fft, hop, samples)

    attempt(128, 64, 4000)                       # unsupported n_fft
    attempt(8192, 400, 4000)
    attempt(512, 401, 4000)                      # n_fft - hop odd
    attempt(512, 0, 4000)
    attempt(512, 400, 4001)                      # a clip beyond the audio buffer
    attempt(512, 400, (512 - 400) // 2)          # N <= pad
    attempt(256, 400, 399)                       # hop > n_fft: less than one hop
    # the first entry keeps its contract
    out = torch.full((257, 64), float("nan"), device=DEV)
    with pytest.raises(_lib.RvcHipError):
        MP.spectrogram_packed(x, np.array([[0, 4000, 0]], dtype=np.int64), 512, 128, 1e-8, True, out)
    assert bool(torch.isnan(out).all())


def test_mel_spectrogram_torch_routes_by_geometry():
    """(1024 | 2048, hop <= n_fft) through the first entry, bit-identical to it; everything else through the new one."""
    MP = _mp()
    x = _signal(40000, 7 * 400 + 123, 21)
    xd = torch.from_numpy(x).to(DEV)
    first = torch.empty(1025, 7, device=DEV)
    MP.spectrogram_packed(xd, np.array([[0, x.shape[0], 0]], dtype=np.int64), 2048, 400, 1e-8, True, first)
    assert torch.equal(MP.spectrogram_torch(xd[None], 2048, 400, 2048)[0], first)
    assert np.array_equal(MP.spectrogram_torch(xd[None], 512, 400, 512)[0].cpu().numpy(), _ms(x, 512, 400))
    with pytest.raises(NotImplementedError):
        MP.spectrogram_torch(xd[None], 512, 400, 512, center=True)
    with pytest.raises(NotImplementedError):
        MP.mel_spectrogram_torch(xd[None, None], 512, 80, 40000, 400, 256, 0.0, None)


# ----------------------------------------------------------------------------------------------------------------- HPSS
@pytest.mark.parametrize("shape", [(2, 20, 32), (1, 125, 15), (1, 15, 45)])
def test_hpss(shape):
    from scipy.ndimage import median_filter
    L = _losses()
    g = np.random.default_rng(sum(shape))
    mag = (g.standard_normal(shape) * 2.0 - 4.0).astype(np.float32)
    mag[0, 3:6, 4:9] = 0.0                       # both medians vanish here: the split-zeros branch
    md = torch.from_numpy(mag).to(DEV)
    mt, mf = (t.cpu().numpy() for t in L.hpss_parts(md, medians=True))
    S, T = np.abs(mag), shape[2]
    for q, k in enumerate(R.HPSS_SIZES):
        assert np.array_equal(mt[..., q * T:(q + 1) * T], median_filter(S, size=(1, 1, k), mode="reflect")), ("time", k)
        assert np.array_equal(mf[..., q * T:(q + 1) * T], median_filter(S, size=(1, k, 1), mode="reflect")), ("mel", k)
    h, p = (t.cpu().numpy() for t in L.hpss_parts(md))
    (h64, p64), (h32, p32) = R.hpss_parts(mag, torch.float64), R.hpss_parts(mag, torch.float32)
    for name, dev, r64, r32 in (("harmonic", h, h64, h32), ("percussive", p, p64, p32)):
        err_dev, err_ref = float(np.abs(dev - r64.numpy()).max()), float(np.abs(r32.numpy().astype(np.float64) - r64.numpy()).max())
        print(f"hpss {shape} {name}: err_dev {err_dev:.3e} err_f32 {err_ref:.3e}")
        _record(f"hpss_{'x'.join(map(str, shape))}_{name}", {"err_dev": err_dev, "err_f32": err_ref})
        assert err_dev <= 4 * err_ref, (name, err_dev, err_ref)
    assert np.all(h[0, 4, 5:8] == 0.0)           # S = 0 there; the mask itself is 0.5
    h2, p2 = L.hpss_parts(md)
    assert np.array_equal(h2.cpu().numpy(), h) and np.array_equal(p2.cpu().numpy(), p)


# ----------------------------------------------------------------------------------------------------------------- losses: references, computed once
_ref = {}


def _aux_ref(name):
    """float64 / float32 restatement of (harmonic loss, tsi dim=-1, tsi dim=-2) and the float32 log-mels of a golden case."""
    if ("aux", name) not in _ref:
        sr, wave, gen = case_waves(golden("aux_loss_cases.npz"), name)
        n_mels, n_fft, hop = AUX[sr]
        out = {}
        for dt in (torch.float64, torch.float32):
            om, gm = R.aux_mags(wave.astype(np.float64 if dt == torch.float64 else np.float32), gen.astype(np.float64 if dt == torch.float64 else np.float32),
                                n_mels, sr, n_fft, hop, 0.0, None, dt)
            out[dt] = np.array([R.harmonic_loss(om, gm, F32_EPS, dt) if om.shape[2] > 14 else np.nan, R.tsi_term(om, gm, -1, F32_EPS, dt),
                                R.tsi_term(om, gm, -2, F32_EPS, dt)])
        _ref[("aux", name)] = out
    return _ref[("aux", name)]


def _aux_rel32():
    """Per quantity: the largest relative float32-vs-float64 difference of the restatement over the golden cases."""
    if "aux_rel" not in _ref:
        rel = np.zeros(3)
        for name in CASES:
            r = _aux_ref(name)
            rel = np.fmax(rel, np.abs(r[torch.float32] - r[torch.float64]) / np.abs(r[torch.float64]))
        _ref["aux_rel"] = rel
    return _ref["aux_rel"]


def _msml_ref(name, key):
    if ("msml", name, key) not in _ref:
        g = golden("aux_loss_cases.npz")
        sr, wave, gen = case_waves(g, name)
        kind, lw, mw, fmin, fmax = msml_args(key, sr)
        out = {}
        for dt, nt in ((torch.float64, np.float64), (torch.float32, np.float32)):
            per, total = R.multiscale(gen.astype(nt), wave.astype(nt), sr, fmin=fmin, fmax=fmax, loss=kind, log_weight=lw, mag_weight=mw, dtype=dt)
            out[dt] = np.array(per + [total])
        _ref[("msml", name, key)] = out
    return _ref[("msml", name, key)]


def _msml_rel32():
    if "msml_rel" not in _ref:
        g = golden("aux_loss_cases.npz")
        rel = 0.0
        for name in CASES:
            for key in msml_keys(g, name):
                r = _msml_ref(name, key)
                rel = max(rel, float(np.max(np.abs(r[torch.float32] - r[torch.float64]) / np.abs(r[torch.float64]))))
        _ref["msml_rel"] = rel
    return _ref["msml_rel"]


def _dev3(x):
    return torch.from_numpy(x).to(DEV)[:, None, :]


@pytest.mark.parametrize("name", CASES)
def test_multiscale_mel_loss(name):
    L = _losses()
    g = golden("aux_loss_cases.npz")
    sr, wave, gen = case_waves(g, name)
    rel32 = _msml_rel32()
    failures = []
    for key in msml_keys(g, name):
        kind, lw, mw, fmin, fmax = msml_args(key, sr)
        m = L.MultiScaleMelSpectrogramLoss(sr, loss=kind, log_weight=lw, mag_weight=mw)
        if key.endswith("saved"):
            m = L.MultiScaleMelSpectrogramLoss(**{**m.to_dict(), "mel_fmin": list(fmin), "mel_fmax": list(fmax)})
        total = m(_dev3(gen), _dev3(wave))
        assert total.dim() == 0 and total.dtype == torch.float32 and total.is_cuda
        got = np.array(m.scale_losses.cpu().tolist() + [float(total)], dtype=np.float64)
        r64 = _msml_ref(name, key)[torch.float64]
        d_gold, d_ref, gate = np.abs(got - g[key]), np.abs(got - r64), 8 * rel32 * np.abs(r64)
        print(key, "vs golden", d_gold.tolist(), "tol", g[key + "_tol"].tolist(), "vs f64", d_ref.tolist(), "gate", gate.tolist())
        _record(key, {"vs_golden": d_gold.tolist(), "golden_tol": g[key + "_tol"].tolist(), "vs_f64": d_ref.tolist(), "gate_f64": gate.tolist()})
        if not (np.all(d_gold <= g[key + "_tol"]) and np.all(d_ref <= gate)):
            failures.append(key)
        again = m(_dev3(gen), _dev3(wave))
        assert torch.equal(again, total) and m.mel_fmin == (list(fmin) if key.endswith("saved") else [50.0] * 6)
    assert not failures, failures


def test_multiscale_adjustment_moves_the_bands_and_reuploads():
    L = _losses()
    sr, wave, gen = case_waves(golden("aux_loss_cases.npz"), "B40")
    m = L.MultiScaleMelSpectrogramLoss(sr, adjustment_factor=0.05)
    a = float(m(_dev3(gen), _dev3(wave)))
    assert m.mel_fmin != [50.0] * 6 or m.mel_fmax != [sr // 2] * 6
    fresh = L.MultiScaleMelSpectrogramLoss(**copy.deepcopy({**m.to_dict(), "adjustment_factor": 0.0}))      # (to_dict hands out the band lists themselves)
    b, c = float(m(_dev3(gen), _dev3(wave))), float(fresh(_dev3(gen), _dev3(wave)))
    assert b == c and a != b                      # the second call ran on the moved bands, as a fresh instance with those bands does


@pytest.mark.parametrize("name", CASES)
def test_aux_losses(name):
    L = _losses()
    g = golden("aux_loss_cases.npz")
    sr, wave, gen = case_waves(g, name)
    n_mels, n_fft, hop = AUX[sr]
    kw = dict(n_mels=n_mels, sample_rate=sr, n_fft=n_fft, hop_length=hop, win_length=n_fft, fmin=0.0, fmax=None)
    r64, rel32 = _aux_ref(name)[torch.float64], _aux_rel32()
    h, te, t = L.combined_aux_loss(_dev3(wave), _dev3(gen), c_tefs=0.0, c_hd=1.0, c_tsi=1.0, **kw)
    assert te == 0 and h.dim() == 0 and t.dim() == 0 and h.dtype == t.dtype == torch.float32 and h.is_cuda
    mag = _mp().mel_spectrogram_torch(torch.cat([_dev3(wave), _dev3(gen)]), n_fft, n_mels, sr, hop, n_fft, 0.0, None)
    B = wave.shape[0]
    parts = [float(L.compute_tsi_loss(mag[:B], mag[B:], dim=d, eps=F32_EPS)) for d in (-1, -2)]
    got = np.array([float(h), parts[0], parts[1]])
    d_ref, gate = np.abs(got - r64), 8 * rel32 * np.abs(r64)
    d_gold = np.abs(np.array([float(h), float(t)]) - g[f"{name}_aux"])
    print(name, "aux (harmonic, tsi -1, tsi -2) vs f64", d_ref.tolist(), "gate", gate.tolist(), "vs golden (harmonic, tsi)", d_gold.tolist(), "tol",
          g[f"{name}_aux_tol"].tolist())
    _record(f"{name}_aux", {"vs_f64": d_ref.tolist(), "gate_f64": gate.tolist(), "vs_golden": d_gold.tolist(), "golden_tol": g[f"{name}_aux_tol"].tolist()})
    assert abs(float(t) - (np.float32(parts[0]) + np.float32(parts[1]))) <= 1e-6
    # same call twice, and the single-term calls
    h2, _, t2 = L.combined_aux_loss(_dev3(wave), _dev3(gen), c_tefs=0.0, c_hd=1.0, c_tsi=1.0, **kw)
    assert torch.equal(h, h2) and torch.equal(t, t2)
    only_h = L.combined_aux_loss(_dev3(wave), _dev3(gen), c_tefs=0.0, c_hd=1.0, c_tsi=0.0, **kw)
    assert only_h[1] == 0 and only_h[2] == 0 and torch.equal(only_h[0], h)
    assert np.all(d_gold <= g[f"{name}_aux_tol"]) and np.all(d_ref <= gate)


@pytest.mark.parametrize("name", ["B40", "B32", "H"])
def test_compute_harmonics_tensors(name):
    L = _losses()
    g = golden("aux_loss_cases.npz")
    eps = 1e-8 if name == "H" else F32_EPS
    mag = g[f"{name}_mag"]
    h, p = L.compute_harmonics(torch.from_numpy(mag).to(DEV), eps=eps)
    (h64, p64), (h32, p32) = R.harmonics(mag, eps, torch.float64), R.harmonics(mag, eps, torch.float32)
    for tag, dev, r64, r32, gold in (("harm", h, h64, h32, g[f"{name}_harm"]), ("perc", p, p64, p32, g[f"{name}_perc"])):
        dev = dev.cpu().numpy()
        err_dev, err_ref = float(np.abs(dev - r64.numpy()).max()), float(np.abs(r32.numpy().astype(np.float64) - r64.numpy()).max())
        err_gold = float(np.abs(dev - gold).max())
        print(f"compute_harmonics {name} {tag}: err_dev {err_dev:.3e} err_f32 {err_ref:.3e} vs golden {err_gold:.3e}")
        _record(f"{name}_{tag}", {"err_dev": err_dev, "err_f32": err_ref, "vs_golden": err_gold})
        assert dev.shape == gold.shape and err_dev <= 8 * err_ref and err_gold <= 8 * err_ref + 4 * F32_EPS, tag


# ----------------------------------------------------------------------------------------------------------------- evaluation
def test_evaluate_checkpoint_follows_the_switches(tmp_path):
    from comfy_rvc_amd import synthetic as S
    from comfy_rvc_amd.lib.train.evaluate import evaluate_checkpoint, load_generator
    from comfy_rvc_amd.lib.train.utils import HParams
    from test_hip_train_forward import HPS_40K
    L = _losses()
    e, g = golden("train_eval_cases.npz"), golden("aux_loss_cases.npz")
    filelist = S.write_train_filelist(str(tmp_path), feat_dim=768, spec_bins=1025)
    sd = {k: torch.from_numpy(v) for k, v in S.synth_train_state_dict(S.CONFIG_40K_V2).items()}
    kw = dict(seed=int(e["walk_seed"]), batch_size=int(e["walk_batch_size"]), boundaries=[int(x) for x in e["walk_boundaries"]])

    def hps(**train):
        return HParams(**{**HPS_40K, "train": {**HPS_40K["train"], **train}})
    net = load_generator({"model": sd}, hps())
    on = dict(use_multiscale=True, c_hd=1.0, c_tsi=1.0, eps=float(g["walk_eps"]))
    r = evaluate_checkpoint(net, filelist, hps(**on), **kw)
    saved = L.MultiScaleMelSpectrogramLoss(40000, epsilon=float(g["walk_eps"]), adjustment_factor=0.03)
    saved.mel_fmin, saved.mel_fmax = list(SAVED["mel_fmin"]), list(SAVED["mel_fmax"])
    r_saved = evaluate_checkpoint({"model": sd, "iteration": 0, "msml": saved.to_dict()}, filelist, hps(**on), **kw)
    failures = []
    for run, names in ((r, (("loss_mel", "loss_mel"), ("harmonic_loss", "harmonic_loss"), ("tsi_loss", "tsi_loss"))), (r_saved, (("loss_mel", "loss_mel_saved"),))):
        assert len(run["batches"]) == 2
        for k, gk in names:
            d, tol = abs(run[k] - float(g[f"walk_{gk}"])), float(g[f"walk_{gk}_tol"])
            db = [abs(row[k] - float(g[f"walk_batch_{gk}"][i])) for i, row in enumerate(run["batches"])]
            print("walk", gk, run[k], "delta", d, "tolerance", tol, "per batch", db, "tolerance", float(g[f"walk_batch_{gk}_tol"]))
            _record(f"evaluate_checkpoint.{gk}", {"delta": d, "tol": tol, "batch_delta": db, "batch_tol": float(g[f"walk_batch_{gk}_tol"])})
            if not (d <= tol and all(x <= float(g[f"walk_batch_{gk}_tol"]) for x in db)):
                failures.append(gk)
    assert not failures, failures
    assert abs(r_saved["loss_mel"] - r["loss_mel"]) > float(g["walk_loss_mel_tol"]) + float(g["walk_loss_mel_saved_tol"])      # the saved bands were used
    assert r_saved["loss_kl"] == r["loss_kl"] and all(np.array_equal(a["ids_slice"], b["ids_slice"]) for a, b in zip(r["batches"], r_saved["batches"]))
    assert all(np.array_equal(row["ids_slice"], e["walk_ids_slice"][i]) for i, row in enumerate(r["batches"]))
    # without the switches: the result as before, key for key
    plain = evaluate_checkpoint(net, filelist, hps(), **kw)
    off = evaluate_checkpoint(net, filelist, hps(use_multiscale=False, c_hd=0.0, c_tsi=0.0), **kw)
    assert sorted(plain) == ["batches", "loss_kl", "loss_mel"] and all(sorted(row) == ["ids_slice", "loss_kl", "loss_mel"] for row in plain["batches"])
    for a, b in ((plain, off),):
        assert a["loss_mel"] == b["loss_mel"] and a["loss_kl"] == b["loss_kl"]
        assert all(x["loss_mel"] == y["loss_mel"] and x["loss_kl"] == y["loss_kl"] and np.array_equal(x["ids_slice"], y["ids_slice"])
                   for x, y in zip(a["batches"], b["batches"]))
    for k in ("loss_mel", "loss_kl"):
        assert abs(plain[k] - float(e[f"walk_{k}"])) <= float(e[f"walk_{k}_tol"]), k
    assert plain["loss_kl"] == r["loss_kl"]


# ----------------------------------------------------------------------------------------------------------------- errors
def test_errors():
    L = _losses()
    x = torch.zeros(1, 1, 12800, device=DEV)
    with pytest.raises(NotImplementedError, match="tefs"):
        L.combined_aux_loss(x, x, c_tefs=0.5, c_hd=1.0, c_tsi=1.0)
    with pytest.raises(NotImplementedError):
        L.MultiScaleMelSpectrogramLoss(40000, center=True)(x, x)
    for shape in ((1, 14, 40), (1, 40, 14)):
        with pytest.raises(ValueError):
            L.compute_harmonics(torch.zeros(shape, device=DEV))
        with pytest.raises(ValueError):
            L.harmonic_loss(torch.zeros(shape, device=DEV), torch.zeros(shape, device=DEV))
    with pytest.raises(ValueError):
        L.combined_aux_loss(x, x, c_tefs=0.0, c_hd=1.0, c_tsi=0.0, n_fft=2048, hop_length=400, win_length=2048, n_mels=14)      # 14 mels
    for fn in (lambda: L.compute_harmonics(torch.zeros(1, 20, 20)), lambda: L.compute_tsi_loss(torch.zeros(1, 20, 20), torch.zeros(1, 20, 20)),
               lambda: L.MultiScaleMelSpectrogramLoss(40000)(x.cpu(), x.cpu()), lambda: L.combined_aux_loss(x.cpu(), x.cpu(), c_tefs=0.0)):
        with pytest.raises(ValueError):
            fn()
    # silence: every term is defined (no NaN)
    h, _, t = L.combined_aux_loss(x, x, c_tefs=0.0)
    assert float(h) == 0.0 and np.isfinite(float(t)) and float(L.MultiScaleMelSpectrogramLoss(40000)(x, x)) == 0.0
