"""GPU: the LDS-FFT spectrogram, the mel projection and the spectrogram cache (csrc/spectrogram.hip, lib/train, preprocessing_utils).

Accuracy metric: err = max |x - f64| / (that frame's peak in f64) against the in-test float64 restatement (spec_ref.spec_f64).  Gate:
err_dev <= 8 err_ref, err_ref = the same figure of the reference's own torch.stft result on the same input (tests/golden/spec_cases.npz where the case
has a golden, torch.stft on the CPU in fp32 otherwise): the reference's FFT behaves like about one rounding of the result; the LDS FFT passes every
value through 5 complex stages, the real-input split and the window product, at most one rounding each.  Every figure is printed (-s); with SPEC_PARITY_DUMP=<file.json> in the
environment they are also written to that file, which is how profiles/spec_cache_parity.json was made."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden
from spec_ref import FRAMES_PER_WG, GEOMETRIES, clip_cases, clip_signal, frame_peak_err, spec_f64, torch_spec_f32

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("min", "l3", "l7", "l17", "zero")
BATCH_ORDER = (3, 0, 4, 2, 1)                 # the ragged batch takes the clips in this order
GAP = 5                                       # unused columns in front of every clip of the batch, NaN before the call


def _mp():
    from comfy_rvc_amd.lib.train import mel_processing as MP
    return MP


def _single(x, n_fft, hop, eps=1e-8, clamp=True):
    """One clip alone, the output row exactly as long as its frames."""
    MP = _mp()
    xd = torch.from_numpy(x).to(DEV)
    out = torch.empty(n_fft // 2 + 1, max(x.shape[0] // hop, 1), device=DEV)
    MP.spectrogram_packed(xd, np.array([[0, x.shape[0], 0]], dtype=np.int64), n_fft, hop, eps, clamp, out)
    return out[:, :x.shape[0] // hop].cpu().numpy()


def _batched(xs, n_fft, hop):
    """All clips in one call, in BATCH_ORDER, GAP poisoned columns in front of each -> (per-clip results in NAMES order, the whole output)."""
    MP = _mp()
    order = [xs[i] for i in BATCH_ORDER]
    table, off, col = [], 0, 0
    for x in order:
        col += GAP
        table.append((off, x.shape[0], col))
        off += x.shape[0]
        col += x.shape[0] // hop
    pitch = col + GAP
    out = torch.full((n_fft // 2 + 1, pitch), float("nan"), device=DEV)
    MP.spectrogram_packed(torch.from_numpy(np.concatenate(order)).to(DEV), np.array(table, dtype=np.int64), n_fft, hop, 1e-8, True, out)
    whole = out.cpu().numpy()
    res = [None] * len(xs)
    used = np.zeros(pitch, dtype=bool)
    for (o, n, c), i in zip(table, BATCH_ORDER):
        res[i] = whole[:, c:c + n // hop]
        used[c:c + n // hop] = True
    return res, whole, used


_cache = {}


def _geometry(g):
    if g not in _cache:
        n_fft, hop, sr = GEOMETRIES[g]
        xs = [clip_signal(g, name) for name in NAMES]
        d = {"xs": xs, "f64": [spec_f64(x, n_fft, hop) for x in xs], "single": [_single(x, n_fft, hop) for x in xs]}
        d["batch"], d["whole"], d["used"] = _batched(xs, n_fft, hop)
        d["batch2"] = _batched(xs, n_fft, hop)[0]
        _cache[g] = d
    return _cache[g]


def _record(key, value):
    path = os.environ.get("SPEC_PARITY_DUMP")
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


@pytest.mark.parametrize("g", range(3))
def test_spectrogram_accuracy(g):
    n_fft, hop, sr = GEOMETRIES[g]
    d = _geometry(g)
    gold = golden("spec_cases.npz")
    failures = []
    for i, name in enumerate(NAMES):
        key = f"g{n_fft}_{hop}_{name}"
        ref32 = gold[key] if key in gold else torch_spec_f32(d["xs"][i], n_fft, hop)
        err_ref = frame_peak_err(ref32, d["f64"][i])
        err_dev = frame_peak_err(d["single"][i], d["f64"][i])
        print(f"{key}: err_dev {err_dev:.3e} err_ref {err_ref:.3e} ({'golden' if key in gold else 'torch.stft'})")
        _record(key, {"err_dev": err_dev, "err_ref": err_ref, "reference": "golden" if key in gold else "torch.stft cpu fp32"})
        assert d["single"][i].shape == (n_fft // 2 + 1, d["xs"][i].shape[0] // hop)
        if not err_dev <= 8 * err_ref:
            failures.append((key, err_dev, err_ref))
    assert not failures, failures


@pytest.mark.parametrize("g", range(3))
def test_spectrogram_exact_conditions(g):
    n_fft, hop, sr = GEOMETRIES[g]
    d = _geometry(g)
    for i, name in enumerate(NAMES):
        n = d["xs"][i].shape[0]
        assert d["single"][i].shape[1] == n // hop and n // hop >= 1, name
        assert np.array_equal(d["batch"][i], d["single"][i]), f"{name}: batched != single"
        assert np.array_equal(d["batch2"][i], d["batch"][i]), f"{name}: two runs differ"
    assert clip_cases(g)["l17"][0] // hop == FRAMES_PER_WG + 1
    # the poisoned gaps (row pitch larger than the frames) are untouched, everything else is written
    assert np.all(np.isnan(d["whole"][:, ~d["used"]])) and not np.any(np.isnan(d["whole"][:, d["used"]]))
    # silence: the epsilon alone
    zi = NAMES.index("zero")
    assert np.all(d["single"][zi] == np.sqrt(np.float32(1e-8))) and d["single"][zi].dtype == np.float32
    assert np.all(_single(d["xs"][zi], n_fft, hop, eps=0.0) == 0.0)
    # the clamp: samples beyond +-1.05 give the clamped signal's spectrum
    x = d["xs"][NAMES.index("l7")]
    assert np.abs(x).max() > 1.05
    clipped = np.clip(x, np.float32(-1.05), np.float32(1.05))
    assert np.array_equal(d["single"][NAMES.index("l7")], _single(clipped, n_fft, hop, clamp=False))
    assert not np.array_equal(d["single"][NAMES.index("l7")], _single(x, n_fft, hop, clamp=False))


def test_spectrogram_torch_batch_rows():
    """The reference-signature entry on a [B, T] batch equals the single-clip results row by row."""
    MP = _mp()
    n_fft, hop, sr = GEOMETRIES[1]
    d = _geometry(1)
    x = d["xs"][NAMES.index("l7")]
    y = torch.from_numpy(np.stack([x, x[::-1].copy(), np.zeros_like(x)])).to(DEV)
    out = MP.spectrogram_torch(y, n_fft, hop, n_fft)
    assert out.shape == (3, n_fft // 2 + 1, x.shape[0] // hop) and out.is_cuda and out.is_contiguous()
    assert np.array_equal(out[0].cpu().numpy(), d["single"][NAMES.index("l7")])
    assert np.array_equal(out[1].cpu().numpy(), _single(x[::-1].copy(), n_fft, hop))
    assert np.array_equal(MP.spectrogram_torch(y[:1].double(), n_fft, hop, n_fft).cpu().numpy(), out[:1].double().cpu().numpy())


def test_spectrogram_errors_leave_output_untouched():
    from comfy_rvc_amd import _lib
    MP = _mp()
    x = torch.from_numpy(clip_signal(1, "l7")).to(DEV)
    n = x.numel()

    def attempt(n_fft, hop, samples):
        out = torch.full((n_fft // 2 + 1, 64), float("nan"), device=DEV)
        with pytest.raises(_lib.RvcHipError):
            MP.spectrogram_packed(x, np.array([[0, n, 0], [0, samples, 16]], dtype=np.int64), n_fft, hop, 1e-8, True, out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), (n_fft, hop, samples)

    attempt(2048, 400, (2048 - 400) // 2)        # N <= pad
    attempt(2048, 401, n)                        # n_fft - hop odd
    attempt(512, 128, n)                         # unsupported n_fft
    attempt(2048, 400, n + 1)                    # a clip beyond the audio buffer
    with pytest.raises(ValueError):
        MP.spectrogram_torch(x[None, :(2048 - 400) // 2], 2048, 400, 2048)


MEL_GEOMETRIES = ((80, 0), (125, 1), (128, 2))      # (n_mels, index into GEOMETRIES)


def _mel_f64(w32, spec32):
    return np.log(np.maximum(w32.astype(np.float64) @ spec32.astype(np.float64), np.float64(np.float32(1e-5))))


@pytest.mark.parametrize("n_mels,g", MEL_GEOMETRIES)
def test_mel(n_mels, g):
    """spec_to_mel_torch and mel_spectrogram_torch against the float64 evaluation of the SAME fp32 filterbank on the same fp32 spectrogram.  Gate on the
    absolute difference of the logs: 4 x the error of torch's fp32 matmul + log on the CPU for that input, not below 2e-6 (two fp32 ulps at |ln 1e-5|)."""
    MP = _mp()
    n_fft, hop, sr = GEOMETRIES[g]
    w = MP.mel_filterbank(sr, n_fft, n_mels, 0.0, None)
    floor = np.float32(np.log(np.float64(np.float32(1e-5))))
    for name in ("l7", "l17"):
        x = clip_signal(g, name)
        for entry in ("spec_to_mel_torch", "mel_spectrogram_torch"):
            if entry == "spec_to_mel_torch":
                spec = _single(x, n_fft, hop)
                dev = MP.spec_to_mel_torch(torch.from_numpy(spec).to(DEV)[None], n_fft, n_mels, sr, 0.0, None)[0].cpu().numpy()
            else:
                spec = _single(x, n_fft, hop, eps=0.0, clamp=False)       # what the entry computes inside (bit-identical: same kernel, same clip)
                dev = MP.mel_spectrogram_torch(torch.from_numpy(x).to(DEV)[None, None], n_fft, n_mels, sr, hop, n_fft, 0.0, None)[0].cpu().numpy()
            assert dev.shape == (n_mels, x.shape[0] // hop) and dev.dtype == np.float32
            ref = _mel_f64(w, spec)
            cpu = torch.log(torch.clamp(torch.matmul(torch.from_numpy(np.array(w)), torch.from_numpy(spec)), min=1e-5)).numpy()
            err_dev, err_cpu = float(np.abs(dev - ref).max()), float(np.abs(cpu - ref).max())
            gate = max(4 * err_cpu, 2e-6)
            print(f"mel {n_mels}/{n_fft} {name} {entry}: err_dev {err_dev:.3e} err_torch {err_cpu:.3e} gate {gate:.3e}")
            _record(f"mel{n_mels}_{n_fft}_{name}_{entry}", {"err_dev": err_dev, "err_torch": err_cpu})
            assert err_dev <= gate, (name, entry, err_dev, err_cpu)
    # silent frames: the floor, exactly log(1e-5f) rounded to fp32, through both entries
    z = torch.zeros(1, 1, 3 * hop + 1, device=DEV)
    m = MP.mel_spectrogram_torch(z, n_fft, n_mels, sr, hop, n_fft, 0.0, None).cpu().numpy()
    assert m.shape == (1, n_mels, 3) and np.all(m == floor)
    m2 = MP.spec_to_mel_torch(torch.zeros(n_fft // 2 + 1, FRAMES_PER_WG * 4 + 1, device=DEV), n_fft, n_mels, sr, 0.0, None).cpu().numpy()
    assert m2.shape == (n_mels, FRAMES_PER_WG * 4 + 1) and np.all(m2 == floor)


def test_mel_ragged_batch_leaves_gaps():
    MP = _mp()
    n_fft, hop, sr = GEOMETRIES[0]
    spec = torch.rand(n_fft // 2 + 1, 150, device=DEV)
    cols = np.array([[3, 70], [80, 1], [100, 65]], dtype=np.int64)
    out = torch.full((80, 210), float("nan"), device=DEV)
    with pytest.raises(Exception):
        MP.mel_packed(spec, cols, n_fft, 80, sr, 0.0, None, out=out)        # the last clip ends beyond the spectrogram's row
    spec = torch.rand(n_fft // 2 + 1, 210, device=DEV)
    MP.mel_packed(spec, cols, n_fft, 80, sr, 0.0, None, out=out)
    got = out.cpu().numpy()
    used = np.zeros(210, dtype=bool)
    for c, n in cols:
        used[c:c + n] = True
    assert np.all(np.isnan(got[:, ~used])) and not np.any(np.isnan(got[:, used]))
    whole = MP.mel_packed(spec, np.array([[0, 210]], dtype=np.int64), n_fft, 80, sr, 0.0, None).cpu().numpy()
    assert np.array_equal(got[:, used], whole[:, used])


def test_cache_and_loader(tmp_path):
    from scipy.io import wavfile
    from comfy_rvc_amd import synthetic as S
    from comfy_rvc_amd.lib.train import data_utils as DU
    from comfy_rvc_amd.lib.train.utils import HParams
    from comfy_rvc_amd.preprocessing_utils import cache_spectrograms_trainset
    n_fft, hop, sr = GEOMETRIES[1]
    lengths = (825, 3 * hop, 7 * hop + 123, 17 * hop + 5, 5 * hop + 1)       # (every clip longer than the 824 samples of reflect padding, as torch requires)

    def make(root):
        os.makedirs(os.path.join(root, "0_gt_wavs"))
        xs = {}
        for i, n in enumerate(lengths):
            xs[f"{i}_0"] = S.spec_test_signal(sr, n, 50 + i)
            wavfile.write(os.path.join(root, "0_gt_wavs", f"{i}_0.wav"), sr, xs[f"{i}_0"])
        return xs

    root = str(tmp_path / "exp")
    xs = make(root)
    assert cache_spectrograms_trainset(root, sr, DEV) == 5
    blobs = {}
    for name, x in xs.items():
        path = os.path.join(root, "0_gt_wavs", f"{name}.spec.pt")
        t = torch.load(path)
        assert t.device.type == "cpu" and t.dtype == torch.float32 and t.shape == (n_fft // 2 + 1, x.shape[0] // hop) and t.is_contiguous()
        assert np.array_equal(t.numpy(), _single(x, n_fft, hop)), name
        blobs[name] = open(path, "rb").read()
    assert cache_spectrograms_trainset(root, HParams(sampling_rate=sr, filter_length=n_fft, hop_length=hop, win_length=n_fft), DEV) == 0
    for name in xs:
        assert open(os.path.join(root, "0_gt_wavs", f"{name}.spec.pt"), "rb").read() == blobs[name]
    # two ranks: disjoint, complete
    root2 = str(tmp_path / "exp2")
    make(root2)
    sets = []
    for rank in (0, 1):
        before = set(os.listdir(os.path.join(root2, "0_gt_wavs")))
        n = cache_spectrograms_trainset(root2, sr, DEV, rank=rank, world=2)
        new = set(os.listdir(os.path.join(root2, "0_gt_wavs"))) - before
        assert len(new) == n
        sets.append(new)
    assert not (sets[0] & sets[1]) and sets[0] | sets[1] == {f"{k}.spec.pt" for k in xs} and len(sets[0]) == 3
    # the loader computes a missing spectrogram on the device, caches it, and returns the reference's 6-tuple cut to the common length
    g = golden("train_loader_cases.npz")
    root3 = str(tmp_path / "exp3")
    filelist = S.write_train_filelist(root3)
    ds = DU.TextAudioLoaderMultiNSFsid(filelist, HParams(max_wav_value=32768.0, sampling_rate=sr, filter_length=n_fft, hop_length=hop, win_length=n_fft))
    assert np.array_equal(np.array(ds.lengths), g["lengths"])
    for i in (1, 3, 6):
        item = ds[i]
        spec, wav, phone, pitch, pitchf, sid = item
        sizes = [spec.shape[0], spec.shape[1], wav.shape[1], phone.shape[0], phone.shape[1], pitch.shape[0], pitchf.shape[0], int(sid)]
        assert sizes == g["item_sizes"][i].tolist(), (i, sizes)
        assert spec.device.type == "cpu" and spec.dtype == torch.float32
        cached = torch.load(os.path.join(root3, "0_gt_wavs", f"{i}_0.spec.pt"))
        full = _single(wavfile.read(os.path.join(root3, "0_gt_wavs", f"{i}_0.wav"))[1], n_fft, hop)
        assert np.array_equal(cached.numpy(), full) and np.array_equal(spec.numpy(), full[:, :spec.shape[1]])
        again = ds[i]
        assert all(torch.equal(a, b) for a, b in zip(item, again))
