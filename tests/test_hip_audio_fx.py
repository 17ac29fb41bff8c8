"""GPU: the audio nodes on the device (csrc/audio_fx.hip, lib/audio_fx.py, lib/audio.py::AudioProcessor, custom_nodes/audio_nodes.py) against scipy /
numpy computed on the test's own inputs and against the reference's results (tests/golden/audio_fx_cases.npz).

Normalise tolerance: the reference subtracts a float32 np.mean.  d = max |reference formula in float32 - the same formula in float64| is measured
with numpy on the test's own input (the reference against itself); the device may differ from the golden by 2 d plus one float32 ulp of the peak.
Measured d (numpy, on the host): 8.14e-08 (n = 4099), 7.09e-08 (n = 20011), for a peak of 0.891 whose float32 ulp is 5.96e-08; the chain test
prints its own d (its input to the normalise step comes from the device)."""
import numpy as np
import pytest
import torch

from test_audio_fx_host import DECLICK_CASES, GATE_CASES, assert_gate_well_posed, cases, declick_signal, gate_signal
from comfy_rvc_amd import synthetic as S

pytestmark = pytest.mark.gpu


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float32)))


def norm_ref(x, db=-1.0):
    """(the reference's float32 steps, the same formula in float64)"""
    a = x.astype(np.float32).copy()
    a -= np.mean(a)
    peak = np.max(np.abs(a))
    if peak > 0:
        a /= peak
        a *= 10 ** (db / 20)
    b = x.astype(np.float64)
    b = b - b.mean()
    pk = np.abs(b).max()
    if pk > 0:
        b = b / pk * 10 ** (db / 20)
    return a, b


# ------------------------------------------------------------------------------------------------------------- click removal
@pytest.mark.parametrize("case", DECLICK_CASES)
def test_declick_mask_and_fills(case):
    """Mask equal to scipy's on the same input and to the golden; median fill bit-equal; interpolation fill within 1 float32 ulp of the golden."""
    import hashlib
    from scipy.ndimage import uniform_filter1d
    from comfy_rvc_amd.lib.audio_fx import declick
    g = cases()
    x, size, ksize, mult, gmask = declick_signal(case)
    n = x.shape[0]
    ill = g[f"dc_{case}_illposed"]
    keep = np.ones(n, dtype=bool)
    keep[ill] = False
    smask = np.abs(x) > mult * np.sqrt(uniform_filter1d(np.square(x), size=size))
    assert np.array_equal(smask, gmask)
    med, mask = declick(x, multiplier=mult, sample_size=size, method="median", kernel_size=ksize, return_mask=True)
    mask, med = mask.cpu().numpy().astype(bool), med.cpu().numpy()
    print(f"{case}: n={n} size={size} kernel={ksize} clicks={int(gmask.sum())} mask differences={int((mask != smask).sum())} ill-posed={ill.size}")
    assert np.array_equal(mask[keep], smask[keep])
    assert med.dtype == np.float32 and np.array_equal(med[~mask], x[~mask])
    both = mask & gmask
    assert np.array_equal(med[both].view(np.uint32), g[f"dc_{case}_median"][both[gmask]].view(np.uint32))
    if ill.size == 0:
        assert np.array_equal(np.frombuffer(hashlib.sha256(med.tobytes()).digest(), dtype=np.uint8), g[f"dc_{case}_sha_median"])
    itp, mask2 = declick(x, multiplier=mult, sample_size=size, method="interpolation", kernel_size=ksize, return_mask=True)
    itp = itp.cpu().numpy()
    assert np.array_equal(mask2.cpu().numpy().astype(bool), mask) and np.array_equal(itp[~mask], x[~mask])
    if ill.size == 0:
        want = g[f"dc_{case}_interp"]
        err = np.abs(itp[mask].astype(np.float64) - want.astype(np.float64))
        print(f"{case}: interpolation fill, worst error {float((err / ulp32(want)).max()):.2f} ulp")
        assert (err <= ulp32(want)).all()


def test_replace_clicks_with_a_given_mask():
    from comfy_rvc_amd.lib.audio import AudioProcessor
    g = cases()
    x, size, ksize, mult, gmask = declick_signal("edges")
    for method, key in (("median", "median"), ("interpolation", "interp")):
        y = AudioProcessor.replace_clicks(x, gmask, method=method, kernel_size=ksize)
        assert isinstance(y, np.ndarray) and np.array_equal(y[~gmask], x[~gmask])
        assert (np.abs(y[gmask].astype(np.float64) - g[f"dc_edges_{key}"]) <= (0 if method == "median" else ulp32(g[f"dc_edges_{key}"]))).all()


def test_declick_errors_launch_nothing():
    from comfy_rvc_amd import _lib as L
    from comfy_rvc_amd.lib.audio import AudioProcessor
    from comfy_rvc_amd.lib.audio_fx import declick
    x = S.slicer_test_signal(40000, 5)[:3999]
    with pytest.raises(ValueError):
        AudioProcessor.dynamic_thresholding(x, sample_size=4000)
    with pytest.raises(ValueError):
        declick(x[:3], sample_size=2, kernel_size=5)
    with pytest.raises(L.RvcHipError, match="kernel_size"):
        declick(x, sample_size=160, kernel_size=33)
    with pytest.raises(ValueError):
        declick(x, sample_size=160, method="mean")


# ------------------------------------------------------------------------------------------------------------- silence gate
@pytest.mark.parametrize("case", GATE_CASES)
def test_gate_equals_reference(case):
    """Range list equal to the golden; output bit-equal to the golden's ranges applied in numpy (and to the reference's output, by its SHA-256)."""
    import hashlib
    from comfy_rvc_amd.lib import audio_fx
    from comfy_rvc_amd.lib.karafan.audio_utils import Silent
    g = cases()
    assert_gate_well_posed(case)
    x, sr, thr = gate_signal(case)
    y, ranges, levels = audio_fx.silence_gate(x, sr, thr, return_ranges=True)
    ref_levels = g[f"gate_{case}_levels"]
    print(f"{case}: window levels vs the reference's, max difference {float(np.abs(levels[:ref_levels.shape[0]] - ref_levels).max()):.2e} dB")
    assert np.array_equal(ranges, g[f"gate_{case}_ranges"])
    fade = audio_fx.gate_params(sr)[2]
    want = x.copy()
    for b, e, kind in g[f"gate_{case}_ranges"]:
        if kind == 1:
            want[b:e] = 0.0
        else:
            want[b:e] *= np.linspace(1.0, 0.0, fade) if kind == 0 else np.linspace(0.0, 1.0, fade)
    y = y.cpu().numpy()
    assert y.dtype == np.float32 and np.array_equal(y.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(np.frombuffer(hashlib.sha256(y.tobytes()).digest(), dtype=np.uint8), g[f"gate_{case}_sha"])
    y2 = Silent(x[None, :], sr, thr)
    assert y2.shape == (1, x.shape[0]) and np.array_equal(y2[0], y)
    with pytest.raises(ValueError):
        Silent(np.stack([x, x]), sr, thr)


# ------------------------------------------------------------------------------------------------------------- normalise
@pytest.mark.parametrize("case", ["n4099", "n20011"])
def test_normalize_against_reference(case):
    from comfy_rvc_amd.lib.karafan.audio_utils import Normalize
    g = cases()
    sr, seed, start, n = (int(v) for v in g[f"norm_{case}_meta"])
    x = S.add_clicks(S.slicer_test_signal(sr, seed), seed)[0][start:start + n]
    a, b = norm_ref(x)
    gold = g[f"norm_{case}_out"]
    assert np.array_equal(a, gold)
    d = float(np.abs(a.astype(np.float64) - b).max())
    y = Normalize(x.copy(), threshold_dB=-1.0)
    tol = 2 * d + float(ulp32(np.abs(gold).max()))
    err = float(np.abs(y.astype(np.float64) - gold.astype(np.float64)).max())
    print(f"normalize {case}: d = {d:.3e}, device - golden = {err:.3e}, tolerance {tol:.3e}, peak {float(np.abs(y).max()):.6f}")
    assert y.dtype == np.float32 and y.shape == x.shape and err <= tol
    z = Normalize(np.zeros(1000, dtype=np.float32))
    assert not z.any()


# ------------------------------------------------------------------------------------------------------------- merge
def _tracks(k, nan=False):
    rng = np.random.default_rng(11 + k)
    lens = [100003, 65567, 4099, 70001][:k]
    t = [rng.standard_normal(n).astype(np.float32) for n in lens]
    if nan:
        t[0][[5, 4098, 70000]] = np.nan
        for a in t[:3]:
            a[17] = np.nan                     # NaN in every track that reaches the column ...
        if k == 4:
            t[3][17] = np.nan                  # ... including the fourth: an all-NaN column
        t[1][[5, 9]] = np.nan
    return t


@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("k", [2, 3, 4])
def test_merge_against_numpy(k, nan):
    import warnings
    from comfy_rvc_amd.lib.audio import pad_audio
    from comfy_rvc_amd.lib.audio_fx import merge_tracks
    tracks = _tracks(k, nan)
    stack = pad_audio(*tracks, axis=0)
    if nan and k == 4:
        assert np.isnan(stack[:, 17]).all()
    for mode, fn in (("min", np.nanmin), ("max", np.nanmax), ("median", np.nanmedian), ("mean", np.nanmean)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = fn(stack, axis=0)
        y = merge_tracks(tracks, mode).cpu().numpy()
        assert y.dtype == ref.dtype == np.float32 and y.shape == ref.shape == (100003,)
        assert np.array_equal(np.isnan(y), np.isnan(ref)), mode
        ok = ~np.isnan(ref)
        if mode == "mean":
            assert (np.abs(y[ok].astype(np.float64) - ref[ok]) <= ulp32(ref[ok])).all()
        else:
            assert np.array_equal(y[ok], ref[ok]), (mode, int((y[ok] != ref[ok]).sum()))


def test_merge_audio_and_node():
    """lib merge_audio (mean + limiter) against numpy; MergeAudioNode of a 40 kHz and a 48 kHz track: AUDIO layout [1, N, 1] at 40 kHz."""
    from comfy_rvc_amd.custom_nodes.audio_nodes import MergeAudioNode
    from comfy_rvc_amd.custom_nodes.rvc_nodes import to_audio_dict
    from comfy_rvc_amd.lib.audio import bytes_to_audio, merge_audio, pad_audio, remix_audio
    a = S.slicer_test_signal(40000, 5)[30000:80000] * np.float32(3.5)
    b = S.slicer_test_signal(40000, 6)[30000:70001] * np.float32(3.5)
    y, sr = merge_audio((a, 40000), (b, 40000), sr=40000)
    m = np.nanmean(pad_audio(remix_audio((a, 40000))[0], remix_audio((b, 40000))[0], axis=0), axis=0)
    assert sr == 40000 and y.dtype == np.float32 and (np.abs(y.astype(np.float64) - m) <= ulp32(m)).all()      # a mean of limited tracks stays below the limit
    from comfy_rvc_amd.lib.audio_fx import peak_limit_
    for scale in (1.0, 3.5):                                            # below the limit: untouched; above: remix_audio's float32 division
        t = a / np.float32(3.5) * np.float32(scale)
        lim = remix_audio((t, 40000))[0]
        assert (np.abs(t).max() > .95) == (scale > 1) and np.array_equal(peak_limit_(torch.from_numpy(t).cuda(), .95).cpu().numpy(), lim)
    c = S.slicer_test_signal(48000, 7)[40000:100001]
    out = MergeAudioNode().merge(to_audio_dict(a / np.float32(3.5), 40000), lambda: (c, 48000), sr="None", merge_type="median", normalize=True)
    vhs, audio = out["result"]
    n = max(a.shape[0], int(np.ceil(c.shape[0] * 40000 / 48000)))
    assert audio["sample_rate"] == 40000 and tuple(audio["waveform"].shape) == (1, n, 1) and audio["waveform"].dtype == torch.float32
    back, rate = bytes_to_audio(vhs())
    assert rate == 40000 and back.shape == (n,) and out["ui"]["preview"][0]["filename"].endswith(".wav")


# ------------------------------------------------------------------------------------------------------------- segment energy, batch values
@pytest.mark.parametrize("k", [2, 7, 256])
def test_segment_energy_against_numpy(k):
    from comfy_rvc_amd.lib.audio_fx import segment_energy
    rng = np.random.default_rng(3)
    x = rng.integers(-32768, 32768, size=100003, dtype=np.int64).astype(np.int16)
    x[:5] = [-32768, 32767, -32768, 0, 1]
    assert x.shape[0] % k != 0
    ref = np.array([np.sum(p.astype(np.int64) ** 2) for p in np.array_split(x, k)], dtype=np.int64)
    y = segment_energy(x, k)
    assert y.dtype == np.int64 and np.array_equal(y, ref)


def test_batch_values_equal_reference():
    from comfy_rvc_amd.custom_nodes.audio_nodes import AudioBatchValueNode
    g = cases()
    sr, seed, n, k, thr = (int(v) for v in g["batch_meta"])
    x = S.slicer_test_signal(sr, seed, (("s", 1.7), ("v", 1.2), ("s", 0.7), ("v", 1.1)))
    assert x.shape == (n,)
    lo, hi = (float(v) for v in g["batch_range"])
    for norm in ("scale", "tanh", "sigmoid"):
        for inverse in (False, True):
            f, i, nv = AudioBatchValueNode().get_frame_weights((x, sr), k, lo, hi, norm, silence_threshold=thr, inverse=inverse)
            want = g[f"batch_{norm}_{int(inverse)}_float"]
            assert np.abs(want - np.round(want)).min() > 1e-9
            assert nv == k and np.allclose(np.array(f), want, rtol=1e-12, atol=0) and list(i) == list(g[f"batch_{norm}_{int(inverse)}_int"])


# ------------------------------------------------------------------------------------------------------------- chain, nodes
def _chain_signal():
    g = cases()
    sr, seed, n = (int(v) for v in g["chain_meta"])
    x = S.slicer_test_signal(sr, seed, tuple((str(k), float(s)) for k, s in zip(g["chain_seg_kind"], g["chain_seg_seconds"])))
    x[g["chain_clicks"]] = np.float32(0.5)
    assert x.shape == (n,)
    return x, sr


def test_audio_processor_chain_equals_reference():
    """AudioProcessor() with defaults: gate and median fill are bit-equal steps, so the end-to-end output carries the normalise tolerance alone."""
    from comfy_rvc_amd.custom_nodes.audio_nodes import ProcessAudioNode
    from comfy_rvc_amd.custom_nodes.rvc_nodes import to_audio_dict
    from comfy_rvc_amd.lib import audio_fx
    from comfy_rvc_amd.lib.audio import AudioProcessor
    g = cases()
    x, sr = _chain_signal()
    gold = g["chain_out"]
    pre = audio_fx.declick(audio_fx.silence_gate(x, sr, -50), multiplier=2.0, sample_size=16000, method="median", kernel_size=5).cpu().numpy()
    assert not pre[:16000].any() and not np.array_equal(pre, x)
    a, b = norm_ref(pre, -1)
    d = float(np.abs(a.astype(np.float64) - b).max())
    tol = 2 * d + float(ulp32(np.abs(gold).max()))
    for y, rate in (AudioProcessor()((x, sr)), AudioProcessor()(x, sr), AudioProcessor()(to_audio_dict(x, sr))):
        err = float(np.abs(y.astype(np.float64) - gold.astype(np.float64)).max())
        print(f"chain: d = {d:.3e}, device - golden = {err:.3e}, tolerance {tol:.3e}")
        assert rate == sr and y.dtype == np.float32 and y.shape == gold.shape and err <= tol
    proc, vhs, audio = ProcessAudioNode().process_audio(True, True, True, audio=to_audio_dict(x, sr))
    assert isinstance(proc, AudioProcessor) and proc.sample_size == 16000 and tuple(audio["waveform"].shape) == (1, x.shape[0], 1)
    assert np.array_equal(audio["waveform"][0, :, 0].numpy(), y) and callable(vhs)
    proc2, none_a, none_b = ProcessAudioNode().process_audio(False, True, False)
    assert str(proc2) == str(AudioProcessor(normalize=False, dynamic_threshold=False)) and none_a is None and none_b is None


def test_preprocess_with_audio_processor(tmp_path):
    """Preprocess(..., preprocessor=AudioProcessor()) cuts the windows that the processor's output, written out and preprocessed plainly, gives."""
    import os
    from scipy.io import wavfile
    from comfy_rvc_amd.lib.audio import AudioProcessor
    from comfy_rvc_amd.preprocessing_utils import Preprocess
    x = S.slicer_test_signal(40000, 5, (("s", 1.7), ("v", 3.2), ("s", 0.4)))
    wavfile.write(str(tmp_path / "a.wav"), 40000, x)
    processed, _ = AudioProcessor()(x, 40000)
    assert not np.array_equal(processed, x)
    wavfile.write(str(tmp_path / "b.wav"), 40000, processed)
    Preprocess(40000, str(tmp_path / "with"), preprocessor=AudioProcessor()).pipeline(str(tmp_path / "a.wav"), 0)
    Preprocess(40000, str(tmp_path / "plain")).pipeline(str(tmp_path / "b.wav"), 0)
    for sub in ("0_gt_wavs", "1_16k_wavs"):
        names = sorted(os.listdir(str(tmp_path / "with" / sub)))
        assert names and names == sorted(os.listdir(str(tmp_path / "plain" / sub)))
        for name in names:
            ra, da = wavfile.read(str(tmp_path / "with" / sub / name))
            rb, db = wavfile.read(str(tmp_path / "plain" / sub / name))
            assert ra == rb and np.array_equal(da, db), (sub, name)
    assert "->Suc." in open(str(tmp_path / "with" / "preprocess.log")).read()


def test_audio_info_node():
    from comfy_rvc_amd.custom_nodes.audio_nodes import AudioInfoNode
    x = S.slicer_test_signal(16000, 1, (("v", 0.5),))
    vhs, audio, seconds, sr = AudioInfoNode().get_info(lambda: (x, 16000))
    assert seconds == 0.5 and sr == 16000 and tuple(audio["waveform"].shape) == (1, 8000, 1) and vhs()[:4] == b"RIFF"
