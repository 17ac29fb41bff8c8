"""GPU: dataset preparation on the device (csrc/dataset_prep.hip, lib/dataset_prep.py, Preprocess, RVCProcessDatasetNode) against scipy, against
the reference's slicer (tests/golden/slicer_cases.npz) and, bit for bit, against this repository's per-window route.

Filter tolerance: scipy.signal.lfilter(bh, ah, x) (what the reference runs) is ill-conditioned at these rates; d = max|lfilter - sosfilt| /
max|lfilter| is measured with scipy on the test's own input (the reference against itself) and the device may differ from lfilter by 4 d (a third
rounding order) and from sosfilt - the same cascade arithmetic - by 1e-11, both relative to the output's peak."""
import json
import os

import numpy as np
import pytest
import torch

from test_dataset_prep_host import CASES, assert_well_posed, case_meta, case_signal, cases
from comfy_rvc_amd import synthetic as S

pytestmark = pytest.mark.gpu
FULL = [c for c in CASES if c != "tiny_40k"]
_memo = {}


def scipy_refs(case):
    """(lfilter, sosfilt, d) of the case's recording, computed once."""
    if ("ref", case) not in _memo:
        from scipy import signal
        sr = case_meta(case)[0]
        x = case_signal(case).astype(np.float64)
        bh, ah = signal.butter(N=5, Wn=48, btype="high", fs=sr)
        tf = signal.lfilter(bh, ah, x)
        so = signal.sosfilt(signal.butter(N=5, Wn=48, btype="high", fs=sr, output="sos"), x)
        _memo["ref", case] = (tf, so, float(np.abs(tf - so).max() / np.abs(tf).max()))
    return _memo["ref", case]


def device_filtered(case, scale=1.0):
    if ("filt", case, scale) not in _memo:
        from comfy_rvc_amd.lib.dataset_prep import lfilter_hp
        x = case_signal(case)
        if scale != 1.0:
            x = (x * np.float32(scale)).astype(np.float32)
        _memo["filt", case, scale] = lfilter_hp(torch.from_numpy(x).cuda(), case_meta(case)[0])
    return _memo["filt", case, scale]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case,n", [("r32k_s1", None), ("r40k_s0", None), ("r48k_s0", None),
                                    ("r40k_s0", 100003),            # neither a multiple of the 256-sample block nor of the 32-sample tile
                                    ("r48k_s0", 65536 + 31),        # one group of 256 blocks and a little: the group chain has two links
                                    ("r40k_s0", 100)])              # shorter than one block
def test_lfilter_hp_against_scipy(case, n, dtype):
    from scipy import signal
    from comfy_rvc_amd.lib.dataset_prep import lfilter_hp
    sr = case_meta(case)[0]
    if n is None:
        x = case_signal(case)
        tf, so, d = scipy_refs(case)
    else:
        x = case_signal(case)[25000:25000 + n]              # from inside the leading silence into the first voiced stretch
        bh, ah = signal.butter(N=5, Wn=48, btype="high", fs=sr)
        tf = signal.lfilter(bh, ah, x.astype(np.float64))
        so = signal.sosfilt(signal.butter(N=5, Wn=48, btype="high", fs=sr, output="sos"), x.astype(np.float64))
        d = float(np.abs(tf - so).max() / np.abs(tf).max())
    y = lfilter_hp(torch.from_numpy(x.astype(dtype)).cuda(), sr)
    assert y.dtype == torch.float64 and y.shape == (x.shape[0],)
    y = y.cpu().numpy()
    e_tf, e_so = float(np.abs(y - tf).max() / np.abs(tf).max()), float(np.abs(y - so).max() / np.abs(so).max())
    print(f"lfilter_hp sr={sr} n={x.shape[0]} {np.dtype(dtype).name}: d={d:.3e} device-lfilter={e_tf:.3e} device-sosfilt={e_so:.3e}")
    assert e_so <= 1e-11
    assert e_tf <= 4 * d


@pytest.mark.parametrize("case", FULL)
def test_frame_rms_against_numpy(case):
    from comfy_rvc_amd.lib.dataset_prep import frame_rms, slicer_params
    sp = slicer_params(case_meta(case)[0])
    win, hop = sp["win_size"], sp["hop_size"]
    filt = device_filtered(case)
    rms = frame_rms(filt, win, hop).cpu().numpy()
    y = np.pad(filt.cpu().numpy(), (win // 2, win // 2))
    nf = (y.shape[0] - win) // hop + 1
    ref = np.sqrt(np.mean(np.lib.stride_tricks.sliding_window_view(y, win)[::hop] ** 2, axis=1))
    assert rms.shape == ref.shape == (nf,) and nf == cases()[f"{case}_rms"].shape[0]
    err = float(np.abs(rms / ref - 1.0).max())
    print(f"frame_rms {case}: {nf} frames, max relative error {err:.3e}")
    assert err <= 1e-12


def test_frame_rms_rejects_wrong_frame_count():
    from comfy_rvc_amd import _lib as L
    y = torch.zeros(1000, dtype=torch.float64, device="cuda")
    out = torch.zeros(64, dtype=torch.float64, device="cuda")
    assert L.lib.rvc_frame_rms(L.current_stream(), L.ptr(y), 1000, 64, 16, L.ptr(out), 64) != 0      # (1000 + 64 - 64) / 16 + 1 = 63


@pytest.mark.parametrize("case", list(CASES))
def test_filter_rms_tags_windows_equal_reference(case):
    """Recording -> filter -> RMS -> tags on the device path: tags and chunk bounds equal to the reference's; the float32 windows within 4 d of the
    reference's (lfilter, the golden bounds, float32)."""
    from comfy_rvc_amd.lib.dataset_prep import chunk_bounds, cut_windows, frame_rms, slice_tags, slicer_params
    assert_well_posed(case)
    g = cases()
    sr, _, _, n = case_meta(case)
    sp = slicer_params(sr)
    filt = device_filtered(case)
    tags, nf = np.zeros((0, 2), dtype=np.int64), 0
    if n > sp["min_length"]:
        rms = frame_rms(filt, sp["win_size"], sp["hop_size"]).cpu().numpy()
        nf = rms.shape[0]
        print(f"{case}: device RMS vs the reference's RMS list, max relative difference {float(np.abs(rms / g[case + '_rms'] - 1).max()):.3e}")
        tags = slice_tags(rms, n, sp)
    assert np.array_equal(tags, g[f"{case}_tags"])
    chunks = chunk_bounds(tags, nf, sp["hop_size"], n)
    assert np.array_equal(np.array(chunks, dtype=np.int64).reshape(-1, 2), g[f"{case}_chunks"])
    tf, _, d = scipy_refs(case)
    wins = [(int(s), int(l)) for s, l, _, _ in g[f"{case}_windows"] if l > 0]
    gt, _ = cut_windows(filt, wins, sr, 0.95)
    worst = 0.0
    for (s, l), a in zip(wins, gt):
        assert a.dtype == np.float32 and a.shape == (l,)
        worst = max(worst, float(np.abs(a.astype(np.float64) - tf[s:s + l].astype(np.float32)).max()))
    print(f"{case}: gt windows vs reference windows {worst / np.abs(tf).max():.3e} of the peak, d = {d:.3e}")
    # (the float32 cast of either side adds at most half a float32 ulp of the peak: 6e-8, inside 4 d at every rate used here)
    assert worst <= 4 * d * np.abs(tf).max()


@pytest.mark.parametrize("max_volume", [0.95, 1.0])
@pytest.mark.parametrize("case,scale", [("r40k_s0", 1.0), ("r40k_s0", 4.0), ("r48k_s0", 1.0), ("r32k_s1", 1.0), ("short_sil_40k", 1.0)])
def test_cut_windows_16k_bit_identical_to_per_window_route(case, scale, max_volume):
    """Every 16 kHz window equals remix_audio((window_f32, sr), target_sr=16000, max_volume=v) of this repository bit for bit: the reference's
    windows of the case (with the 46 800-sample remainder at 40 kHz), a window of one sample, odd lengths and starts, the recording's first and
    last samples; scale 4 puts the voiced peaks (1.2) above max_volume so that the limiter divides."""
    from comfy_rvc_amd.lib.audio import remix_audio
    from comfy_rvc_amd.lib.dataset_prep import cut_windows
    sr, _, _, n = case_meta(case)
    filt = device_filtered(case, scale)
    wins = [(int(s), int(l)) for s, l, _, _ in cases()[f"{case}_windows"]]
    wins += [(60001, 1), (0, 4097), (n - 777, 777), (70003, 12345), (5, 0)]
    if case == "r40k_s0":
        assert (540600, 46800) in wins
    gt, y16 = cut_windows(filt, wins, sr, max_volume)
    host = filt.cpu().numpy()
    limited = 0
    for (s, l), a, b in zip(wins, gt, y16):
        assert np.array_equal(a, host[s:s + l].astype(np.float32))
        if l == 0:
            assert b.shape == (0,)
            continue
        ref, rate = remix_audio((a, sr), target_sr=16000, max_volume=max_volume)
        assert rate == 16000 and b.dtype == ref.dtype == np.float32 and b.shape == ref.shape == (int(np.ceil(l * 16000.0 / sr)),)
        assert np.array_equal(b, ref), (s, l, float(np.abs(b - ref).max()))
        limited += int(np.abs(b).max() >= np.float32(max_volume) * np.float32(1 - 1e-6) and scale > 1)
    assert (limited > 0) == (scale > 1)


def _write_models(models):
    as_t = lambda sd: {k: torch.as_tensor(np.ascontiguousarray(v)).clone() for k, v in sd.items()}   # noqa: E731
    os.makedirs(models, exist_ok=True)
    torch.save(as_t(S.rmvpe_state_dict(0)), os.path.join(models, "rmvpe.pt"))


def test_dataset_end_to_end(tmp_path, monkeypatch):
    """Two 40 kHz recordings -> preprocess_trainset (names, rates and lengths of the reference) -> extract_features_trainset (procedural HuBERT /
    RMVPE weights) -> RVCProcessDatasetNode.process (filelist, mute set, returned dict, cache)."""
    from scipy.io import wavfile
    import comfy_rvc_amd.lib as lib
    import comfy_rvc_amd.pitch_extraction as pe
    from comfy_rvc_amd.custom_nodes import rvc_nodes as N
    from comfy_rvc_amd.lib.infer_pack.loaders import HubertModelWithFinalProj
    from comfy_rvc_amd.preprocessing_utils import extract_features_trainset, preprocess_trainset
    g = cases()
    _write_models(str(tmp_path / "models"))
    for mod in (lib, pe, N):
        monkeypatch.setattr(mod, "BASE_MODELS_DIR", str(tmp_path / "models"), raising=False)
    monkeypatch.setattr(N, "INPUT_DIR", str(tmp_path / "input"))
    monkeypatch.setattr(N, "OUTPUT_DIR", str(tmp_path / "output"))
    rec = tmp_path / "input" / "datasets" / "voice"
    rec.mkdir(parents=True)
    used = ("r40k_s0", "short_sil_40k")                              # idx0 0 and 1: the files are taken in sorted order
    for name, case in zip(("a.wav", "b.wav"), used):
        assert case_meta(case)[2] == ("a.wav", "b.wav").index(name)
        wavfile.write(str(rec / name), 40000, case_signal(case))     # IEEE-float WAV: the samples survive exactly
    # the file each name ends up holding: the LAST written window of that number
    want = {}
    for case in used:
        for s, l, idx1, written in g[f"{case}_windows"]:
            if written:
                want[f"{case_meta(case)[2]}_{idx1}.wav"] = int(l)
    assert sorted(want) == sorted(f"{v}.wav" for case in used for v in g[f"{case}_names"]) and len(want) == 6
    exp = tmp_path / "exp"
    assert preprocess_trainset(str(rec), 40000, 2, str(exp), None, 3.0, .3, 1.) is True
    for sub, rate in (("0_gt_wavs", 40000), ("1_16k_wavs", 16000)):
        assert sorted(os.listdir(str(exp / sub))) == sorted(want)
        for name, l in want.items():
            r, data = wavfile.read(str(exp / sub / name))
            assert r == rate and data.dtype == np.float32 and data.shape == (int(np.ceil(l * rate / 40000.0)),), (sub, name)
    log = open(str(exp / "preprocess.log")).read().split("\n")
    assert log[0] == "start preprocess" and sorted(ln for ln in log if ln.endswith("->Suc.")) == [f"{rec}/a.wav->Suc.", f"{rec}/b.wav->Suc."]
    assert "end preprocess" in log

    hub = HubertModelWithFinalProj(S.hubert_state_dict(0), S.HUBERT_CONFIG)
    assert extract_features_trainset(hub, str(exp), 1, "rmvpe", "cuda:0", "v2", True, 160) is True
    for sub, suffix in (("2a_f0", ".wav.npy"), ("2b-f0nsf", ".wav.npy"), ("3_feature768", ".wav.npy")):
        assert sorted(os.listdir(str(exp / sub))) == sorted("rmvpe," + n[:-4] + suffix for n in want), sub
    feat = np.load(str(exp / "3_feature768" / "rmvpe,0_0.wav.npy"))
    assert feat.dtype == np.float32 and feat.shape == (149, 768)      # 48 000 samples at 16 kHz -> 149 HuBERT frames

    params = {"f0_method": "rmvpe", "crepe_hop_length": 160}
    thunk = lambda: hub   # noqa: E731
    node = N.RVCProcessDatasetNode()
    (pipe,) = node.process("voice-model", "voice", thunk, params, sr="40k", n_threads=1, period=3., overlap=.3, max_volume=1., mute_ratio=.0)
    assert sorted(pipe) == sorted(["sample_rate", "dataset_dir", "name", "training_files", "if_f0", "pitch_extraction_params", "hubert_model"])
    assert pipe["sample_rate"] == "40k" and pipe["name"] == "voice-model" and pipe["if_f0"] is True and pipe["hubert_model"] is thunk
    assert pipe["pitch_extraction_params"] is params
    assert pipe["dataset_dir"] == os.path.join(str(tmp_path / "output"), "dataset", N.get_hash("voice", 3., .3, 1., .0, "40k", "rmvpe", None))
    lines = open(pipe["training_files"]).read().split("\n")
    assert len(lines) == len(want) + 2
    for ln in lines:
        cols = ln.split("|")
        assert len(cols) == 5 and cols[4] == "0" and all(os.path.isfile(c) for c in cols[:4]), ln
    mute = [ln for ln in lines if os.sep + "mute" + os.sep in ln]
    assert len(mute) == 2 and mute[0].startswith(os.path.join(pipe["dataset_dir"], "mute", "0_gt_wavs", "mute40k.wav"))
    r, z = wavfile.read(mute[0].split("|")[0])
    assert r == 40000 and z.shape == (120000,) and not z.any()
    assert sorted(os.path.basename(ln.split("|")[0]) for ln in lines if ln not in mute) == sorted(want)
    stamp = os.stat(pipe["training_files"]).st_mtime_ns
    (pipe2,) = node.process("voice-model", "voice", thunk, params, sr="40k", n_threads=1, period=3., overlap=.3, max_volume=1., mute_ratio=.0)
    assert pipe2["training_files"] == pipe["training_files"] and os.stat(pipe["training_files"]).st_mtime_ns == stamp
    print(json.dumps({"clips": len(want), "filelist_lines": len(lines)}))


def test_dataset_node_reads_a_zip(tmp_path, monkeypatch):
    """A .zip under INPUT_DIR/datasets is extracted flat (directories inside the archive dropped) and processed like a folder; without a pitch method
    the list has gt|feature|0 lines."""
    import zipfile
    from scipy.io import wavfile
    from comfy_rvc_amd.custom_nodes import rvc_nodes as N
    from comfy_rvc_amd.lib.infer_pack.loaders import HubertModelWithFinalProj
    monkeypatch.setattr(N, "INPUT_DIR", str(tmp_path / "input"))
    monkeypatch.setattr(N, "OUTPUT_DIR", str(tmp_path / "output"))
    (tmp_path / "input" / "datasets").mkdir(parents=True)
    wavfile.write(str(tmp_path / "b.wav"), 40000, case_signal("short_sil_40k"))
    with zipfile.ZipFile(str(tmp_path / "input" / "datasets" / "set.zip"), "w") as z:
        z.write(str(tmp_path / "b.wav"), "some/dir/b.wav")
    hub = HubertModelWithFinalProj(S.hubert_state_dict(0), S.HUBERT_CONFIG)
    (pipe,) = N.RVCProcessDatasetNode().process("m", "set.zip", lambda: hub, {}, sr="40k")
    assert os.path.isfile(str(tmp_path / "input" / "datasets" / "set" / "b.wav")) and pipe["if_f0"] is False
    lines = open(pipe["training_files"]).read().split("\n")
    assert len(lines) == 2 + 2                                         # idx0 0: clips 0_1 and 0_2, and two mute lines
    for ln in lines:
        cols = ln.split("|")
        assert len(cols) == 3 and cols[2] == "0" and all(os.path.isfile(c) for c in cols[:2]), ln
