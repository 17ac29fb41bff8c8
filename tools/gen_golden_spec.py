"""Writes tests/golden/spec_cases.npz and tests/golden/train_loader_cases.npz: what the REFERENCE's lib/train makes of this project's synthetic inputs.

Build container only (needs the reference tree: RVC_REFERENCE_ROOT; no test and no GPU job runs this).  The reference's lib/train/mel_processing.py,
utils.py and data_utils.py are loaded by path at run time as a scratch package; `librosa.filters.mel`, which they import and which is not installed
here, is stubbed by this project's mel_filterbank (no golden value depends on it: the spectrogram and the loaders never call it).

spec_cases.npz: per case `{case}` = float32 [n_fft / 2 + 1, n // hop], the reference's spectrogram_torch (torch.stft on the CPU, fp32) of
synthetic.spec_test_signal(sr, n, seed), and `{case}_meta` = int64 (n_fft, hop, sr, n, seed).  No audio: the tests regenerate the signals.
train_loader_cases.npz: synthetic.train_loader_summary of the reference's loaders, collates and samplers over synthetic.write_train_filelist.
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from comfy_rvc_amd import synthetic as S   # noqa: E402

GEOMETRIES = ((1024, 320, 32000), (2048, 400, 40000), (2048, 480, 48000))


def spec_cases():
    """name -> (n_fft, hop, sr, n, seed): per geometry the shortest legal clip and 7 hop + 123 samples."""
    cases = {}
    for g, (n_fft, hop, sr) in enumerate(GEOMETRIES):
        cases[f"g{n_fft}_{hop}_min"] = (n_fft, hop, sr, (n_fft - hop) // 2 + 1, 10 + g)
        cases[f"g{n_fft}_{hop}_l7"] = (n_fft, hop, sr, 7 * hop + 123, 20 + g)
    return cases


def load_reference_train():
    ref_root = os.environ.get("RVC_REFERENCE_ROOT")
    if not ref_root:
        raise SystemExit("set RVC_REFERENCE_ROOT to the reference tree")
    from comfy_rvc_amd.lib.train.mel_processing import mel_filterbank
    if "librosa" not in sys.modules:
        librosa = types.ModuleType("librosa")
        filters = types.ModuleType("librosa.filters")
        filters.mel = lambda sr, n_fft, n_mels, fmin, fmax: np.array(mel_filterbank(sr, n_fft, n_mels, fmin, fmax))
        librosa.filters = filters
        sys.modules["librosa"], sys.modules["librosa.filters"] = librosa, filters
    pkg = types.ModuleType("ref_train")
    pkg.__path__ = [os.path.join(ref_root, "lib", "train")]
    sys.modules["ref_train"] = pkg
    mods = {}
    for name in ("mel_processing", "utils", "data_utils"):
        spec = importlib.util.spec_from_file_location(f"ref_train.{name}", os.path.join(ref_root, "lib", "train", f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"ref_train.{name}"] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


def main():
    mods = load_reference_train()
    out = {}
    for case, (n_fft, hop, sr, n, seed) in spec_cases().items():
        x = torch.from_numpy(S.spec_test_signal(sr, n, seed))[None]
        spec = mods["mel_processing"].spectrogram_torch(x, n_fft, hop, n_fft, center=False)[0]
        assert spec.shape == (n_fft // 2 + 1, n // hop), spec.shape
        out[case] = spec.numpy().astype(np.float32)
        out[f"{case}_meta"] = np.array([n_fft, hop, sr, n, seed], dtype=np.int64)
        print(case, tuple(spec.shape))
    path = os.path.join(ROOT, "tests", "golden", "spec_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")

    hp = mods["utils"].HParams(max_wav_value=32768.0, sampling_rate=40000, filter_length=2048, hop_length=400, win_length=2048)
    with tempfile.TemporaryDirectory() as tmp:
        filelist = S.write_train_filelist(tmp)
        S.write_nof0_filelist(filelist)
        summary = S.train_loader_summary(mods["data_utils"], filelist, hp)
    path = os.path.join(ROOT, "tests", "golden", "train_loader_cases.npz")
    np.savez_compressed(path, **summary)
    print("wrote", path, os.path.getsize(path), "bytes")
    for k in ("lengths", "item_sizes", "dist_2_1_batches", "dist_1_0_boundaries", "dist_1_0_num_samples_per_bucket"):
        print(k, summary[k].tolist())


if __name__ == "__main__":
    main()
