"""Writes tests/golden/audio_fx_cases.npz: what the REFERENCE's Silent, AudioProcessor, Normalize and AudioBatchValueNode make of the recordings of
synthetic.slicer_test_signal with the click recipe of synthetic.add_clicks.

Build container only (needs the reference tree, RVC_REFERENCE_ROOT; no test and no GPU job runs this).  The reference's lib/audio.py and
lib/karafan/audio_utils.py are imported through oracle/ref_shim.py, used as is; AudioBatchValueNode is loaded by path from the reference's
custom_nodes/audio_nodes.py with folder_paths, yt_dlp and the pack's own helper modules stubbed here.  The shim's librosa.feature.rms stand-in pads
every axis of a 2-D input and it has no amplitude_to_db, so this tool installs its own stand-ins for those two before it calls Silent: rms pads the
last axis only, amplitude_to_db follows librosa 0.10.2 (amin=1e-5, ref=1, top_db=80).  Both are restatements of published definitions and cannot
be checked against the real package here: parity unpinned beyond the definition.

The file holds recipes (signal segments, rate, seed, slice, forced clicks), not audio, plus expected results:
  dc_{case}_meta / _forced        int64 [sr, seed, start, n, size, ksize], positions of extra +0.5 clicks written after the recipe's
  dc_{case}_mult                  float64 multiplier
  dc_{case}_mask                  uint8 packbits of the click mask; dc_{case}_illposed int64 indices whose |x| is within 1e-4 of the threshold
  dc_{case}_median / _interp      float32 fill values at the click positions (the output equals the input everywhere else)
  dc_{case}_sha_median            SHA-256 of the whole float32 median output
  gate_{case}_meta                int64 [sr, seed, n, threshold_dB]; gate_{case}_segments the ("s" | "v", seconds) list as two arrays
  gate_{case}_levels / _ranges    float64 window levels (dB) as Silent saw them, int64 [n][3] (begin, end, kind 0 fade-out / 1 zero / 2 fade-in)
  gate_{case}_sha                 SHA-256 of Silent's float32 output
  norm_{case}_meta / _out         int64 [sr, seed, start, n], float32 Normalize output (threshold_dB -1)
  chain_meta / chain_out          the default AudioProcessor's output for a 16 kHz recording with three impulses (chain_clicks)
  hash_params / hash_values       three AudioProcessor parameter sets (JSON) and the reference's str() of each
  batch_*                         AudioBatchValueNode.get_frame_weights FLOAT / INT outputs for scale / tanh / sigmoid, with and without inverse
A case is refused where more than 0.1 % of its samples are ill-posed, where a window level lies within 1 % of the silence threshold, or where a
batch value lies within 1e-9 of an integer.
"""
import hashlib
import importlib
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from comfy_rvc_amd import synthetic as S   # noqa: E402

from oracle.ref_shim import REF_ROOT   # noqa: E402  (RVC_REFERENCE_ROOT, or the shim's default)
SR, SEED = 40000, 5
# name -> (start, n, size, ksize, forced click positions); the 40 kHz recording of seed 5 with its click recipe, sliced
DECLICK_CASES = {
    "full": (0, None, 4000, 5, ()),
    "n100003": (25000, 100003, 4000, 5, ()),            # not a multiple of any block or tile
    "n65567": (25000, 65536 + 31, 4001, 3, ()),         # two links in a scan's group chain; odd size
    "n4099": (33000, 4099, 160, 31, ()),                # the largest median window
    "n_eq_size": (34000, 4000, 4000, 5, ()),            # the RMS window reflects at both ends of every sample
    "edges": (0, 4099, 160, 5, (0, 4098) + tuple(range(2000, 2009))),   # clicks at both ends, a run of 9 > kernel_size
}
GATE_SEGMENTS = (("s", 1.7), ("v", 1.2), ("s", 0.7), ("v", 1.1), ("s", 2.3), ("v", 0.9), ("s", 1.9))
GATE_CASES = {
    "g40k": (40000, 5, GATE_SEGMENTS),                  # silence at the start, a short one, one in the middle, one at the end; last window short
    "g44k": (44100, 6, GATE_SEGMENTS[:-1]),             # ends loud
    "g16k_endexact": (16000, 7, (("v", 1.0), ("s", 2.0))),   # the last window is whole
}
CHAIN = (16000, 5, (("s", 1.7), ("v", 1.2), ("s", 0.4)))
CHAIN_CLICKS = (30000, 35001, 40002)                    # +0.5 impulses inside the voiced stretch
HASH_PARAMS = [{}, {"normalize": False, "sample_size": 4000, "fill_method": "interpolation", "kernel_size": 7},
               {"threshold_silence": False, "dynamic_threshold": False, "normalize_threshold_db": -3}]
BATCH = dict(num_segments=7, output_min=0.25, output_max=9.5, silence_threshold=1000)


def rms_last_axis(*, y, frame_length=2048, hop_length=512, center=True, pad_mode="constant"):
    """librosa.feature.rms (0.10.2) for a [..., n] input: centre-pad the LAST axis, frame it, sqrt(mean(|x|^2)) -> [..., 1, n_frames]."""
    y = np.asarray(y)
    if center:
        y = np.pad(y, [(0, 0)] * (y.ndim - 1) + [(int(frame_length // 2),) * 2], mode=pad_mode)
    n_frames = 1 + (y.shape[-1] - frame_length) // hop_length
    frames = np.stack([y[..., f * hop_length:f * hop_length + frame_length] for f in range(n_frames)], axis=-1)
    return np.sqrt(np.mean(np.abs(frames) ** 2, axis=-2, keepdims=True))


def amplitude_to_db(S_, *, ref=1.0, amin=1e-5, top_db=80.0):
    """librosa.amplitude_to_db (0.10.2) = power_to_db(|S|^2, ref=ref^2, amin=amin^2, top_db)."""
    power = np.square(np.abs(np.asarray(S_)))
    log_spec = 10.0 * np.log10(np.maximum(amin ** 2, power)) - 10.0 * np.log10(np.maximum(amin ** 2, ref ** 2))
    if top_db is not None:
        log_spec = np.maximum(log_spec, log_spec.max() - top_db)
    return log_spec


class _Rec(np.ndarray):
    """The array Silent edits in place; remembers every slice assignment as (begin, end, is_zero)."""
    log = None

    def __setitem__(self, key, value):
        if isinstance(key, tuple) and len(key) == 2 and isinstance(key[1], slice):
            b, e, _ = key[1].indices(self.shape[-1])
            _Rec.log.append((int(b), int(e), bool(np.isscalar(value))))
        super().__setitem__(key, value)


def ranges_of(log):
    """(begin, end, kind) from Silent's assignments: the fades of a stretch come before its zero fill; a fade that ends where the zeros begin is the
    fade-out, one that begins where they end the fade-in."""
    out, fades = [], []
    for b, e, is_zero in log:
        if not is_zero:
            fades.append((b, e))
            continue
        for fb, fe in fades:
            assert fe == b or fb == e, (fb, fe, b, e)
            out.append((fb, fe, 0 if fe == b else 2))
        fades = []
        if e > b:
            out.append((b, e, 1))
    assert not fades
    return np.array(sorted(out), dtype=np.int64).reshape(-1, 3)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def load_batch_node(ns):
    """AudioBatchValueNode of the reference's custom_nodes/audio_nodes.py, its sibling modules and ComfyUI's folder_paths / yt_dlp stubbed."""
    pkg = types.ModuleType("rvcref.custom_nodes")
    pkg.__path__ = []
    settings = types.ModuleType("rvcref.custom_nodes.settings")
    settings.MERGE_OPTIONS = ["median", "mean", "min", "max"]
    utils = types.ModuleType("rvcref.custom_nodes.utils")
    utils.MultipleTypeProxy = type("MultipleTypeProxy", (str,), {})
    utils.increment_filename_no_overwrite = None
    fp = types.ModuleType("folder_paths")
    fp.get_input_directory = fp.get_temp_directory = fp.get_output_directory = lambda: ns.ws
    for name, mod in (("rvcref.custom_nodes", pkg), ("rvcref.custom_nodes.settings", settings), ("rvcref.custom_nodes.utils", utils),
                      ("folder_paths", fp), ("yt_dlp", types.ModuleType("yt_dlp"))):
        sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("rvcref.custom_nodes.audio_nodes", os.path.join(REF_ROOT, "custom_nodes", "audio_nodes.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.AudioBatchValueNode


def main():
    from oracle import ref_shim
    ns = ref_shim.load_reference()
    librosa = sys.modules["librosa"]
    levels_log = []

    def recording_db(S_, **kw):
        r = amplitude_to_db(S_, **kw)
        levels_log.append(float(np.max(r)))
        return r

    librosa.feature.rms = rms_last_axis
    librosa.amplitude_to_db = recording_db
    # the karafan package's __init__ pulls its ONNX inference; only audio_utils.py is wanted, so the package itself is an empty stand-in
    karafan = types.ModuleType(f"{ref_shim.PKG}.lib.karafan")
    karafan.__path__ = [os.path.join(REF_ROOT, "lib", "karafan")]
    sys.modules[karafan.__name__] = karafan
    au = importlib.import_module(f"{ref_shim.PKG}.lib.karafan.audio_utils")
    AP = ns.audio.AudioProcessor
    from scipy.ndimage import uniform_filter1d
    out = {}

    base, _ = S.add_clicks(S.slicer_test_signal(SR, SEED), SEED)
    for case, (start, n, size, ksize, forced) in DECLICK_CASES.items():
        x = base[start:start + n if n else None].copy()
        x[list(forced)] = np.float32(0.5)
        n = x.shape[0]
        mult = 2.0
        thr = mult * np.sqrt(uniform_filter1d(np.square(x), size=int(size)))
        mask = np.abs(x) > thr
        ill = np.flatnonzero(np.abs(np.abs(x).astype(np.float64) - thr) <= 1e-4 * thr)
        assert ill.size <= 1e-3 * n, f"{case}: {ill.size} ill-posed samples"
        assert all(mask[p] for p in forced), f"{case}: a forced click is not detected"
        med = AP.dynamic_thresholding(x, multiplier=mult, sample_size=size, method="median", kernel_size=ksize)
        itp = AP.dynamic_thresholding(x, multiplier=mult, sample_size=size, method="interpolation", kernel_size=ksize)
        assert med.dtype == itp.dtype == np.float32 and np.array_equal(med[~mask], x[~mask]) and np.array_equal(itp[~mask], x[~mask])
        out[f"dc_{case}_meta"] = np.array([SR, SEED, start, n, size, ksize], dtype=np.int64)
        out[f"dc_{case}_forced"] = np.array(forced, dtype=np.int64)
        out[f"dc_{case}_mult"] = np.float64(mult)
        out[f"dc_{case}_mask"] = np.packbits(mask)
        out[f"dc_{case}_illposed"] = ill.astype(np.int64)
        out[f"dc_{case}_median"] = med[mask]
        out[f"dc_{case}_interp"] = itp[mask]
        out[f"dc_{case}_sha_median"] = sha(med)
        print(case, "n", n, "clicks", int(mask.sum()), "ill-posed", ill.size, "within 1e-3", int((np.abs(np.abs(x) - thr) <= 1e-3 * thr).sum()))

    for case, (sr, seed, segments) in GATE_CASES.items():
        x = S.slicer_test_signal(sr, seed, segments)          # no click recipe: ten 0.5 impulses per window would lift every window over the threshold
        thr_db = -50
        del levels_log[:]
        _Rec.log = []
        y = au.Silent(x[None, :].view(_Rec), sample_rate=sr, threshold_dB=thr_db)
        levels = np.array(levels_log, dtype=np.float64)
        ranges = ranges_of(_Rec.log)
        win = int(0.5 * sr)
        assert levels.size <= -(-x.shape[0] // win)
        assert np.abs(levels - thr_db).min() > 0.01 * abs(thr_db), f"{case}: a window level within 1 % of the threshold"
        out[f"gate_{case}_meta"] = np.array([sr, seed, x.shape[0], thr_db], dtype=np.int64)
        out[f"gate_{case}_seg_kind"] = np.array([k for k, _ in segments])
        out[f"gate_{case}_seg_seconds"] = np.array([s_ for _, s_ in segments], dtype=np.float64)
        out[f"gate_{case}_levels"] = levels
        out[f"gate_{case}_ranges"] = ranges
        out[f"gate_{case}_sha"] = sha(np.asarray(y, dtype=np.float32).reshape(-1))
        print(case, "n", x.shape[0], "windows", levels.size, "ranges", ranges.tolist())

    for case, (start, n) in {"n4099": (34000, 4099), "n20011": (30000, 20011)}.items():
        x = base[start:start + n].copy()
        out[f"norm_{case}_meta"] = np.array([SR, SEED, start, n], dtype=np.int64)
        out[f"norm_{case}_out"] = au.Normalize(x.copy(), threshold_dB=-1.0).astype(np.float32)

    sr, seed, segments = CHAIN
    x = S.slicer_test_signal(sr, seed, segments)
    x[list(CHAIN_CLICKS)] = np.float32(0.5)
    del levels_log[:]
    y, sr_out = AP()((x.copy(), sr))
    assert sr_out == sr and y.dtype == np.float32 and y.shape == x.shape
    assert np.abs(np.array(levels_log) + 50).min() > 0.5
    out["chain_meta"] = np.array([sr, seed, x.shape[0]], dtype=np.int64)
    out["chain_seg_kind"] = np.array([k for k, _ in segments])
    out["chain_seg_seconds"] = np.array([s_ for _, s_ in segments], dtype=np.float64)
    out["chain_clicks"] = np.array(CHAIN_CLICKS, dtype=np.int64)
    out["chain_out"] = y

    out["hash_params"] = np.array([json.dumps(p, sort_keys=True) for p in HASH_PARAMS])
    out["hash_values"] = np.array([str(AP(**p)) for p in HASH_PARAMS])

    Node = load_batch_node(ns)
    xb = S.slicer_test_signal(16000, 3, GATE_SEGMENTS[:4])
    out["batch_meta"] = np.array([16000, 3, xb.shape[0], BATCH["num_segments"], BATCH["silence_threshold"]], dtype=np.int64)
    out["batch_range"] = np.array([BATCH["output_min"], BATCH["output_max"]], dtype=np.float64)
    for norm in ("scale", "tanh", "sigmoid"):
        for inverse in (False, True):
            f, i, k = Node().get_frame_weights((xb, 16000), norm=norm, inverse=inverse, **BATCH)
            f = np.array(f, dtype=np.float64)
            assert k == BATCH["num_segments"] and np.abs(f - np.round(f)).min() > 1e-9, (norm, inverse)
            out[f"batch_{norm}_{int(inverse)}_float"] = f
            out[f"batch_{norm}_{int(inverse)}_int"] = np.array(i, dtype=np.int64)
    path = os.path.join(ROOT, "tests", "golden", "audio_fx_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
