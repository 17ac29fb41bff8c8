"""CPU: the host parts of the audio nodes (lib/audio_fx.py, lib/audio.py::AudioProcessor, custom_nodes/audio_nodes.py) against what the
reference made of the same recipes (tests/golden/audio_fx_cases.npz, written by tools/gen_golden_audio_fx.py)."""
import json

import numpy as np
import pytest

from conftest import golden
from comfy_rvc_amd import synthetic as S

GATE_CASES = ("g40k", "g44k", "g16k_endexact")
DECLICK_CASES = ("full", "n100003", "n65567", "n4099", "n_eq_size", "edges")
_memo = {}


def cases():
    if "g" not in _memo:
        _memo["g"] = golden("audio_fx_cases.npz")
    return _memo["g"]


def gate_signal(case):
    g = cases()
    sr, seed, n, thr = (int(v) for v in g[f"gate_{case}_meta"])
    segments = tuple((str(k), float(s)) for k, s in zip(g[f"gate_{case}_seg_kind"], g[f"gate_{case}_seg_seconds"]))
    x = S.slicer_test_signal(sr, seed, segments)
    assert x.shape == (n,)
    return x, sr, thr


def declick_signal(case):
    if ("dc", case) not in _memo:
        g = cases()
        sr, seed, start, n, size, ksize = (int(v) for v in g[f"dc_{case}_meta"])
        if "base" not in _memo:
            _memo["base"] = S.add_clicks(S.slicer_test_signal(sr, seed), seed)[0]
        x = _memo["base"][start:start + n].copy()
        x[g[f"dc_{case}_forced"]] = np.float32(0.5)
        mask = np.unpackbits(g[f"dc_{case}_mask"])[:n].astype(bool)
        _memo["dc", case] = (x, size, ksize, float(g[f"dc_{case}_mult"]), mask)
    return _memo["dc", case]


def assert_gate_well_posed(case):
    g = cases()
    thr = int(g[f"gate_{case}_meta"][3])
    assert np.abs(g[f"gate_{case}_levels"] - thr).min() > 0.01 * abs(thr)


@pytest.mark.parametrize("case", GATE_CASES)
def test_gate_ranges_equal_reference(case):
    """The host scan over the reference's own window levels gives the reference's edits: silence at the start (no fade-out), a silence shorter than
    min_size (untouched), one in the middle (both fades), one at the end (zero up to n), a short and a whole last window."""
    from comfy_rvc_amd.lib import audio_fx
    g = cases()
    assert_gate_well_posed(case)
    sr, _, n, thr = (int(v) for v in g[f"gate_{case}_meta"])
    win, min_size, fade = audio_fx.gate_params(sr)
    ranges = audio_fx.gate_ranges(g[f"gate_{case}_levels"], n, win, min_size, fade, thr)
    assert np.array_equal(ranges, g[f"gate_{case}_ranges"])


def test_gate_cases_cover_the_branches():
    g = cases()
    r40, r16 = g["gate_g40k_ranges"], g["gate_g16k_endexact_ranges"]
    n40 = int(g["gate_g40k_meta"][2])
    assert r40[0, 0] == 0 and r40[0, 2] == 1                         # leading silence: zero from sample 0, no fade-out
    assert any(k == 0 for k in r40[:, 2]) and any(k == 2 for k in r40[:, 2])
    assert r40[-1, 1] == n40 and r40[-1, 2] == 1 and n40 % 20000 != 0   # trailing silence up to n, the last window is short
    assert not ((r40[:, 0] <= 130000) & (r40[:, 1] > 130000)).any()  # the 0.7 s silence (2.9 - 3.6 s) stays
    assert int(g["gate_g16k_endexact_meta"][2]) % 8000 == 0 and r16[-1, 1] == 48000
    assert g["gate_g44k_ranges"][-1, 2] == 2                         # ends loud: the last edit is a fade-in


def test_window_levels_against_numpy_framing():
    """window_levels over numpy sums of squares reproduces the reference's levels (float32 framing there, float64 here: 1e-4 dB)."""
    from comfy_rvc_amd.lib import audio_fx
    g = cases()
    for case in GATE_CASES:
        x, sr, _ = gate_signal(case)
        win = audio_fx.gate_params(sr)[0]
        nw = -(-x.shape[0] // win)
        ss = np.zeros((nw, 2))
        for w in range(nw):
            seg = x[w * win:(w + 1) * win].astype(np.float64)
            for f in range(2):
                a, b = max(f * win - win // 2, 0), min(f * win - win // 2 + win, seg.shape[0])
                ss[w, f] = np.sum(seg[a:b] ** 2) if b > a else 0.0
        lev = audio_fx.window_levels(ss, x.shape[0], win)
        ref = g[f"gate_{case}_levels"]
        assert np.abs(lev[:ref.shape[0]] - ref).max() < 1e-4


def test_audio_processor_hash_equals_reference():
    from comfy_rvc_amd.lib.audio import AudioProcessor
    g = cases()
    assert len(g["hash_params"]) == 3
    for params, want in zip(g["hash_params"], g["hash_values"]):
        assert str(AudioProcessor(**json.loads(str(params)))) == str(want)
    p = AudioProcessor()
    assert (p.normalize, p.threshold_silence, p.dynamic_threshold, p.sample_size, p.multiplier, p.fill_method, p.kernel_size,
            p.silence_threshold_db, p.normalize_threshold_db) == (True, True, True, 16000, 2.0, "median", 5, -50, -1)


def test_node_surfaces_equal_reference():
    """Literals transcribed from reference custom_nodes/audio_nodes.py:54-72, :124-150, :224-249, :280-305."""
    from comfy_rvc_amd.custom_nodes import audio_nodes as A
    proxy = "AUDIO,VHS_AUDIO"
    assert A.AudioInfoNode.INPUT_TYPES() == {"required": {"audio": (proxy,)}}
    assert (A.AudioInfoNode.RETURN_TYPES, A.AudioInfoNode.RETURN_NAMES, A.AudioInfoNode.FUNCTION) == \
        (("VHS_AUDIO", "AUDIO", "FLOAT", "INT"), ("vhs_audio", "audio", "seconds", "sr"), "get_info")
    assert A.MergeAudioNode.INPUT_TYPES() == {
        "required": {"audio1": (proxy,), "audio2": (proxy,)},
        "optional": {"sr": (["None", 32000, 40000, 44100, 48000], {"default": "None"}),
                     "merge_type": (["median", "mean", "min", "max"], {"default": "median"}),
                     "normalize": ("BOOLEAN", {"default": True}),
                     "audio3_opt": (proxy, {"default": None}), "audio4_opt": (proxy, {"default": None})}}
    assert list(A.MergeAudioNode.INPUT_TYPES()["optional"]) == ["sr", "merge_type", "normalize", "audio3_opt", "audio4_opt"]
    assert (A.MergeAudioNode.RETURN_TYPES, A.MergeAudioNode.RETURN_NAMES, A.MergeAudioNode.FUNCTION, A.MergeAudioNode.OUTPUT_NODE) == \
        (("VHS_AUDIO", "AUDIO"), ("vhs_audio", "audio"), "merge", True)
    assert A.ProcessAudioNode.INPUT_TYPES() == {
        "required": {"normalize": ("BOOLEAN", {"default": True}), "threshold_silence": ("BOOLEAN", {"default": True}),
                     "dynamic_threshold": ("BOOLEAN", {"default": True})},
        "optional": {"audio": (proxy, {"default": None}),
                     "dynamic_threshold_sample_size": ("INT", {"default": 4000, "min": 160, "max": 48000, "step": 160}),
                     "dynamic_threshold_multiplier": ("FLOAT", {"default": 2., "min": 1.5, "step": .1}),
                     "dynamic_threshold_fill_method": (["median", "interpolation"], {"default": "median"}),
                     "dynamic_threshold_kernel_size": ("INT", {"default": 5, "min": 3, "step": 2}),
                     "silence_threshold_db": ("INT", {"default": -50, "min": -120, "max": 0}),
                     "normalize_threshold_db": ("INT", {"default": -1, "min": -10, "max": 0})}}
    assert list(A.ProcessAudioNode.INPUT_TYPES()["optional"]) == [
        "audio", "dynamic_threshold_sample_size", "dynamic_threshold_multiplier", "dynamic_threshold_fill_method",
        "dynamic_threshold_kernel_size", "silence_threshold_db", "normalize_threshold_db"]
    assert (A.ProcessAudioNode.RETURN_TYPES, A.ProcessAudioNode.RETURN_NAMES, A.ProcessAudioNode.FUNCTION) == \
        (("AUDIO_PROCESSOR", "VHS_AUDIO", "AUDIO"), ("audio_processor", "vhs_audio", "audio"), "process_audio")
    assert A.AudioBatchValueNode.INPUT_TYPES() == {
        "required": {"audio": (proxy,), "num_segments": ("INT", {"default": 2, "min": 2, "max": 256, "step": 1}),
                     "output_min": ("FLOAT", {"default": 0., "min": -1000., "max": 1000., "step": .01}),
                     "output_max": ("FLOAT", {"default": 1., "min": 0., "max": 1000., "step": .01}),
                     "norm": (["scale", "tanh", "sigmoid"], {"default": "scale"})},
        "optional": {"silence_threshold": ("INT", {"default": 1000, "min": 1, "max": 32768, "step": 1}),
                     "duration_list": ("INT", {"default": 0, "min": 0, "forceInput": True}),
                     "print_output": ("BOOLEAN", {"default": False}), "inverse": ("BOOLEAN", {"default": False})}}
    assert list(A.AudioBatchValueNode.INPUT_TYPES()["required"]) == ["audio", "num_segments", "output_min", "output_max", "norm"]
    assert (A.AudioBatchValueNode.RETURN_TYPES, A.AudioBatchValueNode.RETURN_NAMES, A.AudioBatchValueNode.FUNCTION) == \
        (("FLOAT", "INT", "INT"), ("FLOAT", "INT", "num_values"), "get_frame_weights")
    for node in (A.AudioInfoNode, A.MergeAudioNode, A.ProcessAudioNode, A.AudioBatchValueNode):
        assert node.CATEGORY == "🌺RVC-Studio/audio"
    assert isinstance(A.MergeAudioNode.INPUT_TYPES()["required"]["audio1"][0], A.MultipleTypeProxy)
    assert A.MergeAudioNode.INPUT_TYPES()["required"]["audio1"][0] == "AUDIO"


def test_nodes_registered_in_the_package():
    import comfy_rvc_amd
    from comfy_rvc_amd.custom_nodes import audio_nodes as A
    for name in ("MergeAudioNode", "ProcessAudioNode", "AudioBatchValueNode", "AudioInfoNode"):
        assert comfy_rvc_amd.NODE_CLASS_MAPPINGS[name] is getattr(A, name)
    assert not set(A.NODE_CLASS_MAPPINGS) & set(comfy_rvc_amd.NODE_DISPLAY_NAME_MAPPINGS)


@pytest.mark.parametrize("n,k", [(10, 3), (100003, 7), (100003, 256), (7, 7), (1001, 2), (512, 256)])
def test_split_bounds_equal_array_split(n, k):
    from comfy_rvc_amd.lib.audio_fx import split_bounds
    parts = np.array_split(np.arange(n), k)
    b = split_bounds(n, k)
    assert b.shape == (k + 1,) and b[0] == 0 and b[-1] == n
    assert [int(v) for v in np.diff(b)] == [len(p) for p in parts] and all(int(b[i]) == int(p[0]) for i, p in enumerate(parts))


def test_declick_golden_is_well_posed():
    """At most 0.1 % of a case's samples lie within 1e-4 of their threshold (those are left out of the mask comparison)."""
    g = cases()
    for case in DECLICK_CASES:
        n = int(g[f"dc_{case}_meta"][3])
        assert g[f"dc_{case}_illposed"].size <= 1e-3 * n
    for case in ("full", "n100003", "n65567", "n_eq_size", "edges"):
        assert g[f"dc_{case}_illposed"].size == 0
