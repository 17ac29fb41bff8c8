"""CPU: the host side of dataset preparation against what the reference's Slicer / Preprocess gave (tests/golden/slicer_cases.npz, written by
tools/gen_golden_slicer.py): the silence scan rvc_slice_tags, the chunk / window / name arithmetic, and the dataset node's interface."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
from comfy_rvc_amd import synthetic as S

# case -> the recipe of its recording (rate, seed and length are in the golden's {case}_meta)
CASES = {
    "r40k_s0": S.SLICER_SEGMENTS,
    "short_sil_40k": S.SLICER_SEGMENTS_SHORT_SIL,       # a 0.48 s silence after 2 s of signal: the "<= max_sil_kept" cut position
    "r48k_s0": S.SLICER_SEGMENTS,
    "r32k_s1": S.SLICER_SEGMENTS,
    "tiny_40k": (("v", 0.0025),),                        # 100 samples <= min_length (100 frames): the early return
}
_golden = {}


def cases():
    if not _golden:
        _golden.update(golden("slicer_cases.npz"))
    return _golden


def case_meta(case):
    sr, seed, idx0, n = (int(v) for v in cases()[f"{case}_meta"])
    return sr, seed, idx0, n


def case_signal(case):
    sr, seed, _, n = case_meta(case)
    x = S.slicer_test_signal(sr, seed, CASES[case])
    assert x.shape[0] == n and x.dtype == np.float32
    return x


def assert_well_posed(case):
    """Equality with the reference is only asked where it is well-posed: no reference RMS frame within 1 % of the threshold, and in every range the
    reference took an arg-min over the two smallest values differ by more than 1e-3 relative."""
    from comfy_rvc_amd.lib.dataset_prep import slicer_params
    g = cases()
    rms, thr = g[f"{case}_rms"], slicer_params(case_meta(case)[0])["threshold"]
    if rms.size:
        assert np.abs(rms / thr - 1.0).min() > 0.01, case
    for a, b in g[f"{case}_argmin"]:
        v = np.sort(rms[a:b])
        assert v.size == 1 or v[1] - v[0] > 1e-3 * v[0], (case, a, b)


def test_slicer_params_match_reference_values():
    from comfy_rvc_amd.lib.dataset_prep import slicer_params
    # Slicer(sr, threshold=-50, min_length=1500, min_interval=400, hop_size=15, max_sil_kept=500) of the reference at the three model rates
    want = {32000: (480, 1920, 100, 27, 33), 40000: (600, 2400, 100, 27, 33), 48000: (720, 2880, 100, 27, 33)}
    for sr, (hop, win, ml, mi, ms) in want.items():
        p = slicer_params(sr)
        assert (p["hop_size"], p["win_size"], p["min_length"], p["min_interval"], p["max_sil_kept"]) == (hop, win, ml, mi, ms)
        assert p["threshold"] == 10 ** (-50 / 20.0)
    with pytest.raises(ValueError):
        slicer_params(40000, min_length=100, min_interval=400)


@pytest.mark.parametrize("case", list(CASES))
def test_slice_tags_equal_reference(case):
    from comfy_rvc_amd.lib.dataset_prep import slice_tags, slicer_params
    assert_well_posed(case)
    g = cases()
    sr, _, _, n = case_meta(case)
    tags = slice_tags(g[f"{case}_rms"], n, slicer_params(sr))
    assert tags.dtype == np.int64 and np.array_equal(tags, g[f"{case}_tags"]), (tags.tolist(), g[f"{case}_tags"].tolist())


def test_slice_tags_cases_reach_every_branch():
    """What the cases are there for, read off the reference's tags: a leading cut (0, e), a cut that drops nothing (p, p), one that drops a stretch,
    the trailing tag (p, total + 1) - and arg-min ranges of the three cut positions (1, 3 and 2 ranges per cut)."""
    g = cases()
    t, nf = g["r40k_s0_tags"], g["r40k_s0_rms"].size
    assert t[0][0] == 0 and t[0][1] > 0 and t[-1][1] == nf + 1 and any(b < e for b, e in t[1:-1])
    assert g["short_sil_40k_tags"].tolist() == [[176, 176]] and g["short_sil_40k_argmin"].shape[0] == 1
    assert g["tiny_40k_tags"].shape[0] == 0 and g["tiny_40k_rms"].size == 0


def test_slice_tags_rejects_bad_arguments():
    from comfy_rvc_amd import _lib as L
    rms, tags, nt = np.ones(4), np.zeros((1, 2), dtype=np.int64), C.c_int64()
    assert L.lib.rvc_slice_tags(L.ptr(rms), 4, 1000, 0.5, 2, 0, 2, L.ptr(tags), 1, C.byref(nt)) != 0          # min_interval of 0 frames
    # a buffer that cannot hold the tags is an error, not an overrun: silence, 3 loud frames, silence (leading cut + trailing tag = 2 tags)
    rms = np.array([0.] * 5 + [1.] * 3 + [0.] * 5)
    assert L.lib.rvc_slice_tags(L.ptr(rms), rms.size, 1000, 0.5, 2, 2, 2, L.ptr(tags), 1, C.byref(nt)) != 0
    assert b"tag buffer" in L.lib.rvc_last_error()


@pytest.mark.parametrize("case", list(CASES))
def test_chunks_windows_and_names_equal_reference(case):
    from comfy_rvc_amd.lib.dataset_prep import chunk_bounds, plan_windows, slicer_params
    g = cases()
    sr, _, idx0, n = case_meta(case)
    chunks = chunk_bounds(g[f"{case}_tags"], g[f"{case}_rms"].size, slicer_params(sr)["hop_size"], n)
    assert np.array_equal(np.array(chunks, dtype=np.int64).reshape(-1, 2), g[f"{case}_chunks"])
    plan, ref = plan_windows(chunks, sr, 3.0, .3), g[f"{case}_windows"]
    assert len(plan) == ref.shape[0]
    for (start, length, idx1, written), (rs, rl, ri, rw) in zip(plan, ref):
        assert (length, idx1, written) == (rl, ri, rw) and (start == rs or length == 0)
    names = sorted(set(f"{idx0}_{idx1}" for _, _, idx1, written in plan if written))
    assert names == sorted(str(v) for v in g[f"{case}_names"])


def test_plan_windows_numbering_and_short_remainder():
    """The remainder takes the number after the one the loop stopped at and the next chunk's first window reuses it; a remainder of at most
    2 * overlap s is planned but not written."""
    from comfy_rvc_amd.lib.dataset_prep import plan_windows
    sr = 1000
    plan = plan_windows([(0, 3400), (5000, 5600), (7000, 7000)], sr, 3.0, .3)
    assert plan == [(0, 3000, 0, 1), (2700, 700, 2, 1), (5000, 600, 3, 0), (7000, 0, 4, 0)]
    plan = plan_windows([(0, 3301), (4000, 7301)], sr, 3.0, .3)
    assert [(p[2], p[3]) for p in plan] == [(0, 1), (2, 1), (2, 1), (4, 1)]                # 2 is written twice: the later window wins


def test_dataset_node_interface(tmp_path, monkeypatch):
    """INPUT_TYPES keys and defaults of reference custom_nodes/rvc_nodes.py:211-239 (n_threads' default is machine-dependent there)."""
    from comfy_rvc_amd.custom_nodes import rvc_nodes as N
    assert N.NODE_CLASS_MAPPINGS["RVCProcessDatasetNode"] is N.RVCProcessDatasetNode
    import comfy_rvc_amd
    assert comfy_rvc_amd.NODE_CLASS_MAPPINGS["RVCProcessDatasetNode"] is N.RVCProcessDatasetNode
    monkeypatch.setattr(N, "INPUT_DIR", str(tmp_path))
    (tmp_path / "datasets").mkdir()
    (tmp_path / "datasets" / "voice.zip").write_bytes(b"")
    (tmp_path / "datasets" / "notes.txt").write_bytes(b"")
    it = N.RVCProcessDatasetNode.INPUT_TYPES()
    req, opt = it["required"], it["optional"]
    assert list(req) == ["model_name", "dataset", "hubert_model"]
    assert req["model_name"] == ("STRING", {"default": ""}) and req["hubert_model"] == ("HUBERT_MODEL",)
    assert req["dataset"] == (["", "voice.zip"], {"default": ""})
    assert list(opt) == ["pitch_extraction_params", "sr", "n_threads", "period", "overlap", "max_volume", "mute_ratio", "audio_processor"]
    assert opt["pitch_extraction_params"] == ("PITCH_EXTRACTION", {"default": {}})
    assert opt["sr"] == (["32k", "40k", "48k"], {"default": "40k"})
    assert opt["n_threads"][0] == "INT" and opt["n_threads"][1]["min"] == 1 and 1 <= opt["n_threads"][1]["default"] <= opt["n_threads"][1]["max"]
    assert opt["period"] == ("FLOAT", {"default": 3., "min": 1., "max": 10., "step": .1})
    assert opt["overlap"] == ("FLOAT", {"default": .3, "min": .1, "max": 1., "step": .1})
    assert opt["max_volume"] == ("FLOAT", {"default": .99, "min": .1, "max": 1., "step": .01})
    assert opt["mute_ratio"] == ("FLOAT", {"default": .0, "min": .0, "max": .5, "step": .01})
    assert opt["audio_processor"] == ("AUDIO_PROCESSOR",)
    assert N.RVCProcessDatasetNode.RETURN_TYPES == ("RVC_DATASET_PIPE",) and N.RVCProcessDatasetNode.RETURN_NAMES == ("rvc_dataset_pipe",)
    assert N.RVCProcessDatasetNode.FUNCTION == "process" and N.RVCProcessDatasetNode.CATEGORY == N.CATEGORY
    assert N.SR_MAP == {"32k": 32000, "40k": 40000, "48k": 48000}
    # the cache name: md5 over the concatenated parameter strings
    import hashlib
    assert N.get_hash("a", 3.0, None) == hashlib.md5(b"a3.0None").hexdigest()
