"""CPU: the host side of the index build (lib/feature_index.py::build_ivf / train_index, the three rvc_* entry points behind them)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW_SYMBOLS = ("rvc_kmeans_assign", "rvc_kmeans_update", "rvc_index_train")


def test_symbols_declared_exported_and_signed():
    from comfy_rvc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rvc_hip.h")).read()
    product = hdr[:hdr.index("#ifdef RVC_EXPERIMENTS")]
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, product), f"{s} is not declared in the product section of include/rvc_hip.h"
        assert hasattr(_lib.lib, s), f"{s} is not exported"
        assert s in _lib.SIGNATURES and _lib.SIGNATURES[s][0] is _lib.c_int
    assert len(_lib.SIGNATURES["rvc_kmeans_assign"][1]) == 9
    assert len(_lib.SIGNATURES["rvc_kmeans_update"][1]) == 8
    assert len(_lib.SIGNATURES["rvc_index_train"][1]) == 11


def test_nlist_formula():
    from comfy_rvc_amd.lib.feature_index import default_nlist
    assert [default_nlist(n) for n in (39, 4099, 200_000)] == [1, 105, 5128]
    assert default_nlist(200_000) == min(int(16 * np.sqrt(200_000)), 200_000 // 39)


def test_train_index_concatenates_sorted_files_and_writes_the_trained_cells(tmp_path, monkeypatch):
    from comfy_rvc_amd.lib import feature_index as F
    from comfy_rvc_amd.lib.faiss_io import read_index_vectors
    r = np.random.default_rng(2)
    parts = {"b_1.npy": r.standard_normal((50, 16)), "a_0.npy": r.standard_normal((37, 16)), "c_2.npy": r.standard_normal((13, 16))}
    fdir = tmp_path / "3_feature768"
    fdir.mkdir()
    for name, v in parts.items():
        np.save(fdir / name, v.astype(np.float32))
    whole = np.concatenate([parts[k] for k in ("a_0.npy", "b_1.npy", "c_2.npy")], 0).astype(np.float32)
    calls = []

    def stub(big_npy, nlist=None, niter=10, seed=0, device="cuda:0"):
        calls.append((np.array(big_npy), nlist, niter, seed))
        k = F.default_nlist(big_npy.shape[0]) if nlist is None else nlist
        return np.array(big_npy[:k], dtype=np.float32), np.zeros(big_npy.shape[0], np.int32), np.zeros(niter + 1)
    monkeypatch.setattr(F, "build_ivf", stub)
    path = str(tmp_path / "t.index")
    assert F.train_index(str(fdir), path, seed=7) == path
    shuffled = whole[np.random.default_rng(7).permutation(100)]
    assert len(calls) == 1 and np.array_equal(calls[0][0], shuffled) and calls[0][1:] == (None, 10, 7)
    big, info = read_index_vectors(path)
    assert np.array_equal(big, shuffled)
    assert (info["kind"], info["nlist"], info["nprobe"], info["ntotal"]) == ("ivf_flat", 2, 1, 100)
    assert np.array_equal(info["centroids"], shuffled[:2])
    # above reduce_above the rows are replaced by reduce_to centres first; an array is accepted as well
    calls.clear()
    F.train_index(whole, path, seed=7, reduce_above=99, reduce_to=80, niter=3)
    assert [(c[0].shape[0], c[1], c[2]) for c in calls] == [(100, 80, 3), (80, None, 3)]
    _, info = read_index_vectors(path)
    assert info["ntotal"] == 80 and info["nlist"] == 2


def test_build_ivf_without_a_device_raises():
    import torch
    from comfy_rvc_amd import _lib
    from comfy_rvc_amd.lib.feature_index import build_ivf
    if torch.cuda.is_available():
        return
    with pytest.raises(_lib.RvcHipError, match="(?i)device"):
        build_ivf(np.zeros((100, 16), np.float32))


def test_node_module_exposes_train_index_without_a_training_node():
    src = open(os.path.join(ROOT, "comfy-rvc_amd", "custom_nodes", "rvc_nodes.py")).read()
    assert re.search(r"^def train_index\(dataset_dir, sr, name\):", src, flags=re.M)
    mappings = src[src.index("NODE_CLASS_MAPPINGS"):]
    assert "Train" not in mappings
