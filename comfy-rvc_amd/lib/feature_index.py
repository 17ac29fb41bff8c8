"""Device-resident feature retrieval index.

The reference keeps a faiss IVF-Flat index over the training features `big_npy [N, D]` (built by
custom_nodes/rvc_nodes.py:500-554, loaded by pitch_extraction.py:52-73) and calls `index.search(npy, k=1)` on the HuBERT
frames of every segment (vc_infer_pipeline.py:60-75).  `DeviceIndex` offers that call surface - `search`, `ntotal`,
`reconstruct_n` - over the same `big_npy` on the GPU (rvc_index_*, csrc/index.hip), with the semantics of the object it stands for:

* built from a faiss `IVF*,Flat` file (`ivf=(centroids, list_of, nprobe)`, what lib/faiss_io.py reads out of the file): faiss's
  IndexIVFFlat search - the `nprobe` centroids nearest to the query pick the cells, the nearest vector INSIDE those cells is the answer
  (nprobe 1 as train_index sets it: often not the global nearest neighbour), empty probed cells give label -1 / distance FLT_MAX;
* built from a bare `big_npy` (`.npy` file, the reference's preloaded tuple): no cell structure exists, the search is the exact one.

faiss itself is not available offline: both are pinned against restatements of faiss's published algorithm
(oracle/pipeline.py::index_search_ivf / index_search), not against faiss.
"""
import ctypes as C
import os

import numpy as np
import torch

from .. import _lib


class DeviceIndex:
    def __init__(self, big_npy, device="cuda:0", ivf=None):
        big_npy = np.ascontiguousarray(big_npy, dtype=np.float32)
        assert big_npy.ndim == 2, "big_npy must be [N, D]"
        self.device = torch.device(device)
        self.ntotal, self.d = int(big_npy.shape[0]), int(big_npy.shape[1])
        self._big = big_npy
        self._h = C.c_void_p()
        self.nprobe = 0                                    # 0: exact search
        ctx = _lib.get_ctx(self.device.index or 0)
        with torch.cuda.device(self.device):
            if ivf is None:
                _lib.check(_lib.lib.rvc_index_create(ctx, _lib.ptr(big_npy), self.ntotal, self.d, C.byref(self._h)))
            else:
                centroids, list_of, nprobe = ivf
                centroids = np.ascontiguousarray(centroids, dtype=np.float32)
                list_of = np.ascontiguousarray(list_of, dtype=np.int32)
                assert centroids.ndim == 2 and centroids.shape[1] == self.d and list_of.shape == (self.ntotal,)
                _lib.check(_lib.lib.rvc_index_create_ivf(ctx, _lib.ptr(big_npy), self.ntotal, self.d, _lib.ptr(centroids), int(centroids.shape[0]),
                                                         _lib.ptr(list_of), int(nprobe), C.byref(self._h)))
                self.nprobe = int(_lib.lib.rvc_index_nprobe(self._h))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.lib.rvc_index_destroy(h)
            except Exception:   # noqa: BLE001 - interpreter teardown
                pass
            self._h = C.c_void_p()

    def reconstruct_n(self, i0, n):
        return self._big[i0: i0 + n]

    # ---- device entry points (features channel-major [D][T] on the device)
    def search_device(self, feats_cm, want_score=False):
        T = int(feats_cm.shape[1])
        assert feats_cm.shape[0] == self.d and feats_cm.is_contiguous() and feats_cm.dtype == torch.float32
        idx = torch.empty(T, dtype=torch.int64, device=feats_cm.device)
        score = torch.empty(T, dtype=torch.float32, device=feats_cm.device) if want_score else None
        with torch.cuda.device(feats_cm.device):
            _lib.check(_lib.lib.rvc_index_search(self._h, _lib.current_stream(), _lib.ptr(feats_cm), T, _lib.ptr(idx), _lib.ptr(score)))
        return idx, score

    def blend_device(self, feats_cm, index_rate):
        """index_rate * big_npy[nearest] + (1 - index_rate) * feats  (reference :71-74), channel-major in and out."""
        idx, _ = self.search_device(feats_cm)
        out = torch.empty_like(feats_cm)
        with torch.cuda.device(feats_cm.device):
            _lib.check(_lib.lib.rvc_index_blend(self._h, _lib.current_stream(), _lib.ptr(feats_cm), _lib.ptr(idx), int(feats_cm.shape[1]),
                                                float(index_rate), _lib.ptr(out)))
        return out

    # ---- faiss call surface (host arrays), used by the generic VC.vc path
    def search(self, npy, k=1):
        if k != 1:
            raise NotImplementedError("the reference only ever asks for k = 1 (vc_infer_pipeline.py:65)")
        f = torch.from_numpy(np.ascontiguousarray(npy, dtype=np.float32)).to(self.device).t().contiguous()
        idx, score = self.search_device(f, want_score=True)
        return score.cpu().numpy()[:, None], idx.cpu().numpy()[:, None]


# ---- building the index (RVCTrainModelNode.train_index without faiss): k-means on the device, rvc_index_train (csrc/index_build.hip)
def default_nlist(n):
    """The reference's cell count (custom_nodes/rvc_nodes.py:537)."""
    return min(int(16 * np.sqrt(n)), n // 39)


def build_ivf(big_npy, nlist=None, niter=10, seed=0, device="cuda:0"):
    """Trains the level-1 quantiser of an `IVF{nlist},Flat` index over `big_npy [N, D]` on the GPU and assigns every row to its cell.

    -> (centroids float32 [nlist, D], list_of int32 [N], inertia float64 [niter + 1]).  Lloyd's k-means as faiss's `index.train` runs it
    (`niter` = 10 is what the IVF quantiser trains with; empty clusters by `Clustering.cpp::split_clusters` with the most populated cluster
    as the donor), then one assignment against the final centroids (faiss's `add`).  `nlist` defaults to the reference's
    `min(int(16 * sqrt(N)), N // 39)`; under that formula N / nlist never exceeds faiss's 256 points per centroid, so nothing is subsampled.
    The initial centroids are the rows `np.random.default_rng(seed).permutation(N)[:nlist]`: faiss draws them with its own generator, which
    cannot be reproduced without faiss, so the centroids are those of the same algorithm from a different (documented, seeded) start - not
    faiss's numbers.  `inertia[i]` is the sum of squared distances at assignment i.  There is no CPU path: without a GPU this raises."""
    x = np.ascontiguousarray(big_npy, dtype=np.float32)
    assert x.ndim == 2, "big_npy must be [N, D]"
    n, d = int(x.shape[0]), int(x.shape[1])
    nlist = default_nlist(n) if nlist is None else int(nlist)
    if not 1 <= nlist <= n:
        raise ValueError(f"nlist = {nlist} for {n} rows (the reference's formula needs at least 39 rows)")
    dev = torch.device(device)
    ctx = _lib.get_ctx(dev.index or 0)                    # raises RvcHipError when there is no device
    init = np.ascontiguousarray(np.random.default_rng(seed).permutation(n)[:nlist], dtype=np.int64)
    inertia = np.zeros(int(niter) + 1, dtype=np.float64)
    with torch.cuda.device(dev):
        rows = torch.from_numpy(x).to(dev)
        cent = torch.empty(nlist, d, dtype=torch.float32, device=dev)
        label = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib.rvc_index_train(ctx, _lib.current_stream(), _lib.ptr(rows), n, d, _lib.ptr(init), nlist, int(niter), _lib.ptr(cent),
                                            _lib.ptr(label), _lib.ptr(inertia)))
        return cent.cpu().numpy(), label.cpu().numpy(), inertia


def _load_features(feature_dir_or_array):
    if isinstance(feature_dir_or_array, (str, os.PathLike)):
        names = sorted(f for f in os.listdir(feature_dir_or_array))
        if not names:
            raise ValueError(f"no feature files in {feature_dir_or_array}")
        return np.concatenate([np.load(os.path.join(feature_dir_or_array, f)) for f in names], 0)
    return np.asarray(feature_dir_or_array)


def train_index(feature_dir_or_array, index_file, seed=0, reduce_above=200_000, reduce_to=10_000, niter=10, device="cuda:0"):
    """The body of the reference's RVCTrainModelNode.train_index (custom_nodes/rvc_nodes.py:511-549) with the k-means on the GPU: the `*.npy`
    dumps of a feature directory in sorted order (or an array) are concatenated, the rows shuffled (`np.random.default_rng(seed)`; the
    reference shuffles with numpy's unseeded global generator), the IVF cells trained by `build_ivf` and the result written as a faiss
    `IVF{nlist},Flat` file with nprobe 1, which `VC.load_index` / faiss open.  Returns `index_file`.  The same seed gives the same file.

    Deviation: above `reduce_above` rows the reference replaces the rows by the `reduce_to` centres of `sklearn.MiniBatchKMeans(init="random")`,
    which is stochastic and cannot be pinned; here the same full-batch device k-means (`build_ivf` with `nlist = reduce_to`) provides them.
    The cell of a row in the file is the writer's own float64 assignment against the trained centroids (the search reads the file), which can
    differ from the device's on a near-tie."""
    from . import faiss_io
    x = np.ascontiguousarray(_load_features(feature_dir_or_array), dtype=np.float32)
    assert x.ndim == 2, "features must be [N, D]"
    x = x[np.random.default_rng(seed).permutation(x.shape[0])]
    if x.shape[0] > reduce_above:
        x, _, _ = build_ivf(x, nlist=reduce_to, niter=niter, seed=seed, device=device)
    centroids, _, _ = build_ivf(x, niter=niter, seed=seed, device=device)
    faiss_io.write_ivf_flat(index_file, x, int(centroids.shape[0]), centroids=centroids, nprobe=1)
    return index_file
