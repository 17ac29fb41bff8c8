"""GPU: building the retrieval index on the device (csrc/index_build.hip, lib/feature_index.py::build_ivf / train_index) against a float64 numpy
restatement of the same Lloyd k-means: same initial rows, same empty-cluster rule, same final assignment."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N0, D0, NEAR_TIE, EXCUSED_CAP = 4099, 768, 1e-4, 0.005


@pytest.fixture(scope="module")
def L():
    from comfy_rvc_amd import _lib
    _lib.get_ctx(0)
    return _lib


def _blobs(N, D):
    r = np.random.default_rng(0)
    c = r.standard_normal((24, D))
    x = (c[r.integers(0, 24, N)] + 0.35 * r.standard_normal((N, D))).astype(np.float32)
    return x, r


@pytest.fixture(scope="module")
def common():
    """The common input: x [4099, 768] and the 67 centroids of the assign test (rows of x); left unchanged by every test."""
    x, r = _blobs(N0, D0)
    cent = x[_common_perm()[:67]].copy()
    return x, cent


def _common_perm():
    """The permutation that follows x in the common generator: its first 67 rows are the assign test's centroids, its first 105 the train test's start."""
    _, r = _blobs(N0, D0)
    return r.permutation(N0)


# ---------------------------------------------------------------------------------------------------- float64 restatement
def ref_d2(x, c):
    x, c = x.astype(np.float64), c.astype(np.float64)
    return np.maximum((x * x).sum(1)[:, None] - 2.0 * x @ c.T + (c * c).sum(1)[None], 0.0)


def ref_assign(x, c):
    """-> labels (argmin, first on ties), d1, second-nearest label, relative gap (d2 - d1) / d2 (1 when there is one centroid)."""
    return _nearest_two(ref_d2(x, c))


def _nearest_two(d):
    lab = d.argmin(1)
    rows = np.arange(d.shape[0])
    d1 = d[rows, lab]
    if d.shape[1] == 1:
        return lab, d1, lab, np.ones_like(d1)
    dd = d.copy(); dd[rows, lab] = np.inf
    second = dd.argmin(1)
    d2 = dd[rows, second]
    return lab, d1, second, (d2 - d1) / np.where(d2 > 0, d2, 1.0)


def ref_update(x, lab, cent):
    """Means in float64 rounded once; empty clusters by the split rule.  -> (centroids float32, counts)."""
    K = cent.shape[0]
    cnt = np.bincount(lab, minlength=K).astype(np.int64)
    out = cent.astype(np.float32).copy()
    x64 = x.astype(np.float64)
    order = np.argsort(lab, kind="stable")
    off = np.concatenate([[0], np.cumsum(cnt)])
    for k in np.nonzero(cnt)[0]:
        out[k] = (x64[order[off[k]:off[k + 1]]].sum(0) / cnt[k]).astype(np.float32)
    up, dn = np.float32(1 + 1 / 1024), np.float32(1 - 1 / 1024)
    even = (np.arange(cent.shape[1]) % 2 == 0)
    for j in range(K):
        if cnt[j] == 0:
            c = int(np.argmax(cnt))                        # first maximum = smallest index on ties
            v = out[c].copy()
            out[j] = np.where(even, v * up, v * dn).astype(np.float32)
            out[c] = np.where(even, v * dn, v * up).astype(np.float32)
            cnt[j] = cnt[c] // 2
            cnt[c] -= cnt[j]
    return out, cnt


def ref_train(x, init, niter):
    cent = x[init].astype(np.float32).copy()
    inertia, split_after = [], []
    for _ in range(niter):
        lab, d1, _, _ = ref_assign(x, cent)
        inertia.append(d1.sum())
        split_after.append(bool((np.bincount(lab, minlength=cent.shape[0]) == 0).any()))
        cent, _ = ref_update(x, lab, cent)
    lab, d1, _, _ = ref_assign(x, cent)
    inertia.append(d1.sum())
    return cent, lab, np.array(inertia), split_after


@pytest.fixture(scope="module")
def train_ref(common):
    """Start of the train test: the first 105 rows of the common permutation.  In float64 that start leaves one cluster empty on the way (the split
    rule runs) and the inertia goes 9.310e5 -> 3.742e5.  (The noise floor of the input is 0.35^2 * 768 * 4099 = 3.86e5 less what 105 means absorb; a start
    that covers all 24 blobs begins near 7.2e5 and cannot halve, so "below half the initial" needs a start that misses a blob, as this one does.)"""
    x, _ = common
    init = _common_perm()[:105].astype(np.int64)
    return (init,) + ref_train(x, init, 10)


# ---------------------------------------------------------------------------------------------------- device calls
def dev_assign(L, x, cent, want_dist=True):
    xd, cd = torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(np.ascontiguousarray(cent)).cuda()
    lab = torch.full((x.shape[0],), -7, dtype=torch.int32, device="cuda")
    dist = torch.full((x.shape[0],), float("nan"), device="cuda") if want_dist else None
    L.check(L.lib.rvc_kmeans_assign(L.get_ctx(0), L.current_stream(), L.ptr(xd), x.shape[0], x.shape[1], L.ptr(cd), cent.shape[0], L.ptr(lab), L.ptr(dist)))
    torch.cuda.synchronize()
    return lab.cpu().numpy(), (dist.cpu().numpy() if want_dist else None)


def dev_update(L, x, lab, cent):
    xd, cd = torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(np.ascontiguousarray(cent, dtype=np.float32)).cuda()
    ld = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)).cuda()
    cnt = torch.full((cent.shape[0],), -7, dtype=torch.int32, device="cuda")
    L.check(L.lib.rvc_kmeans_update(L.current_stream(), L.ptr(xd), L.ptr(ld), x.shape[0], x.shape[1], cent.shape[0], L.ptr(cd), L.ptr(cnt)))
    torch.cuda.synchronize()
    return cd.cpu().numpy(), cnt.cpu().numpy()


def check_assign(x, cent, lab, dist, what):
    """Test 1's rule: a row may differ from float64 only if its relative gap is below 1e-4, and then it took float64's second nearest; the share of
    rows that COULD be excused is capped at 0.5 % (from the reference alone); dist within 1e-4 d1 + 1e-3."""
    rl, d1, second, gap = ref_assign(x, cent)
    share = float((gap < NEAR_TIE).mean())
    diff = lab != rl
    print(f"{what}: near-tie share {share:.4%}, rows that differ {int(diff.sum())}")
    assert share <= EXCUSED_CAP, f"{what}: {share:.3%} near-tie rows in the reference"
    assert lab.min() >= 0 and lab.max() < cent.shape[0]
    bad = diff & ~((gap < NEAR_TIE) & (lab == second))
    assert not bad.any(), f"{what}: rows {np.nonzero(bad)[0][:8]} differ from float64 outside a near-tie"
    if dist is not None:
        err = np.abs(dist.astype(np.float64) - d1)
        print(f"{what}: max dist error {err.max():.3e} (d1 up to {d1.max():.1f})")
        assert (err <= 1e-4 * d1 + 1e-3).all(), f"{what}: dist off by {err.max()}"


ASSIGN_SHAPES = [(4099, 256, 67), (4099, 768, 5), (63, 768, 63)]


# ---------------------------------------------------------------------------------------------------- 1. assign
def test_assign_common(L, common):
    x, cent = common
    lab, dist = dev_assign(L, x, cent)
    check_assign(x, cent, lab, dist, "assign 4099 x 768, K 67")
    lab2, _ = dev_assign(L, x, cent, want_dist=False)
    assert np.array_equal(lab, lab2)


@pytest.mark.parametrize("shape", ASSIGN_SHAPES, ids=["d256", "k5", "n63k63"])
def test_assign_shapes(L, shape):
    N, D, K = shape
    x, r = _blobs(N, D)
    cent = x[r.permutation(N)[:K]]
    lab, dist = dev_assign(L, x, cent)
    check_assign(x, cent, lab, dist, f"assign {N} x {D}, K {K}")


def test_assign_many_tiles(L, common):
    """More centroids than one tile and than one K split: 300 centroids (3 tiles, the last ragged) over 33 row tiles."""
    x, _ = common
    cent = x[np.random.default_rng(5).permutation(N0)[:300]]
    lab, dist = dev_assign(L, x, cent)
    check_assign(x, cent, lab, dist, "assign 4099 x 768, K 300")


def test_assign_ties_go_to_the_smaller_index(L, common):
    x, cent = common
    c = np.concatenate([cent, cent[[3, 40]]], 0)           # centroids 67 / 68 repeat 3 / 40 ...
    c[[10, 50]] = cent[[60, 66]]                           # ... and 10 / 50 are copies placed BELOW their originals 60 / 66
    lab, _ = dev_assign(L, x, c)
    assert not np.isin(lab, [67, 68, 60, 66]).any()        # the copy with the larger index never wins
    d = ref_d2(x, c)
    d[:, [67, 68, 60, 66]] = np.inf                        # float64 over the distinct centroids: rows outside a near-tie must agree
    rl, _, _, gap = _nearest_two(d)
    for k in (3, 40, 10, 50):
        assert ((rl == k) & (gap >= NEAR_TIE)).sum() > 0
    assert np.array_equal(lab[gap >= NEAR_TIE], rl[gap >= NEAR_TIE])
    wide = np.concatenate([np.tile(cent[:1], (200, 1)), cent[:1] + 50.0], 0)   # 200 identical centroids across two tiles and both wave rows
    assert (dev_assign(L, x, wide)[0] == 0).all()


# ---------------------------------------------------------------------------------------------------- 2. update
def _ulp_diff(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def test_update_means_counts_and_determinism(L, common):
    x, cent = common
    rl = ref_assign(x, cent)[0]
    assert np.bincount(rl, minlength=67).min() > 0
    want, wcnt = ref_update(x, rl, cent)
    got, cnt = dev_update(L, x, rl, cent)
    assert np.array_equal(cnt, wcnt)
    u = _ulp_diff(got, want)
    print(f"update: centroids differ from the float64 means by at most {int(u.max())} ulp ({int((u > 0).sum())} of {u.size} elements)")
    assert u.max() <= 1
    got2, cnt2 = dev_update(L, x, rl, cent)
    assert np.array_equal(got.view(np.int32), got2.view(np.int32)) and np.array_equal(cnt, cnt2)


def test_update_several_row_blocks(L):
    """More rows than one block of the counting sort (1024) and chunks with repeated labels: 5000 x 8, 7 clusters, against float64."""
    r = np.random.default_rng(3)
    x = r.standard_normal((5000, 8)).astype(np.float32)
    lab = r.integers(0, 7, 5000).astype(np.int32)
    want, wcnt = ref_update(x, lab, np.zeros((7, 8), np.float32))
    got, cnt = dev_update(L, x, lab, np.zeros((7, 8), np.float32))
    assert np.array_equal(cnt, wcnt) and _ulp_diff(got, want).max() <= 1


def test_update_split_rule(L):
    """Two forced empty clusters (2 and 5 of 8).  Small-integer rows: every float64 sum and mean is exact, so the restatement is matched bit for bit."""
    r = np.random.default_rng(1)
    x = r.integers(-8, 9, (1500, 64)).astype(np.float32)
    # 0 and 1 tie as the most populated: the first split takes 0 (smaller index), which leaves 1 as the donor of the second
    lab = r.permutation(np.repeat([0, 1, 3, 4, 6, 7], [400, 400, 200, 200, 150, 150])).astype(np.int32)
    old = r.standard_normal((8, 64)).astype(np.float32)
    want, wcnt = ref_update(x, lab, old)
    assert (np.bincount(lab, minlength=8)[[2, 5]] == 0).all() and wcnt[2] > 0 and wcnt[5] > 0
    got, cnt = dev_update(L, x, lab, old)
    assert np.array_equal(cnt, wcnt), (cnt, wcnt)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


# ---------------------------------------------------------------------------------------------------- 3. train
def test_train(L, common, train_ref):
    """rvc_index_train at K = 105, 10 iterations: inertia non-increasing except right after a split, final below half the initial and at most 1.001 x the
    float64 restatement's from the same start (an excused near-tie flip moves one row's term by < 1e-4 relative; 1e-3 is ten times that).  Measured on
    MI355X: 9.309992e5 -> 3.741828e5, ratio 1.000027 (index build row)."""
    x, _ = common
    init, rcent, rlab, rin, _ = train_ref
    xd = torch.from_numpy(x).cuda()
    cent = torch.empty(105, D0, device="cuda"); lab = torch.empty(N0, dtype=torch.int32, device="cuda")
    inertia = np.zeros(11, dtype=np.float64)
    L.check(L.lib.rvc_index_train(L.get_ctx(0), L.current_stream(), L.ptr(xd), N0, D0, L.ptr(init), 105, 10, L.ptr(cent), L.ptr(lab), L.ptr(inertia)))
    cent, lab = cent.cpu().numpy(), lab.cpu().numpy()
    print("device inertia", " ".join(f"{v:.6e}" for v in inertia))
    print("float64 inertia", " ".join(f"{v:.6e}" for v in rin))
    # a step that follows an update with a split may go up; the device's own labels say where it split
    for i in range(1, 11):
        if inertia[i] > inertia[i - 1]:
            assert _device_split_happened(L, x, init, i - 1), f"inertia rose at step {i} without a split: {inertia[i - 1]} -> {inertia[i]}"
    assert inertia[10] < 0.5 * inertia[0]
    ratio = inertia[10] / rin[10]
    print(f"final inertia: device {inertia[10]:.6e}, float64 restatement {rin[10]:.6e}, ratio {ratio:.6f}")
    assert ratio <= 1.001
    check_assign(x, cent, lab, None, "labels of rvc_index_train against its centroids")


def _device_split_happened(L, x, init, step):
    """True when the update after assign step `step` of the device's run met an empty cluster (re-runs the device's first `step` iterations)."""
    xd = torch.from_numpy(x).cuda()
    K = init.shape[0]
    cent = torch.empty(K, x.shape[1], device="cuda"); lab = torch.empty(x.shape[0], dtype=torch.int32, device="cuda")
    L.check(L.lib.rvc_index_train(L.get_ctx(0), L.current_stream(), L.ptr(xd), x.shape[0], x.shape[1], L.ptr(init), K, step, L.ptr(cent), L.ptr(lab), None))
    return bool((np.bincount(lab.cpu().numpy(), minlength=K) == 0).any())


# ---------------------------------------------------------------------------------------------------- 4. end to end
@pytest.fixture(scope="module")
def built_index(common, tmp_path_factory):
    """train_index on the common input, read back and opened the way VC.load_index opens it, all 4099 stored rows searched once."""
    from comfy_rvc_amd.config import Config
    from comfy_rvc_amd.lib.faiss_io import read_index_vectors
    from comfy_rvc_amd.lib.feature_index import train_index
    from comfy_rvc_amd.pitch_extraction import FeatureExtractor
    x, _ = common
    path = str(tmp_path_factory.mktemp("index") / "a.index")
    assert train_index(x, path) == path
    big, info = read_index_vectors(path)
    index, big2 = FeatureExtractor(40000, Config()).load_index(path)
    assert index is not None and np.array_equal(big2, big)
    score, ix = index.search(big, k=1)
    return path, big, info, index, ix[:, 0], score[:, 0]


def test_train_index_end_to_end(L, common, built_index, tmp_path):
    from comfy_rvc_amd.lib.faiss_io import read_index_vectors
    from comfy_rvc_amd.lib.feature_index import train_index
    x, _ = common
    path, big, info, index, ix, score = built_index
    assert (info["kind"], info["nlist"], info["nprobe"], info["ntotal"]) == ("ivf_flat", 105, 1, N0)
    assert np.array_equal(big, x[np.random.default_rng(0).permutation(N0)])     # a permutation of x: the seeded shuffle
    assert index.ntotal == N0 and index.nprobe == 1
    own = ix == np.arange(N0)
    # a row may miss itself only when it is a near-tie between two cells (the file's float64 cell vs. the search's coarse quantiser)
    gap = ref_assign(big, info["centroids"])[3]
    share = float((gap < NEAR_TIE).mean())
    print(f"end to end: {int((~own).sum())} rows miss themselves, near-tie share {share:.4%}")
    assert share <= EXCUSED_CAP
    assert not (~own & ~(gap < NEAR_TIE)).any()
    path_b = str(tmp_path / "b.index")
    train_index(x, path_b)
    assert open(path, "rb").read() == open(path_b, "rb").read()
    path_c = str(tmp_path / "c.index")
    train_index(x, path_c, reduce_above=2000, reduce_to=500)
    _, info_c = read_index_vectors(path_c)
    assert info_c["ntotal"] == 500 and info_c["nlist"] == min(int(16 * np.sqrt(500)), 500 // 39) == 12


def test_train_index_self_distance(built_index):
    """Every stored row that retrieves itself does so at distance <= 1e-3: the search evaluates the winner's distance directly (a member of the index is
    at 0), not as |x|^2 - 2 score, whose three-term bf16 product left members at ~5e-6 |x|^2 (4.7e-3 on these rows)."""
    _, _, _, _, ix, score = built_index
    own = ix == np.arange(N0)
    print(f"self distance over {int(own.sum())} self-retrieving rows: mean {score[own].mean():.3e}, max {score[own].max():.3e}")
    assert (score[own] <= 1e-3).all(), f"self distance up to {score[own].max()}"


# ---------------------------------------------------------------------------------------------------- 5. under load
def test_assign_and_update_under_load(L, common):
    """Tests 1 and 2 while a second stream runs an unrelated split-resident GEMM loop: labels, distances, centroids and counts unchanged bit for bit."""
    x, cent = common
    lab0, dist0 = dev_assign(L, x, cent)
    rl = ref_assign(x, cent)[0]
    got0, cnt0 = dev_update(L, x, rl, cent)
    Ci, Co, T = 3072, 768, 1599
    g = torch.Generator().manual_seed(11)
    xg = torch.randn(Ci, T, generator=g).cuda()
    wn = (torch.randn(Co, Ci, generator=g) / np.sqrt(Ci)).contiguous().numpy()
    side = torch.cuda.Stream()
    ys = torch.empty(Co, T, device="cuda")
    torch.cuda.synchronize()
    stop, done, errors = threading.Event(), [0], []

    def load():                                             # its own host thread, so that its launches overlap the calls below
        try:
            torch.cuda.set_device(0)
            for _ in range(200):
                if stop.is_set():
                    break
                L.check(L.lib.rvc_op_gemm_split(C.c_void_p(side.cuda_stream), L.ptr(xg), L.ptr(wn), None, None, L.ptr(ys), None, Ci, Co, T, 0, 0.0, 0, 1.0,
                                                0, 0, 0, 1, 1))
                done[0] += 1
        except Exception as e:   # noqa: BLE001 - reported by the assert below
            errors.append(e)
    th = threading.Thread(target=load)
    th.start()
    try:
        for _ in range(3):
            lab, dist = dev_assign(L, x, cent)
            got, cnt = dev_update(L, x, rl, cent)
            assert np.array_equal(lab, lab0) and np.array_equal(dist.view(np.int32), dist0.view(np.int32))
            assert np.array_equal(got.view(np.int32), got0.view(np.int32)) and np.array_equal(cnt, cnt0)
    finally:
        stop.set()
        th.join()
    torch.cuda.synchronize()
    assert not errors and done[0] > 0, errors
    check_assign(x, cent, lab0, dist0, "assign under load")
