"""Times the index build on the GPU: lib/feature_index.py::build_ivf (upload, 10 Lloyd iterations, final assignment, download) and its assign step
alone (rvc_kmeans_assign on resident rows), at the reference's largest un-reduced size 200 000 x 768 (nlist 5128) and at 20 000 x 768.

HIP events, one warm-up, median of 5 runs.  The assign step is priced at its algorithmic 2 N K D FLOP against the 833 TFLOP/s split-bf16 roofline
(three bf16 MFMAs per fp32 product).  A plain tool: bench.py does not call it, nothing is gated on its numbers.

    python tools/bench_index_build.py [--sizes 200000,20000] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from comfy_rvc_amd import _lib  # noqa: E402
from comfy_rvc_amd.lib.feature_index import build_ivf, default_nlist  # noqa: E402

ROOFLINE_TFLOPS = 833.0


def timed(fn, runs=5):
    fn()                                                    # warm-up (scratch allocation, code upload)
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def features(n, d=768, blobs=64, seed=0):
    r = np.random.default_rng(seed)
    c = r.standard_normal((blobs, d), dtype=np.float32)
    return c[r.integers(0, blobs, n)] + np.float32(0.35) * r.standard_normal((n, d), dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200000,20000")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ctx = _lib.get_ctx(0)
    out = []
    for n in (int(v) for v in args.sizes.split(",")):
        x = features(n)
        d, k = x.shape[1], default_nlist(n)
        res = {}

        def build():
            res["inertia"] = build_ivf(x, niter=10, seed=0)[2]
        build_ms = timed(build)
        xd = torch.from_numpy(x).cuda()
        cd = xd[torch.from_numpy(np.random.default_rng(0).permutation(n)[:k]).cuda()].contiguous()
        lab = torch.empty(n, dtype=torch.int32, device="cuda")
        dist = torch.empty(n, device="cuda")

        def assign():
            _lib.check(_lib.lib.rvc_kmeans_assign(ctx, _lib.current_stream(), _lib.ptr(xd), n, d, _lib.ptr(cd), k, _lib.ptr(lab), _lib.ptr(dist)))
        assign_ms = timed(assign)
        tflops = 2.0 * n * k * d / (assign_ms * 1e-3) / 1e12
        row = {"rows": n, "dim": d, "nlist": k, "niter": 10, "build_ivf_ms": round(build_ms, 2), "assign_ms": round(assign_ms, 3),
               "assign_tflops": round(tflops, 1), "assign_fraction_of_833": round(tflops / ROOFLINE_TFLOPS, 3),
               "inertia_first": float(res["inertia"][0]), "inertia_last": float(res["inertia"][-1])}
        print(json.dumps(row))
        out.append(row)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
