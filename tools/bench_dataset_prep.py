"""Times dataset preparation for one hour of 40 kHz audio (the slicer test recording of synthetic.py, tiled) and prints ONE JSON line per part.

  --part device       the device path: rvc_lfilter_hp + rvc_frame_rms + rvc_slice_tags + rvc_cut_windows (lib/dataset_prep.py)
  --part per_window   the per-window route the device path replaces: one remix_audio -> resample_audio -> rvc_resample call per window
  --part reference    the reference's Slicer.slice on the host CPU (needs the reference tree, RVC_REFERENCE_ROOT: build container only)

Each part is its own process so that a GPU job can give each its own time limit and stop at the first failure:
  timeout -k 10 300 python tools/bench_dataset_prep.py --part device && timeout -k 10 600 python tools/bench_dataset_prep.py --part per_window
Launch counts are by construction (dataset_prep.hip: 5 for the filter, 1 for the RMS, 4 for the cut; the per-window route launches rvc_resample once
per window), not counted by a profiler.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def recording(seconds, sr):
    from comfy_rvc_amd import synthetic as S
    one = S.slicer_test_signal(sr, 0)
    return np.tile(one, int(np.ceil(seconds * sr / one.shape[0])))[: int(seconds * sr)]


def plan(x, sr):
    """(filtered device tensor, written windows, timings in ms) of the device path up to the cut."""
    import torch
    from comfy_rvc_amd.lib import dataset_prep as D
    sp = D.slicer_params(sr)
    xd = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    t = {}
    t0 = time.perf_counter()
    filt = D.lfilter_hp(xd, sr)
    torch.cuda.synchronize()
    t["filter_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    rms = D.frame_rms(filt, sp["win_size"], sp["hop_size"])
    torch.cuda.synchronize()
    t["rms_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    rms = rms.cpu().numpy()
    tags = D.slice_tags(rms, x.shape[0], sp)
    wins = [(s, l) for s, l, _, w in D.plan_windows(D.chunk_bounds(tags, rms.shape[0], sp["hop_size"], x.shape[0]), sr) if w]
    t["tags_and_plan_host_ms"] = (time.perf_counter() - t0) * 1e3
    return filt, wins, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["device", "per_window", "reference"], required=True)
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--sr", type=int, default=40000)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    x = recording(a.seconds, a.sr)
    out = {"part": a.part, "seconds": a.seconds, "sr": a.sr, "samples": int(x.shape[0])}
    if a.part == "reference":
        import importlib.util
        spec = importlib.util.spec_from_file_location("ref_slicer2", os.path.join(os.environ.get("RVC_REFERENCE_ROOT", "/root/reference"), "lib", "slicer2.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        sl = mod.Slicer(sr=a.sr, threshold=-50, min_length=1500, min_interval=400, hop_size=15, max_sil_kept=500)
        best = 1e30
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            chunks = sl.slice(x)
            best = min(best, time.perf_counter() - t0)
        out.update(host_slice_ms=best * 1e3, chunks=len(chunks))
    else:
        import torch
        from comfy_rvc_amd.lib import dataset_prep as D
        from comfy_rvc_amd.lib.audio import remix_audio
        plan(x[: a.sr * 15], a.sr)                                   # warm-up: code objects, scratch
        best = None
        for _ in range(a.repeat):
            filt, wins, t = plan(x, a.sr)
            if a.part == "device":
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gt, y16 = D.cut_windows(filt, wins, a.sr, 0.95)      # includes the copy of both packed outputs to the host
                t["cut_with_download_ms"] = (time.perf_counter() - t0) * 1e3
                t["total_ms"] = sum(t.values())
                if best is None or t["total_ms"] < best["total_ms"]:
                    best = t
        if a.part == "device":
            out.update(best, windows=len(wins), launches=5 + 1 + 4)
        else:
            host = filt.cpu().numpy()
            clips = [host[s:s + l].astype(np.float32) for s, l in wins]
            best = 1e30
            for _ in range(a.repeat):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for c in clips:
                    remix_audio((c, a.sr), target_sr=16000, max_volume=0.95)
                torch.cuda.synchronize()
                best = min(best, time.perf_counter() - t0)
            out.update(per_window_resample_ms=best * 1e3, windows=len(wins), launches=len(wins))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
