"""Times the audio effects of the audio nodes on the device against scipy / numpy on the host, in one run.

Input: a 240 s, 44.1 kHz mono track (synthetic.slicer_test_signal segments repeated, with the click recipe inside the voiced parts only).
  chain   upload -> silence gate -> click removal (median, sample_size 16000) -> normalise -> download: HIP events around the device part and wall
          clock around the whole route; the same three steps with numpy / scipy on the host (the reference's formulas).
  merge   four tracks of unequal length, median: device (events, wall clock incl. upload and download) against np.nanmedian of the padded stack.
Launch counts are by construction (lib/audio_fx.py::LAUNCHES) and the same for 1 s and 240 s of audio, which the tool asserts by running both.
Prints one JSON line; --out FILE also writes it there.  Warm-up first, best of `--repeat` runs (host: best of 2).
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


def track(seconds, sr, seed):
    from comfy_rvc_amd import synthetic as S
    unit = (("s", 1.7), ("v", 4.2), ("s", 0.7), ("v", 3.1), ("s", 2.3))
    reps = int(np.ceil(seconds / sum(s for _, s in unit)))
    x = S.slicer_test_signal(sr, seed, unit * reps)[:int(seconds * sr)]
    y, pos = S.add_clicks(x, seed)
    quiet = np.abs(x[pos]) < 1e-2                    # impulses inside a silence would lift its windows over the gate's threshold
    y[pos[quiet]] = x[pos[quiet]]
    return y


def host_chain(x, sr):
    from scipy.ndimage import median_filter, uniform_filter1d
    w, min_size, fade = int(.5 * sr), int(sr), int(.3 * sr)
    a = x.copy()
    start = end = 0
    n = a.shape[0]
    for i in range(0, n, w):
        seg = np.pad(a[i:i + w], w // 2)
        nf = 1 + (seg.shape[0] - w) // w
        rms = max(np.sqrt(np.mean(seg[f * w:f * w + w] ** 2)) for f in range(nf))
        if 20 * np.log10(max(1e-5, rms)) < -50:
            end = i + w
            if i >= n - w and end - start > min_size:
                if start > fade:
                    a[start:start + fade] *= np.linspace(1., 0., fade)
                    start += fade
                a[start:n] = 0.
                break
        else:
            if end - start > min_size:
                if start > fade:
                    a[start:start + fade] *= np.linspace(1., 0., fade)
                    start += fade
                if end < n - fade:
                    a[end - fade:end] *= np.linspace(0., 1., fade)
                    end -= fade
                a[start:end] = 0.
            start = i
    clicks = np.abs(a) > 2.0 * np.sqrt(uniform_filter1d(np.square(a), size=16000))
    a[clicks] = median_filter(a, size=5)[clicks]
    a -= np.mean(a)
    peak = np.max(np.abs(a))
    if peak > 0:
        a /= peak
        a *= 10 ** (-1 / 20)
    return a


def best(fn, repeat):
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--sr", type=int, default=44100)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from comfy_rvc_amd.lib import audio_fx
    from comfy_rvc_amd.lib.audio import AudioProcessor, pad_audio

    proc = AudioProcessor()
    out = {"seconds": args.seconds, "sr": args.sr}
    launches = {}
    for seconds in (1.0, args.seconds):
        x = track(seconds, args.sr, 5)
        proc(x, args.sr)                              # warm-up (scratch allocation, code objects)
        launches[seconds] = audio_fx.LAUNCHES["gate"] + audio_fx.LAUNCHES["declick_median"] + audio_fx.LAUNCHES["normalize"]
    assert launches[1.0] == launches[args.seconds]
    out["chain_launches"] = launches[args.seconds]

    def device_part(xd):
        y = audio_fx.silence_gate(xd, args.sr, -50)
        y = audio_fx.declick(y, multiplier=2.0, sample_size=16000, method="median", kernel_size=5)
        return audio_fx.peak_normalize(y, -1)

    ev = []
    for _ in range(args.repeat):
        xd = torch.from_numpy(x).cuda()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = device_part(xd)
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
    out["chain_device_ms"] = min(ev)
    out["chain_route_wall_ms"] = best(lambda: proc(x, args.sr), args.repeat) * 1e3
    out["chain_host_ms"] = best(lambda: host_chain(x, args.sr), 2) * 1e3
    ref = host_chain(x, args.sr)
    out["chain_max_abs_diff_vs_host"] = float(np.abs(y.cpu().numpy() - ref).max())

    tracks = [track(args.seconds - 3.3 * j, args.sr, 6 + j) for j in range(4)]
    audio_fx.merge_tracks(tracks, "median")
    td = [torch.from_numpy(t).cuda() for t in tracks]
    ev = []
    for _ in range(args.repeat):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m = audio_fx.merge_tracks(td, "median")
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
    out["merge_device_ms"] = min(ev)
    out["merge_route_wall_ms"] = best(lambda: audio_fx.merge_tracks(tracks, "median").cpu().numpy(), args.repeat) * 1e3
    out["merge_host_ms"] = best(lambda: np.nanmedian(pad_audio(*tracks, axis=0), axis=0), 2) * 1e3
    out["merge_equal_to_numpy"] = bool(np.array_equal(m.cpu().numpy(), np.nanmedian(pad_audio(*tracks, axis=0), axis=0)))
    out["merge_launches"] = audio_fx.LAUNCHES["merge"]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
