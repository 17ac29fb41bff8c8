"""Times the multi-scale mel loss and the HPSS / TSI auxiliary losses on the device against their host restatement, in the same run.

    python tools/bench_aux_losses.py [--out profiles/aux_loss_bench.json] [--reps 20] [--threads 16]

Shape: B = 4 segments of T = 12800 samples at 40 kHz (the trainer's segment_size), auxiliary losses at the 40 kHz data settings (n_fft 2048, hop 400,
125 mels).  Device: HIP events around one call, median of --reps after 3 warm-up calls (the calls include their host plumbing: tables, launches).
Baseline: the float32 restatement of tests/aux_loss_ref.py on --threads host threads - torch for the STFTs, projections and reductions,
scipy.ndimage.median_filter for the ten medians of each HPSS, which is how the reference computes that term (on the host, per batch) - median of --reps
wall-clock times.  One JSON object is printed and written to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import aux_loss_ref as R                                               # noqa: E402

SR, B, T = 40000, 4, 12800
AUX = dict(n_mels=125, n_fft=2048, hop=400)
EPS = float(torch.finfo(torch.float32).eps)


def device_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def host_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def host_harmonic(om, gm):
    """harmonic loss with the medians by scipy.ndimage, as the reference's host round trip computes them."""
    from scipy.ndimage import median_filter

    def parts(mag):
        S = np.abs(mag.numpy())
        H, P = [], []
        for k in R.HPSS_SIZES:
            a, b = R.soft_masks(torch.from_numpy(median_filter(S, size=(1, 1, k), mode="reflect")), torch.from_numpy(median_filter(S, size=(1, k, 1), mode="reflect")))
            H.append(torch.from_numpy(S) * a)
            P.append(torch.from_numpy(S) * b)
        return R.minmax(torch.cat(H, -1), EPS), R.minmax(torch.cat(P, -1), EPS)
    (oh, op), (gh, gp) = parts(om), parts(gm)
    return float((gh - oh).abs().mean() + (gp - op).abs().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aux_loss_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    from comfy_rvc_amd.lib.train import losses as L
    from comfy_rvc_amd.lib.train.mel_processing import mel_spectrogram_torch
    torch.set_num_threads(args.threads)
    wave, gen = R.wave_pair(SR, B, T, 1)
    wd, gd = (torch.from_numpy(v).cuda()[:, None, :] for v in (wave, gen))
    m = L.MultiScaleMelSpectrogramLoss(SR)
    kw = dict(n_mels=AUX["n_mels"], sample_rate=SR, n_fft=AUX["n_fft"], hop_length=AUX["hop"], win_length=AUX["n_fft"], fmin=0.0, fmax=None, eps=EPS)
    mag = mel_spectrogram_torch(torch.cat([wd, gd]), AUX["n_fft"], AUX["n_mels"], SR, AUX["hop"], AUX["n_fft"], 0.0, None)
    om_d, gm_d = mag[:B].contiguous(), mag[B:].contiguous()
    om, gm = R.aux_mags(wave, gen, AUX["n_mels"], SR, AUX["n_fft"], AUX["hop"], 0.0, None, torch.float32)
    f32 = torch.float32
    rows = {
        "multiscale_mel_loss": (lambda: m(gd, wd), lambda: R.multiscale(gen, wave, SR, dtype=f32)),
        "harmonic_loss": (lambda: L.harmonic_loss(om_d, gm_d, eps=EPS), lambda: host_harmonic(om, gm)),
        "tsi_loss": (lambda: L._tsi_terms(om_d, gm_d, EPS), lambda: R.tsi_loss(om, gm, EPS, f32)),
        "combined_aux_loss": (lambda: L.combined_aux_loss(wd, gd, c_tefs=0.0, c_hd=1.0, c_tsi=1.0, **kw),
                              lambda: (lambda a, b: (host_harmonic(a, b), R.tsi_loss(a, b, EPS, f32)))(
                                  *R.aux_mags(wave, gen, AUX["n_mels"], SR, AUX["n_fft"], AUX["hop"], 0.0, None, f32))),
    }
    out = {"shape": {"B": B, "T": T, "sampling_rate": SR, **AUX}, "reps": args.reps, "host_threads": args.threads,
           "device": torch.cuda.get_device_name(0), "timing": "device: HIP events around one call, median; host: wall clock, median"}
    for name, (dev_fn, host_fn) in rows.items():
        d, h = device_ms(dev_fn, args.reps), host_ms(host_fn, args.reps)
        out[name] = {"device_ms": d, "host_ms": h, "speedup": h / d}
    dev_vals = [float(m(gd, wd)), float(L.harmonic_loss(om_d, gm_d, eps=EPS)), float(L._tsi_terms(om_d, gm_d, EPS).sum())]
    host_vals = [R.multiscale(gen, wave, SR, dtype=f32)[1], host_harmonic(om, gm), R.tsi_loss(om, gm, EPS, f32)]
    out["values"] = {"device": dev_vals, "host": host_vals}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
