"""Times the spectrogram cache over one hour of synthetic 40 kHz training clips (1455 clips of at most 3.7 s, the lengths Preprocess cuts) and
compares it with torch.stft on the host cores in the same run.  Prints one JSON line:
  kernel_ms   rvc_spectrogram_batch launches of all batches, by device events
  cache_wall_s  cache_spectrograms_trainset end to end: WAV reads, uploads, launches, download, torch.save of every .spec.pt
  host_stft_s   the reference's steps (clamp, reflect pad, torch.stft, magnitude) on the CPU for the same clips, without any file traffic
  usage: python tools/bench_spec_cache.py [--clips 1455] [--threads N]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1455)
    ap.add_argument("--threads", type=int, default=0, help="torch CPU threads of the host leg (0: torch's default)")
    args = ap.parse_args()
    from scipy.io import wavfile
    from comfy_rvc_amd import synthetic as S
    from comfy_rvc_amd.lib.train import mel_processing as MP
    from comfy_rvc_amd.preprocessing_utils import cache_spectrograms_trainset
    sr, n_fft, hop = 40000, 2048, 400
    rng = np.random.default_rng(0)
    lengths = [int(sr * rng.uniform(1.25, 3.7)) for _ in range(args.clips)]          # mean 2.475 s: 1455 clips = one hour
    base = S.spec_test_signal(sr, int(sr * 3.7), 0)
    clips = [np.roll(base, 997 * i)[:n].copy() for i, n in enumerate(lengths)]
    seconds = sum(lengths) / sr
    if args.threads:
        torch.set_num_threads(args.threads)

    # kernel time alone: the clips already on the device, batches as the cache forms them (256 MiB of output)
    dev = "cuda:0"
    per_batch = max(1, (256 << 20) // ((n_fft // 2 + 1) * 4 * (int(sr * 3.7) // hop + 16)))
    batches = [clips[i:i + per_batch] for i in range(0, len(clips), per_batch)]
    MP.spectrogram_batch(batches[0][:2], n_fft, hop, n_fft, device=dev)          # tables, scratch
    torch.cuda.synchronize()
    kernel_ms = 0.0
    for b in batches:
        audio = torch.from_numpy(np.concatenate(b)).to(dev)
        table, off, col = [], 0, 0
        for x in b:
            table.append((off, x.shape[0], col))
            off += x.shape[0]
            col += -(-(x.shape[0] // hop) // 16) * 16
        out = torch.empty(n_fft // 2 + 1, col, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        MP.spectrogram_packed(audio, np.array(table, dtype=np.int64), n_fft, hop, 1e-8, True, out)
        e1.record()
        torch.cuda.synchronize()
        kernel_ms += e0.elapsed_time(e1)
        del out, audio

    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "0_gt_wavs"))
        for i, x in enumerate(clips):
            wavfile.write(os.path.join(tmp, "0_gt_wavs", f"{i}_0.wav"), sr, x)
        t0 = time.perf_counter()
        n = cache_spectrograms_trainset(tmp, sr, dev)
        torch.cuda.synchronize()
        cache_wall = time.perf_counter() - t0
        assert n == len(clips)

    win = torch.hann_window(n_fft)
    pad = (n_fft - hop) // 2
    t0 = time.perf_counter()
    for x in clips:
        y = torch.from_numpy(x)[None].clamp(min=-1.05, max=1.05)
        y = torch.nn.functional.pad(y.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
        z = torch.view_as_real(torch.stft(y, n_fft, hop_length=hop, win_length=n_fft, window=win, center=False, return_complex=True))
        torch.sqrt(z.pow(2).sum(-1) + 1e-8)
    host_s = time.perf_counter() - t0
    print(json.dumps({"bench": "spec_cache", "clips": len(clips), "audio_seconds": round(seconds, 1), "batches": len(batches),
                      "kernel_ms": round(kernel_ms, 3), "cache_wall_s": round(cache_wall, 3), "host_stft_s": round(host_s, 3),
                      "host_threads": torch.get_num_threads()}))


if __name__ == "__main__":
    main()
