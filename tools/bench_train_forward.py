"""Times lib/train/evaluate.py::evaluate_checkpoint over N synthetic clips of 3 s (40k, v2, f0) on the device against the torch restatement of the same
forward and losses (tests/train_forward_ref.py, reference-shaped modules on the host cores) in the same run.  Prints one JSON line.

    python tools/bench_train_forward.py --clips 64 --batch-size 4
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from comfy_rvc_amd import synthetic as S                                        # noqa: E402
from comfy_rvc_amd.lib.train.utils import HParams                               # noqa: E402

HOP, SR, FRAMES = 400, 40000, 300          # 3 s clips


def write_dataset(root, n, seed=0):
    """n clips of 3 s: IEEE-float WAV, 768-d features at 50 fps, pitch, a spectrogram-like {clip}.spec.pt (the loaders then never compute one)."""
    from scipy.io import wavfile
    dirs = {k: os.path.join(root, k) for k in ("0_gt_wavs", "2a_f0", "2b-f0nsf", "3_feature768")}
    for d in dirs.values():
        os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        wav = os.path.join(dirs["0_gt_wavs"], f"{i}_0.wav")
        wavfile.write(wav, SR, S.spec_test_signal(SR, FRAMES * HOP, seed + i))
        paths = [os.path.join(dirs[k], f"{i}_0.npy") for k in ("3_feature768", "2a_f0", "2b-f0nsf")]
        np.save(paths[0], (rng.standard_normal((FRAMES // 2, 768)) * 0.5).astype(np.float32))
        np.save(paths[1], rng.integers(1, 256, size=FRAMES).astype(np.int64))
        np.save(paths[2], S.designed_f0(FRAMES + i)[i:].astype(np.float32))
        torch.save(torch.from_numpy(S.synth_posterior_input(S.CONFIG_40K_V2, [FRAMES], seed + i)[0]), wav.replace(".wav", ".spec.pt"),
                   _use_new_zipfile_serialization=False)
        rows.append("|".join([wav] + paths + [str(i % 3)]))
    filelist = os.path.join(root, "filelist.txt")
    with open(filelist, "w", encoding="utf-8") as f:
        f.write("\n".join(rows) + "\n")
    return filelist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--host-clips", type=int, default=4, help="clips the host restatement is timed on (scaled to --clips)")
    a = ap.parse_args()
    from comfy_rvc_amd.lib.train.evaluate import evaluate_checkpoint, load_generator
    import train_forward_ref as R
    cfg = S.CONFIG_40K_V2
    hps = HParams(data=dict(filter_length=2048, hop_length=HOP, win_length=2048, n_mel_channels=125, sampling_rate=SR, mel_fmin=0.0, mel_fmax=None,
                            max_wav_value=32768.0), train=dict(segment_size=32 * HOP),
                  model=dict(inter_channels=cfg[2], hidden_channels=cfg[3], filter_channels=cfg[4], n_heads=cfg[5], n_layers=cfg[6], kernel_size=cfg[7],
                             p_dropout=0, resblock="1", resblock_kernel_sizes=cfg[10], resblock_dilation_sizes=cfg[11], upsample_rates=cfg[12],
                             upsample_initial_channel=cfg[13], upsample_kernel_sizes=cfg[14], spk_embed_dim=cfg[15], gin_channels=cfg[16]))
    sd = S.synth_train_state_dict(cfg)
    with tempfile.TemporaryDirectory() as tmp:
        filelist = write_dataset(tmp, a.clips)
        net = load_generator({"model": sd}, hps)
        evaluate_checkpoint(net, filelist, hps, batch_size=a.batch_size)      # warm-up: arenas, file cache
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = evaluate_checkpoint(net, filelist, hps, batch_size=a.batch_size)
        torch.cuda.synchronize()
        dev_s = time.perf_counter() - t0
    n = min(a.host_clips, a.clips)
    b = S.synth_train_batch(cfg, "v2", [FRAMES] * n, seed=1)
    g = torch.Generator().manual_seed(0)
    nq, ns = torch.randn(n, cfg[2], FRAMES, generator=g), torch.randn(n, 32 * 400, 1, generator=g)
    t0 = time.perf_counter()
    out = R.forward(sd, cfg, b["phone"], b["lengths"], b["pitch"], b["pitchf"], b["spec"], b["sid"], nq, ns, [0] * n)
    R.kl_loss(out["z_p"], out["logs_q"], out["m_p"], out["logs_p"], np.ones((n, 1, FRAMES)))
    host_s = (time.perf_counter() - t0) * a.clips / n
    print(json.dumps({"clips": a.clips, "batch_size": a.batch_size, "device_s": round(dev_s, 4), "host_s_scaled": round(host_s, 3), "host_clips_timed": n,
                      "host_threads": torch.get_num_threads(), "speedup": round(host_s / dev_s, 1), "loss_mel": r["loss_mel"], "loss_kl": r["loss_kl"]}))


if __name__ == "__main__":
    main()
