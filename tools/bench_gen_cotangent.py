"""Times the generator loss's cotangents on the device: the log-mel vector-Jacobian product against the forward it is the adjoint of, the multi-scale loss with
and without its gradient, and train_step.generator_loss_cotangents against a float32 torch autograd restatement on the host, all in the same run.

    python tools/bench_gen_cotangent.py [--out profiles/gen_cotangent_bench.json] [--reps 20] [--threads 16]

Shape: B = 4 segments of T = 12800 samples at 40 kHz (the trainer's segment_size); discriminators MultiPeriodDiscriminatorV2 with synthetic.disc_state_dict;
KL taps [4, 192, 32].  Device: HIP events around one call, median of --reps after 3 warm-up calls (the calls include their host plumbing: tables, launches,
and for generator_loss_cotangents the balancer's read-backs).  Per geometry of the multi-scale loss and the 40 kHz data setting (2048 / 400, 125 mels):
mel_spectrogram_vjp and, for the same signals, the forward STFT + mel projection (mel_spectrogram_torch); the adjoint runs one forward and one inverse FFT per
frame plus the gather, so it is read against the forward - no ratio is fixed in advance.  Host: the same loss restated with tests/disc_ref.py and
tests/gen_cotangent_ref.py in float32 and differentiated by torch.autograd on --threads threads, wall clock, median of --reps.  One JSON object is printed
and written to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import aux_loss_ref as R                                               # noqa: E402
import disc_ref as D                                                   # noqa: E402
import gen_cotangent_ref as G                                          # noqa: E402
from bench_aux_losses import device_ms, host_ms                        # noqa: E402

SR, B, T = 40000, 4, 12800
DATA = dict(n_fft=2048, hop=400, n_mels=125, fmin=0.0, fmax=None)
WEIGHTS = dict(loss_gen=1., loss_fm=2., loss_mel=45., loss_kl=1.)


def host_generator_loss_grads(W, wave, gen, y_mel, taps, mask):
    """float32 autograd of sum_k w_k loss_k (fixed weights: the balancer's arithmetic is scalar work) at y_hat and at the four KL taps"""
    y_hat = torch.from_numpy(gen)[:, None].clone().requires_grad_(True)
    y = torch.from_numpy(wave)[:, None]
    kl = [torch.from_numpy(t).clone().requires_grad_(True) for t in taps]
    scores, fmap_r, fmap_g = [], [], []
    for i, period in enumerate((0,) + D.PERIODS["v2"]):
        with torch.no_grad():
            fmap_r.append((D.disc_p(W, i, period, y) if period else D.disc_s(W, i, y))[1])
        s, f = D.disc_p(W, i, period, y_hat) if period else D.disc_s(W, i, y_hat)
        scores.append(s)
        fmap_g.append(f)
    loss = (WEIGHTS["loss_gen"] * D.generator_loss(scores)[0] + WEIGHTS["loss_fm"] * D.feature_loss(fmap_r, fmap_g)
            + WEIGHTS["loss_mel"] * G.mel_l1(y_mel, y_hat[:, 0], DATA["n_fft"], DATA["n_mels"], SR, DATA["hop"], DATA["fmin"], DATA["fmax"], torch.float32)
            + WEIGHTS["loss_kl"] * G.kl_loss(*kl, torch.from_numpy(mask)))
    return torch.autograd.grad(loss, [y_hat] + kl)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_cotangent_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    from comfy_rvc_amd import synthetic as S
    from comfy_rvc_amd.lib.infer_pack.models import MultiPeriodDiscriminatorV2
    from comfy_rvc_amd.lib.train import losses as L
    from comfy_rvc_amd.lib.train import mel_processing as MP
    from comfy_rvc_amd.lib.train.train_step import generator_loss_cotangents
    from comfy_rvc_amd.lib.train.utils import HParams
    torch.set_num_threads(args.threads)
    wave, gen = R.wave_pair(SR, B, T, 1)
    wd, gd = (torch.from_numpy(v).cuda()[:, None, :] for v in (wave, gen))
    out = {"shape": {"B": B, "T": T, "sampling_rate": SR}, "reps": args.reps, "host_threads": args.threads, "device": torch.cuda.get_device_name(0),
           "timing": "device: HIP events around one call, median; host: wall clock, median", "mel_spectrogram_vjp": {}}
    rng = np.random.default_rng(3)
    geometries = [(R.window_length(m), SR // 100, m, 50.0, SR // 2) for m in R.DEFAULT_N_MELS] + [tuple(DATA.values())]
    for n_fft, hop, n_mels, fmin, fmax in geometries:
        cot = torch.from_numpy(rng.standard_normal((B, n_mels, T // hop)).astype(np.float32)).cuda()
        fwd = device_ms(lambda: MP.mel_spectrogram_torch(gd, n_fft, n_mels, SR, hop, n_fft, fmin, fmax), args.reps)
        bwd = device_ms(lambda: MP.mel_spectrogram_vjp(gd, cot, n_fft, n_mels, SR, hop, n_fft, fmin, fmax), args.reps)
        out["mel_spectrogram_vjp"][f"{n_fft}_{hop}_{n_mels}"] = {"forward_ms": fwd, "vjp_ms": bwd, "vjp_over_forward": bwd / fwd}
    m = L.MultiScaleMelSpectrogramLoss(SR)
    fwd, both = device_ms(lambda: m.forward(gd, wd), args.reps), device_ms(lambda: m.forward_and_grad(gd, wd), args.reps)
    out["multiscale"] = {"forward_ms": fwd, "forward_and_grad_ms": both, "ratio": both / fwd}

    net = MultiPeriodDiscriminatorV2(False, device="cuda:0").load_state_dict(S.disc_state_dict("v2", 0))
    taps = [rng.standard_normal((B, 192, 32)).astype(np.float32) * s for s in (1.0, 0.3, 1.0, 0.3)]
    mask = np.ones((B, 1, 32), dtype=np.float32)
    taps_d, mask_d = [torch.from_numpy(t).cuda() for t in taps], torch.from_numpy(mask).cuda()
    hps = HParams(data=dict(filter_length=DATA["n_fft"], hop_length=DATA["hop"], win_length=DATA["n_fft"], n_mel_channels=DATA["n_mels"], sampling_rate=SR,
                            mel_fmin=DATA["fmin"], mel_fmax=DATA["fmax"]), train=dict(segment_size=T))
    y_mel_d = MP.mel_spectrogram_torch(wd, DATA["n_fft"], DATA["n_mels"], SR, DATA["hop"], DATA["n_fft"], DATA["fmin"], DATA["fmax"])
    bal = L.LossBalancer(None, initial_weights=dict(WEIGHTS), historical_losses={}, ema_weights={}, weights_decay=.75, loss_decay=.8, use_pareto=False, use_norm=True)
    dev = device_ms(lambda: generator_loss_cotangents(net, bal, wd, gd, y_mel_d, taps_d, mask_d, hps), args.reps)
    W = D.folded(S.disc_state_dict("v2", 0), torch.float32)
    y_mel = y_mel_d.cpu()
    host = host_ms(lambda: host_generator_loss_grads(W, wave, gen, y_mel, taps, mask), args.reps)
    out["generator_loss_cotangents"] = {"device_ms": dev, "host_autograd_ms": host, "speedup": host / dev}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
