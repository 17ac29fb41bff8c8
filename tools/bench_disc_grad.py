"""Times the trainer's gradient penalty on the device - gradient_norm_loss(wave, y_hat, net_d) at B = 4, T = 12800, MultiPeriodDiscriminatorV2: the
interpolation, one forward over the B interpolated signals, the loss cotangents, the input-gradient pass and the norms - with HIP events, beside the
input-gradient pass alone, the forward over the same B signals alone, and the float32 torch-autograd restatement (tests/disc_ref.py, what the term costs on
the host) in the same run.  Writes profiles/disc_grad_bench.json (--out) and prints the same JSON line.

    python tools/bench_disc_grad.py --warmup 3 --repeats 20

The data gradient of a convolution has the forward's multiply-adds, so the FLOPs of the backward pass are the forward's for the same signals (computed from
the shapes, tools/bench_discriminator.py); backward_over_forward is the ratio of the two event times.  The times are end to end (host enqueue included),
not a kernel's share of peak.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from comfy_rvc_amd import synthetic as S                                        # noqa: E402
from bench_discriminator import forward_flops                                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--T", type=int, default=12800)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disc_grad_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU (there is no CPU path)"
    from comfy_rvc_amd.lib.infer_pack.models import MultiPeriodDiscriminatorV2
    from comfy_rvc_amd.lib.train import losses as L
    import disc_ref as R
    sd = S.disc_state_dict("v2", 0)
    net = MultiPeriodDiscriminatorV2().load_state_dict(sd)
    y, y_hat = S.disc_waves(a.batch, a.T, 21)
    yd, yhd = torch.from_numpy(y).cuda(), torch.from_numpy(y_hat).cuda()
    alpha = torch.rand(a.batch, 1, 1, generator=torch.Generator().manual_seed(3))
    xd = torch.from_numpy((alpha * torch.from_numpy(y) + (1 - alpha) * torch.from_numpy(y_hat)).numpy()).cuda()
    fmaps = net.forward_single(xd)
    cots = L._score_cotangents(fmaps, 0)

    def timed(fn):
        for _ in range(a.warmup):
            out = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return out, ms
    pen, ms_pen = timed(lambda: L.gradient_norm_loss(yd, yhd, net, alpha=alpha))
    _, ms_bwd = timed(lambda: net.input_grad(fmaps, cots))
    _, ms_fwd = timed(lambda: net.forward_single(xd))

    torch.set_num_threads(a.host_threads)
    W = R.folded(sd, torch.float32)                     # the fold is load-time work on both sides
    yt, yht = torch.from_numpy(y), torch.from_numpy(y_hat)
    host = []
    for _ in range(a.host_repeats + 1):
        t0 = time.perf_counter()
        x = (alpha * yt + (1 - alpha) * yht).requires_grad_(True)
        loss = 0
        for i, period in enumerate((0,) + R.PERIODS["v2"]):
            score, _ = R.disc_p(W, i, period, x) if period else R.disc_s(W, i, x)
            loss = loss + torch.mean(score ** 2)
        g = torch.autograd.grad(loss, x)[0]
        want = float(((g.reshape(a.batch, -1).square().sum(-1).sqrt() - 1) ** 2).mean())
        host.append(time.perf_counter() - t0)
    host = host[1:]
    flops = forward_flops(net, a.batch, a.T)
    med = lambda v: float(np.median(v))
    out = {"batch": a.batch, "T": a.T, "version": "v2", "signals": a.batch, "launches_forward": net.launch_count(a.batch, a.T),
           "launches_backward": net.backward_launch_count(a.batch, a.T), "forward_gflop": round(flops / 1e9, 2), "backward_gflop": round(flops / 1e9, 2),
           "penalty_ms_median": round(med(ms_pen), 3), "penalty_ms_min": round(min(ms_pen), 3), "penalty_ms_max": round(max(ms_pen), 3),
           "backward_ms_median": round(med(ms_bwd), 3), "backward_ms_min": round(min(ms_bwd), 3),
           "forward_ms_median": round(med(ms_fwd), 3), "forward_ms_min": round(min(ms_fwd), 3),
           "backward_over_forward": round(med(ms_bwd) / med(ms_fwd), 2),
           "backward_tflops_end_to_end": round(flops / (med(ms_bwd) * 1e-3) / 1e12, 2), "forward_tflops_end_to_end": round(flops / (med(ms_fwd) * 1e-3) / 1e12, 2),
           "warmup": a.warmup, "repeats": a.repeats, "timer": "HIP events around the whole call (host enqueue included)",
           "host_fp32_autograd_ms": round(1e3 * med(host), 1), "host_threads": torch.get_num_threads(), "host_repeats": a.host_repeats,
           "speedup_vs_host": round(1e3 * med(host) / med(ms_pen), 1),
           "penalty_device": float(pen), "penalty_host_fp32": want, "penalty_rel_diff": abs(float(pen) - want) / abs(want)}
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
