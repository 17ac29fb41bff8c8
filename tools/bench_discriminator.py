"""Times one trainer-shaped discriminator step on the device - net_d(wave, y_hat) plus discriminator_loss, generator_loss and feature_loss at B = 4,
T = 12800, MultiPeriodDiscriminatorV2 - with HIP events, against the float32 twin of the restatement (tests/disc_ref.py) on the host cores in the same run.
Writes profiles/disc_bench.json (--out) and prints the same JSON line.

    python tools/bench_discriminator.py --warmup 3 --repeats 20

FLOPs are computed from the shapes (2 per multiply-add of every convolution, all 2 B signals); the rate is that count over the event time of the whole call,
an end-to-end figure and not a kernel's share of peak.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from comfy_rvc_amd import synthetic as S                                        # noqa: E402


def forward_flops(net, S_, T):
    """2 x multiply-adds of every convolution for S_ signals, from the tap shapes and the layer table of synthetic.disc_spec"""
    spec = S.disc_spec("v2" if net.VERSION == 2 else "v1")
    total = 0
    for i, rows in enumerate(net.tap_shapes(T)):
        names = [n for n in spec if n.startswith(f"discriminators.{i}.") and n.endswith("weight_v")]
        for (c, h, p), n in zip(rows, names):
            co, ci_g, k = spec[n][:3]
            assert co == c
            total += 2 * S_ * c * h * p * ci_g * k
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--T", type=int, default=12800)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disc_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU (there is no CPU path)"
    from comfy_rvc_amd.lib.infer_pack.models import MultiPeriodDiscriminatorV2
    from comfy_rvc_amd.lib.train.losses import discriminator_loss, feature_loss, generator_loss
    import disc_ref as R
    sd = S.disc_state_dict("v2", 0)
    net = MultiPeriodDiscriminatorV2().load_state_dict(sd)
    y, y_hat = S.disc_waves(a.batch, a.T, 21)
    yd, yhd = torch.from_numpy(y).cuda(), torch.from_numpy(y_hat).cuda()

    def step():
        r = net(yd, yhd)
        return discriminator_loss(r[0], r[1])[0], generator_loss(r[1])[0], feature_loss(r[2], r[3])

    def fwd_only():
        return net(yd, yhd)

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
    losses, ms_step = timed(step)
    _, ms_fwd = timed(fwd_only)
    torch.set_num_threads(a.host_threads)
    W = R.folded(sd, torch.float32)                     # the fold is load-time work on both sides
    host = []
    for _ in range(a.host_repeats + 1):
        t0 = time.perf_counter()
        ref = R.forward(sd, "v2", y, y_hat, torch.float32, W=W)
        want = R.losses(ref)
        host.append(time.perf_counter() - t0)
    host = host[1:]
    flops = forward_flops(net, 2 * a.batch, a.T)
    got = dict(zip(("loss_disc", "loss_gen", "loss_fm"), (float(v) for v in losses)))
    out = {"batch": a.batch, "T": a.T, "version": "v2", "signals": 2 * a.batch, "launches_forward": net.launch_count(2 * a.batch, a.T),
           "forward_gflop": round(flops / 1e9, 2),
           "device_step_ms_median": round(float(np.median(ms_step)), 3), "device_step_ms_min": round(min(ms_step), 3), "device_step_ms_max": round(max(ms_step), 3),
           "device_forward_ms_median": round(float(np.median(ms_fwd)), 3), "device_forward_ms_min": round(min(ms_fwd), 3),
           "forward_tflops_end_to_end": round(flops / (float(np.median(ms_fwd)) * 1e-3) / 1e12, 2),
           "warmup": a.warmup, "repeats": a.repeats, "timer": "HIP events around the whole call (host enqueue included)",
           "host_fp32_step_ms": round(1e3 * float(np.median(host)), 1), "host_threads": torch.get_num_threads(), "host_repeats": a.host_repeats,
           "speedup_vs_host": round(1e3 * float(np.median(host)) / float(np.median(ms_step)), 1),
           "losses_device": got, "losses_host_fp32": want,
           "losses_rel_diff": {k: abs(got[k] - want[k]) / abs(want[k]) for k in want}}
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
