"""Times the discriminators' weight-gradient pass on the device - net_d.weight_grad over the 2 B signals of one discriminator step at B = 4, T = 12800,
MultiPeriodDiscriminatorV2 - with HIP events, beside, in the same run: the forward and the input-gradient pass over the same signals (the yardsticks: the
weight gradient of a convolution has the forward's multiply-adds), the whole losses.discriminator_grads (forward, loss, cotangents, both backward passes),
and float32 torch autograd of the restatement (tests/disc_ref.py with the weight norm applied, what the step's backward costs on the host).  Writes
profiles/disc_wgrad_bench.json (--out) and prints the same JSON line.

    python tools/bench_disc_wgrad.py --warmup 3 --repeats 20

The times are end to end (host enqueue included), not a kernel's share of peak.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disc_wgrad_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU (there is no CPU path)"
    from comfy_rvc_amd.lib.infer_pack.commons import clip_grad_value_
    from comfy_rvc_amd.lib.infer_pack.models import MultiPeriodDiscriminatorV2
    from comfy_rvc_amd.lib.train import losses as L
    import disc_ref as R
    sd = S.disc_state_dict("v2", 0)
    net = MultiPeriodDiscriminatorV2(trainable=True).load_state_dict(sd)
    y, y_hat = S.disc_waves(a.batch, a.T, 21)
    yd, yhd = torch.from_numpy(y).cuda(), torch.from_numpy(y_hat).cuda()
    xd = torch.cat([yd, yhd]).contiguous()
    S_ = 2 * a.batch
    fmaps = net.forward_single(xd)
    real, fake = [torch.flatten(d[-1][:a.batch], 1, -1) for d in fmaps], [torch.flatten(d[-1][a.batch:], 1, -1) for d in fmaps]
    scale = [2.0 / t.numel() for t in real]
    cots = [[None] * (len(d) - 1) + [torch.cat([r, g]).reshape(d[-1].shape)]
            for d, r, g in zip(fmaps, L._cotangents(1, real, None, scale), L._cotangents(0, fake, None, scale))]
    _, deltas = net.input_grad(fmaps, cots, return_deltas=True)

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
    grads, ms_wg = timed(lambda: net.weight_grad(xd, fmaps, deltas))
    _, ms_bwd = timed(lambda: net.input_grad(fmaps, cots))
    _, ms_fwd = timed(lambda: net.forward_single(xd))
    (loss, _), ms_all = timed(lambda: L.discriminator_grads(net, yd, yhd))
    norm = clip_grad_value_(grads.values(), None, batch_size=a.batch)

    torch.set_num_threads(a.host_threads)
    f32 = {k: np.asarray(v, dtype=np.float32) for k, v in sd.items()}
    yt, yht = torch.from_numpy(y), torch.from_numpy(y_hat)
    host = []
    for _ in range(a.host_repeats + 1):
        t0 = time.perf_counter()
        leaves = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in f32.items()}
        W = {}
        for k in f32:
            if k.endswith(".bias"):
                v, g = leaves[k[:-5] + ".weight_v"], leaves[k[:-5] + ".weight_g"]
                W[k[:-5]] = (v * (g / v.reshape(v.shape[0], -1).norm(dim=1).reshape(g.shape)), leaves[k])
        hl = 0
        for i, period in enumerate((0,) + R.PERIODS["v2"]):
            sr, _ = R.disc_p(W, i, period, yt) if period else R.disc_s(W, i, yt)
            sg, _ = R.disc_p(W, i, period, yht) if period else R.disc_s(W, i, yht)
            hl = hl + torch.mean((1 - sr) ** 2) + torch.mean(sg ** 2)
        hl.backward()
        want = float(np.sqrt(sum(float(p.grad.double().norm() / a.batch) ** 2 for p in leaves.values())))
        host.append(time.perf_counter() - t0)
    host = host[1:]
    flops = forward_flops(net, S_, a.T)
    med = lambda v: float(np.median(v))
    out = {"batch": a.batch, "T": a.T, "version": "v2", "signals": S_, "launches_forward": net.launch_count(S_, a.T),
           "launches_input_grad": net.backward_launch_count(S_, a.T), "launches_weight_grad": net.weight_grad_launch_count(S_, a.T),
           "forward_gflop": round(flops / 1e9, 2), "weight_grad_gflop": round(flops / 1e9, 2),
           "weight_grad_ms_median": round(med(ms_wg), 3), "weight_grad_ms_min": round(min(ms_wg), 3), "weight_grad_ms_max": round(max(ms_wg), 3),
           "input_grad_ms_median": round(med(ms_bwd), 3), "input_grad_ms_min": round(min(ms_bwd), 3),
           "forward_ms_median": round(med(ms_fwd), 3), "forward_ms_min": round(min(ms_fwd), 3),
           "discriminator_grads_ms_median": round(med(ms_all), 3), "discriminator_grads_ms_min": round(min(ms_all), 3),
           "weight_grad_over_forward": round(med(ms_wg) / med(ms_fwd), 2),
           "weight_grad_tflops_end_to_end": round(flops / (med(ms_wg) * 1e-3) / 1e12, 2), "forward_tflops_end_to_end": round(flops / (med(ms_fwd) * 1e-3) / 1e12, 2),
           "warmup": a.warmup, "repeats": a.repeats, "timer": "HIP events around the whole call (host enqueue included)",
           "host_fp32_autograd_ms": round(1e3 * med(host), 1), "host_threads": torch.get_num_threads(), "host_repeats": a.host_repeats,
           "speedup_vs_host": round(1e3 * med(host) / med(ms_all), 1),
           "loss_disc_device": float(loss), "loss_disc_host_fp32": float(hl), "grad_norm_d_device": norm, "grad_norm_d_host_fp32": want,
           "grad_norm_d_rel_diff": abs(norm - want) / abs(want)}
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
