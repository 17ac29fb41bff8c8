"""Times the discriminators' optimizer step on the device - rvc_disc_adamw_step on MultiPeriodDiscriminatorV2 - with HIP events, beside, in the same run:
train_discriminator_step (the whole discriminator half of a trainer iteration at B = 4, T = 12800), losses.discriminator_grads, a device-to-device copy of
the step's algorithmic bytes (the yardstick of a pure streaming pass), and float32 torch.optim.AdamW plus the host re-fold (weight norm and the bf16 split
of every dense weight, vectorised) on the CPU.  Writes profiles/disc_optim_bench.json (--out) and prints the same JSON line.

    python tools/bench_disc_optim.py --warmup 3 --repeats 20

Algorithmic bytes of the step: 28 B per parameter for the update (p, m, v read and written, g read), 4 B per weight-normed parameter re-read by the fold
and 4 B per VALU-layer weight written by it, 4 B per dense weight re-read by the image pass and 8 B of images written for it (hi and lo, forward and
transposed).  The times are end to end (host enqueue included).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--T", type=int, default=12800)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disc_optim_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU (there is no CPU path)"
    from comfy_rvc_amd.lib.infer_pack.models import MultiPeriodDiscriminatorV2
    from comfy_rvc_amd.lib.train import losses as L
    from comfy_rvc_amd.lib.train.optim import AdamW
    from comfy_rvc_amd.lib.train.train_step import train_discriminator_step
    sd = S.disc_state_dict("v2", 0)
    net = MultiPeriodDiscriminatorV2(trainable=True).load_state_dict(sd)
    opt = AdamW(net, 1e-4, betas=(0.8, 0.99), eps=1e-9)
    y, y_hat = S.disc_waves(a.batch, a.T, 21)
    yd, yhd = torch.from_numpy(y).cuda(), torch.from_numpy(y_hat).cuda()
    _, grads = L.discriminator_grads(net, yd, yhd)
    clip = float(np.percentile(grads.flat[::16].abs().cpu().numpy(), 99.0))          # a clip that bites, as in the golden

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
    _, ms_step = timed(lambda: opt.step(grads, clip))
    _, ms_all = timed(lambda: train_discriminator_step(net, opt, yd, yhd, clip, a.batch))
    _, ms_grads = timed(lambda: L.discriminator_grads(net, yd, yhd))

    shapes = net.parameter_shapes()
    n_all = sum(int(np.prod(s)) for s in shapes.values())
    n_wn = sum(int(np.prod(s)) for k, s in shapes.items() if k.endswith(".weight_v"))
    n_dense = sum(int(np.prod(s)) for k, s in shapes.items() if k.endswith(".weight_v") and s[2] == 5 and s[1] % 16 == 0)
    step_bytes = 28 * n_all + 4 * n_wn + 4 * (n_wn - n_dense) + 12 * n_dense
    src = torch.empty(step_bytes // 8, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)                                                   # a copy reads and writes: half the bytes each way
    _, ms_copy = timed(lambda: dst.copy_(src))

    torch.set_num_threads(a.host_threads)
    params = [torch.nn.Parameter(torch.from_numpy(np.asarray(v, dtype=np.float32)).clone()) for v in sd.values()]
    hopt = torch.optim.AdamW(params, 1e-4, betas=(0.8, 0.99), eps=1e-9)
    hg = [t.cpu() for t in grads.values()]
    names = list(sd)
    host = []
    for _ in range(a.host_repeats + 1):
        t0 = time.perf_counter()
        for p, g in zip(params, hg):
            p.grad = g.clamp(-clip, clip)
        hopt.step()
        with torch.no_grad():
            for k, name in enumerate(names):
                if name.endswith(".weight_v"):
                    v, g = params[k], params[k - 1]
                    w = v * (g.double() / v.double().reshape(v.shape[0], -1).pow(2).sum(1).sqrt().reshape(g.shape)).float()
                    if v.shape[2] == 5 and v.shape[1] % 16 == 0:
                        hi = w.bfloat16()
                        lo = (w - hi.float()).bfloat16()
                        for img in (hi, lo):
                            img.contiguous()
                            img.transpose(0, 1).contiguous()
        host.append(time.perf_counter() - t0)
    host = host[1:]
    med = lambda v: float(np.median(v))
    out = {"batch": a.batch, "T": a.T, "version": "v2", "parameters": n_all, "dense_parameters": n_dense, "launches_step": net.adamw_step_launch_count(),
           "step_ms_median": round(med(ms_step), 3), "step_ms_min": round(min(ms_step), 3), "step_ms_max": round(max(ms_step), 3),
           "train_discriminator_step_ms_median": round(med(ms_all), 3), "train_discriminator_step_ms_min": round(min(ms_all), 3),
           "discriminator_grads_ms_median": round(med(ms_grads), 3), "discriminator_grads_ms_min": round(min(ms_grads), 3),
           "step_algorithmic_bytes": step_bytes, "copy_ms_median": round(med(ms_copy), 3), "copy_ms_min": round(min(ms_copy), 3),
           "step_over_copy": round(med(ms_step) / med(ms_copy), 2), "step_gbytes_per_s": round(step_bytes / (med(ms_step) * 1e-3) / 1e9, 1),
           "copy_gbytes_per_s": round(step_bytes / (med(ms_copy) * 1e-3) / 1e9, 1),
           "warmup": a.warmup, "repeats": a.repeats, "timer": "HIP events around the whole call (host enqueue included)",
           "host_fp32_adamw_and_refold_ms": round(1e3 * med(host), 1), "host_threads": torch.get_num_threads(), "host_repeats": a.host_repeats,
           "speedup_vs_host": round(1e3 * med(host) / med(ms_step), 1), "clip_value": clip}
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
