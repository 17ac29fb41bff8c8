"""Times the flow's weight-gradient pass on the device (rvc_synth_flow_weight_grad) at B = 4, 40k v2, items of 3 s (300 frames) with HIP events, median of
--repeats after --warmup, beside
  - the flow's data pass on the same (trainable) tapes, re-measured in the same job (rvc_synth_flow_input_grad, its three copies per coupling included);
  - the recording forward of a trainable net against a plain net's recording forward over the same items: the cost of the four additional tape tensors;
  - float32 torch autograd for the flow's parameters (forward and backward, weight norm explicit) through the restated flow (tests/flow_wgrad_ref.py,
    tests/flow_grad_ref.py) on --host-threads host threads;
  - the launch counts and the bytes of the tapes.
Writes profiles/flow_wgrad_bench.json (--out) and prints the same JSON line.  --only-pass: forward, data pass and --repeats weight-gradient passes and nothing
else, the run to put under `rocprofv3 --kernel-trace --stats` for the breakdown by launch class (profiles/flow_wgrad_kernel_stats.csv).

    python tools/bench_flow_wgrad.py --warmup 3 --repeats 20

Times are end to end (host enqueue included).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--only-pass", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_wgrad_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU (there is no CPU path)"
    from comfy_rvc_amd.lib.infer_pack.models import SynthesizerTrnMs768NSFsid
    import flow_wgrad_ref as W
    import flow_grad_ref as FR
    config, B, T = S.CONFIG_40K_V2, a.batch, a.frames
    seg, upp, IC = config[1], int(np.prod(config[12])), config[2]
    sd = S.synth_train_state_dict(config, "v2", 0)
    net = SynthesizerTrnMs768NSFsid(*config, is_half=False, trainable=True)
    net.load_state_dict(sd)
    b = S.synth_train_batch(config, "v2", [T] * B, seed=5)
    t = {k: torch.from_numpy(np.asarray(v)) for k, v in b.items()}
    gen = torch.Generator().manual_seed(1)
    noise = (torch.randn(B, IC, T, generator=gen), torch.randn(B, seg * upp, 1, generator=gen))
    ids = torch.zeros(B, dtype=torch.int64)
    args = (t["phone"], t["lengths"], t["pitch"], t["pitchf"], t["spec"], t["lengths"], t["sid"])
    d = torch.randn(B, IC, T, generator=gen)
    d = (d / d.flatten(1).norm(dim=1).view(B, 1, 1)).cuda()
    res, tape = net.forward_with_tape(*args, noise=noise, ids_slice=ids, record_flow=True)
    net.flow_input_grad(tape, d)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms))

    if a.only_pass:
        for _ in range(a.repeats):
            net.flow_weight_grad(tape)
        torch.cuda.synchronize()
        return
    wg, wg_min = timed(lambda: net.flow_weight_grad(tape))
    bwd, bwd_min = timed(lambda: net.flow_input_grad(tape, d))
    rec, rec_min = timed(lambda: net.forward_with_tape(*args, noise=noise, ids_slice=ids, tape=tape, record_flow=True))
    plain_net = SynthesizerTrnMs768NSFsid(*config, is_half=False)
    plain_net.load_state_dict(sd)
    _, tape_plain = plain_net.forward_with_tape(*args, noise=noise, ids_slice=ids, record_flow=True)
    rec_plain, rec_plain_min = timed(lambda: plain_net.forward_with_tape(*args, noise=noise, ids_slice=ids, tape=tape_plain, record_flow=True))
    bwd_plain, bwd_plain_min = timed(lambda: plain_net.flow_input_grad(tape_plain, d))

    # float32 autograd for the flow's parameters on the host: the raw tensors as leaves, the fold written out
    torch.set_num_threads(a.host_threads)
    raw = {k: torch.from_numpy(np.asarray(v)).float() for k, v in sd.items() if k.startswith("flow.")}
    emb = torch.from_numpy(sd["emb_g.weight"])
    zs, dc, mask = res[4][0].cpu(), d.cpu(), torch.ones(1, 1, T)
    host = []
    for _ in range(a.host_repeats):
        t0 = time.perf_counter()
        leaves = {k: v.clone().requires_grad_() for k, v in raw.items()}
        ws = W.folded_weights(leaves)
        loss = 0
        for i in range(B):
            z_p, _ = FR.forward(ws, zs[i:i + 1], mask, emb[int(b["sid"][i])].view(1, -1, 1))
            loss = loss + (z_p * dc[i:i + 1]).sum()
        torch.autograd.grad(loss, list(leaves.values()))
        host.append((time.perf_counter() - t0) * 1e3)
    out = {"what": f"flow weight-gradient pass, 40k_v2, {T} frames per item", "batch": B, "frames": T, "repeats": a.repeats,
           "weight_grad_ms": wg, "weight_grad_min_ms": wg_min,
           "data_pass_trainable_ms": bwd, "data_pass_trainable_min_ms": bwd_min, "data_pass_plain_ms": bwd_plain, "data_pass_plain_min_ms": bwd_plain_min,
           "weight_grad_over_data_pass": wg / bwd,
           "forward_recording_trainable_ms": rec, "forward_recording_trainable_min_ms": rec_min,
           "forward_recording_plain_ms": rec_plain, "forward_recording_plain_min_ms": rec_plain_min, "four_tensors_cost_ms": rec - rec_plain,
           "host_float32_autograd_forward_backward_ms": float(np.median(host)), "host_threads": a.host_threads,
           "weight_grad_launches": net.flow_weight_grad_launch_count(), "data_pass_launches_per_item_trainable": net.flow_backward_launch_count(),
           "data_pass_launches_per_item_plain": plain_net.flow_backward_launch_count(),
           "tape_bytes_per_item_trainable": tape.nbytes // B, "tape_bytes_per_item_plain": tape_plain.nbytes // B}
    line = json.dumps(out, sort_keys=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(line)


if __name__ == "__main__":
    main()
