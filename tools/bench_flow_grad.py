"""Times the flow's backward data pass on the device (rvc_synth_flow_input_grad) at B = 4, 40k v2, items of 3 s (300 frames) with HIP events, median of
--repeats after --warmup, beside
  - the taped training forward with and without the flow recorded (rvc_synth_forward_tape_flow, record_flow 1 / 0) over the same items: their difference is what
    the recording costs (the 2 H pre-gate rows stored, the gate in a launch of its own, three copies of the residual stream per coupling);
  - in a second pass with the tape's own events on (rvc_gen_tape_timing): the recorded flow forward alone (four couplings and Flips) and the flow backward, summed
    over the items - the yardstick is that flow forward of the same run, and its share of the whole taped forward is reported;
  - float32 torch autograd (forward and backward) through the restated flow (tests/flow_grad_ref.py) on --host-threads host threads;
  - the size of the backward's plan and the bytes of the tapes.
Writes profiles/flow_grad_bench.json (--out) and prints the same JSON line.

    python tools/bench_flow_grad.py --warmup 3 --repeats 20

Times are end to end (host enqueue included); the event pass's intervals are stream time between two events of one item.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_grad_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU (there is no CPU path)"
    from comfy_rvc_amd import _lib
    from comfy_rvc_amd.lib.infer_pack.models import SynthesizerTrnMs768NSFsid
    import flow_grad_ref as FR
    config, B, T = S.CONFIG_40K_V2, a.batch, a.frames
    seg, upp, IC = config[1], int(np.prod(config[12])), config[2]
    sd = S.synth_train_state_dict(config, "v2", 0)
    net = SynthesizerTrnMs768NSFsid(*config, is_half=False)
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
    _, tape_plain = net.forward_with_tape(*args, noise=noise, ids_slice=ids)
    dz = torch.empty(B, IC, T, device="cuda")
    dg = torch.empty(B, config[16], device="cuda")

    def backward():
        st = _lib.current_stream()
        for i in range(B):
            _lib.check(_lib.lib.rvc_synth_flow_input_grad(net._h, st, tape._h[i], _lib.ptr(d[i]), T, _lib.ptr(dz[i]), _lib.ptr(dg[i])))

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

    bwd, bwd_min = timed(backward)
    plain, plain_min = timed(lambda: net.forward_with_tape(*args, noise=noise, ids_slice=ids, tape=tape_plain))
    rec, rec_min = timed(lambda: net.forward_with_tape(*args, noise=noise, ids_slice=ids, tape=tape, record_flow=True))

    # second pass, the tape's events on: the recorded flow forward and the flow backward alone, summed over the items, median over the repeats
    tape.set_timing(True)
    ff, fb = [], []
    for r in range(a.warmup + a.repeats):
        net.forward_with_tape(*args, noise=noise, ids_slice=ids, tape=tape, record_flow=True)
        backward()
        torch.cuda.synchronize()
        tm = [tape.flow_times(i) for i in range(B)]
        if r >= a.warmup:
            ff.append(sum(x["flow_forward"] for x in tm))
            fb.append(sum(x["flow_backward"] for x in tm))
    tape.set_timing(False)
    flow_fwd, flow_bwd = float(np.median(ff)), float(np.median(fb))

    torch.set_num_threads(a.host_threads)
    ws = FR.weights(sd, dtype=torch.float32)
    emb = torch.from_numpy(sd["emb_g.weight"])
    zs = res[4][0].cpu()
    dc, mask = d.cpu(), torch.ones(1, 1, T)
    host = []
    for _ in range(a.host_repeats):
        t0 = time.perf_counter()
        for i in range(B):
            z = zs[i:i + 1].clone().requires_grad_()
            g = emb[int(b["sid"][i])].view(1, -1, 1).clone().requires_grad_()
            z_p, _ = FR.forward(ws, z, mask, g)
            torch.autograd.grad(z_p, [z, g], grad_outputs=dc[i:i + 1])
        host.append((time.perf_counter() - t0) * 1e3)
    out = {"what": f"flow backward data pass, 40k_v2, {T} frames per item", "batch": B, "frames": T, "repeats": a.repeats,
           "backward_ms": bwd, "backward_min_ms": bwd_min,
           "forward_taped_ms": plain, "forward_taped_min_ms": plain_min, "forward_taped_recording_ms": rec, "forward_taped_recording_min_ms": rec_min,
           "recording_cost_ms": rec - plain,
           "flow_forward_recorded_events_ms": flow_fwd, "flow_backward_events_ms": flow_bwd, "backward_over_flow_forward": flow_bwd / flow_fwd,
           "flow_share_of_taped_recording_forward": flow_fwd / rec,
           "host_float32_autograd_forward_backward_ms": float(np.median(host)), "host_threads": a.host_threads,
           "launches_per_item": net.flow_backward_launch_count(), "tape_bytes_per_item": tape.nbytes // B,
           "tape_flow_bytes_per_item": (tape.nbytes - tape_plain.nbytes) // B}
    line = json.dumps(out, sort_keys=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(line)


if __name__ == "__main__":
    main()
