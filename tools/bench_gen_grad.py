"""Times the decoder's backward data pass on the device (rvc_synth_dec_input_grad) at B = 4, 40k v2, segment 32 with HIP events, median of --repeats, beside
  - the taped training forward (rvc_synth_forward_tape) and the fused training forward (rvc_synth_forward, the code before the tape existed) over the same
    items, each item exactly one segment long so that everything in front of the decoder is as small as it gets; their difference is what recording costs;
  - in a second pass with the tape's own events on (rvc_gen_tape_timing): the taped forward's DECODER alone (conv_pre .. y_hat) and the backward's split into
    tanh + conv_post, each stage, and conv_pre + conditioning + noise branch, summed over the items; the fused decoder is then the fused forward minus what the
    taped forward spends in front of its decoder (the same code in both);
  - float32 torch autograd (forward and backward) through the restated decoder (tests/gen_grad_ref.py) on --host-threads host threads;
  - the size of the backward's plan and the bytes of the tapes.
Writes profiles/gen_grad_bench.json (--out) and prints the same JSON line.

    python tools/bench_gen_grad.py --warmup 3 --repeats 20

The two forwards are whole-item times: the text encoder, the posterior encoder and the flow on 32 frames are inside both (and cancel in the difference).  Times are
end to end (host enqueue included); the event pass's intervals are stream time between two events of one item.
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_grad_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU (there is no CPU path)"
    from comfy_rvc_amd import _lib
    from comfy_rvc_amd.lib.infer_pack.models import SynthesizerTrnMs768NSFsid
    import gen_grad_ref as G
    config, B = S.CONFIG_40K_V2, a.batch
    seg, upp = config[1], int(np.prod(config[12]))
    sd = S.synth_train_state_dict(config, "v2", 0)
    net = SynthesizerTrnMs768NSFsid(*config, is_half=False)
    net.load_state_dict(sd)
    b = S.synth_train_batch(config, "v2", [seg] * B, seed=5)
    t = {k: torch.from_numpy(np.asarray(v)) for k, v in b.items()}
    gen = torch.Generator().manual_seed(1)
    noise = (torch.randn(B, config[2], seg, generator=gen), torch.randn(B, seg * upp, 1, generator=gen))
    ids = torch.zeros(B, dtype=torch.int64)
    args = (t["phone"], t["lengths"], t["pitch"], t["pitchf"], t["spec"], t["lengths"], t["sid"])
    d = torch.randn(B, seg * upp, generator=gen)
    d = (d / d.norm(dim=1, keepdim=True)).cuda()
    res, tape = net.forward_with_tape(*args, noise=noise, ids_slice=ids)
    dz = torch.empty(B, config[2], seg, device="cuda")
    dg = torch.empty(B, config[16], device="cuda")
    dhar = torch.empty(B, seg * upp, device="cuda")

    def backward():
        st = _lib.current_stream()
        for i in range(B):
            _lib.check(_lib.lib.rvc_synth_dec_input_grad(net._h, st, tape._h[i], _lib.ptr(d[i]), _lib.ptr(dz[i]), None, _lib.ptr(dg[i]), _lib.ptr(dhar[i])))

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
    fused, fused_min = timed(lambda: net.forward(*args, noise=noise, ids_slice=ids))
    taped, taped_min = timed(lambda: net.forward_with_tape(*args, noise=noise, ids_slice=ids, tape=tape))      # records into the same tapes: no allocation

    # second pass, the tape's events on: the decoder alone and the backward's stages, summed over the items, median over the repeats
    tape.set_timing(True)
    dec, stages = [], {}
    for r in range(a.warmup + a.repeats):
        net.forward_with_tape(*args, noise=noise, ids_slice=ids, tape=tape)
        backward()
        torch.cuda.synchronize()
        tm = [tape.times(i) for i in range(B)]
        if r >= a.warmup:
            dec.append(sum(x["decoder_forward"] for x in tm))
            for k in tm[0]["backward"]:
                stages.setdefault(k, []).append(sum(x["backward"][k] for x in tm))
    tape.set_timing(False)
    dec_taped = float(np.median(dec))
    stage_ms = {k: float(np.median(v)) for k, v in stages.items()}
    front = taped - dec_taped                     # what the taped forward spends outside its decoder: the same code in the fused forward
    dec_fused = fused - front

    torch.set_num_threads(a.host_threads)
    w = G.weights(sd, config, dtype=torch.float32)
    gv = torch.from_numpy(sd["emb_g.weight"])[0].view(1, -1, 1)
    zs = [tape.tensor(i, "z").cpu()[None] for i in range(B)]
    hs = [tape.tensor(i, "har").cpu()[None] for i in range(B)]
    dc = d.cpu()
    host = []
    for _ in range(a.host_repeats):
        t0 = time.perf_counter()
        for i in range(B):
            z = zs[i].clone().requires_grad_()
            y = G.forward(w, config, z, hs[i], gv)["y_hat"]
            torch.autograd.grad(y, z, grad_outputs=dc[i][None])
        host.append((time.perf_counter() - t0) * 1e3)
    out = {"what": "decoder backward data pass, 40k_v2, segment 32", "batch": B, "repeats": a.repeats,
           "backward_ms": bwd, "backward_min_ms": bwd_min,
           "forward_fused_ms": fused, "forward_fused_min_ms": fused_min, "forward_taped_ms": taped, "forward_taped_min_ms": taped_min,
           "tape_cost_ms": taped - fused, "backward_over_taped_forward": bwd / taped,
           "decoder_forward_taped_ms": dec_taped, "decoder_forward_fused_ms": dec_fused, "backward_events_ms": sum(stage_ms.values()),
           "backward_stage_ms": stage_ms, "backward_over_taped_decoder": sum(stage_ms.values()) / dec_taped,
           "host_float32_autograd_forward_backward_ms": float(np.median(host)), "host_threads": a.host_threads,
           "launches": net.dec_backward_launch_count(), "tape_bytes_per_item": tape.nbytes // B, "tape_bytes": tape.nbytes}
    line = json.dumps(out, sort_keys=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(line)


if __name__ == "__main__":
    main()
