"""Times the decoder's weight-gradient pass on the device (rvc_synth_dec_weight_grad) at B = 4, 40k v2, segment 32 with HIP events, median of --repeats, beside
  - the backward data pass (rvc_synth_dec_input_grad, one call per item) on the same tapes, measured again in the same run;
  - in a second pass with the tapes' own events on (rvc_gen_tape_timing): the taped forward's DECODER alone (conv_pre .. y_hat), summed over the items, and the
    weight pass split per stage (the up-sampler and the 18 ResBlock convolutions of a stage, GEMM and finish; then conv_pre and the direct kernels);
  - float32 torch autograd of the parameter gradients through the restated decoder (tests/gen_grad_ref.py) on --host-threads host threads;
  - the size of the plan, the bytes of the tapes with and without the two extra tensors a trainable net records.
Writes profiles/gen_wgrad_bench.json (--out) and prints the same JSON line.

    python tools/bench_gen_wgrad.py --warmup 3 --repeats 20

Times are end to end (host enqueue included); the event pass's intervals are stream time between two events.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_wgrad_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU (there is no CPU path)"
    from comfy_rvc_amd import _lib
    from comfy_rvc_amd.lib.infer_pack.models import SynthesizerTrnMs768NSFsid
    import gen_grad_ref as G
    config, B = S.CONFIG_40K_V2, a.batch
    seg, upp = config[1], int(np.prod(config[12]))
    sd = S.synth_train_state_dict(config, "v2", 0)
    net = SynthesizerTrnMs768NSFsid(*config, is_half=False, trainable=True)
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
    wg, wg_min = timed(lambda: net.dec_weight_grad(tape))

    tape.set_timing(True)
    dec, stages = [], {}
    for r in range(a.warmup + a.repeats):
        net.forward_with_tape(*args, noise=noise, ids_slice=ids, tape=tape)
        backward()
        net.dec_weight_grad(tape)
        torch.cuda.synchronize()
        if r >= a.warmup:
            dec.append(sum(tape.times(i)["decoder_forward"] for i in range(B)))
            for k, v in tape.wgrad_times().items():
                stages.setdefault(k, []).append(v)
    tape.set_timing(False)
    dec_taped = float(np.median(dec))
    stage_ms = {k: float(np.median(v)) for k, v in stages.items()}

    # float32 torch autograd of the parameter gradients through the restated decoder, the weight norm folded inside the graph
    torch.set_num_threads(a.host_threads)
    dec_sd = {k: torch.from_numpy(np.asarray(v)).clone().requires_grad_() for k, v in sd.items() if k.startswith("dec.") and "m_source" not in k}
    gv = torch.from_numpy(sd["emb_g.weight"])[0].view(1, -1, 1)
    zs = [tape.tensor(i, "z").cpu()[None] for i in range(B)]
    hs = [tape.tensor(i, "har").cpu()[None] for i in range(B)]
    dc = d.cpu()
    host = []
    for _ in range(a.host_repeats):
        t0 = time.perf_counter()
        w = G.weights(dec_sd, config, dtype=torch.float32)
        loss = 0.0
        for i in range(B):
            loss = loss + (G.forward(w, config, zs[i], hs[i], gv)["y_hat"] * dc[i][None]).sum()
        torch.autograd.grad(loss, list(dec_sd.values()))
        host.append((time.perf_counter() - t0) * 1e3)
    plain = SynthesizerTrnMs768NSFsid(*config, is_half=False)
    plain.load_state_dict(sd)
    _, ptape = plain.forward_with_tape(*args, noise=noise, ids_slice=ids)
    out = {"what": "decoder weight-gradient pass, 40k_v2, segment 32", "batch": B, "repeats": a.repeats,
           "weight_grad_ms": wg, "weight_grad_min_ms": wg_min, "backward_ms": bwd, "backward_min_ms": bwd_min,
           "decoder_forward_taped_ms": dec_taped, "weight_grad_events_ms": sum(stage_ms.values()), "weight_grad_stage_ms": stage_ms,
           "weight_grad_over_backward": wg / bwd, "weight_grad_over_taped_decoder": wg / dec_taped,
           "host_float32_autograd_forward_backward_ms": float(np.median(host)), "host_threads": a.host_threads,
           "launches": net.dec_weight_grad_launch_count(), "parameters": int(sum(int(np.prod(s)) for s in net.dec_parameter_shapes().values())),
           "tape_bytes_per_item": tape.nbytes // B, "tape_bytes_per_item_plain": ptape.nbytes // B}
    line = json.dumps(out, sort_keys=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(line)


if __name__ == "__main__":
    main()
