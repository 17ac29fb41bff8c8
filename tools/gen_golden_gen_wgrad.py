"""Writes tests/golden/gen_wgrad_40k_v2.npz by running the REAL reference's GeneratorNSF (imported through oracle/ref_shim.py) under float32 autograd: the
gradient of every dec.* parameter for the case of tools/gen_golden_gen_grad.py (item 0 of train_forward_40k_v2.npz, the reference's own z on the slice, that
golden's noise tape, the cotangent stored in gen_grad_40k_v2.npz).

Build container only (needs the reference tree); no test and no GPU job runs this.

    python tools/gen_golden_gen_wgrad.py

Stored: `names`, the dec.* parameter names in the reference module's state-dict order (checked here against synthetic.synth_train_state_dict's order, which
is what the library's parameter list follows); `norms`, each gradient's L2 norm; `sample.{k}`, every `stride`-th element of gradient k flattened.  The file
holds data only.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from oracle import ref_shim                                            # noqa: E402
from oracle.gen_golden import to_torch_sd, OUT                          # noqa: E402
from comfy_rvc_amd import synthetic as S                                # noqa: E402
from gen_golden_gen_grad import OneDraw                                 # noqa: E402

STRIDE = 97


def main():
    ns = ref_shim.load_reference()
    config, version = S.CONFIG_40K_V2, "v2"
    g = dict(np.load(os.path.join(OUT, "train_forward_40k_v2.npz")))
    gg = dict(np.load(os.path.join(OUT, "gen_grad_40k_v2.npz")))
    seg = config[1]
    sd = S.synth_train_state_dict(config, version, int(g["weight_seed"]))
    net = ns.models.SynthesizerTrnMs768NSFsid(*config, is_half=False)
    net.load_state_dict(to_torch_sd(sd), strict=True)
    net.eval()
    names = [k for k in net.state_dict() if k.startswith("dec.")]
    assert names == [k for k in sd if k.startswith("dec.")], "the synthetic state dict's dec.* order is not the reference module's"
    params = dict(net.named_parameters())
    batch = S.synth_train_batch(config, version, [int(x) for x in g["lengths"]], int(g["input_seed"]))
    gen = torch.Generator().manual_seed(int(g["noise_seed"]))
    draws = [torch.randn(tuple(int(v) for v in s), generator=gen) for s in g["draw_shapes"]]
    i0 = int(g["ids_slice"][0])
    assert i0 == int(gg["ids"])
    z = torch.from_numpy(g["z"][0:1, :, i0:i0 + seg]).clone()
    pitchf = torch.from_numpy(batch["pitchf"][0:1, i0:i0 + seg])
    gv = net.emb_g(torch.from_numpy(batch["sid"][0:1])).unsqueeze(-1).detach()
    with OneDraw(draws[1][0:1]) as tape:
        y_hat = net.dec(z, pitchf, g=gv)
    assert tape.calls == 1
    grads = torch.autograd.grad(y_hat, [params[n] for n in names], grad_outputs=torch.from_numpy(gg["d_y_hat"]))
    out = {"names": np.array(names), "stride": np.int64(STRIDE), "norms": np.array([float(t.double().norm()) for t in grads], dtype=np.float64)}
    for k, t in enumerate(grads):
        out[f"sample.{k}"] = t.detach().reshape(-1)[::STRIDE].numpy().astype(np.float32)
    path = os.path.join(OUT, "gen_wgrad_40k_v2.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(names), "tensors")
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()
