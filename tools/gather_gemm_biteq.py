"""Do two builds of the library compute the same bits in the bf16x3 gather GEMMs (conv_x3gather_dev.h: the discriminators' forward, data and weight gradients,
the decoder's data and weight gradients)?  For refactors of those kernels.
    RVC_HIP_LIB=<library> python tools/gather_gemm_biteq.py out.json        (once per library, then compare the "sha256" maps of the two files)
Runs the cases of the committed goldens (the discriminators' cases A and B of both versions and one trainer-size signal; the decoder's 40k_v2 case and the
segment-13 case of tests/test_hip_gen_grad.py; the raw cases of tests/test_hip_gen_wgrad.py) and writes the SHA-256 of every feature map, every input gradient
and delta, every parameter gradient, every tensor of the generator's tapes after forward + input gradient, the flat decoder gradient buffer and the raw
rvc_conv1d_weight_grad outputs."""
import hashlib, json, os, sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from comfy_rvc_amd import _lib as L                      # noqa: E402
from comfy_rvc_amd import synthetic as S                 # noqa: E402

SHA = {}


def put(name, x):
    """x: a tensor, or lists / dicts of tensors (None: skipped), or the decoder's gradient object (its flat buffer)"""
    if x is None:
        return
    if isinstance(x, dict):
        for k in x:
            put(f"{name}.{k}", x[k])
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            put(f"{name}.{i}", v)
    elif isinstance(x, (torch.Tensor, np.ndarray)):
        torch.cuda.synchronize()
        a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x
        SHA[name] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    elif hasattr(x, "flat"):
        put(name, x.flat)
    elif hasattr(x, "items"):
        put(name, dict(x.items()))
    else:
        raise TypeError(f"{name}: {type(x)}")


def discriminators():
    import test_hip_disc_grad as DG
    from comfy_rvc_amd.lib.infer_pack.models import MultiPeriodDiscriminator, MultiPeriodDiscriminatorV2
    shapes = dict(DG.SHAPES, trainer=(12800, 1, 13))
    for version, cls in (("v1", lambda: MultiPeriodDiscriminator(device=DG.DEV, trainable=True)), ("v2", lambda: MultiPeriodDiscriminatorV2(False, device=DG.DEV, trainable=True))):
        net = cls().load_state_dict(S.disc_state_dict(version, 0))
        for case, (T, B, seed) in shapes.items():
            if case == "trainer" and version == "v1":
                continue
            y, y_hat = S.disc_waves(B, T, seed)
            x = DG.dev(np.concatenate([y, y_hat]))
            fmaps = net.forward_single(x)
            gx, deltas = net.input_grad(fmaps, DG.to_dev(DG.random_cotangents(fmaps, 1000 + T)), return_deltas=True)
            tag = f"disc.{version}.{case}"
            put(tag + ".fmap", fmaps)
            put(tag + ".input_grad", gx)
            put(tag + ".delta", deltas)
            put(tag + ".weight_grad", net.weight_grad(x, fmaps, deltas))


def generator():
    import test_hip_gen_wgrad as GW
    for tag in ("40k_v2", GW.SEG13):
        c = GW.WCase(tag)
        names = c.tape.activation_names() + c.tape.delta_names()
        for b in range(c.B):
            for n in names:
                put(f"gen.{tag}.tape{b}.{n}", c.tape.tensor(b, n))
        put(f"gen.{tag}.input_grads", c.input_grads)
        put(f"gen.{tag}.flat_weight_grads", c.grads.flat)
    def raw(name, shapes_p, shapes_g, R, Cc, k, cstride, tstep, off0, sp, sg, seed):
        gen = torch.Generator().manual_seed(seed)
        ops = [torch.randn(*s, generator=gen).to(GW.DEV) for s in shapes_p + shapes_g]
        out = torch.empty(R, Cc * k, device=GW.DEV)
        B = len(shapes_p)
        GW.raw_call(ops[:B], ops[B:], R, Cc, k, shapes_p[0][1], shapes_g[0][1], cstride, tstep, off0, sp, sg, out)
        put(f"raw.{name}", out)
    for R, Cc, k, dil, n, B, slope in GW.CONV_CASES:
        raw(f"conv1d_{R}x{Cc}x{k}_d{dil}_n{n}_b{B}", [(R, n)] * B, [(Cc, n)] * B, R, Cc, k, 1, dil, -((k * dil - dil) // 2), 1.0, slope, R + k + n)
    for Cin, Cout, k, u, n, B in ((64, 32, 4, 2, 65, 2), (512, 256, 16, 10, 13, 2)):
        raw(f"convT_{Cin}x{Cout}x{k}_u{u}_n{n}_b{B}", [(Cin, n)] * B, [(Cout, u * n)] * B, Cin, Cout, k, u, 1, -((k - u) // 2), 0.1, 1.0, Cin + k)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "gather_gemm_biteq.json"
    discriminators()
    generator()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"library": os.path.basename(L.LIB_PATH), "sha256": SHA}, f, indent=1, sort_keys=True)
    print(f"{len(SHA)} hashes -> {out}")


if __name__ == "__main__":
    main()
