"""CPU: pins tests/gen_grad_ref.py - the float64 restatement of the decoder's forward and of its vector-Jacobian product - against float64 autograd through
oracle.nets.generator_forward, and the new entry points' ctypes signatures."""
import numpy as np
import pytest
import torch

from comfy_rvc_amd import synthetic as S
from oracle import nets
import gen_grad_ref as G

CONFIGS = {"40k_v2": (S.CONFIG_40K_V2, "v2"), "32k_v1": (S.CONFIG_32K_V1, "v1")}
SEG = 13


def peak_err(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("tag", list(CONFIGS))
def test_restated_vjp_equals_float64_autograd(tag, monkeypatch):
    config, version = CONFIGS[tag]
    sd = S.synth_train_state_dict(config, version, 3)
    upp = int(np.prod(config[12]))
    gen = torch.Generator().manual_seed(11)
    z = torch.randn(1, config[2], SEG, generator=gen, dtype=torch.float64).requires_grad_()
    g = (torch.randn(1, config[16], 1, generator=gen, dtype=torch.float64) * 0.3).requires_grad_()
    har = torch.tanh(torch.randn(1, 1, SEG * upp, generator=gen, dtype=torch.float64)).requires_grad_()
    dy = torch.randn(1, 1, SEG * upp, generator=gen, dtype=torch.float64)
    dy = dy / dy.norm()
    sd64 = {k: v.double() for k, v in nets.tensors(sd).items()}
    # the oracle computes the harmonic source from f0 inside: hand it the leaf instead, so that autograd reaches the source
    monkeypatch.setattr(nets, "sine_source", lambda *a, **k: har.transpose(1, 2))
    o = nets.generator_forward(sd64, config, z, torch.zeros(1, SEG, dtype=torch.float64), g, None)
    dz, dg, dhar = torch.autograd.grad(o, [z, g, har], grad_outputs=dy)
    w = G.weights(sd, config)
    with torch.no_grad():
        acts = G.forward(w, config, z, har, g)
        assert peak_err(acts["y_hat"], o[0].detach()) < 1e-12
        v = G.vjp(w, config, acts, dy)
    for name, got, want in (("dz", v["dz"], dz[0]), ("dg", v["dg"], dg[0, :, 0]), ("dhar", v["dhar"], dhar[0, 0])):
        e = peak_err(got, want)
        print(tag, name, e)
        assert e < 1e-10, (tag, name, e)
    # every taped name is there, with the shapes the tape has
    nu = len(config[12])
    assert set(acts) == {"z", "har", "pre", "y_hat"} | {f"up{i}" for i in range(nu)} | {f"out{i}" for i in range(nu)} | \
        {f"rb{i}.{j}.y{m}" for i in range(nu) for j in range(3) for m in (1, 2)} | {f"rb{i}.{j}.t{m}" for i in range(nu) for j in range(3) for m in range(3)}
    assert all(("d." + k) in v for k in acts if k not in ("z", "har", "y_hat"))


def test_no_f0_vjp_equals_float64_autograd():
    config, version = CONFIGS["40k_v2"]
    sd = S.synth_train_state_dict(config, version, 3, f0=False)
    upp = int(np.prod(config[12]))
    gen = torch.Generator().manual_seed(12)
    z = torch.randn(1, config[2], SEG, generator=gen, dtype=torch.float64).requires_grad_()
    g = (torch.randn(1, config[16], 1, generator=gen, dtype=torch.float64) * 0.3).requires_grad_()
    dy = torch.randn(1, 1, SEG * upp, generator=gen, dtype=torch.float64)
    sd64 = {k: v.double() for k, v in nets.tensors(sd).items()}
    o = nets.generator_forward(sd64, config, z, None, g, None)
    dz, dg = torch.autograd.grad(o, [z, g], grad_outputs=dy)
    w = G.weights(sd, config, f0=False)
    with torch.no_grad():
        v = G.vjp(w, config, G.forward(w, config, z, None, g), dy, f0=False)
    assert peak_err(v["dz"], dz[0]) < 1e-10 and peak_err(v["dg"], dg[0, :, 0]) < 1e-10 and "dhar" not in v


def test_new_entry_points_have_signatures():
    from comfy_rvc_amd import _lib
    for name in ("rvc_gen_tape_create", "rvc_gen_tape_release", "rvc_gen_tape_bytes", "rvc_gen_tape_tensor", "rvc_synth_forward_tape",
                 "rvc_synth_dec_input_grad", "rvc_synth_dec_input_grad_launch_count"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
