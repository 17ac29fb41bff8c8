"""CPU: the float64 restatement of the flow and of its vector-Jacobian product (tests/flow_grad_ref.py) pinned on its own - the hand-written VJP against float64
autograd through the restated forward, for dz and dg, with ragged masks, at the shipped size and at a tiny net - the restated forward against the training
forward's restatement that the reference's goldens pin, and the new ABI names under the exported-symbol rule of tests/test_abi_symbols.py."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from comfy_rvc_amd import synthetic as S
import flow_grad_ref as FR
from test_abi_symbols import _declared_symbols

NEW_SYMBOLS = ("rvc_synth_forward_tape_flow", "rvc_synth_flow_input_grad", "rvc_synth_flow_input_grad_launch_count", "rvc_gen_tape_flow_times")
TOL = 1e-12      # float64 against float64: the two differ in summation order only (tests/gen_wgrad_ref.py's host test reaches the same level)


def ragged_mask(lengths, T):
    return (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).to(torch.float64)[:, None, :]


def shipped_weights():
    return FR.weights(S.synth_train_state_dict(S.CONFIG_40K_V2, "v2", 3))


@pytest.mark.parametrize("name,inter,hidden,gin,lengths,T", [("shipped", 192, 192, 256, [17, 11], 17), ("tiny", 4, 6, 3, [9, 5, 1], 9)])
def test_vjp_matches_float64_autograd(name, inter, hidden, gin, lengths, T):
    ws = shipped_weights() if name == "shipped" else FR.random_weights(inter, hidden, gin, seed=5)
    assert ws[0]["pre.w"].shape == (hidden, inter // 2, 1) and ws[0]["cond.w"].shape == (6 * hidden, gin, 1) and ws[0]["rs2.w"].shape[0] == hidden
    gen = torch.Generator().manual_seed(11)
    B = len(lengths)
    mask = ragged_mask(lengths, T)
    z = (torch.randn(B, inter, T, generator=gen, dtype=torch.float64) * mask).requires_grad_()
    g = torch.randn(B, gin, 1, generator=gen, dtype=torch.float64).requires_grad_()
    d = torch.randn(B, inter, T, generator=gen, dtype=torch.float64) * mask
    z_p, acts = FR.forward(ws, z, mask, g)
    dz_ref, dg_ref = torch.autograd.grad(z_p, [z, g], grad_outputs=d)
    with torch.no_grad():
        v = FR.vjp(ws, {k: t.detach() for k, t in acts.items()}, d, mask)
    e_dz, e_dg = rel_err(v["dz"].numpy(), dz_ref.numpy()), rel_err(v["dg"].numpy(), dg_ref[:, :, 0].numpy())
    print(name, "dz", e_dz, "dg", e_dg)
    assert e_dz < TOL and e_dg < TOL, (name, e_dz, e_dg)
    assert not (v["dz"] * (1 - mask)).any()      # a masked cotangent stays masked
    for f in range(4):      # d gc is the row sum of d a, slice by slice
        for i in range(3):
            assert not (v[f"d.flow{f}.a{i}"] * (1 - mask)).any()
        assert v[f"d.flow{f}.gc"].shape == (B, 6 * hidden) and v[f"d.flow{f}.m"].shape == (B, inter // 2, T)
        for i in range(3):
            e = rel_err(v[f"d.flow{f}.gc"][:, 2 * hidden * i:2 * hidden * (i + 1)].numpy(), v[f"d.flow{f}.a{i}"].sum(2).numpy())
            assert e < TOL


def test_deltas_are_the_cotangents_at_the_taped_tensors():
    """d.flow{f}.a{i} and d.flow{f}.h0 against autograd at those very tensors: the forward is re-run from each coupling's recorded tensors made leaves."""
    ws = FR.random_weights(4, 6, 3, seed=8)
    gen = torch.Generator().manual_seed(2)
    lengths, T = [7, 4], 7
    mask = ragged_mask(lengths, T)
    z = torch.randn(2, 4, T, generator=gen, dtype=torch.float64) * mask
    g = torch.randn(2, 3, 1, generator=gen, dtype=torch.float64)
    d = torch.randn(2, 4, T, generator=gen, dtype=torch.float64) * mask
    with torch.no_grad():
        _, acts = FR.forward(ws, z, mask, g)
        v = FR.vjp(ws, acts, d, mask)
    # a hook on every recorded tensor of one differentiable run collects its cotangent
    got = {}
    z2, g2 = z.clone().requires_grad_(), g.clone().requires_grad_()
    z_p, acts2 = FR.forward(ws, z2, mask, g2)
    for n, t in acts2.items():
        if ".a" in n:
            t.register_hook(lambda gr, n=n: got.__setitem__(n, gr))
    z_p.backward(d)
    for f in range(4):
        for i in range(3):
            e = rel_err(v[f"d.flow{f}.a{i}"].numpy(), got[f"flow{f}.a{i}"].numpy())
            assert e < TOL, (f, i, e)


def test_restated_forward_matches_the_training_forward_restatement():
    """z -> z_p of tests/train_forward_ref.py (pinned by the reference's goldens in tests/test_train_forward_host.py) at float32 level."""
    from test_train_forward_host import case_inputs
    import train_forward_ref as R
    config, sd, b, noise_q, noise_src, g = case_inputs("40k_v2")
    out = R.forward(sd, config, b["phone"], b["lengths"], b["pitch"], b["pitchf"], b["spec"], b["sid"], noise_q, noise_src, g["ids_slice"])
    from oracle import nets
    lengths = [int(x) for x in b["lengths"]]
    T = max(lengths)
    mask = ragged_mask(lengths, T)
    emb = nets.tensors(sd)["emb_g.weight"].double()
    gv = emb[torch.as_tensor(np.asarray(b["sid"])).long()].unsqueeze(-1)
    z_p, _ = FR.forward(FR.weights(sd), torch.as_tensor(np.asarray(out["z"])).double(), mask, gv)
    e = rel_err(z_p.numpy(), np.asarray(out["z_p"]))
    print("restated flow against the training forward's restatement", e)
    assert e < 1e-4, e


def test_new_abi_names_follow_the_exported_symbol_rule():
    from comfy_rvc_amd import _lib
    syms = _declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in syms, f"{s} is not declared in include/rvc_hip.h"
        assert s in _lib.SIGNATURES and hasattr(_lib.lib, s), s
        assert not s.startswith("rvc_debug_")
    assert set(_lib.SIGNATURES) == set(syms)
