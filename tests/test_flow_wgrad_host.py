"""CPU: the float64 restatement of the flow's parameter gradients (tests/flow_wgrad_ref.py) against float64 torch.autograd.grad through flow_grad_ref.forward
with weight norm applied explicitly; models.flow_parameter_spec against the training state dicts; the calibration of every raw case's gate on its own inputs
(three-term emulation below 1e-5, a product that lost one MFMA above 2e-4; the gate of a gated case is computed with the gate in float32); and the raw cases'
labels against the planner's pure query."""
import pytest
import torch

import flow_grad_ref as FR
import flow_wgrad_ref as W
import gather_gemm_ref as G

F64 = torch.float64
RAW = W.raw_cases()
RAW_IDS = [W.Raw.label(c) for c, _ in RAW]


def test_restatement_matches_autograd_with_explicit_weight_norm():
    """a tiny net, two items of different length: the sum over the items of <z_p, d> differentiated by autograd with respect to every raw parameter (weight_v,
    weight_g, bias; pre / post plain) equals the restatement on the float64 forward's and VJP's own tensors.  flow_grad_ref reached 2e-15; gate 1e-12."""
    inter, hidden, gin, lengths = 8, 16, 6, [9, 14]
    sd = W.random_state_dict(inter, hidden, gin, 3)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    gen = torch.Generator().manual_seed(4)
    zs = [torch.randn(1, inter, L, generator=gen, dtype=F64) for L in lengths]
    gs = [torch.randn(1, gin, 1, generator=gen, dtype=F64) for _ in lengths]
    ds = [torch.randn(1, inter, L, generator=gen, dtype=F64) for L in lengths]
    masks = [torch.ones(1, 1, L, dtype=F64) for L in lengths]
    loss = 0
    for z, g, d, m in zip(zs, gs, ds, masks):
        z_p, _ = FR.forward(W.folded_weights(leaves), z, m, g)
        loss = loss + (z_p * d).sum()
    want = torch.autograd.grad(loss, [leaves[n] for n in W.parameter_names()])
    items = []
    with torch.no_grad():
        ws = W.folded_weights(sd)
        for z, g, d, m in zip(zs, gs, ds, masks):
            z_p, acts = W.forward(ws, z, m, g)
            z_p0, acts0 = FR.forward(ws, z, m, g)
            assert torch.equal(z_p, z_p0) and all(torch.equal(acts[n], acts0[n]) for n in acts0)      # the extension changes nothing of flow_grad_ref's
            v, v0 = W.vjp(ws, acts, d, m), FR.vjp(ws, acts0, d, m)
            assert all(torch.equal(v[n], v0[n]) for n in v0)
            t = {n: acts[n][0] for n in W.WGRAD_ACTIVATIONS}
            t.update({n: v[n][0] for n in W.WGRAD_DELTAS})
            items.append(t)
        got = W.gradients(sd, items, [g.view(-1) for g in gs])
    assert list(got) == W.parameter_names() and len(got) == 100
    worst = 0.0
    for (n, a), b in zip(got.items(), want):
        assert tuple(a.shape) == tuple(b.shape) == tuple(sd[n].shape), n
        e = G.rel_err(a, b)
        worst = max(worst, e)
        assert e < 1e-12, (n, e)
    print("restatement against autograd, worst of 100:", worst)


@pytest.mark.parametrize("tag", ["40k_v2", "32k_v1", "40k_v2_nono"])
def test_flow_parameter_spec_matches_state_dict(tag):
    from comfy_rvc_amd import synthetic as S
    from comfy_rvc_amd.lib.infer_pack import models
    config, version, f0 = {"40k_v2": (S.CONFIG_40K_V2, "v2", True), "32k_v1": (S.CONFIG_32K_V1, "v1", True), "40k_v2_nono": (S.CONFIG_40K_V2, "v2", False)}[tag]
    sd = S.synth_train_state_dict(config, version, 5, f0=f0)
    want = [(k, tuple(v.shape)) for k, v in sd.items() if k.startswith("flow.")]
    spec = models.flow_parameter_spec(config)
    assert list(spec.items()) == want
    assert len(spec) == 100 and list(spec) == W.parameter_names()


@pytest.mark.parametrize("c,seed", RAW, ids=RAW_IDS)
def test_raw_gate_is_calibrated_on_the_cases_own_inputs(c, seed):
    gate, e3, e2 = W.calibrate(c, seed)
    print(W.Raw.label(c), "three-term", e3, "two-term", e2, "gate", gate)
    if gate == G.GATE:
        assert e3 < G.GATE / 2, e3
    else:      # only a gated case, and then twice its own emulation error - never anything the device measured
        assert c["gate"] and gate == 2 * e3 and e3 >= G.GATE / 2
    assert e2 > 10 * G.GATE, e2
    # the float64 statement of the operation is the padded batch's: zero behind an item's length, of P and of the gated G
    i = W.Raw.inputs(c, seed)
    a, b = W.Raw.operands(c, i)
    assert G.rel_err(W.Raw.gemm(c, a.double(), b.double()), W.Raw.reference(c, i)) < (1e-6 if c["gate"] else 1e-12)
    if c["adv"]:      # a split2 that cuts lo off lies above the gate, by the arithmetic of worst_lo
        cut = G.rel_err(G.emulate(lambda u, v: W.Raw.gemm(c, u, v), a, b, 3, G.split_bf16_lo_truncated), W.Raw.reference(c, i))
        print(W.Raw.label(c), "three-term with lo cut off", cut)
        assert 1.5 * G.GATE < cut < 2 * G.GATE, cut


def _lib_or_skip():
    try:
        from comfy_rvc_amd import _lib
        return _lib
    except (OSError, ImportError) as e:
        pytest.skip(f"the library does not load: {e}")


def test_plan_labels_and_instantiations():
    _lib_or_skip()
    plans = [W.plan(c) for c, _ in RAW]
    for (c, _), p in zip(RAW, plans):
        assert p is not None, W.Raw.label(c)
        assert p["bm"] == c["bm"], (W.Raw.label(c), p)
        assert p["stages"] == sum((n + 127) // 128 for n in c["lengths"])
        assert p["gz"] == p["splits"] and p["gy"] == -(-c["R"] // p["bm"]) and p["gx"] == -(-c["C"] * c["k"] // (128 if p["bm"] == 32 else 64))
    # every instantiation: each row tile with the gate on and off
    assert {(p["bm"], c["gate"]) for (c, _), p in zip(RAW, plans)} == {(bm, g) for bm in (128, 64, 32) for g in (0, 1)}
    assert {c["R"] for c, _ in RAW} == {16, 48, 64, 96, 128, 384}
    assert any(p["stages"] == 1 for p in plans)
    assert any(p["splits"] > len(c["lengths"]) and p["per"] > 1 for (c, _), p in zip(RAW, plans))      # a split starts inside an item
    assert any(len(c["lengths"]) == 16 for c, _ in RAW) and any(c["adv"] for c, _ in RAW)
    assert any(c["C"] * c["k"] % 64 for c, _ in RAW)                                                        # a ragged last column tile
    big = [p for (c, _), p in zip(RAW, plans) if c["lengths"] == [2600, 1700]][0]
    assert (big["stages"], big["splits"], big["per"]) == (35, 18, 2)


def test_planner_declines_what_it_documents():
    _lib = _lib_or_skip()
    c = RAW[3][0]
    assert W.plan(c) is not None
    assert W.plan(c, R=40) is None                                           # R % 16
    assert W.plan(c, k=17) is None and W.plan(c, k=16) is not None          # k > 16
    assert W.plan(c, lengths=[5] * 17) is None and W.plan(c, lengths=[5] * 16) is not None
    assert W.plan(c, B=0) is None
    assert W.plan(c, lengths=[5, 0, 7]) is None                              # an N[item] < 1
    assert W.plan(c, lengths=[5, 2 ** 31 - 1]) is None and W.plan(c, lengths=[5, 2 ** 29]) is None      # offsets outside 32 bits
    assert W.plan(c, off0=5000) is None
    assert W.plan(c, R=4096, C=4096, k=2) is None                            # a partial image beyond the bound (16 Mi floats)
    assert W.plan(c, gate=2) is None
    assert b"fit" in _lib.lib.rvc_last_error() or b"length" in _lib.lib.rvc_last_error() or b"items" in _lib.lib.rvc_last_error()
