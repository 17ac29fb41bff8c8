"""GPU: the raw entries of the bf16x3 gather GEMMs (rvc_op_disc_conv, rvc_op_disc_conv_input_grad, rvc_op_disc_conv_weight_grad, rvc_op_conv1d_input_grad) on
the case tables of tests/gather_gemm_ref.py against float64 torch autograd of the forward operation.  Gate: rel_err < 2e-5, calibrated on the same inputs by
tests/test_gather_gemms_host.py (the three-term product lies below 1e-5, a product that lost a cross term above 2e-4).  Every case keeps its inputs in a
NaN-filled pool and its output in a sentinel-filled one (test_hip_disc_grad.carve): every output element is written and finite, nothing outside the output's
extent changes - the pitch columns of a pitched output included - and the entry reports the instantiation the case is labelled with.  Every measured value,
with the emulated three-term value of the same inputs beside it, is kept by conftest.record_parity under gather_gemm.*; profiles/gather_gemm_parity.json is a
copy of those entries.  (conv_gen_wgrad's raw table runs in test_hip_gen_wgrad.py at the same gate.)

Ten hand-applied mutants (arithmetic or in-range addressing only), each run through this file and test_hip_gen_wgrad's raw tests once on the device, and what
failed: the al bh MFMA removed from gather_mfma3_unit: every raw case; lo of split2 cut off instead of rounded: test_disc_conv_weight_grad[..._adv] alone
(3.40e-5, the value the host test predicts; on random operands the cut-off costs one operand at most 1.5e-5 and stays inside the gate, which is why that case
exists); gather_units returning 1 where 2 divides: the twelve U = 2 cases of test_disc_conv, test_disc_conv_input_grad and test_conv1d_input_grad (the reported
units); the tap step without p in conv_x3d: the five test_disc_conv cases with k > 1 and p > 1; phase 2's taps {4, 1} swapped:
test_disc_conv_input_grad[S1_Ci32_Co64_H3_p1_s3_cot1] and [S3_Ci160_Co64_H65_p1_s3_cot1] (the stride-3 cases with a row in phase 2); A >= 0 for A > 0: every
test_disc_conv_input_grad case and every test_conv1d_input_grad case with a mask; the last stage of a multi-stage split dropped:
test_disc_conv_weight_grad[S71_...] and [S33_...]; w1 not wrapped: test_disc_conv_weight_grad[S2_Ci13_Co128_H380_p1_k5_s3] and [S3_Ci13_Co128_H128_p3_k5_s3];
scale applied after Res: test_conv1d_input_grad[t0_Ci20_Co32_..._acc1] and [t0_Ci192_Co32_..._xy7_...]; the tap flip omitted in the Conv1d image: the ten
test_conv1d_input_grad cases of a Conv1d with k > 1 and N > 1."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import record_parity, rel_err
import gather_gemm_ref as G
from test_hip_disc_grad import DEV, SENTINEL, carve

pytestmark = pytest.mark.gpu


def params(kind):
    cs = G.cases(kind)
    return pytest.mark.parametrize("c,seed", cs, ids=[kind.label(c) for c, _ in cs])


def place(tensors, fill):
    """each host tensor (or (tensor, pitch): its rows laid out with that pitch) in one device pool filled with `fill`; returns the pool, the device blocks (the
    pitched ones as [rows][pitch]), and the mask of the elements that belong to a tensor's extent"""
    items = [(t if isinstance(t, tuple) else (t, None)) for t in tensors]
    shapes = [tuple(t.shape) if ld is None else (t.shape[0], ld) for t, ld in items]
    pool, views, inside = carve(shapes, fill)
    inside[:] = False
    for (t, ld), v in zip(items, views):
        w = v if ld is None else v[:, :t.shape[1]]
        w.copy_(t)
        base = (v.data_ptr() - pool.data_ptr()) // 4
        if ld is None:
            inside[base:base + v.numel()] = True
        else:
            inside[base:base + v.numel()].view(t.shape[0], ld)[:, :t.shape[1]] = True
    return pool, views, inside


def finish(kind, c, seed, i, got, pool, inside, before):
    """nothing outside the output's extent changed, everything inside is finite (and written), the error against float64 is below the gate"""
    assert torch.equal(pool[~inside], before[~inside]), "an element outside the output's extent changed"
    assert bool(torch.isfinite(got).all()), "a non-finite output element"
    with torch.enable_grad():
        want = kind.reference(c, i).detach()
        a, b = kind.operands(c, i)
        emu = rel_err(kind.epilogue(c, G.emulate(lambda u, v: kind.gemm(c, u, v).detach(), a, b, 3), i).numpy(), want.numpy())
    e = rel_err(got.cpu().numpy().reshape(tuple(want.shape)), want.numpy())
    print(kind.name, kind.label(c), "device", e, "emulated three-term product", emu)
    record_parity(f"gather_gemm.{kind.name}.{kind.label(c)}", {"measured": e, "gate": G.GATE, "emulated": emu})
    assert e < G.GATE, (kind.label(c), e, emu)


def lib():
    from comfy_rvc_amd import _lib
    return _lib


@params(G.DiscConv)
def test_disc_conv(c, seed):
    L = lib()
    i = G.DiscConv.inputs(c, seed)
    _, (x,), _ = place([i["x"]], float("nan"))
    ho = G.conv_out(c["H"], c["k"], c["stride"], c["pad"])
    pool, (y,), inside = carve([(c["S"], c["Co"], ho, c["p"])], SENTINEL)
    before, units = pool.clone(), C.c_int(-1)
    w, b = i["w"].contiguous().numpy(), i["bias"].contiguous().numpy()
    with torch.cuda.device(DEV):
        L.check(L.lib.rvc_op_disc_conv(L.current_stream(), L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), c["S"], c["Ci"], c["Co"], c["H"], c["p"], c["k"], c["stride"],
                                       c["pad"], c["slope"], C.byref(units)))
    torch.cuda.synchronize()
    assert units.value == c["units"]
    assert not bool((y == SENTINEL).any()), "an output element was not written"
    finish(G.DiscConv, c, seed, i, y, pool, inside, before)


@params(G.DiscBwd)
def test_disc_conv_input_grad(c, seed):
    L = lib()
    i = G.DiscBwd.inputs(c, seed)
    ins = [i["d"], i["a"]] + ([i["cot"]] if c["cot"] else [])
    _, views, _ = place(ins, float("nan"))
    d, a, cot = views[0], views[1], (views[2] if c["cot"] else None)
    pool, (y,), inside = carve([tuple(i["a"].shape)], SENTINEL)
    before, units = pool.clone(), C.c_int(-1)
    w = i["w"].contiguous().numpy()
    with torch.cuda.device(DEV):
        L.check(L.lib.rvc_op_disc_conv_input_grad(L.current_stream(), L.ptr(d), L.ptr(w), L.ptr(cot), L.ptr(a), L.ptr(y), c["S"], c["Ci"], c["Co"], c["H"],
                                                  G.DiscBwd.hd(c), c["p"], c["stride"], c["slope"], C.byref(units)))
    torch.cuda.synchronize()
    assert units.value == c["units"]
    assert not bool((y == SENTINEL).any()), "an output element was not written"
    finish(G.DiscBwd, c, seed, i, y, pool, inside, before)


@params(G.DiscWgrad)
def test_disc_conv_weight_grad(c, seed):
    L = lib()
    i = G.DiscWgrad.inputs(c, seed)
    _, (d, x), _ = place([i["d"], i["x"]], float("nan"))
    pool, (dw,), inside = carve([(c["Co"], c["Ci"], c["k"])], SENTINEL)
    before, splits = pool.clone(), C.c_int(-1)
    with torch.cuda.device(DEV):
        L.check(L.lib.rvc_op_disc_conv_weight_grad(L.current_stream(), L.ptr(d), L.ptr(x), L.ptr(dw), c["S"], c["Ci"], c["Co"], c["H"], c["p"], c["k"], c["stride"],
                                                   c["pad"], C.byref(splits)))
    torch.cuda.synchronize()
    assert splits.value == c["splits"]
    assert not bool((dw == SENTINEL).any()), "an output element was not written"
    finish(G.DiscWgrad, c, seed, i, dw, pool, inside, before)


@params(G.GenBwd)
def test_conv1d_input_grad(c, seed):
    L = lib()
    i = G.GenBwd.inputs(c, seed)
    n, td = c["N"], G.GenBwd.td(c)
    ldd, ldy = td + c["xd"], n + c["xy"]
    ins = [(i["d"], ldd)] + [(i[k], ldy) for k in ("a", "res") if i[k] is not None]
    _, views, _ = place(ins, float("nan"))
    d = views[0]
    a = views[1] if i["a"] is not None else None
    res = views[-1] if i["res"] is not None else None
    y0 = i["y0"] if c["acc"] else torch.full((c["Ci"], n), SENTINEL)
    pool, (y,), inside = place([(y0, ldy)], SENTINEL)
    before, bm, units = pool.clone(), C.c_int(-1), C.c_int(-1)
    w = i["w"].contiguous().numpy()
    with torch.cuda.device(DEV):
        L.check(L.lib.rvc_op_conv1d_input_grad(L.current_stream(), L.ptr(d), L.ptr(w), L.ptr(a), L.ptr(res), L.ptr(y), c["t"], c["Ci"], c["Co"], c["k"], c["step"],
                                               c["pad"], n, td, ldd, ldy, c["slope"], c["scale"], c["acc"], C.byref(bm), C.byref(units)))
    torch.cuda.synchronize()
    assert (bm.value, units.value) == (c["bm"], c["units"])
    got = y[:, :n]
    if not c["acc"]:
        assert not bool((got == SENTINEL).any()), "an output element was not written"
    finish(G.GenBwd, c, seed, i, got, pool, inside, before)
