"""GPU: the flow's parameter gradients (net_g.flow_weight_grad, rvc_synth_flow_weight_grad) and the ragged, gated weight-gradient GEMM behind them
(csrc/conv_flow_wgrad.hip, rvc_gated_conv1d_weight_grad), synthetic weights.

(1) the raw GEMM on the cases of tests/flow_wgrad_ref.py against float64 autograd of the forward operation at the gate tests/test_flow_wgrad_host.py calibrates
on the same inputs (2e-5 for every case), operands in a NaN pool and the output in a sentinel pool; (2) the whole pass against the float64 restatement on the
device's own tapes, gate 1e-3 (conftest.rel_err per tensor, all 100 tensors, summed over the batch), with the four additional tape tensors checked against the
float64 forward / VJP; (3) placement and determinism; (4) a zero cotangent; (5) trainable=True changes nothing else; (6) the launch count; (7) errors; (8)
train_step.generator_flow_grads.  Every figure is printed (-s); with FLOW_WGRAD_PARITY_DUMP=<file.json> in the environment they are also written there
(profiles/flow_wgrad_parity.json).

Launch count.  flow_weight_grad: per coupling pre, three in_layers, three res_skip layers and post are one GEMM launch and one finishing launch each, cond_layer
one float64 launch: 4 (2 (1 + 3 + 3 + 1) + 1) = 68, whatever B and the lengths.  flow_input_grad on a trainable net: the plain net's 49 and per coupling three
copies (d.skip, d.x2, d.x1): 61.

Shapes.  The nets' own rows (192 / 384 / 96) and columns (96, 192 x 5, 192, 256); lengths 13 / 11 (one ragged stage per item), 129 / 128 (a ragged second stage,
and an item that ends exactly on a stage), 21 / 17 and 21 / 15 for the v1 and the no-f0 net."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import rel_err
from comfy_rvc_amd import synthetic as S
from oracle import nets as N
import flow_grad_ref as FR
import flow_wgrad_ref as W
import gather_gemm_ref as G
from test_hip_disc_grad import SENTINEL, carve

pytestmark = pytest.mark.gpu
GATE = 1e-3
DEV = "cuda:0"
F64 = torch.float64
# tag -> (configuration, version, f0, segment, lengths)
CASES = {"40k_v2_T13": (S.CONFIG_40K_V2, "v2", True, 9, [13, 11]), "40k_v2_T129": (S.CONFIG_40K_V2, "v2", True, 13, [129, 128]),
         "32k_v1_T21": (S.CONFIG_32K_V1, "v1", True, 13, [21, 17]), "40k_v2_nono_T21": (S.CONFIG_40K_V2, "v2", False, 13, [21, 15])}
TAGS = list(CASES)
WGRAD_LAUNCHES = 4 * (2 * (1 + 3 + 3 + 1) + 1)
BACKWARD_LAUNCHES_PLAIN, BACKWARD_LAUNCHES_TRAINABLE = 49, 49 + 4 * 3


def record(key, value, gate=GATE):
    print(key, value)
    path = os.environ.get("FLOW_WGRAD_PARITY_DUMP")
    if not path:
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        data = json.load(open(path)) if os.path.isfile(path) else {}
        data[key] = {"measured": float(value), "gate": gate}
        with open(path, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
    except OSError:
        pass


def lib():
    from comfy_rvc_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ 1. the raw GEMM
RAW = W.raw_cases()


def raw_call(c, P, Gm, out):
    L = lib()
    B = len(P)
    pp = (C.c_void_p * B)(*[t.data_ptr() for t in P])
    pg = (C.c_void_p * B)(*[t.data_ptr() for t in Gm])
    n = (C.c_int64 * B)(*c["lengths"])
    with torch.cuda.device(DEV):
        L.check(L.lib.rvc_gated_conv1d_weight_grad(L.current_stream(), pp, pg, B, c["R"], c["C"], c["k"], n, -((c["k"] - 1) // 2), c["gate"], L.ptr(out)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("c,seed", RAW, ids=[W.Raw.label(c) for c, _ in RAW])
def test_raw_gemm_against_float64_autograd(c, seed):
    gate, e3, _ = W.calibrate(c, seed)      # on the CPU, from the case's own inputs
    i = W.Raw.inputs(c, seed)
    B = len(c["lengths"])
    _, views, _ = carve([tuple(t.shape) for t in i["p"] + i["g"]], float("nan"))
    for v, h in zip(views, i["p"] + i["g"]):
        v.copy_(h)
    pool, (out,), inside = carve([(c["R"], c["C"] * c["k"])], SENTINEL)
    before = pool.clone()
    raw_call(c, views[:B], views[B:], out)
    assert torch.equal(pool[~inside], before[~inside]), "an element outside the output changed"
    got = out.cpu()
    assert bool(torch.isfinite(got).all()) and not bool((got == SENTINEL).any()), "an output element was not written"
    want = W.Raw.reference(c, i)
    e = rel_err(got.numpy().reshape(want.shape), want.numpy())
    print(W.Raw.label(c), "device", e, "emulated three-term product", e3, "gate", gate)
    record(f"raw.{W.Raw.label(c)}", e, gate)
    record(f"raw.{W.Raw.label(c)}.emulated", e3, None)
    assert e < gate, (W.Raw.label(c), e, e3)
    out2 = torch.full_like(out, SENTINEL)
    raw_call(c, views[:B], views[B:], out2)
    assert torch.equal(out2, out), "two calls differ"


# ------------------------------------------------------------------------------------------------ 2. the whole pass
class Case:
    """One net (trainable or plain), one batch through forward_with_tape(record_flow=True) and flow_input_grad (cotangent seed 7) once; for a trainable net the
    weight gradients of the whole batch and the float64 restatement on each item's own taped tensors - computed once and left unchanged."""

    def __init__(self, tag, trainable=True):
        from comfy_rvc_amd.lib.infer_pack import models
        config, self.version, self.f0, seg, self.lengths = CASES[tag]
        config = list(config)
        config[1] = seg
        self.tag, self.config, self.seg, self.upp = tag, tuple(config), seg, int(np.prod(config[12]))
        cls = getattr(models, f"SynthesizerTrnMs{768 if self.version == 'v2' else 256}NSFsid" + ("" if self.f0 else "_nono"))
        self.net = cls(*self.config, is_half=False, trainable=trainable) if self.f0 else cls(*self.config, trainable=trainable)
        self.sd = S.synth_train_state_dict(self.config, self.version, 5, f0=self.f0)
        self.net.load_state_dict(self.sd)
        self.B, self.T, self.IC = len(self.lengths), max(self.lengths), self.config[2]
        self.batch = S.synth_train_batch(self.config, self.version, self.lengths, seed=41, f0=self.f0)
        gen = torch.Generator().manual_seed(42)
        nq, ns = torch.randn(self.B, self.IC, self.T, generator=gen), torch.randn(self.B, seg * self.upp, 1, generator=gen)
        self.noise = (nq, ns) if self.f0 else nq
        self.ids = torch.tensor([L - seg for L in self.lengths], dtype=torch.int64)
        self.res, self.tape = self.forward(record_flow=True)
        self.d = self.cotangent(7)
        self.dz, self.dg = self.net.flow_input_grad(self.tape, self.d.to(DEV))
        if not trainable:
            return
        self.grads = self.net.flow_weight_grad(self.tape)
        self.flat = self.grads.flat.clone()
        t64 = {k: v.double() for k, v in N.tensors({k: v for k, v in self.sd.items() if k.startswith("flow.") or k == "emb_g.weight"}).items()}
        self.emb = t64.pop("emb_g.weight")
        self.sd64 = t64
        names = W.WGRAD_ACTIVATIONS + W.WGRAD_DELTAS
        self.items = [{n: self.tape.tensor(b, n).cpu().double() for n in names} for b in range(self.B)]
        self.g = [self.emb[int(s)] for s in self.batch["sid"]]
        for b in range(self.B):
            assert torch.equal(self.tape.tensor(b, "g").cpu().view(-1).double(), self.g[b]), "the tape's g is not the item's emb_g row"
        self._ref = {}

    def ref(self, which):
        if which not in self._ref:
            with torch.no_grad():
                self._ref[which] = W.gradients(self.sd64, [self.items[b] for b in which], [self.g[b] for b in which])
        return self._ref[which]

    def forward(self, record_flow, tape=None):
        t = {k: (None if v is None else torch.from_numpy(np.asarray(v))) for k, v in self.batch.items()}
        args = (t["phone"], t["lengths"], t["pitch"], t["pitchf"], t["spec"], t["lengths"], t["sid"]) if self.f0 else (t["phone"], t["lengths"], t["spec"], t["lengths"], t["sid"])
        return self.net.forward_with_tape(*args, noise=self.noise, ids_slice=self.ids, tape=tape, record_flow=record_flow)

    def cotangent(self, seed):
        """about unit norm per item, exactly 0 behind each length (test_hip_flow_grad.Case.cotangent)"""
        d = torch.randn(self.B, self.IC, self.T, generator=torch.Generator().manual_seed(seed))
        for b, L in enumerate(self.lengths):
            d[b, :, L:] = 0
        return d / d.flatten(1).norm(dim=1).view(self.B, 1, 1)


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(tag, trainable=True):
        if (tag, trainable) not in cache:
            cache[(tag, trainable)] = Case(tag, trainable)
        return cache[(tag, trainable)]
    return get


def raw_pass(net, handles, ptrs):
    L = lib()
    pt = (C.c_void_p * max(1, len(handles)))(*[h.value for h in handles])
    pg = (C.c_void_p * len(ptrs))(*ptrs)
    with torch.cuda.device(DEV):
        rc = L.lib.rvc_synth_flow_weight_grad(net._h, L.current_stream(), pt, len(handles), pg)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("tag", TAGS)
def test_whole_pass_matches_restatement_on_the_tape(tag, cases):
    c = cases(tag)
    want = c.ref(tuple(range(c.B)))      # the sum over ALL items of the batch
    params = c.net.flow_parameter_shapes()
    keys = [k for k in c.sd if k.startswith("flow.")]
    assert list(params) == keys == list(c.grads) == list(want) and len(keys) == 100
    worst, worst_name = 0.0, None
    for n, shape in params.items():
        got = c.grads[n]
        assert tuple(got.shape) == tuple(shape) == tuple(c.sd[n].shape), n
        e = rel_err(got.cpu().numpy(), want[n].numpy())
        record(f"pass_{tag}.{n}", e)
        if e > worst:
            worst, worst_name = e, n
        assert e < GATE, (tag, n, e)
    print(tag, "worst parameter tensor", worst_name, worst, "of", len(params))
    record(f"pass_{tag}.worst", worst)
    # the four additional tape tensors: xin / out against the float64 forward from the device's own z, d.x1 / d.x2 / d.skip against the float64 VJP on the
    # device's own pre-gate activations
    ws = FR.weights(c.sd)
    z = c.res[4][0].cpu().double()
    assert sorted(c.tape.flow_wgrad_names()) == sorted([f"flow{f}.{n}" for f in range(4) for n in ("xin", "out")] + [f"d.flow{f}.{n}" for f in range(4) for n in ("x1", "x2", "skip")])
    worst_f, worst_b = 0.0, 0.0
    for b, L in enumerate(c.lengths):
        ones = torch.ones(1, 1, L, dtype=F64)
        with torch.no_grad():
            _, acts = W.forward(ws, z[b:b + 1, :, :L], ones, c.g[b].view(1, -1, 1))
            v = W.vjp(ws, {n: c.items[b][n][None] for n in W.WGRAD_ACTIVATIONS}, c.d[b:b + 1, :, :L].double(), ones)
        for f in range(4):
            for n in (f"flow{f}.xin", f"flow{f}.out"):
                e = rel_err(c.items[b][n].numpy(), acts[n][0].numpy())
                worst_f = max(worst_f, e)
                assert tuple(c.items[b][n].shape) == tuple(acts[n][0].shape) and e < GATE, (tag, b, n, e)
            for n in (f"d.flow{f}.x1", f"d.flow{f}.x2", f"d.flow{f}.skip"):
                e = rel_err(c.items[b][n].numpy(), v[n][0].numpy())
                worst_b = max(worst_b, e)
                assert tuple(c.items[b][n].shape) == tuple(v[n][0].shape) and e < GATE, (tag, b, n, e)
    record(f"tape_{tag}.xin_out_worst", worst_f)
    record(f"tape_{tag}.dx_dskip_worst", worst_b)


# ------------------------------------------------------------------------------------------------ 3. placement and determinism
def test_placement_determinism_and_the_sum_over_items(cases):
    c = cases("40k_v2_T13")
    params = c.net.flow_parameter_shapes()
    sizes = [int(np.prod(s)) for s in params.values()]
    total = int(lib().lib.rvc_synth_flow_param_total(c.net._h))
    assert total == sum(sizes) == c.flat.numel() and int(lib().lib.rvc_synth_flow_param_count(c.net._h)) == 100

    def call(handles):
        pool, (flat,), inside = carve([(total,)], SENTINEL)
        before = pool.clone()
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        assert raw_pass(c.net, handles, [flat.data_ptr() + 4 * int(o) for o in offs]) == 0, lib().lib.rvc_last_error()
        assert torch.equal(pool[~inside], before[~inside]), "an element outside the flat buffer changed"
        assert bool(torch.isfinite(flat).all()) and not bool((flat == SENTINEL).any()), "a gradient element was not written"
        return flat.clone()
    a, b = call(c.tape._h), call(c.tape._h)
    assert torch.equal(a, b), "two calls differ"
    assert torch.equal(a, c.flat), "the Python surface's buffer is not the raw call's"
    g0, g1 = call(c.tape._h[:1]), call(c.tape._h[1:])
    e = rel_err((g0 + g1).cpu().numpy(), a.cpu().numpy())
    record("sum_over_items_40k_v2_T13", e)
    assert e < GATE
    assert rel_err(g0.cpu().numpy(), a.cpu().numpy()) > 10 * GATE and rel_err(g1.cpu().numpy(), a.cpu().numpy()) > 10 * GATE
    # each single item against its own restatement: lengths mixed up between the items would show here
    for which, got in (((0,), g0), ((1,), g1)):
        want = torch.cat([t.reshape(-1) for t in c.ref(which).values()])
        o = 0
        for n, size in zip(params, sizes):
            e = rel_err(got[o:o + size].cpu().numpy(), want[o:o + size].numpy())
            assert e < GATE, (which, n, e)
            o += size


# ------------------------------------------------------------------------------------------------ 4. a zero cotangent
def test_zero_cotangent_gives_zero_gradients(cases):
    c = cases("40k_v2_T13")
    try:
        c.net.flow_input_grad(c.tape, torch.zeros(c.B, c.IC, c.T, device=DEV))
        g = c.net.flow_weight_grad(c.tape)
        assert not bool(g.flat.any()), "a zero cotangent left a non-zero gradient"
    finally:      # the shared case's deltas back
        c.net.flow_input_grad(c.tape, c.d.to(DEV))
    assert torch.equal(c.net.flow_weight_grad(c.tape).flat, c.flat)


# ------------------------------------------------------------------------------------------------ 5. trainable=True changes nothing else
def test_trainable_changes_nothing_else(cases):
    c, p = cases("40k_v2_T13"), cases("40k_v2_T13", trainable=False)
    assert torch.equal(c.res[4][1], p.res[4][1]) and torch.equal(c.res[4][0], p.res[4][0]) and torch.equal(c.res[0], p.res[0])      # z_p, z, the wave
    assert torch.equal(c.dz, p.dz) and torch.equal(c.dg, p.dg)
    for b in range(c.B):
        for n in c.tape.flow_activation_names() + c.tape.flow_delta_names():
            assert torch.equal(c.tape.tensor(b, n), p.tape.tensor(b, n)), n
        for n in c.tape.flow_wgrad_names():
            c.tape.tensor(b, n)
            with pytest.raises(Exception):
                p.tape.tensor(b, n)
    assert p.tape.nbytes < c.tape.nbytes
    record("tape_bytes_trainable_40k_v2_T13", c.tape.nbytes, None)
    record("tape_bytes_plain_40k_v2_T13", p.tape.nbytes, None)
    with pytest.raises(ValueError):
        p.net.flow_weight_grad(p.tape)
    x = torch.zeros(int(lib().lib.rvc_synth_flow_param_total(p.net._h)), device=DEV)
    assert raw_pass(p.net, p.tape._h, [x.data_ptr()] * 100) != 0 and b"keep_parameters" in lib().lib.rvc_last_error()
    assert p.net.flow_backward_launch_count() == BACKWARD_LAUNCHES_PLAIN
    assert c.net.flow_backward_launch_count() == BACKWARD_LAUNCHES_TRAINABLE
    record("flow_backward_launches_trainable", c.net.flow_backward_launch_count(), None)


# ------------------------------------------------------------------------------------------------ 6. the launch count
def test_launch_count_is_a_constant_of_the_net(cases):
    counts = {tag: cases(tag).net.flow_weight_grad_launch_count() for tag in TAGS}      # lengths 13 / 11, 129 / 128, 21 / 17, 21 / 15; the count takes no B
    record("flow_wgrad_launch_count", counts["40k_v2_T13"], None)
    assert set(counts.values()) == {WGRAD_LAUNCHES}, counts
    assert lib().lib.rvc_synth_flow_weight_grad_launch_count(None) == -1


# ------------------------------------------------------------------------------------------------ 7. errors
def test_errors_raise_and_nothing_faults(cases):
    L = lib()
    c, o, p = cases("40k_v2_T13"), cases("40k_v2_T129"), cases("40k_v2_T13", trainable=False)
    x = torch.zeros(c.flat.numel(), device=DEV)
    ptrs = [x.data_ptr()] * 100

    def refused(net, handles, word):
        assert raw_pass(net, handles, ptrs) != 0
        assert word in L.lib.rvc_last_error(), L.lib.rvc_last_error()
    refused(p.net, p.tape._h, b"keep_parameters")                      # no kept parameters
    refused(c.net, [], b"tapes")                                       # B = 0
    refused(c.net, [c.tape._h[0]] * 17, b"tapes")                      # 17 tapes
    refused(o.net, c.tape._h, b"another")                              # a tape of another handle
    with pytest.raises(ValueError):
        o.net.flow_weight_grad(c.tape)
    _, plain_tape = c.forward(record_flow=False)
    refused(c.net, plain_tape._h, b"record_flow")                      # recorded without record_flow
    with pytest.raises(ValueError):
        c.net.flow_weight_grad(plain_tape)
    _, fresh = c.forward(record_flow=True)
    refused(c.net, fresh._h, b"flow_input_grad")                       # a recording forward not followed by flow_input_grad
    with pytest.raises(Exception):
        c.net.flow_weight_grad(fresh)
    refused(c.net, [c.tape._h[0], fresh._h[1]], b"flow_input_grad")    # one such tape among good ones
    assert not bool(x.any())
    assert torch.equal(c.net.flow_weight_grad(c.tape).flat, c.flat)    # the shared case still gives its bits


# ------------------------------------------------------------------------------------------------ 8. the wiring
def test_generator_flow_grads_is_its_two_parts(cases):
    from comfy_rvc_amd.lib.train import train_step as TS
    c = cases("40k_v2_T13")
    dz, dg, grads = TS.generator_flow_grads(c.net, c.tape, {"z_p": c.d.to(DEV)})
    assert torch.equal(dz, c.dz) and torch.equal(dg, c.dg)
    assert list(grads) == list(c.grads) and torch.equal(grads.flat, c.flat)
