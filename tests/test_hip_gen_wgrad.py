"""GPU: the decoder's weight-gradient pass (rvc_synth_dec_weight_grad, conv_gen_wgrad.hip) and its raw GEMM entry (rvc_conv1d_weight_grad) against float64:
the raw GEMM against float64 torch autograd (gate 2e-5, the bf16x3 product's), the whole pass against the float64 restatement (tests/gen_wgrad_ref.py) on the device's own taped activations and
deltas - given the tape the pass is a bilinear form of what it reads, so the restatement on those tensors is the exact map.  Gate: conftest.rel_err < 1e-3,
the project's fp32 gate.  Every measured value is kept by conftest.record_parity under gen_wgrad.*; profiles/gen_wgrad_parity.json is a copy of those entries.

Ten hand-applied mutants, each run through this file once on the device, and the tests that failed: leaky ReLU not applied to the gathered operand, tap step
without the dilation, pad off by one, last item left out, last split's partial dropped: test_raw_gemm_conv1d_* and test_whole_pass_* (the last two also
test_flat_buffer_*); up-sampler stride dropped: test_raw_gemm_conv_transpose1d_* and test_whole_pass_*; slope 0.1 at conv_post, convs2.2 read from d.rb..y2
instead of d.out, |v|^2 for |v| in grad_g: test_whole_pass_* (all four nets); g's row of the wrong item in cond: test_whole_pass_* (the three cases whose batch
holds more than one item: 32k_v1's golden batch is a single item) and test_flat_buffer_*."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden, record_parity, rel_err
from comfy_rvc_amd import synthetic as S
from oracle import nets as N
import gen_wgrad_ref as W
import gather_gemm_ref as G
import test_hip_gen_grad as H

pytestmark = pytest.mark.gpu
GATE = 1e-3
RAW_GATE = G.GATE      # the raw GEMM: the bf16x3 product's own gate (tests/test_gather_gemms_host.py calibrates it on these cases' shapes)
DEV = H.DEV
SEG13 = H.SEG13
TAGS = ["40k_v2", "32k_v1", "40k_v2_nono", SEG13]
SENTINEL = H.SENTINEL


def record(name, value, gate):
    record_parity(f"gen_wgrad.{name}", {"measured": float(value), "gate": None if gate is None else float(gate)})


# ------------------------------------------------------------------------------------------------ 1. the raw GEMM
def raw_call(P, Gm, R, Cc, k, n, tg, cstride, tstep, off0, sp, sg, out):
    from comfy_rvc_amd import _lib
    B = len(P)
    pp = (C.c_void_p * B)(*[t.data_ptr() for t in P])
    pg = (C.c_void_p * B)(*[t.data_ptr() for t in Gm])
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib.rvc_conv1d_weight_grad(_lib.current_stream(), pp, pg, B, R, Cc, k, n, tg, cstride, tstep, off0, sp, sg, _lib.ptr(out)))
    torch.cuda.synchronize()


def planned_splits(B, R, Cc, k, n, tg, cstride, tstep, off0):
    from comfy_rvc_amd import _lib
    return int(_lib.lib.rvc_conv1d_weight_grad_splits(B, R, Cc, k, n, tg, cstride, tstep, off0))


def run_raw(name, shapes_p, shapes_g, R, Cc, k, cstride, tstep, off0, sp, sg, want_fn, seed):
    """operands in one pool whose gaps are NaN, the output in a pool of sentinels: every output element written and finite, nothing else touched"""
    B = len(shapes_p)
    gen = torch.Generator().manual_seed(seed)
    pool, views, _ = H.carve(shapes_p + shapes_g, float("nan"))
    host = [torch.randn(*s, generator=gen) for s in shapes_p + shapes_g]
    for v, h in zip(views, host):
        v.copy_(h)
    opool, (out,), inside = H.carve([(R, Cc * k)], SENTINEL)
    raw_call(views[:B], views[B:], R, Cc, k, shapes_p[0][1], shapes_g[0][1], cstride, tstep, off0, sp, sg, out)
    assert bool((opool[~inside] == SENTINEL).all()), "an element outside the output changed"
    got = out.cpu()
    assert bool(torch.isfinite(got).all()) and not bool((got == SENTINEL).any()), "an output element was not written"
    want = want_fn([h.double() for h in host[:B]], [h.double() for h in host[B:]])
    e = rel_err(got.numpy().reshape(want.shape), want.numpy())
    print(name, e)
    record(f"raw.{name}", e, RAW_GATE)
    assert e < RAW_GATE, (name, e)


CONV_CASES = G.GEN_WGRAD_CONV_CASES      # with R = 16 and R = 48: the last 32-row tile half empty


@pytest.mark.parametrize("R,Cc,k,dil,n,B,slope", CONV_CASES)
def test_raw_gemm_conv1d_against_float64_autograd(R, Cc, k, dil, n, B, slope):
    pad = (k * dil - dil) // 2

    def want(deltas, xs):
        w = torch.zeros(R, Cc, k, dtype=torch.float64, requires_grad=True)
        loss = sum((F.conv1d(F.leaky_relu(x, slope)[None], w, None, padding=pad, dilation=dil)[0] * d).sum() for d, x in zip(deltas, xs))
        return torch.autograd.grad(loss, w)[0]
    splits = planned_splits(B, R, Cc, k, n, n, 1, dil, -pad)
    assert splits >= 1
    if n == 5200:      # 2 items x 41 stages of 128 columns (the last of each item ragged: 80) in runs of 3: 28 splits, the last one holding a single stage
        record("raw.splits_32x32x3_n5200_b2", splits, None)
        assert splits == 28, splits
    run_raw(f"conv1d_{R}x{Cc}x{k}_d{dil}_n{n}_b{B}", [(R, n)] * B, [(Cc, n)] * B, R, Cc, k, 1, dil, -pad, 1.0, slope, want, seed=R + k + n)


@pytest.mark.parametrize("Cin,Cout,k,u,n,B", [(64, 32, 4, 2, 65, 2), (512, 256, 16, 10, 13, 2)])
def test_raw_gemm_conv_transpose1d_against_float64_autograd(Cin, Cout, k, u, n, B):
    pad = (k - u) // 2

    def want(xs, deltas):
        w = torch.zeros(Cin, Cout, k, dtype=torch.float64, requires_grad=True)
        loss = sum((F.conv_transpose1d(F.leaky_relu(x, 0.1)[None], w, None, stride=u, padding=pad)[0] * d).sum() for x, d in zip(xs, deltas))
        return torch.autograd.grad(loss, w)[0]
    run_raw(f"convT_{Cin}x{Cout}x{k}_u{u}_n{n}_b{B}", [(Cin, n)] * B, [(Cout, u * n)] * B, Cin, Cout, k, u, 1, -pad, 0.1, 1.0, want, seed=Cin + k)


# ------------------------------------------------------------------------------------------------ 2. the whole pass
def make_trainable_net(tag):
    from comfy_rvc_amd.lib.infer_pack import models
    config, version, f0 = H.net_config(tag)
    cls = getattr(models, f"SynthesizerTrnMs{768 if version == 'v2' else 256}NSFsid" + ("" if f0 else "_nono"))
    net = cls(*config, is_half=False, trainable=True) if f0 else cls(*config, trainable=True)
    seed = int(golden(f"train_forward_{'40k_v2' if tag == SEG13 else tag}.npz")["weight_seed"])
    sd = S.synth_train_state_dict(config, version, seed, f0=f0)
    net.load_state_dict(sd)
    return net, sd


class WCase:
    """One trainable net, the batch of test_hip_gen_grad's Case through forward_with_tape and dec_input_grad once (cotangent seed 7), the weight gradients of the
    whole batch, and the float64 restatement on each item's own taped activations and deltas - computed once and left unchanged."""

    def __init__(self, tag):
        self.tag = tag
        self.config, self.version, self.f0 = H.net_config(tag)
        self.net, self.sd = make_trainable_net(tag)
        self.seg, self.upp = self.config[1], int(np.prod(self.config[12]))
        if tag == SEG13:
            self.ids = np.array([9, 0], dtype=np.int64)
            self.batch = S.synth_train_batch(self.config, self.version, [29, 13], seed=41)
            gen = torch.Generator().manual_seed(42)
            self.noise = (torch.randn(2, 192, 29, generator=gen), torch.randn(2, 13 * self.upp, 1, generator=gen))
        else:
            from test_train_forward_host import case_inputs
            _, _, self.batch, noise_q, noise_src, g = case_inputs(tag)
            self.noise = (noise_q, noise_src) if self.f0 else noise_q
            self.ids = np.asarray(g["ids_slice"])
        self.res, self.tape = H.call(self.net, self.f0, self.batch, self.noise, torch.from_numpy(self.ids), True)
        self.B = self.tape.B
        self.d = H.Case.cotangent(self, 7)
        self.input_grads = self.net.dec_input_grad(self.tape, self.d.to(DEV))
        self.grads = self.net.dec_weight_grad(self.tape)
        self._items, self._ref = None, {}

    def items(self):
        if self._items is None:
            emb = N.tensors(self.sd)["emb_g.weight"]
            names = self.tape.activation_names() + [n for n in self.tape.delta_names() if n != "d.g"]
            self._items = []
            for b in range(self.B):
                t = {n: self.tape.tensor(b, n).cpu() for n in names}
                it = {"acts": {n: v for n, v in t.items() if not n.startswith("d.")}, "deltas": {n: v for n, v in t.items() if n.startswith("d.")},
                      "g": self.tape.tensor(b, "g").cpu().view(-1), "sine": self.tape.tensor(b, "sine").cpu().view(-1) if self.f0 else None}
                assert torch.equal(it["g"], emb[int(self.batch["sid"][b])]), "the tape's g is not the item's emb_g row"
                self._items.append(it)
        return self._items

    def ref(self, which):
        """the restatement over the items `which` (a tuple of indices)"""
        if which not in self._ref:
            with torch.no_grad():
                self._ref[which] = W.weight_grads(self.sd, self.config, [self.items()[b] for b in which], f0=self.f0)
        return self._ref[which]


@pytest.fixture(scope="module")
def wcases():
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = WCase(tag)
        return cache[tag]
    return get


@pytest.mark.parametrize("tag", TAGS)
def test_whole_pass_matches_restatement_on_the_tape(tag, wcases):
    c = wcases(tag)
    want = c.ref(tuple(range(c.B)))      # the sum over ALL items of the batch
    params = c.net.dec_parameter_shapes()
    assert list(params) == [k for k in c.sd if k.startswith("dec.")] == list(c.grads) == list(want)
    worst, worst_name = 0.0, None
    for n, shape in params.items():
        got = c.grads[n]
        assert tuple(got.shape) == tuple(shape) == tuple(c.sd[n].shape), n
        e = rel_err(got.cpu().numpy(), want[n].numpy())
        record(f"pass_{tag}.{n}", e, GATE)
        if e > worst:
            worst, worst_name = e, n
        assert e < GATE, (tag, n, e)
    print(tag, "worst parameter tensor", worst_name, worst, "of", len(params))
    if c.f0:      # the source before l_linear is what the tape says it is
        it = c.items()[0]
        w, b = float(c.sd["dec.m_source.l_linear.weight"][0, 0]), float(c.sd["dec.m_source.l_linear.bias"][0])
        e = rel_err(it["acts"]["har"].view(-1).numpy(), torch.tanh(it["sine"].double() * w + b).numpy())
        record(f"pass_{tag}.tape_sine", e, GATE)
        assert e < 1e-5, e


# ------------------------------------------------------------------------------------------------ 3. placement and determinism
def raw_pass(net, handles, ptrs):
    from comfy_rvc_amd import _lib
    pt = (C.c_void_p * len(handles))(*[h.value for h in handles])
    pg = (C.c_void_p * len(ptrs))(*ptrs)
    with torch.cuda.device(DEV):
        rc = _lib.lib.rvc_synth_dec_weight_grad(net._h, _lib.current_stream(), pt, len(handles), pg)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("tag", ["40k_v2", SEG13])
def test_flat_buffer_is_placed_exactly_and_twice_the_same(tag, wcases):
    c = wcases(tag)
    assert c.B >= 2
    shapes = list(c.net.dec_parameter_shapes().values())
    total = sum(int(np.prod(s)) for s in shapes)
    assert c.grads.flat.numel() == total

    def run(handles):
        pool, (flat,), inside = H.carve([(total,)], SENTINEL)
        ptrs, o = [], 0
        for s in shapes:
            ptrs.append(flat.data_ptr() + 4 * o)
            o += int(np.prod(s))
        assert raw_pass(c.net, handles, ptrs) == 0
        assert bool((pool[~inside] == SENTINEL).all()), "an element outside the flat buffer changed"
        assert not bool((flat == SENTINEL).any()) and bool(torch.isfinite(flat).all()), "a gradient element was not written"
        return flat.clone()
    both = run(c.tape._h)
    assert torch.equal(both, run(c.tape._h)), "two calls differ"
    assert torch.equal(both, c.grads.flat), "the Python surface's buffer differs from the raw call's"
    g0, g1 = run(c.tape._h[:1]), run(c.tape._h[1:])
    e = rel_err(both.cpu().numpy(), (g0.double() + g1.double()).cpu().numpy())
    print(tag, "grads of tapes [0, 1] against grads[0] + grads[1]", e)
    record(f"additivity_{tag}", e, GATE)
    assert e < GATE
    assert not torch.equal(g0, g1)


def test_zero_cotangent_gives_zero_grads(wcases):
    c = wcases(SEG13)
    try:
        c.net.dec_input_grad(c.tape, torch.zeros_like(c.d).to(DEV))
        z = c.net.dec_weight_grad(c.tape)
        assert not bool(z.flat.any())
    finally:
        c.net.dec_input_grad(c.tape, c.d.to(DEV))      # the shared case's deltas are those of cotangent 7 again
    assert torch.equal(c.net.dec_weight_grad(c.tape).flat, c.grads.flat)


# ------------------------------------------------------------------------------------------------ 4. trainable=True changes nothing else
def test_trainable_changes_nothing_else(wcases):
    c = wcases("40k_v2")
    plain, _ = H.make_net("40k_v2")
    res, tape = H.call(plain, True, c.batch, c.noise, torch.from_numpy(c.ids), True)
    assert torch.equal(res[0], c.res[0]), "the taped wave differs"
    for n in tape.activation_names():
        assert torch.equal(tape.tensor(0, n), c.tape.tensor(0, n)), n
    got = plain.dec_input_grad(tape, c.d.to(DEV))
    for a, b in zip(got, c.input_grads):
        assert torch.equal(a, b)
    for n in tape.delta_names():
        assert torch.equal(tape.tensor(1, n), c.tape.tensor(1, n)), n
    assert "sine" not in c.tape.activation_names() and "g" not in c.tape.activation_names()
    with pytest.raises(Exception):
        tape.tensor(0, "sine")                       # a plain net's tape holds neither
    with pytest.raises(ValueError):
        plain.dec_weight_grad(tape)
    n = sum(int(np.prod(s)) for s in plain.dec_parameter_shapes().values())
    x = torch.zeros(n, device=DEV)
    assert raw_pass(plain, tape._h, [x.data_ptr()] * len(plain.dec_parameter_shapes())) != 0      # the C entry refuses too
    from comfy_rvc_amd import _lib
    assert b"keep_parameters" in _lib.lib.rvc_last_error()
    assert tape.nbytes < c.tape.nbytes
    record("tape_bytes_trainable_40k_v2_seg32", c.tape.nbytes // c.B, None)


# ------------------------------------------------------------------------------------------------ 5. launch count
def test_launch_count_is_a_constant_of_the_net(wcases):
    a, b = wcases("40k_v2").net.dec_weight_grad_launch_count(), wcases(SEG13).net.dec_weight_grad_launch_count()
    print("launches of the weight-gradient plan", a)
    record("launch_count_40k_v2", a, None)
    # per stage 19 dense layers (the up-sampler, 18 ResBlock convolutions) and conv_pre, two launches each (GEMM, finish); conv_post, cond; per stage one noise
    # convolution and m_source for the f0 family.  Nothing in the plan looks at B or at the segment.
    assert a == b == 2 * (4 * 19 + 1) + 2 + 4 + 1
    assert wcases("40k_v2_nono").net.dec_weight_grad_launch_count() == a - 5      # no noise convolutions (4), no m_source (1)
    assert H.make_net("40k_v2")[0].dec_weight_grad_launch_count() == a             # the plan's size is the net's, kept parameters or not


# ------------------------------------------------------------------------------------------------ 6. errors
def test_errors_raise_and_nothing_faults(wcases):
    from comfy_rvc_amd import _lib
    from comfy_rvc_amd.lib.infer_pack.models import GeneratorTape
    c, o = wcases("40k_v2"), wcases(SEG13)
    with pytest.raises(ValueError):
        o.net.dec_weight_grad(c.tape)                                     # the Python surface refuses another net's tape
    n = len(c.net.dec_parameter_shapes())
    x = torch.zeros(c.grads.flat.numel(), device=DEV)
    ptrs = [x.data_ptr()] * n
    assert raw_pass(o.net, c.tape._h, ptrs) != 0 and b"another" in _lib.lib.rvc_last_error()      # a tape of another handle and another segment
    fresh = GeneratorTape(c.net, 1, [0], 32)
    assert raw_pass(c.net, fresh._h, ptrs) != 0 and b"forward" in _lib.lib.rvc_last_error()       # no taped forward
    res, tape = H.call(c.net, True, c.batch, c.noise, torch.from_numpy(c.ids), True)
    assert raw_pass(c.net, tape._h, ptrs) != 0 and b"backward" in _lib.lib.rvc_last_error()       # no backward pass after the taped forward
    c.net.dec_input_grad(tape, c.d.to(DEV))
    assert raw_pass(c.net, tape._h, ptrs) == 0
    H.call_into(c, tape)                                                                            # recorded again: the deltas are stale
    assert raw_pass(c.net, tape._h, ptrs) != 0 and b"backward" in _lib.lib.rvc_last_error()
    with torch.cuda.device(DEV):
        st = _lib.current_stream()
        pt = (C.c_void_p * 17)(*([c.tape._h[0].value] * 17))
        pg = (C.c_void_p * n)(*ptrs)
        assert _lib.lib.rvc_synth_dec_weight_grad(c.net._h, st, pt, 0, pg) != 0                     # B < 1
        assert _lib.lib.rvc_synth_dec_weight_grad(c.net._h, st, pt, 17, pg) != 0 and b"16" in _lib.lib.rvc_last_error()      # B above the cap
        assert _lib.lib.rvc_synth_dec_weight_grad(c.net._h, st, pt, 16, pg) == 0                    # the cap itself runs
    assert _lib.lib.rvc_synth_dec_weight_grad_launch_count(None) == -1
    assert _lib.lib.rvc_conv1d_weight_grad_splits(1, 40, 32, 3, 100, 100, 1, 1, -1) == -1         # rows not a multiple of 16
    assert _lib.lib.rvc_conv1d_weight_grad_splits(17, 32, 32, 3, 100, 100, 1, 1, -1) == -1
    torch.cuda.synchronize()
    assert torch.equal(c.net.dec_weight_grad(c.tape).flat, c.grads.flat)      # the shared case is what it was


# ------------------------------------------------------------------------------------------------ 7. the reference's autograd, recorded and not gated
def test_distance_to_the_reference_autograd_golden_is_recorded(wcases):
    """tools/gen_golden_gen_wgrad.py: the reference's GeneratorNSF under float32 autograd on item 0 of the 40k_v2 golden batch, from the REFERENCE's z and with
    gen_grad_40k_v2.npz's cotangent.  The device starts from its own z and its own masks: the same ill-conditioned distance as dz's, recorded beside it."""
    c = wcases("40k_v2")
    g, gg = golden("gen_wgrad_40k_v2.npz"), golden("gen_grad_40k_v2.npz")
    names = [str(n) for n in g["names"]]
    assert names == list(c.net.dec_parameter_shapes())
    d = torch.zeros(c.B, 1, c.seg * c.upp)
    d[0] = torch.from_numpy(gg["d_y_hat"][0])
    try:
        c.net.dec_input_grad(c.tape, d.to(DEV))
        got = c.net.dec_weight_grad(c.tape)
        stride = int(g["stride"])
        for k, n in enumerate(names):
            v = got[n].cpu().numpy().reshape(-1)
            norm = float(np.linalg.norm(v.astype(np.float64)))
            e_norm = abs(norm - float(g["norms"][k])) / max(float(g["norms"][k]), 1e-30)
            e = rel_err(v[::stride], g[f"sample.{k}"])
            record(f"reference_golden_40k_v2.{n}", e, None)
            record(f"reference_golden_40k_v2.norm.{n}", e_norm, None)
            assert np.isfinite(e) and np.isfinite(e_norm), n
    finally:
        c.net.dec_input_grad(c.tape, c.d.to(DEV))
