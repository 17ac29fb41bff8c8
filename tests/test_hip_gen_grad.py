"""GPU: the recorded decoder forward (rvc_synth_forward_tape) and the decoder's backward data pass (rvc_synth_dec_input_grad) against the reference's goldens
and the float64 restatement (tests/gen_grad_ref.py).  Gate: conftest.rel_err < 1e-3, the project's fp32 gate.  Every measured value is kept by
conftest.record_parity under gen_grad.*; profiles/gen_grad_parity.json is a copy of those entries.

The parts: (1) the tape against the forward's truth; (2) the VJP GIVEN the tape - the masks come from the tape, so the pass is linear and the restatement on
the device's own activations is the exact map; (3) support; (4) placement and determinism; (5) the end-to-end distance to float64 autograd, recorded and not
gated (masks the forward's rounding flips make it ill conditioned); (6) the reference's own float32 autograd golden; (7) errors."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden, record_parity, rel_err
from comfy_rvc_amd import synthetic as S
from oracle import nets as N
import gen_grad_ref as G
from test_train_forward_host import CASES, TAPS, case_inputs

pytestmark = pytest.mark.gpu
GATE = 1e-3
DEV = "cuda:0"
SEG13 = "40k_v2_seg13"
TAGS = list(CASES) + [SEG13]


def record(name, value, gate):
    record_parity(f"gen_grad.{name}", {"measured": float(value), "gate": None if gate is None else float(gate)})


def net_config(tag):
    if tag == SEG13:      # columns per stage 130 / 1300 / 2600 / 5200: a ragged last tile in every stage (the golden segment of 32 gives multiples of 64 only)
        config, version, f0 = CASES["40k_v2"]
        config = list(config)
        config[1] = 13
        return tuple(config), version, f0
    return CASES[tag]


def make_net(tag):
    from comfy_rvc_amd.lib.infer_pack import models
    config, version, f0 = net_config(tag)
    cls = getattr(models, f"SynthesizerTrnMs{768 if version == 'v2' else 256}NSFsid" + ("" if f0 else "_nono"))
    net = cls(*config, is_half=False) if f0 else cls(*config)
    seed = int(golden(f"train_forward_{'40k_v2' if tag == SEG13 else tag}.npz")["weight_seed"])
    sd = S.synth_train_state_dict(config, version, seed, f0=f0)
    net.load_state_dict(sd)
    return net, sd


def call(net, f0, b, noise, ids, tape):
    t = {k: (None if v is None else torch.from_numpy(np.asarray(v))) for k, v in b.items()}
    fn = net.forward_with_tape if tape else net.forward
    if f0:
        return fn(t["phone"], t["lengths"], t["pitch"], t["pitchf"], t["spec"], t["lengths"], t["sid"], noise=noise, ids_slice=ids)
    return fn(t["phone"], t["lengths"], t["spec"], t["lengths"], t["sid"], noise=noise, ids_slice=ids)


def call_into(c, tape):
    t = {k: (None if v is None else torch.from_numpy(np.asarray(v))) for k, v in c.batch.items()}
    return c.net.forward_with_tape(t["phone"], t["lengths"], t["pitch"], t["pitchf"], t["spec"], t["lengths"], t["sid"], noise=c.noise,
                                   ids_slice=torch.from_numpy(c.ids), tape=tape)


class Case:
    """One net, one batch run through forward_with_tape once; the float64 restatement of item 0 on the device's own z tap, computed once and left unchanged."""

    def __init__(self, tag):
        self.tag = tag
        self.config, self.version, self.f0 = net_config(tag)
        self.net, self.sd = make_net(tag)
        self.seg, self.upp = self.config[1], int(np.prod(self.config[12]))
        if tag == SEG13:
            lengths = [29, 13]
            self.ids = np.array([9, 0], dtype=np.int64)
            self.batch = S.synth_train_batch(self.config, self.version, lengths, seed=41)
            gen = torch.Generator().manual_seed(42)
            self.noise = (torch.randn(2, 192, 29, generator=gen), torch.randn(2, 13 * self.upp, 1, generator=gen))
            self.golden = None
        else:
            _, _, self.batch, noise_q, noise_src, self.golden = case_inputs(tag)
            self.noise = (noise_q, noise_src) if self.f0 else noise_q
            self.ids = np.asarray(self.golden["ids_slice"])
        self.res, self.tape = call(self.net, self.f0, self.batch, self.noise, torch.from_numpy(self.ids), True)
        self.w = G.weights(self.sd, self.config, f0=self.f0)
        self.g = N.tensors(self.sd)["emb_g.weight"][int(self.batch["sid"][0])].double().view(1, -1, 1)
        self.acts_dev = {n: self.tape.tensor(0, n).cpu() for n in self.tape.activation_names()}
        i0 = int(self.ids[0])
        z = self.res[4][0][0:1, :, i0:i0 + self.seg].cpu().double()
        har = self.acts_dev["har"].double()[None] if self.f0 else None
        with torch.no_grad():
            self.acts_ref = G.forward(self.w, self.config, z, har, self.g)

    def acts_of(self, b):
        """item b's own taped activations (item 0's are kept)"""
        return self.acts_dev if b == 0 else {n: self.tape.tensor(b, n).cpu() for n in self.tape.activation_names()}

    def cotangent(self, seed, B=None):
        B = self.tape.B if B is None else B
        d = torch.randn(B, 1, self.seg * self.upp, generator=torch.Generator().manual_seed(seed))
        return d / d.flatten(1).norm(dim=1).view(B, 1, 1)      # about unit norm per item


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = Case(tag)
        return cache[tag]
    return get


# ------------------------------------------------------------------------------------------------ 1. the tape against the forward's truth
@pytest.mark.parametrize("tag", list(CASES))
def test_taped_forward_matches_reference_golden(tag, cases):
    c = cases(tag)
    o, ids_out, _, _, taps = c.res
    g = c.golden
    assert tuple(o.shape) == tuple(g["o"].shape) and np.array_equal(ids_out.cpu().numpy(), c.ids)
    for b, L in enumerate(int(x) for x in g["lengths"]):
        for k, t in zip(TAPS, taps):
            e = rel_err(t[b].cpu().numpy()[:, :L], g[k][b][:, :L])
            record(f"taped_golden_{tag}.item{b}.{k}", e, GATE)
            assert e < GATE, (tag, b, k, e)
        e = rel_err(o[b].cpu().numpy(), g["o"][b])
        print(tag, "item", b, "taped o against the reference", e)
        record(f"taped_golden_{tag}.item{b}.o", e, GATE)
        assert e < GATE, (tag, b, e)


@pytest.mark.parametrize("tag", TAGS)
def test_taped_tensors_match_float64_restatement(tag, cases):
    c = cases(tag)
    assert set(c.acts_dev) == set(c.acts_ref)
    worst = 0.0
    for n, ref in c.acts_ref.items():
        got = c.acts_dev[n]
        assert tuple(got.shape) == tuple(ref.shape), (n, got.shape, ref.shape)
        e = rel_err(got.numpy(), ref.numpy())
        record(f"tape_{tag}.{n}", e, GATE)
        worst = max(worst, e)
        assert e < GATE, (tag, n, e)
    print(tag, "worst taped tensor against the float64 restatement", worst)
    assert torch.equal(c.tape.tensor(0, "y_hat").view(-1), c.res[0][0, 0])      # o is the taped wave
    assert c.tape.nbytes > 0


def test_forward_is_untouched_by_a_taped_forward(cases):
    c = cases("40k_v2")
    ids = torch.from_numpy(c.ids)
    o1 = call(c.net, True, c.batch, c.noise, ids, False)[0].clone()
    o2 = call(c.net, True, c.batch, c.noise, ids, True)[0][0]
    o3 = call(c.net, True, c.batch, c.noise, ids, False)[0]
    assert torch.equal(o1, o3)
    e = rel_err(o2.cpu().numpy(), o1.cpu().numpy())
    print("taped wave against the fused forward's", e)
    record("taped_vs_fused_40k_v2.o", e, GATE)
    assert e < GATE


# ------------------------------------------------------------------------------------------------ 2. the VJP given the tape
@pytest.mark.parametrize("tag", TAGS)
def test_vjp_matches_restatement_on_the_taped_activations(tag, cases):
    c = cases(tag)
    d = c.cotangent(7)
    dz, dg, dhar, deltas = c.net.dec_input_grad(c.tape, d.to(DEV), return_deltas=True)
    assert (dhar is None) == (not c.f0)
    # item 0 and the batch's last item (its own handle, its own slice start; SEG13's is exactly one segment long with ids 0), each on its own taped activations
    for b in sorted({0, c.tape.B - 1}):
        name = f"vjp_{tag}" + ("" if b == 0 else f".item{b}")
        with torch.no_grad():
            v = G.vjp(c.w, c.config, c.acts_of(b), d[b:b + 1].double(), f0=c.f0)
        i0 = int(c.ids[b])
        got = {"dz": dz[b][:, i0:i0 + c.seg], "dg": dg[b]}
        if c.f0:
            got["dhar"] = dhar[b]
        for n, t in got.items():
            e = rel_err(t.cpu().numpy(), v[n].numpy())
            print(name, n, e)
            record(f"{name}.{n}", e, GATE)
            assert e < GATE, (name, n, e)
        outside = dz[b].clone()
        outside[:, i0:i0 + c.seg] = 0
        assert not outside.any()      # zero away from the slice
        # every name of delta_names(): the per-layer deltas under their own names, d.cond / d.g / d.har against the restatement's dcond / dg / dhar
        want = {n: v[n] for n in v if n.startswith("d.")}
        want.update({"d.cond": v["dcond"], "d.g": v["dg"]})
        if c.f0:
            want["d.har"] = v["dhar"]
        assert sorted(want) == sorted(c.tape.delta_names())
        worst = 0.0
        for n in c.tape.delta_names():
            e = rel_err(deltas[b][n].cpu().numpy().reshape(want[n].shape), want[n].numpy())
            record(f"{name}.{n}", e, GATE)
            worst = max(worst, e)
            assert e < GATE, (name, n, e)
        print(name, "worst delta", worst)
        assert torch.equal(deltas[b]["d.g"].view(-1), dg[b])
        if c.f0:
            assert torch.equal(deltas[b]["d.har"].view(-1), dhar[b])      # the tape's copy is what the caller received


# ------------------------------------------------------------------------------------------------ 3. support
def test_support_is_the_decoder_halo(cases):
    from comfy_rvc_amd import _lib
    c = cases("40k_v2")
    halo = int(_lib.lib.rvc_synth_dec_halo(c.net._h))
    assert halo == 11
    for f in (1, c.seg // 2, c.seg - 2):
        d = torch.zeros(c.tape.B, 1, c.seg * c.upp)
        d[:, 0, f * c.upp + c.upp // 2] = 1.0
        dz = c.net.dec_input_grad(c.tape, d.to(DEV))[0][0].cpu()
        i0 = int(c.ids[0])
        s = dz[:, i0:i0 + c.seg]
        lo, hi = max(0, f - halo), min(c.seg, f + halo + 1)
        assert s[:, f].abs().max() > 0
        assert not s[:, :lo].any() and not s[:, hi:].any(), (f, lo, hi)


# ------------------------------------------------------------------------------------------------ 4. placement and determinism
SENTINEL = 12345.0


def carve(shapes, fill, gap=1024):
    """one device pool filled with `fill`; a contiguous block per shape with `gap` untouched elements in front of, between and behind the blocks"""
    sizes = [int(np.prod(s)) for s in shapes]
    pool = torch.full((gap + sum(n + gap for n in sizes),), fill, dtype=torch.float32, device=DEV)
    views, inside, o = [], torch.zeros(pool.numel(), dtype=torch.bool, device=DEV), gap
    for s, n in zip(shapes, sizes):
        views.append(pool[o:o + n].view(*s))
        inside[o:o + n] = True
        o += n + gap
    return pool, views, inside


def raw_grad(c, d, dz, dcond, dg, dhar):
    from comfy_rvc_amd import _lib
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib.rvc_synth_dec_input_grad(c.net._h, _lib.current_stream(), c.tape._h[0], _lib.ptr(d), _lib.ptr(dz), _lib.ptr(dcond), _lib.ptr(dg),
                                                     _lib.ptr(dhar)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("tag", ["40k_v2", SEG13])
def test_outputs_are_placed_exactly_and_twice_the_same(tag, cases):
    c = cases(tag)
    d = c.cotangent(9)[0, 0].to(DEV).contiguous()
    n = c.seg * c.upp
    shapes = [(192, c.seg), (512,), (256,), (n,)]
    pool, (dz, dcond, dg, dhar), inside = carve(shapes, SENTINEL)
    raw_grad(c, d, dz, dcond, dg, dhar)
    assert bool((pool[~inside] == SENTINEL).all()), "an element outside the output blocks changed"
    assert not bool((pool[inside] == SENTINEL).any()), "an output element was not written"
    first = pool.clone()
    raw_grad(c, d, dz, dcond, dg, dhar)
    assert torch.equal(pool, first), "two calls differ"
    for skip in range(3):      # NULL for each optional output leaves the others bit-equal
        pool2, outs, _ = carve(shapes, SENTINEL)
        args = [outs[0]] + [None if k == skip else outs[1 + k] for k in range(3)]
        raw_grad(c, d, *args)
        for k, (a, b) in enumerate(zip(outs, (dz, dcond, dg, dhar))):
            if k == skip + 1:
                assert bool((a == SENTINEL).all())
            else:
                assert torch.equal(a, b), (skip, k)
        # the tape's own copies are written whether or not the caller asked for the output
        for n, ref in (("d.cond", dcond), ("d.g", dg), ("d.har", dhar)):
            assert torch.equal(c.tape.tensor(0, n).view(-1), ref), (skip, n)


def test_launch_count_does_not_depend_on_the_segment(cases):
    a, b = cases("40k_v2").net.dec_backward_launch_count(), cases(SEG13).net.dec_backward_launch_count()
    print("launches of the backward plan", a)
    record("launch_count_40k_v2", a, None)
    assert a == b and 60 < a < 100
    assert cases("40k_v2_nono").net.dec_backward_launch_count() == a - 4      # no noise convolutions
    nbytes = cases("40k_v2").tape.nbytes // cases("40k_v2").tape.B
    print("bytes of one 40k_v2 tape at 32 frames", nbytes)
    record("tape_bytes_40k_v2_seg32", nbytes, None)


# ------------------------------------------------------------------------------------------------ 5. end to end, recorded and not gated
def test_end_to_end_distance_to_float64_autograd_is_recorded(cases):
    c = cases("40k_v2")
    d = c.cotangent(7)
    dz = c.net.dec_input_grad(c.tape, d.to(DEV))[0][0].cpu()
    i0 = int(c.ids[0])
    z = c.acts_dev["z"][None]
    har = c.acts_dev["har"][None]

    def autograd(dtype):
        w = G.weights(c.sd, c.config, dtype=dtype)
        zz = z.to(dtype).requires_grad_()
        y = G.forward(w, c.config, zz, har.to(dtype), c.g.to(dtype))["y_hat"]
        return torch.autograd.grad(y, zz, grad_outputs=d[0].to(dtype))[0][0]
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ref, f32 = autograd(torch.float64), autograd(torch.float32)
    e_dev, e_f32 = rel_err(dz[:, i0:i0 + c.seg].numpy(), ref.numpy()), rel_err(f32.numpy(), ref.numpy())
    print("dz end to end against float64 autograd: device", e_dev, "torch float32 autograd", e_f32)
    record("end_to_end_40k_v2.dz.device", e_dev, None)
    record("end_to_end_40k_v2.dz.torch_float32", e_f32, None)
    assert np.isfinite(e_dev)


# ------------------------------------------------------------------------------------------------ 6. the reference's own float32 autograd
def test_distance_to_the_reference_autograd_golden_is_recorded(cases):
    """tools/gen_golden_gen_grad.py: the reference's GeneratorNSF under float32 autograd on item 0 of the 40k_v2 golden batch, from the REFERENCE's z.  The
    device starts from its own z (1e-5 away) and its own masks: the same ill-conditioned distance as the end-to-end figures, recorded beside them."""
    c = cases("40k_v2")
    g = golden("gen_grad_40k_v2.npz")
    assert int(g["ids"]) == int(c.ids[0])
    e = rel_err(c.res[0][0].cpu().numpy(), g["y_hat"][0])
    record("reference_golden_40k_v2.y_hat", e, GATE)
    assert e < GATE
    d = torch.zeros(c.tape.B, 1, c.seg * c.upp)
    d[0] = torch.from_numpy(g["d_y_hat"][0])
    dz, dg, _ = c.net.dec_input_grad(c.tape, d.to(DEV))
    i0 = int(c.ids[0])
    e_dz, e_dg = rel_err(dz[0][:, i0:i0 + c.seg].cpu().numpy(), g["dz"]), rel_err(dg[0].cpu().numpy(), g["dg"])
    print("against the reference's float32 autograd: dz", e_dz, "dg", e_dg)
    record("reference_golden_40k_v2.dz", e_dz, None)
    record("reference_golden_40k_v2.dg", e_dg, None)
    assert np.isfinite(e_dz) and np.isfinite(e_dg)


# ------------------------------------------------------------------------------------------------ 7. errors
def test_errors_raise_and_nothing_faults(cases):
    from comfy_rvc_amd import _lib
    from comfy_rvc_amd.lib.infer_pack.models import GeneratorTape
    c, o, nono = cases("40k_v2"), cases(SEG13), cases("40k_v2_nono")
    d = c.cotangent(3).to(DEV)
    with pytest.raises(ValueError):
        o.net.dec_input_grad(c.tape, d)                                  # the Python surface refuses another net's tape
    with pytest.raises(ValueError):                                      # and a tape of another batch size to record into
        call_into(c, GeneratorTape(c.net, 1, [0], 32))
    x = torch.zeros(192 * 32 + 12800, device=DEV)
    with torch.cuda.device(DEV):
        st = _lib.current_stream()
        rc = _lib.lib.rvc_synth_dec_input_grad(o.net._h, st, c.tape._h[0], _lib.ptr(x), _lib.ptr(x), None, None, None)
        assert rc != 0 and b"another" in _lib.lib.rvc_last_error()      # a tape from another handle (and another segment)
        fresh = GeneratorTape(c.net, 1, [0], 32)
        rc = _lib.lib.rvc_synth_dec_input_grad(c.net._h, st, fresh._h[0], _lib.ptr(x), _lib.ptr(x), None, None, None)
        assert rc != 0 and b"forward" in _lib.lib.rvc_last_error()      # backward before a taped forward
        rc = _lib.lib.rvc_synth_dec_input_grad(nono.net._h, st, nono.tape._h[0], _lib.ptr(x), _lib.ptr(x), None, None, _lib.ptr(x))
        assert rc != 0 and b"dhar" in _lib.lib.rvc_last_error()         # dhar requested from a no-f0 net
        p, r, k = C.c_void_p(), C.c_int(), C.c_int64()
        assert _lib.lib.rvc_gen_tape_tensor(c.tape._h[0], b"rb9.9.t9", C.byref(p), C.byref(r), C.byref(k)) != 0
    assert _lib.lib.rvc_synth_dec_input_grad_launch_count(None) == -1
    torch.cuda.synchronize()
