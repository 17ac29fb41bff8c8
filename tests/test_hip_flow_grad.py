"""GPU: the recording flow forward (forward_with_tape(..., record_flow=True)) and the flow's backward data pass (net_g.flow_input_grad,
rvc_synth_flow_input_grad) against the float64 restatement (tests/flow_grad_ref.py), synthetic weights.  Gate: conftest.rel_err (max |difference| / peak of the
tensor) < 1e-3, the project's fp32 gate.  Every figure is printed (-s); with FLOW_GRAD_PARITY_DUMP=<file.json> in the environment they are also written there
(profiles/flow_grad_parity.json).

The parts: (1) the VJP GIVEN the tape - the gate's derivative is read from the taped pre-gate activations, so the pass is linear and the restatement on the
device's own activations is the exact map; (2) the taped tensors against the float64 forward from the device's own z; (3) the recording forward against the
non-recording one; (4) masks, determinism, the launch count; (5) errors; (6) train_step.generator_latent_grad; (7) the end-to-end distance to float64 and to
float32 autograd, recorded and not gated.

Shapes.  An item runs at its own length, so its frames are the kernel's columns: 13 and 11 frames (less than one 64-column tile, the second item shorter than the
batch - the forward takes no item below 11 frames, the reach of the text encoder's relative-position window, so 11 stands where a 9-frame item was asked for),
65 and 64 frames (one column past a tile, and exactly one), 21 frames for the 256-feature v1 net and the no-f0 net.  The rows are the nets' own: 192 and 96
(one and a half 64-row tiles and three), K = 96 / 192 / 384 channels (2- and 4-unit stages), 1 and 5 taps."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import rel_err
from comfy_rvc_amd import synthetic as S
from oracle import nets as N
import flow_grad_ref as FR

pytestmark = pytest.mark.gpu
GATE = 1e-3
DEV = "cuda:0"
# tag -> (configuration, version, f0, segment, lengths)
CASES = {"40k_v2_T13": (S.CONFIG_40K_V2, "v2", True, 9, [13, 11]), "40k_v2_T65": (S.CONFIG_40K_V2, "v2", True, 13, [65, 64]),
         "32k_v1_T21": (S.CONFIG_32K_V1, "v1", True, 13, [21, 17]), "40k_v2_nono_T21": (S.CONFIG_40K_V2, "v2", False, 13, [21, 15])}
TAGS = list(CASES)


def record(key, value, gate=GATE):
    print(key, value)
    path = os.environ.get("FLOW_GRAD_PARITY_DUMP")
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


class Case:
    """One net, one batch run through forward_with_tape(record_flow=True) once; the float64 restatement of every item from the device's own z, computed once."""

    def __init__(self, tag):
        from comfy_rvc_amd.lib.infer_pack import models
        config, self.version, self.f0, seg, self.lengths = CASES[tag]
        config = list(config)
        config[1] = seg
        self.tag, self.config, self.seg, self.upp = tag, tuple(config), seg, int(np.prod(config[12]))
        cls = getattr(models, f"SynthesizerTrnMs{768 if self.version == 'v2' else 256}NSFsid" + ("" if self.f0 else "_nono"))
        self.net = cls(*self.config, is_half=False) if self.f0 else cls(*self.config)
        self.sd = S.synth_train_state_dict(self.config, self.version, 5, f0=self.f0)
        self.net.load_state_dict(self.sd)
        self.B, self.T, self.IC = len(self.lengths), max(self.lengths), self.config[2]
        self.batch = S.synth_train_batch(self.config, self.version, self.lengths, seed=41, f0=self.f0)
        gen = torch.Generator().manual_seed(42)
        nq, ns = torch.randn(self.B, self.IC, self.T, generator=gen), torch.randn(self.B, seg * self.upp, 1, generator=gen)
        self.noise = (nq, ns) if self.f0 else nq
        self.ids = torch.tensor([L - seg for L in self.lengths], dtype=torch.int64)
        self.res, self.tape = self.forward(record_flow=True)
        self.ws = FR.weights(self.sd)
        emb = N.tensors(self.sd)["emb_g.weight"].double()
        self.g = [emb[int(s)].view(1, -1, 1) for s in self.batch["sid"]]
        z = self.res[4][0].cpu().double()
        self.ref, self.acts_dev = [], []
        with torch.no_grad():
            for b, L in enumerate(self.lengths):
                self.ref.append(FR.forward(self.ws, z[b:b + 1, :, :L], torch.ones(1, 1, L, dtype=torch.float64), self.g[b]))
                self.acts_dev.append({n: self.tape.tensor(b, n).cpu() for n in self.tape.flow_activation_names()})

    def forward(self, record_flow, tape=None, with_tape=True):
        t = {k: (None if v is None else torch.from_numpy(np.asarray(v))) for k, v in self.batch.items()}
        args = (t["phone"], t["lengths"], t["pitch"], t["pitchf"], t["spec"], t["lengths"], t["sid"]) if self.f0 else (t["phone"], t["lengths"], t["spec"], t["lengths"], t["sid"])
        if not with_tape:
            return self.net.forward(*args, noise=self.noise, ids_slice=self.ids)
        return self.net.forward_with_tape(*args, noise=self.noise, ids_slice=self.ids, tape=tape, record_flow=record_flow)

    def cotangent(self, seed):
        """about unit norm per item, exactly 0 behind each length (as losses.kl_loss_grads leaves it)"""
        d = torch.randn(self.B, self.IC, self.T, generator=torch.Generator().manual_seed(seed))
        for b, L in enumerate(self.lengths):
            d[b, :, L:] = 0
        return d / d.flatten(1).norm(dim=1).view(self.B, 1, 1)


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = Case(tag)
        return cache[tag]
    return get


# ------------------------------------------------------------------------------------------------ 1. the VJP given the tape
@pytest.mark.parametrize("tag", TAGS)
def test_vjp_matches_restatement_on_the_taped_activations(tag, cases):
    c = cases(tag)
    d = c.cotangent(7)
    dz, dg, deltas = c.net.flow_input_grad(c.tape, d.to(DEV), return_deltas=True)
    assert tuple(dz.shape) == (c.B, c.IC, c.T) and tuple(dg.shape) == (c.B, c.config[16])
    names = c.tape.flow_delta_names()
    assert len(names) == 4 * 6 + 1
    for b, L in enumerate(c.lengths):
        acts = {n: t.double()[None] for n, t in c.acts_dev[b].items()}
        with torch.no_grad():
            v = FR.vjp(c.ws, acts, d[b:b + 1, :, :L].double(), torch.ones(1, 1, L, dtype=torch.float64))
        worst = 0.0
        for n, got, want in [("dz", dz[b][:, :L], v["dz"][0]), ("dg", dg[b], v["dg"][0])] + [(n, deltas[b][n], v[n][0]) for n in names]:
            assert got.numel() == want.numel(), (n, tuple(got.shape), tuple(want.shape))
            e = rel_err(got.cpu().numpy().reshape(want.shape), want.numpy())
            record(f"vjp_{tag}.item{b}.{n}", e)
            worst = max(worst, e)
            assert e < GATE, (tag, b, n, e)
        print(tag, "item", b, "worst", worst)
        assert torch.equal(deltas[b]["d.flow.g"].view(-1), dg[b])      # the tape's copy is what the caller received


# ------------------------------------------------------------------------------------------------ 2. the taped tensors
@pytest.mark.parametrize("tag", TAGS)
def test_taped_tensors_match_float64_forward(tag, cases):
    c = cases(tag)
    H = c.config[3]
    for b, L in enumerate(c.lengths):
        z_p_ref, acts_ref = c.ref[b]
        assert sorted(acts_ref) == sorted(c.tape.flow_activation_names())
        for n, want in acts_ref.items():
            got = c.acts_dev[b][n]
            assert tuple(got.shape) == tuple(want[0].shape) == ((2 * H if ".a" in n else H), L), (n, got.shape)
            e = rel_err(got.numpy(), want[0].numpy())
            record(f"tape_{tag}.item{b}.{n}", e)
            assert e < GATE, (tag, b, n, e)
        for f in range(4):
            assert torch.equal(c.acts_dev[b][f"flow{f}.x0"], c.acts_dev[b][f"flow{f}.h0"])
        e = rel_err(c.res[4][1][b, :, :L].cpu().numpy(), z_p_ref[0].numpy())
        record(f"tape_{tag}.item{b}.z_p", e)
        assert e < GATE, (tag, b, e)


# ------------------------------------------------------------------------------------------------ 3. the recording forward against the non-recording one
@pytest.mark.parametrize("tag", ["40k_v2_T13", "40k_v2_nono_T21"])
def test_recording_forward_against_the_non_recording_one(tag, cases):
    c = cases(tag)
    plain, tape0 = c.forward(record_flow=False)
    bytes0 = tape0.nbytes
    rec, tape1 = c.forward(record_flow=True)
    # the wave and the posterior's z do not depend on the flow: equal bits; z_p within the gate (the recording pass gates in a launch of its own)
    assert torch.equal(rec[0], plain[0]) and torch.equal(rec[4][0], plain[4][0])
    e = rel_err(rec[4][1].cpu().numpy(), plain[4][1].cpu().numpy())
    record(f"recording_{tag}.z_p_vs_plain", e)
    record(f"recording_{tag}.z_p_bit_equal", float(torch.equal(rec[4][1], plain[4][1])), None)
    assert e < GATE
    for k in range(2, 6):
        assert torch.equal(rec[4][k], plain[4][k])
    # record_flow=False is today's call: the same decoder tensors, the same byte count, and no flow tensor in the tape
    assert tape1.nbytes > bytes0 and tape0.nbytes == bytes0
    for n in ("z", "pre", "up0", "y_hat"):
        assert torch.equal(tape0.tensor(0, n), tape1.tensor(0, n)), n
    with pytest.raises(Exception):
        tape0.tensor(0, "flow0.h0")
    # forward itself is untouched by either
    assert torch.equal(c.forward(False, with_tape=False)[4][1], plain[4][1])
    # recording into a tape again after a non-recording pass into it: the flow must be recorded again before its backward
    c.forward(record_flow=False, tape=tape1)
    with pytest.raises(ValueError):
        c.net.flow_input_grad(tape1, c.cotangent(1).to(DEV))


# ------------------------------------------------------------------------------------------------ 4. masks, determinism, launch count
@pytest.mark.parametrize("tag", ["40k_v2_T13", "40k_v2_T65"])
def test_zero_behind_each_length_and_twice_the_same(tag, cases):
    c = cases(tag)
    d = c.cotangent(9)
    d_dirty = d.clone()
    for b, L in enumerate(c.lengths):
        d_dirty[b, :, L:] = 3.0      # whatever stands behind an item's length is never read
    dz, dg, deltas = c.net.flow_input_grad(c.tape, d.to(DEV), return_deltas=True)
    dz2, dg2, deltas2 = c.net.flow_input_grad(c.tape, d_dirty.to(DEV), return_deltas=True)
    assert torch.equal(dz, dz2) and torch.equal(dg, dg2), "two calls differ"
    for b, L in enumerate(c.lengths):
        assert not dz[b, :, L:].any()
        assert dz[b, :, :L].abs().max() > 0
        for n in deltas[b]:
            assert torch.equal(deltas[b][n], deltas2[b][n]), n


def test_launch_count_is_a_constant_of_the_net(cases):
    a, b = cases("40k_v2_T13").net.flow_backward_launch_count(), cases("40k_v2_T65").net.flow_backward_launch_count()
    record("launch_count_40k_v2", a, None)
    assert a == b == 49      # per coupling: Flip, post^T, three layers of (res_skip^T, the gate's derivative with its row sums, in_layers^T), pre^T; then cond_layer^T
    assert cases("40k_v2_nono_T21").net.flow_backward_launch_count() == a and cases("32k_v1_T21").net.flow_backward_launch_count() == a
    from comfy_rvc_amd import _lib
    assert _lib.lib.rvc_synth_flow_input_grad_launch_count(None) == -1
    c = cases("40k_v2_T13")
    record("tape_flow_bytes_40k_v2_T13", c.tape.nbytes, None)


# ------------------------------------------------------------------------------------------------ 5. errors
def test_errors_raise_and_nothing_faults(cases):
    from comfy_rvc_amd import _lib
    c, o = cases("40k_v2_T13"), cases("40k_v2_T65")
    d = c.cotangent(3).to(DEV)
    _, plain_tape = c.forward(record_flow=False)
    with pytest.raises(ValueError):
        c.net.flow_input_grad(plain_tape, d)                          # recorded without record_flow
    with pytest.raises(ValueError):
        o.net.flow_input_grad(c.tape, d)                              # a tape of a foreign net
    for shape in [(c.B, c.IC, c.T + 1), (c.B, c.IC - 1, c.T), (c.B + 1, c.IC, c.T), (c.B, c.IC * c.T)]:
        with pytest.raises(ValueError):
            c.net.flow_input_grad(c.tape, torch.zeros(shape, device=DEV))
    x = torch.zeros(c.IC * c.T, device=DEV)
    with torch.cuda.device(DEV):
        st = _lib.current_stream()
        rc = _lib.lib.rvc_synth_flow_input_grad(c.net._h, st, plain_tape._h[0], _lib.ptr(x), c.lengths[0], _lib.ptr(x), None)
        assert rc != 0 and b"record_flow" in _lib.lib.rvc_last_error()
        rc = _lib.lib.rvc_synth_flow_input_grad(o.net._h, st, c.tape._h[0], _lib.ptr(x), c.lengths[0], _lib.ptr(x), None)
        assert rc != 0 and b"another" in _lib.lib.rvc_last_error()
        rc = _lib.lib.rvc_synth_flow_input_grad(c.net._h, st, c.tape._h[0], _lib.ptr(x), c.lengths[0] - 1, _lib.ptr(x), None)
        assert rc != 0 and b"length" in _lib.lib.rvc_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. the wiring
def test_generator_latent_grad_is_the_sum_of_its_parts(cases):
    from comfy_rvc_amd.lib.train import train_step as TS
    c = cases("40k_v2_T13")
    kl = {"z_p": c.cotangent(5).to(DEV)}
    dy = torch.randn(c.B, 1, c.seg * c.upp, generator=torch.Generator().manual_seed(6)).to(DEV) * 1e-3
    dz_d, dg_d, dhar_d = TS.generator_decoder_backward(c.net, c.tape, dy)
    dz_f, dg_f = TS.generator_flow_backward(c.net, c.tape, kl)
    dz, dg, dhar = TS.generator_latent_grad(c.net, c.tape, dy, kl)
    assert torch.equal(dz, dz_d + dz_f) and torch.equal(dg, dg_d + dg_f) and torch.equal(dhar, dhar_d)
    assert torch.equal(dz_f, c.net.flow_input_grad(c.tape, kl["z_p"])[0])
    assert dz_f.abs().max() > 0 and dz_d.abs().max() > 0


# ------------------------------------------------------------------------------------------------ 7. end to end, recorded and not gated
def test_end_to_end_distance_to_autograd_is_recorded(cases):
    c = cases("40k_v2_T65")
    d = c.cotangent(7)
    dz, dg = c.net.flow_input_grad(c.tape, d.to(DEV))
    z = c.res[4][0].cpu()
    L = c.lengths[0]

    def autograd(dtype):
        ws = FR.weights(c.sd, dtype=dtype)
        zz, gg = z[0:1, :, :L].to(dtype).requires_grad_(), c.g[0].to(dtype).requires_grad_()
        z_p, _ = FR.forward(ws, zz, torch.ones(1, 1, L, dtype=dtype), gg)
        a, b = torch.autograd.grad(z_p, [zz, gg], grad_outputs=d[0:1, :, :L].to(dtype))
        return a[0], b[0, :, 0]
    torch.set_num_threads(min(16, torch.get_num_threads()))
    (rz, rg), (fz, fg) = autograd(torch.float64), autograd(torch.float32)
    for n, dev, f32, ref in (("dz", dz[0][:, :L].cpu(), fz, rz), ("dg", dg[0].cpu(), fg, rg)):
        e_dev, e_f32 = rel_err(dev.numpy(), ref.numpy()), rel_err(f32.numpy(), ref.numpy())
        record(f"end_to_end_40k_v2_T65.{n}.device", e_dev, None)
        record(f"end_to_end_40k_v2_T65.{n}.torch_float32", e_f32, None)
        assert np.isfinite(e_dev)
