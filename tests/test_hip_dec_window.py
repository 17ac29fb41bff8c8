"""GPU: the generator's keep window (rvc_synth_infer_window): inside the window every sample is bit for bit what the full-length run writes there.

Procedural 40k_v2 weights.  The full-length references are computed once per (length, pair arithmetic) and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

from comfy_rvc_amd import synthetic as S

pytestmark = pytest.mark.gpu

CONFIG, VERSION, UPP = S.CONFIG_40K_V2, "v2", 400
# T = 300: the fused-pair / bf16x3 kernels of short sequences, a window whose offsets are no multiple of any tile.
# T = 900: the last stage is 360 000 samples, above two rounds of 512-column tiles on 256 CUs: conv_rb3_kernel and the fp16x2 conv_x3q_kernel pairs engage.
CASES = {300: (37, 251), 900: (100, 800)}


def _lib():
    from comfy_rvc_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def net():
    from comfy_rvc_amd.lib.infer_pack import models as M
    n = M.SynthesizerTrnMs768NSFsid(*CONFIG, is_half=False)
    n.load_state_dict(S.synth_state_dict(CONFIG, VERSION, 0))
    return n


@pytest.fixture(scope="module")
def net_nono():
    from comfy_rvc_amd.lib.infer_pack import models as M
    n = M.SynthesizerTrnMs768NSFsid_nono(*CONFIG)
    n.load_state_dict(S.synth_state_dict(CONFIG, VERSION, 0, f0=False))
    return n


def _inputs(T, f0=True):
    rng = np.random.default_rng(1000 + T)
    gen = torch.Generator().manual_seed(T)
    d = {"T": T,
         "phone": torch.from_numpy((rng.standard_normal((T, 768)) * 0.5).astype(np.float32)).cuda(),
         "nz": torch.randn(192, T, generator=gen).cuda()}
    if f0:
        d["pitch"] = torch.from_numpy(rng.integers(1, 256, T).astype(np.int64)).cuda()
        d["pitchf"] = torch.from_numpy(S.designed_f0(T, seed=0).astype(np.float32)).cuda()
        d["ns"] = torch.randn(T * UPP, generator=gen).cuda()
    return d


def _run(n, d, keep=None, halo=None, out=None):
    """keep None: the old entry point.  Returns out [T * upp] (NaN wherever the call did not write, unless `out` is given)."""
    L = _lib()
    T = d["T"]
    if out is None:
        out = torch.full((T * UPP,), float("nan"), device="cuda")
    a = (n._h, None, L.ptr(d["phone"]), 0, L.ptr(d.get("pitch")), L.ptr(d.get("pitchf")), 0, L.ptr(d["nz"]), L.ptr(d.get("ns")), T, L.ptr(out), None)
    with torch.cuda.device(n.device):
        if keep is None:
            L.check(L.lib.rvc_synth_infer(*a))
        elif halo is None:
            L.check(L.lib.rvc_synth_infer_window(*a, keep[0], keep[1]))
        else:
            L.check(L.lib.rvc_synth_infer_window_halo(*a, keep[0], keep[1], halo))
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def full(net):
    """{(T, arithmetic): (inputs, full-length output)}, read-only."""
    L = _lib()
    prev = L.lib.rvc_get_pair_arithmetic()
    res = {}
    try:
        for T in CASES:
            d = _inputs(T)
            for arith in (0, 1):
                L.check(L.lib.rvc_set_pair_arithmetic(arith))
                res[(T, arith)] = (d, _run(net, d))
    finally:
        L.check(L.lib.rvc_set_pair_arithmetic(prev))
    return res


@pytest.fixture
def arith(request):
    L = _lib()
    prev = L.lib.rvc_get_pair_arithmetic()
    L.check(L.lib.rvc_set_pair_arithmetic(request.param))
    yield request.param
    L.check(L.lib.rvc_set_pair_arithmetic(prev))


def _same_in_window(out, ref, k0, k1):
    a, b = k0 * UPP, k1 * UPP
    assert not bool(torch.isnan(out[a:b]).any()), "the window holds samples the call never wrote"
    assert torch.equal(out[a:b], ref[a:b]), (int((out[a:b] != ref[a:b]).sum()), float((out[a:b] - ref[a:b]).abs().max()))


@pytest.mark.parametrize("arith", [0, 1], indirect=True)
@pytest.mark.parametrize("T", sorted(CASES))
def test_window_equals_full_run(net, full, T, arith, tmp_path):
    """out is filled with NaN first: a store shifted by the window's start would leave NaN inside the window or differ from the full run.

    At T = 900 the persistent pair kernel runs: it adds a tile's residual block by block, so a column's sum order depends on its place in the tile and the
    window has to start on a tile boundary of every stage (rvc_synth_window_frames reports the aligned range; a start at k0 - Hd = 89 differed in 278 473 of
    280 000 samples by up to 6.9e-6)."""
    L = _lib()
    d, ref = full[(T, arith)]
    assert not bool(torch.isnan(ref).any())
    k0, k1 = CASES[T]
    csv_path = str(tmp_path / "launches.csv")
    try:
        L.check(L.lib.rvc_prof_enable(1))
        out = _run(net, d, (k0, k1))
        L.check(L.lib.rvc_prof_dump_csv(csv_path.encode()))
    finally:
        L.check(L.lib.rvc_prof_enable(0))
    _same_in_window(out, ref, k0, k1)
    Hd = L.lib.rvc_synth_dec_halo(net._h)
    g0, g1 = C.c_int64(), C.c_int64()
    L.check(L.lib.rvc_synth_window_frames(net._h, T, k0, k1, C.byref(g0), C.byref(g1)))
    g0, g1 = g0.value, g1.value
    # the start moves down to a tile boundary of the pair kernels (at most 256 columns of the first stage: < 128 frames), the end is the halo's
    assert k0 - Hd - 128 < g0 <= k0 - Hd and g1 == k1 + Hd, (g0, g1)
    assert (g0, g1) == ((26, 262) if T == 300 else (64, 811)), (g0, g1)      # T = 300: no pair on the persistent kernel, nothing to align
    assert bool(torch.isnan(out[:g0 * UPP]).all()) and bool(torch.isnan(out[g1 * UPP:]).all()), "nothing is generated outside the reported frames"
    kernels = set(ln.split(",")[1] for ln in open(csv_path).read().strip().split("\n")[1:])
    if T == 900:
        assert "conv_x3q_kernel" in kernels, kernels
        if arith == 1:
            assert "conv_rb3_kernel" in kernels, kernels


def _launch_table(n, d, keep, path):
    """(output, rows of the launch table as dicts) of one run with per-launch profiling on."""
    L = _lib()
    try:
        L.check(L.lib.rvc_prof_enable(1))
        out = _run(n, d, keep)
        L.check(L.lib.rvc_prof_dump_csv(str(path).encode()))
    finally:
        L.check(L.lib.rvc_prof_enable(0))
    lines = open(path).read().strip().split("\n")
    cols = lines[0].split(",")
    return out, [dict(zip(cols, ln.split(","))) for ln in lines[1:]]


@pytest.mark.parametrize("arith", [0, 1], indirect=True)
def test_short_window_of_a_long_sequence_runs_the_full_runs_kernels(net, full, arith, tmp_path):
    """A window far too short to earn the full run's kernels on its own length: every launch is planned for the whole sequence, only its grid follows the window.

    The other cases would also pass with a planner that looked at the window's length (T = 300 runs nothing persistent, [64, 811) of 900 is long enough for
    every kernel of the full run).  Here the last stage has about 53 000 columns where conv_rb3_kernel asks for two rounds of 512-column tiles on 256 CUs and
    the fused pairs for 512 tiles."""
    L = _lib()
    T, (k0, k1) = 900, (400, 500)
    d, ref = full[(T, arith)]
    g0, g1 = C.c_int64(), C.c_int64()
    L.check(L.lib.rvc_synth_window_frames(net._h, T, k0, k1, C.byref(g0), C.byref(g1)))
    g0, g1 = g0.value, g1.value
    assert 0 <= g0 <= k0 and k1 <= g1 <= T and (g1 - g0) * UPP < 2 * 256 * 512, (g0, g1)
    _, rows_full = _launch_table(net, d, None, tmp_path / "full.csv")
    out, rows_win = _launch_table(net, d, (k0, k1), tmp_path / "window.csv")
    _same_in_window(out, ref, k0, k1)
    # the generator's rows: in the windowed table everything behind the last full-length launch (text encoder and flow run on all T frames)
    assert len(rows_full) == len(rows_win), (len(rows_full), len(rows_win))
    first = max(i for i, r in enumerate(rows_win) if int(r["Tout"]) == T) + 1
    assert first < len(rows_win)
    same = ("kernel", "tile", "Ci", "Co", "k", "dil", "stride", "fused_pair", "ksplit", "mfma_per_product")      # only Tout and workgroups may differ
    for i in range(first, len(rows_win)):
        assert [rows_win[i][c] for c in same] == [rows_full[i][c] for c in same], (i, rows_win[i], rows_full[i])
        assert int(rows_win[i]["Tout"]) < int(rows_full[i]["Tout"]), (i, rows_win[i], rows_full[i])
    kernels = set(r["kernel"] for r in rows_win[first:])
    assert "conv_x3q_kernel" in kernels, kernels
    if arith == 1:
        assert "conv_rb3_kernel" in kernels, kernels


@pytest.mark.parametrize("arith", [0, 1], indirect=True)
def test_halo_is_sufficient_and_tight(net, full, arith):
    """The derived halo reproduces the window; one frame less must not (otherwise the derivation is loose by a frame)."""
    L = _lib()
    T = 300
    d, ref = full[(T, arith)]
    k0, k1 = CASES[T]
    Hd = L.lib.rvc_synth_dec_halo(net._h)
    assert Hd == 11          # 40k_v2: 3 -> 63 -> 32 -> 92 -> 47 -> 107 -> 11 -> 71 -> 8 -> 11 (synth_dec_halo_frames)
    _same_in_window(_run(net, d, (k0, k1), halo=Hd), ref, k0, k1)
    short = _run(net, d, (k0, k1), halo=Hd - 1)
    a, b = k0 * UPP, k1 * UPP
    assert not torch.equal(short[a:b], ref[a:b]), "a halo of Hd - 1 frames is enough: synth_dec_halo_frames is loose"


@pytest.mark.parametrize("keep", [(3, 200), (120, 300), (0, 300), (150, 155)], ids=["start_clamped", "to_the_end", "whole", "narrow"])
def test_window_edges(net, full, keep):
    T = 300
    d, ref = full[(T, 1)]
    out = _run(net, d, keep)
    _same_in_window(out, ref, *keep)
    if keep == (0, T):
        assert torch.equal(out, ref)


@pytest.mark.parametrize("keep", [(50, 50), (60, 40), (0, 301), (-1, 10)])
def test_window_rejects_bad_ranges(net, full, keep):
    d, _ = full[(300, 1)]
    with pytest.raises(RuntimeError, match="keep window"):
        _run(net, d, keep)
    assert b"keep window" in _lib().lib.rvc_last_error()


def test_window_no_f0_model(net_nono):
    d = _inputs(300, f0=False)
    ref = _run(net_nono, d)
    for keep in (CASES[300], (0, 300)):
        _same_in_window(_run(net_nono, d, keep), ref, *keep)
    assert _lib().lib.rvc_synth_dec_halo(net_nono._h) == 11


def test_infer_keep_argument(net, full):
    d, ref = full[(300, 1)]
    T = 300
    o, _, _ = net.infer(d["phone"][None], torch.LongTensor([T]), d["pitch"][None], d["pitchf"][None], torch.LongTensor([0]),
                        noise=(d["nz"][None], d["ns"][None, :, None]), keep=CASES[T])
    _same_in_window(o.view(-1), ref, *CASES[T])


@pytest.mark.parametrize("resample_sr", [0, 48000], ids=["device_path", "host_path"])
def test_pipeline_same_int16_with_and_without_window(noise_tape, resample_sr):
    """vc_single on the 2 s clip: the generator on the kept window against the same call with the window forced to [0, T)."""
    from conftest import golden
    from comfy_rvc_amd.config import Config
    from comfy_rvc_amd.lib.infer_pack.loaders import HubertModelWithFinalProj
    from comfy_rvc_amd.vc_infer_pipeline import VC, get_vc, vc_single
    g = golden("pipeline_2s_designed.npz")
    hub = HubertModelWithFinalProj(S.hubert_state_dict(0), S.HUBERT_CONFIG)
    vcd = get_vc(S.synth_checkpoint(CONFIG, VERSION, 0), config=Config())
    outs = []
    for windowed in (True, False):
        vc = VC(40000, Config())
        vc.decoder_window = windowed
        vc.noise_fn = noise_tape(g["noise_seed"])
        vc.f0_method_dict["pm"] = lambda x, **k: S.designed_f0(x.shape[0] // 160 + 1, seed=0).astype(np.float64)
        out = vc_single(cpt=vcd["cpt"], net_g=vcd["net_g"], vc=vc, hubert_model=hub, input_audio=(g["audio"], 16000), sid=0, f0_up_key=0,
                        f0_method="pm", index_rate=0.0, rms_mix_rate=0.25, protect=0.33, resample_sr=resample_sr)
        assert out is not None
        outs.append(out[0])
    assert outs[0].dtype == np.int16 and outs[0].shape == outs[1].shape and np.array_equal(outs[0], outs[1])
