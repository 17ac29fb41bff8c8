"""GPU parity of the model-glue kernels (csrc/ops.hip without the GEMMs, csrc/split2d.hip) one op at a time through the rvc_op_* entry points, against the
float64 restatements of tests/glue_ref.py (pinned on the CPU by tests/test_glue_ref_host.py).

Every input lies inside a larger NaN-filled device buffer (a read one element out of range poisons the result) and every output inside a larger
sentinel-filled one with a pitch beyond its extent (a stray write shows without a fault).  Tolerances: exact where the op copies; 4 * 2^-24 * sum |terms|
where it is a short float32 sum; 2^-16 |v| between an image (bf16 hi + lo) and the fp32 output of the same call; and for the transcendental ops - hubert_conv0,
wn_gate, conv_to1 with tanh, gru_scan - at most 8 x the error torch's own float32 CPU ops make on the same inputs against float64 (floor 4 * 2^-24 * max |ref|):
both errors are recorded through conftest.record_parity under "glue/" keys (committed as profiles/glue_parity.json)."""
import ctypes as C
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_ref as R
from conftest import record_parity

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
FILL = {np.dtype(np.float32): -7777.25, np.dtype(np.float64): -7777.25, np.dtype(np.int64): -7777, np.dtype(np.int16): -7777}


@pytest.fixture(scope="module")
def L():
    from comfy_rvc_amd import _lib
    _lib.get_ctx(0)
    return _lib


def grid(rows, cols, ld, base=0):
    """flat offsets of a [rows][cols] block with row pitch ld"""
    return base + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]


class Buf:
    """A device buffer whose elements at the flat offsets `idx` (from .ptr) hold `values` and every other element - `lead` in front, the gaps a pitch leaves,
    `tail` behind - holds `fill` (NaN for inputs, a sentinel for outputs).  get() returns the block and asserts that nothing else changed."""

    def __init__(self, idx, values=None, dtype=np.float32, lead=64, tail=256, fill=None):
        self.idx = np.asarray(idx, dtype=np.int64)
        self.dtype = np.dtype(dtype)
        self.fill = (np.nan if values is not None else FILL[self.dtype]) if fill is None else fill
        self.lead = lead
        host = np.full(lead + int(self.idx.max()) + 1 + tail, self.fill, self.dtype)
        if values is not None:
            host[lead + self.idx] = np.asarray(values, self.dtype)
        self.before = host
        self.t = torch.from_numpy(host.copy()).cuda()

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + self.lead * self.dtype.itemsize)

    def get(self):
        h = self.t.cpu().numpy()
        outside = np.ones(h.size, bool)
        outside[self.lead + self.idx.ravel()] = False
        assert np.array_equal(h[outside], self.before[outside], equal_nan=True), "the op wrote outside its result"
        return h[self.lead + self.idx]

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy(), self.before, equal_nan=True)


def out_block(rows, cols, ld, dtype=np.float32, lead=64):
    return Buf(grid(rows, cols, ld), dtype=dtype, lead=lead, tail=2 * ld + 64)


def record(name, stats):
    """beside the full-size parity figures (conftest.record_parity), under keys that start with "glue/"; profiles/glue_parity.json is that part of the file"""
    record_parity("glue/" + name, stats)


def check_8x(name, got, ref, f32):
    """the kernel's largest error against float64 is at most 8 x that of torch's float32 CPU ops on the same inputs (floor 4 * 2^-24 * max |ref|)"""
    got, ref, f32 = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(f32, np.float64)
    assert got.shape == ref.shape == f32.shape and np.all(np.isfinite(got))
    ek, ef, floor = float(np.max(np.abs(got - ref))), float(np.max(np.abs(f32 - ref))), 4 * U24 * float(np.max(np.abs(ref)))
    record(name, {"kernel_max_err": ek, "float32_max_err": ef, "floor": floor})
    print(f"{name}: kernel {ek:.3e} float32 {ef:.3e} floor {floor:.3e}")
    assert ek <= max(8 * ef, floor), f"{name}: kernel error {ek:.3e} > 8 x float32 error {ef:.3e} (floor {floor:.3e})"


def check_terms(got, ref, mag, what):
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    excess = np.abs(got - ref) - 4 * U24 * mag
    assert np.all(excess <= 0), f"{what}: {int((excess > 0).sum())} elements beyond 4 * 2^-24 * sum |terms| (worst {float(np.max(np.abs(got - ref) / np.maximum(mag, 1e-300)) / U24):.2f} x 2^-24)"


def check_image(img, y, what):
    img, y = np.asarray(img, np.float64), np.asarray(y, np.float64)
    assert img.shape == y.shape and np.all(np.isfinite(img)), what
    assert np.all(np.abs(img - y) <= 2.0 ** -16 * np.abs(y)), what


# ------------------------------------------------------------------------------------------------ hubert_conv0
CONV0 = [(512, 511), (512, 512), (512, 513), (512, 1023), (512, 1025), (512, 2051), (80, 700), (272, 600), (16, 5)]


def _conv0_case(L, name, C, T1, extra, audio):
    g = np.random.default_rng(1000 * C + T1)
    w = (g.standard_normal((C, 10)) * 0.3).astype(np.float32)
    gamma, beta = g.uniform(0.5, 1.5, C).astype(np.float32), (g.standard_normal(C) * 0.2).astype(np.float32)
    n = audio.size
    assert n == 5 * (T1 - 1) + 10 + extra
    ref = R.hubert_conv0(audio, w, gamma, beta, T1)
    conv = F.conv1d(torch.from_numpy(audio)[None, None], torch.from_numpy(w)[:, None], stride=5)
    f32 = F.gelu(F.group_norm(conv, C, torch.from_numpy(gamma), torch.from_numpy(beta), 1e-5))[0].numpy()
    assert f32.shape == (C, T1)
    ld = T1 + 3
    a, wd, gd, bd = Buf(np.arange(n), audio), Buf(grid(C, 10, 10), w), Buf(np.arange(C), gamma), Buf(np.arange(C), beta)
    out = out_block(C, T1, ld)
    img = out_block(C, T1, ld) if C % 16 == 0 else None
    L.check(L.lib.rvc_op_hubert_conv0(None, a.ptr, n, wd.ptr, gd.ptr, bd.ptr, C, T1, out.ptr, img.ptr if img else None, ld))
    y = out.get()
    check_8x(name, y, ref, f32)
    if img:
        check_image(img.get(), y, name)
        # image alone (the form HuBERT runs): the same values
        img2 = out_block(C, T1, ld)
        L.check(L.lib.rvc_op_hubert_conv0(None, a.ptr, n, wd.ptr, gd.ptr, bd.ptr, C, T1, None, img2.ptr, ld))
        check_image(img2.get(), y, name)


@pytest.mark.parametrize("extra", [0, 1, 4])
@pytest.mark.parametrize("C,T1", CONV0)
def test_hubert_conv0(L, C, T1, extra):
    g = np.random.default_rng(7 * T1 + extra)
    audio = (g.standard_normal(5 * (T1 - 1) + 10 + extra) * 0.1).astype(np.float32)
    _conv0_case(L, f"hubert_conv0[{C}x{T1}+{extra}]", C, T1, extra, audio)


def test_hubert_conv0_dc_offset(L):
    """a DC offset of 0.1 under a signal of rms 0.05 (rvc_hubert_forward is public and does not high-pass): the variance is formed as E[a^2] - mean^2"""
    C, T1 = 512, 1025
    g = np.random.default_rng(99)
    audio = (0.1 + g.standard_normal(5 * (T1 - 1) + 10) * 0.05).astype(np.float32)
    _conv0_case(L, f"hubert_conv0_dc[{C}x{T1}]", C, T1, 0, audio)


# ------------------------------------------------------------------------------------------------ conv_to1
CONV_TO1_T = [1, 3, 4, 7, 8, 9, 1023, 1024, 1025, 1030]


def _conv_to1(L, name, x, w, K, pad, ldx, lead, slope, act, want_kernel, failures):
    Ci, T = x.shape
    ref, mag = R.conv_to1(x, w, pad, slope, act)
    xd, wd = Buf(grid(Ci, T, ldx), x, lead=lead), Buf(grid(Ci, K, K), w)
    out = Buf(np.arange(T))
    which = C.c_int(-1)
    L.check(L.lib.rvc_op_conv_to1(None, xd.ptr, ldx, wd.ptr, Ci, K, pad, T, slope, act, out.ptr, C.byref(which)))
    assert which.value == want_kernel, f"{name}: kernel {which.value} ran, expected {want_kernel}"
    y = out.get()
    s = float(np.float32(slope))
    f32 = F.conv1d(F.leaky_relu(torch.from_numpy(x), s)[None], torch.from_numpy(w)[None], padding=pad)[0, 0]
    if act:
        check_8x(name, y, ref, torch.tanh(f32).numpy())
        return
    # (torch's float32 convolution on the same scale, printed beside the kernel's figure: it is not part of the bound)
    worst = float(np.max(np.abs(y.astype(np.float64) - ref) / mag) / U24)
    worst32 = float(np.max(np.abs(f32.numpy().astype(np.float64) - ref) / mag) / U24)
    print(f"{name}: worst |err| / sum|terms| = {worst:.2f} x 2^-24 (torch float32 conv1d: {worst32:.2f})")
    try:
        check_terms(y, ref, mag, name)
    except AssertionError as e:
        failures.append(f"{e} (torch float32 conv1d: {worst32:.2f} x 2^-24)")


def _conv_to1_variants(L, Ci, T, act):
    g = np.random.default_rng(100 * Ci + T)
    x = g.standard_normal((Ci, T)).astype(np.float32)
    ld4 = (T + 3) // 4 * 4 + 4
    failures = []
    for slope in (0.01, 1.0):
        tag = f"[Ci{Ci} T{T} tanh{act} slope{slope}]"
        w7 = (g.standard_normal((Ci, 7)) / np.sqrt(Ci * 7)).astype(np.float32)
        _conv_to1(L, "conv_to1_x4" + tag, x, w7, 7, 3, ld4, 64, slope, act, 1, failures)          # 16-byte aligned rows: four outputs per thread
        _conv_to1(L, "conv_to1_off1" + tag, x, w7, 7, 3, ld4, 65, slope, act, 0, failures)        # x_dev off by one float
        # ldx = T + 1: the scalar kernel - except where T + 1 is itself a multiple of 4 (T = 3, 7, 1023), where aligned rows of that pitch are the 4-wide
        # kernel's by its own rule; there T + 2 is the odd pitch
        if (T + 1) % 4 == 0:
            _conv_to1(L, "conv_to1_ldT1" + tag, x, w7, 7, 3, T + 1, 64, slope, act, 1, failures)
            _conv_to1(L, "conv_to1_ldT2" + tag, x, w7, 7, 3, T + 2, 64, slope, act, 0, failures)
        else:
            _conv_to1(L, "conv_to1_ldT1" + tag, x, w7, 7, 3, T + 1, 64, slope, act, 0, failures)
        for K, pad in ((5, 2), (9, 4)):
            wk = (g.standard_normal((Ci, K)) / np.sqrt(Ci * K)).astype(np.float32)
            _conv_to1(L, f"conv_to1_k{K}" + tag, x, wk, K, pad, ld4, 64, slope, act, 0, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("T", CONV_TO1_T)
@pytest.mark.parametrize("Ci", [16, 32])
def test_conv_to1_tanh(L, Ci, T):
    """kernel selection (aligned rows / off by one float / odd pitch / k = 5, 9) and the result through tanh, by the 8 x rule"""
    _conv_to1_variants(L, Ci, T, 1)


@pytest.mark.parametrize("T", CONV_TO1_T)
@pytest.mark.parametrize("Ci", [16, 32])
def test_conv_to1_linear(L, Ci, T):
    """the same without tanh: every element within 4 * 2^-24 * sum |terms| of float64.  (One FMA chain over all Ci K products missed this at Ci = 32,
    T >= 1023 - 4.7 to 6.4 x 2^-24 at one or two outputs, torch's float32 conv1d 1.6 to 2.4 on the same inputs; the kernels sum groups of four channels: <= 2.4.)"""
    _conv_to1_variants(L, Ci, T, 0)


# ------------------------------------------------------------------------------------------------ noise_add
def _noise_call(L, x, ld, lead, C_, T, src, Lsrc, k, stride, pad, w, b):
    xd = Buf(grid(C_, T, ld), x, lead=lead, tail=2 * ld + 64)
    sd, wd, bd = Buf(np.arange(Lsrc), src[:Lsrc]), Buf(grid(C_, k, k), w), Buf(np.arange(C_), b)
    ran = C.c_int(-1)
    L.check(L.lib.rvc_op_noise_add(None, xd.ptr, ld, C_, T, sd.ptr, Lsrc, k, stride, pad, wd.ptr, bd.ptr, C.byref(ran)))
    return ran.value, xd


@pytest.mark.parametrize("C_", [16, 32, 24, 8])
@pytest.mark.parametrize("k,stride", [(1, 1), (4, 2), (8, 4)])
def test_noise_add(L, k, stride, C_):
    pad = stride // 2 if k > 1 else 0
    g = np.random.default_rng(10 * k + C_)
    w, b = g.standard_normal((C_, k)).astype(np.float32), g.standard_normal(C_).astype(np.float32)
    for T in (4, 1020, 1024, 1028):
        x, src = g.standard_normal((C_, T)).astype(np.float32), g.standard_normal(T * stride).astype(np.float32)
        for Lsrc in (T * stride, T * stride - stride - 1):
            ran, xd = _noise_call(L, x, T + 4, 64, C_, T, src, Lsrc, k, stride, pad, w, b)
            assert ran == 1
            ref, mag = R.noise_add(x, src[:Lsrc], Lsrc, w, b, stride, pad)
            check_terms(xd.get(), ref, mag, f"noise_add[k{k} C{C_} T{T} L{Lsrc}]")


@pytest.mark.parametrize("what", ["T1022", "ldT+1", "k3", "off1"])
def test_noise_add_declines(L, what):
    g = np.random.default_rng(5)
    C_, T, k, stride, lead = 16, 1024, 4, 2, 64
    if what == "T1022":
        T = 1022
    ld = T + 1 if what == "ldT+1" else (T + 3) // 4 * 4 + 4
    if what == "k3":
        k = 3
    if what == "off1":
        lead = 65
    x, src = g.standard_normal((C_, T)).astype(np.float32), g.standard_normal(T * stride).astype(np.float32)
    w, b = g.standard_normal((C_, k)).astype(np.float32), g.standard_normal(C_).astype(np.float32)
    ran, xd = _noise_call(L, x, ld, lead, C_, T, src, T * stride, k, stride, 1, w, b)
    assert ran == 0 and xd.unchanged()


# ------------------------------------------------------------------------------------------------ transpose, frames, mel_to_unet, feats_prepare
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("Rr,Cc", [(1, 1), (31, 33), (32, 32), (33, 65), (360, 101), (5, 128)])
def test_transpose(L, Rr, Cc, batch):
    g = np.random.default_rng(Rr * 1000 + Cc)
    x = g.standard_normal((batch, Rr, Cc)).astype(np.float32)
    for ldin, ldout, off in ((Cc + 3, Rr + 5, 0), (Cc + 3, Rr + 2, 1)):          # the second: MDX23C's form, the output pointer one float in, pitch R + 2
        bin_, bout = Rr * ldin + 7, Cc * ldout + 11
        iidx = np.arange(batch)[:, None, None] * bin_ + grid(Rr, Cc, ldin)[None]
        oidx = np.arange(batch)[:, None, None] * bout + grid(Cc, Rr, ldout)[None]
        xd, out = Buf(iidx, x), Buf(oidx, lead=64 + off, tail=2 * ldout + 64)
        L.check(L.lib.rvc_op_transpose(None, xd.ptr, out.ptr, Rr, Cc, ldin, ldout, batch, bin_, bout))
        assert np.array_equal(out.get(), x.transpose(0, 2, 1))


@pytest.mark.parametrize("case", [(2000, 1024, 160, 512, 13, 1), (1025, 1024, 160, 512, 7, 1), (100, 8, 4, 2, 25, 0), (100, 8, 4, 2, 26, 0), (37, 4, 2, 1, 19, 0)])
def test_frames(L, case):
    Ls, k, stride, pad, Tout, reflect = case
    src = np.random.default_rng(Ls + Tout).standard_normal(Ls).astype(np.float32)
    sd, out = Buf(np.arange(Ls), src), Buf(grid(k, Tout, Tout))
    L.check(L.lib.rvc_op_frames(None, sd.ptr, out.ptr, Ls, k, stride, pad, Tout, reflect))
    assert np.array_equal(out.get(), R.frames(src, k, stride, pad, Tout, reflect))


@pytest.mark.parametrize("n", [32, 33, 47, 64, 65, 100])
def test_mel_to_unet(L, n):
    Tr = 32 * ((n + 31) // 32)
    mel = (np.random.default_rng(n).standard_normal((128, n)) * 3).astype(np.float32)
    md, out = Buf(grid(128, n, n), mel), Buf(grid(Tr, 128, 128), tail=512)
    L.check(L.lib.rvc_op_mel_to_unet(None, md.ptr, out.ptr, n, Tr, 0.37, -1.25))
    ref, mag = R.mel_to_unet(mel, Tr, 0.37, -1.25)
    check_terms(out.get(), ref, mag, f"mel_to_unet[{n}]")


@pytest.mark.parametrize("Th", [1, 50])
@pytest.mark.parametrize("D", [256, 768])
def test_feats_prepare(L, D, Th):
    T = 2 * Th
    g = np.random.default_rng(D + Th)
    f, f0 = g.standard_normal((D, Th)).astype(np.float32), g.standard_normal((D, Th)).astype(np.float32)
    special = np.array([0.0, 0.5, 1.0, 220.0, -1.0], np.float32)
    if T >= 5:
        pfs = [np.r_[special, g.uniform(0, 400, T - 5).astype(np.float32)]]
        pfs[0][5::7] = 0.0
    else:                                                              # two frames: every special value in turn
        pfs = [np.array(p, np.float32) for p in ((0.0, 0.5), (1.0, 220.0), (-1.0, 0.5), (220.0, 0.0))]
    fd, f0d = Buf(grid(D, Th, Th), f), Buf(grid(D, Th, Th), f0)
    for pf in pfs:
        pd = Buf(np.arange(T), pf)
        for protect in (0.33, 0.5):
            for do_protect in (0, 1):
                for use_f0 in (False, True):
                    out = Buf(grid(D, T, T))
                    L.check(L.lib.rvc_op_feats_prepare(None, fd.ptr, f0d.ptr if use_f0 else None, pd.ptr, out.ptr, D, Th, T, protect, do_protect))
                    ref, mag = R.feats_prepare(f, f0 if use_f0 else None, pf, T, protect, do_protect)
                    check_terms(out.get(), ref, mag, f"feats_prepare[D{D} Th{Th} p{protect} do{do_protect} f0{use_f0}]")


# ------------------------------------------------------------------------------------------------ wn_gate
@pytest.mark.parametrize("T", [1, 255, 256, 257])
@pytest.mark.parametrize("H", [16, 192])
def test_wn_gate(L, H, T):
    g = np.random.default_rng(H + T)
    a = (g.standard_normal((2 * H, T)) * 8).astype(np.float32)
    a[0, 0], a[H, 0], a[1, T - 1], a[H + 1, T - 1] = 30.0, -30.0, -30.0, 30.0          # both halves reach +-30: tanh and the sigmoid saturate
    gg = (g.standard_normal(2 * H) * 0.5).astype(np.float32)
    gg[[0, H, 1, H + 1]] = 0.0
    ad, gd = Buf(grid(2 * H, T, T), a), Buf(np.arange(2 * H), gg)
    out, img = Buf(grid(H, T, T)), Buf(grid(H, T, T))
    L.check(L.lib.rvc_op_wn_gate(None, ad.ptr, gd.ptr, out.ptr, img.ptr, H, T))
    t = torch.from_numpy(a) + torch.from_numpy(gg)[:, None]
    y = out.get()
    check_8x(f"wn_gate[{H}x{T}]", y, R.wn_gate(a, gg), (torch.tanh(t[:H]) * torch.sigmoid(t[H:])).numpy())
    check_image(img.get(), y, "wn_gate image")
    img2 = Buf(grid(H, T, T))
    L.check(L.lib.rvc_op_wn_gate(None, ad.ptr, gd.ptr, None, img2.ptr, H, T))
    check_image(img2.get(), y, "wn_gate image alone")


# ------------------------------------------------------------------------------------------------ split2d
def _three(call, idx):
    """the op with fp32 only, image only and both: -> (y, img of `both`, img alone); the two fp32 results must be equal bit for bit"""
    res = {}
    for mode in ("y", "img", "both"):
        y = Buf(idx, tail=4096) if mode != "img" else None
        im = Buf(idx, tail=4096) if mode != "y" else None
        call(y, im)
        res[mode] = (y.get() if y else None, im.get() if im else None)
    assert np.array_equal(res["y"][0], res["both"][0])
    return res["both"][0], res["both"][1], res["img"][1]


@pytest.mark.parametrize("H,W", [(2, 2), (4, 6), (5, 7), (33, 128), (32, 16)])
@pytest.mark.parametrize("C_", [16, 32])
def test_split2d(L, C_, H, W):
    g = np.random.default_rng(C_ * 100 + H * 7 + W)
    x = g.standard_normal((C_, H, W)).astype(np.float32)
    Wp = W + 2
    nan_cols = np.full((C_, H, 1), np.nan, np.float32)

    # pad2d: plain -> padded fp32 / image; exact copies, exact zero side columns
    ldx, ldy = H * W + 5, H * Wp + 3
    xd = Buf(grid(C_, H * W, ldx), x.reshape(C_, -1))
    pidx = grid(C_, H * Wp, ldy)
    y, im, im1 = _three(lambda yb, ib: L.check(L.lib.rvc_op_pad2d(None, xd.ptr, ldx, C_, H, W, yb.ptr if yb else None, ib.ptr if ib else None, ldy)), pidx)
    want = R.pad2d(x).reshape(C_, -1)
    assert np.array_equal(y, want)
    for i in (im, im1):
        check_image(i, want, "pad2d image")
        assert np.all(i.reshape(C_, H, Wp)[:, :, [0, -1]] == 0)

    # unpad2d: padded (side columns NaN: they must not be read) -> plain; exact
    xpad = np.concatenate([nan_cols, x, nan_cols], 2).reshape(C_, -1)
    xpd = Buf(grid(C_, H * Wp, ldy), xpad)
    out = Buf(grid(C_, H * W, ldx), tail=4096)
    L.check(L.lib.rvc_op_unpad2d(None, xpd.ptr, ldy, C_, H, W, out.ptr, ldx))
    assert np.array_equal(out.get(), x.reshape(C_, -1))

    # pool2_pad from plain and from padded input (side columns NaN)
    Ho, Wo = H // 2, W // 2
    ldo = Ho * (Wo + 2) + 3
    ref, mag = R.pool2_pad(x)
    ref, mag = ref.reshape(C_, -1), mag.reshape(C_, -1)
    for padded, src, lds in ((0, xd, ldx), (1, xpd, ldy)):
        y, im, im1 = _three(lambda yb, ib: L.check(L.lib.rvc_op_pool2_pad(None, src.ptr, lds, padded, C_, H, W, yb.ptr if yb else None, ib.ptr if ib else None, ldo)),
                            grid(C_, Ho * (Wo + 2), ldo))
        check_terms(y, ref, mag, f"pool2_pad[padded{padded}]")
        assert np.all(y.reshape(C_, Ho, Wo + 2)[:, :, [0, -1]] == 0)
        for i in (im, im1):
            check_image(i, y, "pool2_pad image")
            assert np.all(i.reshape(C_, Ho, Wo + 2)[:, :, [0, -1]] == 0)

    # interleave2_pad: ph [4 C][H][W + 2] (side columns NaN) -> level 2 H x 2 W, padded or plain fp32, padded image
    ph = g.standard_normal((4 * C_, H, W)).astype(np.float32)
    nan4 = np.full((4 * C_, H, 1), np.nan, np.float32)
    ldp = H * Wp + 1
    pd = Buf(grid(4 * C_, H * Wp, ldp), np.concatenate([nan4, ph, nan4], 2).reshape(4 * C_, -1))
    want = R.interleave2(ph, C_)
    wantp = R.pad2d(want).reshape(C_, -1)
    P2 = 2 * H * (2 * W + 2)
    ld2 = P2 + 7
    y, im, im1 = _three(lambda yb, ib: L.check(L.lib.rvc_op_interleave2_pad(None, pd.ptr, ldp, C_, H, W, yb.ptr if yb else None, 1, ib.ptr if ib else None, ld2)),
                        grid(C_, P2, ld2))
    assert np.array_equal(y, wantp)
    for i in (im, im1):
        check_image(i, wantp, "interleave2_pad image")
        assert np.all(i.reshape(C_, 2 * H, 2 * W + 2)[:, :, [0, -1]] == 0)
    # plain fp32 output (pitch of its own), alone and beside the (padded) image
    for with_img in (False, True):
        yb, ib = Buf(grid(C_, 4 * H * W, ld2), tail=4096), (Buf(grid(C_, P2, ld2), tail=4096) if with_img else None)
        L.check(L.lib.rvc_op_interleave2_pad(None, pd.ptr, ldp, C_, H, W, yb.ptr, 0, ib.ptr if ib else None, ld2))
        assert np.array_equal(yb.get(), want.reshape(C_, -1))
        if ib:
            check_image(ib.get(), wantp, "interleave2_pad image beside plain fp32")


# ------------------------------------------------------------------------------------------------ gru_scan
@pytest.fixture(scope="module")
def gru_weights():
    g = torch.Generator().manual_seed(77)
    u = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) / 16).numpy()          # nn.GRU's own initialisation: uniform in +-1 / sqrt(hidden)
    return {"b_ih": u(2, 768), "b_hh": u(2, 768), "w_hh": u(2, 768, 256)}


@pytest.mark.parametrize("scale", [1, 20])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 33, 257])
def test_gru_scan(L, gru_weights, T, scale):
    W = gru_weights
    gi = (np.random.default_rng(T).standard_normal((T, 1536)) * scale).astype(np.float32)      # x 20: all three gates saturate
    ref = R.gru_scan(gi, W["b_ih"], W["w_hh"], W["b_hh"])
    # torch's float32 GRU on the same numbers: input = gi itself through one-hot input weights (a product with 1 and sums with 0 are exact)
    gru = torch.nn.GRU(1536, 256, bidirectional=True)
    eye = torch.eye(768)
    with torch.no_grad():
        for sfx, d in (("", 0), ("_reverse", 1)):
            wih = torch.zeros(768, 1536)
            wih[:, d * 768:(d + 1) * 768] = eye
            getattr(gru, "weight_ih_l0" + sfx).copy_(wih)
            getattr(gru, "weight_hh_l0" + sfx).copy_(torch.from_numpy(W["w_hh"][d]))
            getattr(gru, "bias_ih_l0" + sfx).copy_(torch.from_numpy(W["b_ih"][d]))
            getattr(gru, "bias_hh_l0" + sfx).copy_(torch.from_numpy(W["b_hh"][d]))
        f32 = gru(torch.from_numpy(gi)[:, None])[0][:, 0].T.numpy()
    gd = Buf(grid(T, 1536, 1536), gi)
    bi, bh, wh = Buf(np.arange(1536), W["b_ih"].ravel()), Buf(np.arange(1536), W["b_hh"].ravel()), Buf(np.arange(2 * 768 * 256), W["w_hh"].ravel())
    out = Buf(grid(512, T, T), tail=1024)
    err = C.c_int(-1)
    L.check(L.lib.rvc_op_gru_scan(None, gd.ptr, bi.ptr, wh.ptr, bh.ptr, out.ptr, T, C.byref(err)))
    assert err.value == 0, "the scan's hand-off timed out"
    check_8x(f"gru_scan[T{T} x{scale}]", out.get(), ref, f32)


# ------------------------------------------------------------------------------------------------ rmvpe_decode, f0_post, postprocess (public ABI)
@pytest.fixture(scope="module")
def rmvpe_handle(L):
    h = C.c_void_p()
    L.check(L.lib.rvc_rmvpe_create(L.get_ctx(0), C.byref(h)))
    yield h
    L.lib.rvc_rmvpe_destroy(h)


PLANTED = (0, 1, 3, 4, 355, 356, 358, 359)
THRED = 0.03


def _salience(n, rot):
    """frame t is of kind (t + rot) % 11: a maximum planted at one of the edge bins, an exact tie, a maximum equal to the threshold, all zeros"""
    g = np.random.default_rng(n * 13 + rot)
    sal = g.uniform(0, 0.2, (n, 360)).astype(np.float32)
    kinds = (np.arange(n) + rot) % 11
    for t, kd in enumerate(kinds):
        if kd < 8:
            sal[t, PLANTED[kd]] = 0.9
        elif kd == 8:
            sal[t, 50] = sal[t, 200] = 0.95
        elif kd == 9:
            sal[t] = np.minimum(sal[t], np.float32(THRED))
            sal[t, 100] = np.float32(THRED)
        else:
            sal[t] = 0
    return sal, kinds


@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_rmvpe_decode(L, rmvpe_handle, n):
    for rot in (range(11) if n == 1 else (0,)):
        sal, kinds = _salience(n, rot)
        sd, out = Buf(grid(n, 360, 360), sal), Buf(np.arange(n), dtype=np.float64)
        L.check(L.lib.rvc_rmvpe_decode(rmvpe_handle, None, sd.ptr, n, THRED, out.ptr))
        torch.cuda.synchronize()
        f0, ref = out.get(), R.rmvpe_decode(sal, THRED)
        assert np.all(np.isfinite(f0))
        assert np.all(f0[kinds >= 9] == 0) and np.all(ref[kinds >= 9] == 0)          # maximum == thred, all-zero frame: 0, not NaN
        np.testing.assert_allclose(f0, ref, rtol=1e-12, atol=0)
        tie = kinds == 8                                                              # first of two equal maxima wins: the window is around bin 50
        assert np.all(np.abs(1200 * np.log2(f0[tie] / 10) - (20 * 50 + 1997.3794084376191)) < 80)


F0_SPECIAL = (0.0, 30.0, 49.9, 50.0, 1100.0, 1101.0, 5000.0)
MEL_MIN, MEL_MAX = 2595 * np.log10(1 + 50 / 700), 2595 * np.log10(1 + 1100 / 700)
F0_SEED = 2024          # chosen on the CPU: no mel position of any case within 1e-9 of a half-integer (asserted below)


@pytest.mark.parametrize("factor", [1.0, 2 ** (5 / 12), 0.5])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_f0_post(L, n, factor):
    g = np.random.default_rng(F0_SEED + n)
    if n == 1:
        sets = [np.array([v]) for v in F0_SPECIAL]
    else:
        f0 = g.uniform(40, 1300, n)
        f0[:len(F0_SPECIAL)] = F0_SPECIAL
        f0[10::9] = 0.0
        sets = [f0]
    for f0 in sets:
        m = R.f0_mel(f0, factor, MEL_MIN, MEL_MAX, 256)
        assert np.all(np.abs(m - np.floor(m) - 0.5) > 1e-9), "a mel position at a half-integer: pick another F0_SEED"
        fd = Buf(np.arange(f0.size), f0, dtype=np.float64)
        pitch, pitchf = Buf(np.arange(f0.size), dtype=np.int64), Buf(np.arange(f0.size), dtype=np.float32)
        L.check(L.lib.rvc_f0_post(None, fd.ptr, f0.size, factor, MEL_MIN, MEL_MAX, 256, pitch.ptr, pitchf.ptr))
        torch.cuda.synchronize()
        want_pitch, want_pitchf = R.f0_post(f0, factor, MEL_MIN, MEL_MAX, 256)
        assert np.array_equal(pitchf.get().view(np.uint32), want_pitchf.view(np.uint32))
        assert np.array_equal(pitch.get(), want_pitch)


@pytest.mark.parametrize("N", [1, 7999, 8000, 8001, 40000])
def test_postprocess(L, N):
    sr2 = 16000
    g = np.random.default_rng(N)
    x = (g.standard_normal(N) * np.linspace(0.05, 0.4, N)).astype(np.float32)
    n1 = N // (sr2 // 2) + 1 + 2                                     # two frames more than the output's own envelope has
    rms1 = g.uniform(0.02, 0.3, n1)
    for rate in (1.0, 0.25, 0.0):
        for env in (None, rms1):
            xd = Buf(np.arange(N), x)
            rd = Buf(np.arange(n1), env, dtype=np.float64) if env is not None else None
            out = Buf(np.arange(N), dtype=np.int16)
            L.check(L.lib.rvc_postprocess(None, xd.ptr, N, rd.ptr if rd else None, n1 if rd else 0, sr2, rate, out.ptr))
            torch.cuda.synchronize()
            xd.get()
            d = np.abs(out.get().astype(np.int64) - R.postprocess(x, env, sr2, rate))
            assert d.max() <= 1, f"postprocess[N{N} rate{rate} env{env is not None}]: {int((d > 1).sum())} samples beyond 1 LSB (max {int(d.max())})"
    for env, rate in ((None, 1.0), (rms1, 0.25)):                   # an all-zero input stays all zeros
        zd, out = Buf(np.arange(N), np.zeros(N, np.float32)), Buf(np.arange(N), dtype=np.int16)
        rd = Buf(np.arange(n1), env, dtype=np.float64) if env is not None else None
        L.check(L.lib.rvc_postprocess(None, zd.ptr, N, rd.ptr if rd else None, n1 if rd else 0, sr2, rate, out.ptr))
        torch.cuda.synchronize()
        assert np.all(out.get() == 0)
