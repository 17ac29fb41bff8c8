"""The five bf16x3 gather GEMMs of the trainer (csrc/conv_x3gather_dev.h: conv_x3d, conv_x3d_bwd, conv_x3d_wgrad, conv_gen_bwd, conv_gen_wgrad) at the smallest
shapes at which each of their template instantiations and edge paths runs: the case tables, float64 references written as torch autograd of the FORWARD
operation, and the emulation of the kernels' product (operands split into bf16 hi / lo with round-to-nearest-even as split2 does, the products hi hi + hi lo +
lo hi summed in float64; the two-term variant drops lo hi) that calibrates the gate.  Shared by tests/test_gather_gemms_host.py (no GPU) and
tests/test_hip_gather_gemms.py.

Every kernel is a bilinear `gemm(a, b)` of two fp32 operands followed by an element-wise `epilogue`; `reference` is the autograd statement of the whole
operation and the host test checks reference == epilogue(gemm(a, b)) in float64 before the emulation is trusted."""
import numpy as np
import torch
import torch.nn.functional as F

GATE = 2e-5            # test_conv1d_bf16x3's gate: the three-term product measures 4e-6 .. 5e-6, a product that lost a cross term 1e-3 .. 2e-3
F64 = torch.float64


def rel_err(a, b):
    """conftest.rel_err on tensors: max |a - b| / max |b|"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def split_bf16(x):
    """split2: hi = bf16(x), lo = bf16(x - hi), both round-to-nearest-even, the difference formed in float32; returned as float64"""
    assert x.dtype == torch.float32
    hi = x.to(torch.bfloat16).to(torch.float32)
    lo = (x - hi).to(torch.bfloat16).to(torch.float32)
    return hi.double(), lo.double()


def split_bf16_lo_truncated(x):
    """a split2 whose lo is cut off instead of rounded"""
    hi = x.to(torch.bfloat16).to(torch.float32)
    lo = ((x - hi).view(torch.int32) & -65536).view(torch.float32)
    return hi.double(), lo.double()


def worst_lo(t):
    """Every value of t moved to sign(t) 2^e (1 + 2^-9 + 127 2^-23), e = its exponent kept within [-3, 1]: hi = 2^e exactly, and lo = 2^(e - 9) (1 + 127 2^-14) lies
    just below the bf16 value 2^(e - 9) (1 + 2^-7), so rounding lo costs 2^-23 of the value and cutting it off costs 127 2^-23 = 1.5e-5, with the sign of the
    value.  With both operands of a product in this form the cut-off product lacks 3.0e-5 of EVERY term - no cancellation - beside the 2^-18 = 3.8e-6 of the
    lo lo term that the three-term product leaves out by design."""
    e = torch.floor(torch.log2(t.abs().double().clamp_min(1e-30))).clamp(-3, 1)
    v = torch.where(t < 0, -1.0, 1.0).double() * torch.exp2(e) * (1 + 2.0 ** -9 + 127 * 2.0 ** -23)
    out = v.float()
    assert torch.equal(out.double(), v)
    return out


def emulate(gemm, a, b, terms=3, split=split_bf16):
    """the kernels' product of fp32 operands a, b: a_hi b_lo + a_lo b_hi + a_hi b_hi in float64 (terms = 2: without a_lo b_hi)"""
    ah, al = split(a)
    bh, bl = split(b)
    g = gemm(ah, bl) + gemm(ah, bh)
    return g + gemm(al, bh) if terms == 3 else g


def _rows(names, rows):
    out = []
    for r in rows:
        assert len(r) == len(names), r
        out.append(dict(zip(names, r)))
    return out


def conv_out(H, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _mask(a, pos, neg):
    """float64 `pos` where a > 0, `neg` elsewhere (at 0 too)"""
    return torch.where(a > 0, torch.tensor(pos, dtype=F64), torch.tensor(neg, dtype=F64))


def _with_zeros(a):
    a.view(-1)[::7] = 0.0            # exact zeros in the recorded pre-activation: the derivative there is the slope, as in F.leaky_relu
    return a


# ---------------------------------------------------------------------------------------------------------------- conv_x3d_kernel<U>: rvc_op_disc_conv
# units = (Ci / 16) k, U the largest of 4, 2, 1 dividing them, stages = units / U (1: the loop never takes its `more` branch).  N = Hout p columns in tiles of 64.
DISC_CONV = _rows(
    ("S", "Ci", "Co", "H", "p", "k", "stride", "pad", "slope", "units", "stages"),
    [(1, 16, 128, 7, 3, 5, 3, 2, 0.1, 1, 5),        # N = 9 < 64
     (3, 48, 128, 34, 2, 3, 1, 0, 1.0, 1, 9),       # N = 64 exactly, no activation
     (1, 32, 256, 65, 1, 5, 1, 2, 0.1, 2, 5),       # N = 65: a second tile of one column; two row tiles
     (1, 16, 128, 2, 37, 2, 1, 0, 0.1, 2, 1),       # single stage of two units
     (1, 128, 128, 170, 3, 5, 4, 2, 0.1, 4, 10),    # stride 4, N = 43 * 3 = 129: three tiles
     (3, 32, 128, 1, 37, 5, 3, 2, 0.1, 2, 5),       # H = 1 with pad 2: every tap but the centre is out of range
     (1, 16, 128, 32, 2, 1, 1, 0, 0.1, 1, 1),       # single stage, one unit
     (1, 32, 128, 10, 1, 1, 3, 0, 1.0, 2, 1),       # single stage, stride 3
     (3, 64, 256, 43, 3, 1, 1, 0, 0.1, 4, 1)])      # single stage of four units, N = 129


class DiscConv:
    name, table = "disc_conv", DISC_CONV

    @staticmethod
    def label(c):
        return "S{S}_Ci{Ci}_Co{Co}_H{H}_p{p}_k{k}_s{stride}_pad{pad}".format(**c)

    @staticmethod
    def inputs(c, seed):
        g = _gen(seed)
        return {"x": torch.randn(c["S"], c["Ci"], c["H"], c["p"], generator=g), "w": torch.randn(c["Co"], c["Ci"], c["k"], generator=g) / np.sqrt(c["Ci"] * c["k"]),
                "bias": torch.randn(c["Co"], generator=g) * 0.1}

    @staticmethod
    def operands(c, i):
        return i["w"], i["x"]

    @staticmethod
    def gemm(c, w, x):
        return F.conv2d(x, w[..., None], None, stride=(c["stride"], 1), padding=(c["pad"], 0))

    @staticmethod
    def epilogue(c, g, i):
        return F.leaky_relu(g + i["bias"].double()[None, :, None, None], c["slope"])

    @staticmethod
    def reference(c, i):
        return F.leaky_relu(F.conv2d(i["x"].double(), i["w"].double()[..., None], i["bias"].double(), stride=(c["stride"], 1), padding=(c["pad"], 0)), c["slope"])


# ---------------------------------------------------------------------------------------------------------------- conv_x3d_bwd_kernel<U>: rvc_op_disc_conv_input_grad
# k = 5, pad = 2.  Stride 1: one product of 5 taps, units = 5 Co / 16.  Stride 3: phases of 1, 2, 2 taps, U = the smallest over the phases, so phase 0 of every
# stride-3 case is a single-stage launch (stages: the fewest of any phase with rows).  R = Ci rows on 128-row tiles.
DISC_BWD = _rows(
    ("S", "Ci", "Co", "H", "p", "stride", "cot", "slope", "units", "stages"),
    [(1, 1, 16, 1, 37, 3, False, 0.1, 1, 1),        # one row (the row < R guard), H = 1: phases 1 and 2 have no rows
     (3, 20, 32, 2, 3, 3, True, 0.1, 2, 1),         # H = 2: phase 2 without rows
     (1, 32, 64, 3, 1, 3, True, 0.1, 4, 1),         # one row per phase
     (1, 128, 16, 4, 3, 1, True, 0.1, 1, 5),        # a full row tile
     (1, 160, 32, 7, 37, 1, False, 0.1, 2, 5),      # two row tiles, the second ragged; 259 columns
     (3, 160, 64, 65, 1, 3, True, 0.1, 4, 1),       # H = 64 / p + 1: phases of 22, 22, 21 rows
     (1, 20, 64, 22, 3, 1, False, 0.1, 4, 5)])      # H = 64 / p + 1: 66 columns, a second tile of two


class DiscBwd:
    name, table = "disc_conv_input_grad", DISC_BWD

    @staticmethod
    def label(c):
        return "S{S}_Ci{Ci}_Co{Co}_H{H}_p{p}_s{stride}_cot{cot:d}".format(**c)

    @staticmethod
    def hd(c):
        return conv_out(c["H"], 5, c["stride"], 2)

    @staticmethod
    def inputs(c, seed):
        g = _gen(seed)
        shape = (c["S"], c["Ci"], c["H"], c["p"])
        return {"d": torch.randn(c["S"], c["Co"], DiscBwd.hd(c), c["p"], generator=g), "w": torch.randn(c["Co"], c["Ci"], 5, generator=g) / np.sqrt(c["Co"] * 5),
                "cot": torch.randn(*shape, generator=g) if c["cot"] else None, "a": _with_zeros(torch.randn(*shape, generator=g))}

    @staticmethod
    def operands(c, i):
        return i["w"], i["d"]

    @staticmethod
    def gemm(c, w, d):
        x0 = torch.zeros(c["S"], c["Ci"], c["H"], c["p"], dtype=F64, requires_grad=True)
        y = F.conv2d(x0, w[..., None], None, stride=(c["stride"], 1), padding=(2, 0))
        return torch.autograd.grad(y, x0, d)[0]

    @staticmethod
    def epilogue(c, g, i):
        if i["cot"] is not None:
            g = g + i["cot"].double()
        return g * _mask(i["a"], 1.0, c["slope"])

    @staticmethod
    def reference(c, i):
        """d / d pre of <conv(lrelu(pre)), d> + <lrelu(pre), cot> at pre = a"""
        pre = i["a"].double().requires_grad_(True)
        h = F.leaky_relu(pre, c["slope"])
        loss = (F.conv2d(h, i["w"].double()[..., None], None, stride=(c["stride"], 1), padding=(2, 0)) * i["d"].double()).sum()
        if i["cot"] is not None:
            loss = loss + (h * i["cot"].double()).sum()
        return torch.autograd.grad(loss, pre)[0]


# ---------------------------------------------------------------------------------------------------------------- conv_x3d_wgrad_kernel: rvc_op_disc_conv_weight_grad
# Ci k weight columns in tiles of 64; stages of one signal and 128 outputs, lane l holding outputs 2 l, 2 l + 1 (an odd N: the last pair straddles N; p = 1 and
# p = 3: the second output of a pair wraps to column 0 of the next row).  splits / per: the planner's cut of the S ceil(N / 128) stages.
DISC_WGRAD = _rows(
    ("S", "Ci", "Co", "H", "p", "k", "stride", "pad", "splits", "per", "adv"),
    [(1, 1, 128, 1, 1, 5, 1, 2, 1, 1, 0),            # N = 1, 5 columns, one split of one stage
     (2, 13, 128, 380, 1, 5, 3, 2, 2, 1, 0),         # N = 127, 65 columns (a ragged second tile), p = 1 with stride 3: every pair wraps
     (1, 32, 256, 64, 2, 5, 1, 2, 1, 1, 0),          # N = 128, 160 columns, two row tiles
     (3, 13, 128, 128, 3, 5, 3, 2, 6, 1, 0),         # N = 129: a second stage of one output per signal; p = 3 with stride 3
     (71, 1, 128, 5, 2, 5, 1, 2, 36, 2, 0),          # 71 stages in 36 splits of 2, the last holding a single stage
     (33, 1, 128, 43, 3, 5, 1, 2, 33, 2, 0),         # N = 129: 66 stages in 33 splits, each the full and the one-output stage of one signal
     (2, 13, 128, 43, 3, 5, 1, 2, 4, 1, 1)])         # adv: operands whose lo is hardest to round (worst_lo): a split2 that truncates lo misses the gate here


class DiscWgrad:
    name, table = "disc_conv_weight_grad", DISC_WGRAD

    @staticmethod
    def label(c):
        return "S{S}_Ci{Ci}_Co{Co}_H{H}_p{p}_k{k}_s{stride}".format(**c) + ("_adv" if c["adv"] else "")

    @staticmethod
    def inputs(c, seed):
        g = _gen(seed)
        ho = conv_out(c["H"], c["k"], c["stride"], c["pad"])
        f = worst_lo if c["adv"] else (lambda t: t)
        return {"d": f(torch.randn(c["S"], c["Co"], ho, c["p"], generator=g)), "x": f(torch.randn(c["S"], c["Ci"], c["H"], c["p"], generator=g))}

    @staticmethod
    def operands(c, i):
        return i["d"], i["x"]

    @staticmethod
    def gemm(c, d, x):
        w0 = torch.zeros(c["Co"], c["Ci"], c["k"], 1, dtype=F64, requires_grad=True)
        y = F.conv2d(x, w0, None, stride=(c["stride"], 1), padding=(c["pad"], 0))
        return torch.autograd.grad(y, w0, d)[0][..., 0]

    @staticmethod
    def epilogue(c, g, i):
        return g

    @staticmethod
    def reference(c, i):
        return DiscWgrad.gemm(c, i["d"].double(), i["x"].double())


# ---------------------------------------------------------------------------------------------------------------- conv_gen_bwd_kernel<WM, AM, U>: rvc_op_conv1d_input_grad
# t = 0: Conv1d(Ci, Co, k, dilation = step, padding = pad); t = 1: ConvTranspose1d(Ci, Co, k, stride = step, padding = pad).  Rows R = Ci: bm = 32 for R <= 32,
# 128 for R % 128 == 0, 64 otherwise; units = (Co / 16) k.  xd / xy: extra pitch of D / of Y, A and Res.  N: columns of the forward's input.
GEN_BWD = _rows(
    ("t", "Ci", "Co", "k", "step", "pad", "N", "xd", "xy", "A", "Res", "acc", "scale", "slope", "bm", "units", "stages"),
    [(0, 16, 16, 3, 1, 1, 1, 0, 0, True, False, 0, 1.0, 0.1, 32, 1, 3),             # N = 1
     (0, 20, 32, 3, 1, 1, 13, 3, 5, True, True, 1, 1 / 3, 0.1, 32, 2, 3),           # R = 20 on the 32-row tile, both pitches, scale with Res, accumulate
     (0, 32, 64, 7, 3, 9, 129, 0, 0, False, False, 0, 1.0, 0.1, 32, 4, 7),          # 128-column tiles: a second one of one column
     (0, 40, 16, 3, 1, 1, 63, 0, 0, True, True, 0, 1.0, 0.1, 64, 1, 3),             # R = 40 on the 64-row tile
     (1, 64, 16, 4, 2, 1, 64, 0, 0, True, False, 0, 1.0, 0.1, 64, 4, 1),            # ConvTranspose1d(k 4, u 2, pad 1), a single stage of four units
     (0, 192, 32, 3, 1, 1, 65, 0, 7, False, True, 0, 1 / 3, 0.1, 64, 2, 3),         # R = 192: three 64-row tiles
     (0, 128, 16, 3, 1, 1, 127, 2, 0, True, False, 1, 1.0, 0.1, 128, 1, 3),
     (0, 256, 32, 3, 1, 1, 128, 0, 0, True, True, 0, 1.0, 0.1, 128, 2, 3),          # two 128-row tiles
     (1, 128, 64, 16, 10, 3, 13, 2, 3, True, False, 0, 1 / 3, 0.1, 128, 4, 16),     # ConvTranspose1d(k 16, u 10, pad 3)
     (0, 64, 64, 11, 5, 25, 13, 0, 0, True, True, 0, 1.0, 0.1, 64, 4, 11),          # N = 13 is shorter than the halo of 25
     (0, 16, 16, 2, 1, 1, 64, 0, 0, False, False, 0, 1.0, 0.1, 32, 2, 1),           # (16, 2): a single stage of two units
     (0, 32, 16, 1, 1, 0, 65, 0, 0, True, False, 0, 1.0, 0.1, 32, 1, 1),            # k = 1: a single stage of one unit
     (0, 128, 32, 11, 5, 25, 64, 0, 1, True, True, 1, 1.0, 0.1, 128, 2, 11),
     (0, 40, 32, 7, 3, 9, 128, 1, 0, False, False, 0, 1.0, 0.1, 64, 2, 7)])


class GenBwd:
    name, table = "conv1d_input_grad", GEN_BWD

    @staticmethod
    def label(c):
        return "t{t}_Ci{Ci}_Co{Co}_k{k}_step{step}_pad{pad}_N{N}_xd{xd}_xy{xy}_A{A:d}_R{Res:d}_acc{acc}".format(**c)

    @staticmethod
    def td(c):
        return (c["N"] - 1) * c["step"] - 2 * c["pad"] + c["k"] if c["t"] else c["N"] + 2 * c["pad"] - (c["k"] - 1) * c["step"]

    @staticmethod
    def inputs(c, seed):
        g = _gen(seed)
        wshape = (c["Ci"], c["Co"], c["k"]) if c["t"] else (c["Co"], c["Ci"], c["k"])
        shape = (c["Ci"], c["N"])
        return {"d": torch.randn(c["Co"], GenBwd.td(c), generator=g), "w": torch.randn(*wshape, generator=g) / np.sqrt(c["Co"] * c["k"] / (c["step"] if c["t"] else 1)),
                "a": _with_zeros(torch.randn(*shape, generator=g)) if c["A"] else None, "res": torch.randn(*shape, generator=g) if c["Res"] else None,
                "y0": torch.randn(*shape, generator=g) if c["acc"] else None}

    @staticmethod
    def operands(c, i):
        return i["w"], i["d"]

    @staticmethod
    def forward(c, x, w):
        if c["t"]:
            return F.conv_transpose1d(x, w, None, stride=c["step"], padding=c["pad"])
        return F.conv1d(x, w, None, padding=c["pad"], dilation=c["step"])

    @staticmethod
    def gemm(c, w, d):
        x0 = torch.zeros(1, c["Ci"], c["N"], dtype=F64, requires_grad=True)
        return torch.autograd.grad(GenBwd.forward(c, x0, w), x0, d[None])[0][0]

    @staticmethod
    def epilogue(c, g, i):
        g = g * (c["scale"] if i["a"] is None else _mask(i["a"], c["scale"], c["scale"] * c["slope"]))
        if i["res"] is not None:
            g = g + i["res"].double()
        return g + i["y0"].double() if i["y0"] is not None else g

    @staticmethod
    def reference(c, i):
        """d / d pre of <op(scale lrelu(pre)), d> + <pre, res> at pre = a (no a: op(scale pre)), plus the output's previous value where the launch accumulates"""
        pre = (i["a"].double() if i["a"] is not None else torch.zeros(c["Ci"], c["N"], dtype=F64)).requires_grad_(True)
        h = c["scale"] * (F.leaky_relu(pre, c["slope"]) if i["a"] is not None else pre)
        loss = (GenBwd.forward(c, h[None], i["w"].double())[0] * i["d"].double()).sum()
        if i["res"] is not None:
            loss = loss + (pre * i["res"].double()).sum()
        g = torch.autograd.grad(loss, pre)[0]
        return g + i["y0"].double() if i["y0"] is not None else g


# ---------------------------------------------------------------------------------------------------------------- conv_gen_wgrad_kernel<WM, AM>: rvc_conv1d_weight_grad
# test_hip_gen_wgrad.CONV_CASES: (R, C, k, dil, n, B, slope) of a "same" Conv1d(C, R, k, dilation dil), B items.  bm = 128 for R % 128 == 0, 64 for R % 64 == 0,
# 32 otherwise: R = 16 and R = 48 leave the last 32-row tile half empty.
GEN_WGRAD_CONV_CASES = [(32, 32, 11, 5, 1, 1, 0.1), (32, 32, 3, 1, 127, 1, 0.1), (32, 32, 3, 1, 128, 1, 0.1), (32, 32, 3, 1, 129, 1, 0.1), (64, 64, 7, 3, 130, 3, 0.1),
                        (128, 128, 3, 1, 200, 2, 0.1), (256, 256, 11, 5, 130, 2, 0.1), (512, 192, 7, 1, 13, 2, 1.0), (32, 32, 3, 1, 5200, 2, 0.1),
                        (16, 32, 3, 1, 130, 1, 0.1), (48, 32, 3, 1, 130, 2, 0.1)]
GEN_WGRAD = [dict(zip(("R", "C", "k", "dil", "n", "B", "slope"), r), bm=128 if r[0] % 128 == 0 else (64 if r[0] % 64 == 0 else 32)) for r in GEN_WGRAD_CONV_CASES]


class GenWgrad:
    name, table = "conv1d_weight_grad", GEN_WGRAD

    @staticmethod
    def label(c):
        return "R{R}_C{C}_k{k}_d{dil}_n{n}_b{B}".format(**c)

    @staticmethod
    def inputs(c, seed):
        g = _gen(seed)
        return {"d": torch.randn(c["B"], c["R"], c["n"], generator=g), "x": torch.randn(c["B"], c["C"], c["n"], generator=g)}

    @staticmethod
    def operands(c, i):
        return i["d"], torch.maximum(i["x"], i["x"] * np.float32(c["slope"]))       # the kernel applies max(v, slope v) in fp32 before the split

    @staticmethod
    def gemm(c, d, h):
        w0 = torch.zeros(c["R"], c["C"], c["k"], dtype=F64, requires_grad=True)
        y = F.conv1d(h, w0, None, padding=(c["k"] * c["dil"] - c["dil"]) // 2, dilation=c["dil"])
        return torch.autograd.grad(y, w0, d)[0]

    @staticmethod
    def epilogue(c, g, i):
        return g

    @staticmethod
    def reference(c, i):
        return GenWgrad.gemm(c, i["d"].double(), F.leaky_relu(i["x"].double(), c["slope"]))


KINDS = [DiscConv, DiscBwd, DiscWgrad, GenBwd, GenWgrad]
INFO = ("units", "bm", "splits", "gx", "gy", "gz", "stages", "per")


def plan(kind, c, **over):
    """the planner's pure query (no device) for a case, fields overridden by `over`: the info of include/rvc_hip.h as a dict, or None where the planner declines"""
    import ctypes as C
    from comfy_rvc_amd import _lib
    c = dict(c, **over)
    info = (C.c_int * 8)()
    L = _lib.lib
    if kind is DiscConv:
        rc = L.rvc_op_disc_conv_plan(c["S"], c["Ci"], c["Co"], c["H"], c["p"], c["k"], c["stride"], c["pad"], info)
    elif kind is DiscBwd:
        rc = L.rvc_op_disc_conv_input_grad_plan(c["S"], c["Ci"], c["Co"], c["H"], c.get("Hd", DiscBwd.hd(c)), c["p"], c["stride"], info)
    elif kind is DiscWgrad:
        rc = L.rvc_op_disc_conv_weight_grad_plan(c["S"], c["Ci"], c["Co"], c["H"], c["p"], c["k"], c["stride"], c["pad"], info)
    elif kind is GenBwd:
        rc = L.rvc_op_conv1d_input_grad_plan(c["t"], c["Ci"], c["Co"], c["k"], c["step"], c["pad"], c["N"], c.get("Td", GenBwd.td(c)), info)
    else:
        pad = (c["k"] * c["dil"] - c["dil"]) // 2
        rc = L.rvc_conv1d_weight_grad_plan(c["B"], c["R"], c["C"], c["k"], c["n"], c["n"], 1, c["dil"], -pad, info)
    if rc < 0:
        return None
    out = dict(zip(INFO, list(info)))
    assert rc == (out["splits"] if kind in (DiscWgrad, GenWgrad) else out["units"])
    return out


def cases(kind):
    """(case, seed) of a kind's table; the seed is the case's position, so the host calibration and the device test see the same inputs"""
    return [(c, 1000 * (KINDS.index(kind) + 1) + n) for n, c in enumerate(kind.table)]
