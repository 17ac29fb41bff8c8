"""CPU: the case tables of tests/gather_gemm_ref.py against the planners' pure queries (no device), and the calibration of the 2e-5 gate on every case's own
inputs.  (a) each case runs the template instantiation it is labelled with; (b) together the cases run every compiled instantiation of the five bf16x3 gather
GEMMs, a single-stage launch for each U included; (c) on the inputs the device test uses, the kernels' three-term product lies below half the gate and a
product that lost one cross term lies more than ten gates above it, so the gate separates a correct kernel from one that lost an MFMA; (d) the planners
decline what they document."""
import pytest
import torch

import gather_gemm_ref as G

ALL = [(kind, c, seed) for kind in G.KINDS for c, seed in G.cases(kind)]
IDS = [f"{kind.name}-{kind.label(c)}" for kind, c, _ in ALL]


@pytest.mark.parametrize("kind,c,seed", ALL, ids=IDS)
def test_planner_chooses_the_labelled_instantiation(kind, c, seed):
    p = G.plan(kind, c)
    assert p is not None, "the planner declines the case"
    for key in ("units", "bm", "stages", "splits", "per"):
        if key in c:
            assert p[key] == c[key], (key, p, c)
    assert p["gx"] >= 1 and p["gy"] >= 1 and p["gz"] >= 1


def test_cases_cover_every_compiled_instantiation():
    plans = {kind: [G.plan(kind, c) for c in kind.table] for kind in G.KINDS}
    for kind in (G.DiscConv, G.DiscBwd):
        assert {p["units"] for p in plans[kind]} == {1, 2, 4}, kind.name
        assert {p["units"] for p in plans[kind] if p["stages"] == 1} == {1, 2, 4}, (kind.name, "a single-stage launch for each U")
    assert {(p["bm"], p["units"]) for p in plans[G.GenBwd]} == {(bm, u) for bm in (128, 64, 32) for u in (1, 2, 4)}
    assert {p["units"] for p in plans[G.GenBwd] if p["stages"] == 1} == {1, 2, 4}
    assert {p["bm"] for p in plans[G.GenWgrad]} == {128, 64, 32}
    assert {c["R"] for c in G.GEN_WGRAD} >= {16, 48}                     # the last 32-row tile half empty
    w = plans[G.DiscWgrad]
    assert any(c["adv"] for c in G.DISC_WGRAD)
    assert any(p["splits"] == 1 for p in w) and any(p["splits"] > 1 and p["per"] > 1 and p["stages"] % p["per"] == 1 for p in w)      # a last split of one stage
    assert any(p["gx"] > 1 for p in w) and any(p["gy"] > 1 for p in w)
    # more than one tile in every grid dimension of the image kernels, and rows that are no multiple of the tile
    for kind in (G.DiscConv, G.DiscBwd, G.GenBwd):
        assert any(p["gx"] > 1 for p in plans[kind]) and any(p["gy"] > 1 for p in plans[kind]), kind.name
    assert any(p["gz"] > 1 for p in plans[G.DiscConv]) and any(p["gz"] > 1 for p in plans[G.DiscBwd])
    assert any(c["Ci"] % 128 for c in G.DISC_BWD) and any(c["Ci"] % p["bm"] for c, p in zip(G.GEN_BWD, plans[G.GenBwd]))


@pytest.mark.parametrize("kind,c,seed", ALL, ids=IDS)
def test_gate_separates_three_terms_from_two_on_the_cases_own_inputs(kind, c, seed):
    i = kind.inputs(c, seed)
    a, b = kind.operands(c, i)
    with torch.enable_grad():
        want = kind.reference(c, i).detach()
        gemm = lambda u, v: kind.gemm(c, u, v).detach()      # noqa: E731
        exact = kind.epilogue(c, gemm(a.double(), b.double()), i)
        three = kind.epilogue(c, G.emulate(gemm, a, b, 3), i)
        two = kind.epilogue(c, G.emulate(gemm, a, b, 2), i)
    assert tuple(exact.shape) == tuple(want.shape)
    # the autograd statement of the operation and gemm + epilogue are the same map (GenWgrad: but for the fp32 rounding of slope * v)
    assert G.rel_err(exact, want) < (1e-7 if kind is G.GenWgrad else 1e-12)
    e3, e2 = G.rel_err(three, want), G.rel_err(two, want)
    print(kind.name, kind.label(c), "three-term", e3, "two-term", e2)
    assert e3 < G.GATE / 2, e3
    assert e2 > 10 * G.GATE, e2
    if c.get("adv"):      # the inputs built so that a mis-rounded lo shows: a split2 that cuts lo off lies above the gate, by the arithmetic of worst_lo
        cut = G.rel_err(kind.epilogue(c, G.emulate(gemm, a, b, 3, G.split_bf16_lo_truncated), i), want)
        print(kind.name, kind.label(c), "three-term with lo cut off", cut)
        assert 1.5 * G.GATE < cut < 2 * G.GATE, cut


def test_planners_decline_what_they_document():
    c = G.DISC_CONV[0]
    assert G.plan(G.DiscConv, c) is not None
    assert G.plan(G.DiscConv, c, Ci=24) is None                          # Ci % 16
    assert G.plan(G.DiscConv, c, Co=192) is None                         # Co % 128
    assert G.plan(G.DiscConv, c, k=17, H=20) is None and G.plan(G.DiscConv, c, k=16, H=20) is not None      # k > 16
    assert G.plan(G.DiscConv, c, H=1, pad=0) is None                     # no output row
    b = G.DISC_BWD[5]
    assert G.plan(G.DiscBwd, b) is not None
    assert G.plan(G.DiscBwd, b, Co=24) is None                           # Ck % 16
    assert G.plan(G.DiscBwd, b, Hd=G.DiscBwd.hd(b) - 1) is None          # Hj > Hd: a column whose first tap lies below the gradient's rows
    assert G.plan(G.DiscBwd, b, stride=2) is None
    w = G.DISC_WGRAD[1]
    assert G.plan(G.DiscWgrad, w) is not None
    assert G.plan(G.DiscWgrad, w, Co=64) is None and G.plan(G.DiscWgrad, w, k=17) is None
    assert G.plan(G.DiscWgrad, w, Ci=24) is not None                     # any Ci: the columns are Ci k
    g = G.GEN_BWD[1]
    assert G.plan(G.GenBwd, g) is not None
    assert G.plan(G.GenBwd, g, Co=24) is None                            # Ck % 16
    assert G.plan(G.GenBwd, g, k=17, pad=0, N=64) is None and G.plan(G.GenBwd, g, k=16, pad=0, N=64) is not None      # k > 16
    assert G.plan(G.GenBwd, g, pad=3) is None                            # pad beyond the kernel's reach: tap 0 would start right of the column
    assert G.plan(G.GenWgrad, G.GEN_WGRAD[0], R=40) is None              # R % 16
