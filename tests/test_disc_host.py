"""CPU: the restatement the GPU tests lean on (tests/disc_ref.py) against the reference's goldens (tools/gen_golden_discriminator.py), the procedural
discriminator weights against the reference module's recorded names and shapes, and the weight-norm fold."""
import numpy as np
import torch

from conftest import golden, rel_err
from comfy_rvc_amd import synthetic as S
import disc_ref as R

# float64 restatement against the float32 reference: the reference's own rounding, measured by the generator (disc_meta.npz *_ref_err64, at most 1.6e-6) -
# gated at ten times fp32's 2^-23 per layer over the seven layers of the deepest stack
REF_GATE = 7 * 10 * 2.0 ** -23


def case_a():
    m = golden("disc_meta.npz")
    y, y_hat = S.disc_waves(int(m["A_B"]), int(m["A_T"]), int(m["A_wave_seed"]))
    return m, y, y_hat


def case_b():
    g = golden("disc_B_v2.npz")
    y, y_hat = S.disc_waves(int(g["B"]), int(g["T"]), int(g["wave_seed"]))
    return g, y, y_hat


def check_case_a(res, version, gate, record=None, f32=False):
    """every score and every full feature map of a forward result against disc_A_d<i>.npz (f32: and float32 like the reference's); returns the largest error"""
    worst = 0.0
    for i in range(len(R.PERIODS[version]) + 1):
        g = golden(f"disc_A_d{i}.npz")
        assert len(res[2][i]) == len(res[3][i]) == (7 if i == 0 else 6)
        for k, tag in ((0, "r"), (1, "g")):
            a = res[k][i].detach().cpu().numpy()
            assert a.shape == g[f"score_{tag}"].shape and (a.dtype == np.float32 or not f32)
            errs = {"score": rel_err(a, g[f"score_{tag}"])}
            for l, t in enumerate(res[2 + k][i]):
                t = t.detach().cpu().numpy()
                assert t.shape == g[f"fmap_{tag}_{l}"].shape and (t.dtype == np.float32 or not f32), (i, l, t.shape)
                errs[f"fmap{l}"] = rel_err(t, g[f"fmap_{tag}_{l}"])
            for n, e in errs.items():
                if record:
                    record(f"A.{version}.d{i}.{tag}.{n}", e, gate)
                assert e < gate, (version, i, tag, n, e)
                worst = max(worst, e)
    return worst


def check_case_b(res, g, gate, record=None):
    """full scores, 256 sampled positions and mean |.| of every feature map against disc_B_v2.npz"""
    worst = 0.0
    for i in range(9):
        for k, tag in ((0, "r"), (1, "g")):
            a = res[k][i].detach().cpu().numpy()
            assert a.shape == g[f"score_{tag}_{i}"].shape
            errs = {"score": rel_err(a, g[f"score_{tag}_{i}"])}
            for l, t in enumerate(res[2 + k][i]):
                t = t.detach().cpu().numpy()
                assert list(t.shape) == list(g[f"fmap_{tag}_{i}_{l}_shape"]), (i, l, t.shape)
                pos = R.sample_positions(t.size, int(g["sample_seed"]), f"{tag}.{i}.{l}")
                scale = float(g[f"fmap_{tag}_{i}_{l}_max"])          # the normalisation of rel_err over the full tensor
                errs[f"fmap{l}"] = float(np.max(np.abs(t.reshape(-1)[pos].astype(np.float64) - g[f"fmap_{tag}_{i}_{l}_samples"]))) / scale
                errs[f"meanabs{l}"] = abs(float(np.abs(t.astype(np.float64)).mean()) - float(g[f"fmap_{tag}_{i}_{l}_meanabs"])) / scale
            for n, e in errs.items():
                if record:
                    record(f"B.d{i}.{tag}.{n}", e, gate)
                assert e < gate, (i, tag, n, e)
                worst = max(worst, e)
    return worst


def test_restatement_matches_reference_case_a():
    m, y, y_hat = case_a()
    sd = S.disc_state_dict("v2", int(m["weight_seed"]))
    e2 = check_case_a(R.forward(sd, "v2", y, y_hat), "v2", REF_GATE)
    e1 = check_case_a(R.forward(S.disc_state_dict("v1", int(m["weight_seed"])), "v1", y, y_hat), "v1", REF_GATE)
    print("case A restatement vs reference: v2", e2, "v1", e1, "generator measured", float(m["A_ref_err64"]))
    assert abs(e2 - float(m["A_ref_err64"])) < 1e-7          # the same comparison the generator made


def test_restatement_matches_reference_case_b_and_losses():
    g, y, y_hat = case_b()
    res = R.forward(S.disc_state_dict("v2", int(g["weight_seed"])), "v2", y, y_hat)
    print("case B restatement vs reference:", check_case_b(res, g, REF_GATE))
    mine = R.losses(res)
    for k, v in mine.items():
        print(k, v, "reference", float(g[k]), "tolerance", float(g[k + "_tol"]))
        assert abs(v - float(g[k])) <= float(g[k + "_tol"])
    assert len(R.discriminator_loss(res[0], res[1])[1]) == int(g["n_losses_disc"]) == 9 and len(R.generator_loss(res[1])[1]) == int(g["n_losses_gen"]) == 9


def test_state_dict_names_and_shapes_are_the_reference_modules():
    m = golden("disc_meta.npz")
    for v in ("v1", "v2"):
        sd = S.disc_state_dict(v, 0)
        assert list(sd) == list(m[f"names_{v}"])
        assert [",".join(str(s) for s in t.shape) for t in sd.values()] == list(m[f"shapes_{v}"])
        assert all(t.dtype == np.float32 for t in sd.values())


def test_v1_weights_are_v2s_first_seven():
    a, b = S.disc_state_dict("v1", 3), S.disc_state_dict("v2", 3)
    assert all(np.array_equal(a[k], b[k]) for k in a) and len(b) > len(a)


def test_weight_norm_fold():
    rng = np.random.default_rng(0)
    v, g = rng.standard_normal((6, 4, 5, 1)), rng.uniform(0.5, 2.0, (6, 1, 1, 1))
    w = R.fold_weight_norm(v, g).numpy()
    for r in range(6):
        assert np.allclose(np.linalg.norm(w[r]), g[r, 0, 0, 0], rtol=1e-12)
        assert np.allclose(w[r] / np.linalg.norm(w[r]), v[r] / np.linalg.norm(v[r]), rtol=1e-12)
    # torch's own weight norm on the same tensors
    conv = torch.nn.utils.weight_norm(torch.nn.Conv2d(4, 6, (5, 1)).double())
    conv.weight_v.data, conv.weight_g.data = torch.from_numpy(v), torch.from_numpy(g)
    x = torch.from_numpy(rng.standard_normal((1, 4, 9, 2)))
    want = conv(x)
    got = torch.nn.functional.conv2d(x, torch.from_numpy(w), conv.bias)
    assert torch.allclose(want, got, rtol=1e-12, atol=1e-12)
    # a plain weight passes through `folded` unchanged
    W = R.folded({"l.weight": w.astype(np.float32), "l.bias": np.zeros(6, np.float32)})
    assert torch.equal(W["l"][0], torch.from_numpy(w.astype(np.float32)).double())
