"""CPU: the restatement of the training forward (tests/train_forward_ref.py) against the reference's goldens, the slice-start formula against recorded
torch.rand draws, the posterior's state-dict names, and synth_state_dict untouched by the training twin."""
import numpy as np
import pytest
import torch

from conftest import golden, rel_err
from comfy_rvc_amd import synthetic as S
import train_forward_ref as R

CASES = {"40k_v2": (S.CONFIG_40K_V2, "v2", True), "32k_v1": (S.CONFIG_32K_V1, "v1", True), "40k_v2_nono": (S.CONFIG_40K_V2, "v2", False)}
TAPS = ("z", "z_p", "m_p", "logs_p", "m_q", "logs_q")


def case_inputs(tag):
    """(config, state dict, batch, noise_q, noise_src, golden) of one golden case: weights and inputs regenerated from their seeds, noise replayed."""
    config, version, f0 = CASES[tag]
    g = golden(f"train_forward_{tag}.npz")
    sd = S.synth_train_state_dict(config, version, int(g["weight_seed"]), f0=f0)
    batch = S.synth_train_batch(config, version, [int(x) for x in g["lengths"]], int(g["input_seed"]), f0=f0)
    assert np.array_equal(batch["sid"], g["sid"])
    gen = torch.Generator().manual_seed(int(g["noise_seed"]))
    draws = [torch.randn(tuple(int(v) for v in s), generator=gen) for s in g["draw_shapes"]]
    return config, sd, batch, draws[0], (draws[1] if f0 else None), g


@pytest.mark.parametrize("tag", list(CASES))
def test_restatement_matches_reference(tag):
    config, sd, b, noise_q, noise_src, g = case_inputs(tag)
    out = R.forward(sd, config, b["phone"], b["lengths"], b["pitch"], b["pitchf"], b["spec"], b["sid"], noise_q, noise_src, g["ids_slice"])
    for k in TAPS + ("o",):
        e = rel_err(out[k], g[k])
        print(tag, k, e)
        assert e < 1e-3, (tag, k, e)
    T = int(b["lengths"].max())
    mask = (np.arange(T)[None, :] < b["lengths"][:, None]).astype(np.float32)[:, None, :]
    assert np.array_equal(g["y_mask"], mask) and np.array_equal(g["x_mask"], mask)
    for k in TAPS:      # the reference's tensors are exactly 0 beyond each length
        assert not np.any(g[k] * (1 - mask))


def test_slice_start_formula():
    g = golden("train_forward_40k_v2.npz")
    seg = S.CONFIG_40K_V2[1]
    torch.manual_seed(int(g["slice_seed"]))
    rand = torch.rand([len(g["slice_lengths"])])
    assert np.array_equal(rand.numpy(), g["slice_rand"])
    starts = R.slice_starts(rand, g["slice_lengths"], seg).numpy()
    assert np.array_equal(starts, g["slice_starts"])
    assert np.all(starts >= 0) and np.all(starts <= g["slice_lengths"] - seg)
    assert starts[list(g["slice_lengths"]).index(seg)] == 0      # length == segment: 0 is the only legal start


def test_posterior_spec_names():
    g = golden("train_forward_40k_v2.npz")
    spec = S.synth_posterior_spec(S.CONFIG_40K_V2)
    assert list(spec) == [str(n) for n in g["enc_q_names"]]
    sd = S.synth_train_state_dict(S.CONFIG_40K_V2)
    assert all(sd[n].shape == shape and sd[n].dtype == np.float32 for n, shape in spec.items())
    assert spec["enc_q.pre.weight"] == (192, 1025, 1) and spec["enc_q.enc.cond_layer.bias"] == (2 * 192 * 16,)


def test_synth_state_dict_unchanged_by_training_twin():
    for config, version, f0 in CASES.values():
        base = S.synth_state_dict(config, version, 0, f0=f0)
        train = S.synth_train_state_dict(config, version, 0, f0=f0)
        assert list(train)[:len(base)] == list(base)
        assert all(np.array_equal(train[k], base[k]) for k in base)
        extra = [k for k in train if k not in base]
        assert extra == list(S.synth_posterior_spec(config))
    # pinned values: the draw rules did not move when they were factored out
    sd = S.synth_state_dict(S.CONFIG_40K_V2, "v2", 0)
    assert float(sd["enc_p.proj.weight"][0, 0, 0]) == float(np.float32(S._normal(0, "enc_p.proj.weight", (384, 192, 1), 0.5 / np.sqrt(192))[0, 0, 0]).astype(np.float16))


def test_losses_restatement_matches_reference():
    g, e = golden("train_forward_40k_v2.npz"), golden("train_eval_cases.npz")
    kl = R.kl_loss(g["z_p"], g["logs_q"], g["m_p"], g["logs_p"], g["y_mask"])
    assert abs(kl - float(e["batch_loss_kl"])) <= float(e["loss_kl_tol"])
