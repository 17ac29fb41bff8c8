"""CPU: the float64 restatement of the generator-side losses (tests/gen_cotangent_ref.py) against the reference's float64 autograd gradients, the LossBalancer
port against the reference's recorded trajectories, and the refusals of train_step.generator_loss_cotangents.  Golden: tools/gen_golden_gen_cotangent.py."""
import json

import numpy as np
import pytest
import torch

from conftest import golden
import aux_loss_ref as R
import gen_cotangent_ref as G

AUX = {40: dict(sr=40000, n_fft=2048, hop=400, n_mels=125), 32: dict(sr=32000, n_fft=1024, hop=320, n_mels=80)}
MSML = {"msml_l1": dict(loss="l1", log_weight=1.0, mag_weight=0.0), "msml_sl1": dict(loss="smoothl1", log_weight=1.0, mag_weight=0.5)}
N_TRAJ = 5


def case(g, r):
    sr, B, T, seed = (int(v) for v in g[f"c{r}_meta"])
    wave, gen = R.wave_pair(sr, B, T, seed)
    return sr, wave, gen


def peak_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("r", [40, 32])
def test_restatement_gradients_match_the_reference_float64(r):
    g = golden("gen_cotangent_cases.npz")
    sr, wave, gen = case(g, r)
    a = AUX[r]
    y_hat = torch.from_numpy(gen).double().requires_grad_(True)
    got = {"mel": torch.autograd.grad(G.mel_l1(g[f"c{r}_y_mel"], y_hat, a["n_fft"], a["n_mels"], sr, a["hop"], 0.0, None), y_hat)[0]}
    for name, kw in MSML.items():
        got[name] = torch.autograd.grad(G.multiscale(y_hat, torch.from_numpy(wave).double(), sr, **kw), y_hat)[0]
    for name, grad in got.items():
        want = g[f"c{r}_{name}_grad64"][:, 0]
        e = peak_err(grad.numpy(), want)
        print(r, name, "restatement against the reference's float64 gradient, of the peak:", e)
        assert e <= 1e-9, (r, name, e)
        assert abs(G.balancer_norm(grad) - float(g[f"c{r}_{name}_norm64"])) <= 1e-9 * float(g[f"c{r}_{name}_norm64"])


def test_restatement_kl_gradients_match_the_reference_float64():
    g, t = golden("gen_cotangent_cases.npz"), golden("train_forward_40k_v2.npz")
    got = G.kl_grads(t["z_p"], t["logs_q"], t["m_p"], t["logs_p"], t["y_mask"])
    for name in ("z_p", "logs_q", "logs_p"):
        assert peak_err(got[name].numpy()[:, g["kl_channels"]], g["kl_" + name]) <= 1e-9, name
    assert torch.equal(got["m_p"], -got["z_p"])
    dead = np.broadcast_to(t["y_mask"] == 0, t["z_p"].shape)
    assert dead.any() and all(float(np.abs(v.numpy()[dead]).max()) == 0.0 for v in got.values())


def replay(g, i):
    """the port fed trajectory i's losses and norms: (weights after every batch, moving averages, balanced losses, the balancer)"""
    from comfy_rvc_amd.lib.train.losses import LossBalancer
    keys = [str(k) for k in g["keys"]]
    cfg = json.loads(str(g[f"traj{i}_settings"]))
    bal = LossBalancer(None, initial_weights=dict(zip(keys, (float(v) for v in g["initial_weights"]))), historical_losses={}, ema_weights={}, **cfg)
    weights, hist, balanced = [], [], []
    for row, norms in zip(g[f"traj{i}_losses"], g[f"traj{i}_norms"]):
        losses = {k: (torch.tensor(np.float32(v)) if v != 0 else 0) for k, v in zip(keys, row)}
        out = bal.on_train_batch_start(losses, grad_norms={k: float(n) for k, n in zip(keys, norms) if not np.isnan(n)})
        weights.append([float(bal.ema_weights.get(k, np.nan)) for k in keys])
        hist.append([float(bal.historical_losses.get(k, np.nan)) for k in keys])
        balanced.append(float(out))
    return np.array(weights), np.array(hist), np.array(balanced), bal


@pytest.mark.parametrize("i", range(N_TRAJ))
def test_balancer_reproduces_the_reference_trajectory(i):
    g = golden("gen_cotangent_cases.npz")
    weights, hist, balanced, bal = replay(g, i)
    for name, got in (("weights", weights), ("hist", hist), ("balanced", balanced)):
        want = g[f"traj{i}_{name}"]
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        ok = ~np.isnan(want)
        rel = float(np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok])))
        print("trajectory", i, name, "largest relative difference", rel)
        assert rel <= 1e-12, (i, name, rel)
    cfg = json.loads(str(g[f"traj{i}_settings"]))
    if cfg["active"]:
        assert set(bal.last_weights) == {"loss_gen", "loss_fm", "loss_mel", "loss_kl"}
        assert all(bal.last_weights[k] == float(bal.ema_weights[k]) for k in bal.last_weights)
    else:
        assert bal.last_weights["loss_mel"] == 45.0 and bal.last_weights["loss_kl"] == 1.0


def test_balancer_state_round_trips_through_the_constructor():
    from comfy_rvc_amd.lib.train.losses import LossBalancer
    g = golden("gen_cotangent_cases.npz")
    _, _, _, bal = replay(g, 0)
    state = bal.to_dict()
    assert set(state) == {"epsilon", "weights_decay", "loss_decay", "ema_weights", "initial_weights", "historical_losses", "active", "use_pareto", "use_norm"}
    again = LossBalancer(None, **state)
    assert again.to_dict() == state
    assert again.weighted_ema_loss == bal.weighted_ema_loss > 0
    losses = {"loss_gen": torch.tensor(2.0), "loss_fm": torch.tensor(6.0), "loss_mel": torch.tensor(0.8), "loss_kl": torch.tensor(1.5), "tsi_loss": 0}
    twin = LossBalancer(None, **json.loads(json.dumps({k: ({a: float(b) for a, b in v.items()} if isinstance(v, dict) else v) for k, v in state.items()})))
    assert float(again.on_train_batch_start(dict(losses))) == float(twin.on_train_batch_start(dict(losses)))
    again.on_epoch_end(weights_decay=0.9)
    assert again.weights_decay == 0.9


def test_balancer_skip_rules():
    from comfy_rvc_amd.lib.train.losses import LossBalancer
    bal = LossBalancer(None, initial_weights=dict(a=1., b=0., c=3., d=2.), historical_losses={}, ema_weights={}, use_pareto=False)
    out = bal.on_train_batch_start(dict(a=torch.tensor(1.0), b=torch.tensor(5.0), c=torch.tensor(0.0), d=2.0))
    assert set(bal.last_weights) == {"a"} and bal.last_weights["a"] == 1.0 and float(out) == 1.0       # weight 0, loss 0 and a non-tensor are skipped
    assert LossBalancer(None).on_train_batch_start({}) == 0.
    empty = LossBalancer(None, initial_weights=dict(a=0.), historical_losses={}, ema_weights={})
    assert float(empty.on_train_batch_start(dict(a=torch.tensor(1.0)))) == 0.0 and empty.last_weights == {}


@pytest.mark.parametrize("name", ["c_hd", "c_tsi", "c_tefs"])
def test_auxiliary_terms_are_refused(name):
    from comfy_rvc_amd.lib.train.losses import LossBalancer
    from comfy_rvc_amd.lib.train.train_step import generator_loss_cotangents
    from comfy_rvc_amd.lib.train.utils import HParams
    hps = HParams(train={name: 0.5}, data={})
    with pytest.raises(NotImplementedError, match=name):
        generator_loss_cotangents(None, LossBalancer(None), None, None, None, None, None, hps)
