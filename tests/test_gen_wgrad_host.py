"""CPU: pins tests/gen_wgrad_ref.py - the float64 restatement of the decoder's weight and bias gradients, weight norm included - against float64 autograd with
respect to weight_v, weight_g, the biases, the plain weights and m_source.l_linear; the decoder's parameter list against the synthetic state dict's dec.*
entries; and the new entry points' ctypes signatures."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from comfy_rvc_amd import synthetic as S
from oracle import nets
import gen_grad_ref as G
import gen_wgrad_ref as W

SEG, B = 13, 2
BOUND = 1e-9
CONFIGS = {"40k_v2": (S.CONFIG_40K_V2, "v2"), "32k_v1": (S.CONFIG_32K_V1, "v1")}


def make_items(config, gen, f0):
    upp = int(np.prod(config[12]))
    items = []
    for _ in range(B):
        it = {"z": torch.randn(1, config[2], SEG, generator=gen, dtype=torch.float64),
              "g": torch.randn(config[16], generator=gen, dtype=torch.float64) * 0.3,
              "dy": torch.randn(1, 1, SEG * upp, generator=gen, dtype=torch.float64)}
        it["dy"] = it["dy"] / it["dy"].norm()
        if f0:
            it["sine"] = torch.randn(SEG * upp, generator=gen, dtype=torch.float64) * 0.3
        items.append(it)
    return items


@pytest.mark.parametrize("f0", [True, False], ids=["f0", "nono"])
def test_restated_weight_grads_equal_float64_autograd(f0):
    config, version = CONFIGS["40k_v2"]
    sd = S.synth_train_state_dict(config, version, 3, f0=f0)
    dec = {k: torch.from_numpy(np.asarray(v)).double().requires_grad_() for k, v in sd.items() if k.startswith("dec.")}
    items = make_items(config, torch.Generator().manual_seed(21), f0)
    # the graph: weight norm folded inside it (G.weights folds with nets.weight_norm_fold), the source through m_source.l_linear inside it
    w = G.weights(dec, config, f0=f0)
    loss, rec = 0.0, []
    for it in items:
        har = None
        if f0:
            har = torch.tanh(it["sine"] * dec["dec.m_source.l_linear.weight"][0, 0] + dec["dec.m_source.l_linear.bias"][0]).view(1, 1, -1)
        acts = G.forward(w, config, it["z"], har, it["g"].view(1, -1, 1))
        loss = loss + (acts["y_hat"] * it["dy"][0]).sum()
        rec.append({k: v.detach() for k, v in acts.items()})
    names = list(dec)
    want = dict(zip(names, torch.autograd.grad(loss, [dec[n] for n in names])))
    # the restatement: activations of the forward, deltas of the restated VJP, per item
    w0 = {k: v.detach() for k, v in w.items()}
    batch = []
    for it, acts in zip(items, rec):
        with torch.no_grad():
            v = G.vjp(w0, config, acts, it["dy"], f0=f0)
        deltas = {n: t for n, t in v.items() if n.startswith("d.")}
        deltas["d.cond"] = v["dcond"]
        if f0:
            deltas["d.har"] = v["dhar"]
        batch.append({"acts": acts, "deltas": deltas, "g": it["g"], "sine": it.get("sine")})
    got = W.weight_grads({k: v.detach() for k, v in dec.items()}, config, batch, f0=f0)
    assert list(got) == names
    worst = 0.0
    for n in names:
        assert tuple(got[n].shape) == tuple(want[n].shape), n
        e = rel_err(got[n].numpy(), want[n].numpy())
        worst = max(worst, e)
        assert e < BOUND, (n, e)
    print("worst parameter against float64 autograd", worst, "over", len(names), "tensors")


@pytest.mark.parametrize("tag", list(CONFIGS))
@pytest.mark.parametrize("f0", [True, False], ids=["f0", "nono"])
def test_parameter_list_is_the_state_dicts_decoder_in_order(tag, f0):
    from comfy_rvc_amd.lib.infer_pack.models import dec_parameter_spec
    config, version = CONFIGS[tag]
    sd = S.synth_train_state_dict(config, version, 0, f0=f0)
    want = [(k, tuple(v.shape)) for k, v in sd.items() if k.startswith("dec.")]
    assert list(dec_parameter_spec(config, f0=f0).items()) == want
    if tag == "40k_v2" and f0:
        assert len(want) == 243


def test_new_entry_points_have_signatures():
    from comfy_rvc_amd import _lib
    for name in ("rvc_synth_keep_parameters", "rvc_synth_dec_param_count", "rvc_synth_dec_param_info", "rvc_synth_dec_param_total", "rvc_synth_dec_weight_grad",
                 "rvc_synth_dec_weight_grad_launch_count", "rvc_gen_tape_wgrad_times", "rvc_conv1d_weight_grad", "rvc_conv1d_weight_grad_splits"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        assert not name.endswith("_destroy")
