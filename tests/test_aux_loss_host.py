"""CPU: the restatement of the multi-scale mel loss and the HPSS / TSI losses (tests/aux_loss_ref.py) against the reference's goldens
(tests/golden/aux_loss_cases.npz, tools/gen_golden_aux_losses.py), and the host side of MultiScaleMelSpectrogramLoss.

Gate of the restatement: 4 x the reference's own float32-vs-float64 difference stored with each value (the float64 restatement against the reference's
float32 value differs by exactly that rounding error if the two agree), not below 1e-9 (the stored difference of a single value can be zero by chance)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import aux_loss_ref as R

RATES = (40000, 32000)
AUX = {40000: (125, 2048, 400), 32000: (80, 1024, 320)}
SAVED = dict(mel_fmin=[50.0, 60.0, 55.0, 80.0, 50.0, 120.0], mel_fmax=[20000, 18000.0, 19000.0, 20000, 16000.0, 20000])
F32_EPS = float(torch.finfo(torch.float32).eps)


def case_waves(g, name):
    sr, B, T, seed = (int(v) for v in g[f"{name}_meta"])
    return (sr, *R.wave_pair(sr, B, T, seed))


def msml_keys(g, name):
    return sorted(k for k in g if k.startswith(f"{name}_msml_") and not k.endswith(("_tol", "_d64")))


def msml_args(key, sr):
    """(loss, log_weight, mag_weight, fmin, fmax) of a golden key."""
    tail = key.split("_msml_")[1]
    if tail == "saved":
        return "l1", 1.0, 0.0, SAVED["mel_fmin"], [min(v, sr // 2) for v in SAVED["mel_fmax"]]
    kind, lw, mw = tail.split("_")
    return kind, float(lw), float(mw), 50.0, None


@pytest.mark.parametrize("name", ["A40", "B40", "A32", "B32"])
def test_restatement_matches_the_reference(name):
    g = golden("aux_loss_cases.npz")
    sr, wave, gen = case_waves(g, name)
    for key in msml_keys(g, name):
        kind, lw, mw, fmin, fmax = msml_args(key, sr)
        per, total = R.multiscale(gen.astype(np.float64), wave.astype(np.float64), sr, fmin=fmin, fmax=fmax, loss=kind, log_weight=lw, mag_weight=mw)
        got, gate = np.array(per + [total]), np.maximum(4 * g[key + "_d64"], 1e-9)
        print(key, np.abs(got - g[key]).tolist(), gate.tolist())
        assert np.all(np.abs(got - g[key]) <= gate), key
    if f"{name}_aux" in g:
        n_mels, n_fft, hop = AUX[sr]
        om, gm = R.aux_mags(wave.astype(np.float64), gen.astype(np.float64), n_mels, sr, n_fft, hop, 0.0, None)
        got = np.array([R.harmonic_loss(om, gm, F32_EPS), R.tsi_loss(om, gm, F32_EPS)])
        gate = np.maximum(4 * g[f"{name}_aux_d64"], 1e-9)
        print(name, "aux", np.abs(got - g[f"{name}_aux"]).tolist(), gate.tolist())
        assert np.all(np.abs(got - g[f"{name}_aux"]) <= gate)


def test_harmonics_tensors_match_the_reference():
    g = golden("aux_loss_cases.npz")
    for name, eps in (("B40", F32_EPS), ("B32", F32_EPS), ("H", 1e-8)):
        h, p = R.harmonics(g[f"{name}_mag"], eps, torch.float32)
        assert h.shape == g[f"{name}_harm"].shape == (g[f"{name}_mag"].shape[0], g[f"{name}_mag"].shape[1], 5 * g[f"{name}_mag"].shape[2])
        # float32 against float32: the same operations up to the order of two roundings; values are scaled to [0, 1]
        assert np.abs(h.numpy() - g[f"{name}_harm"]).max() <= 4 * F32_EPS and np.abs(p.numpy() - g[f"{name}_perc"]).max() <= 4 * F32_EPS, name
    assert np.any(g["H_mag"] == 0.0)


def test_median_restatement_against_scipy():
    from scipy.ndimage import median_filter
    g = np.random.default_rng(3)
    for shape in ((2, 20, 32), (1, 125, 15), (1, 15, 45)):
        S = np.abs(g.standard_normal(shape)).astype(np.float32)
        S[0, 2, 3:6] = 0.0
        for k in R.HPSS_SIZES:
            assert np.array_equal(R.median_along(S, k, -1).numpy(), median_filter(S, size=(1, 1, k), mode="reflect")), (shape, k)
            assert np.array_equal(R.median_along(S, k, -2).numpy(), median_filter(S, size=(1, k, 1), mode="reflect")), (shape, k)


def _cls():
    from comfy_rvc_amd.lib.train.losses import MultiScaleMelSpectrogramLoss
    return MultiScaleMelSpectrogramLoss


def test_window_lengths():
    M = _cls()
    for sr in (32000, 40000, 48000):
        assert [M.compute_window_length(m, sr) for m in R.DEFAULT_N_MELS] == [256, 1024, 1024, 2048, 2048, 4096]
        assert [R.window_length(m) for m in R.DEFAULT_N_MELS] == [256, 1024, 1024, 2048, 2048, 4096]
        m = M(sr)
        assert [(s.window_length, s.hop_length) for s in m.stft_params] == [(w, sr // 100) for w in (256, 1024, 1024, 2048, 2048, 4096)]
        assert m.fmax == sr // 2 and m.mel_fmin == [50.0] * 6 and m.frequency_buffer == 1


def test_sorted_n_mels_quirk():
    m = _cls()(40000, n_mels=[256, 20, 128])
    assert m.n_mels == [20, 128, 256] and m.window_lengths == [4096, 256, 2048]           # windows in the order given, n_mels sorted
    assert [s.window_length for s in m.stft_params] == [4096, 256, 2048]


def test_to_dict_round_trip():
    M = _cls()
    m = M(40000, loss="l2", mag_weight=0.5, adjustment_factor=0.01, epsilon=1e-9)
    m.mel_fmin, m.mel_fmax = list(SAVED["mel_fmin"]), list(SAVED["mel_fmax"])
    d = m.to_dict()
    assert sorted(d) == sorted(["sampling_rate", "n_mels", "loss", "epsilon", "mag_weight", "log_weight", "adjustment_factor", "fmin", "fmax", "center",
                                "mel_fmin", "mel_fmax"])
    m2 = M(**d)
    assert m2.to_dict() == d and m2.mel_fmin == SAVED["mel_fmin"] and m2.mel_fmax == SAVED["mel_fmax"] and m2.window_lengths == m.window_lengths
    with pytest.raises(ValueError):
        M(40000, loss="huber")


def test_adjust_fmin_fmax_trajectory():
    g = golden("aux_loss_cases.npz")
    m = _cls()(40000, adjustment_factor=0.05, epsilon=1e-8)
    for row, want in zip(g["adjust_losses"], g["adjust_traj"]):
        with np.errstate(all="ignore"):
            m.adjust_fmin_fmax(row.tolist())
        assert np.array_equal(np.array([m.mel_fmin, m.mel_fmax], dtype=np.float64), want)
    assert not np.array_equal(g["adjust_traj"][0], g["adjust_traj"][-1])


def test_errors_without_a_device():
    from comfy_rvc_amd.lib.train import losses as L
    x = torch.zeros(1, 1, 12800)
    with pytest.raises(NotImplementedError, match="tefs"):
        L.combined_aux_loss(x, x, c_tefs=1.0, c_hd=0.0, c_tsi=0.0)
    with pytest.raises(ValueError):
        L.combined_aux_loss(x, x, c_tefs=0.0)
    with pytest.raises(ValueError):
        _cls()(40000)(x, x)
    with pytest.raises(NotImplementedError):
        _cls()(40000, center=True)(x, x)
    assert L.combined_aux_loss(x, x, c_tefs=0.0, c_hd=0.0, c_tsi=0.0) == (0, 0, 0)


def test_new_entries_follow_the_exported_symbol_rule():
    """The rule of tests/test_abi_symbols.py (declared in include/rvc_hip.h <=> exported <=> has a ctypes signature) with the new entries present."""
    from comfy_rvc_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rvc_hip.h")).read(), flags=re.S)
    for s in ("rvc_spectrogram_batch_ms", "rvc_multiscale_mel_loss", "rvc_hpss", "rvc_hpss_l1", "rvc_tsi_terms"):
        assert re.search(rf"\b{s}\s*\(", hdr) and hasattr(_lib.lib, s) and s in _lib.SIGNATURES, s
    import test_abi_symbols as A
    A.test_library_exports_every_declared_symbol()
    A.test_shared_device_helpers_have_one_definition()
    src = {f: open(os.path.join(A.CSRC, f)).read() for f in os.listdir(A.CSRC) if f.endswith((".hip", ".h"))}
    assert [f for f, t in src.items() if re.search(r"void\s+sorted_insert\s*\(", t)] == ["signal_dev.h"]
    assert [f for f, t in src.items() if re.search(r"long long\s+reflect_index\s*\(", t)] == ["signal_dev.h"]
