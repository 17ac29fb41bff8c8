"""CPU: the host side of the training inputs (lib/train): goldens against a float64 restatement, loaders / collates / samplers against the reference's
results, the mel filterbank's properties, the new ABI symbols.  No device: the loaders read pre-written .spec.pt files."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
from spec_ref import GEOMETRIES, clip_cases, clip_signal, frame_peak_err, spec_f64

from comfy_rvc_amd import synthetic as S
from comfy_rvc_amd.lib.train import data_utils as DU
from comfy_rvc_amd.lib.train import mel_processing as MP
from comfy_rvc_amd.lib.train.utils import HParams, get_hparams_from_file

HP = dict(max_wav_value=32768.0, sampling_rate=40000, filter_length=2048, hop_length=400, win_length=2048)


def test_golden_spectrograms_match_float64_restatement():
    """The yardstick: the reference's torch.stft spectrograms against numpy's float64 rfft of the regenerated signals.  err_ref per case, measured on the
    CPU that wrote the goldens: 1.3e-7 .. 1.8e-7 of the frame's peak."""
    g = golden("spec_cases.npz")
    cases = [k for k in g if not k.endswith("_meta")]
    assert len(cases) == 6
    for case in cases:
        n_fft, hop, sr, n, seed = (int(v) for v in g[f"{case}_meta"])
        gi = [i for i, geo in enumerate(GEOMETRIES) if geo == (n_fft, hop, sr)][0]
        assert (n, seed) == clip_cases(gi)[case.rsplit("_", 1)[1]]
        x = S.spec_test_signal(sr, n, seed)
        assert np.abs(x).max() > 1.05, "the signal must exercise the clamp"
        assert np.array_equal(x, clip_signal(gi, case.rsplit("_", 1)[1]))
        ref = spec_f64(x, n_fft, hop)
        assert g[case].dtype == np.float32 and g[case].shape == (n_fft // 2 + 1, n // hop)
        err_ref = frame_peak_err(g[case], ref)
        print(f"{case}: err_ref {err_ref:.3e}")
        assert err_ref < 1e-6, (case, err_ref)
        unclamped = frame_peak_err(g[case], spec_f64(x, n_fft, hop, clamp=False))
        assert unclamped > 1e-4, "without the clamp the restatement must NOT match: the case would not see a missing clamp"


def test_spec_test_signal_has_silent_frames():
    n_fft, hop, sr = GEOMETRIES[2]
    x = S.spec_test_signal(sr, 3 * S.SPEC_ZERO_RUN, 0)
    z = np.flatnonzero(x == 0)
    assert z.size >= n_fft + hop and np.all(np.diff(z[:n_fft + hop]) == 1)
    assert np.sum(np.abs(x) > 1.1) >= 1


@pytest.fixture(scope="module")
def filelist(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("trainset"))
    fl = S.write_train_filelist(root, spec_bins=1025)
    S.write_nof0_filelist(fl)
    return fl


def test_loaders_collates_samplers_match_reference(filelist):
    g = golden("train_loader_cases.npz")
    mine = S.train_loader_summary(DU, filelist, HParams(**HP))
    assert sorted(mine) == sorted(g)
    for k in sorted(g):
        assert mine[k].shape == g[k].shape and np.array_equal(mine[k], g[k]), (k, mine[k], g[k])
    # the quirks the summary must have seen
    assert g["lengths"][0] == os.path.getsize(filelist.replace("filelist.txt", "0_gt_wavs/0_0.wav")) // (3 * 400)
    assert g["item_sizes"][11][3] == 900 and g["item_sizes"][11][1] == 900 and g["item_sizes"][11][2] == 900 * 400
    assert len(g["dist_1_0_boundaries"]) == len(S.TRAIN_FILELIST_BOUNDARIES) - 1 and 180 not in g["dist_1_0_boundaries"]


def test_loader_item_types(filelist):
    ds = DU.TextAudioLoaderMultiNSFsid(filelist, HParams(**HP))
    spec, wav, phone, pitch, pitchf, sid = ds[4]
    assert spec.dtype == torch.float32 and wav.dtype == torch.float32 and phone.dtype == torch.float32 and pitchf.dtype == torch.float32
    assert pitch.dtype == torch.int64 and sid.dtype == torch.int64 and sid.shape == (1,)
    assert spec.shape[1] == phone.shape[0] == pitch.shape[0] == pitchf.shape[0] and wav.shape == (1, spec.shape[1] * 400)
    ds_bad = DU.TextAudioLoaderMultiNSFsid(filelist, HParams(**dict(HP, sampling_rate=48000)))
    with pytest.raises(ValueError):
        ds_bad[0]


def test_shuffled_sampler(filelist):
    ds = DU.TextAudioLoaderMultiNSFsid(filelist, HParams(**HP))
    sm = [DU.DistributedBucketSampler(ds, 2, list(S.TRAIN_FILELIST_BOUNDARIES), num_replicas=2, rank=r, shuffle=True) for r in (0, 1)]
    bucket_of = {i: b for b, members in enumerate(sm[0].buckets) for i in members}
    epochs = []
    for epoch in (0, 1, 2):
        per_rank = []
        for s in sm:
            s.set_epoch(epoch)
            batches = list(iter(s))
            assert len(batches) == len(s)
            assert all(len(set(bucket_of[i] for i in b)) == 1 for b in batches), "a batch crossed a bucket"
            assert list(iter(s)) == batches, "the same epoch must give the same batches"
            per_rank.append(batches)
        # the two ranks partition the epoch: together, per bucket, exactly the filled-up bucket (every member at least once)
        for b, members in enumerate(sm[0].buckets):
            drawn = sorted(i for batches in per_rank for bt in batches for i in bt if bucket_of[i] == b)
            assert len(drawn) == sm[0].num_samples_per_bucket[b] and set(drawn) == set(members)
            counts = np.bincount(drawn, minlength=len(ds))[members]
            assert counts.max() - counts.min() <= 1 or len(members) < 4
        epochs.append(per_rank)
    assert epochs[0] != epochs[1] and epochs[1] != epochs[2]
    single = DU.BucketSampler(ds, 2, list(S.TRAIN_FILELIST_BOUNDARIES), shuffle=True)
    single.set_epoch(3)
    a = list(iter(single))
    assert a == list(iter(single)) and len(a) == len(single)
    single.set_epoch(4)
    assert a != list(iter(single))


@pytest.mark.parametrize("sr,n_fft,n_mels,fmin,fmax", [(32000, 1024, 80, 0.0, None), (40000, 2048, 125, 0.0, None), (48000, 2048, 128, 0.0, None),
                                                       (40000, 2048, 80, 40.0, 16000.0)])
def test_mel_filterbank_properties(sr, n_fft, n_mels, fmin, fmax):
    w = MP.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    assert w.shape == (n_mels, n_fft // 2 + 1) and w.dtype == np.float32
    assert np.all(w >= 0)
    centres = MP.mel_center_frequencies(sr, n_mels, fmin, fmax)[1:-1]
    freqs = np.arange(n_fft // 2 + 1) * (sr / n_fft)
    for m in range(n_mels):
        nz = np.flatnonzero(w[m])
        assert nz.size >= 1 and np.all(np.diff(nz) == 1), f"row {m}: support not contiguous"
        # the peak lies at the centre frequency: on one of the two bins that bracket it
        assert abs(freqs[int(np.argmax(w[m]))] - centres[m]) <= sr / n_fft, (m, freqs[int(np.argmax(w[m]))], centres[m])
    first, count, weights = MP.band_filterbank(w)
    assert first.dtype == np.int32 and count.dtype == np.int32 and weights.dtype == np.float32 and weights.shape[0] == count.sum()
    assert np.array_equal(MP.unband_filterbank(first, count, weights, n_fft // 2 + 1), w)


def test_center_true_raises():
    y = torch.zeros(1, 4000)
    with pytest.raises(NotImplementedError):
        MP.spectrogram_torch(y, 2048, 400, 2048, center=True)
    with pytest.raises(NotImplementedError):
        MP.mel_spectrogram_torch(y[None], 2048, 128, 40000, 400, 2048, 0.0, None, center=True)
    with pytest.raises(NotImplementedError):
        MP.spectrogram_batch([y[0]], 2048, 400, 2048, center=True)


def test_hparams(tmp_path):
    p = tmp_path / "c.json"
    p.write_text('{"train": {"batch_size": 4}, "data": {"sampling_rate": 40000, "hop_length": 400}}')
    hp = get_hparams_from_file(str(p))
    assert hp.data.sampling_rate == 40000 and hp["train"]["batch_size"] == 4 and "data" in hp and len(hp) == 2


def test_new_symbols_declared_exported_and_bound():
    from comfy_rvc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rvc_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in ("rvc_spectrogram_batch", "rvc_mel_filterbank_set", "rvc_spec_to_mel_batch"):
        assert re.search(rf"\b{s}\s*\(", hdr), s
        assert hasattr(_lib.lib, s) and s in _lib.SIGNATURES
