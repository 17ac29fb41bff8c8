"""CPU: the float64 restatements of tests/glue_ref.py against torch's own float64 ops and the oracle, so that a wrong reference fails here and not on the GPU."""
import numpy as np
import torch
import torch.nn.functional as F

import glue_ref as R


def _rng(seed):
    return np.random.default_rng(seed)


def test_hubert_conv0_is_conv_groupnorm_gelu():
    g = _rng(1)
    for C, T1, extra in ((16, 5, 0), (24, 37, 1), (8, 130, 4)):
        L = 5 * (T1 - 1) + 10 + extra
        audio, w = g.standard_normal(L) * 0.1 + 0.05, g.standard_normal((C, 10)) * 0.3
        gamma, beta = g.uniform(0.5, 1.5, C), g.standard_normal(C) * 0.1
        conv = F.conv1d(torch.from_numpy(audio)[None, None], torch.from_numpy(w)[:, None], stride=5)
        assert conv.shape[-1] == T1
        want = F.gelu(F.group_norm(conv, C, torch.from_numpy(gamma), torch.from_numpy(beta), 1e-5))[0].numpy()
        np.testing.assert_allclose(R.hubert_conv0(audio, w, gamma, beta, T1), want, rtol=0, atol=1e-12)
    # audio shorter than the last window: the tail is zero
    T1, C = 9, 8
    audio, w = g.standard_normal(5 * (T1 - 1) + 10), g.standard_normal((C, 10))
    cut = audio.copy()
    cut[-3:] = 0
    np.testing.assert_array_equal(R.hubert_conv0(audio[:-3], w, np.ones(C), np.zeros(C), T1), R.hubert_conv0(cut, w, np.ones(C), np.zeros(C), T1))


def test_conv_to1_is_conv1d_of_the_leaky_relu():
    g = _rng(2)
    for Ci, T, K, pad, slope, act in ((16, 9, 7, 3, 0.01, 1), (4, 1, 7, 3, 1.0, 0), (3, 30, 5, 2, 0.01, 0), (5, 17, 9, 4, 0.01, 1)):
        x, w = g.standard_normal((Ci, T)), g.standard_normal((Ci, K)) * 0.2
        s = float(np.float32(slope))
        want = F.conv1d(F.leaky_relu(torch.from_numpy(x), s)[None], torch.from_numpy(w)[None], padding=pad)[0, 0]
        want = torch.tanh(want) if act else want
        y, mag = R.conv_to1(x, w, pad, slope, act)
        np.testing.assert_allclose(y, want.numpy(), rtol=0, atol=1e-13)
        assert mag.shape == (T,) and np.all(mag >= np.abs(np.arctanh(y) if act else y) - 1e-9)


def test_noise_add_is_strided_conv1d():
    g = _rng(3)
    for k, stride, pad, C, T in ((1, 1, 0, 8, 12), (4, 2, 1, 16, 20), (8, 4, 2, 24, 8)):
        L = T * stride
        x, src, w, b = g.standard_normal((C, T)), g.standard_normal(L), g.standard_normal((C, k)), g.standard_normal(C)
        want = x + F.conv1d(torch.from_numpy(src)[None, None], torch.from_numpy(w)[:, None], torch.from_numpy(b), stride=stride, padding=pad)[0].numpy()
        y, mag = R.noise_add(x, src, L, w, b, stride, pad)
        np.testing.assert_allclose(y, want, rtol=0, atol=1e-13)
        assert np.all(mag >= np.abs(y) - 1e-12)
        # a shorter source = the same source with its tail zeroed
        Ls = L - stride - 1
        cut = src.copy()
        cut[Ls:] = 0
        np.testing.assert_array_equal(R.noise_add(x, src, Ls, w, b, stride, pad)[0], R.noise_add(x, cut, L, w, b, stride, pad)[0])


def test_frames_is_pad_plus_unfold():
    g = _rng(4)
    for L, k, stride, pad, reflect in ((2000, 1024, 160, 512, 1), (1025, 1024, 160, 512, 1), (100, 8, 4, 2, 0), (37, 4, 2, 1, 0)):
        src = g.standard_normal(L).astype(np.float32)
        p = F.pad(torch.from_numpy(src)[None, None], (pad, pad), mode="reflect" if reflect else "constant")[0, 0]
        u = p.unfold(0, k, stride).T.numpy()              # [k][frames]
        Tout = u.shape[1]
        np.testing.assert_array_equal(R.frames(src, k, stride, pad, Tout, reflect), u)
    # one frame more than the padded signal holds: zeros past the end (zero mode)
    src = g.standard_normal(100).astype(np.float32)
    got = R.frames(src, 8, 4, 2, 26, 0)
    np.testing.assert_array_equal(got[:, :25], R.frames(src, 8, 4, 2, 25, 0))
    np.testing.assert_array_equal(got[:, 25], np.r_[src[98:100], np.zeros(6, np.float32)])


def test_mel_to_unet_is_right_reflect_pad_and_transpose():
    g = _rng(5)
    for n in (32, 33, 47, 100):
        Tr = 32 * ((n - 1) // 32 + 1)
        mel = g.standard_normal((128, n))
        want = (F.pad(torch.from_numpy(mel)[None], (0, Tr - n), mode="reflect")[0].T * float(np.float32(0.37)) + float(np.float32(-1.25))).numpy()
        y, mag = R.mel_to_unet(mel, Tr, 0.37, -1.25)
        np.testing.assert_allclose(y, want, rtol=0, atol=1e-14)
        assert y.shape == (Tr, 128) and np.all(mag >= np.abs(y))


def test_feats_prepare_protect_rule():
    g = _rng(6)
    D, Th = 4, 3
    T = 2 * Th
    f, f0 = g.standard_normal((D, Th)), g.standard_normal((D, Th))
    pf = np.array([0.0, 0.5, 1.0, 220.0, -1.0, 0.999], np.float32)
    up = F.interpolate(torch.from_numpy(f)[None], scale_factor=2)[0].numpy()
    up0 = F.interpolate(torch.from_numpy(f0)[None], scale_factor=2)[0].numpy()
    np.testing.assert_array_equal(R.feats_prepare(f, f0, pf, T, 0.33, 0)[0], up)
    p = float(np.float32(0.33))
    w = np.array([p, p, 1.0, 1.0, p, p])            # the reference pipeline: pitchff[pitchf > 0] = 1; pitchff[pitchf < 1] = protect
    np.testing.assert_allclose(R.feats_prepare(f, f0, pf, T, 0.33, 1)[0], up * w + up0 * (1 - w), rtol=0, atol=1e-15)
    np.testing.assert_allclose(R.feats_prepare(f, None, pf, T, 0.33, 1)[0], up, rtol=0, atol=1e-15)


def test_wn_gate():
    g = _rng(7)
    a, gg = g.standard_normal((32, 9)) * 10, g.standard_normal(32)
    t = torch.from_numpy(a + gg[:, None])
    np.testing.assert_allclose(R.wn_gate(a, gg), (torch.tanh(t[:16]) * torch.sigmoid(t[16:])).numpy(), rtol=1e-13, atol=1e-300)


def test_split2d_level_changes():
    g = _rng(8)
    for C, H, W in ((8, 2, 2), (8, 5, 7), (16, 4, 6)):
        x = g.standard_normal((C, H, W))
        y, mag = R.pool2_pad(x)
        np.testing.assert_allclose(R.unpad2d(y), F.avg_pool2d(torch.from_numpy(x)[None], 2)[0].numpy(), rtol=0, atol=1e-15)
        assert np.all(y[:, :, 0] == 0) and np.all(y[:, :, -1] == 0) and np.all(mag >= np.abs(y))
        np.testing.assert_array_equal(R.unpad2d(R.pad2d(x)), x)
        assert R.pad2d(x).shape == (C, H, W + 2) and np.all(R.pad2d(x)[:, :, [0, -1]] == 0)
    # the phase interleave is ConvTranspose2d(kernel 2, stride 2) with one-hot weights: out[c][2h+a][2w+b] = ph[(2a+b) Co + c][h][w]
    Co, H, W = 3, 4, 5
    ph = g.standard_normal((4 * Co, H, W))
    wt = torch.zeros(4 * Co, Co, 2, 2, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            for c in range(Co):
                wt[(2 * a + b) * Co + c, c, a, b] = 1
    np.testing.assert_array_equal(R.interleave2(ph, Co), F.conv_transpose2d(torch.from_numpy(ph)[None], wt, stride=2)[0].numpy())


def test_gru_scan_is_nn_gru():
    g = torch.Generator().manual_seed(9)
    gru = torch.nn.GRU(12, 256, bidirectional=True).double()
    with torch.no_grad():
        for p in gru.parameters():
            p.copy_((torch.rand(p.shape, generator=g, dtype=torch.float64) * 2 - 1) / 16)
    for T in (1, 2, 5):
        x = torch.randn(T, 1, 12, generator=g, dtype=torch.float64)
        with torch.no_grad():
            want = gru(x)[0][:, 0].T.numpy()          # [512][T]
            gi = torch.cat([x[:, 0] @ gru.weight_ih_l0.T, x[:, 0] @ gru.weight_ih_l0_reverse.T], 1).numpy()
        cat = lambda a, b: np.stack([a.detach().numpy(), b.detach().numpy()])
        got = R.gru_scan(gi, cat(gru.bias_ih_l0, gru.bias_ih_l0_reverse), cat(gru.weight_hh_l0, gru.weight_hh_l0_reverse), cat(gru.bias_hh_l0, gru.bias_hh_l0_reverse))
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-14)


def test_rmvpe_decode_is_the_oracles():
    from oracle import nets
    g = _rng(10)
    sal = g.uniform(0, 0.2, (40, 360)).astype(np.float32)
    for t, b in enumerate((0, 1, 3, 4, 355, 356, 358, 359)):
        sal[t, b] = 0.9
    sal[8] = 0.0
    sal[9] = np.minimum(sal[9], np.float32(0.03))
    sal[9, 100] = np.float32(0.03)                       # maximum == thred: unvoiced
    sal[10, 50] = sal[10, 200] = 0.95                    # exact tie: the first bin wins
    with np.errstate(invalid="ignore", divide="ignore"):
        # (handed the same values as float64: on float32 input the oracle sums its denominator in float32, the device and glue_ref in float64)
        want = nets.rmvpe_decode(sal.astype(np.float64), float(np.float32(0.03)))
    got = R.rmvpe_decode(sal, 0.03)
    assert got[8] == 0 and got[9] == 0 and np.all(np.isfinite(got))
    np.testing.assert_allclose(got, np.nan_to_num(want), rtol=1e-13, atol=0)
    assert abs(1200 * np.log2(got[10] / 10) - (20 * 50 + 1997.3794084376191)) < 40


def test_f0_post_is_the_oracles():
    from oracle import pipeline
    f0 = np.array([0, 30, 49.9, 50, 220.5, 1100, 1101, 5000], np.float64)
    mel = lambda f: 1127 * np.log(1 + f / 700)
    for key in (0, 5, -12):
        want_pitch, want_f0 = pipeline.f0_postprocess(f0, f0_up_key=key, f0_min=50, f0_max=1100)
        pitch, pitchf = R.f0_post(f0, pow(2, key / 12), mel(50.0), mel(1100.0), 256)
        np.testing.assert_array_equal(pitchf, want_f0.astype(np.float32))
        # (the oracle's mel is 1127 ln(1 + f / 700), the device's 2595 log10(1 + f / 700) with the same limits passed in: equal to 1e-4 of a bin - the two
        # constants differ by 2e-5 relative - so only positions that close to a half-integer may differ)
        m = R.f0_mel(f0, pow(2, key / 12), 2595 * np.log10(1 + 50 / 700), 2595 * np.log10(1 + 1100 / 700), 256)
        clear = np.abs(m - np.floor(m) - 0.5) > 1e-3
        assert clear.sum() >= 6
        np.testing.assert_array_equal(np.rint(m)[clear], want_pitch[clear])
        assert pitch.min() >= 1 and pitch.max() <= 255


def test_interp_linear_is_f_interpolate():
    g = _rng(11)
    for n, N in ((1, 1), (3, 1), (2, 7), (6, 40000), (9, 7999), (5, 3)):
        a = g.uniform(0.1, 1, n)
        want = F.interpolate(torch.from_numpy(a)[None, None], size=N, mode="linear")[0, 0].numpy()
        np.testing.assert_allclose(R.interp_linear(a, N), want, rtol=1e-12, atol=1e-15)


def test_change_rms_and_postprocess_are_the_oracles():
    from oracle import pipeline
    g = _rng(12)
    sr2 = 16000
    for N, rate in ((40000, 0.25), (8001, 0.0), (7999, 0.25)):
        data1 = g.standard_normal(N // 2 + 9000) * 0.1
        x = (g.standard_normal(N) * np.linspace(0.05, 0.4, N)).astype(np.float32)
        rms1 = pipeline.rms(data1, 16000, 8000)[0]
        np.testing.assert_allclose(R.frame_rms(data1, 16000, 8000), rms1, rtol=1e-13)
        want = pipeline.change_rms(data1, 16000, x.astype(np.float64), sr2, rate)
        got = R.change_rms(x, rms1, sr2, rate)
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-15)
        i16 = R.postprocess(x, rms1, sr2, rate)
        ref = (want * 32768 / (np.abs(want).max() / 0.99)).astype(np.int16).astype(np.int64)
        assert np.max(np.abs(i16 - ref)) <= 1 and np.abs(i16).max() in (32439, 32440)
    x = g.standard_normal(100).astype(np.float32)
    np.testing.assert_array_equal(R.postprocess(x, None, sr2, 0.25), R.postprocess(x, np.ones(3), sr2, 1.0))
