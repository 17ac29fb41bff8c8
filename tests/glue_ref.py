"""float64 restatements of the model-glue device ops (csrc/ops.hip without the GEMMs, csrc/split2d.hip), written from the kernels' comments.

Plain numpy (torch only for erf): what tests/test_hip_glue_ops.py compares the kernels with, and what tests/test_glue_ref_host.py pins against
torch / the oracle on the CPU.  Functions whose tolerance is `4 * 2^-24 * sum |terms|` return (value, sum of |terms|)."""
import numpy as np
import torch

U24 = 2.0 ** -24          # unit roundoff of float32


def f64(x):
    return np.asarray(x, dtype=np.float64)


def gelu(v):
    return 0.5 * v * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(v)) * 0.70710678118654752440).numpy())


def hubert_conv0(audio, w, gamma, beta, T1, eps=1e-5):
    """Conv1d(1, C, 10, stride 5, no bias) -> GroupNorm(C, C) (per-channel statistics over the T1 positions, biased variance) -> GELU; the audio is
    zero beyond its length.  audio [L], w [C][10] -> [C][T1]"""
    audio, w = f64(audio), f64(w)
    need = 5 * (T1 - 1) + 10
    a = np.zeros(need)
    a[:min(need, audio.size)] = audio[:need]
    fr = a[5 * np.arange(T1)[None, :] + np.arange(10)[:, None]]          # [10][T1]
    conv = w @ fr
    mean = conv.mean(1, keepdims=True)
    var = ((conv - mean) ** 2).mean(1, keepdims=True)
    return gelu((conv - mean) / np.sqrt(var + eps) * f64(gamma)[:, None] + f64(beta)[:, None])


def conv_to1(x, w, pad, pre_slope, act_tanh):
    """y[t] = act(sum_c sum_j w[c][j] pre(x[c][t + j - pad])), zero padding, pre(v) = max(v, v * slope).  x [Ci][T], w [Ci][K] -> (y [T], sum |terms| [T])"""
    x, w = f64(x), f64(w)
    Ci, T = x.shape
    K = w.shape[1]
    s = float(np.float32(pre_slope))
    xp = np.zeros((Ci, T + K))
    xp[:, pad:pad + T] = np.maximum(x, x * s)
    y, mag = np.zeros(T), np.zeros(T)
    for j in range(K):
        term = w[:, j:j + 1] * xp[:, j:j + T]
        y += term.sum(0)
        mag += np.abs(term).sum(0)
    return (np.tanh(y) if act_tanh else y), mag


def noise_add(x, src, L, w, b, stride, pad):
    """x[c][t] + b[c] + sum_j w[c][j] src[t stride + j - pad], src zero outside [0, L).  x [C][T], w [C][k] -> (y, sum |terms|)"""
    x, src, w, b = f64(x), f64(src), f64(w), f64(b)
    C, T = x.shape
    k = w.shape[1]
    y, mag = x + b[:, None], np.abs(x) + np.abs(b)[:, None]
    for j in range(k):
        q = np.arange(T) * stride + j - pad
        ok = (q >= 0) & (q < L)
        sv = np.where(ok, src[np.clip(q, 0, L - 1)], 0.0)
        y = y + w[:, j:j + 1] * sv[None, :]
        mag = mag + np.abs(w[:, j:j + 1] * sv[None, :])
    return y, mag


def frames(src, k, stride, pad, Tout, reflect):
    """out[j][t] = src[t stride + j - pad]; outside [0, L): zero, or mirrored about sample 0 / sample L - 1"""
    src = np.asarray(src)
    L = src.size
    q = np.arange(Tout)[None, :] * stride + np.arange(k)[:, None] - pad
    if reflect:
        q = np.where(q < 0, -q, q)
        q = np.where(q >= L, 2 * (L - 1) - q, q)
        return src[q]
    ok = (q >= 0) & (q < L)
    return np.where(ok, src[np.clip(q, 0, L - 1)], src.dtype.type(0))


def mel_to_unet(mel, Tr, a, b):
    """x[t][m] = a mel[m][t'] + b, t < Tr, t' = t mirrored about frame n - 1 where t >= n.  mel [128][n] -> (x [Tr][128], sum |terms|)"""
    mel = f64(mel)
    n = mel.shape[1]
    t = np.arange(Tr)
    t = np.where(t >= n, 2 * (n - 1) - t, t)
    a, b = float(np.float32(a)), float(np.float32(b))
    v = mel[:, t].T * a
    return v + b, np.abs(v) + abs(b)


def feats_prepare(f, f0, pitchf, T, protect, do_protect):
    """Nearest x2 upsampling of f [D][Th] to T frames; with do_protect the blend w f + (1 - w) f0, w = 1 where pitchf > 0, then w = protect where
    pitchf < 1 (so every pitch below 1, negative and fractional ones included, takes `protect`).  f0 None: f0 = f.  -> (out [D][T], sum |terms|)"""
    f = f64(f)
    up = f[:, np.arange(T) >> 1]
    if not do_protect:
        return up, np.abs(up)
    up0 = up if f0 is None else f64(f0)[:, np.arange(T) >> 1]
    pf = f64(pitchf)[:T]
    w = np.where(pf > 0, 1.0, pf)
    w = np.where(pf < 1, float(np.float32(protect)), w)[None, :]
    return up * w + up0 * (1.0 - w), np.abs(up * w) + np.abs(up0 * (1.0 - w))


def wn_gate(a, g):
    """tanh(a[c] + g[c]) sigmoid(a[H + c] + g[H + c]).  a [2 H][T], g [2 H] -> [H][T]"""
    a, g = f64(a), f64(g)
    H = a.shape[0] // 2
    ta, sa = a[:H] + g[:H, None], a[H:] + g[H:, None]
    return np.tanh(ta) / (1.0 + np.exp(-sa))


def pad2d(x):
    """[C][H][W] -> [C][H][W + 2] with a zero column on either side"""
    return np.pad(np.asarray(x), ((0, 0), (0, 0), (1, 1)))


def unpad2d(xp):
    return np.asarray(xp)[:, :, 1:-1]


def pool2_pad(x):
    """AvgPool2d(2) of [C][H][W] (odd rows / columns dropped) as a padded level [C][H / 2][W / 2 + 2] -> (y, sum |terms|)"""
    x = f64(x)
    C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    q = x[:, :2 * Ho, :2 * Wo].reshape(C, Ho, 2, Wo, 2)
    return pad2d(q.sum((2, 4)) * 0.25), pad2d(np.abs(q).sum((2, 4)) * 0.25)


def interleave2(ph, Co):
    """out[c][2 h + a][2 w + b] = ph[(2 a + b) Co + c][h][w].  ph [4 Co][H][W] (plain) -> [Co][2 H][2 W] (plain)"""
    ph = np.asarray(ph)
    _, H, W = ph.shape
    out = np.zeros((Co, 2 * H, 2 * W), dtype=ph.dtype)
    for a in range(2):
        for b in range(2):
            out[:, a::2, b::2] = ph[(2 * a + b) * Co:(2 * a + b + 1) * Co]
    return out


def gru_scan(gi, b_ih, w_hh, b_hh):
    """Bidirectional GRU recurrence, hidden 256, gates in nn.GRU's order r, z, n:  r = s(gi_r + b_ir + W_hr h + b_hr), z likewise,
    n = tanh(gi_n + b_in + r (W_hn h + b_hn)), h' = (1 - z) n + z h; the second direction walks the frames backwards.
    gi [T][2 * 768], b_ih / b_hh [2][768], w_hh [2][768][256] -> [512][T]"""
    gi, b_ih, w_hh, b_hh = f64(gi), f64(b_ih).reshape(2, 768), f64(w_hh).reshape(2, 768, 256), f64(b_hh).reshape(2, 768)
    T = gi.shape[0]
    out = np.zeros((512, T))
    for d in range(2):
        h = np.zeros(256)
        for step in range(T):
            t = T - 1 - step if d else step
            x = gi[t, d * 768:(d + 1) * 768] + b_ih[d]
            gh = w_hh[d] @ h + b_hh[d]
            r = 1.0 / (1.0 + np.exp(-(x[:256] + gh[:256])))
            z = 1.0 / (1.0 + np.exp(-(x[256:512] + gh[256:512])))
            n = np.tanh(x[512:] + r * gh[512:])
            h = (1.0 - z) * n + z * h
            out[d * 256:(d + 1) * 256, t] = h
    return out


def rmvpe_decode(sal, thred):
    """f0 = 10 * 2^(cents / 1200), cents = the salience-weighted mean of 20 c + 1997.3794084376191 over the (at most) nine bins around the first
    arg-max; 0 where the maximum does not exceed thred.  sal float32 [n][360] -> float64 [n]"""
    sal = np.asarray(sal, dtype=np.float32)
    n = sal.shape[0]
    f0 = np.zeros(n)
    for t in range(n):
        am = int(np.argmax(sal[t]))
        if not sal[t, am] > np.float32(thred):
            continue
        c = np.arange(max(am - 4, 0), min(am + 5, 360))
        v = sal[t, c].astype(np.float64)
        cents = np.sum(v * (20.0 * c + 1997.3794084376191)) / np.sum(v)
        f = 10.0 * 2.0 ** (cents / 1200.0)
        f0[t] = 0.0 if f == 10.0 else f
    return f0


def f0_mel(f0, factor, mel_min, mel_max, bins):
    """the clipped float64 mel position whose rint is the coarse pitch"""
    f = f64(f0) * factor
    m = (2595.0 * np.log10(1.0 + f / 700.0) - mel_min) * (bins - 2) / (mel_max - mel_min) + 1.0
    return np.clip(m, 1.0, bins - 1.0)


def f0_post(f0, factor, mel_min, mel_max, bins):
    """-> (pitch int64 = rint of the mel position, pitchf float32 = f0 * factor)"""
    return np.rint(f0_mel(f0, factor, mel_min, mel_max, bins)).astype(np.int64), (f64(f0) * factor).astype(np.float32)


def interp_linear(a, N):
    """1-D linear resize to N samples with half-pixel centres (source x = (i + 0.5) n / N - 0.5, clamped below at 0, the last sample repeated)"""
    a = f64(a)
    n = a.size
    src = np.maximum((np.arange(N) + 0.5) * (n / N) - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = src - i0
    return (1.0 - l1) * a[i0] + l1 * a[i1]


def frame_rms(x, frame, hop):
    """centred frames with zero padding of frame / 2 on both sides: sqrt(mean(x^2)) of 1 + len / hop frames"""
    x = np.pad(f64(x), frame // 2)
    n = 1 + (x.size - frame) // hop
    return np.array([np.sqrt(np.mean(x[i * hop:i * hop + frame] ** 2)) for i in range(n)])


def change_rms(x, rms1, sr2, rate):
    """x * rms1'^(1 - rate) * max(rms2', 1e-6)^(rate - 1), primes = linear resize to len(x); rms2 = frame RMS of x (frame sr2, hop sr2 / 2)"""
    x = f64(x)
    r1 = interp_linear(rms1, x.size)
    r2 = np.maximum(interp_linear(frame_rms(x, sr2 // 2 * 2, sr2 // 2), x.size), 1e-6)
    return x * (r1 ** (1.0 - rate) * r2 ** (rate - 1.0))


def postprocess(x, rms1, sr2, rate):
    """the RMS mix (only when rate < 1 and an input envelope is given), then peak normalisation to 0.99 full scale, truncated to int16"""
    x = f64(x)
    if rate < 1 and rms1 is not None:
        x = change_rms(x, rms1, sr2, float(np.float32(rate)))
    amax = np.abs(x).max() / 0.99
    return np.trunc(x * 32768.0 / amax).astype(np.int64)
