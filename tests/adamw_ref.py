"""torch.optim.AdamW (amsgrad off, maximize off) restated in float64 numpy, the test inputs of the element-wise kernel, and the staged gates the device and
torch's own float32 kernel are held to (tests/test_disc_optim_host.py, tests/test_hip_disc_optim.py)."""
import numpy as np

U = 2.0 ** -24                                     # float32 unit roundoff
SIZES = (1, 3, 63, 64, 65, 255, 256, 257, 1025, 4099)       # every edge of the scalar head / float4 body / scalar tail and of the workgroup's passes
BETAS, EPS, WD = (0.8, 0.99), 1e-9, 0.01
CLIP = float(np.float32(0.0625))


def scalars(lr, beta1, beta2, wd, step):
    """(1 - lr wd, lr / bc1, sqrt(bc2)) as torch forms them, in Python floats"""
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    return 1 - lr * wd, lr / bc1, bc2 ** 0.5


def clamp(g, clip):
    return g if clip is None else np.clip(g, -clip, clip)


def step64(p, g, m, v, lr, betas, eps, wd, step, clip=None):
    """one step on float64 arrays: (p, m, v) after the step being taken `step` (>= 1)"""
    p, g, m, v = (np.asarray(t, dtype=np.float64) for t in (p, g, m, v))
    decay, step_size, sbc2 = scalars(lr, betas[0], betas[1], wd, step)
    g = clamp(g, clip)
    p = p * decay
    m = m + (g - m) * (1 - betas[0])
    v = v * betas[1] + (1 - betas[1]) * g * g
    p = p - step_size * (m / (np.sqrt(v) / sbc2 + eps))
    return p, m, v


def gate_units(p_prev, g, m_prev, v_prev, p, m, v, lr, betas, eps, wd, step, clip=None):
    """The staged gates, each stage's float64 restatement fed the inputs that stage really had (float32 values): the largest of
         |m - m64| / (4u (|m_prev| + |g'|)),   |v - v64| / (4u (v_prev + g'^2)),   |p - p64| / (4u (|p_prev| + |p64| + |delta64|))
    with p64 and delta64 from the GIVEN new m and v.  A result passes when all three are <= 1."""
    p_prev, g, m_prev, v_prev, p, m, v = (np.asarray(t, dtype=np.float64) for t in (p_prev, g, m_prev, v_prev, p, m, v))
    decay, step_size, sbc2 = scalars(lr, betas[0], betas[1], wd, step)
    gc = clamp(g, clip)
    m64 = m_prev + (gc - m_prev) * (1 - betas[0])
    v64 = v_prev * betas[1] + (1 - betas[1]) * gc * gc
    delta64 = step_size * (m / (np.sqrt(v) / sbc2 + eps))
    p64 = p_prev * decay - delta64

    def worst(err, scale):
        err, scale = np.abs(err), 4 * U * scale
        if np.any((scale == 0) & (err != 0)):
            return float("inf")
        return float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), 0.0))) if err.size else 0.0
    return (worst(m - m64, np.abs(m_prev) + np.abs(gc)), worst(v - v64, v_prev + gc * gc), worst(p - p64, np.abs(p_prev) + np.abs(p64) + np.abs(delta64)))


def gradients(rng, n, clip=CLIP):
    """float32: log-normal magnitudes over about 12 decades, every 7th exactly 0, none with 0 < |g| < 1e-15, about 10 % beyond the clip value"""
    mag = np.exp(rng.uniform(np.log(1e-14), np.log(clip), n))
    far = rng.random(n) < 0.1
    mag[far] = clip * (1.0 + 3.0 * rng.random(int(far.sum())) + 1e-3)
    g = (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g[::7] = 0.0
    assert not np.any((g != 0) & (np.abs(g) < 1e-15))
    return g


def case(step, seed=0, sizes=SIZES):
    """[(p, g, m, v)] float32 per tensor: the state before the step being taken `step` (zeros at step 1, a plausible history afterwards)"""
    rng = np.random.default_rng(1000 * seed + step)
    out = []
    for n in sizes:
        p = rng.standard_normal(n).astype(np.float32)
        g = gradients(rng, n)
        if step == 1:
            m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
        else:
            h = gradients(rng, n)
            m = (0.5 * h).astype(np.float32)
            v = (0.3 * h.astype(np.float64) ** 2 + 1e-30).astype(np.float32)
        out.append((p, g, m, v))
    return out
