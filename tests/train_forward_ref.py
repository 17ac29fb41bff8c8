"""CPU restatement of SynthesizerTrnMs{256,768}NSFsid[_nono].forward (reference lib/infer_pack/models.py:781-796,:894-903) for the training-forward
tests: composed from oracle.nets (enc_p_forward, _wn with n_layers=16, generator_forward) plus the forward coupling, the slice and the two losses.
Item by item at its own length, like the library: inside an item's length that is what the reference's padded, masked batch computes, and beyond it every
returned tensor is 0.  Helper module, no tests."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import nets


def posterior_forward(sd, config, y, g, noise_q):
    """PosteriorEncoder.forward (reference models.py:229-238) with a full mask: y [1,spec,T] -> z, m_q, logs_q [1,inter,T]."""
    inter, hidden = config[2], config[3]
    h = F.conv1d(y, sd["enc_q.pre.weight"], sd["enc_q.pre.bias"])
    h = nets._wn(sd, "enc_q.enc.", h, g, hidden, n_layers=16)
    stats = F.conv1d(h, sd["enc_q.proj.weight"], sd["enc_q.proj.bias"])
    m, logs = stats[:, :inter], stats[:, inter:]
    return m + noise_q * torch.exp(logs), m, logs


def flow_forward(sd, config, z, g):
    """ResidualCouplingBlock.forward(reverse=False) (reference models.py:185-189): coupling 0 .. 3, each followed by Flip; mean_only: x1 = m + x1
    (lib/infer_pack/modules.py:436-451)."""
    hidden, half = config[3], config[2] // 2
    x = z
    for f in range(4):
        p = f"flow.flows.{2 * f}."
        x0, x1 = x[:, :half], x[:, half:]
        h = F.conv1d(x0, sd[p + "pre.weight"], sd[p + "pre.bias"])
        h = nets._wn(sd, p + "enc.", h, g, hidden)
        m = F.conv1d(h, sd[p + "post.weight"], sd[p + "post.bias"])
        x = torch.flip(torch.cat([x0, m + x1], 1), [1])
    return x


def slice_starts(rand, lengths, seg):
    """rand_slice_segments (reference lib/infer_pack/commons.py:168-175): ids = (torch.rand([b]) * (lengths - seg + 1)).long()."""
    return (torch.as_tensor(rand) * (torch.as_tensor(lengths) - seg + 1)).to(dtype=torch.long)


def generator_slice(sd, config, z, pitchf, g, noise_src, start):
    """The generator on columns [start, start + seg) of z / pitchf as a sequence of its own (reference models.py:789-795)."""
    seg = config[1]
    zs = z[:, :, start:start + seg]
    pf = None if pitchf is None else pitchf[:, start:start + seg]
    return nets.generator_forward(sd, config, zs, pf, g, noise_src)


def forward(sd, config, phone, lengths, pitch, pitchf, y, ds, noise_q, noise_src, ids_slice):
    """-> dict of float32 arrays: o [B,1,seg*upp], z, z_p, m_p, logs_p, m_q, logs_q [B,inter,T] (zero beyond each length).  pitch = pitchf = noise_src =
    None: the no-f0 family."""
    sd = nets.tensors(sd)
    inter, seg = config[2], config[1]
    upp = int(np.prod(config[12]))
    phone, y, noise_q = nets._t(phone).float(), nets._t(y).float(), nets._t(noise_q).float()
    B, T = y.shape[0], y.shape[2]
    out = {k: torch.zeros(B, inter, T) for k in ("z", "z_p", "m_p", "logs_p", "m_q", "logs_q")}
    out["o"] = torch.zeros(B, 1, seg * upp)
    with torch.no_grad():
        for b in range(B):
            L, start = int(lengths[b]), int(ids_slice[b])
            g = sd["emb_g.weight"][int(ds[b])].view(1, -1, 1)
            pc = None if pitch is None else nets._t(pitch)[b:b + 1, :L].long()
            m_p, logs_p = nets.enc_p_forward(sd, config, phone[b:b + 1, :L], pc)
            z, m_q, logs_q = posterior_forward(sd, config, y[b:b + 1, :, :L], g, noise_q[b:b + 1, :, :L])
            z_p = flow_forward(sd, config, z, g)
            pf = None if pitchf is None else nets._t(pitchf)[b:b + 1, :L].float()
            ns = None if noise_src is None else nets._t(noise_src)[b:b + 1].float()
            out["o"][b:b + 1] = generator_slice(sd, config, z, pf, g, ns, start)
            for k, v in (("z", z), ("z_p", z_p), ("m_p", m_p), ("logs_p", logs_p), ("m_q", m_q), ("logs_q", logs_q)):
                out[k][b, :, :L] = v[0]
    return {k: v.numpy() for k, v in out.items()}


def kl_loss(z_p, logs_q, m_p, logs_p, z_mask):
    """lib/train/losses.py:596-611 in float64."""
    z_p, logs_q, m_p, logs_p, z_mask = (np.asarray(a, dtype=np.float64) for a in (z_p, logs_q, m_p, logs_p, z_mask))
    kl = logs_p - logs_q - 0.5 + 0.5 * (z_p - m_p) ** 2 * np.exp(-2.0 * logs_p)
    return float(np.sum(kl * z_mask) / np.sum(z_mask))


def l1_loss(a, b):
    return float(np.mean(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))
