"""loss/mel and loss/kl of a generator checkpoint over a prepared dataset - the two numbers watched to pick an epoch - from the training forward alone
(no backward pass), formed as the trainer forms them (reference training_cli.py:505-545,:570-571).  With the discriminator checkpoint that the trainer
writes next to it (D_*.pth) also the three adversarial numbers it logs, loss_disc, loss_gen and loss_fm (:545-553,:567-572,:585).  The trainer's
switches are followed: with hps.train.use_multiscale loss_mel is MultiScaleMelSpectrogramLoss(y_hat, wave) (:569), with hps.train.c_hd / c_tsi > 0 the
harmonic_loss / tsi_loss of combined_aux_loss (:573-584) are added, with hps.train.c_gp > 0 and a discriminator the gradient penalty (:552), the one
term here that needs a derivative (the discriminators' input gradient, losses.gradient_norm_loss)."""
import numpy as np
import torch

from ..infer_pack import models
from ..infer_pack.commons import clip_grad_value_
from . import data_utils
from .losses import (MultiScaleMelSpectrogramLoss, combined_aux_loss, discriminator_grads, discriminator_loss, feature_loss, generator_loss,
                     gradient_norm_loss, kl_loss, l1_loss)
from .mel_processing import mel_spectrogram_torch, spec_to_mel_torch


def _slice_segments(x, ids, size):
    """commons.slice_segments (reference lib/infer_pack/commons.py:150-156)."""
    return torch.stack([x[i, :, int(s):int(s) + size] for i, s in enumerate(ids.tolist())])


def _train_get(hps, key, default=0.):
    """hps.train.get(key, default) for an HParams or a plain namespace."""
    tr = hps.train
    return tr.get(key, default) if hasattr(tr, "get") else getattr(tr, key, default)


def multiscale_state(hps, ckpt=None):
    """The MultiScaleMelSpectrogramLoss an evaluation uses: the state the trainer saved with the generator (the checkpoint's "msml" entry, its mel_fmin /
    mel_fmax as saved), else the trainer's fresh one (defaults, epsilon = hps.train.eps).  adjustment_factor is 0 in both: evaluation does not move the bands."""
    saved = ckpt.get("msml") if isinstance(ckpt, dict) else None
    if saved:
        return MultiScaleMelSpectrogramLoss(**{**saved, "adjustment_factor": 0.0})
    return MultiScaleMelSpectrogramLoss(hps.data.sampling_rate, epsilon=_train_get(hps, "eps", 1e-8), adjustment_factor=0.0)


def reconstruction_losses(net_g, batch, hps, generator=None, *, noise=None, ids_slice=None, return_y_hat=False, msml=None):
    """One collated batch (TextAudioCollateMultiNSFsid's nine tensors, or TextAudioCollate's seven) -> {"loss_mel", "loss_kl": 0-dim float32 device tensors,
    "ids_slice": int64 [B]}.  Noise and slice starts are drawn from `generator` (a CPU torch.Generator; None: the global one) in the forward's order;
    noise / ids_slice given explicitly (as to the forward) replace the draws.  return_y_hat: the generated segments [B,1,segment_size] are added as "y_hat".
    hps.train.use_multiscale: loss_mel is msml(y_hat, sliced wave) (msml None: multiscale_state(hps)); hps.train.c_hd / c_tsi > 0: "harmonic_loss" /
    "tsi_loss" of combined_aux_loss(sliced wave, y_hat) are added.  With none of the three set nothing changes."""
    d, seg = hps.data, hps.train.segment_size // hps.data.hop_length
    if len(batch) == 9:
        phone, phone_lengths, pitch, pitchf, spec, spec_lengths, _wave, _wl, sid = batch
    else:
        phone, phone_lengths, spec, spec_lengths, _wave, _wl, sid = batch
        pitch = pitchf = None
    B, T = spec.shape[0], spec.shape[2]
    yl = torch.as_tensor(spec_lengths).reshape(-1).cpu()
    if noise is not None:
        noise_q, noise_src = noise if isinstance(noise, (tuple, list)) else (noise, None)
        ids = ids_slice if ids_slice is not None else (torch.rand([B], generator=generator) * (yl - seg + 1)).to(dtype=torch.long)
    else:
        noise_q = torch.randn(B, net_g.inter_channels, T, generator=generator)
        ids = (torch.rand([B], generator=generator) * (yl - seg + 1)).to(dtype=torch.long)
        if pitch is not None:
            torch.rand(B, 1, generator=generator)
            noise_src = torch.randn(B, seg * net_g.upp, 1, generator=generator)
        if ids_slice is not None:
            ids = ids_slice
    if pitch is not None:
        y_hat, ids_slice, _, z_mask, (_z, z_p, m_p, logs_p, _m_q, logs_q) = net_g(phone, phone_lengths, pitch, pitchf, spec, spec_lengths, sid,
                                                                                  noise=(noise_q, noise_src), ids_slice=ids)
    else:
        y_hat, ids_slice, _, z_mask, (_z, z_p, m_p, logs_p, _m_q, logs_q) = net_g(phone, phone_lengths, spec, spec_lengths, sid, noise=noise_q, ids_slice=ids)
    dev = y_hat.device
    mel = spec_to_mel_torch(spec.to(dev, torch.float32), d.filter_length, d.n_mel_channels, d.sampling_rate, d.mel_fmin, d.mel_fmax)
    y_mel = _slice_segments(mel, ids_slice, seg)
    y_hat_mel = mel_spectrogram_torch(y_hat, d.filter_length, d.n_mel_channels, d.sampling_rate, d.hop_length, d.win_length, d.mel_fmin, d.mel_fmax)
    multiscale, c_hd, c_tsi = bool(_train_get(hps, "use_multiscale", False)), _train_get(hps, "c_hd", 0.), _train_get(hps, "c_tsi", 0.)
    if multiscale or c_hd > 0 or c_tsi > 0:
        wave = _slice_segments(torch.as_tensor(_wave).to(dev, torch.float32), torch.as_tensor(ids_slice).reshape(-1).cpu() * int(d.hop_length),
                               int(y_hat.shape[-1]))
    if multiscale:
        loss_mel = (msml if msml is not None else multiscale_state(hps))(y_hat, wave)
    else:
        loss_mel = l1_loss(y_mel, y_hat_mel)
    out = {"loss_mel": loss_mel, "loss_kl": kl_loss(z_p, logs_q, m_p, logs_p, z_mask), "ids_slice": ids_slice}
    if c_hd > 0 or c_tsi > 0:
        harmonic, _, tsi = combined_aux_loss(wave, y_hat, c_tefs=0., c_hd=c_hd, c_tsi=c_tsi, n_mels=d.n_mel_channels, sample_rate=d.sampling_rate,
                                             n_fft=d.filter_length, hop_length=d.hop_length, win_length=d.win_length, fmin=d.mel_fmin, fmax=d.mel_fmax,
                                             eps=_train_get(hps, "eps", None))
        if c_hd > 0:
            out["harmonic_loss"] = harmonic
        if c_tsi > 0:
            out["tsi_loss"] = tsi
    if return_y_hat:
        out["y_hat"] = y_hat
    return out


def adversarial_losses(net_d, wave, y_hat, ids_slice=None, hps=None, generator=None, grad_norm=False):
    """loss_disc, loss_gen, loss_fm of one batch as the trainer forms them (reference training_cli.py:545-553,:567-572,:585): wave [B,1,Tw] the real waves,
    sliced to y_hat's segments at ids_slice * hop_length when ids_slice is given (wave already sliced otherwise), y_hat [B,1,segment_size].  One
    net_d(wave, y_hat) serves all three: without a backward pass the trainer's two calls compute the same.  0-dim float32 device tensors.
    hps.train.c_gp > 0: "gradient_penalty" = gradient_norm_loss(wave, y_hat, net_d) * c_gp is added, the term the trainer adds to loss_disc (:552), its alpha
    drawn from `generator` (a CPU torch.Generator; None: the global one).  loss_disc itself stays the plain discriminator loss.
    grad_norm: "grad_norm_d" is added, the number the trainer logs for the discriminator step (:562): clip_grad_value_ over d loss_disc / d(parameter)
    (losses.discriminator_grads) with batch_size = hps.train.batch_size and no clipping, a Python float.  net_d must be trainable; with c_gp > 0 the
    penalty's second-order term would be part of it, which is not built: NotImplementedError."""
    y_hat = y_hat.detach()
    wave = torch.as_tensor(wave).to(y_hat.device, torch.float32)
    if ids_slice is not None:
        wave = _slice_segments(wave, torch.as_tensor(ids_slice).reshape(-1).cpu() * int(hps.data.hop_length), int(y_hat.shape[-1]))
    y_d_r, y_d_g, fmap_r, fmap_g = net_d(wave, y_hat)
    loss_disc, _ = discriminator_loss(y_d_r, y_d_g)
    loss_gen, _ = generator_loss(y_d_g)
    out = {"loss_disc": loss_disc, "loss_gen": loss_gen, "loss_fm": feature_loss(fmap_r, fmap_g)}
    c_gp = _train_get(hps, "c_gp", 0.) if hps is not None else 0.
    if c_gp > 0:
        out["gradient_penalty"] = gradient_norm_loss(wave, y_hat, net_d, eps=_train_get(hps, "eps", 1e-8), generator=generator) * c_gp
    if grad_norm:
        _, grads = discriminator_grads(net_d, wave, y_hat, c_gp=c_gp)
        out["grad_norm_d"] = clip_grad_value_(grads.values(), None, batch_size=int(_train_get(hps, "batch_size", 1)) if hps is not None else 1)
    return out


def load_generator(ckpt, hps, version="v2", f0=True, device="cuda:0"):
    """A trainer's G_*.pth ({"model": state_dict, "iteration", ...}, reference lib/train/utils.py:120-131) or a bare state dict -> the loaded synthesizer."""
    cpt = torch.load(ckpt, map_location="cpu") if isinstance(ckpt, str) else ckpt
    sd = cpt["model"] if isinstance(cpt, dict) and "model" in cpt else cpt
    m = hps.model
    cls = getattr(models, f"SynthesizerTrnMs{768 if version == 'v2' else 256}NSFsid" + ("" if f0 else "_nono"))
    net = cls(hps.data.filter_length // 2 + 1, hps.train.segment_size // hps.data.hop_length, m.inter_channels, m.hidden_channels, m.filter_channels,
              m.n_heads, m.n_layers, m.kernel_size, m.p_dropout, m.resblock, m.resblock_kernel_sizes, m.resblock_dilation_sizes, m.upsample_rates,
              m.upsample_initial_channel, m.upsample_kernel_sizes, m.spk_embed_dim, m.gin_channels, hps.data.sampling_rate, device=device)
    net.load_state_dict(sd)
    return net


def load_discriminator(ckpt, version="v2", device="cuda:0", trainable=False):
    """A trainer's D_*.pth ({"model": state_dict, ...}, reference lib/train/utils.py:120-131) or a bare state dict -> the loaded discriminators
    (MultiPeriodDiscriminatorV2 for "v2", MultiPeriodDiscriminator for "v1": training_cli.py picks them by version).  trainable: weight_v / weight_g stay
    on the device, so that the parameter gradients can be formed (grad_norm_d)."""
    cpt = torch.load(ckpt, map_location="cpu") if isinstance(ckpt, str) else ckpt
    sd = cpt["model"] if isinstance(cpt, dict) and "model" in cpt else cpt
    cls = models.MultiPeriodDiscriminatorV2 if version == "v2" else models.MultiPeriodDiscriminator
    return cls(False, device=device, trainable=trainable).load_state_dict(sd)


def evaluate_checkpoint(ckpt, filelist, hps, seed=1337, batch_size=4, boundaries=(32, 100, 200, 300, 400, 500, 600, 700, 800, 900), version="v2", f0=True,
                        device="cuda:0", ckpt_d=None, grad_norm=False):
    """Walks `filelist` through the loader, the collate and the bucket sampler (unshuffled) and returns {"loss_mel", "loss_kl": means over the batches,
    "batches": [{"loss_mel", "loss_kl", "ids_slice"}...]}.  The sampler buckets by file size (dataset.lengths), so a batch may still hold an item whose
    labels are shorter than the segment: such a batch cannot be sliced and is left out.  The draws come from torch.Generator().manual_seed(seed): the same seed gives the same two numbers.
    ckpt_d (a D_*.pth path, a state dict or loaded discriminators): loss_disc, loss_gen and loss_fm are added per batch and as means; None: nothing changes.
    With ckpt_d and hps.train.c_gp > 0 also gradient_penalty (the penalty times c_gp, as the trainer adds it), its alpha drawn from the walk's generator after
    the batch's forward draws; with c_gp absent or 0 no draw is made and the result is what it was.
    grad_norm (needs ckpt_d): also grad_norm_d per batch and as a mean, the trainer's logged gradient norm of the discriminator step; the discriminators are
    then loaded trainable (loaded ones must have been).
    hps.train.use_multiscale / c_hd / c_tsi as in reconstruction_losses; the multi-scale state is the checkpoint's "msml" entry when ckpt is a path or a
    checkpoint dict that has one."""
    cpt = torch.load(ckpt, map_location="cpu") if isinstance(ckpt, str) else ckpt
    msml = multiscale_state(hps, cpt) if _train_get(hps, "use_multiscale", False) else None
    net = cpt if hasattr(cpt, "forward") else load_generator(cpt, hps, version, f0, device)
    net_d = None if ckpt_d is None else (ckpt_d if hasattr(ckpt_d, "forward") else load_discriminator(ckpt_d, version, device, trainable=grad_norm))
    seg = hps.train.segment_size // hps.data.hop_length
    ds = (data_utils.TextAudioLoaderMultiNSFsid if f0 else data_utils.TextAudioLoader)(filelist, hps.data)
    collate = data_utils.TextAudioCollateMultiNSFsid() if f0 else data_utils.TextAudioCollate()
    bounds = list(boundaries)
    sampler = data_utils.BucketSampler(ds, batch_size, bounds, shuffle=False)
    gen = torch.Generator().manual_seed(int(seed))
    rows = []
    for idx in sampler:
        batch = collate([ds[i] for i in idx])
        lens = batch[5 if f0 else 3]
        if int(lens.min()) < seg:
            continue
        r = reconstruction_losses(net, batch, hps, gen, return_y_hat=net_d is not None, msml=msml)
        row = {"loss_mel": float(r["loss_mel"]), "loss_kl": float(r["loss_kl"]), "ids_slice": r["ids_slice"].cpu().numpy()}
        row.update({k: float(r[k]) for k in ("harmonic_loss", "tsi_loss") if k in r})
        if net_d is not None:
            adv = adversarial_losses(net_d, batch[6 if f0 else 4], r["y_hat"], r["ids_slice"], hps, generator=gen, grad_norm=grad_norm)
            row.update({k: float(v) for k, v in adv.items()})
        rows.append(row)
    if not rows:
        raise ValueError("no batch of the file list has every item at least segment_size long")
    names = ["loss_mel", "loss_kl"] + (["loss_disc", "loss_gen", "loss_fm"] if net_d is not None else [])
    names += [k for k in ("gradient_penalty", "grad_norm_d", "harmonic_loss", "tsi_loss") if k in rows[0]]
    out = {k: float(np.mean([r[k] for r in rows])) for k in names}
    out["batches"] = rows
    return out
