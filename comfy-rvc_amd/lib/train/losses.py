"""The trainer's losses on device tensors: the two reconstruction losses (reference lib/train/losses.py:596-611 kl_loss; F.l1_loss as
training_cli.py:570 uses it) and the three GAN losses (:564-593 feature_loss, discriminator_loss, generator_loss).  Each is a fixed-order float64
reduction on the device (rvc_kl_loss per item, rvc_l1_sum; rvc_sqerr_sums / rvc_l1_sums: one segmented reduction over all tensors of a loss) and
returns 0-dim float32 tensors.

One derivative is formed: the gradient of a discriminator-side loss with respect to the input waveform (models._MultiPeriodDiscriminator.input_grad, a
vector-Jacobian product through the discriminators on the device).  gradient_norm_loss (:401-426, the trainer's gradient penalty) and
adversarial_input_grads (the gradients and norms LossBalancer.calculate_gradients reads for loss_gen and loss_fm, :76-92) are built on it.  The same pass
leaves dL / d(pre-activation) of every layer, from which discriminator_grads forms the discriminator step's parameter gradients
(models._MultiPeriodDiscriminator.weight_grad; without the gradient penalty's second-order term).  The optimizer step that consumes them is lib/train/optim.py
(train_step.train_discriminator_step runs the whole discriminator half of an iteration).

The generator half's loss is differentiated as far as the generator's outputs: mel_loss_grad and MultiScaleMelSpectrogramLoss.forward_and_grad return
d loss_mel / d y_hat (mel_processing.mel_spectrogram_vjp behind rvc_mel_loss_cotangents), kl_loss_grads the four cotangents of loss_kl, and LossBalancer is
the reference's class (:14-233) fed those per-loss gradients instead of an autograd graph (train_step.generator_loss_cotangents puts them together).  The
generator's own backward and the gradients of the HPSS / TSI terms are not built.

Also the two generator-side terms the trainer adds on request: MultiScaleMelSpectrogramLoss (:430-561, `hps.train.use_multiscale`) and combined_aux_loss
(:344-399) with its parts compute_harmonics, compute_envelope and compute_tsi_loss.  compute_tefs (the temporal envelope / fine structure term) is not
implemented: combined_aux_loss(c_tefs > 0) raises."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from ... import _lib
from . import mel_processing as MP


def _dev(t):
    if not t.is_cuda:
        raise ValueError("the losses run on the device: pass CUDA tensors (there is no CPU path)")
    return t.detach().to(torch.float32).contiguous()


def _mask_lengths(z_mask, B):
    """int64 [B] on the host: the lengths of a sequence mask [B, 1, T]"""
    mask = z_mask.detach().reshape(B, -1).to("cpu")
    lengths = mask.sum(dim=1).to(torch.int64)
    if not torch.equal(mask, (torch.arange(mask.shape[1])[None, :] < lengths[:, None]).to(mask.dtype)):
        raise ValueError("z_mask must be a sequence mask (ones up to each length, zeros behind)")
    return lengths


def kl_loss(z_p, logs_q, m_p, logs_p, z_mask):
    """z_p, logs_q, m_p, logs_p [B, C, T]; z_mask [B, 1, T], a sequence mask (ones up to each item's length): sum over the unmasked elements of
    logs_p - logs_q - 0.5 + 0.5 (z_p - m_p)^2 exp(-2 logs_p), divided by sum(z_mask)."""
    z_p, logs_q, m_p, logs_p = (_dev(t) for t in (z_p, logs_q, m_p, logs_p))
    B, C, T = z_p.shape
    lengths = _mask_lengths(z_mask, B)
    sums = torch.zeros(B, 2, dtype=torch.float64, device=z_p.device)
    with torch.cuda.device(z_p.device):
        st = _lib.current_stream()
        for b in range(B):
            if int(lengths[b]) > 0:
                _lib.check(_lib.lib.rvc_kl_loss(st, _lib.ptr(z_p[b]), _lib.ptr(logs_q[b]), _lib.ptr(m_p[b]), _lib.ptr(logs_p[b]), C, T, int(lengths[b]),
                                                _lib.ptr(sums[b])))
    tot = sums.sum(dim=0)
    return (tot[0] / tot[1]).to(torch.float32)


def kl_loss_grads(z_p, logs_q, m_p, logs_p, z_mask, scale=1.0):
    """{"z_p", "logs_q", "m_p", "logs_p"} -> d (scale * kl_loss) / d that tensor, each [B, C, T] float32 on the device and exactly 0 behind an item's length
    (rvc_kl_loss_grad, one launch per item)."""
    z_p, logs_q, m_p, logs_p = (_dev(t) for t in (z_p, logs_q, m_p, logs_p))
    B, C, T = z_p.shape
    lengths = _mask_lengths(z_mask, B)
    total = int(lengths.sum())
    out = {k: torch.empty_like(z_p) for k in ("z_p", "logs_q", "m_p", "logs_p")}
    with torch.cuda.device(z_p.device):
        st = _lib.current_stream()
        for b in range(B):
            _lib.check(_lib.lib.rvc_kl_loss_grad(st, _lib.ptr(z_p[b]), _lib.ptr(m_p[b]), _lib.ptr(logs_p[b]), C, T, int(lengths[b]),
                                                 float(scale) / total if total else 0.0, _lib.ptr(out["z_p"][b]), _lib.ptr(out["logs_q"][b]),
                                                 _lib.ptr(out["m_p"][b]), _lib.ptr(out["logs_p"][b])))
    return out


def l1_loss(a, b):
    """mean |a - b| over tensors of one shape."""
    a, b = _dev(a), _dev(b)
    if a.shape != b.shape:
        raise ValueError(f"l1_loss: shapes differ: {tuple(a.shape)} and {tuple(b.shape)}")
    out = torch.zeros(1, dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib.rvc_l1_sum(_lib.current_stream(), _lib.ptr(a), _lib.ptr(b), a.numel(), _lib.ptr(out)))
    return (out[0] / a.numel()).to(torch.float32)


# ------------------------------------------------------------------------------------------------- GAN losses (reference lib/train/losses.py:564-593)
def _segments(tensors):
    ts = [_dev(t) for t in tensors]
    if not ts:
        raise ValueError("no tensors")
    if len(ts) > 64:
        raise ValueError("at most 64 tensors per loss")
    n = (_lib.c_int64 * len(ts))(*[t.numel() for t in ts])
    return ts, (_lib.c_void_p * len(ts))(*[t.data_ptr() for t in ts]), n


def _sqerr_means(tensors, consts):
    """mean (c - x)^2 of every tensor: ONE segmented float64 reduction (rvc_sqerr_sums), float64 [K] on the device."""
    ts, ptrs, n = _segments(tensors)
    c = (_lib.c_float * len(ts))(*consts)
    out = torch.zeros(len(ts), dtype=torch.float64, device=ts[0].device)
    with torch.cuda.device(ts[0].device):
        _lib.check(_lib.lib.rvc_sqerr_sums(_lib.current_stream(), ptrs, n, c, len(ts), _lib.ptr(out)))
    return out / torch.tensor([t.numel() for t in ts], dtype=torch.float64, device=out.device)


def feature_loss(fmap_r, fmap_g):
    """sum over every (real, generated) feature-map pair of mean |r - g| (one segmented reduction, rvc_l1_sums); 0-dim float32."""
    rs, gs = [t for d in fmap_r for t in d], [t for d in fmap_g for t in d]
    if len(rs) != len(gs) or any(r.shape != g.shape for r, g in zip(rs, gs)):
        raise ValueError("feature_loss: the two lists of feature maps differ in structure")
    rs, pr, n = _segments(rs)
    gs, pg, _ = _segments(gs)
    out = torch.zeros(len(rs), dtype=torch.float64, device=rs[0].device)
    with torch.cuda.device(rs[0].device):
        _lib.check(_lib.lib.rvc_l1_sums(_lib.current_stream(), pr, pg, n, len(rs), _lib.ptr(out)))
    means = out / torch.tensor([t.numel() for t in rs], dtype=torch.float64, device=out.device)
    return means.sum().to(torch.float32)


def discriminator_loss(disc_real_outputs, disc_generated_outputs):
    """(sum_i L_i, [L_i]) with L_i = mean (1 - dr_i)^2 + mean dg_i^2; 0-dim float32 tensors."""
    K = len(disc_real_outputs)
    if K != len(disc_generated_outputs):
        raise ValueError("discriminator_loss: lists of different lengths")
    m = _sqerr_means(list(disc_real_outputs) + list(disc_generated_outputs), [1.0] * K + [0.0] * K)
    per = (m[:K] + m[K:]).to(torch.float32)
    return per.sum(), [per[i] for i in range(K)]


def generator_loss(disc_outputs):
    """(sum_i L_i, [L_i]) with L_i = mean (1 - dg_i)^2; 0-dim float32 tensors."""
    per = _sqerr_means(list(disc_outputs), [1.0] * len(disc_outputs)).to(torch.float32)
    return per.sum(), [per[i] for i in range(len(disc_outputs))]


# ------------------------------------------------------------------------------------------------- input gradients (reference lib/train/losses.py:401-426,:76-92)
def _cotangents(kind, a, b, scales):
    """rvc_loss_cotangents over lists of device tensors: one launch, float32 tensors in the shapes of `a`."""
    a, pa, n = _segments(a)
    pb = None
    if b is not None:
        b, pb, _ = _segments(b)
    out = [torch.empty_like(t) for t in a]
    po = (_lib.c_void_p * len(a))(*[t.data_ptr() for t in out])
    sc = (_lib.c_float * len(a))(*scales)
    with torch.cuda.device(a[0].device):
        _lib.check(_lib.lib.rvc_loss_cotangents(_lib.current_stream(), kind, pa, pb, n, sc, len(a), po))
    return out


def _score_cotangents(fmaps, kind):
    """cotangent lists for input_grad with d loss / d score on the last tap of every sub-discriminator: kind 0 for sum mean(s^2), 1 for sum mean((1 - s)^2)"""
    scores = [d[-1] for d in fmaps]
    cots = _cotangents(kind, scores, None, [2.0 / t.numel() for t in scores])
    return [[None] * (len(d) - 1) + [c] for d, c in zip(fmaps, cots)]


def _item_sq_norms(g):
    """float64 [B]: sum of squares of every item of g (rvc_sqerr_sums with c = 0, fixed order)"""
    rows = [g[b] for b in range(g.shape[0])]
    return _sqerr_means(rows, [0.0] * len(rows)) * float(g[0].numel())


def gradient_norm_loss(original_audio, generated_audio, net_d, eps=1e-8, alpha=None, generator=None, return_gradient=False):
    """The trainer's gradient penalty mean_b (||d loss_disc / d x_b||_2 - 1)^2 at x = alpha original + (1 - alpha) generated; 0-dim float32 device tensor.
    alpha [B,1,1] uniform in [0, 1): given, or drawn from `generator` (a CPU torch.Generator; None: the global one - the reference draws it from the global
    generator on the device).  Only the interpolated batch goes through net_d (S = B signals): the real half of the reference's net_d(original,
    interpolated) has no path to the gradient.  eps is unused, as in the reference.  return_gradient: (loss, gradient [B,1,T])."""
    y, y_hat = _dev(original_audio), _dev(generated_audio)
    if y.dim() != 3 or y.shape[1] != 1 or y.shape != y_hat.shape:
        raise ValueError(f"gradient_norm_loss: two [B, 1, T] tensors expected: {tuple(y.shape)} and {tuple(y_hat.shape)}")
    B, T = int(y.shape[0]), int(y.shape[2])
    if alpha is None:
        alpha = torch.rand(B, 1, 1, generator=generator)
    alpha = torch.as_tensor(alpha, dtype=torch.float32)
    if alpha.numel() != B:
        raise ValueError(f"gradient_norm_loss: alpha must be [B, 1, 1] = [{B}, 1, 1]: got {tuple(alpha.shape)}")
    alpha = alpha.reshape(B).to(y.device).contiguous()
    x = torch.empty_like(y)
    with torch.cuda.device(y.device):
        _lib.check(_lib.lib.rvc_interpolate(_lib.current_stream(), _lib.ptr(alpha), _lib.ptr(y), _lib.ptr(y_hat), B, T, _lib.ptr(x)))
    fmaps = net_d.forward_single(x)
    g = net_d.input_grad(fmaps, _score_cotangents(fmaps, 0))
    norms = _item_sq_norms(g).sqrt()
    loss = ((norms - 1.0) ** 2).mean().to(torch.float32)
    return (loss, g) if return_gradient else loss


def adversarial_input_grads(net_d, wave, y_hat, return_losses=False):
    """({"loss_gen": d generator_loss / d y_hat, "loss_fm": d feature_loss / d y_hat}, each [B,1,T] float32, and {"loss_gen": norm, "loss_fm": norm}): the norms
    as LossBalancer.calculate_gradients forms them (per-item 2-norm, mean over the batch), 0-dim float32 device tensors.  One net_d(wave, y_hat) serves both.
    return_losses: a third dict {"loss_gen", "loss_fm"} with generator_loss and feature_loss of the same forward."""
    _, y_d_g, fmap_r, fmap_g = net_d(wave, y_hat)
    fmap_g = [[t.contiguous() for t in d] for d in fmap_g]
    fr, fg = [t for d in fmap_r for t in d], [t for d in fmap_g for t in d]
    it = iter(_cotangents(2, fg, fr, [1.0 / t.numel() for t in fg]))
    grads = {"loss_gen": net_d.input_grad(fmap_g, _score_cotangents(fmap_g, 1)),
             "loss_fm": net_d.input_grad(fmap_g, [[next(it) for _ in d] for d in fmap_g])}
    norms = {k: _item_sq_norms(g).sqrt().mean().to(torch.float32) for k, g in grads.items()}
    if return_losses:
        return grads, norms, {"loss_gen": generator_loss(y_d_g)[0], "loss_fm": feature_loss(fmap_r, fmap_g)}
    return grads, norms


def _mel_cotangents(kind, a, b, log_weight, mag_weight, scales):
    """rvc_mel_loss_cotangents over lists of log-mels (a generated, b target): one launch, float32 tensors in the shapes of `a`."""
    a, pa, n = _segments(a)
    b, pb, _ = _segments(b)
    if len(a) > 8 or any(x.shape != y.shape for x, y in zip(a, b)):
        raise ValueError("mel cotangents: at most 8 pairs of log-mels, each pair of one shape")
    out = [torch.empty_like(t) for t in a]
    po = (_lib.c_void_p * len(a))(*[t.data_ptr() for t in out])
    sc = (_lib.c_float * len(a))(*scales)
    with torch.cuda.device(a[0].device):
        _lib.check(_lib.lib.rvc_mel_loss_cotangents(_lib.current_stream(), len(a), pa, pb, n, _LOSS_KINDS[kind], float(log_weight), float(mag_weight), sc, po))
    return out


def mel_loss_grad(y_mel, y_hat, n_fft, n_mels, sampling_rate, hop_length, win_length, fmin, fmax, return_mel=False):
    """(loss_mel, d loss_mel / d y_hat) for loss_mel = l1_loss(y_mel, mel_spectrogram_torch(y_hat, ...)) (training_cli.py:533-542,:570): y_mel [B, n_mels, frames],
    y_hat [B, 1, T] device tensors; the loss is bit-equal to that expression, the gradient [B, 1, T] float32.  return_mel: also y_hat's log-mel."""
    y_hat_mel = MP.mel_spectrogram_torch(y_hat, n_fft, n_mels, sampling_rate, hop_length, win_length, fmin, fmax)
    loss = l1_loss(y_mel, y_hat_mel)
    gen = _dev(y_hat_mel)
    cot = _mel_cotangents("l1", [gen], [_dev(y_mel)], 1.0, 0.0, [1.0 / gen.numel()])[0]
    grad = MP.mel_spectrogram_vjp(_dev(y_hat), cot, n_fft, n_mels, sampling_rate, hop_length, win_length, fmin, fmax)
    return (loss, grad, y_hat_mel) if return_mel else (loss, grad)


def discriminator_grads(net_d, y, y_hat, c_gp=0.0):
    """(loss_disc, grads): the discriminator step's loss (reference training_cli.py:549-553) and d loss_disc / d(parameter) for every parameter of net_d, what
    loss_disc.backward() leaves in net_d.parameters() (:560).  y, y_hat [B,1,T] device tensors (y_hat is used detached, as the trainer's gen_wave).  ONE
    forward over the 2 B signals, the scores' cotangents from rvc_loss_cotangents (kind 1 on the real rows, kind 0 on the generated rows, scale 2 / numel
    of one half), one input_grad and one weight_grad.  loss_disc is discriminator_loss of those scores (bit-equal); grads is weight_grad's OrderedDict
    (state-dict name -> float32 device tensor, views of one buffer).  net_d must be built with trainable=True.
    The gradient penalty's contribution is NOT built (it needs the second-order term d/dtheta |d loss / d x|): c_gp > 0 raises NotImplementedError."""
    if c_gp and c_gp > 0:
        raise NotImplementedError("discriminator_grads: the gradient penalty's parameter gradient (a second-order term) is not implemented: c_gp must be 0")
    y, y_hat = _dev(y), _dev(y_hat)
    if y.dim() != 3 or y.shape[1] != 1 or y.shape != y_hat.shape:
        raise ValueError(f"discriminator_grads: two [B, 1, T] tensors expected: {tuple(y.shape)} and {tuple(y_hat.shape)}")
    B = int(y.shape[0])
    x = torch.cat([y, y_hat]).contiguous()
    fmaps = net_d.forward_single(x)
    real = [torch.flatten(d[-1][:B], 1, -1) for d in fmaps]
    fake = [torch.flatten(d[-1][B:], 1, -1) for d in fmaps]
    loss_disc, _ = discriminator_loss(real, fake)
    scale = [2.0 / t.numel() for t in real]
    cr, cg = _cotangents(1, real, None, scale), _cotangents(0, fake, None, scale)
    cots = [[None] * (len(d) - 1) + [torch.cat([r, g]).reshape(d[-1].shape)] for d, r, g in zip(fmaps, cr, cg)]
    _, deltas = net_d.input_grad(fmaps, cots, return_deltas=True)
    return loss_disc, net_d.weight_grad(x, fmaps, deltas)


# ------------------------------------------------------------------------------------------------- loss balancer (reference lib/train/losses.py:14-233)
class LossBalancer:
    """The reference's LossBalancer without an autograd graph: the weights of the generator's (or the discriminator's) loss terms, redistributed every batch
    in proportion to each term's gradient norm at the model's output (use_norm) or to the relative change of the loss against its moving average, optionally
    mixed with a Pareto weighting of the moving averages, and smoothed by a moving average of their own.  Host arithmetic on the loss VALUES, step by step as
    the reference (float32 tensors times Python floats; the state dictionaries hold Python / NumPy floats), so a recorded trajectory is reproduced.

    Where the reference differentiates each weighted loss with respect to `input`, on_train_batch_start takes the gradients: input_grads maps a key to
    d(unweighted loss) / d input, [B, 1, T] on the device, or to None; the norm is the per-item 2-norm, mean over the batch, of nan_to_num(weight * gradient,
    epsilon), formed on the device (_item_sq_norms).  grad_norms maps a key to that norm where the caller already holds it.  A key in neither has norm 0 and,
    as every norm <= epsilon, falls back to the loss's relative change - what the reference's materialize_grads=True gives a loss without a path to `input`
    (loss_kl).  With both None the reference's `input=None` path is taken.  `model` is kept for the signature and may be None.
    last_weights: key -> float, the weights of the last balanced sum."""

    def __init__(self, model=None, initial_weights={}, historical_losses={}, ema_weights={}, epsilon=1e-8, weights_decay=0., loss_decay=.0, active=True,
                 use_pareto=True, use_norm=False):
        self.model = model
        self.epsilon = epsilon
        self.weights_decay = weights_decay
        self.loss_decay = loss_decay
        self.initial_weights = initial_weights
        self.ema_weights = ema_weights
        self.historical_losses = historical_losses
        self.active = active
        self.use_pareto = use_pareto
        self.use_norm = use_norm
        self.last_weights = {}

    def to_dict(self):
        return dict(epsilon=self.epsilon, weights_decay=self.weights_decay, loss_decay=self.loss_decay, ema_weights=self.ema_weights,
                    initial_weights=self.initial_weights, historical_losses=self.historical_losses, active=self.active, use_pareto=self.use_pareto,
                    use_norm=self.use_norm)

    def update_ema_weights(self, new_weights):
        if not self.ema_weights:
            self.ema_weights = dict(**new_weights)
        else:
            d = self.weights_decay
            self.ema_weights = {k: np.nan_to_num(d * self.ema_weights.get(k, 1.) + (1 - d) * new_weights[k], nan=self.epsilon) for k in new_weights}
        return dict(**self.ema_weights)

    def update_historical_losses(self, new_losses):
        if not self.historical_losses:
            self.historical_losses = dict(**new_losses)
        else:
            d = self.loss_decay
            for k, v in new_losses.items():
                self.historical_losses[k] = np.nan_to_num(d * self.historical_losses.get(k, v) + (1 - d) * v, nan=self.epsilon)
        return dict(**self.historical_losses)

    def calculate_loss_slope(self, key, current_loss):
        """|current - average| / average of a 0-dim tensor against the loss's moving average (itself when the key is new)"""
        ema_loss = self.historical_losses.get(key, current_loss) + self.epsilon
        return ((current_loss - ema_loss) / ema_loss).abs()

    def calculate_gradients(self, key, current_loss, weight, grad, norm=None):
        """The norm of weight * grad (or `norm`, or 0 without either) as a 0-dim float32 tensor; the loss's slope where that is <= epsilon."""
        if norm is not None:
            grad_norm = torch.tensor(float(norm), dtype=torch.float32)
        elif grad is not None:
            g = (_dev(grad) * weight).nan_to_num(self.epsilon)
            g = g if g.dim() > 1 else g[None]
            grad_norm = _item_sq_norms(g).sqrt().mean().to(torch.float32).cpu()
        else:
            grad_norm = torch.zeros((), dtype=torch.float32)
        if grad_norm <= self.epsilon:
            grad_norm = self.calculate_loss_slope(key, current_loss)
        return grad_norm

    def pareto_normalizer(self, loss_dict, weight=.8):
        """The losses' shares with the largest contributors - those that reach `weight` of the total between them - counted len(losses) times."""
        keys = list(loss_dict.keys())
        losses = np.array(list(loss_dict.values()))
        share = losses / np.sum(losses)
        order = np.argsort(share)[::-1]
        top = np.argmax(np.cumsum(share[order]) >= weight)
        factor = np.ones_like(losses)
        factor[order[:top + 1]] = len(losses)
        out = losses * factor
        out /= np.sum(out) + self.epsilon
        return {keys[i]: out[i] for i in range(len(keys))}

    def redistribute_weights(self, gradients):
        pareto = self.pareto_normalizer(self.historical_losses) if self.use_pareto else {}
        inverse_total = 1. / (sum(gradients.values()) + self.epsilon)
        spare = sum(self.initial_weights.values()) - len(gradients)           # the weight to hand out above 1 per term
        if spare < 0:
            return {k: 1. for k in gradients}
        out = {}
        for k, g in gradients.items():
            ratio = g * inverse_total
            out[k] = 1. + spare * (pareto.get(k, ratio) * .5 + ratio * .5)
        return out

    def on_train_batch_start(self, losses, input_grads=None, grad_norms=None):
        """losses: key -> 0-dim tensor (or a Python number, which is skipped) -> the balanced sum, a 0-dim float32 tensor on the losses' device."""
        self.last_weights = {}
        if len(losses) == 0:
            return 0.
        if not self.initial_weights:
            self.initial_weights = {k: 1. for k in losses}
        if not self.ema_weights:
            self.ema_weights = {k: 1. for k in losses}
        device = next((v.device for v in losses.values() if isinstance(v, torch.Tensor)), torch.device("cpu"))
        host = {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in losses.items()}
        if not self.active:
            self.update_historical_losses({k: v.item() * self.initial_weights.get(k, 1.) for k, v in host.items() if v > 0})
            self.last_weights = {k: float(self.initial_weights.get(k, 1.)) for k in host}
            total = sum(v * self.initial_weights.get(k, 1.) for k, v in host.items())
            return total.to(device) if isinstance(total, torch.Tensor) else total
        with_norm = self.use_norm and (input_grads is not None or grad_norms is not None)
        gradients, valid = {}, {}
        for key, loss in host.items():
            weight = self.initial_weights.get(key, 1.)
            if weight == 0 or loss == 0 or not isinstance(loss, torch.Tensor):
                continue
            weighted = loss * weight
            if with_norm:
                measure = self.calculate_gradients(key, weighted, weight, (input_grads or {}).get(key), (grad_norms or {}).get(key))
            else:
                measure = self.calculate_loss_slope(key, weighted)
            gradients[key] = max(measure.item(), self.epsilon)
            valid[key] = loss.nan_to_num(self.epsilon)
        if not valid or not gradients:
            return torch.tensor(0.0)
        self.update_historical_losses({k: v.item() for k, v in valid.items()})
        weights = self.redistribute_weights(gradients) if len(valid) > 1 else {k: self.initial_weights.get(k, 1.) for k in valid}
        weights = self.update_ema_weights(weights)
        balanced = 0
        for k, v in valid.items():
            balanced += weights.get(k, 1.) * v
        self.last_weights = {k: float(weights.get(k, 1.)) for k in valid}
        return balanced.to(device)

    def on_epoch_end(self, weights_decay=None, loss_decay=None):
        if weights_decay is not None:
            self.weights_decay = weights_decay
        if loss_decay is not None:
            self.loss_decay = loss_decay
        weights = dict(sorted(self.ema_weights.items(), key=lambda kv: kv[1], reverse=True))
        losses = dict(sorted(self.historical_losses.items(), key=lambda kv: kv[1], reverse=True))
        print(f"|| EMA weights: {weights} ({self.weights_decay=})")
        print(f"|| EMA losses: {losses} ({self.loss_decay=})")
        print(f"===> Weighted EMA loss: {self.weighted_ema_loss:.3f} <====")

    @property
    def weighted_ema_loss(self):
        return sum(v * self.ema_weights.get(k, 1.) for k, v in self.historical_losses.items())


# ------------------------------------------------------------------------------------------------- multi-scale mel loss (reference lib/train/losses.py:430-561)
STFTParams = namedtuple("STFTParams", ["window_length", "hop_length"])
_LOSS_KINDS = {"l1": 0, "l2": 1, "smoothl1": 2}


class MultiScaleMelSpectrogramLoss:
    """The reference's class on the device; forward_and_grad adds the gradient at its first argument.  x and y go through each STFT together (2 B rows in one launch, one STFT per distinct window
    length), then one kernel per scale projects both spectrograms, forms the pointwise loss and reduces it in float64; the log-mels are never stored.
    Launches per call: (distinct window lengths) + (scales) + 1 = 4 + 6 + 1 = 11 with the default n_mels, whatever B and T."""

    def __init__(self, sampling_rate, n_mels=[20, 64, 80, 128, 160, 256], loss="l1", epsilon=1e-8, mag_weight=0.0, log_weight=1.0, adjustment_factor=0.0,
                 fmin=50., fmax=None, center=False, **kwargs):
        if loss not in _LOSS_KINDS:
            raise ValueError(f"loss must be one of {sorted(_LOSS_KINDS)}: {loss!r}")
        self.sampling_rate = sampling_rate
        window_lengths = [self.compute_window_length(mel, sampling_rate) for mel in n_mels]      # in the order GIVEN; n_mels itself is sorted (reference quirk)
        self.stft_params = [STFTParams(window_length=w, hop_length=sampling_rate // 100) for w in window_lengths]
        self.n_mels = sorted(n_mels)
        self.loss = loss
        self.epsilon = epsilon
        self.log_weight = log_weight
        self.mag_weight = mag_weight
        self.center = center
        if fmax is None:
            fmax = sampling_rate // 2
        self.fmax = fmax
        self.fmin = fmin
        self.mel_fmin = [fmin for _ in n_mels]
        self.mel_fmax = [fmax for _ in n_mels]
        self.adjustment_factor = adjustment_factor
        self.frequency_buffer = int(sampling_rate * adjustment_factor) + 1
        self.window_lengths = window_lengths
        for k, v in kwargs.items():                  # a to_dict() result restores mel_fmin / mel_fmax here
            setattr(self, k, v)
        self.scale_losses = None                     # the last forward's per-scale losses (float32 device tensor [scales])

    def to_dict(self):
        return dict(sampling_rate=self.sampling_rate, n_mels=self.n_mels, loss=self.loss, epsilon=self.epsilon, mag_weight=self.mag_weight,
                    log_weight=self.log_weight, adjustment_factor=self.adjustment_factor, fmin=self.fmin, fmax=self.fmax, center=self.center,
                    mel_fmin=self.mel_fmin, mel_fmax=self.mel_fmax)

    def show_freqs(self):
        print("MultiScaleMelSpectrogramLoss:\n\tn_mels \twindow \tfmin \tfmax")
        for i in range(len(self.mel_fmax)):
            print(f"\t{self.n_mels[i]} \t{self.window_lengths[i]} \t{self.mel_fmin[i]:.0f} \t{self.mel_fmax[i]:.0f}")

    @staticmethod
    def compute_window_length(n_mels, sample_rate):
        """The largest power of two not above 8 n_mels / (sample_rate / 2) seconds: 2^floor(log2(16 n_mels)) samples at every rate."""
        window_length = int(8 * n_mels / (sample_rate / 2 - 0) * sample_rate)
        return 2 ** (window_length.bit_length() - 1)

    def adjust_fmin_fmax(self, scale_losses):
        """Moves every scale's band by at most adjustment_factor, relatively: host arithmetic on the per-scale losses, step by step as the reference."""
        median_loss = np.nanmedian(scale_losses)
        cumloss = np.cumsum(scale_losses)
        cutoff_index = np.argmax(cumloss >= median_loss * len(scale_losses))
        median_low = np.nanmedian(scale_losses[:cutoff_index])
        median_high = np.nanmedian(scale_losses[cutoff_index:])
        for i, scale_loss in enumerate(scale_losses):
            high = i >= cutoff_index
            threshold = median_high if high else median_low
            deviation = (scale_loss - threshold) / (threshold + self.epsilon)
            adjustment = min(abs(self.adjustment_factor * deviation), self.adjustment_factor)
            if high:
                self.mel_fmax[i] = min(self.mel_fmax[i] * (1 + adjustment), self.fmax)
                if deviation > self.epsilon:
                    self.mel_fmin[i] = min(self.mel_fmin[i] * (1 + adjustment), self.mel_fmax[i] - self.frequency_buffer)
                elif deviation < -self.epsilon:
                    self.mel_fmin[i] = max(self.mel_fmin[i] * (1 - adjustment), self.fmin)
            else:
                self.mel_fmin[i] = max(self.mel_fmin[i] * (1 - adjustment), self.fmin)
                if deviation > self.epsilon:
                    self.mel_fmax[i] = min(self.mel_fmax[i] * (1 + adjustment), self.fmax)
                elif deviation < -self.epsilon:
                    self.mel_fmax[i] = max(self.mel_fmax[i] * (1 - adjustment), self.mel_fmin[i] + self.frequency_buffer)

    def _scales(self, x, y):
        """(per-scale losses [K] float32 on the device, the packed spectrograms per scale, both waves [2 B, T], frames): everything forward computes"""
        if self.center:
            raise NotImplementedError("center=True is not implemented (the reference never passes it)")
        x, y = _dev(x), _dev(y)
        if x.shape != y.shape or x.dim() != 3:
            raise ValueError(f"MultiScaleMelSpectrogramLoss: [B, C, T] tensors of one shape expected: {tuple(x.shape)} and {tuple(y.shape)}")
        T = x.shape[-1]
        both = torch.cat([x.reshape(-1, T), y.reshape(-1, T)], dim=0)
        B, K = both.shape[0] // 2, len(self.n_mels)
        hop = self.stft_params[0].hop_length
        dev_index = MP._dev_index(both)
        specs = {}
        with torch.cuda.device(both.device):
            for s in self.stft_params:
                if s.window_length not in specs:
                    specs[s.window_length] = MP.rows_spectrogram_packed(both, s.window_length, s.hop_length, 0.0, False)
            for n_mels, fmin, fmax, s in zip(self.n_mels, self.mel_fmin, self.mel_fmax, self.stft_params):
                MP.ensure_bank(dev_index, s.window_length, n_mels, self.sampling_rate, fmin, fmax)
            nf = MP.frames_of(T, hop)
            per = [specs[s.window_length] for s in self.stft_params]
            ptrs = (_lib.c_void_p * K)(*[p[0].data_ptr() for p in per])
            pitch = (_lib.c_int64 * K)(*[p[0].shape[1] for p in per])
            stride = (_lib.c_int64 * K)(*[p[2] for p in per])
            n_fft = (ctypes.c_int32 * K)(*[s.window_length for s in self.stft_params])
            n_mel = (ctypes.c_int32 * K)(*self.n_mels)
            sums = torch.zeros(K, 2, dtype=torch.float64, device=both.device)
            _lib.check(_lib.lib.rvc_multiscale_mel_loss(_lib.get_ctx(dev_index), _lib.current_stream(), K, ptrs, pitch, stride, B, nf, n_fft, n_mel,
                                                        _LOSS_KINDS[self.loss], int(self.mag_weight > 0), _lib.ptr(sums)))
        count = torch.tensor([B * m * nf for m in self.n_mels], dtype=torch.float64, device=sums.device)
        means = (sums / count[:, None]).to(torch.float32)                    # the reference's loss_fn results, float32
        scale = torch.zeros(K, dtype=torch.float32, device=sums.device)
        if self.log_weight > 0:
            scale = scale + self.log_weight * means[:, 0]
        if self.mag_weight > 0:
            scale = scale + self.mag_weight * means[:, 1]
        self.scale_losses = scale
        return scale, per, both, nf

    def forward(self, x, y):
        """x, y [B, 1, T] device tensors -> the mean over the scales of log_weight * loss(log-mels) + mag_weight * loss(exp(log-mels)), 0-dim float32."""
        scale = self._scales(x, y)[0]
        if self.adjustment_factor > 0:
            self.adjust_fmin_fmax([float(v) for v in scale.tolist()])
        return scale.sum() / len(self.n_mels)

    def forward_and_grad(self, x, y, return_mels=False):
        """(loss, d loss / d x) with x the first argument, as the trainer calls MultiscaleMelLoss(y_hat, wave): loss is forward(x, y) bit for bit (the same
        launches), the gradient has x's shape, float32.  adjust_fmin_fmax runs after both, so the gradient belongs to the bands the loss used.
        On top of the forward's launches (one STFT per distinct window length W, K + 1 for the K scales' losses) the log-mels of both signals are stored -
        they are small - and differentiated: K projections, K copies that split them into the two signals, 1 launch for all cotangents
        (rvc_mel_loss_cotangents), 2 K for the vector-Jacobian products (rvc_mel_spectrogram_vjp per scale) and 1 sum over the scales:
        W + 5 K + 3 = 37 launches with the default n_mels (W = 4, K = 6), whatever B and T.
        return_mels: also [(log-mel of x, log-mel of y)] per scale, each [n_mels, B, frames]."""
        scale, per, both, nf = self._scales(x, y)
        B, K = both.shape[0] // 2, len(self.n_mels)
        T = both.shape[1]
        gen, tgt = [], []
        with torch.cuda.device(both.device):
            for n_mels, fmin, fmax, s, (spec, _, nfa) in zip(self.n_mels, self.mel_fmin, self.mel_fmax, self.stft_params, per):
                cols = np.array([(r * nfa, nf) for r in range(2 * B)], dtype=np.int64)
                mel = MP.mel_packed(spec, cols, s.window_length, n_mels, self.sampling_rate, fmin, fmax)      # (the alignment columns stay unwritten and unread)
                halves = mel.view(n_mels, 2, B * nfa).permute(1, 0, 2).contiguous()
                gen.append(halves[0])
                tgt.append(halves[1])
            cots = _mel_cotangents(self.loss, gen, tgt, self.log_weight, self.mag_weight, [1.0 / (K * B * m * nf) for m in self.n_mels])
            grads = torch.empty(K, B, T, device=both.device, dtype=torch.float32)
            for k, (n_mels, fmin, fmax, s, (_, _, nfa)) in enumerate(zip(self.n_mels, self.mel_fmin, self.mel_fmax, self.stft_params, per)):
                MP.mel_vjp_packed(both[:B].reshape(-1), np.array([(r * T, T, r * nfa) for r in range(B)], dtype=np.int64), cots[k], s.window_length,
                                  s.hop_length, 0.0, False, n_mels, self.sampling_rate, fmin, fmax, out=grads[k].view(-1))
            grad = grads.sum(dim=0).view(x.shape)
        if self.adjustment_factor > 0:
            self.adjust_fmin_fmax([float(v) for v in scale.tolist()])
        loss = scale.sum() / K
        if return_mels:
            return loss, grad, [(g.view(g.shape[0], B, -1)[:, :, :nf], t.view(t.shape[0], B, -1)[:, :, :nf]) for g, t in zip(gen, tgt)]
        return loss, grad

    __call__ = forward


# ------------------------------------------------------------------------------------------------- auxiliary losses (reference lib/train/losses.py:235-399)
HPSS_KERNEL_SIZES = (3, 7, 13, 19, 29)


def _mag3(t, name):
    t = _dev(t)
    if t.dim() != 3:
        raise ValueError(f"{name}: a [B, n_mels, T] tensor expected, got {tuple(t.shape)}")
    return t


def _hpss_check(F, T):
    if F <= 14 or T <= 14:
        raise ValueError(f"compute_harmonics: both spectrogram axes must be longer than 14 (the largest median window is 29): got {F} x {T}")


def hpss_parts(mag, medians=False):
    """mag [B, n_mels, T] float32 device tensor -> (harmonic, percussive) [B, n_mels, 5 T] before the min-max scaling: |mag| times its soft masks for the
    kernel sizes 3 | 7 | 13 | 19 | 29 side by side (rvc_hpss, one launch).  medians: the median along time and the median along mel instead."""
    B, F, T = mag.shape
    _hpss_check(F, T)
    h = torch.empty(B, F, 5 * T, dtype=torch.float32, device=mag.device)
    p = torch.empty_like(h)
    with torch.cuda.device(mag.device):
        _lib.check(_lib.lib.rvc_hpss(_lib.current_stream(), _lib.ptr(mag), B, F, T, _lib.ptr(h), _lib.ptr(p), int(bool(medians))))
    return h, p


def compute_harmonics(mag, kernel_sizes=HPSS_KERNEL_SIZES, eps=1e-8):
    """mag [B, n_mels, T] -> (harmonic, percussive), each [B, n_mels, 5 T]: librosa.decompose.hpss(|mag|, kernel_size=k) for k = 3, 7, 13, 19, 29 side by
    side along the last axis (rvc_hpss, one launch), then each tensor min-max scaled by its own global extremes and nan_to_num(eps)."""
    if tuple(kernel_sizes) != HPSS_KERNEL_SIZES:
        raise NotImplementedError(f"compute_harmonics: the kernel sizes are fixed to {HPSS_KERNEL_SIZES}")
    h, p = hpss_parts(_mag3(mag, "compute_harmonics"))
    out = []
    for t in (h, p):
        mn, mx = t.min(), t.max()
        out.append(((t - mn) / (mx - mn + eps)).nan_to_num(eps))
    return out[0], out[1]


def harmonic_loss(org_mag, gen_mag, eps=1e-8):
    """L1(gen harmonic, org harmonic) + L1(gen percussive, org percussive) of compute_harmonics' tensors without forming them (rvc_hpss_l1: one min / max
    reduction, one scaled-L1 reduction in float64); 0-dim float32."""
    org_mag, gen_mag = _mag3(org_mag, "harmonic_loss"), _mag3(gen_mag, "harmonic_loss")
    if org_mag.shape != gen_mag.shape:
        raise ValueError(f"harmonic_loss: shapes differ: {tuple(org_mag.shape)} and {tuple(gen_mag.shape)}")
    B, F, T = org_mag.shape
    _hpss_check(F, T)
    sums = torch.zeros(2, dtype=torch.float64, device=org_mag.device)
    with torch.cuda.device(org_mag.device):
        _lib.check(_lib.lib.rvc_hpss_l1(_lib.current_stream(), _lib.ptr(org_mag), _lib.ptr(gen_mag), B, F, T, float(eps), _lib.ptr(sums)))
    means = (sums / float(B * F * 5 * T)).to(torch.float32)
    return means[0] + means[1]


def compute_envelope(log_magnitude, dim=-1, kernel_size=3, eps=1e-8):
    """[B, n_mels, T] -> the envelope summed along dim: L2-normalise along dim, max over three neighbours along the LAST axis (whatever dim is, as the
    reference's max_pool1d), nan_to_num(eps), sum along dim.  Host-side plumbing of the public name only: compute_tsi_loss runs rvc_tsi_terms."""
    if kernel_size != 3:
        raise NotImplementedError("compute_envelope: kernel_size is fixed to 3")
    x = _mag3(log_magnitude, "compute_envelope")
    x = torch.nn.functional.normalize(x, dim=dim, eps=eps)
    return torch.nn.functional.max_pool1d(x, kernel_size=3, stride=1, padding=1).nan_to_num(eps).sum(dim)


def _tsi_terms(org, gen, eps):
    org, gen = _mag3(org, "compute_tsi_loss"), _mag3(gen, "compute_tsi_loss")
    if org.shape != gen.shape:
        raise ValueError(f"compute_tsi_loss: shapes differ: {tuple(org.shape)} and {tuple(gen.shape)}")
    B, F, T = org.shape
    out = torch.zeros(2, B, dtype=torch.float64, device=org.device)
    with torch.cuda.device(org.device):
        _lib.check(_lib.lib.rvc_tsi_terms(_lib.current_stream(), _lib.ptr(org), _lib.ptr(gen), B, F, T, float(eps), _lib.ptr(out)))
    return out.to(torch.float32).mean(dim=1)


def compute_tsi_loss(original_log_magnitude, generated_log_magnitude, dim=-1, eps=1e-8):
    """mean over the batch of 1 - Pearson correlation of the two envelopes (rvc_tsi_terms, one launch); 0-dim float32."""
    if dim not in (-1, -2, 1, 2):
        raise ValueError(f"compute_tsi_loss: dim must be -1 or -2: {dim}")
    return _tsi_terms(original_log_magnitude, generated_log_magnitude, eps)[0 if dim in (-1, 2) else 1]


def combined_aux_loss(original_audio, generated_audio, c_tefs=1., c_hd=1., c_tsi=1., n_mels=128, sample_rate=40000, n_fft=1024, hop_length=320,
                      win_length=1024, fmin=0, fmax=None, eps=None):
    """(harmonic_loss, tefs_loss, tsi_loss) of [B, 1, T] device waves as the trainer forms them; a term whose coefficient is 0 is the Python 0.  Both waves go
    through ONE STFT and ONE mel projection.  The temporal envelope / fine structure term is not implemented: c_tefs > 0 raises."""
    if c_tefs > 0:
        raise NotImplementedError("tefs_loss (compute_tefs, the temporal envelope / fine structure term) is not implemented: pass c_tefs=0")
    if eps is None:
        eps = torch.finfo(original_audio.dtype).eps
    harmonic, tsi = 0, 0
    if c_hd + c_tsi > 0:
        if not original_audio.is_cuda or not generated_audio.is_cuda:
            raise ValueError("the losses run on the device: pass CUDA tensors (there is no CPU path)")
        if original_audio.shape != generated_audio.shape or original_audio.dim() != 3:
            raise ValueError("combined_aux_loss: [B, C, T] tensors of one shape expected")
        both = torch.cat([_dev(original_audio), _dev(generated_audio)], dim=0)
        mag = MP.mel_spectrogram_torch(both, n_fft, n_mels, sample_rate, hop_length, win_length, fmin, fmax)
        R = mag.shape[0] // 2
        org_mag, gen_mag = mag[:R].contiguous(), mag[R:].contiguous()
        if c_hd > 0:
            harmonic = harmonic_loss(org_mag, gen_mag, eps=eps)
        if c_tsi > 0:
            terms = _tsi_terms(org_mag, gen_mag, eps)
            tsi = terms[0] + terms[1]
    return harmonic, 0, tsi
