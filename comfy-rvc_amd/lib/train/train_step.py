"""The discriminator half of one trainer iteration on the device (reference training_cli.py:549-563): forward, discriminator_loss, backward,
clip_grad_value_, optim_d.step().  fp32 only: the reference's GradScaler with fp16_run off is the identity, and autocast is not implemented.  The gradient
penalty's parameter gradient is not built: c_gp > 0 raises (losses.discriminator_grads).

Of the generator half (:565-601) the loss and its cotangents at the generator's outputs: generator_loss_cotangents; and the first step of the generator's own
backward, the decoder's data pass from d_y_hat to the sliced latent's, the speaker conditioning's and the harmonic source's cotangents:
generator_decoder_backward over a net_g.forward_with_tape(...) pass; and its second step, the gradient of every dec.* parameter (weight norm included) from the
deltas that pass leaves: generator_decoder_grads; its third step, the flow's data pass from the KL loss's cotangent at z_p: generator_flow_backward; and its
fourth, the gradient of every flow.* parameter from the deltas that pass leaves: generator_flow_grads.  The backward of enc_q, enc_p and emb_g, grad_norm_g, the
generator's optimizer step and the gradients of the HPSS / TSI / TEFS terms are not built."""
import torch

from ..infer_pack.commons import clip_grad_value_
from .evaluate import _train_get, multiscale_state
from .losses import adversarial_input_grads, discriminator_grads, kl_loss, kl_loss_grads, mel_loss_grad


def train_discriminator_step(net_d, optim_d, y, y_hat, clip_value=None, batch_size=1, c_gp=0.0):
    """(loss_disc, grad_norm_d) of one discriminator step on y, y_hat [B,1,T] device tensors (y_hat is used detached, the trainer's gen_wave), after which net_d
    holds the stepped parameters.  loss_disc: 0-dim float32 device tensor, the loss BEFORE the update; grad_norm_d: the trainer's logged number, a Python float,
    the norm of the UNCLAMPED gradients (the reference takes the norm before it clamps).  clip_value (None: no clipping) is applied by the step as it reads the
    gradients; the gradient buffer itself stays as weight_grad wrote it."""
    loss_disc, grads = discriminator_grads(net_d, y, y_hat, c_gp=c_gp)
    optim_d.zero_grad()
    grad_norm_d = clip_grad_value_(grads.values(), None, batch_size=batch_size)
    optim_d.step(grads, clip_value)
    return loss_disc, grad_norm_d


GEN_LOSS_KEYS = ("loss_gen", "loss_fm", "loss_mel", "loss_kl", "harmonic_loss", "tsi_loss", "tefs_loss")      # the order the trainer hands them to balancer_g


def generator_loss_cotangents(net_d, balancer_g, wave, y_hat, y_mel, kl_taps, z_mask, hps, msml=None):
    """The generator's loss of one iteration and what its backward pass starts from (reference training_cli.py:567-595 and the first step of :598).
    wave, y_hat [B,1,T] device tensors (the sliced real waves and the generated segments), y_mel [B, n_mels, frames] the sliced target log-mel, kl_taps =
    (z_p, logs_q, m_p, logs_p) [B,C,T'] with their mask z_mask [B,1,T'], balancer_g a losses.LossBalancer.  ONE net_d(wave, y_hat) gives loss_gen, loss_fm
    and their gradients at y_hat (losses.adversarial_input_grads); loss_mel is l1_loss on the log-mels or, with hps.train.use_multiscale, msml(y_hat, wave)
    (msml None: evaluate.multiscale_state(hps)), each with its gradient; loss_kl has none at y_hat.  The balancer reads the losses and those gradients
    (use_norm) and weighs the terms.  Returns
      loss_gen_all   the balanced sum, 0-dim float32 device tensor;
      terms          key -> loss in the trainer's order (GEN_LOSS_KEYS; the three auxiliary terms are the Python 0);
      d_y_hat        d loss_gen_all / d y_hat = sum_k w_k d loss_k / d y_hat over the terms the balancer kept, [B,1,T] float32 (summed in float64, rounded once);
      kl_cotangents  losses.kl_loss_grads scaled by loss_kl's weight: d loss_gen_all / d (z_p, logs_q, m_p, logs_p).
    The weights are balancer_g.last_weights and are constants of the backward pass, as in the reference (they are floats there).
    The gradients of the auxiliary terms are not built: hps.train.c_hd, c_tsi or c_tefs > 0 raises NotImplementedError."""
    for name in ("c_hd", "c_tsi", "c_tefs"):
        if _train_get(hps, name, 0.) > 0:
            raise NotImplementedError(f"generator_loss_cotangents: hps.train.{name} > 0: the backward of the auxiliary losses is not implemented")
    d = hps.data
    grads, _, adv = adversarial_input_grads(net_d, wave, y_hat, return_losses=True)
    if bool(_train_get(hps, "use_multiscale", False)):
        loss_mel, grads["loss_mel"] = (msml if msml is not None else multiscale_state(hps)).forward_and_grad(y_hat, wave)
    else:
        loss_mel, grads["loss_mel"] = mel_loss_grad(y_mel, y_hat, d.filter_length, d.n_mel_channels, d.sampling_rate, d.hop_length, d.win_length, d.mel_fmin,
                                                    d.mel_fmax)
    z_p, logs_q, m_p, logs_p = kl_taps
    terms = dict(loss_gen=adv["loss_gen"], loss_fm=adv["loss_fm"], loss_mel=loss_mel, loss_kl=kl_loss(z_p, logs_q, m_p, logs_p, z_mask), harmonic_loss=0,
                 tsi_loss=0, tefs_loss=0)
    loss_gen_all = balancer_g.on_train_batch_start(terms, input_grads={**grads, "loss_kl": None})
    w = balancer_g.last_weights
    d_y_hat = torch.zeros(y_hat.shape, dtype=torch.float64, device=y_hat.device)
    for k, g in grads.items():
        if k in w:
            d_y_hat += w[k] * g.view(y_hat.shape).double()
    kl_cot = kl_loss_grads(z_p, logs_q, m_p, logs_p, z_mask, scale=w.get("loss_kl", 0.0))
    return loss_gen_all, terms, d_y_hat.to(torch.float32), kl_cot


def generator_decoder_backward(net_g, tape, d_y_hat):
    """(dz [B,inter,Ty], dg [B,gin], dhar [B,seg*upp] or None) from d_y_hat [B,1,seg*upp] (generator_loss_cotangents' third result) and the GeneratorTape of
    `net_g.forward_with_tape(...)`: the decoder's vector-Jacobian product (net_g.dec_input_grad), every per-layer delta left in the tape for the weight-gradient
    pass.  dz is what autograd leaves in z.grad from the decoder branch; the KL cotangents join it in the passes that are not built yet."""
    return net_g.dec_input_grad(tape, d_y_hat)


def generator_decoder_grads(net_g, tape, d_y_hat):
    """(dz, dg, dhar, grads): generator_decoder_backward's three results and the gradient of every dec.* parameter, summed over the batch - the second step of the
    generator's backward (net_g.dec_weight_grad on the deltas the data pass has just left in the tape).  grads is an OrderedDict from state-dict name to a float32
    device tensor, views of one flat buffer (`grads.flat`) in net_g.dec_parameter_shapes() order; net_g must have been built with trainable=True."""
    dz, dg, dhar = net_g.dec_input_grad(tape, d_y_hat)
    return dz, dg, dhar, net_g.dec_weight_grad(tape)


def generator_flow_backward(net_g, tape, kl_cotangents):
    """(dz_flow [B,inter,Ty], dg_flow [B,gin]) from kl_cotangents["z_p"] (generator_loss_cotangents' fourth result) and a GeneratorTape recorded with
    `net_g.forward_with_tape(..., record_flow=True)`: the flow's vector-Jacobian product (net_g.flow_input_grad), the third step of the generator's backward.
    Its per-layer deltas stay in the tape for the flow's weight gradients."""
    return net_g.flow_input_grad(tape, kl_cotangents["z_p"])


def generator_flow_grads(net_g, tape, kl_cotangents):
    """generator_flow_backward's two results and grads: the gradient of every flow.* parameter, weight norm included, summed over the batch - the fourth step of the
    generator's backward (net_g.flow_weight_grad on the deltas the data pass has just left in the tape).  grads is an OrderedDict from state-dict name to a float32
    device tensor, views of one flat buffer (`grads.flat`) in net_g.flow_parameter_shapes() order; net_g must have been built with trainable=True."""
    dz_flow, dg_flow = net_g.flow_input_grad(tape, kl_cotangents["z_p"])
    return dz_flow, dg_flow, net_g.flow_weight_grad(tape)


def generator_latent_grad(net_g, tape, d_y_hat, kl_cotangents):
    """(dz_total, dg_total, dhar): the complete z.grad - the decoder's branch (generator_decoder_backward) plus the flow's (generator_flow_backward) - that the
    posterior encoder's backward starts from, the two branches' gradient at the speaker embedding, and the decoder's dhar.  kl_cotangents["logs_q"] reaches the
    posterior's statistics directly and is not part of this."""
    dz, dg, dhar = generator_decoder_backward(net_g, tape, d_y_hat)
    dz_flow, dg_flow = generator_flow_backward(net_g, tape, kl_cotangents)
    return dz + dz_flow, dg + dg_flow, dhar
