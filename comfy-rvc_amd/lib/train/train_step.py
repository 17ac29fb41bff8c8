"""The discriminator half of one trainer iteration on the device (reference training_cli.py:549-563): forward, discriminator_loss, backward,
clip_grad_value_, optim_d.step().  fp32 only: the reference's GradScaler with fp16_run off is the identity, and autocast is not implemented.  The gradient
penalty's parameter gradient is not built: c_gp > 0 raises (losses.discriminator_grads)."""
from ..infer_pack.commons import clip_grad_value_
from .losses import discriminator_grads


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
