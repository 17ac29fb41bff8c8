"""The trainer's helpers on gradients (reference lib/infer_pack/commons.py): clip_grad_value_, which the discriminator step runs between backward and the
optimizer (training_cli.py:562) and whose return value is the logged grad_norm_d."""
import torch

from ... import _lib


def _sq_sums(tensors):
    """float64 sum of squares of every tensor: device tensors through rvc_sqerr_sums (c = 0, at most 64 tensors per call, a fixed order: two calls give the
    same bits), host tensors in torch float64."""
    out = [None] * len(tensors)
    dev = [(k, t.detach().to(torch.float32).contiguous()) for k, t in enumerate(tensors) if t.is_cuda and t.numel() > 0]
    for k, t in enumerate(tensors):
        if not t.is_cuda or t.numel() == 0:
            out[k] = float(t.detach().to(torch.float64).square().sum())
    for o in range(0, len(dev), 64):
        part = dev[o:o + 64]
        ts = [t for _, t in part]
        if len({t.device for t in ts}) != 1:
            raise ValueError("clip_grad_value_: the gradients of one call must lie on one device")
        K = len(ts)
        ptrs = (_lib.c_void_p * K)(*[t.data_ptr() for t in ts])
        n = (_lib.c_int64 * K)(*[t.numel() for t in ts])
        c = (_lib.c_float * K)(*([0.0] * K))
        sums = torch.zeros(K, dtype=torch.float64, device=ts[0].device)
        with torch.cuda.device(ts[0].device):
            _lib.check(_lib.lib.rvc_sqerr_sums(_lib.current_stream(), ptrs, n, c, K, _lib.ptr(sums)))
        for (k, _), v in zip(part, sums.tolist()):
            out[k] = v
    return out


def clip_grad_value_(parameters, clip_value, norm_type=2, batch_size=1):
    """The reference's function: (sum_k (|grad_k|_norm_type / batch_size)^norm_type)^(1 / norm_type) over the gradients AS GIVEN, a Python float, and - when
    clip_value is not None - every gradient clamped in place to [-clip_value, clip_value] afterwards.  parameters: a tensor or an iterable of objects with
    `.grad` (those whose grad is None are skipped) or of gradient tensors themselves (the values of models.*.weight_grad's dict).  norm_type 2 sums the
    squares in float64 (rvc_sqerr_sums for device tensors); other norm types use Tensor.norm."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = []
    for p in parameters:
        if isinstance(p, torch.Tensor) and getattr(p, "grad", None) is None and not p.requires_grad:
            grads.append(p)                                  # a gradient tensor itself
        elif getattr(p, "grad", None) is not None:
            grads.append(p.grad.data)
    norm_type = float(norm_type)
    if clip_value is not None:
        clip_value = float(clip_value)
    if norm_type == 2.0:
        norms = [s ** 0.5 for s in _sq_sums(grads)]
    else:
        norms = [float(g.detach().norm(norm_type)) for g in grads]
    total_norm = 0.0
    for g, n in zip(grads, norms):
        total_norm += (n / batch_size) ** norm_type
        if clip_value is not None:
            g.clamp_(min=-clip_value, max=clip_value)
    return total_norm ** (1.0 / norm_type)
