"""The discriminators' optimizer on the device (reference training_cli.py: optim_d = torch.optim.AdamW(net_d.parameters(), lr, betas, eps), scheduler_d =
ExponentialLR(optim_d, gamma=lr_decay, last_epoch=...)).

AdamW(net_d, ...) steps the parameters the discriminator handle holds (rvc_disc_adamw_step: the update, then the folded weights and weight images re-derived
on the device) from the flat gradient buffer of net_d.weight_grad.  Its state lives in two flat float32 device buffers in parameter order; state_dict() /
load_state_dict() speak torch.optim.AdamW's format, so a D_*.pth written here resumes in the reference's trainer and the other way round.  The conversion
between the flat buffers and that dict (state_from_flat / state_to_flat) is pure host code.  fp32 only; amsgrad and maximize are not implemented.

ExponentialLR is torch's scheduler for this optimizer (torch's own class refuses what is not a torch.optim.Optimizer)."""
import numpy as np
import torch


def torch_group_defaults():
    """The keys and default values torch.optim.AdamW puts into a param group (read from the installed torch, so a saved checkpoint carries exactly its keys)."""
    p = torch.nn.Parameter(torch.zeros(1))
    group = dict(torch.optim.AdamW([p]).state_dict()["param_groups"][0])
    group.pop("params")
    return group


def state_from_flat(step, exp_avg, exp_avg_sq, shapes):
    """torch.optim.AdamW's `state`: {k: {"step", "exp_avg", "exp_avg_sq"}} with k the parameter's index in `shapes` (an ordered name -> shape mapping), from
    the two flat host buffers.  step 0 (nothing stepped yet) is torch's empty state."""
    if int(step) == 0:
        return {}
    exp_avg, exp_avg_sq = (torch.as_tensor(t, dtype=torch.float32).reshape(-1).cpu() for t in (exp_avg, exp_avg_sq))
    total = sum(int(np.prod(s)) for s in shapes.values())
    if exp_avg.numel() != total or exp_avg_sq.numel() != total:
        raise ValueError(f"state_from_flat: buffers of {total} elements expected, got {exp_avg.numel()} and {exp_avg_sq.numel()}")
    state, o = {}, 0
    for k, shape in enumerate(shapes.values()):
        n = int(np.prod(shape))
        state[k] = {"step": torch.tensor(float(step)), "exp_avg": exp_avg[o:o + n].view(tuple(shape)).clone(),
                    "exp_avg_sq": exp_avg_sq[o:o + n].view(tuple(shape)).clone()}
        o += n
    return state


def state_to_flat(state, shapes):
    """The inverse: (step, exp_avg flat, exp_avg_sq flat) as host float32 tensors.  Every parameter must be present with its shape and all must share one step
    (they do in a checkpoint of the trainer: every parameter has a gradient at every step); an empty state is step 0 with zero buffers."""
    total = sum(int(np.prod(s)) for s in shapes.values())
    m, v = torch.zeros(total, dtype=torch.float32), torch.zeros(total, dtype=torch.float32)
    if not state:
        return 0, m, v
    if sorted(int(k) for k in state) != list(range(len(shapes))):
        raise ValueError(f"optimizer state: one entry per parameter (0 .. {len(shapes) - 1}) expected, got {sorted(state)[:4]} ... ({len(state)} entries)")
    steps, o = set(), 0
    by_index = {int(k): s for k, s in state.items()}
    for k, (name, shape) in enumerate(shapes.items()):
        s, n = by_index[k], int(np.prod(shape))
        for key, dst in (("exp_avg", m), ("exp_avg_sq", v)):
            t = torch.as_tensor(s[key])
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"optimizer state {k} ({name}): {key} has shape {tuple(t.shape)}, the parameter {tuple(shape)}")
            dst[o:o + n] = t.detach().to("cpu", torch.float32).reshape(-1)
        steps.add(float(s["step"]))
        o += n
    if len(steps) != 1 or next(iter(steps)) != int(next(iter(steps))) or next(iter(steps)) < 0:
        raise ValueError(f"optimizer state: one whole step count shared by every parameter expected, got {sorted(steps)[:4]}")
    return int(next(iter(steps))), m, v


class AdamW:
    """torch.optim.AdamW(net_d.parameters(), lr, betas, eps, weight_decay) for a discriminator net built with trainable=True.  param_groups is a list with
    one dict carrying torch's keys; it is read at every step, so a scheduler or a user may write `lr`."""

    def __init__(self, net_d, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        self.net_d = net_d
        group = torch_group_defaults()
        group.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        self.param_groups = [group]
        self._step = 0
        self._m = self._v = None                   # flat float32 device buffers in parameter order, made by the first step

    def _shapes(self):
        shapes = self.net_d.parameter_shapes()
        self.param_groups[0]["params"] = list(range(len(shapes)))
        return shapes

    def _buffers(self):
        if self._m is None:
            n = self.net_d.parameter_count()
            self._m = torch.zeros(n, dtype=torch.float32, device=self.net_d.device)
            self._v = torch.zeros(n, dtype=torch.float32, device=self.net_d.device)
        return self._m, self._v

    def zero_grad(self, set_to_none=True):
        """Nothing to do: the gradients are the result of weight_grad, fully written by every call."""

    def step(self, grads, clip_value=None):
        """One step from `grads`, net_d.weight_grad's result (its `.flat` buffer is read, never written).  clip_value: clamp every gradient element to
        [-clip_value, clip_value] on read, what clip_grad_value_ does to the gradients in place before the reference's step."""
        if not getattr(self.net_d, "trainable", False):
            raise ValueError("AdamW.step: the discriminators were built without trainable=True")
        g = self.param_groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise NotImplementedError("AdamW: amsgrad and maximize are not implemented")
        flat = getattr(grads, "flat", None)
        n = self.net_d.parameter_count()
        if not isinstance(flat, torch.Tensor) or flat.dim() != 1 or flat.numel() != n or flat.dtype != torch.float32 or not flat.is_cuda:
            raise ValueError(f"AdamW.step: grads must be the result of net_d.weight_grad (a `.flat` float32 device buffer of {n} elements)")
        m, v = self._buffers()
        self.net_d.adamw_step(flat.contiguous(), m, v, g["lr"], g["betas"], g["eps"], g["weight_decay"], self._step + 1, clip_value)
        self._step += 1

    def state_dict(self):
        shapes = self._shapes()
        if self._step == 0:
            state = {}
        else:
            state = state_from_flat(self._step, self._m.cpu(), self._v.cpu(), shapes)
        return {"state": state, "param_groups": [dict(g) for g in self.param_groups]}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != 1:
            raise ValueError(f"AdamW.load_state_dict: one param group expected, got {len(groups)}")
        if groups[0].get("amsgrad") or groups[0].get("maximize"):
            raise NotImplementedError("AdamW.load_state_dict: amsgrad and maximize are not implemented")
        shapes = self._shapes()
        if len(groups[0].get("params", [])) != len(shapes):
            raise ValueError(f"AdamW.load_state_dict: the group holds {len(groups[0].get('params', []))} parameters, the net {len(shapes)}")
        step, m, v = state_to_flat(sd["state"], shapes)
        group = dict(groups[0])
        group["betas"] = tuple(group["betas"])
        group["params"] = list(range(len(shapes)))
        self.param_groups = [group]
        self._step = step
        if step == 0:
            self._m = self._v = None
        else:
            self._m, self._v = m.to(self.net_d.device), v.to(self.net_d.device)


class ExponentialLR:
    """torch.optim.lr_scheduler.ExponentialLR for the AdamW above: lr of every group times gamma at every step().  As torch's: construction with
    last_epoch == -1 records `initial_lr` in the groups; with last_epoch >= 0 the groups must carry it already (a resumed optimizer) or KeyError is raised;
    construction itself performs the initial step, which advances last_epoch by one and leaves lr as it is."""

    def __init__(self, optimizer, gamma, last_epoch=-1):
        self.optimizer = optimizer
        self.gamma = gamma
        if last_epoch == -1:
            for group in optimizer.param_groups:
                group.setdefault("initial_lr", group["lr"])
        else:
            for i, group in enumerate(optimizer.param_groups):
                if "initial_lr" not in group:
                    raise KeyError(f"param 'initial_lr' is not specified in param_groups[{i}] when resuming scheduler with last_epoch >= 0")
        self.base_lrs = [group["initial_lr"] for group in optimizer.param_groups]
        self.last_epoch = last_epoch
        self._step_count = 0
        self._advance(initial=True)

    def _advance(self, initial):
        self._step_count += 1
        self.last_epoch += 1
        for group in self.optimizer.param_groups:
            if not initial:
                group["lr"] = group["lr"] * self.gamma
        self._last_lr = [group["lr"] for group in self.optimizer.param_groups]

    def step(self):
        self._advance(initial=False)

    def get_last_lr(self):
        return self._last_lr

    def get_lr(self):
        return [group["lr"] * self.gamma for group in self.optimizer.param_groups]

    def state_dict(self):
        return {k: v for k, v in self.__dict__.items() if k != "optimizer"}

    def load_state_dict(self, state_dict):
        self.__dict__.update(state_dict)
