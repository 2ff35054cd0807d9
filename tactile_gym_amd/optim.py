"""Adam in device memory with the global-norm clip in front of it: torch.nn.utils.clip_grad_norm_ and torch.optim.Adam's step over every
tensor of the optimiser in two launches, the plain step in one (csrc/tg_optim.h, compiled in tg_loss_head.hip).

    opt = tg.DeviceAdam(policy.parameters(), lr=3e-4, eps=1e-5)                 # SB3: optimizer_class=tg.DeviceAdam, optimizer_kwargs=dict(eps=1e-5)
    opt.zero_grad(); loss.backward()
    opt.step(max_grad_norm=0.5)                                                  # clip_grad_norm_(params, 0.5); opt.step() - what tg.train.ppo_train calls
    opt.total_norm                                                               # the gradients' norm, a float32 device scalar; nothing here reads it

    tg.DeviceAdam(params, max_grad_norm=0.5).step()                              # the clip as a property of the optimiser: every plain step() clips

A torch.optim.Optimizer: param_groups, state_dict, zero_grad (torch's own, set_to_none=True: there are no persistent gradient buffers) and
learning-rate schedules that write param_groups[i]["lr"] work as with torch's Adam, and a state_dict goes to and from torch.optim.Adam (the
state is torch's: step, a float32 CPU scalar, exp_avg and exp_avg_sq per parameter, created at the parameter's first gradient).  A parameter
whose grad is None is skipped and its step does not advance, so the bias corrections are per tensor.  The clip spans every param group, as
SB3's call over policy.parameters() does, and it does NOT rescale p.grad: the coefficient is applied inside the step, to the values the step
reads, and the gradients stay as backward left them (torch's clip_grad_norm_ scales them in place).  Gradients that are not finite behave as
under clip_grad_norm_(error_if_nonfinite=False): the coefficient, NaN for a NaN norm and 0 for an infinite one, meets every gradient.  The
arithmetic is restated in tests/optim_ref.py.  There is no CPU path.
"""
import ctypes as C
import math

import torch

from . import _capi as capi
from ._device import call, checked_f32, on_device, ptr, ptrs, stream_of, workspace

__all__ = ["DeviceAdam", "chunk_prefix"]

_REFUSED = ("amsgrad", "maximize", "capturable", "foreach", "fused", "differentiable", "decoupled_weight_decay")


def chunk_prefix(counts):
    """[first chunk of tensor 0, of tensor 1, ..., the total]: a tensor of n elements takes ceil(n / OPTIM_CHUNK) chunks, and a chunk never
    spans tensors (the kernels' tg::optim_chunks)."""
    prefix = [0]
    for n in counts:
        if n < 1:
            raise ValueError(f"a tensor of {n} elements has no chunk")
        prefix.append(prefix[-1] + (n + capi.OPTIM_CHUNK - 1) // capi.OPTIM_CHUNK)
    return prefix


class DeviceAdam(torch.optim.Optimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) on float32 device parameters, with clip_grad_norm_(params, max_grad_norm) in
    front of the step when max_grad_norm is given, here or to step().  weight_decay is Adam's L2 term (not AdamW's).  amsgrad, maximize,
    capturable, foreach, fused, differentiable and decoupled_weight_decay are refused."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None, amsgrad=False, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        if max_grad_norm is not None and not float(max_grad_norm) >= 0:
            raise ValueError(f"max_grad_norm must be None or >= 0, got {max_grad_norm}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.total_norm = None                        # float32 device scalar, made at the first clipped step and rewritten by every one
        self._partials = None                         # the chunks' sums of squares (float64, on the device)
        self._step_views = {}                         # parameter -> (its state's step tensor, that tensor's numpy view)
        # torch.optim.Adam's own keys, so that a state_dict of either loads into the other
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        self._check_group(defaults)
        super().__init__(params, defaults)

    # ------------------------------------------------------------------------------------------------------------ refusals
    def _is_device(self, t):
        return t.is_cuda

    @staticmethod
    def _check_group(group):
        lr, (beta1, beta2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
        if isinstance(lr, torch.Tensor):
            raise ValueError("lr must be a float (a tensor lr would be read on the host every step)")
        if not lr >= 0:
            raise ValueError(f"lr must be >= 0, got {lr}")
        if not (0 <= beta1 < 1 and 0 <= beta2 < 1):
            raise ValueError(f"betas must lie in [0, 1), got {(beta1, beta2)}")
        if not eps >= 0:
            raise ValueError(f"eps must be >= 0, got {eps}")
        if not wd >= 0:
            raise ValueError(f"weight_decay must be >= 0, got {wd}")
        for name in _REFUSED:
            if group.get(name):
                raise ValueError(f"{name}={group[name]!r} is not supported: DeviceAdam is plain Adam in its own launches")

    def _check_param(self, p, device):
        checked_f32(p, "a parameter", [tuple(p.shape)], device, "the other parameters' device", self._is_device)

    def _refuse(self, p, g, device):
        """Raises what the step's quick test found, in _device.py's words and order."""
        self._check_param(p, device)
        if g.is_sparse:
            raise RuntimeError("DeviceAdam does not support sparse gradients")
        checked_f32(g, "a gradient", [tuple(p.shape)], device, "its parameter's device", self._is_device)

    def _advance(self, p, step):
        """state[p]["step"] += 1 and its new value.  Through a numpy view of the float32 CPU scalar, kept per parameter: a torch operation
        on it costs the host more than the rest of the tensor's share of a step."""
        kept = self._step_views.get(p)
        if kept is None or kept[0] is not step:
            kept = self._step_views[p] = (step, step.numpy())
        value = float(kept[1]) + 1.0
        kept[1][()] = value
        return value

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._check_group(self.param_groups[-1])
        device = self.param_groups[0]["params"][0].device
        for p in self.param_groups[-1]["params"]:
            self._check_param(p, device)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._check_group(group)
        for p, st in self.state.items():
            if not st:
                continue
            for key in ("exp_avg", "exp_avg_sq"):
                checked_f32(st[key], key, [tuple(p.shape)], p.device, "its parameter's device", self._is_device)
            # a float32 CPU scalar of this optimiser's own: torch's load hands over the very tensor it was given, which the optimiser that
            # made the state_dict would go on counting in
            st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)

    # ------------------------------------------------------------------------------------------------------------ the C calls (the CPU tests replace them)
    def _c_sumsq(self, dev, grads, counts):
        with on_device(dev):
            call("tg_optim_sumsq", len(grads), ptrs(grads), (C.c_int64 * len(counts))(*counts), ptr(self._partials),
                 self._partials.numel() * 8, stream_of(dev))

    def _c_adam(self, dev, hyper, rows, max_norm, n_partials):
        beta1, beta2, eps, wd = hyper
        n = len(rows)
        clip = max_norm is not None
        with on_device(dev):
            call("tg_optim_adam", n, ptrs([r[0] for r in rows]), ptrs([r[1] for r in rows]), ptrs([r[2] for r in rows]),
                 ptrs([r[3] for r in rows]), (C.c_int64 * n)(*[r[0].numel() for r in rows]), (C.c_float * n)(*[r[4] for r in rows]),
                 (C.c_float * n)(*[r[5] for r in rows]), beta1, beta2, eps, wd, 1 if clip else 0, max_norm if clip else 0.0,
                 ptr(self._partials if clip else None), n_partials if clip else 0, ptr(self.total_norm if clip else None), stream_of(dev))

    def _reserve(self, dev, n_partials):
        if self.total_norm is None or self.total_norm.device != dev:
            self.total_norm = torch.zeros((), dtype=torch.float32, device=dev)
            self._partials = None
        if self._partials is None or self._partials.numel() < n_partials:
            self._partials = torch.empty(workspace("tg_optim_workspace", n_partials) // 8, dtype=torch.float64, device=dev)

    # ------------------------------------------------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None, max_grad_norm=None):
        """Adam over every parameter that has a grad, one launch per TG_OPTIM_MAX_TENSORS tensors; with max_grad_norm (None: the
        constructor's), clip_grad_norm_ over all of them first - one more launch that writes the chunks' sums of squares, which the Adam
        launch adds up itself.  p.grad is not rescaled."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        max_norm = self.max_grad_norm if max_grad_norm is None else float(max_grad_norm)
        if max_norm is not None and not max_norm >= 0:
            raise ValueError(f"max_grad_norm must be None or >= 0, got {max_grad_norm}")
        device = None
        work = {}                                     # (beta1, beta2, eps, weight_decay) -> [(lr, p, g)]: groups that differ in lr alone share a launch
        for group in self.param_groups:
            self._check_group(group)
            hyper = (float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]), float(group["weight_decay"]))
            lr = group["lr"]
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if device is None:
                    device = p.device
                    self._check_param(p, device)      # once a step: that this device is the ROCm device
                # the refusals' conditions, cheaply (this loop is most of what a step costs the host); _refuse finds the words
                if g.is_sparse or p.dtype is not torch.float32 or p.device != device or not p.is_contiguous() or not g.is_contiguous():
                    self._refuse(p, g, device)
                if p.numel():
                    work.setdefault(hyper, []).append((lr, p, g))
        if not work:
            return loss
        calls = []
        for hyper, entries in work.items():           # nothing was refused: the steps advance
            beta1, beta2 = hyper[:2]
            corrections = {}
            rows = []
            for lr, p, g in entries:
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                key = (self._advance(p, st["step"]), lr)
                if key not in corrections:            # torch's single-tensor Adam, in double
                    t = key[0]
                    corrections[key] = (-lr / (1 - beta1 ** t), math.sqrt(1 - beta2 ** t))
                rows.append((p, g, st["exp_avg"], st["exp_avg_sq"]) + corrections[key])
            calls.append((hyper, rows))
        n_partials = 0
        if max_norm is not None:
            grads = [r[1] for _, rows in calls for r in rows]
            counts = [g.numel() for g in grads]
            n_partials = chunk_prefix(counts)[-1]
            self._reserve(device, n_partials)
            self._c_sumsq(device, grads, counts)
        for hyper, rows in calls:
            self._c_adam(device, hyper, rows, max_norm, n_partials)
        return loss
