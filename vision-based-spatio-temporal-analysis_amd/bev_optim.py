"""Adam / AdamW with the native parameter update (csrc/bev_optim.hip): the reference's build_optimizer
(train.py:46-52) and its step (train.py:238-255) without torch's per-op launches and without GradScaler's host wait.

    opt = bev_optim.Adam(model.parameters(), lr=1e-4, weight_decay=1e-4)      # for torch.optim.Adam
    opt = bev_optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-2)     # for torch.optim.AdamW

* One launch per parameter group and device updates every tensor that has a gradient (bev_native.adam_step).
* `_step_supports_amp_scaling`: torch.amp.GradScaler hands `grad_scale` / `found_inf` over as device tensors and
  never reads them back; the kernel unscales the gradients as it reads them (they are not modified in memory) and
  writes nothing when found_inf is set.  step() itself reads nothing back either.
* State and param_groups have torch.optim.Adam's keys and types (`step` an fp32 0-dim tensor, `exp_avg`,
  `exp_avg_sq`), so state dicts load both ways; `lr` is read from the group at every step, so torch's schedulers work.
* CPU parameters take bev_adam_step_host, the same arithmetic compiled for the host.
* Every step advances the version counter of each updated parameter, `exp_avg` and `exp_avg_sq`
  (bev_native.mark_written), as torch.optim.Adam's in-place ops do: the models' packed-weight caches, keyed on
  (data_ptr, _version), re-pack at their next forward.  Host bookkeeping only: no launch, no read-back.

The arithmetic is a defined fp32 sequence (csrc/bev_optim.h): torch's single-tensor Adam op for op with every fused
multiply-add split in two.  Not offered: amsgrad, maximize, capturable / differentiable, tensor learning rates,
sparse gradients, parameters that are not fp32.
"""
from __future__ import annotations

import numpy as np
import torch

import bev_native as _nat

__all__ = ["Adam", "AdamW"]

_TABLE_CACHE_MAX = 4  # tables kept per (group, device): the two step-buffer parities, twice


def _dense(t: torch.Tensor) -> bool:
    return t.is_contiguous() or torch._prims_common.is_non_overlapping_and_dense(t)


class Adam(torch.optim.Optimizer):
    _step_supports_amp_scaling = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *,
                 maximize=False, decoupled_weight_decay=False):
        if isinstance(lr, torch.Tensor):
            raise ValueError("bev_optim.Adam takes a Python float lr (a tensor lr would be read back every step)")
        if amsgrad:
            raise ValueError("bev_optim.Adam does not offer amsgrad")
        if maximize:
            raise ValueError("bev_optim.Adam does not offer maximize")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # every key torch.optim.Adam's groups carry, with its defaults for the ones this class does not act on
        defaults = dict(torch.optim.Adam([torch.zeros(1)]).defaults)
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        decoupled_weight_decay=decoupled_weight_decay)
        super().__init__(params, defaults)
        for group in self.param_groups:
            for p in group["params"]:
                self._check_param(p)
        self._spare = {}   # parameter -> the second step buffer (the kernel reads one and writes the other)
        self._tables = {}  # (group index, device) -> {pointer tuple: (device table, T, total chunks)}

    @staticmethod
    def _check_param(p):
        if p.dtype != torch.float32:
            raise ValueError(f"bev_optim.Adam takes fp32 parameters, got {p.dtype}")
        if p.is_sparse or p.layout != torch.strided:
            raise ValueError("bev_optim.Adam takes dense (strided) parameters")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for p in self.param_groups[-1]["params"]:
            self._check_param(p)

    def _check_group(self, group):
        if group.get("amsgrad") or group.get("maximize"):
            raise ValueError("bev_optim.Adam does not offer amsgrad / maximize")
        if group.get("capturable") or group.get("differentiable"):
            raise ValueError("bev_optim.Adam does not offer capturable / differentiable")
        if isinstance(group["lr"], torch.Tensor):
            raise ValueError("bev_optim.Adam takes a Python float lr")

    def _operands(self, p):
        """(p, g, m, v, step_in, step_out) of a parameter that has a gradient, the state created on first use, all
        dense in one element order and on p's device."""
        g = p.grad
        if g.is_sparse or g.layout != torch.strided:
            raise ValueError("bev_optim.Adam does not take sparse gradients")
        if g.dtype != torch.float32:
            raise ValueError(f"bev_optim.Adam takes fp32 gradients, got {g.dtype}")
        if not _dense(p):
            raise ValueError("bev_optim.Adam takes parameters that are dense in memory")
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        step = st["step"]
        if not isinstance(step, torch.Tensor):  # a state dict of the time when torch kept a Python number
            step = torch.tensor(float(step), dtype=torch.float32)
        if step.device != p.device or step.dtype != torch.float32 or step.dim() != 0:
            step = step.detach().to(device=p.device, dtype=torch.float32).reshape(())  # torch keeps it on the host
        st["step"] = step
        strides = p.stride()
        for key in ("exp_avg", "exp_avg_sq"):
            if st[key].stride() != strides or st[key].dtype != torch.float32 or st[key].device != p.device:
                st[key] = torch.empty_like(p, memory_format=torch.preserve_format).copy_(st[key])
        if g.stride() != strides:
            g = torch.empty_like(p, memory_format=torch.preserve_format).copy_(g)  # the gradient in p's layout
        spare = self._spare.get(p)
        if spare is None or spare.device != p.device:
            spare = self._spare[p] = torch.zeros((), dtype=torch.float32, device=p.device)
        return p, g, st["exp_avg"], st["exp_avg_sq"], step, spare

    def _scaler_scalars(self, device):
        out = []
        for name in ("grad_scale", "found_inf"):
            t = getattr(self, name, None)
            if t is not None:
                if t.dtype != torch.float32 or t.numel() != 1:
                    raise ValueError(f"bev_optim.Adam: {name} is a single fp32 value")
                if t.device != device:
                    t = t.to(device, non_blocking=True)
            out.append(t)
        return out

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)
            by_device = {}
            for p in group["params"]:
                if p.grad is not None:
                    by_device.setdefault(p.device, []).append(p)
            beta1, beta2 = group["betas"]
            hyper = (float(group["lr"]), float(beta1), float(beta2), float(group["eps"]),
                     float(group["weight_decay"]), bool(group.get("decoupled_weight_decay", False)))
            for device, params in by_device.items():
                ops = [self._operands(p) for p in params]
                grad_scale, found_inf = self._scaler_scalars(device)
                records = [(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), s_in.data_ptr(), s_out.data_ptr(),
                            p.numel()) for p, g, m, v, s_in, s_out in ops]
                if device.type == "cuda":
                    self._launch(gi, device, records, hyper, grad_scale, found_inf)
                else:
                    table, _ = _nat.adam_table(records)
                    _nat.adam_step_host(table, len(records), *hyper, grad_scale=grad_scale, found_inf=found_inf)
                # the update went through raw pointers: advance the version counters as torch's in-place ops would,
                # so operands cached under (data_ptr, _version) are rebuilt.  Unconditional -- found_inf lives on the
                # device and is not read here; a skipped step costs one needless re-pack
                _nat.mark_written(*[t for p, _, m, v, _, _ in ops for t in (p, m, v)])
                for p, _, _, _, s_in, s_out in ops:  # the swap: what the launch wrote is the parameter's step now
                    self.state[p]["step"] = s_out
                    self._spare[p] = s_in
        return loss

    def _launch(self, gi, device, records, hyper, grad_scale, found_inf):
        cache = self._tables.setdefault((gi, device), {})
        key = tuple(records)
        hit = cache.get(key)
        if hit is None:
            # a pointer changed (the first steps, a reallocated gradient, a loaded state dict): build and upload
            table, chunks = _nat.adam_table(records)
            pinned = torch.empty(table.size, dtype=torch.int64, pin_memory=True)
            pinned.numpy()[:] = table.reshape(-1)
            dev = torch.empty(table.size, dtype=torch.int64, device=device)
            dev.copy_(pinned, non_blocking=True)
            while len(cache) >= _TABLE_CACHE_MAX:
                cache.pop(next(iter(cache)))
            hit = cache[key] = (dev, len(records), chunks)
        dev, T, chunks = hit
        with torch.cuda.device(device):
            _nat.adam_step(dev, T, chunks, *hyper, grad_scale=grad_scale, found_inf=found_inf)


class AdamW(Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *,
                 maximize=False, decoupled_weight_decay=True):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize,
                         decoupled_weight_decay=True)
