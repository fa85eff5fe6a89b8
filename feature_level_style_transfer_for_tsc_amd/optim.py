"""Adam for modules made of MANY small tensors (CPC: 256 separate ``Wk[i]`` Linear layers + a GRU = 516 tensors).

``torch.optim.Adam(capturable=True)`` keeps one 0-dim device ``step`` tensor PER parameter; its bias-correction
arithmetic runs as foreach ops over lists of 0-dim tensors, which take the per-tensor slow path: ≈4 000 tiny kernels
(fills, adds, divisions) per optimiser step for this module — a tenth of the whole train step.  All parameters of a
group advance together, so ONE shared device counter is enough: the bias corrections become a handful of scalar ops
and the update itself a dozen multi-tensor kernels.  The update formula is torch's (capturable branch):

    m ← β₁m + (1−β₁)g;  v ← β₂v + (1−β₂)g²;  p ← p − (lr / (1−β₁ᵗ)) · m / (√v / √(1−β₂ᵗ) + ε)

Graph-capture safe (the counter lives on the device, no host reads).

Learning rates under graph replay.  By default ``step()`` reads ``group["lr"]`` on the host and hands it to the kernel by value: a
captured step keeps the rate it was captured with.  ``lr_on_device=True`` (both optimisers) keeps one fp32 device tensor
``lr_dev`` with an element per param group, which the ``*_dev`` kernels read when they run; ``push_lr`` copies every
``group["lr"]`` a scheduler has changed into it, so a replayed graph follows a stock ``torch.optim.lr_scheduler``.  ``lr_dev``
lives outside ``param_groups`` and ``state``: ``state_dict()`` does not save it and ``load_state_dict()`` does not replace it (a
captured graph holds its address); the next ``push_lr`` brings it in line with the loaded ``group["lr"]``.
"""
from __future__ import annotations

import ctypes
from typing import Iterable, List, Sequence

import numpy as np
import torch


def _f32(v) -> float:
    """The fp32 value a kernel receives for a Python-float hyper-parameter."""
    return float(np.float32(v))


class _DeviceLR:
    """Mixin of the two optimisers: the learning rates as a device tensor beside ``param_groups``."""
    lr_on_device = False

    def enable_lr_on_device(self) -> None:
        """Create ``lr_dev`` (one fp32 element per param group, on the parameters' device) from ``group["lr"]``; from now on
        ``step()`` launches the kernels that read it.  Idempotent.  Not under a resident capture of a host-lr step."""
        if self.lr_on_device:
            return
        self._lr_pushed = [_f32(g["lr"]) for g in self.param_groups]      # what lr_dev holds, known without reading it back
        self.lr_dev = torch.tensor(self._lr_pushed, dtype=torch.float32, device=self.param_groups[0]["params"][0].device)
        self.lr_on_device = True


def push_lr(optimisers) -> int:
    """Write every ``group["lr"]`` whose fp32 value differs from the one last pushed into its optimiser's ``lr_dev``, on the
    current stream and without waiting for the device (the device reads the new values in stream order: a graph replayed
    afterwards sees them).  Optimisers without ``lr_on_device`` are passed over.  Returns the number of groups that changed."""
    changed = 0
    for o in optimisers:
        if not getattr(o, "lr_on_device", False):
            continue
        new = [_f32(g["lr"]) for g in o.param_groups]
        n = sum(a != b for a, b in zip(new, o._lr_pushed))
        if n:
            host = torch.tensor(new, dtype=torch.float32)
            if o.lr_dev.is_cuda:
                host = host.pin_memory()             # a pageable source would make the copy wait for the device
            o.lr_dev.copy_(host, non_blocking=True)
            o._lr_pushed = new
            changed += n
    return changed


def _capturing(t: torch.Tensor) -> bool:
    return t.is_cuda and torch.cuda.is_current_stream_capturing()


class SharedStepAdam(_DeviceLR, torch.optim.Optimizer):
    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 lr_on_device: bool = False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        if lr_on_device:
            self.enable_lr_on_device()
        for group in self.param_groups:
            ps = group["params"]
            dev = ps[0].device
            group["step"] = torch.zeros((), dtype=torch.float32, device=dev)     # shared by every tensor of the group
            group["betas_dev"] = (torch.tensor(group["betas"][0], dtype=torch.float32, device=dev),
                                  torch.tensor(group["betas"][1], dtype=torch.float32, device=dev))   # no H2D inside step()
            for p in ps:
                self.state[p]["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                self.state[p]["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            self.state[ps[0]]["step"] = group["step"]                             # visible to state snapshots

    @torch.no_grad()
    def step(self, closure=None):
        assert closure is None
        if self.lr_on_device and not _capturing(self.lr_dev):
            push_lr([self])                                                     # eager: follow group["lr"] as the host-lr step does
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            if ps[0].is_cuda:
                # one single-pass multi-tensor launch per 64 tensors (csrc/optim.hip) instead of eleven foreach passes
                from . import _lib
                lib = _lib.load()
                t = group["step"]
                t += 1
                grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in ps]
                m = [self.state[p]["exp_avg"] for p in ps]
                v = [self.state[p]["exp_avg_sq"] for p in ps]
                b1, b2 = group["betas"]
                if self.lr_on_device:
                    _lib.check(lib.fst_adam_multi_dev(_ptr_array(ps), _ptr_array(grads), _ptr_array(m), _ptr_array(v),
                                                      _i64_array([p.numel() for p in ps]), len(ps), t.data_ptr(),
                                                      self.lr_dev[gi].data_ptr(), b1, b2, group["eps"], _lib.stream_ptr()),
                               "fst_adam_multi_dev")
                    continue
                _lib.check(lib.fst_adam_multi(_ptr_array(ps), _ptr_array(grads), _ptr_array(m), _ptr_array(v),
                                              _i64_array([p.numel() for p in ps]), len(ps), t.data_ptr(), group["lr"], b1, b2,
                                              group["eps"], _lib.stream_ptr()), "fst_adam_multi")
                continue
            grads = [p.grad for p in ps]
            m = [self.state[p]["exp_avg"] for p in ps]
            v = [self.state[p]["exp_avg_sq"] for p in ps]
            b1, b2 = group["betas"]
            t = group["step"]
            t += 1
            b1_t, b2_t = group["betas_dev"]
            bc1 = 1.0 - torch.pow(b1_t, t)
            bc2_sqrt = torch.sqrt(1.0 - torch.pow(b2_t, t))
            torch._foreach_mul_(m, b1)
            torch._foreach_add_(m, grads, alpha=1.0 - b1)
            torch._foreach_mul_(v, b2)
            torch._foreach_addcmul_(v, grads, grads, value=1.0 - b2)
            denom = torch._foreach_sqrt(v)
            torch._foreach_div_(denom, bc2_sqrt)
            torch._foreach_add_(denom, group["eps"])
            upd = torch._foreach_div(m, denom)
            torch._foreach_mul_(upd, (self.lr_dev[gi] if self.lr_on_device else group["lr"]) / bc1)
            torch._foreach_sub_(ps, upd)
        return None


def _ptr_array(tensors: Sequence[torch.Tensor]):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _i64_array(values: Sequence[int]):
    return (ctypes.c_int64 * len(values))(*values)


class FusedRMSprop(_DeviceLR, torch.optim.Optimizer):
    """``torch.optim.RMSprop(params, lr)`` with its defaults (alpha 0.99, eps 1e-8, not centered, no momentum, no weight decay —
    what train_and_test.py:97-106 constructs) whose step is ONE pass over every tensor: v ← αv + (1−α)g², p ← p − lr·g/(√v + ε)
    in torch's operation order, up to 64 tensors per launch (csrc/optim.hip).  ``rmsprop_step_many`` steps several of these
    optimisers (one per module, each with its own learning rate) with the same launches: the joint step's ten RMSprops are 4
    launches instead of ~70 foreach launches (1.6 ms of five-pass multi-tensor kernels).  State: ``square_avg`` per parameter,
    created on first use; hipGraph-capture safe once created (the warm-up steps do that).  ``lr_on_device``: see the module
    docstring."""

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-2, alpha: float = 0.99, eps: float = 1e-8,
                 lr_on_device: bool = False):
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps))
        if lr_on_device:
            self.enable_lr_on_device()

    @torch.no_grad()
    def step(self, closure=None):
        assert closure is None
        rmsprop_step_many([self])
        return None


@torch.no_grad()
def rmsprop_step_many(opts: Sequence[FusedRMSprop]) -> None:
    """One step of several FusedRMSprops: one series of launches for the optimisers with host learning rates and one for those
    with ``lr_on_device`` (whose ``lr_dev`` is brought up to date first, except under stream capture)."""
    host = [o for o in opts if not o.lr_on_device]
    dev = [o for o in opts if o.lr_on_device]
    if host:
        _rmsprop_launch(host, False)
    if dev:
        if not _capturing(dev[0].lr_dev):
            push_lr(dev)
        _rmsprop_launch(dev, True)


def _rmsprop_launch(opts: Sequence[FusedRMSprop], on_device: bool) -> None:
    ps: List[torch.Tensor] = []
    grads: List[torch.Tensor] = []
    vs: List[torch.Tensor] = []
    lrs: list = []                                                            # floats, or 0-dim views of lr_dev
    alpha = eps = None
    for o in opts:
        for gi, group in enumerate(o.param_groups):
            if alpha is None:
                alpha, eps = group["alpha"], group["eps"]
            assert (group["alpha"], group["eps"]) == (alpha, eps), "rmsprop_step_many: one (alpha, eps) per call"
            lr = o.lr_dev[gi] if on_device else float(group["lr"])
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = o.state[p]
                if "square_avg" not in st:
                    st["square_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                ps.append(p)
                grads.append(p.grad if p.grad.is_contiguous() else p.grad.contiguous())
                vs.append(st["square_avg"])
                lrs.append(lr)
    if not ps:
        return
    if not ps[0].is_cuda:                                                     # CPU tests of the host logic: torch's own formula
        for p, g, v, lr in zip(ps, grads, vs, lrs):
            v.mul_(alpha).addcmul_(g, g, value=1 - alpha)
            if on_device:
                p.sub_(lr * (g / v.sqrt().add_(eps)))
            else:
                p.addcdiv_(g, v.sqrt().add_(eps), value=-lr)
        return
    from . import _lib
    lib = _lib.load()
    assert all(p.is_contiguous() for p in ps)
    if on_device:
        _lib.check(lib.fst_rmsprop_multi_dev(_ptr_array(ps), _ptr_array(grads), _ptr_array(vs), _i64_array([p.numel() for p in ps]),
                                             _ptr_array(lrs), len(ps), alpha, eps, _lib.stream_ptr()), "fst_rmsprop_multi_dev")
        return
    _lib.check(lib.fst_rmsprop_multi(_ptr_array(ps), _ptr_array(grads), _ptr_array(vs), _i64_array([p.numel() for p in ps]),
                                     (ctypes.c_float * len(lrs))(*lrs), len(ps), alpha, eps, _lib.stream_ptr()), "fst_rmsprop_multi")
