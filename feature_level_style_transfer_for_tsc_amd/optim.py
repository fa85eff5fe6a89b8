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

Anomaly guard.  ``count_nonfinite`` counts NaN / inf elements of many tensors per group on the device and, given an
``AnomalyGuard``, leaves its verdict there; ``rmsprop_step_many(opts, guard=...)`` and ``SharedStepAdam.step(guard=...)`` then
launch the same updates behind that verdict word (``fst_*_multi_guard``): a step with a non-finite gradient writes nothing, and
nothing waits for the host.

Gradient norms and clipping.  ``sumsq_norms`` takes the L2 norms of many tensors per group on the device and leaves, next to them,
the factors that cap each group and then the whole (``clip_coefficients`` is their definition; ``GradClip`` holds the device
words); ``scale_by_group`` multiplies the tensors by those factors, read when the kernels run: what
``torch.nn.utils.clip_grad_norm_`` does with a host decision, usable inside a replayed graph.

Weight averaging.  ``ema_update`` keeps an exponential moving average of many tensors per group, its weight derived on the device
from the words of a ``WeightAverage`` (decay, warm-up, update counts) when the kernels run; ``swap_tensors`` exchanges two lists of
tensors in place — the averages into the modules' own storage for evaluation, and back.

Gradient accumulation.  ``accumulate`` folds gradients into fp32 accumulators over a window of k calls and leaves their mean in
the gradient tensors on the call that closes it; the position in the window is a word of a ``GradAccumulation`` that the kernels
read when they run, so one captured launch series serves every position.
"""
from __future__ import annotations

import contextlib
import ctypes
from typing import Iterable, List, Optional, Sequence

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


def push_words(dst: torch.Tensor, host: torch.Tensor) -> None:
    """Copy the host tensor into the device words ``dst`` on the current stream, without waiting for the device."""
    if dst.is_cuda:
        host = host.pin_memory()                     # a pageable source would make the copy wait for the device
    dst.copy_(host, non_blocking=True)


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
            push_words(o.lr_dev, torch.tensor(new, dtype=torch.float32))
            o._lr_pushed = new
            changed += n
    return changed


def _capturing(t: torch.Tensor) -> bool:
    return t.is_cuda and torch.cuda.is_current_stream_capturing()


def _scan_slots(owner, n_words: int, like: torch.Tensor) -> torch.Tensor:
    """``owner._slots``, the scratch of a scan, grown to ``n_words`` words of the dtype and device of ``like`` — outside captures only."""
    if owner._slots is None or owner._slots.numel() < n_words:
        if _capturing(like):
            raise RuntimeError(f"{type(owner).__name__}: the scan's slot array would have to grow inside a stream capture; run one "
                               "eager step of the same tensors first")
        owner._slots = torch.empty(max(n_words, 1), dtype=like.dtype, device=like.device)
    return owner._slots


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
    def step(self, closure=None, guard: Optional["AnomalyGuard"] = None):
        """``guard``: the update runs behind ``guard.verdict`` (read on the device when the kernels run) and the shared counter
        advances by ``guard.ok``: after a non-zero verdict parameters, moments and counter are what they were."""
        assert closure is None
        if self.lr_on_device and not _capturing(self.lr_dev):
            push_lr([self])                                                     # eager: follow group["lr"] as the host-lr step does
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            m = [self.state[p]["exp_avg"] for p in ps]
            v = [self.state[p]["exp_avg_sq"] for p in ps]
            b1, b2 = group["betas"]
            t = group["step"]
            if ps[0].is_cuda:
                # one single-pass multi-tensor launch per 64 tensors (csrc/optim.hip) instead of eleven foreach passes
                from . import _lib
                lib = _lib.load()
                t += 1 if guard is None else guard.ok
                grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in ps]
                lr_dev = self.lr_dev[gi].data_ptr() if self.lr_on_device else None
                if guard is not None:                                           # either rate form: lr_dev is None or not
                    name, rate, verdict = "fst_adam_multi_guard", (group["lr"], lr_dev), (guard.verdict.data_ptr(),)
                elif self.lr_on_device:
                    name, rate, verdict = "fst_adam_multi_dev", (lr_dev,), ()
                else:
                    name, rate, verdict = "fst_adam_multi", (group["lr"],), ()
                _lib.check(getattr(lib, name)(_ptr_array(ps), _ptr_array(grads), _ptr_array(m), _ptr_array(v),
                                              _i64_array([p.numel() for p in ps]), len(ps), t.data_ptr(), *rate, b1, b2, group["eps"],
                                              *verdict, _lib.stream_ptr()), name)
                continue
            grads = [p.grad for p in ps]
            if guard is not None:                                               # CPU: the unguarded arithmetic on copies, kept where ok
                old = [t.clone()] + [x.detach().clone() for x in list(ps) + m + v]
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
            if guard is not None:
                keep = guard.ok > 0
                for x, o in zip([t] + list(ps) + m + v, old):
                    x.copy_(torch.where(keep, x, o))
        return None


def _ptr_array(tensors: Sequence[torch.Tensor]):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _i64_array(values: Sequence[int]):
    return (ctypes.c_int64 * len(values))(*values)


def _i32_array(values: Sequence[int]):
    return (ctypes.c_int32 * len(values))(*values)


def _mask_i32(mask: int) -> int:
    """A mask of 32 group bits as the int32 the C ABI takes it in."""
    return mask - (1 << 32) if mask >> 31 else mask


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
    def step(self, closure=None, guard: Optional["AnomalyGuard"] = None):
        assert closure is None
        rmsprop_step_many([self], guard)
        return None


@torch.no_grad()
def rmsprop_step_many(opts: Sequence[FusedRMSprop], guard: Optional["AnomalyGuard"] = None) -> None:
    """One step of several FusedRMSprops: one series of launches for the optimisers with host learning rates and one for those
    with ``lr_on_device`` (whose ``lr_dev`` is brought up to date first, except under stream capture).  ``guard``: the updates run
    behind ``guard.verdict``, read on the device when the kernels run; with a non-zero verdict no parameter and no moment changes
    (moments created by this call stay zero)."""
    host = [o for o in opts if not o.lr_on_device]
    dev = [o for o in opts if o.lr_on_device]
    if host:
        _rmsprop_launch(host, False, guard)
    if dev:
        if not _capturing(dev[0].lr_dev):
            push_lr(dev)
        _rmsprop_launch(dev, True, guard)


def _rmsprop_launch(opts: Sequence[FusedRMSprop], on_device: bool, guard: Optional["AnomalyGuard"] = None) -> None:
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
            if guard is not None:
                old_p, old_v = p.detach().clone(), v.clone()
            v.mul_(alpha).addcmul_(g, g, value=1 - alpha)
            if on_device:
                p.sub_(lr * (g / v.sqrt().add_(eps)))
            else:
                p.addcdiv_(g, v.sqrt().add_(eps), value=-lr)
            if guard is not None:
                keep = guard.ok > 0
                p.copy_(torch.where(keep, p, old_p)); v.copy_(torch.where(keep, v, old_v))
        return
    from . import _lib
    lib = _lib.load()
    assert all(p.is_contiguous() for p in ps)
    rates = _ptr_array(lrs) if on_device else (ctypes.c_float * len(lrs))(*lrs)
    if guard is not None:                                                     # either rate form: by value, or by address
        name, rate, verdict = "fst_rmsprop_multi_guard", ((None, rates) if on_device else (rates, None)), (guard.verdict.data_ptr(),)
    else:
        name, rate, verdict = ("fst_rmsprop_multi_dev" if on_device else "fst_rmsprop_multi"), (rates,), ()
    _lib.check(getattr(lib, name)(_ptr_array(ps), _ptr_array(grads), _ptr_array(vs), _i64_array([p.numel() for p in ps]), *rate,
                                  len(ps), alpha, eps, *verdict, _lib.stream_ptr()), name)


# ---- anomaly guard: a device-side verdict on the values a step's update consumes
MAX_GROUPS = 32


class AnomalyGuard:
    """The device words of the anomaly guard: ``counts`` (int32[32], non-finite elements per group of the last
    ``count_nonfinite``), ``verdict`` (int32, 1 if a group of the verdict mask counted anything), ``ok`` (fp32, 1 − verdict: what a
    shared step counter advances by) and ``skipped`` (int32, the cumulative number of non-zero verdicts).  The kernels of the
    guarded optimisers read ``verdict`` when they run; the host reads any of these only when it chooses to."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.counts = torch.zeros(MAX_GROUPS, dtype=torch.int32, device=device)
        self.verdict = torch.zeros(1, dtype=torch.int32, device=device)
        self.ok = torch.ones((), dtype=torch.float32, device=device)
        self.skipped = torch.zeros(1, dtype=torch.int32, device=device)
        self._slots = None                                                    # scratch of the scan, grown outside captures

    def slots(self, n_words: int) -> torch.Tensor:
        return _scan_slots(self, n_words, self.verdict)


@torch.no_grad()
def count_nonfinite(tensors: Sequence[torch.Tensor], groups: Sequence[int], n_groups: int, guard: Optional[AnomalyGuard] = None,
                    verdict_groups: Optional[Sequence[int]] = None) -> torch.Tensor:
    """Number of non-finite (NaN, ±inf) elements of the fp32 ``tensors`` per group: ``groups[i]`` in ``range(n_groups)``,
    ``n_groups`` ≤ 32.  Returns an int32 tensor of ``n_groups`` counts on the tensors' device, without waiting for it: on the GPU
    one ``fst_nonfinite_multi`` launch per 64 tensors plus a finalising one; the tensors are only read (views that start 4 bytes
    off a 16-byte boundary included; non-contiguous ones are copied first).  With a ``guard`` the counts go into ``guard.counts``
    (a view of it is returned) and the call leaves ``guard.verdict`` = 1 if a group of ``verdict_groups`` (default: every group)
    counted anything, ``guard.ok`` = 1 − verdict, and adds the verdict to ``guard.skipped``."""
    if not 0 < n_groups <= MAX_GROUPS:
        raise ValueError(f"count_nonfinite: n_groups must be in 1..{MAX_GROUPS}, got {n_groups}")
    if len(tensors) != len(groups):
        raise ValueError(f"count_nonfinite: {len(tensors)} tensors, {len(groups)} group ids")
    for i, (t, g) in enumerate(zip(tensors, groups)):
        if not 0 <= int(g) < n_groups:
            raise ValueError(f"count_nonfinite: tensor {i}: group {g} is not in range({n_groups})")
        if t.dtype != torch.float32:
            raise TypeError(f"count_nonfinite: tensor {i} must be float32, got {t.dtype}")
    mask = (1 << MAX_GROUPS) - 1
    if verdict_groups is not None:
        mask = sum(1 << int(g) for g in set(verdict_groups))
    keep = [(t, int(g)) for t, g in zip(tensors, groups) if t.numel() > 0]
    dev = guard.device if guard is not None else (tensors[0].device if tensors else torch.device("cpu"))
    if dev.type != "cuda":                                                    # CPU tests of the host logic
        counts = torch.zeros(MAX_GROUPS, dtype=torch.int32)
        for t, g in keep:
            counts[g] += int((~torch.isfinite(t)).sum())
        if guard is not None:
            bad = int(any(int(counts[g]) > 0 for g in range(MAX_GROUPS) if (mask >> g) & 1))
            guard.counts.copy_(counts)
            guard.verdict.fill_(bad); guard.ok.fill_(1.0 - bad); guard.skipped.add_(bad)
            counts = guard.counts
        return counts[:n_groups]
    from . import _lib
    lib = _lib.load()
    xs = [t if t.is_contiguous() else t.contiguous() for t, _ in keep]
    n_slots = int(lib.fst_nonfinite_slots(len(xs)))
    if guard is None:
        counts, slots = torch.empty(MAX_GROUPS, dtype=torch.int32, device=dev), torch.empty(max(n_slots, 1), dtype=torch.int32, device=dev)
        words = (None, None, None)
    else:
        counts, slots = guard.counts, guard.slots(n_slots)
        words = (guard.verdict.data_ptr(), guard.ok.data_ptr(), guard.skipped.data_ptr())
    _lib.check(lib.fst_nonfinite_multi(_ptr_array(xs), _i64_array([x.numel() for x in xs]), _i32_array([g for _, g in keep]), len(xs),
                                       _mask_i32(mask), slots.data_ptr(), slots.numel(), counts.data_ptr(), *words, _lib.stream_ptr()),
               "fst_nonfinite_multi")
    return counts[:n_groups]


@torch.no_grad()
def guard_copy(dst: Sequence[torch.Tensor], src: Sequence[torch.Tensor], guard: Optional[AnomalyGuard] = None, when: bool = True) -> None:
    """Copy every ``src[i]`` into ``dst[i]`` (same shape and dtype, contiguous, elements of 4 or 8 bytes) as one multi-tensor
    launch per 64 tensors: at once without a ``guard``, otherwise only if ``(guard.verdict != 0) == when`` at the time the kernel
    runs — the save and the roll-back of state that cannot be guarded where it is written."""
    for d, s in zip(dst, src):
        if d.shape != s.shape or d.dtype != s.dtype or not (d.is_contiguous() and s.is_contiguous()) or d.element_size() % 4:
            raise ValueError(f"guard_copy: {tuple(s.shape)} {s.dtype} -> {tuple(d.shape)} {d.dtype}: contiguous tensors of one shape "
                             "and dtype with elements of 4 or 8 bytes")
    pairs = [(d, s) for d, s in zip(dst, src) if d.numel() > 0]
    if not pairs:
        return
    if not pairs[0][0].is_cuda:
        if guard is None or bool(guard.verdict.item() != 0) == bool(when):
            for d, s in pairs:
                d.copy_(s)
        return
    from . import _lib
    _lib.check(_lib.load().fst_guard_copy_multi(_ptr_array([d for d, _ in pairs]), _ptr_array([s for _, s in pairs]),
                                                _i64_array([d.numel() * d.element_size() // 4 for d, _ in pairs]), len(pairs),
                                                None if guard is None else guard.verdict.data_ptr(), int(bool(when)),
                                                _lib.stream_ptr()), "fst_guard_copy_multi")


# ---- gradient norms and clipping: per-group L2 norms and the factors that cap them, decided and applied on the device
def clip_coefficients(norms, limits):
    """The factors ``fst_sumsq_multi``'s finaliser derives from 32 per-group L2 norms and 33 limits (``limits[32]`` caps the norm
    over all groups; ``inf`` = no limit), in fp64 — the definition of the clipping, and what the CPU tests compare with torch:

        c_g = min(1, limits[g] / (norms[g] + 1e-6))                            each group by its own cap, as clip_grad_norm_ would
        c   = min(1, limits[32] / (sqrt(Σ_g (c_g·norms[g])²) + 1e-6))          then the whole by what the group caps left of it
        coef[g] = c_g · c

    The constant and the clamp are ``torch.nn.utils.clip_grad_norm_``'s.  One deliberate difference: if any norm (or their total)
    is not finite, every factor is 1.0 where torch would multiply every gradient by NaN — the gradients are left alone, the norms
    are reported as they came out, and the anomaly guard or the user decides about the step.  ``norms``: 32 values, or 33 of
    which the last (the total before clipping, as the kernel reports it) only takes part in that test.  Returns a float64 tensor
    of 32 factors; the kernel rounds the same product to fp32."""
    norms = torch.as_tensor(norms, dtype=torch.float64).reshape(-1)
    limits = torch.as_tensor(limits, dtype=torch.float64).reshape(-1)
    if norms.numel() not in (MAX_GROUPS, MAX_GROUPS + 1) or limits.numel() != MAX_GROUPS + 1:
        raise ValueError(f"clip_coefficients: {norms.numel()} norms and {limits.numel()} limits; {MAX_GROUPS} (or {MAX_GROUPS + 1}) and "
                         f"{MAX_GROUPS + 1} wanted")
    n = norms[:MAX_GROUPS].tolist()
    total = float(torch.sqrt(sum(v * v for v in norms[:MAX_GROUPS])))
    if not all(np.isfinite(v) for v in n + norms[MAX_GROUPS:].tolist() + [total]):
        return torch.ones(MAX_GROUPS, dtype=torch.float64)
    lim = limits.tolist()
    c_g = [min(1.0, float(np.float64(lim[g]) / np.float64(n[g] + 1e-6))) for g in range(MAX_GROUPS)]
    rest = 0.0
    for g in range(MAX_GROUPS):
        rest += (c_g[g] * n[g]) * (c_g[g] * n[g])
    c = min(1.0, float(np.float64(lim[MAX_GROUPS]) / np.float64(float(np.sqrt(rest)) + 1e-6)))
    return torch.tensor([c_g[g] * c for g in range(MAX_GROUPS)], dtype=torch.float64)


class GradClip:
    """The device words of the gradient clipping: ``limits`` (fp32[33]: a cap per group and, last, the cap on the norm over all
    groups; ``inf`` = none), ``norms`` (fp32[33], the L2 norms of the last ``sumsq_norms``, last the total, before clipping),
    ``coef`` (fp32[32], the factors of the last ``sumsq_norms``, 1 where nothing is clipped) and the scan's slot array.
    ``limits_host`` is what ``limits`` holds, known without reading it back; ``set_limits`` changes both with one stream-ordered
    copy, which a graph replayed afterwards sees."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.limits_host = [float("inf")] * (MAX_GROUPS + 1)
        self.limits = torch.full((MAX_GROUPS + 1,), float("inf"), dtype=torch.float32, device=device)
        self.norms = torch.zeros(MAX_GROUPS + 1, dtype=torch.float32, device=device)
        self.coef = torch.ones(MAX_GROUPS, dtype=torch.float32, device=device)
        self._slots = None                                                    # scratch of the scan, grown outside captures

    def slots(self, n_words: int) -> torch.Tensor:
        return _scan_slots(self, n_words, self.limits)

    def set_limits(self, limits: Sequence[float]) -> bool:
        """``limits``: 33 caps (``inf`` = none; negative or NaN values are refused).  Copies them to the device if they differ from
        what it holds, on the current stream and without waiting for it.  Returns whether anything changed."""
        new = [_f32(v) for v in limits]
        if len(new) != MAX_GROUPS + 1:
            raise ValueError(f"GradClip.set_limits: {len(new)} limits, {MAX_GROUPS + 1} wanted")
        if any(not v >= 0.0 for v in new):
            raise ValueError("GradClip.set_limits: a limit must be a non-negative number or inf")
        if new == self.limits_host:
            return False
        push_words(self.limits, torch.tensor(new, dtype=torch.float32))
        self.limits_host = new
        return True


def _group_tensors(who: str, tensors, groups):
    from . import _lib
    if len(tensors) != len(groups):
        raise ValueError(f"{who}: {len(tensors)} tensors, {len(groups)} group ids")
    for i, (t, g) in enumerate(zip(tensors, groups)):
        if not 0 <= int(g) < MAX_GROUPS:
            raise ValueError(f"{who}: tensor {i}: group {g} is not in range({MAX_GROUPS})")
        _lib.require_gpu_tensor(t, f"{who}: tensor {i}")                       # no CPU fallback: a missing GPU is an error
    return [(t, int(g)) for t, g in zip(tensors, groups) if t.numel() > 0]


def _words(who: str, name: str, t: torch.Tensor, n: int) -> torch.Tensor:
    from . import _lib
    _lib.require_gpu_tensor(t, f"{who}: {name}")
    if t.numel() < n or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous float32 tensor of {n} elements, got {tuple(t.shape)} {t.dtype}")
    return t


@torch.no_grad()
def sumsq_norms(tensors: Sequence[torch.Tensor], groups: Sequence[int], limits: torch.Tensor, out_norms: torch.Tensor,
                out_coef: torch.Tensor, slots: Optional[torch.Tensor] = None) -> None:
    """L2 norms of the fp32 GPU ``tensors`` per group (``groups[i]`` in 0..31) into ``out_norms`` (fp32[33], last the norm over all
    groups) and the clipping factors of ``clip_coefficients(out_norms, limits)`` into ``out_coef`` (fp32[32]); ``limits`` is
    fp32[33] on the device.  One ``fst_sumsq_multi`` launch per 64 tensors plus a finalising one, nothing waits for the device,
    the tensors are only read and must be contiguous (a copy could not be scaled afterwards).  ``slots``: fp32 scratch of
    ``fst_sumsq_slots(len(tensors))`` words (allocated here if None — not under capture).  Deterministic: the same values give the
    same words.  A non-finite norm makes every factor 1.0 (see ``clip_coefficients``)."""
    keep = _group_tensors("sumsq_norms", tensors, groups)
    for name, t, n in (("limits", limits, MAX_GROUPS + 1), ("out_norms", out_norms, MAX_GROUPS + 1), ("out_coef", out_coef, MAX_GROUPS)):
        _words("sumsq_norms", name, t, n)
    if any(not t.is_contiguous() for t, _ in keep):
        raise ValueError("sumsq_norms: the tensors must be contiguous")
    from . import _lib
    lib = _lib.load()
    n_slots = int(lib.fst_sumsq_slots(len(keep)))
    if slots is None:
        slots = torch.empty(max(n_slots, 1), dtype=torch.float32, device=out_norms.device)
    _words("sumsq_norms", "slots", slots, n_slots)
    xs = [t for t, _ in keep]
    _lib.check(lib.fst_sumsq_multi(_ptr_array(xs), _i64_array([x.numel() for x in xs]), _i32_array([g for _, g in keep]), len(xs), slots.data_ptr(), slots.numel(), limits.data_ptr(), out_norms.data_ptr(),
                                   out_coef.data_ptr(), _lib.stream_ptr()), "fst_sumsq_multi")


@torch.no_grad()
def scale_by_group(tensors: Sequence[torch.Tensor], groups: Sequence[int], coef: torch.Tensor) -> None:
    """``tensors[i] *= coef[groups[i]]`` in place (fp32 GPU tensors, contiguous; ``coef`` fp32[32] on the device, read when the
    kernels run): one ``fst_scale_multi`` launch per 64 tensors.  A tensor whose factor is exactly 1.0 is neither read nor
    written: it keeps its bits, NaN payloads and −0 included."""
    keep = _group_tensors("scale_by_group", tensors, groups)
    _words("scale_by_group", "coef", coef, MAX_GROUPS)
    if any(not t.is_contiguous() for t, _ in keep):
        raise ValueError("scale_by_group: the tensors must be contiguous (a copy would be scaled in their place)")
    if not keep:
        return
    from . import _lib
    xs = [t for t, _ in keep]
    _lib.check(_lib.load().fst_scale_multi(_ptr_array(xs), _i64_array([x.numel() for x in xs]), _i32_array([g for _, g in keep]),
                                           len(xs), coef.data_ptr(), _lib.stream_ptr()), "fst_scale_multi")


# ---- weight averaging: an exponential moving average of the weights, kept and steered on the device
class WeightAverage:
    """The device words of the weight averaging, one block of 66 4-byte words (``fst_ema_multi``'s ``state_dev``): ``decay``
    (fp32), ``warmup`` (int32 flag), ``count`` (int32[32], completed updates per group) and ``w`` (fp32[32], the weight the last
    ``ema_update`` applied per group, 0 for a group it left alone) are views of ``words``.  ``decay_host`` / ``warmup_host`` are what
    the first two hold, known without reading them back; ``set_decay`` changes both sides with one stream-ordered copy, which a
    graph replayed afterwards sees."""

    def __init__(self, device, decay: float = 0.999, warmup: bool = True):
        self.device = torch.device(device)
        self.decay_host, self.warmup_host = self._checked(decay), bool(warmup)
        self.words = torch.zeros(2 + 2 * MAX_GROUPS, dtype=torch.int32, device=device)
        self.decay = self.words[0:1].view(torch.float32)
        self.warmup = self.words[1:2]
        self.count = self.words[2: 2 + MAX_GROUPS]
        self.w = self.words[2 + MAX_GROUPS:].view(torch.float32)
        self.words[:2].copy_(self._head())

    @staticmethod
    def _checked(decay) -> float:
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"weight average: decay must be a number in [0, 1], got {decay!r}")
        return _f32(decay)

    def _head(self) -> torch.Tensor:
        return torch.cat([torch.tensor([self.decay_host], dtype=torch.float32).view(torch.int32),
                          torch.tensor([int(self.warmup_host)], dtype=torch.int32)])

    def set_decay(self, decay: Optional[float] = None, warmup: Optional[bool] = None) -> bool:
        """``decay`` in [0, 1] and / or the warm-up flag (None keeps the current one).  Copies them to the device if they differ
        from what it holds, on the current stream and without waiting for it.  Returns whether anything changed."""
        new = (self.decay_host if decay is None else self._checked(decay), self.warmup_host if warmup is None else bool(warmup))
        if new == (self.decay_host, self.warmup_host):
            return False
        self.decay_host, self.warmup_host = new
        push_words(self.words[:2], self._head())
        return True


def _pairs(who: str, a: Sequence[torch.Tensor], b: Sequence[torch.Tensor]):
    if len(a) != len(b):
        raise ValueError(f"{who}: {len(a)} and {len(b)} tensors")
    for i, (x, y) in enumerate(zip(a, b)):
        if x.dtype != torch.float32 or y.dtype != torch.float32:
            raise TypeError(f"{who}: pair {i} must be float32, got {x.dtype} and {y.dtype}")
        if x.shape != y.shape or x.device != y.device:
            raise ValueError(f"{who}: pair {i}: {tuple(x.shape)} on {x.device} and {tuple(y.shape)} on {y.device}")
        if not (x.is_contiguous() and y.is_contiguous()):
            raise ValueError(f"{who}: pair {i} must be contiguous (a copy would be written in its place)")


def _active_mask(who: str, active) -> int:
    if isinstance(active, int) and not isinstance(active, bool):
        if not 0 <= active < 1 << MAX_GROUPS:
            raise ValueError(f"{who}: the mask of active groups must fit {MAX_GROUPS} bits, got {active}")
        return active
    mask = 0
    for g in active:
        if not 0 <= int(g) < MAX_GROUPS:
            raise ValueError(f"{who}: active group {g} is not in range({MAX_GROUPS})")
        mask |= 1 << int(g)
    return mask


@torch.no_grad()
def ema_update(avg: Sequence[torch.Tensor], live: Sequence[torch.Tensor], groups: Sequence[int], state: WeightAverage, active,
               guard: Optional[AnomalyGuard] = None) -> None:
    """One update of the averages: ``avg[i] = fma(w, live[i] − avg[i], avg[i])`` with ``w = state.w[groups[i]]``, which this call
    first sets on the device, from the words as they are when the kernels run: for a group of ``active`` (group ids, or a bit mask)
    ``w = 1 − d``, ``d = state.decay`` or, warming up, ``min(decay, (1 + count) / (10 + count))`` — the warm-up of
    ``tf.train.ExponentialMovingAverage(num_updates=)`` — and ``state.count`` advances; every other group, and every group when ``guard.verdict`` is non-zero,
    takes ``w = 0`` and keeps averages and count bit for bit.  fp32 tensors, contiguous, same shapes; ``live`` is only read.  One
    ``fst_ema_multi`` launch per 64 pairs behind a one-workgroup prologue; nothing waits for the device.  On CPU tensors the same
    words and ``torch.lerp`` (host-logic tests): the same quantity, not the same bits — for ``w`` ≥ 0.5 lerp evaluates
    ``live − (live − avg)·(1 − w)``, and below it may or may not fuse the multiply-add; the kernel's formula is the definition."""
    _pairs("ema_update", avg, live)
    if len(groups) != len(avg):
        raise ValueError(f"ema_update: {len(avg)} tensors, {len(groups)} group ids")
    for i, g in enumerate(groups):
        if not 0 <= int(g) < MAX_GROUPS:
            raise ValueError(f"ema_update: tensor {i}: group {g} is not in range({MAX_GROUPS})")
    mask = _active_mask("ema_update", active)
    keep = [(a, l, int(g)) for a, l, g in zip(avg, live, groups) if a.numel() > 0]
    if state.device.type != "cuda":
        skip = guard is not None and int(guard.verdict.item()) != 0
        d, warm = state.decay.clone(), bool(int(state.warmup))
        for g in range(MAX_GROUPS):
            if skip or not (mask >> g) & 1:
                state.w[g] = 0.0
                continue
            c = state.count[g].to(torch.float32)
            state.w[g] = (1.0 - (torch.minimum(d, (1.0 + c) / (10.0 + c)) if warm else d))[0]
            state.count[g] += 1
        for a, l, g in keep:
            w = float(state.w[g])
            if w == 1.0:
                a.copy_(l)
            elif w != 0.0:
                a.lerp_(l, w)
        return
    from . import _lib
    for i, (a, l, _) in enumerate(keep):
        _lib.require_gpu_tensor(a, f"ema_update: avg {i}"); _lib.require_gpu_tensor(l, f"ema_update: live {i}")
    _lib.check(_lib.load().fst_ema_multi(_ptr_array([a for a, _, _ in keep]), _ptr_array([l for _, l, _ in keep]),
                                         _i64_array([a.numel() for a, _, _ in keep]), _i32_array([g for _, _, g in keep]), len(keep),
                                         _mask_i32(mask), state.words.data_ptr(), None if guard is None else guard.verdict.data_ptr(),
                                         _lib.stream_ptr()), "fst_ema_multi")


@torch.no_grad()
def swap_tensors(a: Sequence[torch.Tensor], b: Sequence[torch.Tensor]) -> None:
    """Exchange ``a[i]`` and ``b[i]`` in place, element for element (fp32, contiguous, same shapes): one ``fst_swap_multi`` launch
    per 64 pairs.  Twice is the identity on every bit.  No version counter moves: whatever was derived from either tensor before
    (a packed weight image, a folded BatchNorm) is stale afterwards."""
    _pairs("swap_tensors", a, b)
    keep = [(x, y) for x, y in zip(a, b) if x.numel() > 0]
    if not keep:
        return
    if not keep[0][0].is_cuda:
        for x, y in keep:
            t = x.clone()
            x.copy_(y); y.copy_(t)
        return
    from . import _lib
    for i, (x, y) in enumerate(keep):
        _lib.require_gpu_tensor(x, f"swap_tensors: a {i}"); _lib.require_gpu_tensor(y, f"swap_tensors: b {i}")
    _lib.check(_lib.load().fst_swap_multi(_ptr_array([x for x, _ in keep]), _ptr_array([y for _, y in keep]),
                                          _i64_array([x.numel() for x, _ in keep]), len(keep), _lib.stream_ptr()), "fst_swap_multi")


@contextlib.contextmanager
def exchanged(a: Sequence[torch.Tensor], b: Sequence[torch.Tensor], caches, owner, flag: str, who: str):
    """The scope of ``averaged_weights()`` and ``best_weights()``: ``swap_tensors(a, b)`` on entry and again on exit, the
    ``W_inverse`` attributes that the objects ``caches`` hold (derived from the weights outside any ``ops.pack_cache()``) set aside
    meanwhile — what is cached inside belongs to the exchanged weights and is dropped — and ``owner.<flag>`` true inside.
    Refuses when nested and inside an open ``ops.pack_cache()`` scope; ``who`` names the caller in the messages."""
    from . import ops
    if getattr(owner, flag):
        raise RuntimeError(f"{who}: already inside; the context does not nest")
    if ops._PACK_CACHE is not None:
        raise RuntimeError(f"{who}: inside an ops.pack_cache() scope, whose packed weights and BatchNorm folds would be stale "
                           "after the exchange; enter it outside")
    swap_tensors(a, b)                                                        # (refuses before it exchanges anything)
    aside = [c.__dict__.pop("W_inverse", None) for c in caches]
    setattr(owner, flag, True)
    try:
        yield owner
    finally:
        try:
            swap_tensors(a, b)
        finally:
            setattr(owner, flag, False)
            for c, w in zip(caches, aside):
                c.__dict__.pop("W_inverse", None)
                if w is not None:
                    c.W_inverse = w


# ---- gradient accumulation: one optimiser step over a window of k calls, the position in the window a device word
class GradAccumulation:
    """The device words of the gradient accumulation, one 16-byte aligned block of eight 4-byte words (``fst_accum_multi``'s
    ``state_dev``): ``k`` (int32, calls per window), ``j`` (int32, folds done in the open window), ``inv_k`` (fp32,
    ``float32(1 / k)``) and ``windows`` (int32, closed windows) are views of ``words``; four words are reserved.  ``steps_host`` is
    what ``k`` holds and ``pending`` what ``j`` holds once the stream has run what was issued, both known without reading them
    back: ``accumulate(..., advance=True)`` moves ``pending`` with the launch it issues, and whoever replays a captured such launch
    calls ``advance_host()`` beside it.  ``set_steps`` changes ``k`` and ``inv_k`` with one stream-ordered copy, which a graph replayed
    afterwards reads."""

    def __init__(self, device, steps: int = 1):
        self.device = torch.device(device)
        self.steps_host, self.pending = self._checked(steps), 0
        self.words = torch.zeros(8, dtype=torch.int32, device=device)
        if self.words.data_ptr() % 16:
            raise RuntimeError("GradAccumulation: the allocator returned a block off a 16-byte boundary")
        self.k, self.j, self.windows = self.words[0:1], self.words[1:2], self.words[3:4]
        self.inv_k = self.words[2:3].view(torch.float32)
        self.words[:3].copy_(self._head())

    @staticmethod
    def _checked(steps) -> int:
        if isinstance(steps, bool) or not isinstance(steps, int) or not 1 <= steps < 1 << 24:
            raise ValueError(f"gradient accumulation: steps must be an integer in 1..2^24 - 1, got {steps!r}")
        return steps

    def _head(self) -> torch.Tensor:
        """k, j = 0 and inv_k: the first three words between two windows."""
        inv = torch.tensor([np.float32(1.0) / np.float32(self.steps_host)], dtype=torch.float32)
        return torch.cat([torch.tensor([self.steps_host, 0], dtype=torch.int32), inv.view(torch.int32)])

    def set_steps(self, steps: int) -> bool:
        """Calls per window from now on.  Between windows only (``pending == 0``, where ``j`` is 0 as well: the one copy carries
        ``k``, that 0 and ``inv_k`` from pinned memory, on the current stream and without waiting for it).  Returns whether
        anything changed."""
        steps = self._checked(steps)
        if self.pending != 0:
            raise RuntimeError(f"gradient accumulation: a window is open ({self.pending} of {self.steps_host} calls done); change "
                               "the number of steps between windows")
        if steps == self.steps_host:
            return False
        self.steps_host = steps
        push_words(self.words[:3], self._head())
        return True

    @property
    def closing_next(self) -> bool:
        """Will the next advancing call close its window?"""
        return self.pending + 1 >= self.steps_host

    def advance_host(self) -> None:
        self.pending = 0 if self.closing_next else self.pending + 1


@torch.no_grad()
def accumulate(acc: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], state: GradAccumulation, advance: bool = True) -> None:
    """Fold ``grads[i]`` into ``acc[i]`` (fp32, contiguous, same shapes) at the window position the device words of ``state`` hold
    when the kernels run: ``acc = g`` on a window's first call (``acc`` is not read), ``acc += g`` on the others, and on the call
    that closes the window also ``g = acc · inv_k`` in place; on every other call ``g`` is only read, and with ``k == 1`` nothing
    is touched.  ``advance``: move the window on behind the folds (``j`` and ``state.pending``); several calls with
    ``advance=False`` and a last one with ``advance=True`` all fold at the same position.  One ``fst_accum_multi`` launch per 64
    pairs; nothing waits for the device.  On CPU tensors the same recurrence in plain torch fp32 — every operation is one IEEE
    addition or multiplication, so the bits are the kernel's."""
    _pairs("accumulate", acc, grads)
    keep = [(a, g) for a, g in zip(acc, grads) if a.numel() > 0]
    if any(a.device != state.words.device for a, _ in keep):
        raise ValueError(f"accumulate: the tensors must live on the state's device, {state.words.device}")
    if state.device.type != "cuda":
        k, j = int(state.k), int(state.j)
        first, closing = j == 0, j + 1 >= k
        if k > 1:
            for a, g in keep:
                if first:
                    a.copy_(g)
                else:
                    a.add_(g)
                if closing:
                    torch.mul(a, state.inv_k[0], out=g)
        if advance:
            state.j.fill_(0 if closing else j + 1)
            state.windows.add_(int(closing))
            state.advance_host()
        return
    from . import _lib
    for i, (a, g) in enumerate(keep):
        _lib.require_gpu_tensor(a, f"accumulate: acc {i}"); _lib.require_gpu_tensor(g, f"accumulate: grad {i}")
    _lib.check(_lib.load().fst_accum_multi(_ptr_array([a for a, _ in keep]), _ptr_array([g for _, g in keep]),
                                           _i64_array([a.numel() for a, _ in keep]), len(keep), state.words.data_ptr(),
                                           int(bool(advance)), _lib.stream_ptr()), "fst_accum_multi")
    if advance and not _capturing(state.words):                               # a captured launch has not run: its replayer counts
        state.advance_host()
