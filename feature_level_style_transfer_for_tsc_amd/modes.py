"""The device-side modes the two trainers of step.py share, as mixins.

Weight averaging (``enable_weight_average()``): an exponential moving average of the weights, moved on the device as the last thing
of a step, in eager and in captured steps alike; ``averaged_weights()`` puts it to use.

Gradient accumulation (``enable_grad_accumulation(steps)``): one optimiser step over ``steps`` consecutive calls, each on its own
micro-batch; the gradients, GradNorm's ten scalars and the loss scalars are folded into fp32 accumulators at a window position kept
on the device, and everything behind the backward runs on the call that closes the window, on their means.

Device-resident input (``attach_feeder()``): a ``data.EpochFeeder`` plans an epoch once and the ``*_fed`` methods draw every batch
from device memory.
"""
from __future__ import annotations

import contextlib
from typing import Dict, Optional

import torch
import torch.nn as nn

from .optim import _capturing, AnomalyGuard, GradAccumulation, WeightAverage, accumulate, ema_update, exchanged


def _enable_from_arg(enable, arg, scalar: str) -> None:
    """A constructor's mode argument: None / False leave the mode off; True calls ``enable()``, a dict ``enable(**arg)`` and
    anything else ``enable(<scalar>=arg)``."""
    if arg is None or arg is False:
        return
    if arg is True:
        enable()
    elif isinstance(arg, dict):
        enable(**arg)
    else:
        enable(**{scalar: arg})


class _Mode:
    """What the mixins ask of a trainer: ``device`` and ``_capture_resident()``."""

    def _capture_resident(self) -> bool:
        """Is a capture resident, whose launches are those of the modes as they were then?"""
        raise NotImplementedError

    def _refuse_resident(self, what: str) -> None:
        if self._capture_resident():
            raise RuntimeError(f"{what}: a capture is resident; enable the mode before capturing")


class _WeightAveraging(_Mode):
    """Weight averaging of the two trainers.  A trainer supplies ``_ema_modules()`` ({group name: module}, in group order); it
    calls ``_ema_update`` as the last thing of a step and ``_ema_no_step`` as the first."""
    weight_average: Optional[WeightAverage] = None                            # the device words; None while the mode is off
    _ema_avg: Dict[str, Dict[str, torch.Tensor]] = {}                         # module -> state_dict name -> the average
    _ema_live: Dict[str, Dict[str, torch.Tensor]] = {}                        # ... -> the live tensor (addresses never change)
    _ema_inside = False                                                       # inside averaged_weights()

    def _ema_modules(self) -> Dict[str, nn.Module]:
        raise NotImplementedError

    def enable_weight_average(self, decay: float = 0.999, warmup: bool = True) -> None:
        """From now on every step ends by moving an exponential moving average of the weights towards the weights it has just
        written: for every module a copy of each parameter and of each fp32 buffer of its ``state_dict()`` (BatchNorm running
        statistics are averaged like parameters, as timm's ``ModelEma`` does; integer buffers are not averaged),
        ``avg ← avg + w·(live − avg)`` with ``w = 1 − decay``, or while ``warmup`` lasts ``1 − min(decay, (1 + n) / (10 + n))``
        after ``n`` updates of that module.  Decided and applied on the device with no host read, alike in eager and in captured
        steps; only the modules a step's optimisers stepped are averaged, and a step the anomaly guard skips leaves averages
        and counts as they were.  The averages only read the weights: the training trajectory is that of the mode off, bit for
        bit.  ``averaged_weights()`` puts them to use; ``set_weight_average`` steers the decay, under resident captures too.
        Idempotent (a second call changes nothing, its arguments included); raises while a capture is resident, whose launches lack the update."""
        if self.weight_average is not None:
            return
        state = WeightAverage(self.device, decay, warmup)                     # (refuses a bad decay before anything changes)
        self._refuse_resident("enable_weight_average()")
        # the live tensors are listed once: every loader of this package writes them in place, and the exchange of
        # averaged_weights() depends on their addresses staying what they are anyway
        self._ema_live = {k: {n: t for n, t in mod.state_dict().items() if t.dtype == torch.float32}
                          for k, mod in self._ema_modules().items()}
        self._ema_avg = {k: {n: t.detach().clone(memory_format=torch.contiguous_format) for n, t in d.items()}
                         for k, d in self._ema_live.items()}
        self.weight_average = state

    def set_weight_average(self, decay: Optional[float] = None, warmup: Optional[bool] = None) -> bool:
        """Change the decay and / or the warm-up flag (an argument left out keeps its value).  Legal while captures are
        resident: one stream-ordered copy into the device words, which a graph replayed afterwards reads — no re-capture.
        Returns whether the device words changed."""
        if self.weight_average is None:
            raise RuntimeError("set_weight_average(): call enable_weight_average() first")
        return self.weight_average.set_decay(decay, warmup)

    def _ema_pairs(self, names):
        """(averages, live tensors, group ids) of the modules ``names``, in a fixed order."""
        order = list(self._ema_avg)
        avg, live, groups = [], [], []
        for k in names:
            for n, a in self._ema_avg[k].items():
                avg.append(a); live.append(self._ema_live[k][n]); groups.append(order.index(k))
        return avg, live, groups

    def _ema_update(self, names, guard: Optional[AnomalyGuard] = None) -> None:
        if self.weight_average is None:
            return
        avg, live, groups = self._ema_pairs(names)
        ema_update(avg, live, groups, self.weight_average, sorted(set(groups)), guard)

    def _ema_no_step(self, what: str) -> None:
        if self._ema_inside:
            raise RuntimeError(f"{what}: inside averaged_weights() the modules hold the averages and the averages' tensors the live "
                               "weights; leave the context first")

    def _ema_report(self, live: bool = False) -> Dict[str, torch.Tensor]:
        """The mode's report entries: fresh copies, or with ``live`` views of the device words themselves."""
        n = len(self._ema_avg)
        out = {"ema_weight": self.weight_average.w[:n], "ema_steps": self.weight_average.count[:n]}
        return out if live else {k: v.clone() for k, v in out.items()}

    def _ema_caches(self) -> list:
        """Objects whose attribute ``W_inverse`` caches something derived from the weights outside any ``ops.pack_cache()``."""
        return []

    @contextlib.contextmanager
    def averaged_weights(self):
        """Context manager: inside it the modules hold the AVERAGED weights and fp32 buffers — one in-place exchange with the
        averages on entry, the same exchange on exit, after which every live bit is what it was.  The addresses do not change,
        so captured graphs stay valid, and ``eval_accuracy``, ``collect_logits`` and the ``save_*_classification_modules``
        functions work on the averaged model unchanged: a checkpoint saved inside is a reference-format ``.tar`` of it.  The
        modules' train / eval mode is the caller's business, as in ``eval_accuracy``.  The flow's cached 1x1 inverses (quirk Q2)
        are set aside on entry and put back on exit; what is cached inside belongs to the averaged weights and is dropped.
        Raises inside an open ``ops.pack_cache()`` scope (the exchange moves no version counter: a packed image or a BatchNorm
        fold made before it would be stale) and when nested; inside it the trainer's step, replay and capture methods and its
        state methods (``snapshot`` / ``restore`` / ``state_dict`` / ``load_state_dict``) raise: they would train on, or save
        and load, the two sets exchanged."""
        if self.weight_average is None:
            raise RuntimeError("averaged_weights(): call enable_weight_average() first")
        avg, live, _ = self._ema_pairs(list(self._ema_avg))
        with exchanged(avg, live, self._ema_caches(), self, "_ema_inside", "averaged_weights()"):
            yield self

    def _ema_state_dict(self) -> dict:
        st = self.weight_average
        return {"decay": st.decay_host, "warmup": st.warmup_host, "counts": st.count.cpu().tolist(),
                "tensors": {k: {n: t.detach().cpu().clone() for n, t in d.items()} for k, d in self._ema_avg.items()}}

    def _ema_load_state_dict(self, sd: dict) -> None:
        """In place: a resident capture keeps valid addresses."""
        if self.weight_average is None:
            self.enable_weight_average(sd["decay"], sd["warmup"])
        self.weight_average.set_decay(sd["decay"], sd["warmup"])
        with torch.no_grad():
            self.weight_average.count.copy_(torch.tensor(sd["counts"], dtype=torch.int32))
            for k, d in self._ema_avg.items():
                if set(d) != set(sd["tensors"][k]):
                    raise KeyError(f"weight average of {k!r}: the checkpoint's tensors are not this module's")
                for n, t in d.items():
                    t.copy_(sd["tensors"][k][n])


class _GradAccumulating(_Mode):
    """Gradient accumulation of the two trainers: one optimiser step over a WINDOW of ``steps`` consecutive calls, each on its own
    micro-batch.  A trainer calls ``_accum_fold`` behind a micro-step's backward and runs its update only on the call that closes a
    window (``_closing``, read before the fold that moves the window on)."""
    grad_accumulation: Optional[GradAccumulation] = None                      # the device words; None while the mode is off
    _accum: Dict[nn.Parameter, torch.Tensor] = {}                             # parameter -> its fp32 accumulator (addresses never change)

    def enable_grad_accumulation(self, steps: int = 1) -> None:
        """From now on ``steps`` consecutive calls of ``step`` / ``replay`` / ``phase_step`` form a window.  Every call runs its own
        forward and backward unchanged — batch-coupled quantities (BatchNorm moments, CPC negatives, NoiseTransfer means, CDAN
        sums) are per micro-batch, and what is stateful (BatchNorm running statistics, ``NoiseTransfer.advance``, the GRL counters)
        advances per call — and then folds each gradient into a persistent fp32 accumulator: ``acc = g`` on a window's first
        call, ``acc += g`` after; the call that closes the window writes ``g = acc · float32(1 / steps)`` back into the gradient
        tensors and alone runs what follows the backward: the data-parallel all-reduce, ``on_grads_ready``, clip, guard,
        GradNorm's weight update, the optimisers, the WGAN clamps, the roll-back and the weight average.  A call that does not
        close a window changes no parameter, no optimiser moment, no GradNorm weight and no average.  The position in the window
        is a device word (``optim.GradAccumulation``), so one captured micro-step serves every position; ``accum_pending`` is
        its host mirror.  ``steps == 1`` computes the bits of the mode off.  ``set_grad_accumulation`` steers ``steps`` between
        windows, under resident captures too.  Idempotent (a second call changes nothing, its argument included); raises while
        a capture is resident, whose launches are the one-graph layout."""
        if self.grad_accumulation is not None:
            return
        state = GradAccumulation(self.device, steps)                          # (refuses a bad count before anything changes)
        self._refuse_resident("enable_grad_accumulation()")
        self._accum = {}
        self.grad_accumulation = state

    def set_grad_accumulation(self, steps: int) -> bool:
        """Calls per window from now on; between windows only.  Legal while captures are resident: one stream-ordered copy into
        the device words, which a graph replayed afterwards reads — no re-capture.  Returns whether the device words changed."""
        if self.grad_accumulation is None:
            raise RuntimeError("set_grad_accumulation(): call enable_grad_accumulation() first")
        return self.grad_accumulation.set_steps(steps)

    @property
    def accum_pending(self) -> int:
        """Calls done in the open window (0 between windows, and with the mode off)."""
        return 0 if self.grad_accumulation is None else self.grad_accumulation.pending

    @property
    def _closing(self) -> bool:
        """Will the next call close its window?  Always, with the mode off."""
        return self.grad_accumulation is None or self.grad_accumulation.closing_next

    def _accum_closed(self, what: str) -> None:
        if self.accum_pending:
            raise RuntimeError(f"{what}: a gradient-accumulation window is open ({self.accum_pending} of "
                               f"{self.grad_accumulation.steps_host} calls done); close it first")

    def _accum_fold(self, params, advance: bool) -> None:
        """Fold the gradients of ``params`` at the window's current position; the accumulators are made at a parameter's first fold."""
        acc, grads = [], []
        for p in params:
            if p.grad is None:
                continue
            if not p.grad.is_contiguous():
                p.grad = p.grad.contiguous()
            a = self._accum.get(p)
            if a is None:
                if _capturing(p.grad):
                    raise RuntimeError("gradient accumulation: a gradient has no accumulator yet; run one eager window before capturing")
                a = self._accum[p] = torch.empty_like(p.grad, memory_format=torch.contiguous_format)
            acc.append(a); grads.append(p.grad)
        accumulate(acc, grads, self.grad_accumulation, advance)


class _WindowOpens:
    """``guard_copy``'s predicate word of a save under gradient accumulation: the window's position ``j`` in the place of a verdict."""

    def __init__(self, acc: GradAccumulation):
        self.verdict = acc.j


class _Fed:
    """Device-resident input of the two trainers: an attached ``data.EpochFeeder`` plans an epoch once and the ``*_fed`` methods
    draw every batch from device memory — into the captures' own static inputs, or into buffers kept here for the eager steps.
    A fed method creates no tensor on the host, issues no host-to-device copy and waits for nothing: the feed is one launch pair
    in front of what the unfed method issues, and is never captured."""
    feeder = None
    _fed_kind: Optional[str] = None                                           # what begin_epoch planned ("joint", a phase, "classifier")
    _fed_buf: Optional[dict] = None                                           # the eager steps' batch, CPC indices and ratios

    def attach_feeder(self, feeder) -> None:
        """Use ``feeder`` from now on (None: detach).  An epoch has to be begun (``begin_epoch``) before the first fed call."""
        if feeder is not None and torch.device(feeder.device).type != torch.device(self.device).type:
            raise ValueError(f"attach_feeder(): the feeder lives on {feeder.device}, the trainer on {self.device}")
        self.feeder, self._fed_kind, self._fed_buf = feeder, None, None

    def _fed_begin(self, kind: str, ratios=None) -> int:
        if self.feeder is None:
            raise RuntimeError("begin_epoch(): call attach_feeder() first")
        rounds = self.feeder.begin_epoch(ratios)
        self._fed_kind = kind
        return rounds

    def _fed_check(self, kind: str, what: str) -> None:
        if self.feeder is None:
            raise RuntimeError(f"{what}: call attach_feeder() and begin_epoch() first")
        if self._fed_kind is None:
            raise RuntimeError(f"{what}: no epoch is planned; call begin_epoch() first")
        if kind != self._fed_kind:
            raise RuntimeError(f"{what}: the epoch was begun for {self._fed_kind!r}, not for {kind!r}")

    def _fed_eager(self) -> dict:
        """Feed the current round into the buffers the trainer keeps for its eager steps (made at the first call)."""
        f = self.feeder
        if self._fed_buf is None:
            batch = []
            for d, b in zip(f.sets, f.batch):
                batch += [torch.empty((b,) + tuple(d.x.shape[1:]), dtype=torch.float32, device=f.device),
                          torch.empty((b,) + tuple(d.y.shape[1:]), dtype=torch.int64, device=f.device)]
            self._fed_buf = {"batch": batch, "t": torch.zeros(2, dtype=torch.int32, device=f.device), "r": torch.ones(2, device=f.device)}
        b = self._fed_buf
        f.feed(*b["batch"], t=b["t"], r=b["r"])
        return b

    def _fed_state_dict(self) -> dict:
        return {} if self.feeder is None else {"feeder": {"kind": self._fed_kind, **self.feeder.state_dict()}}

    def _fed_load_state_dict(self, sd: dict) -> None:
        """A "feeder" entry goes into the attached feeder; without one attached, or without the entry, nothing happens."""
        if "feeder" in sd and self.feeder is not None:
            self.feeder.load_state_dict(sd["feeder"])
            self._fed_kind = sd["feeder"]["kind"]
