"""Evaluation on the device (the pass of utils.py:27-183, which the reference runs up to four times per epoch).

``Evaluator`` ties three pieces together: a resident ``DeviceDataset`` served by a sequential ``EvalPlan`` (``fst_feed_batch``),
the folded-BatchNorm inference forward, and ``ops.eval_fold`` / ``ops.eval_finish`` (csrc/eval.hip), which keep rows seen, hits,
the confusion matrix, the fp64 loss, every prediction and the best-so-far words on the device.  ``run()`` is one eager pass;
``capture()`` / ``replay()`` run the same pass as two hipGraphs that share a pool — a *prepare* graph (rewind, zero the words, and
round 0, whose forward folds the BatchNorms and packs the weights from the live parameter storage) and a *batch* graph (feed,
forward, fold) replayed once per later round — with no host tensor, no copy and no wait.  ``track_best`` keeps the weights of the
best pass in a shadow on the device (``optim.guard_copy`` under the ``improved`` word), so model selection needs no host round
trip either.

Every batch, the last partial one included, runs at the static shape ``[B, ...]``: the tail is padded with the set's last row and
``eval_fold`` reads only the valid rows.  Eager and replayed passes so issue the same kernels on the same inputs.
"""
from __future__ import annotations

import contextlib
from typing import Dict, Optional, Sequence, Union

import torch
import torch.nn as nn

from . import ops
from .data import DeviceDataset, EvalPlan
from .optim import guard_copy, swap_tensors

__all__ = ["Evaluator"]

_CAPTURE_MODE = "thread_local"
_METRICS = {"accuracy": 0, "loss": 1}


class _Improved:
    """``guard_copy``'s predicate word of the best-weights save: the ``improved`` word of ``fst_eval_finish`` in the place of a verdict."""

    def __init__(self, best: torch.Tensor):
        self.verdict = best[ops.EVAL_IMPROVED: ops.EVAL_IMPROVED + 1]


class Evaluator:
    """Evaluate ``classification_module(feature_trans(feature_extraction_module(x)))`` over ``data`` in batches of ``batch_size``.

    ``n_class``: the number of classes (default: ``classification_module.hidden.out_features``).  ``feature_trans``: the source
    side's DimensionUnification.  ``keep_logits``: also keep every row's logits, ``[N, C]``, on the device.  The classifier may
    return the logits or a tuple whose first entry they are.  ``accuracy`` and the mean ``loss`` divide by ``len(data)``."""

    def __init__(self, feature_extraction_module: nn.Module, classification_module: nn.Module, data: DeviceDataset, batch_size: int,
                 n_class: Optional[int] = None, feature_trans: Optional[nn.Module] = None, keep_logits: bool = False):
        if n_class is None:
            hidden = getattr(classification_module, "hidden", None)
            if not isinstance(hidden, nn.Linear):
                raise ValueError("Evaluator: n_class is needed (the classifier has no Linear `hidden` to read it from)")
            n_class = hidden.out_features
        if isinstance(n_class, bool) or not isinstance(n_class, int) or not 1 <= n_class <= ops.EVAL_MAX_C:
            raise ValueError(f"Evaluator: n_class must be in 1..{ops.EVAL_MAX_C}, got {n_class!r}")
        self.fe, self.clf, self.feature_trans = feature_extraction_module, classification_module, feature_trans
        self.data, self.device, self.n_class, self.keep_logits = data, data.device, n_class, bool(keep_logits)
        self.plan = EvalPlan(data, batch_size)
        self.batch, self.rounds, self.n = batch_size, self.plan.rounds, len(data)
        dev, B, C, N = self.device, batch_size, n_class, self.n
        # the static inputs of every batch, eager or captured
        self._x = torch.zeros((B,) + tuple(data.x.shape[1:]), dtype=torch.float32, device=dev)
        self._y = torch.zeros(B, dtype=torch.int64, device=dev)
        self._valid = torch.zeros(1, dtype=torch.int32, device=dev)
        # the words of a pass as ONE block, zeroed by one fill: state (8 int32), loss (fp64), confusion (C x C int32)
        self._pass = torch.zeros(10 + C * C, dtype=torch.int32, device=dev)
        if self._pass.data_ptr() % 16:
            raise RuntimeError("Evaluator: the allocator returned a block off a 16-byte boundary")
        self.state, self.loss, self.confusion = self._pass[:8], self._pass[8:10].view(torch.float64), self._pass[10:].view(C, C)
        self.predictions = torch.zeros(N, dtype=torch.int64, device=dev)
        self.logits = torch.zeros(N, C, dtype=torch.float32, device=dev) if keep_logits else None
        self.best = ops.eval_best_block(dev)
        self._scratch = ops.eval_scratch(B, dev) if dev.type == "cuda" else None
        self.metric = "accuracy"
        self._finish_call = ops.EvalFinishCall(self.state, self.loss, N, self.best, 0)
        self._improved = _Improved(self.best)
        self._live: Dict[str, torch.Tensor] = {}                              # track_best: name -> live tensor
        self._shadow: Dict[str, torch.Tensor] = {}                            # ... -> the copy of the best pass
        self._tracked: Sequence[nn.Module] = ()
        self._inside = False                                                  # inside best_weights()
        self._graphs = None                                                   # (prepare, batch) once captured
        self._cache: Optional[dict] = None                                    # the capture-time pack cache, kept alive here

    # ------------------------------------------------------------------ the pass
    def _modules(self):
        return [m for m in (self.fe, self.feature_trans, self.clf) if m is not None]

    @contextlib.contextmanager
    def _eval_mode(self):
        mods = self._modules()
        modes = [m.training for m in mods]
        for m in mods:
            m.eval()
        try:
            with torch.no_grad():
                yield
        finally:
            for m, mode in zip(mods, modes):
                m.train(mode)

    def _forward(self) -> torch.Tensor:
        f = self.fe(self._x)
        if self.feature_trans is not None:
            f = self.feature_trans(f)
        out = self.clf(f)
        logits = out[0] if isinstance(out, (tuple, list)) else out
        if logits.dim() != 2 or logits.shape != (self.batch, self.n_class) or logits.dtype != torch.float32:
            raise ValueError(f"Evaluator: the classifier returned {tuple(logits.shape)} {logits.dtype}; fp32 [{self.batch}, {self.n_class}] expected")
        return logits

    def _fold_call(self, logits: torch.Tensor) -> ops.EvalFoldCall:
        return ops.EvalFoldCall(logits, self._y, self._valid, self.state, self.loss, self.confusion, self.predictions, self.logits,
                                capacity=self.n, scratch=self._scratch)

    def _begin(self) -> None:
        self.plan.rewind()
        self._pass.zero_()

    def _round(self) -> None:
        self.plan.feed(self._x, self._y, self._valid)
        self._fold_call(self._forward())()

    def _finish(self) -> None:
        self._finish_call()
        if self._shadow:
            names = list(self._shadow)
            guard_copy([self._shadow[k] for k in names], [self._live[k] for k in names], self._improved, when=True)

    def _no_pass(self, what: str) -> None:
        if self._inside:
            raise RuntimeError(f"{what}: inside best_weights() the modules hold the best weights and the shadow the live ones; a pass "
                               "could overwrite them; leave the context first")

    def run(self) -> Dict[str, torch.Tensor]:
        """One eager pass: the modules in eval mode (their modes restored afterwards), under ``torch.no_grad()`` and one
        ``ops.pack_cache()``; per round feed, forward, ``eval_fold``; then ``eval_finish`` (and the best-weights save, if tracked).
        Returns ``report()``: device tensors, no host read."""
        self._no_pass("run()")
        with self._eval_mode(), ops.pack_cache():
            self._begin()
            for _ in range(self.rounds):
                self._round()
        self._finish()
        return self.report()

    def capture(self, warmup: int = 1) -> None:
        """Capture the pass as two hipGraphs sharing a pool.  *prepare*: rewind the plan, zero the pass's words and run round 0 —
        feed, forward, ``eval_fold`` —, whose forward does what the first forward of a pass does once: the BatchNorm folds and the
        weight packing.  *batch*: feed + forward + ``eval_fold`` of every later round, served by the folds and images of
        *prepare*.  Those are recomputed in place by every replay of *prepare* from the live parameter storage, so a replay
        evaluates the weights as they are then.  (A *prepare* that only folded and packed would need a forward whose logits nobody
        reads: one batch's time per pass.)  The objects of the capture-time pack cache are kept alive here; the global
        ``ops.pack_cache()`` scope is left before this returns."""
        self._no_pass("capture()")
        if self.device.type != "cuda":
            raise RuntimeError("Evaluator.capture(): a GPU is needed")
        if ops._PACK_CACHE is not None:
            raise RuntimeError("Evaluator.capture(): inside an ops.pack_cache() scope; capture outside it")
        with self._eval_mode():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(max(1, warmup)):
                    with ops.pack_cache():
                        self._begin()
                        self._round()
                self._begin()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            cache = ops.pack_cache()
            prepare, batch = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with cache:
                self._cache = ops._PACK_CACHE
                with torch.cuda.graph(prepare, capture_error_mode=_CAPTURE_MODE):
                    self._begin()
                    self._g_first = self._captured_round()
                with torch.cuda.graph(batch, pool=prepare.pool(), capture_error_mode=_CAPTURE_MODE):
                    self._g_next = self._captured_round()
        self._graphs = (prepare, batch)

    def _captured_round(self):
        """A round inside a stream capture; returns what must stay alive as long as the graph: the logits and the fold's call."""
        self.plan.feed(self._x, self._y, self._valid)
        logits = self._forward()
        call = self._fold_call(logits)
        call()
        return logits, call

    def replay(self, report: bool = True) -> Optional[Dict[str, torch.Tensor]]:
        """One captured pass: *prepare* once (round 0 with it), *batch* ``rounds - 1`` times, then ``eval_finish`` (and the best-weights save, if
        tracked): launches only — no host tensor, no host-to-device copy, no wait.  Returns ``report()`` (device-side copies of the
        words), or nothing with ``report=False``."""
        self._no_pass("replay()")
        if self._graphs is None:
            raise RuntimeError("call capture() first")
        prepare, batch = self._graphs
        prepare.replay()
        for _ in range(self.rounds - 1):
            batch.replay()
        self._finish()
        return self.report() if report else None

    def release(self) -> None:
        """Drop the captured graphs and what they kept alive."""
        self._graphs = self._cache = None
        self._g_first = self._g_next = None

    # ------------------------------------------------------------------ what a pass leaves
    def report(self) -> Dict[str, torch.Tensor]:
        """The last pass as fresh DEVICE tensors (copies within device memory; no host read): ``seen``, ``hits``, ``accuracy``
        (fp64), ``loss`` (the mean, fp64), ``confusion`` [C, C], ``predictions`` [N], ``labels`` (the resident ``data.y``
        itself), ``logits`` [N, C] with ``keep_logits``; ``improved``, ``best_accuracy`` (NaN before a first best), ``best_loss``,
        ``best_pass``, ``passes``; the counters ``batches``, ``bad_label``, ``nonfinite``, ``overflow``, ``incomplete``."""
        st, best = self.state.clone(), self.best.clone()
        hits, best_hits = st[ops.EVAL_HITS], best[ops.EVAL_BEST_HITS]
        out = {"seen": st[ops.EVAL_SEEN], "hits": hits, "accuracy": hits.to(torch.float64) / self.n,
               "loss": self.loss[0] / self.n, "confusion": self.confusion.clone(), "predictions": self.predictions.clone(),
               "labels": self.data.y, "improved": best[ops.EVAL_IMPROVED],
               "best_accuracy": torch.where(best_hits >= 0, best_hits.to(torch.float64) / self.n, float("nan")),
               "best_loss": ops.eval_best_loss(best)[0] / self.n, "best_pass": best[ops.EVAL_BEST_PASS], "passes": best[ops.EVAL_PASSES],
               "batches": st[ops.EVAL_BATCHES], "bad_label": st[ops.EVAL_BAD_LABEL], "nonfinite": st[ops.EVAL_NONFINITE],
               "overflow": st[ops.EVAL_OVERFLOW], "incomplete": best[ops.EVAL_INCOMPLETE]}
        if self.logits is not None:
            out["logits"] = self.logits.clone()
        return out

    def _read(self, tensors: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """Several device tensors in ONE device-to-host copy (as bytes, widest elements first so every view stays aligned)."""
        order = sorted(tensors, key=lambda k: -tensors[k].element_size())
        flat = torch.cat([tensors[k].contiguous().view(-1).view(torch.uint8) for k in order]).cpu()
        out, at = {}, 0
        for k in order:
            t = tensors[k]
            n = t.numel() * t.element_size()
            out[k] = flat[at: at + n].view(t.dtype).view(t.shape)
            at += n
        return out

    def result(self) -> dict:
        """The last pass with ONE host read (this waits for the device): Python numbers for the words (``loss`` the mean), CPU
        tensors for ``confusion``, ``predictions`` and, with ``keep_logits``, ``logits``; ``feed`` holds the plan's counters."""
        parts = {"state": self.state, "best": self.best, "loss": self.loss, "feed": self.plan.state, "confusion": self.confusion,
                 "predictions": self.predictions}
        if self.logits is not None:
            parts["logits"] = self.logits
        h = self._read(parts)
        st, best = h["state"].tolist(), h["best"].tolist()
        best_loss = float(ops.eval_best_loss(h["best"])[0])
        out = {"seen": st[ops.EVAL_SEEN], "hits": st[ops.EVAL_HITS], "accuracy": st[ops.EVAL_HITS] / self.n,
               "loss": float(h["loss"][0]) / self.n, "confusion": h["confusion"].clone(), "predictions": h["predictions"].clone(),
               "improved": bool(best[ops.EVAL_IMPROVED]),
               "best_accuracy": best[ops.EVAL_BEST_HITS] / self.n if best[ops.EVAL_BEST_HITS] >= 0 else float("nan"),
               "best_loss": best_loss / self.n, "best_pass": best[ops.EVAL_BEST_PASS], "passes": best[ops.EVAL_PASSES],
               "batches": st[ops.EVAL_BATCHES], "bad_label": st[ops.EVAL_BAD_LABEL], "nonfinite": st[ops.EVAL_NONFINITE],
               "overflow": st[ops.EVAL_OVERFLOW], "incomplete": best[ops.EVAL_INCOMPLETE],
               "feed": {"overrun": int(h["feed"][ops.FEED_OVERRUN]), "bad_index": int(h["feed"][ops.FEED_BAD_INDEX])}}
        if self.logits is not None:
            out["logits"] = h["logits"].clone()
        return out

    def check(self) -> None:
        """One host read; raises if the last pass overflowed its capacity or met a label outside ``0..C-1``, if any pass so far
        was incomplete, or if the plan was fed past its end or held an index outside the data set."""
        h = self._read({"state": self.state, "best": self.best, "feed": self.plan.state})
        st, best, feed = h["state"].tolist(), h["best"].tolist(), h["feed"].tolist()
        found = {"overflow": st[ops.EVAL_OVERFLOW], "bad_label": st[ops.EVAL_BAD_LABEL], "incomplete": best[ops.EVAL_INCOMPLETE],
                 "overrun": feed[ops.FEED_OVERRUN], "bad_index": feed[ops.FEED_BAD_INDEX]}
        if any(found.values()):
            raise RuntimeError("Evaluator: " + ", ".join(f"{k} = {v}" for k, v in found.items() if v))

    # ------------------------------------------------------------------ best weights
    def track_best(self, modules: Union[None, nn.Module, Sequence[nn.Module], Dict[str, nn.Module]] = None, metric: str = "accuracy") -> None:
        """From now on every pass, eager or replayed, ends by copying the weights into a shadow if the pass improved on the best so
        far — decided and done on the device (``optim.guard_copy`` under the ``improved`` word, read when the kernel runs).
        ``modules``: a module, a sequence or a dict of them (default: the evaluated ones); the shadow holds a copy of every
        parameter and fp32 buffer of their ``state_dict()``.  ``metric``: "accuracy" (more hits) or "loss" (a smaller fp64 loss
        sum; a NaN never improves).  A tie keeps the earlier pass.  Calling it again starts over: new shadows, fresh best words."""
        self._no_pass("track_best()")
        if metric not in _METRICS:
            raise ValueError(f"track_best(): metric must be one of {sorted(_METRICS)}, got {metric!r}")
        if modules is None:
            modules = self._modules()
        if isinstance(modules, nn.Module):
            modules = [modules]
        named = modules if isinstance(modules, dict) else {str(i): m for i, m in enumerate(modules)}
        live = {f"{k}.{n}": t for k, m in named.items() for n, t in m.state_dict().items() if t.dtype == torch.float32}
        for k, t in live.items():
            if not t.is_contiguous():
                raise ValueError(f"track_best(): {k} is not contiguous")
        self._tracked = list(named.values())
        self._live = live
        self._shadow = {k: t.detach().clone() for k, t in live.items()}
        self.metric = metric
        self.best.copy_(ops.eval_best_block(self.device))
        self._finish_call = ops.EvalFinishCall(self.state, self.loss, self.n, self.best, _METRICS[metric])

    def _caches(self) -> list:
        """Submodules that cache something derived from the weights in an attribute ``W_inverse`` outside any ``ops.pack_cache()``."""
        return [s for m in self._tracked for s in m.modules()]

    def best_weights(self):
        """Context manager: inside it the tracked modules hold the weights of the BEST pass — one in-place exchange with the shadow
        on entry, the same exchange on exit, after which every live bit is what it was.  The addresses do not change, so captured
        graphs stay valid.  Cached ``W_inverse`` attributes of the tracked modules are set aside on entry and put back on exit.
        Raises inside an open ``ops.pack_cache()`` scope (a packed image or a BatchNorm fold made before the exchange would be
        stale) and when nested; inside it ``run``, ``replay``, ``capture`` and ``track_best`` raise."""
        @contextlib.contextmanager
        def scope():
            if not self._shadow:
                raise RuntimeError("best_weights(): call track_best() first")
            if self._inside:
                raise RuntimeError("best_weights(): already inside; the context does not nest")
            if ops._PACK_CACHE is not None:
                raise RuntimeError("best_weights(): inside an ops.pack_cache() scope, whose packed weights and BatchNorm folds would "
                                   "be stale after the exchange; enter it outside")
            names = list(self._shadow)
            shadow, live = [self._shadow[k] for k in names], [self._live[k] for k in names]
            swap_tensors(shadow, live)                                        # (refuses before it exchanges anything)
            caches = self._caches()
            aside = [c.__dict__.pop("W_inverse", None) for c in caches]
            self._inside = True
            try:
                yield self
            finally:
                try:
                    swap_tensors(shadow, live)
                finally:
                    self._inside = False
                    for c, w in zip(caches, aside):
                        c.__dict__.pop("W_inverse", None)
                        if w is not None:
                            c.W_inverse = w
        return scope()

    def state_dict(self) -> dict:
        """The best words and the shadows (CPU copies; waits for the device)."""
        self._no_pass("state_dict()")
        return {"metric": self.metric, "best": self.best.cpu().clone(),
                "shadow": {k: t.detach().cpu().clone() for k, t in self._shadow.items()}}

    def load_state_dict(self, sd: dict) -> None:
        """In place: the addresses that captured graphs and the save hold stay valid.  ``track_best`` must have been called with
        the same modules (and is called for the metric, if it differs)."""
        self._no_pass("load_state_dict()")
        if set(sd["shadow"]) != set(self._shadow):
            raise KeyError("Evaluator: the checkpoint's shadow tensors are not those of the tracked modules; call track_best() first")
        if sd["metric"] != self.metric:
            self.metric = sd["metric"]
            self._finish_call = ops.EvalFinishCall(self.state, self.loss, self.n, self.best, _METRICS[self.metric])
        with torch.no_grad():
            self.best.copy_(sd["best"].to(torch.int32))
            for k, t in self._shadow.items():
                t.copy_(sd["shadow"][k])
