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

``VotingEvaluator`` (``make_voter``) is the multi-source vote of multi_source_voting.py:265-429 in the same manner: a weighing pass
over the train set (K forwards and K ``eval_fold`` calls per batch, then ``ops.vote_weights``) and a vote pass over the test set
(K forwards and one ``ops.vote_fold`` per batch, csrc/vote.hip), eager or as captured graphs.
"""
from __future__ import annotations

import contextlib
from typing import Dict, Optional, Sequence, Union

import torch
import torch.nn as nn

from . import _capture, ops
from .data import DeviceDataset, EvalPlan
from .optim import exchanged, guard_copy

__all__ = ["Evaluator", "VotingEvaluator", "make_voter"]

_METRICS = {"accuracy": 0, "loss": 1}
# report() / result(): the name of every counter of a pass's state block and of a plan's feed block -> its word
_STATE_WORDS = {"seen": ops.EVAL_SEEN, "hits": ops.EVAL_HITS, "batches": ops.EVAL_BATCHES, "bad_label": ops.EVAL_BAD_LABEL,
                "nonfinite": ops.EVAL_NONFINITE, "overflow": ops.EVAL_OVERFLOW}
_FEED_WORDS = {"overrun": ops.FEED_OVERRUN, "bad_index": ops.FEED_BAD_INDEX}


def _named(words, table: Dict[str, int]) -> dict:
    """The entries of ``table`` out of a block of words: a tensor (0-d views) or the list read from one (Python numbers)."""
    return {k: words[i] for k, i in table.items()}


def _read_once(tensors: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
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


class _Improved:
    """``guard_copy``'s predicate word of the best-weights save: the ``improved`` word of ``fst_eval_finish`` in the place of a verdict."""

    def __init__(self, best: torch.Tensor):
        self.verdict = best[ops.EVAL_IMPROVED: ops.EVAL_IMPROVED + 1]


def _n_class(who: str, n_class: Optional[int], clf: nn.Module, whose: str) -> int:
    """The number of classes: given, or the width of ``clf.hidden``."""
    if n_class is None:
        hidden = getattr(clf, "hidden", None)
        if not isinstance(hidden, nn.Linear):
            raise ValueError(f"{who}: n_class is needed ({whose} classifier has no Linear `hidden` to read it from)")
        n_class = hidden.out_features
    if isinstance(n_class, bool) or not isinstance(n_class, int) or not 1 <= n_class <= ops.EVAL_MAX_C:
        raise ValueError(f"{who}: n_class must be in 1..{ops.EVAL_MAX_C}, got {n_class!r}")
    return n_class


def _logits(fe, trans, clf, x: torch.Tensor, batch: int, n_class: int, who: str) -> torch.Tensor:
    """``clf(trans(fe(x)))``, or its first entry: fp32 ``[batch, n_class]``; ``who`` names the classifier in the message."""
    f = fe(x)
    if trans is not None:
        f = trans(f)
    out = clf(f)
    logits = out[0] if isinstance(out, (tuple, list)) else out
    if logits.dim() != 2 or logits.shape != (batch, n_class) or logits.dtype != torch.float32:
        raise ValueError(f"{who} classifier returned {tuple(logits.shape)} {logits.dtype}; fp32 [{batch}, {n_class}] expected")
    return logits


def _replay_pass(prepare, batch, rounds: int) -> None:
    """A captured pass: *prepare* once (round 0 with it), *batch* ``rounds - 1`` times."""
    prepare.replay()
    for _ in range(rounds - 1):
        batch.replay()


class _Passes:
    """What ``Evaluator`` and ``VotingEvaluator`` share: the static inputs of a batch, the modules' eval mode, and the capture of
    a pass — (begin, round) — as a (prepare, batch) pair of hipGraphs.  An owner supplies ``_modules()``, ``device`` and ``batch``."""
    _graphs = None                                                            # (prepare, batch) of every captured pass, in a row
    _caches = None                                                            # the capture-time pack caches, kept alive here
    _held = None                                                              # what the captured rounds returned: logits and calls, likewise

    def _static_inputs(self, data: DeviceDataset, *blocks: torch.Tensor) -> None:
        """The static inputs of every batch, eager or captured; ``blocks``: the words of the passes, which the kernels take
        in 16-byte pieces."""
        dev, B = data.device, self.batch
        self._x = torch.zeros((B,) + tuple(data.x.shape[1:]), dtype=torch.float32, device=dev)
        self._y = torch.zeros(B, dtype=torch.int64, device=dev)
        self._valid = torch.zeros(1, dtype=torch.int32, device=dev)
        if any(b.data_ptr() % 16 for b in blocks):
            raise RuntimeError(f"{type(self).__name__}: the allocator returned a block off a 16-byte boundary")

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

    def _capture_passes(self, passes, warmup: int) -> None:
        """Capture every (begin, round) of ``passes`` as two hipGraphs, all in one pool.  *prepare*: ``begin`` — rewind the plan,
        zero the pass's words — and round 0, whose forwards do what the first forward of a pass does once: the BatchNorm folds
        and the weight packing.  *batch*: every later round, served by the folds and images of *prepare*.  Each pass is captured
        under a pack cache of its own, whose objects are kept alive here, so a replay of *prepare* recomputes them in place from
        the live parameter storage; the global ``ops.pack_cache()`` scope is left before this returns."""
        who = type(self).__name__
        if self.device.type != "cuda":
            raise RuntimeError(f"{who}.capture(): a GPU is needed")
        if ops._PACK_CACHE is not None:
            raise RuntimeError(f"{who}.capture(): inside an ops.pack_cache() scope; capture outside it")
        with self._eval_mode():
            with _capture.warmup_stream(self.device):
                for begin, one_round in passes:
                    for _ in range(max(1, warmup)):
                        with ops.pack_cache():
                            begin()
                            one_round()
                    begin()
            graphs, caches, held, pool = [], [], [], None
            for begin, one_round in passes:
                prepare, batch = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                with ops.pack_cache():
                    caches.append(ops._PACK_CACHE)
                    with _capture.graph(prepare, pool):
                        begin()
                        held.append(one_round())
                    pool = prepare.pool()
                    with _capture.graph(batch, pool):
                        held.append(one_round())
                graphs += [prepare, batch]
        self._graphs, self._caches, self._held = tuple(graphs), caches, held

    def release(self) -> None:
        """Drop the captured graphs and what they kept alive."""
        self._graphs = self._caches = self._held = None


class Evaluator(_Passes):
    """Evaluate ``classification_module(feature_trans(feature_extraction_module(x)))`` over ``data`` in batches of ``batch_size``.

    ``n_class``: the number of classes (default: ``classification_module.hidden.out_features``).  ``feature_trans``: the source
    side's DimensionUnification.  ``keep_logits``: also keep every row's logits, ``[N, C]``, on the device.  The classifier may
    return the logits or a tuple whose first entry they are.  ``accuracy`` and the mean ``loss`` divide by ``len(data)``."""

    def __init__(self, feature_extraction_module: nn.Module, classification_module: nn.Module, data: DeviceDataset, batch_size: int,
                 n_class: Optional[int] = None, feature_trans: Optional[nn.Module] = None, keep_logits: bool = False):
        n_class = _n_class("Evaluator", n_class, classification_module, "the")
        self.fe, self.clf, self.feature_trans = feature_extraction_module, classification_module, feature_trans
        self.data, self.device, self.n_class, self.keep_logits = data, data.device, n_class, bool(keep_logits)
        self.plan = EvalPlan(data, batch_size)
        self.batch, self.rounds, self.n = batch_size, self.plan.rounds, len(data)
        dev, B, C, N = self.device, batch_size, n_class, self.n
        # the words of a pass as ONE block, zeroed by one fill: state (8 int32), loss (fp64), confusion (C x C int32)
        self._pass = torch.zeros(10 + C * C, dtype=torch.int32, device=dev)
        self._static_inputs(data, self._pass)
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

    # ------------------------------------------------------------------ the pass
    def _modules(self):
        return [m for m in (self.fe, self.feature_trans, self.clf) if m is not None]

    def _fold_call(self, logits: torch.Tensor) -> ops.EvalFoldCall:
        return ops.EvalFoldCall(logits, self._y, self._valid, self.state, self.loss, self.confusion, self.predictions, self.logits,
                                capacity=self.n, scratch=self._scratch)

    def _begin(self) -> None:
        self.plan.rewind()
        self._pass.zero_()

    def _round(self):
        """Feed, forward, ``eval_fold``; returns what a graph that captured the round must keep alive: the logits and the call."""
        self.plan.feed(self._x, self._y, self._valid)
        logits = _logits(self.fe, self.feature_trans, self.clf, self._x, self.batch, self.n_class, "Evaluator: the")
        call = self._fold_call(logits)
        call()
        return logits, call

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
        """Capture the pass as two hipGraphs sharing a pool (``_capture_passes``): *prepare* — rewind the plan, zero the pass's
        words and run round 0 — and *batch*, every later round.  Every replay of *prepare* recomputes the BatchNorm folds and the
        packed weights from the live parameter storage, so a replay evaluates the weights as they are then.  (A *prepare* that
        only folded and packed would need a forward whose logits nobody reads: one batch's time per pass.)"""
        self._no_pass("capture()")
        self._capture_passes([(self._begin, self._round)], warmup)

    def replay(self, report: bool = True) -> Optional[Dict[str, torch.Tensor]]:
        """One captured pass: *prepare* once (round 0 with it), *batch* ``rounds - 1`` times, then ``eval_finish`` (and the best-weights save, if
        tracked): launches only — no host tensor, no host-to-device copy, no wait.  Returns ``report()`` (device-side copies of the
        words), or nothing with ``report=False``."""
        self._no_pass("replay()")
        if self._graphs is None:
            raise RuntimeError("call capture() first")
        _replay_pass(*self._graphs, self.rounds)
        self._finish()
        return self.report() if report else None

    # ------------------------------------------------------------------ what a pass leaves
    def report(self) -> Dict[str, torch.Tensor]:
        """The last pass as fresh DEVICE tensors (copies within device memory; no host read): ``seen``, ``hits``, ``accuracy``
        (fp64), ``loss`` (the mean, fp64), ``confusion`` [C, C], ``predictions`` [N], ``labels`` (the resident ``data.y``
        itself), ``logits`` [N, C] with ``keep_logits``; ``improved``, ``best_accuracy`` (NaN before a first best), ``best_loss``,
        ``best_pass``, ``passes``; the counters ``batches``, ``bad_label``, ``nonfinite``, ``overflow``, ``incomplete``."""
        st, best = self.state.clone(), self.best.clone()
        hits, best_hits = st[ops.EVAL_HITS], best[ops.EVAL_BEST_HITS]
        out = {**_named(st, _STATE_WORDS), "accuracy": hits.to(torch.float64) / self.n,
               "loss": self.loss[0] / self.n, "confusion": self.confusion.clone(), "predictions": self.predictions.clone(),
               "labels": self.data.y, "improved": best[ops.EVAL_IMPROVED],
               "best_accuracy": torch.where(best_hits >= 0, best_hits.to(torch.float64) / self.n, float("nan")),
               "best_loss": ops.eval_best_loss(best)[0] / self.n, "best_pass": best[ops.EVAL_BEST_PASS], "passes": best[ops.EVAL_PASSES],
               "incomplete": best[ops.EVAL_INCOMPLETE]}
        if self.logits is not None:
            out["logits"] = self.logits.clone()
        return out

    def _read(self, tensors: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        return _read_once(tensors)

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
        out = {**_named(st, _STATE_WORDS), "accuracy": st[ops.EVAL_HITS] / self.n,
               "loss": float(h["loss"][0]) / self.n, "confusion": h["confusion"].clone(), "predictions": h["predictions"].clone(),
               "improved": bool(best[ops.EVAL_IMPROVED]),
               "best_accuracy": best[ops.EVAL_BEST_HITS] / self.n if best[ops.EVAL_BEST_HITS] >= 0 else float("nan"),
               "best_loss": best_loss / self.n, "best_pass": best[ops.EVAL_BEST_PASS], "passes": best[ops.EVAL_PASSES],
               "incomplete": best[ops.EVAL_INCOMPLETE], "feed": _named(h["feed"].tolist(), _FEED_WORDS)}
        if self.logits is not None:
            out["logits"] = h["logits"].clone()
        return out

    def check(self) -> None:
        """One host read; raises if the last pass overflowed its capacity or met a label outside ``0..C-1``, if any pass so far
        was incomplete, or if the plan was fed past its end or held an index outside the data set."""
        h = self._read({"state": self.state, "best": self.best, "feed": self.plan.state})
        st, best, feed = h["state"].tolist(), h["best"].tolist(), h["feed"].tolist()
        found = {"overflow": st[ops.EVAL_OVERFLOW], "bad_label": st[ops.EVAL_BAD_LABEL], "incomplete": best[ops.EVAL_INCOMPLETE],
                 **_named(feed, _FEED_WORDS)}
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

    @contextlib.contextmanager
    def best_weights(self):
        """Context manager: inside it the tracked modules hold the weights of the BEST pass — one in-place exchange with the shadow
        on entry, the same exchange on exit, after which every live bit is what it was.  The addresses do not change, so captured
        graphs stay valid.  Cached ``W_inverse`` attributes of the tracked modules are set aside on entry and put back on exit.
        Raises inside an open ``ops.pack_cache()`` scope (a packed image or a BatchNorm fold made before the exchange would be
        stale) and when nested; inside it ``run``, ``replay``, ``capture`` and ``track_best`` raise."""
        if not self._shadow:
            raise RuntimeError("best_weights(): call track_best() first")
        names = list(self._shadow)
        # the submodules may cache something derived from the weights in an attribute ``W_inverse`` outside any ``ops.pack_cache()``
        caches = [s for m in self._tracked for s in m.modules()]
        with exchanged([self._shadow[k] for k in names], [self._live[k] for k in names], caches, self, "_inside", "best_weights()"):
            yield self

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


class VotingEvaluator(_Passes):
    """The multi-source vote of multi_source_voting.py:265-429 as passes that stay on the device.  ``members``: K (1..16) target-side
    pipelines, each ``(fe, clf)`` or ``(fe, clf, feature_trans)``; ``train_data`` and ``test_data``: resident ``DeviceDataset``s of
    one series shape.  A *weighing* pass over ``train_data`` folds every member's predictions into its own confusion matrix
    (K unchanged ``ops.eval_fold`` calls per batch, the batch fed once) and ends in ``ops.vote_weights``: per-class precision
    weights relative to the mean over the members, and ``scale = base ** weights``.  A *vote* pass over ``test_data`` runs the K
    forwards on each batch and folds them with one ``ops.vote_fold`` (csrc/vote.hip): every member's softmax sharpened by its
    confidence, ``p (1 + sharpen exp(-H(p)))``, scaled per class, summed and argmax-ed, in fp64.  ``base=1, sharpen=2`` is the
    entropy-only vote.  ``keep_scores``: also keep every row's summed scores, fp64 ``[N, C]``.

    ``run()`` is eager; ``capture()`` / ``replay()`` run the same passes as hipGraphs (a prepare and a batch graph per pass, as
    ``Evaluator.capture``) with no host tensor, no copy and no wait.  Every batch runs at the static shape ``[B, ...]``."""

    def __init__(self, members, train_data: DeviceDataset, test_data: DeviceDataset, batch_size: int, n_class: Optional[int] = None,
                 sharpen: float = 120.0, base: float = 9.0, keep_scores: bool = False):
        members = [tuple(m) for m in members]
        if not 1 <= len(members) <= ops.VOTE_MAX_K:
            raise ValueError(f"VotingEvaluator: {len(members)} members; 1..{ops.VOTE_MAX_K}")
        if any(len(m) not in (2, 3) for m in members):
            raise ValueError("VotingEvaluator: a member is (fe, clf) or (fe, clf, feature_trans)")
        self.members = [(m[0], m[1], m[2] if len(m) == 3 else None) for m in members]
        n_class = _n_class("VotingEvaluator", n_class, self.members[0][1], "member 0's")
        for k, (_, clf, _) in enumerate(self.members):
            w = clf.hidden.out_features if isinstance(getattr(clf, "hidden", None), nn.Linear) else n_class
            if w != n_class:
                raise ValueError(f"VotingEvaluator: member {k}'s classifier has {w} classes, n_class is {n_class}")
        if train_data.device != test_data.device or train_data.x.shape[1:] != test_data.x.shape[1:]:
            raise ValueError(f"VotingEvaluator: the two data sets must live on one device and hold one series shape, got "
                             f"{tuple(train_data.x.shape[1:])} on {train_data.device} and {tuple(test_data.x.shape[1:])} on {test_data.device}")
        self.sharpen, self.base = ops._vote_f32(sharpen), ops._vote_f32(base)           # as the library receives them
        if not (self.base > 0.0 and self.base < float("inf")) or not (0.0 <= self.sharpen < float("inf")):
            raise ValueError(f"VotingEvaluator: base must be positive and finite and sharpen finite and not negative, got {base!r}, {sharpen!r}")
        self.train_data, self.test_data, self.device = train_data, test_data, test_data.device
        self.n_class, self.keep_scores, self.batch = n_class, bool(keep_scores), batch_size
        self.train_plan, self.test_plan = EvalPlan(train_data, batch_size), EvalPlan(test_data, batch_size)
        self.n_train, self.n = len(train_data), len(test_data)
        dev, B, C, K = self.device, batch_size, n_class, len(self.members)
        self.K = K
        # the words of a vote pass as ONE block, zeroed by one fill: state (8 int32), member_hits (16), confusion (C x C)
        self._pass = torch.zeros(24 + C * C, dtype=torch.int32, device=dev)
        # ... and of a weighing pass: per member state (8), loss (fp64), confusion (C x C), each on a 16-byte boundary
        stride = (10 + C * C + 3) // 4 * 4
        self._weigh_pass = torch.zeros(K * stride, dtype=torch.int32, device=dev)
        self._static_inputs(test_data, self._pass, self._weigh_pass)          # of every batch of either pass
        self.state, self.member_hits, self.confusion = self._pass[:8], self._pass[8: 8 + K], self._pass[24:].view(C, C)
        blocks = [self._weigh_pass[k * stride: k * stride + 10 + C * C] for k in range(K)]
        self._member_state = [b[:8] for b in blocks]
        self._member_loss = [b[8:10].view(torch.float64) for b in blocks]
        self.member_confusion = [b[10:].view(C, C) for b in blocks]
        self.weights = torch.zeros(K, C, dtype=torch.float64, device=dev)
        self.scale = torch.ones(K, C, dtype=torch.float64, device=dev)
        self.predictions = torch.zeros(self.n, dtype=torch.int64, device=dev)
        self.scores = torch.zeros(self.n, C, dtype=torch.float64, device=dev) if keep_scores else None
        on_gpu = dev.type == "cuda"
        self._scratch = ops.eval_scratch(B, dev) if on_gpu else None
        self._vote_scratch = ops.vote_scratch(B, dev) if on_gpu else None
        self._weights_call = ops.VoteWeightsCall(self.member_confusion, self.weights, self.scale, self.base)
        self._weighted = False                                                # weights are in place: weigh() or set_weights()
        self._weighed_here = False                                            # ... by a weighing pass of this object

    # ------------------------------------------------------------------ the passes
    def _modules(self):
        seen, out = set(), []
        for member in self.members:
            for m in member:
                if m is not None and id(m) not in seen:
                    seen.add(id(m))
                    out.append(m)
        return out

    def _forward(self, k: int) -> torch.Tensor:
        fe, clf, trans = self.members[k]
        return _logits(fe, trans, clf, self._x, self.batch, self.n_class, f"VotingEvaluator: member {k}'s")

    def _weigh_begin(self) -> None:
        self.train_plan.rewind()
        self._weigh_pass.zero_()

    def _weigh_round(self):
        """Feed once, K forwards, K ``eval_fold`` calls; returns what a graph that captured the round must keep alive."""
        self.train_plan.feed(self._x, self._y, self._valid)
        held = []
        for k in range(self.K):
            logits = self._forward(k)
            call = ops.EvalFoldCall(logits, self._y, self._valid, self._member_state[k], self._member_loss[k], self.member_confusion[k],
                                    capacity=self.n_train, scratch=self._scratch)
            call()
            held.append((logits, call))
        return held

    def _vote_begin(self) -> None:
        self.test_plan.rewind()
        self._pass.zero_()

    def _vote_round(self):
        """Feed once, K forwards, one ``vote_fold``."""
        self.test_plan.feed(self._x, self._y, self._valid)
        logits = [self._forward(k) for k in range(self.K)]
        call = ops.VoteFoldCall(logits, self.scale, self._y, self._valid, self.state, self.member_hits, self.confusion, self.predictions,
                                self.scores, sharpen=self.sharpen, capacity=self.n, scratch=self._vote_scratch)
        call()
        return logits, call

    def _need_weights(self, what: str) -> None:
        if not self._weighted:
            raise RuntimeError(f"{what}: no weights yet; call weigh() or set_weights() first, or pass weigh=True")

    def weigh(self) -> torch.Tensor:
        """One eager weighing pass over ``train_data`` and ``ops.vote_weights``; returns ``weights`` (the resident tensor)."""
        with self._eval_mode(), ops.pack_cache():
            self._weigh_begin()
            for _ in range(self.train_plan.rounds):
                self._weigh_round()
        self._weights_call()
        self._weighted = self._weighed_here = True
        return self.weights

    @torch.no_grad()
    def set_weights(self, w) -> None:
        """Weights computed elsewhere, ``[K, C]``, in the place of a weighing pass: written into ``weights`` and, as ``base ** w``,
        into ``scale``, in place."""
        w = torch.as_tensor(w, dtype=torch.float64)
        if w.shape != self.weights.shape:
            raise ValueError(f"set_weights(): [{self.K}, {self.n_class}] expected, got {tuple(w.shape)}")
        self.weights.copy_(w)
        torch.pow(torch.tensor(self.base, dtype=torch.float64, device=self.device), self.weights, out=self.scale)
        self._weighted = True

    def run(self, weigh: bool = False) -> Dict[str, torch.Tensor]:
        """One eager vote pass over ``test_data`` (after a weighing pass with ``weigh=True``): the modules in eval mode (their modes
        restored afterwards), under ``torch.no_grad()`` and one ``ops.pack_cache()``.  Returns ``report()``: no host read."""
        if weigh:
            self.weigh()
        self._need_weights("run()")
        with self._eval_mode(), ops.pack_cache():
            self._vote_begin()
            for _ in range(self.test_plan.rounds):
                self._vote_round()
        return self.report()

    def capture(self, warmup: int = 1) -> None:
        """Capture both passes as hipGraphs sharing one pool, each as ``Evaluator.capture`` does: a *prepare* graph (rewind, zero the
        pass's words, round 0, whose forwards fold the BatchNorms and pack the weights) and a *batch* graph for every later round.
        Each pass is captured under a pack cache of its own, so either prepare graph recomputes the folds and images it is served
        by from the live parameter storage: replaying the vote pass alone evaluates the weights as they are then."""
        self._capture_passes([(self._weigh_begin, self._weigh_round), (self._vote_begin, self._vote_round)], warmup)

    def replay(self, weigh: bool = False, report: bool = True) -> Optional[Dict[str, torch.Tensor]]:
        """The captured vote pass (after the captured weighing pass and ``vote_weights`` with ``weigh=True``): launches only — no
        host tensor, no host-to-device copy, no wait.  Returns ``report()``, or nothing with ``report=False``."""
        if self._graphs is None:
            raise RuntimeError("call capture() first")
        if weigh:
            _replay_pass(*self._graphs[:2], self.train_plan.rounds)
            self._weights_call()
            self._weighted = self._weighed_here = True
        self._need_weights("replay()")
        _replay_pass(*self._graphs[2:], self.test_plan.rounds)
        return self.report() if report else None

    # ------------------------------------------------------------------ what a pass leaves
    def report(self) -> Dict[str, torch.Tensor]:
        """The last vote pass as fresh DEVICE tensors (copies within device memory; no host read): ``seen``, ``hits``, ``accuracy``
        (fp64), ``confusion`` [C, C], ``predictions`` [N], ``labels`` (the resident ``test_data.y`` itself), ``member_hits`` [K],
        ``member_accuracy`` (fp64 [K]), ``weights`` and ``scale`` (fp64 [K, C]), ``scores`` (fp64 [N, C]) with ``keep_scores``; the
        counters ``batches``, ``bad_label``, ``nonfinite``, ``overflow``."""
        st, member_hits = self.state.clone(), self.member_hits.clone()
        hits = st[ops.EVAL_HITS]
        out = {**_named(st, _STATE_WORDS), "accuracy": hits.to(torch.float64) / self.n, "confusion": self.confusion.clone(),
               "predictions": self.predictions.clone(), "labels": self.test_data.y, "member_hits": member_hits,
               "member_accuracy": member_hits.to(torch.float64) / self.n, "weights": self.weights.clone(), "scale": self.scale.clone()}
        if self.scores is not None:
            out["scores"] = self.scores.clone()
        return out

    def result(self) -> dict:
        """The last vote pass with ONE host read (this waits for the device): Python numbers for the words, CPU tensors for
        ``confusion``, ``predictions``, ``member_hits``, ``member_accuracy``, ``weights``, ``scale`` and, with ``keep_scores``,
        ``scores``; ``feed`` holds the test plan's counters."""
        parts = {"pass": self._pass, "feed": self.test_plan.state, "predictions": self.predictions, "weights": self.weights,
                 "scale": self.scale}
        if self.scores is not None:
            parts["scores"] = self.scores
        h = _read_once(parts)
        C, K = self.n_class, self.K
        st, member_hits = h["pass"][:8].tolist(), h["pass"][8: 8 + K].clone()
        out = {**_named(st, _STATE_WORDS), "accuracy": st[ops.EVAL_HITS] / self.n,
               "confusion": h["pass"][24:].view(C, C).clone(), "predictions": h["predictions"].clone(), "member_hits": member_hits,
               "member_accuracy": member_hits.to(torch.float64) / self.n, "weights": h["weights"].clone(), "scale": h["scale"].clone(),
               "feed": _named(h["feed"].tolist(), _FEED_WORDS)}
        if self.scores is not None:
            out["scores"] = h["scores"].clone()
        return out

    def check(self) -> None:
        """One host read; raises if the last vote pass (or, where this object weighed, the last weighing pass) overflowed its
        capacity, met a label outside ``0..C-1`` or did not see every row, or if a plan was fed past its end or held an index
        outside its data set."""
        parts = {"state": self.state, "feed": self.test_plan.state, "train_feed": self.train_plan.state}
        parts.update({f"member {k}": s for k, s in enumerate(self._member_state)})
        h = {k: v.tolist() for k, v in _read_once(parts).items()}
        found = {}
        blocks = [("", h["state"], self.n)]
        if self._weighed_here:
            blocks += [(f"member {k} ", h[f"member {k}"], self.n_train) for k in range(self.K)]
        for who, st, rows in blocks:
            found[who + "overflow"], found[who + "bad_label"] = st[ops.EVAL_OVERFLOW], st[ops.EVAL_BAD_LABEL]
            found[who + "rows missing"] = rows - st[ops.EVAL_SEEN]
        for who, feed in (("", h["feed"]), ("train ", h["train_feed"])):
            found[who + "overrun"], found[who + "bad_index"] = feed[ops.FEED_OVERRUN], feed[ops.FEED_BAD_INDEX]
        if any(found.values()):
            raise RuntimeError("VotingEvaluator: " + ", ".join(f"{k} = {v}" for k, v in found.items() if v))


def make_voter(trainers, train_data: DeviceDataset, test_data: DeviceDataset, batch_size: int, **kw) -> VotingEvaluator:
    """A ``VotingEvaluator`` over K trained pipelines: each entry a ``JointTrainer`` (its target side, ``fe_t`` and ``clf_t``), a
    ``ClassifierTrainer`` (``fe`` and ``clf``) or a ``(fe, clf[, feature_trans])`` tuple; ``kw`` are ``VotingEvaluator``'s other
    arguments."""
    members = []
    for k, t in enumerate(trainers):
        if isinstance(t, (tuple, list)):
            members.append(tuple(t))
        elif isinstance(getattr(t, "m", None), dict) and "fe_t" in t.m and "clf_t" in t.m:
            members.append((t.m["fe_t"], t.m["clf_t"]))
        elif hasattr(t, "fe") and hasattr(t, "clf"):
            members.append((t.fe, t.clf))
        else:
            raise ValueError(f"make_voter(): entry {k} is neither a trainer nor a (fe, clf) tuple: {type(t).__name__}")
    return VotingEvaluator(members, train_data, test_data, batch_size, **kw)
