"""Evaluation on the device, the parts that need no GPU: the ABI and the exports, the CPU branch of ``ops.eval_fold`` (the
executable specification the GPU tests compare the kernel with) against an independent computation written here, ``eval_finish``,
``EvalPlan``, ``Evaluator.run()`` on stub modules, and the voting weights from confusion matrices.

The independent computation: the prediction row by row with explicit NaN handling, each row's loss in numpy fp64 and their sum by
``math.fsum``, the confusion matrix by counting.  Loss gate: both sides are fp64 with at most C + a few roundings per row, so
``|a - b| <= 1e-11 * rows * max(1, max|finite logit|)`` is three orders above the expected error and far below fp32's."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import _lib, ops, voting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
SHAPES = [(1, 1), (5, 3), (8, 64), (7, 65), (3, 130)]
# rows of four logits and the prediction torch.argmax gives on the CPU, stated literally
SPECIAL = [([1.0, NAN, 3.0, NAN], 1), ([0.0, -0.0, 0.0, -1.0], 0), ([INF, INF, 1.0, 2.0], 0), ([-INF] * 4, 0), ([2.0, INF, NAN, 1.0], 2)]


# ---------------------------------------------------------------------------------------------- shared with tests/test_gpu_evaluate.py
def make_calls(B, C, valids, seed=0, ld=None):
    """One (logits [B, C] — a view of [B, ld] if given —, labels, valid) per entry of ``valids``; random finite rows, a tie in row 0."""
    gen = torch.Generator().manual_seed(seed * 7919 + B * 131 + C)
    calls = []
    for v in valids:
        wide = torch.randn(B, ld or C, generator=gen) * 3
        x = wide[:, :C]
        if C > 1:
            x[0, C - 1] = x[0, 0] = x[0].max() + 1                            # the maximum twice: the lower index wins
        calls.append((x, torch.randint(C, (B,), generator=gen), v))
    return calls


def special_calls():
    x = torch.tensor([row for row, _ in SPECIAL] + [[0.5, 0.25, -1.0, 4.0]])
    y = torch.tensor([1, 0, 3, 2, 2, 3])
    return [(x, y, 6)]


def fold_ref(calls, C, capacity):
    """The independent computation.  Returns (state words, loss, confusion, predictions, stored logits as int32 words)."""
    st = [0] * 8
    cm = np.zeros((C, C), dtype=np.int64)
    pred_out, rows_out, nlls, scale = [], [], [], 1.0
    for x, y, valid in calls:
        B = x.shape[0]
        valid = min(max(valid, 0), B)
        if st[ops.EVAL_SEEN] + valid > capacity:
            st[ops.EVAL_OVERFLOW] += 1
            continue
        xs, ys = x.numpy().astype(np.float32), y.numpy()
        for r in range(valid):
            row = xs[r]
            nan_at = [i for i, v in enumerate(row) if v != v]
            if nan_at:
                p = nan_at[0]
            else:
                p = 0
                for i, v in enumerate(row):
                    if v > row[p]:
                        p = i
            pred_out.append(p)
            rows_out.append(row.view(np.int32).copy())
            finite = row[np.isfinite(row)]
            if finite.size:
                scale = max(scale, float(np.abs(finite).max()))
            if not np.isfinite(row).all():
                st[ops.EVAL_NONFINITE] += 1
            label = int(ys[r])
            if not 0 <= label < C:
                st[ops.EVAL_BAD_LABEL] += 1
                continue
            with np.errstate(all="ignore"):
                d = row.astype(np.float64)
                m = np.float64(NAN) if nan_at else d.max()
                z = d - m
                s = math.fsum(np.exp(z).tolist()) if np.isfinite(z).all() else float(np.exp(z).sum())
                nlls.append(float(-(z[label] - np.log(np.float64(s)))))
            cm[label, p] += 1
            st[ops.EVAL_HITS] += int(p == label)
        st[ops.EVAL_BATCHES] += 1
        st[ops.EVAL_SEEN] += valid
    loss = math.fsum(nlls) if all(math.isfinite(v) for v in nlls) else NAN
    return st, loss, cm, pred_out, rows_out, scale


def new_words(C, capacity):
    return (torch.zeros(8, dtype=torch.int32), torch.zeros(1, dtype=torch.float64), torch.zeros(C, C, dtype=torch.int32),
            torch.full((capacity,), -7, dtype=torch.int64), torch.full((capacity, C), -7.0))


def fold_cpu(calls, C, capacity):
    """The CPU branch.  Returns (state, loss, confusion, pred_out, logits_out) tensors."""
    st, loss, cm, pred, keep = new_words(C, capacity)
    for x, y, valid in calls:
        ops.eval_fold(x, y, torch.tensor([valid], dtype=torch.int32), st, loss, cm, pred, keep)
    return st, loss, cm, pred, keep


def loss_close(a, b, rows, scale):
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return abs(a - b) <= 1e-11 * max(rows, 1) * max(1.0, scale)


def check_cpu_against_ref(calls, C, capacity):
    st, loss, cm, pred, keep = fold_cpu(calls, C, capacity)
    r_st, r_loss, r_cm, r_pred, r_rows, scale = fold_ref(calls, C, capacity)
    n = r_st[ops.EVAL_SEEN]
    assert st.tolist() == r_st
    assert torch.equal(cm.long(), torch.from_numpy(r_cm))
    assert pred[:n].tolist() == r_pred and (pred[n:] == -7).all()
    if n:
        assert np.array_equal(keep[:n].contiguous().view(torch.int32).numpy(), np.stack(r_rows))
    assert (keep[n:] == -7.0).all()
    print(f"loss: cpu branch {float(loss):.17g}, independent {r_loss:.17g}")
    assert loss_close(float(loss), r_loss, n, scale), (float(loss), r_loss)
    return st, float(loss), cm, pred


# ---------------------------------------------------------------------------------------------- ABI and exports
def test_abi_and_exports():
    text = open(os.path.join(ROOT, "include", "fst_hip.h")).read()
    version = int(re.search(r"#define\s+FST_ABI_VERSION\s+(\d+)", text).group(1))
    assert version == _lib.ABI_VERSION >= 26
    for name in ("fst_eval_fold", "fst_eval_finish"):
        assert name in _lib.EXPORTED_SYMBOLS and re.search(r"\bint\s+%s\s*\(" % name, text)
    for name in ("Evaluator", "EvalPlan", "eval_fold", "eval_finish", "precision_weights_from_confusion"):
        assert hasattr(fst, name), name
    assert (ops.EVAL_SEEN, ops.EVAL_HITS, ops.EVAL_BATCHES, ops.EVAL_BAD_LABEL, ops.EVAL_NONFINITE, ops.EVAL_OVERFLOW) == tuple(range(6))
    assert (ops.EVAL_IMPROVED, ops.EVAL_PASSES, ops.EVAL_BEST_HITS, ops.EVAL_BEST_PASS, ops.EVAL_BEST_LOSS, ops.EVAL_INCOMPLETE) == (0, 1, 2, 3, 4, 6)


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libfst_hip.so not built (run __graft_entry__.build())")
def test_library_refuses_null_arguments():
    lib = _lib.load()
    assert lib.fst_version() >= 26
    assert lib.fst_eval_fold(None, 0, None, 0, 0, None, None, None, None, None, None, 0, None, None) == -1 and lib.fst_last_error()
    assert lib.fst_eval_finish(None, None, 0, None, 0, None) == -1 and lib.fst_last_error()


# ---------------------------------------------------------------------------------------------- eval_fold, the CPU branch
@pytest.mark.parametrize("B,C", SHAPES)
def test_fold_equals_independent_computation(B, C):
    for valid in sorted({0, 1, B - 1, B}):
        st, _, cm, _ = check_cpu_against_ref(make_calls(B, C, [valid]), C, capacity=B)
        assert st[ops.EVAL_SEEN] == valid and int(cm.sum()) == valid
    check_cpu_against_ref(make_calls(B, C, [B], ld=C + 3), C, capacity=B)     # rows strided: ld > C


@pytest.mark.parametrize("B,C", SHAPES)
def test_three_calls_accumulate(B, C):
    calls = make_calls(B, C, [B, B - 1, B], seed=1, ld=C + 1)
    st, _, cm, _ = check_cpu_against_ref(calls, C, capacity=3 * B)
    assert st[ops.EVAL_SEEN] == 3 * B - 1 == int(cm.sum()) and st[ops.EVAL_BATCHES] == 3


def test_special_rows():
    st, loss, cm, pred = check_cpu_against_ref(special_calls(), 4, capacity=6)
    assert pred.tolist() == [p for _, p in SPECIAL] + [3]
    assert st.tolist() == [6, 4, 1, 0, 4, 0, 0, 0] and math.isnan(loss)      # hits: rows 0, 1, 4 and 5; only rows 1 and 5 are finite
    # what F.cross_entropy gives on the same rows in fp64: NaN for every row holding a NaN or an inf, and the finite rows' value
    x, y, _ = special_calls()[0]
    ce = torch.nn.functional.cross_entropy(x.double(), y, reduction="none")
    assert torch.isnan(ce).tolist() == [True, False, True, True, True, False]
    finite = [(x[[1, 5]], y[[1, 5]], 2)]
    _, loss2, _, _ = check_cpu_against_ref(finite, 4, capacity=2)
    assert abs(loss2 - float(ce[[1, 5]].sum())) <= 1e-13


def test_bad_label_is_counted_and_kept_out():
    x, y, v = make_calls(5, 3, [5], seed=3)[0]
    y = y.clone(); y[1], y[3] = 3, -1
    st, loss, cm, pred = check_cpu_against_ref([(x, y, v)], 3, capacity=5)
    assert st[ops.EVAL_BAD_LABEL] == 2 and int(cm.sum()) == 3 and pred.tolist() == x.argmax(1).tolist()
    keep = torch.tensor([0, 2, 4])
    assert abs(loss - float(torch.nn.functional.cross_entropy(x[keep].double(), y[keep], reduction="sum"))) <= 1e-12


def test_capacity_overflow_writes_nothing_else():
    calls = make_calls(5, 3, [5, 5, 2], seed=4)
    st, loss, cm, pred = check_cpu_against_ref(calls, 3, capacity=8)          # 5, then 5 more do not fit, then 2 do
    assert st.tolist()[ops.EVAL_SEEN] == 7 and st[ops.EVAL_OVERFLOW] == 1 and st[ops.EVAL_BATCHES] == 2
    assert pred[5:7].tolist() == calls[2][0][:2].argmax(1).tolist() and pred[7] == -7
    with pytest.raises(ValueError):
        ops.eval_fold(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(8, dtype=torch.int32),
                      torch.zeros(1, dtype=torch.float64), torch.zeros(3, 3, dtype=torch.int32))      # no capacity given
    with pytest.raises(ValueError):
        ops.eval_fold(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(8, dtype=torch.int32),
                      torch.zeros(1, dtype=torch.float64), torch.zeros(2, 2, dtype=torch.int32), capacity=4)   # confusion of another C


# ---------------------------------------------------------------------------------------------- eval_finish
def finish(best, seen, hits, loss, expect, mode, overflow=0, bad=0):
    st = torch.zeros(8, dtype=torch.int32)
    st[ops.EVAL_SEEN], st[ops.EVAL_HITS], st[ops.EVAL_OVERFLOW], st[ops.EVAL_BAD_LABEL] = seen, hits, overflow, bad
    ops.eval_finish(st, torch.tensor([loss], dtype=torch.float64), expect, best, mode)
    return best.tolist()[:4] + [float(ops.eval_best_loss(best)[0])] + [int(best[ops.EVAL_INCOMPLETE])]


def test_finish_by_hits():
    best = ops.eval_best_block("cpu")
    assert best.tolist()[:4] == [0, 0, -1, 0] and float(ops.eval_best_loss(best)[0]) == INF
    assert finish(best, 10, 0, 5.0, 10, 0) == [1, 1, 0, 1, 5.0, 0]            # zero hits beat the initial -1
    assert finish(best, 10, 4, 7.0, 10, 0) == [1, 2, 4, 2, 7.0, 0]
    assert finish(best, 10, 4, 1.0, 10, 0) == [0, 3, 4, 2, 7.0, 0]            # a tie does not improve
    assert finish(best, 10, 3, 0.5, 10, 0) == [0, 4, 4, 2, 7.0, 0]
    assert finish(best, 10, 9, NAN, 10, 0)[:4] == [1, 5, 9, 5]                # by hits a NaN loss is no obstacle


def test_finish_by_loss():
    best = ops.eval_best_block("cpu")
    assert finish(best, 10, 2, 5.0, 10, 1) == [1, 1, 2, 1, 5.0, 0]
    assert finish(best, 10, 9, 5.0, 10, 1) == [0, 2, 2, 1, 5.0, 0]            # a tie does not improve
    assert finish(best, 10, 9, NAN, 10, 1) == [0, 3, 2, 1, 5.0, 0]            # a NaN loss never does
    assert finish(best, 10, 1, 4.5, 10, 1) == [1, 4, 1, 4, 4.5, 0]
    fresh = ops.eval_best_block("cpu")
    assert finish(fresh, 10, 1, NAN, 10, 1) == [0, 1, -1, 0, INF, 0]


def test_finish_incomplete_pass():
    best = ops.eval_best_block("cpu")
    assert finish(best, 9, 9, 0.1, 10, 0) == [0, 1, -1, 0, INF, 1]            # a row short
    assert finish(best, 10, 9, 0.1, 10, 0, overflow=1) == [0, 2, -1, 0, INF, 2]
    assert finish(best, 10, 9, 0.1, 10, 1, bad=2) == [0, 3, -1, 0, INF, 3]
    assert finish(best, 10, 1, 9.0, 10, 0) == [1, 4, 1, 4, 9.0, 3]
    with pytest.raises(ValueError):
        ops.eval_finish(torch.zeros(8, dtype=torch.int32), torch.zeros(1, dtype=torch.float64), 10, best, 2)


# ---------------------------------------------------------------------------------------------- EvalPlan
@pytest.mark.parametrize("N", [1, 8, 9, 26])
def test_eval_plan(N):
    B = 8
    gen = torch.Generator().manual_seed(N)
    data = fst.DeviceDataset(torch.randn(N, 2, 5, generator=gen), torch.randint(-2 ** 40, 2 ** 40, (N,), generator=gen), "cpu")
    plan = fst.EvalPlan(data, B)
    R = -(-N // B)
    assert plan.rounds == len(plan) == R
    assert plan.index.dtype == torch.int32 and plan.index.reshape(-1).tolist() == [min(i, N - 1) for i in range(R * B)]
    assert plan.valid.reshape(-1).tolist() == [min(B, N - r * B) for r in range(R)]
    x, y, valid = torch.zeros(B, 2, 5), torch.zeros(B, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    for sweep in range(2):
        xs, ys = [], []
        for r in range(R):
            plan.feed(x, y, valid)
            v = int(valid)
            assert v == min(B, N - r * B)
            assert torch.equal(x[v:], data.x[N - 1].expand(B - v, -1, -1)) and (y[v:] == data.y[N - 1]).all()      # the padding: the last row
            xs.append(x[:v].clone()); ys.append(y[:v].clone())
        assert torch.equal(torch.cat(xs), data.x) and torch.equal(torch.cat(ys), data.y)
        assert plan.counters().tolist()[:5] == [R, R, R * (sweep + 1), 0, 0]
        plan.check()
        plan.rewind()
        assert plan.counters().tolist()[:5] == [0, R, R * (sweep + 1), 0, 0]
    for _ in range(R + 1):
        plan.feed(x, y, valid)
    with pytest.raises(RuntimeError, match="past the end"):
        plan.check()
    with pytest.raises(ValueError):
        fst.EvalPlan(data, 0)


# ---------------------------------------------------------------------------------------------- Evaluator.run() on stub modules
class StubFE(nn.Module):
    """Features whose every row is computed from that row alone, in an order that does not depend on the batch size."""

    def __init__(self, gen):
        super().__init__()
        self.w = nn.Parameter(torch.randn(6, 10, generator=gen))
        self.register_buffer("shift", torch.randn(6, generator=gen))
        self.register_buffer("calls", torch.zeros((), dtype=torch.int64))     # an integer buffer: not shadowed

    def forward(self, x):
        return (x.flatten(1).unsqueeze(1) * self.w.unsqueeze(0)).sum(dim=2) + self.shift


class StubClf(nn.Module):
    def __init__(self, gen, C=3):
        super().__init__()
        self.hidden = nn.Linear(6, C)
        with torch.no_grad():
            self.hidden.weight.copy_(torch.randn(C, 6, generator=gen)); self.hidden.bias.copy_(torch.randn(C, generator=gen))

    def forward(self, f):
        return (f.unsqueeze(1) * self.hidden.weight.unsqueeze(0)).sum(dim=2) + self.hidden.bias, f


def stub_pipeline(N=26, seed=0):
    gen = torch.Generator().manual_seed(seed)
    data = fst.DeviceDataset(torch.randn(N, 2, 5, generator=gen), torch.randint(3, (N,), generator=gen), "cpu")
    return StubFE(gen), StubClf(gen), data


def whole_set(fe, clf, data):
    with torch.no_grad():
        logits = clf(fe(data.x))[0]
    pred = logits.argmax(1)
    cm = torch.zeros(3, 3, dtype=torch.int32)
    for t, p in zip(data.y.tolist(), pred.tolist()):
        cm[t, p] += 1
    loss = float(torch.nn.functional.cross_entropy(logits.double(), data.y, reduction="sum"))
    return logits, pred, cm, int((pred == data.y).sum()), loss


@pytest.mark.parametrize("N", [26, 24, 3])
def test_run_equals_the_whole_set_at_once(N):
    fe, clf, data = stub_pipeline(N)
    fe.train(); clf.eval()
    ev = fst.Evaluator(fe, clf, data, 8, keep_logits=True)
    rep = ev.run()
    assert fe.training and not clf.training                                   # modes restored
    logits, pred, cm, hits, loss = whole_set(fe, clf, data)
    assert torch.equal(rep["logits"], logits) and torch.equal(rep["predictions"], pred) and torch.equal(rep["confusion"], cm)
    assert int(rep["seen"]) == N and int(rep["hits"]) == hits and float(rep["accuracy"]) == hits / N
    assert rep["accuracy"].dtype == rep["loss"].dtype == torch.float64 and rep["labels"] is data.y
    assert abs(float(rep["loss"]) * N - loss) <= 1e-11 * N * max(1.0, float(logits.abs().max()))
    assert int(rep["batches"]) == -(-N // 8) and int(rep["improved"]) == 1 and int(rep["passes"]) == 1
    assert [int(rep[k]) for k in ("bad_label", "nonfinite", "overflow", "incomplete")] == [0, 0, 0, 0]
    res = ev.result()
    assert res["hits"] == hits and res["seen"] == N and torch.equal(res["predictions"], pred) and torch.equal(res["logits"], logits)
    assert res["loss"] == float(rep["loss"]) and res["feed"] == {"overrun": 0, "bad_index": 0} and res["improved"] is True
    ev.check()
    rep2 = ev.run()                                                           # a second pass starts from zeroed words
    assert int(rep2["seen"]) == N and int(rep2["passes"]) == 2 and int(rep2["improved"]) == 0 and torch.equal(rep2["confusion"], cm)
    assert "logits" not in fst.Evaluator(fe, clf, data, 8).run()
    with pytest.raises(ValueError, match="n_class"):
        fst.Evaluator(fe, fe, data, 8)


def test_check_raises_on_a_bad_label():
    fe, clf, data = stub_pipeline()
    data.y[5] = 3
    ev = fst.Evaluator(fe, clf, data, 8)
    rep = ev.run()
    assert int(rep["bad_label"]) == 1 and int(rep["improved"]) == 0 and int(rep["incomplete"]) == 1
    with pytest.raises(RuntimeError, match="bad_label = 1"):
        ev.check()


@pytest.mark.parametrize("metric", ["accuracy", "loss"])
def test_track_best_keeps_the_best_of_three_passes(metric):
    fe, clf, data = stub_pipeline(seed=2)
    ev = fst.Evaluator(fe, clf, data, 8)
    ev.track_best([fe, clf], metric=metric)
    assert set(ev._shadow) == {"0.w", "0.shift", "1.hidden.weight", "1.hidden.bias"}
    gen = torch.Generator().manual_seed(11)
    saved, scores, improved = [], [], []
    for epoch in range(3):
        with torch.no_grad():
            for p in list(fe.parameters()) + list(clf.parameters()) + [fe.shift]:
                p.add_(torch.randn(p.shape, generator=gen) * (0.0 if epoch == 0 else 1.0))
        saved.append({k: v.clone() for k, v in ev._live.items()})
        rep = ev.run()
        scores.append(int(rep["hits"]) if metric == "accuracy" else -float(rep["loss"]))
        improved.append(int(rep["improved"]))
    best = max(range(3), key=lambda i: (scores[i], -i))                       # the first among equals
    assert improved == [int(scores[i] > max(scores[:i], default=-INF)) for i in range(3)]
    assert all(torch.equal(ev._shadow[k], saved[best][k]) for k in saved[best])
    assert int(ev.report()["best_pass"]) == best + 1
    # best_weights(): an exchange, restored bit for bit
    live_before = {k: v.clone() for k, v in ev._live.items()}
    with ev.best_weights():
        assert all(torch.equal(ev._live[k], saved[best][k]) for k in saved[best])
        assert all(torch.equal(ev._shadow[k], live_before[k]) for k in live_before)
        for call in (ev.run, ev.track_best, ev.state_dict):
            with pytest.raises(RuntimeError, match="best_weights"):
                call()
        with pytest.raises(RuntimeError, match="nest"):
            with ev.best_weights():
                pass
    assert all(torch.equal(ev._live[k].view(torch.int32), live_before[k].view(torch.int32)) for k in live_before)
    assert all(torch.equal(ev._shadow[k], saved[best][k]) for k in saved[best])
    with ops.pack_cache():
        with pytest.raises(RuntimeError, match="pack_cache"):
            with ev.best_weights():
                pass
    # the state_dict round trip: into an evaluator of a fresh pipeline
    sd = ev.state_dict()
    fe2, clf2, _ = stub_pipeline(seed=5)
    ev2 = fst.Evaluator(fe2, clf2, data, 8)
    with pytest.raises(KeyError):
        ev2.load_state_dict(sd)
    ev2.track_best([fe2, clf2])
    ev2.load_state_dict(sd)
    assert ev2.metric == metric and torch.equal(ev2.best, ev.best)
    assert all(torch.equal(ev2._shadow[k], ev._shadow[k]) for k in ev._shadow)
    with ev2.best_weights():
        assert torch.equal(whole_set(fe2, clf2, data)[0], whole_set_with(saved[best], data))


def whole_set_with(weights, data):
    gen = torch.Generator().manual_seed(0)
    fe, clf = StubFE(gen), StubClf(gen)
    with torch.no_grad():
        fe.w.copy_(weights["0.w"]); fe.shift.copy_(weights["0.shift"])
        clf.hidden.weight.copy_(weights["1.hidden.weight"]); clf.hidden.bias.copy_(weights["1.hidden.bias"])
    return whole_set(fe, clf, data)[0]


def test_feature_trans_is_applied():
    fe, clf, data = stub_pipeline()
    trans = nn.Linear(6, 6)
    ev = fst.Evaluator(fe, clf, data, 8, feature_trans=trans, n_class=3)
    with torch.no_grad():
        want = torch.cat([clf(trans(fe(data.x[i: i + 8])))[0].argmax(1) for i in range(0, 26, 8)])
    assert torch.equal(ev.run()["predictions"], want)


# ---------------------------------------------------------------------------------------------- voting
def test_precision_weights_from_confusion_equal_precision_weights():
    gen = torch.Generator().manual_seed(8)
    K, N, C = 3, 60, 5
    logits = torch.randn(K, N, C, generator=gen)
    logits[:, :, 4] = -50.0                                                   # a class no model predicts
    logits[1:, :, 3] = -50.0                                                  # a class only model 0 predicts
    labels = torch.randint(C, (N,), generator=gen)
    cm = torch.zeros(K, C, C, dtype=torch.int32)
    for k in range(K):
        for t, p in zip(labels.tolist(), logits[k].argmax(1).tolist()):
            cm[k, t, p] += 1
    assert int(cm[:, :, 4].sum()) == 0 and int(cm[0, :, 3].sum()) > 0 and int(cm[1:, :, 3].sum()) == 0
    want = voting.precision_weights(logits, labels)
    got = voting.precision_weights_from_confusion(cm)
    assert got.dtype == torch.float64 and torch.equal(got, want)
    assert (got[:, 4] == 0).all() and got[0, 3] > 0 and (got[1:, 3] == 0).all()
    with pytest.raises(ValueError):
        voting.precision_weights_from_confusion(cm[0])
