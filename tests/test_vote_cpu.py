"""Multi-source voting on the device, the parts that need no GPU: the ABI and the exports, the CPU branches of ``ops.vote_weights``
and ``ops.vote_fold`` (the executable specification the GPU tests compare the kernels with) against the golden vectors of the
reference block and against an independent fp64 computation written here, and ``VotingEvaluator.run()`` on stub modules.

Gates.  fp64 scores against fp64 scores: ``rtol = 1e-10``.  Every sum is over same-signed terms, so reordering C <= 4096 terms moves
it by at most C * 2^-53 = 4.5e-13 relative; exp and log add a few ulp; the absolute error of H <= ln C = 8.3 enters exp(-H) as a
relative error of the same size: 1e-10 is over 100x that bound, and a wrong term is an error of order 1.  Against the float32 golden
scores: ``rtol = 2e-5``, tests/test_voting_cpu.py's bound for ``voting.vote_scores``; weights: its ``rtol = 1e-12``.  Voted
predictions on random inputs are compared exactly only after asserting that every row's fp64 top-two relative score gap exceeds
1e-6 (no row is left out; the seeds were chosen so that the independent computation alone meets it); the constructed tie rows are
exempt, their equality being exact by construction.  Integer outputs are always compared exactly."""
import math
import os
import re

import numpy as np
import pytest
import torch

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import _lib, ops, voting
from test_evaluate_cpu import StubClf, StubFE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAN, INF = float("nan"), float("inf")
SHAPES = [(1, 1, 1), (3, 5, 2), (2, 8, 64), (4, 7, 65), (16, 3, 130)]         # (K, B, C)
RTOL, MIN_GAP = 1e-10, 1e-6


# ---------------------------------------------------------------------------------------------- shared with tests/test_gpu_vote.py
def make_calls(K, B, C, valids, seed=0, ld=None):
    """One (K logits [B, C] — views of [B, ld] if given —, labels, valid) per entry of ``valids``; random finite rows, and in row 0
    of member 0 the maximum twice (its own prediction: the lower index)."""
    gen = torch.Generator().manual_seed(seed * 7919 + K * 1009 + B * 131 + C)
    calls = []
    for v in valids:
        xs = [(torch.randn(B, ld or C, generator=gen) * 3)[:, :C] for _ in range(K)]
        if C > 1:
            xs[0][0, C - 1] = xs[0][0, 0] = xs[0][0].max() + 1
        calls.append((xs, torch.randint(C, (B,), generator=gen), v))
    return calls


def make_scale(K, C, seed=0, base=9.0):
    """(weights, scale) fp64 [K, C]: weights as a weighing pass leaves them, non-negative with mean 1 over the members."""
    gen = torch.Generator().manual_seed(seed * 31 + K * 17 + C)
    w = torch.rand(K, C, generator=gen, dtype=torch.float64)
    w = w / w.mean(dim=0, keepdim=True)
    return w, torch.pow(torch.tensor(base, dtype=torch.float64), w)


def argmax_ref(row):
    """torch.argmax on the CPU, spelled out: the first NaN, else the first maximum."""
    nan_at = [i for i, v in enumerate(row) if v != v]
    if nan_at:
        return nan_at[0]
    p = 0
    for i, v in enumerate(row):
        if v > row[p]:
            p = i
    return p


def vote_ref(calls, scale, C, capacity, sharpen=120.0):
    """The independent computation in numpy fp64: p by a plain softmax, H = -sum p log p over p > 0, the K terms added in order.
    Returns (state words, member hits, confusion, predictions, scores [rows, C], the smallest top-two relative gap of a finite row)."""
    K = len(calls[0][0])
    st, mh = [0] * 8, [0] * K
    cm = np.zeros((C, C), dtype=np.int64)
    preds, scores, gap = [], [], INF
    sc = scale.numpy()
    for xs, y, valid in calls:
        B = xs[0].shape[0]
        valid = min(max(valid, 0), B)
        if st[ops.EVAL_SEEN] + valid > capacity:
            st[ops.EVAL_OVERFLOW] += 1
            continue
        for r in range(valid):
            label = int(y[r])
            ok = 0 <= label < C
            total = np.zeros(C, dtype=np.float64)
            odd = False
            for k in range(K):
                row = xs[k][r].numpy().astype(np.float32)
                odd |= not np.isfinite(row).all()
                if ok and argmax_ref(row) == label:
                    mh[k] += 1
                with np.errstate(all="ignore"):
                    d = row.astype(np.float64)
                    m = np.float64(NAN) if np.isnan(d).any() else d.max()
                    e = np.exp(d - m)
                    p = e / e.sum()
                    H = -np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), np.where(np.isnan(p), p, 0.0)).sum()
                    total = total + p * (1.0 + sharpen * np.exp(-H)) * sc[k]
            pred = argmax_ref(total)
            preds.append(pred)
            scores.append(total)
            st[ops.EVAL_NONFINITE] += int(odd)
            if np.isfinite(total).all() and C > 1:
                top = np.sort(total)[::-1]
                gap = min(gap, float((top[0] - top[1]) / top[0]))
            if not ok:
                st[ops.EVAL_BAD_LABEL] += 1
                continue
            cm[label, pred] += 1
            st[ops.EVAL_HITS] += int(pred == label)
        st[ops.EVAL_BATCHES] += 1
        st[ops.EVAL_SEEN] += valid
    return st, mh, cm, preds, (np.stack(scores) if scores else np.zeros((0, C))), gap


def new_words(K, C, capacity):
    return (torch.zeros(8, dtype=torch.int32), torch.zeros(K, dtype=torch.int32), torch.zeros(C, C, dtype=torch.int32),
            torch.full((capacity,), -7, dtype=torch.int64), torch.full((capacity, C), -7.0, dtype=torch.float64))


def vote_cpu(calls, scale, C, capacity, sharpen=120.0):
    """The CPU branch.  Returns (state, member_hits, confusion, pred_out, scores_out) tensors."""
    K = len(calls[0][0])
    st, mh, cm, pred, keep = new_words(K, C, capacity)
    for xs, y, valid in calls:
        ops.vote_fold(xs, scale, y, torch.tensor([valid], dtype=torch.int32), st, mh, cm, pred, keep, sharpen=sharpen)
    return st, mh, cm, pred, keep


def check_cpu_against_ref(calls, scale, C, capacity, sharpen=120.0, ties=False):
    st, mh, cm, pred, keep = vote_cpu(calls, scale, C, capacity, sharpen)
    r_st, r_mh, r_cm, r_pred, r_scores, gap = vote_ref(calls, scale, C, capacity, sharpen)
    n = r_st[ops.EVAL_SEEN]
    print(f"smallest top-two gap {gap:.3e}")
    assert ties or gap > MIN_GAP, f"the inputs do not separate the two best classes: gap {gap:.3e}"
    if n:
        got = keep[:n].numpy()
        with np.errstate(all="ignore"):
            err = np.abs(got - r_scores) / np.abs(r_scores)
        print(f"scores: largest relative difference {np.nanmax(err) if np.isfinite(err).any() else 0.0:.3e}")
        np.testing.assert_allclose(got, r_scores, rtol=RTOL, atol=0, equal_nan=True)
    assert (keep[n:] == -7.0).all() and (pred[n:] == -7).all()
    assert st.tolist() == r_st and mh.tolist() == r_mh
    assert torch.equal(cm.long(), torch.from_numpy(r_cm)) and pred[:n].tolist() == r_pred
    return st, mh, cm, pred, keep


SPECIAL_X0 = [[0.5, 0.5, 0.5, 0.5], [1.0, -INF, 0.5, 0.0], [1.0, 2.0, 0.5, 0.0], [1.0, INF, 0.5, 0.0], [0.0, 1.0, 4.0, 2.0],
              [3.0, 1.0, 0.0, 2.0], [NAN, 2.0, 0.5, 0.0]]
SPECIAL_X1 = [[-2.0, -2.0, -2.0, -2.0], [0.0, -INF, 1.5, 1.0], [1.0, 2.0, NAN, 0.0], [1.0, 0.0, 0.5, 0.0], [0.5, 0.0, 3.0, 1.0],
              [2.5, 0.0, 1.0, 2.0], [1.0, NAN, 0.5, 0.0]]
SPECIAL_PRED = [0, 2, 0, 0, 2, 0, 0]                                          # all equal; finite; the NaN rule three times over; two plain rows
SPECIAL_Y = [0, 2, 1, 1, 2, 1, 3]


def special_calls():
    return [([torch.tensor(SPECIAL_X0), torch.tensor(SPECIAL_X1)], torch.tensor(SPECIAL_Y), 7)]


def special_scale():
    """Equal over the classes: an all-equal row keeps equal scores."""
    return torch.tensor([[2.0] * 4, [3.0] * 4], dtype=torch.float64)


def golden_confusions(votes, case):
    logits, labels = torch.tensor(votes[f"{case}.train_logits"]), torch.tensor(votes[f"{case}.train_labels"])
    K, _, C = logits.shape
    cm = torch.zeros(K, C, C, dtype=torch.int32)
    for k in range(K):
        for t, p in zip(labels.tolist(), logits[k].argmax(1).tolist()):
            cm[k, t, p] += 1
    return cm


def golden_calls(votes, case):
    """The golden test logits as three calls of unequal ``valid`` (the padding rows hold NaN logits and a label of -1)."""
    logits, labels = torch.tensor(votes[f"{case}.test_logits"]), torch.tensor(votes[f"{case}.test_labels"])
    K, M, C = logits.shape
    B = -(-M // 3) + 2
    cuts = [0, B, 2 * B - 5, M]
    assert cuts[2] < M <= cuts[2] + B
    calls = []
    for lo, hi in zip(cuts, cuts[1:]):
        xs = [torch.full((B, C), NAN) for _ in range(K)]
        y = torch.full((B,), -1, dtype=torch.int64)
        for k in range(K):
            xs[k][: hi - lo] = logits[k, lo:hi]
        y[: hi - lo] = labels[lo:hi]
        calls.append((xs, y, hi - lo))
    return calls


@pytest.fixture(scope="module")
def votes():
    return dict(np.load(os.path.join(GOLDEN, "voting_small.npz"), allow_pickle=False))


# ---------------------------------------------------------------------------------------------- ABI and exports
def test_abi_and_exports():
    text = open(os.path.join(ROOT, "include", "fst_hip.h")).read()
    version = int(re.search(r"#define\s+FST_ABI_VERSION\s+(\d+)", text).group(1))
    assert version == _lib.ABI_VERSION >= 27
    for name in ("fst_vote_weights", "fst_vote_fold"):
        assert name in _lib.EXPORTED_SYMBOLS and re.search(r"\bint\s+%s\s*\(" % name, text)
    for name in ("VotingEvaluator", "make_voter", "vote_fold", "vote_weights"):
        assert hasattr(fst, name), name
    assert ops.VOTE_MAX_K == 16 and ops.vote_scratch(5, "cpu").numel() == 10


def test_library_refuses_null_arguments():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfst_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    assert lib.fst_version() >= 27
    rc = lib.fst_vote_weights(None, 3, 4, 9.0, None, None, None)
    assert rc == -1 and b"fst_vote_weights" in lib.fst_last_error()
    rc = lib.fst_vote_fold(None, 3, 4, None, 5, 4, None, None, None, None, None, None, None, 120.0, 5, None, None)
    assert rc == -1 and b"fst_vote_fold" in lib.fst_last_error()


# ---------------------------------------------------------------------------------------------- the golden vectors
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_golden_weights(votes, case):
    cm = golden_confusions(votes, case)
    K, C = cm.shape[:2]
    w, scale = torch.full((K, C), -7.0, dtype=torch.float64), torch.full((K, C), -7.0, dtype=torch.float64)
    ops.vote_weights(list(cm), w, scale)
    np.testing.assert_allclose(w.numpy(), votes[f"{case}.weights"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(w.numpy(), voting.precision_weights_from_confusion(cm).numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(scale.numpy(), 9.0 ** votes[f"{case}.weights"], rtol=1e-12, atol=0)
    if case == "c":
        assert (w[:, 4] == 0).all() and (scale[:, 4] == 1).all()              # the never-predicted class: 0 / 0 -> 0


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_golden_scores(votes, case):
    cm = golden_confusions(votes, case)
    K, C = cm.shape[:2]
    M = votes[f"{case}.test_labels"].shape[0]
    w, scale = torch.zeros(K, C, dtype=torch.float64), torch.zeros(K, C, dtype=torch.float64)
    ops.vote_weights(list(cm), w, scale)
    st, mh, _, pred, keep = vote_cpu(golden_calls(votes, case), scale, C, capacity=M)
    err = np.abs(keep.numpy() - votes[f"{case}.scores"]) / votes[f"{case}.scores"]
    print(f"scores against the reference block: largest relative difference {err.max():.3e}")
    np.testing.assert_allclose(keep.numpy(), votes[f"{case}.scores"], rtol=2e-5, atol=0)
    assert np.array_equal(pred.numpy(), votes[f"{case}.pred"])
    assert st.tolist() == [M, int(st[ops.EVAL_HITS]), 3, 0, 0, 0, 0, 0] and int(st[ops.EVAL_HITS]) / M == float(votes[f"{case}.acc"])
    own = torch.tensor(votes[f"{case}.test_logits"]).argmax(2) == torch.tensor(votes[f"{case}.test_labels"])
    assert mh.tolist() == own.sum(1).tolist()


# ---------------------------------------------------------------------------------------------- vote_fold, the CPU branch
@pytest.mark.parametrize("K,B,C", SHAPES)
def test_fold_equals_independent_computation(K, B, C):
    _, scale = make_scale(K, C)
    for valid in sorted({0, 1, B - 1, B}):
        st, _, cm, _, _ = check_cpu_against_ref(make_calls(K, B, C, [valid]), scale, C, capacity=B)
        assert st[ops.EVAL_SEEN] == valid == int(cm.sum())
    ld = C + 3 if (K, B, C) == (4, 7, 65) else None                           # rows strided: ld > C
    st, _, cm, _, _ = check_cpu_against_ref(make_calls(K, B, C, [B, B - 1, B], seed=1, ld=ld), scale, C, capacity=3 * B)
    assert st[ops.EVAL_SEEN] == 3 * B - 1 == int(cm.sum()) and st[ops.EVAL_BATCHES] == 3
    check_cpu_against_ref(make_calls(K, B, C, [B], seed=2), torch.ones(K, C, dtype=torch.float64), C, capacity=B, sharpen=2.0)


def test_special_rows():
    st, mh, cm, pred, keep = check_cpu_against_ref(special_calls(), special_scale(), 4, capacity=7, ties=True)
    assert pred.tolist() == SPECIAL_PRED
    # rows 1, 2, 3 and 6 hold a NaN or an inf (row 6 in both members: counted once); hits: rows 0, 1 and 4
    assert st.tolist() == [7, 3, 1, 0, 4, 0, 0, 0]
    assert len(set(keep[0].tolist())) == 1                                    # the all-equal row: equal scores, class 0 wins
    assert torch.isfinite(keep[1]).all() and keep[1, 1] == 0                  # -inf in both members: probability 0, no NaN
    assert torch.isnan(keep[[2, 3, 6]]).all() and torch.isfinite(keep[[4, 5]]).all()
    assert mh.tolist() == [4, 3]                                              # member 0: rows 0, 2, 3 (the inf) and 4; member 1: rows 0, 1 and 4
    # the -inf row with one member alone: what the plain formula gives on the three finite classes
    x = torch.tensor([SPECIAL_X0[1]])
    _, _, _, _, alone = vote_cpu([([x], torch.tensor([0]), 1)], torch.ones(1, 4, dtype=torch.float64), 4, capacity=1)
    p = torch.softmax(x[0, [0, 2, 3]].double(), 0)
    want = p * (1 + 120 * torch.exp((p * p.log()).sum()))
    np.testing.assert_allclose(alone[0, [0, 2, 3]].numpy(), want.numpy(), rtol=RTOL)


def test_bad_label_is_counted_and_kept_out():
    K, B, C = 3, 5, 3
    xs, y, v = make_calls(K, B, C, [B], seed=3)[0]
    y = y.clone(); y[1], y[3] = 3, -1
    _, scale = make_scale(K, C)
    st, mh, cm, pred, _ = check_cpu_against_ref([(xs, y, v)], scale, C, capacity=B)
    assert st[ops.EVAL_BAD_LABEL] == 2 and st[ops.EVAL_SEEN] == 5 and int(cm.sum()) == 3 and (pred >= 0).all()
    keep = torch.tensor([0, 2, 4])
    assert mh.tolist() == [int((x[keep].argmax(1) == y[keep]).sum()) for x in xs]
    assert int(st[ops.EVAL_HITS]) == int((pred[keep] == y[keep]).sum())


def test_capacity_overflow_writes_nothing_else():
    K, B, C = 2, 5, 3
    _, scale = make_scale(K, C)
    calls = make_calls(K, B, C, [5, 5, 2], seed=4)
    st, mh, cm, pred, keep = check_cpu_against_ref(calls, scale, C, capacity=8)   # 5, then 5 more do not fit, then 2 do
    assert st.tolist()[:6] == [7, int(st[ops.EVAL_HITS]), 2, 0, 0, 1] and pred[7] == -7 and (keep[7] == -7.0).all()
    first = vote_cpu(calls[:1], scale, C, capacity=8)
    both = vote_cpu(calls[:2], scale, C, capacity=8)
    assert both[0].tolist()[:6] == first[0].tolist()[:5] + [1]
    assert all(torch.equal(a, b) for a, b in zip(first[1:], both[1:]))
    st = check_cpu_against_ref(make_calls(K, B, C, [9, -4], seed=5), scale, C, capacity=5)[0]      # valid is clamped to 0..B
    assert st.tolist()[:3] == [5, int(st[ops.EVAL_HITS]), 2]


def test_arguments_are_validated():
    K, B, C = 2, 3, 4
    xs, y, _ = make_calls(K, B, C, [B])[0]
    _, scale = make_scale(K, C)
    st, mh, cm, pred, keep = new_words(K, C, B)
    valid = torch.tensor([B], dtype=torch.int32)
    ops.vote_fold(xs, scale, y, valid, st, mh, cm, pred, keep)
    for bad in (dict(logits=xs * 9), dict(logits=[]), dict(logits=[xs[0], xs[1][:, :3]]), dict(scale=scale[:1]), dict(scale=scale.float()),
                dict(member_hits=torch.zeros(3, dtype=torch.int32)), dict(confusion=torch.zeros(3, 3, dtype=torch.int32)),
                dict(pred_out=None), dict(scores_out=torch.zeros(B, C)), dict(sharpen=-1.0), dict(sharpen=INF), dict(capacity=B + 1),
                dict(labels=y[:2]), dict(state=torch.zeros(6, dtype=torch.int32))):
        args = dict(logits=xs, scale=scale, labels=y, valid=valid, state=st, member_hits=mh, confusion=cm, pred_out=pred,
                    scores_out=keep, sharpen=120.0, capacity=None)
        args.update(bad)
        with pytest.raises(ValueError, match="vote_fold"):
            ops.vote_fold(**args)
    cms = [torch.zeros(C, C, dtype=torch.int32) for _ in range(K)]
    w = torch.zeros(K, C, dtype=torch.float64)
    for bad in (dict(confusions=cms * 9), dict(confusions=[cms[0], cms[1][:3, :3]]), dict(confusions=[c.long() for c in cms]),
                dict(weights_out=w[:1]), dict(scale_out=w.float()), dict(base=0.0), dict(base=INF), dict(base=NAN)):
        args = dict(confusions=cms, weights_out=w, scale_out=w.clone(), base=9.0)
        args.update(bad)
        with pytest.raises(ValueError, match="vote_weights"):
            ops.vote_weights(**args)


def test_weights_of_an_all_zero_column_and_a_single_member():
    cm = torch.tensor([[[3, 0, 1], [1, 0, 0], [0, 0, 2]], [[1, 0, 2], [0, 0, 1], [2, 0, 1]]], dtype=torch.int32)
    w, scale = torch.zeros(2, 3, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.float64)
    ops.vote_weights(list(cm), w, scale, base=4.0)
    prec = np.array([[3 / 4, 0, 2 / 3], [1 / 3, 0, 1 / 4]])
    want = np.where(prec.mean(0) > 0, prec / np.where(prec.mean(0) > 0, prec.mean(0), 1), 0)
    np.testing.assert_allclose(w.numpy(), want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(scale.numpy(), 4.0 ** want, rtol=1e-12, atol=0)
    w1, s1 = torch.zeros(1, 3, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.float64)
    ops.vote_weights([cm[0]], w1, s1)
    assert w1.tolist() == [[1.0, 0.0, 1.0]] and s1.tolist() == [[9.0, 1.0, 9.0]]


# ---------------------------------------------------------------------------------------------- VotingEvaluator.run() on stub modules
def stub_members(K=3, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [(StubFE(gen), StubClf(gen)) for _ in range(K)]


def stub_sets(n_train, n_test, seed=0):
    gen = torch.Generator().manual_seed(100 + seed)
    train = fst.DeviceDataset(torch.randn(n_train, 2, 5, generator=gen), torch.randint(3, (n_train,), generator=gen), "cpu")
    test = fst.DeviceDataset(torch.randn(n_test, 2, 5, generator=gen), torch.randint(3, (n_test,), generator=gen), "cpu")
    return train, test


def score_gap(scores):
    top = torch.sort(scores, dim=1, descending=True).values
    return float(((top[:, 0] - top[:, 1]) / top[:, 0]).min())


@pytest.mark.parametrize("n_test", [26, 24, 3])
def test_voting_evaluator_equals_multi_source_voting(n_test):
    members = stub_members()
    train, test = stub_sets(26, n_test)
    members[0][0].train(); members[1][1].train(); members[2][0].eval()
    modes = [(fe.training, clf.training) for fe, clf in members]
    ve = fst.VotingEvaluator(members, train, test, 8, keep_scores=True)
    with pytest.raises(RuntimeError, match="weigh"):
        ve.run()
    rep = ve.run(weigh=True)
    assert [(fe.training, clf.training) for fe, clf in members] == modes      # modes restored
    for fe, clf in members:
        fe.eval(); clf.eval()
    w, scores, pred, acc = voting.multi_source_voting(members, train.batches(8), test.batches(8))
    gap = score_gap(rep["scores"])
    print(f"smallest top-two gap {gap:.3e}")
    assert gap > MIN_GAP
    np.testing.assert_allclose(rep["weights"].numpy(), w.numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(rep["scale"].numpy(), (9.0 ** w).numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(rep["scores"].numpy(), scores.numpy(), rtol=2e-5, atol=0)
    assert torch.equal(rep["predictions"], pred) and float(rep["accuracy"]) == acc
    with torch.no_grad():
        own = [int((clf(fe(test.x))[0].argmax(1) == test.y).sum()) for fe, clf in members]
    assert rep["member_hits"].tolist() == own and rep["member_accuracy"].tolist() == [h / n_test for h in own]
    assert int(rep["seen"]) == n_test and int(rep["batches"]) == -(-n_test // 8) and rep["labels"] is test.y
    assert [int(rep[k]) for k in ("bad_label", "nonfinite", "overflow")] == [0, 0, 0]
    assert int(rep["confusion"].sum()) == n_test and int(torch.diagonal(rep["confusion"]).sum()) == int(rep["hits"])
    res = ve.result()
    assert res["hits"] == int(rep["hits"]) and res["accuracy"] == acc and torch.equal(res["predictions"], pred)
    assert torch.equal(res["scores"], rep["scores"]) and res["feed"] == {"overrun": 0, "bad_index": 0}
    assert res["member_hits"].tolist() == own and torch.equal(res["weights"], rep["weights"])
    ve.check()
    # weights computed elsewhere in the place of the weighing pass: the same vote
    other = fst.VotingEvaluator(members, train, test, 8, keep_scores=True)
    other.set_weights(rep["weights"])
    rep2 = other.run()
    for k in rep:
        assert torch.equal(rep[k], rep2[k]), k
    other.check()
    assert "scores" not in fst.VotingEvaluator(members, train, test, 8).run(weigh=True)


class StubTrans(torch.nn.Module):
    """Elementwise, so a row's features do not depend on the batch it arrives in."""

    def forward(self, f):
        return f * 0.5 + 1.0


def test_entropy_only_vote_and_a_feature_trans():
    members = stub_members(2, seed=3)
    trans = StubTrans()
    members[1] = members[1] + (trans,)
    train, test = stub_sets(9, 11, seed=1)
    ve = fst.make_voter(members, train, test, 4, base=1.0, sharpen=2.0, keep_scores=True, n_class=3)
    rep = ve.run(weigh=True)
    assert (rep["scale"] == 1).all()
    with torch.no_grad():
        logits = [members[0][1](members[0][0](test.x))[0], members[1][1](trans(members[1][0](test.x)))[0]]
    p = torch.softmax(torch.stack(logits).double(), 2)
    H = -(p * p.log()).sum(2, keepdim=True)
    np.testing.assert_allclose(rep["scores"].numpy(), (p * (1 + 2 * torch.exp(-H))).sum(0).numpy(), rtol=RTOL, atol=0)


def test_voting_evaluator_refuses():
    train, test = stub_sets(9, 9)
    with pytest.raises(ValueError, match="17 members"):
        fst.VotingEvaluator(stub_members(17), train, test, 8)
    with pytest.raises(ValueError, match="0 members"):
        fst.VotingEvaluator([], train, test, 8)
    with pytest.raises(ValueError, match="n_class"):
        fst.VotingEvaluator(stub_members(2), train, test, 8, n_class=4)       # the classifiers have 3 classes
    gen = torch.Generator().manual_seed(0)
    with pytest.raises(ValueError, match="n_class"):
        fst.VotingEvaluator([(StubFE(gen), StubClf(gen)), (StubFE(gen), StubClf(gen, C=4))], train, test, 8)
    for kw in (dict(base=0.0), dict(base=INF), dict(sharpen=-1.0), dict(sharpen=NAN)):
        with pytest.raises(ValueError, match="base"):
            fst.VotingEvaluator(stub_members(2), train, test, 8, **kw)
    short = fst.DeviceDataset(torch.randn(4, 2, 6), torch.zeros(4, dtype=torch.int64), "cpu")
    with pytest.raises(ValueError, match="series shape"):
        fst.VotingEvaluator(stub_members(2), train, short, 8)
    with pytest.raises(ValueError, match="make_voter"):
        fst.make_voter([object()], train, test, 8)
    ve = fst.VotingEvaluator(stub_members(2), train, test, 8)
    with pytest.raises(ValueError, match="set_weights"):
        ve.set_weights(torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        ve.capture()
    test.y[2] = 5
    ve.run(weigh=True)
    with pytest.raises(RuntimeError, match="bad_label = 1"):
        ve.check()
