"""Evaluation on the GPU: ``fst_eval_fold`` / ``fst_eval_finish`` against the CPU branch of ``ops.eval_fold`` inside guard bands,
then ``Evaluator`` on the real pipelines: the eager pass against the forward run by hand, the replayed pass against the eager one,
the best weights kept under replay, the source side, and the vote from confusion matrices.

Gates.  Predictions, confusion, every state word and the stored logits: ``torch.equal`` (the logits on int32 views, so NaN
payloads and -0.0 count).  The loss sum: ``|gpu - cpu| <= 1e-11 * rows * max(1, max|finite logit|)``: both sides are fp64 with at
most C + a few roundings per row, about (C + 10) * 2^-53 = 2e-14 per row at C = 130; the gate sits three orders above that and
four below what an fp32 accumulation would give.  Replayed against eager passes: the same kernels on the same inputs, so
``torch.equal`` on everything, the loss word bit for bit.  The hand-run forwards use the SAME padded batches as the evaluator: a
shorter tail batch may take another kernel instance and round differently."""
import contextlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import _lib, checkpoint, ops, voting
from test_evaluate_cpu import SHAPES, SPECIAL, fold_cpu, loss_close, make_calls, special_calls
from test_gpu_phase_graphs import toy

DEV = "cuda"
BAND = 64                                                                     # words of sentinel on each side of a tensor
SENTINEL = 0x5A5A5A5A                                                         # outputs' bands
NAN_WORD = 0x7FC00000                                                         # inputs' bands: a NaN that must reach no output


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int64)


class Banded:
    """A CPU tensor's words on the device between two bands of ``fill``, ``off`` words behind a 256-byte boundary."""

    def __init__(self, cpu, fill, off=0):
        words = cpu.contiguous().view(torch.int32).reshape(-1)
        self.lo, self.n, self.fill = BAND + off, words.numel(), fill
        self.buf = torch.full((self.lo + self.n + BAND,), fill, dtype=torch.int32, device=DEV)
        assert self.buf.data_ptr() % 256 == 0
        self.buf[self.lo: self.lo + self.n] = words.to(DEV)
        self.view = self.buf[self.lo: self.lo + self.n].view(cpu.dtype).view(cpu.shape)
        assert self.view.data_ptr() % 16 == (4 * off) % 16 and self.view.is_contiguous()
        self.initial = self.buf.clone()

    def bands_intact(self):
        return bool((self.buf[: self.lo] == self.fill).all()) and bool((self.buf[self.lo + self.n:] == self.fill).all())

    def untouched(self):
        return torch.equal(self.buf, self.initial)


class Words:
    """The outputs of a fold on the device, each inside bands: state, loss, confusion, pred_out, logits_out and the scratch."""

    def __init__(self, B, C, capacity):
        self.state = Banded(torch.zeros(8, dtype=torch.int32), SENTINEL)
        self.loss = Banded(torch.zeros(1, dtype=torch.float64), SENTINEL)
        self.confusion = Banded(torch.zeros(C, C, dtype=torch.int32), SENTINEL)
        self.pred = Banded(torch.full((capacity,), -7, dtype=torch.int64), SENTINEL)
        self.keep = Banded(torch.full((capacity, C), -7.0), SENTINEL)
        self.scratch = Banded(torch.zeros(B + (B + 1) // 2, dtype=torch.float64), SENTINEL)
        self.all = (self.state, self.loss, self.confusion, self.pred, self.keep, self.scratch)
        assert self.state.view.data_ptr() % 16 == 0 and self.loss.view.data_ptr() % 8 == 0 and self.scratch.view.data_ptr() % 8 == 0

    def outputs(self):
        return tuple(b.view.cpu() for b in self.all[:5])


def fold_gpu(calls, C, capacity, off=0):
    """The kernel on ``calls``: inputs inside NaN bands (``off`` words off a 16-byte boundary for the logits), outputs inside
    sentinel bands.  Returns the outputs on the CPU after checking bands and inputs."""
    B = calls[0][0].size(0)
    w = Words(B, C, capacity)
    held = []
    for x, y, valid in calls:
        wide = x._base if x._base is not None else x                          # the [B, ld] tensor a strided case views
        gx = Banded(wide, NAN_WORD, off)
        gy = Banded(y, NAN_WORD)
        gv = Banded(torch.tensor([valid], dtype=torch.int32), NAN_WORD)
        ops.eval_fold(gx.view[:, :C], gy.view, gv.view, w.state.view, w.loss.view, w.confusion.view, w.pred.view, w.keep.view,
                      scratch=w.scratch.view)
        held.append((gx, gy, gv, wide, y, valid))
    for gx, gy, gv, wide, y, valid in held:
        assert gx.bands_intact() and gy.bands_intact() and gv.bands_intact()
        assert torch.equal(bits(gx.view.cpu()), bits(wide)) and torch.equal(gy.view.cpu(), y) and int(gv.view) == valid, "an input was written"
    assert all(b.bands_intact() for b in w.all), "a guard band was written"
    return w.outputs()


def check_gpu_against_cpu(calls, C, capacity, off=0):
    got = fold_gpu(calls, C, capacity, off)
    want = fold_cpu(calls, C, capacity)
    names = ("state", "loss", "confusion", "pred_out", "logits_out")
    for name, g, c in zip(names, got, want):
        if name == "loss":
            finite = torch.cat([x[:max(0, min(v, x.size(0)))].reshape(-1) for x, _, v in calls])
            finite = finite[torch.isfinite(finite)]
            scale = float(finite.abs().max()) if finite.numel() else 1.0
            rows = int(want[0][ops.EVAL_SEEN])
            print(f"loss: gpu {float(g):.17g}, cpu {float(c):.17g}, gate {1e-11 * max(rows, 1) * max(1.0, scale):.3e}")
            assert loss_close(float(g), float(c), rows, scale), (float(g), float(c))
        else:
            assert torch.equal(bits(g), bits(c)), f"{name}: the kernel differs from the CPU branch"
    again = fold_gpu(calls, C, capacity, off)                                 # a second run of the same calls: the same words
    for name, g, a in zip(names, got, again):
        assert torch.equal(bits(g), bits(a)), f"{name}: two runs differ"
    return got


# ---------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("B,C", SHAPES)
def test_kernel_equals_cpu_branch(B, C):
    for valid in sorted({0, 1, B - 1, B}):
        state = check_gpu_against_cpu(make_calls(B, C, [valid]), C, capacity=B)[0]
        assert state[ops.EVAL_SEEN] == valid
    check_gpu_against_cpu(make_calls(B, C, [B], ld=C + 3), C, capacity=B)     # rows strided: ld > C
    check_gpu_against_cpu(make_calls(B, C, [B]), C, capacity=B, off=1)        # logits 4 bytes off a 16-byte boundary
    state = check_gpu_against_cpu(make_calls(B, C, [B, B - 1, B], seed=1, ld=C + 1), C, capacity=3 * B, off=1)[0]
    assert state.tolist() == [3 * B - 1, int(state[ops.EVAL_HITS]), 3, 0, 0, 0, 0, 0]


def test_more_rows_than_one_pass_of_the_advance_kernel():
    """B = 600: 150 workgroups of rows, three 256-row tiles of the loss chain."""
    state = check_gpu_against_cpu(make_calls(600, 10, [600, 599], seed=2), 10, capacity=1200)[0]
    assert state[ops.EVAL_SEEN] == 1199


def test_special_rows():
    state, loss, _, pred, _ = check_gpu_against_cpu(special_calls(), 4, capacity=6)
    assert pred.tolist() == [p for _, p in SPECIAL] + [3]
    assert state.tolist() == [6, 4, 1, 0, 4, 0, 0, 0] and math.isnan(float(loss))
    state, loss, _, _, _ = check_gpu_against_cpu(special_calls(), 4, capacity=6, off=1)
    x, y, _ = special_calls()[0]
    finite = [(x[[1, 5]].contiguous(), y[[1, 5]].contiguous(), 2)]
    loss2 = check_gpu_against_cpu(finite, 4, capacity=2)[1]
    assert abs(float(loss2) - float(torch.nn.functional.cross_entropy(finite[0][0].double(), finite[0][1], reduction="sum"))) <= 1e-12


def test_bad_label_and_overflow():
    x, y, v = make_calls(5, 3, [5], seed=3)[0]
    y = y.clone(); y[1], y[3] = 3, -1
    state = check_gpu_against_cpu([(x, y, v)], 3, capacity=5)[0]
    assert state[ops.EVAL_BAD_LABEL] == 2 and state[ops.EVAL_SEEN] == 5
    state, _, _, pred, _ = check_gpu_against_cpu(make_calls(5, 3, [5, 5, 2], seed=4), 3, capacity=8)
    assert state.tolist()[:6] == [7, int(state[ops.EVAL_HITS]), 2, 0, 0, 1] and pred[7] == -7
    state = check_gpu_against_cpu(make_calls(5, 3, [9, -4], seed=5), 3, capacity=5)[0]      # valid is clamped to 0..B
    assert state.tolist()[:3] == [5, int(state[ops.EVAL_HITS]), 2]


def test_padding_rows_are_never_read():
    B, C = 7, 65
    x, y, _ = make_calls(B, C, [B], seed=6)[0]
    dirty_x, dirty_y = x.clone(), y.clone()
    dirty_x[4:], dirty_y[4:] = float("nan"), 2 ** 40
    clean = check_gpu_against_cpu([(x, y, 4)], C, capacity=B)
    dirty = check_gpu_against_cpu([(dirty_x, dirty_y, 4)], C, capacity=B)
    for c, d in zip(clean, dirty):
        assert torch.equal(bits(c), bits(d))
    assert dirty[0].tolist()[:6] == [4, int(clean[0][ops.EVAL_HITS]), 1, 0, 0, 0]
    assert not torch.isnan(dirty[4][:4]).any() and (dirty[4][4:] == -7.0).all() and (dirty[3][4:] == -7).all()


def test_finish_equals_cpu_branch():
    steps = [(10, 0, 5.0, 10, 0, 0), (10, 4, 7.0, 10, 0, 0), (10, 4, 1.0, 10, 0, 0), (9, 9, 0.5, 10, 0, 0), (10, 9, 0.5, 10, 1, 0),
             (10, 9, 0.5, 10, 0, 2), (10, 9, float("nan"), 10, 0, 0)]
    for mode in (0, 1):
        cpu_best, gpu_best = ops.eval_best_block("cpu"), Banded(ops.eval_best_block("cpu"), SENTINEL)
        for seen, hits, loss, expect, overflow, bad in steps:
            st = torch.zeros(8, dtype=torch.int32)
            st[ops.EVAL_SEEN], st[ops.EVAL_HITS], st[ops.EVAL_OVERFLOW], st[ops.EVAL_BAD_LABEL] = seen, hits, overflow, bad
            lo = torch.tensor([loss], dtype=torch.float64)
            ops.eval_finish(st, lo, expect, cpu_best, mode)
            ops.eval_finish(st.to(DEV), lo.to(DEV), expect, gpu_best.view, mode)
            assert gpu_best.view.cpu().tolist() == cpu_best.tolist(), (mode, seen, hits, loss)
        assert gpu_best.bands_intact() and cpu_best[ops.EVAL_PASSES] == len(steps) and cpu_best[ops.EVAL_INCOMPLETE] == 3


def test_bad_arguments_are_refused_before_the_first_launch():
    lib = _lib.load()
    B, C, cap = 5, 3, 8
    x, y, _ = make_calls(B, C, [B])[0]
    gx, gy, gv = Banded(x, NAN_WORD), Banded(y, NAN_WORD), Banded(torch.tensor([B], dtype=torch.int32), NAN_WORD)
    w = Words(B, C, cap)
    p = {"logits": gx.view.data_ptr(), "ld": C, "labels": gy.view.data_ptr(), "B": B, "C": C, "valid": gv.view.data_ptr(),
         "state": w.state.view.data_ptr(), "loss": w.loss.view.data_ptr(), "confusion": w.confusion.view.data_ptr(),
         "pred_out": w.pred.view.data_ptr(), "logits_out": w.keep.view.data_ptr(), "capacity": cap, "scratch": w.scratch.view.data_ptr()}
    order = list(p)
    bad = [("B", 0), ("B", 1 << 31), ("C", 0), ("C", 4097), ("ld", C - 1), ("capacity", 0), ("capacity", 1 << 31)]
    bad += [(k, None) for k in ("logits", "labels", "valid", "state", "loss", "confusion", "scratch")]
    bad += [("logits", p["logits"] + 2), ("valid", p["valid"] + 2), ("confusion", p["confusion"] + 2), ("logits_out", p["logits_out"] + 2),
            ("labels", p["labels"] + 4), ("loss", p["loss"] + 4), ("pred_out", p["pred_out"] + 4), ("scratch", p["scratch"] + 4),
            ("state", p["state"] + 8)]
    bad += [("pred_out", p["labels"]), ("logits_out", p["logits"]), ("confusion", p["state"]), ("scratch", p["loss"]),
            ("loss", p["valid"] - 4), ("pred_out", p["logits_out"])]
    for key, value in bad:
        args = dict(p)
        args[key] = value
        rc = lib.fst_eval_fold(*[args[k] for k in order], None)
        msg = lib.fst_last_error()
        assert rc == -1 and msg and b"fst_eval_fold" in msg, (key, value, rc, msg)
    torch.cuda.synchronize()
    assert all(b.untouched() for b in w.all), "a refused call wrote something"
    best = Banded(ops.eval_best_block("cpu"), SENTINEL)
    q = {"state": p["state"], "loss": p["loss"], "expect": 5, "best": best.view.data_ptr(), "mode": 0}
    for key, value in [("state", None), ("loss", None), ("best", None), ("state", q["state"] + 4), ("best", q["best"] + 8),
                       ("loss", q["loss"] + 4), ("mode", 2), ("mode", -1), ("expect", -1), ("expect", 1 << 31), ("best", q["state"])]:
        args = dict(q)
        args[key] = value
        rc = lib.fst_eval_finish(*[args[k] for k in q], None)
        msg = lib.fst_last_error()
        assert rc == -1 and msg and b"fst_eval_finish" in msg, (key, value, rc, msg)
    torch.cuda.synchronize()
    assert best.untouched() and w.state.untouched()


# ---------------------------------------------------------------------------------------------- the evaluator on the real pipelines
def series(n, length, n_class, seed, channels=1):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, channels, length, generator=gen), torch.randint(n_class, (n,), generator=gen)


def classifier(seed=5, steps=3, **kw):
    """``ClassifierTrainer(64, 1, 3)`` after ``steps`` train steps on a fixed batch; returns (trainer, that batch)."""
    torch.manual_seed(seed)
    tr = fst.ClassifierTrainer(64, 1, 3, DEV, **kw)
    x, y = series(8, 64, 3, seed + 100)
    x, y = x.to(DEV), y.to(DEV)
    for _ in range(steps):
        tr.step(x, y)
    return tr, (x, y)


def by_hand(mods, data, B, trans=None):
    """Eval-mode logits of the pipeline on the evaluator's own padded batches, [N, C]."""
    fe, clf = mods
    N = len(data)
    modes = [m.training for m in (fe, clf)]
    fe.eval(); clf.eval()
    out = []
    with torch.no_grad():
        for i in range(0, N, B):
            idx = torch.arange(i, i + B).clamp(max=N - 1).to(DEV)
            f = fe(data.x.index_select(0, idx))
            if trans is not None:
                f = trans(f)
            out.append(clf(f)[0][: min(B, N - i)])
    fe.train(modes[0]); clf.train(modes[1])
    return torch.cat(out)


@contextlib.contextmanager
def no_host_sync():
    """Inside, torch raises on anything that makes the host wait for the device: a host read, a blocking copy, a synchronise."""
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def same_reports(a, b, what, skip=()):
    assert set(a) == set(b), what
    for k in a:
        if k not in skip:
            assert torch.equal(bits(a[k]), bits(b[k])), f"{what}: {k} differs"


def fresh(ev):
    """Forget the passes so far, so that two passes' reports can be compared key for key."""
    ev.best.copy_(ops.eval_best_block(DEV))


def test_eager_pass_on_the_classifier():
    tr, _ = classifier()
    x, y = series(26, 64, 3, 1)
    data = fst.DeviceDataset(x, y, DEV)
    ev = tr.make_evaluator(data, 8, keep_logits=True)
    rep = ev.run()
    assert tr.fe.training and tr.clf.training
    want = by_hand((tr.fe, tr.clf), data, 8)
    assert torch.equal(bits(rep["logits"]), bits(want)), "the stored logits differ from the forward run by hand"
    st, loss, cm, pred, _ = fold_cpu([(want.cpu(), y, 26)], 3, 26)            # every metric: the CPU branch on those logits
    assert torch.equal(rep["predictions"].cpu(), pred) and torch.equal(rep["confusion"].cpu(), cm)
    assert [int(rep[k]) for k in ("seen", "hits", "bad_label", "nonfinite", "overflow")] == [26, int(st[ops.EVAL_HITS]), 0, 0, 0]
    assert int(rep["batches"]) == 4 and int(rep["improved"]) == 1 and float(rep["accuracy"]) == int(st[ops.EVAL_HITS]) / 26
    print(f"loss sum: gpu {float(rep['loss']) * 26:.17g}, cpu {float(loss):.17g}")
    assert loss_close(float(rep["loss"]) * 26, float(loss), 26, float(want.abs().max()))
    ev.check()
    # no tail: accuracy and predictions are eval_accuracy's over the resident set's batches, exactly
    data24 = fst.DeviceDataset(x[:24], y[:24], DEV)
    rep24 = tr.make_evaluator(data24, 8).run()
    tr.fe.eval(); tr.clf.eval()
    acc, preds = checkpoint.eval_accuracy(tr.fe, tr.clf, data24.batches(8))
    tr.fe.train(); tr.clf.train()
    assert torch.equal(rep24["predictions"], preds) and float(rep24["accuracy"]) == acc and "logits" not in rep24


def test_replay_equals_eager():
    tr, (bx, by) = classifier(weight_average={"decay": 0.5, "warmup": False})
    x, y = series(26, 64, 3, 2)
    data = fst.DeviceDataset(x, y, DEV)
    ev = tr.make_evaluator(data, 8, keep_logits=True)
    eager = ev.run()
    ev.capture()
    assert ops._PACK_CACHE is None and tr.fe.training and tr.clf.training
    fresh(ev)
    with no_host_sync():                                                      # launches only: nothing in a replay waits for the device
        replayed = ev.replay()
    same_reports(replayed, eager, "replay against run()")
    assert torch.equal(bits(replayed["logits"]), bits(by_hand((tr.fe, tr.clf), data, 8)))
    # two consecutive replays are equal, and passes counts both
    second = ev.replay()
    same_reports(second, replayed, "two replays", skip=("improved", "passes"))
    assert int(replayed["passes"]) == 1 and int(second["passes"]) == 2 and int(replayed["improved"]) == 1 and int(second["improved"]) == 0
    # three train replays later the replayed pass evaluates the weights as they now are
    tr.capture(bx, by)
    for _ in range(3):
        tr.replay(bx, by)
    fresh(ev)
    after = ev.replay()
    fresh(ev)
    same_reports(after, ev.run(), "replay against run() after three train replays")
    assert not torch.equal(after["logits"], replayed["logits"]), "the replay did not follow the live weights"
    # inside averaged_weights() it evaluates the averages
    with tr.averaged_weights():
        fresh(ev)
        avg = ev.replay()
        fresh(ev)
        same_reports(avg, ev.run(), "replay against run() inside averaged_weights()")
    assert not torch.equal(avg["logits"], after["logits"]), "the averaged weights gave the live weights' logits"
    fresh(ev)
    same_reports(ev.replay(), after, "back on the live weights")
    ev.check()
    assert ev.result()["passes"] == 1


def test_replay_of_a_single_round():
    """N <= B: the whole pass is the prepare graph's round; the batch graph is never replayed."""
    tr, _ = classifier()
    x, y = series(5, 64, 3, 7)
    data = fst.DeviceDataset(x, y, DEV)
    ev = tr.make_evaluator(data, 8, keep_logits=True)
    eager = ev.run()
    ev.capture()
    fresh(ev)
    same_reports(ev.replay(), eager, "one round")
    assert int(eager["seen"]) == 5 and int(eager["batches"]) == 1 and ev.replay(report=False) is None
    assert torch.equal(bits(eager["logits"]), bits(by_hand((tr.fe, tr.clf), data, 8)))
    ev.check()


def test_best_weights_under_replay():
    tr, (bx, by) = classifier(steps=1)
    x, y = series(26, 64, 3, 3)
    data = fst.DeviceDataset(x, y, DEV)
    ev = tr.make_evaluator(data, 8)
    ev.track_best({"fe": tr.fe, "clf": tr.clf})
    ev.capture()
    tr.capture(bx, by)
    reports, saved = [], []
    with no_host_sync():                                                      # nothing in this loop reads the device
        for epoch in range(5):
            for _ in range(2):
                tr.replay(bx, by)
            reports.append(ev.replay())
            saved.append({k: v.clone() for k, v in ev._live.items()})
    hits = [int(r["hits"]) for r in reports]
    print("hits per epoch:", hits)
    best = max(range(5), key=lambda i: (hits[i], -i))                         # the first epoch wins among equals
    assert [int(r["improved"]) for r in reports] == [int(hits[i] > max(hits[:i], default=-1)) for i in range(5)]
    assert all(torch.equal(bits(ev._shadow[k]), bits(saved[best][k])) for k in saved[best])
    assert int(reports[-1]["best_pass"]) == best + 1 and float(reports[-1]["best_accuracy"]) == hits[best] / 26
    live = {k: v.clone() for k, v in ev._live.items()}
    with ev.best_weights():
        assert all(torch.equal(bits(ev._live[k]), bits(saved[best][k])) for k in live)
        with pytest.raises(RuntimeError, match="best_weights"):
            ev.replay()
    assert all(torch.equal(bits(ev._live[k]), bits(live[k])) for k in live)
    sd = ev.state_dict()
    assert all(torch.equal(sd["shadow"][k], saved[best][k].cpu()) for k in live) and sd["best"].tolist() == ev.best.cpu().tolist()
    ev.check()


def test_source_side_and_the_vote_from_confusion():
    a, args, ts = toy()
    b, _, _ = toy()
    b.step(*args, epoch=0, t_samples=ts)                                      # a second model: one train step away
    x_t, y_t, x_s, y_s = args
    cfg = a.cfg
    # the source side, through dimunif, with a tail
    sx, sy = series(2 * 4 + 1, x_s.size(2), cfg.n_class_s, 4, channels=x_s.size(1))
    sdata = fst.DeviceDataset(sx, sy, DEV)
    ev_s = a.make_evaluator("source", sdata, 4, keep_logits=True)
    ev_s.capture()
    rep = ev_s.replay()
    want = by_hand((a.m["fe_s"], a.m["clf_s"]), sdata, 4, trans=a.m["dimunif"].eval())
    a.m["dimunif"].train()
    assert torch.equal(bits(rep["logits"]), bits(want)) and int(rep["seen"]) == 9
    ev_s.check()
    # K = 2 target-side models vote: weights from the train set's confusion matrices, scores from the test set's kept logits
    trx, try_ = series(8, x_t.size(2), cfg.n_class_t, 5, channels=x_t.size(1))
    tex, tey = series(8, x_t.size(2), cfg.n_class_t, 6, channels=x_t.size(1))
    train, test = fst.DeviceDataset(trx, try_, DEV), fst.DeviceDataset(tex, tey, DEV)
    cms, logits = [], []
    for tr in (a, b):
        cms.append(tr.make_evaluator("target", train, 4).run()["confusion"])
        ev = tr.make_evaluator("target", test, 4, keep_logits=True)
        ev.capture()
        logits.append(ev.replay()["logits"])
    w = voting.precision_weights_from_confusion(torch.stack(cms))
    scores = voting.vote_scores(torch.stack(logits), w)
    models = [(tr.m["fe_t"].eval(), tr.m["clf_t"].eval()) for tr in (a, b)]
    tr_logits, tr_labels = voting.collect_logits(models, train.batches(4))
    te_logits, te_labels = voting.collect_logits(models, test.batches(4))
    w_ref, scores_ref, pred_ref, _ = voting.multi_source_vote(tr_logits, tr_labels, te_logits, te_labels)
    assert torch.equal(torch.stack(logits), te_logits) and not torch.equal(logits[0], logits[1])
    assert torch.equal(w, w_ref) and torch.equal(scores, scores_ref) and torch.equal(scores.argmax(1), pred_ref)
