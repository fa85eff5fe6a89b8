"""Gradient accumulation on the device (``fst_accum_multi`` in csrc/guard.hip, ``optim.GradAccumulation`` / ``accumulate``, the
trainers' ``enable_grad_accumulation``): one optimiser step over a window of k calls whose position is a device word.  Needs an
MI355X.

The definition is sequential fp32 in call order — one IEEE addition per fold, one multiplication by float32(1/k) on the closing
call — so torch on the CPU reproduces it bit for bit and no test below has a measured tolerance: the kernel tests compare bits
(NaN against NaN), the trainer tests follow ``same_step`` of test_gpu_anomaly_guard.py (bits in the default arithmetic; under
FST_MATH=f32 the joint reports at its 1e-5 and no state, since RandomLayer's K-split GEMM adds with float atomics there).  Every
buffer of the kernel tests, the state words included, lies between canary bands (``placed``)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import _lib, ops
from feature_level_style_transfer_for_tsc_amd.optim import GradAccumulation, accumulate
from test_gpu_anomaly_guard import NAN, INF, counts_of, follow_host_counters, placed, poisoned, same_step, unchanged
from test_gpu_dist import _build_small_trainer, _collect, _global_data, _guarded
from test_gpu_phase_graphs import batch_b, clone, toy
from test_gpu_schedules import assert_bands_untouched

DEV = "cuda"
KS = (1, 2, 3, 5)
SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 1025, 64 * 256 * 4 + 1)                # the last: past 64 workgroups x 256 quads, into the grid stride
OFFSETS = ((0, 0), (1, 1), (0, 2), (3, 1), (2, 0), (3, 3))                    # (acc, g) floats behind a 16-byte boundary; (0, 0) goes in quads


def inv_of(k):
    return np.float32(1.0) / np.float32(k)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    """Bit equality, a NaN equal to any NaN (IEEE leaves the payload of a produced NaN open)."""
    a, b = a.cpu(), b.cpu()
    return bool(((bits(a) == bits(b)) | (torch.isnan(a) & torch.isnan(b))).all())


class Window:
    """The eight state words between canary bands, set from the host."""

    def __init__(self, k, j=0, windows=0):
        self.buf, (v,) = placed([(8, 0)])
        self.view, self.words = v, v.view(torch.int32)
        self.set(k, j, windows)

    def set(self, k, j=0, windows=0):
        host = torch.zeros(8, dtype=torch.int32)
        host[0], host[1], host[3] = k, j, windows
        host[2:3] = torch.tensor([inv_of(k)]).view(torch.int32)
        self.words.copy_(host)

    def get(self):
        assert_bands_untouched(self.buf, [[self.view]], "the state words")
        w = self.words.tolist()
        assert w[4:] == [0, 0, 0, 0]
        return w[0], w[1], w[3]


def raw_fold(acc, gs, words, advance, numel=None, ptrs=None):
    n = len(acc)
    A, B = ptrs if ptrs is not None else ([t.data_ptr() for t in acc], [t.data_ptr() for t in gs])
    ne = numel if numel is not None else [t.numel() for t in acc]
    return _lib.load().fst_accum_multi((ctypes.c_void_p * n)(*A), (ctypes.c_void_p * n)(*B), (ctypes.c_int64 * n)(*ne), n,
                                       words.data_ptr(), int(advance), _lib.stream_ptr())


class Recurrence:
    """The definition on the CPU in torch fp32: ``fold(gs)`` returns what the gradients hold after the call."""

    def __init__(self, k):
        self.k, self.j, self.acc, self.inv = k, 0, None, torch.tensor(inv_of(k))

    def fold(self, gs):
        gs = [g.detach().cpu().clone() for g in gs]
        if self.k == 1:
            return gs
        self.acc = gs if self.j == 0 else [a + g for a, g in zip(self.acc, gs)]
        closing = self.j + 1 >= self.k
        self.j = 0 if closing else self.j + 1
        return [a * self.inv for a in self.acc] if closing else gs


# ---------------------------------------------------------------------------------------------- 1. the fold, every size and offset
@pytest.mark.parametrize("k", KS)
def test_fold_equals_the_cpu_recurrence_bit_for_bit(k):
    entries = [(n, o) for n in SIZES for pair in OFFSETS for o in pair]       # acc, g, acc, g, ...
    buf, views = placed(entries)
    acc, gs = views[0::2], views[1::2]
    assert len(acc) == 60 and acc[1].data_ptr() % 16 == 4 and gs[2].data_ptr() % 16 == 8 and acc[0].data_ptr() % 16 == gs[0].data_ptr() % 16 == 0
    for a in acc:
        a.fill_(NAN)                                                          # what a window's first fold must not read
    st, ref, gen = Window(k), Recurrence(k), torch.Generator().manual_seed(k)
    for call in range(2 * k):
        j = call % k
        host = [torch.randn(g.numel(), generator=gen) * 10.0 ** (j - 1) for g in gs]
        for g, h in zip(gs, host):
            g.copy_(h)
        acc_before = [a.clone() for a in acc]
        assert raw_fold(acc, gs, st.words, True) == 0, _lib.load().fst_last_error()
        torch.cuda.synchronize()
        assert_bands_untouched(buf, [views], f"k {k}, call {call}")
        assert st.get() == (k, (j + 1) % k, (call + 1) // k), f"k {k}, call {call}: the state words"
        want = ref.fold(host)
        for i, (g, w) in enumerate(zip(gs, want)):
            assert torch.equal(bits(g.cpu()), bits(w)), f"k {k}, call {call}, pair {i} ({entries[2 * i]}, {entries[2 * i + 1]}): gradient"
        if k == 1:
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(acc, acc_before)), "k = 1 touches no accumulator"
        else:
            for i, (a, w) in enumerate(zip(acc, ref.acc)):
                assert torch.equal(bits(a.cpu()), bits(w)), f"k {k}, call {call}, pair {i}: accumulator"


# ---------------------------------------------------------------------------------------------- 2. one position for a whole call series
def test_130_pairs_in_three_launches_share_one_position():
    n = 130
    entries = [(1 + (7 * i) % 23, (i + s) % 4) for i in range(n) for s in (0, 1)]
    buf, views = placed(entries)
    acc, gs = views[0::2], views[1::2]
    st, ref, gen = Window(2), Recurrence(2), torch.Generator().manual_seed(2)
    for call in range(4):
        host = [torch.randn(g.numel(), generator=gen) for g in gs]
        for g, h in zip(gs, host):
            g.copy_(h)
        if call < 2:                                                          # one call: three launches and the advance behind them
            assert raw_fold(acc, gs, st.words, True) == 0
        else:                                                                 # three calls: only the last one moves the window on
            for lo, hi in ((0, 64), (64, 128), (128, n)):
                assert raw_fold(acc[lo:hi], gs[lo:hi], st.words, hi == n) == 0
        torch.cuda.synchronize()
        assert_bands_untouched(buf, [views], f"call {call}")
        assert st.get() == (2, (call + 1) % 2, (call + 1) // 2)
        want = ref.fold(host)
        assert all(torch.equal(bits(g.cpu()), bits(w)) for g, w in zip(gs, want)), f"call {call}: a pair folded at another position"
        assert all(torch.equal(bits(a.cpu()), bits(w)) for a, w in zip(acc, ref.acc)), f"call {call}: accumulators"
    assert raw_fold([], [], st.words, True) == 0                              # no tensors: the advance alone
    torch.cuda.synchronize()
    assert st.get() == (2, 1, 2)


# ---------------------------------------------------------------------------------------------- 3. non-finite values
@pytest.mark.parametrize("bad_call", [0, 1, 2])
def test_non_finite_values_reach_the_closing_gradient(bad_call):
    n, k = 1025, 3
    buf, views = placed([(n, 0), (n, 0), (n, 1), (n, 3)])
    acc, gs = views[0::2], views[1::2]
    st, ref, gen = Window(k), Recurrence(k), torch.Generator().manual_seed(3)
    for call in range(k):
        host = [torch.randn(n, generator=gen) for _ in gs]
        for h in host:
            if call == bad_call:
                h[0], h[1], h[5], h[1023], h[1024] = NAN, INF, -INF, INF, NAN
            elif call == (bad_call + 1) % k:
                h[5], h[1023] = INF, INF                                      # inf + (-inf) at 5, inf + inf at 1023
        for g, h in zip(gs, host):
            g.copy_(h)
        assert raw_fold(acc, gs, st.words, True) == 0
        want = ref.fold(host)
    torch.cuda.synchronize()
    assert_bands_untouched(buf, [views], "non-finite values")
    for g, w in zip(gs, want):
        assert same_bits(g, w)
        got = g.cpu()
        assert bool(torch.isnan(got[[0, 5, 1024]]).all()) and float(got[1]) == INF and float(got[1023]) == INF
        assert int((~torch.isfinite(got)).sum()) == 5, "a non-finite value spread"


# ---------------------------------------------------------------------------------------------- 4. refusals
BAD = [("null accumulator", lambda A, B, ne, i: A.__setitem__(i, None)), ("null gradient", lambda A, B, ne, i: B.__setitem__(i, None)),
       ("misaligned accumulator", lambda A, B, ne, i: A.__setitem__(i, A[i] + 2)), ("overlap", lambda A, B, ne, i: B.__setitem__(i, A[i] + 4)),
       ("no elements", lambda A, B, ne, i: ne.__setitem__(i, 0)), ("2^31 elements", lambda A, B, ne, i: ne.__setitem__(i, 2 ** 31))]


@pytest.mark.parametrize("at", [0, 64, 129], ids=["first", "middle", "last"])
def test_a_bad_entry_is_refused_before_the_first_launch(at):
    n = 130
    buf, views = placed([(9, i % 4) for i in range(2 * n)])
    acc, gs = views[0::2], views[1::2]
    for v in views:
        v.copy_(torch.randn(9))
    st = Window(2, 1, 7)
    before = buf.clone()
    for what, spoil in BAD:
        A, B, ne = [t.data_ptr() for t in acc], [t.data_ptr() for t in gs], [9] * n
        spoil(A, B, ne, at)
        assert raw_fold(acc, gs, st.words, True, numel=ne, ptrs=(A, B)) == -1, what
        assert f"tensor {at}:".encode() in _lib.load().fst_last_error(), what
    for words in (None, st.words[1:]):                                        # a null state block; one off its 16-byte boundary
        rc = _lib.load().fst_accum_multi((ctypes.c_void_p * n)(*[t.data_ptr() for t in acc]), (ctypes.c_void_p * n)(*[t.data_ptr() for t in gs]),
                                         (ctypes.c_int64 * n)(*[9] * n), n, None if words is None else words.data_ptr(), 1, _lib.stream_ptr())
        assert rc == -1 and b"state" in _lib.load().fst_last_error()
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), bits(before)) and st.get() == (2, 1, 7), "a refused call wrote something"


# ---------------------------------------------------------------------------------------------- 5. under graph replay
def test_captured_fold_serves_every_position_and_follows_set_steps():
    sizes = [(1025, 0), (1025, 0), (65, 1), (65, 2), (4, 0), (4, 0)]
    buf, views = placed(sizes)
    acc, gs = views[0::2], views[1::2]
    scal_acc, scal = torch.empty(10, device=DEV), torch.empty(10, device=DEV)
    st = GradAccumulation(DEV, 2)
    gen = torch.Generator().manual_seed(5)
    fresh = lambda: [torch.randn(g.numel(), generator=gen) for g in gs + [scal]]
    for g, h in zip(gs + [scal], fresh()):
        g.copy_(h)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                             # one eager window (loads the code object)
        for _ in range(2):
            accumulate(acc, gs, st, advance=False)
            accumulate([scal_acc], [scal], st)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert st.pending == 0 and st.words.tolist()[:4] == [2, 0, int(torch.tensor([0.5]).view(torch.int32)), 1]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        accumulate(acc, gs, st, advance=False)                                # as a step does: the gradients, then later the scalars
        accumulate([scal_acc], [scal], st)
    assert st.pending == 0, "a captured launch has not run: the mirror stays"
    windows = 1
    for k in (2, 2, 3):                                                       # two windows of two; then three, steered between windows
        if k != st.steps_host:
            assert st.set_steps(k) is True
        ref = Recurrence(k)
        for j in range(k):
            host = fresh()
            for g, h in zip(gs + [scal], host):
                g.copy_(h)
            graph.replay()
            st.advance_host()
            if j < k - 1:
                with pytest.raises(RuntimeError, match="window is open"):
                    st.set_steps(7)
            torch.cuda.synchronize()
            want = ref.fold(host)
            assert_bands_untouched(buf, [views], f"k {k}, replay {j}")
            assert all(torch.equal(bits(g.cpu()), bits(w)) for g, w in zip(gs + [scal], want)), f"k {k}, replay {j}"
            assert all(torch.equal(bits(a.cpu()), bits(w)) for a, w in zip(acc + [scal_acc], ref.acc)), f"k {k}, replay {j}: accumulators"
            windows += (j + 1) // k
            assert st.words.tolist()[:4] == [k, (j + 1) % k, int(torch.tensor([inv_of(k)]).view(torch.int32)), windows] and st.pending == (j + 1) % k


# ---------------------------------------------------------------------------------------------- the trainers, toy fixture
def live(tr):
    """A copy of every state tensor (``snapshot`` refuses while a window is open)."""
    return {k: v.detach().clone() for k, v in tr._state_tensors().items()}


def steady(before, after, what, opening):
    """After a call that does not close its window: optimiser moments, GradNorm weights, averages and parameters keep their bits
    (``opening``, against the state before the window: but for the omni-scale conv weights, whose masked taps, moved by the last
    update, the first forward zeroes again: Q1)."""
    moved = [n for n, v in before.items() if not torch.equal(after[n], v) and
             (n.startswith(("o.", "w_", "ema.")) or (n.startswith("m.") and not n.endswith(("running_mean", "running_var", "num_batches_tracked"))
                                                      and not (opening and n.endswith("conv1d.weight"))))]
    assert not moved, f"{what}: a call inside a window moved {len(moved)} tensors, e.g. {moved[:5]}"


def micro_batches(args, k):
    out = [args, batch_b(args)]
    gen = torch.Generator().manual_seed(123)
    while len(out) < k:
        out.append([torch.randn(args[0].shape, generator=gen).to(DEV), args[1].roll(1).contiguous(),
                    torch.randn(args[2].shape, generator=gen).to(DEV), args[3].flip(0).contiguous()])
    return out[:k]


def composed_window(twin, batches, ts, k):
    """The window on a trainer WITHOUT the mode, from its own parts: ``_step_part_a`` per micro-batch, the fold in CPU torch fp32
    on copies of ``.grad``, of ``scal`` and of the losses, the means written back, then ``_step_part_b``."""
    ref = Recurrence(k)
    for b in batches:
        twin._set_epoch(0)
        ratios = twin.m["noise"].advance(b[0].size(0), b[2].size(0))
        mid = twin._step_part_a(*b, 0, ts, ratios)
        gs = [p.grad for p in twin.parameters() if p.grad is not None] + [mid["scal"]]
        losses = torch.stack([mid["report"][n] for n in mid["loss_keys"]])
        means = ref.fold(gs + [losses])
    for g, m in zip(gs, means):
        g.copy_(m)
    return twin._step_part_b(mid), means[-1]


def test_one_step_per_window_is_the_mode_off():
    on, args, ts = toy()
    off, _, _ = toy()
    on.enable_grad_accumulation()
    on.enable_grad_accumulation(4)                                            # idempotent
    assert on.grad_accumulation.steps_host == 1 and off.grad_accumulation is None and off.accum_pending == 0
    batches = micro_batches(args, 3)
    for i, b in enumerate(batches):
        ra, rb = on.step(*b, epoch=0, t_samples=ts), off.step(*b, epoch=0, t_samples=ts)
        assert int(ra["accum_index"]) == 0 and on.accum_pending == 0 and "accum_index" not in rb
        same_step(ra, rb, on.snapshot()["t"], off.snapshot()["t"], f"eager step {i}")
        assert same_bits(ra["window_losses"], torch.stack([rb[n] for n in ("nf_t", "nf_s", "ce_t", "sl_t", "ce_s", "sl_s", "cdan", "ce_s2t2s", "fd_s")]))
    for tr in (on, off):
        torch.manual_seed(4)
        tr.capture(*args, epoch=0)
    assert len(on._graphs) == 2 and len(off._graphs) == 1
    with pytest.raises(RuntimeError, match="capture is resident"):
        off.enable_grad_accumulation()
    on.restore(off.snapshot())
    for i, b in enumerate(batches):
        ra, rb = clone(on.replay(*b, ts)), clone(off.replay(*b, ts))
        same_step(ra, rb, on.snapshot()["t"], off.snapshot()["t"], f"replay {i}")
    assert int(on.grad_accumulation.windows) >= 6


@pytest.mark.parametrize("k", [2, 3])
def test_a_window_is_the_composition_of_its_parts(k):
    tr, args, ts = toy()
    twin, _, _ = toy()
    tr.enable_grad_accumulation(k)
    tr.enable_grad_clip()
    twin.enable_grad_clip()
    batches = micro_batches(args, k)
    for window in range(2):
        before = live(tr)
        for j, b in enumerate(batches):
            rep = tr.step(*b, epoch=0, t_samples=ts)
            assert int(rep["accum_index"]) == (j + 1) % k == tr.accum_pending
            if j < k - 1:
                assert "w_t" not in rep and "grad_l2" not in rep and "window_losses" not in rep and "nf_t" in rep and "logit_t" in rep
                now = live(tr)
                steady(before if j == 0 else prev, now, f"k {k}, window {window}, call {j}", j == 0)
                prev = now
        want, want_losses = composed_window(twin, batches, ts, k)
        same_step(rep, want, tr.snapshot()["t"], twin.snapshot()["t"], f"k {k}, window {window}")
        assert torch.equal(bits(rep["window_losses"].cpu()), bits(want_losses)), "window_losses are the folded means"
        batches = batches[::-1]
    assert int(tr.grad_accumulation.windows) == 2


def test_replay_equals_eager_and_follows_set_grad_accumulation():
    tr, args, ts = toy()
    tr.enable_grad_accumulation(2)
    tr.enable_weight_average()
    torch.manual_seed(4)
    tr.capture(*args, epoch=0)                                                # warm-up: whole windows
    assert tr.accum_pending == 0 and len(tr._graphs) == 2
    with pytest.raises(RuntimeError, match="capture is resident"):
        tr.enable_anomaly_guard()
    snap = tr.snapshot()
    n0 = int(snap["t"]["ema.count"][0])
    assert n0 == 6, "a warm-up of 11 is rounded up to 6 whole windows, each one update"
    batches = micro_batches(args, 3)

    def windows(run, ks):
        tr.restore(snap)
        reps = []
        for k in ks:
            tr.set_grad_accumulation(k)
            for j, b in enumerate(batches[:k]):
                rep = clone(run(b))
                assert int(rep["accum_index"]) == (j + 1) % k == tr.accum_pending
                assert ("w_t" in rep) == (j == k - 1)
                if j < k - 1:
                    with pytest.raises(RuntimeError, match="window is open"):
                        tr.set_grad_accumulation(5)
            reps.append(rep)
        return reps, tr.snapshot()["t"]

    ks = (2, 2, 3)
    graph_reps, graph_state = windows(lambda b: tr.replay(*b, ts), ks)
    eager_reps, eager_state = windows(lambda b: tr.step(*b, epoch=0, t_samples=ts), ks)
    for i, (ra, rb) in enumerate(zip(graph_reps, eager_reps)):
        same_step(ra, rb, graph_state, eager_state, f"window {i} of {ks}")
    assert graph_reps[-1]["ema_steps"].tolist()[0] == n0 + 3, "the average moves once per window"
    tr.set_grad_accumulation(2)


@pytest.mark.parametrize("replayed", [False, True], ids=["eager", "replayed"])
def test_a_window_with_a_bad_micro_batch_is_skipped_as_a_whole(replayed):
    tr, args, ts = toy()
    twin, _, _ = toy()
    for t in (tr, twin):
        t.enable_anomaly_guard()
        t.enable_grad_accumulation(2)
        if replayed:
            torch.manual_seed(4)
            t.capture(*args, epoch=0)
        else:
            for b in micro_batches(args, 2):
                t.step(*b, epoch=0, t_samples=ts)
    run = (lambda t, b: clone(t.replay(*b, ts))) if replayed else (lambda t, b: t.step(*b, epoch=0, t_samples=ts))
    twin.restore(tr.snapshot())
    before = tr.snapshot()
    skipped = int(tr.skipped_steps)
    good = micro_batches(args, 2)
    rep = run(tr, poisoned(args, 0, NAN))                                     # micro-batch 0 of the window is the bad one
    assert "skipped" not in rep and tr.accum_pending == 1
    rep = run(tr, good[1])
    assert int(rep["skipped"]) == 1 and counts_of(rep)["fe_t"] > 0 and int(tr.skipped_steps) == skipped + 1
    assert tr.accum_pending == 0 and int(rep["accum_index"]) == 0, "a skipped window still closes"
    unchanged(before["t"], tr.snapshot()["t"], "a window with a NaN micro-batch")
    for b in good:                                                            # the calls of the skipped window were counted
        follow_host_counters(twin, tr, b)
    for b in good[::-1]:
        ra, rb = run(tr, b), run(twin, b)
    assert int(ra["skipped"]) == 0
    same_step(ra, rb, tr.snapshot()["t"], twin.snapshot()["t"], "the window after a skipped one")


def test_clip_and_average_see_the_window_mean():
    tr, args, ts = toy()
    tr.enable_grad_accumulation(2)
    tr.enable_grad_clip(max_norm=1e-3)
    tr.enable_weight_average()
    seen = {}

    def hook():
        gs = [p.grad.double() for k in tr.MODULES for p in tr.m[k].parameters() if p.grad is not None]
        seen["l2"] = float(torch.sqrt(sum((g * g).sum() for g in gs)))
        seen["calls"] = seen.get("calls", 0) + 1
    tr.on_grads_ready = hook
    for window in range(2):
        for j, b in enumerate(micro_batches(args, 2)):
            rep = tr.step(*b, epoch=0, t_samples=ts)
            assert seen.get("calls", 0) == window + j, "on_grads_ready fires on the closing call only"
            assert ("grad_l2" in rep) == ("ema_steps" in rep) == ("clip_coef" in rep) == (j == 1)
        total = float(rep["grad_l2"][-1])
        assert abs(total - seen["l2"]) <= 1e-5 * seen["l2"], (total, seen["l2"])   # an fp32 norm of fp32 sums against fp64: rounding room
        assert rep["ema_steps"].tolist() == [window + 1] * len(tr.MODULES)
        assert float(rep["clip_coef"].max()) < 1.0, "the window mean is what gets clipped"


def test_classifier_trainer_window():
    gen = torch.Generator().manual_seed(7)
    mk = lambda: (torch.randn(8, 1, 64, generator=gen).to(DEV), torch.randint(3, (8,), generator=gen).to(DEV))
    batches = [mk() for _ in range(4)]
    torch.manual_seed(5)
    twin = fst.ClassifierTrainer(64, 1, 3, DEV)
    tr = fst.ClassifierTrainer(64, 1, 3, DEV, grad_accumulation=2)
    tr.fe.load_state_dict(twin.fe.state_dict()); tr.clf.load_state_dict(twin.clf.state_dict())

    def state(t):
        out = dict(("fe." + k, v.clone()) for k, v in t.fe.state_dict().items())
        out.update(("clf." + k, v.clone()) for k, v in t.clf.state_dict().items())
        for name, o in (("opt_fe", t.opt_fe), ("opt_clf", t.opt_clf)):
            for i, p in enumerate(o.param_groups[0]["params"]):
                if "square_avg" in o.state[p]:
                    out[f"{name}.{i}"] = o.state[p]["square_avg"].clone()
        return out

    def composed(pair):
        ref = Recurrence(2)
        for x, y in pair:
            twin.opt_fe.zero_grad(set_to_none=True); twin.opt_clf.zero_grad(set_to_none=True)
            twin._fwd_bwd(x, y)
            gs = [p.grad for p in twin.parameters() if p.grad is not None]
            means = ref.fold(gs)
        for g, m in zip(gs, means):
            g.copy_(m)
        twin._update()

    def check(run, pair, what):
        inside = None
        for j, (x, y) in enumerate(pair):
            loss, logits = run(x, y)
            assert tr.accum_pending == (j + 1) % 2
            if j == 0:
                inside = state(tr)
        composed(pair)
        sa, sb = state(tr), state(twin)
        differing = [k for k in sb if not torch.equal(sa[k], sb[k])]
        assert set(sa) == set(sb) and not differing, f"{what}: {differing[:5]}"
        return inside

    start = state(tr)
    inside = check(tr.step, batches[:2], "eager window")
    assert all(torch.equal(inside[k], v) for k, v in start.items()
               if "running" not in k and "num_batches" not in k and not k.endswith("conv1d.weight")), "a call inside a window updated"   # (Q1: the forward masks taps)
    tr.capture(*batches[2], warmup=3)                                         # rounded up to two whole windows
    assert tr.accum_pending == 0 and tr._graph_update is not None
    composed([batches[2]] * 2); composed([batches[2]] * 2)                    # the twin follows the warm-up
    sa, sb = state(tr), state(twin)
    assert not [k for k in sb if not torch.equal(sa[k], sb[k])], "the capture's warm-up is two whole windows"
    check(tr.replay, batches[2:], "replayed window")
    assert tr.set_grad_accumulation(1) is True
    tr.replay(*batches[0])
    twin.opt_fe.zero_grad(set_to_none=True); twin.opt_clf.zero_grad(set_to_none=True)
    twin._fwd_bwd(*batches[0]); twin._update()
    sa, sb = state(tr), state(twin)
    assert not [k for k in sb if not torch.equal(sa[k], sb[k])], "one step per window, set under the resident capture"


@pytest.mark.parametrize("phase", ["ssl_with_ce", "nf"])
def test_phase_step_window(phase):
    tr, args, ts = toy()
    twin, _, _ = toy()
    tr.enable_grad_accumulation(2)
    batches = micro_batches(args, 2)
    for window in range(2):
        for j, b in enumerate(batches):
            rep = tr.phase_step(phase, *b, t_samples=ts)
            assert int(rep["accum_index"]) == (j + 1) % 2 == tr.accum_pending and "total" in rep
        ref = Recurrence(2)
        for b in batches:
            want = twin._phase_fwd_bwd(phase, *b, ts)
            gs = [p.grad for p in twin.parameters() if p.grad is not None]
            means = ref.fold(gs)
        for g, m in zip(gs, means):
            g.copy_(m)
        twin._phase_update(phase)
        same_step(rep, want, tr.snapshot()["t"], twin.snapshot()["t"], f"{phase}, window {window}", joint=False)
    with pytest.raises(RuntimeError, match=r"phase_step\(\)"):
        tr.capture_phase(phase, *args)
    assert tr.captured_phases() == ()
    tr.set_grad_accumulation(1)
    tr.capture_phase(phase, *args)                                            # one step per window: a captured phase is whole
    tr.set_grad_accumulation(2)
    with pytest.raises(RuntimeError, match=r"phase_step\(\)"):
        tr.replay_phase(phase, *args, ts)


def test_checkpoints_between_windows_only(tmp_path):
    tr, args, ts = toy()
    tr.enable_grad_accumulation(2)
    batches = micro_batches(args, 2)
    for b in batches:
        tr.step(*b, epoch=0, t_samples=ts)
    sd = tr.state_dict()
    assert sd["grad_accumulation"] == {"steps": 2}
    tr.step(*batches[0], epoch=0, t_samples=ts)
    for call in (tr.state_dict, tr.snapshot, lambda: tr.save_state(str(tmp_path / "x.pt")), lambda: tr.load_state_dict(sd)):
        with pytest.raises(RuntimeError, match="window is open"):
            call()
    assert not (tmp_path / "x.pt").exists()
    tr.step(*batches[1], epoch=0, t_samples=ts)
    tr.save_state(str(tmp_path / "x.pt"))
    resumed, _, _ = toy()
    resumed.load_state(str(tmp_path / "x.pt"))                                # enables the mode
    assert resumed.grad_accumulation is not None and resumed.grad_accumulation.steps_host == 2 and resumed.accum_pending == 0
    for b in batches[::-1]:
        ra, rb = tr.step(*b, epoch=0, t_samples=ts), resumed.step(*b, epoch=0, t_samples=ts)
    same_step(ra, rb, tr.snapshot()["t"], resumed.snapshot()["t"], "a resumed run")
    tr.set_grad_accumulation(3)
    resumed.load_state_dict(tr.state_dict())                                  # a second load: through set_steps
    assert resumed.grad_accumulation.steps_host == 3 and resumed.grad_accumulation.k.tolist() == [3]


# ---------------------------------------------------------------------------------------------- data parallel: one all-reduce per window
def _worker_bucket(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    bucket = fst.GradBucket(always_reduce=True)
    tr, meta = _build_small_trainer(fst, dev, bucket, "ddp")
    ref, _ = _build_small_trainer(fst, dev, None, "ddp")
    calls = {"begin": 0, "scalars": 0}
    begin, scalars = bucket._begin, bucket.mean_scalars

    def counted_begin(grads):
        calls["begin"] += 1
        return begin(grads)

    def counted_scalars(t):
        calls["scalars"] += 1
        return scalars(t)
    bucket._begin, bucket.mean_scalars = counted_begin, counted_scalars
    (x_t, y_t), (x_s, y_s) = _global_data(meta, meta["B"])
    a = [v.to(dev) for v in (x_t, y_t, x_s, y_s)]
    b = [a[0].flip(0).contiguous(), a[1].flip(0).contiguous(), a[2].flip(0).contiguous(), a[3].flip(0).contiguous()]
    for t in (tr, ref):
        t.enable_grad_accumulation(2)
    out = {}
    for window in range(2):
        for batch in (a, b):
            ra, rb = tr.step(*batch, epoch=0, t_samples=(2, 5)), ref.step(*batch, epoch=0, t_samples=(2, 5))
    out["eager_calls"] = dict(calls)
    sa, sb = tr.snapshot()["t"], ref.snapshot()["t"]
    out["eager_differing"] = [k for k, v in sb.items() if not torch.equal(sa[k], v)][:5] if ops.MATH == "bf16x3" else []
    for t in (tr, ref):
        torch.manual_seed(9)
        t.capture(*a, epoch=0)
    out["graphs"] = (len(tr._graphs), len(ref._graphs))
    tr.restore(ref.snapshot())
    calls.update(begin=0, scalars=0)
    for window in range(2):
        for batch in (a, b):
            ra, rb = tr.replay(*batch, (1, 3)), ref.replay(*batch, (1, 3))
    torch.cuda.synchronize()
    out["replay_calls"] = dict(calls)
    sa, sb = tr.snapshot()["t"], ref.snapshot()["t"]
    out["replay_differing"] = [k for k, v in sb.items() if not torch.equal(sa[k], v)][:5] if ops.MATH == "bf16x3" else []
    out["w_t"] = float(ra["w_t"].sum())
    q.put((0, out))
    dist.destroy_process_group()


def _run_worker(name, rank, world, port, q):
    _guarded(globals()[name])(rank, world, port, q)


def test_the_bucket_reduces_once_per_window_on_one_rccl_rank():
    world, port = 1, 29683
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_run_worker, args=("_worker_bucket", 0, world, port, q))]
    procs[0].start()
    (_, out), = _collect(q, world, procs)
    assert out["eager_calls"] == {"begin": 2, "scalars": 2}, out
    assert out["replay_calls"] == {"begin": 2, "scalars": 2} and out["graphs"] == (3, 2), out
    assert not out["eager_differing"] and not out["replay_differing"] and abs(out["w_t"] - 7.0) < 1e-4, out
