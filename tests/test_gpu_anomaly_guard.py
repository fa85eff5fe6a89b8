"""The anomaly guard on the device (csrc/guard.hip, the ``*_multi_guard`` kernels of csrc/optim.hip, ``JointTrainer.
enable_anomaly_guard``): a step whose update would consume a NaN or an inf is a no-op on the trainer's state, decided without the
host, in eager and in replayed steps; a clean step computes the bits of the unguarded step.  Needs an MI355X.

Every output, slot array and shadow of the kernel tests lies between canary bands (``banded`` / ``assert_bands_untouched`` of
test_gpu_schedules.py; ``placed`` below lays tensors at chosen distances from a 16-byte boundary in the same manner).  Integer
outputs are int32 views of such float buffers.  Expected counts come from ``torch.isfinite`` on the CPU; every state comparison is
bit for bit (``torch.equal``), except under FST_MATH=f32 where the joint step's reports are compared at the 1e-5 of
test_full_batch_graph_replay_equals_eager_step and its state is not compared (RandomLayer's K-split GEMM adds with float atomics
there)."""
import ctypes
import multiprocessing as mp
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import _lib, ops
from feature_level_style_transfer_for_tsc_amd.optim import (AnomalyGuard, FusedRMSprop, SharedStepAdam, count_nonfinite, guard_copy,
                                                            rmsprop_step_many)
from test_gpu_conv_routes import CANARY
from test_gpu_dist import _build_small_trainer, _collect, _guarded
from test_gpu_optim import _grads, _sizes, _start, f32
from test_gpu_phase_graphs import batch_b, clone, fixture, toy
from test_gpu_schedules import BAND, assert_bands_untouched, banded

DEV = "cuda"
NAN, INF, FMAX = float("nan"), float("inf"), float(torch.finfo(torch.float32).max)
BAD = (NAN, INF, -INF)
BENIGN = (-0.0, 1e-40, FMAX, -FMAX)                                          # −0, a denormal, ±3.4028235e38: finite
REC = 65                                                                     # a tensor's record in the slot array: group id, 64 counts
G = fst.JointTrainer.ANOMALY_GROUPS


def placed(entries):
    """(buffer, views): one fp32 tensor per (numel, off) entry in ONE canary-filled buffer, each starting ``off`` floats behind a
    16-byte boundary, at least ``BAND`` canary floats in front of each and behind the last."""
    at, starts = 0, []
    for n, off in entries:
        start = (at + BAND + 3) // 4 * 4 + off
        starts.append(start)
        at = start + n
    buf = torch.full((at + BAND,), CANARY, device=DEV, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    views = [buf[s: s + n] for s, (n, _) in zip(starts, entries)]
    assert all(v.data_ptr() % 16 == 4 * off for v, (_, off) in zip(views, entries))
    return buf, views


class Words:
    """slots, counts[32], verdict, ok, skipped of one scan between canary bands."""

    def __init__(self, n_tensors):
        self.n_slots = int(_lib.load().fst_nonfinite_slots(n_tensors))
        assert self.n_slots == REC * n_tensors
        self.buf, (v,) = banded([max(self.n_slots, 1), 32, 1, 1, 1], 1)
        self.views = v
        self.slots, self.counts, self.verdict, self.skipped = (v[i].view(torch.int32) for i in (0, 1, 2, 4))
        self.ok = v[3]
        self.skipped.zero_()

    def scan(self, tensors, groups, mask=-1):
        lib = _lib.load()
        n = len(tensors)
        _lib.check(lib.fst_nonfinite_multi((ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors]),
                                           (ctypes.c_int64 * n)(*[t.numel() for t in tensors]), (ctypes.c_int32 * n)(*groups), n, mask,
                                           self.slots.data_ptr(), self.n_slots, self.counts.data_ptr(), self.verdict.data_ptr(),
                                           self.ok.data_ptr(), self.skipped.data_ptr(), _lib.stream_ptr()), "fst_nonfinite_multi")
        torch.cuda.synchronize()
        assert_bands_untouched(self.buf, [self.views], "the scan's slots and words")
        return self.counts.tolist(), int(self.verdict), float(self.ok), int(self.skipped)


def want_counts(tensors, groups):
    want = [0] * 32
    for t, g in zip(tensors, groups):
        want[g] += int((~torch.isfinite(t.cpu())).sum())
    return want


# ---------------------------------------------------------------------------------------------- 1. the scan
SCAN_SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1025, 65_537)                  # 65 537: past 64 workgroups x 1024 into the grid stride


def _plant(host, i):
    """Index 0 and the last; 3 and 4 (the head boundary at every start offset); 255, 256, 1023, 1024; the last three (the tail)."""
    n = host.numel()
    values = BAD + BENIGN
    for j, at in enumerate(sorted({p for p in (0, 3, 4, 255, 256, 1023, 1024, n - 3, n - 2, n - 1) if 0 <= p < n})):
        host[at] = values[(i + j) % len(values)]


def test_scan_edges_every_size_at_every_start_offset():
    entries = [(n, off) for n in SCAN_SIZES for off in range(4)]
    buf, views = placed(entries)
    gen = torch.Generator().manual_seed(5)
    hosts = []
    for i, v in enumerate(views):
        hosts.append(torch.randn(v.numel(), generator=gen))
        _plant(hosts[-1], i)
        v.copy_(hosts[-1])
    for p in (0, 3, 4, 255, 256, 1023, 1024, -1, -2, -3):                      # each place holds a bad and a benign value somewhere
        at = [bool(torch.isfinite(h[p])) for h in hosts if h.numel() > max(p, 5)]
        assert any(at) and not all(at), p
    before = buf.view(torch.int32).clone()
    w = Words(len(views))
    groups = [i % 5 for i in range(len(views))]
    counts, verdict, ok, skipped = w.scan(views, groups)                       # ONE call: 40 tensors, five groups
    assert counts == want_counts(views, groups) and sum(counts) > 40
    assert (verdict, ok, skipped) == (1, 0.0, 1)
    for lo in range(0, len(views), 20):                                        # and every tensor as a group of its own
        part = views[lo: lo + 20]
        counts, *_ = w.scan(part, list(range(len(part))))
        assert counts == want_counts(part, list(range(len(part)))), f"tensors {lo}..{lo + 19}: {entries[lo: lo + 20]}"
    assert torch.equal(buf.view(torch.int32), before), "the scan wrote into its inputs or their bands"
    # the Python entry point on the same views
    assert count_nonfinite(views, groups, 5).tolist() == want_counts(views, groups)[:5]


def test_scan_of_65_tensors_crosses_the_chunk():
    sizes = _sizes("65")
    buf, (views,) = banded(sizes, 1)
    gen = torch.Generator().manual_seed(6)
    for i, v in enumerate(views):
        host = torch.randn(v.numel(), generator=gen)
        host[(i * 37 + 11) % v.numel()] = BAD[i % 3]                          # exactly one plant per tensor, at another place each
        v.copy_(host)
    groups = [i % 3 for i in range(65)]
    w = Words(65)
    counts, verdict, ok, skipped = w.scan(views, groups)
    assert counts == [22, 22, 21] + [0] * 29
    rec = w.slots[: 65 * REC].view(65, REC).cpu()
    assert rec[:, 0].tolist() == groups and rec[:, 1:].sum(dim=1).tolist() == [1] * 65, "every tensor contributes exactly 1"
    assert (verdict, ok, skipped) == (1, 0.0, 1)
    assert_bands_untouched(buf, [views], "the scanned tensors")
    # a group outside the verdict mask is counted and does not decide
    counts, verdict, ok, skipped = w.scan(views[:2], [0, 1], mask=0b100)
    assert counts[:3] == [1, 1, 0] and (verdict, ok, skipped) == (0, 1.0, 1)


def test_clean_data_is_a_clean_verdict_and_bad_calls_are_counted():
    buf, views = placed([(n, off) for n, off in ((1, 1), (257, 3), (70_000, 2))])
    gen = torch.Generator().manual_seed(8)
    for i, v in enumerate(views):
        host = torch.randn(v.numel(), generator=gen)
        host[0], host[-1] = BENIGN[i], BENIGN[i + 1]
        v.copy_(host)
    w = Words(3)
    w.skipped.fill_(5)
    assert w.scan(views, [0, 1, 2]) == ([0] * 32, 0, 1.0, 5)
    views[2][69_999] = -INF
    assert w.scan(views, [0, 1, 2])[1:] == (1, 0.0, 6)
    assert w.scan(views, [0, 1, 2])[1:] == (1, 0.0, 7)
    views[2][69_999] = 0.0
    assert w.scan(views, [0, 1, 2]) == ([0] * 32, 0, 1.0, 7)
    # the guard object: same words through the Python entry point
    guard = AnomalyGuard(DEV)
    assert count_nonfinite(views, [0, 1, 2], 3, guard).tolist() == [0, 0, 0]
    assert (int(guard.verdict), float(guard.ok), int(guard.skipped)) == (0, 1.0, 0)


def test_scan_refuses_a_bad_entry_before_the_first_launch():
    buf, (views,) = banded([4] * 66, 1)
    w = Words(66)
    w.counts.fill_(7)
    lib = _lib.load()
    groups = [0] * 65 + [32]                                                  # the bad entry is in the second chunk
    rc = lib.fst_nonfinite_multi((ctypes.c_void_p * 66)(*[t.data_ptr() for t in views]), (ctypes.c_int64 * 66)(*[4] * 66),
                                 (ctypes.c_int32 * 66)(*groups), 66, -1, w.slots.data_ptr(), w.n_slots, w.counts.data_ptr(),
                                 w.verdict.data_ptr(), w.ok.data_ptr(), w.skipped.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and w.counts.tolist() == [7] * 32 and int(w.skipped) == 0
    assert bool((w.views[0] == CANARY).all()), "a refused call wrote slots"


# ---------------------------------------------------------------------------------------------- 2. the guarded optimisers
def _banded_guard(verdict):
    buf, (v,) = banded([1, 1], 1)
    guard = AnomalyGuard(DEV)
    guard.verdict, guard.ok = v[0].view(torch.int32), v[1][0]
    guard.verdict.fill_(verdict); guard.ok.fill_(1.0 - verdict)
    return guard, (buf, [v])


@pytest.mark.parametrize("on_device", [False, True], ids=["lr_by_value", "lr_on_device"])
@pytest.mark.parametrize("layout", ["one", "65"])
def test_guarded_rmsprop(layout, on_device):
    sizes = _sizes(layout)
    p0 = _start(sizes, 11)
    lrs = [f32(1e-2), f32(3e-2), f32(2e-2)]
    parts = [idx for idx in ([list(range(i, len(sizes), 3)) for i in range(3)] if len(sizes) >= 3 else [[0]]) if idx]
    buf, (pv, vv) = banded(sizes, 2)
    for view, p in zip(pv, p0):
        view.copy_(p)
    dev = [torch.nn.Parameter(v) for v in pv]
    twin = [torch.nn.Parameter(p.clone().to(DEV)) for p in p0]
    g_opts = [FusedRMSprop([dev[i] for i in idx], lr=lr, lr_on_device=on_device) for idx, lr in zip(parts, lrs)]
    t_opts = [FusedRMSprop([twin[i] for i in idx], lr=lr, lr_on_device=on_device) for idx, lr in zip(parts, lrs)]
    for o, idx in zip(g_opts, parts):
        for i in idx:
            o.state[dev[i]]["square_avg"] = vv[i].zero_()
    guard, gband = _banded_guard(0)
    for t in range(1, 4):                                                     # verdict 0: three steps, the unguarded twin's bits
        for pd, pt, g in zip(dev, twin, _grads(sizes, t, 11)):
            pd.grad, pt.grad = g.to(DEV), g.to(DEV)
        rmsprop_step_many(g_opts, guard)
        rmsprop_step_many(t_opts)
    sq = lambda pt: [o for o in t_opts if pt in o.state][0].state[pt]["square_avg"]
    for i, (pd, pt) in enumerate(zip(dev, twin)):
        assert torch.equal(pd, pt) and not torch.equal(pt.detach().cpu(), p0[i]), f"parameter {i} ({sizes[i]} elements)"
        assert torch.equal(vv[i], sq(pt)), f"square_avg {i}"
    guard.verdict.fill_(1); guard.ok.fill_(0.0)                               # verdict 1, NaN in every gradient: nothing moves
    before = buf.view(torch.int32).clone()
    for pd, g in zip(dev, _grads(sizes, 4, 11)):
        g[g.numel() // 2] = NAN
        pd.grad = g.to(DEV)
    rmsprop_step_many(g_opts, guard)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before), "a skipped RMSprop step wrote parameters, moments or bands"
    assert_bands_untouched(buf, (pv, vv), f"guarded RMSprop {layout}")
    assert_bands_untouched(*gband, "the verdict words")


@pytest.mark.parametrize("on_device", [False, True], ids=["lr_by_value", "lr_on_device"])
@pytest.mark.parametrize("layout", ["one", "65"])
def test_guarded_adam(layout, on_device):
    sizes = _sizes(layout)
    p0 = _start(sizes, 7)
    buf, (pv, mv, vv) = banded(sizes, 3)
    for view, p in zip(pv, p0):
        view.copy_(p)
    dev = [torch.nn.Parameter(v) for v in pv]
    twin = [torch.nn.Parameter(p.clone().to(DEV)) for p in p0]
    g_opt = SharedStepAdam(dev, lr=f32(1e-2), lr_on_device=on_device)
    t_opt = SharedStepAdam(twin, lr=f32(1e-2), lr_on_device=on_device)
    for i, pd in enumerate(dev):
        g_opt.state[pd]["exp_avg"], g_opt.state[pd]["exp_avg_sq"] = mv[i].zero_(), vv[i].zero_()
    guard, gband = _banded_guard(0)
    for t in range(1, 4):
        for pd, pt, g in zip(dev, twin, _grads(sizes, t, 7)):
            pd.grad, pt.grad = g.to(DEV), g.to(DEV)
        g_opt.step(guard=guard)
        t_opt.step()
    assert torch.equal(g_opt.param_groups[0]["step"], t_opt.param_groups[0]["step"]) and float(g_opt.param_groups[0]["step"]) == 3.0
    for i, (pd, pt) in enumerate(zip(dev, twin)):
        assert torch.equal(pd, pt) and not torch.equal(pt.detach().cpu(), p0[i]), f"parameter {i} ({sizes[i]} elements)"
        assert torch.equal(mv[i], t_opt.state[pt]["exp_avg"]) and torch.equal(vv[i], t_opt.state[pt]["exp_avg_sq"]), f"moments {i}"
    guard.verdict.fill_(1); guard.ok.fill_(0.0)
    before = buf.view(torch.int32).clone()
    for pd, g in zip(dev, _grads(sizes, 4, 7)):
        g[0] = NAN
        pd.grad = g.to(DEV)
    g_opt.step(guard=guard)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before), "a skipped Adam step wrote parameters, moments or bands"
    assert float(g_opt.param_groups[0]["step"]) == 3.0, "the shared counter advances by ok"
    assert_bands_untouched(buf, (pv, mv, vv), f"guarded Adam {layout}")
    assert_bands_untouched(*gband, "the verdict words")


# ---------------------------------------------------------------------------------------------- 3. the conditional copy
@pytest.mark.parametrize("verdict", [None, 0, 1])
@pytest.mark.parametrize("when", [False, True])
def test_guard_copy(verdict, when):
    """fp32 tensors of 1 and 1025 elements (both 16-byte aligned: the 16-byte moves; the destination one float off: 4-byte words)
    and an int64 tensor of 3 elements (two words each)."""
    #          src          dst          src             dst             src (int64)  dst (int64)   src     dst
    entries = [(1025, 0), (1025, 0), (1025, 0), (1025, 1), (6, 2), (6, 0), (1, 3), (1, 0)]
    buf, views = placed(entries)
    gen = torch.Generator().manual_seed(9)
    for v in views:
        v.copy_(torch.randn(v.numel(), generator=gen))
    src = [views[0], views[2], views[4].view(torch.int64), views[6]]
    dst = [views[1], views[3], views[5].view(torch.int64), views[7]]
    src[2].copy_(torch.tensor([2 ** 40 + 3, -1, 7]))
    guard, gband = (None, None) if verdict is None else _banded_guard(verdict)
    before = buf.view(torch.int32).clone()
    guard_copy(dst, src, guard, when=when)
    torch.cuda.synchronize()
    if verdict is None or bool(verdict) == when:
        for i, (d, s) in enumerate(zip(dst, src)):
            assert torch.equal(d, s), f"tensor {i} was not copied"
        assert dst[2].tolist() == [2 ** 40 + 3, -1, 7]
        for s in (views[0], views[2], views[4], views[6]):
            o = s.storage_offset()
            assert torch.equal(s.view(torch.int32), before[o: o + s.numel()]), "the copy wrote into its source"
    else:
        assert torch.equal(buf.view(torch.int32), before), "a copy that was not to run wrote"
    assert_bands_untouched(buf, [views], "the copied tensors")
    if gband is not None:
        assert_bands_untouched(*gband, "the verdict words")


# ---------------------------------------------------------------------------------------------- 4. the trainer, toy fixture
def same_step(rep_a, rep_b, st_a, st_b, what, joint=True):
    """Guard on (a) against guard off (b), or two runs of the same step: the reports without the guard's two entries, and every
    state tensor of b."""
    exact = ops.MATH == "bf16x3" or not joint
    for k, v in rep_b.items():
        if k in ("skipped", "anomaly"):
            continue
        diff = float((rep_a[k].double() - v.double()).abs().max())
        if exact:
            assert torch.equal(rep_a[k], v), f"{what}: report {k} differs by {diff:.3e}"
        else:
            assert diff <= 1e-5 * max(1.0, float(v.double().abs().max())), f"{what}: report {k} differs by {diff:.3e}"
    if exact:
        differing = [k for k, v in st_b.items() if not torch.equal(st_a[k], v)]
        assert not differing, f"{what}: {len(differing)} state tensors differ, e.g. {differing[:5]}"


def unchanged(before, after, what):
    differing = [k for k, v in before.items() if not torch.equal(after[k], v)]
    assert not differing, f"{what}: a skipped step moved {len(differing)} state tensors, e.g. {differing[:5]}"
    assert not [k for k in after if k not in before and bool(after[k].any())], f"{what}: a skipped step created non-zero state"


def counts_of(rep):
    return dict(zip(G, rep["anomaly"].tolist()))


def poisoned(args, which, value, at=(0, 0, 0)):
    out = [a.clone() for a in args]
    out[which][at] = value
    return out


def follow_host_counters(twin, tr, args):
    """The host-side call counters count calls, skipped or not: the twin that never saw the bad batch is brought to the same
    count — NoiseTransfer's by one ``advance()`` call, the GRL counters (whose coefficient still moves on the first steps, Q7) by
    taking the trainer's."""
    twin.m["noise"].advance(args[0].size(0), args[2].size(0))
    twin.m["ad_net"].iter_num, twin.m["fd_s"].iter_num = tr.m["ad_net"].iter_num, tr.m["fd_s"].iter_num


def test_clean_eager_steps_equal_the_unguarded_steps():
    on, args, ts = toy()
    off, _, _ = toy()
    on.enable_anomaly_guard()
    on.enable_anomaly_guard()                                                 # idempotent
    for i, batch in enumerate((args, batch_b(args))):
        ra, rb = on.step(*batch, epoch=0, t_samples=ts), off.step(*batch, epoch=0, t_samples=ts)
        assert int(ra["skipped"]) == 0 and not any(ra["anomaly"].tolist()) and "skipped" not in rb
        same_step(ra, rb, on.snapshot()["t"], off.snapshot()["t"], f"clean eager step {i}")
    assert int(on.skipped_steps) == 0 and off.skipped_steps is None


def test_a_nan_batch_is_skipped_and_leaves_no_trace():
    tr, args, ts = toy()
    twin, _, _ = toy()
    tr.enable_anomaly_guard()
    # the very first step is the bad one: init_t / init_s stay unset, moments the step created stay zero
    first = tr.snapshot()
    rep = tr.step(*poisoned(args, 0, NAN), epoch=0, t_samples=ts)
    assert int(rep["skipped"]) == 1 and counts_of(rep)["fe_t"] > 0 and tr.init_t is None and tr.init_s is None
    unchanged(first["t"], tr.snapshot()["t"], "first step")
    follow_host_counters(twin, tr, args)
    # a clean step, then the bad batch again, with moments and init_t / init_s alive
    ra, rb = tr.step(*args, epoch=0, t_samples=ts), twin.step(*args, epoch=0, t_samples=ts)
    same_step(ra, rb, tr.snapshot()["t"], twin.snapshot()["t"], "clean step after a skipped first step")
    before = tr.snapshot()
    rep = tr.step(*poisoned(args, 0, NAN), epoch=0, t_samples=ts)
    assert int(rep["skipped"]) == 1 and counts_of(rep)["fe_t"] > 0 and int(tr.skipped_steps) == 2
    unchanged(before["t"], tr.snapshot()["t"], "second bad step")
    follow_host_counters(twin, tr, args)
    b = batch_b(args)
    ra, rb = tr.step(*b, epoch=0, t_samples=ts), twin.step(*b, epoch=0, t_samples=ts)
    assert int(ra["skipped"]) == 0
    same_step(ra, rb, tr.snapshot()["t"], twin.snapshot()["t"], "clean step after a skipped step")


def test_one_poisoned_gradient_is_found_in_its_group():
    tr, args, ts = toy()
    tr.enable_anomaly_guard()
    tr.step(*args, epoch=0, t_samples=ts)
    before = tr.snapshot()

    def poison():
        tr.m["clf_s"].hidden.bias.grad[0] = INF
    tr.on_grads_ready = poison
    rep = tr.step(*args, epoch=0, t_samples=ts)
    want = {k: int(k == "clf_s") for k in G}
    assert counts_of(rep) == want and int(rep["skipped"]) == 1
    unchanged(before["t"], tr.snapshot()["t"], "poisoned gradient")


def _replay_checks(on, off, replay, bad, clean, what, joint):
    """``replay(trainer, batch)`` replays a captured step.  A clean replay equals the guard-off one; a bad one leaves the state as
    it was; the next clean one equals the clean replay from the restored snapshot."""
    on.restore(off.snapshot())                                                 # the same state, whatever the captures left
    snap = on.snapshot()
    ra, rb = clone(replay(on, clean)), clone(replay(off, clean))
    assert int(ra["skipped"]) == 0
    same_step(ra, rb, on.snapshot()["t"], off.snapshot()["t"], f"{what}: clean replay, guard on vs off", joint)
    on.restore(snap)
    skipped_before = int(on.skipped_steps)
    rep = replay(on, bad)
    assert int(rep["skipped"]) == 1 and int(on.skipped_steps) == skipped_before + 1
    unchanged(snap["t"], on.snapshot()["t"], f"{what}: bad replay")
    r1 = clone(replay(on, clean))
    s1 = on.snapshot()["t"]
    assert int(r1["skipped"]) == 0
    on.restore(snap)
    if joint:
        on.m["noise"].advance(clean[0].size(0), clean[2].size(0))              # the skipped call was counted
    r2 = replay(on, clean)
    same_step(r1, r2, s1, on.snapshot()["t"], f"{what}: clean replay after a bad one vs from the restored snapshot", joint)


def test_joint_capture_and_replay_with_the_guard():
    on, args, ts = toy()
    off, _, _ = toy()
    on.enable_anomaly_guard()
    for tr in (on, off):
        torch.manual_seed(4)
        tr.capture(*args, epoch=0)
    assert int(on.skipped_steps) == 0
    with pytest.raises(RuntimeError, match="capture is resident"):
        off.enable_anomaly_guard()
    _replay_checks(on, off, lambda tr, b: tr.replay(*b, ts), poisoned(args, 2, INF, (1, 0, 3)), batch_b(args), "joint", True)
    assert int(on.skipped_steps) == 1


@pytest.mark.parametrize("phase", ["nf", "target_pretrain"])
def test_phase_capture_and_replay_with_the_guard(phase):
    """"target_pretrain" steps CPC: its shared Adam counter is among the state a skipped replay must leave alone."""
    on, args, ts = toy()
    off, _, _ = toy()
    on.enable_anomaly_guard()
    for tr in (on, off):
        tr.capture_phase(phase, *args)
    with pytest.raises(RuntimeError, match="capture is resident"):
        off.enable_anomaly_guard()
    on.replay_phase(phase, *args, t_samples=ts); off.replay_phase(phase, *args, t_samples=ts)   # moments and counters alive
    if phase == "target_pretrain":
        assert float(on.opt_cpc.param_groups[0]["step"]) == 1.0
    _replay_checks(on, off, lambda tr, b: tr.replay_phase(phase, *b, t_samples=ts), poisoned(args, 0, INF, (1, 0, 2)), batch_b(args),
                   phase, False)
    assert int(on.skipped_steps) == 1
    # the eager phase step takes the same decision
    before = on.snapshot()
    rep = on.phase_step(phase, *poisoned(args, 0, NAN), t_samples=ts)
    # "nf" detaches the features, so fe_t has no gradient — but its fused ReLUs hand the NaN on as torch's do: the flow's own
    # gradients see it, and so do fe_t's running statistics (the second line, without a GradBucket)
    hit = ("buffers", "nf") if phase == "nf" else ("fe_t",)
    assert int(rep["skipped"]) == 1 and all(counts_of(rep)[k] > 0 for k in hit) and counts_of(rep)["gradnorm"] == 0
    unchanged(before["t"], on.snapshot()["t"], f"eager {phase}")


# ---------------------------------------------------------------------------------------------- 5. data parallel, one rank over RCCL
def _worker_guard_rccl(rank, world, port, q):
    """One rank, backend "nccl" (= RCCL), the bucket forced to issue its collectives: the joint capture is three graphs, the save in
    the first and the verdict and the roll-back in the last."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    g = fixture("joint_small")
    args = [torch.tensor(g[f"s0.{k}"], device=dev) for k in ("x_t", "y_t", "x_s", "y_s")]
    ts = tuple(int(v) for v in g["s0.t_samples"])
    on, _ = _build_small_trainer(fst, dev, fst.GradBucket(always_reduce=True), "ddp")
    off, _ = _build_small_trainer(fst, dev, fst.GradBucket(always_reduce=True), "ddp")
    on.enable_anomaly_guard()
    for tr in (on, off):
        torch.manual_seed(4)
        tr.capture(*args, epoch=0)
    out = {"graphs": (len(on._graphs), len(off._graphs))}
    try:
        _replay_checks(on, off, lambda tr, b: tr.replay(*b, ts), poisoned(args, 0, INF, (1, 0, 2)), batch_b(args), "three graphs", True)
        out["checks"] = None
    except AssertionError as e:
        out["checks"] = str(e)
    out["skipped"] = int(on.skipped_steps)
    # With a bucket the forward-written buffers stay out of the verdict ("buffers" == 0): a NaN sample is caught through the
    # gradients alone, also in the "nf" phase, whose features are detached — the fused ReLUs do not turn it into 0.
    try:
        for what, run in (("nf", lambda b: on.phase_step("nf", *b, t_samples=ts)), ("joint", lambda b: on.step(*b, epoch=0, t_samples=ts))):
            before = on.snapshot()
            rep = run(poisoned(args, 0, NAN))
            assert int(rep["skipped"]) == 1 and counts_of(rep)["buffers"] == 0, f"eager {what} step on a NaN sample: {counts_of(rep)}"
            unchanged(before["t"], on.snapshot()["t"], f"eager {what} step, one RCCL rank")
        out["eager"] = None
    except AssertionError as e:
        out["eager"] = str(e)
    q.put((0, out))
    dist.destroy_process_group()


def _run_worker(name, rank, world, port, q):
    _guarded(globals()[name])(rank, world, port, q)


def test_data_parallel_capture_keeps_the_guard_on_one_rccl_rank():
    world, port = 1, 29691
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_run_worker, args=("_worker_guard_rccl", 0, world, port, q))]
    procs[0].start()
    (_, out), = _collect(q, world, procs)
    assert out["graphs"] == (3, 3), out
    assert out["checks"] is None, out["checks"]
    assert out["skipped"] == 1
    assert out["eager"] is None, out["eager"]


# ---------------------------------------------------------------------------------------------- 6. the real tensor count
def test_metric_network_eager_steps_with_the_guard():
    """JointConfig(L=512) at B=4: about 780 gradient tensors, 13 chunks of the scan and of the guarded updates."""
    def build():
        torch.manual_seed(1234)
        return fst.JointTrainer(fst.JointConfig(L_t=512, L_s=512, dropout_p=0.0), DEV)
    on, off = build(), build()
    on.enable_anomaly_guard()
    gen = torch.Generator().manual_seed(7)

    def pair():
        x = torch.randn(4, 1, 512, generator=gen)
        return ((x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True)).to(DEV), torch.randint(4, (4,), generator=gen).to(DEV)
    (x_t, y_t), (x_s, y_s) = pair(), pair()
    args = [x_t, y_t, x_s, y_s]
    ra, rb = on.step(*args, epoch=0, t_samples=(31, 77)), off.step(*args, epoch=0, t_samples=(31, 77))
    assert int(ra["skipped"]) == 0
    same_step(ra, rb, on.snapshot()["t"], off.snapshot()["t"], "metric network, clean step")
    before = on.snapshot()
    cpu = {}

    def count():
        n = 0
        for k in on.MODULES:
            grads = [p.grad for p in on.m[k].parameters() if p.grad is not None]
            cpu[k] = sum(int((~torch.isfinite(g.cpu())).sum()) for g in grads)
            n += len(grads)
        cpu["tensors"] = n
    on.on_grads_ready = count
    rep = on.step(*poisoned(args, 0, NAN), epoch=0, t_samples=(31, 77))
    assert cpu["tensors"] > 10 * 64, cpu["tensors"]
    got = counts_of(rep)
    assert int(rep["skipped"]) == 1 and {k: got[k] for k in on.MODULES} == {k: cpu[k] for k in on.MODULES}
    assert sum(got[k] for k in on.MODULES) == sum(cpu[k] for k in on.MODULES) > 0
    unchanged(before["t"], on.snapshot()["t"], "metric network, NaN batch")
