"""Gradient norms and clipping on the device (``fst_sumsq_multi`` / ``fst_scale_multi`` of csrc/guard.hip, ``optim.sumsq_norms`` /
``scale_by_group``, ``JointTrainer.enable_grad_clip`` / ``set_grad_clip``).  Needs an MI355X.

Kernel tests.  Every tensor, slot array and output word lies between canary bands (``placed`` of test_gpu_anomaly_guard.py and
``banded`` of test_gpu_schedules.py, in the manner of test_gpu_pointwise_edges.py).  Element counts 1, 3, 5, 1023, 1024, 1025 and
65 543 (one quad past a full 64 x 256 x 4 grid pass: some threads take a second stride), each as a view 0, 1, 2 and 3 floats behind
a 16-byte boundary; values are randn times 1e-3 .. 1e3.

Accuracy gate.  The reference is the fp64 sum of squares of the same fp32 values.  A thread adds at most 2 quads here (64 on a
tensor of 2^20 elements) in one fma chain, the workgroup adds 8 levels, the finaliser adds 64 slots in fp64: (64 + 8) * 2^-24 is about
4e-6, and the gate is five times that: 2e-5 relative on a sum, 1e-5 on a norm.  The tests print the largest error they saw.

Trainer tests: the toy configuration of the anomaly-guard tests.  State comparisons are bit for bit in the default arithmetic; under
FST_MATH=f32 the joint step is compared as test_gpu_anomaly_guard.same_step does (RandomLayer's K-split GEMM uses float atomics
there)."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import _lib, ops
from feature_level_style_transfer_for_tsc_amd.optim import GradClip, clip_coefficients, scale_by_group, sumsq_norms
from test_gpu_anomaly_guard import follow_host_counters, placed, poisoned, same_step, unchanged
from test_gpu_conv_routes import CANARY
from test_gpu_modules import close
from test_gpu_phase_graphs import batch_b, clone, real_gradient_gate, same_losses, toy, unstepped_untouched
from test_gpu_schedules import assert_bands_untouched, banded

DEV = "cuda"
INF, NAN = float("inf"), float("nan")
REC = 65                                                                     # a tensor's record in the slot array: group id, 64 partial sums
COUNTS = (1, 3, 5, 1023, 1024, 1025, 65_543)
ENTRIES = [(n, off) for n in COUNTS for off in range(4)]                     # 28 tensors
SCALES = (1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3)
SUM_GATE, NORM_GATE = 2e-5, 1e-5
M = fst.JointTrainer.MODULES


class Words:
    """slots, limits[33], norms[33], coef[32] of one scan between canary bands."""

    def __init__(self, n_tensors, limits=None):
        self.n_slots = int(_lib.load().fst_sumsq_slots(n_tensors))
        assert self.n_slots == REC * n_tensors
        self.buf, (v,) = banded([max(self.n_slots, 1), 33, 33, 32], 1)
        self.views = v
        self.slots, self.limits, self.norms, self.coef = v
        self.limits.copy_(torch.tensor([INF] * 33 if limits is None else limits, dtype=torch.float32))

    def scan(self, tensors, groups):
        n = len(tensors)
        _lib.check(_lib.load().fst_sumsq_multi((ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors]),
                                               (ctypes.c_int64 * n)(*[t.numel() for t in tensors]), (ctypes.c_int32 * n)(*groups), n,
                                               self.slots.data_ptr(), self.n_slots, self.limits.data_ptr(), self.norms.data_ptr(),
                                               self.coef.data_ptr(), _lib.stream_ptr()), "fst_sumsq_multi")
        torch.cuda.synchronize()
        assert_bands_untouched(self.buf, [self.views], "the scan's slots and words")
        return self.norms.cpu(), self.coef.cpu()

    def sums(self, n_tensors):
        """(group ids, fp64 sum of each tensor's slots) as the scan left them."""
        rec = self.slots[: n_tensors * REC].view(n_tensors, REC).cpu()
        return rec[:, 0].tolist(), rec[:, 1:].double().sum(dim=1)


def scale_raw(tensors, groups, coef):
    n = len(tensors)
    return _lib.load().fst_scale_multi((ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors]), (ctypes.c_int64 * n)(*[t.numel() for t in tensors]),
                                       (ctypes.c_int32 * n)(*groups), n, coef.data_ptr(), _lib.stream_ptr())


@functools.lru_cache(maxsize=None)
def case():
    """(host tensors, fp64 sums of squares): the 28 tensors' values, drawn once and never changed."""
    gen = torch.Generator().manual_seed(11)
    hosts = [torch.randn(n, generator=gen) * SCALES[i % len(SCALES)] for i, (n, _) in enumerate(ENTRIES)]
    return hosts, [float((h.double() ** 2).sum()) for h in hosts]


def on_device(entries=ENTRIES, hosts=None):
    hosts = case()[0] if hosts is None else hosts
    buf, views = placed(entries)
    for v, h in zip(views, hosts):
        v.copy_(h)
    return buf, views


def rel(got, want):
    return abs(got - want) / want if want else abs(got)


def ulps(a, b):
    """Distance in fp32 steps of two tensors of positive floats."""
    return int((a.float().view(torch.int32) - b.float().view(torch.int32)).abs().max())


# ---------------------------------------------------------------------------------------------- 1. the scan
def test_sumsq_every_count_at_every_start_offset():
    hosts, want = case()
    buf, views = on_device()
    before = buf.view(torch.int32).clone()
    w = Words(len(views))
    groups = list(range(len(views)))                                          # every tensor a group of its own
    norms, coef = w.scan(views, groups)
    ids, sums = w.sums(len(views))
    assert ids == [float(g) for g in groups]
    worst_sum = max(rel(float(s), v) for s, v in zip(sums, want))
    worst_norm = max(rel(float(norms[g]), v ** 0.5) for g, v in enumerate(want))
    total = rel(float(norms[32]), sum(want) ** 0.5)
    print(f"sumsq: largest relative error of a sum {worst_sum:.3e}, of a norm {worst_norm:.3e}, of the total {total:.3e}")
    for i, (s, v) in enumerate(zip(sums, want)):
        assert rel(float(s), v) <= SUM_GATE, f"tensor {ENTRIES[i]}: sum {float(s)!r} vs {v!r}"
        assert rel(float(norms[i]), v ** 0.5) <= NORM_GATE, f"tensor {ENTRIES[i]}: norm {float(norms[i])!r} vs {v ** 0.5!r}"
    assert total <= NORM_GATE and norms[28:32].tolist() == [0.0] * 4 and coef.tolist() == [1.0] * 32
    assert torch.equal(buf.view(torch.int32), before), "the scan wrote into its inputs or their bands"
    # the same words on every run
    first = (w.norms.view(torch.int32).clone(), w.coef.view(torch.int32).clone(), w.slots.view(torch.int32).clone())
    w.scan(views, groups)
    again = (w.norms.view(torch.int32), w.coef.view(torch.int32), w.slots.view(torch.int32))
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "two scans of the same values differ"


def test_130_tensors_in_groups_0_and_31_with_nothing_between():
    """Three launches (64 + 64 + 2 tensors); the groups' sums collect tensors of every launch."""
    entries = [(COUNTS[i % 6], i % 4) for i in range(130)]                     # the counts below 65 543, every offset
    gen = torch.Generator().manual_seed(12)
    hosts = [torch.randn(n, generator=gen) * SCALES[i % len(SCALES)] for i, (n, _) in enumerate(entries)]
    buf, views = on_device(entries, hosts)
    groups = [0 if i % 3 else 31 for i in range(130)]
    want = {g: sum(float((h.double() ** 2).sum()) for h, gi in zip(hosts, groups) if gi == g) for g in (0, 31)}
    w = Words(130)
    norms, coef = w.scan(views, groups)
    ids, sums = w.sums(130)
    assert ids == [float(g) for g in groups]
    for g in (0, 31):
        got = float(sum(s for s, gi in zip(sums, groups) if gi == g))
        print(f"group {g}: sum off by {rel(got, want[g]):.3e}, norm by {rel(float(norms[g]), want[g] ** 0.5):.3e}")
        assert rel(got, want[g]) <= SUM_GATE and rel(float(norms[g]), want[g] ** 0.5) <= NORM_GATE
    assert norms[1:31].tolist() == [0.0] * 30 and rel(float(norms[32]), (want[0] + want[31]) ** 0.5) <= NORM_GATE
    assert_bands_untouched(buf, [views], "the scanned tensors")
    # the Python entry point: the same words
    clip = GradClip(DEV)
    sumsq_norms(views, groups, clip.limits, clip.norms, clip.coef)
    assert torch.equal(clip.norms.cpu().view(torch.int32), norms.view(torch.int32)) and clip.coef.tolist() == [1.0] * 32


def test_an_overflowing_group_switches_all_clipping_off():
    hosts = [h.clone() for h in case()[0][:8]]
    hosts[5][2] = 1e20                                                        # its square is not an fp32 number
    buf, views = on_device(ENTRIES[:8], hosts)
    groups = [0, 0, 3, 3, 3, 7, 7, 31]
    w = Words(8, limits=[1e-6] * 33)                                          # limits that clip every group that has a gradient
    norms, coef = w.scan(views, groups)
    assert float(norms[7]) == INF and float(norms[32]) == INF and bool(torch.isfinite(norms[:7]).all()) and float(norms[3]) > 0
    assert coef.tolist() == [1.0] * 32
    before = buf.view(torch.int32).clone()
    scale_by_group(views, groups, w.coef)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before), "unit coefficients changed a bit"
    # the same with a NaN; and with the bad value gone the limits bite again
    views[5][2] = NAN
    norms, coef = w.scan(views, groups)
    assert bool(torch.isnan(norms[7])) and bool(torch.isnan(norms[32])) and coef.tolist() == [1.0] * 32
    views[5][2] = 0.5
    norms, coef = w.scan(views, groups)
    assert bool((coef[[0, 3, 7, 31]] < 1.0).all())


@pytest.mark.parametrize("name, limits", [
    ("global cap", {32: 7.0}), ("group caps", {0: 1e-5, 3: 5.0, 7: 1e6}), ("both", {0: 1e-5, 3: 5.0, 32: 2.5}),
    ("a cap on an empty group", {1: 1e-9, 32: 100.0}), ("a zero cap", {3: 0.0, 32: 1.0}), ("none", {})])
def test_coefficients_are_clip_coefficients_of_the_reported_norms(name, limits):
    buf, views = on_device(ENTRIES[:12])
    groups = [0, 0, 0, 3, 3, 3, 7, 7, 7, 31, 31, 31]
    lim = [INF] * 33
    for g, v in limits.items():
        lim[g] = v
    w = Words(12, limits=lim)
    norms, coef = w.scan(views, groups)
    want = clip_coefficients(norms, w.limits.cpu())
    assert bool((want[[0, 3, 7, 31]] < 1.0).any()) == (name != "none")
    got, want32 = coef, want.float()
    zero = want32 == 0
    assert torch.equal(got[zero], want32[zero]) and ulps(got[~zero], want32[~zero]) <= 1, (name, got.tolist(), want.tolist())
    # and through the Python entry points the tensors shrink by exactly these factors
    clip = GradClip(DEV)
    clip.set_limits(lim)
    sumsq_norms(views, groups, clip.limits, clip.norms, clip.coef)
    assert torch.equal(clip.coef.cpu(), coef)
    scale_by_group(views, groups, clip.coef)
    torch.cuda.synchronize()
    for v, h, g in zip(views, case()[0], groups):
        assert torch.equal(v.cpu(), h * coef[g]), (name, g)
    assert_bands_untouched(buf, [views], f"scaled tensors ({name})")


# ---------------------------------------------------------------------------------------------- 2. the scale
def test_a_unit_coefficient_keeps_every_bit():
    buf, views = on_device()
    odd = torch.tensor([-0.0, 1e-40, -1e-45, INF, -INF], dtype=torch.float32).view(torch.int32).tolist() + [0x7FC12345, -0x3FEDCB]
    for i, v in enumerate(views):                                             # −0, denormals, infinities, NaNs with payloads: first and last
        bits = v.view(torch.int32)
        bits[0] = odd[i % len(odd)]
        bits[-1] = odd[(i + 3) % len(odd)]
    before = buf.view(torch.int32).clone()
    buf_c, (cv,) = banded([32], 1)
    cv[0].fill_(1.0)
    assert scale_raw(views, [i % 32 for i in range(len(views))], cv[0]) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before), "a coefficient of 1.0f changed a bit"
    assert_bands_untouched(buf_c, [cv], "the coefficients")


def test_half_is_an_exact_halving_and_stays_inside_the_tensor():
    hosts = case()[0]
    buf, views = on_device()
    buf_c, (cv,) = banded([32], 1)
    cv[0].fill_(0.5)
    assert scale_raw(views, [(5 * i) % 32 for i in range(len(views))], cv[0]) == 0
    torch.cuda.synchronize()
    for e, v, h in zip(ENTRIES, views, hosts):
        assert torch.equal(v.cpu(), h * 0.5), f"{e}: not every element was halved exactly once"
    assert_bands_untouched(buf, [views], "halved tensors")
    assert_bands_untouched(buf_c, [cv], "the coefficients")


def test_each_group_takes_its_own_coefficient_in_one_launch():
    hosts = case()[0]
    pick = [5, 14, 27, 22]                                                    # (3, off 1), (1023, off 2), (65 543, off 3), (1025, off 2)
    buf, views = on_device([ENTRIES[i] for i in pick], [hosts[i] for i in pick])
    coef = torch.ones(32, device=DEV)
    coef[3], coef[7], coef[31] = 0.5, 0.25, 3.0
    groups = [3, 7, 31, 4]
    scale_by_group(views, groups, coef)
    torch.cuda.synchronize()
    for v, i, c in zip(views, pick, (0.5, 0.25, 3.0, 1.0)):
        assert torch.equal(v.cpu(), hosts[i] * c), (ENTRIES[i], c)
    assert_bands_untouched(buf, [views], "tensors of four groups")


def test_scale_refuses_a_bad_entry_before_the_first_launch():
    buf, (views,) = banded([4] * 66, 1)
    before = buf.clone()
    coef = torch.full((32,), 0.5, device=DEV)
    assert scale_raw(views, [0] * 65 + [32], coef) == -1                      # the bad entry is in the second chunk
    assert b"group 32" in _lib.load().fst_last_error()
    w = Words(66)
    n = 66
    rc = _lib.load().fst_sumsq_multi((ctypes.c_void_p * n)(*[t.data_ptr() for t in views]), (ctypes.c_int64 * n)(*[4] * 65 + [0]),
                                     (ctypes.c_int32 * n)(*[0] * n), n, w.slots.data_ptr(), w.n_slots, w.limits.data_ptr(),
                                     w.norms.data_ptr(), w.coef.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and torch.equal(buf, before), "a refused call wrote"
    assert bool((w.slots == CANARY).all()) and bool((w.norms == CANARY).all()) and bool((w.coef == CANARY).all())


# ---------------------------------------------------------------------------------------------- 3. the trainer, toy fixture
EXACT = ops.MATH == "bf16x3"


def flat(sd, prefix=""):
    """Every tensor of a (nested) state_dict by its path."""
    out = {}
    items = sd.items() if isinstance(sd, dict) else enumerate(sd) if isinstance(sd, (list, tuple)) else ()
    for k, v in items:
        if isinstance(v, torch.Tensor):
            out[f"{prefix}{k}"] = v
        else:
            out.update(flat(v, f"{prefix}{k}."))
    return out


def grad_norms(tr, modules=M):
    """fp64 norms of the .grad tensors as they are now: per module of MODULES (0 outside ``modules``) and, last, over all."""
    sq = [sum(float((p.grad.double() ** 2).sum()) for p in tr.m[k].parameters() if p.grad is not None) if k in modules else 0.0 for k in M]
    return torch.tensor([v ** 0.5 for v in sq] + [sum(sq) ** 0.5], dtype=torch.float64)


def scale_hook(tr, coef, modules=M):
    """What a user would do by hand: multiply each module's gradients by the fp32 factor the clipped trainer reported."""
    def hook():
        for k in modules:
            for p in tr.m[k].parameters():
                if p.grad is not None:
                    p.grad.mul_(coef[M.index(k)])
    return hook


def same_state(a, b, what):
    differing = [k for k, v in b.items() if not torch.equal(a[k], v)]
    assert not differing, f"{what}: {len(differing)} state tensors differ, e.g. {differing[:5]}"


def test_report_only_is_a_no_op_and_reports_the_norms_of_the_gradients():
    on, args, ts = toy()
    off, _, _ = toy()
    on.enable_grad_clip()
    on.enable_grad_clip()                                                     # idempotent
    seen = {}
    on.on_grads_ready = lambda: seen.update(norms=grad_norms(on))
    for i, batch in enumerate((args, batch_b(args), args)):
        ra, rb = on.step(*batch, epoch=0, t_samples=ts), off.step(*batch, epoch=0, t_samples=ts)
        assert "grad_l2" not in rb and "clip_coef" not in rb
        assert ra["grad_l2"].shape == (len(M) + 1,) and ra["clip_coef"].tolist() == [1.0] * len(M)
        same_step(ra, rb, on.snapshot()["t"], off.snapshot()["t"], f"report-only step {i}")
        err = ((ra["grad_l2"].double().cpu() - seen["norms"]).abs() / seen["norms"].clamp_min(1e-30)).max()
        print(f"step {i}: grad_l2 off the fp64 norms of the gradients by {float(err):.3e} at most")
        assert float(seen["norms"][-1]) > 0 and int((seen["norms"] > 0).sum()) >= len(M) - 1
        assert float(err) <= NORM_GATE, (ra["grad_l2"].tolist(), seen["norms"].tolist())
    sa, sb = on.state_dict(), off.state_dict()
    assert sa.pop("grad_clip") == {"max_norm": None, "per_module": {}} and "grad_clip" not in sb
    fa, fb = flat(sa), flat(sb)
    assert set(fa) == set(fb) and len(fb) > 100
    if EXACT:
        same_state(fa, fb, "state_dict after three steps")


def test_clipping_is_the_scaling_it_reports():
    on, args, ts = toy()
    twin, _, _ = toy()
    on.enable_grad_clip()
    for tr in (on, twin):
        tr.step(*args, epoch=0, t_samples=ts)                                 # moments and init_t / init_s alive
    b = batch_b(args)
    snap, snap_twin = on.snapshot(), twin.snapshot()
    free = clone(on.step(*b, epoch=0, t_samples=ts))
    unclipped = on.snapshot()["t"]
    total, nf = float(free["grad_l2"][-1]), float(free["grad_l2"][M.index("nf")])

    # a cap on the whole at half of what the step measured
    on.restore(snap)
    assert on.set_grad_clip(max_norm=total / 2) is True
    rep = clone(on.step(*b, epoch=0, t_samples=ts))
    coef = rep["clip_coef"]
    assert torch.equal(rep["grad_l2"], free["grad_l2"]), "the norms are those before clipping"
    assert bool((coef < 1.0).all()) and bool((coef > 0.49).all()) and float(coef.max() - coef.min()) == 0.0, coef.tolist()
    twin.on_grads_ready = scale_hook(twin, coef)
    twin.step(*b, epoch=0, t_samples=ts)
    if EXACT:
        same_state(on.snapshot()["t"], twin.snapshot()["t"], "max_norm against gradients scaled by hand")
    assert on.state_dict()["grad_clip"] == {"max_norm": total / 2, "per_module": {}}

    # a cap on the flow alone
    on.restore(snap); twin.restore(snap_twin)
    on.set_grad_clip(max_norm=None, per_module={"nf": nf / 2})
    rep = clone(on.step(*b, epoch=0, t_samples=ts))
    coef = rep["clip_coef"]
    others = [i for i, k in enumerate(M) if k != "nf"]
    assert coef[others].tolist() == [1.0] * len(others) and 0.49 < float(coef[M.index("nf")]) < 0.51, coef.tolist()
    twin.on_grads_ready = scale_hook(twin, coef)
    twin.step(*b, epoch=0, t_samples=ts)
    after = on.snapshot()["t"]
    if EXACT:
        same_state(after, twin.snapshot()["t"], "a cap on nf against gradients scaled by hand")
        moved = [k for k, v in unclipped.items() if not torch.equal(after[k], v)]
        assert moved and all(k.startswith(("m.nf.", "o.nf.")) for k in moved), f"a cap on nf moved {moved[:5]}"
    # the checkpoint carries the limits while the mode is on; one without the entry leaves the mode as it is
    assert not twin.grad_clip and "grad_clip" not in twin.state_dict()
    limits = list(on._clip.limits_host)
    on.load_state_dict(twin.state_dict())
    assert on.grad_clip and on._clip.limits_host == limits
    twin.on_grads_ready = None
    twin.load_state_dict(on.state_dict())
    assert twin.grad_clip and twin._clip.limits_host == limits and twin._clip.limits.tolist() == limits
    ra, rb = on.step(*b, epoch=0, t_samples=ts), twin.step(*b, epoch=0, t_samples=ts)
    assert float(rb["clip_coef"][M.index("nf")]) < 1.0 and rb["clip_coef"][others].tolist() == [1.0] * len(others)
    if EXACT:
        assert torch.equal(ra["clip_coef"], rb["clip_coef"]) and torch.equal(ra["grad_l2"], rb["grad_l2"])


def test_capture_and_replay_follow_the_limits():
    on, args, ts = toy()
    on.enable_grad_clip()
    torch.manual_seed(4)
    on.capture(*args, epoch=0)
    b = batch_b(args)
    snap = on.snapshot()
    free = clone(on.replay(*b, ts))
    total = float(free["grad_l2"][-1])
    assert free["clip_coef"].tolist() == [1.0] * len(M) and total > 0
    on.restore(snap)
    assert on.set_grad_clip(max_norm=total / 2) is True                       # legal under the resident capture: no re-capture
    r1 = clone(on.replay(*b, ts))
    s1 = on.snapshot()["t"]
    assert bool((r1["clip_coef"] < 1.0).all()) and bool((r1["clip_coef"] > 0.49).all()), r1["clip_coef"].tolist()
    on.restore(snap)
    r2 = on.replay(*b, ts)
    same_step(r1, r2, s1, on.snapshot()["t"], "two replays with limits")
    if EXACT:
        assert torch.equal(r1["grad_l2"], free["grad_l2"]), "the norms are those before clipping"
        assert torch.equal(r1["grad_l2"], r2["grad_l2"]) and torch.equal(r1["clip_coef"], r2["clip_coef"])
    # the eager step from the same state: the gates of test_full_batch_graph_replay_equals_eager_step
    on.restore(snap)
    eager = on.step(*b, epoch=0, t_samples=ts)
    for k in ("nf_t", "nf_s", "ce_t", "sl_t", "ce_s", "sl_s", "cdan", "ce_s2t2s", "fd_s"):
        x, y = float(r1[k]), float(eager[k])
        assert abs(x - y) <= 1e-6 * max(1.0, abs(y)), (k, x, y)
    for k in ("w_t", "w_s", "norms_t", "norms_s", "grad_l2", "clip_coef"):
        close(r1[k], eager[k], 1e-5, f"graph vs eager {k}")
    after_eager = on.snapshot()["t"]
    for k in ("m.fe_t.net_1.net.net.1.conv1d.weight", "m.cpc.Wk.0.weight", "m.clf_t.hidden.weight"):
        real_gradient_gate(s1, after_eager, k, "clipped replay vs eager")
    on.set_grad_clip(max_norm=None, per_module=None)
    on.restore(snap)
    assert on.replay(*b, ts)["clip_coef"].tolist() == [1.0] * len(M)


def test_phase_steps_clip_what_the_phase_updates():
    on, args, ts = toy()
    off, _, _ = toy()
    on.enable_grad_clip()
    inside = fst.JointTrainer.PHASES["nf"]
    for tr in (on, off):
        tr.capture_phase("nf", *args)                                         # (first: it creates the moments the steps update)
    with pytest.raises(RuntimeError, match="capture is resident"):
        off.enable_grad_clip()
    seen = {}
    on.on_grads_ready = lambda: seen.update(norms=grad_norms(on, inside))
    before = on.snapshot()
    rep = on.phase_step("nf", *args, t_samples=ts)
    on.on_grads_ready = None
    l2, i_nf = rep["grad_l2"], M.index("nf")
    assert [float(v) for i, v in enumerate(l2[:-1]) if i != i_nf] == [0.0] * (len(M) - 1), "the features are detached: the flow alone"
    assert float(l2[i_nf]) > 0 and float(l2[-1]) == float(l2[i_nf]), "the total is the flow's norm"
    assert rel(float(l2[i_nf]), float(seen["norms"][i_nf])) <= NORM_GATE and rep["clip_coef"].tolist() == [1.0] * len(M)
    unstepped_untouched("nf", before["t"], on.snapshot()["t"], "eager nf")
    # replayed: the same, and a cap set under the resident capture
    b = batch_b(args)
    snap = on.snapshot()
    free = clone(on.replay_phase("nf", *b, t_samples=ts))
    assert set(free) == {"nf_t", "nf_s", "total", "grad_l2", "clip_coef"} and free["clip_coef"].tolist() == [1.0] * len(M)
    on.restore(snap)
    on.set_grad_clip(max_norm=float(free["grad_l2"][-1]) / 2)
    rep = clone(on.replay_phase("nf", *b, t_samples=ts))
    after_graph = on.snapshot()["t"]
    coef = rep["clip_coef"]
    assert 0.49 < float(coef[i_nf]) < 0.51 and [float(c) for i, c in enumerate(coef) if M[i] not in inside] == [1.0] * (len(M) - len(inside))
    assert torch.equal(rep["grad_l2"], free["grad_l2"]) and float(rep["grad_l2"][-1]) == float(rep["grad_l2"][i_nf])
    unstepped_untouched("nf", snap["t"], after_graph, "clipped nf replay")
    on.restore(snap)
    eager = on.phase_step("nf", *b, t_samples=ts)
    same_losses({k: rep[k] for k in ("nf_t", "nf_s", "total")}, {k: eager[k] for k in ("nf_t", "nf_s", "total")}, "clipped nf replay vs eager")
    assert torch.equal(eager["grad_l2"], rep["grad_l2"]) and torch.equal(eager["clip_coef"], coef)
    same_state(after_graph, on.snapshot()["t"], "clipped nf replay vs eager")  # "nf" runs no CPC: identical launches


def test_a_skipped_step_is_not_clipped_and_the_next_one_is():
    on, args, ts = toy()
    twin, _, _ = toy()
    on.enable_anomaly_guard()
    on.enable_grad_clip()
    for tr in (twin, on):
        tr.step(*args, epoch=0, t_samples=ts)                                 # moments and init_t / init_s alive
    b = batch_b(args)
    before = on.snapshot()
    free = clone(on.step(*b, epoch=0, t_samples=ts))                          # what the clean step measures, unclipped
    on.restore(before)
    on.set_grad_clip(max_norm=float(free["grad_l2"][-1]) / 4)
    rep = on.step(*poisoned(b, 0, NAN), epoch=0, t_samples=ts)
    assert int(rep["skipped"]) == 1 and rep["clip_coef"].tolist() == [1.0] * len(M) and not bool(torch.isfinite(rep["grad_l2"][-1]))
    unchanged(before["t"], on.snapshot()["t"], "NaN batch with both modes on")
    follow_host_counters(twin, on, args)
    rep = on.step(*b, epoch=0, t_samples=ts)
    coef = rep["clip_coef"].clone()
    # (the host-side call counters counted the skipped call, so NoiseTransfer's ratios and with them the gradients are not those of
    # the unclipped run above to the bit: the cap at a quarter of that run's norm gives factors near a quarter, and the twin decides)
    assert int(rep["skipped"]) == 0 and bool(torch.isfinite(rep["grad_l2"]).all())
    assert bool((coef < 0.26).all()) and bool((coef > 0.24).all()), (coef.tolist(), rep["grad_l2"].tolist(), free["grad_l2"].tolist())
    twin.on_grads_ready = scale_hook(twin, coef)
    rb = twin.step(*b, epoch=0, t_samples=ts)
    same_step(rep, rb, on.snapshot()["t"], twin.snapshot()["t"], "clean clipped step after a skipped one")
