"""Weight averaging on the device (``fst_ema_multi`` / ``fst_swap_multi`` of csrc/guard.hip, ``optim.ema_update`` /
``swap_tensors`` / ``WeightAverage``, ``enable_weight_average`` / ``set_weight_average`` / ``averaged_weights`` of the two
trainers).  Needs an MI355X.

Kernel tests.  Every tensor and every state word lies between canary bands (``placed`` of test_gpu_anomaly_guard.py, ``banded`` of
test_gpu_schedules.py).  Element counts 1, 3, 5, 1023, 1024, 1025 and 65 543 (one quad past a full 64 x 256 x 4 pass: some threads
stride twice).  The average is a view 0..3 floats behind a 16-byte boundary and the live tensor one float further (mod 4): the
dword walk with every mix of alignments; and every count once more with both on a boundary: the 16-byte walk with its dword tail.
Values are randn times 1e-3 .. 1e3.

Gates.  One update: the kernel computes fma(w, live - avg, avg), the subtraction the same IEEE operation as the reference's and the
fma rounded once; the reference, float32(w * float32(live - avg) + avg) evaluated in fp64, can miss a rounding midpoint by one fp32
step — so one step, per element.  The weight words: the fp32 cast of the decay, one division and one subtraction, all on values in
[0, 1]: 8 * 2^-24 absolute.  K trainer steps against the fp64 recurrence with the reported weights: 3 * K * 2^-24 * M per tensor,
M the largest magnitude of the operands so far, the average before each update and the live tensor (the new average lies between
them; per step 2^-23 * M from the difference and 2^-24 * M from the fma, the earlier error damped by 1 - w <= 1).  Everything else is bit for bit.

Trainer tests: the toy configuration of test_gpu_phase_graphs.toy().  State comparisons are bit for bit in the default arithmetic;
under FST_MATH=f32 the joint step is compared as test_gpu_anomaly_guard.same_step does, as the clipping tests do."""
import ctypes
import functools
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import _lib, ops
from feature_level_style_transfer_for_tsc_amd.optim import WeightAverage, ema_update, swap_tensors
from test_gpu_anomaly_guard import placed, poisoned, same_step, unchanged
from test_gpu_conv_routes import CANARY
from test_gpu_phase_graphs import batch_b, clone, fixture, toy
from test_gpu_schedules import assert_bands_untouched, banded

DEV = "cuda"
INF, NAN = float("inf"), float("nan")
COUNTS = (1, 3, 5, 1023, 1024, 1025, 65_543)
# (numel, offset of the average, offset of the live tensor) in floats behind a 16-byte boundary
ENTRIES = [(n, off, (off + 1) % 4) for n in COUNTS for off in range(4)] + [(n, 0, 0) for n in COUNTS]     # 35 pairs
SCALES = (1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3)
W_GATE = 8 * 2.0 ** -24
M = fst.JointTrainer.MODULES
EXACT = ops.MATH == "bf16x3"
DECAY, WARMUP, COUNT, W = 0, 1, slice(2, 34), slice(34, 66)                  # words of the state block


class State:
    """The 66 state words between canary bands, and the guard's verdict word between its own."""

    def __init__(self, decay, warmup, counts=None, verdict=None):
        self.buf, (v,) = banded([66, 1], 1)
        self.views = v
        self.f, self.i = v[0], v[0].view(torch.int32)
        self.verdict = v[1].view(torch.int32)
        self.i.zero_()
        self.f[DECAY] = decay
        self.i[WARMUP] = int(warmup)
        if counts:
            for g, c in counts.items():
                self.i[COUNT][g] = c
        self.verdict.fill_(0 if verdict is None else verdict)
        self.use_verdict = verdict is not None

    def update(self, avg, live, groups, mask):
        n = len(avg)
        rc = _lib.load().fst_ema_multi((ctypes.c_void_p * n)(*[t.data_ptr() for t in avg]), (ctypes.c_void_p * n)(*[t.data_ptr() for t in live]),
                                       (ctypes.c_int64 * n)(*[t.numel() for t in avg]), (ctypes.c_int32 * n)(*groups), n,
                                       mask - (1 << 32) if mask >> 31 else mask,
                                       self.f.data_ptr(), self.verdict.data_ptr() if self.use_verdict else None, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert_bands_untouched(self.buf, [self.views], "the state words")
        return rc

    @property
    def w(self):
        return self.f[W].cpu()

    @property
    def count(self):
        return self.i[COUNT].cpu()


def swap_raw(a, b, numel=None):
    n = len(a)
    return _lib.load().fst_swap_multi((ctypes.c_void_p * n)(*[t.data_ptr() for t in a]), (ctypes.c_void_p * n)(*[t.data_ptr() for t in b]),
                                      (ctypes.c_int64 * n)(*(numel or [t.numel() for t in a])), n, _lib.stream_ptr())


@functools.lru_cache(maxsize=None)
def case():
    """(averages, live tensors) on the host for ENTRIES, drawn once and never changed."""
    gen = torch.Generator().manual_seed(21)
    avg = [torch.randn(n, generator=gen) * SCALES[i % len(SCALES)] for i, (n, _, _) in enumerate(ENTRIES)]
    live = [torch.randn(n, generator=gen) * SCALES[(i + i // 7) % len(SCALES)] for i, (n, _, _) in enumerate(ENTRIES)]
    return avg, live


def on_device(entries=ENTRIES, hosts=None):
    """((buffer, views) of the averages, (buffer, views) of the live tensors)."""
    hosts = case() if hosts is None else hosts
    out = []
    for side, h in enumerate(hosts):
        buf, views = placed([(e[0], e[1 + side]) for e in entries])
        for v, t in zip(views, h):
            v.copy_(t)
        out.append((buf, views))
    return out


def ordered(t):
    """fp32 bits as integers that grow with the value: the distance of two floats in fp32 steps is their difference."""
    b = t.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(b < 0, -(b & 0x7FFFFFFF), b)


def steps(a, b):
    return int((ordered(a) - ordered(b)).abs().max())


def bits(t):
    """The words of an fp32 tensor (NaN payloads and −0 compare as what they are); an integer buffer as it is."""
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def want_update(avg, live, w):
    """float32(w * float32(live - avg) + avg), the product and the sum in fp64."""
    return (float(w) * (live - avg).double() + avg.double()).float()


# ---------------------------------------------------------------------------------------------- 1. one update
def test_one_update_is_one_fma_on_every_count_and_alignment():
    avg_h, live_h = case()
    (abuf, avg), (lbuf, live) = on_device()
    groups = [i % 32 for i in range(len(ENTRIES))]
    st = State(0.9, warmup=False)
    live_before = lbuf.view(torch.int32).clone()
    assert st.update(avg, live, groups, 0xFFFFFFFF) == 0
    w = st.w
    assert w.tolist() == [float(torch.tensor(1.0) - torch.tensor(0.9))] * 32 and st.count.tolist() == [1] * 32
    worst = 0
    for e, a, ah, lh, g in zip(ENTRIES, avg, avg_h, live_h, groups):
        d = steps(a.cpu(), want_update(ah, lh, w[g]))
        worst = max(worst, d)
        assert d <= 1, f"{e}: {d} fp32 steps off the exactly rounded update"
        assert not torch.equal(a.cpu(), ah), f"{e}: not updated"
    print(f"one update: at most {worst} fp32 step(s) off float32(w * float32(live - avg) + avg) evaluated in fp64")
    assert torch.equal(lbuf.view(torch.int32), live_before), "the update wrote into the live tensors or their bands"
    assert_bands_untouched(abuf, [avg], "the averages")
    # the same bits from the same inputs
    first = abuf.view(torch.int32).clone()
    for a, ah in zip(avg, avg_h):
        a.copy_(ah)
    assert st.update(avg, live, groups, 0xFFFFFFFF) == 0 and st.count.tolist() == [2] * 32
    assert torch.equal(abuf.view(torch.int32), first), "two updates of the same values differ"


# ---------------------------------------------------------------------------------------------- 2. w = 1 and w = 0
def test_decay_zero_copies_the_live_tensor_bit_for_bit():
    (abuf, avg), (lbuf, live) = on_device()
    st = State(0.0, warmup=False)
    assert st.update(avg, live, [(3 * i) % 32 for i in range(len(avg))], 0xFFFFFFFF) == 0
    assert st.w.tolist() == [1.0] * 32
    for e, a, l in zip(ENTRIES, avg, live):
        assert torch.equal(bits(a), bits(l)), f"{e}: w = 1 did not leave the live tensor in the average"
    assert_bands_untouched(abuf, [avg], "the averages")
    assert_bands_untouched(lbuf, [live], "the live tensors")


@pytest.mark.parametrize("how", ["inactive group", "verdict 1"])
def test_weight_zero_keeps_every_bit_and_the_count(how):
    (abuf, avg), (lbuf, live) = on_device()
    for i, l in enumerate(live):                                              # what must not reach an average that is left alone
        l[0] = (NAN, INF, -INF)[i % 3]
        l[-1] = (INF, NAN)[i % 2]
    odd = torch.tensor([-0.0, 1e-40, -1e-45], dtype=torch.float32).view(torch.int32).tolist() + [0x7FC12345, -0x3FEDCB]
    for i, a in enumerate(avg):                                               # −0, denormals, NaNs with payloads in the averages
        bits(a)[0] = odd[i % len(odd)]
    before = abuf.view(torch.int32).clone()
    groups = [5] * len(avg)
    if how == "inactive group":
        st = State(0.5, warmup=False, counts={5: 3, 6: 4})
        assert st.update(avg, live, groups, 0xFFFFFFFF & ~(1 << 5)) == 0
        want_count = [1] * 32
        want_count[5], want_count[6] = 3, 5
        assert float(st.w[5]) == 0.0 and float(st.w[6]) == 0.5
    else:
        st = State(0.5, warmup=False, counts={5: 3, 6: 4}, verdict=1)
        assert st.update(avg, live, groups, 0xFFFFFFFF) == 0
        want_count = [0] * 32
        want_count[5], want_count[6] = 3, 4
        assert st.w.tolist() == [0.0] * 32
    assert st.count.tolist() == want_count
    assert torch.equal(abuf.view(torch.int32), before), f"{how}: an average that was to be left alone changed"
    if how == "verdict 1":                                                    # and with the verdict clear the same call averages
        st.verdict.fill_(0)
        assert st.update(avg, live, groups, 0xFFFFFFFF) == 0
        assert float(st.w[5]) == 0.5 and int(st.count[5]) == 4 and all(bool(torch.isnan(a[0]) | torch.isinf(a[0])) for a in avg)


# ---------------------------------------------------------------------------------------------- 3. launches and groups
def test_130_pairs_in_groups_0_and_31_with_nothing_between():
    """Three launches (64 + 64 + 2 pairs).  Only the groups of the mask move; each group takes its own weight in one call."""
    entries = [(COUNTS[i % 6], i % 4, (i + (i // 4) % 2) % 4) for i in range(130)]   # the counts below 65 543; aligned alike or not
    gen = torch.Generator().manual_seed(22)
    hosts = ([torch.randn(n, generator=gen) * SCALES[i % len(SCALES)] for i, (n, _, _) in enumerate(entries)],
             [torch.randn(n, generator=gen) * SCALES[(i + 2) % len(SCALES)] for i, (n, _, _) in enumerate(entries)])
    (abuf, avg), (lbuf, live) = on_device(entries, hosts)
    groups = [0 if i % 3 else 31 for i in range(130)]
    st = State(0.75, warmup=False)
    assert st.update(avg, live, groups, 1 << 31) == 0
    assert st.w.tolist() == [0.0] * 31 + [0.25] and st.count.tolist() == [0] * 31 + [1]
    for i, (a, ah, lh, g) in enumerate(zip(avg, *hosts, groups)):
        if g == 0:
            assert torch.equal(bits(a.cpu()), bits(ah)), f"pair {i} of the inactive group moved"
        else:
            assert steps(a.cpu(), want_update(ah, lh, 0.25)) <= 1, f"pair {i} of group 31"
    # warming up from different counts: w[0] = 1 - 1/10, w[31] = 1 - 6/15, both in one call
    for a, ah in zip(avg, hosts[0]):
        a.copy_(ah)
    st = State(0.999, warmup=True, counts={31: 5})
    assert st.update(avg, live, groups, (1 << 31) | 1) == 0
    w = st.w
    assert abs(float(w[0]) - 0.9) <= W_GATE and abs(float(w[31]) - 0.6) <= W_GATE and w[1:31].tolist() == [0.0] * 30
    assert st.count.tolist() == [1] + [0] * 30 + [6]
    for i, (a, ah, lh, g) in enumerate(zip(avg, *hosts, groups)):
        assert steps(a.cpu(), want_update(ah, lh, w[g])) <= 1, f"pair {i} of group {g}"
    assert_bands_untouched(abuf, [avg], "the averages")
    assert_bands_untouched(lbuf, [live], "the live tensors")
    # the Python entry point: the same bits
    first = [a.clone() for a in avg]
    for a, ah in zip(avg, hosts[0]):
        a.copy_(ah)
    wa = WeightAverage(DEV, 0.999, warmup=True)
    wa.count[31] = 5
    ema_update(avg, live, groups, wa, [0, 31])
    torch.cuda.synchronize()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(avg, first)) and torch.equal(wa.w.cpu(), w) and wa.count.tolist() == st.count.tolist()


# ---------------------------------------------------------------------------------------------- 4. the weight words
def test_the_weights_warm_up_as_the_formula_says():
    decay = 0.999
    (abuf, avg), (lbuf, live) = on_device(ENTRIES[:4])
    st = State(decay, warmup=True)
    worst = 0.0
    for t in range(12):
        assert st.update(avg, live, [2, 2, 9, 9], (1 << 2) | (1 << 9)) == 0
        want = 1.0 - min(decay, (1 + t) / (10 + t))
        w = st.w
        for g in (2, 9):
            worst = max(worst, abs(float(w[g]) - want))
            assert abs(float(w[g]) - want) <= W_GATE, (t, g, float(w[g]), want)
        assert [float(w[g]) for g in range(32) if g not in (2, 9)] == [0.0] * 30
        assert st.count.tolist() == [(t + 1) * (g in (2, 9)) for g in range(32)]
    print(f"weight words: at most {worst:.3e} off the fp64 formula (gate {W_GATE:.3e})")
    # a decay written later is followed; without warm-up it is the decay alone
    st.f[DECAY] = 0.25
    assert st.update(avg, live, [2, 2, 9, 9], 1 << 2) == 0 and float(st.w[2]) == 0.75 and float(st.w[9]) == 0.0
    st.i[WARMUP] = 0
    st.f[DECAY] = decay
    assert st.update(avg, live, [2, 2, 9, 9], 1 << 9) == 0
    assert abs(float(st.w[9]) - (1.0 - decay)) <= W_GATE and st.count[9] == 13 and st.count[2] == 13


# ---------------------------------------------------------------------------------------------- 5. the exchange
def test_swap_exchanges_exactly_and_twice_is_the_identity():
    avg_h, live_h = case()
    (abuf, a), (bbuf, b) = on_device()
    odd = torch.tensor([-0.0, 1e-40, INF], dtype=torch.float32).view(torch.int32).tolist() + [0x7FC12345, -0x3FEDCB]
    for i, (x, y) in enumerate(zip(a, b)):
        bits(x)[0], bits(y)[-1] = odd[i % len(odd)], odd[(i + 2) % len(odd)]
    a0, b0 = abuf.view(torch.int32).clone(), bbuf.view(torch.int32).clone()
    xa, xb = [bits(x).clone() for x in a], [bits(y).clone() for y in b]
    assert swap_raw(a, b) == 0
    torch.cuda.synchronize()
    for e, x, y, wa, wb in zip(ENTRIES, a, b, xa, xb):
        assert torch.equal(bits(x), wb) and torch.equal(bits(y), wa), f"{e}: not exchanged element for element"
    assert_bands_untouched(abuf, [a], "the first list")
    assert_bands_untouched(bbuf, [b], "the second list")
    swap_tensors(a, b)                                                        # back, through the Python entry point
    torch.cuda.synchronize()
    assert torch.equal(abuf.view(torch.int32), a0) and torch.equal(bbuf.view(torch.int32), b0), "two exchanges are not the identity"


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_a_bad_entry_is_refused_before_the_first_launch():
    abuf, (a,) = banded([4] * 130, 1)
    bbuf, (b,) = banded([4] * 130, 1)
    before = (abuf.clone(), bbuf.clone())
    st = State(0.0, warmup=False)
    words = st.buf.clone()
    assert st.update(a, b, [0] * 129 + [32], 0xFFFFFFFF) == -1                 # the bad entry is in the third chunk
    assert b"tensor 129: group 32" in _lib.load().fst_last_error()
    assert swap_raw(a, b, numel=[4] * 129 + [0]) == -1
    assert b"tensor 129" in _lib.load().fst_last_error()
    torch.cuda.synchronize()
    assert torch.equal(abuf, before[0]) and torch.equal(bbuf, before[1]) and torch.equal(st.buf, words), "a refused call wrote"
    with pytest.raises(ValueError, match="contiguous"):
        swap_tensors([abuf[:8].view(2, 4).t()], [bbuf[:8].view(2, 4).t()])
    with pytest.raises(TypeError, match="float32"):
        ema_update([abuf[:8].half()], [bbuf[:8].half()], [0], WeightAverage(DEV), [0])
    assert float(abuf[0]) == CANARY


# ---------------------------------------------------------------------------------------------- 7.-13. JointTrainer, toy fixture
def ema_of(tr):
    """{name: clone} of the averages and the counts as the snapshot names them."""
    return {k: v.clone() for k, v in tr._state_tensors().items() if k.startswith("ema.")}


def live_of(tr):
    """{module: {name: clone}} of the live tensors that are averaged."""
    return {k: {n: tr.m[k].state_dict()[n].clone() for n in d} for k, d in tr._ema_avg.items()}


def recurrence_gate(ref, got, live_now, w, k_steps, seen, what):
    """One step of the fp64 recurrence on ``ref`` (in place) with the reported weight, then the gate of the module docstring."""
    worst = 0.0
    for n, r in ref.items():
        seen[n] = max(seen.get(n, 0.0), float(r.abs().max()), float(live_now[n].abs().max()))   # the operands: the average BEFORE
        r += float(w) * (live_now[n].double() - r)
        err, bound = float((got[n].double() - r).abs().max()), 3 * k_steps * 2.0 ** -24 * seen[n]
        assert err <= bound, f"{what} {n}: {err:.3e} off the fp64 recurrence, bound {bound:.3e}"
        worst = max(worst, err / bound if bound else 0.0)
    return worst


def test_the_training_trajectory_does_not_move():
    on, args, ts = toy()
    off, _, _ = toy()
    on.enable_weight_average()
    on.enable_weight_average(decay=0.5)                                       # idempotent
    assert on.weight_average.decay_host == float(torch.tensor(0.999))
    for i, batch in enumerate((args, batch_b(args), args)):
        ra, rb = on.step(*batch, epoch=0, t_samples=ts), off.step(*batch, epoch=0, t_samples=ts)
        assert "ema_weight" not in rb and "ema_steps" not in rb
        assert ra["ema_weight"].shape == (len(M),) and ra["ema_weight"].dtype == torch.float32 and bool((ra["ema_weight"] > 0).all())
        assert ra["ema_steps"].dtype == torch.int32 and ra["ema_steps"].tolist() == [i + 1] * len(M)
        sa, sb = on.snapshot()["t"], off.snapshot()["t"]
        assert {k for k in sa if k not in sb} == set(ema_of(on)) and "ema.count" in sa
        same_step(ra, rb, sa, sb, f"step {i} with the weight average on against off")
    assert off.weight_average is None and "weight_average" not in off.state_dict()
    with pytest.raises(RuntimeError, match="enable_weight_average"):
        off.set_weight_average(decay=0.9)


def test_the_averages_are_what_the_formula_says():
    on, args, ts = toy()
    on.enable_weight_average()
    ref = {k: {n: t.double().clone() for n, t in d.items()} for k, d in on._ema_avg.items()}
    assert any(n.endswith("running_var") for n in ref["fe_t"]) and not any(n.endswith("num_batches_tracked") for d in ref.values() for n in d)
    assert all(n in ref[k] for k in M for n, _ in on.m[k].named_parameters())
    seen, worst, K = {k: {} for k in M}, 0.0, 4
    for i in range(K):
        rep = on.step(*(args if i % 2 == 0 else batch_b(args)), epoch=0, t_samples=ts)
        live, w = live_of(on), rep["ema_weight"].cpu()
        want_w = 1.0 - min(0.999, (1 + i) / (10 + i))
        assert all(abs(float(v) - want_w) <= W_GATE for v in w), (i, w.tolist(), want_w)
        for gi, k in enumerate(M):
            worst = max(worst, recurrence_gate(ref[k], on._ema_avg[k], live[k], w[gi], i + 1, seen[k], f"step {i} {k}"))
    print(f"{K} steps: the averages use at most {worst:.3f} of the bound 3 K 2^-24 max(|avg|, |live|)")
    moved = [k for k in M if any(not torch.equal(on._ema_avg[k][n], t) for n, t in live_of(on)[k].items())]
    assert set(moved) == set(M), "an average that equals its live tensor after four steps was not averaged"


class _Resident(fst.JointTrainer):
    """A trainer that only says a capture is resident."""

    def __init__(self, graphs=(object(),), phase=None):
        self.device, self._graphs, self._phase, self.m = torch.device(DEV), graphs, phase or {}, {}


@functools.lru_cache(maxsize=None)
def captured():
    """(trainer with the mode on and the joint step captured, batch A, CPC indices, snapshot after the capture) — shared by the
    tests that need a resident capture; each restores the snapshot first."""
    on, args, ts = toy()
    on.enable_weight_average()
    torch.manual_seed(4)
    on.capture(*args, epoch=0)
    return on, args, ts, on.snapshot()


def test_replay_equals_eager_and_follows_the_decay():
    on, args, ts, snap = captured()
    on.restore(snap)
    on.set_weight_average(decay=0.999)
    with pytest.raises(RuntimeError, match="capture is resident"):
        _Resident().enable_weight_average()
    b = batch_b(args)
    n0 = int(snap["t"]["ema.count"][0])
    assert n0 >= 11 and snap["t"]["ema.count"][: len(M)].tolist() == [n0] * len(M), "the warm-up steps train, and average"

    def both(what):
        on.restore(snap)
        rep = clone(on.replay(*b, ts))
        after_graph = on.snapshot()["t"]
        on.restore(snap)
        eager = on.step(*b, epoch=0, t_samples=ts)
        after_eager = on.snapshot()["t"]
        assert torch.equal(rep["ema_weight"], eager["ema_weight"]) and torch.equal(rep["ema_steps"], eager["ema_steps"]), what
        assert rep["ema_steps"].tolist() == [n0 + 1] * len(M) and torch.equal(after_graph["ema.count"], after_eager["ema.count"])
        live_same = all(torch.equal(after_graph[k], v) for k, v in after_eager.items() if not k.startswith("ema."))
        differing = [k for k, v in after_eager.items() if k.startswith("ema.") and not torch.equal(after_graph[k], v)]
        print(f"{what}: live state of replay and eager step bit-equal: {live_same}; averages that differ: {len(differing)}")
        if EXACT:
            assert not differing, f"{what}: {len(differing)} averages differ between replay and eager step, e.g. {differing[:5]}"
        else:
            for k in differing:
                d = float((after_graph[k].double() - after_eager[k].double()).abs().max())
                assert d <= 1e-5 * max(1.0, float(after_eager[k].abs().max())), (what, k, d)
        moved = [k for k, v in snap["t"].items() if k.startswith("ema.") and not torch.equal(after_graph[k], v)]
        assert len(moved) > len(M)
        return rep

    rep = both("decay 0.999")
    want = 1.0 - min(0.999, (1 + n0) / (10 + n0))
    assert all(abs(float(v) - want) <= W_GATE for v in rep["ema_weight"]), (rep["ema_weight"].tolist(), want)
    on.restore(snap)
    assert on.set_weight_average(decay=0.5) is True                            # legal under the resident capture: no re-capture
    rep = both("decay 0.5 set under the resident capture")
    assert rep["ema_weight"].tolist() == [0.5] * len(M), "(1 + n) / (10 + n) is above 0.5 from the second update on"
    on.set_weight_average(decay=0.999)


@pytest.mark.parametrize("phase", ["nf", "target_pretrain"])
def test_a_phase_averages_the_modules_it_steps(phase):
    on, args, ts = toy()
    on.enable_weight_average(decay=0.75, warmup=False)
    inside = fst.JointTrainer.PHASES[phase]
    on.capture_phase(phase, *args)                                            # (first: it creates the moments the steps update)
    assert not any(on.weight_average.count.tolist()), "capture_phase has no training side effect: the counts too"
    with pytest.raises(RuntimeError, match="capture is resident"):
        _Resident(graphs=None, phase={phase: object()}).enable_weight_average()

    def check(before, after, rep, what):
        assert rep["ema_weight"].tolist() == [0.25 if k in inside else 0.0 for k in M], what
        assert rep["ema_steps"].tolist() == [int(before["ema.count"][i]) + (k in inside) for i, k in enumerate(M)], what
        assert torch.equal(after["ema.count"][: len(M)], rep["ema_steps"]) and not bool(after["ema.count"][len(M):].any())
        any_moved = []
        for k in M:
            names = [n for n in before if n.startswith(f"ema.{k}.")]
            moved = [n for n in names if not torch.equal(after[n], before[n])]
            if k in inside:                                                   # towards the live tensor, wherever that is another value
                differ = [n for n in names if not torch.equal(after["m." + n[4:]], before[n])]
                assert moved == differ, f"{what}: averages of {k} that moved {moved[:3]}, live tensors off their average {differ[:3]}"
                any_moved.append(bool(moved))
            else:
                assert not moved, f"{what}: {k} is not stepped by {phase!r}, yet {moved[:3]} moved"
        assert sum(any_moved) >= 2, f"{what}: the phase trains, so averages move (\"nf\" detaches the features: only buffers move there)"

    b = batch_b(args)
    snap = on.snapshot()
    rep_e = clone(on.phase_step(phase, *b, t_samples=ts))
    after_e = on.snapshot()["t"]
    check(snap["t"], after_e, rep_e, f"eager {phase}")
    on.restore(snap)
    rep_g = clone(on.replay_phase(phase, *b, t_samples=ts))
    after_g = on.snapshot()["t"]
    check(snap["t"], after_g, rep_g, f"replayed {phase}")
    assert torch.equal(rep_g["ema_weight"], rep_e["ema_weight"]) and torch.equal(rep_g["ema_steps"], rep_e["ema_steps"])
    if phase == "nf":                                                         # no CPC: identical launches, identical bits
        differing = [k for k, v in after_e.items() if not torch.equal(after_g[k], v)]
        assert not differing, f"replayed nf against eager: {differing[:5]}"
    # a second replay goes on from the first: the counts are device words, nothing is baked in
    rep_2 = on.replay_phase(phase, *args, t_samples=ts)
    assert rep_2["ema_steps"].tolist() == [2 * (k in inside) for k in M]


def test_a_skipped_step_leaves_the_averages_and_the_next_one_averages():
    on, args, ts = toy()
    on.enable_anomaly_guard()
    on.enable_weight_average()
    on.step(*args, epoch=0, t_samples=ts)                                     # moments and init_t / init_s alive
    b = batch_b(args)
    before = on.snapshot()
    rep = on.step(*poisoned(b, 0, NAN), epoch=0, t_samples=ts)
    assert int(rep["skipped"]) == 1 and rep["ema_weight"].tolist() == [0.0] * len(M) and rep["ema_steps"].tolist() == [1] * len(M)
    after = on.snapshot()["t"]
    assert sum(k.startswith("ema.") for k in before["t"]) > len(M)
    unchanged(before["t"], after, "NaN batch with the weight average on")
    rep = on.step(*b, epoch=0, t_samples=ts)
    want = 1.0 - 2 / 11
    assert int(rep["skipped"]) == 0 and rep["ema_steps"].tolist() == [2] * len(M)
    assert all(abs(float(v) - want) <= W_GATE for v in rep["ema_weight"]), rep["ema_weight"].tolist()
    after = on.snapshot()["t"]
    assert all(any(not torch.equal(after[n], v) for n, v in before["t"].items() if n.startswith(f"ema.{k}.")) for k in M)


def fresh_target_modules():
    """Newly built (feature extractor, classifier) of the toy trainer's target side, with their own initial weights."""
    meta = json.loads(str(fixture("joint_small")["meta"]))
    tup = lambda lp: [[tuple(t) for t in l] for l in lp]
    return fst.OS_CNN_res(tup(meta["lp_t"])).to(DEV), fst.OS_CNN(tup(meta["lp_clf"]), meta["ncls_t"]).to(DEV)


def _logits(fe, clf, x):
    with torch.no_grad(), ops.pack_cache():
        return clf(fe(x))[0].clone()


def test_averaged_weights_puts_the_averages_into_the_modules(tmp_path):
    on, args, ts = toy()
    on.enable_weight_average(decay=0.5, warmup=False)
    for batch in (args, batch_b(args)):
        on.step(*batch, epoch=0, t_samples=ts)
    fe, clf = on.m["fe_t"], on.m["clf_t"]
    x, y = args[0], args[1]
    batches = [(x[:3], y[:3]), (x[3:], y[3:])]
    inv = on.m["nf"].convinv
    caches = [c.W_inverse for c in inv]                                       # the step's infer() cached them (Q2)
    cache_bits = [bits(c).clone() for c in caches]
    entry = on.state_dict()["weight_average"]
    assert entry["decay"] == 0.5 and entry["warmup"] is False and entry["counts"][: len(M)] == [2] * len(M)
    fe.eval(); clf.eval()
    live_logits = _logits(fe, clf, x)                                         # (a forward re-masks the omni-scale weights in place: Q1)
    live = {k: {n: t.clone() for n, t in on.m[k].state_dict().items()} for k in M}
    with on.averaged_weights():
        assert not any(hasattr(c, "W_inverse") for c in inv), "the live flow's inverses are set aside"
        for k in M:                                                           # the modules hold the averages, integer buffers their own
            for n, t in on.m[k].state_dict().items():
                want = entry["tensors"][k][n] if n in entry["tensors"][k] else live[k][n].cpu()
                assert torch.equal(t.cpu(), want), f"inside: {k}.{n}"
        inside = _logits(fe, clf, x)
        acc, preds = fst.eval_accuracy(fe, clf, batches)
        assert torch.equal(preds, inside.argmax(dim=1)) and acc == float((preds == y).double().mean())
        with torch.no_grad():
            on.m["nf"].infer(torch.randn_like(fe(x)))
        assert all(hasattr(c, "W_inverse") for c in inv), "the averaged flow inverts its own weights"
        path = fst.save_target_classification_modules(fe, clf, 3, str(tmp_path / "averaged.tar"))
        for call in (lambda: on.replay(*args, ts), lambda: on.step(*args, epoch=0, t_samples=ts),
                     lambda: on.phase_step("nf", *args), lambda: on.replay_phase("nf", *args)):
            with pytest.raises(RuntimeError, match="inside averaged_weights"):
                call()
        with pytest.raises(RuntimeError, match="does not nest"):
            on.averaged_weights().__enter__()
    assert not torch.equal(inside, live_logits), "the averaged model is another model"
    for k in M:
        for n, t in on.m[k].state_dict().items():
            assert torch.equal(bits(t), bits(live[k][n])), f"after the context {k}.{n} is not what it was"
    assert all(c.W_inverse is w and torch.equal(bits(w), b) for c, w, b in zip(inv, caches, cache_bits)), "the live caches are put back"
    assert torch.equal(_logits(fe, clf, x), live_logits)
    # freshly built modules with the averaged tensors of the checkpoint entry, and with the .tar written inside the context
    for how in ("state_dict entry", "checkpoint"):
        f2, c2 = fresh_target_modules()
        if how == "checkpoint":
            assert fst.load_target_classification_modules(path, f2, c2) == 3   # strict
        else:
            for mod, k in ((f2, "fe_t"), (c2, "clf_t")):
                mod.load_state_dict({n: entry["tensors"][k].get(n, live[k][n].cpu()) for n in live[k]}, strict=True)
        f2.eval(); c2.eval()
        assert torch.equal(_logits(f2, c2, x), inside), f"fresh modules loaded from the {how} give other logits"
    with ops.pack_cache():
        with pytest.raises(RuntimeError, match="pack_cache"):
            on.averaged_weights().__enter__()
    on.step(*args, epoch=0, t_samples=ts)                                     # and training goes on


def test_resume_equals_the_uninterrupted_run():
    a, args, ts = toy()
    a.enable_weight_average()
    a.step(*args, epoch=0, t_samples=ts)
    sd = a.state_dict()
    r, _, _ = toy()
    assert r.weight_average is None
    r.load_state_dict(sd)                                                     # enables the mode
    assert r.weight_average is not None and r.weight_average.count.tolist() == a.weight_average.count.tolist()
    assert (r.weight_average.decay_host, r.weight_average.warmup_host) == (a.weight_average.decay_host, True)
    for i, batch in enumerate((batch_b(args), args)):
        ra, rr = a.step(*batch, epoch=0, t_samples=ts), r.step(*batch, epoch=0, t_samples=ts)
        sa, sr = a.snapshot()["t"], r.snapshot()["t"]
        assert set(sa) == set(sr) and torch.equal(sa["ema.count"], sr["ema.count"]) and torch.equal(ra["ema_weight"], rr["ema_weight"])
        same_step(rr, ra, sr, sa, f"step {i} after the resume against the uninterrupted run")
    # a checkpoint without the entry leaves the mode as it is
    off, _, _ = toy()
    r.load_state_dict(off.state_dict())
    assert r.weight_average is not None and r.weight_average.count[0] == 3


def test_a_load_under_a_resident_capture_keeps_the_addresses():
    on, args, ts, snap = captured()
    on.restore(snap)
    ptrs = {k: v.data_ptr() for k, v in on._state_tensors().items() if k.startswith("ema.")}
    words = on.weight_average.words.data_ptr()
    sd = on.state_dict()
    on.replay(*batch_b(args), ts)                                             # move on, then go back through the checkpoint
    on.load_state_dict(sd)
    now = on._state_tensors()
    assert {k: v.data_ptr() for k, v in now.items() if k.startswith("ema.")} == ptrs and on.weight_average.words.data_ptr() == words
    assert all(torch.equal(now[k], v) for k, v in snap["t"].items() if k.startswith("ema."))
    rep = on.replay(*batch_b(args), ts)                                       # the resident graph averages into the loaded tensors
    assert rep["ema_steps"].tolist() == [int(snap["t"]["ema.count"][0]) + 1] * len(M)
    assert any(not torch.equal(on._state_tensors()[k], v) for k, v in snap["t"].items() if k.startswith("ema.m") or k.startswith("ema.nf"))


# ---------------------------------------------------------------------------------------------- 14. ClassifierTrainer
def test_classifier_trainer_averages_in_eager_and_replayed_steps():
    gen = torch.Generator().manual_seed(7)
    mk = lambda: (torch.randn(8, 1, 64, generator=gen).to(DEV), torch.randint(3, (8,), generator=gen).to(DEV))
    batches = [mk() for _ in range(4)]
    torch.manual_seed(5)
    off = fst.ClassifierTrainer(64, 1, 3, DEV)
    on = fst.ClassifierTrainer(64, 1, 3, DEV, weight_average=dict(decay=0.9, warmup=True))
    assert off.weight_average is None and isinstance(on.weight_average, WeightAverage)
    with pytest.raises(RuntimeError, match="enable_weight_average"):
        off.set_weight_average(decay=0.5)
    on.fe.load_state_dict(off.fe.state_dict()); on.clf.load_state_dict(off.clf.state_dict())
    for k, mod in (("fe", on.fe), ("clf", on.clf)):                           # (the averages start from the weights at enable time)
        for n, t in on._ema_avg[k].items():
            t.copy_(mod.state_dict()[n])

    def state(tr):
        out = dict(("fe." + k, v.clone()) for k, v in tr.fe.state_dict().items())
        out.update(("clf." + k, v.clone()) for k, v in tr.clf.state_dict().items())
        for name, o in (("opt_fe", tr.opt_fe), ("opt_clf", tr.opt_clf)):
            for i, p in enumerate(o.param_groups[0]["params"]):
                if "square_avg" in o.state[p]:
                    out[f"{name}.{i}"] = o.state[p]["square_avg"].clone()
        return out

    def same_trajectory(what):
        sa, sb = state(on), state(off)
        differing = [k for k in sb if not torch.equal(sa[k], sb[k])]
        assert set(sa) == set(sb) and not differing, f"{what}: the mode moved the training: {differing[:5]}"

    ref = {k: {n: t.double().clone() for n, t in d.items()} for k, d in on._ema_avg.items()}
    seen, worst, n_upd = {"fe": {}, "clf": {}}, 0.0, 0

    def follow(what, k_steps):
        """The words after update number ``n_upd`` and the averages against the recurrence, ``k_steps`` updates after ``ref`` was exact."""
        nonlocal worst
        w = on.weight_average.w.cpu()
        want = 1.0 - min(0.9, n_upd / (9 + n_upd))
        assert abs(float(w[0]) - want) <= W_GATE and float(w[0]) == float(w[1]) and w[2:].tolist() == [0.0] * 30, (what, w.tolist())
        assert on.weight_average.count.tolist() == [n_upd, n_upd] + [0] * 30
        for gi, (k, mod) in enumerate((("fe", on.fe), ("clf", on.clf))):
            live = {n: mod.state_dict()[n] for n in ref[k]}
            worst = max(worst, recurrence_gate(ref[k], on._ema_avg[k], live, w[gi], k_steps, seen[k], f"{what} {k}"))

    for i, (x, y) in enumerate(batches[:2]):
        la, lb = on.step(x, y), off.step(x, y)
        assert isinstance(la, tuple) and len(la) == 2 and torch.equal(la[0], lb[0]) and torch.equal(la[1], lb[1])
        same_trajectory(f"eager step {i}")
        n_upd += 1
        follow(f"eager step {i}", i + 1)
    on.capture(*batches[2], warmup=2); off.capture(*batches[2], warmup=2)
    with pytest.raises(RuntimeError, match="capture is resident"):
        off.enable_weight_average()
    same_trajectory("the capture's warm-up")
    n_upd += 2                                                                # the warm-up's two eager steps train, and average
    ref = {k: {n: t.double().clone() for n, t in d.items()} for k, d in on._ema_avg.items()}   # the recurrence goes on from here
    for i, (x, y) in enumerate(batches[2:]):
        la, lb = on.replay(x, y), off.replay(x, y)
        assert torch.equal(la[0], lb[0]) and torch.equal(la[1], lb[1])
        same_trajectory(f"replay {i}")
        n_upd += 1
        follow(f"replay {i}", i + 1)
    assert on.set_weight_average(decay=0.25) is True                          # steered under the resident capture
    on.replay(*batches[0]); off.replay(*batches[0])
    assert on.weight_average.w[:2].tolist() == [0.75, 0.75]
    same_trajectory("a replay after set_weight_average")
    print(f"classifier: the averages use at most {worst:.3f} of the bound")
    # the context round-trips
    live = state(on)
    avgs = {k: {n: t.clone() for n, t in d.items()} for k, d in on._ema_avg.items()}
    with on.averaged_weights():
        for k, mod in (("fe", on.fe), ("clf", on.clf)):
            for n, t in mod.state_dict().items():
                want = avgs[k][n] if n in avgs[k] else live[f"{k}.{n}"]
                assert torch.equal(bits(t), bits(want)), f"inside: {k}.{n}"
        for call in (lambda: on.step(*batches[0]), lambda: on.replay(*batches[0])):
            with pytest.raises(RuntimeError, match="inside averaged_weights"):
                call()
    after = state(on)
    assert all(torch.equal(bits(after[k]), bits(v)) for k, v in live.items()), "after the context a live bit is not what it was"
    assert all(torch.equal(on._ema_avg[k][n], t) for k, d in avgs.items() for n, t in d.items())
