"""Host side of the device weight averaging (no GPU): the two new symbols in header, ctypes table and library; the launchers' and
the wrappers' refusals; the arithmetic of ``optim.ema_update``'s CPU branch against ``torch.optim.swa_utils.get_ema_multi_avg_fn``
and against the warm-up formula; and the trainer's switch.  The kernels and the trainers' steps are tested in
test_gpu_weight_average.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import _lib, ops, optim
from feature_level_style_transfer_for_tsc_amd.optim import AnomalyGuard, WeightAverage, ema_update, swap_tensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fst_ema_multi", "fst_swap_multi")
N = 130                                                                      # entries of a call: three launches' worth


def test_header_binding_and_library_agree_on_the_new_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fst_hip.h")).read(), flags=re.S)
    for name in NEW:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, f"{name} is not declared in include/fst_hip.h"
        res, args = _lib._SIGNATURES[name]
        assert res is _lib.c_int and len(args) == decl.group(1).count(",") + 1, f"{name}: the ctypes table and the header disagree"
    version = int(re.search(r"#define\s+FST_ABI_VERSION\s+(\d+)", text).group(1))
    assert version == _lib.ABI_VERSION >= 23
    lib = _lib.load()
    assert lib.fst_version() == version
    for name in NEW:
        assert hasattr(lib, name), name
    assert all(hasattr(fst, k) for k in ("WeightAverage", "ema_update", "swap_tensors"))
    # refused on the host before any launch (there is no device here: a launch would return another code)
    assert lib.fst_ema_multi(None, None, None, None, 0, 0, None, None, None) == -1 and lib.fst_last_error()
    assert lib.fst_swap_multi(None, None, None, 1, None) == -1 and lib.fst_last_error()


def _call(at=None, a=None, b=None, numel=None, group=None, state_off=0, verdict_off=None):
    """Both launchers on 130 made-up entries, of which entry ``at`` is changed into one they must REFUSE (nothing here may reach a
    launch: these are no device pointers); the state block and the verdict are aligned host words that are never dereferenced."""
    lib = _lib.load()
    A = [0x100000 + 4096 * i for i in range(N)]
    B = [0x900000 + 4096 * i for i in range(N)]
    ne, gr = [8 + i for i in range(N)], [i % 32 for i in range(N)]
    if at is not None:
        for lst, v in ((A, a), (B, b), (ne, numel), (gr, group)):
            if v is not None:
                lst[at] = v if v != "null" else None
    words = np.zeros(80, dtype=np.int32)
    arrays = ((ctypes.c_void_p * N)(*A), (ctypes.c_void_p * N)(*B), (ctypes.c_int64 * N)(*ne), (ctypes.c_int32 * N)(*gr))
    verdict = None if verdict_off is None else words.ctypes.data + 4 * 70 + verdict_off
    ema = lib.fst_ema_multi(*arrays, N, -1, words.ctypes.data + state_off, verdict, None)
    if at is None:                                                            # only the state words are bad: the swap takes none
        return ema, None
    swap = lib.fst_swap_multi(arrays[0], arrays[1], arrays[2], N, None)
    assert not words.any(), "a refused call wrote into the state block"
    return ema, swap


BAD = [("null average", dict(a="null")), ("null live tensor", dict(b="null")), ("average 2 bytes off", dict(a=0x100002)),
       ("live tensor 1 byte off", dict(b=0x900001)), ("no elements", dict(numel=0)), ("negative count", dict(numel=-3)),
       ("2^31 elements", dict(numel=2 ** 31))]


@pytest.mark.parametrize("at", [0, 64, N - 1], ids=["first", "middle", "last"])
@pytest.mark.parametrize("what, entry", BAD, ids=[w for w, _ in BAD])
def test_launchers_refuse_a_bad_entry_on_the_host(what, entry, at):
    assert _call(at, **entry) == (-1, -1), what
    assert f"tensor {at}:".encode() in _lib.load().fst_last_error()


@pytest.mark.parametrize("at", [0, 64, N - 1], ids=["first", "middle", "last"])
@pytest.mark.parametrize("group", [32, -1])
def test_ema_refuses_a_bad_group(group, at):
    lib = _lib.load()
    arrays = ((ctypes.c_void_p * N)(*[0x100000 + 64 * i for i in range(N)]), (ctypes.c_void_p * N)(*[0x900000 + 64 * i for i in range(N)]),
              (ctypes.c_int64 * N)(*[4] * N), (ctypes.c_int32 * N)(*[group if i == at else 31 for i in range(N)]))
    words = np.zeros(66, dtype=np.int32)
    assert lib.fst_ema_multi(*arrays, N, 1, words.ctypes.data, None, None) == -1
    assert f"tensor {at}: group {group}".encode() in lib.fst_last_error() and not words.any()


def test_launchers_refuse_overlapping_pairs_and_misaligned_state_words():
    assert _call(64, b=0x100000 + 4096 * 64 + 16) == (-1, -1)                 # live starts inside its average
    assert b"overlap" in _lib.load().fst_last_error()
    assert _call(state_off=2)[0] == -1 and b"state" in _lib.load().fst_last_error()
    assert _call(verdict_off=2)[0] == -1 and b"verdict" in _lib.load().fst_last_error()
    lib = _lib.load()
    arrays = ((ctypes.c_void_p * 1)(4096), (ctypes.c_void_p * 1)(8192), (ctypes.c_int64 * 1)(4), (ctypes.c_int32 * 1)(0))
    assert lib.fst_ema_multi(*arrays, 1, 1, None, None, None) == -1, "a null state block"
    assert lib.fst_ema_multi(arrays[0], arrays[1], arrays[2], None, 1, 1, 4096, None, None) == -1, "no group ids"


def test_wrappers_refuse_what_the_kernels_cannot_take():
    st = WeightAverage("cpu")
    x, y = torch.randn(4, 6), torch.randn(4, 6)
    for a, b in (([x.t()], [y.t()]), ([x], [y.t().contiguous().t()])):
        with pytest.raises(ValueError, match="contiguous"):
            ema_update(a, b, [0], st, [0])
        with pytest.raises(ValueError, match="contiguous"):
            swap_tensors(a, b)
    for a, b in (([x.double()], [y.double()]), ([x], [y.half()]), ([x.int()], [y.int()])):
        with pytest.raises(TypeError, match="float32"):
            ema_update(a, b, [0], st, [0])
        with pytest.raises(TypeError, match="float32"):
            swap_tensors(a, b)
    with pytest.raises(ValueError, match="1 and 2 tensors"):
        swap_tensors([x], [y, y])
    with pytest.raises(ValueError):
        ema_update([x], [torch.randn(6, 4)], [0], st, [0])
    with pytest.raises(ValueError, match="group 32"):
        ema_update([x], [y], [32], st, [0])
    with pytest.raises(ValueError, match="active group 40"):
        ema_update([x], [y], [0], st, [40])
    with pytest.raises(ValueError, match="1 tensors, 2 group ids"):
        ema_update([x], [y], [0, 1], st, [0])
    assert st.count.tolist() == [0] * 32 and st.w.tolist() == [0.0] * 32, "a refused call must leave the words alone"


def test_the_holder_keeps_a_host_copy_of_its_words():
    st = WeightAverage("cpu")
    assert st.words.shape == (66,) and st.words.dtype == torch.int32 and st.count.shape == (32,) and st.w.shape == (32,)
    f32 = lambda v: float(np.float32(v))
    assert (st.decay_host, st.warmup_host) == (f32(0.999), True) and st.decay.tolist() == [f32(0.999)] and st.warmup.tolist() == [1]
    assert st.set_decay(0.5) is True and st.set_decay(0.5) is False and st.set_decay(warmup=True) is False
    assert st.decay.tolist() == [0.5] and st.warmup.tolist() == [1] and st.decay_host == 0.5
    assert st.set_decay(warmup=False) is True and st.warmup.tolist() == [0] and st.decay.tolist() == [0.5]
    for bad in (-0.1, 1.5, float("nan"), "0.9", True):
        with pytest.raises(ValueError, match="decay"):
            st.set_decay(bad)
        with pytest.raises(ValueError, match="decay"):
            WeightAverage("cpu", bad)
    assert st.decay.tolist() == [0.5] and st.decay_host == 0.5
    st.count[3] = 7                                                           # the views are the block's own words
    assert int(st.words[2 + 3]) == 7


# ---------------------------------------------------------------------------------------------- the arithmetic
def _tensors(seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=gen) * scale for s in ((7,), (3, 130), (1,), (2, 5, 9))]


@pytest.mark.parametrize("decay", [0.75, 1 - 2.0 ** -10])                     # fp32 numbers: 1 − decay is the same word in both
def test_without_warmup_it_is_torchs_ema_multi_avg_fn(decay):
    fn = torch.optim.swa_utils.get_ema_multi_avg_fn(decay)
    st = WeightAverage("cpu", decay, warmup=False)
    mine, theirs = _tensors(1), _tensors(1)
    for k in range(5):
        live = _tensors(10 + k, scale=10.0 ** (k - 2))
        before = [t.clone() for t in live]
        ema_update(mine, live, [0, 0, 5, 31], st, [0, 5, 31])
        fn(theirs, live, k + 1)
        assert all(torch.equal(a, b) for a, b in zip(live, before)), "the live tensors are only read"
        for i, (a, b) in enumerate(zip(mine, theirs)):
            assert torch.equal(a, b), f"update {k}, tensor {i}: off torch's by {float((a - b).abs().max()):.3e}"
    w = float(np.float32(1) - np.float32(decay))
    assert [st.count[g].item() for g in (0, 5, 31)] == [5, 5, 5] and int(st.count.sum()) == 15
    assert [st.w[g].item() for g in (0, 5, 31)] == [w, w, w] and float(st.w.sum()) == 3 * w


def test_with_warmup_the_weights_follow_the_formula():
    decay = 0.999
    st = WeightAverage("cpu", decay, warmup=True)
    avg, live = _tensors(2), _tensors(3)
    ref = [t.double() for t in avg]
    for t in range(12):
        ema_update(avg, live, [4] * 4, st, [4])
        want = 1.0 - min(decay, (1 + t) / (10 + t))
        got = float(st.w[4])
        assert abs(got - want) <= 8 * 2.0 ** -24, (t, got, want)
        assert int(st.count[4]) == t + 1
        ref = [r + got * (l.double() - r) for r, l in zip(ref, live)]
        for a, r, l in zip(avg, ref, live):                                   # the recurrence with the weight it reports
            bound = 3 * (t + 1) * 2.0 ** -24 * float(torch.maximum(r.abs(), l.abs().double()).max())
            assert float((a.double() - r).abs().max()) <= bound
    assert float(st.w[4]) > 1 - decay, "twelve updates are still warming up"
    st.set_decay(0.5)                                                         # below the warm-up's value: the decay decides
    ema_update(avg, live, [4] * 4, st, [4])
    assert float(st.w[4]) == 0.5


def test_an_inactive_group_and_a_skipped_step_keep_every_bit():
    st = WeightAverage("cpu", 0.9, warmup=False)
    avg, live = _tensors(4), _tensors(5)
    live[1][0, 0], live[3][0, 0, 0] = float("nan"), float("inf")
    groups = [0, 7, 7, 31]
    ema_update(avg, live, groups, st, [0, 31])                                # group 7 is not in the mask
    keep = [a.clone() for a in avg]
    assert st.count.tolist() == [1] + [0] * 30 + [1] and float(st.w[7]) == 0.0 and float(st.w[0]) == float(st.w[31]) > 0
    assert bool(torch.isfinite(avg[1]).all()) and bool(torch.isinf(avg[3]).any())
    guard = AnomalyGuard("cpu")
    guard.verdict.fill_(1)
    counts = st.count.clone()
    ema_update(avg, live, groups, st, [0, 7, 31], guard)                      # a step the guard skips: nothing moves
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(avg, keep))
    assert torch.equal(st.count, counts) and st.w.tolist() == [0.0] * 32
    guard.verdict.fill_(0)
    ema_update(avg, live, groups, st, 1 << 7, guard)                          # the mask as an integer
    assert st.count.tolist() == [1] + [0] * 6 + [1] + [0] * 23 + [1] and bool(torch.isnan(avg[1]).any())
    assert torch.equal(avg[0], keep[0]) and torch.equal(avg[3].view(torch.int32), keep[3].view(torch.int32))


def test_swap_exchanges_and_twice_is_the_identity():
    a, b = _tensors(6), _tensors(7)
    a[0][0], b[1][0, 0] = float("nan"), -0.0
    a0, b0 = [t.clone() for t in a], [t.clone() for t in b]
    bits = lambda ts: [t.view(torch.int32) for t in ts]
    swap_tensors(a, b)
    assert all(torch.equal(x, y) for x, y in zip(bits(a), bits(b0))) and all(torch.equal(x, y) for x, y in zip(bits(b), bits(a0)))
    swap_tensors(a, b)
    assert all(torch.equal(x, y) for x, y in zip(bits(a), bits(a0))) and all(torch.equal(x, y) for x, y in zip(bits(b), bits(b0)))


# ---------------------------------------------------------------------------------------------- the trainer's switch
class _Bare(fst.JointTrainer):
    """The mode switch without the networks (JointTrainer's constructor needs a GPU stream): every module a small CPU stand-in
    with parameters, fp32 BatchNorm buffers and an integer one."""

    def __init__(self):
        self.device = torch.device("cpu")
        self._graphs, self._phase = None, {}
        torch.manual_seed(0)
        self.m = {k: nn.Sequential(nn.Conv1d(1, 2, 3), nn.BatchNorm1d(2)) for k in self.MODULES}
        self.m["nf"].convinv = [nn.Identity(), nn.Identity()]


def test_enable_and_set_weight_average_arguments():
    T = fst.JointTrainer
    assert inspect.signature(T.__init__).parameters["weight_average"].default is None
    assert inspect.signature(fst.ClassifierTrainer.__init__).parameters["weight_average"].default is None
    assert len(T.MODULES) <= optim.MAX_GROUPS
    tr = _Bare()
    with pytest.raises(RuntimeError, match="enable_weight_average"):
        tr.set_weight_average(decay=0.9)
    with pytest.raises(RuntimeError, match="enable_weight_average"):
        tr.averaged_weights().__enter__()
    for bad in (-0.5, 1.01, float("nan"), "0.999"):
        with pytest.raises(ValueError, match="decay"):
            tr.enable_weight_average(decay=bad)
    assert tr.weight_average is None and tr._ema_avg == {}, "a refused call must not switch the mode on"
    for resident in (dict(_phase={"nf": object()}), dict(_graphs=[object()])):  # a phase capture, the joint capture
        other = _Bare()
        other.__dict__.update(resident)
        with pytest.raises(RuntimeError, match="capture is resident"):
            other.enable_weight_average()
        assert other.weight_average is None
    tr.enable_weight_average()
    st = tr.weight_average
    assert (st.decay_host, st.warmup_host) == (float(np.float32(0.999)), True)
    names = set(tr._ema_avg["nf"])
    assert names == {"0.weight", "0.bias", "1.weight", "1.bias", "1.running_mean", "1.running_var"}, "fp32 buffers yes, integer ones no"
    assert set(tr._ema_avg) == set(T.MODULES)
    for k in T.MODULES:
        for n, t in tr._ema_avg[k].items():
            live = tr.m[k].state_dict()[n]
            assert torch.equal(t, live) and t.data_ptr() != live.data_ptr()
    first = {n: t.data_ptr() for n, t in tr._ema_avg["nf"].items()}
    tr.enable_weight_average(decay=0.5, warmup=False)                         # idempotent: nothing changes
    assert tr.weight_average is st and st.decay_host == float(np.float32(0.999)) and st.warmup_host
    assert {n: t.data_ptr() for n, t in tr._ema_avg["nf"].items()} == first
    assert tr.set_weight_average(decay=0.5) is True and tr.set_weight_average(decay=0.5) is False
    assert st.decay.tolist() == [0.5] and st.warmup.tolist() == [1]
    for bad in (2.0, -1e-9, float("nan"), "x"):
        with pytest.raises(ValueError, match="decay"):
            tr.set_weight_average(decay=bad)
    assert st.decay.tolist() == [0.5], "a refused call must leave the decay alone"
    tr._phase = {"nf": object()}                                              # legal under a resident capture
    assert tr.set_weight_average(warmup=False) is True and st.warmup.tolist() == [0]


def test_averaged_weights_swaps_in_and_out_and_refuses_to_nest():
    tr = _Bare()
    tr.enable_weight_average(decay=0.75, warmup=False)
    live0 = {k: {n: t.clone() for n, t in tr.m[k].state_dict().items()} for k in tr.MODULES}
    with torch.no_grad():
        for k in tr.MODULES:
            for p in tr.m[k].parameters():
                p.add_(1.0)
            tr.m[k][1].running_mean.add_(2.0)
            tr.m[k][1].num_batches_tracked.add_(3)
    tr._ema_update(("nf", "fe_t"))
    rep = tr._ema_report()
    i_nf, i_fe = tr.MODULES.index("nf"), tr.MODULES.index("fe_t")
    assert rep["ema_weight"].tolist() == [0.25 if i in (i_nf, i_fe) else 0.0 for i in range(len(tr.MODULES))]
    assert rep["ema_steps"].tolist() == [int(i in (i_nf, i_fe)) for i in range(len(tr.MODULES))]
    live1 = {k: {n: t.clone() for n, t in tr.m[k].state_dict().items()} for k in tr.MODULES}
    inv = tr.m["nf"].convinv
    inv[0].W_inverse = stale = torch.eye(2)
    with tr.averaged_weights() as inside:
        assert inside is tr
        assert not hasattr(inv[0], "W_inverse"), "the live flow's cached inverse is set aside"
        inv[1].W_inverse = torch.zeros(2, 2)                                  # cached inside: belongs to the averaged weights
        for k in tr.MODULES:
            sd = tr.m[k].state_dict()
            moved = 0.25 if k in ("nf", "fe_t") else 0.0
            torch.testing.assert_close(sd["0.weight"], live0[k]["0.weight"] + moved, rtol=0, atol=1e-6)
            torch.testing.assert_close(sd["1.running_mean"], live0[k]["1.running_mean"] + 2 * moved, rtol=0, atol=1e-6)
            assert int(sd["1.num_batches_tracked"]) == 3, "an integer buffer stays the live one"
        with pytest.raises(RuntimeError, match="does not nest"):
            tr.averaged_weights().__enter__()
        for call in (lambda: tr.step(None, None, None, None), lambda: tr.phase_step("nf", None, None, None, None),
                     lambda: tr.replay(None, None, None, None, (0, 0)), lambda: tr.replay_phase("nf", None, None, None, None),
                     lambda: tr.capture(None, None, None, None), lambda: tr.capture_phase("nf", None, None, None, None),
                     tr.snapshot, tr.state_dict, lambda: tr.restore({}), lambda: tr.load_state_dict({})):
            with pytest.raises(RuntimeError, match="inside averaged_weights"):
                call()
    for k in tr.MODULES:
        for n, t in tr.m[k].state_dict().items():
            assert torch.equal(t, live1[k][n]), f"{k}.{n} is not what it was before the context"
    assert inv[0].W_inverse is stale and not hasattr(inv[1], "W_inverse")
    with ops.pack_cache():
        with pytest.raises(RuntimeError, match="pack_cache"):
            tr.averaged_weights().__enter__()
    good = tr._ema_live["nf"]["0.weight"]                                     # an exchange that is refused on entry changes nothing
    tr._ema_live["nf"]["0.weight"] = good.transpose(0, 1)
    with pytest.raises(ValueError, match="swap_tensors: pair"):
        tr.averaged_weights().__enter__()
    tr._ema_live["nf"]["0.weight"] = good
    assert inv[0].W_inverse is stale and not tr._ema_inside
    assert all(torch.equal(t, live1[k][n]) for k in tr.MODULES for n, t in tr.m[k].state_dict().items())
    with pytest.raises(ZeroDivisionError):                                    # an exception inside still swaps back
        with tr.averaged_weights():
            1 / 0
    assert torch.equal(tr.m["nf"].state_dict()["0.weight"], live1["nf"]["0.weight"]) and not tr._ema_inside


def test_the_checkpoint_entry_round_trips_in_place():
    tr = _Bare()
    tr.enable_weight_average(decay=0.75, warmup=False)
    with torch.no_grad():
        for p in tr.m["cpc"].parameters():
            p.mul_(3.0)
    tr._ema_update(("cpc",))
    entry = tr._ema_state_dict()
    assert entry["decay"] == 0.75 and entry["warmup"] is False and entry["counts"][tr.MODULES.index("cpc")] == 1
    assert sum(entry["counts"]) == 1 and len(entry["counts"]) == 32
    other = _Bare()
    other._ema_load_state_dict(entry)                                         # enables the mode
    st = other.weight_average
    assert st is not None and (st.decay_host, st.warmup_host) == (0.75, False) and st.count.tolist() == entry["counts"]
    ptrs = {(k, n): t.data_ptr() for k, d in other._ema_avg.items() for n, t in d.items()}
    for k, d in tr._ema_avg.items():
        for n, t in d.items():
            assert torch.equal(other._ema_avg[k][n], t)
    tr._ema_update(("cpc", "nf"))
    other._ema_load_state_dict(tr._ema_state_dict())                          # the second load: in place
    assert {(k, n): t.data_ptr() for k, d in other._ema_avg.items() for n, t in d.items()} == ptrs
    assert other.weight_average is st and st.count.tolist() == tr.weight_average.count.tolist()
