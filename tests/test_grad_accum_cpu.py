"""Host side of the device gradient accumulation (no GPU): the new symbol in header, ctypes table and library; the launcher's and
the wrappers' refusals; the arithmetic of ``optim.accumulate``'s CPU branch against a numpy float32 recurrence, bit for bit, and
against the fp64 mean within the bound the definition gives; the host mirror of the window; and the trainers' switch.  The kernel
and the trainers' steps are tested in test_gpu_grad_accum.py.

The bound.  The fold is k − 1 fp32 additions of partial sums, one rounding of 1/k to fp32 and one fp32 multiplication, so the
closing gradient lies within (k + 2) · 2⁻²⁴ · Σ_j |g_j| / k + 2⁻¹⁴⁹ of the exact mean (every partial sum is at most Σ|g_j| in
magnitude; the last term is half the smallest denormal, for a product that underflows)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import _lib
from feature_level_style_transfer_for_tsc_amd.optim import GradAccumulation, accumulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 130                                                                      # entries of a call: three launches' worth
KS = (1, 2, 3, 5)


def test_header_binding_and_library_agree_on_the_new_symbol():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fst_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+fst_accum_multi\s*\(([^;]*)\)\s*;", text)
    assert decl, "fst_accum_multi is not declared in include/fst_hip.h"
    res, args = _lib._SIGNATURES["fst_accum_multi"]
    assert res is _lib.c_int and len(args) == decl.group(1).count(",") + 1 == 7, "the ctypes table and the header disagree"
    assert "fst_accum_multi" in _lib.EXPORTED_SYMBOLS
    version = int(re.search(r"#define\s+FST_ABI_VERSION\s+(\d+)", text).group(1))
    assert version == _lib.ABI_VERSION >= 24
    lib = _lib.load()
    assert lib.fst_version() == version and hasattr(lib, "fst_accum_multi")
    assert all(hasattr(fst, k) for k in ("GradAccumulation", "accumulate"))
    # refused on the host before any launch (there is no device here: a launch would return another code)
    assert lib.fst_accum_multi(None, None, None, 1, None, 1, None) == -1 and lib.fst_last_error()


def _call(at=None, a=None, b=None, numel=None, state_off=0, state="words", advance=1):
    """The launcher on 130 made-up entries, of which entry ``at`` is changed into one it must REFUSE (nothing here may reach a
    launch: these are no device pointers); the state block is a 16-byte aligned run of host words that is never dereferenced."""
    lib = _lib.load()
    A = [0x100000 + 4096 * i for i in range(N)]
    B = [0x900000 + 4096 * i for i in range(N)]
    ne = [8 + i for i in range(N)]
    if at is not None:
        for lst, v in ((A, a), (B, b), (ne, numel)):
            if v is not None:
                lst[at] = v if v != "null" else None
    raw = np.zeros(24, dtype=np.int32)
    first = (-raw.ctypes.data % 16) // 4                                      # the first word on a 16-byte boundary
    words = raw[first: first + 8]
    words[:] = (3, 1, 0, 5, 0, 0, 0, 0)
    assert words.ctypes.data % 16 == 0
    arrays = ((ctypes.c_void_p * N)(*A), (ctypes.c_void_p * N)(*B), (ctypes.c_int64 * N)(*ne))
    rc = lib.fst_accum_multi(*arrays, N, None if state is None else words.ctypes.data + state_off, advance, None)
    assert words.tolist() == [3, 1, 0, 5, 0, 0, 0, 0], "a refused call wrote into the state block"
    return rc


BAD = [("null accumulator", dict(a="null")), ("null gradient", dict(b="null")), ("accumulator 2 bytes off", dict(a=0x100002)),
       ("gradient 1 byte off", dict(b=0x900001)), ("no elements", dict(numel=0)), ("2^31 elements", dict(numel=2 ** 31))]


@pytest.mark.parametrize("at", [0, 64, N - 1], ids=["first", "middle", "last"])
@pytest.mark.parametrize("what, entry", BAD, ids=[w for w, _ in BAD])
def test_launcher_refuses_a_bad_entry_on_the_host(what, entry, at):
    assert _call(at, **entry) == -1, what
    assert f"tensor {at}:".encode() in _lib.load().fst_last_error()


def test_launcher_refuses_overlapping_pairs_and_bad_state_pointers():
    lib = _lib.load()
    assert _call(64, b=0x100000 + 4096 * 64 + 16) == -1 and b"overlap" in lib.fst_last_error()   # the gradient starts inside its accumulator
    assert _call(N - 1, a=0x900000 + 4096 * (N - 1) - 8) == -1 and b"overlap" in lib.fst_last_error()
    assert _call(state=None) == -1 and b"state" in lib.fst_last_error()
    for off in (4, 8, 12, 2):
        assert _call(state_off=off) == -1 and b"state" in lib.fst_last_error(), f"a state block {off} bytes off a 16-byte boundary"
    assert _call(state=None, advance=0) == -1
    assert lib.fst_accum_multi(None, None, None, 0, None, 1, None) == -1, "no tensors, but the advance needs its words"
    assert lib.fst_accum_multi(None, None, None, -1, 4096, 1, None) == -1
    assert lib.fst_accum_multi(None, None, None, 3, 4096, 1, None) == -1, "three tensors and no arrays"


# ---------------------------------------------------------------------------------------------- the arithmetic
SHAPES = ((7,), (3, 130), (1,), (2, 5, 9), ())


def _grads(seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=gen) * scale for s in SHAPES]


def recurrence(gs, k):
    """The definition in numpy float32: the accumulator after every call of a window and the closing gradient."""
    acc = None
    for g in gs:
        acc = g.astype(np.float32) if acc is None else (acc + g).astype(np.float32)
    return acc, (acc * (np.float32(1.0) / np.float32(k))).astype(np.float32)


@pytest.mark.parametrize("k", KS)
def test_cpu_branch_is_the_float32_recurrence_and_within_the_bound_of_the_mean(k):
    st = GradAccumulation("cpu", k)
    assert float(st.inv_k) == float(np.float32(1.0) / np.float32(k))
    acc = [torch.full(s, float("nan")) for s in SHAPES]                       # never read when a window opens: no zero fill
    for window in range(2):
        micro = [_grads(100 * window + j, scale=10.0 ** (j - 1)) for j in range(k)]
        for j, gs in enumerate(micro):
            before = [g.clone() for g in gs]
            keep = [a.clone() for a in acc]
            accumulate(acc, gs, st)
            if k == 1:
                assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(acc, keep)), "k = 1 touches nothing"
            if j < k - 1 or k == 1:
                assert all(torch.equal(g, b) for g, b in zip(gs, before)), "a gradient is only read before the closing call"
            assert int(st.j) == st.pending == (j + 1) % k and int(st.windows) == window + (j + 1) // k
        if k == 1:
            continue
        for i in range(len(SHAPES)):
            want_acc, want_g = recurrence([m[i].numpy() if j < k - 1 else before[i].numpy() for j, m in enumerate(micro)], k)
            assert np.array_equal(acc[i].numpy().view(np.int32), want_acc.view(np.int32)), f"window {window}, tensor {i}: accumulator"
            assert np.array_equal(micro[-1][i].numpy().view(np.int32), want_g.view(np.int32)), f"window {window}, tensor {i}: mean"
            parts = [m[i].double() if j < k - 1 else before[i].double() for j, m in enumerate(micro)]
            mean, mass = sum(parts) / k, sum(p.abs() for p in parts) / k
            err = (micro[-1][i].double() - mean).abs()
            assert bool((err <= (k + 2) * 2.0 ** -24 * mass + 2.0 ** -149).all()), f"window {window}, tensor {i}: {float(err.max()):.3e}"


def test_non_finite_values_go_the_way_ieee_sends_them():
    st = GradAccumulation("cpu", 3)
    nan, inf = float("nan"), float("inf")
    micro = [torch.tensor([1.0, inf, 2.0, nan, -inf, 3.0]), torch.tensor([1.0, 1.0, -inf, 1.0, inf, 3.0]), torch.tensor([1.0, -inf, 0.0, 0.0, 0.0, inf])]
    acc = [torch.empty(6)]
    for g in micro:
        accumulate(acc, [g], st)
    got = micro[-1]
    assert float(got[0]) == float(np.float32(3.0) * (np.float32(1) / np.float32(3)))
    assert bool(torch.isnan(got[1])) and float(got[2]) == -inf and bool(torch.isnan(got[3])) and bool(torch.isnan(got[4])) and float(got[5]) == inf


def test_several_calls_without_advance_fold_at_one_position():
    st = GradAccumulation("cpu", 2)
    a, b = [torch.empty(4)], [torch.empty(3)]
    g1, h1, g2, h2 = torch.ones(4), torch.full((3,), 2.0), torch.full((4,), 3.0), torch.full((3,), 6.0)
    accumulate(a, [g1], st, advance=False)
    assert st.pending == 0 and int(st.j) == 0
    accumulate(b, [h1], st, advance=True)
    assert st.pending == 1 and int(st.j) == 1 and int(st.windows) == 0
    accumulate(a, [g2], st, advance=False)
    accumulate(b, [h2], st)
    assert st.pending == 0 and st.words.tolist()[:2] == [2, 0] and int(st.windows) == 1
    assert g2.tolist() == [2.0] * 4 and h2.tolist() == [4.0] * 3 and g1.tolist() == [1.0] * 4
    accumulate([], [], st)                                                    # the advance alone
    assert st.pending == 1 and int(st.j) == 1


# ---------------------------------------------------------------------------------------------- the holder and the wrappers
def test_the_holder_keeps_a_host_copy_of_its_words():
    st = GradAccumulation("cpu")
    assert st.words.shape == (8,) and st.words.dtype == torch.int32 and st.words.data_ptr() % 16 == 0
    assert (st.steps_host, st.pending) == (1, 0) and st.words.tolist() == [1, 0, 0x3F800000, 0, 0, 0, 0, 0]
    assert st.set_steps(4) is True and st.set_steps(4) is False
    assert st.steps_host == 4 and st.k.tolist() == [4] and st.inv_k.tolist() == [0.25] and st.words[3:].tolist() == [0] * 5
    for bad in (0, -2, 2.0, "3", True, None, 1 << 24):
        with pytest.raises(ValueError, match="steps"):
            st.set_steps(bad)
        with pytest.raises(ValueError, match="steps"):
            GradAccumulation("cpu", bad)
    assert st.k.tolist() == [4] and st.steps_host == 4
    g = [torch.ones(3)]
    accumulate([torch.empty(3)], g, st)
    assert st.pending == 1
    with pytest.raises(RuntimeError, match="window is open"):
        st.set_steps(2)
    with pytest.raises(RuntimeError, match="window is open"):
        st.set_steps(4)                                                       # refused mid-window whatever the value
    assert st.words.tolist()[:2] == [4, 1] and st.steps_host == 4
    for _ in range(3):
        assert not st.pending == 0
        accumulate([torch.empty(3)], g, st)
    assert st.pending == 0 and st.set_steps(2) is True and st.words.tolist()[:4] == [2, 0, 0x3F000000, 1]


def test_wrapper_refuses_what_the_kernel_cannot_take():
    st = GradAccumulation("cpu", 2)
    x, y = torch.randn(4, 6), torch.randn(4, 6)
    for a, b in (([x.t()], [y.t()]), ([x], [y.t().contiguous().t()])):
        with pytest.raises(ValueError, match="contiguous"):
            accumulate(a, b, st)
    for a, b in (([x.double()], [y.double()]), ([x], [y.half()]), ([x.int()], [y.int()])):
        with pytest.raises(TypeError, match="float32"):
            accumulate(a, b, st)
    with pytest.raises(ValueError, match="1 and 2 tensors"):
        accumulate([x], [y, y], st)
    with pytest.raises(ValueError):
        accumulate([x], [torch.randn(6, 4)], st)
    with pytest.raises(ValueError, match="device"):
        accumulate([x.to("meta")], [y.to("meta")], st)
    assert st.pending == 0 and st.words.tolist()[:4] == [2, 0, 0x3F000000, 0], "a refused call must leave the words alone"


# ---------------------------------------------------------------------------------------------- the trainers' switch
class _Bare(fst.JointTrainer):
    """The mode switch without the networks (JointTrainer's constructor needs a GPU stream)."""

    def __init__(self):
        self.device = torch.device("cpu")
        self._graphs, self._phase = None, {}
        self.sync, self.bucket = "ddp", None
        torch.manual_seed(0)
        self.m = {k: nn.Sequential(nn.Conv1d(1, 2, 3), nn.BatchNorm1d(2)) for k in self.MODULES}


class _BareClassifier(fst.ClassifierTrainer):
    def __init__(self):
        self.device = torch.device("cpu")
        self._graph = None


@pytest.mark.parametrize("bare", [_Bare, _BareClassifier])
def test_enable_and_set_grad_accumulation(bare):
    T = type(bare()).__mro__[1]
    assert inspect.signature(T.__init__).parameters["grad_accumulation"].default is None
    tr = bare()
    assert tr.grad_accumulation is None and tr.accum_pending == 0
    with pytest.raises(RuntimeError, match="enable_grad_accumulation"):
        tr.set_grad_accumulation(2)
    for bad in (0, -1, 1.5, "2"):
        with pytest.raises(ValueError, match="steps"):
            tr.enable_grad_accumulation(bad)
    assert tr.grad_accumulation is None, "a refused call must not switch the mode on"
    residents = (dict(_phase={"nf": object()}), dict(_graphs=[object()])) if bare is _Bare else (dict(_graph=object()),)
    for resident in residents:
        other = bare()
        other.__dict__.update(resident)
        with pytest.raises(RuntimeError, match="capture is resident"):
            other.enable_grad_accumulation(2)
        assert other.grad_accumulation is None
    tr.enable_grad_accumulation(3)
    st = tr.grad_accumulation
    assert st.steps_host == 3 and st.k.tolist() == [3]
    tr.enable_grad_accumulation(5)                                            # idempotent: nothing changes, the argument included
    assert tr.grad_accumulation is st and st.steps_host == 3
    assert tr.set_grad_accumulation(2) is True and tr.set_grad_accumulation(2) is False and st.k.tolist() == [2]
    tr.__dict__.update(residents[0])                                          # legal under a resident capture
    assert tr.set_grad_accumulation(4) is True and st.inv_k.tolist() == [0.25]
    # a window opens: the fold makes the accumulators, keyed by parameter, and they keep their addresses
    params = [nn.Parameter(torch.randn(3, 2)), nn.Parameter(torch.randn(5)), nn.Parameter(torch.randn(2))]
    params[0].grad, params[1].grad = torch.randn(3, 2), torch.randn(5, 7)[:, 0]   # the second: not contiguous; the third: no gradient
    tr._accum_fold(params, advance=True)
    assert tr.accum_pending == 1 and set(tr._accum) == set(params[:2]) and params[1].grad.is_contiguous()
    ptrs = {p: a.data_ptr() for p, a in tr._accum.items()}
    with pytest.raises(RuntimeError, match="window is open"):
        tr.set_grad_accumulation(2)
    for _ in range(3):
        tr._accum_fold(params, advance=True)
    assert tr.accum_pending == 0 and {p: a.data_ptr() for p, a in tr._accum.items()} == ptrs
    assert torch.equal(tr._accum[params[0]] * 0.25, params[0].grad)


def test_state_methods_and_captures_refuse_an_open_window():
    tr = _Bare()
    tr.enable_grad_accumulation(2)
    tr._accum_fold([], advance=True)
    assert tr.accum_pending == 1
    for call in (tr.snapshot, tr.state_dict, lambda: tr.save_state(os.devnull), lambda: tr.load_state_dict({}),
                 lambda: tr.capture(None, None, None, None), lambda: tr.capture_phase("nf", None, None, None, None, warmup=1),
                 lambda: tr.replay_phase("nf", None, None, None, None)):
        with pytest.raises(RuntimeError, match="window is open"):
            call()
    tr._accum_fold([], advance=True)
    assert tr.accum_pending == 0
    for call in (lambda: tr.capture_phase("nf", None, None, None, None), lambda: tr.replay_phase("nf", None, None, None, None)):
        with pytest.raises(RuntimeError, match=r"phase_step\(\)"):            # between windows: captured phases do not accumulate
            call()
