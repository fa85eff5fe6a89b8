"""The WN forward that no backward follows: fst_wn_layer_infer / fst_wn_stack_infer (csrc/wn_fused.hip: wn_layer_infer_kernel<4 | 8>,
wn_stack_infer_kernel — the saving kernels' tile body with the t,s / acts stores compiled out) and the route ``ops._wn_forward``
takes to them when nothing requires a gradient.

C-ABI cases follow tests/test_gpu_wn_routes.py, whose helpers are imported, not copied: inputs sit between NaN bands (a / u0 also
between NaN guard channels), outputs between canary bands and pre-filled with NaN, the route record is asserted after every launch,
every launch is repeated and must give the same bits, every refusal must leave every output untouched.

What is asserted is EQUALITY OF BITS with the saving launches on the same operands (``torch.equal``): the infer kernels run the same
instructions in the same order minus the stores, so there is no tolerance to choose.  One stack case is also held against the fp64
torch reference, layer by layer as test_wn_stack_fwd_vs_fp64 does (each layer against the fp64 layer applied to the input the
kernel itself handed on), at that test's gate — 2e-5 of max|want| for a_next and out — so that this file has an anchor that does not
go through the saving kernels.

tests/test_wn_infer_cpu.py checks, without a GPU, that the case lists below declare a case for every kernel instance the two
launchers can pick.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import pytest
import torch

from feature_level_style_transfer_for_tsc_amd import _lib, ops
from test_gpu_wn_routes import (DEV, LAYER_FWD, STACK_FWD, _cus, _gen, _layer_forward_f64, _layer_image, _layer_weights, assert_close,
                                assert_fence, assert_untouched, bf3_only, check_rc, last_route, layer_fwd_expect, nan_in, out_buf,
                                ptrs, rnd, wn_fwd_lds)

LAYER_INFER, STACK_INFER = ops.WN_ROUTE_LAYER_INFER, ops.WN_ROUTE_STACK_INFER
EXTRA = 2                 # NaN guard channels around the a / u0 slices: one before, one after


def layer_infer_expect(B: int, L: int, cus: int = 256):
    """The route record of fst_wn_layer_infer: that of fst_wn_layer_fwd on the same shape, under the infer family."""
    return (LAYER_INFER,) + layer_fwd_expect(B, L, cus)[1:]


def stack_infer_expect(B: int, L: int, nl: int, cus: int = 256):
    return (STACK_INFER, 8, 0, 0, 0, min(B, cus), 1, 1, L // 256, 3, nl, wn_fwd_lds(8))


def _batch(B, cus: int) -> int:
    """A case's batch size: a number, or "cus" / "cus+1" — the device's CU count (+ 1)."""
    return {"cus": cus, "cus+1": cus + 1}.get(B, B)


# --------------------------------------------------------------------------------------------------
# one layer: fst_wn_layer_infer against fst_wn_layer_fwd
# --------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Li:
    nw: int
    n: int
    h: int
    B: object           # int or "cus"
    L: int
    dil: int
    first: bool
    last: bool

    @property
    def id(self) -> str:
        return (f"nw{self.nw}-n{self.n}h{self.h}-B{self.B}L{self.L}d{self.dil}" + ("-first" if self.first else "") +
                ("-last" if self.last else ""))


_FORMS = [(f, l) for f in (True, False) for l in (True, False)]
# the 4-wave instance: L = 160 = 128 + 32 (a ragged last tile); dilation 1 and a dilation beyond the sequence (both outer taps read
# nothing but padding); n = 8 (one row block, mostly empty), 127 (the most the spare bias row allows), 120 (the metric width)
LI_CASES = [Li(4, n, h, 2, 160, dil, f, l) for (n, h) in ((8, 3), (127, 32), (120, 25)) for dil in (1, 256) for f, l in _FORMS]
# the 8-wave instance: as many 256-sample tiles as the device has CUs
LI_CASES += [Li(8, 8, 3, "cus", 256, 2, f, l) for f, l in _FORMS]


@bf3_only
@pytest.mark.gpu
@pytest.mark.parametrize("c", LI_CASES, ids=lambda c: c.id)
def test_wn_layer_infer_equals_the_saving_launch(c: Li):
    lib, g = _lib.load(), _gen("li" + c.id)
    n, h, L, B = c.n, c.h, c.L, _batch(c.B, _cus())
    route = layer_infer_expect(B, L, _cus())
    assert route[1] == c.nw
    w = _layer_weights(g, n, h, c.last)
    a64, u64, out0 = rnd(g, B, n, L), rnd(g, B, h, L), rnd(g, B, n, L)
    img = _layer_image(w, n, h, c.last)
    a, u0 = nan_in(a64, EXTRA, 1), nan_in(u64, EXTRA, 1)

    def run(infer: bool):
        o = {"out": out_buf((B, n, L), init=None if c.first else out0)}
        if not c.last:
            o["a_next"] = out_buf((B, n, L))
        if not infer:
            o["ts"] = out_buf((B, 2 * n, L))
        p = lambda k: o[k][1].data_ptr() if k in o else None
        head = (a.data_ptr(), (n + EXTRA) * L, u0.data_ptr(), (h + EXTRA) * L, img.data_ptr(), img.numel() * 4)
        tail = (int(c.first), int(c.last), B, L, n, h, c.dil, B * n * L, _lib.stream_ptr())
        if infer:
            check_rc(lib.fst_wn_layer_infer(*head, p("a_next"), p("out"), *tail), c.id)
            last_route(route, c.id)
        else:
            check_rc(lib.fst_wn_layer_fwd(*head, p("ts"), None, p("a_next"), p("out"), *tail), c.id)
            last_route((LAYER_FWD,) + route[1:], c.id + " (saving)")
        for k, (buf, v) in o.items():
            assert_fence(buf, v, k)
        return {k: v for k, (_, v) in o.items()}

    want, got = run(False), run(True)
    for k in got:
        assert not bool(torch.isnan(got[k]).any()), f"{k}: an element nobody wrote (or a NaN band that was read)"
        assert torch.equal(got[k], want[k]), f"{k}: fst_wn_layer_infer and fst_wn_layer_fwd differ"
    again = run(True)
    for k in got:
        assert torch.equal(again[k], got[k]), f"{k} differs between two identical launches"


# --------------------------------------------------------------------------------------------------
# a stack: fst_wn_stack_infer against the chain of fst_wn_layer_infer launches and against fst_wn_stack_fwd
# --------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Si:
    n: int
    h: int
    B: object           # int or "cus+1"
    L: int
    nl: int

    @property
    def id(self) -> str:
        return f"n{self.n}h{self.h}-B{self.B}L{self.L}-nl{self.nl}"


# nl = 1, 2, 3, 8: no a_next at all, one, and chains that end in either of the two alternating buffers; B = CUs + 1: one workgroup
# walks two batch elements; L = 512: two tiles per sequence and layer; the metric shape
SI_CASES = [Si(8, 3, "cus+1", 256, nl) for nl in (1, 2, 3, 8)] + [Si(16, 5, 3, 512, 3), Si(120, 25, 256, 512, 8)]


def _stack_operands(c: Si, B: int):
    g = _gen("si" + c.id)
    ws = [_layer_weights(g, c.n, c.h, i == c.nl - 1) for i in range(c.nl)]
    imgs = [_layer_image(w, c.n, c.h, i == c.nl - 1) for i, w in enumerate(ws)]
    a0_64, u64 = rnd(g, B, c.n, c.L), rnd(g, B, c.h, c.L)
    return ws, imgs, a0_64, u64, nan_in(a0_64), nan_in(u64, EXTRA, 1)


def _stack_infer_call(lib, a_in, imgs, u0, out, nl, B, L, n, h, numel=None, a_next=None, L_arg=None):
    bs = (ctypes.c_int64 * nl)(*([n * L] * nl))
    a_next = list(a_in[1:]) + [None] if a_next is None else a_next
    return lib.fst_wn_stack_infer(ptrs(a_in), bs, ptrs(imgs), imgs[0].numel() * 4, ptrs(a_next), u0.data_ptr(), (h + EXTRA) * L, out.data_ptr(),
                                  nl, B, L if L_arg is None else L_arg, n, h, B * n * L if numel is None else numel, _lib.stream_ptr())


@bf3_only
@pytest.mark.gpu
@pytest.mark.parametrize("c", SI_CASES, ids=lambda c: c.id)
def test_wn_stack_infer_equals_the_layer_chain_and_the_saving_stack(c: Si):
    lib = _lib.load()
    n, h, L, nl, B = c.n, c.h, c.L, c.nl, _batch(c.B, _cus())
    assert lib.fst_wn_stack_fwd_ok(n, h, L, nl) == 1
    ws, imgs, a0_64, u64, a0, u0 = _stack_operands(c, B)
    a0_before = a0.clone()
    route = stack_infer_expect(B, L, nl, _cus())

    def alternating(first=None):
        """(buffers, a_in): layer inputs a0, X, Y, X, ... — or, given ``first`` (an output buffer holding a copy of a0), first, X,
        first, X, ...: the two tensors ``ops._wn_forward`` alternates, the start conv's output being overwritten by layer 1."""
        if first is None:
            pair = [out_buf((B, n, L)) for _ in range(min(nl - 1, 2))]
            return pair, [a0] + [pair[(i - 1) % 2][1] for i in range(1, nl)]
        pair = [first] + [out_buf((B, n, L)) for _ in range(min(nl - 1, 1))]
        return pair, [pair[i % 2][1] for i in range(nl)]

    def stack_infer(first=None):
        bufs, a_in = alternating(first)
        bo, out = out_buf((B, n, L))
        check_rc(_stack_infer_call(lib, a_in, imgs, u0, out, nl, B, L, n, h), c.id)
        last_route(route, c.id)
        for k, (buf, v) in enumerate(bufs + [(bo, out)]):
            assert_fence(buf, v, f"output {k}")
        return out, a_in[nl - 1]

    def layer_chain():
        bufs, a_in = alternating()
        bo, out = out_buf((B, n, L))
        for i in range(nl):
            last = i == nl - 1
            check_rc(lib.fst_wn_layer_infer(a_in[i].data_ptr(), n * L, u0.data_ptr(), (h + EXTRA) * L, imgs[i].data_ptr(), imgs[i].numel() * 4,
                                            None if last else a_in[i + 1].data_ptr(), out.data_ptr(), int(i == 0), int(last), B, L, n, h,
                                            1 << i, B * n * L, _lib.stream_ptr()), f"layer {i}")
            last_route(layer_infer_expect(B, L, _cus()), f"layer {i}")
        for k, (buf, v) in enumerate(bufs + [(bo, out)]):
            assert_fence(buf, v, f"output {k}")
        return out, a_in[nl - 1]

    def saving_stack():
        ts = [out_buf((B, 2 * n, L)) for _ in range(nl)]
        an = [out_buf((B, n, L)) for _ in range(nl - 1)]
        bo, out = out_buf((B, n, L))
        a_in = [a0] + [v for _, v in an]
        bs = (ctypes.c_int64 * nl)(*([n * L] * nl))
        check_rc(lib.fst_wn_stack_fwd(ptrs(a_in), bs, ptrs(imgs), imgs[0].numel() * 4, ptrs([v for _, v in ts]),
                                      ptrs([v for _, v in an] + [None]), u0.data_ptr(), (h + EXTRA) * L, out.data_ptr(), nl, B, L, n, h,
                                      B * n * L, _lib.stream_ptr()), "saving stack")
        last_route((STACK_FWD,) + route[1:], "saving stack")
        return out, a_in[nl - 1]

    out, a_last = stack_infer()
    assert not bool(torch.isnan(out).any()), "out: an element nobody wrote (or a NaN band that was read)"
    assert torch.equal(a0, a0_before), "the stack's input was written"
    for what, (o2, a2) in (("the chain of fst_wn_layer_infer launches", layer_chain()), ("fst_wn_stack_fwd", saving_stack()),
                           ("a second identical launch", stack_infer())):
        assert torch.equal(out, o2), f"out differs from {what}"
        assert torch.equal(a_last, a2), f"the last layer's input differs from {what}"
    # two tensors in alternation, the first holding the input (a_next[1] = a_in[0]): what ops._wn_forward passes
    o3, _ = stack_infer(first=out_buf((B, n, L), init=a0))
    assert torch.equal(out, o3), "out differs when layer 1 overwrites the stack's input"
    assert torch.equal(a0, a0_before)


@bf3_only
@pytest.mark.gpu
def test_wn_stack_infer_vs_fp64():
    """Every layer has a buffer of its own here (allowed: the alternation is an option), so each layer is checked against the fp64
    layer applied to the input the kernel itself handed on; ``out`` against the fp64 sum of those layers' skip rows."""
    lib = _lib.load()
    c = Si(16, 5, 3, 512, 3)
    n, h, L, nl, B = c.n, c.h, c.L, c.nl, c.B
    ws, imgs, a0_64, u64, a0, u0 = _stack_operands(c, B)
    an = [out_buf((B, n, L)) for _ in range(nl - 1)]
    bo, out = out_buf((B, n, L))
    a_in = [a0] + [v for _, v in an]
    check_rc(_stack_infer_call(lib, a_in, imgs, u0, out, nl, B, L, n, h), c.id)
    last_route(stack_infer_expect(B, L, nl, _cus()), c.id)
    for k, (buf, v) in enumerate(an + [(bo, out)]):
        assert_fence(buf, v, f"output {k}")
    want_out = 0
    for i in range(nl):
        a_i = a0_64 if i == 0 else a_in[i].double()
        _, _, _, res, skip = _layer_forward_f64(ws[i], a_i, u64, 1 << i, i == nl - 1)
        if i < nl - 1:
            assert_close(a_in[i + 1], a_i + res, 2e-5, f"layer {i} a_next")
        want_out = want_out + skip
    assert_close(out, want_out, 2e-5, "out")


def _refused(lib, rc: int, name: bytes, outputs, what: str):
    assert rc == -1, f"{what}: rc={rc}"
    assert ops.wn_last_route() == (0,) * ops.WN_ROUTE_LEN, what
    assert name in lib.fst_last_error(), f"{what}: {lib.fst_last_error()}"
    torch.cuda.synchronize()
    for k, (buf, v) in enumerate(outputs):
        assert_untouched(buf, v, f"{what}: output {k}")


@bf3_only
@pytest.mark.gpu
def test_wn_stack_infer_refusals_write_nothing():
    lib = _lib.load()
    c = Si(8, 3, 2, 256, 3)
    n, h, L, nl, B = c.n, c.h, c.L, c.nl, c.B
    ws, imgs, a0_64, u64, a0, u0 = _stack_operands(c, B)
    x, y, o = out_buf((B, n, L)), out_buf((B, n, L)), out_buf((B, n, L))
    outs = [x, y, o]
    a_in = [a0, x[1], y[1]]
    call = lambda **kw: _stack_infer_call(lib, kw.pop("a_in", a_in), kw.pop("imgs", imgs), u0, o[1], nl, B, L, n, h, **kw)
    name = b"fst_wn_stack_infer"
    _refused(lib, call(imgs=[imgs[0], None, imgs[2]]), name, outs, "null image")
    _refused(lib, call(a_in=[a0, None, y[1]], a_next=[x[1], y[1], None]), name, outs, "null layer input")
    _refused(lib, call(a_next=[x[1], None, None]), name, outs, "null a_next below the top layer")
    _refused(lib, call(a_in=[a0, x[1], x[1]]), name, outs, "a_next[1] == a_in[1]")
    _refused(lib, call(a_in=[a0, a0, y[1]]), name, outs, "a_next[0] == a_in[0]")
    _refused(lib, call(a_next=[y[1], x[1], None]), name, outs, "a broken chain")
    _refused(lib, call(numel=B * n * L + 1), name, outs, "element count")
    _refused(lib, call(L_arg=L // 2, numel=B * n * L // 2), name, outs, "L % 256 != 0")

    class Off:                                                 # a tensor's address, 4 bytes on
        def __init__(self, t): self.t = t
        def data_ptr(self): return self.t.data_ptr() + 4
    _refused(lib, call(a_in=[Off(a0), x[1], y[1]]), name, outs, "misaligned input")
    _refused(lib, call(a_in=[a0, Off(x[1]), y[1]], a_next=[Off(x[1]), y[1], None]), name, outs, "misaligned a_next")
    # and the call the refusals were variations of goes through
    check_rc(call(), "the unmodified call")
    last_route(stack_infer_expect(B, L, nl, _cus()), "the unmodified call")


@bf3_only
@pytest.mark.gpu
def test_wn_layer_infer_refusals_write_nothing():
    lib, g = _lib.load(), _gen("li-refusals")
    n, h, B, L = 8, 3, 2, 160
    w = _layer_weights(g, n, h, False)
    img = _layer_image(w, n, h, False)
    a, u0 = nan_in(rnd(g, B, n, L)), nan_in(rnd(g, B, h, L))
    an, o = out_buf((B, n, L)), out_buf((B, n, L))
    outs = [an, o]

    def call(a_ptr=a.data_ptr(), an_ptr=an[1].data_ptr(), numel=B * n * L, nbytes=img.numel() * 4, last=0, L_=L):
        return lib.fst_wn_layer_infer(a_ptr, n * L, u0.data_ptr(), h * L, img.data_ptr(), nbytes, an_ptr, o[1].data_ptr(), 1, last, B, L_, n, h, 4,
                                      numel, _lib.stream_ptr())
    name = b"fst_wn_layer_infer"
    _refused(lib, call(an_ptr=a.data_ptr()), name, outs, "a_next == a")
    _refused(lib, call(an_ptr=None), name, outs, "no a_next below the top layer")
    _refused(lib, call(numel=B * n * L - 1), name, outs, "element count")
    _refused(lib, call(nbytes=img.numel() * 4 - 16), name, outs, "short image")
    _refused(lib, call(a_ptr=a.data_ptr() + 4), name, outs, "misaligned a")
    _refused(lib, call(an_ptr=an[1].data_ptr() + 8), name, outs, "misaligned a_next")
    check_rc(call(), "the unmodified call")
    last_route(layer_infer_expect(B, L, _cus()), "the unmodified call")


# --------------------------------------------------------------------------------------------------
# the module surface: WaveGlow.forward / infer and WN.forward pick the route by themselves
# --------------------------------------------------------------------------------------------------
def _waveglow(n_group: int, n: int, seed: int):
    from feature_level_style_transfer_for_tsc_amd import WaveGlow
    torch.manual_seed(seed)
    wg = WaveGlow(3, n_group, n).to(DEV)
    for wn in wg.WN:
        wn.end.weight.data.normal_(0, 0.05); wn.end.bias.data.normal_(0, 0.05)
    return wg


def _timed_keys(fn):
    timer = ops.KernelTimer()
    ops.KERNEL_TIMER = timer
    try:
        res = fn()
    finally:
        ops.KERNEL_TIMER = None
    return res, set(timer.summary())


def _round_trip(wg, x):
    z, log_s, _ = wg(x)
    return [z.detach(), wg.infer(z.detach()).detach()] + [s.detach() for s in log_s]


# (B, n_group, n, L): the metric widths on the per-layer route; a shape of the one-launch route (B >= 256, B·L/256 >= 512) with few rows
MODULE_SHAPES = [(3, 50, 120, 128, "layer"), (256, 6, 8, 512, "stack")]


@bf3_only
@pytest.mark.gpu
@pytest.mark.parametrize("B,C,n,L,kind", MODULE_SHAPES, ids=lambda v: str(v))
def test_waveglow_without_grad_takes_the_infer_kernels_and_returns_the_same_bits(B, C, n, L, kind, monkeypatch):
    monkeypatch.delenv("FST_WN_INFER", raising=False)
    assert ops.wn_stack_fwd_ok(n, C // 2, L, 8, B) == (kind == "stack")
    wg = _waveglow(C, n, 11)
    x = torch.randn(B, C, L, device=DEV)
    saving, infer = f"wn_{kind}_fwd_kernel", f"wn_{kind}_infer_kernel"
    want, keys = _timed_keys(lambda: _round_trip(wg, x))                      # grad mode on, parameters require a gradient
    assert saving in keys and infer not in keys, sorted(keys)
    with torch.no_grad():
        got, keys = _timed_keys(lambda: _round_trip(wg, x))
    assert infer in keys and not any(k.startswith(("wn_layer_fwd_kernel", "wn_stack_fwd_kernel")) for k in keys), sorted(keys)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"tensor {i} of (z, inverse, log_s...) differs between no_grad and grad mode"
    # a grad-requiring input under frozen weights: the saving launches; frozen weights and a detached input: the infer kernels
    for p in wg.parameters():
        p.requires_grad_(False)
    _, keys = _timed_keys(lambda: wg(x.clone().requires_grad_(True)))
    assert saving in keys and infer not in keys, sorted(keys)
    got, keys = _timed_keys(lambda: _round_trip(wg, x))
    assert infer in keys and saving not in keys, sorted(keys)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # FST_WN_INFER=0: the saving launches whatever requires a gradient
    monkeypatch.setenv("FST_WN_INFER", "0")
    with torch.no_grad():
        got, keys = _timed_keys(lambda: _round_trip(wg, x))
    assert saving in keys and infer not in keys, sorted(keys)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@bf3_only
@pytest.mark.gpu
def test_wn_module_forward_without_grad_equals_with_grad():
    from feature_level_style_transfer_for_tsc_amd.waveglow import WN
    torch.manual_seed(4)
    wn = WN(25, 8, 120, 3).to(DEV)
    wn.end.weight.data.normal_(0, 0.05); wn.end.bias.data.normal_(0, 0.05)
    u0 = torch.randn(3, 25, 132, device=DEV)
    want, keys = _timed_keys(lambda: wn(u0).detach())
    assert "wn_layer_fwd_kernel" in keys
    with torch.no_grad():
        got, keys = _timed_keys(lambda: wn(u0))
    assert "wn_layer_infer_kernel" in keys and "wn_layer_fwd_kernel" not in keys, sorted(keys)
    assert torch.equal(got, want)


@bf3_only
@pytest.mark.gpu
def test_a_captured_no_grad_pass_replays_to_the_eager_bits():
    wg = _waveglow(50, 120, 12)
    x = torch.randn(3, 50, 128, device=DEV)
    x2 = torch.randn(3, 50, 128, device=DEV)
    with torch.no_grad():
        want, want2 = _round_trip(wg, x), _round_trip(wg, x2)      # (also loads every code object and caches the 1x1 inverses)
        static = x.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _round_trip(wg, static)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            got = _round_trip(wg, static)
    for src, ref in ((x, want), (x2, want2), (x, want)):
        static.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a, b), f"tensor {i}: the replay differs from the eager pass"


@bf3_only
@pytest.mark.gpu
def test_a_forward_without_grad_keeps_a_fraction_of_the_memory(monkeypatch):
    """B = 8, n = 120, h = 25, L = 512, 8 layers.  In [B, n, L] units (1.97 MB): with a backward to come the pass allocates 8 layer
    inputs, 8 gate-half tensors of two units each and out — 25 — plus the [B, 2h, L] output and the weight images (8 × 0.5 MB, the
    same in both passes); without, two alternating layer inputs and out.  The bound is the issue's: less than half."""
    monkeypatch.delenv("FST_WN_INFER", raising=False)
    h, n, nl, B, L = 25, 120, 8, 8, 512
    S = ops.WNSpecs(h, n, nl)
    g = torch.Generator(device=DEV).manual_seed(7)
    flat = S.flatten([torch.randn(*sh, generator=g, device=DEV) * (0.05 if len(sh) == 3 else 0.1) for sh in S.shapes])
    u0 = torch.randn(B, h, L, generator=g, device=DEV)
    ops.WNFn.apply(S, u0, flat)                                      # conv plans, code objects: not part of either rise
    torch.cuda.synchronize()

    def rise(u):
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        o = ops.WNFn.apply(S, u, flat)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, o.detach()

    unit = B * n * L * 4
    with_grad, o1 = rise(u0.clone().requires_grad_(True))
    without, o2 = rise(u0)
    print(f"  rise with grad {with_grad / unit:.2f} units, without {without / unit:.2f} units of {unit} bytes")
    assert torch.equal(o1, o2)
    assert without < 0.5 * with_grad, (without, with_grad)
