"""No kernel swallows a non-finite value, and none spreads one.

Every other GPU module compares a kernel with fp64 on FINITE data between NaN and canary bands.  Here one element INSIDE an
operand (an activation or a cotangent, never a weight) is NaN, +inf or -inf, and the op — called through ``ops.py``'s autograd
functions and launch helpers, so the routing is exercised too — is held to three rules by ``check_nonfinite``:

* no swallowing — wherever the fp64 CPU composition of a poisoned run is non-finite, the device result is non-finite (NaN and
  inf are not told apart);
* containment — let *outside* be the elements where the fp64 result of the NaN run is finite and bit-equal to the fp64 clean
  result: there the device results of all three poisoned runs carry the bits of the device's clean run;
* not vacuous — the fp64 NaN run has a non-finite element, and every non-scalar output has an element outside (outputs a case
  names in ``all_inside`` excepted: a gradient that may sum over the poisoned element in every entry).  Both are checked on the CPU,
  from the reference alone, before the first launch.

Inside the cone nothing is asserted where fp64 is finite (relu(-inf) = 0, sigmoid(inf) = 1, a ReLU mask that drops a NaN cotangent).

Accepted once, for every split-bf16 product: x = hi + lo with hi = bf16(x), lo = x - hi turns an inf into hi = inf,
lo = inf - inf = NaN, so an inf operand gives NaN where fp32 torch gives inf.  The rules do not tell the two apart.

The ReLU backward reference is torch's own (``threshold_backward`` through autograd, or ``where(y > 0, dy, 0)`` for the bare
helpers): a NaN cotangent under a closed mask is dropped by torch and by the kernels alike.

FOUND BY THIS MODULE and fixed with it: the conv engine's item-table weight gradient (conv_wgrad_kernel) spread a NaN inside its
own channel at a ragged sequence end.  x[0, 16, 131] = NaN at L = 132 turned dw[:, 16, 0] into NaN — 33 elements that fp64 leaves
bit-equal to clean, because tap 0 pairs x[131] with dy[135], which does not exist.  The kernel stages 32-sample tiles; in the
last, partial tile (L % 32 != 0) the dy columns t >= L are zeros, but the x sample a tap with a negative shift pairs with them
is real data: 0·NaN.  Such a tile now takes its x operand through a select on the tile column.  19 cases failed on it
(``conv-bf3-*`` / ``conv-window-*`` with x planted at t = 128, 130, 131 of L = 132, ``conv-scalar-*`` at t = 68, 69 of L = 70,
``item_wgrad-x*.16.131``).

Every kernel these cases reach was read for loops whose exit depends on data before the module first ran on a GPU: the conv
engine's ``while`` loops walk the integer plan tables, fst_logdet_inv's pivot search and the CPC panel merge are counted
``for`` loops whose comparisons only choose a value (a NaN fails them and leaves the index inside its range), the recurrences
run to an integer step count.  A NaN cannot make any of them spin.  (fst_logdet_inv takes a weight and is not poisoned here.)
"""
from __future__ import annotations

import functools
import math
import os
import zlib
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Sequence, Tuple

import pytest
import torch
import torch.nn.functional as F

from feature_level_style_transfer_for_tsc_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN, INF = float("nan"), float("inf")
POISONS = (NAN, INF, -INF)          # the NaN run comes first: it defines *outside*
BF3 = ops.MATH == "bf16x3"
Tensors = Dict[str, torch.Tensor]


def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def rnd(g, *shape, k: float = 1.0) -> torch.Tensor:
    """Seeded fp32 draws of order k: the values the device receives; the reference takes them as fp64."""
    return torch.randn(*shape, generator=g) * k


# --------------------------------------------------------------------------------------------------
# the helper
# --------------------------------------------------------------------------------------------------
@dataclass
class Op:
    """An op as a pair (GPU callable, fp64 CPU callable) with its clean inputs.  Each callable maps the dict of inputs to a dict
    of outputs; an input ``d_<output>`` is that output's cotangent; ``diff`` names the inputs whose gradients are examined (as
    ``grad_<input>``)."""
    dev: Callable[[Tensors], Tensors]
    ref: Callable[[Tensors], Tensors]
    clean: Tensors
    diff: Tuple[str, ...] = ()
    _ref_clean: Optional[Tensors] = field(default=None, repr=False)

    def ref_clean(self) -> Tensors:
        """The fp64 clean run: computed once per op, shared by its cases, never changed."""
        if self._ref_clean is None:
            self._ref_clean = _run(self.ref, _to(self.clean, "cpu", torch.float64), self.diff)
        return self._ref_clean


def _to(t: Tensors, device: str, dtype) -> Tensors:
    return {k: v.to(device=device, dtype=dtype) for k, v in t.items()}


def _run(fn, t: Tensors, diff: Sequence[str]) -> Tensors:
    """Outputs of ``fn`` and the gradients of the inputs ``diff`` under the cotangents ``d_*``, detached on the CPU."""
    leaves = {k: v.clone().requires_grad_(k in diff) for k, v in t.items() if not k.startswith("d_")}
    outs = fn(leaves)
    res = {k: v.detach() for k, v in outs.items()}
    pairs = [(outs[k[2:]], v) for k, v in t.items() if k.startswith("d_") and outs[k[2:]].requires_grad]
    if diff and pairs:
        grads = torch.autograd.grad([o for o, _ in pairs], [leaves[k] for k in diff], [c for _, c in pairs], allow_unused=True)
        res.update({"grad_" + k: g.detach() for k, g in zip(diff, grads) if g is not None})
    return {k: v.cpu().contiguous() for k, v in res.items()}


def _planted(t: Tensors, which: str, index: Tuple[int, ...], value: float) -> Tensors:
    t = dict(t)
    x = t[which].clone()
    x[index] = value
    t[which] = x
    return t


def _bits(x: torch.Tensor) -> torch.Tensor:
    return x.reshape(-1).view(torch.int64 if x.dtype == torch.float64 else torch.int32)


def reference_runs(op: Op, which: str, index: Tuple[int, ...], values=POISONS, all_inside: Sequence[str] = (), relu_cone: bool = False):
    """The fp64 runs of a case (clean, then one per value) and *outside* per output; asserts that the case is not vacuous.
    Runs on the CPU alone.
    ``relu_cone`` — EXCEPTION for an activation planted in front of a fused ReLU: *outside* is what ALL THREE fp64 poisoned runs
    leave finite and bit-equal to clean, not the NaN run alone.  Behind a ReLU the gradients depend on the planted value through
    the mask, and the NaN run cannot show it where the clean mask is closed: NaN keeps it closed (fp64 = clean, bit for bit), +inf
    opens it wherever the weight is positive, -inf wherever it is negative (f32 arithmetic; a split-bf16 product turns both into
    NaN).  Those gradients do depend on the planted element; the union of the three runs' cones says so."""
    assert values[0] != values[0], "the first planted value is the NaN that defines *outside*"
    clean64 = _to(op.clean, "cpu", torch.float64)
    ref = [op.ref_clean()] + [_run(op.ref, _planted(clean64, which, index, v), op.diff) for v in values]
    assert all(bool(torch.isfinite(v).all()) for v in ref[0].values()), "the clean fp64 run is not finite"
    outside = {k: torch.isfinite(ref[1][k]).reshape(-1) & (_bits(ref[1][k]) == _bits(ref[0][k])) for k in ref[0]}
    if relu_cone:
        for r in ref[2:]:
            outside = {k: o & torch.isfinite(r[k]).reshape(-1) & (_bits(r[k]) == _bits(ref[0][k])) for k, o in outside.items()}
    assert any(bool((~torch.isfinite(v)).any()) for v in ref[1].values()), "vacuous: the fp64 NaN run is finite everywhere"
    for k, o in outside.items():
        if ref[0][k].dim() > 0 and ref[0][k].numel() > 1 and k not in all_inside:
            assert bool(o.any()), f"vacuous: no element of {k} lies outside the cone of {which}{list(index)}"
    return ref, outside


def check_nonfinite(op: Op, which: str, index: Tuple[int, ...], values=POISONS, all_inside: Sequence[str] = (), relu_cone: bool = False):
    """Plant each of ``values`` at ``op.clean[which][index]``; hold the device to the module's three rules."""
    ref, outside = reference_runs(op, which, index, values, all_inside, relu_cone)
    clean32 = _to(op.clean, DEV, torch.float32)
    dev = [_run(op.dev, clean32, op.diff)] + [_run(op.dev, _planted(clean32, which, index, v), op.diff) for v in values]
    assert set(dev[0]) <= set(ref[0]), f"device outputs {sorted(set(dev[0]) - set(ref[0]))} have no reference"
    for k, v in dev[0].items():
        assert v.shape == ref[0][k].shape, f"{k}: device shape {tuple(v.shape)}, reference {tuple(ref[0][k].shape)}"
        assert bool(torch.isfinite(v).all()), f"{k}: the clean device run is not finite"
    problems = []
    for value, r, d in zip(values, ref[1:], dev[1:]):
        for k in dev[0]:
            swallowed = (~torch.isfinite(r[k])).reshape(-1) & torch.isfinite(d[k]).reshape(-1)
            if bool(swallowed.any()):
                i = int(swallowed.nonzero()[0])
                problems.append(f"{k}: {value} at {which}{list(index)} swallowed at {int(swallowed.sum())} elements "
                                f"(first flat index {i}: fp64 {float(r[k].reshape(-1)[i])}, device {float(d[k].reshape(-1)[i])})")
            spread = outside[k] & (_bits(d[k]) != _bits(dev[0][k]))
            if bool(spread.any()):
                i = int(spread.nonzero()[0])
                problems.append(f"{k}: {value} at {which}{list(index)} spread to {int(spread.sum())} elements outside its cone "
                                f"(first flat index {i}: clean {float(dev[0][k].reshape(-1)[i])}, now {float(d[k].reshape(-1)[i])})")
    assert not problems, "\n".join(problems)


@dataclass(frozen=True)
class Case:
    id: str
    op: Callable[[], Op]
    which: str
    index: Tuple[int, ...]
    all_inside: Tuple[str, ...] = ()
    open_mask: str = ""          # a cotangent planted under a ReLU: the output whose clean value must be > 0 there (``open_index``)
    relu_cone: bool = False      # an activation planted in front of a fused ReLU (``reference_runs``)


def _cases(prefix: str, op: Callable[[], Op], which: str, indices, all_inside=(), open_mask: str = "", relu_cone: bool = False) -> list:
    return [Case(f"{prefix}-{which}{'.'.join(str(i) for i in ix)}", op, which, tuple(ix), tuple(all_inside), open_mask, relu_cone)
            for ix in indices]


def open_index(y: torch.Tensor, index: Tuple[int, ...]) -> Tuple[int, ...]:
    """The first index at or after ``index`` (row-major, wrapping) where the clean fp64 output ``y`` is positive.  A cotangent
    under a closed ReLU mask is dropped by torch and by the kernels alike: planted there, the reference alone stays finite."""
    flat = (y.reshape(-1) > 0).nonzero().reshape(-1)
    at = int(torch.tensor(index).mul(torch.tensor(y.stride())).sum()) if index else 0
    nxt = flat[flat >= at]
    return tuple(int(i) for i in torch.unravel_index(nxt[0] if nxt.numel() else flat[0], y.shape))


def _dedup(indices) -> list:
    out = []
    for ix in indices:
        if ix not in out:
            out.append(ix)
    return out


def ncl_indices(B: int, C: int, L: int, halo: int = 0, tile: int = 128) -> list:
    """The index scheme on a [B, C, L] tensor: element 0 and the last element; time 31 / 32 and 127 / 128; L-1 and L-2; the last
    channel; channels 15 / 16 (the pipelined kernel's 16-channel stage); the last sample; within ``halo`` of a tile edge; and the
    last element of sample B-2, whose successor must stay clean."""
    b, c = min(1, B - 1), min(3, C - 1)
    ix = [(0, 0, 0), (B - 1, C - 1, L - 1), (b, c, L - 1), (b, c, L - 2), (b, C - 1, L // 2), (B - 1, c, 1), (B - 2, C - 1, L - 1)]
    ix += [(b, c, t) for t in (31, 32, 127, 128) if t < L]
    ix += [(b, ch, L // 2 + 1) for ch in (15, 16) if ch < C]
    if halo:
        ix += [(b, c, t) for t in (tile - halo, tile + halo - 1) if 0 <= t < L]
    return _dedup(ix)


# --------------------------------------------------------------------------------------------------
# the fused activations of the reference compositions
# --------------------------------------------------------------------------------------------------
class _Relu(torch.autograd.Function):
    """relu as the fused ops define it.  Forward: torch.relu, NaN stays NaN.  Backward: the mask [out > 0], which is closed at a NaN
    output — EXCEPTION to "as fp32 torch": torch's threshold_backward is ``x <= 0 ? 0 : g`` and so hands the cotangent through
    where the output is NaN.  Either way the element is inside the cone; with torch's form fp64 would call the gradients behind
    a NaN output "clean" wherever the clean mask was open, which the kernels (the backward masks are [o > 0]) are not."""

    @staticmethod
    def forward(ctx, x):
        out = torch.relu(x)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        return torch.where(out > 0, g, torch.zeros_like(g))


SELU_ALPHA, SELU_SCALE = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946


class _Selu(torch.autograd.Function):
    """selu with its derivative written out, scale·(x > 0 ? 1 : alpha·exp(x)): NaN for NaN, scale at +inf, 0 at -inf.  torch's own
    elu_backward answers a NaN input differently in its vector body and in its scalar tail, and autograd through
    ``where(x > 0, x, alpha·expm1(x))`` gives 0·inf = NaN at +inf."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return SELU_SCALE * torch.where(x > 0, x, SELU_ALPHA * torch.expm1(x))

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * SELU_SCALE * torch.where(x > 0, torch.ones_like(x), SELU_ALPHA * torch.exp(x))


# --------------------------------------------------------------------------------------------------
# conv engine: ConvFn, ConvReluFn, the two-input forms, the weight gradients
# --------------------------------------------------------------------------------------------------
def omni_live(M: int, ntaps: int) -> list:
    """Omni-scale live tap ranges: the first 32 rows live at the middle tap only, the rest at every tap.  The table is uniform
    inside each 32-row M-group and each 16-channel K-chunk ON PURPOSE: the plans skip a tap for a whole group / chunk (the union of
    its rows' ranges), so inside a group a row's masked taps ARE multiplied by its zero weights, as torch does (measured: with
    ranges that widen row by row, a NaN reached 68 outputs of the narrower rows of its group).  With a uniform table "live taps
    of the row" and "live taps of the group" are the same reference."""
    c = ntaps // 2
    return [(c, c + 1) if m < 32 else (0, ntaps) for m in range(M)]


def ref_conv(x, w, dil: int, pad: int, live=None):
    """y[b,m,t] = Σ_{c,k live} w[m,c,k]·x[b,c,t + k·dil - pad], zero outside [0, L).  With ``live``, one conv1d per run of rows that
    share a live tap range, over those taps only: the device skips masked taps, so a NaN under a masked (zero) weight does not
    reach the row — the documented exception to "fp32 torch multiplies it by the zero"."""
    ntaps, L = w.size(2), x.size(2)
    xp = F.pad(x, (pad, (ntaps - 1) * dil - pad))
    if live is None:
        return F.conv1d(xp, w, dilation=dil)
    ys, m = [], 0
    while m < len(live):
        e = m
        while e < len(live) and live[e] == live[m]:
            e += 1
        lo, hi = live[m]
        ys.append(F.conv1d(xp[:, :, lo * dil: lo * dil + L + (hi - lo - 1) * dil], w[m:e, :, lo:hi], dilation=dil))
        m = e
    return torch.cat(ys, 1)


def _ref_dw(dy, x, ntaps: int, dil: int, pad: int):
    """dw[m,c,k] = Σ_{b,t} dy[b,m,t]·x[b,c,t + k·dil - pad]: a NaN in x[b,c,t] stays in dw[:, c, :]."""
    L = x.size(2)
    xp = F.pad(x, (pad, (ntaps - 1) * dil - pad))
    return torch.stack([torch.einsum("bmt,bct->mc", dy, xp[:, :, k * dil: k * dil + L]) for k in range(ntaps)], dim=2)


class _OmniConv(torch.autograd.Function):
    """A masked (omni-scale) conv as the layers run it: forward and data gradient over the live taps, the weight gradient DENSE —
    every tap of every row, masked ones too, which is what torch's conv backward returns as well (quirk Q1: the mask is applied
    to ``.data`` before each forward, not to the gradient)."""

    @staticmethod
    def forward(ctx, x, w, dil, pad, live):
        ctx.save_for_backward(x, w)
        ctx.geo = (dil, pad, live)
        return ref_conv(x, w, dil, pad, live)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        dil, pad, live = ctx.geo
        with torch.enable_grad():
            x_ = x.detach().requires_grad_(True)
            (dx,) = torch.autograd.grad(ref_conv(x_, w.detach(), dil, pad, live), x_, g)
        return dx, _ref_dw(g, x, w.size(2), dil, pad), None, None, None


CONV_ROUTES = {          # name: (L, C0, ntaps, dil, omni, the forward's route family in split-bf16 mode)
    "bf3": (132, 17, 3, 4, False, ops.ROUTE_BF3),        # split-bf16 pipelined kernel: 16-channel stages, L % 4 == 0
    "scalar": (70, 17, 3, 4, False, ops.ROUTE_PIPE),     # L % 4 != 0: the f32 pipelined kernel with scalar staging
    "window": (132, 9, 9, 1, True, ops.ROUTE_WIN_BF3),   # omni-scale masks: rows 0..31 are live at tap 4 only
}


@functools.lru_cache(maxsize=None)
def conv_op(route: str, relu: bool, bias: bool) -> Op:
    L, C0, ntaps, dil, omni, family = CONV_ROUTES[route]
    M, B, pad = 33, 3, (ntaps - 1) * dil // 2
    live = omni_live(M, ntaps) if omni else None
    if omni:
        assert live[0] == (ntaps // 2, ntaps // 2 + 1)
    spec = ops.ConvSpec(M, C0, ntaps, dil, pad, row_live=live)
    g = _gen(f"conv-{route}")
    w = rnd(g, M, C0, ntaps, k=(C0 * ntaps) ** -0.5)
    if omni:
        for m, (lo, hi) in enumerate(live):
            w[m, :, :lo] = 0
            w[m, :, hi:] = 0
    clean = dict(x=rnd(g, B, C0, L), w=w, d_y=rnd(g, B, M, L))
    if bias:
        clean["b"] = rnd(g, M, k=0.3)
    fn = ops.ConvReluFn if relu else ops.ConvFn

    def dev(t):
        y = fn.apply(spec, t["x"], t["w"], t.get("b"))
        got = ops.last_route()
        assert not BF3 or got[0] == family, f"forward ran {ops.route_kernel_name(got)}, wanted family {family}"
        return {"y": y}

    def ref(t):
        y = _OmniConv.apply(t["x"], t["w"], dil, pad, live) if omni else ref_conv(t["x"], t["w"], dil, pad)
        if bias:
            y = y + t["b"][None, :, None]
        return {"y": _Relu.apply(y) if relu else y}

    return Op(dev, ref, clean, ("x", "w") + (("b",) if bias else ()))


def conv_cases() -> list:
    out = []
    for route, (L, C0, ntaps, dil, omni, _) in CONV_ROUTES.items():
        ix = ncl_indices(3, C0, L, halo=(ntaps - 1) * dil // 2)
        for relu, bias, sub in ((True, True, ix), (False, False, ix), (True, False, ix[:2]), (False, True, ix[:2])):
            name = f"{'convrelu' if relu else 'conv'}-{route}-{'bias' if bias else 'nobias'}"
            # (behind the ReLU every row's mask can move: the weight and bias gradients are wholly inside the cone)
            out += _cases(name, functools.partial(conv_op, route, relu, bias), "x", sub, ("grad_w", "grad_b") if relu else (), relu_cone=relu)
        # the cotangent: through relu_bwd, the data-gradient plan (taps flipped) and the weight gradient's dy operand
        out += _cases(f"convrelu-{route}-bias", functools.partial(conv_op, route, True, True), "d_y",
                      [(0, 0, 0), (2, 32, L - 1), (1, 31, min(127, L - 2))], open_mask="y")
        out += _cases(f"conv-{route}-nobias", functools.partial(conv_op, route, False, False), "d_y",
                      [(0, 0, 0), (2, 32, L - 1), (1, 32, min(128 - 4, L - 3))])
    return out


@functools.lru_cache(maxsize=None)
def conv2_op() -> Op:
    """The two-input form (the WN in_layer with its conditioning rows): forward, and both data gradients in one launch (grad_x01)."""
    M, C0, C1, ntaps, dil, pad, B, L = 33, 17, 5, 3, 4, 4, 3, 132
    spec = ops.ConvSpec(M, C0, ntaps, dil, pad, C1=C1)
    g = _gen("conv2")
    clean = dict(x0=rnd(g, B, C0, L), x1=rnd(g, B, C1, L), w0=rnd(g, M, C0, ntaps, k=(C0 * ntaps) ** -0.5), w1=rnd(g, M, C1, 1, k=C1 ** -0.5),
                 b=rnd(g, M, k=0.3), dy=rnd(g, B, M, L), res0=rnd(g, B, C0, L), acc1=rnd(g, B, C1, L))

    def dev(t):
        y = spec.forward(t["x0"], t["x1"], t["w0"], t["w1"], t["b"])
        acc1 = t["acc1"].clone()
        dx0 = spec.grad_x01(t["dy"], t["w0"], t["w1"], t["res0"], acc1)
        return {"y": y, "dx0": dx0, "dx1": acc1}

    def ref(t):
        y = ref_conv(t["x0"], t["w0"], dil, pad) + F.conv1d(t["x1"], t["w1"]) + t["b"][None, :, None]
        x0, x1 = torch.zeros_like(t["x0"], requires_grad=True), torch.zeros_like(t["x1"], requires_grad=True)
        with torch.enable_grad():
            g0, g1 = torch.autograd.grad(ref_conv(x0, t["w0"], dil, pad) + F.conv1d(x1, t["w1"]), (x0, x1), t["dy"])
        return {"y": y, "dx0": t["res0"] + g0, "dx1": t["acc1"] + g1}

    return Op(dev, ref, clean)


def conv2_cases() -> list:
    return (_cases("conv2", conv2_op, "x1", [(0, 0, 0), (2, 4, 131), (1, 2, 127)]) + _cases("conv2", conv2_op, "x0", [(1, 16, 128)]) +
            _cases("conv2", conv2_op, "dy", [(0, 0, 0), (2, 32, 131), (1, 31, 127), (1, 32, 124), (0, 15, 131)]) +
            _cases("conv2", conv2_op, "res0", [(1, 16, 131)]) + _cases("conv2", conv2_op, "acc1", [(1, 4, 131)]))


@functools.lru_cache(maxsize=None)
def dense_wgrad_op(kind: str) -> Op:
    """``ConvSpec.grad_w`` called from this thread, so that the route record can be read: ``items`` = the conv engine's item-table
    kernel (the route ConvFn's backward takes at this shape), ``dense`` = fst_dense_tap_wgrad (many taps from pre-shifted copies of
    one window), ``tap`` = fst_tap_wgrad (FST_TAP_WGRAD=1; shifts of +-1 read the 16 bytes of slack either side of x)."""
    M, C, K, dil, pad, B, L = {"dense": (33, 3, 37, 1, 18, 3, 96), "tap": (33, 64, 3, 1, 1, 3, 64), "items": (33, 17, 3, 4, 4, 3, 132)}[kind]
    spec = ops.ConvSpec(M, C, K, dil, pad)
    g = _gen("wgrad-" + kind)
    clean = dict(x=rnd(g, B, C, L), dy=rnd(g, B, M, L))

    def dev(t):
        x = ops.empty_with_slack(B, C, L, DEV)
        x.copy_(t["x"])
        dy = t["dy"].contiguous()
        prev = os.environ.get("FST_TAP_WGRAD")
        os.environ["FST_TAP_WGRAD"] = "1" if kind == "tap" else "0"
        try:
            assert spec.dense_tap_wgrad_ok(B, L, x, dy) == (kind == "dense") and spec.tap_wgrad_ok(B, L, x, dy) == (kind == "tap")
            dw, _ = spec.grad_w(x, None, dy)
        finally:
            if prev is None:
                del os.environ["FST_TAP_WGRAD"]
            else:
                os.environ["FST_TAP_WGRAD"] = prev
        if kind == "items":
            assert ops.last_route()[0] == ops.ROUTE_WGRAD, ops.last_route()
        else:
            assert ops.wn_last_route()[0] == (ops.WN_ROUTE_TZ if kind == "dense" else ops.WN_ROUTE_WGRAD), ops.wn_last_route()
        return {"dw": dw}

    return Op(dev, lambda t: {"dw": _ref_dw(t["dy"], t["x"], K, dil, pad)}, clean)


def dense_wgrad_cases() -> list:
    out = _cases("dense_tap_wgrad", functools.partial(dense_wgrad_op, "dense"), "x",
                 [(0, 0, 0), (2, 2, 95), (0, 2, 95), (1, 0, 0), (1, 1, 31), (1, 1, 32), (1, 1, 94)])
    out += _cases("dense_tap_wgrad", functools.partial(dense_wgrad_op, "dense"), "dy", [(0, 0, 0), (2, 32, 95), (1, 31, 32)])
    out += _cases("tap_wgrad", functools.partial(dense_wgrad_op, "tap"), "x",
                  [(0, 0, 0), (2, 63, 63), (0, 63, 63), (2, 0, 0), (1, 15, 63), (1, 16, 0), (1, 31, 31), (1, 32, 32)])
    out += _cases("tap_wgrad", functools.partial(dense_wgrad_op, "tap"), "dy", [(0, 0, 0), (2, 32, 63), (1, 31, 31)])
    out += _cases("item_wgrad", functools.partial(dense_wgrad_op, "items"), "x", [(0, 0, 0), (2, 16, 131), (1, 15, 31), (1, 16, 32), (0, 16, 131)])
    out += _cases("item_wgrad", functools.partial(dense_wgrad_op, "items"), "dy", [(0, 0, 0), (2, 32, 131), (1, 31, 128)])
    return out


@functools.lru_cache(maxsize=None)
def wn_wgrad_in_op(dil: int) -> Op:
    """fst_wn_wgrad_in: dilation 4 (aligned shifts) and dilation 2 on a slack tensor, whose 16-byte pieces start two samples
    outside a row — in the neighbouring row, sample or slack — and are patched at the sequence boundary in LDS."""
    n, h, B, L = 16, 5, 3, 64
    g = _gen(f"wn-wgrad-in{dil}")
    clean = dict(dg=rnd(g, B, 2 * n, L), a=rnd(g, B, n, L), u0=rnd(g, B, h, L))

    def dev(t):
        a = ops.empty_with_slack(B, n, L, DEV)
        a.copy_(t["a"])
        assert ops.wn_wgrad_ok(0, B, L, n, h, dil, a)
        dw_in = torch.empty(2 * n, n, 3, device=DEV)
        dw_cond = torch.empty(2 * n, h, 1, device=DEV)
        ops.wn_wgrad_in(t["dg"].contiguous(), a, t["u0"].contiguous(), dw_in, dw_cond, n, h, dil)
        assert ops.wn_last_route()[0] == ops.WN_ROUTE_WGRAD
        return {"dw_in": dw_in, "dw_cond": dw_cond}

    def ref(t):
        return {"dw_in": _ref_dw(t["dg"], t["a"], 3, dil, dil), "dw_cond": _ref_dw(t["dg"], t["u0"], 1, 1, 0)}

    return Op(dev, ref, clean)


@functools.lru_cache(maxsize=None)
def wn_wgrad_rs_op(last: bool) -> Op:
    """fst_wn_wgrad_rs: acts = t·s is re-formed from the gate halves while staging, so a NaN in either half of channel c stays in
    column c of dw_rs."""
    n, B, L = 16, 3, 64
    g = _gen(f"wn-wgrad-rs{last}")
    clean = dict(ts=rnd(g, B, 2 * n, L), dout=rnd(g, B, n, L))
    if not last:
        clean["da"] = rnd(g, B, n, L)

    def dev(t):
        assert ops.wn_wgrad_ok(1, B, L, n, 5, 4)
        dw = torch.empty(n if last else 2 * n, n, 1, device=DEV)
        ops.wn_wgrad_rs(None if last else t["da"].contiguous(), t["dout"].contiguous(), t["ts"].contiguous(), dw, last, n)
        assert ops.wn_last_route()[0] == ops.WN_ROUTE_WGRAD
        return {"dw_rs": dw}

    def ref(t):
        dy = t["dout"] if last else torch.cat([t["da"], t["dout"]], 1)
        return {"dw_rs": torch.einsum("bmt,bct->mc", dy, t["ts"][:, :n] * t["ts"][:, n:])[:, :, None]}

    return Op(dev, ref, clean)


def wn_wgrad_cases() -> list:
    out = []
    for dil in (4, 2):
        op = functools.partial(wn_wgrad_in_op, dil)
        # the last element of sample 0 and the first of sample 2: the neighbours the shifted pieces and the slack reads touch
        out += _cases(f"wn_wgrad_in-d{dil}", op, "a", [(0, 15, 63), (2, 0, 0), (0, 0, 0), (2, 15, 63), (1, 7, 63), (1, 8, 0),
                                                      (1, 3, 31), (1, 3, 32), (1, 3, 62)])
        out += _cases(f"wn_wgrad_in-d{dil}", op, "u0", [(0, 0, 0), (2, 4, 63), (1, 4, 31)])
        out += _cases(f"wn_wgrad_in-d{dil}", op, "dg", [(0, 0, 0), (2, 31, 63), (1, 15, 32)])
    for last in (False, True):
        op = functools.partial(wn_wgrad_rs_op, last)
        out += _cases(f"wn_wgrad_rs-{'last' if last else 'mid'}", op, "ts", [(0, 0, 0), (2, 31, 63), (0, 15, 63), (2, 16, 0), (1, 3, 31), (1, 19, 32)])
        out += _cases(f"wn_wgrad_rs-{'last' if last else 'mid'}", op, "dout", [(0, 0, 0), (2, 15, 63)])
    out += _cases("wn_wgrad_rs-mid", functools.partial(wn_wgrad_rs_op, False), "da", [(0, 0, 0), (2, 15, 63)])
    return out


# --------------------------------------------------------------------------------------------------
# dense GEMMs: LinearActFn, RandomLayerFn, FixedMatmulFn, nt_gemm
# --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def linear_op(act: int) -> Op:
    lead, K, N, slope = (3, 11), 36, 40, 0.2
    g = _gen(f"linear{act}")
    clean = dict(x=rnd(g, *lead, K), W=rnd(g, N, K, k=K ** -0.5), b=rnd(g, N, k=0.3), d_y=rnd(g, *lead, N))

    def dev(t):
        return {"y": ops.LinearActFn.apply(t["x"], t["W"], t["b"], act, slope)}

    def ref(t):
        y = F.linear(t["x"], t["W"], t["b"])
        return {"y": _Relu.apply(y) if act == ops.ACT_RELU else F.leaky_relu(y, slope) if act == ops.ACT_LEAKY else y}

    return Op(dev, ref, clean, ("x", "W", "b"))


def linear_cases() -> list:
    out = []
    for act, name in ((ops.ACT_NONE, "none"), (ops.ACT_RELU, "relu"), (ops.ACT_LEAKY, "leaky")):
        op = functools.partial(linear_op, act)
        out += _cases(f"linear-{name}", op, "x", [(0, 0, 0), (2, 10, 35), (1, 5, 31), (1, 5, 32), (2, 9, 15), (2, 10, 16)],
                      ("grad_W", "grad_b") if act == ops.ACT_RELU else (), relu_cone=act == ops.ACT_RELU)
        out += _cases(f"linear-{name}", op, "d_y", [(0, 0, 0), (2, 10, 39), (1, 5, 31), (1, 5, 32)], open_mask="y" if act == ops.ACT_RELU else "")
    return out


GEMM_SHAPES = {"small": (3, 5, 32), "odd": (33, 129, 64), "back": (33, 160, 64)}       # M, N, K


@functools.lru_cache(maxsize=None)
def random_layer_op(shape: str) -> Op:
    """RandomLayerFn: (x·R0·scale) ⊙ (p·R1).  Its input gradient is a second nt_gemm whose reduction runs over N, which that kernel
    takes in multiples of 32: the ``back`` shape examines it, the two odd-N shapes examine the forward and the gradient of p."""
    M, N, K = GEMM_SHAPES[shape]
    ncls, scale = 4, N ** -0.5
    g = _gen("randlayer" + shape)
    clean = dict(x=rnd(g, M, K), p=rnd(g, M, ncls), R0=rnd(g, K, N), R1=rnd(g, ncls, N), d_y=rnd(g, M, N))

    def dev(t):
        return {"y": ops.RandomLayerFn.apply(t["x"], t["p"], t["R0"], t["R0"].t().contiguous(), t["R1"], scale)}

    def ref(t):
        return {"y": (t["x"] @ t["R0"]) * scale * (t["p"] @ t["R1"])}

    return Op(dev, ref, clean, ("x", "p") if N % 32 == 0 else ("p",))


@functools.lru_cache(maxsize=None)
def fixed_matmul_op(shape: str) -> Op:
    """EXCEPTION: FixedMatmulFn splits its reduction over workgroups that add into the output with float atomics.  Up to two
    16-channel chunks the sum has one order; beyond that two clean runs already differ in their last bits, and containment cannot
    be asked bit for bit.  So the odd shape runs at K = 32 (two chunks) instead of 64, forward only: its backward reduces over
    N = 129 (nine chunks).  The small shape (reductions of 32 and 5) is examined both ways."""
    M, N, K = GEMM_SHAPES[shape]
    K = min(K, 32)
    g = _gen("fixedmm" + shape)
    clean = dict(x=rnd(g, M, K), R=rnd(g, K, N, k=K ** -0.5))
    if shape == "small":
        clean["d_y"] = rnd(g, M, N)

    def dev(t):
        return {"y": ops.FixedMatmulFn.apply(t["x"], t["R"], t["R"].t().contiguous())}

    return Op(dev, lambda t: {"y": t["x"] @ t["R"]}, clean, ("x",) if shape == "small" else ())


@functools.lru_cache(maxsize=None)
def nt_gemm_op(shape: str) -> Op:
    M, N, K = GEMM_SHAPES[shape]
    g = _gen("ntgemm" + shape)
    clean = dict(A=rnd(g, M, K), Bm=rnd(g, N, K, k=K ** -0.5))

    def dev(t):
        assert ops.nt_gemm_ok(M, N, K, t["A"], t["Bm"])
        return {"C": ops.nt_gemm(t["A"], t["Bm"])}

    return Op(dev, lambda t: {"C": t["A"] @ t["Bm"].t()}, clean)


def gemm_cases() -> list:
    out = []
    for shape, (M, N, K) in GEMM_SHAPES.items():
        rows = _dedup([(0, 0), (M - 1, K - 1), (M // 2, 31), (M - 1, 0)])
        out += _cases(f"random_layer-{shape}", functools.partial(random_layer_op, shape), "x", rows)
        out += _cases(f"random_layer-{shape}", functools.partial(random_layer_op, shape), "p", [(0, 0), (M - 1, 3)])
        out += _cases(f"random_layer-{shape}", functools.partial(random_layer_op, shape), "d_y", [(0, 0), (M - 1, N - 1)])
        if shape != "back":
            out += _cases(f"fixed_matmul-{shape}", functools.partial(fixed_matmul_op, shape), "x", _dedup([(0, 0), (M - 1, 31), (M // 2, 15), (M - 1, 0)]))
            if shape == "small":
                out += _cases(f"fixed_matmul-{shape}", functools.partial(fixed_matmul_op, shape), "d_y", [(0, 0), (M - 1, N - 1)])
            out += _cases(f"nt_gemm-{shape}", functools.partial(nt_gemm_op, shape), "A", rows)
    return out


# --------------------------------------------------------------------------------------------------
# BatchNorm: BNActFn, BNAddBNReluFn
# --------------------------------------------------------------------------------------------------
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def _bn_params(g, C: int, tag: str) -> Tensors:
    return {f"g{tag}": rnd(g, C, k=0.3) + 1.0, f"b{tag}": rnd(g, C, k=0.3), f"rm{tag}": rnd(g, C, k=0.3), f"rv{tag}": rnd(g, C, k=0.1).abs() + 0.8}


@functools.lru_cache(maxsize=None)
def bn_op(training: bool, relu: bool, L: int) -> Op:
    """The running statistics after the call are outputs: in train mode a NaN sample reaches them (and the ``buffers`` group of
    the anomaly guard), in eval mode they must keep their bits."""
    B, C = 3, 5
    g = _gen(f"bn{training}{relu}{L}")
    clean = dict(y=rnd(g, B, C, L), d_out=rnd(g, B, C, L), **_bn_params(g, C, ""))

    def dev(t):
        rm, rv = t["rm"].clone(), t["rv"].clone()
        out = ops.BNActFn.apply(t["y"], t["g"], t["b"], rm, rv, training, relu, BN_EPS, BN_MOMENTUM)
        return {"out": out, "rm_after": rm, "rv_after": rv}

    def ref(t):
        rm, rv = t["rm"].detach().clone(), t["rv"].detach().clone()
        out = F.batch_norm(t["y"], rm, rv, t["g"], t["b"], training, BN_MOMENTUM, BN_EPS)
        return {"out": _Relu.apply(out) if relu else out, "rm_after": rm, "rv_after": rv}

    return Op(dev, ref, clean, ("y", "g", "b"))


@functools.lru_cache(maxsize=None)
def bn_join_op(training: bool, L: int) -> Op:
    B, C = 3, 5
    g = _gen(f"bnjoin{training}{L}")
    clean = dict(ya=rnd(g, B, C, L), yb=rnd(g, B, C, L), d_out=rnd(g, B, C, L), **_bn_params(g, C, "a"), **_bn_params(g, C, "b"))

    def dev(t):
        st = {k: t[k].clone() for k in ("rma", "rva", "rmb", "rvb")}
        out = ops.BNAddBNReluFn.apply(t["ya"], t["ga"], t["ba"], st["rma"], st["rva"], t["yb"], t["gb"], t["bb"], st["rmb"], st["rvb"],
                                      training, BN_EPS, BN_MOMENTUM)
        return {"out": out, **{k + "_after": v for k, v in st.items()}}

    def ref(t):
        st = {k: t[k].detach().clone() for k in ("rma", "rva", "rmb", "rvb")}
        out = _Relu.apply(F.batch_norm(t["ya"], st["rma"], st["rva"], t["ga"], t["ba"], training, BN_MOMENTUM, BN_EPS) +
                          F.batch_norm(t["yb"], st["rmb"], st["rvb"], t["gb"], t["bb"], training, BN_MOMENTUM, BN_EPS))
        return {"out": out, **{k + "_after": v for k, v in st.items()}}

    return Op(dev, ref, clean, ("ya", "ga", "ba", "yb", "gb", "bb"))


def bn_cases() -> list:
    out = []
    for L in (12, 257):                      # the 16-byte and the dword paths
        ix = _dedup([(0, 0, 0), (2, 4, L - 1), (1, 2, L - 2), (1, 4, L // 2), (0, 4, L - 1), (2, 0, 0)] +
                    [(1, 2, t) for t in (31, 32, 127, 128, 255, 256) if t < L])
        for training, relu in ((True, True), (False, True), (True, False)):
            name = f"bn-{'train' if training else 'eval'}{'-relu' if relu else ''}-L{L}"
            op = functools.partial(bn_op, training, relu, L)
            # eval mode does not touch the running statistics: nothing of them is in the cone (and nothing non-finite)
            out += _cases(name, op, "y", ix, relu_cone=relu)
            out += _cases(name, op, "d_out", [(0, 0, 0), (2, 4, L - 1), (1, 2, L // 2)], open_mask="out" if relu else "")
        for training in (True, False):
            name = f"bnjoin-{'train' if training else 'eval'}-L{L}"
            op = functools.partial(bn_join_op, training, L)
            out += _cases(name, op, "ya", ix[:4], relu_cone=True) + _cases(name, op, "yb", ix[1:5], relu_cone=True)
            out += _cases(name, op, "d_out", [(0, 0, 0), (2, 4, L - 1)], open_mask="out")
    return out


# --------------------------------------------------------------------------------------------------
# WaveGlow: WNFn, FlowFn, CouplingFn, CouplingInvFn
# --------------------------------------------------------------------------------------------------
WN_N, WN_H, WN_LAYERS = 16, 5, 3
WN_CONE = sum(2 ** i for i in range(WN_LAYERS))       # 7 samples either side of a poisoned one


@functools.lru_cache(maxsize=None)
def wn_specs() -> "ops.WNSpecs":
    return ops.WNSpecs(WN_H, WN_N, WN_LAYERS)


def wn_flat(g) -> torch.Tensor:
    S = wn_specs()
    ws = []
    for sh in S.shapes:
        fan = math.prod(sh[1:]) if len(sh) == 3 else 0
        ws.append(rnd(g, *sh, k=fan ** -0.5 if fan else 0.3))
    return S.flatten(ws)


def wn_ref(u0, flat):
    """The gated dilated-conv stack in plain torch (the reference's WN.forward on the effective weights)."""
    S, n, nl = wn_specs(), WN_N, WN_LAYERS
    W = S.unflatten(flat)
    a, out = F.conv1d(u0, W[0], W[1]), 0
    for i in range(nl):
        in_w, cond_w, in_b, cond_b, rs_w, rs_b = ops._wn_layer(S, W, i)
        gate = F.conv1d(a, in_w, in_b, dilation=2 ** i, padding=2 ** i) + F.conv1d(u0, cond_w, cond_b)
        r = F.conv1d(torch.tanh(gate[:, :n]) * torch.sigmoid(gate[:, n:]), rs_w, rs_b)
        if i < nl - 1:
            a, out = a + r[:, :n], out + r[:, n:]
        else:
            out = out + r
    return F.conv1d(out, W[4], W[5])


WN_SHAPES = {        # name: (B, L, the fused forward's route family with / without a backward to save for)
    "L512": (3, 512, ops.WN_ROUTE_LAYER_FWD, ops.WN_ROUTE_LAYER_INFER),        # two whole 256-sample tiles per sequence
    "L132": (3, 132, ops.WN_ROUTE_LAYER_FWD, ops.WN_ROUTE_LAYER_INFER),        # a partial last tile
    "stack": (256, 512, ops.WN_ROUTE_STACK_FWD, ops.WN_ROUTE_STACK_INFER),     # one persistent launch: needs a sample per CU
}


@functools.lru_cache(maxsize=None)
def wn_op(shape: str, mode: str) -> Op:
    """``train``: WNFn forward and backward (the one-launch stack backward at L <= 512, then the weight gradients);
    ``partial``: the backward inside ``partial_backward()`` — no weight gradients, the skip cotangent taken from before the end
    conv (fst_wn_stack_bwd_proj); ``infer``: no gradient wanted — the kernels that save no gate halves."""
    B, L, fam_train, fam_infer = WN_SHAPES[shape]
    S = wn_specs()
    g = _gen("wn" + shape)
    clean = dict(u0=rnd(g, B, WN_H, L), flat=wn_flat(g))
    if mode != "infer":
        clean["do" if mode == "partial" else "d_o"] = rnd(g, B, 2 * WN_H, L)

    def dev(t):
        if mode == "partial":
            # autograd would run the backward after this function returns: take the gradient here, inside the context
            u0 = t["u0"].detach().requires_grad_(True)
            o = ops.WNFn.apply(S, u0, t["flat"].detach().requires_grad_(True))
            with ops.partial_backward():
                # (autograd launches from its own thread, whose route record this one cannot read: the routing predicates instead)
                assert not BF3 or (ops.wn_stack_bwd_ok(WN_N, WN_H, L, WN_LAYERS) and ops.wn_skip_proj_ok(WN_H, False))
                (du0,) = torch.autograd.grad(o, u0, t["do"])
            return {"o": o.detach(), "du0": du0}
        o = ops.WNFn.apply(S, t["u0"], t["flat"])
        assert not BF3 or ops.wn_last_route()[0] == (fam_infer if mode == "infer" else fam_train), ops.wn_last_route()
        return {"o": o}

    def ref(t):
        if mode == "partial":
            u0 = t["u0"].detach().requires_grad_(True)
            with torch.enable_grad():
                o = wn_ref(u0, t["flat"].detach())
                (du0,) = torch.autograd.grad(o, u0, t["do"])
            return {"o": o.detach(), "du0": du0}
        return {"o": wn_ref(t["u0"], t["flat"])}

    return Op(dev, ref, clean, ("u0", "flat") if mode == "train" else ())


def wn_cases() -> list:
    out = []
    # 250: the cone [243, 257] crosses the 256-sample tile boundary through the dilated taps; 255 / 256: the boundary itself
    ix512 = [(0, 0, 0), (2, 4, 511), (1, 2, 250), (1, 2, 255), (1, 2, 256), (1, 4, 510), (1, 4, 511), (1, 0, 127), (1, 0, 128)]
    ix132 = [(0, 0, 0), (2, 4, 131), (1, 2, 125), (1, 2, 128), (1, 4, 130), (1, 4, 131), (1, 0, 31), (1, 0, 32)]
    for shape, ix in (("L512", ix512), ("L132", ix132)):
        out += _cases(f"wn-{shape}-train", functools.partial(wn_op, shape, "train"), "u0", ix)
        out += _cases(f"wn-{shape}-infer", functools.partial(wn_op, shape, "infer"), "u0", ix)
        L = WN_SHAPES[shape][1]
        # a poisoned cotangent of either half of o (b | log_s), through wn_stack_bwd and, in a partial pass, wn_stack_bwd_proj
        out += _cases(f"wn-{shape}-train", functools.partial(wn_op, shape, "train"), "d_o", [(0, 0, 0), (2, 9, L - 1), (1, 4, 125), (1, 5, 128)])
        out += _cases(f"wn-{shape}-partial", functools.partial(wn_op, shape, "partial"), "do", [(0, 0, 0), (2, 9, L - 1), (1, 4, 125), (1, 5, 128)])
        out += _cases(f"wn-{shape}-partial", functools.partial(wn_op, shape, "partial"), "u0", ix[1:3])
    out += _cases("wn-stack-train", functools.partial(wn_op, "stack", "train"), "u0", [(128, 2, 250)])
    out += _cases("wn-stack-infer", functools.partial(wn_op, "stack", "infer"), "u0", [(255, 4, 511)])
    return out


def _coupling_ref(u, o, inverse: bool):
    """EXCEPTION (inverse, log_s = +inf): the output is (x1 - b)·exp(-inf) = 0 either way, but autograd through the reference's
    division (x1 - b) / exp(log_s) gives d log_s = 0·inf = NaN, where the kernel's backward, written from the output as
    -x_next·d x_next, gives the limit -0.  The reference multiplies by exp(-log_s), whose gradient is that limit too."""
    h = u.size(1) // 2
    b, log_s = o[:, :h], o[:, h:]
    if inverse:
        return torch.cat([u[:, :h], (u[:, h:] - b) * torch.exp(-log_s)], 1), None, None
    xn = torch.cat([u[:, :h], torch.exp(log_s) * u[:, h:] + b], 1)
    return xn, log_s.sum(), (xn * xn).sum()


@functools.lru_cache(maxsize=None)
def coupling_op(inverse: bool, L: int) -> Op:
    B, h = 3, WN_H
    g = _gen(f"coupling{inverse}{L}")
    clean = dict(u=rnd(g, B, 2 * h, L), o=rnd(g, B, 2 * h, L, k=0.5), d_xn=rnd(g, B, 2 * h, L))
    if not inverse:
        clean.update(d_s_ls=rnd(g, 1).reshape(()), d_s_sq=rnd(g, 1).reshape(()))

    def dev(t):
        if inverse:
            return {"xn": ops.CouplingInvFn.apply(t["u"], t["o"])}
        xn, s_ls, s_sq = ops.CouplingFn.apply(t["u"], t["o"])
        return {"xn": xn, "s_ls": s_ls, "s_sq": s_sq}

    def ref(t):
        xn, s_ls, s_sq = _coupling_ref(t["u"], t["o"], inverse)
        return {"xn": xn} if inverse else {"xn": xn, "s_ls": s_ls, "s_sq": s_sq}

    return Op(dev, ref, clean, ("u", "o"))


@functools.lru_cache(maxsize=None)
def flow_op(inverse: bool, L: int) -> Op:
    """One flow step: the WN on the first h channels (fused at L = 12, the conv engine at L = 257: L % 4 != 0), the coupling, and
    in the backward the WN's input gradient accumulated into the coupling's."""
    B, h, S = 3, WN_H, wn_specs()
    g = _gen(f"flow{inverse}{L}")
    clean = dict(x=rnd(g, B, 2 * h, L), flat=wn_flat(g), d_xn=rnd(g, B, 2 * h, L))
    if not inverse:
        clean.update(d_s_ls=rnd(g, 1).reshape(()), d_s_sq=rnd(g, 1).reshape(()))

    def dev(t):
        xn, o, s_ls, s_sq = ops.FlowFn.apply(S, t["x"], t["flat"], inverse)
        return {"xn": xn, "o": o} if inverse else {"xn": xn, "o": o, "s_ls": s_ls, "s_sq": s_sq}

    def ref(t):
        o = wn_ref(t["x"][:, :h], t["flat"])
        xn, s_ls, s_sq = _coupling_ref(t["x"], o, inverse)
        return {"xn": xn, "o": o} if inverse else {"xn": xn, "o": o, "s_ls": s_ls, "s_sq": s_sq}

    return Op(dev, ref, clean, ("x", "flat"))


def flow_cases() -> list:
    out = []
    for L in (12, 257):
        ix = _dedup([(0, 0, 0), (2, 9, L - 1), (1, 4, L - 2), (1, 5, L // 2), (0, 9, L - 1), (1, 2, L - 1)] +
                    [(1, c, t) for c, t in ((2, 127), (7, 128), (4, 255), (5, 256)) if t < L])
        for inverse in (False, True):
            name = "inv" if inverse else "fwd"
            out += _cases(f"coupling-{name}-L{L}", functools.partial(coupling_op, inverse, L), "u", ix)
            out += _cases(f"coupling-{name}-L{L}", functools.partial(coupling_op, inverse, L), "o", ix[:4])
            out += _cases(f"coupling-{name}-L{L}", functools.partial(coupling_op, inverse, L), "d_xn", ix[1:4])
            # a NaN in the WN's input (the first h channels) reaches every weight gradient of the stack
            out += _cases(f"flow-{name}-L{L}", functools.partial(flow_op, inverse, L), "x", [i for i in ix if i[1] < WN_H], ("grad_flat",))
            out += _cases(f"flow-{name}-L{L}", functools.partial(flow_op, inverse, L), "x", [i for i in ix if i[1] >= WN_H])
            out += _cases(f"flow-{name}-L{L}", functools.partial(flow_op, inverse, L), "d_xn", ix[1:4])
    return out


# --------------------------------------------------------------------------------------------------
# NoiseTransferFn, CPCNceFn, GRULastFn, LSTM2Fn
# --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noise_transfer_op() -> Op:
    """out = selu(W·((avg_t + r_t·mean_b z_t) - (avg_s + r_s·mean_b z_s)) + bias) + z_s: the 1x1 conv mixes channels and the batch mean
    mixes samples, so a NaN at time l reaches every sample and channel of time l and nothing else.  The updated running sums
    are outputs.  dW and db sum over time: wholly inside the cone."""
    B, C, L, r_t, r_s = 7, 6, 12, 0.5, 0.25
    g = _gen("noise-transfer")
    clean = dict(z_t=rnd(g, B, C, L), z_s=rnd(g, B, C, L), W=rnd(g, C, C, 1, k=C ** -0.5), bias=rnd(g, C, k=0.3), avg_t=rnd(g, C, L),
                 avg_s=rnd(g, C, L), d_out=rnd(g, B, C, L))

    def dev(t):
        avg_t, avg_s = t["avg_t"].detach().clone(), t["avg_s"].detach().clone()
        out = ops.NoiseTransferFn.apply(t["z_t"], t["z_s"], t["W"], t["bias"], avg_t, avg_s, r_t, r_s)
        return {"out": out, "avg_t_after": avg_t, "avg_s_after": avg_s}

    def ref(t):
        new_t, new_s = t["avg_t"] + r_t * t["z_t"].mean(0), t["avg_s"] + r_s * t["z_s"].mean(0)
        out = _Selu.apply(F.conv1d((new_t - new_s)[None], t["W"], t["bias"])[0]) + t["z_s"]
        return {"out": out, "avg_t_after": new_t.detach(), "avg_s_after": new_s.detach()}

    return Op(dev, ref, clean, ("z_t", "z_s", "W", "bias"))


def noise_transfer_cases() -> list:
    ix = [(0, 0, 0), (6, 5, 11), (3, 2, 10), (6, 0, 5)]
    return (_cases("noise_transfer", noise_transfer_op, "z_t", ix, ("grad_W", "grad_bias")) +
            _cases("noise_transfer", noise_transfer_op, "z_s", ix, ("grad_W", "grad_bias")) +
            _cases("noise_transfer", noise_transfer_op, "d_out", ix))


@functools.lru_cache(maxsize=None)
def cpc_op() -> Op:
    """The panelled form: Bc = 260 > 256 prediction columns, the positives in columns 254..258 (both panels).  The loss is a
    scalar: only the first rule applies to it; the gradients are outside the cone at every other time step."""
    B, C, L, T, Bc, t0, off = 5, 6, 20, 10, 260, 3, 254
    g = _gen("cpc")
    clean = dict(feat=rnd(g, B, C, L), pred=rnd(g, T, Bc, C, k=0.3), d_nce=torch.tensor(1.7))

    def dev(t):
        return {"nce": ops.CPCNceFn.apply(t["feat"], t["pred"], t0, T, off)}

    def ref(t):
        enc = t["feat"][:, :, t0: t0 + T].permute(2, 0, 1)
        total = torch.bmm(enc, t["pred"].transpose(1, 2))
        rows = torch.arange(B)
        return {"nce": -(total[:, rows, off + rows] - torch.logsumexp(total, dim=-1)).sum() / (B * T)}

    return Op(dev, ref, clean, ("feat", "pred"))


def cpc_cases() -> list:
    return (_cases("cpc", cpc_op, "feat", [(0, 0, 3), (4, 5, 12), (2, 3, 7), (4, 0, 11)]) +
            _cases("cpc", cpc_op, "pred", [(0, 0, 0), (9, 259, 5), (4, 255, 2), (4, 256, 2), (5, 100, 3)]) +
            _cases("cpc", cpc_op, "d_nce", [()], ("grad_pred",)))


GRU_H = 64       # csrc/gru.hip is built for this hidden size; one workgroup owns two batch rows


@functools.lru_cache(maxsize=None)
def gru_op() -> Op:
    """B = 3: rows 0 and 1 share a workgroup (and its LDS), row 2 has one of its own with an idle second row.  The input
    projection is torch's; the recurrent weight gradients sum over every row and step: wholly inside the cone."""
    B, S, C, H, t_last = 3, 9, 7, GRU_H, 6
    g = _gen("gru")
    clean = dict(x=rnd(g, B, S, C), w_ih=rnd(g, 3 * H, C, k=C ** -0.5), b_ih=rnd(g, 3 * H, k=0.1), w_hh=rnd(g, 3 * H, H, k=H ** -0.5),
                 b_hh=rnd(g, 3 * H, k=0.1), d_h=rnd(g, B, H))

    def dev(t):
        return {"h": ops.GRULastFn.apply(F.linear(t["x"], t["w_ih"], t["b_ih"]), t["w_hh"], t["b_hh"], t_last)}

    def ref(t):
        xp = F.linear(t["x"], t["w_ih"], t["b_ih"])
        h = xp.new_zeros(B, H)
        for s in range(t_last + 1):
            (xr, xz, xn), (hr, hz, hn) = xp[:, s].split(H, -1), (h @ t["w_hh"].t() + t["b_hh"]).split(H, -1)
            r, z = torch.sigmoid(xr + hr), torch.sigmoid(xz + hz)
            h = (1 - z) * torch.tanh(xn + r * hn) + z * h
        return {"h": h}

    return Op(dev, ref, clean, ("x", "w_hh", "b_hh"))


@functools.lru_cache(maxsize=None)
def lstm2_op() -> Op:
    B, H = 5, 7
    g = _gen("lstm2")
    clean = dict(xproj=rnd(g, B, 4 * H), w_hh=rnd(g, 4 * H, H, k=H ** -0.5), d_h2=rnd(g, B, H))

    def dev(t):
        return {"h2": ops.LSTM2Fn.apply(t["xproj"], t["w_hh"])}

    def ref(t):
        def act(p):
            i, f, gg, o = p.split(H, -1)
            return torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
        i1, f1, g1, o1 = act(t["xproj"])
        c1 = i1 * g1
        h1 = o1 * torch.tanh(c1)
        i2, f2, g2, o2 = act(t["xproj"] + h1 @ t["w_hh"].t())
        return {"h2": o2 * torch.tanh(f2 * c1 + i2 * g2)}

    return Op(dev, ref, clean, ("xproj", "w_hh"))


def recurrence_cases() -> list:
    # an inner time step (4 of 0..6), every batch row in turn; a step beyond t_last reaches nothing and is not a case
    return (_cases("gru", gru_op, "x", [(0, 4, 0), (1, 4, 6), (2, 4, 3), (2, 6, 6), (1, 0, 0)], ("grad_w_hh", "grad_b_hh")) +
            _cases("gru", gru_op, "d_h", [(0, 0), (2, 63), (1, 31)], ("grad_w_hh", "grad_b_hh")) +
            _cases("lstm2", lstm2_op, "xproj", [(0, 0), (4, 27), (2, 13), (4, 0), (3, 14)], ("grad_w_hh",)) +
            _cases("lstm2", lstm2_op, "d_h2", [(0, 0), (4, 6)], ("grad_w_hh",)))


# --------------------------------------------------------------------------------------------------
# the small pointwise launches: relu_bwd, act_bwd, row_sum, bcast_add, add_slices  (n = 4·k + 3: a float4 body and a tail)
# --------------------------------------------------------------------------------------------------
PW_N = 4 * 256 + 3
PW_IX = [(0,), (PW_N - 1,), (PW_N - 4,), (1023,), (1024,), (515,)]


@functools.lru_cache(maxsize=None)
def act_bwd_op(relu: bool) -> Op:
    """dy·[y > 0] (+ slope·dy elsewhere): the planted cotangents sit where the mask is open — under a closed ReLU mask torch's
    threshold_backward drops them too, and the reference alone would be finite."""
    g = _gen(f"actbwd{relu}")
    y = rnd(g, PW_N)
    for (i,) in PW_IX:
        y[i] = y[i].abs() + 0.1
    clean = dict(dy=rnd(g, PW_N), y=y)
    slope = 0.2

    def dev(t):
        return {"dx": ops.relu_bwd(t["dy"], t["y"]) if relu else ops.act_bwd(t["dy"], t["y"], slope)}

    def ref(t):
        return {"dx": torch.where(t["y"] > 0, t["dy"], torch.zeros_like(t["dy"]) if relu else slope * t["dy"])}

    return Op(dev, ref, clean)


@functools.lru_cache(maxsize=None)
def row_sum_op() -> Op:
    B, C, L = 3, 5, 4 * 64 + 3
    clean = dict(x=rnd(_gen("rowsum"), B, C, L))
    return Op(lambda t: {"s": ops.row_sum(t["x"].contiguous())}, lambda t: {"s": t["x"].sum(dim=(0, 2))}, clean)


@functools.lru_cache(maxsize=None)
def bcast_add_op() -> Op:
    """out[b] = x[b] + v (fst_bcast_add refuses a row length that is no multiple of 4: N = 4·11)."""
    B, N = 3, 44
    g = _gen("bcast")
    clean = dict(x=rnd(g, B, N), v=rnd(g, N))

    def dev(t):
        out = torch.empty(B, N, device=DEV)
        _lib.check(_lib.load().fst_bcast_add(out.data_ptr(), t["x"].data_ptr(), t["v"].data_ptr(), B, N, _lib.stream_ptr()), "fst_bcast_add")
        return {"out": out}

    return Op(dev, lambda t: {"out": t["x"] + t["v"][None]}, clean)


@functools.lru_cache(maxsize=None)
def add_slices_op() -> Op:
    """dst[b] = a[b] + b[b] over channel slices of wider tensors (batch strides larger than C·L = 15 = 4·3 + 3)."""
    B, C, L, wide = 3, 3, 5, 5
    g = _gen("addslices")
    clean = dict(a=rnd(g, B, wide, L), b=rnd(g, B, wide, L))

    def dev(t):
        dst = torch.zeros(B, wide, L, device=DEV)
        a, b = t["a"][:, 1: 1 + C], t["b"][:, 2: 2 + C]
        _lib.check(_lib.load().fst_add_slices(dst[:, 1:].data_ptr(), wide * L, a.data_ptr(), wide * L, b.data_ptr(), wide * L, B, C, L,
                                              _lib.stream_ptr()), "fst_add_slices")
        return {"dst": dst}

    def ref(t):
        dst = torch.zeros_like(t["a"])
        dst[:, 1: 1 + C] = t["a"][:, 1: 1 + C] + t["b"][:, 2: 2 + C]
        return {"dst": dst}

    return Op(dev, ref, clean)


def pointwise_cases() -> list:
    return (_cases("relu_bwd", functools.partial(act_bwd_op, True), "dy", PW_IX) +
            _cases("act_bwd", functools.partial(act_bwd_op, False), "dy", PW_IX) +
            _cases("row_sum", row_sum_op, "x", [(0, 0, 0), (2, 4, 258), (1, 2, 255), (1, 2, 256), (2, 0, 0), (0, 4, 258)]) +
            _cases("bcast_add", bcast_add_op, "x", [(0, 0), (2, 43), (1, 20)]) + _cases("bcast_add", bcast_add_op, "v", [(0,), (43,)]) +
            _cases("add_slices", add_slices_op, "a", [(0, 1, 0), (2, 3, 4), (1, 2, 2)]) +
            _cases("add_slices", add_slices_op, "b", [(0, 2, 0), (2, 4, 4)]))


CASES = (conv_cases() + conv2_cases() + dense_wgrad_cases() + wn_wgrad_cases() + linear_cases() + gemm_cases() + bn_cases() +
         wn_cases() + flow_cases() + noise_transfer_cases() + cpc_cases() + recurrence_cases() + pointwise_cases())


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_nonfinite_is_neither_swallowed_nor_spread(c: Case):
    op = c.op()
    index = open_index(op.ref_clean()[c.open_mask], c.index) if c.open_mask else c.index
    check_nonfinite(op, c.which, index, POISONS, c.all_inside, c.relu_cone)
