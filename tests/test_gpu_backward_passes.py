"""Repeated and partial backward passes over ONE retained graph — what the joint step does to every autograd Function of
ops.py (``total.backward(retain_graph=True)``, then GradNorm's ``autograd.grad`` passes under ``ops.partial_backward()``, all in
one ``pack_cache`` scope) and what the single-forward / single-backward suites never do.  Needs an MI355X.

``run_passes`` applies one protocol to a Function: forward once; pass A (all inputs, cotangent c1), pass B (data inputs under
``partial_backward``, c2), pass C (= A again), pass D (= B again), each against the fp64 composition in plain torch on the CPU;
after the forward and after every pass every saved tensor, every input and both cotangents are bit-equal to clones taken
before; then one fresh forward per subset of ``requires_grad`` flags (each input alone, the data inputs alone) whose gradients
must be pass A's.  Running state (BatchNorm's running moments, NoiseTransfer's running sums) moves once per forward — checked
against the fp64 single update — and never in a backward.

Comparison rule of a repeated pass (C vs A, D vs B, subset vs A), and where the tolerances against fp64 come from:

| Function                  | repeat rule | why                                                                   | tolerances (source)                                         |
|---------------------------|-------------|-----------------------------------------------------------------------|-------------------------------------------------------------|
| ConvFn, ConvReluFn        | bitwise     | weight-gradient slabs added in a fixed order           | 2e-5 out / dx, 1e-4 dw / db (test_gpu_kernels.py:80-95)     |
| LinearActFn               | bitwise     | fst_gemm: fixed-order slab sum, asserted in test_gpu_gemm.py:123      | 2e-5 out, 5e-5 gradients (test_gpu_gemm.py:117-119)         |
| BNActFn, BNAddBNReluFn    | bitwise     | per-slot sums merged in slot order          | 1e-5 out, 5e-5 gradients (test_gpu_kernels.py:186-189, 237) |
| WNFn, FlowFn              | bitwise     | asserted for the stack backward in test_gpu_full_size.py:374; the     | 2e-5 out, 5e-5 d_u0 / dx, 1e-4 per weight segment           |
|                           |             | layer-wise and conv-engine routes: fixed-order sums    | (test_gpu_full_size.py:362-367)                             |
| CouplingFn, CouplingInvFn | bitwise     | pointwise kernels, per-workgroup slots added by the caller            | 1e-5 (test_gpu_kernels.py:270-290)                          |
| WNFoldFn                  | bitwise     | one row per wave, no cross-workgroup sum                              | 1e-5 out, 5e-5 gradients (test_gpu_rowvec_edges.py:243-247) |
| NoiseTransferFn           | bitwise     | asserted in test_gpu_kernels.py:649                                   | 1e-5 out, 2e-5 gradients (test_gpu_kernels.py:643-647)      |
| LogDetFn                  | bitwise     | single workgroup                                                      | 1e-6 out, 2e-6 gradient (test_gpu_kernels.py:605-606)       |
| CPCNceFn, one panel       | bitwise     | per-workgroup slots added in slot order                | 2e-5 out, 5e-5 gradients (test_gpu_kernels.py:306-307)      |
| CPCNceFn, two panels      | tolerance   | ``denc`` float atomics with > 1 column panel           | the same                                                    |
| GRULastFn                 | bitwise     | persistent launch, dW on fst_gemm; db a torch sum over one dimension  | 2e-5 h, 5e-5 gradients (test_gpu_kernels.py:534-538)        |
| LSTM2Fn                   | bitwise     | one launch each way, one workgroup-private row per sample             | 1e-5 h, 2e-5 gradients (test_gpu_kernels.py:558-561)        |
| RandomLayerFn             | bitwise     | fst_nt_gemm: asserted in test_gpu_kernels.py:661                      | 2e-5 (test_gpu_kernels.py:681-683)                          |
| FixedMatmulFn             | tolerance   | K-split epilogue of fst_conv_gemm: float atomics       | 2e-5 (test_gpu_kernels.py:342)                              |
"""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import ops
from oracle import restatement as R
from test_gpu_kernels import assert_close, bf3_only, ref_conv

DEV = "cuda"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rnd(g, *shape, k=1.0):
    return torch.randn(*shape, generator=g) * k


def _err(got, want, tol, scale=None):
    """None if ``got`` is within tol·scale of ``want`` (scale: max |want| as in ``assert_close`` unless given), else a message."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    if tuple(got.shape) != tuple(want.shape):
        return f"shape {tuple(got.shape)} vs {tuple(want.shape)}"
    scale = max(1e-6, float(want.abs().max())) if scale is None else scale
    err = float((got - want).abs().max()) if got.numel() else 0.0
    return None if err <= tol * scale else f"max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


class Op:
    """One case of the protocol.  ``inputs``: name -> fp32 CPU tensor, every differentiable input of the Function; ``data``: the
    names that are activations (the rest are parameters).  ``apply(t, box)``: calls the Function on the device tensors ``t`` and
    returns its output(s); it may leave ``box["state"]`` = the running-state tensors that this forward updated in place.
    ``ref(t64)``: the same outputs in fp64 plain torch; an output may be a (value, scale) pair; with ``state_ref`` it returns
    (outputs, fp64 state after ONE update).  ``tol``: name -> tolerance of that input's gradient; ``out_tol``: of the outputs.
    ``cot``: indices of the outputs that receive a cotangent (default: every tensor output).  ``const``: device tensors the
    Function reads besides its inputs (index tensors, ratios): never written.  ``segments``: offsets that cut the named 1-d
    input's gradient into the pieces compared each at its own scale."""

    def __init__(self, inputs, data, apply, ref, tol, out_tol, bitwise=True, cot=None, const=(), segments=None, state_tol=None):
        self.inputs, self.data, self.apply, self.ref, self.tol, self.out_tol = inputs, list(data), apply, ref, tol, out_tol
        self.bitwise, self.cot, self.const, self.segments, self.state_tol = bitwise, cot, list(const), segments or {}, state_tol


def run_passes(op: Op):
    bad = []
    names = list(op.inputs)

    def close(got, want, name, what, tol=None, scale=None):
        tol = op.tol[name] if tol is None else tol
        cuts = op.segments.get(name)
        pieces = [(got, want, "")] if cuts is None else [(got[lo:hi], want[lo:hi], f" segment {i}")
                                                         for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:]))]
        for g_, w_, seg in pieces:
            msg = _err(g_, w_, tol, scale)
            if msg:
                bad.append(f"{what}: d{name}{seg}: {msg}")

    def same(got, want, name, what):
        """The rule of a repeated pass: the same bits, or (float atomics) the op's tolerance."""
        if op.bitwise:
            if not torch.equal(got, want):
                bad.append(f"{what}: d{name} differs from the earlier pass by {float((got - want).abs().max()):.3e} (bitwise rule)")
        else:
            close(got, want, name, what)

    def build(requires):
        t = {k: v.to(DEV).requires_grad_(k in requires) for k, v in op.inputs.items()}
        before = {k: v.detach().clone() for k, v in t.items()}
        box = {}
        outs = op.apply(t, box)
        outs = tuple(outs) if isinstance(outs, (tuple, list)) else (outs,)
        for k in names:
            if not torch.equal(t[k].detach(), before[k]):
                bad.append(f"forward wrote its input {k}")
        return t, outs, box.get("state", [])

    with ops.pack_cache():
        const0 = [c.clone() for c in op.const]
        t, outs, state = build(set(names))
        sel = [i for i, o in enumerate(outs) if o is not None] if op.cot is None else list(op.cot)
        g = torch.Generator(device=DEV).manual_seed(1234)
        c1 = [torch.randn(outs[i].shape, generator=g, device=DEV) for i in sel]
        c2 = [torch.randn(outs[i].shape, generator=g, device=DEV) for i in sel]
        saved = [s for s in outs[sel[0]].grad_fn.saved_tensors if s is not None]
        watch = ([(f"saved tensor {i}", s) for i, s in enumerate(saved)] + [(f"input {k}", t[k].detach()) for k in names]
                 + [(f"cotangent {i}", c) for i, c in enumerate(c1 + c2)] + [(f"running state {i}", s) for i, s in enumerate(state)]
                 + [(f"constant {i}", c) for i, c in enumerate(op.const)])
        clones = [w.detach().clone() for _, w in watch]

        def untouched(what):
            for (name, w), c in zip(watch, clones):
                if not torch.equal(w.detach(), c):
                    bad.append(f"{what} wrote {name}: max change {float((w.detach().double() - c.double()).abs().max()):.3e}")

        # ---- the fp64 composition: outputs, running state after one update, gradients for c1 (all inputs) and c2 (data inputs)
        t64 = {k: v.double().requires_grad_(True) for k, v in op.inputs.items()}
        outs64 = op.ref(t64)
        if op.state_tol is not None:
            outs64, state64 = outs64
            for i, (s, s64) in enumerate(zip(state, state64)):
                msg = _err(s, s64, op.state_tol)
                if msg:
                    bad.append(f"running state {i} after one forward is not the fp64 single update: {msg}")
        outs64 = tuple(outs64) if isinstance(outs64, (tuple, list)) else (outs64,)
        for i, o in enumerate(outs):
            if o is not None:
                w, scale = outs64[i] if isinstance(outs64[i], tuple) else (outs64[i], None)
                msg = _err(o, w, op.out_tol, scale)
                if msg:
                    bad.append(f"output {i}: {msg}")
        first = lambda o: o[0] if isinstance(o, tuple) else o
        for c, c0 in zip(op.const, const0):
            if not torch.equal(c, c0):
                bad.append("forward wrote a constant operand")

        def want(wrt, cot):
            got = torch.autograd.grad([first(outs64[i]) for i in sel], [t64[k] for k in wrt], [c.double().cpu() for c in cot],
                                      retain_graph=True)
            return dict(zip(wrt, got))

        def grads(tt, oo, wrt, cot, partial=False):
            with (ops.partial_backward() if partial else contextlib.nullcontext()):
                got = torch.autograd.grad([oo[i] for i in sel], [tt[k] for k in wrt], cot, retain_graph=True)
            return dict(zip(wrt, got))

        wantA, wantB = want(names, c1), (want(op.data, c2) if op.data else {})
        done = {}
        for label, wrt, cot, ref, partial, earlier in (("pass A", names, c1, wantA, False, None), ("pass B", op.data, c2, wantB, True, None),
                                                       ("pass C", names, c1, wantA, False, "pass A"), ("pass D", op.data, c2, wantB, True, "pass B")):
            if not wrt:
                continue                                               # a Function of parameters only has no partial pass
            done[label] = grads(t, outs, wrt, cot, partial)
            for k in wrt:
                close(done[label][k], ref[k], k, f"{label} vs fp64")
                if earlier is not None:
                    same(done[label][k], done[earlier][k], k, f"{label} vs {earlier}")
            untouched(label)

        # ---- subsets: needs_input_grad removes outputs, it never changes the ones that remain
        subsets = [[k] for k in names] + ([op.data] if 1 < len(op.data) < len(names) else [])
        for sub in subsets:
            if len(sub) == len(names):
                continue
            t2, outs2, _ = build(set(sub))
            got = grads(t2, outs2, sub, c1)
            for k in sub:
                same(got[k], done["pass A"][k], k, f"only {'+'.join(sub)} requiring grad vs pass A")
        untouched("the subset forwards")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ conv engine
# ConvFn takes no 1x1 side input, so the scalar-path case of test_gpu_kernels.CASES runs without its C1 = 3 rows.
@pytest.mark.parametrize("fn", ["ConvFn", "ConvReluFn"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("M,C0,ntaps,dil,pad,B,L", [(16, 8, 3, 4, 4, 3, 70),        # L % 4 != 0: the scalar path in both arithmetics
                                                    (64, 20, 2, 1, 0, 3, 128)])     # the split-bf16 path (default arithmetic)
def test_conv_passes(fn, bias, M, C0, ntaps, dil, pad, B, L):
    g = _gen(M + L)
    spec = ops.ConvSpec(M, C0, ntaps, dil, pad)
    inputs = {"x": _rnd(g, B, C0, L), "w": _rnd(g, M, C0, ntaps, k=(C0 * ntaps) ** -0.5)}
    if bias:
        inputs["b"] = _rnd(g, M)
    Fn = getattr(ops, fn)

    def ref(t):
        y = ref_conv(t["x"], t["w"], t.get("b"), dil, pad, ntaps)
        return F.relu(y) if fn == "ConvReluFn" else y
    run_passes(Op(inputs, ["x"], lambda t, box: Fn.apply(spec, t["x"], t["w"], t.get("b")), ref,
                  {"x": 2e-5, "w": 1e-4, "b": 1e-4}, 2e-5))


@bf3_only
@pytest.mark.parametrize("lead,K,N,act,slope", [((9, 25), 96, 64, ops.ACT_NONE, 0.0), ((9, 25), 96, 64, ops.ACT_RELU, 0.0),
                                                ((9, 25), 96, 64, ops.ACT_LEAKY, 0.2), ((9, 25), 50, 1, ops.ACT_RELU, 0.0)])
def test_linear_act_passes(lead, K, N, act, slope):
    g = _gen(K + N + act)
    inputs = {"x": _rnd(g, *lead, K), "W": _rnd(g, N, K, k=K ** -0.5), "b": _rnd(g, N)}

    def ref(t):
        v = F.linear(t["x"], t["W"], t["b"])
        return v if act == ops.ACT_NONE else torch.where(v > 0, v, (slope if act == ops.ACT_LEAKY else 0.0) * v)
    run_passes(Op(inputs, ["x"], lambda t, box: ops.LinearActFn.apply(t["x"], t["W"], t["b"], act, slope), ref,
                  {"x": 5e-5, "W": 5e-5, "b": 5e-5}, 2e-5))


# ------------------------------------------------------------------------------------------------ BatchNorm
def _bn_state(g, C, box, n=1):
    rm = [(_rnd(g, C).to(DEV), (torch.rand(C, generator=g) + 0.5).to(DEV)) for _ in range(n)]
    box["state"] = [s for pair in rm for s in pair]
    return rm


@pytest.mark.parametrize("L", [12, 257])                                           # the 16-byte path and the dword path
@pytest.mark.parametrize("training,relu", [(True, True), (True, False), (False, True)])
def test_bn_act_passes(training, relu, L):
    B, C = 7, 5
    g = _gen(3 + L)
    inputs = {"y": _rnd(g, B, C, L, k=2.0) + 0.7, "gamma": torch.rand(C, generator=g) + 0.5, "beta": _rnd(g, C)}
    rm0, rv0 = _rnd(g, C), torch.rand(C, generator=g) + 0.5

    def apply(t, box):
        box["state"] = [rm0.to(DEV), rv0.to(DEV)]
        return ops.BNActFn.apply(t["y"], t["gamma"], t["beta"], *box["state"], training, relu, 1e-5, 0.1)

    def ref(t):
        rm, rv = rm0.double(), rv0.double()
        out = F.batch_norm(t["y"], rm, rv, t["gamma"], t["beta"], training, 0.1, 1e-5)
        return (F.relu(out) if relu else out), [rm, rv]
    run_passes(Op(inputs, ["y"], apply, ref, {"y": 5e-5, "gamma": 5e-5, "beta": 5e-5}, 1e-5, state_tol=1e-5))


@pytest.mark.parametrize("L", [12, 257])
def test_bn_add_bn_relu_passes(L):
    """The subsets of the protocol are the need_dxa / need_dxb branches of ``_bn_backward_join``: ya alone, yb alone, each parameter
    alone (no dx at all), and ya + yb without parameters."""
    B, C = 7, 5
    g = _gen(4 + L)
    inputs = {"ya": _rnd(g, B, C, L), "ga": _rnd(g, C), "ba": _rnd(g, C), "yb": _rnd(g, B, C, L, k=3.0) - 1, "gb": _rnd(g, C), "bb": _rnd(g, C)}

    def apply(t, box):
        box["state"] = [torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV)]
        s = box["state"]
        return ops.BNAddBNReluFn.apply(t["ya"], t["ga"], t["ba"], s[0], s[1], t["yb"], t["gb"], t["bb"], s[2], s[3], True, 1e-5, 0.1)

    def ref(t):
        s = [torch.zeros(C).double(), torch.ones(C).double(), torch.zeros(C).double(), torch.ones(C).double()]
        out = F.relu(F.batch_norm(t["ya"], s[0], s[1], t["ga"], t["ba"], True, 0.1, 1e-5)
                     + F.batch_norm(t["yb"], s[2], s[3], t["gb"], t["bb"], True, 0.1, 1e-5))
        return out, s
    run_passes(Op(inputs, ["ya", "yb"], apply, ref, {k: 5e-5 for k in inputs}, 1e-5, state_tol=1e-5))


@pytest.mark.parametrize("need_a,need_b", [(True, True), (True, False), (False, True), (False, False)])
def test_bn_join_requires_grad_combinations(need_a, need_b):
    """All four (ya, yb) requires_grad combinations WITH the parameters requiring grad — (False, False) is the branch in which only
    the parameter gradients are wanted — each on its own forward, twice over the retained graph, against the all-inputs pass."""
    B, C, L = 7, 5, 12
    g = _gen(17)
    vals = {"ya": _rnd(g, B, C, L), "ga": _rnd(g, C), "ba": _rnd(g, C), "yb": _rnd(g, B, C, L, k=3.0) - 1, "gb": _rnd(g, C), "bb": _rnd(g, C)}
    cot = _rnd(g, B, C, L).to(DEV)

    def run(requires):
        t = {k: v.to(DEV).requires_grad_(k in requires) for k, v in vals.items()}
        s = [torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV)]
        out = ops.BNAddBNReluFn.apply(t["ya"], t["ga"], t["ba"], s[0], s[1], t["yb"], t["gb"], t["bb"], s[2], s[3], True, 1e-5, 0.1)
        wrt = [k for k in vals if k in requires]
        passes = [dict(zip(wrt, torch.autograd.grad(out, [t[k] for k in wrt], cot, retain_graph=True))) for _ in range(2)]
        return passes

    full = run(set(vals))[0]
    requires = {"ga", "ba", "gb", "bb"} | ({"ya"} if need_a else set()) | ({"yb"} if need_b else set())
    first, second = run(requires)
    for k in first:
        assert torch.equal(first[k], second[k]), f"d{k}: the second pass over the retained graph differs"
        assert torch.equal(first[k], full[k]), f"d{k} depends on which inputs require grad: {float((first[k] - full[k]).abs().max()):.3e}"


# ------------------------------------------------------------------------------------------------ WN stack, flow, coupling
def _wn_weights(S, g, end_k=1.0):
    ws = []
    for j, sh in enumerate(S.shapes):
        fan = sh[1] * sh[2] if len(sh) == 3 else 1
        ws.append(_rnd(g, *sh, k=(1.0 / fan ** 0.5 if len(sh) == 3 else 0.1) * (end_k if j in (4, 5) else 1.0)))
    return S.flatten(ws)


def _wn_f64(S, u0, flat):
    """The WN stack on folded weights in fp64 (the composition of test_gpu_full_size._wn_reference_f64)."""
    nl, n = S.n_layers, S.n
    w = S.unflatten(flat)
    in_w, in_b = w[6: 6 + nl], w[6 + nl: 6 + 2 * nl]
    rs_w, rs_b = w[6 + 2 * nl: 6 + 3 * nl], w[6 + 3 * nl: 6 + 4 * nl]
    a = F.conv1d(u0, w[0], w[1])
    cond = F.conv1d(u0, w[2], w[3])
    out = 0
    for i in range(nl):
        gg = F.conv1d(a, in_w[i], in_b[i], dilation=2 ** i, padding=2 ** i) + cond[:, 2 * n * i: 2 * n * (i + 1)]
        rs = F.conv1d(torch.tanh(gg[:, :n]) * torch.sigmoid(gg[:, n:]), rs_w[i], rs_b[i])
        if i < nl - 1:
            a, out = a + rs[:, :n], out + rs[:, n:]
        else:
            out = out + rs
    return F.conv1d(out, w[4], w[5])


WN_TOL = {"u0": 5e-5, "x": 5e-5, "flat": 1e-4}        # d_u0 (and the flow's dx, which carries it) 5e-5; weight segments 1e-4


@bf3_only
@pytest.mark.parametrize("stack", ["1", "0"])
@pytest.mark.parametrize("n,h,B,L,nl", [(16, 5, 5, 64, 3), (8, 3, 3, 32, 2)])
def test_wn_passes(n, h, B, L, nl, stack, monkeypatch):
    """The whole stack in one launch (FST_WN_STACK=1: partial passes rewrite one dg / d_a scratch tensor layer after layer) and
    the fused launches layer by layer (=0)."""
    monkeypatch.setenv("FST_WN_STACK", stack)
    g = _gen(n * 31 + L + nl)
    S = ops.WNSpecs(h, n, nl)
    assert ops.wn_stack_bwd_ok(n, h, L, nl) == (stack == "1")
    inputs = {"u0": _rnd(g, B, h, L), "flat": _wn_weights(S, g)}
    run_passes(Op(inputs, ["u0"], lambda t, box: ops.WNFn.apply(S, t["u0"], t["flat"]), lambda t: _wn_f64(S, t["u0"], t["flat"]),
                  WN_TOL, 2e-5, segments={"flat": S.offsets}))


def test_wn_passes_after_an_unfused_forward():
    """A length that is no multiple of 4 fails ``wn_fused_ok`` in either arithmetic: the conv engine runs the stack, the gate
    kernel writes acts from the gate input it overwrites in place, and ``_wn_backward_unfused`` walks the layers."""
    n, h, B, L, nl = 8, 3, 3, 30, 2
    g = _gen(77)
    S = ops.WNSpecs(h, n, nl)
    probe = torch.empty(B, n, L, device=DEV)
    assert not ops.wn_fused_ok(n, h, L, probe, probe)
    inputs = {"u0": _rnd(g, B, h, L), "flat": _wn_weights(S, g)}
    run_passes(Op(inputs, ["u0"], lambda t, box: ops.WNFn.apply(S, t["u0"], t["flat"]), lambda t: _wn_f64(S, t["u0"], t["flat"]),
                  WN_TOL, 2e-5, segments={"flat": S.offsets}))


def _coupling_f64(x, o, h, inverse):
    if inverse:
        return torch.cat([x[:, :h], (x[:, h:] - o[:, :h]) / torch.exp(o[:, h:])], 1)
    return torch.cat([x[:, :h], torch.exp(o[:, h:]) * x[:, h:] + o[:, :h]], 1)


def _sums_f64(xn, o, h):
    """(Σ log_s, Σ x_next²) with the scale test_gpu_kernels.py:270-271 holds them to: the sum of the terms' magnitudes."""
    return (o[:, h:].sum(), float(o[:, h:].detach().abs().sum())), ((xn * xn).sum(), float((xn * xn).detach().sum()))


@bf3_only
@pytest.mark.parametrize("inverse,cot", [(False, (0, 2, 3)),        # d_o_ext is None: nobody differentiates the returned WN output
                                         (False, (0, 1, 2, 3)),     # ... and a tensor
                                         (True, (0,)), (True, (0, 1))])
def test_flow_passes(inverse, cot):
    """FlowFn without a pool: the WN backward ACCUMULATES its input gradient into the first h channels of the coupling's dx."""
    n, h, B, L, nl = 16, 5, 5, 64, 3
    g = _gen(9 + len(cot))
    S = ops.WNSpecs(h, n, nl)
    inputs = {"x": _rnd(g, B, 2 * h, L), "flat": _wn_weights(S, g, end_k=0.3)}

    def ref(t):
        o = _wn_f64(S, t["x"][:, :h], t["flat"])
        xn = _coupling_f64(t["x"], o, h, inverse)
        return (xn, o, None, None) if inverse else (xn, o, *_sums_f64(xn, o, h))
    run_passes(Op(inputs, ["x"], lambda t, box: ops.FlowFn.apply(S, t["x"], t["flat"], inverse, None), ref, WN_TOL, 2e-5, cot=cot,
                  segments={"flat": S.offsets}))


@pytest.mark.parametrize("cot", [(0, 1, 2), (1, 2), (0,)])           # every cotangent; only the sums; only xn (set_materialize_grads(False))
def test_coupling_passes(cot):
    B, h, L = 3, 7, 33
    g = _gen(5)
    inputs = {"u": _rnd(g, B, 2 * h, L), "o": _rnd(g, B, 2 * h, L, k=0.3)}

    def ref(t):
        xn = _coupling_f64(t["u"], t["o"], h, False)
        return (xn, *_sums_f64(xn, t["o"], h))
    run_passes(Op(inputs, ["u", "o"], lambda t, box: ops.CouplingFn.apply(t["u"], t["o"]), ref, {"u": 1e-5, "o": 1e-5}, 1e-5, cot=cot))


def test_coupling_inverse_passes():
    B, h, L = 3, 7, 33
    g = _gen(6)
    inputs = {"x": _rnd(g, B, 2 * h, L), "o": _rnd(g, B, 2 * h, L, k=0.3)}
    run_passes(Op(inputs, ["x", "o"], lambda t, box: ops.CouplingInvFn.apply(t["x"], t["o"]),
                  lambda t: _coupling_f64(t["x"], t["o"], h, True), {"x": 1e-5, "o": 1e-5}, 1e-5))


def test_wn_fold_passes():
    n, h, nl = 50, 7, 3
    specs = ops.WNSpecs(h, n, nl)
    normed = [True, False, True, False, False, False] + [True] * nl + [False] * nl + [True] * nl + [False] * nl
    plan = ops.WNFoldPlan(specs, normed)
    g = _gen(n + h)
    inputs, order = {}, []
    for i, (sh, nm) in enumerate(zip(specs.shapes, normed)):
        inputs[f"v{i}"] = _rnd(g, *sh)
        order.append((f"v{i}", f"g{i}" if nm else None))
        if nm:
            inputs[f"g{i}"] = torch.rand(sh[0], *([1] * (len(sh) - 1)), generator=g) + 0.5

    def ref(t):
        return torch.cat([(t[v] if gk is None else torch._weight_norm(t[v], t[gk], 0)).reshape(-1) for v, gk in order])
    run_passes(Op(inputs, [], lambda t, box: ops.WNFoldFn.apply(plan, *[t[k] for k in inputs]), ref, {k: 5e-5 for k in inputs}, 1e-5))


# ------------------------------------------------------------------------------------------------ widgets, losses, recurrences
@pytest.mark.parametrize("B,C,L,device_ratios", [(7, 6, 10, True), (3, 5, 4, False)])
def test_noise_transfer_passes(B, C, L, device_ratios):
    """The running sums are the documented exception to 'a forward writes nothing it was given': they move once per forward (held
    to the fp64 single update) and never in a backward."""
    g = _gen(B + C + L)
    inputs = {"z_t": _rnd(g, B, C, L), "z_s": _rnd(g, B, C, L), "W": _rnd(g, C, C, 1, k=0.2), "bias": _rnd(g, C, k=0.1)}
    avg_t0, avg_s0 = _rnd(g, C, L), _rnd(g, C, L)
    r = (0.37, 1.9)
    rr = tuple(torch.tensor(v, device=DEV) for v in r) if device_ratios else r

    def apply(t, box):
        box["state"] = [avg_t0.to(DEV), avg_s0.to(DEV)]
        return ops.NoiseTransferFn.apply(t["z_t"], t["z_s"], t["W"], t["bias"], *box["state"], rr[0], rr[1])

    def ref(t):
        nt, ns = avg_t0.double() + r[0] * t["z_t"].mean(0), avg_s0.double() + r[1] * t["z_s"].mean(0)
        return F.selu(F.conv1d((nt - ns)[None], t["W"], t["bias"]))[0] + t["z_s"], [nt, ns]
    run_passes(Op(inputs, ["z_t", "z_s"], apply, ref, {k: 2e-5 for k in inputs}, 1e-5, const=rr if device_ratios else (), state_tol=1e-6))


@pytest.mark.parametrize("n", [6, 50])
def test_logdet_passes(n):
    g = torch.Generator().manual_seed(n)
    W = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))[0] + 0.3 * torch.randn(n, n, generator=g, dtype=torch.float64)
    if np.linalg.slogdet(W.numpy())[0] < 0:
        W[:, 0] = -W[:, 0]

    def ref(t):
        ld = torch.logdet(t["W"])
        return ((ld, max(1.0, abs(float(ld.detach())))),)
    run_passes(Op({"W": W.float()}, [], lambda t, box: ops.LogDetFn.apply(t["W"]), ref, {"W": 2e-6}, 1e-6))


@pytest.mark.parametrize("B,Bc,off,C,L,T,t0,dev_t0,bitwise", [
    (37, 37, 0, 50, 128, 64, 9, False, True),          # split-bf16 forward
    (16, 16, 0, 144, 128, 64, 5, False, True),         # C > 64: exact-f32 forward
    (40, 300, 259, 50, 128, 64, 3, False, False),      # two column panels: denc by float atomics -> tolerance
    (37, 37, 0, 50, 128, 64, 9, True, True)])          # the start index as a 0-d int32 device tensor
def test_cpc_nce_passes(B, Bc, off, C, L, T, t0, dev_t0, bitwise):
    g = _gen(B + Bc)
    inputs = {"feat": _rnd(g, B, C, L), "pred": _rnd(g, T, Bc, C, k=0.3)}
    t0_arg = torch.tensor(t0, dtype=torch.int32, device=DEV) if dev_t0 else t0

    def ref(t):
        enc = t["feat"][:, :, t0:t0 + T].permute(2, 0, 1)
        lsm = F.log_softmax(torch.bmm(enc, t["pred"].transpose(1, 2)), dim=-1)
        nce = -lsm[:, torch.arange(B), off + torch.arange(B)].sum() / (B * T)
        return ((nce, max(1.0, abs(float(nce.detach())))),)
    run_passes(Op(inputs, ["feat", "pred"], lambda t, box: ops.CPCNceFn.apply(t["feat"], t["pred"], t0_arg, T, off), ref,
                  {"feat": 5e-5, "pred": 5e-5}, 2e-5, bitwise=bitwise, const=[t0_arg] if dev_t0 else ()))


@pytest.mark.parametrize("B,S,C,t_last,dev_index", [(5, 9, 7, 8, False), (33, 40, 50, 0, True)])
def test_gru_last_passes(B, S, C, t_last, dev_index):
    """The input projection is a torch matmul in front of the Function, as in test_gru_recurrence_matches_torch_gru."""
    H = 64
    torch.manual_seed(B * 100 + S)
    gru = torch.nn.GRU(C, H, num_layers=1, batch_first=True)
    inputs = {"x": torch.randn(B, S, C), "w_ih": gru.weight_ih_l0.detach().clone(), "b_ih": gru.bias_ih_l0.detach().clone(),
              "w_hh": gru.weight_hh_l0.detach().clone(), "b_hh": gru.bias_hh_l0.detach().clone()}
    t_arg = torch.tensor(t_last, dtype=torch.int32, device=DEV) if dev_index else t_last

    def ref(t):
        hcur = torch.zeros(B, H, dtype=torch.float64)
        for s in range(t_last + 1):
            xp, hp = t["x"][:, s] @ t["w_ih"].t() + t["b_ih"], hcur @ t["w_hh"].t() + t["b_hh"]
            rg, zg = torch.sigmoid(xp[:, :H] + hp[:, :H]), torch.sigmoid(xp[:, H:2 * H] + hp[:, H:2 * H])
            ng = torch.tanh(xp[:, 2 * H:] + rg * hp[:, 2 * H:])
            hcur = (1 - zg) * ng + zg * hcur
        return hcur + 0.0 * t["x"].sum()                  # steps beyond t_last: a zero gradient, not an unused input
    run_passes(Op(inputs, ["x"], lambda t, box: ops.GRULastFn.apply(torch.matmul(t["x"], t["w_ih"].t()) + t["b_ih"], t["w_hh"], t["b_hh"], t_arg),
                  ref, {k: 5e-5 for k in inputs}, 2e-5, const=[t_arg] if dev_index else ()))


@pytest.mark.parametrize("B,H", [(5, 50), (2, 7)])
def test_lstm2_passes(B, H):
    torch.manual_seed(H + B)
    lstm = torch.nn.LSTM(H, H, batch_first=True)
    inputs = {"xproj": torch.randn(B, 4 * H), "w_hh": lstm.weight_hh_l0.detach().clone()}

    def ref(t):
        def step(pre, c):
            i, f, gg, o = (torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]),
                           torch.sigmoid(pre[:, 3 * H:]))
            c = f * c + i * gg
            return o * torch.tanh(c), c
        h1, c1 = step(t["xproj"], torch.zeros(B, H, dtype=torch.float64))
        return step(t["xproj"] + h1 @ t["w_hh"].t(), c1)[0]
    run_passes(Op(inputs, ["xproj"], lambda t, box: ops.LSTM2Fn.apply(t["xproj"], t["w_hh"]), ref, {"xproj": 2e-5, "w_hh": 2e-5}, 1e-5))


@bf3_only
def test_random_layer_passes():
    Bq, D, O, ncls = 7, 288, 96, 3
    g = _gen(Bq + D)
    inputs = {"x": _rnd(g, Bq, D), "p": torch.softmax(_rnd(g, Bq, ncls), 1)}
    R0, R1 = _rnd(g, D, O).to(DEV), _rnd(g, ncls, O).to(DEV)
    R0t = R0.t().contiguous()
    run_passes(Op(inputs, ["x", "p"], lambda t, box: ops.RandomLayerFn.apply(t["x"], t["p"], R0, R0t, R1, 1.0 / O ** 0.5),
                  lambda t: (t["x"] @ R0.double().cpu()) / O ** 0.5 * (t["p"] @ R1.double().cpu()), {"x": 2e-5, "p": 2e-5}, 2e-5,
                  const=[R0, R0t, R1]))


def test_fixed_matmul_passes():
    Bx, D, O = 7, 640, 64
    g = _gen(9)
    Rm = _rnd(g, D, O).to(DEV)
    Rt = Rm.t().contiguous()
    run_passes(Op({"x": _rnd(g, Bx, D)}, ["x"], lambda t, box: ops.FixedMatmulFn.apply(t["x"], Rm, Rt), lambda t: t["x"] @ Rm.double().cpu(),
                  {"x": 2e-5}, 2e-5, bitwise=False, const=[Rm, Rt]))


# ------------------------------------------------------------------------------------------------ the WaveGlow pool
@bf3_only
def test_waveglow_pool_over_step_shaped_passes(monkeypatch):
    """Three applications of one small WaveGlow (two forward, one inverse) on a shared input inside one ``pack_cache`` +
    ``shared_fold`` scope, walked as step.py walks its graph: (a) the weighted total with retain_graph, (b) one partial pass per
    loss, (e) the total again, (f) a data-gradient pass made WITHOUT ``partial_backward`` — whose deferred operands the join never
    sees — and the total once more.  fp64: oracle.restatement.

    Tolerances: a WN holds its weight gradients to 1e-4 and its input gradient to 5e-5 (test_gpu_full_size.py:364-367); the three
    flows of an application are chained, each taking the cotangent the one above left, and the errors of a chain of linear maps
    add: n_flows x 1e-4 for parameters, n_flows x 5e-5 for the shared input."""
    n_flows, n_group, n, B, L = 3, 6, 8, 3, 64
    h = n_group // 2
    torch.manual_seed(5)
    wg = fst.WaveGlow(n_flows, n_group, n).to(DEV)
    with torch.no_grad():
        for wn in wg.WN:                                   # the end conv starts at zero: give the WN something to pass back
            wn.end.weight.normal_(0.0, 0.05)
            wn.end.bias.normal_(0.0, 0.05)
    assert any(ops.wn_wgrad_ok(kind, B, L, n, h, 2 ** i) for kind in (0, 1) for i in range(8))
    adds, add0 = [], ops.WNGradPool.add
    monkeypatch.setattr(ops.WNGradPool, "add", lambda self, key, operands: (adds.append(key), add0(self, key, operands))[1])
    g = _gen(41)
    s_host, r2, r3, ri = _rnd(g, B, n_group, L), _rnd(g, B, n_group, L), _rnd(g, B, n_group, L), _rnd(g, B, n_group, L)
    wts = (1.0, 0.5, 2.0)
    tol_p, tol_x = n_flows * 1e-4, n_flows * 5e-5

    def losses(s, forward, infer, f):
        out = [forward(s), forward(0.7 * s + f(r2))]
        return out + [(infer(f(r3) - 0.5 * s) * f(ri)).sum() / ri.numel()]

    s = s_host.to(DEV).requires_grad_(True)
    params = dict(wg.named_parameters())
    grads_now = lambda: {k: p.grad.clone() for k, p in params.items() if p.grad is not None}
    bitwise = ops.wn_stack_bwd_ok(n, h, L, 8)              # the stack backward's run-to-run claim (test_gpu_full_size.py:374)
    with ops.pack_cache(), wg.shared_fold():
        ls = losses(s, lambda u: fst.WaveGlowLoss()(wg(u)), wg.infer, lambda t: t.to(DEV))
        pools = [wn._fold_cache[0][1] for wn in wg.WN]
        assert all(p is not None for p in pools)
        total = sum(w * l for w, l in zip(wts, ls))
        total.backward(retain_graph=True)                                               # (a)
        assert adds, "no application deferred a weight gradient: the pool path did not run"
        assert all(p.pending == {} for p in pools), "operands left in a pool after the full pass"
        ga, ds_a, n_adds = grads_now(), s.grad.clone(), len(adds)
        partial = []
        for l in ls:                                                                    # (b)
            with ops.partial_backward():
                partial.append(torch.autograd.grad(l, s, retain_graph=True)[0])
            assert all(p.pending == {} for p in pools), "operands left in a pool after a partial pass"
        assert len(adds) == n_adds, "a partial pass deferred weight-gradient operands"
        wg.zero_grad()                                                                  # (e)
        total.backward(retain_graph=True)
        ge = grads_now()
        torch.autograd.grad(ls[0], [s], retain_graph=True)                              # (f): a data gradient, no partial_backward
        wg.zero_grad()
        total.backward(retain_graph=True)
        gf = grads_now()
        assert all(p.pending == {} for p in pools)
        inv = {k: wg.convinv[k].W_inverse.double().cpu() for k in range(n_flows)}

    # (c) fp64
    P = R.to_params({k: v.detach().double().cpu().numpy() for k, v in wg.state_dict().items()})
    s64 = s_host.double().requires_grad_(True)
    ls64 = losses(s64, lambda u: R.waveglow_loss(R.waveglow_forward(u, P, n_flows)), lambda z: R.waveglow_infer(z, P, n_flows, inv),
                  lambda t: t.double())
    total64 = sum(w * l for w, l in zip(wts, ls64))
    for l, l64 in zip(ls, ls64):
        assert_close(l, l64, 1e-4, "loss")
    want = dict(zip(params, torch.autograd.grad(total64, [P[k] for k in params], retain_graph=True, allow_unused=True)))
    assert set(ga) == {k for k, v in want.items() if v is not None}
    for k, v in ga.items():
        assert_close(v, want[k], tol_p, f"(a) {k}")
    assert_close(ds_a, torch.autograd.grad(total64, s64, retain_graph=True)[0], tol_x, "(a) shared input")
    for i, (got, l64) in enumerate(zip(partial, ls64)):
        assert_close(got, torch.autograd.grad(l64, s64, retain_graph=True)[0], tol_x, f"(b) partial pass {i}")
    for label, again in (("(e) the total again", ge), ("(f) after a data-gradient pass outside partial_backward", gf)):
        assert set(again) == set(ga)
        for k, v in ga.items():
            if bitwise:
                assert torch.equal(again[k], v), f"{label}: {k} differs by {float((again[k] - v).abs().max()):.3e}"
            else:
                assert_close(again[k], v, tol_p, f"{label}: {k}")


@bf3_only
@pytest.mark.parametrize("apps", [(("fwd", 3), ("fwd", 5), ("inv", 5)),                  # the joint step's three, target batch 3, source 5
                                  (("fwd", 3), ("fwd", 5), ("inv", 5), ("fwd", 2)),     # more sets per key than WN_WGRAD_MAX_SETS, three shapes
                                  (("fwd", 5), ("fwd", 5), ("inv", 5), ("fwd", 5), ("fwd", 3))],   # one shape alone fills more than a launch
                         ids=["3-5-5", "3-5-5-2", "5-5-5-5-3"])
def test_waveglow_pool_over_uneven_batches(apps, monkeypatch):
    """The applications of one small WaveGlow inside one ``pack_cache`` + ``shared_fold`` scope differ in BATCH SIZE, as the flow
    passes of a train step do whenever the target and the source batch differ: every (kind, layer) key of a pool then holds
    operand sets of several shapes, which no single weight-gradient launch can sum.  Every parameter gradient and every input
    gradient against oracle.restatement in fp64, and against the same losses taken outside ``shared_fold`` (no pool: every
    application launches its own weight gradients).  Tolerances: those of test_waveglow_pool_over_step_shaped_passes."""
    n_flows, n_group, n, L = 3, 6, 8, 64
    h = n_group // 2
    assert len(apps) > ops.WN_WGRAD_MAX_SETS or len({B for _, B in apps}) > 1
    torch.manual_seed(5)
    wg = fst.WaveGlow(n_flows, n_group, n).to(DEV)
    with torch.no_grad():
        for wn in wg.WN:
            wn.end.weight.normal_(0.0, 0.05)
            wn.end.bias.normal_(0.0, 0.05)
    assert all(any(ops.wn_wgrad_ok(kind, B, L, n, h, 2 ** i) for kind in (0, 1) for i in range(8)) for _, B in apps)
    adds, add0 = [], ops.WNGradPool.add
    monkeypatch.setattr(ops.WNGradPool, "add", lambda self, key, operands: (adds.append(key), add0(self, key, operands))[1])
    g = _gen(43)
    xs_host = [_rnd(g, B, n_group, L) for _, B in apps]
    rs_host = [_rnd(g, B, n_group, L) for _, B in apps]
    wts = (1.0, 0.5, 2.0, 1.5, 0.75)[: len(apps)]
    tol_p, tol_x = n_flows * 1e-4, n_flows * 5e-5

    def losses(xs, rs, forward, infer):
        return [forward(x) if way == "fwd" else (infer(x) * r).sum() / r.numel() for (way, _), x, r in zip(apps, xs, rs)]

    params = dict(wg.named_parameters())

    def device_pass(scope):
        xs = [x.to(DEV).requires_grad_(True) for x in xs_host]
        wg.zero_grad()
        with ops.pack_cache(), scope():
            ls = losses(xs, [r.to(DEV) for r in rs_host], lambda u: fst.WaveGlowLoss()(wg(u)), wg.infer)
            pools = [wn._fold_cache[0][1] for wn in wg.WN] if wg.WN[0]._fold_cache is not None else []
            sum(w * l for w, l in zip(wts, ls)).backward()
            assert all(p.pending == {} for p in pools), "operands left in a pool after the pass"
        return ls, {k: p.grad.clone() for k, p in params.items() if p.grad is not None}, [x.grad.clone() for x in xs], pools

    ls, got, dxs, pools = device_pass(wg.shared_fold)
    assert len(pools) == n_flows and all(p is not None for p in pools)
    assert adds, "no application deferred a weight gradient: the pool path did not run"
    n_adds = len(adds)
    _, alone, dxs_alone, _ = device_pass(contextlib.nullcontext)
    assert len(adds) == n_adds, "an application outside shared_fold left operands in a pool"
    inv = {k: wg.convinv[k].W_inverse.double().cpu() for k in range(n_flows)}

    P = R.to_params({k: v.detach().double().cpu().numpy() for k, v in wg.state_dict().items()})
    xs64 = [x.double().requires_grad_(True) for x in xs_host]
    ls64 = losses(xs64, [r.double() for r in rs_host], lambda u: R.waveglow_loss(R.waveglow_forward(u, P, n_flows)),
                  lambda z: R.waveglow_infer(z, P, n_flows, inv))
    total64 = sum(w * l for w, l in zip(wts, ls64))
    for l, l64 in zip(ls, ls64):
        assert_close(l, l64, 1e-4, "loss")
    want = dict(zip(params, torch.autograd.grad(total64, [P[k] for k in params], retain_graph=True, allow_unused=True)))
    assert set(got) == set(alone) == {k for k, v in want.items() if v is not None}
    for k, v in got.items():
        assert_close(v, want[k], tol_p, f"pooled {k} vs fp64")
        assert_close(v, alone[k], tol_p, f"pooled {k} vs every application on its own")
    for i, (dx, dx_alone, dx64) in enumerate(zip(dxs, dxs_alone, torch.autograd.grad(total64, xs64))):
        assert_close(dx, dx64, tol_x, f"input {i} {apps[i]} vs fp64")
        assert_close(dx, dx_alone, tol_x, f"input {i} {apps[i]} vs every application on its own")


# ------------------------------------------------------------------------------------------------ _RowSums across passes
def _conv_bn(two_consumers):
    """conv -> BNActFn at OS-CNN size; with ``two_consumers`` the conv output also feeds a plain scaling, so autograd SUMS two
    cotangents and the tensor the conv receives is not the one the BatchNorm backward tagged."""
    B, C, L, C0 = 4, 5, 32, 3
    g = _gen(23)
    vals = {"x": _rnd(g, B, C0, L), "w": _rnd(g, C, C0, 3, k=(3 * C0) ** -0.5), "b": _rnd(g, C), "gamma": torch.rand(C, generator=g) + 0.5,
            "beta": _rnd(g, C)}
    cot, cot2 = _rnd(g, B, C, L), _rnd(g, B, C, L)
    spec = ops.ConvSpec(C, C0, 3, 1, 1)
    t = {k: v.to(DEV).requires_grad_(True) for k, v in vals.items()}
    y = ops.ConvFn.apply(spec, t["x"], t["w"], t["b"])
    y.retain_grad()
    out = ops.BNActFn.apply(y, t["gamma"], t["beta"], torch.zeros(C, device=DEV), torch.ones(C, device=DEV), True, True, 1e-5, 0.1)
    outs, cots = [out], [cot.to(DEV)]
    t64 = {k: v.double().requires_grad_(True) for k, v in vals.items()}
    y64 = ref_conv(t64["x"], t64["w"], t64["b"], 1, 1, 3)
    outs64 = [F.relu(F.batch_norm(y64, torch.zeros(C).double(), torch.ones(C).double(), t64["gamma"], t64["beta"], True, 0.1, 1e-5))]
    if two_consumers:
        outs, cots, outs64 = outs + [y * 1.5], cots + [cot2.to(DEV)], outs64 + [y64 * 1.5]
    db64, dy64 = torch.autograd.grad(outs64, [t64["b"], y64], [c.double().cpu() for c in cots])
    return t, outs, cots, db64, float(dy64.abs().sum(dim=(0, 2)).max())


@pytest.mark.parametrize("two_consumers", [False, True])
def test_row_sums_across_passes(two_consumers, monkeypatch):
    """The conv's bias gradient over two passes of one retained graph: from the BatchNorm backward's per-(sample, channel) sums when
    the BatchNorm is the only consumer (no row-sum launch), from the conv's own reduction of the SUMMED cotangent otherwise — held
    to fp64 relative to the scale of Σ|dy|, as test_conv_bias_gradient_comes_from_the_batchnorm_backward_launch does (2e-6)."""
    calls, row_sum0 = [], ops.row_sum
    monkeypatch.setattr(ops, "row_sum", lambda *a, **k: (calls.append(1), row_sum0(*a, **k))[1])
    with ops.pack_cache():
        t, outs, cots, db64, scale = _conv_bn(two_consumers)
        passes = [torch.autograd.grad(outs, [t["b"], t["x"], t["w"]], cots, retain_graph=True) for _ in range(2)]
    assert len(calls) == (2 if two_consumers else 0), f"{len(calls)} row-sum launches over two passes"
    for i, p in enumerate(passes):
        err = float((p[0].double().cpu() - db64).abs().max())
        assert err <= 2e-6 * scale, f"pass {i}: bias gradient off by {err:.3e} at scale {scale:.3e}"
    assert all(torch.equal(a, b) for a, b in zip(*passes)), "the second pass over the retained graph differs"
