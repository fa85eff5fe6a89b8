"""The WN stack backward on the end conv's cotangent (fst_wn_pack_bwd_proj_stack / fst_wn_stack_bwd_proj): the skip half of
GEMM 3 as (W_end·W_skip,i)ᵀ·do instead of W_skip,iᵀ·(W_endᵀ·do).

The reference of every check is fp64 of the UNFOLDED formula — dacts = W_rsᵀ·[d_a ; W_endᵀ·do] — never the code under test.
Inputs sit between NaN bands and outputs between canary bands (the helpers of tests/test_gpu_wn_routes.py)."""
from __future__ import annotations

import os

import pytest
import torch

from feature_level_style_transfer_for_tsc_amd import _lib, ops
from test_gpu_wn_routes import (STACK_BWD, _cus, _dgrad_f64, _f32, _gate_backward_f64, _gen, assert_close, assert_dg,
                                assert_fence, assert_row_sums, bf3_only, check_rc, dgrad_slot, last_route,
                                max_stack_bwd_layers, nan_in, out_buf, ptrs, rnd)

# (n, h, B, L, nl): the smallest shapes that reach each edge of the skip operand
CASES = [(8, 3, 3, 132, 1),          # h2 = 6: one stage, lane half 1 all dead, top layer only
         (16, 5, 5, 500, "max"),     # h2 = 10: straddles the lane halves, partial column block
         (33, 31, 2, 100, 4),        # h2 = 62: last stage partly live
         (128, 32, 2, 512, 2),       # h2 = 64: four full stages, n = 128
         (8, 3, 300, 64, 3),         # more batch elements than CUs: the grid loop and `primed`
         (120, 25, 4, 512, 8)]       # the workload's channel counts at a small batch


def _layers(nl, n, h, L):
    return max_stack_bwd_layers(n, h, L) if nl == "max" else nl


def _decode(img: torch.Tensor, stages: int) -> torch.Tensor:
    """[stages·16, 128] fp64: hi + lo of an image's stages, row = 16c + 8(l>>5) + j, column = blk·32 + (l&31)."""
    v = img.view(torch.bfloat16)[: stages * 4 * 2 * 64 * 8].view(stages, 4, 2, 2, 32, 8).double()
    return (v[:, :, 0] + v[:, :, 1]).permute(0, 2, 4, 1, 3).reshape(stages * 16, 128)      # [st, hh, j, blk, l31]


def _pack_proj(rs_w32, end_w32, n, h2):
    lib, nl = _lib.load(), len(rs_w32)
    sizes = [lib.fst_wn_bwd_proj_image_bytes(n, h2, int(i == nl - 1)) for i in range(nl)]
    imgs = [out_buf((sz // 4,)) for sz in sizes]
    check_rc(lib.fst_wn_pack_bwd_proj_stack(ptrs(rs_w32), end_w32.data_ptr(), nl, n, h2, ptrs([v for _, v in imgs]),
                                            lib.fst_wn_bwd_proj_image_bytes(n, h2, 0), _lib.stream_ptr()), "pack proj")
    for k, (b, v) in enumerate(imgs):
        assert_fence(b, v, f"image {k}")
    return [v for _, v in imgs], sizes


@bf3_only
@pytest.mark.gpu
@pytest.mark.parametrize("n,h,nl", [(8, 3, 1), (16, 5, 3), (33, 31, 4), (128, 32, 2), (120, 25, 8)])
def test_pack_proj_vs_fp64(n, h, nl):
    lib, g, h2 = _lib.load(), _gen(f"pp{n}-{h}-{nl}"), 2 * h
    CH, CHO = (n + 15) // 16, (h2 + 15) // 16
    rs_w = [rnd(g, n if i == nl - 1 else 2 * n, n, k=n ** -0.5) for i in range(nl)]
    end_w = rnd(g, h2, n, k=n ** -0.5)
    rs32, end32 = [nan_in(w) for w in rs_w], nan_in(end_w)
    imgs, sizes = _pack_proj(rs32, end32, n, h2)
    for i in range(nl):
        last = i == nl - 1
        n_da = 0 if last else CH
        assert sizes[i] == (n_da + CHO) * 8192 + 16
        assert not bool(torch.isnan(imgs[i]).any()), "part of the image was not written"
        w_skip, w_end = rs32[i][(0 if last else n):].double(), end32.double()          # the fp32 values the kernel reads
        got = _decode(imgs[i][n_da * 2048:], CHO)
        want = torch.zeros(CHO * 16, 128, device=got.device, dtype=torch.float64)
        want[:h2, :n] = w_end @ w_skip
        # hi + lo keeps 16 significant bits; the fp32 fmaf chain over n products rounds n times at 2^-24 of the running magnitude
        bound = torch.zeros_like(want)
        bound[:h2, :n] = 2.0 ** -16 * want[:h2, :n].abs() + n * 2.0 ** -24 * (w_end.abs() @ w_skip.abs())
        err = (got - want).abs()
        print(f"  layer {i}: max err {float(err.max()):.3e}, largest bound {float(bound.max()):.3e}, "
              f"worst err/bound {float((err[:h2, :n] / bound[:h2, :n]).max()):.3f}")
        assert bool((err <= bound).all()), f"layer {i}: F outside its bound"
        dead = got.clone()
        dead[:h2, :n] = 0
        assert int((dead != 0).sum()) == 0 and int((imgs[i][-4:] != 0).sum()) == 0, "dead rows / columns / the tail must be exact zeros"
        if not last:                                       # the d_a stages: the bytes of the accumulator-order image
            ref = ops.wn_pack_bwd(rs32[i].contiguous(), n, False, acc_order=True)
            assert torch.equal(imgs[i][: CH * 2048].view(torch.int32), ref[: CH * 2048].view(torch.int32)), f"layer {i}: d_a stages"
    again, _ = _pack_proj(rs32, end32, n, h2)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(again, imgs)), "two packs differ"


@bf3_only
@pytest.mark.gpu
def test_pack_proj_refusals():
    lib = _lib.load()
    w, e = torch.zeros(16, 8, device="cuda"), torch.zeros(6, 8, device="cuda")
    sz = lib.fst_wn_bwd_proj_image_bytes(8, 6, 0)
    buf, img = out_buf((sz // 4,))
    assert lib.fst_wn_bwd_proj_image_bytes(0, 6, 0) == -1 and lib.fst_wn_bwd_proj_image_bytes(8, 0, 1) == -1
    for bad in (dict(h2=65), dict(nl=11), dict(nbytes=sz - 16), dict(end=None)):
        rc = lib.fst_wn_pack_bwd_proj_stack(ptrs([w] * min(bad.get("nl", 2), 10)), None if "end" in bad else e.data_ptr(), bad.get("nl", 2),
                                            8, bad.get("h2", 6), ptrs([img] * min(bad.get("nl", 2), 10)), bad.get("nbytes", sz),
                                            _lib.stream_ptr())
        assert rc == -1, bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(img).all())
    assert_fence(buf, img, "image of a refused pack")


@bf3_only
@pytest.mark.gpu
@pytest.mark.parametrize("n,h,B,L,nl", CASES)
def test_wn_stack_bwd_proj_vs_fp64(n, h, B, L, nl):
    """test_wn_stack_bwd_vs_fp64 layer by layer, with d_out = W_endᵀ·do formed in fp64: the full pass with row sums, a second run
    bit for bit, and the partial pass against the full one."""
    lib, g, h2 = _lib.load(), _gen(f"sp{n}-{B}-{L}-{nl}"), 2 * h
    nl = _layers(nl, n, h, L)
    assert lib.fst_wn_stack_bwd_ok(n, h, L, nl) == 1
    rs_w = [rnd(g, n if i == nl - 1 else 2 * n, n, k=n ** -0.5) for i in range(nl)]
    end_w = rnd(g, h2, n, k=h2 ** -0.5)
    in_w = [rnd(g, 2 * n, n, 3, k=(3 * n) ** -0.5) for _ in range(nl)]
    cond_w = [rnd(g, 2 * n, h, 1, k=h ** -0.5) for _ in range(nl)]
    t = [torch.tanh(rnd(g, B, n, L)) for _ in range(nl)]
    s = [torch.sigmoid(rnd(g, B, n, L)) for _ in range(nl)]
    do64, du64 = rnd(g, B, h2, L), rnd(g, B, h, L)
    rs32, end32 = [_f32(w) for w in rs_w], _f32(end_w)
    # the reference uses the fp32 weights the kernel is given, unfolded: d_out = W_endᵀ·do
    d_out64 = torch.einsum("rm,brt->bmt", end32.double(), do64.float().double())
    img_b, _ = _pack_proj(rs32, end32, n, h2)
    img_d = [ops.wn_pack_dgrad(_f32(in_w[i]), _f32(cond_w[i]), n, h) for i in range(nl)]
    ts = [nan_in(torch.cat([t[i], s[i]], 1)) for i in range(nl)]
    d_o = nan_in(do64)
    grid = min(B, _cus())
    lds = max([16 * 8192 + 8192] + [2 * dgrad_slot(1 << i) for i in range(nl)])
    route = (STACK_BWD, 0, 0, 0, 0, grid, 1, 1, 1, 2, nl, lds)

    def run(partial: bool):
        dgs = [out_buf((B, 2 * n, L))] * nl if partial else [out_buf((B, 2 * n, L)) for _ in range(nl)]
        das = [out_buf((B, n, L))] + [None if partial else out_buf((B, n, L)) for _ in range(nl - 1)]
        bu, d_u0 = out_buf((B, h, L), 3, 1, init=du64)
        rb = None if partial else [out_buf((256, B)) for _ in range(nl)]
        rd = None if partial else [out_buf((128, B)) for _ in range(nl)]
        check_rc(lib.fst_wn_stack_bwd_proj(ptrs(ts), ptrs(img_b), ptrs(img_d), ptrs([v for _, v in dgs]),
                                           ptrs([None if x is None else x[1] for x in das]),
                                           None if partial else ptrs([v for _, v in rb]), None if partial else ptrs([v for _, v in rd]),
                                           d_o.data_ptr(), h2, B * h2 * L, d_u0.data_ptr(), (h + 3) * L, nl, B, L, n, h, B * n * L,
                                           _lib.stream_ptr()), "stack bwd proj")
        last_route(route, f"stack bwd proj (partial={partial})")
        for k, x in enumerate(dgs[:1] if partial else dgs):
            assert_fence(*x, f"dg {k}")
        for k, x in enumerate(das):
            if x is not None:
                assert_fence(*x, f"d_a {k}")
        assert_fence(bu, d_u0, "d_u0")
        for k, x in enumerate((rb or []) + (rd or [])):
            assert_fence(*x, f"row-sum table {k}")
        return ([v for _, v in dgs], [None if x is None else x[1] for x in das], d_u0,
                None if rb is None else [v for _, v in rb], None if rd is None else [v for _, v in rd])

    dgs, das, d_u0, rb, rd = run(False)
    want_u0 = du64
    for i in reversed(range(nl)):
        d_a_in = None if i == nl - 1 else das[i + 1].double()
        dacts, want_dg = _gate_backward_f64(rs32[i].double(), d_a_in, d_out64, t[i], s[i])
        assert_dg(dgs[i], want_dg, dacts, f"layer {i} dg")
        da_ref, du_ref = _dgrad_f64(in_w[i], cond_w[i], dgs[i].double(), 1 << i)
        want_da = da_ref + (0 if d_a_in is None else d_a_in)
        assert_close(das[i], want_da, 2e-5, f"layer {i} d_a")
        want_u0 = want_u0 + du_ref
        assert_row_sums(rb[i][: 2 * n].sum(dim=1), want_dg, f"layer {i} row sums of dg")
        assert_row_sums(rd[i][:n].sum(dim=1), want_da, f"layer {i} row sums of d_a")
    assert_close(d_u0, want_u0, 2e-5, "d_u0")
    again = run(False)
    assert torch.equal(again[2], d_u0) and all(torch.equal(x, y) for x, y in zip(again[0] + again[1], dgs + das))
    assert all(torch.equal(x[: 2 * n], y[: 2 * n]) for x, y in zip(again[3], rb))
    assert all(torch.equal(x[:n], y[:n]) for x, y in zip(again[4], rd))
    p_dgs, p_das, p_u0, _, _ = run(True)
    assert_close(p_das[0], das[0], 2e-5, "partial pass: layer 0 d_a vs the full pass")
    assert_close(p_u0, d_u0, 2e-5, "partial pass: d_u0 vs the full pass")
    assert_close(p_dgs[0], dgs[0], 2e-5, "partial pass: the scratch dg holds layer 0's")


@bf3_only
@pytest.mark.gpu
def test_wn_stack_bwd_proj_refusals_launch_nothing():
    lib, n, h, B, L, nl = _lib.load(), 8, 3, 2, 64, 2
    z = lambda *sh: torch.zeros(*sh, device="cuda")
    ts, dgs, das = [z(B, 2 * n, L)] * nl, [z(B, 2 * n, L)] * nl, [z(B, n, L)] * nl
    imgs = [z(4 * 8192)] * nl
    (bu, d_u0), d_o = out_buf((B, h, L)), z(B, 2 * h, L)

    def call(h2=2 * h, numel_o=B * 2 * h * L, do_ptr=d_o.data_ptr(), Lx=L):
        return lib.fst_wn_stack_bwd_proj(ptrs(ts), ptrs(imgs), ptrs(imgs), ptrs(dgs), ptrs(das), None, None, do_ptr, h2, numel_o,
                                         d_u0.data_ptr(), h * L, nl, B, Lx, n, h, B * n * Lx, _lib.stream_ptr())
    for kw in (dict(h2=65, numel_o=B * 65 * L), dict(h2=0, numel_o=0), dict(numel_o=B * 2 * h * L - 1), dict(do_ptr=d_o.data_ptr() + 4),
               dict(do_ptr=None), dict(Lx=1024, numel_o=B * 2 * h * 1024)):
        assert call(**kw) == -1 and ops.wn_last_route() == (0,) * ops.WN_ROUTE_LEN, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(d_u0).all())
    assert_fence(bu, d_u0, "d_u0 of refused calls")


def _module_inputs(n=16, h=5, B=5, L=500, nl=4):
    g = _gen("skip-proj-module")
    S = ops.WNSpecs(h, n, nl)
    ws = [_f32(rnd(g, *sh, k=(sh[1] * sh[2]) ** -0.5 if len(sh) == 3 else 0.1)) for sh in S.shapes]
    flat = S.flatten(ws).requires_grad_(True)
    x, do = _f32(rnd(g, B, 2 * h, L)), _f32(rnd(g, B, 2 * h, L))
    return S, flat, x, do


def _module_backward(S, flat, x, do, switch: str, partial: bool):
    old = os.environ.get("FST_WN_SKIP_PROJ")
    os.environ["FST_WN_SKIP_PROJ"] = switch
    try:
        u0 = x[:, : S.h].detach().requires_grad_(True)
        o = ops.WNFn.apply(S, u0, flat)
        if partial:
            with ops.partial_backward():
                return torch.autograd.grad(o, (u0,), do)
        return torch.autograd.grad(o, (u0, flat), do)
    finally:
        if old is None:
            del os.environ["FST_WN_SKIP_PROJ"]
        else:
            os.environ["FST_WN_SKIP_PROJ"] = old


@bf3_only
@pytest.mark.gpu
def test_module_backward_switch_on_vs_off():
    """WNFn's backward at (n=16, h=5, B=5, L=500, nl=4).  Switch "2" (the projected form in every pass) against "0" (the d_out
    form): the input gradient and every weight-gradient segment agree to 2e-5 of their scale, and two runs are bit-identical.
    The default "1": a pass with weight gradients keeps the d_out form — the same bits as "0", so the weights an optimiser
    steps to do not move — and a partial pass takes the projected form: one conv-engine launch fewer (the end conv's data
    gradient, the only producer of a [B, n, L] d_out) and the same single stack launch."""
    S, flat, x, do = _module_inputs()
    assert ops.wn_stack_bwd_ok(S.n, S.h, x.size(2), S.n_layers)
    d_u_off, d_w_off = _module_backward(S, flat, x, do, "0", False)
    d_u_on, d_w_on = _module_backward(S, flat, x, do, "2", False)
    assert_close(d_u_on, d_u_off, 2e-5, "d_u0")
    assert not torch.equal(d_u_on, d_u_off), "switch 2 did not take the projected form"
    for k, (a, b) in enumerate(zip(S.unflatten(d_w_on.contiguous()), S.unflatten(d_w_off.contiguous()))):
        assert_close(a, b, 2e-5, f"weight-gradient segment {k}")
    d_u_2, d_w_2 = _module_backward(S, flat, x, do, "2", False)
    assert torch.equal(d_u_2, d_u_on) and torch.equal(d_w_2, d_w_on), "two runs of the projected form differ"
    d_u_def, d_w_def = _module_backward(S, flat, x, do, "1", False)
    assert torch.equal(d_u_def, d_u_off) and torch.equal(d_w_def, d_w_off), "the default moved a pass with weight gradients"

    counts = {}
    p_u = {}
    for switch in ("0", "1", "2"):
        ops.KERNEL_TIMER = ops.KernelTimer()
        try:
            (d_u_p,) = _module_backward(S, flat, x, do, switch, True)
            summ = ops.KERNEL_TIMER.summary()
        finally:
            ops.KERNEL_TIMER = None
        assert_close(d_u_p, d_u_off, 2e-5, f"partial pass (switch {switch}) d_u0")
        p_u[switch] = d_u_p
        fwd_convs = 2                                                         # start and end conv of the forward
        counts[switch] = (sum(v["launches"] for k, v in summ.items() if k.startswith("conv_")) - fwd_convs,
                          summ["wn_stack_bwd_kernel"]["launches"])
        print(f"  switch {switch}: conv-engine launches of the partial backward {counts[switch][0]}, stack launches {counts[switch][1]}")
    # off: W_endᵀ·do and the start conv's; on: the start conv's
    assert counts["0"] == (2, 1) and counts["1"] == (1, 1) and counts["2"] == (1, 1), counts
    assert torch.equal(p_u["1"], p_u["2"]) and not torch.equal(p_u["1"], p_u["0"]), "the default partial pass is the projected form"
