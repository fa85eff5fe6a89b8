"""HIP kernels vs plain torch references (fp64 on the CPU), through the C ABI.  Needs an MI355X.

Tolerances: the f32 MFMA is an exact fp32 FMA chain, so conv results match an fp64 reference to
~1e-6 relative to the operand scale; the split-bf16 path (three bf16 MFMAs per product, fp32
accumulate — the default for 16-byte-alignable shapes) measures ~5e-6.  We assert 2e-5·scale
(forward/data-grad) and 1e-4·scale for weight gradients (fp32 atomics across (b,t) splits, sums of
B·L terms) in BOTH arithmetic modes (``ops.MATH`` = "bf16x3" | "f32").
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from feature_level_style_transfer_for_tsc_amd import ops
from feature_level_style_transfer_for_tsc_amd.structure import generate_layer_parameter_list, out_channels, row_live_ranges

DEV = "cuda"
# kernels that exist in the split-bf16 arithmetic only: skipped when the whole suite runs under FST_MATH=f32
bf3_only = pytest.mark.skipif(ops.MATH != "bf16x3", reason="split-bf16 kernel; FST_MATH=f32 routes around it")


def ref_conv(x, w, bias, dil, pad_left, ntaps):
    halo = (ntaps - 1) * dil
    xp = F.pad(x.double(), (pad_left, halo - pad_left))
    return F.conv1d(xp, w.double(), None if bias is None else bias.double(), dilation=dil)


def assert_close(got, want, tol, what=""):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    scale = max(1e-6, float(want.abs().max()))
    err = float((got - want).abs().max())
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


CASES = [  # M, C0, ntaps, dil, pad_left, C1, B, L
    (8, 6, 1, 1, 0, 0, 3, 40),
    (50, 50, 1, 1, 0, 0, 4, 512),
    (120, 25, 1, 1, 0, 0, 2, 150),
    (50, 120, 1, 1, 0, 0, 2, 300),
    (240, 120, 3, 1, 1, 25, 2, 200),
    (240, 120, 3, 8, 8, 25, 2, 300),
    (240, 120, 3, 128, 128, 25, 2, 512),
    (16, 8, 3, 4, 4, 3, 3, 70),
    (300, 33, 2, 1, 0, 0, 2, 129),
    (240, 120, 3, 2, 2, 25, 2, 512),      # tap shifts -2 / 0 / +2: 16-byte staging that starts 2 samples early
    (240, 120, 3, 1, 1, 25, 3, 100),      # shifts -1 / 0 / +1, a partial last 32-sample tile
    (64, 20, 2, 1, 0, 0, 3, 128),         # one-block rows, shifts 0 / +1
    (100, 30, 3, 3, 3, 0, 2, 64),         # shifts -3 / 0 / +3
]


@pytest.fixture(params=["bf16x3", "f32"])
def arithmetic(request):
    """Run a test once per GEMM arithmetic (ops.MATH), restoring the default afterwards."""
    prev, ops.MATH = ops.MATH, request.param
    yield request.param
    ops.MATH = prev


@pytest.mark.parametrize("M,C0,ntaps,dil,pad_left,C1,B,L", CASES)
def test_conv_forward_backward(M, C0, ntaps, dil, pad_left, C1, B, L, arithmetic):
    g = torch.Generator().manual_seed(M + 7 * C0 + L)
    spec = ops.ConvSpec(M, C0, ntaps, dil, pad_left, C1=C1)
    x0 = torch.randn(B, C0, L, generator=g, dtype=torch.float64, requires_grad=True)
    w0 = (torch.randn(M, C0, ntaps, generator=g, dtype=torch.float64) / (C0 * ntaps) ** 0.5).requires_grad_(True)
    bias = torch.randn(M, generator=g, dtype=torch.float64, requires_grad=True)
    want = ref_conv(x0, w0, bias, dil, pad_left, ntaps)
    x1 = w1 = None
    if C1:
        x1 = torch.randn(B, C1, L, generator=g, dtype=torch.float64, requires_grad=True)
        w1 = (torch.randn(M, C1, 1, generator=g, dtype=torch.float64) / C1 ** 0.5).requires_grad_(True)
        want = want + ref_conv(x1, w1, None, 1, 0, 1)
    dy = torch.randn(B, M, L, generator=g, dtype=torch.float64)
    (want * dy).sum().backward()

    f = lambda t: None if t is None else t.detach().float().to(DEV)
    y = spec.forward(f(x0), f(x1), f(w0), f(w1), f(bias))
    assert_close(y, want, 2e-5, "forward")
    dx0 = spec.grad_x0(f(dy), f(w0))
    assert_close(dx0, x0.grad, 2e-5, "dx0")
    if C1:
        assert_close(spec.grad_x1(f(dy), f(w1)), x1.grad, 2e-5, "dx1")
        res0 = torch.randn(B, C0, L, generator=g)                  # fused: dx0 = res0 + ..., acc1 += ...
        acc1 = torch.randn(B, C1, L, generator=g)
        acc1_d = acc1.to(DEV).clone()
        fused = spec.grad_x01(f(dy), f(w0), f(w1), res0.to(DEV), acc1_d)
        assert_close(fused, res0.double() + x0.grad, 2e-5, "fused dx0")
        assert_close(acc1_d, acc1.double() + x1.grad, 2e-5, "fused dx1")
    dw0, dw1 = spec.grad_w(f(x0), f(x1), f(dy))
    assert_close(dw0, w0.grad, 1e-4, "dw0")
    if C1:
        assert_close(dw1, w1.grad, 1e-4, "dw1")
    assert_close(ops.row_sum(f(dy)), bias.grad, 1e-4, "dbias")


def test_conv_epilogues_split_residual_accumulate():
    g = torch.Generator().manual_seed(1)
    B, L, n = 2, 100, 24
    spec = ops.ConvSpec(2 * n, n)
    x, w, b = torch.randn(B, n, L, generator=g), torch.randn(2 * n, n, 1, generator=g) / n ** 0.5, torch.randn(2 * n, generator=g)
    a, out0 = torch.randn(B, n, L, generator=g), torch.randn(B, n, L, generator=g)
    rs = ref_conv(x, w, b, 1, 0, 1)
    a_next = torch.empty(B, n, L, device=DEV)
    out = out0.to(DEV).clone()
    spec.forward(x.to(DEV), None, w.to(DEV), None, b.to(DEV), y=a_next, res=a.to(DEV), y2=out, msplit=n, flags=ops.EPI_ACC2)
    assert_close(a_next, a.double() + rs[:, :n], 2e-5, "residual half")
    assert_close(out, out0.double() + rs[:, n:], 2e-5, "accumulated half")
    # channel-slice views (explicit batch stride) as input and ACC1 output
    wide = torch.randn(B, 2 * n, L, generator=g).to(DEV)
    spec2 = ops.ConvSpec(n, n)
    w2 = torch.randn(n, n, 1, generator=g) / n ** 0.5
    acc = torch.ones(B, 2 * n, L, device=DEV)
    ops.conv_gemm(spec2.fwd_plan(1), ops.pack_weights(spec2.fwd_plan(1), n, w2.to(DEV), spec2.s_w0()), wide[:, n:], None,
                  None, B, L, n, acc[:, :n], nb=1, flags=ops.EPI_ACC1)
    assert_close(acc[:, :n], 1.0 + ref_conv(wide[:, n:].cpu(), w2, None, 1, 0, 1), 2e-5, "view in / ACC1 out")
    assert float((acc[:, n:] - 1).abs().max()) == 0.0


@pytest.mark.parametrize("which", ["L0", "L1", "L2", "CLF0", "small"])
def test_omni_scale_layers(which, arithmetic):
    """The metric config's omni-scale layers (L=512, C_in=1): masked-tap skipping forward / data-grad, and
    DENSE weight gradients (quirk Q1)."""
    if which == "small":
        lp = generate_layer_parameter_list(1, 13, [41 * 3, 41 * 12 * 2], 2)
        layer, B, L = lp[1], 3, 77
    else:
        lp = generate_layer_parameter_list(1, 89, [1024, 229376], 1)
        layer = {"L0": lp[0], "L1": lp[1], "L2": lp[2], "CLF0": [(50, o, k) for (_, o, k) in lp[0]]}[which]
        B, L = 2, 512
    C0, kmax, M = layer[0][0], layer[-1][2], out_channels(layer)
    live = row_live_ranges(layer)
    g = torch.Generator().manual_seed(len(layer) + M)
    mask = torch.zeros(M, C0, kmax, dtype=torch.float64)
    for m, (lo, hi) in enumerate(live):
        mask[m, :, lo:hi] = 1
    w_raw = torch.randn(M, C0, kmax, generator=g, dtype=torch.float64) / (C0 * 3) ** 0.5
    w = (w_raw * mask).requires_grad_(True)
    x = torch.randn(B, C0, L, generator=g, dtype=torch.float64, requires_grad=True)
    bias = torch.randn(M, generator=g, dtype=torch.float64)
    pl = int((kmax - 1) / 2)
    want = ref_conv(x, w, bias, 1, pl, kmax)
    dy = torch.randn(B, M, L, generator=g, dtype=torch.float64)
    (want * dy).sum().backward()
    spec = ops.ConvSpec(M, C0, kmax, 1, pl, row_live=live, dense_dw=True)
    wd = w_raw.float().to(DEV)
    lo_t = torch.tensor([r[0] for r in live], dtype=torch.int32, device=DEV)
    hi_t = torch.tensor([r[1] for r in live], dtype=torch.int32, device=DEV)
    ops.mask_taps_(wd, lo_t, hi_t)
    assert_close(wd, w, 1e-7, "mask_taps")
    f = lambda t: t.detach().float().to(DEV)
    assert_close(spec.forward(f(x), None, wd, None, f(bias)), want, 2e-5, "omni forward")
    assert_close(spec.grad_x0(f(dy), wd), x.grad, 2e-5, "omni dx")
    dw, _ = spec.grad_w(f(x), None, f(dy))
    assert_close(dw, w.grad, 1e-4, "omni dense dW")               # w.grad is dense: masked taps included
    live_spec = ops.ConvSpec(M, C0, kmax, 1, pl, row_live=live, dense_dw=False)
    dw_live, _ = live_spec.grad_w(f(x), None, f(dy))
    # live-only plans compute a per-block superset of the live taps: exact on live taps, and wherever a masked
    # tap is produced at all it carries the dense value (never garbage)
    assert_close(dw_live.double().cpu() * mask, w.grad * mask, 1e-4, "omni live-only dW (live taps)")
    extra = dw_live.double().cpu() * (1 - mask)
    bad = (extra != 0) & ((extra - w.grad).abs() > 1e-4 * float(w.grad.abs().max()))
    assert not bool(bad.any()), "live-only dW wrote a wrong value on a masked tap"


@pytest.mark.parametrize("L", [70, 72, 512, 1028])      # dword path; 16-byte path with a partial, an exact and >1 row pass
@pytest.mark.parametrize("training,relu", [(True, True), (True, False), (False, True)])
def test_batch_norm(training, relu, L):
    g = torch.Generator().manual_seed(3)
    B, C = 5, 13
    y = (torch.randn(B, C, L, generator=g, dtype=torch.float64) * 2 + 0.7).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    rm_ref, rv_ref = rm.clone(), rv.clone()
    out = F.batch_norm(y, rm_ref, rv_ref, gamma, beta, training, 0.1, 1e-5)
    out = F.relu(out) if relu else out
    dout = torch.randn(B, C, L, generator=g, dtype=torch.float64)
    (out * dout).sum().backward()
    f = lambda t: t.detach().float().to(DEV)
    yd, gd, bd = f(y).requires_grad_(True), f(gamma).requires_grad_(True), f(beta).requires_grad_(True)
    rmd, rvd = f(rm), f(rv)
    got = ops.BNActFn.apply(yd, gd, bd, rmd, rvd, training, relu, 1e-5, 0.1)
    (got * f(dout)).sum().backward()
    assert_close(got, out, 1e-5, "bn out")
    assert_close(yd.grad, y.grad, 5e-5, "bn dx")
    assert_close(gd.grad, gamma.grad, 5e-5, "bn dgamma")
    assert_close(bd.grad, beta.grad, 5e-5, "bn dbeta")
    assert_close(rmd, rm_ref, 1e-5, "running mean")
    assert_close(rvd, rv_ref, 1e-5, "running var")


@pytest.mark.parametrize("B,L", [(256, 512), (7, 70)])
def test_batch_norm_moments_of_an_ill_conditioned_channel(B, L):
    """|mean| / std in the hundreds (the 1x1 shortcut of a univariate extractor, y = w·x + b with a small |w|: 903 measured at
    the metric configuration): Σx² − (Σx)²/N in fp32 has no correct digit of the variance there.  The kernels merge
    (count, mean, M2) partials instead — checked against fp64 — and give the same bits on every run (no atomics)."""
    g = torch.Generator().manual_seed(31)
    C = 6
    ratio = torch.tensor([0.0, 3.0, 50.0, 900.0, 2.0e4, 900.0])
    std = torch.tensor([1.0, 0.5, 0.02, 1e-3, 1e-3, 5.0])
    y = (torch.randn(B, C, L, generator=g, dtype=torch.float64) * std.view(1, C, 1) + (ratio * std).view(1, C, 1)).float()
    yd = y.to(DEV)
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    outs = []
    for _ in range(2):
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        outs.append((ops.BNActFn.apply(yd, gamma, beta, rm, rv, True, False, 0.0, 0.1), rm, rv))
    m64, v64 = y.double().mean(dim=(0, 2)), y.double().var(dim=(0, 2), unbiased=False)
    want = (y.double() - m64.view(1, C, 1)) / torch.sqrt(v64.view(1, C, 1))
    out, rm, rv = outs[0]
    # the input itself is fp32: (x − mean) carries eps·|mean| of representation error, i.e. eps·ratio of a standard deviation
    for c in range(C):
        tol = 2e-5 + 3e-7 * float(ratio[c])
        assert_close(out[:, c], want[:, c], tol, f"normalised channel {c} (|mean|/std = {float(ratio[c]):g})")
    assert_close(rv, 0.9 + 0.1 * y.double().var(dim=(0, 2), unbiased=True), 1e-5, "running variance")
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][2], outs[1][2]), "two runs differ: the reduction is not deterministic"


@pytest.mark.parametrize("L", [50, 52, 512])
def test_bn_add_bn_relu(L):
    g = torch.Generator().manual_seed(4)
    B, C = 4, 9
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ya, yb = mk(B, C, L).requires_grad_(True), (mk(B, C, L) * 3 - 1).requires_grad_(True)
    ga, ba, gb, bb = [mk(C).requires_grad_(True) for _ in range(4)]
    rma, rva, rmb, rvb = torch.zeros(C).double(), torch.ones(C).double(), torch.zeros(C).double(), torch.ones(C).double()
    out = F.relu(F.batch_norm(ya, rma, rva, ga, ba, True, 0.1, 1e-5) + F.batch_norm(yb, rmb, rvb, gb, bb, True, 0.1, 1e-5))
    dout = mk(B, C, L)
    (out * dout).sum().backward()
    f = lambda t: t.detach().float().to(DEV)
    d = [f(t).requires_grad_(True) for t in (ya, ga, ba, yb, gb, bb)]
    bufs = [torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV)]
    got = ops.BNAddBNReluFn.apply(d[0], d[1], d[2], bufs[0], bufs[1], d[3], d[4], d[5], bufs[2], bufs[3], True, 1e-5, 0.1)
    (got * f(dout)).sum().backward()
    assert_close(got, out, 1e-5, "out")
    for t, r, name in zip(d, (ya, ga, ba, yb, gb, bb), ("dya", "dga", "dba", "dyb", "dgb", "dbb")):
        assert_close(t.grad, r.grad, 5e-5, name)
    assert_close(bufs[0], rma, 1e-5); assert_close(bufs[3], rvb, 1e-5)


def test_gate_and_coupling():
    lib_ops = ops
    g = torch.Generator().manual_seed(5)
    B, n, L = 3, 10, 33
    gg = torch.randn(B, 2 * n, L, generator=g, dtype=torch.float64, requires_grad=True)
    acts = torch.tanh(gg[:, :n]) * torch.sigmoid(gg[:, n:])
    dacts = torch.randn(B, n, L, generator=g, dtype=torch.float64)
    (acts * dacts).sum().backward()
    from feature_level_style_transfer_for_tsc_amd import _lib
    lib = _lib.load()
    gd = gg.detach().float().to(DEV).clone()
    ad = torch.empty(B, n, L, device=DEV)
    _lib.check(lib.fst_gate_fwd(gd.data_ptr(), ad.data_ptr(), B, n, L, ad.numel(), _lib.stream_ptr()), "gate_fwd")
    assert_close(ad, acts, 1e-5, "gate acts")
    dg = torch.empty(B, 2 * n, L, device=DEV)
    _lib.check(lib.fst_gate_bwd(gd.data_ptr(), dacts.float().to(DEV).data_ptr(), dg.data_ptr(), B, n, L, ad.numel(), _lib.stream_ptr()), "gate_bwd")
    assert_close(dg, gg.grad, 1e-5, "gate grad")

    h = 7
    u = torch.randn(B, 2 * h, L, generator=g, dtype=torch.float64, requires_grad=True)
    o = (torch.randn(B, 2 * h, L, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
    xn = torch.cat([u[:, :h], torch.exp(o[:, h:]) * u[:, h:] + o[:, :h]], 1)
    r = torch.randn(B, 2 * h, L, generator=g, dtype=torch.float64)
    ((xn * r).sum() + o[:, h:].sum() * 0.5 + (xn * xn).sum() * 0.25).backward()
    ud, od = u.detach().float().to(DEV).requires_grad_(True), o.detach().float().to(DEV).requires_grad_(True)
    xnd, s_ls, s_sq = ops.CouplingFn.apply(ud, od)                       # Σ log_s, Σ xn²: reduced in the same pass
    sums = (s_ls, s_sq)
    assert abs(float(sums[0]) - float(o[:, h:].sum())) <= 1e-5 * float(o[:, h:].abs().sum())
    assert abs(float(sums[1]) - float((xn * xn).sum())) <= 1e-5 * float((xn * xn).sum())
    ((xnd * r.float().to(DEV)).sum() + sums[0] * 0.5 + sums[1] * 0.25).backward()
    assert_close(xnd, xn, 1e-5, "coupling fwd"); assert_close(ud.grad, u.grad, 1e-5, "du"); assert_close(od.grad, o.grad, 1e-5, "do")
    # only the sums are used (no gradient reaches xn directly)
    ud2, od2 = ud.detach().clone().requires_grad_(True), od.detach().clone().requires_grad_(True)
    _, *sums2 = ops.CouplingFn.apply(ud2, od2)
    (sums2[1] * 0.5 - sums2[0]).backward()
    u3, o3 = u.detach().clone().requires_grad_(True), o.detach().clone().requires_grad_(True)
    xn3 = torch.cat([u3[:, :h], torch.exp(o3[:, h:]) * u3[:, h:] + o3[:, :h]], 1)
    ((xn3 * xn3).sum() * 0.5 - o3[:, h:].sum()).backward()
    assert_close(ud2.grad, u3.grad, 1e-5, "du (sums only)"); assert_close(od2.grad, o3.grad, 1e-5, "do (sums only)")

    x = torch.randn(B, 2 * h, L, generator=g, dtype=torch.float64, requires_grad=True)
    o2 = (torch.randn(B, 2 * h, L, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
    xi = torch.cat([x[:, :h], (x[:, h:] - o2[:, :h]) / torch.exp(o2[:, h:])], 1)
    (xi * r).sum().backward()
    xd, o2d = x.detach().float().to(DEV).requires_grad_(True), o2.detach().float().to(DEV).requires_grad_(True)
    xid = ops.CouplingInvFn.apply(xd, o2d)
    (xid * r.float().to(DEV)).sum().backward()
    assert_close(xid, xi, 1e-5, "inv fwd"); assert_close(xd.grad, x.grad, 1e-5, "inv dx"); assert_close(o2d.grad, o2.grad, 1e-5, "inv do")


@pytest.mark.parametrize("B,C,L,T,t0", [(4, 6, 20, 10, 3), (37, 50, 128, 64, 9), (256, 50, 512, 256, 101),
                                        (50, 130, 150, 75, 11), (16, 144, 128, 64, 5)])        # feature widths > 128 (L = 150, 128)
def test_cpc_nce(B, C, L, T, t0):
    g = torch.Generator().manual_seed(B + C)
    feat = torch.randn(B, C, L, generator=g, dtype=torch.float64, requires_grad=True)
    pred = (torch.randn(T, B, C, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
    enc = feat[:, :, t0:t0 + T].permute(2, 0, 1)                  # [T, B, C]
    total = torch.bmm(enc, pred.transpose(1, 2))
    nce = -torch.diagonal(F.log_softmax(total, dim=-1), dim1=1, dim2=2).sum() / (B * T)
    (nce * 1.7).backward()
    fd, pd = feat.detach().float().to(DEV).requires_grad_(True), pred.detach().float().to(DEV).requires_grad_(True)
    got = ops.CPCNceFn.apply(fd, pd, t0, T)
    (got * 1.7).backward()
    assert abs(got.item() - nce.item()) <= 2e-5 * max(1.0, abs(nce.item()))
    assert_close(fd.grad, feat.grad, 5e-5, "dfeat"); assert_close(pd.grad, pred.grad, 5e-5, "dpred")


@pytest.mark.parametrize("B,Bc,off,C,L,T,t0", [(4, 12, 4, 6, 20, 10, 3), (37, 111, 74, 50, 128, 64, 9), (64, 256, 128, 50, 512, 256, 7),
                                               (64, 2048, 1792, 50, 512, 256, 7),      # 8 ranks x 256: eight column panels
                                               (40, 300, 259, 50, 128, 64, 3), (256, 512, 256, 50, 512, 32, 100)])   # ragged last panel
def test_cpc_nce_rows_against_gathered_columns(B, Bc, off, C, L, T, t0):
    """Global-batch data parallelism: B local rows scored against Bc gathered predictions, positives at column off+b."""
    g = torch.Generator().manual_seed(B + Bc)
    feat = torch.randn(B, C, L, generator=g, dtype=torch.float64, requires_grad=True)
    pred = (torch.randn(T, Bc, C, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
    enc = feat[:, :, t0:t0 + T].permute(2, 0, 1)                  # [T, B, C]
    lsm = F.log_softmax(torch.bmm(enc, pred.transpose(1, 2)), dim=-1)          # [T, B, Bc]
    pos = lsm[:, torch.arange(B), off + torch.arange(B)]
    nce = -pos.sum() / (B * T)
    (nce * 0.9).backward()
    fd, pd = feat.detach().float().to(DEV).requires_grad_(True), pred.detach().float().to(DEV).requires_grad_(True)
    got = ops.CPCNceFn.apply(fd, pd, t0, T, off)
    (got * 0.9).backward()
    assert abs(got.item() - nce.item()) <= 2e-5 * max(1.0, abs(nce.item()))
    assert_close(fd.grad, feat.grad, 5e-5, "dfeat"); assert_close(pd.grad, pred.grad, 5e-5, "dpred")


def test_fixed_matmul(arithmetic):
    g = torch.Generator().manual_seed(9)
    Bx, D, O = 7, 640, 64
    x = torch.randn(Bx, D, generator=g, dtype=torch.float64, requires_grad=True)
    R = torch.randn(D, O, generator=g, dtype=torch.float64)
    y = x @ R
    dy = torch.randn(Bx, O, generator=g, dtype=torch.float64)
    (y * dy).sum().backward()
    xd = x.detach().float().to(DEV).requires_grad_(True)
    Rd = R.float().to(DEV)
    got = ops.FixedMatmulFn.apply(xd, Rd, Rd.t().contiguous())
    (got * dy.float().to(DEV)).sum().backward()
    assert_close(got, y, 2e-5, "x@R"); assert_close(xd.grad, x.grad, 2e-5, "dx")


def test_argument_errors_are_reported_not_launched():
    spec = ops.ConvSpec(8, 4)
    x = torch.randn(2, 4, 16, device=DEV)
    w = torch.randn(8, 4, 1, device=DEV)
    plan = spec.fwd_plan(1)
    a = ops.pack_weights(plan, 8, w, spec.s_w0())
    with pytest.raises(RuntimeError, match="msplit"):
        ops.conv_gemm(plan, a, x, None, None, 2, 16, 8, torch.empty(2, 8, 16, device=DEV), msplit=9)
    with pytest.raises(RuntimeError, match="M="):
        ops.conv_gemm(plan, a, x, None, None, 2, 16, 999, torch.empty(2, 8, 16, device=DEV))
    with pytest.raises(ValueError):
        ops.conv_gemm(plan, a, x.transpose(1, 2), None, None, 2, 16, 8, torch.empty(2, 8, 16, device=DEV))


def test_batch_norm_global_batch_arguments_stay_inside_their_buffers():
    """Round-1 fault class (DESIGN.md "Fault log"): the SyncBN path hands the kernels TWO batches — B, the samples the
    tensors hold (launch extent), and B_total >= B, the samples the moments were summed over (only a divisor).  Calling
    fst_bn_finalize / fst_bn_bwd_apply with B_total = 3*B on buffers padded with canaries must (1) leave the padding
    untouched, (2) divide by B_total*L, and (3) a launch batch that does not describe the buffers is refused on the host."""
    from feature_level_style_transfer_for_tsc_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(11)
    B, C, L, PAD, CANARY = 4, 6, 40, 4096, 1234.5
    n = B * C * L

    def padded(src=None):
        buf = torch.full((PAD + n + PAD,), CANARY, device=DEV)
        body = buf[PAD: PAD + n].view(B, C, L)
        if src is not None:
            body.copy_(src)
        return buf, body

    y_h, dy_h = torch.randn(B, C, L, generator=g), torch.randn(B, C, L, generator=g)
    (ybuf, y), (dybuf, dy), (dxbuf, dx) = padded(y_h), padded(dy_h), padded()
    gamma, beta = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV)
    rmean, rvar = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    part = torch.full((C, ops.BN_SLOTS, 4), CANARY, device=DEV)      # every slot must be written by the kernel (no zero fill)
    _lib.check(lib.fst_bn_stats(y.data_ptr(), B, C, L, part.data_ptr(), n, _lib.stream_ptr()), "bn_stats")
    assert float(part[:, :, 0].sum(dim=1).min()) == B * L and float(part[:, :, 0].sum(dim=1).max()) == B * L
    B_total = 3 * B
    part_g = part.repeat(1, 3, 1).contiguous()                      # as if two more ranks held the same samples
    stats = torch.empty(4 * C, device=DEV)
    _lib.check(lib.fst_bn_finalize(part_g.data_ptr(), 3 * ops.BN_SLOTS, gamma.data_ptr(), beta.data_ptr(), rmean.data_ptr(),
                                   rvar.data_ptr(), 1, C, 1e-5, 0.1, stats.data_ptr(), _lib.stream_ptr()), "bn_finalize")
    assert_close(stats[:C], y_h.mean(dim=(0, 2)), 1e-5, "mean over B_total*L samples")
    assert_close(1.0 / stats[C: 2 * C].double() ** 2 - 1e-5, y_h.double().var(dim=(0, 2), unbiased=False), 1e-5, "variance over B_total*L samples")
    red = torch.full((2, C, ops.BN_SLOTS), CANARY, device=DEV)
    _lib.check(lib.fst_bn_bwd_reduce(dy.data_ptr(), y.data_ptr(), None, stats.data_ptr(), B, C, L, 0, red.data_ptr(), n,
                                     _lib.stream_ptr()), "bn_bwd_reduce")
    red_g = (red.sum(dim=2) * 3).view(2 * C).contiguous()
    rsum = torch.full((B * C + 2 * PAD,), CANARY, device=DEV)
    _lib.check(lib.fst_bn_bwd_apply(dy.data_ptr(), y.data_ptr(), None, stats.data_ptr(), red_g.data_ptr(), 1, None, dx.data_ptr(),
                                    rsum[PAD:].data_ptr(), B, C, L, 0, 1, B_total, n, _lib.stream_ptr()), "bn_bwd_apply")
    torch.cuda.synchronize()
    # the per-(sample, channel) sums of dx the launch leaves for the bias gradient of the conv in front
    assert bool((rsum[:PAD] == CANARY).all()) and bool((rsum[PAD + B * C:] == CANARY).all()), "row sums: padding was written"
    rs_err = float((rsum[PAD: PAD + B * C].view(B, C).double() - dx.double().sum(dim=2)).abs().max())
    assert rs_err <= 1e-5 * float(dx.abs().sum(dim=2).max()), f"row sums of dx: {rs_err:.3e}"
    for name, buf in (("y", ybuf), ("dy", dybuf), ("dx", dxbuf)):
        assert bool((buf[:PAD] == CANARY).all()) and bool((buf[PAD + n:] == CANARY).all()), f"{name}: padding was written"
    # the same formula in fp64: means over the B_total*L global samples (three copies of the local ones)
    yd, dyd = y_h.double(), dy_h.double()
    mean, var = yd.mean(dim=(0, 2), keepdim=True), yd.var(dim=(0, 2), unbiased=False, keepdim=True)
    xh = (yd - mean) / torch.sqrt(var + 1e-5)
    want = gamma.double().cpu().view(1, C, 1) / torch.sqrt(var + 1e-5) * (
        dyd - dyd.mean(dim=(0, 2), keepdim=True) - xh * (dyd * xh).mean(dim=(0, 2), keepdim=True))
    assert_close(dx, want, 1e-4, "dx with B_total = 3B")
    # (3) the round-1 bug itself — the global batch passed as the launch batch — is now an error return, not a walk
    rc = lib.fst_bn_bwd_apply(dy.data_ptr(), y.data_ptr(), None, stats.data_ptr(), red_g.data_ptr(), 1, None, dx.data_ptr(), None,
                              B_total, C, L, 0, 1, B_total, n, _lib.stream_ptr())
    assert rc < 0 and b"element count" in lib.fst_last_error()
    rc = lib.fst_bn_apply(y.data_ptr(), stats.data_ptr(), None, None, dx.data_ptr(), B_total, C, L, 0, n, _lib.stream_ptr())
    assert rc < 0
    rc = lib.fst_gate_fwd(y.data_ptr(), dx.data_ptr(), 2 * B, C, L, n, _lib.stream_ptr())
    assert rc < 0
    torch.cuda.synchronize()
    assert bool((dxbuf[:PAD] == CANARY).all()) and bool((dxbuf[PAD + n:] == CANARY).all())


@bf3_only
@pytest.mark.parametrize("n,h,B,L,dil,first,last", [
    (120, 25, 2, 512, 1, True, False), (120, 25, 2, 512, 8, False, False), (120, 25, 3, 512, 128, False, False),
    (120, 25, 2, 512, 128, False, True), (120, 25, 2, 200, 4, False, False),      # partial last tile (200 = 128 + 72)
    (8, 3, 3, 40, 2, False, False), (8, 3, 2, 40, 1, True, True), (127, 16, 1, 256, 16, False, False), (33, 31, 2, 132, 64, False, False)])
def test_fused_wn_layer_forward(n, h, B, L, dil, first, last):
    """fst_wn_layer_fwd (dilated conv + cond rows + bias -> gate -> res_skip + bias -> residual / skip adds in ONE launch)
    against fp64 torch; the saved gate halves and acts too."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(n * 1000 + L + dil)
    rnd = lambda *s, k=1.0: torch.randn(*s, generator=g, dtype=torch.float64) * k
    a, u0full = rnd(B, n, L), rnd(B, 2 * h, L)
    u0 = u0full[:, :h]                                                     # a channel-slice view, as WaveGlow passes it
    in_w, cond_w = rnd(2 * n, n, 3, k=(3 * n) ** -0.5), rnd(2 * n, h, 1, k=h ** -0.5)
    in_b, cond_b = rnd(2 * n, k=0.3), rnd(2 * n, k=0.3)
    R = n if last else 2 * n
    rs_w, rs_b = rnd(R, n, 1, k=n ** -0.5), rnd(R, k=0.3)
    out0 = rnd(B, n, L)
    gg = F.conv1d(a, in_w, in_b, dilation=dil, padding=dil) + F.conv1d(u0, cond_w, cond_b)
    t, s = torch.tanh(gg[:, :n]), torch.sigmoid(gg[:, n:])
    acts = t * s
    r = F.conv1d(acts, rs_w, rs_b)
    a_next = None if last else a + r[:, :n]
    out = (0 if first else out0) + (r if last else r[:, n:])
    f = lambda x: x.float().to(DEV).contiguous()
    ad, u0d = f(a), f(u0full)[:, :h]
    img = ops.wn_pack_layer(f(in_w), f(cond_w), f(in_b), f(cond_b), f(rs_w), f(rs_b), n, h, last)
    ts_d, acts_d = torch.full((B, 2 * n, L), 7.0, device=DEV), torch.full((B, n, L), 7.0, device=DEV)
    an_d = None if last else torch.full((B, n, L), 7.0, device=DEV)
    out_d = torch.full((B, n, L), 7.0, device=DEV) if first else f(out0)
    assert ops.wn_fused_ok(n, h, L, ad, u0d)
    ops.wn_layer_fwd(ad, u0d, img, ts_d, acts_d, an_d, out_d, first, last, n, h, dil)
    # the gate halves inherit the GEMM's error (split-bf16: ~5e-6 of the pre-activation scale) through tanh' <= 1
    gtol = 1e-5 * float(gg.abs().max())
    assert_close(ts_d[:, :n], t, gtol, "t")
    assert_close(ts_d[:, n:], s, gtol, "s")
    assert_close(acts_d, acts, gtol, "acts")
    if not last:
        assert_close(an_d, a_next, 2e-5, "a_next")
    assert_close(out_d, out, 2e-5, "out")
    # and without the optional acts output
    ts2, out2 = torch.empty_like(ts_d), (torch.empty_like(out_d) if first else f(out0))
    an2 = None if last else torch.empty_like(an_d)
    ops.wn_layer_fwd(ad, u0d, img, ts2, None, an2, out2, first, last, n, h, dil)
    assert torch.equal(ts2, ts_d) and torch.equal(out2, out_d)


@bf3_only
@pytest.mark.parametrize("n,B,L,last", [(120, 2, 512, False), (120, 3, 512, True), (120, 2, 200, False), (8, 3, 40, False),
                                        (8, 2, 40, True), (128, 1, 256, False), (33, 2, 132, False)])
def test_fused_wn_layer_backward(n, B, L, last):
    """fst_wn_layer_bwd (transposed res_skip GEMM over [d_a ; d_out] -> gate backward in registers) against fp64 torch."""
    g = torch.Generator().manual_seed(n * 100 + L + int(last))
    rnd = lambda *s, k=1.0: torch.randn(*s, generator=g, dtype=torch.float64) * k
    R = n if last else 2 * n
    rs_w = rnd(R, n, k=n ** -0.5)
    d_a, d_out = (None if last else rnd(B, n, L)), rnd(B, n, L)
    t, s = torch.tanh(rnd(B, n, L)), torch.sigmoid(rnd(B, n, L))
    d_r = d_out if last else torch.cat([d_a, d_out], 1)
    dacts = torch.einsum("rm,brt->bmt", rs_w, d_r)
    want = torch.cat([dacts * s * (1 - t * t), dacts * t * s * (1 - s)], 1)
    f = lambda x: None if x is None else x.float().to(DEV).contiguous()
    dg = torch.full((B, 2 * n, L), 7.0, device=DEV)
    sums = ops.wn_layer_bwd(f(d_a), f(d_out), f(torch.cat([t, s], 1)), ops.wn_pack_bwd(f(rs_w), n, last), dg, last, n,
                            want_row_sums=True)
    assert_close(dg, want, 1e-5 * float(dacts.abs().max()) / max(1e-6, float(want.abs().max())) + 1e-6, "dg")
    assert_close(sums, want.sum(dim=(0, 2)), 2e-5 * float(want.abs().sum(dim=(0, 2)).max()) / max(1e-9, float(want.sum(dim=(0, 2)).abs().max())),
                 "row sums of dg (bias gradient)")
    dg2 = torch.empty_like(dg)
    assert ops.wn_layer_bwd(f(d_a), f(d_out), f(torch.cat([t, s], 1)), ops.wn_pack_bwd(f(rs_w), n, last), dg2, last, n) is None
    assert torch.equal(dg2, dg)


def test_weight_gradient_with_product_operand(arithmetic):
    """res_skip weight gradient with x = t·s formed while staging (x0 = the t rows of the saved [B, 2n, L] gate halves,
    x0_mul_off = n·L to the s rows) equals the gradient against a materialised acts tensor."""
    g = torch.Generator().manual_seed(77)
    for n, B, L, M in ((120, 2, 512, 240), (8, 3, 40, 8), (34, 2, 132, 68), (33, 2, 132, 33)):
        ts = torch.randn(B, 2 * n, L, generator=g, dtype=torch.float64)
        dy = torch.randn(B, M, L, generator=g, dtype=torch.float64)
        acts = ts[:, :n] * ts[:, n:]
        want = torch.einsum("bmt,bct->mc", dy, acts)
        spec = ops.ConvSpec(M, n)
        tsd = ts.float().to(DEV)
        if M == 2 * n:
            dyd = dy.float().to(DEV)
            dw, _ = spec.grad_w(tsd[:, :n], None, dyd[:, :n].contiguous(), dyd[:, n:].contiguous(), msplit=n, x0_mul_off=n * L)
        else:
            dw, _ = spec.grad_w(tsd[:, :n], None, dy.float().to(DEV), x0_mul_off=n * L)
        assert_close(dw[:, :, 0], want, 1e-4, f"dW with product operand n={n}")


@pytest.mark.parametrize("B,S,C,t_last,dev_index", [(5, 9, 7, 8, False), (256, 128, 50, 77, True), (33, 40, 50, 0, False),
                                                    (64, 128, 50, 127, True), (3, 1, 4, 0, False)])
def test_gru_recurrence_matches_torch_gru(B, S, C, t_last, dev_index):
    """ops.GRULastFn (input projection GEMM outside, the recurrence as one persistent launch each way) against
    torch.nn.GRU in float64 on the CPU: h at step t_last, gradients of the input and of all four parameter tensors."""
    H = 64
    torch.manual_seed(B * 100 + S)
    gru = torch.nn.GRU(C, H, num_layers=1, batch_first=True).double()
    x = torch.randn(B, S, C, dtype=torch.float64, requires_grad=True)
    r = torch.randn(B, H, dtype=torch.float64)
    out, _ = gru(x)
    (out[:, t_last] * r).sum().backward()
    f = lambda t: t.detach().float().to(DEV).requires_grad_(True)
    xd, w_ih, w_hh, b_ih, b_hh = f(x), f(gru.weight_ih_l0), f(gru.weight_hh_l0), f(gru.bias_ih_l0), f(gru.bias_hh_l0)
    xproj = torch.matmul(xd, w_ih.t()) + b_ih
    t_arg = torch.tensor(t_last, dtype=torch.int32, device=DEV) if dev_index else t_last
    h = ops.GRULastFn.apply(xproj, w_hh, b_hh, t_arg)
    (h * r.float().to(DEV)).sum().backward()
    assert_close(h, out[:, t_last], 2e-5, "h_t")
    assert_close(xd.grad, x.grad, 5e-5, "dx")
    for got, want, name in ((w_ih, gru.weight_ih_l0, "dW_ih"), (w_hh, gru.weight_hh_l0, "dW_hh"), (b_ih, gru.bias_ih_l0, "db_ih"),
                            (b_hh, gru.bias_hh_l0, "db_hh")):
        assert_close(got.grad, want.grad, 5e-5, name)
    assert float(xd.grad[:, t_last + 1:].abs().max()) == 0.0 if t_last + 1 < S else True      # steps beyond t_last: no gradient


@pytest.mark.parametrize("B,H", [(5, 50), (256, 175), (3, 256), (2, 7)])
def test_two_step_lstm_matches_torch_lstm(B, H):
    """fst_lstm2_fwd / _bwd (ProbTransfer: nn.LSTM over the pooled feature repeated twice, h_n) against torch.nn.LSTM in
    fp64 — output and every gradient (input, W_ih, W_hh, both biases)."""
    from feature_level_style_transfer_for_tsc_amd.widgets import ProbTransfer
    torch.manual_seed(H + B)
    ref = torch.nn.LSTM(H, H, batch_first=True).double()
    x = torch.randn(B, H, dtype=torch.float64, requires_grad=True)
    _, (h_n, _) = ref(torch.stack([x, x], dim=1))
    w = torch.randn(B, H, dtype=torch.float64)
    (h_n[0] * w).sum().backward()
    pt = ProbTransfer(H).to(DEV)
    pt.model.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    xd = x.detach().float().to(DEV).requires_grad_(True)
    out = pt(xd)
    (out * w.float().to(DEV)).sum().backward()
    assert_close(out, h_n[0], 1e-5, "h_n")
    assert_close(xd.grad, x.grad, 2e-5, "dx")
    for name in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
        assert_close(getattr(pt.model, name).grad, getattr(ref, name).grad, 2e-5, name)


@bf3_only
@pytest.mark.parametrize("n,h,B,L,dil,res", [(120, 25, 2, 512, 1, True), (120, 25, 2, 512, 2, True), (120, 25, 3, 512, 16, True),
                                             (120, 25, 2, 512, 128, False), (120, 25, 2, 1024, 64, True), (120, 25, 2, 200, 4, True),
                                             (8, 3, 3, 40, 2, True), (128, 32, 1, 256, 32, False), (33, 31, 2, 132, 8, True),
                                             # more tiles than CUs: persistent workgroups, the next tile's first stages
                                             # streaming in under the epilogue (the ring has 2 slots at every dilation)
                                             (8, 3, 131, 1024, 2, True), (16, 5, 67, 2048, 128, True), (8, 3, 300, 500, 16, False)])
def test_fused_wn_layer_data_gradient(n, h, B, L, dil, res):
    """fst_wn_layer_dgrad (transposed dilated 3-tap conv with one tap-merged window per 16 channels + the transposed
    conditioning 1x1 as a fifth row block) against autograd of the fp64 forward convs."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(n + L + dil)
    rnd = lambda *s, k=1.0: torch.randn(*s, generator=g, dtype=torch.float64) * k
    in_w, cond_w = rnd(2 * n, n, 3, k=(3 * n) ** -0.5), rnd(2 * n, h, 1, k=h ** -0.5)
    a, u0 = rnd(B, n, L).requires_grad_(True), rnd(B, h, L).requires_grad_(True)
    gg = F.conv1d(a, in_w, None, dilation=dil, padding=dil) + F.conv1d(u0, cond_w)
    dg = rnd(B, 2 * n, L)
    da_ref, du_ref = torch.autograd.grad(gg, (a, u0), dg)
    d_a_in, d_u0_in = (rnd(B, n, L) if res else None), rnd(B, h, L)
    f = lambda x: None if x is None else x.float().to(DEV).contiguous()
    d_u0 = f(d_u0_in)
    got, sums = ops.wn_layer_dgrad(f(dg), ops.wn_pack_dgrad(f(in_w), f(cond_w), n, h), f(d_a_in), d_u0, n, h, dil, want_row_sums=True)
    want_da = da_ref + (d_a_in if res else 0)
    assert_close(got, want_da, 2e-5, "d_a")
    assert_close(d_u0, du_ref + d_u0_in, 2e-5, "d_u0")
    assert_close(sums, want_da.sum(dim=(0, 2)), 2e-5 * float(want_da.abs().sum(dim=(0, 2)).max()) / max(1e-9, float(want_da.sum(dim=(0, 2)).abs().max())),
                 "row sums of d_a (bias gradient)")


@pytest.mark.parametrize("n", [1, 2, 6, 50, 96])
def test_logdet_and_inverse_transpose_kernel(n):
    """fst_logdet_inv against fp64 numpy: log|det W|, its gradient W^{-T}, and torch.logdet's conventions for det <= 0."""
    import numpy as np
    g = torch.Generator().manual_seed(n)
    W = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))[0] + 0.3 * torch.randn(n, n, generator=g, dtype=torch.float64)
    if np.linalg.slogdet(W.numpy())[0] < 0:
        W[:, 0] = -W[:, 0]
    Wd = W.float().to(DEV).requires_grad_(True)
    ld = ops.logdet(Wd)
    (ld * 1.7).backward()
    sign, want = np.linalg.slogdet(W.float().double().numpy())
    assert sign > 0 and abs(float(ld) - want) <= 1e-6 * max(1.0, abs(want))
    assert_close(Wd.grad, 1.7 * torch.linalg.inv(W.float().double()).t(), 2e-6, "d logdet / dW = W^-T")
    if n >= 2:
        Wn = W.clone(); Wn[0] = -Wn[0]                                        # negative determinant -> NaN, like torch.logdet
        assert torch.isnan(ops.logdet(Wn.float().to(DEV)))
        Ws = W.clone(); Ws[1] = Ws[0]                                          # singular: -inf, or the log of a rounding-level pivot
        sing = float(ops.logdet(Ws.float().to(DEV)))
        assert sing == float("-inf") or sing != sing or sing < -25.0
        assert float(ops.logdet(torch.zeros(n, n, device=DEV))) == float("-inf")   # an exactly zero pivot



@pytest.mark.parametrize("B,C,L,device_ratios", [(256, 50, 512, False), (7, 6, 10, True), (33, 50, 64, True), (3, 5, 4, False)])
def test_noise_transfer_kernels_vs_fp64_composition(B, C, L, device_ratios):
    """csrc/widgets.hip (ops.NoiseTransferFn) against the reference's composition (widgets.py:150-167) in fp64: output, the
    in-place running sums, and the gradients of both latent batches and of the 1x1 conv; bit-identical when repeated."""
    g = torch.Generator(device=DEV).manual_seed(B + C + L)
    rnd = lambda *s: torch.randn(*s, generator=g, device=DEV)
    z_t, z_s = rnd(B, C, L).requires_grad_(True), rnd(B, C, L).requires_grad_(True)
    W, bias = (rnd(C, C, 1) * 0.2).requires_grad_(True), (rnd(C) * 0.1).requires_grad_(True)
    avg_t0, avg_s0 = rnd(C, L), rnd(C, L)
    r = (0.37, 1.9)
    cot = rnd(B, C, L)

    def run():
        avg_t, avg_s = avg_t0.clone(), avg_s0.clone()
        rr = tuple(torch.tensor(v, device=DEV) for v in r) if device_ratios else r
        out = ops.NoiseTransferFn.apply(z_t, z_s, W, bias, avg_t, avg_s, rr[0], rr[1])
        grads = torch.autograd.grad(out, (z_t, z_s, W, bias), cot)
        return out.detach(), avg_t, avg_s, grads

    out, avg_t, avg_s, grads = run()
    zt64, zs64 = z_t.detach().double().requires_grad_(True), z_s.detach().double().requires_grad_(True)
    W64, b64 = W.detach().double().requires_grad_(True), bias.detach().double().requires_grad_(True)
    nt = avg_t0.double() + r[0] * zt64.mean(0)
    ns = avg_s0.double() + r[1] * zs64.mean(0)
    want = F.selu(F.conv1d((nt - ns)[None], W64, b64))[0] + zs64
    wg = torch.autograd.grad(want, (zt64, zs64, W64, b64), cot.double())
    assert_close(out, want.detach(), 1e-5, "NoiseTransfer out")
    assert_close(avg_t, nt.detach(), 1e-6, "running sum (target)")
    assert_close(avg_s, ns.detach(), 1e-6, "running sum (source)")
    for got, ref, name in zip(grads, wg, ("dz_t", "dz_s", "dW", "dbias")):
        assert_close(got, ref, 2e-5, name)
    out2, avg_t2, avg_s2, grads2 = run()
    assert torch.equal(out, out2) and torch.equal(avg_t, avg_t2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))


@bf3_only
@pytest.mark.parametrize("M,N,K", [(256, 1024, 25600), (256, 25600, 1024), (3, 5, 32), (200, 130, 96), (33, 129, 64), (1, 1, 32),
                                   (100, 200, 8192), (37, 70, 4096)])      # dead row / k-row blocks AND several stages per workgroup
def test_nt_gemm_vs_fp64(M, N, K):
    """fst_nt_gemm (C = A·Bmᵀ on the time-as-k kernel, K split into slabs added in a fixed order) against fp64; bit-identical twice."""
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    A, Bm = torch.randn(M, K, generator=g, device=DEV), torch.randn(N, K, generator=g, device=DEV)
    C = ops.nt_gemm(A, Bm)
    assert_close(C, A.double() @ Bm.double().t(), 2e-5, f"nt_gemm {M}x{N}x{K}")
    assert torch.equal(C, ops.nt_gemm(A, Bm))
    with pytest.raises(ValueError):
        ops.nt_gemm(A[:, : K - 1].contiguous(), Bm[:, : K - 1].contiguous())           # K % 32 != 0


@bf3_only
@pytest.mark.parametrize("Bq,D,O,ncls", [(256, 25600, 1024, 4), (7, 288, 96, 3)])
def test_random_layer_fused_vs_composition(Bq, D, O, ncls):
    """ops.RandomLayerFn (the product, the 1/√O scale and the Hadamard product with p·R₁ in one GEMM epilogue) against the
    reference's composition (C_DAN.py:18-25) in fp64, forward and both input gradients."""
    g = torch.Generator(device=DEV).manual_seed(Bq + D)
    x = torch.randn(Bq, D, generator=g, device=DEV, requires_grad=True)
    p = torch.softmax(torch.randn(Bq, ncls, generator=g, device=DEV), 1).requires_grad_(True)
    R0, R1 = torch.randn(D, O, generator=g, device=DEV), torch.randn(ncls, O, generator=g, device=DEV)
    cot = torch.randn(Bq, O, generator=g, device=DEV)
    out = ops.RandomLayerFn.apply(x, p, R0, R0.t().contiguous(), R1, 1.0 / O ** 0.5)
    gx, gp = torch.autograd.grad(out, (x, p), cot)
    x64, p64 = x.detach().double().requires_grad_(True), p.detach().double().requires_grad_(True)
    want = (x64 @ R0.double()) / O ** 0.5 * (p64 @ R1.double())
    wx, wp = torch.autograd.grad(want, (x64, p64), cot.double())
    assert_close(out, want, 2e-5, "random layer out")
    assert_close(gx, wx, 2e-5, "random layer dx")
    assert_close(gp, wp, 2e-5, "random layer dp")


@bf3_only
@pytest.mark.parametrize("M,C,ntaps,dil,pad,Bq,L", [(50, 225, 2, 1, 0, 256, 512), (50, 225, 2, 1, 0, 3, 64), (33, 70, 3, 4, 4, 2, 96),
                                                    (8, 64, 4, 1, 1, 2, 32), (256, 130, 3, 1, 1, 2, 64)])
def test_few_tap_dense_weight_gradient_vs_fp64(M, C, ntaps, dil, pad, Bq, L, monkeypatch):
    """fst_tap_wgrad (the dense gradient of a conv with 2-4 taps on the time-as-k kernel; ConvSpec.grad_w routes the shared
    omni-scale block's last layer there) against an fp64 einsum, x between NaN-poisoned guard bands; bit-identical twice."""
    monkeypatch.setenv("FST_TAP_WGRAD", "1")                    # (off by default: slower than the item-table kernel where it fits)
    g = torch.Generator(device=DEV).manual_seed(M + C + L)
    x = ops.empty_with_slack(Bq, C, L, DEV)
    x.untyped_storage().copy_(torch.full((Bq * C * L + 8,), float("nan")).untyped_storage())
    x.copy_(torch.randn(Bq, C, L, generator=g, device=DEV))
    dy = torch.randn(Bq, M, L, generator=g, device=DEV)
    spec = ops.ConvSpec(M, C, ntaps, dil, pad)
    assert spec.tap_wgrad_ok(Bq, L, x, dy)
    dw, _ = spec.grad_w(x, None, dy)
    halo = (ntaps - 1) * dil
    xp = F.pad(x.double(), (pad, halo - pad))
    want = torch.stack([torch.einsum("bmt,bct->mc", dy.double(), xp[:, :, k * dil: k * dil + L]) for k in range(ntaps)], dim=2)
    assert_close(dw, want, 1e-4, "few-tap dW")
    again, _ = spec.grad_w(x, None, dy)
    assert torch.equal(dw, again)
    if any((k * dil - pad) % 4 for k in range(ntaps)):
        assert not spec.tap_wgrad_ok(Bq, L, x.clone(), dy)                      # no slack: the generic kernel serves it


@bf3_only
@pytest.mark.parametrize("M,C,K,pad,Bq,L", [(225, 25, 89, 44, 256, 512), (25, 1, 89, 44, 256, 512), (25, 50, 89, 44, 256, 512), (100, 9, 45, 22, 2, 64), (225, 25, 89, 44, 2, 64), (33, 3, 37, 18, 3, 96),
                                            (7, 2, 5, 2, 1, 32), (256, 5, 96, 47, 2, 64), (40, 4, 8, 3, 2, 128),
                                            (129, 3, 89, 44, 1, 32), (65, 5, 33, 0, 2, 64), (64, 9, 96, 95, 2, 32)])     # one-row second half; pad 0; pad K-1
def test_dense_many_tap_weight_gradient_vs_fp64(M, C, K, pad, Bq, L):
    """fst_dense_tap_wgrad (the dense Q1 gradient of an omni-scale layer: every tap from eight pre-shifted copies of one staged window
    per channel) against an fp64 einsum — through ConvSpec.grad_w, which routes dense plans there; bit-identical twice."""
    g = torch.Generator(device=DEV).manual_seed(M + C + K + L)
    x, dy = torch.randn(Bq, C, L, generator=g, device=DEV), torch.randn(Bq, M, L, generator=g, device=DEV)
    spec = ops.ConvSpec(M, C, K, 1, pad)
    assert spec.dense_tap_wgrad_ok(Bq, L, x, dy)
    dw, _ = spec.grad_w(x, None, dy)
    xp = F.pad(x.double(), (pad, K - 1 - pad))
    want = torch.stack([torch.einsum("bmt,bct->mc", dy.double(), xp[:, :, k: k + L]) for k in range(K)], dim=2)
    assert_close(dw, want, 1e-4, "dense many-tap dW")
    again, _ = spec.grad_w(x, None, dy)
    assert torch.equal(dw, again)
