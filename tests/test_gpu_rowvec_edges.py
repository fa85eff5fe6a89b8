"""The shape-selected code paths of the small bandwidth kernels against fp64 references.  Needs an MI355X.

The per-row kernels (BatchNorm, row sums) map a row of L/4 float4 onto 2^shift threads, shift = 0..8 by L, and fall back to a
scalar path when L % 4 != 0 or a base is not 16-byte aligned; the last workgroup of a launch holds idle row groups unless B·C is a
multiple of the rows per block.  The coupling kernels cap the grid at 64 workgroups per sample and grid-stride beyond it; the
WN fold walks a row table a wave per row; the elementwise helpers have n % 4 tails and capped grids.  Each test below sweeps
those paths.  None of these kernels depends on ops.MATH: every test runs unchanged under FST_MATH=f32.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from feature_level_style_transfer_for_tsc_amd import _lib, ops

DEV = "cuda"
EPS32 = float(np.finfo(np.float32).eps)


def assert_close(got, want, tol, what=""):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    scale = max(1e-6, float(want.abs().max()))
    err = float((got - want).abs().max())
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


# L -> threads per row 2^shift = min(256, pow2ceil(L/4)): 4 -> 1, 8 -> 2, 12 -> 4, 24 -> 8, 60 -> 16, 100 -> 32, 132 and 256 -> 64,
# 260 -> 128, 1024 and 5000 -> 256 (5000: five passes per row); 5 and 257 take the scalar path
BN_LENGTHS = [4, 8, 12, 24, 60, 100, 132, 256, 260, 1024, 5000, 5, 257]
# (B, C): 85 and 7 rows leave idle row groups in the last workgroup at every shift below 8; B = 1 and 17 around the 16 BN slots
BN_BATCHES = [(17, 5), (1, 7)]


def _relu64(v, dev_out):
    """ReLU of the fp64 reference with the DEVICE's mask: an fp32 output within rounding of 0 may land on the other side of it,
    and would move that element's gradient by a whole |dy|."""
    return v * (dev_out.detach().cpu() > 0).double()


def _bn_inputs(B, C, L, seed):
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(B, C, L, generator=g, dtype=torch.float64) * 2 + 0.7)
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    dout = torch.randn(B, C, L, generator=g, dtype=torch.float64)
    return y, gamma, beta, rm, rv, dout


@pytest.mark.parametrize("B,C", BN_BATCHES)
@pytest.mark.parametrize("L", BN_LENGTHS)
def test_bn_act_every_row_mapping(B, C, L):
    f = lambda t: t.detach().float().to(DEV)
    for training, relu in ((True, True), (True, False), (False, True), (False, False)):
        y, gamma, beta, rm, rv, dout = _bn_inputs(B, C, L, 3 * L + B)
        yd, gd, bd = f(y).requires_grad_(True), f(gamma).requires_grad_(True), f(beta).requires_grad_(True)
        rmd, rvd = f(rm), f(rv)
        got = ops.BNActFn.apply(yd, gd, bd, rmd, rvd, training, relu, 1e-5, 0.1)
        (got * f(dout)).sum().backward()
        y.requires_grad_(True); gamma.requires_grad_(True); beta.requires_grad_(True)
        rm_ref, rv_ref = rm.clone(), rv.clone()
        out = F.batch_norm(y, rm_ref, rv_ref, gamma, beta, training, 0.1, 1e-5)
        out = _relu64(out, got) if relu else out
        (out * dout).sum().backward()
        what = f"L={L} B={B} train={training} relu={relu}"
        assert_close(got, out, 1e-5, what + " out")
        assert_close(yd.grad, y.grad, 5e-5, what + " dx")
        assert_close(gd.grad, gamma.grad, 5e-5, what + " dgamma")
        assert_close(bd.grad, beta.grad, 5e-5, what + " dbeta")
        assert_close(rmd, rm_ref, 1e-5, what + " running mean")
        assert_close(rvd, rv_ref, 1e-5, what + " running var")


@pytest.mark.parametrize("B,C", BN_BATCHES)
@pytest.mark.parametrize("L", BN_LENGTHS)
def test_bn_backward_row_sums(B, C, L):
    """The per-(sample, channel) Σ_t dx that fst_bn_bwd_apply leaves for the bias gradient of the conv in front (ConvFn takes them
    via _RowSums): against fp64 Σ_t dx of F.batch_norm's backward, and against the device dx's own sums."""
    f = lambda t: t.detach().float().to(DEV)
    for training, relu in ((True, True), (True, False), (False, True)):
        y, gamma, beta, rm, rv, dout = _bn_inputs(B, C, L, 7 * L + B)
        yd = f(y)
        out = ops.BNActFn.apply(yd, f(gamma), f(beta), f(rm), f(rv), training, relu, 1e-5, 0.1)
        y.requires_grad_(True)
        out64 = F.batch_norm(y, rm.clone(), rv.clone(), gamma, beta, training, 0.1, 1e-5)
        out64 = _relu64(out64, out) if relu else out64
        (out64 * dout).sum().backward()
        want = y.grad.sum(dim=2)
        stats = ops._bn_stats(yd, f(gamma), f(beta), f(rm), f(rv), training, 1e-5, 0.1)
        dx, _, _ = ops._bn_backward(f(dout), yd, out if relu else None, stats, relu, training)
        rs = ops._RowSums.take(dx)
        assert rs is not None and tuple(rs.shape) == (B, C)
        what = f"L={L} B={B} train={training} relu={relu}"
        bound = float(y.grad.abs().sum(dim=2).max())
        err = float((rs.double().cpu() - want).abs().max())
        assert err <= 2e-5 * bound, f"{what}: row sums vs fp64: {err:.3e} (Σ|dx| up to {bound:.3e})"
        own = float((rs.double() - dx.double().sum(dim=2)).abs().max())
        assert own <= 1e-5 * bound, f"{what}: row sums vs the launch's own dx: {own:.3e}"


@pytest.mark.parametrize("B,C", BN_BATCHES)
@pytest.mark.parametrize("L", [4, 12, 24, 60, 132, 260, 5000, 5, 257])
def test_bn_add_bn_relu_every_row_mapping(B, C, L):
    g = torch.Generator().manual_seed(L + 100 * B)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ya, yb = mk(B, C, L).requires_grad_(True), (mk(B, C, L) * 3 - 1).requires_grad_(True)
    ga, ba, gb, bb = [(mk(C) + 1.5).requires_grad_(True) for _ in range(4)]
    dout = mk(B, C, L)
    f = lambda t: t.detach().float().to(DEV)
    d = [f(t).requires_grad_(True) for t in (ya, ga, ba, yb, gb, bb)]
    bufs = [torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV)]
    got = ops.BNAddBNReluFn.apply(d[0], d[1], d[2], bufs[0], bufs[1], d[3], d[4], d[5], bufs[2], bufs[3], True, 1e-5, 0.1)
    (got * f(dout)).sum().backward()
    out = _relu64(F.batch_norm(ya, torch.zeros(C).double(), torch.ones(C).double(), ga, ba, True, 0.1, 1e-5)
                  + F.batch_norm(yb, torch.zeros(C).double(), torch.ones(C).double(), gb, bb, True, 0.1, 1e-5), got)
    (out * dout).sum().backward()
    assert_close(got, out, 1e-5, f"L={L} B={B} out")
    for t, r, name in zip(d, (ya, ga, ba, yb, gb, bb), ("dya", "dga", "dba", "dyb", "dgb", "dbb")):
        assert_close(t.grad, r.grad, 5e-5, f"L={L} B={B} {name}")


@pytest.mark.parametrize("L", [4, 8, 12, 24, 60, 100, 132, 256, 260, 1024, 5000, 5, 257])
@pytest.mark.parametrize("B,C", [(1, 3), (17, 5), (40, 2)])
def test_row_sum_every_row_mapping(B, C, L):
    g = torch.Generator().manual_seed(L + B)
    x = torch.randn(B, C, L, generator=g)
    want = x.double().sum(dim=(0, 2))
    err = float((ops.row_sum(x.to(DEV)).double().cpu() - want).abs().max())
    assert err <= 1e-5 * float(x.abs().sum(dim=(0, 2)).max()), f"row_sum B={B} C={C} L={L}: {err:.3e}"


@pytest.mark.parametrize("L", [8, 60, 256, 1024, 5000])
def test_row_sum_of_views(L):
    """A channel slice of a wider tensor (batch stride > C·L, still 16-byte aligned when L % 4 == 0) and the same data one
    element off 16-byte alignment (must take the scalar path and still be right)."""
    g = torch.Generator().manual_seed(L)
    B, C, C2, c0 = 9, 3, 8, 4
    wide = torch.randn(B, C2, L, generator=g)
    wd = wide.to(DEV)
    view = wd[:, c0:c0 + C]
    assert view.stride(0) == C2 * L > C * L
    want = wide[:, c0:c0 + C].double().sum(dim=(0, 2))
    bound = float(wide.abs().sum(dim=(0, 2)).max())
    assert float((ops.row_sum(view).double().cpu() - want).abs().max()) <= 1e-5 * bound, f"channel slice L={L}"
    buf = torch.empty(B * C * L + 1, device=DEV)
    odd = buf[1:].view(B, C, L)
    assert odd.data_ptr() % 16 != 0
    odd.copy_(wide[:, c0:c0 + C])
    assert float((ops.row_sum(odd).double().cpu() - want).abs().max()) <= 1e-5 * bound, f"misaligned base L={L}"
    odd_view = torch.empty(B * C2 * L + 1, device=DEV)[1:].view(B, C2, L)
    odd_view.copy_(wide)
    assert float((ops.row_sum(odd_view[:, c0:c0 + C]).double().cpu() - want).abs().max()) <= 1e-5 * bound, f"misaligned slice L={L}"


# ------------------------------------------------------------------ BatchNorm entry points off 16-byte alignment
PAD, CANARY, BN_EPS = 64, 1234.5, 1e-5          # PAD floats = 256 bytes: a body at PAD is 16-byte aligned, at PAD + 1 one float past


class _Canaried:
    """Device tensors inside canary-filled buffers, each a chosen number of floats past a 16-byte boundary."""

    def __init__(self):
        self.bufs = {}

    def put(self, name, t, off):
        n = t.numel()
        buf = torch.full((PAD + off + n + PAD,), CANARY, device=DEV)
        body = buf[PAD + off: PAD + off + n].view(t.shape)
        body.copy_(t)
        assert body.data_ptr() % 16 == 4 * off
        self.bufs[name] = (buf, body)
        return body

    def new(self, name, shape, off):
        return self.put(name, torch.full(shape, CANARY), off)

    def assert_only_bodies_written(self, outputs):
        for name, (buf, body) in self.bufs.items():
            lo, n = body.storage_offset(), body.numel()
            assert bool((buf[:lo] == CANARY).all()) and bool((buf[lo + n:] == CANARY).all()), f"{name}: written outside the tensor"
        for name in outputs:
            assert not bool((self.bufs[name][1] == CANARY).any()), f"{name}: not every element was written"


@pytest.mark.parametrize("case", ["every tensor", "written tensor only"])
@pytest.mark.parametrize("L", [8, 256])
def test_bn_entry_points_off_16_byte_alignment(L, case):
    """L % 4 == 0 with a base one float past a 16-byte boundary must take the scalar path: every BatchNorm entry point through
    its raw symbol, against fp64, on operands that are all misaligned or of which only the written tensor is (`out` of the
    forward, `dx` of the backward, `dxa` alone of the join).  L = 256 is L/4 = 64, where the 16-byte kernels' row sums go from
    the in-wave butterfly to the LDS step.  Canary words on both sides of every tensor: nothing outside the outputs is written."""
    lib = _lib.load()
    B, C = 3, 5
    rd = 1 if case == "every tensor" else 0                                   # offset of everything but the written tensor
    g = torch.Generator().manual_seed(11 * L + rd)
    mk = lambda *s: torch.randn(*s, generator=g)
    n, sp, S = B * C * L, _lib.stream_ptr, ops.BN_SLOTS
    host = dict(ya=mk(B, C, L) * 2 + 0.7, yb=mk(B, C, L) * 3 - 1, dy=mk(B, C, L), ga=torch.rand(C, generator=g) + 0.5,
                gb=torch.rand(C, generator=g) + 0.5, ba=mk(C), bb=mk(C), rm=mk(C), rv=torch.rand(C, generator=g) + 0.5)
    m = _Canaried()
    d = {k: m.put(k, v, rd) for k, v in host.items()}
    p = lambda t: t.data_ptr()

    stats = {}
    for k in "ab":
        part, stats[k] = m.new("part_" + k, (C, S, 4), rd), m.new("stats_" + k, (4 * C,), rd)
        rm, rv = m.put("rm_" + k, host["rm"], rd), m.put("rv_" + k, host["rv"], rd)
        _lib.check(lib.fst_bn_stats(p(d["y" + k]), B, C, L, p(part), n, sp()), "bn_stats")
        _lib.check(lib.fst_bn_finalize(p(part), S, p(d["g" + k]), p(d["b" + k]), p(rm), p(rv), 1, C, BN_EPS, 0.1, p(stats[k]), sp()),
                   "bn_finalize")
    out, out_j = m.new("out", (B, C, L), 1), m.new("out_join", (B, C, L), 1)
    _lib.check(lib.fst_bn_apply(p(d["ya"]), p(stats["a"]), None, None, p(out), B, C, L, 1, n, sp()), "bn_apply")
    _lib.check(lib.fst_bn_apply(p(d["ya"]), p(stats["a"]), p(d["yb"]), p(stats["b"]), p(out_j), B, C, L, 1, n, sp()), "bn_apply join")

    h64 = {k: v.double().requires_grad_(k != "dy") for k, v in host.items() if k not in ("rm", "rv")}
    rm64 = {k: host["rm"].double() for k in "ab"}
    rv64 = {k: host["rv"].double() for k in "ab"}
    pre = {k: F.batch_norm(h64["y" + k], rm64[k], rv64[k], h64["g" + k], h64["b" + k], True, 0.1, BN_EPS) for k in "ab"}
    what = f"L={L} {case}: "
    assert_close(out, _relu64(pre["a"], out), 1e-5, what + "out")
    assert_close(out_j, _relu64(pre["a"] + pre["b"], out_j), 1e-5, what + "out of the join")
    for k in "ab":
        assert_close(m.bufs["rm_" + k][1], rm64[k], 1e-5, what + f"running mean {k}")
        assert_close(m.bufs["rv_" + k][1], rv64[k], 1e-5, what + f"running var {k}")

    def assert_branch(tag, dx, red, rs, want_dx, want_dgamma, want_dbeta):
        assert_close(dx, want_dx, 5e-5, what + tag + " dx")
        assert_close(red[:C], want_dbeta, 5e-5, what + tag + " dbeta")
        assert_close(red[C:], want_dgamma, 5e-5, what + tag + " dgamma")
        bound = float(want_dx.abs().sum(dim=2).max())                          # the measure of test_bn_backward_row_sums
        err = float((rs.double().cpu() - want_dx.sum(dim=2)).abs().max())
        assert err <= 2e-5 * bound, f"{what}{tag} row sums vs fp64: {err:.3e} (Σ|dx| up to {bound:.3e})"

    # single branch; the backward reads the forward's output from a buffer placed like the other operands it reads
    out_in = m.put("out_in", out, rd)
    part, red = m.new("bwd_part", (2, C, S), rd), m.new("red", (2 * C,), rd)
    dx, rs = m.new("dx", (B, C, L), 1), m.new("rs", (B, C), rd)
    _lib.check(lib.fst_bn_bwd_reduce(p(d["dy"]), p(d["ya"]), p(out_in), p(stats["a"]), B, C, L, 1, p(part), n, sp()), "bn_bwd_reduce")
    _lib.check(lib.fst_bn_bwd_apply(p(d["dy"]), p(d["ya"]), p(out_in), p(stats["a"]), p(part), S, p(red), p(dx), p(rs), B, C, L, 1,
                                    1, B, n, sp()), "bn_bwd_apply")
    want = torch.autograd.grad((_relu64(pre["a"], out) * h64["dy"]).sum(), [h64["ya"], h64["ga"], h64["ba"]], retain_graph=True)
    assert_branch("single", dx, red, rs, *want)

    # the join: dxa alone is the misaligned one of "written tensor only"
    jp = {k: m.new("join_part_" + k, (2, C, S), rd) for k in "ab"}
    jr = {k: m.new("join_red_" + k, (2 * C,), rd) for k in "ab"}
    jdx = dict(a=m.new("dxa", (B, C, L), 1), b=m.new("dxb", (B, C, L), rd))
    jrs = {k: m.new("join_rs_" + k, (B, C), rd) for k in "ab"}
    _lib.check(lib.fst_bn_bwd_reduce_join(p(d["dy"]), p(d["ya"]), p(d["yb"]), p(stats["a"]), p(stats["b"]), B, C, L, p(jp["a"]),
                                          p(jp["b"]), n, sp()), "bn_bwd_reduce_join")
    _lib.check(lib.fst_bn_bwd_apply_join(p(d["dy"]), p(d["ya"]), p(d["yb"]), p(stats["a"]), p(stats["b"]), p(jp["a"]), p(jp["b"]), S,
                                         p(jr["a"]), p(jr["b"]), p(jdx["a"]), p(jdx["b"]), p(jrs["a"]), p(jrs["b"]), B, C, L, 1, B, n,
                                         sp()), "bn_bwd_apply_join")
    want = torch.autograd.grad((_relu64(pre["a"] + pre["b"], out_j) * h64["dy"]).sum(),
                               [h64[k + b] for b in "ab" for k in ("y", "g", "b")])
    for i, k in enumerate("ab"):
        assert_branch("join " + k, jdx[k], jr[k], jrs[k], *want[3 * i: 3 * i + 3])

    m.assert_only_bodies_written(["part_a", "part_b", "stats_a", "stats_b", "out", "out_join", "bwd_part", "red", "dx", "rs",
                                  "join_part_a", "join_part_b", "join_red_a", "join_red_b", "dxa", "dxb", "join_rs_a", "join_rs_b"])


# ------------------------------------------------------------------ affine coupling
COUPLING_SHAPES = [(1, 1, 3), (256, 25, 512), (2, 40, 5000)]       # the last: h·L > 64 workgroups x 1024 -> grid-stride


def _coupling_inputs(B, h, L, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(B, 2 * h, L, generator=g, dtype=torch.float64)
    o = torch.randn(B, 2 * h, L, generator=g, dtype=torch.float64) * 0.5
    dxn = torch.randn(B, 2 * h, L, generator=g, dtype=torch.float64)
    return u, o, dxn


def _coupling64(u, o):
    h = u.size(1) // 2
    b, s = o[:, :h], o[:, h:]
    xn = torch.cat([u[:, :h], torch.exp(s) * u[:, h:] + b], dim=1)
    return xn, s.sum(), (xn * xn).sum()


@pytest.mark.parametrize("B,h,L", COUPLING_SHAPES)
def test_coupling_forward_sums_and_backward(B, h, L):
    u, o, dxn = _coupling_inputs(B, h, L, B + h + L)
    a_ls, a_sq = 0.37, -0.011
    f = lambda t: t.detach().float().to(DEV)
    ud, od = f(u).requires_grad_(True), f(o).requires_grad_(True)
    xn, s_ls, s_sq = ops.CouplingFn.apply(ud, od)
    u64, o64 = u.clone().requires_grad_(True), o.clone().requires_grad_(True)
    xn64, ls64, sq64 = _coupling64(u64, o64)
    assert_close(xn, xn64, 1e-5, "xn")
    assert abs(s_ls.item() - ls64.item()) <= 1e-5 * float(o[:, h:].abs().sum()), ("Σ log_s", s_ls.item(), ls64.item())
    assert abs(s_sq.item() - sq64.item()) <= 1e-5 * sq64.item(), ("Σ xn²", s_sq.item(), sq64.item())
    cases = (("dxn only", lambda x, l, q, c: (x * c).sum()),
             ("sums only (dxn is None)", lambda x, l, q, c: a_ls * l + a_sq * q),
             ("dxn and sums", lambda x, l, q, c: (x * c).sum() + a_ls * l + a_sq * q))
    for name, loss in cases:
        got = torch.autograd.grad(loss(xn, s_ls, s_sq, f(dxn)), [ud, od], retain_graph=True)
        want = torch.autograd.grad(loss(xn64, ls64, sq64, dxn), [u64, o64], retain_graph=True)
        assert_close(got[0], want[0], 2e-5, f"{name}: du")
        assert_close(got[1], want[1], 2e-5, f"{name}: do")


@pytest.mark.parametrize("B,h,L", COUPLING_SHAPES)
def test_coupling_inverse_forward_backward(B, h, L):
    x, o, dxn = _coupling_inputs(B, h, L, 3 * B + h + L)
    f = lambda t: t.detach().float().to(DEV)
    xd, od = f(x).requires_grad_(True), f(o).requires_grad_(True)
    xn = ops.CouplingInvFn.apply(xd, od)
    x64, o64 = x.clone().requires_grad_(True), o.clone().requires_grad_(True)
    xn64 = torch.cat([x64[:, :h], (x64[:, h:] - o64[:, :h]) / torch.exp(o64[:, h:])], dim=1)
    assert_close(xn, xn64, 1e-5, "inverse xn")
    got = torch.autograd.grad((xn * f(dxn)).sum(), [xd, od])
    want = torch.autograd.grad((xn64 * dxn).sum(), [x64, o64])
    assert_close(got[0], want[0], 2e-5, "inverse dx")
    assert_close(got[1], want[1], 2e-5, "inverse do")


# ------------------------------------------------------------------ WN weight-norm fold
# n_layers = 3 so that the row count (6·n·nl + 2·nl + 4) is not a multiple of the four rows per workgroup: the last is partial.
# Row lengths: h (7, 25: < 64), n (50 < 64, 64, 120 > 64), 3n (150, 192, 360); plain copies of 14..720 elements.
@pytest.mark.parametrize("n,h", [(50, 7), (120, 25), (64, 7)])
def test_wn_fold_vs_weight_norm(n, h):
    nl = 3
    specs = ops.WNSpecs(h, n, nl)
    normed = [True, False, True, False, False, False] + [True] * nl + [False] * nl + [True] * nl + [False] * nl
    plan = ops.WNFoldPlan(specs, normed)
    assert plan.n_rows % 4 != 0
    g = torch.Generator().manual_seed(n + h)
    inputs64 = []
    for sh, nm in zip(specs.shapes, normed):
        inputs64.append(torch.randn(*sh, generator=g, dtype=torch.float64))
        if nm:
            inputs64.append(torch.rand(sh[0], *([1] * (len(sh) - 1)), generator=g, dtype=torch.float64) + 0.5)
    for t in inputs64:
        t.requires_grad_(True)
    parts, it = [], iter(inputs64)
    for nm in normed:
        if nm:
            v, gg = next(it), next(it)
            parts.append(torch._weight_norm(v, gg, 0).reshape(-1))
        else:
            parts.append(next(it).reshape(-1))
    flat64 = torch.cat(parts)
    d_flat = torch.randn(specs.flat_numel, generator=g, dtype=torch.float64)
    want = torch.autograd.grad((flat64 * d_flat).sum(), inputs64)
    dev = [t.detach().float().to(DEV).requires_grad_(True) for t in inputs64]
    flat = ops.WNFoldFn.apply(plan, *dev)
    assert_close(flat, flat64, 1e-5, f"flat n={n} h={h}")
    got = torch.autograd.grad((flat * d_flat.float().to(DEV)).sum(), dev)
    for i, (a, w) in enumerate(zip(got, want)):
        assert tuple(a.shape) == tuple(w.shape)
        assert_close(a, w, 5e-5, f"gradient of fold input {i} {tuple(w.shape)}")


# ------------------------------------------------------------------ elementwise helpers
ELEM_SIZES = [1, 3, 5, 1021, 9 * 2 ** 20 + 3]          # the last: past relu_bwd's 8192-workgroup cap, with a tail of 3


def _dy_y(n, seed):
    g = torch.Generator().manual_seed(seed)
    dy, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    y[torch.rand(n, generator=g) < 0.2] = 0.0                      # exact zeros: act'(0) is the negative side's
    return dy.to(DEV), y.to(DEV)


@pytest.mark.parametrize("n", ELEM_SIZES)
def test_relu_bwd_exact(n):
    dy, y = _dy_y(n, n)
    assert torch.equal(ops.relu_bwd(dy, y), torch.where(y > 0, dy, torch.zeros_like(dy)))


@pytest.mark.parametrize("slope", [0.0, 0.2])
@pytest.mark.parametrize("n", ELEM_SIZES)
def test_act_bwd_exact(n, slope):
    dy, y = _dy_y(n, n + 1)
    want = torch.where(y > 0, dy, dy * torch.tensor(slope, dtype=torch.float32, device=DEV))
    assert torch.equal(ops.act_bwd(dy, y, slope), want)


def test_elementwise_backward_of_a_misaligned_cotangent():
    """An odd-offset slice as dy (contiguous, not 16-byte aligned): copied, not refused."""
    dy_buf, y = torch.randn(1 + 1021, device=DEV), torch.randn(1021, device=DEV)
    dy = dy_buf[1:]
    assert dy.data_ptr() % 16 != 0
    assert torch.equal(ops.relu_bwd(dy, y), torch.where(y > 0, dy, torch.zeros_like(dy)))
    s = torch.tensor(0.2, device=DEV)
    assert torch.equal(ops.act_bwd(dy, y, 0.2), torch.where(y > 0, dy, dy * s))


@pytest.mark.parametrize("B,N", [(1, 4), (3, 4 * 2 ** 20 + 8)])          # the second: 12.6 M floats > 8192 workgroups x 1024
def test_bcast_add_exact(B, N):
    lib = _lib.load()
    g = torch.Generator().manual_seed(N)
    x, v = torch.randn(B, N, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)
    out = torch.empty(B, N, device=DEV)
    _lib.check(lib.fst_bcast_add(out.data_ptr(), x.data_ptr(), v.data_ptr(), B, N, _lib.stream_ptr()), "fst_bcast_add")
    assert torch.equal(out, x + v)


@pytest.mark.parametrize("n", [1, 7, 4096 * 256 * 3 + 5])                  # the last: past the 4096-workgroup cap
def test_axpy(n):
    lib = _lib.load()
    g = torch.Generator().manual_seed(n)
    y0, x = torch.randn(n, generator=g), torch.randn(n, generator=g)
    alpha = float(np.float32(-0.7))
    yd = y0.to(DEV)
    _lib.check(lib.fst_axpy(yd.data_ptr(), x.to(DEV).data_ptr(), alpha, n, _lib.stream_ptr()), "fst_axpy")
    want = y0.double() + alpha * x.double()
    err = (yd.double().cpu() - want).abs()
    ulp = EPS32 * torch.maximum(want.abs(), torch.maximum(y0.double().abs(), (alpha * x.double()).abs()))
    assert bool((err <= ulp).all()), f"axpy n={n}: {int((err > ulp).sum())} elements beyond one ulp"


@pytest.mark.parametrize("B,C,L,with_b", [(3, 50, 512, True), (3, 50, 512, False), (1, 2, 3, True), (2, 33, 1000, True)])
def test_add_slices_of_strided_views(B, C, L, with_b):
    """dst[:, c0:c0+C] = a[:, ...] (+ b) on channel slices of wider tensors (C·L = 25 600 and 33 000 > 64 workgroups x 256:
    grid-stride); everything outside the destination slice keeps its value."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(C * L)
    a_w, b_w = torch.randn(B, C + 3, L, generator=g).to(DEV), torch.randn(B, 2 * C, L, generator=g).to(DEV)
    dst_w = torch.full((B, C + 5, L), 1234.5, device=DEV)
    a, b, dst = a_w[:, 3:], b_w[:, C:], dst_w[:, 2:2 + C]
    _lib.check(lib.fst_add_slices(dst.data_ptr(), dst.stride(0), a.data_ptr(), a.stride(0), b.data_ptr() if with_b else None,
                                  b.stride(0), B, C, L, _lib.stream_ptr()), "fst_add_slices")
    assert torch.equal(dst, a + b if with_b else a)
    assert bool((dst_w[:, :2] == 1234.5).all()) and bool((dst_w[:, 2 + C:] == 1234.5).all())


# ------------------------------------------------------------------ linear_act on inputs nn.Linear accepts
def _linear_act64(x, W, b, act, slope, dev_out):
    h = F.linear(x, W, b)
    if act == ops.ACT_NONE or h.numel() == 0:
        return F.relu(h) if act == ops.ACT_RELU else (F.leaky_relu(h, slope) if act == ops.ACT_LEAKY else h)
    pos = dev_out.detach().cpu() > 0                         # the device's side of 0 (see _relu64)
    return torch.where(pos, h, h * slope)


@pytest.mark.parametrize("act,slope", [(ops.ACT_NONE, 0.0), (ops.ACT_RELU, 0.0), (ops.ACT_LEAKY, 0.2)])
@pytest.mark.parametrize("case", ["empty batch", "expanded rows", "misaligned cotangent"])
def test_linear_act_edge_inputs(case, act, slope):
    """linear_act = F.linear + the aten activation in value and in all three gradients, on an empty batch, on an expanded x
    (stride(0) < K: rows that overlap) and under a dy that is not 16-byte aligned (an odd-offset slice of a larger buffer)."""
    g = torch.Generator().manual_seed(len(case) + act)
    K, N = 12, 7
    lin = torch.nn.Linear(K, N).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(N, K, generator=g) / K ** 0.5)
        lin.bias.copy_(torch.randn(N, generator=g))
    M = 0 if case == "empty batch" else 6
    if case == "expanded rows":
        base = torch.randn(1, K, generator=g).to(DEV).requires_grad_(True)
        x = base.expand(M, K)
        assert x.stride(0) < K
    else:
        base = torch.randn(M, K, generator=g).to(DEV).requires_grad_(True)
        x = base
    cot_buf = torch.randn(M * N + 1, generator=g).to(DEV)
    cot = cot_buf[1:].view(M, N) if case == "misaligned cotangent" else cot_buf[:M * N].view(M, N)
    y = ops.linear_act(x, lin, act, slope)
    got = torch.autograd.grad(y, [base, lin.weight, lin.bias], cot, allow_unused=False)
    b64, W64, bias64 = (t.detach().double().cpu().requires_grad_(True) for t in (base, lin.weight, lin.bias))
    x64 = b64.expand(M, K) if case == "expanded rows" else b64
    want = _linear_act64(x64, W64, bias64, act, slope, y)
    wg = torch.autograd.grad(want, [b64, W64, bias64], cot.double().cpu())
    assert tuple(y.shape) == (M, N)
    if M == 0:
        for a, w in zip(got, wg):
            assert tuple(a.shape) == tuple(w.shape) and float(a.abs().sum()) == 0.0
        return
    assert_close(y, want, 2e-5, f"{case}: y")
    for a, w, name in zip(got, wg, ("dx", "dW", "db")):
        assert_close(a, w, 5e-5, f"{case}: {name}")
