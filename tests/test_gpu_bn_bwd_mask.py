"""BatchNorm backward without ``out``, and the fused backward of the residual join.

The backward kernels need the forward output only as the ReLU mask [out > 0].  With ``out = None`` they take the mask from the
sign of the pre-activation recomputed from ``y`` and ``stats`` by the function the forward itself calls, and the join's backward
(`fst_bn_bwd_reduce_join` / `fst_bn_bwd_apply_join`) does both branches in one pass pair.  Both must leave the BITS the kernels
leave when ``out`` is passed (the path that is still in the build): every comparison between device paths here is
``torch.equal``.  The inputs put part of ``y`` exactly on the mask boundary — the float nearest the root of the pre-activation
and its two neighbours — where a pre-activation evaluated in any other way than the forward's would flip the mask.

Shapes (B, C, L): (3, 5, 4) 16-byte path with one thread per row; (3, 5, 7) dword path; (3, 5, 64) a row inside one wave;
(2, 3, 512) rows wider than a wave (totals through LDS); (70, 3, 8) more row groups than one block, idle ones in the last."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from feature_level_style_transfer_for_tsc_amd import _lib, ops

DEV = "cuda"
SHAPES = [(3, 5, 4), (3, 5, 7), (3, 5, 64), (2, 3, 512), (70, 3, 8)]
GAMMA = {5: [1.3, -0.7, 0.0, 0.5, -1.1], 3: [0.9, -0.6, 0.0]}            # positive, negative and exactly 0
EPS, PAD, CANARY = 1e-5, 64, 1234.5                                          # PAD floats = 256 bytes: the bodies stay 16-byte aligned
INF = float("inf")


def assert_close(got, want, tol, what=""):                                   # the measure of tests/test_gpu_kernels.py
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    scale = max(1e-6, float(want.abs().max()))
    err = float((got - want).abs().max())
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def _stats(y, gamma, beta, train):
    """stats = (mean | invstd | scale | shift) from the library's own forward kernels."""
    lib = _lib.load()
    B, C, L = y.shape
    g = torch.Generator().manual_seed(C)
    rm, rv = torch.randn(C, generator=g).to(DEV), (torch.rand(C, generator=g) + 0.5).to(DEV)
    part = torch.empty(C, ops.BN_SLOTS, 4, device=DEV)
    if train:
        _lib.check(lib.fst_bn_stats(y.data_ptr(), B, C, L, part.data_ptr(), y.numel(), _lib.stream_ptr()), "bn_stats")
    stats = torch.empty(4 * C, device=DEV)
    _lib.check(lib.fst_bn_finalize(part.data_ptr(), ops.BN_SLOTS, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                                   int(train), C, EPS, 0.1, stats.data_ptr(), _lib.stream_ptr()), "bn_finalize")
    return stats


def _three_floats(x64):
    """The float nearest each fp64 value, and its two neighbours."""
    mid = x64.float()
    return torch.stack([torch.nextafter(mid, torch.full_like(mid, -INF)), mid, torch.nextafter(mid, torch.full_like(mid, INF))])


def _forced_idx(B, L):
    """Positions of a channel's [B·L] elements that are put on the boundary: 3·n evenly spread ones, at most half of them."""
    n = max(1, min(4, (B * L) // 6))
    return [j * (B * L // (3 * n)) for j in range(3 * n)]


@functools.lru_cache(maxsize=None)
def _single_case(shape, train):
    """y with a subset on the root of pre(y) = y·scale + shift and on its neighbouring floats, the device's out, dy."""
    lib = _lib.load()
    B, C, L = shape
    g = torch.Generator().manual_seed(1000 + B * 31 + L)
    gamma, beta = torch.tensor(GAMMA[C]).to(DEV), (torch.randn(C, generator=g) * 0.5).to(DEV)
    y = (torch.randn(B, C, L, generator=g) * 2 + 0.7).to(DEV)
    # stats first, the boundary values after: the backward kernels take `stats` as given, so the roots stay exact
    stats = _stats(y, gamma, beta, train)
    sc, sh = stats[2 * C: 3 * C].double().cpu(), stats[3 * C:].double().cpu()
    idx = _forced_idx(B, L)
    forced = torch.zeros(B, C, L, dtype=torch.bool)
    yh = y.cpu()
    for c in (c for c in range(C) if GAMMA[C][c] != 0.0):
        vals = _three_floats((-sh[c] / sc[c]).reshape(1)).view(3)
        flat = yh[:, c, :].reshape(-1).clone()
        for k, j in enumerate(idx):
            flat[j] = vals[k % 3]
        m = torch.zeros(B * L, dtype=torch.bool)
        m[idx] = True
        yh[:, c, :] = flat.view(B, L)
        forced[:, c, :] = m.view(B, L)
    y = yh.to(DEV)
    out = torch.empty_like(y)
    _lib.check(lib.fst_bn_apply(y.data_ptr(), stats.data_ptr(), None, None, out.data_ptr(), B, C, L, 1, y.numel(), _lib.stream_ptr()),
               "bn_apply")
    dy = torch.randn(B, C, L, generator=g).to(DEV)
    return y, stats, out, dy, forced


@functools.lru_cache(maxsize=None)
def _join_case(shape, train):
    """As _single_case for the join: a subset of ya on the root of pre_a(ya) + pre_b(yb) for the yb at the same position."""
    lib = _lib.load()
    B, C, L = shape
    g = torch.Generator().manual_seed(2000 + B * 31 + L)
    ga, gb = torch.tensor(GAMMA[C]).to(DEV), torch.tensor(GAMMA[C][::-1]).to(DEV)        # γ_b = 0 on another channel than γ_a
    ba, bb = (torch.randn(C, generator=g) * 0.5).to(DEV), (torch.randn(C, generator=g) * 0.5).to(DEV)
    ya, yb = (torch.randn(B, C, L, generator=g) * 2 + 0.7).to(DEV), (torch.randn(B, C, L, generator=g) * 3 - 1).to(DEV)
    sa, sb = _stats(ya, ga, ba, train), _stats(yb, gb, bb, train)
    sca, sha = sa[2 * C: 3 * C].double().cpu(), sa[3 * C:].double().cpu()
    scb, shb = sb[2 * C: 3 * C].double().cpu(), sb[3 * C:].double().cpu()
    idx = _forced_idx(B, L)
    forced = torch.zeros(B, C, L, dtype=torch.bool)
    yah, ybh = ya.cpu(), yb.cpu()
    for c in (c for c in range(C) if GAMMA[C][c] != 0.0):
        fa, fb = yah[:, c, :].reshape(-1).clone(), ybh[:, c, :].reshape(-1)
        pre_b = (fb[idx].double() * scb[c] + shb[c]).float().double()                  # branch b's value as the kernel rounds it
        vals = _three_floats((-pre_b - sha[c]) / sca[c])                                # [3][len(idx)]
        for k, j in enumerate(idx):
            fa[j] = vals[k % 3, k]
        m = torch.zeros(B * L, dtype=torch.bool)
        m[idx] = True
        yah[:, c, :] = fa.view(B, L)
        forced[:, c, :] = m.view(B, L)
    ya = yah.to(DEV)
    out = torch.empty_like(ya)
    _lib.check(lib.fst_bn_apply(ya.data_ptr(), sa.data_ptr(), yb.data_ptr(), sb.data_ptr(), out.data_ptr(), B, C, L, 1, ya.numel(),
                                _lib.stream_ptr()), "bn_apply")
    dy = torch.randn(B, C, L, generator=g).to(DEV)
    return ya, yb, sa, sb, out, dy, forced


def _assert_on_boundary(out, forced):
    """On the CPU, from the forward output: the forced subset straddles the mask boundary."""
    sub = out.cpu()[forced]
    assert sub.numel() > 0 and bool((sub == 0).any()) and bool((sub > 0).any()), \
        f"forced subset does not straddle the ReLU boundary: {int((sub == 0).sum())} zero, {int((sub > 0).sum())} positive"


def _padded(*shape):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((PAD + n + PAD,), CANARY, device=DEV)
    return buf, buf[PAD: PAD + n].view(*shape)


def _assert_canaries(bufs):
    for name, (buf, body) in bufs.items():
        n = body.numel()
        assert bool((buf[:PAD] == CANARY).all()) and bool((buf[PAD + n:] == CANARY).all()), f"{name}: padding was written"


def _single_bwd(dy, y, out, stats, train, caller_summed):
    """fst_bn_bwd_reduce + fst_bn_bwd_apply with relu = 1; out may be None.  caller_summed: the n_slots = 1 form with the sums
    of three 'ranks' holding the same samples (B_total = 3B)."""
    lib = _lib.load()
    B, C, L = y.shape
    n, po = y.numel(), None if out is None else out.data_ptr()
    part = torch.full((2, C, ops.BN_SLOTS), CANARY, device=DEV)
    _lib.check(lib.fst_bn_bwd_reduce(dy.data_ptr(), y.data_ptr(), po, stats.data_ptr(), B, C, L, 1, part.data_ptr(), n,
                                     _lib.stream_ptr()), "bn_bwd_reduce")
    red_in, n_slots, B_total = (((part.sum(dim=2) * 3).view(2 * C).contiguous(), 1, 3 * B) if caller_summed
                                else (part, ops.BN_SLOTS, B))
    red, dx, rs = torch.full((2 * C,), CANARY, device=DEV), torch.full_like(y, CANARY), torch.full((B, C), CANARY, device=DEV)
    _lib.check(lib.fst_bn_bwd_apply(dy.data_ptr(), y.data_ptr(), po, stats.data_ptr(), red_in.data_ptr(), n_slots, red.data_ptr(),
                                    dx.data_ptr(), rs.data_ptr(), B, C, L, 1, int(train), B_total, n, _lib.stream_ptr()), "bn_bwd_apply")
    return dict(part=part, red=red, dx=dx, rs=rs)


def _join_bwd(dy, ya, yb, sa, sb, train, caller_summed, null_dx=None):
    """The fused pair, every output in a canary-padded buffer.  null_dx: 0 or 1 — that branch gets no dx and no row sums."""
    lib = _lib.load()
    B, C, L = ya.shape
    n = ya.numel()
    bufs = {}
    for i, k in enumerate("ab"):
        bufs["part_" + k] = _padded(2, C, ops.BN_SLOTS)
        bufs["red_" + k] = _padded(2 * C)
        bufs["dx_" + k] = _padded(B, C, L)
        bufs["rs_" + k] = _padded(B, C)
    body = {k: v[1] for k, v in bufs.items()}
    _lib.check(lib.fst_bn_bwd_reduce_join(dy.data_ptr(), ya.data_ptr(), yb.data_ptr(), sa.data_ptr(), sb.data_ptr(), B, C, L,
                                          body["part_a"].data_ptr(), body["part_b"].data_ptr(), n, _lib.stream_ptr()),
               "bn_bwd_reduce_join")
    if caller_summed:
        reds = [(body["part_" + k].sum(dim=2) * 3).view(2 * C).contiguous() for k in "ab"]
        n_slots, B_total = 1, 3 * B
    else:
        reds, n_slots, B_total = [body["part_a"], body["part_b"]], ops.BN_SLOTS, B
    p = lambda k, i: None if null_dx == i else body[k].data_ptr()
    _lib.check(lib.fst_bn_bwd_apply_join(dy.data_ptr(), ya.data_ptr(), yb.data_ptr(), sa.data_ptr(), sb.data_ptr(),
                                         reds[0].data_ptr(), reds[1].data_ptr(), n_slots, body["red_a"].data_ptr(),
                                         body["red_b"].data_ptr(), p("dx_a", 0), p("dx_b", 1), p("rs_a", 0), p("rs_b", 1),
                                         B, C, L, int(train), B_total, n, _lib.stream_ptr()), "bn_bwd_apply_join")
    torch.cuda.synchronize()
    return body, bufs


MODES = [(True, False), (True, True), (False, False)]          # (train, caller-summed n_slots = 1 with B_total = 3B)


@pytest.mark.parametrize("train,caller_summed", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_mask_from_y_is_the_mask_from_out(shape, train, caller_summed):
    y, stats, out, dy, forced = _single_case(shape, train)
    _assert_on_boundary(out, forced)
    with_out = _single_bwd(dy, y, out, stats, train, caller_summed)
    without = _single_bwd(dy, y, None, stats, train, caller_summed)
    for k in ("part", "red", "dx", "rs"):
        assert not bool((without[k] == CANARY).any()), f"{k}: not every element was written"
        assert torch.equal(with_out[k], without[k]), f"{k}: the mask from y differs from the mask from out"


@pytest.mark.parametrize("null_dx", [None, 0, 1])
@pytest.mark.parametrize("train,caller_summed", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_join_equals_two_single_branch_launches(shape, train, caller_summed, null_dx):
    ya, yb, sa, sb, out, dy, forced = _join_case(shape, train)
    _assert_on_boundary(out, forced)
    want = [_single_bwd(dy, ya, out, sa, train, caller_summed), _single_bwd(dy, yb, out, sb, train, caller_summed)]
    got, _ = _join_bwd(dy, ya, yb, sa, sb, train, caller_summed, null_dx)
    for i, k in enumerate("ab"):
        assert torch.equal(got["part_" + k], want[i]["part"]), f"branch {k}: slot partials"
        assert torch.equal(got["red_" + k], want[i]["red"]), f"branch {k}: red_out"
        if null_dx != i:
            assert torch.equal(got["dx_" + k], want[i]["dx"]), f"branch {k}: dx"
            assert torch.equal(got["rs_" + k], want[i]["rs"]), f"branch {k}: row sums"


@pytest.mark.parametrize("null_dx", [None, 0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_join_writes_nothing_outside_its_outputs(shape, null_dx):
    ya, yb, sa, sb, out, dy, forced = _join_case(shape, True)
    got, bufs = _join_bwd(dy, ya, yb, sa, sb, True, False, null_dx)
    _assert_canaries(bufs)
    for i, k in enumerate("ab"):
        for name in ("dx_" + k, "rs_" + k):
            if null_dx == i:
                assert bool((got[name] == CANARY).all()), f"{name}: written although the branch has no dx"
            else:
                assert not bool((got[name] == CANARY).any()), f"{name}: not every element was written"
        assert not bool((got["part_" + k] == CANARY).any()) and not bool((got["red_" + k] == CANARY).any())


def test_join_refuses_a_batch_that_does_not_describe_the_buffers():
    lib = _lib.load()
    ya, yb, sa, sb, out, dy, _ = _join_case(SHAPES[0], True)
    B, C, L = ya.shape
    part = torch.empty(2, 2, C, ops.BN_SLOTS, device=DEV)
    rc = lib.fst_bn_bwd_reduce_join(dy.data_ptr(), ya.data_ptr(), yb.data_ptr(), sa.data_ptr(), sb.data_ptr(), 3 * B, C, L,
                                    part[0].data_ptr(), part[1].data_ptr(), ya.numel(), _lib.stream_ptr())
    assert rc < 0 and b"element count" in lib.fst_last_error()
    dx = torch.empty_like(ya)
    rc = lib.fst_bn_bwd_apply_join(dy.data_ptr(), ya.data_ptr(), yb.data_ptr(), sa.data_ptr(), sb.data_ptr(), part[0].data_ptr(),
                                   part[1].data_ptr(), ops.BN_SLOTS, None, None, dx.data_ptr(), None, None, None, 3 * B, C, L, 1,
                                   3 * B, ya.numel(), _lib.stream_ptr())
    assert rc < 0 and b"element count" in lib.fst_last_error()


# ------------------------------------------------------------------------------------------------ against fp64
@functools.lru_cache(maxsize=None)
def _module_single(shape, training):
    """BNActFn (ReLU) forward and backward on the device, and the fp64 composition with the ReLU mask taken from the device's
    own output (a value within rounding of 0 may fall on either side; the derivative is checked on the side the device took)."""
    B, C, L = shape
    g = torch.Generator().manual_seed(3000 + B * 31 + L)
    y = (torch.randn(B, C, L, generator=g, dtype=torch.float64) * 2 + 0.7).requires_grad_(True)
    gamma = torch.tensor(GAMMA[C], dtype=torch.float64, requires_grad=True)
    beta = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    dout = torch.randn(B, C, L, generator=g, dtype=torch.float64)
    f = lambda t: t.detach().float().to(DEV)
    d = [f(t).requires_grad_(True) for t in (y, gamma, beta)]
    got = ops.BNActFn.apply(d[0], d[1], d[2], f(rm), f(rv), training, True, EPS, 0.1)
    (got * f(dout)).sum().backward()
    pre = F.batch_norm(y, rm.clone(), rv.clone(), gamma, beta, training, 0.1, EPS)
    (pre * (got.detach() > 0).cpu() * dout).sum().backward()
    return got.detach(), F.relu(pre).detach(), [t.grad for t in d], [y.grad, gamma.grad, beta.grad]


@functools.lru_cache(maxsize=None)
def _module_join(shape):
    B, C, L = shape
    g = torch.Generator().manual_seed(4000 + B * 31 + L)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ya, yb = mk(B, C, L).requires_grad_(True), (mk(B, C, L) * 3 - 1).requires_grad_(True)
    ga = torch.tensor(GAMMA[C], dtype=torch.float64, requires_grad=True)
    gb = torch.tensor(GAMMA[C][::-1], dtype=torch.float64, requires_grad=True)
    ba, bb = mk(C).requires_grad_(True), mk(C).requires_grad_(True)
    dout = mk(B, C, L)
    f = lambda t: t.detach().float().to(DEV)
    ref = (ya, ga, ba, yb, gb, bb)
    d = [f(t).requires_grad_(True) for t in ref]
    bufs = [torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV)]
    got = ops.BNAddBNReluFn.apply(d[0], d[1], d[2], bufs[0], bufs[1], d[3], d[4], d[5], bufs[2], bufs[3], True, EPS, 0.1)
    (got * f(dout)).sum().backward()
    z, o = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    pre = F.batch_norm(ya, z.clone(), o.clone(), ga, ba, True, 0.1, EPS) + F.batch_norm(yb, z.clone(), o.clone(), gb, bb, True, 0.1, EPS)
    (pre * (got.detach() > 0).cpu() * dout).sum().backward()
    return got.detach(), F.relu(pre).detach(), [t.grad for t in d], [t.grad for t in ref]


# tolerances: those of test_batch_norm / test_bn_add_bn_relu in tests/test_gpu_kernels.py (1e-5 forward, 5e-5 gradients)
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_backward_without_out_against_fp64(shape, training):
    _, _, got, want = _module_single(shape, training)
    for a, b, name in zip(got, want, ("dx", "dgamma", "dbeta")):
        assert_close(a, b, 5e-5, name)


@pytest.mark.parametrize("shape", SHAPES)
def test_join_backward_against_fp64(shape):
    _, _, got, want = _module_join(shape)
    for a, b, name in zip(got, want, ("dya", "dga", "dba", "dyb", "dgb", "dbb")):
        assert_close(a, b, 5e-5, name)


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_unchanged_against_fp64(shape):
    for training in (True, False):
        got, want, _, _ = _module_single(shape, training)
        assert_close(got, want, 1e-5, f"BNActFn out (training={training})")
    got, want, _, _ = _module_join(shape)
    assert_close(got, want, 1e-5, "BNAddBNReluFn out")
    # and without the ReLU (the same pre-activation function, no max)
    B, C, L = shape
    g = torch.Generator().manual_seed(5000 + L)
    y = torch.randn(B, C, L, generator=g, dtype=torch.float64) * 2 + 0.7
    gamma, beta = torch.tensor(GAMMA[C], dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    f = lambda t: t.float().to(DEV)
    got = ops.BNActFn.apply(f(y), f(gamma), f(beta), torch.zeros(C, device=DEV), torch.ones(C, device=DEV), True, False, EPS, 0.1)
    assert_close(got, F.batch_norm(y, torch.zeros(C).double(), torch.ones(C).double(), gamma, beta, True, 0.1, EPS), 1e-5, "BN out")
