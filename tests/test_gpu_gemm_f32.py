"""fst_gemm_f32 (csrc/gemm.hip: gemm_f32_kernel<TM, TN>) — fst_gemm's contract in exact fp32 on the fp32 matrix-core instruction —
through ``ops.gemm_f32`` and the C ABI on the MI355X, ``ops.FixedGemmF32Fn`` on it, and ``RandomLayer``'s route to it under
FST_MATH=f32.  The kernel does not read ``ops.MATH``: nothing here is skipped in either arithmetic.

1. Exactness.  Integer operands whose product fp32 holds exactly in any order (tests/test_gemm_f32_cpu.py builds them and shows on
   the CPU that fp32 is exact and split-bf16 wrong in most elements): the result equals the fp64 product bit for bit.
2. Random operands at the shapes of tests/test_gpu_gemm.py against fp64 at that file's gate, 2e-5 of max|want| (the project's
   fp32 products measure about 1e-6 of it; 5e-6 would mean bf16 crept in), and the same bits on a second call.
3. Bands: pitched, unaligned operands between NaN bands, C with ldc > N between canaries, a workspace of exactly the queried size.
4. Ragged edges in M, N and K.   5. Refusals write nothing.   6. A NaN / inf stays in its row (column).
7. ``FixedGemmF32Fn`` and ``RandomLayer`` under both arithmetics.

Instance and K split of the exactness shapes on the 256 compute units of an MI355X (gm_geometry; the split is read off
fst_gemm_f32_workspace_floats / (M·N), the instance from the rule restated in tests/test_gpu_seq_edges.py) — GEOMETRY_256 below:
<1, 1> = 64 x 64 tiles, <2, 2> = 128 x 128 tiles."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import _lib, ops
from test_gemm_f32_cpu import EXACT_SHAPES, exact_operands
from test_gpu_gemm import SHAPES, act64, close
from test_gpu_seq_edges import GEMM_CASES, LDC_PAD, Gm, assert_written, gm_geometry, pitched, rnd32, same_bits
from test_gpu_wn_routes import (CANARY, DEV, NAN, assert_close, assert_fence, assert_untouched, check_rc, fenced, nan_in,
                                workspace)

LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]
# shape -> (128 x 128 tiles, K split) on 256 compute units
GEOMETRY_256 = {
    (37, 70, 45): (False, 1), (3, 4, 200): (False, 1), (96, 130, 700): (False, 5), (256, 1024, 1024): (True, 8),
    (130, 96, 4100): (False, 26),
    (95, 130, 16384): (False, 40), (96, 130, 16384): (True, 128), (130, 95, 16384): (False, 40), (130, 96, 16384): (True, 128),
    (128, 128, 16383): (False, 64), (128, 128, 16384): (True, 128), (37, 70, 255): (False, 1), (37, 70, 256): (False, 2),
    (1024, 1024, 1024): (True, 4), (2100, 2100, 300): (True, 1),
}
WORST = {"ratio": 0.0}


def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def _laid_out(X: torch.Tensor, t: bool) -> torch.Tensor:
    """[rows, K] on the host -> the device matrix ``gemm_f32`` reads with flag ``t`` ([K, rows] when set)."""
    X = X.t() if t else X
    return torch.empty(X.shape).copy_(X).to(DEV)                       # (not .contiguous(): it keeps the strides of a [K, 1] view)


# --------------------------------------------------------------------------------------------------
# 1. exactness
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse_a", [True, False], ids=["sparseA", "sparseB"])
@pytest.mark.parametrize("M,N,K", EXACT_SHAPES)
def test_integer_product_is_exact_in_every_layout(M, N, K, sparse_a):
    A, B, want = exact_operands(M, N, K, sparse_a)
    ws_n = _lib.load().fst_gemm_f32_workspace_floats(M, N, K)
    big, ksplit, _ = gm_geometry(M, N, K, _cus())
    assert ws_n == (ksplit * M * N if ksplit > 1 else 0), f"workspace query {ws_n} vs K split {ksplit}"
    if _cus() == 256:
        assert (big, ksplit) == GEOMETRY_256[(M, N, K)], f"{M}x{N}x{K}: 128-tile {big}, K split {ksplit}"
    want = want.to(DEV)
    for ta, tb in LAYOUTS:
        got = ops.gemm_f32(_laid_out(A, ta), ta, _laid_out(B, tb), tb)
        wrong = int((got.double() != want).sum())
        assert wrong == 0, (f"{M}x{N}x{K} ta={ta} tb={tb}: {wrong} of {M * N} elements are not the exact product, "
                            f"max difference {float((got.double() - want).abs().max())}")


# --------------------------------------------------------------------------------------------------
# 2. random operands against fp64
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_layouts_vs_fp64(M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A0, B0, bias0 = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    want = A0.double() @ B0.double().t()
    bias = bias0.to(DEV)
    scale = float(want.abs().max())
    for ta, tb in LAYOUTS:
        A, B = _laid_out(A0, ta), _laid_out(B0, tb)
        got = ops.gemm_f32(A, ta, B, tb)
        ratio = float((got.double().cpu() - want).abs().max()) / scale
        WORST["ratio"] = max(WORST["ratio"], ratio)
        print(f"  gemm_f32 {M}x{N}x{K} ta={ta} tb={tb}: max err / max|want| = {ratio:.3e} (worst so far {WORST['ratio']:.3e})")
        close(got, want, 2e-5, f"gemm_f32 {M}x{N}x{K} ta={ta} tb={tb}")
        for act, slope in ((ops.ACT_RELU, 0.0), (ops.ACT_LEAKY, 0.2)):
            close(ops.gemm_f32(A, ta, B, tb, bias, act, slope), act64(want + bias0.double(), act, slope), 2e-5,
                  f"gemm_f32+bias+act{act} {M}x{N}x{K} ta={ta} tb={tb}")
        assert torch.equal(ops.gemm_f32(A, ta, B, tb), got), "two calls differ (no epilogue)"
        assert torch.equal(ops.gemm_f32(A, ta, B, tb, bias, ops.ACT_RELU), ops.gemm_f32(A, ta, B, tb, bias, ops.ACT_RELU))


# --------------------------------------------------------------------------------------------------
# 3. + 4. bands and ragged edges through the C ABI
# --------------------------------------------------------------------------------------------------
# last K slice of 1 (K % 32 == 1) and of 31, M / N of 1, 31, 33, 65, 129, a single output column, and (4099: tests/test_gpu_seq_edges.py
# shows every admissible k_per_split leaves it ragged) a last split shorter than the others
RAGGED = [Gm(1, 31, 33), Gm(31, 1, 63), Gm(33, 65, 33), Gm(65, 129, 63), Gm(129, 33, 95), Gm(129, 129, 97),
          Gm(129, 1, 4099, split=True), Gm(31, 33, 4099, split=True)]


@pytest.mark.parametrize("c", GEMM_CASES + RAGGED, ids=lambda c: c.id)
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_pitched_operands_and_output_in_bands(ta, tb, c: Gm):
    lib = _lib.load()
    g = torch.Generator().manual_seed(c.M * 1000003 + c.N * 1009 + c.K + 2 * ta + tb)
    M, N, K = c.M, c.N, c.K
    A64, B64, bias64 = rnd32(g, M, K), rnd32(g, N, K), rnd32(g, N)
    want = A64 @ B64.t()
    Ad, lda = pitched((A64.t() if ta else A64).contiguous(), c.aligned)
    Bd, ldb = pitched((B64.t() if tb else B64).contiguous(), c.aligned)
    if not c.aligned:
        assert Ad.data_ptr() % 16 != 0 and Bd.data_ptr() % 16 != 0
    bias = nan_in(bias64)
    ws_n = lib.fst_gemm_f32_workspace_floats(M, N, K)
    big, ksplit, kps = gm_geometry(M, N, K, _cus())
    assert (big, ksplit > 1) == (c.big, c.split), f"{c.id} on {_cus()} compute units: 128-tile {big}, K split {ksplit}"
    assert ws_n == (ksplit * M * N if ksplit > 1 else 0)
    if c.split:
        assert K % kps != 0, "the last split is not shorter than the others"

    def run(with_bias, act, slope, ws_floats=None, expect_ok=True):
        bC, full = fenced((M, N + LDC_PAD), CANARY, CANARY)
        Cv = full[:, :N]
        Cv.fill_(NAN)
        bw, ws = workspace(ws_n) if ws_n else (None, None)
        rc = lib.fst_gemm_f32(Ad.data_ptr(), lda, ta, Bd.data_ptr(), ldb, tb, Cv.data_ptr(), N + LDC_PAD, M, N, K,
                              bias.data_ptr() if with_bias else None, act, slope, _lib.ptr(ws), ws_n if ws_floats is None else ws_floats,
                              _lib.stream_ptr())
        torch.cuda.synchronize()
        if not expect_ok:
            assert rc != 0 and b"fst_gemm_f32" in lib.fst_last_error(), "a workspace one float short was accepted"
            assert_untouched(bC, Cv, "C"), assert_untouched(bw, ws, "slab workspace")
            return None
        check_rc(rc, c.id)
        assert_fence(bC, Cv, "C (pad columns and bands)")
        if ws is not None:
            assert_fence(bw, ws, "slab workspace")
        assert_written(Cv, "C")
        return Cv

    plain = run(False, ops.ACT_NONE, 0.0)
    assert_close(plain.cpu(), want, 2e-5, f"C ta={ta} tb={tb}")
    wb = want + bias64
    assert_close(run(True, ops.ACT_NONE, 0.0).cpu(), wb, 2e-5, "C + bias")
    relu = run(True, ops.ACT_RELU, 0.0)
    assert_close(relu.cpu(), wb.clamp_min(0), 2e-5, "relu(C + bias)")          # (either branch of a ~0 unit is ~0)
    assert_close(run(True, ops.ACT_LEAKY, 0.2).cpu(), torch.where(wb > 0, wb, 0.2 * wb), 2e-5, "leaky(C + bias)")
    assert same_bits(run(False, ops.ACT_NONE, 0.0), plain), "two identical launches differ (no epilogue)"
    assert same_bits(run(True, ops.ACT_RELU, 0.0), relu), "two identical launches differ (bias + ReLU)"
    if c.split:
        run(False, ops.ACT_NONE, 0.0, ws_floats=ws_n - 1, expect_ok=False)


# --------------------------------------------------------------------------------------------------
# 5. refusals
# --------------------------------------------------------------------------------------------------
def test_refusals_name_the_entry_point_and_write_nothing():
    lib = _lib.load()
    M, N, K = 256, 1024, 1024
    ws_n = lib.fst_gemm_f32_workspace_floats(M, N, K)
    assert ws_n > 0 and ws_n % (M * N) == 0
    x, w = torch.zeros(1024, 1024, device=DEV), torch.zeros(1024, 1024, device=DEV)
    bC, Cv = fenced((M, N), CANARY, NAN)
    bw, ws = workspace(ws_n)
    ok = dict(lda=1024, ta=0, ldb=1024, tb=0, ldc=N, act=0, ws=ws.data_ptr(), ws_n=ws_n, a=x.data_ptr(), b=w.data_ptr(), c=Cv.data_ptr())
    bad = [("lda < K", dict(lda=K - 1)), ("k-major lda < M", dict(ta=1, lda=M - 1)), ("ldb < K", dict(ldb=K - 1)),
           ("k-major ldb < N", dict(tb=1, ldb=N - 1)), ("ldc < N", dict(ldc=N - 1)), ("activation 3", dict(act=3)),
           ("workspace one float short", dict(ws_n=ws_n - 1)), ("no workspace with a split", dict(ws=None, ws_n=0)),
           ("null A", dict(a=None)), ("null B", dict(b=None)), ("null C", dict(c=None))]
    for what, change in bad:
        a = dict(ok, **change)
        rc = lib.fst_gemm_f32(a["a"], a["lda"], a["ta"], a["b"], a["ldb"], a["tb"], a["c"], a["ldc"], M, N, K, None, a["act"], 0.0,
                              a["ws"], a["ws_n"], _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc != 0 and b"fst_gemm_f32" in lib.fst_last_error(), f"{what}: rc={rc}, {lib.fst_last_error()}"
        assert_untouched(bC, Cv, f"C ({what})"), assert_untouched(bw, ws, f"slab workspace ({what})")
    for M_, N_, K_ in ((0, N, K), (M, -1, K), (M, N, 0)):
        assert lib.fst_gemm_f32(ok["a"], 1024, 0, ok["b"], 1024, 0, ok["c"], N, M_, N_, K_, None, 0, 0.0, ok["ws"], ws_n, _lib.stream_ptr()) != 0
        assert b"fst_gemm_f32" in lib.fst_last_error() and lib.fst_gemm_f32_workspace_floats(M_, N_, K_) == -1
    torch.cuda.synchronize()
    assert_untouched(bC, Cv, "C (sizes)")
    with pytest.raises(ValueError):
        ops.gemm_f32(x, False, w[:, :512], False)                             # reduction lengths differ
    with pytest.raises(ValueError):
        ops.gemm_f32(x, False, w, False, torch.zeros(7, device=DEV))          # bias is not [N]


# --------------------------------------------------------------------------------------------------
# 6. non-finite values
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("M,N,K", [(130, 70, 100), (130, 130, 8192)], ids=["tile64", "tile128"])
def test_a_non_finite_operand_stays_in_its_row_or_column(M, N, K, value):
    """One NaN / +inf in A[m0, k0] (then in B[n0, k0]): row m0 (column n0) of C is non-finite wherever the fp64 product is, and every
    other row (column) carries the bits of the clean run.  Places: element 0, the last element, either side of a stage edge
    (k = 31 | 32), either side of a tile edge (row 127 | 128; also an edge of the 64-row tiles)."""
    if _cus() == 256:
        assert gm_geometry(M, N, K, 256)[0] == (K == 8192)
    g = torch.Generator().manual_seed(M + N + K)
    A0, B0 = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    clean = ops.gemm_f32(A0.to(DEV), False, B0.to(DEV), False)
    assert bool(torch.isfinite(clean).all())
    for r0, k0 in ((0, 0), (M - 1, K - 1), (5, 31), (5, 32), (127, 7), (128, 7)):
        Ap = A0.clone()
        Ap[r0, k0] = value
        got = ops.gemm_f32(Ap.to(DEV), False, B0.to(DEV), False)
        want_bad = ~torch.isfinite(Ap.double() @ B0.double().t())
        assert bool(want_bad[r0].all()) and int(want_bad.sum()) == N
        assert not bool(torch.isfinite(got[r0].cpu())[want_bad[r0]].any()), f"A[{r0}, {k0}] = {value}: row {r0} has finite elements"
        keep = torch.arange(M, device=DEV) != r0
        assert same_bits(got[keep], clean[keep]), f"A[{r0}, {k0}] = {value}: another row of C moved"
    for c0, k0 in ((0, 0), (N - 1, K - 1), (5, 31), (5, 32), (63, 7), (64, 7)) + (((127, 7), (128, 7)) if N > 128 else ()):
        Bp = B0.clone()
        Bp[c0, k0] = value
        got = ops.gemm_f32(A0.to(DEV), False, Bp.to(DEV), False)
        assert not bool(torch.isfinite(got[:, c0]).any()), f"B[{c0}, {k0}] = {value}: column {c0} has finite elements"
        keep = torch.arange(N, device=DEV) != c0
        assert same_bits(got[:, keep], clean[:, keep]), f"B[{c0}, {k0}] = {value}: another column of C moved"


# --------------------------------------------------------------------------------------------------
# 7. FixedGemmF32Fn and RandomLayer's route
# --------------------------------------------------------------------------------------------------
def test_fixed_gemm_fn_reads_one_copy_of_the_matrix():
    g = torch.Generator().manual_seed(5)
    x0, R, cot = torch.randn(7, 300, generator=g), torch.randn(300, 130, generator=g), torch.randn(7, 130, generator=g)
    Rt = R.t().contiguous().to(DEV)
    x = x0.to(DEV).requires_grad_(True)
    y = ops.FixedGemmF32Fn.apply(x, Rt)
    dx, = torch.autograd.grad(y, [x], cot.to(DEV))
    close(y, x0.double() @ R.double(), 2e-5, "y = x R")
    close(dx, cot.double() @ R.double().t(), 2e-5, "dx = dy Rt")
    # a cotangent that is an expanded scalar (strides (0, 0)) is copied, not read with overlapping rows
    dx1, = torch.autograd.grad(ops.FixedGemmF32Fn.apply(x, Rt).sum(), [x])
    close(dx1, torch.ones(7, 130, dtype=torch.float64) @ R.double().t(), 2e-5, "dx of sum(y)")


@pytest.mark.parametrize("B,D", [(4, 310), (4, 320), (4, 330), (4, 5200), (256, 25600)])
def test_random_layer_routes_by_arithmetic(B, D, monkeypatch):
    torch.manual_seed(D)
    rl = fst.RandomLayer([D, 3], 1024).to(DEV)
    x0, p0, cot = torch.randn(B, D, device=DEV), torch.softmax(torch.randn(B, 3, device=DEV), 1), torch.randn(B, 1024, device=DEV)

    def run():
        timer = ops.KernelTimer()
        monkeypatch.setattr(ops, "KERNEL_TIMER", timer)
        x, p = x0.clone().requires_grad_(True), p0.clone().requires_grad_(True)
        out = rl([x, p])
        got = (out.detach(),) + torch.autograd.grad(out, (x, p), cot)
        monkeypatch.setattr(ops, "KERNEL_TIMER", None)
        return got, {k: v["launches"] for k, v in timer.summary().items()}

    monkeypatch.setattr(ops, "MATH", "f32")
    got, keys = run()
    again, _ = run()
    assert keys == {"gemm_f32_kernel f32": 2}, f"FST_MATH=f32 launched {keys}"
    assert not [k for k in keys if k.startswith(("conv_", "gemm_bf3", "nt_gemm"))]
    x, p = x0.double().requires_grad_(True), p0.double().requires_grad_(True)       # (the fp64 reference on the device: 27 GFLOP at the bench shape)
    R0, R1 = (m.double() for m in rl.random_matrix)
    want = (x @ R0) / 32.0 * (p @ R1)
    want = (want.detach(),) + torch.autograd.grad(want, (x, p), cot.double())
    for name, g_, a_, w_ in zip(("out", "dx", "dp"), got, again, want):
        close(g_, w_, 2e-5, f"RandomLayer B={B} D={D} {name}")
        assert torch.equal(g_, a_), f"RandomLayer B={B} D={D}: {name} differs between two runs"
    monkeypatch.setattr(ops, "MATH", "bf16x3")
    _, keys = run()
    assert set(keys) == {"nt_gemm (wn_wgrad_kernel<2, 2>) bf3"} and keys["nt_gemm (wn_wgrad_kernel<2, 2>) bf3"] == 2, f"split-bf16 launched {keys}"
