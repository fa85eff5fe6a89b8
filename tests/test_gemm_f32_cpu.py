"""The inputs of the exact-fp32 GEMM's sharpest test (tests/test_gpu_gemm_f32.py), and what they can and cannot tell apart — no GPU.

``exact_operands`` builds integer-valued fp32 operands whose product fp32 holds EXACTLY in any order of summation: entries in
[-511, 511], one side dense, the other with at most 64 non-zero entries per row, so that every partial sum of every element is an
integer of magnitude <= 64·511² = 16 711 744 < 2²⁴.  A kernel that multiplies and adds in fp32 therefore returns the fp64 product
bit for bit, whatever its k order, its K split or its slab order.  A split-bf16 kernel does not: an odd integer above 256 has a
non-zero low half, and the lo·lo term that arithmetic drops is a whole number.  The tests below hold both statements on the CPU
for every shape the GPU test uses, so that the GPU test can neither ask more than fp32 gives nor pass a split-bf16 product."""
import functools

import pytest
import torch

from feature_level_style_transfer_for_tsc_amd import ops

NNZ = 64                  # non-zero entries per row of the sparse side
VMAX = 511                # |entry| <= VMAX: NNZ · VMAX² < 2²⁴

# M, N, K.  The first five are the issue's; the rest sit on either side of every threshold of gm_geometry (csrc/gemm.hip) on the
# 256 compute units of an MI355X — tests/test_gpu_gemm_f32.py lists the instance and the K split each one takes.
EXACT_SHAPES = [
    (37, 70, 45), (3, 4, 200), (96, 130, 700), (256, 1024, 1024), (130, 96, 4100),
    (95, 130, 16384), (96, 130, 16384),        # M < 96 | M >= 96 (first clause of the 128-tile rule)
    (130, 95, 16384), (130, 96, 16384),        # N < 96 | N >= 96
    (128, 128, 16383), (128, 128, 16384),      # tiles · (K / 128) below | at half the compute units
    (37, 70, 255), (37, 70, 256),              # fewer than two splits of four stages: no split | two splits
    (1024, 1024, 1024),                        # the split count set by the compute units (4), not by K (8)
    (2100, 2100, 300),                         # more tiles than compute units: no split although K allows two
]


@functools.lru_cache(maxsize=None)
def exact_operands(M: int, N: int, K: int, sparse_a: bool = True):
    """(A [M, K], B [N, K], A·Bᵀ in fp64): integer-valued fp32 operands, the sparse side with at most NNZ non-zero entries per row
    at random k.  Cached: the tests that share a shape share one reference, and must leave it unchanged."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K + (7 if sparse_a else 0))

    def ints(rows):
        return torch.randint(-VMAX, VMAX + 1, (rows, K), generator=g).float()

    def sparse(rows):
        keep = torch.rand(rows, K, generator=g).argsort(dim=1)[:, :NNZ]
        mask = torch.zeros(rows, K).scatter_(1, keep, 1.0)
        return ints(rows) * mask
    A, B = (sparse(M), ints(N)) if sparse_a else (ints(M), sparse(N))
    return A, B, A.double() @ B.double().t()


def split_bf16_product(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """hi·hi + hi·lo + lo·hi of the split-bf16 kernels, the three products summed without rounding (fp64)."""
    def split(x):
        hi = x.bfloat16().float()
        return hi.double(), (x - hi).bfloat16().double()
    ah, al = split(A)
    bh, bl = split(B)
    return ah @ bh.t() + ah @ bl.t() + al @ bh.t()


@pytest.mark.parametrize("sparse_a", [True, False])
@pytest.mark.parametrize("M,N,K", EXACT_SHAPES)
def test_fp32_holds_the_product_exactly_and_split_bf16_does_not(M, N, K, sparse_a):
    A, B, want = exact_operands(M, N, K, sparse_a)
    assert int((A != 0).sum(1).max() if sparse_a else (B != 0).sum(1).max()) <= NNZ
    assert float(A.abs().max()) <= VMAX and float(B.abs().max()) <= VMAX and float(want.abs().max()) < 2 ** 24
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(K))
    assert torch.equal((A @ B.t()).double(), want), "fp32 product in storage order is not exact"
    assert torch.equal((A[:, perm] @ B[:, perm].t()).double(), want), "fp32 product in a permuted k order is not exact"
    wrong = float((split_bf16_product(A, B) != want).double().mean())
    print(f"  {M}x{N}x{K} sparse_a={sparse_a}: split-bf16 differs in {100 * wrong:.0f} % of the elements")
    assert wrong >= 0.5, f"a split-bf16 product would pass the exactness test in {100 * (1 - wrong):.0f} % of the elements"


def test_gemm_f32_refuses_cpu_tensors():
    a = torch.zeros(4, 4)
    assert not ops.gemm_f32_ok(a, a)
    with pytest.raises(ValueError):
        ops.gemm_f32(a, False, a, False)


def test_gemm_f32_ok_does_not_read_the_arithmetic_mode(monkeypatch):
    class Loud:
        def __eq__(self, other):
            raise AssertionError("gemm_f32_ok compared ops.MATH")
        __ne__ = __eq__
        __hash__ = None
    a = torch.zeros(4, 4)
    monkeypatch.setattr(ops, "MATH", Loud())
    assert ops.gemm_f32_ok(a) is False                                  # (a CPU tensor; answered without touching MATH)
    monkeypatch.setattr(ops, "MATH", "f32")
    f32 = ops.gemm_f32_ok(a, a[:, :2])
    monkeypatch.setattr(ops, "MATH", "bf16x3")
    assert ops.gemm_f32_ok(a, a[:, :2]) is f32
