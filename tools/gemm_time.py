#!/usr/bin/env python3
"""Diagnostics: HIP-event time of fst_gemm (split-bf16) and fst_gemm_f32 (exact fp32) against the library GEMM (torch.mm / addmm:
hipBLASLt, exact f32) at the dense products the joint step runs (tools/gemm_census.py), per operand layout; and RandomLayer's two
products on gemm_f32 against the route they took before it (FixedMatmulFn: the conv engine's K-split GEMM, float atomics) under
ops.MATH = "f32", alternating in one process, three repeats each, as a share of the 85 us compute floor (13.4 GFLOP over the
157.3 TFLOP/s fp32 matrix-core peak)."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feature_level_style_transfer_for_tsc_amd import ops

dev = "cuda"


def t_us(fn, n=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return 1000 * e0.elapsed_time(e1) / n


SHAPES = [("dimunif", 12800, 512, 512), ("ad_net", 256, 1024, 1024), ("fd 800-400", 256, 400, 800), ("fd 50-800", 256, 800, 50),
          ("cpc proj", 20992, 192, 50)]
for name, M, N, K in SHAPES:
    x, W, b, g = torch.randn(M, K, device=dev), torch.randn(N, K, device=dev), torch.randn(N, device=dev), torch.randn(M, N, device=dev)
    rows = [
        ("fwd  y=xW^T+b,relu", lambda: ops.gemm(x, False, W, False, b, ops.ACT_RELU), lambda: torch.relu(torch.addmm(b, x, W.t()))),
        ("dx = g W          ", lambda: ops.gemm(g, False, W, True), lambda: g @ W),
        ("dW = g^T x        ", lambda: ops.gemm(g, True, x, True), lambda: g.t() @ x),
    ]
    rows32 = [lambda: ops.gemm_f32(x, False, W, False, b, ops.ACT_RELU), lambda: ops.gemm_f32(g, False, W, True),
              lambda: ops.gemm_f32(g, True, x, True)]
    for (what, ours, lib), ours32 in zip(rows, rows32):
        a, a32, c = t_us(ours), t_us(ours32), t_us(lib)
        print(f"{name:12s} M={M:6d} N={N:5d} K={K:5d}  {what}  fst_gemm {a:7.1f} us ({2e-6 * M * N * K / a:6.1f} TFLOP/s)   "
              f"gemm_f32 {a32:7.1f} us ({2e-6 * M * N * K / a32:6.1f} TFLOP/s)   library {c:7.1f} us")

# RandomLayer (C_DAN.py:21): x [256, 25600] · R0 [25600, 1024] and its data gradient dy [256, 1024] · R0ᵀ
x, R0, dy = torch.randn(256, 25600, device=dev), torch.randn(25600, 1024, device=dev), torch.randn(256, 1024, device=dev)
R0t = R0.t().contiguous()
for what, ours, lib in [("x R0   (R0 k-major)     ", lambda: ops.gemm(x, False, R0, True), lambda: x @ R0),
                        ("x R0   (R0^T contiguous)", lambda: ops.gemm(x, False, R0t, False), lambda: x @ R0),
                        ("dy R0^T (R0 rows = n)   ", lambda: ops.gemm(dy, False, R0, False), lambda: dy @ R0.t()),
                        ("nt_gemm fwd             ", lambda: ops.nt_gemm(x, R0t), lambda: x @ R0),
                        ("nt_gemm dgrad           ", lambda: ops.nt_gemm(dy, R0), lambda: dy @ R0.t())]:
    a, c = t_us(ours), t_us(lib)
    print(f"random layer  {what}  ours {a:7.1f} us   library {c:7.1f} us")

# RandomLayer in exact fp32: gemm_f32 against the conv engine's K-split GEMM it replaces, alternating, three repeats
FLOOR_US = 2.0 * 256 * 1024 * 25600 / 157.3e12 * 1e6
prev, ops.MATH = ops.MATH, "f32"
try:
    for what, new, old in [("x R0    256 x 1024 x 25600", lambda: ops.gemm_f32(x, False, R0t, False), lambda: ops._fixed_matmul(x, R0, 256, 25600, 1024)),
                           ("dy R0^T 256 x 25600 x 1024", lambda: ops.gemm_f32(dy, False, R0t, True), lambda: ops._fixed_matmul(dy, R0t, 256, 1024, 25600))]:
        for rep in range(3):
            a, c = t_us(new), t_us(old)
            print(f"random layer f32  {what}  repeat {rep}  gemm_f32 {a:7.1f} us ({100 * FLOOR_US / a:5.1f} % of the {FLOOR_US:.0f} us floor)   "
                  f"FixedMatmulFn route {c:7.1f} us ({100 * FLOOR_US / c:5.1f} %)")
finally:
    ops.MATH = prev
