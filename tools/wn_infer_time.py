#!/usr/bin/env python3
"""Diagnostics: the saving WN forward kernels against the ones that store no gate halves (fst_wn_stack_infer / fst_wn_layer_infer) on
the same operands — the stack at the metric shape (n=120, h=25, B=256, L=512, 8 layers), the 4-wave layer pair at B=32 and the 8-wave
pair at B=256 — in alternating rounds of K launches each, HIP events around each batch; outputs compared bit for bit first."""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from feature_level_style_transfer_for_tsc_amd import ops

dev = "cuda"
g = torch.Generator(device=dev).manual_seed(5)
rnd = lambda *s, k=1.0: torch.randn(*s, generator=g, device=dev) * k
say = lambda s: print(s, flush=True)

def layer_w(n, h, last):
    R = n if last else 2 * n
    return (rnd(2 * n, n, 3, k=(3 * n) ** -0.5), rnd(2 * n, h, 1, k=h ** -0.5), rnd(2 * n, k=0.3), rnd(2 * n, k=0.3), rnd(R, n, 1, k=n ** -0.5), rnd(R, k=0.3))

def timed(fn, K):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(K): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000.0 / K          # us per launch

def compare(name, fa, fb, K, rounds):
    for _ in range(3): fa(); fb()
    torch.cuda.synchronize()
    A, Bv = [], []
    for r in range(rounds):
        if r % 2 == 0: A.append(timed(fa, K)); Bv.append(timed(fb, K))
        else: Bv.append(timed(fb, K)); A.append(timed(fa, K))
    f = lambda v: f"median {statistics.median(v):8.1f} us  min {min(v):8.1f}  max {max(v):8.1f}"
    say(f"{name}: {rounds} alternating rounds of {K} launches")
    say(f"  saving: {f(A)}")
    say(f"  infer : {f(Bv)}")
    say(f"  per-round infer/saving ratio: median {statistics.median([b / a for a, b in zip(A, Bv)]):.3f}  min {min(b / a for a, b in zip(A, Bv)):.3f}  max {max(b / a for a, b in zip(A, Bv)):.3f}")

say(f"device: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs")
# ---- the stack at the metric shape
n, h, B, L, nl = 120, 25, 256, 512, 8
imgs = [ops.wn_pack_layer(*layer_w(n, h, i == nl - 1), n, h, i == nl - 1) for i in range(nl)]
u0 = rnd(B, h, L)
a_s = [rnd(B, n, L)] + [torch.empty(B, n, L, device=dev) for _ in range(nl - 1)]
ts = [torch.empty(B, 2 * n, L, device=dev) for _ in range(nl)]
out_s, out_i = torch.empty(B, n, L, device=dev), torch.empty(B, n, L, device=dev)
a0 = a_s[0]
x, y = torch.empty_like(a0), torch.empty_like(a0)
a_i = [a0] + [(x, y)[(i - 1) % 2] for i in range(1, nl)]
f_s = lambda: ops.wn_stack_fwd(a_s, u0, imgs, ts, out_s, n, h)
f_i = lambda: ops.wn_stack_infer(a_i, u0, imgs, out_i, n, h)
f_s(); f_i(); torch.cuda.synchronize()
assert torch.equal(out_s, out_i), "stack: out differs"
say(f"stack n={n} h={h} B={B} L={L} nl={nl}: out bit-equal; routes {ops.wn_route_kernel_name(ops.wn_last_route())}")
compare("wn_stack_fwd_kernel vs wn_stack_infer_kernel (metric shape)", f_s, f_i, 20, 20)
del a_s, ts, x, y
# ---- the 4-wave layer pair at B=32, L=512 (a middle layer, dilation 16)
B = 32
img = ops.wn_pack_layer(*layer_w(n, h, False), n, h, False)
a, u0 = rnd(B, n, L), rnd(B, h, L)
ts1 = torch.empty(B, 2 * n, L, device=dev)
an_s, an_i = torch.empty(B, n, L, device=dev), torch.empty(B, n, L, device=dev)
o0 = rnd(B, n, L)
o_s, o_i = o0.clone(), o0.clone()
ops.wn_layer_fwd(a, u0, img, ts1, None, an_s, o_s, False, False, n, h, 16)
r1 = ops.wn_route_kernel_name(ops.wn_last_route())
ops.wn_layer_infer(a, u0, img, an_i, o_i, False, False, n, h, 16)
r2 = ops.wn_route_kernel_name(ops.wn_last_route())
torch.cuda.synchronize()
assert torch.equal(an_s, an_i) and torch.equal(o_s, o_i), "layer: outputs differ"
say(f"layer n={n} h={h} B={B} L={L} dil=16: a_next, out bit-equal; routes {r1} / {r2}")
compare(f"{r1} vs {r2}", lambda: ops.wn_layer_fwd(a, u0, img, ts1, None, an_s, o_s, False, False, n, h, 16),
        lambda: ops.wn_layer_infer(a, u0, img, an_i, o_i, False, False, n, h, 16), 200, 20)
# ---- the 8-wave layer pair at the metric batch, for the record
B = 256
a, u0 = rnd(B, n, L), rnd(B, h, L)
ts1 = torch.empty(B, 2 * n, L, device=dev)
an_s, an_i = torch.empty(B, n, L, device=dev), torch.empty(B, n, L, device=dev)
o_s, o_i = rnd(B, n, L), torch.empty(B, n, L, device=dev)
o_i.copy_(o_s)
compare("wn_layer_fwd_kernel<8> vs wn_layer_infer_kernel<8> (B=256, L=512, dil=16)",
        lambda: ops.wn_layer_fwd(a, u0, img, ts1, None, an_s, o_s, False, False, n, h, 16),
        lambda: ops.wn_layer_infer(a, u0, img, an_i, o_i, False, False, n, h, 16), 50, 20)
