#!/usr/bin/env python3
"""Diagnostics: HIP-event time of the 16 weight-gradient launches of one WN (8 layers x in_layer / res_skip, csrc/wn_wgrad.hip) at
the bench's shapes, with every launch adding its own slabs (fst_wn_wgrad_in / _rs) and with one reduction launch for all of them
(fst_wn_wgrad_reduce_many).  SETS=<k>: k operand sets per launch."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feature_level_style_transfer_for_tsc_amd import ops

dev = "cuda"
B, L, n, h, nl = 256, int(os.environ.get("L", 512)), 120, 25, 8
NS = int(os.environ.get("SETS", 3))
g = torch.Generator(device=dev).manual_seed(0)
rnd = lambda *s: torch.randn(*s, generator=g, device=dev)


def slack(t):
    return ops.empty_with_slack(*t.shape, dev).copy_(t)


a, dg, ts, d_a, d_out = ([x] * NS for x in (slack(rnd(B, n, L)), rnd(B, 2 * n, L), rnd(B, 2 * n, L), rnd(B, n, L), rnd(B, n, L)))
u0 = [rnd(B, 2 * h, L)[:, :h]] * NS
dw_in = [torch.empty(2 * n, n, 3, device=dev) for _ in range(nl)]
dw_cond = [torch.empty(2 * n, h, 1, device=dev) for _ in range(nl)]
dw_rs = [torch.empty(n if i == nl - 1 else 2 * n, n, 1, device=dev) for i in range(nl)]


def stack(batched):
    slabs = [] if batched else None
    for i in reversed(range(nl)):
        last = i == nl - 1
        ops.wn_wgrad_rs(None if last else d_a, d_out, ts, dw_rs[i], last, n, slabs=slabs)
        ops.wn_wgrad_in(dg, a, u0, dw_in[i], dw_cond[i], n, h, 2 ** i, slabs=slabs)
    if batched:
        ops.wn_wgrad_reduce_many(slabs, B, L, n, h)


def timed(fn, reps=10):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


stack(False)
want = [t.clone() for t in dw_in + dw_cond + dw_rs]
stack(True)
same = all(torch.equal(x, y) for x, y in zip(want, dw_in + dw_cond + dw_rs))
per_layer, batched = timed(lambda: stack(False)), timed(lambda: stack(True))
print(f"sets={NS}  16 launches, own reductions: {per_layer:7.1f} us   one reduction: {batched:7.1f} us   same bits: {same}")
