#!/usr/bin/env python3
"""Timing: what gradient accumulation (``JointTrainer.enable_grad_accumulation``) costs a replayed joint micro-step at the bench
configuration (L=512, 256 pairs): the captured step with the mode off (one graph), on with one step per window (``k1``: the
micro-step graph, whose folds return at once, and the update graph behind every call) and on with four (``k4``: the folds' memory
passes on every call, the update graph on every fourth).

    python tools/accum_cost.py [--steps N] [--repeats R] [--batch B] [--length L] [--modes off,k1,k4] [--root DIR --label NAME]

One trainer per mode, built from the same seed, each with its joint capture resident.  R rounds that alternate one timed run of
N replays per mode (N a multiple of 4: whole accumulation windows), each timed with device events around it, each starting from
the trainer's restored snapshot and after one untimed accumulation window.  Prints one JSON line per mode: ``ms`` is the median of
the R runs' ms per replay — per MICRO-step, so an optimiser step of ``k4`` costs four of them —, ``ms_runs`` the R figures
themselves and ``spread_pct`` their (max − min) / median — what a difference between two lines has to exceed.  With the mode on
the line carries ``gradient_tensors``, ``fold_mb`` (the bytes one closing fold moves: accumulator read and written, gradient read
and written) and ``launches``: the launches the mode adds to a micro-step (fold chunks of the gradients, the scalars' fold, the
advance; the position's report costs one small torch launch more).

``--root DIR`` imports the package from another checkout (one that has built its library), e.g. the parent commit's, and
``--label`` names its lines; a checkout without the mode is measured with ``--modes off``.  Lines of different processes are
comparable when they ran in one session on one box, one after the other."""
import argparse
import json
import os
import statistics
import sys

import torch

STEPS = {"off": None, "k1": 1, "k4": 4}


def batch(B, L, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, L, generator=gen)
    x = (x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True)
    return x.to(dev), torch.randint(4, (B,), generator=gen).to(dev)


def timed(step, n):
    """ms per call of ``step`` over ``n`` calls, between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="replays per timed run (a multiple of 4)")
    ap.add_argument("--repeats", type=int, default=5, help="timed runs per mode; the median is reported")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--length", type=int, default=512)
    ap.add_argument("--modes", default="off,k1,k4")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to import the package from")
    ap.add_argument("--label", default="", help="prefix of the 'config' field of this run's lines")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("accum_cost.py needs an MI355X (a time taken anywhere else says nothing)")
    if a.steps % 4:
        raise SystemExit("--steps must be a multiple of 4: a timed run is a whole number of accumulation windows")
    sys.path.insert(0, os.path.abspath(a.root))
    import feature_level_style_transfer_for_tsc_amd as fst
    from feature_level_style_transfer_for_tsc_amd import ops
    dev = torch.device("cuda:0")
    (x_t, y_t), (x_s, y_s) = batch(a.batch, a.length, 1000, dev), batch(a.batch, a.length, 2000, dev)
    args = (x_t, y_t, x_s, y_s)
    T_half = max(1, (a.length // 2) // 2)
    draw = lambda: (int(torch.randint(T_half, (1,))), int(torch.randint(T_half, (1,))))
    modes = a.modes.split(",")
    tr, snap = {}, {}
    for m in modes:
        if m not in STEPS:
            raise SystemExit(f"unknown mode {m!r}: one of {sorted(STEPS)}")
        torch.manual_seed(1234)
        tr[m] = fst.JointTrainer(fst.JointConfig(L_t=a.length, L_s=a.length), dev)
        if STEPS[m] is not None:
            tr[m].enable_grad_accumulation(STEPS[m])
        tr[m].capture(*args, epoch=0)
        snap[m] = tr[m].snapshot()
    torch.manual_seed(4321)
    replay = lambda t: t.replay(*args, draw())
    runs = {m: [] for m in modes}
    for _ in range(a.repeats):
        for m in modes:
            tr[m].restore(snap[m])
            for _ in range(STEPS[m] or 1):                                    # untimed: this trainer's first window after the other's
                replay(tr[m])
            runs[m].append(timed(lambda: replay(tr[m]), a.steps))
    for m in modes:
        ms = statistics.median(runs[m])
        for _ in range(STEPS[m] or 1):
            rep = replay(tr[m])                                               # the last one closes a window: the whole report
        line = {"workload": "joint", "config": (a.label + " " if a.label else "") + "mode " + m, "ms": round(ms, 3),
                "pairs_per_s": round(1e3 * a.batch / ms, 1), "ms_runs": [round(v, 3) for v in runs[m]],
                "spread_pct": round(100 * (max(runs[m]) - min(runs[m])) / ms, 2), "steps_per_run": a.steps,
                "runs": a.repeats, "batch": a.batch, "length": a.length, "arithmetic": ops.MATH,
                "losses_finite": all(bool(torch.isfinite(v).all()) for k, v in rep.items() if v.dtype.is_floating_point)}
        if STEPS[m] is not None:
            grads = [p.grad for p in tr[m].parameters() if p.grad is not None]
            line.update(steps_per_window=STEPS[m], graphs=len(tr[m]._graphs), gradient_tensors=len(grads),
                        fold_mb=round(4 * 4 * sum(g.numel() for g in grads) / 1e6, 1), launches=(len(grads) + 63) // 64 + 2,
                        windows_closed=int(tr[m].grad_accumulation.windows))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
