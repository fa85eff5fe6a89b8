#!/usr/bin/env python3
"""Timing: what the gradient norms and clipping (``JointTrainer.enable_grad_clip``) cost a replayed joint step at the bench
configuration (L=512, 256 pairs): the captured step with the mode off, on with no limit (``on``: the scan's read pass and a
scale that returns at once) and on with a cap at half the measured norm (``clip``: the scale's read-modify-write pass too).

    python tools/clip_cost.py [--steps N] [--repeats R] [--batch B] [--length L] [--modes off,on,clip] [--root DIR --label NAME]

One trainer per mode, built from the same seed, each with its joint capture resident.  R rounds that alternate one window of N
replays per mode, each window timed with device events around it, each starting from the trainer's restored snapshot and after
one untimed replay.  Prints one JSON line per mode: ``ms`` is the median of the R windows' ms per replay, ``ms_runs`` the R
figures themselves and ``spread_pct`` their (max − min) / median — what a difference between two lines has to exceed.  With the
mode on the line carries ``grad_l2_total`` and the smallest ``clip_coef`` of the last replay, and ``launches``: the launches the
mode adds to the graph (scan chunks + finaliser + scale chunks; the two report tensors cost four small torch launches more).

``--root DIR`` imports the package from another checkout (one that has built its library), e.g. the parent commit's, and
``--label`` names its lines; a checkout without the mode is measured with ``--modes off``.  Lines of different processes are
comparable when they ran in one session on one box, one after the other."""
import argparse
import json
import os
import statistics
import sys

import torch


def batch(B, L, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, L, generator=gen)
    x = (x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True)
    return x.to(dev), torch.randint(4, (B,), generator=gen).to(dev)


def window(step, n):
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
    ap.add_argument("--steps", type=int, default=20, help="replays per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="windows per mode; the median is reported")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--length", type=int, default=512)
    ap.add_argument("--modes", default="off,on,clip")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to import the package from")
    ap.add_argument("--label", default="", help="prefix of the 'config' field of this run's lines")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_cost.py needs an MI355X (a time taken anywhere else says nothing)")
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
        if m not in ("off", "on", "clip"):
            raise SystemExit(f"unknown mode {m!r}: off, on or clip")
        torch.manual_seed(1234)
        tr[m] = fst.JointTrainer(fst.JointConfig(L_t=a.length, L_s=a.length), dev)
        if m != "off":
            tr[m].enable_grad_clip()
        tr[m].capture(*args, epoch=0)
        snap[m] = tr[m].snapshot()
        if m == "clip":                                                       # set under the resident capture
            total = float(tr[m].replay(*args, draw())["grad_l2"][-1])
            tr[m].set_grad_clip(max_norm=total / 2)
    torch.manual_seed(4321)
    replay = lambda t: t.replay(*args, draw())
    runs = {m: [] for m in modes}
    for _ in range(a.repeats):
        for m in modes:
            tr[m].restore(snap[m])
            replay(tr[m])                                                     # untimed: this trainer's first replay after the other's
            runs[m].append(window(lambda: replay(tr[m]), a.steps))
    for m in modes:
        ms = statistics.median(runs[m])
        rep = replay(tr[m])
        line = {"workload": "joint", "config": (a.label + " " if a.label else "") + "mode " + m, "ms": round(ms, 3),
                "pairs_per_s": round(1e3 * a.batch / ms, 1), "ms_runs": [round(v, 3) for v in runs[m]],
                "spread_pct": round(100 * (max(runs[m]) - min(runs[m])) / ms, 2), "steps_per_window": a.steps,
                "windows": a.repeats, "batch": a.batch, "length": a.length, "arithmetic": ops.MATH,
                "losses_finite": all(bool(torch.isfinite(v).all()) for k, v in rep.items() if v.dtype.is_floating_point)}
        if m != "off":
            n = sum(1 for k in tr[m].MODULES for p in tr[m].m[k].parameters())
            chunks = (n + 63) // 64
            line.update(grad_l2_total=round(float(rep["grad_l2"][-1]), 6), clip_coef_min=round(float(rep["clip_coef"].min()), 6),
                        gradient_tensors=n, launches=2 * chunks + 1)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
