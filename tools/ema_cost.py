#!/usr/bin/env python3
"""Timing: what the weight averaging (``JointTrainer.enable_weight_average``) costs a replayed joint step at the bench
configuration (L=512, 256 pairs): the captured step with the mode off and with it on (``on``: one read-modify-write pass over a
copy of every parameter and fp32 buffer plus a read pass over the live ones, behind a one-workgroup prologue).

    python tools/ema_cost.py [--steps N] [--repeats R] [--batch B] [--length L] [--modes off,on] [--root DIR --label NAME]

One trainer per mode, built from the same seed, each with its joint capture resident.  R rounds that alternate one window of N
replays per mode, each window timed with device events around it, each starting from the trainer's restored snapshot and after
one untimed replay.  Prints one JSON line per mode: ``ms`` is the median of the R windows' ms per replay, ``ms_runs`` the R
figures themselves and ``spread_pct`` their (max − min) / median — what a difference between two lines has to exceed.  With the
mode on the line carries the tensors and bytes averaged (``averaged_mb``: one copy; the pass moves three times that: it reads
average and live tensor and writes the average), ``launches`` (chunks of 64 tensors + the prologue; the two report tensors cost
two small torch launches more) and the weight and update count of the last replay.

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
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to import the package from")
    ap.add_argument("--label", default="", help="prefix of the 'config' field of this run's lines")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_cost.py needs an MI355X (a time taken anywhere else says nothing)")
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
        if m not in ("off", "on"):
            raise SystemExit(f"unknown mode {m!r}: off or on")
        torch.manual_seed(1234)
        tr[m] = fst.JointTrainer(fst.JointConfig(L_t=a.length, L_s=a.length), dev)
        if m == "on":
            tr[m].enable_weight_average()
        tr[m].capture(*args, epoch=0)
        snap[m] = tr[m].snapshot()
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
        if m == "on":
            ts = [t for d in tr[m]._ema_avg.values() for t in d.values()]
            line.update(averaged_tensors=len(ts), averaged_mb=round(sum(t.numel() for t in ts) * 4 / 1e6, 3),
                        launches=(len(ts) + 63) // 64 + 1, ema_weight=round(float(rep["ema_weight"][0]), 6),
                        ema_steps=int(rep["ema_steps"][0]))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
