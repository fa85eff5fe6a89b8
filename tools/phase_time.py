#!/usr/bin/env python3
"""Timing: one batch of each pre-training phase at the bench configuration (L=512, 256 pairs), eager ``phase_step`` against the
captured ``replay_phase``.

    python tools/phase_time.py [--steps N] [--repeats R] [--batch B] [--length L] [--phases a,b,...]

Per phase: capture, then R rounds that alternate a window of N eager steps and a window of N replays, each window timed with
device events around it (the second event is recorded after the last step and waited for), each starting from the same
restored snapshot and after one untimed step of its own kind.  Prints one JSON line per phase: ``eager_ms`` and ``replay_ms``
are the medians of the R windows' ms per step, ``pairs_per_s`` is the batch over ``replay_ms``; the R figures themselves are in
``eager_ms_runs`` / ``replay_ms_runs`` (their spread is what a difference has to exceed), and ``arithmetic`` says which product
arithmetic ran (``FST_MATH``).  Inputs are seeded and resident in HBM; CPC start indices are drawn per step on the host, as a
training loop draws them."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import feature_level_style_transfer_for_tsc_amd as fst  # noqa: E402
from feature_level_style_transfer_for_tsc_amd import ops  # noqa: E402


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
    ap.add_argument("--steps", type=int, default=20, help="steps per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="windows per mode; the median is reported")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--length", type=int, default=512)
    ap.add_argument("--phases", default=",".join(fst.JointTrainer.PHASES))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("phase_time.py needs an MI355X (a time taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    tr = fst.JointTrainer(fst.JointConfig(L_t=a.length, L_s=a.length), dev)
    (x_t, y_t), (x_s, y_s) = batch(a.batch, a.length, 1000, dev), batch(a.batch, a.length, 2000, dev)
    args = (x_t, y_t, x_s, y_s)
    T_half = max(1, (a.length // 2) // 2)
    torch.manual_seed(4321)
    draw = lambda: (int(torch.randint(T_half, (1,))), int(torch.randint(T_half, (1,))))
    for phase in a.phases.split(","):
        tr.capture_phase(phase, *args)
        snap = tr.snapshot()
        modes = {"eager": lambda: tr.phase_step(phase, *args, t_samples=draw()),
                 "replay": lambda: tr.replay_phase(phase, *args, t_samples=draw())}
        runs = {"eager": [], "replay": []}
        for _ in range(a.repeats):
            for name, step in modes.items():
                tr.restore(snap)
                step()                                                       # untimed: this mode's first step after the other's
                runs[name].append(window(step, a.steps))
        finite = all(bool(torch.isfinite(v)) for v in tr.replay_phase(phase, *args, t_samples=draw()).values())
        tr.restore(snap)
        tr.release_phase(phase)
        eager_ms, replay_ms = statistics.median(runs["eager"]), statistics.median(runs["replay"])
        print(json.dumps({"phase": phase, "eager_ms": round(eager_ms, 3), "replay_ms": round(replay_ms, 3),
                          "pairs_per_s": round(1e3 * a.batch / replay_ms, 1), "eager_pairs_per_s": round(1e3 * a.batch / eager_ms, 1),
                          "eager_ms_runs": [round(v, 3) for v in runs["eager"]], "replay_ms_runs": [round(v, 3) for v in runs["replay"]],
                          "steps_per_window": a.steps, "windows": a.repeats, "batch": a.batch, "length": a.length,
                          "arithmetic": ops.MATH, "losses_finite": finite}), flush=True)


if __name__ == "__main__":
    main()
