#!/usr/bin/env python3
"""Timing: what one evaluation pass over a resident data set costs, at the bench configuration (L=512, B=256, 4096 series) with
the classifier pipeline (``ClassifierTrainer``'s OS_CNN_res + OS_CNN), three ways:

  eval_accuracy     ``checkpoint.eval_accuracy`` over ``DeviceDataset.batches`` — the eager loop the package had before
                    ``Evaluator``, its host read of the hit count at the end included;
  Evaluator.run     one eager pass: feed, forward and ``eval_fold`` per round, ``eval_finish``, the report's device-side copies;
  Evaluator.replay  the same pass as captured graphs: prepare (round 0 in it) once, batch per later round, ``eval_finish``,
                    the report's copies.

    python tools/eval_cost.py [--repeats R] [--series N] [--batch B] [--length L]

One process, one set of weights.  R rounds; in each, one timed pass per variant, the variants alternating, each between two device
events and after one untimed pass of its own.  Prints one JSON line per variant: ``ms`` is the median of the R passes, ``ms_runs``
the R figures and ``spread_pct`` their (max − min) / median — what a difference between two lines has to exceed; ``host_ms`` is
the host time until the call returned (for ``eval_accuracy`` that includes its wait for the device: it ends in a host read).  The last line
is the ``eval_fold`` launch pair alone: ``us`` per call on a static batch of logits, with nothing else on the stream."""
import argparse
import json
import os
import statistics
import sys
import time

import torch


def timed(run):
    """(ms of ``run()`` between two device events, ms of host time until ``run()`` returned)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    run()
    host = 1e3 * (time.perf_counter() - t0)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5, help="timed passes per variant (at least 3); the median is reported")
    ap.add_argument("--series", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--length", type=int, default=512)
    ap.add_argument("--classes", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_cost.py needs an MI355X (a time taken anywhere else says nothing)")
    if a.repeats < 3:
        raise SystemExit("--repeats: at least three windows per line")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import feature_level_style_transfer_for_tsc_amd as fst
    from feature_level_style_transfer_for_tsc_amd import checkpoint, ops
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1000)
    x = torch.randn(a.series, 1, a.length, generator=gen)
    x = (x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True)
    y = torch.randint(a.classes, (a.series,), generator=gen)
    torch.manual_seed(1234)
    tr = fst.ClassifierTrainer(a.length, 1, a.classes, dev)
    data = fst.DeviceDataset(x, y, dev)
    for xb, yb in list(data.batches(a.batch))[:3]:                            # three train steps: running statistics off their initial values
        tr.step(xb, yb)
    ev = tr.make_evaluator(data, a.batch)
    ev.capture()

    def parent():
        tr.fe.eval(); tr.clf.eval()
        try:
            return checkpoint.eval_accuracy(tr.fe, tr.clf, data.batches(a.batch))
        finally:
            tr.fe.train(); tr.clf.train()

    variants = {"eval_accuracy": parent, "Evaluator.run": ev.run, "Evaluator.replay": ev.replay}
    acc = parent()[0]
    ev.run()
    got = ev.result()
    if a.series % a.batch == 0 and got["accuracy"] != acc:
        raise SystemExit(f"the variants disagree: eval_accuracy {acc}, Evaluator {got['accuracy']}")
    runs, host = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(a.repeats):
        for k, run in variants.items():
            run()                                                             # untimed: this variant's first pass after another's
            ms, h = timed(run)
            runs[k].append(ms); host[k].append(h)
    ev.check()
    rounds = ev.rounds
    for k, r in runs.items():
        ms = statistics.median(r)
        print(json.dumps({"variant": k, "ms": round(ms, 3), "series_per_s": round(1e3 * a.series / ms, 1),
                          "ms_runs": [round(v, 3) for v in r], "spread_pct": round(100 * (max(r) - min(r)) / ms, 2),
                          "host_ms": round(statistics.median(host[k]), 3), "host_ms_runs": [round(v, 3) for v in host[k]],
                          "rounds_per_pass": rounds, "runs": a.repeats, "batch": a.batch, "length": a.length, "series": a.series,
                          "accuracy": got["accuracy"], "arithmetic": ops.MATH}), flush=True)
    logits = torch.randn(a.batch, a.classes, device=dev)
    labels = torch.randint(a.classes, (a.batch,), device=dev)
    valid = torch.full((1,), a.batch, dtype=torch.int32, device=dev)
    words = torch.zeros(10 + a.classes * a.classes, dtype=torch.int32, device=dev)
    pred = torch.zeros(a.series, dtype=torch.int64, device=dev)
    call = ops.EvalFoldCall(logits, labels, valid, words[:8], words[8:10].view(torch.float64), words[10:].view(a.classes, a.classes), pred)

    def fold_only():
        words.zero_()
        for _ in range(rounds):
            call()

    fold_only()
    alone = [1e3 * timed(fold_only)[0] / rounds for _ in range(a.repeats)]
    us = statistics.median(alone)
    print(json.dumps({"variant": "eval_fold launch pair alone", "us": round(us, 2), "us_runs": [round(v, 2) for v in alone],
                      "spread_pct": round(100 * (max(alone) - min(alone)) / us, 2), "calls_per_run": rounds, "runs": a.repeats,
                      "batch": a.batch, "classes": a.classes}), flush=True)


if __name__ == "__main__":
    main()
