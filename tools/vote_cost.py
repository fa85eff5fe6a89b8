#!/usr/bin/env python3
"""Timing: what one multi-source vote (weights from the train set, vote on the test set) costs with K = 4 classifier pipelines
(``ClassifierTrainer``'s OS_CNN_res + OS_CNN) at the bench configuration (L=512, B=256, 4096 series per set), three ways:

  multi_source_voting      ``voting.multi_source_voting`` over ``DeviceDataset.batches`` — the eager loop the package had before
                           ``VotingEvaluator``: logits concatenated batch by batch, the vote as torch ops, a host read at the end;
  VotingEvaluator.run      ``run(weigh=True)``: both passes eagerly, per round one feed, K forwards and the folds;
  VotingEvaluator.replay   ``replay(weigh=True)``: the same passes as captured graphs.

    python tools/vote_cost.py [--repeats R] [--series N] [--batch B] [--length L] [--members K]

One process, one set of weights.  R rounds; in each, one timed pass per variant, the variants alternating, each between two device
events and after one untimed pass of its own.  Prints one JSON line per variant: ``ms`` is the median of the R passes, ``ms_runs``
the R figures and ``spread_pct`` their (max − min) / median — what a difference between two lines has to exceed; ``host_ms`` is
the host time until the call returned (for ``multi_source_voting`` that includes its wait for the device: it ends in a host read).
The last line is the ``vote_fold`` launch pair alone: ``us`` per call on static logits, with nothing else on the stream."""
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
    ap.add_argument("--members", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vote_cost.py needs an MI355X (a time taken anywhere else says nothing)")
    if a.repeats < 3:
        raise SystemExit("--repeats: at least three windows per line")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import feature_level_style_transfer_for_tsc_amd as fst
    from feature_level_style_transfer_for_tsc_amd import ops, voting
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1000)

    def make_set():
        x = torch.randn(a.series, 1, a.length, generator=gen)
        x = (x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True)
        return fst.DeviceDataset(x, torch.randint(a.classes, (a.series,), generator=gen), dev)

    train, test = make_set(), make_set()
    trainers = []
    for k in range(a.members):
        torch.manual_seed(1234 + k)
        tr = fst.ClassifierTrainer(a.length, 1, a.classes, dev)
        for xb, yb in list(train.batches(a.batch))[:3]:                       # three train steps: running statistics off their initial values
            tr.step(xb, yb)
        trainers.append(tr)
    ve = fst.make_voter(trainers, train, test, a.batch)
    ve.capture()
    models = [(tr.fe, tr.clf) for tr in trainers]

    def parent():
        for fe, clf in models:
            fe.eval(); clf.eval()
        try:
            return voting.multi_source_voting(models, train.batches(a.batch), test.batches(a.batch))
        finally:
            for fe, clf in models:
                fe.train(); clf.train()

    variants = {"multi_source_voting": parent, "VotingEvaluator.run": lambda: ve.run(weigh=True),
                "VotingEvaluator.replay": lambda: ve.replay(weigh=True)}
    acc = parent()[3]
    ve.run(weigh=True)
    got = ve.result()
    if a.series % a.batch == 0 and got["accuracy"] != acc:
        raise SystemExit(f"the variants disagree: multi_source_voting {acc}, VotingEvaluator {got['accuracy']}")
    runs, host = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(a.repeats):
        for k, run in variants.items():
            run()                                                             # untimed: this variant's first pass after another's
            ms, h = timed(run)
            runs[k].append(ms); host[k].append(h)
    ve.check()
    rounds = ve.test_plan.rounds
    for k, r in runs.items():
        ms = statistics.median(r)
        print(json.dumps({"variant": k, "ms": round(ms, 3), "ms_runs": [round(v, 3) for v in r],
                          "spread_pct": round(100 * (max(r) - min(r)) / ms, 2), "host_ms": round(statistics.median(host[k]), 3),
                          "host_ms_runs": [round(v, 3) for v in host[k]], "members": a.members,
                          "rounds_per_pass": [ve.train_plan.rounds, rounds], "runs": a.repeats, "batch": a.batch, "length": a.length,
                          "series": a.series, "accuracy": got["accuracy"], "arithmetic": ops.MATH}), flush=True)
    K, C = a.members, a.classes
    logits = [torch.randn(a.batch, C, device=dev) for _ in range(K)]
    labels = torch.randint(C, (a.batch,), device=dev)
    valid = torch.full((1,), a.batch, dtype=torch.int32, device=dev)
    words = torch.zeros(24 + C * C, dtype=torch.int32, device=dev)
    pred = torch.zeros(a.series, dtype=torch.int64, device=dev)
    scale = torch.ones(K, C, dtype=torch.float64, device=dev)
    call = ops.VoteFoldCall(logits, scale, labels, valid, words[:8], words[8: 8 + K], words[24:].view(C, C), pred)

    def fold_only():
        words.zero_()
        for _ in range(rounds):
            call()

    fold_only()
    alone = [1e3 * timed(fold_only)[0] / rounds for _ in range(a.repeats)]
    us = statistics.median(alone)
    print(json.dumps({"variant": "vote_fold launch pair alone", "us": round(us, 2), "us_runs": [round(v, 2) for v in alone],
                      "spread_pct": round(100 * (max(alone) - min(alone)) / us, 2), "calls_per_run": rounds, "runs": a.repeats,
                      "batch": a.batch, "classes": C, "members": K}), flush=True)


if __name__ == "__main__":
    main()
