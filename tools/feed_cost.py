#!/usr/bin/env python3
"""Timing: what the host side of a replayed step's INPUT costs, and what a device-resident data set (``DeviceDataset`` /
``EpochFeeder``) makes of it, at the bench configuration (L=512, 256 pairs) over a synthetic data set of 4096 series a side:
the replayed "target_pretrain" and "ssl" phases and the joint ``replay``, each fed by ``DeviceLoader`` (host gather into pinned
memory, two host-to-device copies, the copies into the capture's static inputs, a host tensor for the CPC indices and the ratios)
and by the feeder (one launch pair that writes the static inputs), and the feed launch pair alone.

    python tools/feed_cost.py [--repeats R] [--series N] [--batch B] [--length L] [--workloads target_pretrain,ssl,joint]

One trainer with every capture resident.  R rounds; in each, per workload, one timed EPOCH per feed (N // B batches), the two feeds
alternating within the process, each between two device events, each from the trainer's restored snapshot and after one untimed
batch.  Prints one JSON line per workload and feed: ``ms`` is the median of the R runs' ms per batch, ``ms_runs`` the R figures
themselves and ``spread_pct`` their (max − min) / median — what a difference between two lines has to exceed.  The planning and
the upload of an epoch (``begin_epoch``; the loaders' ``randperm``) are inside the timed epoch on both sides.  The last line is the
feed launch pair alone: ``us`` per call into the joint capture's inputs, with nothing else on the stream."""
import argparse
import json
import os
import statistics
import sys

import torch


def series(n, L, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 1, L, generator=gen)
    return (x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True), torch.randint(4, (n,), generator=gen)


def timed(run):
    """ms of ``run()`` between two device events; ``run`` returns the number of batches it served."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    n = run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5, help="timed epochs per workload and feed (at least 3); the median is reported")
    ap.add_argument("--series", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--length", type=int, default=512)
    ap.add_argument("--workloads", default="target_pretrain,ssl,joint")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("feed_cost.py needs an MI355X (a time taken anywhere else says nothing)")
    if a.repeats < 3:
        raise SystemExit("--repeats: at least three windows per line")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import feature_level_style_transfer_for_tsc_amd as fst
    from feature_level_style_transfer_for_tsc_amd import ops
    dev = torch.device("cuda:0")
    (x_t, y_t), (x_s, y_s) = series(a.series, a.length, 1000), series(a.series, a.length, 2000)
    torch.manual_seed(1234)
    tr = fst.JointTrainer(fst.JointConfig(L_t=a.length, L_s=a.length), dev)
    T = tr.m["cpc"].timestep
    gen = torch.Generator().manual_seed(5)
    loaders = [fst.DeviceLoader(x, y, a.batch, dev, generator=gen, drop_last=True) for x, y in ((x_t, y_t), (x_s, y_s))]
    feeder = fst.EpochFeeder(fst.DeviceDataset(x_t, y_t, dev), fst.DeviceDataset(x_s, y_s, dev), batch_size=a.batch,
                             generator=torch.Generator().manual_seed(5), cpc_timestep=T)
    tr.attach_feeder(feeder)
    feeder.begin_epoch()
    first = feeder.peek()[:4]
    workloads = a.workloads.split(",")
    for w in workloads:
        if w == "joint":
            tr.capture(*first, epoch=0)
        else:
            tr.capture_phase(w, *first)
    snap = tr.snapshot()
    torch.manual_seed(4321)
    draw = lambda: (int(torch.randint(max(1, T // 2), (1,))), int(torch.randint(max(1, T // 2), (1,))))

    def by_loader(w):
        n = 0
        for (xt, yt), (xs, ys) in zip(*loaders):
            if w == "joint":
                tr.replay(xt, yt, xs, ys, draw())
            else:
                tr.replay_phase(w, xt, yt, xs, ys, draw())
            n += 1
        return n

    def by_feeder(w):
        n = tr.begin_epoch(w)
        for _ in range(n):
            if w == "joint":
                tr.replay_fed()
            else:
                tr.replay_phase_fed(w)
        return n

    feeds = {"DeviceLoader": by_loader, "EpochFeeder": by_feeder}
    runs = {(w, f): [] for w in workloads for f in feeds}
    for _ in range(a.repeats):
        for w in workloads:
            for f, run in feeds.items():
                tr.restore(snap)
                if w == "joint":                                              # untimed: this workload's first batch after the other's
                    tr.replay(*first, draw())
                else:
                    tr.replay_phase(w, *first, draw())
                runs[(w, f)].append(timed(lambda: run(w)))
    for (w, f), r in runs.items():
        ms = statistics.median(r)
        print(json.dumps({"workload": w, "feed": f, "ms": round(ms, 3), "pairs_per_s": round(1e3 * a.batch / ms, 1),
                          "ms_runs": [round(v, 3) for v in r], "spread_pct": round(100 * (max(r) - min(r)) / ms, 2),
                          "batches_per_run": a.series // a.batch, "runs": a.repeats, "batch": a.batch, "length": a.length,
                          "series": a.series, "arithmetic": ops.MATH}), flush=True)
    bufs = [torch.empty_like(t) for t in first]
    t, r = torch.zeros(2, dtype=torch.int32, device=dev), torch.ones(2, device=dev)

    def feed_only():
        n = feeder.begin_epoch()
        for _ in range(n):
            feeder.feed(*bufs, t=t, r=r)
        return n

    feed_only()
    alone = [1e3 * timed(feed_only) for _ in range(a.repeats)]
    feeder.check()
    us = statistics.median(alone)
    moved = 2 * sum(b.numel() * b.element_size() for b in bufs)
    print(json.dumps({"workload": "feed launch pair alone", "us": round(us, 2), "us_runs": [round(v, 2) for v in alone],
                      "spread_pct": round(100 * (max(alone) - min(alone)) / us, 2), "bytes_moved": moved,
                      "calls_per_run": a.series // a.batch, "runs": a.repeats, "batch": a.batch, "length": a.length}), flush=True)


if __name__ == "__main__":
    main()
