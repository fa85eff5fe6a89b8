#!/usr/bin/env python3
"""Timing: what the transfer monitor (``JointTrainer.enable_transfer_monitor``) costs, at the bench configuration (L=512, 256 pairs).

    python tools/transfer_monitor_cost.py [--steps N] [--repeats R] [--batch B] [--length L] [--parts joint,launch] [--out FILE]

joint   (a) the captured joint step with the monitor off and on: one trainer per mode, built from the same seed, each with its
        capture resident; R rounds that alternate one window of N replays per mode, each window timed with device events around
        it, each starting from the trainer's restored snapshot and after one untimed replay.
launch  (b) the monitor's launch set alone on the feature-space triple (three fp32 [B, 225 L] sets, R = 3 B rows): ``mmd_centre`` +
        ``mmd_gram`` + ``mmd_fold`` for the two pairs; and the Gram launch pair alone;
        (c) what a user could write without it: the centre by ``mean``, three centred copies, the six 256-row blocks of the Gram as
        six ``ops.nt_gemm`` calls, the blocks put together and an fp64 epilogue in torch for the two pairs (no host read either);
        and the six ``nt_gemm`` calls alone, on copies centred beforehand.
        Windows of N calls alternate between the four, R rounds.

One JSON line per configuration: ``ms`` is the median of the R windows' ms per call, ``ms_runs`` the R figures themselves and
``spread_pct`` their (max − min) / median — what a difference between two lines has to exceed.  ``--out FILE`` appends the lines
to FILE as well.  Lines are comparable when they ran in one session on one box."""
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


def line_of(config, runs, n, extra):
    ms = statistics.median(runs)
    return {"config": config, "ms": round(ms, 4), "ms_runs": [round(v, 4) for v in runs], "spread_pct": round(100 * (max(runs) - min(runs)) / ms, 2),
            "calls_per_window": n, "windows": len(runs), **extra}


def torch_epilogue(G, n, m, kernels=5, mul=2.0):
    """``monitor.mmd2_from_gram`` without its host read: fp64 torch on the device, for a Gram of x (n rows) then y (m rows)."""
    G = G.double()
    g = G.diagonal()
    d2 = (g[:, None] + g[None, :] - 2.0 * G).clamp(min=0.0)
    d2.fill_diagonal_(0.0)
    N = n + m
    xx, yy, xy = d2[:n, :n].sum(), d2[n:, n:].sum(), d2[:n, n:].sum()
    bw = (xx + yy + 2.0 * xy) / (N * N - N)
    safe = torch.where(bw == 0, torch.ones_like(bw), bw)
    k = torch.zeros_like(d2)
    for q in range(kernels):
        k += torch.exp(-d2 / (safe * mul ** (q - kernels // 2)))
    k.fill_diagonal_(0.0)
    mmd2 = k[:n, :n].sum() / (n * (n - 1)) + k[n:, n:].sum() / (m * (m - 1)) - 2.0 * k[:n, n:].sum() / (n * m)
    return torch.stack([torch.where(bw == 0, torch.zeros_like(mmd2), mmd2), bw, xx / (n * (n - 1)), yy / (m * (m - 1)), xy / (n * m)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="windows per configuration; the median is reported")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--length", type=int, default=512)
    ap.add_argument("--parts", default="joint,launch")
    ap.add_argument("--out", default="", help="append the JSON lines to this file too")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transfer_monitor_cost.py needs an MI355X (a time taken anywhere else says nothing)")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import feature_level_style_transfer_for_tsc_amd as fst
    from feature_level_style_transfer_for_tsc_amd import monitor, ops
    dev = torch.device("cuda:0")
    B, L = a.batch, a.length
    common = {"batch": B, "length": L, "arithmetic": ops.MATH}

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")

    parts = a.parts.split(",")
    if "launch" in parts:
        D = 225 * L
        gen = torch.Generator(device=dev).manual_seed(7)
        xs = [torch.relu(torch.randn(B, D, generator=gen, device=dev) + 0.5 + 0.05 * i) for i in range(3)]
        rows, pairs = [B] * 3, [(0, 1), (0, 2)]
        out, sums = torch.empty(2, 5, dtype=torch.float64, device=dev), torch.zeros(2, 5, dtype=torch.float64, device=dev)
        count, bad = torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        centre = ops.mmd_centre(xs[0])
        centred = [x - centre for x in xs]

        def launch_set():
            ops.mmd_fold(ops.mmd_gram(xs, ops.mmd_centre(xs[0])), rows, pairs, 5, 2.0, out, sums, count, bad)
            return out

        def gram_only():
            return ops.mmd_gram(xs, centre)

        def six_gemms(zs):
            G = torch.empty(3 * B, 3 * B, device=dev)
            for i in range(3):
                for j in range(i, 3):
                    blk = ops.nt_gemm(zs[i], zs[j])
                    G[B * i: B * (i + 1), B * j: B * (j + 1)] = blk
                    if i != j:
                        G[B * j: B * (j + 1), B * i: B * (i + 1)] = blk.t()
            return G

        def composed():
            c = xs[0].mean(dim=0)
            G = six_gemms([x - c for x in xs])
            idx = torch.cat([torch.arange(B, device=dev), torch.arange(2 * B, 3 * B, device=dev)])
            return torch.stack([torch_epilogue(G[: 2 * B, : 2 * B], B, B), torch_epilogue(G[idx][:, idx], B, B)])

        configs = {"(b) launch set: mmd_centre + mmd_gram + mmd_fold, two pairs": launch_set, "(b') mmd_gram alone (two launches)": gram_only,
                   "(c) composed: mean, centred copies, six nt_gemm, fp64 torch epilogue, two pairs": composed,
                   "(c') six nt_gemm alone, on copies centred beforehand": lambda: six_gemms(centred)}
        got, want = launch_set().clone(), composed()
        agree = float(((got - want).abs() / want.abs().clamp(min=1e-300)).max())
        runs = {k: [] for k in configs}
        for fn in configs.values():
            fn()                                                              # untimed: allocations, first launches
        for _ in range(a.repeats):
            for k, fn in configs.items():
                fn()
                runs[k].append(window(fn, a.steps))
        for k in configs:
            emit(line_of(k, runs[k], a.steps, {**common, "rows": 3 * B, "columns": D, "slabs": ops.mmd_gram_splits(3 * B, D),
                                               "mmd2": [round(v, 6) for v in got[:, 0].tolist()], "launch_set_vs_composed_max_rel": agree}))
        del xs, centred

    if "joint" in parts:
        (x_t, y_t), (x_s, y_s) = batch(B, L, 1000, dev), batch(B, L, 2000, dev)
        args = (x_t, y_t, x_s, y_s)
        T_half = max(1, (L // 2) // 2)
        draw = lambda: (int(torch.randint(T_half, (1,))), int(torch.randint(T_half, (1,))))
        tr, snap = {}, {}
        for m in ("off", "on"):
            torch.manual_seed(1234)
            tr[m] = fst.JointTrainer(fst.JointConfig(L_t=L, L_s=L), dev)
            if m == "on":
                tr[m].enable_transfer_monitor()
            tr[m].capture(*args, epoch=0)
            snap[m] = tr[m].snapshot()
        torch.manual_seed(4321)
        replay = lambda t: t.replay(*args, draw())
        runs = {m: [] for m in tr}
        for _ in range(a.repeats):
            for m in tr:
                tr[m].restore(snap[m])
                replay(tr[m])                                                 # untimed: this trainer's first replay after the other's
                runs[m].append(window(lambda: replay(tr[m]), a.steps))
        for m in tr:
            rep = replay(tr[m])
            extra = {**common, "workload": "joint", "pairs_per_s": round(1e3 * B / statistics.median(runs[m]), 1),
                     "losses_finite": all(bool(torch.isfinite(v).all()) for k, v in rep.items() if v.dtype.is_floating_point)}
            if m == "on":
                extra["transfer"] = {p: {f: float(v) for f, v in zip(monitor.FIELDS, row)} for p, row in zip(monitor.PAIRS, rep["transfer"].tolist())}
            emit(line_of(f"(a) joint replay, monitor {m}", runs[m], a.steps, extra))


if __name__ == "__main__":
    main()
