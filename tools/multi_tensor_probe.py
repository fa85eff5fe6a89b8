#!/usr/bin/env python3
"""The thirteen multi-tensor entry points (csrc/optim.hip, csrc/guard.hip) through the raw C ABI: what they write, and what a call costs.

    python tools/multi_tensor_probe.py --digest            one line "<entry> <case> <sha256>" per entry and case
    python tools/multi_tensor_probe.py --time [--calls N] [--windows W] [--label NAME]     one JSON line per entry

The library is the one ``_lib`` loads: the tree's, or the one ``FST_HIP_LIB`` names.  Two libraries are compared by running this tool
in a fresh process per library, one after the other on one box, and comparing the lines.

``--digest``: seeded inputs; per case 65 or 130 tensors of 1, 3, 1023, 1025 and 70 001 elements in turn, cut out of one arena per role
(parameters, gradients, moments, ...) with eight words of guard band around each, every tensor starting 0, 4, 8 or 12 bytes past a
16-byte boundary (the case's offset).  Guarded entries run with the verdict word 0 and 1, the optimisers with their rates by value and
by device address, the accumulation on a window's opening, middle and closing call and with k = 1.  The sha256 of a case covers every
arena (guard bands included) and every word block the entry may write, as they are after the call.

``--time``: the joint trainer's own parameter list (tensor count and sizes; each tensor 256-byte aligned), W windows of N calls per
entry between two device events after one untimed call; ``us`` is the median of the windows' us per call, ``us_runs`` the W figures.
The time of a call includes its host side (the argument fills and the launches of its chunks)."""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feature_level_style_transfer_for_tsc_amd import _lib                     # noqa: E402

SIZES = (1, 3, 1023, 1025, 70001)
GUARD = 8                                                                      # words of guard band on either side of a tensor
GROUPS = 32


def ptrs(values):
    return (ctypes.c_void_p * len(values))(*values)


def i64s(values):
    return (ctypes.c_int64 * len(values))(*values)


def i32s(values):
    return (ctypes.c_int32 * len(values))(*values)


class Arena:
    """Tensors cut out of one flat fp32 device buffer; ``starts[i]`` is tensor i's first element."""

    def __init__(self, sizes, offset_bytes, seed, dev, align_words=4, kind="normal"):
        self.sizes, self.starts, cur = list(sizes), [], 0
        for n in sizes:
            cur = (cur + align_words - 1) // align_words * align_words + GUARD + offset_bytes // 4
            self.starts.append(cur)
            cur += n
        gen = torch.Generator().manual_seed(seed)
        host = torch.randn(cur + GUARD, generator=gen)
        if kind == "positive":
            host = host.abs()
        self.buf = host.to(dev)

    def addr(self):
        return [self.buf.data_ptr() + 4 * s for s in self.starts]

    def poke(self, i, k, value):
        self.buf[self.starts[i] + k] = value

    def bytes(self):
        return self.buf.cpu().numpy().tobytes()


def words(values, dtype, dev):
    return torch.tensor(values, dtype=dtype, device=dev)


def digest(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p.bytes() if isinstance(p, Arena) else p.cpu().numpy().tobytes())
    return h.hexdigest()


def call(lib, name, *args):
    _lib.check(getattr(lib, name)(*args, _lib.stream_ptr()), name)
    torch.cuda.synchronize()


def digest_cases(lib, dev):
    for n in (65, 130):
        sizes = [SIZES[i % len(SIZES)] for i in range(n)]
        numel, groups = i64s(sizes), i32s([(7 * i) % GROUPS for i in range(n)])
        for off in (0, 4, 8, 12):
            tag = f"n={n} off={off}"
            mk = lambda seed, kind="normal": Arena(sizes, off, 1000 * n + 10 * off + seed, dev, kind=kind)
            rates_host = [1e-3 * (1 + i % 7) for i in range(n)]
            rates_val = (ctypes.c_float * n)(*rates_host)
            rates_dev = words([1e-3 * (1 + k) for k in range(7)], torch.float32, dev)
            rates_addr = ptrs([rates_dev.data_ptr() + 4 * (i % 7) for i in range(n)])
            step = words([3.0], torch.float32, dev)
            lr_adam = words([2e-3], torch.float32, dev)
            verdicts = {v: words([v], torch.int32, dev) for v in (0, 1)}

            # ---- RMSprop and Adam: plain, rates on the device, and behind the verdict word in both rate forms
            for form in ("val", "dev"):
                for verdict in (None, 0, 1):
                    p, g, v = mk(1), mk(2), mk(3, "positive")
                    head = (ptrs(p.addr()), ptrs(g.addr()), ptrs(v.addr()), numel)
                    if verdict is None:
                        name = "fst_rmsprop_multi" if form == "val" else "fst_rmsprop_multi_dev"
                        call(lib, name, *head, rates_val if form == "val" else rates_addr, n, 0.99, 1e-8)
                    else:
                        name = "fst_rmsprop_multi_guard"
                        call(lib, name, *head, rates_val if form == "val" else None, rates_addr if form == "dev" else None, n, 0.99, 1e-8,
                             verdicts[verdict].data_ptr())
                    yield name, f"{tag} rate={form} verdict={verdict}", digest(p, g, v)
                    p, g, m, v = mk(1), mk(2), mk(4), mk(3, "positive")
                    head = (ptrs(p.addr()), ptrs(g.addr()), ptrs(m.addr()), ptrs(v.addr()), numel, n, step.data_ptr())
                    if verdict is None and form == "val":
                        name = "fst_adam_multi"
                        call(lib, name, *head, 2e-3, 0.9, 0.999, 1e-8)
                    elif verdict is None:
                        name = "fst_adam_multi_dev"
                        call(lib, name, *head, lr_adam.data_ptr(), 0.9, 0.999, 1e-8)
                    else:
                        name = "fst_adam_multi_guard"
                        call(lib, name, *head, 2e-3, lr_adam.data_ptr() if form == "dev" else None, 0.9, 0.999, 1e-8,
                             verdicts[verdict].data_ptr())
                    yield name, f"{tag} rate={form} verdict={verdict}", digest(p, g, m, v, step)

            # ---- the scan for non-finite values: NaN and inf at the head, in the middle and at the tail of some tensors
            x = mk(5)
            for i in range(0, n, 3):
                x.poke(i, 0, float("nan")); x.poke(i, sizes[i] - 1, float("inf")); x.poke(i, sizes[i] // 2, float("-inf"))
            n_slots = int(lib.fst_nonfinite_slots(n))
            slots = torch.full((n_slots + GUARD,), -7, dtype=torch.int32, device=dev)
            counts, verdict, skipped = (torch.full((k,), -7, dtype=torch.int32, device=dev) for k in (GROUPS, 1, 1))
            ok = words([-7.0], torch.float32, dev)
            call(lib, "fst_nonfinite_multi", ptrs(x.addr()), numel, groups, n, 0x0000ffff, slots.data_ptr(), n_slots, counts.data_ptr(),
                 verdict.data_ptr(), ok.data_ptr(), skipped.data_ptr())
            yield "fst_nonfinite_multi", tag, digest(x, slots, counts, verdict, ok, skipped)

            # ---- the copy: unconditional, and behind the verdict word either way round
            for verdict, when in ((None, 1), (0, 0), (0, 1), (1, 0), (1, 1)):
                d, s = mk(6), mk(7)
                call(lib, "fst_guard_copy_multi", ptrs(d.addr()), ptrs(s.addr()), numel, n,
                     None if verdict is None else verdicts[verdict].data_ptr(), when)
                yield "fst_guard_copy_multi", f"{tag} verdict={verdict} when={when}", digest(d, s)

            # ---- norms and clipping factors, and the scale by them
            x = mk(8)
            fslots = torch.full((n_slots + GUARD,), -7.0, dtype=torch.float32, device=dev)
            limits = words([0.5 * (1 + k % 5) if k % 3 else float("inf") for k in range(GROUPS)] + [20.0], torch.float32, dev)
            norms, coef = torch.full((GROUPS + 1,), -7.0, device=dev), torch.full((GROUPS,), -7.0, device=dev)
            call(lib, "fst_sumsq_multi", ptrs(x.addr()), numel, groups, n, fslots.data_ptr(), n_slots, limits.data_ptr(), norms.data_ptr(),
                 coef.data_ptr())
            yield "fst_sumsq_multi", tag, digest(x, fslots, norms, coef)
            call(lib, "fst_scale_multi", ptrs(x.addr()), numel, groups, n, coef.data_ptr())
            yield "fst_scale_multi", tag, digest(x, coef)

            # ---- weight averaging: no guard, and behind the verdict word
            for verdict in (None, 0, 1):
                avg, live = mk(9), mk(10)
                state = torch.zeros(2 + 2 * GROUPS, dtype=torch.int32, device=dev)
                state[0:1].view(torch.float32).fill_(0.999); state[1] = 1
                state[2:2 + GROUPS] = torch.arange(GROUPS, dtype=torch.int32, device=dev) * 5
                call(lib, "fst_ema_multi", ptrs(avg.addr()), ptrs(live.addr()), numel, groups, n, 0x55aa55aa, state.data_ptr(),
                     None if verdict is None else verdicts[verdict].data_ptr())
                yield "fst_ema_multi", f"{tag} verdict={verdict}", digest(avg, live, state)

            a, b = mk(11), mk(12)
            call(lib, "fst_swap_multi", ptrs(a.addr()), ptrs(b.addr()), numel, n)
            yield "fst_swap_multi", tag, digest(a, b)

            # ---- accumulation: a window of three on its opening, middle and closing call, and a window of one
            for k, j in ((3, 0), (3, 1), (3, 2), (1, 0)):
                acc, g = mk(13), mk(14)
                state = torch.zeros(8, dtype=torch.int32, device=dev)
                state[0], state[1] = k, j
                state[2:3].view(torch.float32).fill_(1.0 / k)
                call(lib, "fst_accum_multi", ptrs(acc.addr()), ptrs(g.addr()), numel, n, state.data_ptr(), 1)
                yield "fst_accum_multi", f"{tag} k={k} j={j}", digest(acc, g, state)


def trainer_sizes():
    import feature_level_style_transfer_for_tsc_amd as fst
    torch.manual_seed(1234)
    tr = fst.JointTrainer(fst.JointConfig(L_t=512, L_s=512), torch.device("cuda:0"))
    return [p.numel() for p in tr.parameters() if p.numel() > 0]


def time_entries(lib, dev, calls, windows):
    sizes = trainer_sizes()
    n = len(sizes)
    numel, groups = i64s(sizes), i32s([i * GROUPS // n for i in range(n)])
    mk = lambda seed, kind="normal": Arena(sizes, 0, seed, dev, align_words=64, kind=kind)
    p, g, m, v, q = mk(1), mk(2), mk(4), mk(3, "positive"), mk(5)
    P, G, M, V, Q = (ptrs(a.addr()) for a in (p, g, m, v, q))
    rates_val = (ctypes.c_float * n)(*[1e-5] * n)
    rates_dev = words([1e-5] * 10, torch.float32, dev)
    rates_addr = ptrs([rates_dev.data_ptr() + 4 * (i % 10) for i in range(n)])
    step, lr_adam, zero = words([10.0], torch.float32, dev), words([1e-5], torch.float32, dev), words([0], torch.int32, dev)
    n_slots = int(lib.fst_nonfinite_slots(n))
    slots, fslots = torch.zeros(n_slots, dtype=torch.int32, device=dev), torch.zeros(n_slots, device=dev)
    counts, verdict, skipped, ok = torch.zeros(GROUPS, dtype=torch.int32, device=dev), words([0], torch.int32, dev), words([0], torch.int32, dev), words([1.0], torch.float32, dev)
    limits, norms, coef = torch.full((GROUPS + 1,), float("inf"), device=dev), torch.zeros(GROUPS + 1, device=dev), torch.full((GROUPS,), 0.9999, device=dev)
    own_coef = torch.zeros(GROUPS, device=dev)                                # the scan's own factors; the scale keeps its 0.9999
    ema = torch.zeros(2 + 2 * GROUPS, dtype=torch.int32, device=dev)
    ema[0:1].view(torch.float32).fill_(0.999)
    acc = torch.zeros(8, dtype=torch.int32, device=dev)
    acc[0] = 4
    acc[2:3].view(torch.float32).fill_(0.25)
    s = _lib.stream_ptr()
    entries = {
        "fst_rmsprop_multi": lambda: lib.fst_rmsprop_multi(P, G, V, numel, rates_val, n, 0.99, 1e-8, s),
        "fst_rmsprop_multi_dev": lambda: lib.fst_rmsprop_multi_dev(P, G, V, numel, rates_addr, n, 0.99, 1e-8, s),
        "fst_rmsprop_multi_guard val": lambda: lib.fst_rmsprop_multi_guard(P, G, V, numel, rates_val, None, n, 0.99, 1e-8, zero.data_ptr(), s),
        "fst_rmsprop_multi_guard dev": lambda: lib.fst_rmsprop_multi_guard(P, G, V, numel, None, rates_addr, n, 0.99, 1e-8, zero.data_ptr(), s),
        "fst_adam_multi": lambda: lib.fst_adam_multi(P, G, M, V, numel, n, step.data_ptr(), 1e-5, 0.9, 0.999, 1e-8, s),
        "fst_adam_multi_dev": lambda: lib.fst_adam_multi_dev(P, G, M, V, numel, n, step.data_ptr(), lr_adam.data_ptr(), 0.9, 0.999, 1e-8, s),
        "fst_adam_multi_guard val": lambda: lib.fst_adam_multi_guard(P, G, M, V, numel, n, step.data_ptr(), 1e-5, None, 0.9, 0.999, 1e-8, zero.data_ptr(), s),
        "fst_adam_multi_guard dev": lambda: lib.fst_adam_multi_guard(P, G, M, V, numel, n, step.data_ptr(), 0.0, lr_adam.data_ptr(), 0.9, 0.999, 1e-8, zero.data_ptr(), s),
        "fst_nonfinite_multi": lambda: lib.fst_nonfinite_multi(G, numel, groups, n, -1, slots.data_ptr(), n_slots, counts.data_ptr(), verdict.data_ptr(), ok.data_ptr(), skipped.data_ptr(), s),
        "fst_guard_copy_multi": lambda: lib.fst_guard_copy_multi(Q, P, numel, n, None, 1, s),
        "fst_sumsq_multi": lambda: lib.fst_sumsq_multi(G, numel, groups, n, fslots.data_ptr(), n_slots, limits.data_ptr(), norms.data_ptr(), own_coef.data_ptr(), s),
        "fst_scale_multi": lambda: lib.fst_scale_multi(Q, numel, groups, n, coef.data_ptr(), s),
        "fst_ema_multi": lambda: lib.fst_ema_multi(Q, P, numel, groups, n, -1, ema.data_ptr(), None, s),
        "fst_swap_multi": lambda: lib.fst_swap_multi(Q, M, numel, n, s),
        "fst_accum_multi": lambda: lib.fst_accum_multi(Q, G, numel, n, acc.data_ptr(), 1, s),
    }
    for name, fn in entries.items():
        _lib.check(fn(), name)
        runs = []
        for _ in range(windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                rc = fn()
            e1.record()
            e1.synchronize()
            _lib.check(rc, name)
            runs.append(1e3 * e0.elapsed_time(e1) / calls)
        yield {"entry": name, "us": round(statistics.median(runs), 2), "us_runs": [round(r, 2) for r in runs], "tensors": n,
               "elements": sum(sizes), "launches": (n + 63) // 64, "calls_per_window": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--digest", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=5, help="windows per entry; the median is reported")
    ap.add_argument("--label", default="", help="a 'config' field for this run's lines")
    a = ap.parse_args()
    if a.digest == a.time:
        raise SystemExit("one of --digest and --time")
    if not torch.cuda.is_available():
        raise SystemExit("multi_tensor_probe.py needs an MI355X")
    dev, lib = torch.device("cuda:0"), _lib.load()
    if a.digest:
        for name, case, sha in digest_cases(lib, dev):
            print(name, case.replace(" ", ","), sha, flush=True)
        return
    for line in time_entries(lib, dev, a.calls, a.windows):
        if a.label:
            line["config"] = a.label
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
