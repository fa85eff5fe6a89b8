#!/usr/bin/env python3
"""The seven weight-image entry points of the fused WN kernels (csrc/wn_fused.hip) through the raw C ABI: what they write, and what a
call costs.

    python tools/wn_pack_probe.py --digest            one line "<entry> <case> <sha256>" per entry and case
    python tools/wn_pack_probe.py --time [--calls N] [--windows W] [--label NAME]     one JSON line per entry

The library is the one ``_lib`` loads: the tree's, or the one ``FST_HIP_LIB`` names.  Two libraries are compared by running this tool
in a fresh process per library, one after the other on one box, and comparing the lines.

``--digest``: seeded randn weights; the shapes of tests/test_gpu_wn_images.py (forward (n, h) x last, backward n x last x acc_order,
data gradient (n, h), projected n = 17 with h2 = 6 and 64 over three layers, stacks of 1, 2 and 10 layers) and the workload's own
n = 120, h = 25, eight layers (h2 = 50).  Every image lies between two bands of 64 canary words; the sha256 of a case covers the whole
buffers of all its layers, bands included, as they are after the call.

``--time``: the workload's shape; per entry W windows of N calls between two device events after one untimed call; ``us`` is the
median of the windows' us per call, ``us_runs`` the W figures.  A per-layer entry packs one layer (layer 0, not the last) per call, a
stack entry all eight."""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feature_level_style_transfer_for_tsc_amd import _lib                     # noqa: E402
from feature_level_style_transfer_for_tsc_amd.ops import _ptr_table as tbl    # noqa: E402

BAND, CANARY = 64, 0x4B1D4B1D
WORKLOAD = dict(n=120, h=25, nl=8)                                             # WaveGlow(3, 50, 120): WN(h = 25, eight layers, n = 120)


def weights(n, h, lasts, seed, dev):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g).to(dev)
    return [(r(2 * n, n, 3), r(2 * n, h, 1), r(2 * n), r(2 * n), r(n if last else 2 * n, n, 1), r(n if last else 2 * n)) for last in lasts]


def image(nbytes, dev):
    buf = torch.full((nbytes // 4 + 2 * BAND,), CANARY, device=dev, dtype=torch.int32)
    return buf[BAND: BAND + nbytes // 4], buf


def sha(images):
    h = hashlib.sha256()
    for _, buf in images:
        h.update(buf.cpu().numpy().tobytes())
    return h.hexdigest()


def call(lib, name, *args):
    _lib.check(getattr(lib, name)(*args, _lib.stream_ptr()), name)
    torch.cuda.synchronize()


def col(W, j):
    return tbl([l[j] for l in W])


def digest_fwd(lib, dev, n, h, lasts, seed):
    W, nb = weights(n, h, lasts, seed, dev), lib.fst_wn_image_bytes(n, h)
    for i, l in enumerate(W):
        img = image(nb, dev)
        call(lib, "fst_wn_pack", *[t.data_ptr() for t in l], n, h, 3, int(lasts[i]), img[0].data_ptr(), nb)
        yield "fst_wn_pack", f"n={n} h={h} nl={len(W)} layer={i} last={int(lasts[i])} seed={seed}", sha([img])
    imgs = [image(nb, dev) for _ in W]
    call(lib, "fst_wn_pack_stack", *[col(W, j) for j in range(6)], len(W), n, h, 3, tbl([m[0] for m in imgs]), nb)
    yield "fst_wn_pack_stack", f"n={n} h={h} nl={len(W)} seed={seed}", sha(imgs)


def digest_bwd(lib, dev, n, lasts, acc_order, seed):
    W = weights(n, 1, lasts, seed, dev)
    sizes = [lib.fst_wn_bwd_image_bytes(n, int(last)) for last in lasts]
    for i, l in enumerate(W):
        img = image(sizes[i], dev)
        call(lib, "fst_wn_pack_bwd", l[4].data_ptr(), n, int(lasts[i]), acc_order, img[0].data_ptr(), sizes[i])
        yield "fst_wn_pack_bwd", f"n={n} nl={len(W)} layer={i} last={int(lasts[i])} acc_order={acc_order} seed={seed}", sha([img])
    imgs = [image(s, dev) for s in sizes]
    call(lib, "fst_wn_pack_bwd_stack", col(W, 4), len(W), n, acc_order, tbl([m[0] for m in imgs]), lib.fst_wn_bwd_image_bytes(n, 0))
    yield "fst_wn_pack_bwd_stack", f"n={n} nl={len(W)} acc_order={acc_order} seed={seed}", sha(imgs)


def digest_dgrad(lib, dev, n, h, nl, seed):
    W, nb = weights(n, h, [False] * nl, seed, dev), lib.fst_wn_dgrad_image_bytes(n)
    for i, l in enumerate(W):
        img = image(nb, dev)
        call(lib, "fst_wn_pack_dgrad", l[0].data_ptr(), l[1].data_ptr(), n, h, 3, img[0].data_ptr(), nb)
        yield "fst_wn_pack_dgrad", f"n={n} h={h} nl={nl} layer={i} seed={seed}", sha([img])
    imgs = [image(nb, dev) for _ in W]
    call(lib, "fst_wn_pack_dgrad_stack", col(W, 0), col(W, 1), nl, n, h, 3, tbl([m[0] for m in imgs]), nb)
    yield "fst_wn_pack_dgrad_stack", f"n={n} h={h} nl={nl} seed={seed}", sha(imgs)


def digest_proj(lib, dev, n, h2, nl, seed):
    W = weights(n, 1, [i == nl - 1 for i in range(nl)], seed, dev)
    end_w = torch.randn(h2, n, generator=torch.Generator().manual_seed(seed + 1)).to(dev)
    sizes = [lib.fst_wn_bwd_proj_image_bytes(n, h2, int(i == nl - 1)) for i in range(nl)]
    imgs = [image(s, dev) for s in sizes]
    call(lib, "fst_wn_pack_bwd_proj_stack", col(W, 4), end_w.data_ptr(), nl, n, h2, tbl([m[0] for m in imgs]), sizes[0])
    yield "fst_wn_pack_bwd_proj_stack", f"n={n} h2={h2} nl={nl} seed={seed}", sha(imgs)


def digest_cases(lib, dev):
    top = lambda nl: [i == nl - 1 for i in range(nl)]
    for n, h in ((1, 1), (15, 15), (16, 16), (17, 31), (127, 25)):
        for nl in (1, 2):                                                     # a stack of one: layer 0 is the last; of two: it is not
            yield from digest_fwd(lib, dev, n, h, top(nl), 1000 * n + 10 * h + nl)
    for n in (1, 16, 17, 128):
        for nl in (1, 2):
            for acc_order in (0, 1):
                yield from digest_bwd(lib, dev, n, top(nl), acc_order, 100 * n + 2 * nl + acc_order)
    for n, h in ((1, 1), (8, 32), (17, 5), (128, 32)):
        yield from digest_dgrad(lib, dev, n, h, 2, 1000 * n + h)
    for h2 in (6, 64):
        yield from digest_proj(lib, dev, 17, h2, 3, 7 + h2)
    for nl in (1, 2, 10):
        yield from digest_fwd(lib, dev, 17, 16, top(nl), 50 + nl)
        for acc_order in (0, 1):
            yield from digest_bwd(lib, dev, 17, top(nl), acc_order, 70 + nl)
        yield from digest_dgrad(lib, dev, 17, 5, nl, 60 + nl)
    n, h, nl = WORKLOAD["n"], WORKLOAD["h"], WORKLOAD["nl"]
    yield from digest_fwd(lib, dev, n, h, top(nl), 1)
    for acc_order in (0, 1):
        yield from digest_bwd(lib, dev, n, top(nl), acc_order, 2)
    yield from digest_dgrad(lib, dev, n, h, nl, 3)
    yield from digest_proj(lib, dev, n, 2 * h, nl, 4)


def time_entries(lib, dev, calls, windows):
    n, h, nl = WORKLOAD["n"], WORKLOAD["h"], WORKLOAD["nl"]
    W = weights(n, h, [i == nl - 1 for i in range(nl)], 1, dev)
    end_w = torch.randn(2 * h, n, generator=torch.Generator().manual_seed(2)).to(dev)
    s = _lib.stream_ptr()
    buf = lambda sizes: [torch.zeros(b // 4, dtype=torch.int32, device=dev) for b in sizes]
    nb_f, nb_d = lib.fst_wn_image_bytes(n, h), lib.fst_wn_dgrad_image_bytes(n)
    nb_b = [lib.fst_wn_bwd_image_bytes(n, int(i == nl - 1)) for i in range(nl)]
    nb_p = [lib.fst_wn_bwd_proj_image_bytes(n, 2 * h, int(i == nl - 1)) for i in range(nl)]
    f, b, p, d = buf([nb_f] * nl), buf(nb_b), buf(nb_p), buf([nb_d] * nl)
    F, B, P, D = tbl(f), tbl(b), tbl(p), tbl(d)
    cols = [col(W, j) for j in range(6)]
    l0 = [t.data_ptr() for t in W[0]]
    entries = {
        "fst_wn_pack": lambda: lib.fst_wn_pack(*l0, n, h, 3, 0, f[0].data_ptr(), nb_f, s),
        "fst_wn_pack_stack": lambda: lib.fst_wn_pack_stack(*cols, nl, n, h, 3, F, nb_f, s),
        "fst_wn_pack_bwd": lambda: lib.fst_wn_pack_bwd(l0[4], n, 0, 1, b[0].data_ptr(), nb_b[0], s),
        "fst_wn_pack_bwd_stack": lambda: lib.fst_wn_pack_bwd_stack(cols[4], nl, n, 1, B, nb_b[0], s),
        "fst_wn_pack_bwd_proj_stack": lambda: lib.fst_wn_pack_bwd_proj_stack(cols[4], end_w.data_ptr(), nl, n, 2 * h, P, nb_p[0], s),
        "fst_wn_pack_dgrad": lambda: lib.fst_wn_pack_dgrad(l0[0], l0[1], n, h, 3, d[0].data_ptr(), nb_d, s),
        "fst_wn_pack_dgrad_stack": lambda: lib.fst_wn_pack_dgrad_stack(cols[0], cols[1], nl, n, h, 3, D, nb_d, s),
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
        yield {"entry": name, "us": round(statistics.median(runs), 2), "us_runs": [round(r, 2) for r in runs], "n": n, "h": h,
               "layers": nl if name.endswith("_stack") else 1, "calls_per_window": calls}


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
        raise SystemExit("wn_pack_probe.py needs an MI355X")
    dev, lib = torch.device("cuda:0"), _lib.load()
    if a.digest:
        for name, case, sha256 in digest_cases(lib, dev):
            print(name, case.replace(" ", ","), sha256, flush=True)
        return
    for line in time_entries(lib, dev, a.calls, a.windows):
        if a.label:
            line["config"] = a.label
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
