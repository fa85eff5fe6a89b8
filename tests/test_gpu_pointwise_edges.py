"""The bandwidth-bound kernels — BatchNorm, gate, affine coupling, weight-norm fold, log|det W| (csrc/pointwise.hip), NoiseTransfer
(csrc/widgets.hip), fst_mask_taps (csrc/conv_engine.hip) and the multi-tensor optimisers (csrc/optim.hip) — through the C ABI,
inside guard bands, against fp64 on the CPU.

Conventions of tests/test_gpu_wn_routes.py (its helpers are imported, not copied): inputs sit between 64-float NaN bands (and NaN
guard channels where an entry point takes a batch stride), outputs between canary bands, pre-filled with NaN where the kernel
stores and with the previous value where it accumulates.  Every launch is repeated on fresh buffers and must give the same bits
(none of these kernels uses atomics), every refusal must leave every output untouched and a message in fst_last_error().
References are fp64 torch / numpy on the CPU, computed from the fp32-rounded operands the device receives.  No kernel here
depends on ops.MATH: the module is the same under FST_MATH=f32.

Gates: the ones the suite already applies to these operations (tests/test_gpu_kernels.py: 1e-5 of max|want| for outputs, 2e-5
for gradients, 1e-5·Σ|terms| for sums), tightened to 2e-6 / 4e-6 for outputs / gradients (OUT_TOL, GRAD_TOL).  The saturated and wide-range cases use bounds
derived from the operands, stated next to each; for every derived bound a test WITHOUT the gpu marker evaluates the same operation
in fp32 torch on the CPU and holds it to the same bound, so a bound plain fp32 cannot meet is never held against a kernel.
"""
from __future__ import annotations

import ctypes
import functools
import math
import zlib

import numpy as np
import pytest
import torch

from feature_level_style_transfer_for_tsc_amd import _lib
from test_gpu_wn_routes import (BAND, CANARY, DEV, NAN, assert_close, assert_fence, assert_untouched, check_rc, fenced, nan_in,
                                out_buf, ptrs)

EPS32 = 2.0 ** -24        # unit roundoff of fp32
SLOTS = 16                # FST_BN_SLOTS
# Gates of assert_close (error against max|want|).  The suite holds these operations to 1e-5 (outputs) and 2e-5 / 5e-5 (gradients)
# through ops.*; every kernel here is a handful of fp32 operations per element or a short dot product, and measures below 6e-7
# and 5e-7, so the gates are tightened to a few times that.
OUT_TOL, GRAD_TOL = 2e-6, 4e-6
F32 = lambda v: float(np.float32(v))


def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def r32(g, *shape, k: float = 1.0, add=0.0) -> torch.Tensor:
    """fp32 draws (the values the device receives), held in fp64."""
    return (torch.randn(*shape, generator=g) * k + add).float().double()


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def host(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().clone()


def sync():
    torch.cuda.synchronize()


class Keep:
    """Holds the device tensors of one launch until it has run: ``k(t)`` is ``t.data_ptr()`` (None for None) of a tensor kept alive —
    a temporary freed right after its address was taken would be handed out again for the next operand."""

    def __init__(self):
        self.held = []

    def __call__(self, t):
        self.held.append(t)
        return None if t is None else t.data_ptr()


def stream():
    return _lib.stream_ptr()


def repeat_equal(go, what: str):
    """Runs ``go`` (fresh buffers, one launch sequence, returns a dict of host tensors) twice: the same bits both times."""
    a, b = go(), go()
    for k in a:
        assert same_bits(a[k], b[k]), f"{what}: {k} differs between two launches on the same inputs"
    return a


def assert_written(t: torch.Tensor, what: str):
    left = int(torch.isnan(t).sum())
    assert left == 0, f"{what}: {left} elements were never written (or are NaN)"


def shifted(shape, band_fill: float, fill: float, off: int):
    """(buffer, view) like ``fenced``, but the view starts ``off`` floats past a 16-byte boundary (the spare floats hold the band
    value).  Only for pointers a launcher's vec_ok list names (it then takes the dword path) or fst_aligned16 refuses."""
    n = int(np.prod(shape))
    buf, body = fenced((n + 4,), band_fill, band_fill)
    v = body[off: off + n].view(*shape)
    v.fill_(fill)
    return buf, v


def nan_in_off(x: torch.Tensor, off: int) -> torch.Tensor:
    _, v = shifted(tuple(x.shape), NAN, 0.0, off)
    v.copy_(x)
    return v


def last_error(lib) -> str:
    msg = lib.fst_last_error()
    return msg.decode() if msg else ""


def assert_refused(rc: int, lib, who: str, what: str):
    assert rc < 0, f"{what}: accepted (rc={rc})"
    assert who in last_error(lib), f"{what}: fst_last_error() = {last_error(lib)!r} does not name {who}"


def assert_within(got, want, bound, what: str):
    """|got − want| <= bound elementwise (``bound`` a tensor or a number); prints the worst ratio."""
    got, want = got.detach().double(), want.detach().double()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(want)
    err = (got - want).abs()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"  {what}: worst error / bound = {ratio:.3f} (max err {float(err.max()) if err.numel() else 0.0:.3e})")
    assert bool((err <= bound).all()), f"{what}: error up to {ratio:.3f} of the bound"
    return ratio


# --------------------------------------------------------------------------------------------------
# A. BatchNorm through the ABI: fst_bn_stats, fst_bn_finalize, fst_bn_apply, fst_bn_bwd_reduce / fst_bn_bwd_apply
# --------------------------------------------------------------------------------------------------
# L = 4 .. 1024: the 16-byte path at shift 0, 2, 4, 6, 7 (rows wider than a wave: the LDS leg of the row sums), 8; L = 5: the dword path
BN_L = [4, 12, 60, 132, 260, 1024, 5]


@functools.lru_cache(maxsize=None)
def bn_input(B: int, C: int, L: int):
    g = _gen(f"bn{B}.{C}.{L}")
    mean = torch.linspace(-3.0, 5.0, C).view(1, C, 1)
    return r32(g, B, C, L, k=2.0, add=mean), r32(g, B, C, L), r32(g, B, C, L, k=1.5, add=0.3)     # y, dy, res


def check_slots(part: torch.Tensor, y: torch.Tensor, what: str):
    """Row b of a channel belongs to slot b mod 16 on both paths of bn_stats_kernel: the dword one walks b = blockIdx.y,
    blockIdx.y + 16, ...; the 16-byte one's row group r walks b = blockIdx.y + 16·(r + j·rows_per_pass) — the same residue class, regrouped.
    Bounds, from the inherited 1e-5·Σ|terms| for sums: with d = x − k, |Σd − s1| <= 1e-5·Σ|d| and |Σd² − s2| <= 1e-5·Σd²; then
    mean = k + s1/n is off by <= 1e-5·Σ|d|/n and M2 = s2 − s1²/n by <= 1e-5·(Σd² + 2·|Σd|·Σ|d|/n) (first order in the two errors)."""
    B, C, L = y.shape
    p = part.double()
    assert_written(part, what)
    for c in range(C):
        assert float(p[c, :, 0].sum()) == B * L, f"{what}: the counts of channel {c} add up to {float(p[c, :, 0].sum())}, not {B * L}"
        for s in range(SLOTS):
            rows = list(range(s, B, SLOTS))
            n = len(rows) * L
            assert float(p[c, s, 0]) == n, f"{what}: slot {s} of channel {c} counts {float(p[c, s, 0])} samples, its rows hold {n}"
            if n == 0:
                continue
            x = y[rows, c, :].reshape(-1)
            k, s1, s2 = (float(v) for v in p[c, s, 1:])
            d = x - k
            sd, sad, sdd = float(d.sum()), float(d.abs().sum()), float((d * d).sum())
            assert abs(s1 - sd) <= 1e-5 * sad + 1e-30, f"{what}: Σ(x−k) of slot {s}, channel {c}: {s1} vs {sd}"
            assert abs(s2 - sdd) <= 1e-5 * sdd + 1e-30, f"{what}: Σ(x−k)² of slot {s}, channel {c}: {s2} vs {sdd}"
            mean, m2 = k + s1 / n, s2 - s1 * s1 / n
            wm = float(x.mean())
            wm2 = float(((x - wm) ** 2).sum())
            assert abs(mean - wm) <= 1e-5 * sad / n + 1e-30, f"{what}: mean of slot {s}, channel {c}: {mean} vs {wm}"
            assert abs(m2 - wm2) <= 1e-5 * (sdd + 2 * abs(sd) * sad / n) + 1e-30, f"{what}: M2 of slot {s}, channel {c}: {m2} vs {wm2}"


@pytest.mark.gpu
@pytest.mark.parametrize("B,C", [(1, 3), (15, 3), (17, 5), (33, 2)])
def test_bn_stats_slots(B, C):
    lib = _lib.load()
    # (L, offset of the base in floats): L = 5 and a base one float off 16 bytes (vec_ok names y) take the dword kernel
    for L, off in [(L, 0) for L in BN_L] + [(8, 1)]:
        y = bn_input(B, C, L)[0]
        what = f"bn_stats B{B} C{C} L{L}+{off}"

        def go():
            yd = nan_in_off(y, off) if off else nan_in(y)
            b_part, part = out_buf((C, SLOTS, 4))
            check_rc(lib.fst_bn_stats(yd.data_ptr(), B, C, L, part.data_ptr(), B * C * L, stream()), what)
            sync()
            assert_fence(b_part, part, what)
            return dict(part=host(part))
        check_slots(repeat_equal(go, what)["part"], y, what)


def finalize_case(C: int, n_slots: int):
    """Synthetic partials (fp32 values in fp64) with empty slots, and the fp64 merge of them."""
    g = _gen(f"fin{C}.{n_slots}")
    cnt = torch.randint(0, 4, (C, n_slots), generator=g).double() * 37
    cnt[:, 0], cnt[:, 3] = 74.0, 0.0                                    # at least one live and one empty slot per channel
    k = r32(g, C, n_slots, k=3.0)
    s1 = (r32(g, C, n_slots, k=0.5) * cnt).float().double()
    s2 = ((s1 * s1 / cnt.clamp_min(1) + cnt * (0.5 + torch.rand(C, n_slots, generator=g).double())) * (1 + 1e-6)).float().double()
    part = torch.stack([cnt, k, s1, s2], dim=-1)
    part[cnt == 0] = torch.tensor([0.0, 1.25, 0.0, 0.0], dtype=torch.float64)      # what fst_bn_stats leaves in an empty slot
    n = part[..., 0]
    mb = part[..., 1] + part[..., 2] / n.clamp_min(1)
    Mb = (part[..., 3] - part[..., 2] ** 2 / n.clamp_min(1)).clamp_min(0)
    N = n.sum(1)
    mean = (n * mb).sum(1) / N
    M2 = (Mb + n * (mb - mean[:, None]) ** 2).sum(1)
    return part, mean, M2 / N, M2 / (N - 1), g


@pytest.mark.gpu
@pytest.mark.parametrize("train", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("C", [1, 63, 64, 65])
def test_bn_finalize(C, train):
    lib = _lib.load()
    n_slots = 32 if C == 65 else SLOTS                                  # 32: two ranks' partials gathered (SyncBN)
    part, mean, var, unb, g = finalize_case(C, n_slots)
    gamma, beta, rm0 = r32(g, C, add=1.0), r32(g, C), r32(g, C)
    rv0 = (torch.rand(C, generator=g) + 0.5).float().double()
    eps, mom = F32(1e-5), F32(0.1)
    if not train:
        mean, var = rm0, rv0
    invstd = 1.0 / torch.sqrt(var + eps)
    want = torch.stack([mean, invstd, gamma * invstd, beta - mean * gamma * invstd])
    what = f"bn_finalize C{C} train{train}"

    def go():
        k = Keep()
        pd = nan_in(part) if train else None
        b_rm, rm = out_buf((C,), init=rm0)
        b_rv, rv = out_buf((C,), init=rv0)
        b_st, st = out_buf((4, C))
        check_rc(lib.fst_bn_finalize(_lib.ptr(pd), n_slots if train else 0, k(nan_in(gamma)), k(nan_in(beta)), rm.data_ptr(),
                                     rv.data_ptr(), train, C, eps, mom, st.data_ptr(), stream()), what)
        sync()
        assert_fence(b_rm, rm, "running_mean"), assert_fence(b_rv, rv, "running_var"), assert_fence(b_st, st, "stats")
        return dict(rm=host(rm), rv=host(rv), stats=host(st))
    got = repeat_equal(go, what)
    assert_written(got["stats"], what)
    for i, name in enumerate(("mean", "invstd", "scale", "shift")):
        assert_close(got["stats"][i], want[i], OUT_TOL, f"{what} {name}")
    if train:
        assert_close(got["rm"], (1.0 - mom) * rm0 + mom * mean, OUT_TOL, what + " running mean")
        assert_close(got["rv"], (1.0 - mom) * rv0 + mom * unb, OUT_TOL, what + " running var")
    else:
        assert same_bits(got["rm"], rm0.float()) and same_bits(got["rv"], rv0.float()), f"{what}: eval mode changed the running statistics"


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [0, 1], ids=["linear", "relu"])
@pytest.mark.parametrize("variant", ["plain", "res+res_stats", "res"])
@pytest.mark.parametrize("B,C", [(17, 5), (1, 7)])               # B·C = 85 and 7 rows: idle row groups in the last workgroup
def test_bn_apply(B, C, variant, relu):
    lib = _lib.load()
    g = _gen(f"apply{B}.{C}")
    stats, rstats = r32(g, 4, C), r32(g, 4, C)
    for L in BN_L:
        y, _, res = bn_input(B, C, L)
        want = y * stats[2].view(1, C, 1) + stats[3].view(1, C, 1)
        if variant == "res+res_stats":
            want = want + (res * rstats[2].view(1, C, 1) + rstats[3].view(1, C, 1))
        elif variant == "res":
            want = want + res
        if relu:
            want = want.clamp_min(0)
        what = f"bn_apply B{B} C{C} L{L} {variant} relu{relu}"

        def go(off=0):
            k = Keep()
            rd = nan_in(res) if variant != "plain" else None
            rsd = nan_in(rstats) if variant == "res+res_stats" else None
            b_out, out = shifted((B, C, L), CANARY, NAN, off) if off else out_buf((B, C, L))
            check_rc(lib.fst_bn_apply(k(nan_in(y)), k(nan_in(stats)), _lib.ptr(rd), _lib.ptr(rsd), out.data_ptr(), B, C, L,
                                      relu, B * C * L, stream()), what)
            sync()
            assert_fence(b_out, out, what)
            return dict(out=host(out))
        got = repeat_equal(go, what)["out"]
        assert_written(got, what)
        assert_close(got, want, OUT_TOL, what)
        # `out` one float off 16 bytes (vec_ok names it): the dword kernel, the same explicit fused multiply-adds, the same bits
        assert same_bits(go(1)["out"], got), f"{what}: the dword path and the 16-byte path differ"


def bn_bwd_reference(B, C, L, mode):
    """fp64 backward of one BatchNorm (+ ReLU) from fp32-rounded operands.  mode: plain | relu-out | relu-y | eval."""
    y, dy, _ = bn_input(B, C, L)
    g = _gen(f"bnbwd{B}.{C}.{L}")
    mean = y.mean(dim=(0, 2)).float().double()
    invstd = (1.0 / torch.sqrt(y.var(dim=(0, 2), unbiased=False) + 1e-5)).float().double()
    gamma, beta = r32(g, C, add=1.0), r32(g, C, k=0.3)
    scale = (gamma * invstd).float().double()
    shift = (beta - mean * scale).float().double()
    stats = torch.stack([mean, invstd, scale, shift])
    v = lambda t: t.view(1, C, 1)
    out = None
    if mode == "relu-out":
        out = r32(g, B, C, L)                                           # any tensor: only its sign is read
        mask = out > 0
    elif mode == "relu-y":
        # sign of fma(y, scale, shift): the product of two fp32 numbers is exact in fp64 and rounding is monotone, so the fp64
        # value has the sign of the exact one, and so has the device's correctly rounded fused multiply-add
        mask = (y * v(scale) + v(shift)) > 0
    else:
        mask = torch.ones_like(y, dtype=torch.bool)
    gm = dy * mask
    xh = (y - v(mean)) * v(invstd)
    return dict(y=y, dy=dy, out=out, stats=stats, gm=gm, xh=xh, scale=scale, relu=int(mode.startswith("relu")), train=int(mode != "eval"))


def slot_sums(t: torch.Tensor):
    """[B, C, L] → ([C, 16] per-slot sums over the rows b ≡ slot (mod 16), [C, 16] sums of |terms|)."""
    B, C, _ = t.shape
    s, a = torch.zeros(C, SLOTS, dtype=torch.float64), torch.zeros(C, SLOTS, dtype=torch.float64)
    for k in range(min(SLOTS, B)):
        s[:, k], a[:, k] = t[k::SLOTS].sum(dim=(0, 2)), t[k::SLOTS].abs().sum(dim=(0, 2))
    return s, a


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "relu-out", "relu-y", "eval"])
@pytest.mark.parametrize("B,C", [(17, 5), (1, 7)])
def test_bn_backward_single_branch(B, C, mode):
    lib = _lib.load()
    for L in BN_L:
        r = bn_bwd_reference(B, C, L, mode)
        what = f"bn_bwd B{B} C{C} L{L} {mode}"
        numel, relu, train = B * C * L, r["relu"], r["train"]
        v = lambda t: t.view(1, C, 1)

        def launch(red_dev, n_slots, B_total, with_red_out=True, with_row_sums=True):
            k = Keep()
            od = nan_in(r["out"]) if r["out"] is not None else None
            b_ro, ro = out_buf((2 * C,))
            b_dx, dx = out_buf((B, C, L))
            b_rs, rs = out_buf((B, C))
            check_rc(lib.fst_bn_bwd_apply(k(nan_in(r["dy"])), k(nan_in(r["y"])), _lib.ptr(od), k(nan_in(r["stats"])),
                                          _lib.ptr(red_dev), n_slots, ro.data_ptr() if with_red_out else None, dx.data_ptr(),
                                          rs.data_ptr() if with_row_sums else None, B, C, L, relu, train, B_total, numel, stream()), what)
            sync()
            assert_fence(b_ro, ro, "red_out"), assert_fence(b_dx, dx, "dx"), assert_fence(b_rs, rs, "row_sums")
            if not with_red_out:
                assert_untouched(b_ro, ro, "red_out (not passed)")
            if not with_row_sums:
                assert_untouched(b_rs, rs, "row_sums (not passed)")
            return host(ro), host(dx), host(rs)

        def go():
            k = Keep()
            od = nan_in(r["out"]) if r["out"] is not None else None
            b_red, red = out_buf((2, C, SLOTS))
            check_rc(lib.fst_bn_bwd_reduce(k(nan_in(r["dy"])), k(nan_in(r["y"])), _lib.ptr(od), k(nan_in(r["stats"])),
                                           B, C, L, relu, red.data_ptr(), numel, stream()), what)
            sync()
            assert_fence(b_red, red, "red")
            ro, dx, rs = launch(red if train else None, SLOTS if train else 0, B, with_red_out=bool(train))
            return dict(red=host(red), red_out=ro, dx=dx, row_sums=rs)
        got = repeat_equal(go, what)
        assert_written(got["red"], what + " red"), assert_written(got["dx"], what + " dx"), assert_written(got["row_sums"], what + " row sums")
        # the partial sums, slot by slot
        for i, terms in enumerate((r["gm"], r["gm"] * r["xh"])):
            want, mass = slot_sums(terms)
            assert_within(got["red"][i], want, 1e-5 * mass + 1e-30, f"{what} red[{i}]")
        r0, r1 = r["gm"].sum(dim=(0, 2)), (r["gm"] * r["xh"]).sum(dim=(0, 2))
        m0, m1 = r["gm"].abs().sum(dim=(0, 2)), (r["gm"] * r["xh"]).abs().sum(dim=(0, 2))
        N = B * L
        dx = v(r["scale"]) * (r["gm"] - v(r0) / N - r["xh"] * v(r1) / N) if train else v(r["scale"]) * r["gm"]
        assert_close(got["dx"], dx, GRAD_TOL, what + " dx")
        if train:
            assert_within(got["red_out"], torch.cat([r0, r1]), 1e-5 * torch.cat([m0, m1]) + 1e-30, what + " red_out")
        assert_within(got["row_sums"], dx.sum(dim=2), 1e-5 * dx.abs().sum(dim=2) + 1e-30, what + " row sums vs fp64")
        assert_within(got["row_sums"], got["dx"].double().sum(dim=2), 1e-5 * got["dx"].double().abs().sum(dim=2) + 1e-30,
                      what + " row sums vs the kernel's own dx")
        if not train:
            continue
        # n_slots = 1 with the slots added by the caller in slot order (fp32, from zero: what bn_red_sums does): the same bits
        acc = torch.zeros(2, C)
        for s in range(SLOTS):
            acc = acc + got["red"][:, :, s]
        ro1, dx1, rs1 = launch(nan_in(acc), 1, B)
        assert same_bits(dx1, got["dx"]) and same_bits(ro1, got["red_out"]) and same_bits(rs1, got["row_sums"]), f"{what}: n_slots = 1 differs"
        # B_total = 3B: red summed over three ranks' batches by the caller, N = 3·B·L; neither red_out nor row_sums asked for
        red3 = (acc.double() * 3.0 + r32(_gen(what), 2, C)).float()
        _, dx3, _ = launch(nan_in(red3), 1, 3 * B, with_red_out=False, with_row_sums=False)
        q0, q1 = red3[0].double(), red3[1].double()
        assert_close(dx3, v(r["scale"]) * (r["gm"] - v(q0) / (3 * N) - r["xh"] * v(q1) / (3 * N)), GRAD_TOL, what + " dx, B_total = 3B")


BN_REFUSALS = ["stats numel", "apply numel", "reduce numel", "bwd_apply numel", "B_total < B", "red_out without red",
               "finalize train part = NULL", "finalize train n_slots = 0"]


@pytest.mark.gpu
@pytest.mark.parametrize("what", BN_REFUSALS)
def test_bn_refusals_write_nothing(what):
    lib = _lib.load()
    B, C, L = 3, 5, 12
    y, dy, _ = bn_input(B, C, L)
    n = B * C * L
    yd, dyd, st = nan_in(y), nan_in(dy), nan_in(r32(_gen("st"), 4, C))
    outs = dict(part=out_buf((C, SLOTS, 4)), out=out_buf((B, C, L)), red=out_buf((2, C, SLOTS)), red_out=out_buf((2 * C,)),
                dx=out_buf((B, C, L)), row_sums=out_buf((B, C)), stats=out_buf((4, C)), rm=out_buf((C,)), rv=out_buf((C,)))
    p = {k: v[1].data_ptr() for k, v in outs.items()}
    red_in = nan_in(torch.zeros(2, C, SLOTS))
    if what == "stats numel":
        rc, who = lib.fst_bn_stats(yd.data_ptr(), B, C, L, p["part"], n - 1, stream()), "fst_bn_stats"
    elif what == "apply numel":
        rc, who = lib.fst_bn_apply(yd.data_ptr(), st.data_ptr(), None, None, p["out"], B + 1, C, L, 1, n, stream()), "fst_bn_apply"
    elif what == "reduce numel":
        rc, who = lib.fst_bn_bwd_reduce(dyd.data_ptr(), yd.data_ptr(), None, st.data_ptr(), B, C, L + 4, 0, p["red"], n, stream()), "fst_bn_bwd_reduce"
    elif what == "bwd_apply numel":
        rc, who = lib.fst_bn_bwd_apply(dyd.data_ptr(), yd.data_ptr(), None, st.data_ptr(), red_in.data_ptr(), SLOTS, p["red_out"], p["dx"],
                                       p["row_sums"], 3 * B, C, L, 0, 1, 3 * B, n, stream()), "fst_bn_bwd_apply"       # the recorded fault's call
    elif what == "B_total < B":
        rc, who = lib.fst_bn_bwd_apply(dyd.data_ptr(), yd.data_ptr(), None, st.data_ptr(), red_in.data_ptr(), SLOTS, p["red_out"], p["dx"],
                                       p["row_sums"], B, C, L, 0, 1, B - 1, n, stream()), "fst_bn_bwd_apply"
    elif what == "red_out without red":
        rc, who = lib.fst_bn_bwd_apply(dyd.data_ptr(), yd.data_ptr(), None, st.data_ptr(), None, 0, p["red_out"], p["dx"],
                                       p["row_sums"], B, C, L, 0, 0, B, n, stream()), "fst_bn_bwd_apply"
    else:
        part = None if "part" in what else red_in.data_ptr()
        rc, who = lib.fst_bn_finalize(part, 0 if "n_slots" in what else SLOTS, st.data_ptr(), st.data_ptr(), p["rm"], p["rv"], 1, C, F32(1e-5),
                                      F32(0.1), p["stats"], stream()), "fst_bn_finalize"
    assert_refused(rc, lib, who, what)
    sync()
    for k, (buf, view) in outs.items():
        assert_untouched(buf, view, f"{what}: {k}")


# ---- the shift sample on a zero-padded edge
EDGE_RATIOS = [0.0, 50.0, 900.0, 2.0e4]                 # |mean| / std per channel (std = 1)


@functools.lru_cache(maxsize=None)
def edge_case(B: int, L: int, P: int):
    """A series with an offset behind a wide 'same'-padded conv: the first P positions of every row ramp from half the channel
    mean up to the mean.  Returns the fp32 input, the fp64 results and the errors of fp32 torch (the yardstick) per channel."""
    g = _gen(f"edge{B}.{L}.{P}")
    C = len(EDGE_RATIOS)
    ratio = torch.tensor(EDGE_RATIOS, dtype=torch.float64)
    y = torch.randn(B, C, L, generator=g, dtype=torch.float64) + ratio.view(1, C, 1)
    for j in range(P):
        y[:, :, j] += ratio.view(1, C) * (0.5 * j / P - 0.5)
    y32 = y.float()
    y = y32.double()
    m, var, unb = y.mean(dim=(0, 2)), y.var(dim=(0, 2), unbiased=False), y.var(dim=(0, 2), unbiased=True)
    want = (y - m.view(1, C, 1)) / torch.sqrt(var.view(1, C, 1))
    rm, rv = torch.zeros(C), torch.zeros(C)
    out32, _, invstd32 = torch.native_batch_norm(y32, torch.ones(C), torch.zeros(C), rm, rv, True, 1.0, 0.0)    # momentum 1: rv = unbiased variance
    rel = lambda got, ref: ((got.double() - ref).abs() / ref)
    yard = dict(out=(out32.double() - want).abs().amax(dim=(0, 2)) / want.abs().amax(dim=(0, 2)),
                var=rel(1.0 / invstd32.double() ** 2, var), rvar=rel(rv, unb))
    return dict(y=y, want=want, var=var, unb=unb, ratio=ratio, yard=yard)


def edge_bound(case, key):
    """The error of fp32 torch on the same input plus the representation term tests/test_gpu_kernels.py already allows — the input
    is fp32, so (x − mean) carries eps·|mean|: 3e-7·|mean|/std — times 4 for the different summation order.  torch's error is
    taken over the whole input (the worst of its channels): it accumulates in double, so what is left is the rounding of its
    fp32 results, which does not depend on |mean|/std — per channel it is one draw of that rounding, anywhere between nothing and
    half an ulp (6e-9 and 1.1e-7 of the variance on one and the same input), and no fp32 result can be held to a lucky draw."""
    yard, rep = case["yard"][key], 3e-7 * case["ratio"]
    # the worst channel stands in for each channel only where that changes nothing: wherever the representation term is non-zero
    # it is far larger than the difference, so the 50 / 900 / 2e4 channels are held to what their own yardstick gives
    assert bool(((yard.max() - yard)[rep > 0] < 0.01 * rep[rep > 0]).all()), f"{key}: the yardsticks of the channels differ by {float((yard.max() - yard).max()):.2e}"
    return 4.0 * (yard.max() + rep)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 8])
@pytest.mark.parametrize("B,L", [(16, 5000), (64, 1024)])
def test_bn_shift_sample_on_a_padded_edge(B, L, P):
    """bn_stats* shift by k = y[0, c, 0], here |mean|/2 away from the data.  Normalised output, batch variance (1 / invstd², eps = 0)
    and running variance (momentum 1) against fp64.  Measured on an MI355X, worst of the four cases, at |mean|/std = 0 / 50 / 900 /
    2e4: variance 1.3e-7 / 3.2e-6 / 1.5e-4 / 4.9e-5, output 1.2e-7 / 1.6e-6 / 7.5e-5 / 2.4e-5 (fp32 torch: <= 1.8e-7 everywhere);
    bounds 2.4e-7 / 6.0e-5 / 1.1e-3 / 2.4e-2 — the single sample costs accuracy, but less than the fp32 input already does."""
    lib = _lib.load()
    case = edge_case(B, L, P)
    C = len(EDGE_RATIOS)
    what = f"bn edge B{B} L{L} P{P}"

    def go():
        yd = nan_in(case["y"])
        b_part, part = out_buf((C, SLOTS, 4))
        b_rm, rm = out_buf((C,), init=torch.zeros(C))
        b_rv, rv = out_buf((C,), init=torch.zeros(C))
        b_st, st = out_buf((4, C))
        b_out, out = out_buf((B, C, L))
        one, zero = nan_in(torch.ones(C)), nan_in(torch.zeros(C))
        check_rc(lib.fst_bn_stats(yd.data_ptr(), B, C, L, part.data_ptr(), B * C * L, stream()), what)
        check_rc(lib.fst_bn_finalize(part.data_ptr(), SLOTS, one.data_ptr(), zero.data_ptr(), rm.data_ptr(), rv.data_ptr(), 1, C, 0.0, 1.0,
                                     st.data_ptr(), stream()), what)
        check_rc(lib.fst_bn_apply(yd.data_ptr(), st.data_ptr(), None, None, out.data_ptr(), B, C, L, 0, B * C * L, stream()), what)
        sync()
        for b, v_, n in ((b_part, part, "part"), (b_rm, rm, "running_mean"), (b_rv, rv, "running_var"), (b_st, st, "stats"), (b_out, out, "out")):
            assert_fence(b, v_, n)
        return dict(part=host(part), rv=host(rv), stats=host(st), out=host(out))
    got = repeat_equal(go, what)
    err = dict(out=(got["out"].double() - case["want"]).abs().amax(dim=(0, 2)) / case["want"].abs().amax(dim=(0, 2)),
               var=(1.0 / got["stats"][1].double() ** 2 - case["var"]).abs() / case["var"],
               rvar=(got["rv"].double() - case["unb"]).abs() / case["unb"])
    bad = []
    for key in ("out", "var", "rvar"):
        bound = edge_bound(case, key)
        for c, ratio in enumerate(EDGE_RATIOS):
            print(f"  {what} {key} |mean|/std = {ratio:g}: kernel {float(err[key][c]):.3e}, fp32 torch {float(case['yard'][key][c]):.3e}, "
                  f"bound {float(bound[c]):.3e}")
            if not float(err[key][c]) <= float(bound[c]):
                bad.append((key, ratio, float(err[key][c]), float(bound[c])))
    assert not bad, f"{what}: (quantity, |mean|/std, error, bound) = {bad}"


# --------------------------------------------------------------------------------------------------
# F(c). The multi-tensor optimiser launchers through the ABI: 65 tensors = one full chunk of 64 and a second launch of one
# --------------------------------------------------------------------------------------------------
OPT_N = 65
OPT_SIZES = [1, 3, 1023, 1025, 70_001]                # 70 001 > 64 workgroups x 1024: the grid-stride loop
OPT_LAUNCHERS = ["rmsprop", "rmsprop_dev", "adam", "adam_dev"]


class OptCase:
    """65 (p, g, m, v) tuples, each tensor its own banded buffer: p, m, v between canary bands (updated in place), g between NaN."""

    def __init__(self, name: str):
        g = _gen("opt" + name)
        self.n = [OPT_SIZES[i % len(OPT_SIZES)] if i % 13 else 70_001 for i in range(OPT_N)]
        self.n[64] = 1025                                               # the tensor of the second launch
        mk = lambda n, k=1.0: r32(g, n, k=k)
        self.p0, self.g0 = [mk(n) for n in self.n], [mk(n, 0.5) for n in self.n]
        self.m0, self.v0 = [mk(n, 0.1) for n in self.n], [(mk(n, 0.3) ** 2 + 0.01).float().double() for n in self.n]
        self.lr = [F32(1e-2 * (1 + i % 5)) for i in range(OPT_N)]
        self.p, self.m, self.v = ([out_buf((n,), init=t) for n, t in zip(self.n, src)] for src in (self.p0, self.m0, self.v0))
        self.g = [nan_in(t) for t in self.g0]
        self.lr_dev = nan_in(torch.tensor(self.lr, dtype=torch.float64))
        self.step = nan_in(torch.tensor([3.0], dtype=torch.float64))
        self.adam_lr = nan_in(torch.tensor([F32(2e-2)], dtype=torch.float64))

    def call(self, lib, launcher: str, null_g=None, zero_count=None):
        P, G = ptrs([v for _, v in self.p]), ptrs([None if i == null_g else t for i, t in enumerate(self.g)])
        M, V = ptrs([v for _, v in self.m]), ptrs([v for _, v in self.v])
        numel = (ctypes.c_int64 * OPT_N)(*[0 if i == zero_count else n for i, n in enumerate(self.n)])
        alpha, eps, b1, b2 = F32(0.99), F32(1e-8), F32(0.9), F32(0.999)
        if launcher == "rmsprop":
            return lib.fst_rmsprop_multi(P, G, V, numel, (ctypes.c_float * OPT_N)(*self.lr), OPT_N, alpha, eps, stream())
        if launcher == "rmsprop_dev":
            lrs = (ctypes.c_void_p * OPT_N)(*[self.lr_dev.data_ptr() + 4 * i for i in range(OPT_N)])
            return lib.fst_rmsprop_multi_dev(P, G, V, numel, lrs, OPT_N, alpha, eps, stream())
        if launcher == "adam":
            return lib.fst_adam_multi(P, G, M, V, numel, OPT_N, self.step.data_ptr(), F32(2e-2), b1, b2, eps, stream())
        return lib.fst_adam_multi_dev(P, G, M, V, numel, OPT_N, self.step.data_ptr(), self.adam_lr.data_ptr(), b1, b2, eps, stream())

    def assert_fences(self):
        for name, bufs in (("p", self.p), ("m", self.m), ("v", self.v)):
            for i, (buf, view) in enumerate(bufs):
                assert_fence(buf, view, f"{name}[{i}]")

    def state(self):
        return {f"{name}{i}": host(view) for name, bufs in (("p", self.p), ("m", self.m), ("v", self.v)) for i, (_, view) in enumerate(bufs)}


def opt_reference(c: OptCase, launcher: str):
    """One step in fp64 from the fp32 operands, by the formulas in the comments of csrc/optim.hip (= torch's operation order)."""
    alpha, eps, b1, b2, lr, t = F32(0.99), F32(1e-8), F32(0.9), F32(0.999), F32(2e-2), 3.0
    out = []
    for i in range(OPT_N):
        p, g, m, v = c.p0[i], c.g0[i], c.m0[i], c.v0[i]
        if launcher.startswith("rmsprop"):
            v = v * alpha + F32(1.0 - np.float32(alpha)) * g * g             # (1 − α) is formed in fp32 on the device
            out.append((p - c.lr[i] * (g / (v.sqrt() + eps)), m, v))
        else:
            m = m * b1 + F32(1.0 - np.float32(b1)) * g
            v = v * b2 + F32(1.0 - np.float32(b2)) * g * g
            out.append((p - (lr / (1 - b1 ** t)) * (m / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps)), m, v))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("launcher", OPT_LAUNCHERS)
def test_optimiser_step_in_bands(launcher):
    lib = _lib.load()

    def go():
        c = OptCase(launcher)
        check_rc(c.call(lib, launcher), launcher)
        sync()
        c.assert_fences()
        go.case = c
        return c.state()
    got = repeat_equal(go, launcher)
    want = opt_reference(go.case, launcher)
    worst = 0.0
    for i, (p, m, v) in enumerate(want):
        # the gate of tests/test_gpu_optim.py for one step: 4·eps32·|p| + 1e-5·lr for the parameter, 1e-5 of max|want| for the moments
        lr = go.case.lr[i] if launcher.startswith("rmsprop") else F32(2e-2)
        err = (got[f"p{i}"].double() - p).abs()
        tol = 4 * EPS32 * p.abs() + 1e-5 * lr
        worst = max(worst, float((err / tol).max()))
        assert bool((err <= tol).all()), f"{launcher}: parameter {i} ({go.case.n[i]} elements): {float((err / tol).max()):.3f} of the gate"
        for name, w in (("m", m), ("v", v)):
            assert float((got[f"{name}{i}"].double() - w).abs().max()) <= 1e-5 * float(w.abs().max()) + 1e-30, f"{launcher}: {name} of tensor {i}"
    print(f"  {launcher}: worst parameter error / gate = {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["null g", "count 0"])
@pytest.mark.parametrize("launcher", OPT_LAUNCHERS)
def test_optimiser_refusal_has_updated_nothing(launcher, bad):
    """Entry 64 of 65 is invalid: the call returns < 0 and the 64 tensors of the first chunk keep their bits — every entry is
    validated on the host before the first launch (the header's promise; the launchers used to validate chunk by chunk)."""
    lib = _lib.load()
    c = OptCase(launcher)
    rc = c.call(lib, launcher, null_g=64 if bad == "null g" else None, zero_count=64 if bad == "count 0" else None)
    sync()
    assert_refused(rc, lib, "tensor 64", f"{launcher}, {bad} at entry 64")
    c.assert_fences()
    for i in range(OPT_N):
        for name, bufs, src in (("p", c.p, c.p0), ("m", c.m, c.m0), ("v", c.v, c.v0)):
            assert same_bits(host(bufs[i][1]), src[i].float()), f"{launcher}, {bad}: the refused call changed {name}[{i}]"


# --------------------------------------------------------------------------------------------------
# B. WaveGlow gate and affine coupling
# --------------------------------------------------------------------------------------------------
FLT_MIN = 2.0 ** -126     # smallest normal fp32: below it a result has no relative accuracy (and may be flushed to zero)
GATE_SHAPES = [(1, 1, 1), (3, 10, 33), (2, 33, 500)]          # n·L = 16 500 > 64 workgroups x 256: the grid-stride loop
GATE_SPECIALS = [0.0, 1e-30, -1e-30, 8.0, -8.0, 17.0, -17.0, 40.0, -40.0, 89.0, -89.0, 100.0, -100.0]


def gate_f64(g: torch.Tensor, n: int):
    t, s = torch.tanh(g[:, :n]), torch.sigmoid(g[:, n:])
    return t, s, t * s


def gate_bwd_f64(ts: torch.Tensor, d: torch.Tensor, n: int):
    t, s = ts[:, :n], ts[:, n:]
    return torch.cat([d * s * (1 - t * t), d * t * s * (1 - s)], dim=1)


def run_gate(lib, g: torch.Tensor, dacts: torch.Tensor, what: str):
    """Guarded forward (g_ts overwritten in place, acts written) and backward from the forward's own (t, s)."""
    B, n2, L = g.shape
    n = n2 // 2

    def go():
        k = Keep()
        b_ts, ts = out_buf((B, n2, L), init=g)
        b_a, acts = out_buf((B, n, L))
        check_rc(lib.fst_gate_fwd(ts.data_ptr(), acts.data_ptr(), B, n, L, B * n * L, stream()), what)
        sync()
        assert_fence(b_ts, ts, "g_ts"), assert_fence(b_a, acts, "acts")
        b_dg, dg = out_buf((B, n2, L))
        check_rc(lib.fst_gate_bwd(k(nan_in(host(ts))), k(nan_in(dacts)), dg.data_ptr(), B, n, L, B * n * L, stream()), what)
        sync()
        assert_fence(b_dg, dg, "dg")
        return dict(ts=host(ts), acts=host(acts), dg=host(dg))
    got = repeat_equal(go, what)
    for name in got:
        assert_written(got[name], f"{what} {name}")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("B,n,L", GATE_SHAPES)
def test_gate_in_bands(B, n, L):
    lib, g = _lib.load(), _gen(f"gate{B}.{n}.{L}")
    x, d = r32(g, B, 2 * n, L, k=1.5), r32(g, B, n, L)
    got = run_gate(lib, x, d, f"gate B{B} n{n} L{L}")
    t, s, acts = gate_f64(x, n)
    assert_close(got["ts"], torch.cat([t, s], dim=1), OUT_TOL, "t | s")
    assert_close(got["acts"], acts, OUT_TOL, "acts")
    assert_close(got["dg"], gate_bwd_f64(got["ts"].double(), d, n), GRAD_TOL, "dg")


@functools.lru_cache(maxsize=None)
def saturated_gate_input():
    g = _gen("gate-saturated")
    B, n, L = 2, 6, 40
    x = r32(g, B, 2 * n, L, k=2.0).reshape(-1)
    sp = torch.tensor(GATE_SPECIALS, dtype=torch.float64)
    idx = torch.arange(0, x.numel(), 3)                                  # every third element, both halves, all thirteen values
    x[idx] = sp[torch.arange(idx.numel()) % sp.numel()]
    return x.view(B, 2 * n, L).float().double(), (r32(g, B, n, L) * 3.0).float().double(), n


def assert_saturated_gate(ts, acts, dg, what: str):
    """Bounds from the operands.  tanhf / expf are good to a few ulp: |Δt| <= 8·eps32·|t| (4 ulp).  s = 1 / (1 + expf(−x)) adds
    one addition and one division: 8·eps32·s, plus FLT_MIN — sigmoid(−89) = 2e-39 is below the normal range, and expf(89)
    overflows, so 0 is the fp32 answer.  acts = t·s: |s|·|Δt| + |t|·|Δs| + eps32·|t·s|.
    dg from the (t, s) given: 1 − t² has an ABSOLUTE error of about eps32 (no relative accuracy near |t| = 1), and |s| <= 1,
    |t·s·(1 − s)| <= 1/4, so both halves are within 8·eps32·|dacts| (+ FLT_MIN) of the fp64 value."""
    x, d, n = saturated_gate_input()
    t, s, a = gate_f64(x, n)
    bt, bs = 8 * EPS32 * t.abs() + FLT_MIN, 8 * EPS32 * s + FLT_MIN
    worst = [assert_within(ts[:, :n], t, bt, what + " t"), assert_within(ts[:, n:], s, bs, what + " s"),
             assert_within(acts, a, s * bt + t.abs() * bs + EPS32 * a.abs() + FLT_MIN, what + " acts"),
             assert_within(dg, gate_bwd_f64(ts.double(), d, n), (8 * EPS32 * d.abs() + FLT_MIN).repeat(1, 2, 1), what + " dg")]
    return max(worst)


@pytest.mark.gpu
def test_gate_saturated():
    x, d, n = saturated_gate_input()
    got = run_gate(_lib.load(), x, d, "saturated gate")
    assert_saturated_gate(got["ts"], got["acts"], got["dg"], "saturated gate")


def test_gate_saturated_bounds_hold_for_fp32_torch():
    x, d, n = saturated_gate_input()
    x32, d32 = x.float(), d.float()
    t, s = torch.tanh(x32[:, :n]), torch.sigmoid(x32[:, n:])
    dg = torch.cat([d32 * s * (1 - t * t), d32 * t * s * (1 - s)], dim=1)
    assert_saturated_gate(torch.cat([t, s], dim=1), t * s, dg, "fp32 torch, saturated gate")


# ---- affine coupling.  u, o, xn: [B, 2h, L]; o[:, :h] = b, o[:, h:] = log_s
COUPLING_SHAPES = [(1, 1, 1), (3, 7, 33), (2, 40, 1700)]      # h·L = 68 000 > 64 workgroups x 1024: grid-stride, 64 slots per sample


def coupling_f64(u, o, h):
    return torch.cat([u[:, :h], torch.exp(o[:, h:]) * u[:, h:] + o[:, :h]], dim=1)


def coupling_inv_f64(x, o, h):
    return torch.cat([x[:, :h], (x[:, h:] - o[:, :h]) / torch.exp(o[:, h:])], dim=1)


def coupling_bwd_f64(u, o, h, dxn=None, dlogs=None, g_ls=None, g_sq=None):
    """(du, d_o, Σ|terms| of du, Σ|terms| of d_o) by the formulas in front of coupling_bwd_kernel."""
    es, u0, u1, b = torch.exp(o[:, h:]), u[:, :h], u[:, h:], o[:, :h]
    z = torch.zeros_like(u0)
    q = 0.0 if g_sq is None else 2.0 * g_sq
    d0, d1 = (z, z) if dxn is None else (dxn[:, :h], dxn[:, h:])
    g0, g1 = d0 + q * u0, d1 + q * (es * u1 + b)
    m0, m1 = d0.abs() + abs(q) * u0.abs(), d1.abs() + abs(q) * ((es * u1).abs() + b.abs())
    ds, ms = g1 * u1 * es, m1 * u1.abs() * es
    if g_ls is not None:
        ds, ms = ds + g_ls, ms + abs(g_ls)
    if dlogs is not None:
        ds, ms = ds + dlogs, ms + dlogs.abs()
    return torch.cat([g0, g1 * es], 1), torch.cat([g1, ds], 1), torch.cat([m0, m1 * es], 1), torch.cat([m1, ms], 1)


def coupling_inv_bwd_f64(xn, o, dxn, h):
    ies, g1 = 1.0 / torch.exp(o[:, h:]), dxn[:, h:]
    return torch.cat([dxn[:, :h], g1 * ies], 1), torch.cat([-g1 * ies, -g1 * xn[:, h:]], 1)


def coupling_slot_of(B, h, L, blocks):
    """Element i of a sample's half is summed by workgroup (i / 256) mod blocks (coupling_fwd_kernel's grid-stride loop), into
    slot b·blocks + that."""
    i = torch.arange(h * L)
    return (torch.arange(B).view(B, 1) * blocks + ((i // 256) % blocks).view(1, -1)).reshape(-1)


def run_coupling(lib, u, o, h, what, extra=None, sums=True):
    """Guarded forward (with the slot sums), inverse of the forward's own output, both backwards.  extra: dict(dxn, dlogs, g_ls,
    g_sq) of the forward's backward (fp64 host values or None)."""
    B, _, L = u.shape
    numel = u.numel()
    extra = extra or {}
    n_slots = lib.fst_coupling_sum_slots(B, h, L)
    assert n_slots == B * min(64, max(1, -(-h * L // 1024))), f"{what}: fst_coupling_sum_slots = {n_slots}"

    def go():
        k = Keep()
        ud, od = nan_in(u), nan_in(o)
        b_xn, xn = out_buf(tuple(u.shape))
        b_sl, sl = out_buf((n_slots, 2))
        check_rc(lib.fst_coupling_fwd(ud.data_ptr(), od.data_ptr(), xn.data_ptr(), B, h, L, numel, sl.data_ptr() if sums else None, stream()), what)
        sync()
        assert_fence(b_xn, xn, "xn"), assert_fence(b_sl, sl, "sums")
        if not sums:
            assert_untouched(b_sl, sl, "sums (not passed)")
        b_ui, ui = out_buf(tuple(u.shape))
        check_rc(lib.fst_coupling_inv_fwd(k(nan_in(host(xn))), od.data_ptr(), ui.data_ptr(), B, h, L, numel, stream()), what + " inverse")
        dev = {n: (None if v is None else nan_in(v if torch.is_tensor(v) else torch.tensor([v], dtype=torch.float64))) for n, v in extra.items()}
        b_du, du = out_buf(tuple(u.shape))
        b_do, d_o = out_buf(tuple(u.shape))
        out = dict(xn=xn, sums=sl, inv=ui)
        if any(v is not None for v in extra.values()):
            check_rc(lib.fst_coupling_bwd(ud.data_ptr(), od.data_ptr(), _lib.ptr(dev.get("dxn")), _lib.ptr(dev.get("dlogs")), _lib.ptr(dev.get("g_ls")),
                                          _lib.ptr(dev.get("g_sq")), du.data_ptr(), d_o.data_ptr(), B, h, L, numel, stream()), what + " bwd")
            out.update(du=du, d_o=d_o)
        b_dx, dx = out_buf(tuple(u.shape))
        b_dio, dio = out_buf(tuple(u.shape))
        if extra.get("dxn") is not None:
            check_rc(lib.fst_coupling_inv_bwd(k(nan_in(host(xn))), od.data_ptr(), dev["dxn"].data_ptr(), dx.data_ptr(), dio.data_ptr(), B, h, L,
                                              numel, stream()), what + " inverse bwd")
            out.update(dx=dx, dio=dio)
        sync()
        for b_, v_, n_ in ((b_ui, ui, "inverse xn"), (b_du, du, "du"), (b_do, d_o, "d_o"), (b_dx, dx, "dx"), (b_dio, dio, "inverse d_o")):
            assert_fence(b_, v_, n_)
        return {n: host(v) for n, v in out.items()}
    return repeat_equal(go, what)


@pytest.mark.gpu
@pytest.mark.parametrize("combo", ["g_sq", "g_ls", "dxn+dlogs", "dxn", "all", "no sums"])
@pytest.mark.parametrize("B,h,L", COUPLING_SHAPES)
def test_coupling_in_bands(B, h, L, combo):
    lib, g = _lib.load(), _gen(f"coupling{B}.{h}.{L}")
    u, o = r32(g, B, 2 * h, L), r32(g, B, 2 * h, L, k=0.5)
    dxn, dlogs, g_ls, g_sq = r32(g, B, 2 * h, L), r32(g, B, h, L), F32(-0.37), F32(0.21)
    extra = {"g_sq": dict(g_sq=g_sq), "g_ls": dict(g_ls=g_ls), "dxn+dlogs": dict(dxn=dxn, dlogs=dlogs), "dxn": dict(dxn=dxn),
             "all": dict(dxn=dxn, dlogs=dlogs, g_ls=g_ls, g_sq=g_sq), "no sums": dict(dxn=dxn)}[combo]
    what = f"coupling B{B} h{h} L{L} {combo}"
    got = run_coupling(lib, u, o, h, what, extra, sums=combo != "no sums")
    for name in got:
        if not (name == "sums" and combo == "no sums"):
            assert_written(got[name], f"{what} {name}")
    xn = coupling_f64(u, o, h)
    assert_close(got["xn"], xn, OUT_TOL, what + " xn")
    assert_close(got["inv"], coupling_inv_f64(got["xn"].double(), o, h), OUT_TOL, what + " inverse of the kernel's xn")
    du, d_o, _, _ = coupling_bwd_f64(u, o, h, **extra)
    assert_close(got["du"], du, GRAD_TOL, what + " du"), assert_close(got["d_o"], d_o, GRAD_TOL, what + " d_o")
    if "dx" in got:
        dx, dio = coupling_inv_bwd_f64(got["xn"].double(), o, extra["dxn"], h)
        assert_close(got["dx"], dx, GRAD_TOL, what + " inverse dx"), assert_close(got["dio"], dio, GRAD_TOL, what + " inverse d_o")
    if combo == "no sums":
        return
    # the two loss reductions: slot by slot, added in slot order, and against the kernel's own xn
    blocks = got["sums"].shape[0] // B
    slot = coupling_slot_of(B, h, L, blocks)
    for i, (terms, own) in enumerate(((o[:, h:], o[:, h:]), (u[:, :h] ** 2 + xn[:, h:] ** 2, got["xn"].double()[:, :h] ** 2 + got["xn"].double()[:, h:] ** 2))):
        name = ("Σ log_s", "Σ xn²")[i]
        want = torch.zeros(B * blocks, dtype=torch.float64).index_add_(0, slot, terms.reshape(-1))
        mass = torch.zeros(B * blocks, dtype=torch.float64).index_add_(0, slot, terms.abs().reshape(-1))
        assert_within(got["sums"][:, i], want, 1e-5 * mass + 1e-30, f"{what} {name} per slot")
        total = 0.0
        for v in got["sums"][:, i].double().tolist():
            total += v
        assert abs(total - float(terms.sum())) <= 1e-5 * float(terms.abs().sum()), f"{what}: {name} = {total} vs {float(terms.sum())}"
        assert abs(total - float(own.sum())) <= 1e-5 * float(own.abs().sum()), f"{what}: {name} = {total} vs the kernel's own output {float(own.sum())}"


@functools.lru_cache(maxsize=None)
def wide_coupling_input():
    """log_s spread over [−40, 40]: exp(40) = 2.4e17, so xn reaches 1e18 and its square 1e36 — finite in fp32, and so is the sum
    of the 231 squares a slot adds (< 3.4e38).  g_sq is small enough that 2·g_sq·xn·u·exp(s) (<= 1e33) stays finite too."""
    g = _gen("coupling-wide")
    B, h, L = 3, 7, 33
    u, o = r32(g, B, 2 * h, L), r32(g, B, 2 * h, L)
    o[:, h:] = (torch.rand(B, h, L, generator=g) * 80.0 - 40.0).float().double()
    return u, o, h, dict(dxn=r32(g, B, 2 * h, L), dlogs=r32(g, B, h, L), g_ls=F32(-0.37), g_sq=F32(1e-3))


def assert_wide_coupling(got, what: str):
    """Bounds relative to Σ|terms| of each element.  expf is good to 2 ulp, every product, sum and quotient adds half an ulp:
    xn₁ = e·u₁ + b and its inverse pass one expf and two roundings — 8·eps32·(|e·u₁| + |b|) resp. 8·eps32·(|x₁| + |b|)/e has
    margin; the backward's terms hold up to two factors e and four more operations: 16·eps32·Σ|terms|.
    inverse(forward(u)) against u: the forward's error bound divided by e, plus the inverse's own bound on the fp32 xn."""
    u, o, h, extra = wide_coupling_input()
    es, b = torch.exp(o[:, h:]), o[:, :h]
    z = torch.zeros_like(b)
    xn = coupling_f64(u, o, h)
    bf = torch.cat([z, 8 * EPS32 * ((es * u[:, h:]).abs() + b.abs())], 1)
    worst = [assert_within(got["xn"], xn, bf, what + " xn")]
    x32 = got["xn"].double()
    bi = torch.cat([z, 8 * EPS32 * (x32[:, h:].abs() + b.abs()) / es], 1)
    worst.append(assert_within(got["inv"], coupling_inv_f64(x32, o, h), bi, what + " inverse of the fp32 xn"))
    worst.append(assert_within(got["inv"], u, bi + torch.cat([z, bf[:, h:] / es], 1), what + " inverse(forward(u)) vs u"))
    du, d_o, mu, mo = coupling_bwd_f64(u, o, h, **extra)
    worst.append(assert_within(got["du"], du, 16 * EPS32 * mu, what + " du"))
    worst.append(assert_within(got["d_o"], d_o, 16 * EPS32 * mo, what + " d_o"))
    dx, dio = coupling_inv_bwd_f64(x32, o, extra["dxn"], h)
    worst.append(assert_within(got["dx"], dx, 8 * EPS32 * dx.abs(), what + " inverse dx"))
    worst.append(assert_within(got["dio"], dio, 8 * EPS32 * dio.abs(), what + " inverse d_o"))
    return max(worst)


def coupling_fp32_torch(u, o, h, extra):
    """The four coupling passes in fp32 torch on the CPU, in the kernels' operation order."""
    u, o = u.float(), o.float()
    es, u0, u1, b = torch.exp(o[:, h:]), u[:, :h], u[:, h:], o[:, :h]
    x1 = es * u1 + b
    xn = torch.cat([u0, x1], 1)
    inv = torch.cat([u0, (x1 - b) / es], 1)
    dxn = extra["dxn"].float()
    q = 2.0 * np.float32(extra["g_sq"]) if extra.get("g_sq") is not None else np.float32(0.0)
    g0, g1 = dxn[:, :h] + q * u0, dxn[:, h:] + q * x1
    ds = g1 * u1 * es
    if extra.get("g_ls") is not None:
        ds = ds + np.float32(extra["g_ls"])
    if extra.get("dlogs") is not None:
        ds = ds + extra["dlogs"].float()
    ies, d1 = 1.0 / es, dxn[:, h:]
    return dict(xn=xn, inv=inv, du=torch.cat([g0, g1 * es], 1), d_o=torch.cat([g1, ds], 1), dx=torch.cat([dxn[:, :h], d1 * ies], 1),
                dio=torch.cat([-d1 * ies, -d1 * x1], 1))


@pytest.mark.gpu
def test_coupling_wide_log_s():
    u, o, h, extra = wide_coupling_input()
    got = run_coupling(_lib.load(), u, o, h, "coupling, |log_s| <= 40", extra)
    assert_wide_coupling(got, "coupling, |log_s| <= 40")
    assert bool(torch.isfinite(got["sums"]).all()), "the slot sums overflowed"


def test_coupling_wide_log_s_bounds_hold_for_fp32_torch():
    u, o, h, extra = wide_coupling_input()
    assert_wide_coupling(coupling_fp32_torch(u, o, h, extra), "fp32 torch, |log_s| <= 40")


def same_pattern(got, want, what: str):
    """NaN where fp32 torch has NaN, ±inf where it has ±inf, and the finite values within 4 ulp (+ FLT_MIN) of its finite values."""
    nan_bad = int((torch.isnan(got) != torch.isnan(want)).sum())
    inf = torch.isinf(want)
    inf_bad = int((torch.isinf(got) != inf).sum()) + int((torch.sign(got[inf]) != torch.sign(want[inf])).sum())
    fin = torch.isfinite(want) & torch.isfinite(got)
    g_, w_ = got[fin].double(), want[fin].double()
    fin_bad = int(((g_ - w_).abs() > 8 * EPS32 * w_.abs() + FLT_MIN).sum())
    print(f"  {what}: {int(torch.isnan(want).sum())} NaN, {int(inf.sum())} inf, {int(fin.sum())} finite in fp32 torch; mismatches {nan_bad} / {inf_bad} / {fin_bad}")
    assert nan_bad == 0 and inf_bad == 0 and fin_bad == 0, f"{what}: {nan_bad} NaN, {inf_bad} inf and {fin_bad} finite elements differ from fp32 torch"


@pytest.mark.gpu
def test_coupling_overflowing_log_s_matches_fp32_torch():
    """log_s = ±100: expf overflows to inf or underflows to the subnormal 4e-44.  The non-finite pattern and the finite values of
    the forward, the inverse and both backwards are fp32 torch's."""
    g = _gen("coupling-100")
    B, h, L = 2, 5, 12
    u, o = r32(g, B, 2 * h, L, add=3.0), r32(g, B, 2 * h, L)           # u away from 0: no 0·inf
    o[:, h:] = torch.where(torch.rand(B, h, L, generator=g) < 0.5, -100.0, 100.0).double()
    extra = dict(dxn=r32(g, B, 2 * h, L, add=3.0))
    got = run_coupling(_lib.load(), u, o, h, "coupling, log_s = ±100", extra, sums=False)
    want = coupling_fp32_torch(u, o, h, extra)
    # the inverse pair starts from the kernel's own xn, which is torch's where finite (checked first)
    for name in ("xn", "du", "d_o"):
        same_pattern(got[name], want[name], name)
    assert bool(torch.isinf(want["xn"]).any()) and bool(torch.isfinite(want["xn"][:, h:]).any()), "the case no longer holds both patterns"
    # the inverse and its backward ran on the kernel's own xn: fp32 torch from that same tensor.  log_s = +100: (±inf − b)/inf = NaN,
    # 1/inf = 0, −g·(±inf) = ∓inf; log_s = −100: xn₁ is b itself, (b − b)/4e-44 = 0 (the subnormal divisor survives on the device as
    # on the CPU; flushed, it would be 0/0), 1/4e-44 overflows to inf
    x, o32, d32 = got["xn"], o.float(), extra["dxn"].float()
    es, x1, b, d1 = torch.exp(o32[:, h:]), x[:, h:], o32[:, :h], d32[:, h:]
    ies = 1.0 / es
    inverse = dict(inv=torch.cat([x[:, :h], (x1 - b) / es], 1), dx=torch.cat([d32[:, :h], d1 * ies], 1), dio=torch.cat([-d1 * ies, -d1 * x1], 1))
    for name, w in inverse.items():
        same_pattern(got[name], w, name)
    assert bool(torch.isnan(inverse["inv"]).any()) and bool((inverse["inv"][:, h:] == 0).any()) and bool(torch.isinf(inverse["dx"]).any())


COUPLING_REFUSALS = ["fwd numel", "inv_fwd numel", "bwd numel", "inv_bwd numel", "bwd without any cotangent", "gate_fwd numel", "gate_bwd numel"]


@pytest.mark.gpu
@pytest.mark.parametrize("what", COUPLING_REFUSALS)
def test_gate_and_coupling_refusals_write_nothing(what):
    lib, g = _lib.load(), _gen("coupling-refusals")
    B, h, L = 2, 3, 8
    n = B * 2 * h * L
    u, o, d = nan_in(r32(g, B, 2 * h, L)), nan_in(r32(g, B, 2 * h, L)), nan_in(r32(g, B, 2 * h, L))
    outs = dict(a=out_buf((B, 2 * h, L)), b=out_buf((B, 2 * h, L)), sums=out_buf((B, 2)), acts=out_buf((B, h, L)))
    pa, pb = outs["a"][1].data_ptr(), outs["b"][1].data_ptr()
    if what == "fwd numel":
        rc, who = lib.fst_coupling_fwd(u.data_ptr(), o.data_ptr(), pa, B + 1, h, L, n, outs["sums"][1].data_ptr(), stream()), "fst_coupling"
    elif what == "inv_fwd numel":
        rc, who = lib.fst_coupling_inv_fwd(u.data_ptr(), o.data_ptr(), pa, B, h + 1, L, n, stream()), "fst_coupling"
    elif what == "bwd numel":
        rc, who = lib.fst_coupling_bwd(u.data_ptr(), o.data_ptr(), d.data_ptr(), None, None, None, pa, pb, B, h, L, n + 1, stream()), "fst_coupling_bwd"
    elif what == "inv_bwd numel":
        rc, who = lib.fst_coupling_inv_bwd(u.data_ptr(), o.data_ptr(), d.data_ptr(), pa, pb, B, h, L + 1, n, stream()), "fst_coupling_inv_bwd"
    elif what == "bwd without any cotangent":
        rc, who = lib.fst_coupling_bwd(u.data_ptr(), o.data_ptr(), None, d.data_ptr(), None, None, pa, pb, B, h, L, n, stream()), "fst_coupling_bwd"
    elif what == "gate_fwd numel":           # g_ts is an in/out operand: here the NaN-filled `a`, so a write shows
        rc, who = lib.fst_gate_fwd(pa, outs["acts"][1].data_ptr(), B, h, L, B * h * L + 1, stream()), "fst_gate_fwd"
    else:
        rc, who = lib.fst_gate_bwd(u.data_ptr(), d.data_ptr(), pa, B, h, L + 1, B * h * L, stream()), "fst_gate_bwd"
    assert_refused(rc, lib, who, what)
    sync()
    for k, (buf, view) in outs.items():
        assert_untouched(buf, view, f"{what}: {k}")


# --------------------------------------------------------------------------------------------------
# C. Weight-norm fold with a hand-built row table
# --------------------------------------------------------------------------------------------------
FOLD_LENS = [1, 7, 63, 64, 65, 192, 384, 7, 65]              # a wave per row: one lane, a partial pass, 1 / 1+ / 3 / 6 passes
FOLD_GAP = 5                                                 # canary floats between the rows of flat and of dpar


class FoldCase:
    """n_rows rows; row r is a plain copy when r % 3 == 2, else normed with its own g.  flat and dpar hold the rows with gaps."""

    def __init__(self, n_rows: int, scales=None, gs=None, name="fold"):
        g = _gen(f"{name}{n_rows}")
        self.n_rows, self.lens = n_rows, FOLD_LENS[:n_rows]
        self.plain = [r % 3 == 2 for r in range(n_rows)]
        scales = scales or [1.0] * n_rows
        self.v = [r32(g, n, k=scales[r]) for r, n in enumerate(self.lens)]
        self.g = torch.tensor(gs, dtype=torch.float64) if gs is not None else r32(g, n_rows, add=0.2)
        self.dw = [r32(g, n) for n in self.lens]
        self.dst, self.dv, self.dg = [], [], []
        off = 3
        for n in self.lens:
            self.dst.append(off)
            off += n + FOLD_GAP
        self.flat_n = off
        off = 2
        for r, n in reversed(list(enumerate(self.lens))):               # dpar in another order than flat
            self.dv.append(off)
            self.dg.append(off + n + 1)
            off += n + 2 + FOLD_GAP
        self.dv.reverse(), self.dg.reverse()
        self.dpar_n = off

    def device(self):
        self.vd = [nan_in(v) for v in self.v]
        self.gd = nan_in(self.g)
        rows = [[self.vd[r].data_ptr(), 0 if self.plain[r] else self.gd.data_ptr() + 4 * r, self.dst[r], self.lens[r], self.dv[r], self.dg[r]]
                for r in range(self.n_rows)]
        self.table = torch.tensor(rows, dtype=torch.int64, device=DEV)
        self.b_flat, self.flat = fenced((self.flat_n,), CANARY, CANARY)
        self.b_dpar, self.dpar = fenced((self.dpar_n,), CANARY, CANARY)
        self.b_norms, self.norms = out_buf((self.n_rows,))
        self.dflat = nan_in(torch.full((self.flat_n,), NAN, dtype=torch.float64))       # the gaps of d_flat hold NaN: reading one shows
        for r, n in enumerate(self.lens):
            self.flat[self.dst[r]: self.dst[r] + n] = NAN
            self.dflat[self.dst[r]: self.dst[r] + n] = self.dw[r].float().to(DEV)
            self.dpar[self.dv[r]: self.dv[r] + n] = NAN
            if not self.plain[r]:
                self.dpar[self.dg[r]] = NAN

    def assert_gaps(self):
        """Bands and gaps of flat / dpar still hold the canary, the norms entries of the plain-copy rows were not written."""
        for buf, view, segs, what in ((self.b_flat, self.flat, [(self.dst[r], n) for r, n in enumerate(self.lens)], "flat"),
                                      (self.b_dpar, self.dpar, [(self.dv[r], n) for r, n in enumerate(self.lens)] +
                                       [(self.dg[r], 1) for r in range(self.n_rows) if not self.plain[r]], "dpar")):
            probe = buf.clone()
            pv = probe[BAND: BAND + view.numel()]
            for a, n in segs:
                pv[a: a + n] = CANARY
            bad = int((probe != CANARY).sum())
            assert bad == 0, f"{what}: {bad} elements outside the rows were written"
        assert_fence(self.b_norms, self.norms, "norms")
        for r in range(self.n_rows):
            assert bool(torch.isnan(self.norms[r])) == self.plain[r], f"norms[{r}]: " + ("written for a plain-copy row" if self.plain[r] else "not written")

    def run(self, lib, what):
        def go():
            self.device()
            check_rc(lib.fst_wn_fold_fwd(self.table.data_ptr(), self.n_rows, self.flat.data_ptr(), self.norms.data_ptr(), stream()), what)
            sync()
            norms_in = nan_in(host(self.norms))
            check_rc(lib.fst_wn_fold_bwd(self.table.data_ptr(), self.n_rows, self.dflat.data_ptr(), norms_in.data_ptr(), self.dpar.data_ptr(), stream()), what)
            sync()
            self.assert_gaps()
            return dict(flat=host(self.flat), dpar=host(self.dpar), norms=host(self.norms))
        return repeat_equal(go, what)

    def reference(self, r: int):
        """fp64 torch._weight_norm of row r and its autograd: (w, dv, dg, Σ|terms| of dv, Σ|terms| of dg)."""
        v, dw = self.v[r].clone().view(1, -1).requires_grad_(True), self.dw[r].view(1, -1)
        if self.plain[r]:
            return self.v[r], self.dw[r], None, self.dw[r].abs(), None
        gg = self.g[r].clone().view(1, 1).requires_grad_(True)
        w = torch._weight_norm(v, gg, 0)
        (w * dw).sum().backward()
        norm = float(self.v[r].norm())
        adot = float((self.dw[r] * self.v[r]).abs().sum())
        mass_v = abs(float(self.g[r])) / norm * (self.dw[r].abs() + self.v[r].abs() * adot / norm ** 2)
        return w.detach().view(-1), v.grad.view(-1), float(gg.grad), mass_v, adot / norm


def check_fold(c: FoldCase, got, what: str):
    """w: 1e-6 of the row's max (a 384-term sum of squares, a square root, a quotient and a product; the suite's gate for outputs
    is 1e-5).  dv and dg are sums with cancellation (dv of a one-element row is an exact zero in exact arithmetic), so they are
    held to 2e-6·Σ|terms|: |g|/‖v‖·(|dw_j| + |v_j|·Σ|dw·v|/‖v‖²) and Σ|dw·v|/‖v‖ (the suite's 2e-5 for gradients, tightened)."""
    worst = 0.0
    for r, n in enumerate(c.lens):
        w, dv, dg, mass_v, mass_g = c.reference(r)
        gw, gdv = got["flat"][c.dst[r]: c.dst[r] + n], got["dpar"][c.dv[r]: c.dv[r] + n]
        if c.plain[r]:
            assert same_bits(gw, w.float()) and same_bits(gdv, dv.float()), f"{what}: plain-copy row {r} is not a copy"
            continue
        worst = max(worst, assert_within(gw, w, 1e-6 * float(w.abs().max()), f"{what} row {r} (len {n}) w"))
        assert abs(float(got["norms"][r]) - float(c.v[r].norm())) <= 1e-6 * float(c.v[r].norm()), f"{what}: norms[{r}]"
        worst = max(worst, assert_within(gdv, dv, 2e-6 * mass_v, f"{what} row {r} dv"))
        worst = max(worst, assert_within(got["dpar"][c.dg[r]], torch.tensor(dg, dtype=torch.float64), 2e-6 * mass_g, f"{what} row {r} dg"))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", [1, 5, 9])                 # four rows per workgroup: the last one holds 1, 1 and 1 live waves
def test_wn_fold_hand_built_table(n_rows):
    c = FoldCase(n_rows)
    check_fold(c, c.run(_lib.load(), f"fold {n_rows} rows"), f"fold {n_rows} rows")


FOLD_SCALES = [1e-15, 1e15, 1e-8, 1e8, 1.0, 1e-15, 1e15, 1e3, 1e-3]     # ‖v‖² from 1e-30 to 4e32: inside the normal fp32 range
FOLD_GS = [1.5, -0.7, 0.0, 0.0, -2.0, 1e3, -1e-3, 0.0, 3.0]             # positive, negative and exactly 0


@pytest.mark.gpu
def test_wn_fold_row_scales_and_g_signs():
    c = FoldCase(9, FOLD_SCALES, FOLD_GS, name="fold-scales")
    check_fold(c, c.run(_lib.load(), "fold, row scales 1e-15..1e15"), "fold, row scales 1e-15..1e15")


def test_wn_fold_bounds_hold_for_fp32_torch():
    c = FoldCase(9, FOLD_SCALES, FOLD_GS, name="fold-scales")
    flat, dpar, norms = torch.full((c.flat_n,), NAN), torch.full((c.dpar_n,), NAN), torch.full((9,), NAN)
    for r, n in enumerate(c.lens):
        v, dw = c.v[r].float(), c.dw[r].float()
        if c.plain[r]:
            flat[c.dst[r]: c.dst[r] + n], dpar[c.dv[r]: c.dv[r] + n] = v, dw
            continue
        gg, norm, dot = c.g[r].float(), (v * v).sum().sqrt(), (dw * v).sum()
        flat[c.dst[r]: c.dst[r] + n] = v * (gg / norm)
        dpar[c.dv[r]: c.dv[r] + n] = (gg / norm) * (dw - v * (dot / (norm * norm)))
        dpar[c.dg[r]], norms[r] = dot / norm, norm
    check_fold(c, dict(flat=flat, dpar=dpar, norms=norms), "fp32 torch, fold")


@pytest.mark.gpu
def test_wn_fold_out_of_range_norms_match_fp32_torch():
    """‖v‖² underflows to 0 (|v| ~ 1e-30) or overflows to inf (|v| ~ 1e25): fp32 torch._weight_norm on the CPU forms the norm in
    fp32 too and gives w = v·(g/0) = ±inf resp. v·(g/inf) = ±0; the kernel must give the same pattern (signs of zero included).
    The backward from those norms is pinned too: dg to torch's autograd, dv to the documented formula (see below)."""
    c = FoldCase(2, [1e-30, 1e25], [1.5, -0.7], name="fold-range")
    got = c.run(_lib.load(), "fold, ‖v‖² out of range")
    for r, n in enumerate(c.lens):
        want = torch._weight_norm(c.v[r].float().view(1, -1), c.g[r].float().view(1, 1), 0).view(-1)
        assert same_bits(got["flat"][c.dst[r]: c.dst[r] + n], want), f"row {r}: {got['flat'][c.dst[r]: c.dst[r] + n]} vs fp32 torch {want}"
    assert float(got["norms"][0]) == 0.0 and math.isinf(float(got["norms"][1]))
    # backward with norms = 0 / inf.  dg is fp32 torch autograd's (±inf resp. ±0).  dv is the header's formula evaluated in fp32 as
    # written — (g/‖v‖)·(dw − v·(dw·v)/‖v‖²): ±inf everywhere for ‖v‖ = 0, where torch's autograd groups the terms differently and
    # has NaN in some elements (include/fst_hip.h says so; non-finite either way), and torch's ±0 for ‖v‖ = inf
    for r, n in enumerate(c.lens):
        v, dw, gg = c.v[r].float(), c.dw[r].float(), c.g[r].float()
        vt, gt = v.clone().view(1, -1).requires_grad_(True), gg.clone().view(1, 1).requires_grad_(True)
        (torch._weight_norm(vt, gt, 0) * dw.view(1, -1)).sum().backward()
        norm, dot = (v * v).sum().sqrt(), (dw * v).sum()
        dv, dg = got["dpar"][c.dv[r]: c.dv[r] + n], got["dpar"][c.dg[r]].view(1)
        same_pattern(dg, gt.grad.view(1), f"row {r} dg")
        same_pattern(dv, (gg / norm) * (dw - v * (dot / (norm * norm))), f"row {r} dv vs the formula in fp32")
        if r == 0:
            assert not bool(torch.isfinite(dv).any()) and not bool(torch.isfinite(vt.grad).any()), "‖v‖ = 0: dv is non-finite on both sides"
        else:
            same_pattern(dv, vt.grad.view(-1), f"row {r} dv vs fp32 torch autograd")


# --------------------------------------------------------------------------------------------------
# D. log|det W| and W⁻ᵀ
# --------------------------------------------------------------------------------------------------
def run_logdet(lib, W: torch.Tensor, what: str):
    n = W.shape[0]

    def go():
        k = Keep()
        b_out, out = out_buf((2,))
        b_inv, inv = out_buf((n, n))
        check_rc(lib.fst_logdet_inv(k(nan_in(W)), n, out.data_ptr(), inv.data_ptr(), stream()), what)
        sync()
        assert_fence(b_out, out, "out"), assert_fence(b_inv, inv, "inv_t")
        return dict(out=host(out), inv=host(inv))
    return repeat_equal(go, what)


def perm_parity(p):
    seen, sign = [False] * len(p), 1
    for i in range(len(p)):
        if not seen[i]:
            j, length = i, 0
            while not seen[j]:
                seen[j], j, length = True, p[j], length + 1
            sign *= -1 if length % 2 == 0 else 1
    return sign


def permutations_of(n: int):
    g = _gen(f"perm{n}")
    swap = list(range(n))
    swap[0], swap[n - 1] = swap[n - 1], swap[0]
    out = {"anti-diagonal": list(range(n - 1, -1, -1)), "transposition": swap}
    while len(out) < 4:
        p = torch.randperm(n, generator=g).tolist()
        out.setdefault("random even" if perm_parity(p) > 0 else "random odd", p)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 50, 96])
def test_logdet_of_permutations_is_exact(n):
    lib, g = _lib.load(), _gen(f"signed{n}")
    for name, p in permutations_of(n).items():
        W = torch.zeros(n, n, dtype=torch.float64)
        W[torch.arange(n), torch.tensor(p)] = 1.0
        par = perm_parity(p)
        got = run_logdet(lib, W, f"{name} permutation, n = {n}")
        assert float(got["out"][1]) == par, f"{name}, n = {n}: sign {float(got['out'][1])}, parity {par}"
        assert (float(got["out"][0]) == 0.0) if par > 0 else math.isnan(float(got["out"][0])), f"{name}, n = {n}: log|det| = {float(got['out'][0])}"
        assert same_bits(got["inv"], W.float()), f"{name}, n = {n}: W⁻ᵀ of a permutation is the permutation itself, bit for bit (zeros are +0)"
        # signed scaled: entries ±10^k, k in [−6, 6]
        d = (10.0 ** torch.randint(-6, 7, (n,), generator=g).double() * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)).float().double()
        Ws = torch.zeros(n, n, dtype=torch.float64)
        Ws[torch.arange(n), torch.tensor(p)] = d
        got = run_logdet(lib, Ws, f"signed scaled {name}, n = {n}")
        sign = par * int(torch.sign(d).prod())
        assert float(got["out"][1]) == sign, f"signed scaled {name}, n = {n}: sign {float(got['out'][1])} vs {sign}"
        ld = float(torch.log(d.abs()).sum())
        if sign > 0:
            assert float(got["out"][0]) == F32(ld) or abs(float(got["out"][0]) - ld) <= EPS32 * abs(ld) * 1.0000001 + 1e-12 * n, \
                f"signed scaled {name}, n = {n}: log|det| {float(got['out'][0])} vs {ld}"
        else:
            assert math.isnan(float(got["out"][0]))
        want = torch.zeros(n, n, dtype=torch.float64)
        want[torch.arange(n), torch.tensor(p)] = 1.0 / d
        assert same_bits(got["inv"], want.float()), f"signed scaled {name}, n = {n}: W⁻ᵀ is not the correctly rounded reciprocals"


def logdet_reference(W: torch.Tensor):
    a = W.numpy()
    sign, ld = np.linalg.slogdet(a)
    return float(sign), float(ld), torch.from_numpy(np.linalg.inv(a).T.copy())


@pytest.mark.gpu
def test_logdet_pivot_ties():
    """A column holding +a and −a at several rows: the pivot search must pick the same row every time (the lowest index)."""
    lib, g = _lib.load(), _gen("ties")
    n = 7
    W = r32(g, n, n)
    W[:, 0] = torch.tensor([2.5, -2.5, 2.5, 0.3, -2.5, 2.5, -2.5], dtype=torch.float64)
    W[2:, 1] = torch.tensor([1.75, -1.75, 0.1, 1.75, -1.75], dtype=torch.float64)
    got = run_logdet(lib, W, "pivot ties")
    sign, ld, inv_t = logdet_reference(W)
    assert float(got["out"][1]) == sign
    if sign > 0:
        assert abs(float(got["out"][0]) - ld) <= 1e-5 * max(1.0, abs(ld))
    assert_close(got["inv"], inv_t, 1e-5, "pivot ties: inv_t")


def hilbert_like(n: int) -> torch.Tensor:
    i = torch.arange(n, dtype=torch.float64)
    return (1.0 / (i.view(-1, 1) + i.view(1, -1) + 1.0)).float().double()          # fp32-rounded, then exact in fp64


def assert_ill_conditioned(inv_t, W, what: str):
    """The kernel eliminates in double: Gauss-Jordan with partial pivoting is backward stable up to a modest growth factor, so
    its inverse is off by about κ·n·2⁻⁵²·max|inv| before the result is rounded to fp32, which adds eps32·|inv| per element:
    |Δinv_ij| <= eps32·|inv_ij| + κ·n·2⁻⁵²·max|inv|.  W·inv_tᵀ − I then is bounded by Σ_k |W_ik|·|Δinv_kj| (plus the n·2⁻⁵²
    of forming the product in fp64).  An fp32 solver has κ·eps32 > 1 here and cannot be held to this — the companion test
    evaluates the bound for an fp64 solve rounded to fp32, which is what the kernel's arithmetic amounts to."""
    n = W.shape[0]
    _, _, ref = logdet_reference(W)
    kappa = float(np.linalg.cond(W.numpy()))
    bound = EPS32 * ref.abs() + kappa * n * 2.0 ** -52 * float(ref.abs().max())
    a = assert_within(inv_t, ref, bound, f"{what} inv_t (κ = {kappa:.2e})")
    resid = W @ inv_t.double().T - torch.eye(n, dtype=torch.float64)
    b = assert_within(resid, torch.zeros(n, n, dtype=torch.float64), W.abs() @ bound.T + n * 2.0 ** -52 * (W.abs() @ ref.abs().T), what + " W·inv_tᵀ − I")
    return max(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [6, 8])
def test_logdet_ill_conditioned(n):
    W = hilbert_like(n)
    got = run_logdet(_lib.load(), W, f"Hilbert-like n = {n}")
    sign, ld, _ = logdet_reference(W)
    assert float(got["out"][1]) == sign == 1.0
    assert abs(float(got["out"][0]) - ld) <= 2 * EPS32 * abs(ld) + 1e-9, f"log|det| {float(got['out'][0])} vs {ld}"
    assert_ill_conditioned(got["inv"], W, f"Hilbert-like n = {n}")


@pytest.mark.parametrize("n", [6, 8])
def test_logdet_ill_conditioned_bound_holds_for_an_fp64_solve_rounded_to_fp32(n):
    W = hilbert_like(n)
    assert_ill_conditioned(torch.linalg.inv(W).T.float(), W, f"fp64 torch rounded to fp32, Hilbert-like n = {n}")


@pytest.mark.gpu
def test_logdet_refusals_and_the_singular_case():
    lib = _lib.load()
    W = nan_in(torch.eye(4, dtype=torch.float64))
    for n in (0, 97):
        b_out, out = out_buf((2,))
        b_inv, inv = out_buf((4, 4))
        assert_refused(lib.fst_logdet_inv(W.data_ptr(), n, out.data_ptr(), inv.data_ptr(), stream()), lib, "fst_logdet_inv", f"n = {n}")
        sync()
        assert_untouched(b_out, out, f"n = {n}: out"), assert_untouched(b_inv, inv, f"n = {n}: inv_t")
    Ws = r32(_gen("singular"), 5, 5)
    Ws[:, 2] = 0.0                     # a zero column stays exactly zero under the elimination: the third pivot is an exact 0
    got = run_logdet(lib, Ws, "singular")
    assert float(got["out"][0]) == -math.inf and float(got["out"][1]) == 0.0 and bool(torch.isnan(got["inv"]).all())


# --------------------------------------------------------------------------------------------------
# E. NoiseTransfer, kernel by kernel
# --------------------------------------------------------------------------------------------------
SELU_ALPHA, SELU_SCALE = 1.6732632423543772, 1.0507009873554805
BCAST_CAP = 8192 * 256        # float4 one pass of fst_bcast_add / fst_noise_transfer_bwd_apply covers (8192 workgroups x 256): the
BIG_B, BIG_N = 129, 65_540    # grid-stride cases need B·N/4 beyond it — restated here so a changed cap cannot silently untest the loop


def ratio_args(mode: str, r_t: float, r_s: float, k: Keep):
    """(r_t_dev, r_s_dev, r_t, r_s): the ratios as host values, or as device scalars beside host values that must then be ignored."""
    if mode == "host":
        return None, None, r_t, r_s
    return k(nan_in(torch.tensor([r_t], dtype=torch.float64))), k(nan_in(torch.tensor([r_s], dtype=torch.float64))), 777.0, -777.0


@pytest.mark.gpu
@pytest.mark.parametrize("two", [False, True], ids=["x1 = NULL", "x0 and x1"])
@pytest.mark.parametrize("N", [4, 1028])                      # 1028 = 257 float4: the second workgroup holds one live thread
@pytest.mark.parametrize("B,S", [(1, 1), (7, 7), (7, 3), (33, 16)])       # S = 3 over 7 samples: slices of 2, 2 and 3
def test_batch_sum_slices(B, S, N, two):
    lib, g = _lib.load(), _gen(f"bsum{B}.{S}.{N}")
    xs = [r32(g, B, N, add=0.5) for _ in range(2 if two else 1)]
    what = f"batch_sum B{B} S{S} N{N}"

    def go():
        k = Keep()
        b_part, part = out_buf((len(xs), S, N))
        check_rc(lib.fst_batch_sum(k(nan_in(xs[0])), k(nan_in(xs[1])) if two else None, part.data_ptr(), B, N, S, stream()), what)
        sync()
        assert_fence(b_part, part, "part")
        return dict(part=host(part))
    got = repeat_equal(go, what)["part"]
    assert_written(got, what)
    for z, x in enumerate(xs):
        for s in range(S):
            rows = x[s * B // S: (s + 1) * B // S]                      # the kernel's slice: samples [⌊sB/S⌋, ⌊(s+1)B/S⌋)
            assert rows.shape[0] >= 1
            assert_within(got[z, s], rows.sum(0), 1e-5 * rows.abs().sum(0) + 1e-30, f"{what} tensor {z} slice {s}")


def nt_case(C: int, L: int, S_: int = 3, B: int = 7):
    g = _gen(f"nt{C}.{L}")
    N = C * L
    return dict(C=C, L=L, S=S_, B=B, part=r32(g, 2, S_, N, k=2.0), avg_t=r32(g, C, L), avg_s=r32(g, C, L), W=r32(g, C, C, k=1.0 / math.sqrt(C)),
                bias=r32(g, C, k=0.3), r_t=F32(0.7), r_s=F32(0.45), gpart=r32(g, S_, N), g=g)


def selu_f64(x):
    return SELU_SCALE * torch.where(x > 0, x, SELU_ALPHA * torch.expm1(x))


def selu_grad_f64(x):
    return SELU_SCALE * torch.where(x > 0, torch.ones_like(x), SELU_ALPHA * torch.exp(x))


def nt_forward_f64(c):
    B = float(c["B"])
    nt = c["avg_t"] + c["r_t"] * (c["part"][0].sum(0).view(c["C"], c["L"]) / B)
    ns = c["avg_s"] + c["r_s"] * (c["part"][1].sum(0).view(c["C"], c["L"]) / B)
    pre = c["W"] @ (nt - ns) + c["bias"].view(-1, 1)
    return nt, ns, nt - ns, pre, selu_f64(pre)


def run_nt_forward(lib, c, mode: str, what: str):
    C, L = c["C"], c["L"]

    def go():
        k = Keep()
        b_at, at = out_buf((C, L), init=c["avg_t"])
        b_as, as_ = out_buf((C, L), init=c["avg_s"])
        outs = [out_buf((C, L)) for _ in range(3)]
        rtd, rsd, rt, rs = ratio_args(mode, c["r_t"], c["r_s"], k)
        check_rc(lib.fst_noise_transfer_fwd(k(nan_in(c["part"])), c["S"], c["B"], rtd, rsd, rt, rs, at.data_ptr(), as_.data_ptr(), k(nan_in(c["W"])),
                                            k(nan_in(c["bias"])), outs[0][1].data_ptr(), outs[1][1].data_ptr(), outs[2][1].data_ptr(), C, L, stream()), what)
        sync()
        assert_fence(b_at, at, "avg_t"), assert_fence(b_as, as_, "avg_s")
        for (b_, v_), n_ in zip(outs, ("dist", "pre", "learned")):
            assert_fence(b_, v_, n_)
        return dict(avg_t=host(at), avg_s=host(as_), dist=host(outs[0][1]), pre=host(outs[1][1]), learned=host(outs[2][1]))
    got = repeat_equal(go, what)
    for n_ in got:
        assert_written(got[n_], f"{what} {n_}")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("C,L", [(1, 1), (5, 63), (6, 65), (50, 64), (200, 70)])       # C = 200: 51 200 bytes of LDS, past the 48 KiB default
def test_noise_transfer_forward_and_backward(C, L, mode):
    lib = _lib.load()
    c = nt_case(C, L)
    what = f"noise_transfer C{C} L{L} {mode} ratios"
    got = run_nt_forward(lib, c, mode, what)
    nt, ns, dist, pre, learned = nt_forward_f64(c)
    for name, want in (("avg_t", nt), ("avg_s", ns), ("dist", dist), ("pre", pre), ("learned", learned)):
        assert_close(got[name], want, OUT_TOL, f"{what} {name}")
    # backward from the forward's own pre: dpre = Σ_s gpart · selu'(pre), dd = Wᵀ·dpre
    pre32 = got["pre"].double()

    def go():
        k = Keep()
        b_dp, dp = out_buf((C, L))
        b_dd, dd = out_buf((C, L))
        check_rc(lib.fst_noise_transfer_bwd(k(nan_in(c["gpart"])), c["S"], k(nan_in(pre32)), k(nan_in(c["W"])), dp.data_ptr(), dd.data_ptr(), C, L, stream()), what)
        sync()
        assert_fence(b_dp, dp, "dpre"), assert_fence(b_dd, dd, "dd")
        return dict(dpre=host(dp), dd=host(dd))
    bw = repeat_equal(go, what + " bwd")
    assert_written(bw["dpre"], what + " dpre"), assert_written(bw["dd"], what + " dd")
    dpre = c["gpart"].sum(0).view(C, L) * selu_grad_f64(pre32)
    assert_close(bw["dpre"], dpre, GRAD_TOL, what + " dpre")
    assert_close(bw["dd"], c["W"].T @ dpre, GRAD_TOL, what + " dd")


SELU_POINTS = [-100.0, -20.0, -1e-8, 0.0, 1e-8, 20.0]


def assert_selu(pre, learned, dpre, what: str):
    """pre is forced (W = 0): it must BE the bias.  selu and selu' against fp64 within an absolute 4·eps32·scale·max(1, |x|) — a few
    roundings of a value of that size (expm1f / expf are good to 2 ulp of at most α).  selu'(0) is the x > 0 ? 1 : α·eˣ branch: scale·α."""
    x = torch.tensor(SELU_POINTS, dtype=torch.float64).float().double().view(-1, 1).expand(-1, pre.shape[1])
    assert torch.equal(pre.double(), x), f"{what}: pre is not the bias"
    bound = 4 * EPS32 * SELU_SCALE * x.abs().clamp_min(1.0)
    a = assert_within(learned, selu_f64(x), bound, what + " selu")
    b = assert_within(dpre, selu_grad_f64(x), bound, what + " selu'")
    at0 = dpre[SELU_POINTS.index(0.0)].double()
    assert bool(((at0 - SELU_SCALE * SELU_ALPHA).abs() <= 4 * EPS32 * SELU_SCALE * SELU_ALPHA).all()), f"{what}: selu'(0) = {float(at0[0])}"
    return max(a, b)


@pytest.mark.gpu
def test_noise_transfer_selu_at_forced_points():
    lib = _lib.load()
    C, L = len(SELU_POINTS), 5
    c = nt_case(C, L)
    c["W"], c["bias"] = torch.zeros(C, C, dtype=torch.float64), torch.tensor(SELU_POINTS, dtype=torch.float64).float().double()
    got = run_nt_forward(lib, c, "host", "selu points")
    k = Keep()
    b_dp, dp = out_buf((C, L))
    b_dd, dd = out_buf((C, L))
    ones = torch.ones(1, C * L, dtype=torch.float64)                     # S = 1, G = 1: dpre is selu'(pre) itself
    check_rc(lib.fst_noise_transfer_bwd(k(nan_in(ones)), 1, k(nan_in(got["pre"])), k(nan_in(c["W"])), dp.data_ptr(), dd.data_ptr(), C, L, stream()), "selu points")
    sync()
    assert_fence(b_dp, dp, "dpre"), assert_fence(b_dd, dd, "dd")
    assert_selu(got["pre"], got["learned"], host(dp), "selu points")
    assert bool((host(dd) == 0).all()), "dd = Wᵀ·dpre with W = 0"


def test_selu_bounds_hold_for_fp32_torch():
    x = torch.tensor(SELU_POINTS).view(-1, 1).expand(-1, 5)
    learned = np.float32(SELU_SCALE) * torch.where(x > 0, x, np.float32(SELU_ALPHA) * torch.expm1(x))
    dpre = np.float32(SELU_SCALE) * torch.where(x > 0, torch.ones_like(x), np.float32(SELU_ALPHA) * torch.exp(x))
    assert_selu(x, learned, dpre, "fp32 torch, selu points")


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3, 4, 5])                   # the bias row (c = C) falls to wave C mod 4
@pytest.mark.parametrize("L", [1, 63, 64, 65, 130])
def test_noise_transfer_dw(C, L):
    lib, g = _lib.load(), _gen(f"ntdw{C}.{L}")
    dpre, dist = r32(g, C, L), r32(g, C, L, add=0.3)
    what = f"noise_transfer_dw C{C} L{L}"

    def go():
        k = Keep()
        b_dw, dw = out_buf((C, C))
        b_db, db = out_buf((C,))
        check_rc(lib.fst_noise_transfer_dw(k(nan_in(dpre)), k(nan_in(dist)), dw.data_ptr(), db.data_ptr(), C, L, stream()), what)
        sync()
        assert_fence(b_dw, dw, "dW"), assert_fence(b_db, db, "dbias")
        return dict(dW=host(dw), dbias=host(db))
    got = repeat_equal(go, what)
    assert_written(got["dW"], what + " dW"), assert_written(got["dbias"], what + " dbias")
    assert_within(got["dW"], dpre @ dist.T, 1e-5 * (dpre.abs() @ dist.abs().T) + 1e-30, what + " dW")
    assert_within(got["dbias"], dpre.sum(1), 1e-5 * dpre.abs().sum(1) + 1e-30, what + " dbias")


def run_bwd_apply(lib, g_, dd, B, N, outs: str, mode: str, what: str):
    r_t, r_s = F32(0.7), F32(0.45)

    def go():
        k = Keep()
        b_t, dzt = out_buf((B, N))
        b_s, dzs = out_buf((B, N))
        rtd, rsd, rt, rs = ratio_args(mode, r_t, r_s, k)
        check_rc(lib.fst_noise_transfer_bwd_apply(k(nan_in(g_)), k(nan_in(dd)), rtd, rsd, rt, rs, B, dzt.data_ptr() if "t" in outs else None,
                                                  dzs.data_ptr() if "s" in outs else None, N, stream()), what)
        sync()
        assert_fence(b_t, dzt, "dz_t"), assert_fence(b_s, dzs, "dz_s")
        if "t" not in outs:
            assert_untouched(b_t, dzt, "dz_t (not passed)")
        if "s" not in outs:
            assert_untouched(b_s, dzs, "dz_s (not passed)")
        return dict(dz_t=host(dzt), dz_s=host(dzs))
    got = repeat_equal(go, what)
    # three roundings per element (ratio / B, the product, the difference): 1e-6 of the largest value, tighter than the suite's 2e-5
    if "t" in outs:
        assert_close(got["dz_t"], ((r_t / B) * dd).view(1, N).expand(B, N), 1e-6, what + " dz_t")
    if "s" in outs:
        assert_close(got["dz_s"], g_ - (r_s / B) * dd.view(1, N), 1e-6, what + " dz_s")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("outs", ["t", "s", "ts"], ids=["dz_s = NULL", "dz_t = NULL", "both"])
@pytest.mark.parametrize("B,N", [(1, 4), (7, 5 * 64), (3, 6 * 66)])
def test_noise_transfer_bwd_apply(B, N, outs, mode):
    g = _gen(f"ntapply{B}.{N}")
    run_bwd_apply(_lib.load(), r32(g, B, N), r32(g, N), B, N, outs, mode, f"bwd_apply B{B} N{N} {outs} {mode}")


@functools.lru_cache(maxsize=None)
def big_rows():
    assert BIG_B * BIG_N // 4 > BCAST_CAP, "the grid-stride cases no longer exceed what one pass covers"
    g = _gen("big")
    return r32(g, BIG_B, BIG_N), r32(g, BIG_N)


@pytest.mark.gpu
def test_noise_transfer_bwd_apply_grid_stride():
    x, v = big_rows()
    run_bwd_apply(_lib.load(), x, v, BIG_B, BIG_N, "ts", "host", "bwd_apply grid-stride")


@pytest.mark.gpu
def test_bcast_add_grid_stride():
    lib = _lib.load()
    x, v = big_rows()

    def go():
        k = Keep()
        b_out, out = out_buf((BIG_B, BIG_N))
        check_rc(lib.fst_bcast_add(out.data_ptr(), k(nan_in(x)), k(nan_in(v)), BIG_B, BIG_N, stream()), "bcast_add")
        sync()
        assert_fence(b_out, out, "out")
        return dict(out=host(out))
    got = repeat_equal(go, "bcast_add grid-stride")["out"]
    assert same_bits(got, (x + v.view(1, -1)).float()), "out = x + v is one correctly rounded addition per element"


NT_REFUSALS = ["batch_sum N % 4", "batch_sum S > B", "batch_sum misaligned x0", "fwd C > 512", "bwd C > 512", "bwd_apply both NULL",
               "bwd_apply N % 4", "bwd_apply misaligned dz_s", "bcast_add N % 4", "bcast_add misaligned out"]


@pytest.mark.gpu
@pytest.mark.parametrize("what", NT_REFUSALS)
def test_noise_transfer_refusals_write_nothing(what):
    lib, g = _lib.load(), _gen("nt-refusals")
    B, N = 4, 24
    x, v = nan_in(r32(g, B, N)), nan_in(r32(g, N))
    x_off = nan_in_off(r32(g, B, N), 1)
    outs = dict(a=out_buf((2, B, N)), b=out_buf((B, N)), c=out_buf((B, N)), off=shifted((B, N), CANARY, NAN, 1))
    pa, pb, pc, poff = (outs[n][1].data_ptr() for n in ("a", "b", "c", "off"))
    if what == "batch_sum N % 4":
        rc, who = lib.fst_batch_sum(x.data_ptr(), None, pa, B, N - 2, 2, stream()), "fst_batch_sum"
    elif what == "batch_sum S > B":
        rc, who = lib.fst_batch_sum(x.data_ptr(), None, pa, B, N, B + 1, stream()), "fst_batch_sum"
    elif what == "batch_sum misaligned x0":
        rc, who = lib.fst_batch_sum(x_off.data_ptr(), None, pa, B, N, 2, stream()), "fst_batch_sum"
    elif what == "fwd C > 512":
        rc, who = lib.fst_noise_transfer_fwd(x.data_ptr(), 1, B, None, None, 0.5, 0.5, pa, pb, v.data_ptr(), v.data_ptr(), pc, pc, pc, 513, 1, stream()), "fst_noise_transfer_fwd"
    elif what == "bwd C > 512":
        rc, who = lib.fst_noise_transfer_bwd(x.data_ptr(), 1, x.data_ptr(), v.data_ptr(), pb, pc, 513, 1, stream()), "fst_noise_transfer_bwd"
    elif what == "bwd_apply both NULL":
        rc, who = lib.fst_noise_transfer_bwd_apply(x.data_ptr(), v.data_ptr(), None, None, 0.5, 0.5, B, None, None, N, stream()), "fst_noise_transfer_bwd_apply"
    elif what == "bwd_apply N % 4":
        rc, who = lib.fst_noise_transfer_bwd_apply(x.data_ptr(), v.data_ptr(), None, None, 0.5, 0.5, B, pb, pc, N - 2, stream()), "fst_noise_transfer_bwd_apply"
    elif what == "bwd_apply misaligned dz_s":
        rc, who = lib.fst_noise_transfer_bwd_apply(x.data_ptr(), v.data_ptr(), None, None, 0.5, 0.5, B, pb, poff, N, stream()), "fst_noise_transfer_bwd_apply"
    elif what == "bcast_add N % 4":
        rc, who = lib.fst_bcast_add(pb, x.data_ptr(), v.data_ptr(), B, N - 2, stream()), "fst_bcast_add"
    else:
        rc, who = lib.fst_bcast_add(poff, x.data_ptr(), v.data_ptr(), B, N, stream()), "fst_bcast_add"
    assert_refused(rc, lib, who, what)
    sync()
    for k_, (buf, view) in outs.items():
        assert_untouched(buf, view, f"{what}: {k_}")


# --------------------------------------------------------------------------------------------------
# F(a, b). fst_mask_taps and fst_row_sum
# --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,C,K", [(1, 1, 1), (5, 3, 7), (130, 65, 64)])         # 540 800 elements > 2048 workgroups x 256: grid-stride
def test_mask_taps_is_exact(M, C, K):
    lib, g = _lib.load(), _gen(f"mask{M}.{C}.{K}")
    w = r32(g, M, C, K)
    lo = torch.randint(0, K + 1, (M,), generator=g)
    hi = torch.maximum(lo, torch.randint(0, K + 1, (M,), generator=g))
    lo[0], hi[0] = 0, K                                                 # a full range ...
    if M > 1:
        lo[1], hi[1] = K // 2, K // 2                                   # ... and an empty one (lo == hi)
    live = (torch.arange(K).view(1, 1, K) >= lo.view(M, 1, 1)) & (torch.arange(K).view(1, 1, K) < hi.view(M, 1, 1))
    want = torch.where(live, w, torch.zeros_like(w)).float()
    what = f"mask_taps M{M} C{C} K{K}"

    def go():
        k = Keep()
        b_w, wd = out_buf((M, C, K), init=w)
        check_rc(lib.fst_mask_taps(wd.data_ptr(), k(lo.to(torch.int32).to(DEV)), k(hi.to(torch.int32).to(DEV)), M, C, K, stream()), what)
        sync()
        assert_fence(b_w, wd, "w")
        return dict(w=host(wd))
    assert same_bits(repeat_equal(go, what)["w"], want), f"{what}: W ⊙ mask is exact"


@pytest.mark.gpu
@pytest.mark.parametrize("L", [4, 60, 5])                      # 16-byte path at two widths, dword path
def test_row_sum_of_a_channel_slice(L):
    lib, g = _lib.load(), _gen(f"rowsum{L}")
    B, C, extra = 17, 3, 2                                               # 17 rows: the second pass of the dword kernel's 16 waves
    x = r32(g, B, C, L, add=0.25)
    what = f"row_sum L{L}"

    def go():
        k = Keep()
        xd = nan_in(x, extra, 1)                                        # channels [1, 1 + C) of a [B, C + 2, L] block of NaN
        b_out, out = out_buf((C,))
        check_rc(lib.fst_row_sum(k(xd), (C + extra) * L, B, C, L, out.data_ptr(), stream()), what)
        sync()
        assert_fence(b_out, out, "out")
        return dict(out=host(out))
    got = repeat_equal(go, what)["out"]
    assert_within(got, x.sum(dim=(0, 2)), 1e-5 * x.abs().sum(dim=(0, 2)), what)
    b_out, out = out_buf((C,))
    xd = nan_in(x, extra, 1)
    assert_refused(lib.fst_row_sum(xd.data_ptr(), C * L - 1, B, C, L, out.data_ptr(), stream()), lib, "fst_row_sum", "batch stride < C·L")
    sync()
    assert_untouched(b_out, out, "row_sum refused: out")
