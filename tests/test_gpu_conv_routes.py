"""Every kernel instance of the conv engine (csrc/conv_engine.hip) against an fp64 reference, at the edges where it could go wrong.

Each case calls ``ops.conv_gemm`` / ``ops.conv_wgrad`` directly with a plan built for the wanted MB and an explicit NB, so no
launch depends on the batch-size heuristics, and asserts through ``fst_conv_last_route`` (the library's own record of the
launch) that the intended instance and epilogue ran.  Inputs sit inside NaN guard bands (storage in front of and behind
them, and extra channels when the batch stride is larger than C·L): a kernel that reads one sample outside its rows turns the
result into NaN.  Outputs sit inside canary bands that must stay untouched.  Every non-atomic launch is repeated and must
be bit-identical.  Gates: 2e-5 of the output scale forward, 1e-4 for weight gradients (tests/test_gpu_kernels.py).

The forward cases name the instance they pin, not an arithmetic: the split-bf16 families (conv_gemm_bf3_kernel,
conv_win_bf3_kernel, conv_win_rows_kernel) are launched with the FST_GEMM_BF16X3 flag, the f32 families without it, whatever
FST_MATH says.  The weight-gradient cases set ``ops.MATH`` to the arithmetic of the instance they pin.

``test_every_instance_is_covered`` runs without a GPU: it reads the pickers of conv_engine.hip and fails when an instance
exists that no case here pins.
"""
from __future__ import annotations

import itertools
import os
import re
import zlib
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import pytest
import torch
import torch.nn.functional as F

from feature_level_style_transfer_for_tsc_amd import ops
from feature_level_style_transfer_for_tsc_amd.plan import Segment, build_plan

DEV = "cuda"
CANARY = -4242.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = os.path.join(ROOT, "feature_level_style_transfer_for_tsc_amd", "csrc", "conv_engine.hip")

GEMM, PIPE, BF3, WIN, ROWS, WGRAD = ops.ROUTE_GEMM, ops.ROUTE_PIPE, ops.ROUTE_BF3, ops.ROUTE_WIN_BF3, ops.ROUTE_WIN_ROWS, ops.ROUTE_WGRAD
FAMILY_NAME = {GEMM: "gemm", PIPE: "pipe", BF3: "bf3", WIN: "win", ROWS: "rows", WGRAD: "wgrad"}


def assert_close(got, want, tol, what=""):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    scale = max(1e-6, float(want.abs().max()))
    err = float((got - want).abs().max())
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def guarded(B: int, C: int, L: int, fill: float, front: int = 4, extra: int = 0, row0: int = 0):
    """(buffer, view): a [B, C, L] view with channel stride L and batch stride (C + extra)·L, channels [row0, row0 + C) of each
    sample, inside a flat buffer filled with ``fill``; ``front`` floats of it before the first sample (4: 16-byte aligned,
    5: 4 bytes off), 8 behind the last."""
    bs = (C + extra) * L
    buf = torch.full((front + B * bs + 8,), fill, device=DEV, dtype=torch.float32)
    return buf, buf[front: front + B * bs].view(B, C + extra, L)[:, row0: row0 + C]


def assert_band_untouched(buf: torch.Tensor, view: torch.Tensor, what: str):
    """Everything of ``buf`` outside ``view`` still holds the canary."""
    probe = buf.clone()
    probe.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(CANARY)
    bad = int((probe != CANARY).sum())
    assert bad == 0, f"{what}: {bad} elements outside the output were written"


def ref_conv(x: torch.Tensor, w: torch.Tensor, dil: int, pad_left: int) -> torch.Tensor:
    """y[b,m,t] = Σ_{c,k} w[m,c,k]·x[b,c,t + k·dil − pad_left], zero outside [0, L), in fp64."""
    halo = (w.size(2) - 1) * dil
    return F.conv1d(F.pad(x.double(), (pad_left, halo - pad_left)), w.double(), dilation=dil)


def omni_live(M: int, ntaps: int) -> list:
    """Omni-scale style live tap ranges: centred on the middle tap, widening with the row index (so with the M-group)."""
    c = ntaps // 2
    return [(c - m * (c + 1) // M, c + m * (c + 1) // M + 1) for m in range(M)]


# --------------------------------------------------------------------------------------------------
# forward / data-gradient instances
# --------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Fwd:
    fam: int
    MB: int
    NB: int
    VEC: int            # conv_gemm_pipe_kernel's VEC; 0 for the other families
    M: int
    C0: int
    ntaps: int
    dil: int
    pad_left: int
    L: int
    B: int = 2
    C1: int = 0         # second input: one tap (ntaps // 2) of C1 channels
    extra: int = 0      # guard channels per sample around the input / output rows: batch stride > C·L
    xfront: int = 4     # 5: input base 4 bytes off a 16-byte boundary
    epi: str = "plain"  # plain relu res acc1 acc2 atomic
    wide: bool = False  # the 16-byte epilogue (needs L % 4 == 0); False: the dword form
    omni: bool = False  # omni-scale row_live masks
    bias: bool = True
    ksplit: int = 1
    chunk_c: int = 16

    @property
    def id(self) -> str:
        inst = "rows" if self.fam == ROWS else f"{FAMILY_NAME[self.fam]}{self.MB}x{self.NB}" + ("v" if self.VEC else "") * (self.fam == PIPE)
        return (f"{inst}-{self.epi}{'16' if self.wide else '4'}-M{self.M}C{self.C0}k{self.ntaps}d{self.dil}p{self.pad_left}"
                f"-B{self.B}L{self.L}" + (f"x1_{self.C1}" if self.C1 else "") + ("-omni" if self.omni else "") +
                (f"-ks{self.ksplit}" if self.ksplit > 1 else "") + ("-mis" if self.xfront % 4 else "") +
                ("-nobias" if not self.bias else ""))

    @property
    def bf3(self) -> bool:
        return self.fam in (BF3, WIN, ROWS)

    @property
    def instance(self) -> str:
        return ops.route_kernel_name(self.route[:6] + (0, 0))

    @property
    def epi_mode(self) -> int:
        if self.epi == "atomic":
            return ops.ROUTE_EPI_ATOMIC
        add = self.epi in ("res", "acc1", "acc2")
        if self.wide:
            return ops.ROUTE_EPI_VEC_ADD if add else ops.ROUTE_EPI_VEC
        return ops.ROUTE_EPI_ADD if add else ops.ROUTE_EPI_PLAIN

    @property
    def route(self) -> Tuple[int, ...]:
        if self.fam == ROWS:
            return (ROWS, 0, 0, 0, 0, 0, self.epi_mode, self.ksplit)
        return (self.fam, self.MB, self.NB, self.VEC, 0, 0, self.epi_mode, self.ksplit)

    @property
    def x1_tap(self) -> int:
        return self.ntaps // 2

    def plan(self):
        segs = [Segment(0, self.C0, 0, self.ntaps)]
        if self.C1:
            segs.append(Segment(1, self.C1, self.x1_tap, self.x1_tap + 1))
        split = self.fam in (PIPE, BF3)
        live = omni_live(self.M, self.ntaps) if self.omni else None
        return build_plan(self.M, segs, self.ntaps, self.dil, self.pad_left, MB=1 if self.fam == ROWS else self.MB,
                          chunk_c=self.chunk_c, split_taps=split, row_live=live)

    def splits(self) -> Tuple[int, int]:
        """(msplit, m2_start)"""
        if self.epi == "res":
            return self.M // 2 + 3, self.M // 2 + 3
        if self.epi == "acc2":
            return self.M // 3, self.M // 3 + 7
        return self.M, self.M


def _tile_l(NB: int, r: int) -> int:
    return 128 * NB + r


# geometry pools: (C0, ntaps, dil, pad_left, C1, B, extra, L(NB) or None for the NB default, omni)
_WIN_GEOS = [
    (12, 5, 1, 2, 0, 2, 2, lambda nb: _tile_l(nb, 84), False),     # centred taps, batch stride > C·L, partial last tile
    (20, 4, 1, 0, 5, 1, 0, lambda nb: _tile_l(nb, 61), False),     # pad_left 0: taps run off the right end; x1; L % 4 != 0
    (9, 3, 30, 60, 0, 3, 1, lambda nb: 52, False),                 # dilation 30 > L/2, pad_left = (ntaps-1)·dil: off the left end
    (16, 7, 1, 3, 3, 2, 1, lambda nb: _tile_l(nb, 84), True),      # omni-scale masks, x1
]
_PIPE_GEOS = [
    (24, 1, 1, 0, 0, 2, 1, lambda nb: _tile_l(nb, 84), False),     # 1x1, two 16-channel chunks (8 + 16 of them padded)
    (10, 3, 8, 8, 6, 1, 0, lambda nb: _tile_l(nb, 116), False),    # shifts -8 / 0 / +8, x1
    (7, 3, 40, 0, 0, 3, 2, lambda nb: 60, False),                  # dilation 40 > L/2, pad_left 0; odd channel count
    (12, 3, 4, 8, 0, 2, 1, lambda nb: _tile_l(nb, 4), False),      # pad_left = (ntaps-1)·dil
    (18, 2, 3, 3, 0, 2, 0, lambda nb: _tile_l(nb, 84), False),     # shifts -3 / 0: not a multiple of 4 (no 16-byte staging)
    (5, 3, 2, 2, 4, 1, 1, lambda nb: _tile_l(nb, 45), False),      # L % 4 != 0
]


def _vec_geo(g) -> bool:
    """The geometry allows 16-byte loads of the input (pipe VEC): shifts and L multiples of 4."""
    C0, ntaps, dil, pad, C1, B, extra, Lf, omni = g
    return pad % 4 == 0 and (ntaps == 1 or dil % 4 == 0) and Lf(1) % 4 == 0 and Lf(2) % 4 == 0


def _make(fam, MB, NB, VEC, g, **kw) -> Fwd:
    C0, ntaps, dil, pad, C1, B, extra, Lf, omni = g
    R = 32 * MB
    M = kw.pop("M", R + 13 * MB + 3 if MB < 8 else R + 37)          # two M-groups, the last one partial
    return Fwd(fam, MB, NB, VEC, M, C0, ntaps, dil, pad, Lf(NB), B, C1, extra, omni=omni, **kw)


# (epilogue, 16-byte form) each family runs besides plain; atomic has only the dword form
_EPIS = [("relu", True), ("relu", False), ("res", True), ("res", False), ("acc1", True), ("acc1", False),
         ("acc2", True), ("acc2", False), ("atomic", False)]


def _family_cases(fam, insts, geos, fits):
    """Every instance of a family plain, then every epilogue on some instance of it; ``fits(inst, geo)`` picks geometries."""
    out = []
    for i, inst in enumerate(insts):
        g = [g for g in itertools.islice(itertools.cycle(geos), i, i + len(geos)) if fits(inst, g, False)][0]
        L = g[7](inst[1])
        out.append(_fix(_make(fam, *inst, g, wide=(L % 4 == 0 and i % 2 == 0), bias=i % 3 != 2)))
    for j, (epi, wide) in enumerate(_EPIS):
        for step in range(len(insts) * len(geos)):
            inst = insts[(3 * j + 1 + step) % len(insts)]
            g = geos[(j + step) % len(geos)]
            if fits(inst, g, wide) and (epi != "atomic" or _n_chunks(fam, inst, g) >= 2):
                break
        ks = min(3, _n_chunks(fam, inst, g)) if epi == "atomic" else 1
        out.append(_fix(_make(fam, *inst, g, epi=epi, wide=wide, ksplit=ks)))
    return out


def _n_chunks(fam, inst, g) -> int:
    return _make(fam, *inst, g).plan().n_chunks


def _fix(c: Fwd) -> Fwd:
    """Input alignment the instance needs: pipe VEC=false on a 16-byte-capable geometry gets a base 4 bytes off."""
    if c.fam == PIPE and not c.VEC and _vec_geo((c.C0, c.ntaps, c.dil, c.pad_left, c.C1, c.B, c.extra, lambda nb: c.L, c.omni)):
        return replace(c, xfront=5)
    return c


GEMM_INSTS = [(1, 1, 0), (2, 1, 0), (4, 1, 0), (8, 1, 0), (1, 2, 0), (2, 2, 0), (4, 2, 0), (1, 4, 0), (2, 4, 0)]
PIPE_INSTS = [(mb, nb, v) for v in (1, 0) for (mb, nb) in ((1, 1), (2, 1), (4, 1), (8, 1), (1, 2), (2, 2), (4, 2))]
BF3_INSTS = [(1, 1, 0), (2, 1, 0), (4, 1, 0), (8, 1, 0), (1, 2, 0), (2, 2, 0), (4, 2, 0)]
WIN_INSTS = [(1, 1, 0), (2, 1, 0), (4, 1, 0), (1, 2, 0), (2, 2, 0), (1, 4, 0)]


def _fits_any(inst, g, wide):
    return not wide or g[7](inst[1]) % 4 == 0


def _fits_pipe(inst, g, wide):
    return _fits_any(inst, g, wide) and (_vec_geo(g) if inst[2] else True)


def _fits_bf3(inst, g, wide):
    return g[7](inst[1]) % 4 == 0                                     # split-bf16 stages: L % 4 == 0, aligned inputs


FWD_CASES = (_family_cases(GEMM, GEMM_INSTS, _WIN_GEOS, _fits_any) +
             [Fwd(GEMM, 2, 1, 0, 77, 40, 1, 1, 0, 150, B=2, extra=1, chunk_c=32),         # 1x1 with 32-channel chunks: not pipeable
              Fwd(GEMM, 8, 1, 0, 300, 40, 2, 1, 1, 212, B=1, chunk_c=32, epi="atomic", ksplit=2)] +
             _family_cases(PIPE, PIPE_INSTS, _PIPE_GEOS, _fits_pipe) +
             _family_cases(BF3, BF3_INSTS, _PIPE_GEOS, _fits_bf3) +
             _family_cases(WIN, WIN_INSTS, _WIN_GEOS, _fits_any))

# conv_win_rows_kernel: 32-row M-groups (MB = 1), NB = 2, resident windows, >= 4 M-groups, plain stores.  Wave w takes groups
# 4i + w / 4i + 3 - w: group counts 4, 5, 6, 7 and 10 leave different waves idle in the last round.
ROWS_CASES = [
    Fwd(ROWS, 1, 2, 0, 100, 12, 5, 1, 2, 340, B=2, extra=1, wide=True),                # 4 groups
    Fwd(ROWS, 1, 2, 0, 150, 16, 9, 1, 4, 317, B=1, omni=True),                         # 5 groups, L % 4 != 0, omni
    Fwd(ROWS, 1, 2, 0, 180, 20, 7, 1, 3, 276, B=2, omni=True, wide=True, C1=3),        # 6 groups, two chunks + x1, omni
    Fwd(ROWS, 1, 2, 0, 220, 9, 3, 40, 80, 60, B=3, extra=2, epi="relu", wide=True),    # 7 groups, dilation 40 > L/2
    Fwd(ROWS, 1, 2, 0, 300, 14, 11, 1, 0, 512, B=2, omni=True, epi="relu"),            # 10 groups, pad_left 0
    Fwd(ROWS, 1, 2, 0, 290, 8, 6, 1, 5, 260, B=1, bias=False),                         # 10 groups, last one 2 rows
]
# the same plans with an epilogue the rows kernel does not have: conv_win_bf3_kernel<1, 2>
ROWS_FALLBACK = [replace(ROWS_CASES[1], fam=WIN, epi="res"), replace(ROWS_CASES[2], fam=WIN, epi="acc1", wide=True),
                 replace(ROWS_CASES[0], fam=WIN, epi="acc2", wide=False), replace(ROWS_CASES[4], fam=WIN, epi="atomic"),
                 replace(ROWS_CASES[2], fam=WIN, epi="atomic", ksplit=2, wide=False)]
FWD_CASES += ROWS_CASES + ROWS_FALLBACK


def _run_fwd(c: Fwd, plan, a, x0, x1, bias, init):
    """One launch on fresh output buffers initialised from ``init``; returns {name: (buffer, view)} of the outputs."""
    msplit, m2 = c.splits()
    ofront = 4 if c.wide else 5 if c.L % 4 == 0 else 4
    outs = {}
    if msplit > 0:
        outs["y"] = guarded(c.B, msplit, c.L, CANARY, ofront, c.extra, row0=min(1, c.extra))
    if msplit < c.M:
        outs["y2"] = guarded(c.B, c.M - m2, c.L, CANARY, 4, c.extra)
    for k, v in init.items():
        if k in outs:
            outs[k][1].copy_(v)
    flags = {"relu": ops.EPI_RELU, "acc1": ops.EPI_ACC1, "acc2": ops.EPI_ACC2, "atomic": ops.EPI_ATOMIC}.get(c.epi, 0)
    ops.conv_gemm(plan, a, x0, x1, bias, c.B, c.L, c.M, outs["y"][1] if "y" in outs else None, res=init.get("res"),
                  y2=outs["y2"][1] if "y2" in outs else None, msplit=msplit, nb=c.NB, ksplit=c.ksplit, flags=flags, m2_start=m2,
                  bf3=c.bf3)
    route = ops.last_route()
    assert route == c.route, f"launched {ops.route_kernel_name(route)} epi={route[6]} ksplit={route[7]}, wanted {c.instance} {c.route}"
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("c", FWD_CASES, ids=lambda c: c.id)
def test_forward_instance_vs_fp64(c: Fwd):
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    plan = c.plan()
    w0 = torch.randn(c.M, c.C0, c.ntaps, generator=g, dtype=torch.float64) / (c.C0 * c.ntaps) ** 0.5
    if c.omni:
        mask = torch.zeros_like(w0)
        for m, (lo, hi) in enumerate(omni_live(c.M, c.ntaps)):
            mask[m, :, lo:hi] = 1
        w0 = w0 * mask
    x0 = torch.randn(c.B, c.C0, c.L, generator=g, dtype=torch.float64)
    want = ref_conv(x0, w0, c.dil, c.pad_left)
    w1 = x1 = None
    if c.C1:
        w1 = torch.randn(c.M, c.C1, generator=g, dtype=torch.float64) / c.C1 ** 0.5
        x1 = torch.randn(c.B, c.C1, c.L, generator=g, dtype=torch.float64)
        w1full = torch.zeros(c.M, c.C1, c.ntaps, dtype=torch.float64)
        w1full[:, :, c.x1_tap] = w1
        want = want + ref_conv(x1, w1full, c.dil, c.pad_left)
    bias = torch.randn(c.M, generator=g, dtype=torch.float64) if c.bias else None
    if bias is not None:
        want = want + bias[None, :, None]

    xbuf0, x0d = guarded(c.B, c.C0, c.L, float("nan"), c.xfront, c.extra, row0=min(1, c.extra))
    x0d.copy_(x0)
    x1d = None
    if c.C1:
        _, x1d = guarded(c.B, c.C1, c.L, float("nan"), c.xfront, c.extra)
        x1d.copy_(x1)
    a = ops.pack_weights(plan, c.M, w0.float().to(DEV), (0, c.C0 * c.ntaps, c.ntaps, 1),
                         None if w1 is None else w1.float().to(DEV), (0, c.C1, 1, 0), bf3=c.bf3)
    bd = None if bias is None else bias.float().to(DEV)

    msplit, m2 = c.splits()
    init, res = {}, None
    if c.epi in ("acc1", "atomic"):
        init["y"] = torch.randn(c.B, msplit, c.L, generator=g)
    if c.epi == "acc2":
        init["y2"] = torch.randn(c.B, c.M - m2, c.L, generator=g)
    if c.epi == "res":
        res = torch.randn(c.B, msplit, c.L, generator=g)
    dev_init = {k: v.to(DEV) for k, v in init.items()}
    if res is not None:
        _, rd = guarded(c.B, msplit, c.L, float("nan"), 4 if c.wide else 5 if c.L % 4 == 0 else 4, c.extra)
        rd.copy_(res)
        dev_init["res"] = rd

    outs = _run_fwd(c, plan, a, x0d, x1d, bd, dev_init)
    want_y, want_y2 = want[:, :msplit], want[:, m2:]
    if c.epi == "relu":
        want_y = want_y.clamp_min(0)
    if c.epi == "res":
        want_y = want_y + res.double()
    if c.epi in ("acc1", "atomic"):
        want_y = want_y + init["y"].double()
    if c.epi == "acc2":
        want_y2 = want_y2 + init["y2"].double()
    if "y" in outs:
        assert_close(outs["y"][1], want_y, 2e-5, f"{c.id} y")
        assert_band_untouched(*outs["y"], f"{c.id} y")
    if "y2" in outs:
        assert_close(outs["y2"][1], want_y2, 2e-5, f"{c.id} y2")
        assert_band_untouched(*outs["y2"], f"{c.id} y2")

    if c.epi != "atomic":                                          # (atomic K slices add in any order)
        again = _run_fwd(c, plan, a, x0d, x1d, bd, dev_init)
        for k in outs:
            assert torch.equal(outs[k][0], again[k][0]), f"{c.id}: {k} differs between two identical launches"


# --------------------------------------------------------------------------------------------------
# weight-gradient instances
# --------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Wg:
    CB: int             # 1: M <= 128 (plan MB 4), 2: M > 128 (MB 8)
    wide: bool
    VEC: int
    bf3: bool
    M: int
    C0: int
    ntaps: int
    dil: int
    pad_left: int
    L: int
    B: int = 2
    C1: int = 0
    xfront: int = 4
    extra: int = 0
    msplit: Optional[int] = None    # dy rows [0, msplit), dy2 rows [msplit, M)
    mul: bool = False               # x0_mul_off: the x operand is x0[i]·x0[i + C0·L]
    ksplit: Optional[int] = None    # None: ops.wgrad_ksplit

    @property
    def id(self) -> str:
        return (f"cb{self.CB}{'wide' if self.wide else 'narrow'}v{self.VEC}{'bf3' if self.bf3 else 'f32'}-M{self.M}C{self.C0}"
                f"k{self.ntaps}d{self.dil}p{self.pad_left}-B{self.B}L{self.L}" + (f"x1_{self.C1}" if self.C1 else "") +
                (f"-ms{self.msplit}" if self.msplit is not None else "") + ("-mul" if self.mul else "") +
                (f"-ks{self.ksplit}" if self.ksplit else "") + ("-mis" if self.xfront % 4 else ""))

    @property
    def route(self) -> Tuple[int, ...]:
        return (WGRAD, self.CB, 32, int(self.wide), self.VEC, int(self.bf3), -1)

    @property
    def instance(self) -> str:
        return ops.route_kernel_name(self.route + (0,))


def _wg_cases():
    out = []
    for CB, bf3 in itertools.product((1, 2), (False, True)):
        M = 100 if CB == 1 else 150
        M2 = 120 if CB == 1 else 250
        out += [
            # wide, VEC 1: windows start on a multiple of 4 samples (pad 4 of 5 taps) and are 4 wide past the tile
            Wg(CB, True, 1, bf3, M, 20, 5, 1, 4, 256, B=2, extra=1),
            # wide, VEC 0 with 16-byte aligned tensors: the windows start 2 samples off a multiple of 4
            Wg(CB, True, 0, bf3, M2, 40, 5, 1, 2, 128, B=1, msplit=M2 // 4 * 2),
            # narrow, VEC 2: tap shifts -1 / 0 / +1; x1; fewer (b,t) tiles than the requested K split
            Wg(CB, False, 2, bf3, M, 24, 3, 1, 1, 96, B=2, C1=7, extra=2, ksplit=1000),
            # narrow, VEC 1: shifts -4 / 0 / +4 (and the product operand on a 1x1 case below)
            Wg(CB, False, 1, bf3, M2, 36, 3, 4, 4, 164, B=3, msplit=40),
            # narrow, VEC 0: a base 4 bytes off 16
            Wg(CB, False, 0, bf3, M, 33, 2, 5, 5, 100, B=2, xfront=5, C1=4),
        ]
    out += [
        Wg(1, False, 1, True, 66, 34, 1, 1, 0, 132, B=2, mul=True),
        Wg(2, False, 1, False, 250, 40, 1, 1, 0, 64, B=3, mul=True, msplit=124),
        Wg(1, True, 0, True, 90, 12, 9, 1, 4, 77, B=3, ksplit=64),            # wide, L % 4 != 0, ksplit > tiles
        Wg(2, False, 0, False, 140, 10, 3, 2, 0, 61, B=1, ksplit=7),          # narrow, L % 4 != 0, pad_left 0
        Wg(1, True, 1, False, 64, 70, 5, 1, 0, 200, B=2, C1=9),                # wide with x1, two 64-channel windows
    ]
    return out


WG_CASES = _wg_cases()


def _wg_reference(c: Wg, x0, x1, dy, x1_tap: int):
    halo = (c.ntaps - 1) * c.dil
    xp = F.pad(x0, (c.pad_left, halo - c.pad_left))
    xcol = torch.stack([xp[:, :, k * c.dil: k * c.dil + c.L] for k in range(c.ntaps)], dim=2)       # [B, C, K, L]
    dw0 = torch.einsum("bml,bckl->mck", dy, xcol)
    dw1 = None
    if c.C1:
        s = x1_tap * c.dil - c.pad_left                                                           # the x1 tap's shift (0)
        x1s = F.pad(x1, (max(0, -s), max(0, s)))[:, :, max(0, s): max(0, s) + c.L]
        dw1 = torch.einsum("bml,bcl->mc", dy, x1s)[:, :, None]
    return dw0, dw1


@pytest.mark.gpu
@pytest.mark.parametrize("c", WG_CASES, ids=lambda c: c.id)
def test_weight_gradient_instance_vs_fp64(c: Wg, monkeypatch):
    monkeypatch.setattr(ops, "MATH", "bf16x3" if c.bf3 else "f32")
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    spec = ops.ConvSpec(c.M, c.C0, c.ntaps, c.dil, c.pad_left, C1=c.C1)
    plan = spec.wg_plan()
    x0 = torch.randn(c.B, c.C0, c.L, generator=g, dtype=torch.float64)
    x1 = torch.randn(c.B, c.C1, c.L, generator=g, dtype=torch.float64) if c.C1 else None
    dy = torch.randn(c.B, c.M, c.L, generator=g, dtype=torch.float64)
    if c.mul:
        s = torch.randn(c.B, c.C0, c.L, generator=g, dtype=torch.float64)
        _, tsd = guarded(c.B, 2 * c.C0, c.L, float("nan"), c.xfront)
        tsd.copy_(torch.cat([x0, s], dim=1))
        x0d, operand = tsd[:, :c.C0], x0 * s
    else:
        _, x0d = guarded(c.B, c.C0, c.L, float("nan"), c.xfront, c.extra, row0=min(1, c.extra))
        x0d.copy_(x0)
        operand = x0
    x1d = None
    if c.C1:
        _, x1d = guarded(c.B, c.C1, c.L, float("nan"), c.xfront, c.extra)
        x1d.copy_(x1)
    msplit = c.M if c.msplit is None else c.msplit
    _, dyd = guarded(c.B, msplit, c.L, float("nan"), c.xfront, c.extra)
    dyd.copy_(dy[:, :msplit])
    dy2d = None
    if msplit < c.M:
        _, dy2d = guarded(c.B, c.M - msplit, c.L, float("nan"), 4, c.extra)
        dy2d.copy_(dy[:, msplit:])
    n_wg = max(1, len(plan.items()) // 4)
    ksplit = c.ksplit if c.ksplit is not None else ops.wgrad_ksplit(c.B, c.L, n_wg)
    tiles = c.B * ((c.L + 31) // 32)
    want0, want1 = _wg_reference(c, operand, x1, dy, spec.x1_tap)

    def run():
        da = ops.conv_wgrad(plan, x0d, x1d, dyd, dy2d, msplit, c.B, c.L, c.M, ksplit, c.C0 * c.L if c.mul else 0)
        route = ops.last_route()
        assert route[:7] == c.route, f"launched {ops.route_kernel_name(route)}, wanted {c.instance}"
        assert route[7] == min(ksplit, tiles) == da.size(0), \
            f"library K split {route[7]} vs {da.size(0)} slabs allocated (requested {ksplit}, {tiles} tiles)"
        dw0 = torch.full((c.M, c.C0, c.ntaps), float("nan"), device=DEV)
        dw1 = torch.full((c.M, c.C1, 1), float("nan"), device=DEV) if c.C1 else None
        ops.unpack_weights(plan, c.M, da, dw0, spec.s_w0(), dw1, spec.s_w1())
        return da, dw0, dw1

    da, dw0, dw1 = run()
    assert_close(dw0, want0, 1e-4, f"{c.id} dw0")
    if c.C1:
        assert_close(dw1, want1, 1e-4, f"{c.id} dw1")
    da2, _, _ = run()
    assert torch.equal(da, da2), f"{c.id}: partial-sum slabs differ between two identical launches"


# --------------------------------------------------------------------------------------------------
# completeness (no GPU): every instance the launchers can pick has a case above
# --------------------------------------------------------------------------------------------------
def _engine_forward_instances() -> set:
    text = open(ENGINE).read()
    found = set()
    for fn in re.finditer(r"static conv_gemm_fn (pick_conv_\w+)\(int MB, int NB\) \{(.*?)\n\}", text, re.S):
        for name, args in re.findall(r"return (conv_\w+_kernel)<([^>]*)>;", fn.group(2)):
            args = [a.strip() for a in args.split(",")]
            for vec in (("true", "false") if "VEC" in args else (None,)):
                found.add(f"{name}<{', '.join(vec if a == 'VEC' else a for a in args)}>")
    assert re.search(r"fn = conv_win_rows_kernel;", text), "the launcher no longer dispatches conv_win_rows_kernel"
    return found | {"conv_win_rows_kernel"}


def _engine_wgrad_instances() -> set:
    text = open(ENGINE).read()
    macro = re.search(r"#define FST_WGRAD_PICK\(CBV, BF\)(.*?)\n  if \(bf3\)", text, re.S).group(1)
    shapes = re.findall(r"conv_wgrad_kernel<CBV, TW, (true|false), (\d), BF>", macro)
    uses = re.findall(r"FST_WGRAD_PICK\((\d), (true|false)\)", text)
    assert len(shapes) == 5 and len(uses) == 4, (shapes, uses)
    return {f"conv_wgrad_kernel<{cb}, 32, {wide}, {vec}, {bf}>" for (wide, vec), (cb, bf) in itertools.product(shapes, uses)}


def test_every_instance_is_covered():
    fwd = _engine_forward_instances()
    assert len(fwd) == 37, sorted(fwd)
    covered = {c.instance for c in FWD_CASES}
    assert covered == fwd, f"not covered: {sorted(fwd - covered)}; not an instance: {sorted(covered - fwd)}"
    wg = _engine_wgrad_instances()
    assert len(wg) == 20, sorted(wg)
    covered = {c.instance for c in WG_CASES}
    assert covered == wg, f"not covered: {sorted(wg - covered)}; not an instance: {sorted(covered - wg)}"


def test_every_family_sees_every_epilogue():
    """plain on every instance; ReLU, res, ACC1, ACC2 in both widths and ATOMIC (K split, bias) on some instance of each family."""
    for fam in (GEMM, PIPE, BF3, WIN):
        cs = [c for c in FWD_CASES if c.fam == fam]
        seen = {(c.epi, c.wide) for c in cs}
        for epi, wide in _EPIS:
            assert (epi, wide) in seen, (FAMILY_NAME[fam], epi, wide)
        assert any(c.epi == "atomic" and c.ksplit > 1 and c.bias for c in cs), FAMILY_NAME[fam]
        assert {c.instance for c in cs if c.epi == "plain"} == {c.instance for c in cs}, FAMILY_NAME[fam]
    rows = [c for c in FWD_CASES if c.fam == ROWS]
    assert {c.M // 32 + (c.M % 32 > 0) for c in rows} >= {4, 5, 6, 7, 10}
    assert {(c.epi, c.wide) for c in rows} >= {("plain", True), ("plain", False), ("relu", True), ("relu", False)}
    assert any(c.ksplit and c.ksplit > c.B * ((c.L + 31) // 32) for c in WG_CASES)     # the library clamps the K split
    assert any(c.mul for c in WG_CASES) and any(c.C1 for c in WG_CASES) and any(c.msplit is not None for c in WG_CASES)
    for c in FWD_CASES:
        assert not c.wide or c.L % 4 == 0, c.id
        assert c.epi != "atomic" or (c.ksplit <= c.plan().n_chunks and (c.fam == WIN or c.ksplit > 1)), c.id
