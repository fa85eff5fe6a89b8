"""Every kernel instance of the time-as-k weight gradients (csrc/wn_wgrad.hip) and of the fused WN kernels (csrc/wn_fused.hip)
against an fp64 reference, at the edges of their pickers.

Each case calls the C entry point itself, so the test owns every buffer: inputs sit between NaN bands (and, where a batch
stride is larger than a sample, NaN guard channels), outputs between canary bands that must stay untouched and pre-filled
with NaN so an element nobody wrote shows; the slab workspace has exactly the size the ``*_workspace_floats`` query returns,
NaN-filled, with a canary band behind it.  A case asserts the launch-route record first (``fst_wn_last_route``: the library's
own record of the instance, grid, K split and ring it launched), then compares with fp64, then repeats the launch and
requires the same bits (no kernel here uses atomics).

Gates are the ones the suite already uses for these kernels, against max|want| (tests/test_gpu_kernels.py,
tests/test_gpu_full_size.py): 1e-4 weight gradients, 2e-5 forward outputs and data gradients, 1e-5·max|pre-activation| for the
gate halves, and for row sums 2e-5 of the largest Σ|term| (a sum's error scales with its terms, not with its value).

The ``*_expect`` functions restate the launchers' geometry (pickers, K split, grid); the cases' ``inst`` fields say which
instance a case is there for.  tests/test_wn_routes_cpu.py checks both against the sources without a GPU.
"""
from __future__ import annotations

import ctypes
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import pytest
import torch
import torch.nn.functional as F

from feature_level_style_transfer_for_tsc_amd import _lib, ops

DEV = "cuda"
CANARY = -4242.0
NAN = float("nan")
BAND = 64                 # floats of guard band on either side of every buffer (256 bytes: the body stays 16-byte aligned)
WS_MAXL = 10              # csrc/wn_fused.hip
bf3_only = pytest.mark.skipif(ops.MATH != "bf16x3", reason="split-bf16 kernel; FST_MATH=f32 routes around it")

WGRAD, TZ, LAYER_FWD, STACK_FWD, LAYER_BWD, LAYER_DGRAD, STACK_BWD = (
    ops.WN_ROUTE_WGRAD, ops.WN_ROUTE_TZ, ops.WN_ROUTE_LAYER_FWD, ops.WN_ROUTE_STACK_FWD, ops.WN_ROUTE_LAYER_BWD,
    ops.WN_ROUTE_LAYER_DGRAD, ops.WN_ROUTE_STACK_BWD)


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


# --------------------------------------------------------------------------------------------------
# the launchers' geometry, restated (checked against the route record by every case, against the sources by the CPU test)
# --------------------------------------------------------------------------------------------------
def _ww_route(KT, M, K_main, ne, mul, n_tiles, n_sets, misaligned, cus, reduce=1):
    kb = cdiv(K_main, 32)
    ng = cdiv(kb, 2 * KT)
    xr = 64 * KT
    RX = xr * (1 + mul) + 8 * ne
    ks = max(n_sets, min(cus // ng, n_tiles * n_sets))
    full = cdiv(M, 32) == 8 and kb % (2 * KT) == 0
    lds = 3 * 256 * 128 + 2 * RX * 128
    need = ks * 256 * (ng * xr + 2)
    return (WGRAD, KT, int(full), mul, ne, ks, ng, 1, n_sets, int(misaligned), reduce, lds), need


def wn_wgrad_expect(kind: int, B: int, L: int, n: int, h: int, last: bool, n_sets: int, dil: int, cus: int = 256):
    """(route record, workspace floats the launch needs) of fst_wn_wgrad_in (kind 0) / fst_wn_wgrad_rs (kind 1)."""
    M = 2 * n if kind == 0 or not last else n
    K = 3 * n + h if kind == 0 else n
    ne = int(kind == 0 and K % 32 == 1)
    return _ww_route(3 if kind == 0 else 2, M, K - ne, ne, int(kind == 1), B * (L // 32), n_sets, kind == 0 and dil % 4 != 0, cus)


def tap_wgrad_expect(B: int, L: int, M: int, C: int, ntaps: int, dil: int, pad_left: int, cus: int = 256):
    mis = any((t * dil - pad_left) % 4 != 0 for t in range(ntaps))
    return _ww_route(3, M, ntaps * C, 0, 0, B * (L // 32), 1, mis, cus)


def nt_gemm_expect(M: int, N: int, K: int, epi: bool, cus: int = 256):
    route, need = _ww_route(2, M, N, 0, 0, K // 32, 1, False, cus)
    direct = route[5] == 1 and M == 256 and route[6] * 128 == N and not epi
    return route[:10] + (int(not direct),) + route[11:], need


def tz_expect(B: int, L: int, M: int, C: int, K: int, cus: int = 256):
    """(route record, workspace floats) of fst_dense_tap_wgrad."""
    MP = 1 if M <= 64 else 2
    cw = 8 // MP
    halves = 2 if M > 128 else 1
    ng = cdiv(C, cw)
    ks = max(1, min(cus // (ng * halves), B * (L // 32)))
    last_half = M - (halves - 1) * 128
    full = K > 64 and (last_half > 96 if halves > 1 else M > (128 if MP == 2 else 64) - 32)
    lds = 4 * (64 if MP == 1 else 128) * 128 + 4 * cw * 1024 + 2 * cw * 2 * 8 * 288
    return (TZ, MP, int(full), 0, 0, ks, ng, halves, 1, 0, 1, lds), ks * 256 * ng * cw * 96


def wn_fwd_lds(nw: int) -> int:
    return 3 * (8 * 2048 + 2 * ((nw + 1) * 1024 + 128))


def layer_fwd_expect(B: int, L: int, cus: int = 256):
    nw = 8 if L % 256 == 0 and B * (L // 256) >= cus else 4
    tps = cdiv(L, 32 * nw)
    return (LAYER_FWD, nw, 0, 0, 0, B * tps, 1, 1, tps, 3, 1, wn_fwd_lds(nw))


def dgrad_slot(dil: int) -> int:
    nblkw = (512 + 2 * dil + 3 + 31) // 32
    return 13 * 2048 + 2 * (nblkw * 1024 + 128)


def dgrad_ring_slots(dil: int) -> int:
    return 3 if 3 * dgrad_slot(dil) <= 160 * 1024 else 2


def layer_dgrad_expect(B: int, L: int, dil: int, cus: int = 256):
    tps = cdiv(L, 512)
    ns = dgrad_ring_slots(dil)
    lds = max(ns * dgrad_slot(dil), 8 * 32 * 36 * 4 + 4096)
    grid = cus if B * tps > cus and 2 * lds > 160 * 1024 else B * tps
    return (LAYER_DGRAD, 0, 0, 0, 0, grid, 1, 1, tps, ns, 1, lds)


def wn_wgrad_instance(route) -> str:
    return ops.wn_route_kernel_name(route)


# --------------------------------------------------------------------------------------------------
# buffers
# --------------------------------------------------------------------------------------------------
def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def _gen(name: str) -> torch.Generator:
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(name.encode()))


def rnd(g, *shape, k: float = 1.0) -> torch.Tensor:
    return torch.randn(*shape, generator=g, device=DEV, dtype=torch.float64) * k


def fenced(shape, band_fill: float, fill: float, extra: int = 0, row0: int = 0):
    """(buffer, view): a [B, C, L] (or any-shape, extra = 0) fp32 view inside a flat buffer with BAND floats of ``band_fill`` on
    either side; with ``extra`` the view is channels [row0, row0 + C) of a [B, C + extra, L] block whose other channels hold
    ``band_fill`` too (batch stride (C + extra)·L).  The view itself is filled with ``fill``."""
    if extra:
        B, C, L = shape
        numel = B * (C + extra) * L
    else:
        numel = 1
        for s in shape:
            numel *= s
    buf = torch.full((numel + 2 * BAND,), band_fill, device=DEV, dtype=torch.float32)
    body = buf[BAND: BAND + numel]
    view = body.view(B, C + extra, L)[:, row0: row0 + C] if extra else body.view(*shape)
    view.fill_(fill)
    return buf, view


def nan_in(x: torch.Tensor, extra: int = 0, row0: int = 0) -> torch.Tensor:
    """fp32 device copy of ``x`` between NaN bands (and NaN guard channels)."""
    _, v = fenced(tuple(x.shape), NAN, 0.0, extra, row0)
    v.copy_(x)
    return v


def out_buf(shape, extra: int = 0, row0: int = 0, init: Optional[torch.Tensor] = None):
    """(buffer, view) of an output between canary bands, pre-filled with NaN (``init``: an accumulated output's start value)."""
    buf, v = fenced(tuple(shape), CANARY, NAN, extra, row0)
    if init is not None:
        v.copy_(init)
    return buf, v


def assert_fence(buf: torch.Tensor, view: torch.Tensor, what: str):
    probe = buf.clone()
    probe.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(CANARY)
    bad = int((probe != CANARY).sum())
    assert bad == 0, f"{what}: {bad} elements outside the output were written"


def assert_untouched(buf: torch.Tensor, view: torch.Tensor, what: str):
    """A refused call wrote nothing: the bands hold the canary, the body still its NaN."""
    assert_fence(buf, view, what)
    assert bool(torch.isnan(view).all()), f"{what}: a refused call wrote into the output"


def assert_close(got, want, tol, what=""):
    got, want = got.detach().double(), want.detach().double()
    scale = max(1e-6, float(want.abs().max()))
    err = float((got - want).abs().max())
    print(f"  {what}: max err {err:.3e}, scale {scale:.3e}, gate {tol * scale:.3e}")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def assert_row_sums(got, terms, what):
    """Row sums of ``terms`` [B, rows, L] over (b, t): 2e-5 of the largest Σ|term| (the formula of test_fused_wn_layer_backward)."""
    want = terms.sum(dim=(0, 2))
    mass = float(terms.abs().sum(dim=(0, 2)).max())
    assert_close(got, want, 2e-5 * mass / max(1e-9, float(want.abs().max())), what)


def workspace(ws_n: int):
    """(buffer, view): exactly ``ws_n`` floats of NaN with a canary band on either side."""
    return fenced((ws_n,), CANARY, NAN)


def ptrs(ts):
    arr = (ctypes.c_void_p * len(ts))()
    for i, t in enumerate(ts):
        arr[i] = None if t is None else t.data_ptr()
    return arr


def last_route(want, what: str):
    got = ops.wn_last_route()
    print(f"  {what}: {ops.wn_route_kernel_name(got) if got[0] else 'nothing'} {got}")
    assert got == tuple(want), f"{what}: launched {got}, expected {tuple(want)}"


def check_rc(rc: int, what: str):
    assert rc == 0, f"{what}: rc={rc}: {_lib.load().fst_last_error()}"


# --------------------------------------------------------------------------------------------------
# in_layer + cond_layer weight gradients: wn_wgrad_kernel<2, 3, FULL, false, NE>
# --------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class WIn:
    inst: str           # the instance this case is here for
    n: int
    h: int
    B: int
    L: int
    dil: int
    n_sets: int = 1
    u0_extra: int = 3   # guard channels of the u0 slice (batch stride (h + extra)·L)

    @property
    def id(self) -> str:
        return f"n{self.n}h{self.h}-B{self.B}L{self.L}d{self.dil}-s{self.n_sets}"


F0, F1, P0, P1 = ("wn_wgrad_kernel<2, 3, true, false, 0>", "wn_wgrad_kernel<2, 3, true, false, 1>",
                  "wn_wgrad_kernel<2, 3, false, false, 0>", "wn_wgrad_kernel<2, 3, false, false, 1>")
WIN_CASES = [
    # FULL, no leftover row: K = 384 (two groups of 6 blocks); M = 226: the last row block has 2 live rows
    WIn(F0, 120, 24, 48, 512, 4), WIn(F0, 120, 24, 3, 64, 1), WIn(F0, 113, 32, 2, 96, 2, n_sets=2), WIn(F0, 113, 32, 2, 64, 8),
    # partial + the VALU leftover row: one group (K_main = 32); two groups; 8 row blocks but 11 k-row blocks
    WIn(P1, 8, 9, 3, 64, 1), WIn(P1, 8, 9, 1, 32, 32), WIn(P1, 100, 21, 5, 320, 4, n_sets=2), WIn(P1, 100, 21, 2, 64, 3),
    WIn(P1, 116, 5, 48, 512, 8), WIn(P1, 116, 5, 2, 96, 2, n_sets=3),
    # FULL + leftover row
    WIn(F1, 127, 4, 2, 128, 4), WIn(F1, 127, 4, 5, 320, 1, n_sets=3), WIn(F1, 120, 25, 16, 512, 128),
    # partial, no leftover row; three groups (13 blocks); h = 1 / 32, n = 1 / 127
    WIn(P0, 127, 32, 3, 96, 4), WIn(P0, 127, 32, 2, 64, 3, n_sets=3), WIn(P0, 16, 1, 2, 64, 1), WIn(P0, 1, 32, 1, 32, 2),
    # (not n = 1 with h = 1: dW_cond then has two elements and max|want| is the larger of two draws of a sum that cancels — 0.32
    # against Σ|terms| = 81 on the first input tried, where the kernel's 8.9e-5 = 1.1e-6 of the terms, the error every other case
    # shows, missed 1e-4·max|want|; with 32 elements or more the scale is the sum's spread, which is what the gate assumes)
    WIn(P0, 16, 5, 5, 320, 4, n_sets=3),         # 50 tiles per set over 85 / 85 / 86 workgroups of a set
    WIn(P0, 48, 5, 7, 352, 4, n_sets=2),         # 77 tiles per set over 64 workgroups of a set: uneven shares
    WIn(P0, 33, 31, 1, 32, 4, n_sets=1),         # one tile: the K split is clamped to 1
    WIn(P0, 33, 31, 1, 32, 64, n_sets=3),        # one tile per set, dilation > L: taps 0 and 2 wholly outside the sequence
    WIn(P0, 16, 16, 2, 64, 64),                  # dilation == L
]


def _in_reference(dg, a, u0, dil, L):
    ap = F.pad(a, (dil, dil))
    w_in = torch.stack([torch.einsum("bmt,bct->mc", dg, ap[:, :, k * dil: k * dil + L]) for k in range(3)], dim=2)
    return w_in, torch.einsum("bmt,bct->mc", dg, u0)


@bf3_only
@pytest.mark.gpu
@pytest.mark.parametrize("c", WIN_CASES, ids=lambda c: c.id)
def test_wn_wgrad_in_instance_vs_fp64(c: WIn):
    lib, g = _lib.load(), _gen("in" + c.id)
    n, h, B, L = c.n, c.h, c.B, c.L
    route, need = wn_wgrad_expect(0, B, L, n, h, False, c.n_sets, c.dil, _cus())
    assert wn_wgrad_instance(route) == c.inst
    dg64 = [rnd(g, B, 2 * n, L) for _ in range(c.n_sets)]
    a64 = [rnd(g, B, n, L) for _ in range(c.n_sets)]
    u64 = [rnd(g, B, h, L) for _ in range(c.n_sets)]
    want_in = want_cond = 0
    for s in range(c.n_sets):
        wi, wc = _in_reference(dg64[s], a64[s], u64[s], c.dil, L)
        want_in, want_cond = want_in + wi, want_cond + wc
    dg = [nan_in(x) for x in dg64]
    a = [nan_in(x) for x in a64]                         # the NaN bands are the 16 readable bytes of slack (dilation 1-3)
    u0 = [nan_in(x, c.u0_extra, 1) for x in u64]
    ws_n = lib.fst_wn_wgrad_workspace_floats(0, B, L, n, h, 0)
    assert ws_n >= need
    assert lib.fst_wn_wgrad_ok(0, B, L, n, h, c.dil) == (1 if c.dil % 4 == 0 else 2)

    def run():
        (bi, dw_in), (bc, dw_cond), (bw, ws) = out_buf((2 * n, n, 3)), out_buf((2 * n, h)), workspace(ws_n)
        check_rc(lib.fst_wn_wgrad_in(ptrs(dg), ptrs(a), ptrs(u0), c.n_sets, (h + c.u0_extra) * L, dw_in.data_ptr(), dw_cond.data_ptr(),
                                     ws.data_ptr(), ws_n, B, L, n, h, c.dil, 1, B * n * L, _lib.stream_ptr()), c.id)
        last_route(route, c.id)
        assert_fence(bi, dw_in, "dw_in"), assert_fence(bc, dw_cond, "dw_cond"), assert_fence(bw, ws, "slab workspace")
        return dw_in, dw_cond

    dw_in, dw_cond = run()
    assert_close(dw_in, want_in, 1e-4, "in_layer dW")
    assert_close(dw_cond, want_cond, 1e-4, "cond_layer dW")
    again_in, again_cond = run()
    assert torch.equal(again_in, dw_in) and torch.equal(again_cond, dw_cond), "two identical launches differ"


# --------------------------------------------------------------------------------------------------
# res_skip weight gradient: wn_wgrad_kernel<2, 2, FULL, true, 0>
# --------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class WRs:
    inst: str
    n: int
    B: int
    L: int
    last: bool
    n_sets: int = 1

    @property
    def id(self) -> str:
        return f"n{self.n}-B{self.B}L{self.L}-{'last' if self.last else 'mid'}-s{self.n_sets}"


MF, MP_ = "wn_wgrad_kernel<2, 2, true, true, 0>", "wn_wgrad_kernel<2, 2, false, true, 0>"
WRS_CASES = [
    WRs(MF, 120, 16, 512, False), WRs(MF, 113, 2, 96, False, n_sets=3), WRs(MF, 127, 5, 320, False, n_sets=2),
    WRs(MP_, 120, 3, 64, True), WRs(MP_, 112, 2, 64, False),            # 7 row blocks
    WRs(MP_, 96, 2, 64, False), WRs(MP_, 1, 2, 64, False), WRs(MP_, 1, 1, 32, True), WRs(MP_, 33, 1, 32, False, n_sets=3),
    WRs(MP_, 127, 2, 96, True, n_sets=2), WRs(MP_, 48, 7, 352, False, n_sets=2),
]


@bf3_only
@pytest.mark.gpu
@pytest.mark.parametrize("c", WRS_CASES, ids=lambda c: c.id)
def test_wn_wgrad_rs_instance_vs_fp64(c: WRs):
    lib, g = _lib.load(), _gen("rs" + c.id)
    n, B, L = c.n, c.B, c.L
    M = n if c.last else 2 * n
    route, need = wn_wgrad_expect(1, B, L, n, 0, c.last, c.n_sets, 4, _cus())
    assert wn_wgrad_instance(route) == c.inst
    ts64 = [rnd(g, B, 2 * n, L) for _ in range(c.n_sets)]
    da64 = [rnd(g, B, n, L) for _ in range(c.n_sets)]
    do64 = [rnd(g, B, n, L) for _ in range(c.n_sets)]
    want = 0
    for s in range(c.n_sets):
        dy = do64[s] if c.last else torch.cat([da64[s], do64[s]], 1)
        want = want + torch.einsum("bmt,bct->mc", dy, ts64[s][:, :n] * ts64[s][:, n:])
    ts, d_a, d_out = [nan_in(x) for x in ts64], [nan_in(x) for x in da64], [nan_in(x) for x in do64]
    ws_n = lib.fst_wn_wgrad_workspace_floats(1, B, L, n, 0, int(c.last))
    assert ws_n >= need

    def run():
        (bd, dw), (bw, ws) = out_buf((M, n)), workspace(ws_n)
        check_rc(lib.fst_wn_wgrad_rs(None if c.last else ptrs(d_a), ptrs(d_out), ptrs(ts), c.n_sets, dw.data_ptr(), ws.data_ptr(), ws_n,
                                     int(c.last), B, L, n, B * n * L, _lib.stream_ptr()), c.id)
        last_route(route, c.id)
        assert_fence(bd, dw, "dw_rs"), assert_fence(bw, ws, "slab workspace")
        return dw

    dw = run()
    assert_close(dw, want, 1e-4, "res_skip dW")
    assert torch.equal(run(), dw), "two identical launches differ"


# --------------------------------------------------------------------------------------------------
# few-tap conv weight gradient on wn_wgrad_kernel<2, 3, FULL, false, 0>
# --------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Tap:
    inst: str
    M: int
    C: int
    ntaps: int
    dil: int
    pad: int
    B: int
    L: int

    @property
    def id(self) -> str:
        return f"M{self.M}C{self.C}k{self.ntaps}d{self.dil}p{self.pad}-B{self.B}L{self.L}"


TAP_CASES = [
    Tap(F0, 240, 96, 2, 4, 4, 3, 96),            # FULL: 8 row blocks, 6 k-row blocks
    Tap(F0, 225, 64, 3, 1, 1, 2, 64),            # FULL with shifts -1 / 0 / +1 (patched pieces); the last row block has one row
    Tap(P0, 40, 144, 4, 4, 8, 2, 64),            # the LDS limit: 18 k-row blocks, three groups
    Tap(P0, 50, 225, 2, 1, 0, 3, 64),            # the omni-scale block's last layer: shifts 0 / +1
    Tap(P0, 256, 7, 1, 1, 0, 2, 32),             # one tap, 256 rows, one k-row block
]


@bf3_only
@pytest.mark.gpu
@pytest.mark.parametrize("c", TAP_CASES, ids=lambda c: c.id)
def test_tap_wgrad_instance_vs_fp64(c: Tap):
    lib, g = _lib.load(), _gen("tap" + c.id)
    route, need = tap_wgrad_expect(c.B, c.L, c.M, c.C, c.ntaps, c.dil, c.pad, _cus())
    assert wn_wgrad_instance(route) == c.inst
    dy64, x64 = rnd(g, c.B, c.M, c.L), rnd(g, c.B, c.C, c.L)
    halo = (c.ntaps - 1) * c.dil
    xp = F.pad(x64, (c.pad, max(0, halo - c.pad) + c.pad))
    want = torch.stack([torch.einsum("bmt,bct->mc", dy64, xp[:, :, k * c.dil: k * c.dil + c.L]) for k in range(c.ntaps)], dim=2)
    dy, x = nan_in(dy64), nan_in(x64)
    ws_n = lib.fst_tap_wgrad_workspace_floats(c.B, c.L, c.M, c.C, c.ntaps)
    assert ws_n == need

    def run():
        (bd, dw), (bw, ws) = out_buf((c.M, c.C, c.ntaps)), workspace(ws_n)
        check_rc(lib.fst_tap_wgrad(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws_n, c.B, c.L, c.M, c.C, c.ntaps, c.dil,
                                   c.pad, 1, dy.numel(), x.numel(), _lib.stream_ptr()), c.id)
        last_route(route, c.id)
        assert_fence(bd, dw, "dw"), assert_fence(bw, ws, "slab workspace")
        return dw

    dw = run()
    assert_close(dw, want, 1e-4, "few-tap dW")
    assert torch.equal(run(), dw), "two identical launches differ"


@pytest.mark.gpu
def test_tap_wgrad_refuses_a_nineteenth_k_row_block():
    lib = _lib.load()
    assert lib.fst_tap_wgrad_ok(2, 64, 40, 144, 4, 4, 8) == 1 and lib.fst_tap_wgrad_ok(2, 64, 40, 145, 4, 4, 8) == 0
    assert lib.fst_tap_wgrad_workspace_floats(2, 64, 40, 145, 4) == -1
    dy, x = nan_in(torch.zeros(2, 40, 64)), nan_in(torch.zeros(2, 145, 64))
    (bd, dw), (bw, ws) = out_buf((40, 145, 4)), workspace(4096)
    rc = lib.fst_tap_wgrad(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), ws.data_ptr(), 1 << 40, 2, 64, 40, 145, 4, 4, 8, 1, dy.numel(),
                           x.numel(), _lib.stream_ptr())
    assert rc == -1 and ops.wn_last_route() == (0,) * ops.WN_ROUTE_LEN
    torch.cuda.synchronize()
    assert_untouched(bd, dw, "dw"), assert_untouched(bw, ws, "workspace")


# --------------------------------------------------------------------------------------------------
# C = A·Bᵀ: wn_wgrad_kernel<2, 2, FULL, false, 0>, the direct-store path and RandomLayer's epilogue
# --------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Nt:
    inst: str
    M: int
    N: int
    K: int
    epi: int = 0        # 0 none, 1 the epilogue, 2 the epilogue and the raw product
    direct: bool = False

    @property
    def id(self) -> str:
        return f"M{self.M}N{self.N}K{self.K}" + ("", "-epi", "-epi+raw")[self.epi] + ("-direct" if self.direct else "")


GF, GP = "wn_wgrad_kernel<2, 2, true, false, 0>", "wn_wgrad_kernel<2, 2, false, false, 0>"
NT_CASES = [
    Nt(GF, 256, 128, 32, direct=True),           # one K tile: one workgroup per group stores straight into C
    Nt(GF, 256, 25600, 64, direct=True),         # 200 groups on 256 CUs: K split 1, two stages
    Nt(GF, 255, 128, 32),                        # near misses of the direct path: the reduce pass runs
    Nt(GF, 256, 100, 32),                        # N != the slab row length (the fourth k-row block has 4 live rows)
    Nt(GF, 256, 128, 64),                        # K split 2
    Nt(GF, 256, 128, 32, epi=1),                 # the epilogue needs the reduce pass
    Nt(GP, 37, 130, 96, epi=1), Nt(GP, 37, 130, 96, epi=2), Nt(GP, 200, 130, 96), Nt(GP, 1, 1, 32),
]


@bf3_only
@pytest.mark.gpu
@pytest.mark.parametrize("c", NT_CASES, ids=lambda c: c.id)
def test_nt_gemm_instance_vs_fp64(c: Nt):
    lib, g = _lib.load(), _gen("nt" + c.id)
    route, need = nt_gemm_expect(c.M, c.N, c.K, c.epi > 0, _cus())
    assert wn_wgrad_instance(route) == c.inst and route[10] == int(not c.direct)
    A64, B64 = rnd(g, c.M, c.K), rnd(g, c.N, c.K)
    raw = A64 @ B64.t()
    ncls, scale = 3, 0.37
    p64, r64 = rnd(g, c.M, ncls), rnd(g, ncls, c.N)
    want = raw * scale * (p64 @ r64) if c.epi else raw
    A, Bm = nan_in(A64), nan_in(B64)
    pd, rd = (nan_in(p64), nan_in(r64)) if c.epi else (None, None)
    ws_n = lib.fst_nt_gemm_workspace_floats(c.M, c.N, c.K)
    assert ws_n == need

    def run():
        (bC, C), (bw, ws) = out_buf((c.M, c.N)), workspace(ws_n)
        bR, R = out_buf((c.M, c.N)) if c.epi == 2 else (None, None)
        check_rc(lib.fst_nt_gemm(A.data_ptr(), Bm.data_ptr(), C.data_ptr(), ws.data_ptr(), ws_n, c.M, c.N, c.K, _lib.ptr(pd), _lib.ptr(rd),
                                 ncls if c.epi else 0, scale, _lib.ptr(R), _lib.stream_ptr()), c.id)
        last_route(route, c.id)
        assert_fence(bC, C, "C"), assert_fence(bw, ws, "slab workspace")
        if c.direct:
            assert bool(torch.isnan(ws).all()), "the direct path wrote into the workspace"
        if R is not None:
            assert_fence(bR, R, "raw product")
        return C, R

    C, R = run()
    assert_close(C, want, 1e-4, "C")
    if R is not None:
        assert_close(R, raw, 1e-4, "raw product")
    C2, R2 = run()
    assert torch.equal(C2, C) and (R is None or torch.equal(R2, R)), "two identical launches differ"


# --------------------------------------------------------------------------------------------------
# refusals of the weight-gradient launchers: an error, no route, nothing written
# --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("what", ["workspace one float short", "dilation 2 without slack", "dilation 6", "L % 32 != 0", "4 sets"])
def test_wn_wgrad_in_refusals_write_nothing(what):
    lib = _lib.load()
    n, h, B, L, dil, n_sets, slack = 16, 5, 2, 64, 4, 3, 1
    if what == "dilation 2 without slack":
        dil, slack = 2, 0
    elif what == "dilation 6":
        dil = 6
    elif what == "L % 32 != 0":
        L = 48
    dg = [nan_in(torch.zeros(B, 2 * n, L)) for _ in range(4)]
    a = [nan_in(torch.zeros(B, n, L)) for _ in range(4)]
    u0 = [nan_in(torch.zeros(B, h, L)) for _ in range(4)]
    ws_n = lib.fst_wn_wgrad_workspace_floats(0, B, 64, n, h, 0)
    _, need = wn_wgrad_expect(0, B, 64, n, h, False, 3, 4, _cus())
    assert ws_n == need                                       # three sets: the launch needs all the query returns
    (bi, dw_in), (bc, dw_cond), (bw, ws) = out_buf((2 * n, n, 3)), out_buf((2 * n, h)), workspace(ws_n)
    if what == "workspace one float short":
        ws_n -= 1
    if what == "4 sets":
        n_sets = 4
    rc = lib.fst_wn_wgrad_in(ptrs(dg[:n_sets]), ptrs(a[:n_sets]), ptrs(u0[:n_sets]), n_sets, h * L, dw_in.data_ptr(), dw_cond.data_ptr(),
                             ws.data_ptr(), ws_n, B, L, n, h, dil, slack, B * n * L, _lib.stream_ptr())
    assert rc == -1 and lib.fst_last_error(), what
    assert ops.wn_last_route() == (0,) * ops.WN_ROUTE_LEN
    torch.cuda.synchronize()
    assert_untouched(bi, dw_in, "dw_in"), assert_untouched(bc, dw_cond, "dw_cond"), assert_untouched(bw, ws, "workspace")


# --------------------------------------------------------------------------------------------------
# dense many-tap weight gradient: tz_wgrad_kernel<MP, FULL>
# --------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Tz:
    inst: str
    M: int
    C: int
    K: int
    pad: int
    B: int = 2
    L: int = 96

    @property
    def id(self) -> str:
        return f"M{self.M}C{self.C}K{self.K}p{self.pad}-B{self.B}L{self.L}"


T1F, T1P, T2F, T2P = ("tz_wgrad_kernel<1, true>", "tz_wgrad_kernel<1, false>", "tz_wgrad_kernel<2, true>", "tz_wgrad_kernel<2, false>")
TZ_CASES = [
    # both sides of every threshold of the `full` predicate, K = 89 > 64
    Tz(T1P, 32, 9, 89, 44), Tz(T1F, 33, 9, 89, 44), Tz(T1F, 64, 3, 89, 0), Tz(T2P, 65, 5, 89, 88),
    Tz(T2P, 96, 5, 89, 44), Tz(T2F, 97, 2, 89, 44), Tz(T2F, 128, 4, 89, 1), Tz(T2P, 129, 3, 89, 44),       # 129: a row half of one row
    Tz(T2P, 224, 2, 89, 44), Tz(T2F, 225, 5, 89, 44, B=3, L=128), Tz(T2F, 256, 1, 96, 95),
    # K = 64 / 65 with row counts that are FULL at K > 64
    Tz(T1P, 50, 9, 64, 32), Tz(T1F, 50, 9, 65, 32), Tz(T2P, 100, 5, 64, 31), Tz(T2F, 100, 5, 65, 33), Tz(T2P, 225, 3, 64, 32),
    Tz(T1P, 1, 1, 5, 2, B=1, L=32),                                                # the smallest shape served
    Tz(T1F, 40, 17, 70, 35, B=40, L=160),                                          # three groups, 200 tiles over 85 workgroups
]


@bf3_only
@pytest.mark.gpu
@pytest.mark.parametrize("c", TZ_CASES, ids=lambda c: c.id)
def test_dense_tap_wgrad_instance_vs_fp64(c: Tz):
    lib, g = _lib.load(), _gen("tz" + c.id)
    route, need = tz_expect(c.B, c.L, c.M, c.C, c.K, _cus())
    assert ops.wn_route_kernel_name(route) == c.inst
    dy64, x64 = rnd(g, c.B, c.M, c.L), rnd(g, c.B, c.C, c.L)
    xp = F.pad(x64, (c.pad, c.K - 1 - c.pad))
    want = torch.einsum("bmt,bctk->mck", dy64, xp.unfold(2, c.L, 1).transpose(2, 3))       # x[b, c, t + k − pad]
    dy, x = nan_in(dy64), nan_in(x64)
    ws_n = lib.fst_dense_tap_wgrad_workspace_floats(c.B, c.L, c.M, c.C, c.K)
    assert ws_n == need

    def run():
        (bd, dw), (bw, ws) = out_buf((c.M, c.C, c.K)), workspace(ws_n)
        check_rc(lib.fst_dense_tap_wgrad(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws_n, c.B, c.L, c.M, c.C, c.K, c.pad,
                                         dy.numel(), x.numel(), _lib.stream_ptr()), c.id)
        last_route(route, c.id)
        assert_fence(bd, dw, "dw"), assert_fence(bw, ws, "slab workspace")
        return dw

    dw = run()
    assert_close(dw, want, 1e-4, "dense many-tap dW")
    assert torch.equal(run(), dw), "two identical launches differ"
    (bd, dw2), (bw, ws) = out_buf((c.M, c.C, c.K)), workspace(ws_n)
    rc = lib.fst_dense_tap_wgrad(dy.data_ptr(), x.data_ptr(), dw2.data_ptr(), ws.data_ptr(), ws_n - 1, c.B, c.L, c.M, c.C, c.K, c.pad,
                                 dy.numel(), x.numel(), _lib.stream_ptr())
    assert rc == -1 and ops.wn_last_route() == (0,) * ops.WN_ROUTE_LEN            # workspace one float short
    torch.cuda.synchronize()
    assert_untouched(bd, dw2, "dw"), assert_untouched(bw, ws, "workspace")


# --------------------------------------------------------------------------------------------------
# fused layer forward: wn_layer_fwd_kernel<4 | 8>
# --------------------------------------------------------------------------------------------------
def _layer_weights(g, n, h, last):
    R = n if last else 2 * n
    return dict(in_w=rnd(g, 2 * n, n, 3, k=(3 * n) ** -0.5), cond_w=rnd(g, 2 * n, h, 1, k=h ** -0.5), in_b=rnd(g, 2 * n, k=0.3),
                cond_b=rnd(g, 2 * n, k=0.3), rs_w=rnd(g, R, n, 1, k=n ** -0.5), rs_b=rnd(g, R, k=0.3))


def _f32(x):
    return x.float().contiguous()


def _layer_image(w, n, h, last):
    return ops.wn_pack_layer(_f32(w["in_w"]), _f32(w["cond_w"]), _f32(w["in_b"]), _f32(w["cond_b"]), _f32(w["rs_w"]), _f32(w["rs_b"]),
                             n, h, last)


def _layer_forward_f64(w, a, u0, dil, last):
    """(pre-activation, t, s, residual rows or None, skip rows) of one WN layer in fp64."""
    n = a.size(1)
    gg = F.conv1d(a, w["in_w"], w["in_b"], dilation=dil, padding=dil) + F.conv1d(u0, w["cond_w"], w["cond_b"])
    t, s = torch.tanh(gg[:, :n]), torch.sigmoid(gg[:, n:])
    r = F.conv1d(t * s, w["rs_w"], w["rs_b"])
    return gg, t, s, (None if last else r[:, :n]), (r if last else r[:, n:])


@dataclass(frozen=True)
class Fw:
    nw: int
    n: int
    h: int
    B: int
    L: int
    dil: int
    first: bool
    last: bool
    acts: bool = True
    extra: int = 2      # guard channels around the a / u0 slices

    @property
    def id(self) -> str:
        return (f"nw{self.nw}-n{self.n}h{self.h}-B{self.B}L{self.L}d{self.dil}" + ("-first" if self.first else "") +
                ("-last" if self.last else "") + ("" if self.acts else "-noacts"))


FW_CASES = [
    Fw(4, 33, 7, 2, 200, 4, True, False), Fw(4, 33, 7, 2, 200, 1, False, False, acts=False),          # partial last tile (128 + 72)
    Fw(4, 33, 7, 1, 132, 64, False, True), Fw(4, 8, 3, 2, 40, 2, True, True, acts=False),
    Fw(4, 127, 32, 1, 256, 16, False, False), Fw(4, 8, 3, 3, 256, 1, True, False),                   # L % 256 == 0 but too few tiles
    # (n >= 8 here: with n = 1 a res_skip row is ONE weight times acts, so the gate halves' allowance — 1e-5·max|pre-activation| =
    # 4.5e-5, used: 2.5e-5 — reaches `out` undamped, where 2e-5·max|out| = 1.5e-5 has no room for it; measured 2.6e-5.  That is
    # the gate's error, not GEMM 2's; over n >= 8 rows it averages out below the gate as in every other case)
    Fw(4, 120, 25, 2, 512, 128, False, False, acts=False),
    Fw(8, 16, 5, 256, 256, 8, True, False), Fw(8, 8, 3, 128, 512, 2, False, False, acts=False),
    Fw(8, 8, 3, 256, 256, 1, False, True), Fw(8, 33, 31, 300, 256, 256, True, True, acts=False),    # dilation == L
]


@bf3_only
@pytest.mark.gpu
@pytest.mark.parametrize("c", FW_CASES, ids=lambda c: c.id)
def test_wn_layer_fwd_instance_vs_fp64(c: Fw):
    lib, g = _lib.load(), _gen("fw" + c.id)
    n, h, B, L = c.n, c.h, c.B, c.L
    route = layer_fwd_expect(B, L, _cus())
    assert route[1] == c.nw
    w = _layer_weights(g, n, h, c.last)
    a64, u64, out0 = rnd(g, B, n, L), rnd(g, B, h, L), rnd(g, B, n, L)
    gg, t, s, res, skip = _layer_forward_f64(w, a64, u64, c.dil, c.last)
    want_out = skip if c.first else out0 + skip
    img = _layer_image(w, n, h, c.last)
    a, u0 = nan_in(a64, c.extra, 1), nan_in(u64, c.extra, 1)

    def run():
        o = {"ts": out_buf((B, 2 * n, L)), "out": out_buf((B, n, L), init=None if c.first else out0)}
        if c.acts:
            o["acts"] = out_buf((B, n, L))
        if not c.last:
            o["a_next"] = out_buf((B, n, L))
        p = lambda k: o[k][1].data_ptr() if k in o else None
        check_rc(lib.fst_wn_layer_fwd(a.data_ptr(), (n + c.extra) * L, u0.data_ptr(), (h + c.extra) * L, img.data_ptr(), img.numel() * 4,
                                      p("ts"), p("acts"), p("a_next"), p("out"), int(c.first), int(c.last), B, L, n, h, c.dil, B * n * L,
                                      _lib.stream_ptr()), c.id)
        last_route(route, c.id)
        for k, (buf, v) in o.items():
            assert_fence(buf, v, k)
        return {k: v for k, (_, v) in o.items()}

    o = run()
    gtol = 1e-5 * float(gg.abs().max())      # the gate halves inherit the GEMM's error through tanh' <= 1 (test_fused_wn_layer_forward)
    assert_close(o["ts"][:, :n], t, gtol, "t")
    assert_close(o["ts"][:, n:], s, gtol, "s")
    if c.acts:
        assert_close(o["acts"], t * s, gtol, "acts")
    if not c.last:
        assert_close(o["a_next"], a64 + res, 2e-5, "a_next")
    assert_close(o["out"], want_out, 2e-5, "out")
    o2 = run()
    for k in o:
        assert torch.equal(o[k], o2[k]), f"{k} differs between two identical launches"


# --------------------------------------------------------------------------------------------------
# fused layer backward through res_skip and the gate: wn_layer_bwd_kernel
# --------------------------------------------------------------------------------------------------
def _gate_backward_f64(rs_w, d_a, d_out, t, s):
    """(dacts, dg) — rs_w [R, n]; d_a None on the last layer."""
    d_r = d_out if d_a is None else torch.cat([d_a, d_out], 1)
    dacts = torch.einsum("rm,brt->bmt", rs_w, d_r)
    return dacts, torch.cat([dacts * s * (1 - t * t), dacts * t * s * (1 - s)], 1)


def assert_dg(got, want, dacts, what):
    # 1e-5 of the GEMM's scale max|dacts|, expressed against max|want| (test_fused_wn_layer_backward)
    assert_close(got, want, 1e-5 * float(dacts.abs().max()) / max(1e-6, float(want.abs().max())) + 1e-6, what)


@bf3_only
@pytest.mark.gpu
@pytest.mark.parametrize("n,B,L,last,sums", [(128, 1, 256, False, True), (128, 2, 200, True, False), (1, 3, 40, False, True),
                                             (1, 2, 132, True, True), (33, 2, 200, False, False), (120, 3, 512, True, True),
                                             (120, 2, 328, False, True)])
def test_wn_layer_bwd_vs_fp64(n, B, L, last, sums):
    lib, g = _lib.load(), _gen(f"bw{n}-{B}-{L}-{last}")
    rs_w = rnd(g, n if last else 2 * n, n, k=n ** -0.5)
    d_a64, d_o64 = (None if last else rnd(g, B, n, L)), rnd(g, B, n, L)
    t, s = torch.tanh(rnd(g, B, n, L)), torch.sigmoid(rnd(g, B, n, L))
    dacts, want = _gate_backward_f64(rs_w, d_a64, d_o64, t, s)
    img = ops.wn_pack_bwd(_f32(rs_w), n, last)
    d_a, d_out, ts = (None if last else nan_in(d_a64)), nan_in(d_o64), nan_in(torch.cat([t, s], 1))
    n_wg = B * cdiv(L, 128)
    route = (LAYER_BWD, 0, 0, 0, 0, n_wg, 1, 1, cdiv(L, 128), 3, 1, 3 * (4 * 2048 + 2 * (4 * 1024 + 128)))

    def run():
        (bg, dg), (bs, rs) = out_buf((B, 2 * n, L)), (out_buf((256, n_wg)) if sums else (None, None))
        check_rc(lib.fst_wn_layer_bwd(_lib.ptr(d_a), d_out.data_ptr(), ts.data_ptr(), img.data_ptr(), img.numel() * 4, dg.data_ptr(),
                                      _lib.ptr(rs), n_wg if sums else 0, int(last), B, L, n, B * n * L, _lib.stream_ptr()), "bwd")
        last_route(route, "layer bwd")
        assert_fence(bg, dg, "dg")
        if sums:
            assert_fence(bs, rs, "row-sum table")
        return dg, rs

    dg, rs = run()
    assert_dg(dg, want, dacts, "dg")
    if sums:
        assert_row_sums(rs[: 2 * n].sum(dim=1), want, "row sums of dg")
    dg2, rs2 = run()
    assert torch.equal(dg2, dg) and (not sums or torch.equal(rs2[: 2 * n], rs[: 2 * n])), "two identical launches differ"
    if sums:                                                   # a table of the wrong extent is refused, nothing written
        (bg, dg3), (bs, rs3) = out_buf((B, 2 * n, L)), out_buf((256, n_wg))
        rc = lib.fst_wn_layer_bwd(_lib.ptr(d_a), d_out.data_ptr(), ts.data_ptr(), img.data_ptr(), img.numel() * 4, dg3.data_ptr(),
                                  rs3.data_ptr(), n_wg - 1, int(last), B, L, n, B * n * L, _lib.stream_ptr())
        assert rc == -1 and ops.wn_last_route() == (0,) * ops.WN_ROUTE_LEN
        torch.cuda.synchronize()
        assert_untouched(bg, dg3, "dg"), assert_untouched(bs, rs3, "row-sum table")


# --------------------------------------------------------------------------------------------------
# fused data gradient of in_layer + cond_layer: wn_layer_dgrad_kernel
# --------------------------------------------------------------------------------------------------
def _dgrad_f64(in_w, cond_w, dg, dil):
    """(W_inᵀ (*) dg, W_condᵀ·dg): the input gradients of the two forward convs, by autograd in fp64."""
    B, n2, L = dg.shape
    a = torch.zeros(B, n2 // 2, L, device=dg.device, dtype=torch.float64, requires_grad=True)
    u = torch.zeros(B, cond_w.size(1), L, device=dg.device, dtype=torch.float64, requires_grad=True)
    gg = F.conv1d(a, in_w, None, dilation=dil, padding=dil) + F.conv1d(u, cond_w)
    return torch.autograd.grad(gg, (a, u), dg)


def max_dgrad_dilation(n: int, h: int) -> int:
    lib = _lib.load()
    d = 1
    while lib.fst_wn_dgrad_fits(n, h, d + 1):
        d += 1
        assert d < 4096
    return d


@dataclass(frozen=True)
class Dg:
    n: int
    h: int
    B: int
    L: int
    dil: object         # int, or "max": the largest dilation fst_wn_dgrad_fits accepts
    res: bool = True
    sums: bool = True
    extra: int = 3      # guard channels of the d_u0 slice

    @property
    def id(self) -> str:
        return f"n{self.n}h{self.h}-B{self.B}L{self.L}d{self.dil}" + ("" if self.res else "-nores") + ("" if self.sums else "-nosums")


DG_CASES = [
    Dg(120, 25, 2, 512, 1), Dg(33, 31, 2, 1024, 16, res=False), Dg(16, 5, 3, 512, 64, sums=False), Dg(128, 32, 1, 512, 128),
    Dg(8, 3, 2, 200, 4), Dg(1, 1, 2, 132, 2, res=False, sums=False),
    Dg(8, 3, 300, 500, 16), Dg(8, 3, 131, 1024, 2, res=False),                   # more tiles than CUs: the persistent grid
    Dg(8, 3, 256, 512, 8),                                                      # as many tiles as CUs: one workgroup per tile
    Dg(16, 5, 2, 512, "max"), Dg(120, 25, 1, 200, "max", res=False),
]


@bf3_only
@pytest.mark.gpu
@pytest.mark.parametrize("c", DG_CASES, ids=lambda c: c.id)
def test_wn_layer_dgrad_vs_fp64(c: Dg):
    lib, g = _lib.load(), _gen("dg" + c.id)
    n, h, B, L = c.n, c.h, c.B, c.L
    dil = max_dgrad_dilation(n, h) if c.dil == "max" else c.dil
    route = layer_dgrad_expect(B, L, dil, _cus())
    assert route[9] == 2, "a dilation with a 3-slot ring"      # 3·slot > 160 KiB at every dilation >= 1 (512-sample tiles)
    n_wg = B * cdiv(L, 512)
    assert route[5] == (min(n_wg, _cus()))
    in_w, cond_w = rnd(g, 2 * n, n, 3, k=(3 * n) ** -0.5), rnd(g, 2 * n, h, 1, k=h ** -0.5)
    dg64, da64, du64 = rnd(g, B, 2 * n, L), (rnd(g, B, n, L) if c.res else None), rnd(g, B, h, L)
    da_ref, du_ref = _dgrad_f64(in_w, cond_w, dg64, dil)
    want_da = da_ref + (da64 if c.res else 0)
    img = ops.wn_pack_dgrad(_f32(in_w), _f32(cond_w), n, h)
    dg, d_a = nan_in(dg64), (nan_in(da64) if c.res else None)

    def call(dil_, d_a_new, d_u0, rs):
        return lib.fst_wn_layer_dgrad(dg.data_ptr(), img.data_ptr(), img.numel() * 4, _lib.ptr(d_a), d_a_new.data_ptr(), d_u0.data_ptr(),
                                      _lib.ptr(rs), n_wg if rs is not None else 0, B, L, n, h, dil_, B * n * L, (h + c.extra) * L,
                                      _lib.stream_ptr())

    def bufs(init_u0=True):
        return (out_buf((B, n, L)), out_buf((B, h, L), c.extra, 1, init=du64 if init_u0 else None),
                (out_buf((128, n_wg)) if c.sums else (None, None)))

    def run():
        (ba, d_a_new), (bu, d_u0), (bs, rs) = bufs()
        check_rc(call(dil, d_a_new, d_u0, rs), c.id)
        last_route(route, c.id)
        assert_fence(ba, d_a_new, "d_a_new"), assert_fence(bu, d_u0, "d_u0")
        if c.sums:
            assert_fence(bs, rs, "row-sum table")
        return d_a_new, d_u0, rs

    d_a_new, d_u0, rs = run()
    assert_close(d_a_new, want_da, 2e-5, "d_a")
    assert_close(d_u0, du_ref + du64, 2e-5, "d_u0")
    if c.sums:
        assert_row_sums(rs[:n].sum(dim=1), want_da, "row sums of d_a")
    again = run()
    assert torch.equal(again[0], d_a_new) and torch.equal(again[1], d_u0) and (not c.sums or torch.equal(again[2][:n], rs[:n]))
    if c.dil == "max":                                         # the first dilation that does not fit: refused, nothing written
        assert not lib.fst_wn_dgrad_fits(n, h, dil + 1)
        (ba, x), (bu, y), (bs, z) = bufs(init_u0=False)
        assert call(dil + 1, x, y, z) == -1 and ops.wn_last_route() == (0,) * ops.WN_ROUTE_LEN
        torch.cuda.synchronize()
        assert_untouched(ba, x, "d_a_new"), assert_untouched(bu, y, "d_u0")
        if c.sums:
            assert_untouched(bs, z, "row-sum table")


# --------------------------------------------------------------------------------------------------
# the forward of a WN stack in one launch: wn_stack_fwd_kernel
# --------------------------------------------------------------------------------------------------
@bf3_only
@pytest.mark.gpu
@pytest.mark.parametrize("n,h,B,L,nl", [(8, 3, 255, 256, 1), (8, 3, 256, 256, WS_MAXL), (16, 5, 257, 256, 3), (33, 7, 3, 1024, 4),
                                        (120, 25, 256, 512, 8)])
def test_wn_stack_fwd_vs_fp64(n, h, B, L, nl):
    """Layer i is checked against the fp64 layer applied to the a the kernel itself handed on (its a_next of layer i − 1), so
    the per-layer gates apply to every layer; ``out`` against the fp64 sum of those layers' skip rows."""
    lib, g = _lib.load(), _gen(f"sf{n}-{B}-{L}-{nl}")
    assert lib.fst_wn_stack_fwd_ok(n, h, L, nl) == 1 and lib.fst_wn_stack_fwd_ok(n, h, L, WS_MAXL + 1) == 0
    assert lib.fst_wn_stack_fwd_ok(n, h, L + 128, nl) == 0
    ws = [_layer_weights(g, n, h, i == nl - 1) for i in range(nl)]
    imgs = [_layer_image(w, n, h, i == nl - 1) for i, w in enumerate(ws)]
    a0_64, u64 = rnd(g, B, n, L), rnd(g, B, h, L)
    a0, u0 = nan_in(a0_64), nan_in(u64, 2, 1)
    grid = min(B, _cus())
    route = (STACK_FWD, 8, 0, 0, 0, grid, 1, 1, L // 256, 3, nl, wn_fwd_lds(8))

    def run():
        ts = [out_buf((B, 2 * n, L)) for _ in range(nl)]
        an = [out_buf((B, n, L)) for _ in range(nl - 1)]
        bo, out = out_buf((B, n, L))
        a_in = [a0] + [v for _, v in an]
        bs = (ctypes.c_int64 * nl)(*([n * L] * nl))
        check_rc(lib.fst_wn_stack_fwd(ptrs(a_in), bs, ptrs(imgs), imgs[0].numel() * 4, ptrs([v for _, v in ts]),
                                      ptrs([v for _, v in an] + [None]), u0.data_ptr(), (h + 2) * L, out.data_ptr(), nl, B, L, n, h,
                                      B * n * L, _lib.stream_ptr()), "stack fwd")
        last_route(route, "stack fwd")
        for k, (buf, v) in enumerate(ts + an + [(bo, out)]):
            assert_fence(buf, v, f"output {k}")
        return [v for _, v in ts], a_in, out

    ts, a_in, out = run()
    want_out = 0
    for i in range(nl):
        a_i = a0_64 if i == 0 else a_in[i].double()
        gg, t, s, res, skip = _layer_forward_f64(ws[i], a_i, u64, 1 << i, i == nl - 1)
        gtol = 1e-5 * float(gg.abs().max())
        assert_close(ts[i][:, :n], t, gtol, f"layer {i} t")
        assert_close(ts[i][:, n:], s, gtol, f"layer {i} s")
        if i < nl - 1:
            assert_close(a_in[i + 1], a_i + res, 2e-5, f"layer {i} a_next")
        want_out = want_out + skip
    assert_close(out, want_out, 2e-5, "out")
    ts2, a2, out2 = run()
    assert torch.equal(out2, out) and all(torch.equal(x, y) for x, y in zip(ts2, ts)) and all(torch.equal(x, y) for x, y in zip(a2, a_in))


# --------------------------------------------------------------------------------------------------
# the backward of a WN stack in one launch: wn_stack_bwd_kernel
# --------------------------------------------------------------------------------------------------
def max_stack_bwd_layers(n: int, h: int, L: int) -> int:
    lib = _lib.load()
    return max(nl for nl in range(1, WS_MAXL + 1) if lib.fst_wn_stack_bwd_ok(n, h, L, nl))


@bf3_only
@pytest.mark.gpu
@pytest.mark.parametrize("n,h,B,L,nl,sums", [(8, 3, 3, 132, 1, True), (16, 5, 5, 500, "max", True), (33, 31, 2, 100, 4, False),
                                             (8, 3, 300, 64, 3, True), (128, 32, 2, 512, 2, True), (120, 25, 256, 512, "max", True)])
def test_wn_stack_bwd_vs_fp64(n, h, B, L, nl, sums):
    """The full pass keeps every layer's dg and input cotangent: layer i is checked against the fp64 layer applied to the
    cotangent the kernel itself stored for layer i + 1.  The partial pass (one scratch dg, only layer 0's cotangent) is the same
    arithmetic with fewer stores: compared with the full pass at the data-gradient gate."""
    lib, g = _lib.load(), _gen(f"sb{n}-{B}-{L}-{nl}")
    if nl == "max":
        nl = max_stack_bwd_layers(n, h, L)
        assert nl < WS_MAXL and not lib.fst_wn_stack_bwd_ok(n, h, L, nl + 1)
        assert (1 << (nl - 1)) <= max_dgrad_dilation(n, h) < (1 << nl)
    assert lib.fst_wn_stack_bwd_ok(n, h, L, nl) == 1
    rs_w = [rnd(g, n if i == nl - 1 else 2 * n, n, k=n ** -0.5) for i in range(nl)]
    in_w = [rnd(g, 2 * n, n, 3, k=(3 * n) ** -0.5) for _ in range(nl)]
    cond_w = [rnd(g, 2 * n, h, 1, k=h ** -0.5) for _ in range(nl)]
    t = [torch.tanh(rnd(g, B, n, L)) for _ in range(nl)]
    s = [torch.sigmoid(rnd(g, B, n, L)) for _ in range(nl)]
    d_out64, du64 = rnd(g, B, n, L), rnd(g, B, h, L)
    img_b = [ops.wn_pack_bwd(_f32(rs_w[i]), n, i == nl - 1, acc_order=True) for i in range(nl)]
    img_d = [ops.wn_pack_dgrad(_f32(in_w[i]), _f32(cond_w[i]), n, h) for i in range(nl)]
    ts = [nan_in(torch.cat([t[i], s[i]], 1)) for i in range(nl)]
    d_out = nan_in(d_out64)
    grid = min(B, _cus())
    lds = max([16 * 8192 + 8192] + [2 * dgrad_slot(1 << i) for i in range(nl)])
    route = (STACK_BWD, 0, 0, 0, 0, grid, 1, 1, 1, 2, nl, lds)

    def run(partial: bool):
        dgs = [out_buf((B, 2 * n, L))] * nl if partial else [out_buf((B, 2 * n, L)) for _ in range(nl)]
        das = [out_buf((B, n, L))] + [None if partial else out_buf((B, n, L)) for _ in range(nl - 1)]
        bu, d_u0 = out_buf((B, h, L), 3, 1, init=du64)
        with_sums = sums and not partial
        rb = [out_buf((256, B)) for _ in range(nl)] if with_sums else None
        rd = [out_buf((128, B)) for _ in range(nl)] if with_sums else None
        check_rc(lib.fst_wn_stack_bwd(ptrs(ts), ptrs(img_b), ptrs(img_d), ptrs([v for _, v in dgs]),
                                      ptrs([None if x is None else x[1] for x in das]),
                                      ptrs([v for _, v in rb]) if with_sums else None, ptrs([v for _, v in rd]) if with_sums else None,
                                      d_out.data_ptr(), d_u0.data_ptr(), (h + 3) * L, nl, B, L, n, h, B * n * L, _lib.stream_ptr()),
                 "stack bwd")
        last_route(route, f"stack bwd (partial={partial})")
        for k, x in enumerate(dgs[:1] if partial else dgs):
            assert_fence(*x, f"dg {k}")
        for k, x in enumerate(das):
            if x is not None:
                assert_fence(*x, f"d_a {k}")
        assert_fence(bu, d_u0, "d_u0")
        for k, x in enumerate((rb or []) + (rd or [])):
            assert_fence(*x, f"row-sum table {k}")
        return ([v for _, v in dgs], [None if x is None else x[1] for x in das], d_u0,
                None if rb is None else [v for _, v in rb], None if rd is None else [v for _, v in rd])

    dgs, das, d_u0, rb, rd = run(False)
    want_u0 = du64
    for i in reversed(range(nl)):
        d_a_in = None if i == nl - 1 else das[i + 1].double()
        dacts, want_dg = _gate_backward_f64(rs_w[i], d_a_in, d_out64, t[i], s[i])
        assert_dg(dgs[i], want_dg, dacts, f"layer {i} dg")
        da_ref, du_ref = _dgrad_f64(in_w[i], cond_w[i], dgs[i].double(), 1 << i)
        want_da = da_ref + (0 if d_a_in is None else d_a_in)
        assert_close(das[i], want_da, 2e-5, f"layer {i} d_a")
        want_u0 = want_u0 + du_ref
        if sums:
            assert_row_sums(rb[i][: 2 * n].sum(dim=1), want_dg, f"layer {i} row sums of dg")
            assert_row_sums(rd[i][:n].sum(dim=1), want_da, f"layer {i} row sums of d_a")
    assert_close(d_u0, want_u0, 2e-5, "d_u0")
    again = run(False)
    assert torch.equal(again[2], d_u0) and all(torch.equal(x, y) for x, y in zip(again[0] + again[1], dgs + das))
    if sums:
        assert all(torch.equal(x[: 2 * n], y[: 2 * n]) for x, y in zip(again[3], rb))
        assert all(torch.equal(x[:n], y[:n]) for x, y in zip(again[4], rd))
    p_dgs, p_das, p_u0, _, _ = run(True)
    assert_close(p_das[0], das[0], 2e-5, "partial pass: layer 0 d_a vs the full pass")
    assert_close(p_u0, d_u0, 2e-5, "partial pass: d_u0 vs the full pass")
    assert_close(p_dgs[0], dgs[0], 2e-5, "partial pass: the scratch dg holds layer 0's")
