"""The four weight-image formats of the fused WN kernels (csrc/wn_fused.hip), byte for byte against a plain-torch restatement of the
layout comments there: forward, backward (acc_order off and on), data gradient, and the d_a stages and closing zeros of the projected
backward format (its skip stages hold an fp32 fmaf chain: tests/test_gpu_wn_skip_proj.py).  Every image is packed through the raw ABI,
by the per-layer entry point and by the stack entry point, between two canary bands, and compared as int32 with no tolerance: an
image holds copies of weights split as  hi = bf16(v), lo = bf16(v - hi)  (two roundings torch reproduces exactly).

The restatement, shared by all formats: a 2 KiB block = 64 lanes x 8 bf16 of hi, then the same of lo; lane l holds row l & 31 of the
block's 32 rows at k = 8 (l >> 5) + j; the first element of a pair sits in the low half of its dword."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from feature_level_style_transfer_for_tsc_amd import _lib, ops

DEV = "cuda"
BAND = 64                                     # int32 words either side of an image; keeps it 16-byte aligned
CANARY = 0x4B1D4B1D
ONE = 0x3F800000


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _blocks(rows_k: torch.Tensor) -> torch.Tensor:
    """[nb, 32 rows, 2 lane halves, 8] fp32 (row r, element j of half hh) -> the nb blocks as int32 words."""
    v = rows_k.permute(0, 2, 1, 3).contiguous()                               # lane = 32 hh + r
    hi = v.bfloat16()
    lo = (v - hi.float()).bfloat16()
    return torch.stack([hi, lo], 1).contiguous().view(torch.int16).view(torch.int32).reshape(-1)


def _stage(m: torch.Tensor) -> torch.Tensor:
    """A stage [32 nb rows, 16 k] in plain order (k = 8 hh + j) -> int32 words of its nb row blocks."""
    return _blocks(m.reshape(-1, 32, 2, 8))


def _acc_k() -> torch.Tensor:
    """[2 hh, 8 j] -> 8 (j >> 2) + 4 hh + (j & 3): the order in which a 32x32 accumulator tile delivers 16 of its rows as a B operand."""
    hh, j = torch.arange(2).view(2, 1), torch.arange(8).view(1, 8)
    return 8 * (j >> 2) + 4 * hh + (j & 3)


def _tail(*words) -> torch.Tensor:
    return torch.tensor([w for w in words for _ in range(4)], dtype=torch.int32)


def _chunk_tap_order(CH):
    """GEMM-1 stages: chunks in groups of two, tap-major inside a group."""
    for g in range(0, CH, 2):
        for tap in range(3):
            for c in range(g, min(g + 2, CH)):
                yield c, tap


def fwd_image(in_w, cond_w, in_b, cond_b, rs_w, rs_b, n, h, last):
    CH, CH2 = (n + 15) // 16, (h + 1 + 15) // 16
    g1 = torch.zeros(3, 256, CH * 16)                                          # rows: blocks 0-3 tanh, 4-7 sigmoid
    cond = torch.zeros(256, CH2 * 16)
    for half in (0, 1):
        rows = slice(half * n, (half + 1) * n)
        g1[:, half * 128: half * 128 + n, :n] = in_w[rows].permute(2, 0, 1)
        cond[half * 128: half * 128 + n, :h] = cond_w[rows].reshape(n, h)
        cond[half * 128: half * 128 + n, h] = in_b[rows] + cond_b[rows]        # the constant-one channel carries the biases
    parts = [_stage(g1[tap][:, 16 * c: 16 * c + 16]) for c, tap in _chunk_tap_order(CH)]
    parts += [_stage(cond[:, 16 * s: 16 * s + 16]) for s in range(CH2)]
    g2 = torch.zeros(256, 128)                                                 # rows: blocks 0-3 residual, 4-7 skip; k = n carries b_rs
    if not last:
        g2[:n, :n], g2[:n, n] = rs_w[:n].reshape(n, n), rs_b[:n]
    skip = slice(0, n) if last else slice(n, 2 * n)
    g2[128: 128 + n, :n], g2[128: 128 + n, n] = rs_w[skip].reshape(n, n), rs_b[skip]
    for kb in range(4):
        for s in range(2):
            parts.append(_blocks(g2[:, kb * 32 + 16 * s + _acc_k()].reshape(8, 32, 2, 8)))
    return torch.cat(parts + [_tail(0, ONE)])


def bwd_stage(rs_w, n, src, c, acc):
    """Stage (src, c) of W_rs transposed: element (hh, j) = channel row src n + 16 c + k(hh, j), block rows = acts channels."""
    CH = (n + 15) // 16
    wt = torch.zeros(CH * 16, 128)
    wt[:n, :n] = rs_w[src * n: (src + 1) * n].reshape(n, n)
    hh, j = torch.arange(2).view(2, 1), torch.arange(8).view(1, 8)
    k = _acc_k() if acc else 8 * hh + j
    return _blocks(wt[16 * c + k].permute(2, 0, 1).reshape(4, 32, 2, 8))


def bwd_image(rs_w, n, last, acc_order):
    CH = (n + 15) // 16
    parts = [bwd_stage(rs_w, n, src, c, bool(acc_order) and not last and src == 0) for src in range(1 if last else 2) for c in range(CH)]
    return torch.cat(parts + [_tail(0)])


def dgrad_image(in_w, cond_w, n, h):
    CHK = (2 * n + 15) // 16
    wt = torch.zeros(3, 128, CHK * 16)                                         # [tap][d_a row m][dg channel k]
    wt[:, :n, : 2 * n] = in_w.permute(2, 1, 0)
    ct = torch.zeros(32, CHK * 16)                                             # [d_u0 row][dg channel k]
    ct[:h, : 2 * n] = cond_w.reshape(2 * n, h).t()
    parts = []
    for c in range(CHK):
        k = slice(16 * c, 16 * c + 16)
        parts += [_stage(wt[0][:, k]), _stage(wt[1][:, k]), _stage(ct[:, k]), _stage(wt[2][:, k])]
    return torch.cat(parts + [_tail(0)])


# ---------------------------------------------------------------------------------------------------------------- the device side
def _weights(n, h, nl, seed, lasts=None):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g)
    lasts = [i == nl - 1 for i in range(nl)] if lasts is None else lasts
    return [(r(2 * n, n, 3), r(2 * n, h, 1), r(2 * n), r(2 * n), r(n if last else 2 * n, n, 1), r(n if last else 2 * n)) for last in lasts]


def _dev(layers):
    return [tuple(t.to(DEV) for t in l) for l in layers]


def _image(nbytes):
    buf = torch.full((nbytes // 4 + 2 * BAND,), CANARY, device=DEV, dtype=torch.int32)
    return buf[BAND: BAND + nbytes // 4], buf


def _assert_image(got, want, what):
    view, buf = got
    assert want.numel() == view.numel(), f"{what}: the restatement has {want.numel()} words, the image {view.numel()}"
    band = torch.full((BAND,), CANARY, dtype=torch.int32)
    host = buf.cpu()
    diff = (host != torch.cat([band, want, band])).nonzero().flatten()
    assert diff.numel() == 0, f"{what}: {diff.numel()} words differ, the first at word {int(diff[0]) - BAND} of {want.numel()}"


def _pack(entry, *args):
    _lib.check(getattr(_lib.load(), entry)(*args, _lib.stream_ptr()), entry)


def _check_fwd(W, n, h, lasts):
    """Every layer by fst_wn_pack, then the stack (its top layer the last one) by fst_wn_pack_stack."""
    lib, D, tbl = _lib.load(), _dev(W), ops._ptr_table
    want = [fwd_image(*l, n, h, last) for l, last in zip(W, lasts)]
    nb = lib.fst_wn_image_bytes(n, h)
    for i, l in enumerate(D):
        img = _image(nb)
        _pack("fst_wn_pack", *[t.data_ptr() for t in l], n, h, 3, int(lasts[i]), img[0].data_ptr(), nb)
        _assert_image(img, want[i], f"fst_wn_pack n={n} h={h} last={int(lasts[i])}")
    imgs = [_image(nb) for _ in D]
    _pack("fst_wn_pack_stack", *[tbl([l[j] for l in D]) for j in range(6)], len(D), n, h, 3, tbl([m[0] for m in imgs]), nb)
    for i, img in enumerate(imgs):
        _assert_image(img, want[i], f"fst_wn_pack_stack n={n} h={h} layer {i} of {len(D)}")


def _check_bwd(W, n, lasts, acc_order):
    lib, D, tbl = _lib.load(), _dev(W), ops._ptr_table
    want = [bwd_image(l[4], n, last, acc_order) for l, last in zip(W, lasts)]
    sizes = [lib.fst_wn_bwd_image_bytes(n, int(last)) for last in lasts]
    for i, l in enumerate(D):
        img = _image(sizes[i])
        _pack("fst_wn_pack_bwd", l[4].data_ptr(), n, int(lasts[i]), acc_order, img[0].data_ptr(), sizes[i])
        _assert_image(img, want[i], f"fst_wn_pack_bwd n={n} last={int(lasts[i])} acc_order={acc_order}")
    imgs = [_image(s) for s in sizes]
    _pack("fst_wn_pack_bwd_stack", tbl([l[4] for l in D]), len(D), n, acc_order, tbl([m[0] for m in imgs]), lib.fst_wn_bwd_image_bytes(n, 0))
    for i, img in enumerate(imgs):
        _assert_image(img, want[i], f"fst_wn_pack_bwd_stack n={n} acc_order={acc_order} layer {i} of {len(D)}")


def _check_dgrad(W, n, h):
    lib, D, tbl = _lib.load(), _dev(W), ops._ptr_table
    want = [dgrad_image(l[0], l[1], n, h) for l in W]
    nb = lib.fst_wn_dgrad_image_bytes(n)
    for i, l in enumerate(D):
        img = _image(nb)
        _pack("fst_wn_pack_dgrad", l[0].data_ptr(), l[1].data_ptr(), n, h, 3, img[0].data_ptr(), nb)
        _assert_image(img, want[i], f"fst_wn_pack_dgrad n={n} h={h}")
    imgs = [_image(nb) for _ in D]
    _pack("fst_wn_pack_dgrad_stack", tbl([l[0] for l in D]), tbl([l[1] for l in D]), len(D), n, h, 3, tbl([m[0] for m in imgs]), nb)
    for i, img in enumerate(imgs):
        _assert_image(img, want[i], f"fst_wn_pack_dgrad_stack n={n} h={h} layer {i} of {len(D)}")


# a stack entry point packs its top layer as the last one: last = 1 goes through a stack of one, last = 0 is layer 0 of a stack of two
def _lasts(last):
    return [True] if last else [False, True]


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("n,h", [(1, 1), (15, 15), (16, 16), (17, 31), (127, 25)])
def test_forward_image(n, h, last):
    lasts = _lasts(last)
    _check_fwd(_weights(n, h, len(lasts), 1000 * n + 10 * h + last, lasts), n, h, lasts)


@pytest.mark.parametrize("acc_order", [0, 1])
@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("n", [1, 16, 17, 128])
def test_backward_image(n, last, acc_order):
    lasts = _lasts(last)
    _check_bwd(_weights(n, 1, len(lasts), 100 * n + 2 * last + acc_order, lasts), n, lasts, acc_order)


@pytest.mark.parametrize("n,h", [(1, 1), (8, 32), (17, 5), (128, 32)])
def test_data_gradient_image(n, h):
    _check_dgrad(_weights(n, h, 2, 1000 * n + h), n, h)


@pytest.mark.parametrize("h2", [6, 64])
def test_projected_image_d_a_stages_and_tail(h2):
    lib, tbl, n, nl = _lib.load(), ops._ptr_table, 17, 3
    CH, CHO = (n + 15) // 16, (h2 + 15) // 16
    W = _weights(n, 1, nl, 7 + h2)
    end_w = torch.randn(h2, n, generator=torch.Generator().manual_seed(h2)).to(DEV)
    rs = [l[4].to(DEV) for l in W]
    sizes = [lib.fst_wn_bwd_proj_image_bytes(n, h2, int(i == nl - 1)) for i in range(nl)]
    imgs = [_image(s) for s in sizes]
    _pack("fst_wn_pack_bwd_proj_stack", tbl(rs), end_w.data_ptr(), nl, n, h2, tbl([m[0] for m in imgs]), sizes[0])
    band = torch.full((BAND,), CANARY, dtype=torch.int32)
    for i, (view, buf) in enumerate(imgs):
        n_da = 0 if i == nl - 1 else CH
        assert sizes[i] == (n_da + CHO) * 8192 + 16
        host = buf.cpu()
        assert torch.equal(host[:BAND], band) and torch.equal(host[-BAND:], band), f"layer {i} wrote outside its image"
        img = host[BAND: -BAND]
        assert not bool((img == CANARY).any()), f"layer {i} left part of its image unwritten"
        want = torch.cat([bwd_stage(W[i][4], n, 0, c, True) for c in range(n_da)] + [torch.zeros(0, dtype=torch.int32)])
        assert torch.equal(img[: n_da * 2048], want), f"layer {i}: d_a stages"
        assert torch.equal(img[(n_da + CHO) * 2048:], _tail(0)), f"layer {i}: closing zeros"


@pytest.mark.parametrize("nl", [1, 2, 10])
def test_stack_images(nl):
    n = 17
    W = _weights(n, 16, nl, 50 + nl)
    lasts = [i == nl - 1 for i in range(nl)]
    _check_fwd(W, n, 16, lasts)
    for acc_order in (0, 1):
        _check_bwd(W, n, lasts, acc_order)
    _check_dgrad(_weights(n, 5, nl, 60 + nl), n, 5)
