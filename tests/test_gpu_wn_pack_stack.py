"""fst_wn_pack_stack / fst_wn_pack_bwd_stack / fst_wn_pack_dgrad_stack (the weight images of every layer of a WN stack in one
launch per format) against the per-layer calls fst_wn_pack / fst_wn_pack_bwd / fst_wn_pack_dgrad: the images are the same bytes,
and nothing is written outside them (canary bands either side of every image)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from feature_level_style_transfer_for_tsc_amd import _lib, ops

DEV = "cuda"
BAND = 64                                     # floats; keeps the images 16-byte aligned
CANARY = 0x4B1D4B1D                           # an int32 pattern (the images are compared as int32: bf16 pairs may look like NaNs)


def _image(nbytes):
    buf = torch.full((nbytes // 4 + 2 * BAND,), CANARY, device=DEV, dtype=torch.int32)
    return buf[BAND: BAND + nbytes // 4], buf


def _intact(buf):
    return bool((buf[:BAND] == CANARY).all()) and bool((buf[-BAND:] == CANARY).all())


def _weights(n, h, nl, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g, device=DEV, dtype=torch.float32)
    layers = []
    for i in range(nl):
        rows = n if i == nl - 1 else 2 * n
        layers.append((r(2 * n, n, 3), r(2 * n, h, 1), r(2 * n), r(2 * n), r(rows, n, 1), r(rows)))
    return layers


def _compare(per_layer, stacked, what):
    for i, ((a, abuf), (b, bbuf)) in enumerate(zip(per_layer, stacked)):
        assert _intact(abuf) and _intact(bbuf), f"{what}: layer {i} wrote outside its image"
        assert not bool((b == CANARY).any()), f"{what}: layer {i} left part of its image unwritten"
        assert torch.equal(a, b), f"{what}: layer {i} differs from the per-layer image"


@pytest.mark.parametrize("nl", [3, 8])
@pytest.mark.parametrize("h", [5, 25])
@pytest.mark.parametrize("n", [16, 120])
def test_stack_images_equal_per_layer_images(n, h, nl):
    lib, stream, tbl = _lib.load(), _lib.stream_ptr(), ops._ptr_table
    W = _weights(n, h, nl, seed=n + 7 * h + nl)
    col = lambda j: tbl([l[j] for l in W])

    nb = lib.fst_wn_image_bytes(n, h)
    one, many = [_image(nb) for _ in range(nl)], [_image(nb) for _ in range(nl)]
    for i, l in enumerate(W):
        assert lib.fst_wn_pack(*[t.data_ptr() for t in l], n, h, 3, int(i == nl - 1), one[i][0].data_ptr(), nb, stream) == 0
    assert lib.fst_wn_pack_stack(*[col(j) for j in range(6)], nl, n, h, 3, tbl([m[0] for m in many]), nb, stream) == 0
    _compare(one, many, "forward image")

    nb = lib.fst_wn_dgrad_image_bytes(n)
    one, many = [_image(nb) for _ in range(nl)], [_image(nb) for _ in range(nl)]
    for i, l in enumerate(W):
        assert lib.fst_wn_pack_dgrad(l[0].data_ptr(), l[1].data_ptr(), n, h, 3, one[i][0].data_ptr(), nb, stream) == 0
    assert lib.fst_wn_pack_dgrad_stack(col(0), col(1), nl, n, h, 3, tbl([m[0] for m in many]), nb, stream) == 0
    _compare(one, many, "data-gradient image")

    for acc_order in (0, 1):
        sizes = [lib.fst_wn_bwd_image_bytes(n, int(i == nl - 1)) for i in range(nl)]
        assert sizes[-1] < sizes[0]                                     # the top layer has the skip rows only
        one, many = [_image(s) for s in sizes], [_image(s) for s in sizes]
        for i, l in enumerate(W):
            assert lib.fst_wn_pack_bwd(l[4].data_ptr(), n, int(i == nl - 1), acc_order, one[i][0].data_ptr(), sizes[i], stream) == 0
        assert lib.fst_wn_pack_bwd_stack(col(4), nl, n, acc_order, tbl([m[0] for m in many]), sizes[0], stream) == 0
        _compare(one, many, f"backward image (acc_order={acc_order})")


def test_stack_pack_refuses_bad_tables():
    lib, stream, tbl = _lib.load(), _lib.stream_ptr(), ops._ptr_table
    n, h, nl = 16, 5, 3
    W = _weights(n, h, nl, seed=1)
    col = lambda j: tbl([l[j] for l in W])
    nb = lib.fst_wn_image_bytes(n, h)
    imgs = [_image(nb) for _ in range(nl)]
    assert lib.fst_wn_pack_stack(*[col(j) for j in range(6)], 11, n, h, 3, tbl([m[0] for m in imgs]), nb, stream) != 0   # > 10 layers
    assert lib.fst_wn_pack_stack(*[col(j) for j in range(6)], nl, n, h, 3, tbl([m[0] for m in imgs]), nb - 16, stream) != 0
    assert lib.fst_wn_pack_stack(*[col(j) for j in range(6)], nl, n, h, 3, tbl([imgs[0][0], None, imgs[2][0]]), nb, stream) != 0
    torch.cuda.synchronize()
    assert all(bool((m[1] == CANARY).all()) for m in imgs)
