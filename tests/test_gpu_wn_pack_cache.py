"""The Python wrappers of the four WN weight-image formats (ops.wn_pack_layer(s), wn_pack_bwd(_layers) with acc_order off and on,
wn_pack_bwd_proj_layers, wn_pack_dgrad(_layers)) and their use of ``ops.pack_cache``: which call launches, which returns a cached
object, what a partial hit does, what a cache entry keeps alive.  The images themselves are checked against the C entry points
in tests/test_gpu_wn_pack_stack.py and against fp64 in tests/test_gpu_wn_skip_proj.py; here they are only compared with each
other, as int32 (bf16 pairs may look like NaNs)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from feature_level_style_transfer_for_tsc_amd import _lib, ops

DEV = "cuda"
N, H, H2, NL = 8, 3, 6, 3


def _weights(nl, seed, strided=False):
    """Per layer (in_w, cond_w, in_b, cond_b, rs_w, rs_b), and end_w.  ``strided``: the weight every format reads (in_w for the data
    gradient, rs_w for the others) is a non-contiguous view."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g, device=DEV, dtype=torch.float32)
    view = (lambda t: torch.stack((t, t), dim=1)[:, 0]) if strided else (lambda t: t)      # (the same values, every other row)
    layers = []
    for i in range(nl):
        rows = N if i == nl - 1 else 2 * N
        layers.append((view(r(2 * N, N, 3)), r(2 * N, H, 1), r(2 * N), r(2 * N), view(r(rows, N, 1)), r(rows)))
    return layers, r(H2, N, 1)


class Format:
    """One image format: ``stack(W, end_w)`` the call for a whole stack, ``one(W, i)`` the per-layer call (None: the format has
    none), ``weight(W, i)`` a weight of layer i that the image is made of."""

    def __init__(self, name, stack, one, weight):
        self.name, self.stack, self.one, self.weight = name, stack, one, weight

    def __repr__(self):
        return self.name


def _bwd(acc_order):
    return Format(f"bwd-acc{int(acc_order)}", lambda W, e: ops.wn_pack_bwd_layers([l[4] for l in W], N, acc_order),
                  lambda W, i: ops.wn_pack_bwd(W[i][4], N, i == len(W) - 1, acc_order), lambda W, i: W[i][4])


FORMATS = [Format("fwd", lambda W, e: ops.wn_pack_layers(W, N, H), lambda W, i: ops.wn_pack_layer(*W[i], N, H, i == len(W) - 1),
                  lambda W, i: W[i][4]),
           _bwd(False), _bwd(True),
           Format("proj", lambda W, e: ops.wn_pack_bwd_proj_layers([l[4] for l in W], e, N), None, lambda W, i: W[i][4]),
           Format("dgrad", lambda W, e: ops.wn_pack_dgrad_layers([l[0] for l in W], [l[1] for l in W], N, H),
                  lambda W, i: ops.wn_pack_dgrad(W[i][0], W[i][1], N, H), lambda W, i: W[i][0])]
formats = pytest.mark.parametrize("f", FORMATS, ids=repr)


def _bits(img):
    return img.view(torch.int32)


def _same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _proj_abi(W, end_w):
    """fst_wn_pack_bwd_proj_stack on the same weights, through the ABI."""
    lib, nl = _lib.load(), len(W)
    sizes = [lib.fst_wn_bwd_proj_image_bytes(N, H2, int(i == nl - 1)) for i in range(nl)]
    imgs = [torch.empty(s // 4, device=DEV, dtype=torch.float32) for s in sizes]
    src = [l[4].contiguous() for l in W]
    assert lib.fst_wn_pack_bwd_proj_stack(ops._ptr_table(src), end_w.data_ptr(), nl, N, H2, ops._ptr_table(imgs), sizes[0],
                                          _lib.stream_ptr()) == 0
    return imgs


def _per_layer(f, W, end_w):
    """The images of the stack, not from the stack call: the per-layer calls, or the C entry point for the projected form."""
    assert ops._PACK_CACHE is None
    return _proj_abi(W, end_w) if f.one is None else [f.one(W, i) for i in range(len(W))]


@formats
def test_outside_the_scope_every_call_launches(f):
    W, e = _weights(NL, 1)
    assert ops._PACK_CACHE is None
    a, b = f.stack(W, e), f.stack(W, e)
    assert len(a) == NL and _same_bits(a, _per_layer(f, W, e))
    assert _same_bits(a, b) and all(x is not y and x.data_ptr() != y.data_ptr() for x, y in zip(a, b))
    if f.one is not None:
        assert f.one(W, 1) is not f.one(W, 1)
    assert ops._PACK_CACHE is None


@formats
def test_inside_the_scope_the_second_call_is_a_hit(f):
    W, e = _weights(NL, 2)
    with ops.pack_cache():
        a = f.stack(W, e)
        b = f.stack(W, e)
        assert all(x is y for x, y in zip(a, b)) and len(ops._PACK_CACHE) == NL
        if f.one is not None:                                   # the per-layer key is the stack's key of that layer
            assert all(f.one(W, i) is a[i] for i in range(NL)) and len(ops._PACK_CACHE) == NL
    assert ops._PACK_CACHE is None and _same_bits(a, _per_layer(f, W, e))


@formats
def test_partial_hit(f):
    W, e = _weights(NL, 3)
    want = _per_layer(f, W, e)
    with ops.pack_cache():
        if f.one is not None:                                   # layer 1 is cached: the stack call keeps it and packs the others
            mid = f.one(W, 1)
            got = f.stack(W, e)
            assert got[1] is mid and got[0] is not mid and got[2] is not mid
            assert f.stack(W, e)[0] is got[0]                   # ... under their own keys
        else:                                                   # no per-layer call: the whole stack is packed again
            first = f.stack(W, e)
            version = W[1][4]._version
            W[1][4].add_(0)
            assert W[1][4]._version > version
            got = f.stack(W, e)
            assert all(x is not y for x, y in zip(got, first))
            assert all(x is y for x, y in zip(f.stack(W, e), got))        # and the entries were overwritten
        assert len(got) == NL and _same_bits(got, want)


@formats
def test_a_changed_weight_gives_a_new_image_of_that_layer_only(f):
    W, e = _weights(NL, 4)
    with ops.pack_cache():
        before = f.stack(W, e)
        f.weight(W, 1).mul_(2.0)
        after = f.stack(W, e)
        assert after[1] is not before[1] and not torch.equal(_bits(after[1]), _bits(before[1]))
        for i in (0, 2):
            assert torch.equal(_bits(after[i]), _bits(before[i]))
            assert (after[i] is before[i]) == (f.one is not None)
    assert _same_bits(after, _per_layer(f, W, e))


@formats
def test_a_stack_deeper_than_the_layer_tables(f):
    nl = ops.WN_PACK_MAX_LAYERS + 1
    assert nl == 11
    W, e = _weights(nl, 5)
    if f.one is None:
        with pytest.raises(ValueError, match="at most 10 layers"):
            f.stack(W, e)
        return
    want = _per_layer(f, W, e)
    assert _same_bits(f.stack(W, e), want)
    with ops.pack_cache():
        got = f.stack(W, e)
        assert _same_bits(got, want) and all(f.one(W, i) is got[i] for i in range(nl))


def _flat(entry):
    for x in entry:
        if isinstance(x, (tuple, list)):
            yield from _flat(x)
        else:
            yield x


@formats
def test_an_entry_keeps_the_weights_and_their_contiguous_copies(f):
    W, e = _weights(NL, 6, strided=True)
    dense, _ = _weights(NL, 6)
    assert all(not f.weight(W, i).is_contiguous() and torch.equal(f.weight(W, i), f.weight(dense, i)) for i in range(NL))
    calls = [lambda: f.stack(W, e)] + ([] if f.one is None else [lambda: [f.one(W, 1)]])      # a stack's entries, a per-layer call's
    for call in calls:
        with ops.pack_cache():
            for img in call():
                (entry,) = [v for v in ops._PACK_CACHE.values() if v[0] is img]
                i = next(i for i in range(NL) if any(x is f.weight(W, i) for x in _flat(entry)))      # the original weight
                kept = [x for x in _flat(entry) if isinstance(x, torch.Tensor) and x is not img]
                assert any(x.is_contiguous() and x.shape == f.weight(W, i).shape and torch.equal(x, f.weight(W, i))
                           and x.data_ptr() != f.weight(W, i).data_ptr() for x in kept), (f, i)
    assert _same_bits(f.stack(W, e), _per_layer(f, dense, e))      # and the image is the dense weights' image
