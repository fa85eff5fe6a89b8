"""fst_wn_wgrad_in_slabs / _rs_slabs + fst_wn_wgrad_reduce_many (one reduction launch for the slab sets of a WN's layers) through
the C ABI: bit for bit the gradients of the per-layer entry points fst_wn_wgrad_in / _rs, which add their own slabs, and within
1e-4 of fp64 einsums (the tolerance of test_time_as_k_weight_gradient_kernels).  Gradients sit between canary bands, workspaces
have exactly the queried size (a band behind them too); a refused call writes nothing."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from feature_level_style_transfer_for_tsc_amd import _lib, ops
from test_gpu_kernels import assert_close

DEV = "cuda"
BAND, CANARY = 64, 12345.0


def _rnd(gen, *shape):
    return torch.randn(*shape, generator=gen, device=DEV, dtype=torch.float32)


def _banded(*shape):
    """A contiguous tensor of ``shape`` with BAND canary floats either side in the same allocation; returns (view, whole buffer)."""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((numel + 2 * BAND,), CANARY, device=DEV)
    return buf[BAND: BAND + numel].view(*shape), buf


def _bands_intact(buf):
    return bool((buf[:BAND] == CANARY).all()) and bool((buf[-BAND:] == CANARY).all())


class _Stack:
    """Operands of the entries (kind, layer) of one WN: ``n_sets`` applications, layer i at dilation dils[i]."""

    def __init__(self, n, h, B, L, dils, n_sets, entries, seed):
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.n, self.h, self.B, self.L, self.dils, self.ns, self.entries, self.nl = n, h, B, L, dils, n_sets, entries, len(dils)
        self.u0 = [_rnd(g, B, 2 * h, L)[:, :h] for _ in range(n_sets)]          # channel-slice views, as the flow passes them
        self.d_out = [_rnd(g, B, n, L) for _ in range(n_sets)]
        self.a, self.dg, self.ts, self.d_a = {}, {}, {}, {}
        for kind, i in entries:
            if kind == 0:
                self.a[i] = []
                for _ in range(n_sets):
                    t = ops.empty_with_slack(B, n, L, DEV)                      # (dilations 1-3 read up to 3 floats outside a row)
                    t.untyped_storage().copy_(torch.full((B * n * L + 8,), float("nan")).untyped_storage())
                    t.copy_(_rnd(g, B, n, L))
                    self.a[i].append(t)
                self.dg[i] = [_rnd(g, B, 2 * n, L) for _ in range(n_sets)]
            else:
                self.ts[i] = [_rnd(g, B, 2 * n, L) for _ in range(n_sets)]
                self.d_a[i] = [_rnd(g, B, n, L) for _ in range(n_sets)]
        self.lib = _lib.load()

    def last(self, i):
        return i == self.nl - 1

    def targets(self):
        """Per entry (dw0, dw1 | None) between canary bands, and the buffers that hold them."""
        out, bufs = [], []
        n, h = self.n, self.h
        for kind, i in self.entries:
            if kind == 0:
                (t0, b0), (t1, b1) = _banded(2 * n, n, 3), _banded(2 * n, h, 1)
                out.append((t0, t1))
                bufs += [b0, b1]
            else:
                t0, b0 = _banded(n if self.last(i) else 2 * n, n, 1)
                out.append((t0, None))
                bufs.append(b0)
        return out, bufs

    def workspace(self, kind, i):
        ws_n = self.lib.fst_wn_wgrad_workspace_floats(kind, self.B, self.L, self.n, self.h, int(kind == 1 and self.last(i)))
        assert ws_n > 0
        buf = torch.full((ws_n + BAND,), CANARY, device=DEV)                   # exactly ws_n floats are the kernel's
        return buf[:ws_n], ws_n, buf

    def product(self, kind, i, ws, ws_n, dw, reduce):
        """The (kind, layer) product: with its own reduction into ``dw`` (the per-layer entry points) or leaving its slabs."""
        lib, B, L, n, h, P, stream = self.lib, self.B, self.L, self.n, self.h, ops._ptr_sets, _lib.stream_ptr()
        numel = B * n * L
        if kind == 0:
            u0_bs = self.u0[0].stride(0)
            head = (P(self.dg[i]), P(self.a[i]), P(self.u0), self.ns, u0_bs)
            tail = (ws.data_ptr(), ws_n, B, L, n, h, self.dils[i], 1, numel, stream)
            if reduce:
                return lib.fst_wn_wgrad_in(*head, dw[0].data_ptr(), dw[1].data_ptr(), *tail)
            return lib.fst_wn_wgrad_in_slabs(*head, *tail)
        last = self.last(i)
        head = (None if last else P(self.d_a[i]), P(self.d_out), P(self.ts[i]), self.ns)
        tail = (ws.data_ptr(), ws_n, int(last), B, L, n, numel, stream)
        if reduce:
            return lib.fst_wn_wgrad_rs(*head, dw[0].data_ptr(), *tail)
        return lib.fst_wn_wgrad_rs_slabs(*head, *tail)

    def reduce_many(self, wss, targets, n_entries=None, ws_floats=None, null_dw1=False):
        ne = len(self.entries)
        i32 = lambda vals: (ctypes.c_int32 * ne)(*[int(v) for v in vals])
        ws_floats = [w[1] for w in wss] if ws_floats is None else ws_floats
        dw1 = [None if null_dw1 else t[1] for t in targets]
        return self.lib.fst_wn_wgrad_reduce_many(
            i32(k for k, _ in self.entries), i32(k == 1 and self.last(i) for k, i in self.entries), i32([self.ns] * ne),
            ops._ptr_table([w[0] for w in wss]), (ctypes.c_int64 * ne)(*ws_floats), ops._ptr_table([t[0] for t in targets]),
            ops._ptr_table(dw1), ne if n_entries is None else n_entries, self.B, self.L, self.n, self.h, _lib.stream_ptr())

    def want(self, kind, i):
        """fp64 gradients of the entry, summed over the operand sets."""
        L, n = self.L, self.n
        if kind == 0:
            dil, w_in, w_cond = self.dils[i], 0, 0
            for s in range(self.ns):
                ap, dg = F.pad(self.a[i][s].double(), (dil, dil)), self.dg[i][s].double()
                w_in = w_in + torch.stack([torch.einsum("bmt,bct->mc", dg, ap[:, :, k * dil: k * dil + L]) for k in range(3)], dim=2)
                w_cond = w_cond + torch.einsum("bmt,bct->mc", dg, self.u0[s].double())
            return w_in, w_cond.unsqueeze(2)
        w = 0
        for s in range(self.ns):
            ts = self.ts[i][s].double()
            dy = self.d_out[s] if self.last(i) else torch.cat([self.d_a[i][s], self.d_out[s]], 1)
            w = w + torch.einsum("bmt,bct->mc", dy.double(), ts[:, :n] * ts[:, n:])
        return w.unsqueeze(2), None


def _layers(nl):
    return [(kind, i) for i in reversed(range(nl)) for kind in (1, 0)]         # the order the backward pass leaves them in


CASES = [  # n, h, B, L, dilations (one per layer), operand sets, entries
    pytest.param(16, 5, 2, 64, (1, 2, 4), 1, _layers(3), id="n16h5-3layers-1set"),
    pytest.param(8, 9, 3, 64, (1, 2, 4), 3, _layers(3), id="n8h9-leftover-k-row-3sets"),        # 3n + h = 33
    pytest.param(48, 5, 64, 256, (1, 2, 4), 1, _layers(3), id="n48h5-dead-k-blocks-B64-L256"),  # several stages per workgroup
    pytest.param(16, 5, 2, 64, (1, 2, 4, 8, 16, 4, 8, 2), 3, _layers(8), id="16-entries-3sets"),
    pytest.param(16, 5, 2, 64, (4,), 1, [(0, 0)], id="1-entry-in"),
    pytest.param(8, 9, 2, 64, (4,), 3, [(1, 0)], id="1-entry-rs-last"),                         # M = n
]


@pytest.mark.parametrize("n,h,B,L,dils,n_sets,entries", CASES)
def test_batched_reduction_equals_per_layer_entry_points(n, h, B, L, dils, n_sets, entries):
    S = _Stack(n, h, B, L, dils, n_sets, entries, seed=n * 31 + h + L + len(entries))
    for kind, i in entries:
        assert S.lib.fst_wn_wgrad_ok(kind, B, L, n, h, dils[i]) in (1, 2)
    ref, ref_bufs = S.targets()
    for (kind, i), dw in zip(entries, ref):
        ws, ws_n, _ = S.workspace(kind, i)
        assert S.product(kind, i, ws, ws_n, dw, reduce=True) == 0
    runs = []
    for _ in range(2):
        got, bufs = S.targets()
        wss = [S.workspace(kind, i) for kind, i in entries]                    # all live at once, as in the join's backward
        for (kind, i), w in zip(entries, wss):
            assert S.product(kind, i, w[0], w[1], None, reduce=False) == 0
        assert all(bool((t == CANARY).all()) for dw in got for t in dw if t is not None)   # the products write no gradient
        assert S.reduce_many(wss, got) == 0
        torch.cuda.synchronize()
        assert all(_bands_intact(b) for b in bufs), "a gradient's guard band was written"
        assert all(bool((w[2][w[1]:] == CANARY).all()) for w in wss), "written behind a workspace"
        runs.append(got)
    assert all(_bands_intact(b) for b in ref_bufs)
    for (kind, i), r, g0, g1 in zip(entries, ref, runs[0], runs[1]):
        for j in range(2):
            if r[j] is not None:
                assert torch.equal(g0[j], r[j]), f"entry {(kind, i)} output {j}: not the per-layer launch's bits"
                assert torch.equal(g1[j], g0[j]), f"entry {(kind, i)} output {j}: not repeatable"
        want = S.want(kind, i)
        assert_close(g0[0], want[0], 1e-4, f"entry {(kind, i)} dW")
        if kind == 0:
            assert_close(g0[1], want[1], 1e-4, f"entry {(kind, i)} cond dW")


def test_refused_reduction_writes_nothing():
    n, h, B, L = 8, 9, 2, 64
    entries = _layers(2)
    S = _Stack(n, h, B, L, (4, 8), 1, entries, seed=5)
    got, bufs = S.targets()
    wss = [S.workspace(kind, i) for kind, i in entries]
    for (kind, i), w in zip(entries, wss):
        assert S.product(kind, i, w[0], w[1], None, reduce=False) == 0
    short = [w[1] for w in wss]
    short[-1] = 256                                                            # (the query's size covers three sets: far below it)
    assert S.reduce_many(wss, got, n_entries=17) != 0                          # more entries than the table holds
    assert S.reduce_many(wss, got, n_entries=0) != 0
    assert S.reduce_many(wss, got, ws_floats=short) != 0                       # the LAST entry's workspace is too small
    assert S.reduce_many(wss, got, null_dw1=True) != 0                         # an in_layer entry without its cond target
    torch.cuda.synchronize()
    assert all(bool((b == CANARY).all()) for b in bufs)
    assert S.reduce_many(wss, got) == 0
    torch.cuda.synchronize()
    assert all(_bands_intact(b) for b in bufs) and not any(bool((t[0] == CANARY).any()) for t in got)
