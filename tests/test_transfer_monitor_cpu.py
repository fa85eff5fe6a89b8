"""Host side of the transfer monitor (no GPU): the new symbols in header, ctypes table and library and their refusals; the fp64
definition ``monitor.mmd2_reference`` against a known answer and its invariances; the trainer's switch.  The kernels and the
trainer's steps are tested in test_gpu_transfer_monitor.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import _lib, monitor, ops
from feature_level_style_transfer_for_tsc_amd.monitor import FIELDS, PAIRS, TransferMonitor, mmd2_from_gram, mmd2_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fst_mmd_gram", "fst_mmd_fold", "fst_mmd_centre", "fst_mmd_gram_splits", "fst_mmd_gram_workspace_floats")


def test_header_binding_and_library_agree_on_the_new_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fst_hip.h")).read(), flags=re.S)
    for name in NEW:
        decl = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, f"{name} is not declared in include/fst_hip.h"
        res, args = _lib._SIGNATURES[name]
        assert len(args) == decl.group(2).count(",") + 1, f"{name}: the ctypes table and the header disagree on the argument count"
        assert (res is _lib.c_int64) == (decl.group(1) == "int64_t"), name
    version = int(re.search(r"#define\s+FST_ABI_VERSION\s+(\d+)", text).group(1))
    assert version == _lib.ABI_VERSION >= 28
    lib = _lib.load()
    assert lib.fst_version() == version
    for name in NEW:
        assert hasattr(lib, name), name
    for name, value in (("SETS", ops.MMD_MAX_SETS), ("ROWS", ops.MMD_MAX_ROWS), ("PAIRS", ops.MMD_MAX_PAIRS), ("KERNELS", ops.MMD_MAX_KERNELS)):
        assert int(re.search(r"#define\s+FST_MMD_MAX_" + name + r"\s+(\d+)", text).group(1)) == value


def test_slabs_depend_on_the_columns_alone_and_the_workspace_holds_whole_upper_tiles():
    lib = _lib.load()
    assert [lib.fst_mmd_gram_splits(4, D) for D in (1, 8192, 8193, 115200)] == [1, 1, 2, 15]
    assert {lib.fst_mmd_gram_splits(R, 20000) for R in (2, 129, 768, 1024)} == {3}
    tile = 128 * 128
    assert [lib.fst_mmd_gram_workspace_floats(R, 64) for R in (2, 128, 129, 768, 1024)] == [tile, tile, 3 * tile, 21 * tile, 36 * tile]
    assert lib.fst_mmd_gram_workspace_floats(768, 115200) == 15 * 21 * tile
    for R, D in ((0, 4), (1025, 4), (4, 0), (4, -1)):
        assert lib.fst_mmd_gram_splits(R, D) == -1 and lib.fst_mmd_gram_workspace_floats(R, D) == -1


def _words(n=4096):
    """Aligned host words that a refused call never dereferences."""
    buf = np.zeros(n + 8, dtype=np.float64)
    return buf, (buf.ctypes.data + 63) & ~63                                   # (the first word on a 64-byte boundary)


def test_launchers_refuse_bad_arguments_on_the_host():
    """Refused before any launch (there is no device here: a launch would return another code)."""
    lib = _lib.load()
    keep, w = _words()

    def gram(x=w, rows=(4, 4), ld=(8, 8), D=8, centre=None, G=w + 4096, ws=w + 8192, ws_n=128 * 128):
        n = len(rows)
        xs = (ctypes.c_void_p * n)(*([x] * n if not isinstance(x, tuple) else x))
        return lib.fst_mmd_gram(xs, (ctypes.c_int32 * n)(*rows), (ctypes.c_int64 * n)(*ld), n, D, centre, G, ws, ws_n, None)

    for what, kw in (("no rows", dict(rows=(0, 4))), ("too many rows", dict(rows=(1000, 25), ld=(8, 8))), ("five sets", dict(rows=(2,) * 5, ld=(8,) * 5)),
                     ("stride below D", dict(ld=(8, 7))), ("D = 0", dict(D=0)), ("null set", dict(x=(w, None))), ("set 4 bytes off", dict(x=(w, w + 4))),
                     ("null G", dict(G=None)), ("short workspace", dict(ws_n=128 * 128 - 1)), ("workspace off", dict(ws=w + 8196)),
                     ("G is a set", dict(G=w)), ("centre 2 bytes off", dict(centre=w + 16386))):
        assert gram(**kw) == -1, what
        assert b"fst_mmd_gram" in lib.fst_last_error(), what

    assert lib.fst_mmd_centre(None, 8, 4, 8, w, None) == -1 and b"fst_mmd_centre" in lib.fst_last_error()
    assert lib.fst_mmd_centre(w, 7, 4, 8, w + 4096, None) == -1
    assert lib.fst_mmd_centre(w, 8, 4, 8, w + 64, None) == -1 and b"overlaps" in lib.fst_last_error()

    def fold(rows=(4, 4, 4), pairs=((0, 1), (0, 2)), kernels=5, mul=2.0, G=w, out=w + 4096, sums=w + 8192, count=w + 12288, nonfinite=w + 12544,
             bw=None, live=None):
        n, P = len(rows), len(pairs)
        return lib.fst_mmd_fold(G, (ctypes.c_int32 * n)(*rows), n, (ctypes.c_int32 * (2 * P))(*[v for p in pairs for v in p]), P, kernels, mul,
                                bw, live, out, sums, count, nonfinite, None)

    for what, kw in (("a pair with itself", dict(pairs=((1, 1),))), ("set 3 of 3", dict(pairs=((0, 3),))), ("nine pairs", dict(pairs=((0, 1),) * 9)),
                     ("no pair", dict(pairs=())), ("a set of one row", dict(rows=(4, 1, 4))), ("no kernel", dict(kernels=0)),
                     ("17 kernels", dict(kernels=17)), ("mul 0", dict(mul=0.0)), ("mul nan", dict(mul=float("nan"))), ("null out", dict(out=None)),
                     ("out 4 bytes off", dict(out=w + 4100)), ("sums on out", dict(sums=w + 4096)), ("bandwidth word 4 bytes off", dict(bw=w + 20004))):
        assert fold(**kw) == -1, what
        assert b"fst_mmd_fold" in lib.fst_last_error(), what
    assert keep.sum() == 0.0


def test_wrappers_refuse_what_the_kernels_do_not_serve():
    x = torch.zeros(4, 8)
    for call in (lambda: ops.mmd_centre(x), lambda: ops.mmd_gram([x, x]), lambda: monitor.mmd2(x, x)):
        with pytest.raises(_lib.FstLibraryError, match="lives on cpu"):
            call()
    with pytest.raises(ValueError, match="5 sets"):
        ops.mmd_gram([x] * 5)
    with pytest.raises(_lib.FstLibraryError, match="lives on cpu"):
        ops.mmd_fold(torch.zeros(8, 8), [4, 4], [(0, 1)], 5, 2.0, *[torch.zeros(1)] * 4)
    for bad in (dict(kernels=0), dict(kernels=2.0), dict(kernels=True), dict(mul=0.0), dict(mul="2"), dict(bandwidth=0.0), dict(bandwidth=float("inf")),
                dict(bandwidth=float("nan"))):
        with pytest.raises(ValueError, match="transfer monitor"):
            monitor.mmd2(x, x, **bad)
        with pytest.raises(ValueError, match="transfer monitor"):
            mmd2_reference(x, x, **bad)


# ---------------------------------------------------------------------------------------------- the definition
def test_known_answer():
    """x = {0, 1}, y = {2, 4} on the line: d² within x 1, within y 4, between (4 + 16 + 1 + 9) / 4; bw = 2 (1 + 4 + 30) / 12."""
    got = mmd2_reference(torch.tensor([[0.0], [1.0]]), torch.tensor([[2.0], [4.0]]))
    assert got.dtype == torch.float64 and got.shape == (len(FIELDS),)
    want = [2.0380001677155475, 35.0 / 6.0, 1.0, 4.0, 7.5]
    for name, a, b in zip(FIELDS, got.tolist(), want):
        assert abs(a - b) <= 1e-12, (name, a, b)


def _draw(seed, n, m, D, shift=0.0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, D, generator=gen, dtype=torch.float64), torch.randn(m, D, generator=gen, dtype=torch.float64) + shift


def test_symmetric_in_its_two_sets():
    x, y = _draw(1, 7, 12, 20, 0.3)
    a, b = mmd2_reference(x, y), mmd2_reference(y, x)
    assert abs(float(a[0]) - float(b[0])) <= 1e-12 and abs(float(a[1]) - float(b[1])) <= 1e-12 * float(a[1])
    assert abs(float(a[2]) - float(b[3])) <= 1e-12 * float(a[2]), "the two within-set means change places"


def test_a_constant_added_to_every_column_changes_nothing():
    x, y = _draw(2, 16, 9, 33, 0.5)
    c = torch.linspace(-40.0, 90.0, 33, dtype=torch.float64)
    a, b = mmd2_reference(x, y), mmd2_reference(x + c, y + c)
    assert abs(float(a[0]) - float(b[0])) <= 1e-9, (float(a[0]), float(b[0]))


def test_all_equal_rows_give_zero_not_nan():
    got = mmd2_reference(torch.full((3, 5), 2.5), torch.full((4, 5), 2.5))
    assert got.tolist() == [0.0] * 5


def test_inputs_of_any_rank_are_flattened_per_row_and_a_given_bandwidth_is_used():
    x, y = _draw(3, 5, 6, 24)
    assert torch.equal(mmd2_reference(x.view(5, 2, 12), y.view(6, 4, 6)), mmd2_reference(x, y))
    got = mmd2_reference(x, y, kernels=3, mul=3.0, bandwidth=7.0)
    assert float(got[1]) == 7.0 and float(got[0]) != float(mmd2_reference(x, y, kernels=3, mul=3.0)[0])
    Zc = torch.cat([x, y]) - x.mean(dim=0)
    assert torch.equal(mmd2_from_gram(Zc @ Zc.t(), 5, 6), mmd2_reference(x, y))
    with pytest.raises(ValueError):
        mmd2_reference(x[:1], y)
    with pytest.raises(ValueError):
        mmd2_reference(x, y[:, :5])


def test_a_nan_row_gives_a_nan_not_a_number():
    x, y = _draw(4, 5, 6, 8)
    y[2, 3] = float("nan")
    assert torch.isnan(mmd2_reference(x, y)[0])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_two_sample_sanity(seed):
    """n = m = 64, D = 96, standard normal: the same distribution gives about 0, a shift of 0.5 per column does not.  (In fp64 over
    20 draws: same-distribution values in [-0.0094, 0.0089], shifted ones in [0.244, 0.323].)"""
    gen = torch.Generator().manual_seed(seed)
    x, y = torch.randn(64, 96, generator=gen), torch.randn(64, 96, generator=gen)
    same, shifted = float(mmd2_reference(x, y)[0]), float(mmd2_reference(x, y + 0.5)[0])
    print(f"seed {seed}: same {same:.5f}, shifted {shifted:.5f}")
    assert abs(same) < 0.05
    assert shifted > 0.15


# ---------------------------------------------------------------------------------------------- the trainer's switch
class _Bare(fst.JointTrainer):
    """The mode switch without the networks (JointTrainer's constructor needs a GPU stream)."""

    def __init__(self):
        self.device = torch.device("cpu")
        self._graphs, self._phase = None, {}


def test_enable_and_set_transfer_monitor_arguments():
    T = fst.JointTrainer
    assert inspect.signature(T.__init__).parameters["transfer_monitor"].default is None
    assert PAIRS == ("t|s2t", "t|s", "s|t2s", "s|s2t2s")
    tr = _Bare()
    assert tr.transfer_monitor is None
    for call in (lambda: tr.set_transfer_bandwidth(1.0), tr.transfer_mean, tr.reset_transfer_monitor):
        with pytest.raises(RuntimeError, match="enable_transfer_monitor"):
            call()
    for bad in (dict(kernels=0), dict(kernels=17), dict(kernels=2.5), dict(mul=-2.0), dict(mul=float("nan")), dict(bandwidth=-1.0), dict(bandwidth="1")):
        with pytest.raises(ValueError, match="transfer monitor"):
            tr.enable_transfer_monitor(**bad)
    assert tr.transfer_monitor is None, "a refused call must not switch the mode on"
    tr.enable_transfer_monitor()
    mon = tr.transfer_monitor
    assert (mon.kernels, mon.mul, mon.bandwidth) == (5, 2.0, None) and float(mon.word) == 0.0
    assert mon.sums.shape == (4, 5) and mon.sums.dtype == torch.float64 and mon.counts.tolist() == [0] * 4 and mon.nonfinite.tolist() == [0]
    tr.enable_transfer_monitor()
    assert tr.transfer_monitor is mon, "a second call keeps the device words"
    assert tr.set_transfer_bandwidth(3.5) is True and tr.set_transfer_bandwidth(3.5) is False and float(mon.word) == 3.5
    with pytest.raises(ValueError, match="transfer monitor"):
        tr.set_transfer_bandwidth(0.0)
    assert mon.bandwidth == 3.5 and float(mon.word) == 3.5, "a refused call must leave the word alone"
    assert tr.set_transfer_bandwidth(None) is True and float(mon.word) == 0.0
    assert bool(torch.isnan(tr.transfer_mean()).all()), "no measurement yet"
    for resident in (dict(_phase={"nf": object()}), dict(_graphs=[object()])):  # a phase capture, the joint capture
        other = _Bare()
        other.__dict__.update(resident)
        with pytest.raises(RuntimeError, match="capture is resident"):
            other.enable_transfer_monitor()
        assert other.transfer_monitor is None
    tr._graphs = [object()]                                                   # under a resident capture:
    assert tr.set_transfer_bandwidth(2.0) is True and float(mon.word) == 2.0   # ... the word may move
    tr.enable_transfer_monitor(bandwidth=4.0)                                 # ... through the switch too
    assert float(mon.word) == 4.0
    with pytest.raises(RuntimeError, match="capture is resident"):
        tr.enable_transfer_monitor(kernels=3)                                 # ... what the launches hold by value may not
    assert mon.kernels == 5


def test_state_dict_round_trip_of_the_settings_and_sums():
    mon = TransferMonitor("cpu", kernels=3, mul=1.5, bandwidth=0.25)
    mon.sums += torch.arange(20, dtype=torch.float64).view(4, 5)
    mon.counts += torch.tensor([2, 2, 1, 0], dtype=torch.int32)
    mon.nonfinite += 1
    sd = mon.state_dict()
    mon.sums += 1.0                                                           # the entry is a copy
    tr = _Bare()
    tr._transfer_load_state_dict(sd)
    got = tr.transfer_monitor
    assert (got.kernels, got.mul, got.bandwidth) == (3, 1.5, 0.25) and float(got.word) == 0.25
    assert torch.equal(got.sums, torch.arange(20, dtype=torch.float64).view(4, 5)) and got.counts.tolist() == [2, 2, 1, 0]
    assert got.nonfinite.tolist() == [1]
    mean = tr.transfer_mean()
    assert torch.equal(mean[0], torch.arange(5, dtype=torch.float64) / 2) and bool(torch.isnan(mean[3]).all())
    tr.reset_transfer_monitor()
    assert float(got.sums.abs().sum()) == 0.0 and got.counts.tolist() == [0] * 4 and got.nonfinite.tolist() == [0]
    words = (got.sums, got.counts, got.word)
    tr._transfer_load_state_dict(sd)                                          # into a monitor that is on: in place
    assert tr.transfer_monitor is got and all(a is b for a, b in zip(words, (got.sums, got.counts, got.word)))
    assert got.counts.tolist() == [2, 2, 1, 0]
