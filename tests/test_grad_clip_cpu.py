"""Host side of the device gradient clipping (no GPU): the new symbols in header, ctypes table and library; the wrappers'
refusals; ``optim.clip_coefficients`` — the documented definition of what ``fst_sumsq_multi``'s finaliser computes — against
``torch.nn.utils.clip_grad_norm_`` on fp64 CPU tensors; and the trainer's argument checks.  The kernels and the trainer's steps are
tested in test_gpu_grad_clip.py."""
import inspect
import os
import re

import pytest
import torch

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import _lib, optim
from feature_level_style_transfer_for_tsc_amd.optim import GradClip, clip_coefficients, scale_by_group, sumsq_norms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
NEW = ("fst_sumsq_slots", "fst_sumsq_multi", "fst_scale_multi")


def test_header_binding_and_library_agree_on_the_new_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fst_hip.h")).read(), flags=re.S)
    for name in NEW:
        decl = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, f"{name} is not declared in include/fst_hip.h"
        res, args = _lib._SIGNATURES[name]
        assert len(args) == decl.group(2).count(",") + 1, f"{name}: the ctypes table and the header disagree on the argument count"
        assert (res is _lib.c_int64) == (decl.group(1) == "int64_t"), name
    version = int(re.search(r"#define\s+FST_ABI_VERSION\s+(\d+)", text).group(1))
    assert version == _lib.ABI_VERSION >= 22
    lib = _lib.load()
    assert lib.fst_version() == version
    for name in NEW:
        assert hasattr(lib, name), name
    # the slot array of n tensors: n records of a group word and 64 partial sums; a negative count is refused
    assert [lib.fst_sumsq_slots(n) for n in (0, 1, 64, 130)] == [0, 65, 64 * 65, 130 * 65] and lib.fst_sumsq_slots(-1) < 0
    # refused on the host before any launch (there is no device here: a launch would return another code)
    assert lib.fst_sumsq_multi(None, None, None, 0, None, 0, None, None, None, None) == -1 and lib.fst_last_error()
    assert lib.fst_scale_multi(None, None, None, 0, None, None) == -1 and lib.fst_last_error()


def _host_call(x_ptr, numel, group, slots_len=65, scale=True):
    """The launchers on one made-up tensor entry that they must REFUSE (nothing here may reach a launch: these are no device
    pointers); the other pointers are aligned host words that are never dereferenced."""
    import ctypes
    import numpy as np
    lib = _lib.load()
    words = np.zeros(256, dtype=np.float32)
    w = words.ctypes.data
    xs, ne, gr = (ctypes.c_void_p * 1)(x_ptr), (ctypes.c_int64 * 1)(numel), (ctypes.c_int32 * 1)(group)
    return (lib.fst_sumsq_multi(xs, ne, gr, 1, w, slots_len, w + 400, w + 540, w + 680, None),
            lib.fst_scale_multi(xs, ne, gr, 1, w, None) if scale else None)


@pytest.mark.parametrize("what, entry", [("null pointer", (None, 8, 0)), ("pointer 2 bytes off", (4098, 8, 0)), ("no elements", (4096, 0, 0)),
                                         ("negative count", (4096, -3, 0)), ("2^31 elements", (4096, 2 ** 31, 0)),
                                         ("group 32", (4096, 8, 32)), ("group -1", (4096, 8, -1))])
def test_launchers_refuse_bad_entries_on_the_host(what, entry):
    assert _host_call(*entry) == (-1, -1), what
    assert _lib.load().fst_last_error()


def test_scan_refuses_a_short_slot_array():
    assert _host_call(4096, 8, 0, slots_len=64, scale=False)[0] == -1         # (the scale takes no slots: this entry is valid for it)
    assert b"slots" in _lib.load().fst_last_error()


def test_wrappers_refuse_cpu_tensors():
    clip = GradClip("cpu")
    x = [torch.randn(5)]
    with pytest.raises(_lib.FstLibraryError, match="lives on cpu"):
        sumsq_norms(x, [0], clip.limits, clip.norms, clip.coef)
    with pytest.raises(_lib.FstLibraryError, match="lives on cpu"):
        scale_by_group(x, [0], clip.coef)
    with pytest.raises(ValueError, match="group 32"):
        scale_by_group(x, [32], clip.coef)
    with pytest.raises(ValueError, match="1 tensors, 2 group ids"):
        sumsq_norms(x, [0, 1], clip.limits, clip.norms, clip.coef)


def test_grad_clip_holder_keeps_a_host_copy_of_its_limits():
    clip = GradClip("cpu")
    assert clip.limits.shape == (33,) and clip.norms.shape == (33,) and clip.coef.shape == (32,)
    assert clip.limits_host == [INF] * 33 and bool(torch.isinf(clip.limits).all()) and bool((clip.coef == 1).all())
    new = [INF] * 33
    new[6], new[32] = 0.1, 2.5
    assert clip.set_limits(new) is True and clip.set_limits(new) is False
    assert clip.limits.tolist() == clip.limits_host == [float(torch.tensor(v, dtype=torch.float32)) for v in new]
    for bad in ([1.0] * 32, [-1.0] + [INF] * 32, [NAN] + [INF] * 32):
        with pytest.raises(ValueError):
            clip.set_limits(bad)
    assert clip.limits.tolist() == clip.limits_host


# ---------------------------------------------------------------------------------------------- the arithmetic against torch
def _modules(seed, scales):
    """One list of fp64 'gradient' tensors per module."""
    gen = torch.Generator().manual_seed(seed)
    return [[torch.randn(n, generator=gen, dtype=torch.float64) * s for n in (7, 130, 1)] for s in scales]


def _norms(mods):
    return [float(torch.linalg.vector_norm(torch.cat(ts))) for ts in mods] + [0.0] * (32 - len(mods))


def _torch_clipped(mods, caps, max_norm):
    """clip_grad_norm_ per module with its cap, then over everything with max_norm: the factor each module ended up with."""
    ps = [[torch.nn.Parameter(torch.zeros_like(t)) for t in ts] for ts in mods]
    for m, ts in zip(ps, mods):
        for p, t in zip(m, ts):
            p.grad = t.clone()
    for m, cap in zip(ps, caps):
        if cap is not None:
            torch.nn.utils.clip_grad_norm_(m, cap)
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_([p for m in ps for p in m], max_norm)
    return [float((m[1].grad / ts[1])[0]) for m, ts in zip(ps, mods)]


@pytest.mark.parametrize("max_norm", [0.5, 30.0, 1e9])
def test_global_cap_matches_clip_grad_norm(max_norm):
    mods = _modules(1, (1e-3, 1.0, 10.0, 0.3))
    limits = [INF] * 32 + [max_norm]
    got = clip_coefficients(_norms(mods), limits)
    want = _torch_clipped(mods, [None] * 4, max_norm)
    assert got.dtype == torch.float64 and got.shape == (32,)
    assert len(set(got.tolist())) == 1, "one factor for everything"
    torch.testing.assert_close(got[:4], torch.tensor(want, dtype=torch.float64), rtol=1e-12, atol=0)
    assert (max_norm == 1e9) == bool((got == 1.0).all())


def test_per_module_caps_match_clip_grad_norm_called_per_module():
    mods = _modules(2, (1e-3, 1.0, 10.0, 0.3))
    caps = [1.0, 0.25, None, 2.0]                                              # module 0 is below its cap, module 2 has none
    limits = [INF if c is None else c for c in caps] + [INF] * 28 + [INF]
    got = clip_coefficients(_norms(mods), limits)
    want = _torch_clipped(mods, caps, None)
    torch.testing.assert_close(got[:4], torch.tensor(want, dtype=torch.float64), rtol=1e-12, atol=0)
    assert got[0] == 1.0 and got[2] == 1.0 and got[3] < 1.0 and got[1] < 1.0 and bool((got[4:] == 1.0).all())
    # and both kinds together: the global cap works on what the module caps left
    limits[32] = 1.0
    got = clip_coefficients(_norms(mods), limits)
    want = _torch_clipped(mods, caps, 1.0)
    torch.testing.assert_close(got[:4], torch.tensor(want, dtype=torch.float64), rtol=1e-12, atol=0)
    assert bool((got < 1.0).all())


@pytest.mark.parametrize("bad", [INF, NAN])
def test_a_non_finite_norm_gives_all_ones(bad):
    norms = _norms(_modules(3, (1.0, 5.0)))
    norms[1] = bad
    limits = [0.1] * 33
    assert clip_coefficients(norms, limits).tolist() == [1.0] * 32
    ok = _norms(_modules(3, (1.0, 5.0)))
    assert bool((clip_coefficients(ok, limits)[:2] < 1.0).all())
    assert clip_coefficients(ok + [bad], limits).tolist() == [1.0] * 32, "the reported total takes part in the test"
    with pytest.raises(ValueError):
        clip_coefficients(ok[:5], limits)


# ---------------------------------------------------------------------------------------------- the trainer's switch
class _Bare(fst.JointTrainer):
    """The mode switch without the networks (JointTrainer's constructor needs a GPU stream)."""

    def __init__(self):
        self.device = torch.device("cpu")
        self._graphs, self._phase = None, {}
        self.grad_clip, self._clip, self._clip_max, self._clip_per, self._clip_masks = False, None, None, {}, {}


def test_enable_and_set_grad_clip_arguments():
    T = fst.JointTrainer
    assert inspect.signature(T.__init__).parameters["grad_clip"].default is None
    assert len(T.MODULES) <= optim.MAX_GROUPS
    tr = _Bare()
    with pytest.raises(RuntimeError, match="enable_grad_clip"):
        tr.set_grad_clip(max_norm=1.0)
    with pytest.raises(ValueError, match="unknown module 'flow'"):
        tr.enable_grad_clip(per_module={"flow": 1.0})
    with pytest.raises(ValueError, match="non-negative"):
        tr.enable_grad_clip(max_norm=-1.0)
    assert not tr.grad_clip and tr._clip is None, "a refused call must not switch the mode on"
    tr.enable_grad_clip()                                                     # report only
    clip = tr._clip
    assert tr.grad_clip and clip.limits_host == [INF] * 33
    tr.enable_grad_clip()                                                     # idempotent
    assert tr._clip is clip
    assert tr.set_grad_clip(max_norm=2.0, per_module={"nf": 0.5}) is True
    want = [INF] * 33
    want[T.MODULES.index("nf")], want[32] = 0.5, 2.0
    assert clip.limits_host == want and clip.limits.tolist() == want
    assert tr.set_grad_clip(max_norm=2.0) is False and clip.limits_host == want, "an argument left out keeps its value"
    for bad in (dict(per_module={"nf": -0.5}), dict(max_norm=NAN), dict(per_module={"wn": 1.0}), dict(max_norm="1")):
        with pytest.raises(ValueError):
            tr.set_grad_clip(**bad)
    assert clip.limits_host == want, "a refused call must leave the limits alone"
    tr.set_grad_clip(max_norm=None)
    want[32] = INF
    assert clip.limits_host == want
    tr.set_grad_clip(per_module=None)
    assert clip.limits_host == [INF] * 33
    for resident in (dict(_phase={"nf": object()}), dict(_graphs=[object()])):  # a phase capture, the joint capture
        other = _Bare()
        other.__dict__.update(resident)
        with pytest.raises(RuntimeError, match="capture is resident"):
            other.enable_grad_clip()
        assert not other.grad_clip
    tr._phase = {"nf": object()}                                              # legal under a resident capture
    assert tr.set_grad_clip(max_norm=1.0) is True and clip.limits_host[32] == 1.0
