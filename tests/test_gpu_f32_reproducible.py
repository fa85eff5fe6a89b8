"""A joint step under FST_MATH=f32 reproduces its own bits.

It did not while RandomLayer's [B, C·L] x [C·L, O] product and its data gradient ran on the conv engine's K-split GEMM, whose
slices are added with float atomics: the CDAN loss moved by 7.6e-6 between two replays at the bench shape and by 2.7e-6 between two
trainers at the toy geometry, and every gradient upstream of the CDAN branch with it.  With the products on ``gemm_f32`` (slabs
added in slab order) no launch of the step adds with float atomics, so everything below is ``torch.equal``: every reported tensor,
and every tensor the step mutates (parameters, BatchNorm buffers, optimiser moments, GradNorm weights).

Geometry: the joint fixture's (feature width 10, L = 32: C·L_t = 320 >= 256, so RandomLayer takes the big-GEMM branch, and
gemm_f32 splits K = 320 in two), dropout 0; once the default geometry at L = 128, B = 4 (C·L_t = 25600)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import ops
from test_gpu_full_step import _pair
from test_gpu_phase_graphs import clone, toy

DEV = "cuda"


@pytest.fixture(autouse=True)
def f32(monkeypatch):
    monkeypatch.setattr(ops, "MATH", "f32")


def assert_same(rep_a, rep_b, st_a, st_b, what, skip=()):
    for k, v in rep_b.items():
        if k in skip:
            continue
        diff = float((rep_a[k].double() - v.double()).abs().max())
        assert torch.equal(rep_a[k], v), f"{what}: report {k} differs by {diff:.3e}"
    assert set(st_b) <= set(st_a), f"{what}: state tensors missing: {sorted(set(st_b) - set(st_a))[:5]}"
    differing = [(k, float((st_a[k].double() - v.double()).abs().max())) for k, v in st_b.items() if not torch.equal(st_a[k], v)]
    assert not differing, f"{what}: {len(differing)} of {len(st_b)} state tensors differ, e.g. {differing[:5]}"


def twice_from_one_snapshot(tr, run, what):
    snap = tr.snapshot()
    rep1 = clone(run())
    state1 = tr.snapshot()["t"]
    tr.restore(snap)
    rep2 = run()
    assert_same(rep2, rep1, tr.snapshot()["t"], state1, what)
    return rep1


def test_random_layer_of_the_fixture_takes_the_big_gemm_branch():
    tr, args, _ = toy()
    R0 = tr.random_layer.random_matrix[0]
    assert R0.shape[0] >= 256 and R0.is_cuda and ops.gemm_f32_ok(tr.random_layer._rt(0))


def test_two_eager_steps_from_one_snapshot_are_bit_identical():
    tr, args, ts = toy()
    tr.step(*args, epoch=0, t_samples=ts)                                    # (creates the optimiser moments the snapshot then holds)
    timer = ops.KernelTimer()
    ops.KERNEL_TIMER = timer
    try:
        rep = twice_from_one_snapshot(tr, lambda: tr.step(*args, epoch=0, t_samples=ts), "two eager steps")
    finally:
        ops.KERNEL_TIMER = None
    keys = timer.summary()
    assert keys["gemm_f32_kernel f32"]["launches"] == 8, {k: v["launches"] for k, v in keys.items()}   # 2 steps x 2 sides x (fwd + dgrad)
    assert bool(torch.isfinite(rep["cdan"]).all())


def test_two_replays_from_one_snapshot_are_bit_identical():
    tr, args, ts = toy()
    torch.manual_seed(4)
    tr.capture(*args, epoch=0)
    twice_from_one_snapshot(tr, lambda: tr.replay(*args, ts), "two replays")


def test_a_clean_guarded_step_has_the_bits_of_the_unguarded_step():
    on, args, ts = toy()
    off, _, _ = toy()
    on.enable_anomaly_guard()
    ra, rb = on.step(*args, epoch=0, t_samples=ts), off.step(*args, epoch=0, t_samples=ts)
    assert int(ra["skipped"]) == 0 and not any(ra["anomaly"].tolist())
    assert_same(ra, rb, on.snapshot()["t"], off.snapshot()["t"], "guard on vs off")


def test_two_eager_steps_at_the_default_geometry():
    B, L = 4, 128
    torch.manual_seed(1234)
    tr = fst.JointTrainer(fst.JointConfig(L_t=L, L_s=L, dropout_p=0.0), DEV)
    gen = torch.Generator().manual_seed(7)
    (x_t, y_t), (x_s, y_s) = _pair(gen, B, 1, L, 4), _pair(gen, B, 1, L, 4)
    args = (x_t.to(DEV), y_t.to(DEV), x_s.to(DEV), y_s.to(DEV))
    tr.step(*args, epoch=0, t_samples=(16, 8))
    twice_from_one_snapshot(tr, lambda: tr.step(*args, epoch=0, t_samples=(16, 8)), "two eager steps, L = 128")
