"""Host logic of the anomaly guard on CPU tensors (no GPU): ``optim.count_nonfinite``, the guarded branches of
``rmsprop_step_many`` / ``SharedStepAdam.step`` and the trainer's group table.  The device kernels are tested in
test_gpu_anomaly_guard.py."""
import inspect

import torch

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import optim
from feature_level_style_transfer_for_tsc_amd.optim import AnomalyGuard, FusedRMSprop, SharedStepAdam, count_nonfinite, rmsprop_step_many

NAN, INF = float("nan"), float("inf")


def _tensors():
    g = torch.Generator().manual_seed(3)
    ts = [torch.randn(n, generator=g) for n in (1, 7, 300, 5)]
    ts[1][0], ts[1][6] = NAN, -INF
    ts[2][17], ts[2][299], ts[2][0] = INF, NAN, -0.0
    ts[3][2] = torch.finfo(torch.float32).max                            # 3.4028235e38: finite
    return ts


def test_count_nonfinite_matches_isfinite_per_group():
    ts, groups = _tensors(), [2, 0, 2, 1]
    want = torch.zeros(4, dtype=torch.int64)
    for t, g in zip(ts, groups):
        want[g] += (~torch.isfinite(t)).sum()
    before = [t.clone() for t in ts]
    got = count_nonfinite(ts, groups, 4)
    assert got.dtype == torch.int32 and got.tolist() == want.tolist() == [2, 0, 2, 0]
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ts, before))
    assert fst.count_nonfinite is count_nonfinite


def test_count_nonfinite_with_a_guard_writes_the_three_words():
    ts, groups = _tensors(), [2, 0, 2, 1]
    guard = AnomalyGuard("cpu")
    assert count_nonfinite([ts[0], ts[3]], [0, 1], 4, guard).tolist() == [0, 0, 0, 0]
    assert (int(guard.verdict), float(guard.ok), int(guard.skipped)) == (0, 1.0, 0)
    count_nonfinite(ts, groups, 4, guard)
    count_nonfinite(ts, groups, 4, guard)
    assert (int(guard.verdict), float(guard.ok), int(guard.skipped)) == (1, 0.0, 2)
    # a group outside the verdict mask is counted but does not decide
    assert count_nonfinite(ts, groups, 4, guard, verdict_groups=[1, 3]).tolist() == [2, 0, 2, 0]
    assert (int(guard.verdict), float(guard.ok), int(guard.skipped)) == (0, 1.0, 2)


def _guard(ok):
    g = AnomalyGuard("cpu")
    g.ok.fill_(ok); g.verdict.fill_(1 - ok)
    return g


def _params(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.rand(n, generator=g) * 2 - 1) for n in sizes]


def _set_grads(ps, step, poison=False):
    g = torch.Generator().manual_seed(100 + step)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g)
        if poison:
            p.grad[0] = NAN


def test_guarded_rmsprop_on_cpu():
    sizes = [1, 5, 40]
    for on_device in (False, True):
        a, b = _params(sizes, 1), _params(sizes, 1)
        oa = [FusedRMSprop(a[:2], lr=1e-2, lr_on_device=on_device), FusedRMSprop(a[2:], lr=3e-2, lr_on_device=on_device)]
        ob = [FusedRMSprop(b[:2], lr=1e-2, lr_on_device=on_device), FusedRMSprop(b[2:], lr=3e-2, lr_on_device=on_device)]
        for step in range(3):                                                 # ok = 1: the unguarded step, bit for bit
            _set_grads(a, step); _set_grads(b, step)
            rmsprop_step_many(oa, _guard(1))
            rmsprop_step_many(ob)
        state = lambda ps, os_: [p.detach().clone() for p in ps] + [o.state[p]["square_avg"].clone() for o in os_ for p in o.param_groups[0]["params"]]
        assert all(torch.equal(x, y) for x, y in zip(state(a, oa), state(b, ob)))
        before = state(a, oa)
        _set_grads(a, 9, poison=True)                                         # ok = 0: nothing moves although the gradients hold NaN
        rmsprop_step_many(oa, _guard(0))
        assert all(torch.equal(x, y) for x, y in zip(state(a, oa), before))
        assert all(bool(torch.isfinite(x).all()) for x in state(a, oa))


def test_guarded_shared_step_adam_on_cpu():
    sizes = [1, 5, 40]
    for on_device in (False, True):
        a, b = _params(sizes, 2), _params(sizes, 2)
        oa, ob = SharedStepAdam(a, lr=2e-3, lr_on_device=on_device), SharedStepAdam(b, lr=2e-3, lr_on_device=on_device)
        for step in range(3):
            _set_grads(a, step); _set_grads(b, step)
            oa.step(guard=_guard(1))
            ob.step()
        state = lambda ps, o: [p.detach().clone() for p in ps] + [o.state[p][n].clone() for p in ps for n in ("exp_avg", "exp_avg_sq")] \
            + [o.param_groups[0]["step"].clone()]
        assert all(torch.equal(x, y) for x, y in zip(state(a, oa), state(b, ob)))
        assert float(oa.param_groups[0]["step"]) == 3.0
        before = state(a, oa)
        _set_grads(a, 9, poison=True)
        oa.step(guard=_guard(0))
        assert all(torch.equal(x, y) for x, y in zip(state(a, oa), before))
        assert float(oa.param_groups[0]["step"]) == 3.0, "the shared counter advances by ok"


def test_anomaly_groups_cover_every_module():
    T = fst.JointTrainer
    assert T.ANOMALY_GROUPS[: len(T.MODULES)] == T.MODULES
    assert T.ANOMALY_GROUPS[len(T.MODULES):] == ("gradnorm", "losses", "buffers")
    assert len(set(T.ANOMALY_GROUPS)) == len(T.ANOMALY_GROUPS) <= optim.MAX_GROUPS
    assert set(T.LRS) | {"cpc"} == set(T.MODULES), "every module has an optimiser, so every gradient group is one the update reads"
    assert inspect.signature(T.__init__).parameters["anomaly_guard"].default is False


class _Bare(fst.JointTrainer):
    """The mode switch without the networks (JointTrainer's constructor needs a GPU stream)."""

    def __init__(self):
        self.device = torch.device("cpu")
        self._graphs, self._phase = None, {}
        self.anomaly_guard, self._guard = False, None
        self.w_t, self.w_s = torch.nn.Parameter(torch.tensor([2.0, 5.0])), torch.nn.Parameter(torch.tensor([2.0, 2.0, 4.0]))
        self.opt_w_t, self.opt_w_s = torch.optim.Adam([self.w_t], lr=2e-4), torch.optim.Adam([self.w_s], lr=1e-3)


def test_enabling_the_mode_twice_is_a_no_op_and_a_resident_capture_refuses():
    tr = _Bare()
    assert tr.skipped_steps is None
    tr.enable_anomaly_guard()
    guard, step = tr._guard, tr.opt_w_t.state[tr.w_t]["step"]
    assert tr.anomaly_guard and int(tr.skipped_steps) == 0
    tr.enable_anomaly_guard()
    assert tr._guard is guard and tr.opt_w_t.state[tr.w_t]["step"] is step
    assert sorted(tr.opt_w_s.state[tr.w_s]) == ["exp_avg", "exp_avg_sq", "step"]
    other = _Bare()
    other._phase = {"nf": object()}
    try:
        other.enable_anomaly_guard()
    except RuntimeError as e:
        assert "capture is resident" in str(e)
    else:
        raise AssertionError("enable_anomaly_guard() with a resident capture did not raise")
