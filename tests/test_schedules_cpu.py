"""Host logic of the device-resident learning rates (optim.push_lr, ``lr_on_device``) and of the reference's scheduler table
(step.make_schedulers / step.step_schedulers, train_and_test.py:118-134 and the scheduler calls after each kind of epoch), on
CPU tensors: no GPU, no library.  The expectations are literals written from the reference's lines, not from the tables of
step.py."""
import numpy as np
import pytest
import torch

from feature_level_style_transfer_for_tsc_amd import step as fst_step
from feature_level_style_transfer_for_tsc_amd.optim import FusedRMSprop, SharedStepAdam, push_lr, rmsprop_step_many

f32 = lambda v: float(np.float32(v))


def _params(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(k + 2, generator=g)) for k in range(n)]


def _set_grads(ps, seed):
    g = torch.Generator().manual_seed(seed)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g)


# ---------------------------------------------------------------------------------------------- lr_on_device optimisers
def test_push_lr_counts_changed_groups_and_is_quiet_the_second_time():
    a, b = _params(2, 1), _params(2, 2)
    rms = FusedRMSprop([{"params": a, "lr": 0.01}, {"params": b, "lr": 0.02}], lr_on_device=True)
    adam = SharedStepAdam(_params(3, 3), lr=0.002, lr_on_device=True)
    host = FusedRMSprop(_params(1, 4), lr=0.5)                              # no lr_dev: passed over
    assert rms.lr_dev.dtype == torch.float32 and rms.lr_dev.shape == (2,) and adam.lr_dev.shape == (1,)
    assert rms.lr_dev.tolist() == [f32(0.01), f32(0.02)] and adam.lr_dev.tolist() == [f32(0.002)]
    assert not hasattr(host, "lr_dev")
    assert push_lr([rms, adam, host]) == 0                                  # initialised from group["lr"]
    rms.param_groups[1]["lr"] = 0.5
    adam.param_groups[0]["lr"] = 0.001
    host.param_groups[0]["lr"] = 0.25
    assert push_lr([rms, adam, host]) == 2
    assert rms.lr_dev.tolist() == [f32(0.01), f32(0.5)] and adam.lr_dev.tolist() == [f32(0.001)]
    assert push_lr([rms, adam, host]) == 0
    rms.param_groups[0]["lr"] = 0.01 * (1 + 1e-12)                          # the same fp32 value: nothing to write
    assert push_lr([rms]) == 0


@pytest.mark.parametrize("kind", ["step", "plateau"])
def test_stock_schedulers_reach_lr_dev(kind):
    ps = _params(3, 5)
    opt = FusedRMSprop(ps, lr=0.01, lr_on_device=True)
    adam = SharedStepAdam(_params(2, 6), lr=0.002, lr_on_device=True)
    sch = torch.optim.lr_scheduler
    if kind == "step":
        scheds = [sch.StepLR(opt, 3, 0.8), sch.StepLR(adam, 2, 0.7)]
        step = lambda e: [s.step() for s in scheds]
    else:
        scheds = [sch.ReduceLROnPlateau(opt, "min", factor=0.7, patience=1), sch.ReduceLROnPlateau(adam, "min", factor=0.5, patience=0)]
        step = lambda e: [s.step(1.0 + e) for s in scheds]                  # a rising metric
    seen = set()
    for epoch in range(8):
        _set_grads(ps, epoch)
        opt.step()
        step(epoch)
        push_lr([opt, adam])
        for o in (opt, adam):
            assert o.lr_dev.tolist() == [f32(g["lr"]) for g in o.param_groups], (kind, epoch)
        seen.add(opt.param_groups[0]["lr"])
    assert len(seen) >= 3, seen                                             # the rate really moved, more than once


def test_lr_dev_stays_out_of_the_state_dict_and_survives_loading():
    for make in (lambda ps, **k: FusedRMSprop(ps, lr=0.01, **k), lambda ps, **k: SharedStepAdam(ps, lr=0.01, **k)):
        ps, qs = _params(2, 7), _params(2, 7)
        dev, host = make(ps, lr_on_device=True), make(qs)
        for o, p in ((dev, ps), (host, qs)):
            _set_grads(p, 1)
            o.step()
        sd, sd_host = dev.state_dict(), host.state_dict()
        assert sorted(sd) == sorted(sd_host)
        assert [sorted(g) for g in sd["param_groups"]] == [sorted(g) for g in sd_host["param_groups"]]
        assert [sorted(map(str, st)) for st in sd["state"].values()] == [sorted(map(str, st)) for st in sd_host["state"].values()]
        for p, q in zip(ps, qs):                                            # and the CPU formula reads lr_dev to the same effect
            assert torch.allclose(p, q, rtol=0, atol=1e-7)
        saved = dev.state_dict()
        saved["param_groups"][0]["lr"] = 0.004
        before = dev.lr_dev
        dev.load_state_dict(saved)
        assert dev.lr_dev is before and dev.lr_dev.tolist() == [f32(0.01)]  # same tensor, not yet told
        assert push_lr([dev]) == 1 and dev.lr_dev is before and dev.lr_dev.tolist() == [f32(0.004)]


def test_cpu_step_reads_lr_dev_and_eager_step_pushes_first():
    ps, qs = _params(3, 9), _params(3, 9)
    dev, host = FusedRMSprop(ps[:2], lr=0.01, lr_on_device=True), FusedRMSprop(qs[:2], lr=0.01)
    dev2, host2 = FusedRMSprop(ps[2:], lr=0.03), FusedRMSprop(qs[2:], lr=0.03)     # one call mixes both kinds
    for t in range(3):
        _set_grads(ps, t); _set_grads(qs, t)
        if t == 1:
            dev.param_groups[0]["lr"] = host.param_groups[0]["lr"] = 0.005   # no explicit push: the eager step does it
        rmsprop_step_many([dev, dev2])
        rmsprop_step_many([host, host2])
    assert dev.lr_dev.tolist() == [f32(0.005)]
    for p, q in zip(ps, qs):
        assert torch.allclose(p, q, rtol=0, atol=1e-6)
    assert not torch.equal(ps[0], _params(3, 9)[0])


# ---------------------------------------------------------------------------------------------- the scheduler table
NAMES = ("fe_t", "clf_t", "fe_s", "dimunif", "clf_s", "probtransfer", "nf", "noise", "ad_net", "fd_s", "cpc")
LR0 = {"fe_t": 0.001, "clf_t": 0.003, "fe_s": 0.001, "dimunif": 0.001, "clf_s": 0.003, "probtransfer": 0.001, "nf": 0.001,
       "noise": 0.005, "ad_net": 0.001, "fd_s": 0.001, "cpc": 0.002}        # train_and_test.py:97-106, :133
# train_and_test.py:118-134
STEP_SCHED = {"fe_t": (25, 0.8), "clf_t": (25, 0.8), "fe_s": (25, 0.8), "dimunif": (25, 0.8), "clf_s": (25, 0.8), "cpc": (25, 0.7),
              "noise": (55, 0.6)}
PLATEAU_SCHED = ("probtransfer", "nf", "ad_net", "fd_s")
# the scheduler calls after each kind of epoch: :172-174, :211-213, :275-280, :343-348, :436-442, :491-494, :767-777
STEPPED = {
    "target_pretrain": {"fe_t", "clf_t", "cpc"},
    "source_pretrain": {"fe_s", "dimunif", "clf_s"},
    "ssl_with_ce": {"fe_t", "clf_t", "cpc", "fe_s", "dimunif", "clf_s"},
    "ssl": {"fe_t", "cpc", "fe_s", "dimunif"},
    "nf_with_ce": {"fe_t", "clf_t", "fe_s", "dimunif", "clf_s", "cpc", "nf"},
    "nf": {"fe_t", "fe_s", "dimunif", "nf"},
    "joint": set(NAMES),
}
REPORT_KEYS = ("nf_t", "nf_s", "ce_t", "sl_t", "ce_s", "sl_s", "cdan", "ce_s2t2s", "fd_s", "total")


def _dummy():
    opts = {k: (SharedStepAdam if k == "cpc" else FusedRMSprop)(_params(1, i), lr=LR0[k], lr_on_device=True)
            for i, k in enumerate(NAMES)}
    return opts, fst_step.make_schedulers(opts)


def _report(epoch, falling=True):
    """Every loss falls (or rises) by the epoch, each from its own level: a plateau scheduler that reads the right key of a
    falling report never cuts its rate."""
    return {k: torch.tensor((100.0 + i) * (0.5 ** epoch if falling else 1.0 + epoch)) for i, k in enumerate(REPORT_KEYS)}


def test_make_schedulers_builds_the_references_eleven():
    opts, scheds = _dummy()
    assert sorted(scheds) == sorted(NAMES)
    sch = torch.optim.lr_scheduler
    for k, s in scheds.items():
        assert s.optimizer is opts[k]
        if k in STEP_SCHED:
            assert type(s) is sch.StepLR and (s.step_size, s.gamma) == STEP_SCHED[k], k
        else:
            assert k in PLATEAU_SCHED and type(s) is sch.ReduceLROnPlateau, k
            assert (s.mode, s.factor, s.patience, s.min_lrs) == ("min", 0.7, 10, [0.0001]), k


@pytest.mark.parametrize("kind", sorted(STEPPED))
def test_each_kind_of_epoch_steps_the_references_schedulers(kind):
    opts, scheds = _dummy()
    fst_step.step_schedulers(scheds, kind, _report(0))
    assert {k for k, s in scheds.items() if s.last_epoch == 1} == STEPPED[kind]
    assert {k for k, s in scheds.items() if s.last_epoch == 0} == set(NAMES) - STEPPED[kind]
    for epoch in range(1, 25):
        fst_step.step_schedulers(scheds, kind, _report(epoch))
    assert push_lr(opts.values()) == len([k for k in STEPPED[kind] if k in STEP_SCHED and k != "noise"]) + \
        (2 if kind == "joint" else 0)
    for k in NAMES:
        want = LR0[k]
        if k in STEPPED[kind] and STEP_SCHED.get(k, (0, 0))[0] == 25:
            want = LR0[k] * STEP_SCHED[k][1]                                 # 25 epochs: one StepLR(25) cut; StepLR(55) not yet
        if kind == "joint" and k in ("ad_net", "fd_s"):
            want = LR0[k] * 0.7 * 0.7                                       # the 0.0 quirk: cut after epochs 12 and 23
        assert opts[k].param_groups[0]["lr"] == pytest.approx(want, rel=1e-12), (kind, k)
        assert opts[k].lr_dev.tolist() == [f32(want)], (kind, k)


def test_unknown_kind_is_refused():
    _, scheds = _dummy()
    with pytest.raises(ValueError, match="unknown kind"):
        fst_step.step_schedulers(scheds, "pretrain", _report(0))


def test_joint_epoch_feeds_zero_to_ad_net_and_fd_s():
    """train_and_test.py:739-740 zero cdan_loss.data and feature_discriminator_s_loss.data before :776-777 hand them to the
    schedulers: the metric is 0.0 every epoch whatever the losses were.  ReduceLROnPlateau (patience 10): the first 0.0 is the
    best, the next eleven are bad epochs, so the twelfth call cuts the rate by 0.7 — and again every eleven epochs down to
    min_lr = 1e-4.  probtransfer and nf read ce_s2t2s and nf_t of the report: rising, they are cut on the same calendar; a
    scheduler fed 0.0 instead would behave the same, so the keys are told apart by ``best``."""
    opts, scheds = _dummy()
    for epoch in range(11):
        fst_step.step_schedulers(scheds, "joint", _report(epoch, falling=False))
    for k in ("ad_net", "fd_s"):
        assert opts[k].param_groups[0]["lr"] == 0.001 and scheds[k].best == 0.0 and scheds[k].num_bad_epochs == 10, k
    rep0 = _report(0, falling=False)
    assert scheds["probtransfer"].best == pytest.approx(float(rep0["ce_s2t2s"])) and scheds["nf"].best == pytest.approx(float(rep0["nf_t"]))
    fst_step.step_schedulers(scheds, "joint", _report(11, falling=False))
    for k in PLATEAU_SCHED:
        assert opts[k].param_groups[0]["lr"] == pytest.approx(0.0007, rel=1e-12), k
    for epoch in range(12, 120):
        fst_step.step_schedulers(scheds, "joint", _report(epoch, falling=False))
        assert all(opts[k].param_groups[0]["lr"] >= 0.0001 for k in PLATEAU_SCHED)
    for k in PLATEAU_SCHED:                                                  # 0.001 · 0.7⁷ < 1e-4: the floor
        assert opts[k].param_groups[0]["lr"] == 0.0001, k
    # a falling report leaves probtransfer and nf alone while ad_net / fd_s are still cut: they do not look at the report
    opts, scheds = _dummy()
    for epoch in range(12):
        fst_step.step_schedulers(scheds, "joint", _report(epoch))
    assert [opts[k].param_groups[0]["lr"] for k in PLATEAU_SCHED] == pytest.approx([0.001, 0.001, 0.0007, 0.0007], rel=1e-12)


def test_nf_phases_feed_the_phase_total_to_nf():
    for kind in ("nf", "nf_with_ce"):
        _, scheds = _dummy()
        rep = _report(0)
        fst_step.step_schedulers(scheds, kind, rep)
        assert scheds["nf"].best == pytest.approx(float(rep["total"])), kind


class _StubBucket:
    """Stands for dist.GradBucket over two ranks: the other rank's metrics are 3.0 higher."""
    def __init__(self):
        self.seen = []

    def mean_scalars(self, t):
        self.seen.append(t.clone())
        return (t + (t + 3.0)) / 2


def test_plateau_metrics_are_rank_means():
    _, scheds = _dummy()
    bucket, rep = _StubBucket(), _report(0)
    fst_step.step_schedulers(scheds, "joint", rep, bucket)
    assert len(bucket.seen) == 1 and bucket.seen[0].tolist() == [float(rep["ce_s2t2s"]), float(rep["nf_t"])]
    assert scheds["probtransfer"].best == pytest.approx(float(rep["ce_s2t2s"]) + 1.5)
    assert scheds["nf"].best == pytest.approx(float(rep["nf_t"]) + 1.5)
    assert scheds["ad_net"].best == 0.0 and scheds["fd_s"].best == 0.0       # constants: nothing to average
    _, scheds = _dummy()
    bucket = _StubBucket()
    fst_step.step_schedulers(scheds, "ssl", _report(0), bucket)             # no plateau scheduler: no collective
    assert bucket.seen == []
