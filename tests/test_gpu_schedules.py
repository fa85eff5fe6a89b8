"""Learning rates and epoch coefficients on the device (csrc/optim.hip: fst_rmsprop_multi_dev / fst_adam_multi_dev behind
``lr_on_device``; ``optim.push_lr``; ``enable_device_hparams()`` of the two trainers): a captured step follows a schedule.
Needs an MI355X.

Gates.  The device-lr kernels call the update bodies of the host-lr kernels, so equal fp32 rates give EQUAL bits: ``torch.equal``
wherever a device-lr run is compared with a host-lr run of the same launches.  Against float64 torch under the same stock
schedulers: ``_assert_steps_close`` of test_gpu_optim.py at the initial (largest) rate.  Trainer replays against the eager step:
the gates the existing replay tests use (1e-6 on losses, bit-equality of a no-CPC phase, the real-gradient gate on state)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd.optim import FusedRMSprop, SharedStepAdam, push_lr, rmsprop_step_many
from oracle import restatement as R
from test_gpu_conv_routes import CANARY
from test_gpu_modules import _joint_trainer, close, load
from test_gpu_optim import _assert_steps_close, _grads, _sizes, _start, f32
from test_gpu_phase_graphs import JOINT_LOSSES, clone, real_gradient_gate, same_losses, same_state

DEV = "cuda"
BAND = 8                                                                    # floats of canary around every tensor


def banded(sizes, copies):
    """(buffer, views): ``copies`` tensors per entry of ``sizes`` laid one after the other in ONE flat buffer, ``BAND`` canary
    floats in front of each and behind the last, in the manner of ``guarded`` of test_gpu_conv_routes.py.  views[c][i]."""
    total = BAND + sum((n + BAND) * copies for n in sizes)
    buf = torch.full((total,), CANARY, device=DEV, dtype=torch.float32)
    views, at = [[] for _ in range(copies)], BAND
    for n in sizes:
        for c in range(copies):
            views[c].append(buf[at: at + n])
            at += n + BAND
    assert at == total
    return buf, views


def assert_bands_untouched(buf, views, what):
    probe = buf.clone()
    for vs in views:
        for v in vs:
            probe[v.storage_offset(): v.storage_offset() + v.numel()] = CANARY
    bad = int((probe != CANARY).sum())
    assert bad == 0, f"{what}: {bad} elements outside the tensors were written"


def _three_way(sizes):
    return [list(range(i, len(sizes), 3)) for i in range(3)] if len(sizes) >= 3 else [[0], [], []]


# ---------------------------------------------------------------------------------------------- 1. bitwise twin
@pytest.mark.parametrize("layout", ["one", "65"])
def test_rmsprop_device_lr_is_the_bitwise_twin_of_host_lr(layout):
    sizes = _sizes(layout)
    p0 = _start(sizes, 11)
    lrs = [f32(1e-2), f32(3e-2), f32(2e-2)]
    parts = _three_way(sizes)
    buf, (pv, vv) = banded(sizes, 2)
    for view, p in zip(pv, p0):
        view.copy_(p)
    dev = [torch.nn.Parameter(v) for v in pv]
    host = [torch.nn.Parameter(p.clone().to(DEV)) for p in p0]
    d_opts = [FusedRMSprop([dev[i] for i in idx], lr=lr, lr_on_device=True) for idx, lr in zip(parts, lrs) if idx]
    h_opts = [FusedRMSprop([host[i] for i in idx], lr=lr) for idx, lr in zip(parts, lrs) if idx]
    for o, idx in zip(d_opts, [idx for idx in parts if idx]):                # the moments inside the bands too
        for i in idx:
            o.state[dev[i]]["square_avg"] = vv[i].zero_()
    for t in range(1, 4):
        for pd, ph, g in zip(dev, host, _grads(sizes, t, 11)):
            pd.grad, ph.grad = g.to(DEV), g.to(DEV)
        rmsprop_step_many(d_opts)
        rmsprop_step_many(h_opts)
    assert all(pd.data_ptr() == v.data_ptr() for pd, v in zip(dev, pv))
    for i, (pd, ph) in enumerate(zip(dev, host)):
        assert torch.equal(pd, ph), f"RMSprop {layout}: parameter {i} ({sizes[i]} elements) differs from the host-lr twin"
        assert not torch.equal(ph.detach().cpu(), p0[i])
        sq = [o for o in h_opts if ph in o.state][0].state[ph]["square_avg"]
        assert torch.equal(vv[i], sq), f"RMSprop {layout}: square_avg {i} differs from the host-lr twin"
    assert_bands_untouched(buf, (pv, vv), f"RMSprop {layout}")


@pytest.mark.parametrize("layout", ["one", "65"])
def test_adam_device_lr_is_the_bitwise_twin_of_host_lr(layout):
    sizes = _sizes(layout)
    p0 = _start(sizes, 7)
    buf, (pv, mv, vv) = banded(sizes, 3)
    for view, p in zip(pv, p0):
        view.copy_(p)
    dev = [torch.nn.Parameter(v) for v in pv]
    host = [torch.nn.Parameter(p.clone().to(DEV)) for p in p0]
    d_opt, h_opt = SharedStepAdam(dev, lr=f32(1e-2), lr_on_device=True), SharedStepAdam(host, lr=f32(1e-2))
    for i, pd in enumerate(dev):
        d_opt.state[pd]["exp_avg"], d_opt.state[pd]["exp_avg_sq"] = mv[i].zero_(), vv[i].zero_()
    for t in range(1, 4):
        for pd, ph, g in zip(dev, host, _grads(sizes, t, 7)):
            pd.grad, ph.grad = g.to(DEV), g.to(DEV)
        d_opt.step()
        h_opt.step()
    assert float(d_opt.param_groups[0]["step"]) == 3.0
    for i, (pd, ph) in enumerate(zip(dev, host)):
        assert torch.equal(pd, ph), f"Adam {layout}: parameter {i} ({sizes[i]} elements) differs from the host-lr twin"
        assert not torch.equal(ph.detach().cpu(), p0[i])
        assert torch.equal(mv[i], h_opt.state[ph]["exp_avg"]) and torch.equal(vv[i], h_opt.state[ph]["exp_avg_sq"]), \
            f"Adam {layout}: moments of tensor {i} differ from the host-lr twin"
    assert_bands_untouched(buf, (pv, mv, vv), f"Adam {layout}")


# ---------------------------------------------------------------------------------------------- 2. schedules against fp64
def test_scheduled_steps_vs_torch_float64():
    """Ten steps under stock schedulers: StepLR(3, 0.8) on one RMSprop, ReduceLROnPlateau(0.7, patience 1) with a rising metric
    on another — both in one rmsprop_step_many — and StepLR(3, 0.7) on the Adam, against torch.optim in float64 under the same
    schedulers.  A rate that stayed where it started is 50 % off by the tenth step."""
    steps, sizes = 10, _sizes("65")
    alpha, eps, betas = f32(0.99), f32(1e-8), (f32(0.9), f32(0.999))
    lr_a, lr_b, lr_c = f32(3e-2), f32(2e-2), f32(1e-2)
    sch = torch.optim.lr_scheduler
    p0, q0 = _start(sizes, 11), _start(sizes, 7)
    even, odd = list(range(0, len(sizes), 2)), list(range(1, len(sizes), 2))
    dev = [torch.nn.Parameter(p.clone().to(DEV)) for p in p0]
    ref = [torch.nn.Parameter(p.double()) for p in p0]
    adev = [torch.nn.Parameter(p.clone().to(DEV)) for p in q0]
    aref = [torch.nn.Parameter(p.double()) for p in q0]
    o_a = FusedRMSprop([dev[i] for i in even], lr=lr_a, alpha=alpha, eps=eps, lr_on_device=True)
    o_b = FusedRMSprop([dev[i] for i in odd], lr=lr_b, alpha=alpha, eps=eps, lr_on_device=True)
    o_c = SharedStepAdam(adev, lr=lr_c, betas=betas, eps=eps, lr_on_device=True)
    r_a = torch.optim.RMSprop([ref[i] for i in even], lr=lr_a, alpha=alpha, eps=eps, foreach=False)
    r_b = torch.optim.RMSprop([ref[i] for i in odd], lr=lr_b, alpha=alpha, eps=eps, foreach=False)
    r_c = torch.optim.Adam(aref, lr=lr_c, betas=betas, eps=eps, foreach=False)
    plain = [sch.StepLR(o_a, 3, 0.8), sch.StepLR(r_a, 3, 0.8), sch.StepLR(o_c, 3, 0.7), sch.StepLR(r_c, 3, 0.7)]
    plateau = [sch.ReduceLROnPlateau(o_b, "min", factor=0.7, patience=1), sch.ReduceLROnPlateau(r_b, "min", factor=0.7, patience=1)]
    for t in range(1, steps + 1):
        for pd, pr, g in zip(dev, ref, _grads(sizes, t, 11)):
            pd.grad, pr.grad = g.to(DEV), g.double()
        for pd, pr, g in zip(adev, aref, _grads(sizes, t, 7)):
            pd.grad, pr.grad = g.to(DEV), g.double()
        rmsprop_step_many([o_a, o_b])                                       # eager: pushes the rates the schedulers set
        o_c.step()
        for o in (r_a, r_b, r_c):
            o.step()
        for s in plain:
            s.step()
        for s in plateau:
            s.step(float(t))
    # cuts after steps 3, 6, 9 (StepLR) and 3, 5, 7, 9 (plateau: patience 1 under a metric that only rises)
    assert o_a.param_groups[0]["lr"] == r_a.param_groups[0]["lr"] == pytest.approx(lr_a * 0.8 ** 3, rel=1e-12)
    assert o_b.param_groups[0]["lr"] == r_b.param_groups[0]["lr"] == pytest.approx(lr_b * 0.7 ** 4, rel=1e-12)
    assert o_c.param_groups[0]["lr"] == r_c.param_groups[0]["lr"] == pytest.approx(lr_c * 0.7 ** 3, rel=1e-12)
    assert push_lr([o_a, o_b, o_c]) == 0                                    # the tenth step pushed the last cut itself
    for o in (o_a, o_b, o_c):
        assert o.lr_dev.tolist() == [f32(o.param_groups[0]["lr"])]
    _assert_steps_close([dev[i] for i in even], [ref[i] for i in even], lr_a, steps, "RMSprop under StepLR(3, 0.8)")
    _assert_steps_close([dev[i] for i in odd], [ref[i] for i in odd], lr_b, steps, "RMSprop under ReduceLROnPlateau")
    _assert_steps_close(adev, aref, lr_c, steps, "Adam under StepLR(3, 0.7)")


# ---------------------------------------------------------------------------------------------- 3. a captured update follows a push
def test_captured_update_follows_push_lr():
    sizes = [1, 70_000, 5]
    p0, q0 = _start(sizes, 3), _start(sizes, 4)
    mk = lambda src: [torch.nn.Parameter(p.clone().to(DEV)) for p in src]
    dev, host, adev, ahost = mk(p0), mk(p0), mk(q0), mk(q0)
    grads = [g.to(DEV) for g in _grads(sizes, 1, 3)]
    for ps in (dev, host, adev, ahost):
        for p, g in zip(ps, grads):
            p.grad = g                                                      # static gradients, shared by every optimiser
    lr1, lr2, lr3 = f32(1e-2), f32(3e-2), f32(2e-3)
    d1, d2 = FusedRMSprop(dev[:2], lr=lr1, lr_on_device=True), FusedRMSprop(dev[2:], lr=lr2, lr_on_device=True)
    h1, h2 = FusedRMSprop(host[:2], lr=lr1), FusedRMSprop(host[2:], lr=lr2)
    d3, h3 = SharedStepAdam(adev, lr=lr3, lr_on_device=True), SharedStepAdam(ahost, lr=lr3)
    for o, ps in ((d1, dev[:2]), (d2, dev[2:])):                            # the moments a graph updates exist before capture
        for p in ps:
            o.state[p]["square_avg"] = torch.zeros_like(p)
    # every code object loaded before the capture: one eager step of both kernels on throw-away tensors
    w = [torch.nn.Parameter(torch.ones(3, device=DEV))]
    w[0].grad = torch.ones(3, device=DEV)
    FusedRMSprop(w, lr=lr1, lr_on_device=True).step()
    SharedStepAdam(w, lr=lr1, lr_on_device=True).step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rmsprop_step_many([d1, d2])
        d3.step()
    torch.cuda.synchronize()
    for p, q in zip(dev + adev, p0 + q0):
        assert torch.equal(p.detach().cpu(), q), "capturing must not run the update"

    def twin_step():
        rmsprop_step_many([h1, h2])
        h3.step()

    def assert_equal(what):
        for i, (a, b) in enumerate(zip(dev + adev, host + ahost)):
            assert torch.equal(a, b), f"{what}: parameter {i} differs from the eager host-lr twin"
        for od, oh, pd, ph in ((d1, h1, dev[:2], host[:2]), (d2, h2, dev[2:], host[2:])):
            for a, b in zip(pd, ph):
                assert torch.equal(od.state[a]["square_avg"], oh.state[b]["square_avg"]), what
        for a, b in zip(adev, ahost):
            assert torch.equal(d3.state[a]["exp_avg"], h3.state[b]["exp_avg"]), what
            assert torch.equal(d3.state[a]["exp_avg_sq"], h3.state[b]["exp_avg_sq"]), what

    graph.replay(); twin_step()
    assert_equal("first replay")
    d1.param_groups[0]["lr"] = h1.param_groups[0]["lr"] = lr1 * 0.5
    assert push_lr([d1, d2, d3]) == 1
    before = dev[1].detach().clone()
    graph.replay(); twin_step()
    assert_equal("replay after halving one RMSprop rate")
    assert not torch.equal(dev[1], before)
    d3.param_groups[0]["lr"] = h3.param_groups[0]["lr"] = lr3 * 0.5
    assert push_lr([d1, d2, d3]) == 1
    graph.replay(); twin_step()
    assert_equal("replay after halving the Adam rate")
    assert float(d3.param_groups[0]["step"]) == 3.0


# ---------------------------------------------------------------------------------------------- 4. trainers
def toy(device_hparams=True):
    g = load("joint_small")
    tr = _joint_trainer(g)
    if device_hparams:
        tr.enable_device_hparams()
        tr.enable_device_hparams()                                          # idempotent
    args = [torch.tensor(g[f"s0.{k}"], device=DEV) for k in ("x_t", "y_t", "x_s", "y_s")]
    return tr, args


def test_phase_replay_follows_a_changed_learning_rate():
    """"source_pretrain" replays bit-equal to the eager step (no CPC, nothing read from a device scalar but the rates): after
    halving fe_s's rate — no re-capture — it still does.  With the rates baked into the graph, fe_s would move by the old one."""
    phase = "source_pretrain"
    tr, args = toy()
    tr.capture_phase(phase, *args)
    snap = tr.snapshot()
    tr.opts["fe_s"].param_groups[0]["lr"] *= 0.5
    rep = clone(tr.replay_phase(phase, *args))
    assert tr.opts["fe_s"].lr_dev.tolist() == [f32(0.0005)]
    after_graph = tr.snapshot()["t"]
    tr.restore(snap)
    eager = tr.phase_step(phase, *args)
    same_losses(rep, eager, phase)
    same_state(phase, after_graph, tr.snapshot()["t"], phase + " at half fe_s's rate")
    # and the halved rate is what moved fe_s: RMSprop's first step is 10·lr·sign(g) wherever |g| >> eps
    key = "m.fe_s.net_1.net.net.1.conv1d.weight"
    moved = (after_graph[key] - snap["t"][key]).abs()
    assert float(moved.max()) <= 10 * 0.0005 * (1 + 1e-3), float(moved.max())
    assert float(moved.max()) >= 10 * 0.0005 * (1 - 1e-2), float(moved.max())


def test_joint_replay_follows_the_epoch():
    tr, args = toy()
    ts = (3, 5)
    torch.manual_seed(5)
    tr.capture(*args, epoch=0)
    snap = tr.snapshot()
    w = tr.m["cpc"].Wk[0].weight
    tr.replay(*args, ts, epoch=0)
    g0 = w.grad.detach().clone()
    tr.restore(snap)
    rep = clone(tr.replay(*args, ts, epoch=50))
    g50 = w.grad.detach().clone()
    after_graph = tr.snapshot()["t"]
    # CPC's gradient is 2·(c·∇sl_t + d·∇sl_s) with (c, d) = (2, 2) at epoch 0 and (2.5, 2.5) at epoch 50
    scale = float((1.25 * g0).abs().max())
    err = float((g50 - 1.25 * g0).abs().max())
    print(f"cpc.Wk[0].weight.grad: epoch 50 vs 1.25 x epoch 0: max diff {err:.3e}, scale {scale:.3e}")
    assert scale > 0 and err <= 7e-5 * scale, (err, scale)
    tr.restore(snap)
    eager = tr.step(*args, epoch=50, t_samples=ts)
    same_losses({k: rep[k] for k in JOINT_LOSSES}, {k: eager[k] for k in JOINT_LOSSES}, "joint replay(epoch=50) vs eager")
    after_eager = tr.snapshot()["t"]
    for k in ("m.fe_t.net_1.net.net.1.conv1d.weight", "m.nf.WN.0.in_layers.3.weight_v", "m.clf_t.hidden.weight", "m.cpc.Wk.0.weight", "w_s"):
        real_gradient_gate(after_graph, after_eager, k, "joint replay(epoch=50) vs eager")


def test_classifier_replay_follows_a_changed_learning_rate():
    gen = torch.Generator().manual_seed(7)
    fe_spec, clf_spec = R.train_specs(64, 1)
    Pf, Pc = R.init_feature_extractor(fe_spec, gen), R.init_classifier(clf_spec, 3, gen)
    mk = lambda: (torch.randn(8, 1, 64, generator=gen).to(DEV), torch.randint(3, (8,), generator=gen).to(DEV))
    (x0, y0), (x1, y1) = mk(), mk()
    tr = fst.ClassifierTrainer(64, 1, 3, DEV, device_hparams=True)
    tr.fe.load_state_dict({k: v.detach() for k, v in Pf.items()}); tr.clf.load_state_dict({k: v.detach() for k, v in Pc.items()})
    tr.capture(x0, y0, warmup=2)
    tr.replay(x1, y1)
    tr.opt_clf.param_groups[0]["lr"] *= 0.5

    def state():
        out = dict(("fe." + k, v) for k, v in tr.fe.state_dict().items())
        out.update(("clf." + k, v) for k, v in tr.clf.state_dict().items())
        for name, o in (("opt_fe", tr.opt_fe), ("opt_clf", tr.opt_clf)):
            for i, p in enumerate(o.param_groups[0]["params"]):
                out[f"{name}.{i}"] = o.state[p]["square_avg"]
        return out
    snap = {k: v.detach().clone() for k, v in state().items()}
    loss, logits = tr.replay(x0, y0)
    params = lambda: torch.cat([p.detach().flatten() for p in tr.parameters()]).clone()
    got = (float(loss), logits.clone(), {k: v.detach().clone() for k, v in state().items()}, params())
    assert tr.opt_clf.lr_dev.tolist() == [f32(0.0015)] and tr.opt_fe.lr_dev.tolist() == [f32(0.001)]
    with torch.no_grad():
        for k, v in state().items():
            v.copy_(snap[k])
    loss_e, logits_e = tr.step(x0, y0)                                       # eager, at the halved rate
    assert abs(got[0] - float(loss_e)) <= 1e-5 * max(1.0, abs(float(loss_e)))
    close(got[1], logits_e, 1e-4, "graph logits")
    diff = (got[3] - params()).abs()
    print(f"classifier replay vs eager at half opt_clf's rate: max diff {float(diff.max()):.3e}, "
          f"fraction beyond 1e-4 {float((diff > 1e-4).double().mean()):.4f}")
    assert float(diff.max()) <= 0.061 and float((diff > 1e-4).double().mean()) < 0.05
    # the classifier's dense layer has real gradients throughout: there the replay and the eager step agree element by element
    # (a replay at the captured 0.003 would be off by half a step everywhere)
    real_gradient_gate(got[2], state(), "clf.hidden.weight", "classifier replay vs eager")


def test_end_epoch_steps_pushes_and_survives_a_checkpoint():
    tr, args = toy()
    assert "schedules" not in tr.state_dict()
    with pytest.raises(RuntimeError, match="make_schedulers"):
        tr.end_epoch("nf", {})
    scheds = tr.make_schedulers()
    assert sorted(scheds) == sorted(tr.MODULES) and scheds is tr.schedulers
    rep = tr.step(*args, epoch=13, t_samples=(3, 5))
    rep["total"] = rep["nf_t"] + rep["nf_s"]
    pushed = [tr.end_epoch("nf_with_ce", rep) for _ in range(25)]           # the same report every epoch: a plateau for nf
    # fe_t, clf_t, fe_s, dimunif, clf_s, cpc after the 25th epoch (StepLR 25); nf after the 12th and the 23rd (patience 10)
    assert [i + 1 for i, n in enumerate(pushed) if n] == [12, 23, 25] and pushed[24] == 6 and pushed[11] == 1, pushed
    want = {"fe_t": 0.0008, "clf_t": 0.0024, "fe_s": 0.0008, "dimunif": 0.0008, "clf_s": 0.0024, "cpc": 0.0014, "nf": 0.00049,
            "noise": 0.005, "probtransfer": 0.001, "ad_net": 0.001, "fd_s": 0.001}
    opts = dict(tr.opts, cpc=tr.opt_cpc)
    for k, lr in want.items():
        assert opts[k].param_groups[0]["lr"] == pytest.approx(lr, rel=1e-12), k
        assert opts[k].lr_dev.tolist() == [f32(opts[k].param_groups[0]["lr"])], k
    sd = tr.state_dict()
    assert sd["schedules"]["epoch"] == 13 and sd["schedules"]["coefficients"] == (2, 3, 1.8, 1.5)
    other, _ = toy()
    addresses = [o.lr_dev.data_ptr() for o in other._scheduled_opts()]
    other.load_state_dict(sd)                                               # builds the schedulers itself
    opts2 = dict(other.opts, cpc=other.opt_cpc)
    for k, lr in want.items():
        assert opts2[k].param_groups[0]["lr"] == opts[k].param_groups[0]["lr"], k
        assert opts2[k].lr_dev.tolist() == [f32(opts[k].param_groups[0]["lr"])], k
        assert other.schedulers[k].state_dict() == scheds[k].state_dict(), k
    assert [o.lr_dev.data_ptr() for o in other._scheduled_opts()] == addresses
    assert other._coef.tolist() == [f32(v) for v in (2, 3, 1.8, 1.5)]
    assert other.end_epoch("nf_with_ce", rep) == 0 and tr.end_epoch("nf_with_ce", rep) == 0
    assert other.schedulers["nf"].state_dict() == scheds["nf"].state_dict()
    del sd["schedules"]                                                     # a checkpoint from before make_schedulers()
    third, _ = toy()
    third.load_state_dict(sd)
    assert third.schedulers is None and "schedules" not in third.state_dict()


def test_guards():
    tr, args = toy(device_hparams=False)
    tr.capture_phase("source_pretrain", *args)
    with pytest.raises(RuntimeError, match="capture is resident"):
        tr.enable_device_hparams()
    tr.release_phase()
    torch.manual_seed(5)
    tr.capture(*args, epoch=0)
    with pytest.raises(RuntimeError, match="capture is resident"):
        tr.enable_device_hparams()
    with pytest.raises(ValueError, match="captured at epoch 0"):
        tr.replay(*args, (3, 5), epoch=50)
    assert not tr.device_hparams and not any(o.lr_on_device for o in tr._scheduled_opts())
    ct = fst.ClassifierTrainer(64, 1, 3, DEV)
    x, y = torch.randn(8, 1, 64, device=DEV), torch.randint(3, (8,), device=DEV)
    ct.capture(x, y, warmup=1)
    with pytest.raises(RuntimeError, match="capture is resident"):
        ct.enable_device_hparams()
