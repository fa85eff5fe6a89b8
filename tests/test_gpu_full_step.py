"""The WHOLE joint step (train_and_test.py:539-766) at the sizes BASELINE.json names, forward AND backward:

* configs[1] geometry (univariate, L=512): nine losses, logits, GradNorm norms/weights and every accumulated gradient
  (the reference's double backward, quirk Q3) against the CPU oracle at B=4;
* the same at configs[4]'s length (L=1024), B=2;
* configs[2]: four source domains -> four independent pipelines trained one step each -> K=4 eval forward -> vote
  (main.py:7-11, multi_source_voting.py:265-277,281-424), every pipeline's step against the oracle and the vote
  against the restated voting block on oracle logits;
* at the metric's full batch (B=256, L=512): capture() + replay() == step() from the same snapshot.
"""
import contextlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import ops as _ops
from oracle import restatement as R
from test_gpu_modules import close, live_masks

DEV = "cuda"
LOSSES = ("nf_t", "nf_s", "ce_t", "sl_t", "ce_s", "sl_s", "cdan", "ce_s2t2s", "fd_s")


def _pair(gen, B, C_in, L, ncls):
    x = torch.randn(B, C_in, L, generator=gen)
    x = (x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True)
    return x, torch.randint(ncls, (B,), generator=gen)


def _trainer_from(js, L_t, L_s, ncls):
    cfg = fst.JointConfig(L_t=L_t, C_in_t=1, L_s=L_s, C_in_s=1, n_class_t=ncls, n_class_s=ncls, dropout_p=0.0)
    tr = fst.JointTrainer(cfg, DEV)
    tr.load_params({k: {n: t.detach() for n, t in v.items()} for k, v in js.m.items()}, js.mats)
    return tr


FLIP_BOUND = 1e-4      # an imposed branch may differ from the oracle's own only where |pre-activation| <= this · max|pre-activation|


@contextlib.contextmanager
def _head_unit_branches(record=None, impose=None, flips=None):
    """The branch every unit of the ReLU / LeakyReLU layers that run as torch ops takes — the MLP heads (2-D: adversarial
    net, feature discriminator) and the dimension unification (3-D, 512 units per (sample, channel) row) — recorded from
    one run, or imposed on another.  Gradients of a piecewise-linear network are comparable only on the same piece: a unit
    whose pre-activation is within rounding distance of zero takes either branch depending on the last bits, and one such
    unit at B = 3 moves every gradient upstream of it by percent.  The forward VALUE is unaffected (the pre-activation is
    ~0 either way), so the oracle is stepped on the piece the device run was on and then compared tightly.  The ReLUs
    fused into the BatchNorm kernels (the omni-scale convolutions) are recorded from the launches' outputs (out > 0).
    Imposing is BOUNDED: wherever the imposed branch differs from the one the oracle's own pre-activation selects, that
    pre-activation must be within FLIP_BOUND of zero relative to the layer's largest — a unit the device got wrong by more
    than rounding fails here instead of dragging the oracle along.  ``flips`` (a list) receives (layer index, units
    flipped, largest |x|/max|x| among them) per layer with any."""
    relu0, leaky0, dimunif0 = F.relu, F.leaky_relu, R.dimension_unification
    it = iter(impose) if impose is not None else None
    inside = [0]
    layer_no = [0]

    def bounded(x, m):
        layer_no[0] += 1
        diff = (x.detach() > 0) != m
        if bool(diff.any()):
            worst = float(x.detach()[diff].abs().max()) / max(1e-30, float(x.detach().abs().max()))
            if flips is not None:
                flips.append((layer_no[0], int(diff.sum()), worst))
            assert worst <= FLIP_BOUND, (f"layer {layer_no[0]}: {int(diff.sum())} unit(s) take the other branch on the device with "
                                         f"|x|/max|x| up to {worst:.2e} — not a rounding-level disagreement")

    # record mode sees the layers that call F.relu on the device (heads, dimension unification) plus — through the wrappers
    # below — the ReLUs fused into the BatchNorm launches; impose mode consumes one recorded mask per ReLU of the oracle
    def relu(x, inplace=False):
        if record is not None:
            record.append((x > 0).cpu())
            return relu0(x, inplace)
        m = next(it)
        assert m.shape == x.shape, (m.shape, x.shape)
        bounded(x, m)
        return x * m.to(x.dtype)

    def leaky(x, negative_slope=0.01, inplace=False):
        if record is not None:
            record.append((x > 0).cpu())
            return leaky0(x, negative_slope, inplace)
        m = next(it)
        assert m.shape == x.shape, (m.shape, x.shape)
        bounded(x, m)
        return torch.where(m, x, negative_slope * x)

    def dimunif(*a, **k):
        inside[0] += 1
        try:
            return dimunif0(*a, **k)
        finally:
            inside[0] -= 1

    from feature_level_style_transfer_for_tsc_amd import ops as _ops
    F.relu, F.leaky_relu = relu, leaky
    if impose is not None:
        R.dimension_unification = dimunif
    if record is not None:
        # the omni-scale layers' ReLUs run inside the BatchNorm kernels: record the branch from the launch's output
        bn_act, bn_join = _ops.BNActFn.apply, _ops.BNAddBNReluFn.apply

        def bn_act_rec(*a):
            out = bn_act(*a)
            if a[6]:                                               # relu flag of BNActFn.forward
                record.append((out.detach() > 0).cpu())
            return out

        def bn_join_rec(*a):
            out = bn_join(*a)
            record.append((out.detach() > 0).cpu())
            return out
        _ops.BNActFn.apply, _ops.BNAddBNReluFn.apply = bn_act_rec, bn_join_rec
        # the heads' ReLU / LeakyReLU layers run in the epilogues of their GEMMs (LinearActFn: out > 0 <=> pre-activation > 0
        # for both), the dimension unification's second ReLU in the epilogue of its 1x1 conv
        lin_act, conv_relu = _ops.LinearActFn.apply, _ops.ConvReluFn.apply

        def epi_rec(fn, act_arg=None):
            def wrapped(*a):
                out = fn(*a)
                if act_arg is None or a[act_arg] != _ops.ACT_NONE:
                    record.append((out.detach() > 0).cpu())
                return out
            return wrapped
        _ops.LinearActFn.apply, _ops.ConvReluFn.apply = epi_rec(lin_act, 3), epi_rec(conv_relu)
    try:
        yield
        if it is not None:
            assert next(it, None) is None, "the oracle evaluated fewer synchronised layers than the device run"
    finally:
        F.relu, F.leaky_relu, R.dimension_unification = relu0, leaky0, dimunif0
        if record is not None:
            del _ops.BNActFn.apply, _ops.BNAddBNReluFn.apply       # back to the inherited Function.apply
            del _ops.LinearActFn.apply, _ops.ConvReluFn.apply


def _step_both(js, tr, batch, ts):
    """One step of the HIP trainer and of the oracle from identical state, the oracle on the linear piece the device run
    took in the MLP heads; returns (oracle report, oracle grads, trainer report, trainer grads) with the gradients taken
    right before the optimisers consume them."""
    (x_t, y_t), (x_s, y_s) = batch
    grads, branches = {}, []

    def grab():
        for name in tr.MODULES:
            grads[name] = {n: p.grad.detach().clone() for n, p in tr.m[name].named_parameters() if p.grad is not None}
    tr.on_grads_ready = grab
    with _head_unit_branches(record=branches):
        rep = tr.step(x_t.to(DEV), y_t.to(DEV), x_s.to(DEV), y_s.to(DEV), epoch=0, t_samples=ts)
    tr.on_grads_ready = None
    assert branches, "no head layer went through torch.nn.functional"
    flips = []
    with _head_unit_branches(impose=branches, flips=flips):
        rep_o = js.step(x_t, y_t, x_s, y_s, epoch=0, t_samples=ts)
    if os.environ.get("FST_GRAD_REPORT"):
        print(f"[branch report] {sum(int(b.numel()) for b in branches)} synchronised units, flipped (layer, units, |x|/max): {flips}")
    want = {name: {n: p.grad.detach().numpy().copy() for n, p in P.items() if p.requires_grad and p.grad is not None}
            for name, P in js.m.items()}
    return rep_o, want, rep, grads


def _phase_both(js, tr, phase, batch, ts):
    """``_step_both`` for one batch of a pre-training phase: ``tr.phase_step`` and ``js.phase_step`` from identical state, the
    oracle on the device run's ReLU branches; same return value.  ``js`` must be fresh: the oracle's ``phase_step`` never zeroes
    its gradients, so a leaf's ``.grad`` is what this one pass left there (None where the phase does not reach it)."""
    (x_t, y_t), (x_s, y_s) = batch
    grads, branches = {}, []

    def grab():
        for name in tr.MODULES:
            grads[name] = {n: p.grad.detach().clone() for n, p in tr.m[name].named_parameters() if p.grad is not None}
    tr.on_grads_ready = grab
    with _head_unit_branches(record=branches):
        rep = tr.phase_step(phase, x_t.to(DEV), y_t.to(DEV), x_s.to(DEV), y_s.to(DEV), t_samples=ts)
    tr.on_grads_ready = None
    assert branches, "no ReLU layer of the phase was recorded"
    assert all(p.grad is None for P in js.m.values() for p in P.values()), "the oracle carries gradients of an earlier pass"
    flips = []
    with _head_unit_branches(impose=branches, flips=flips):
        rep_o = js.phase_step(phase, x_t, y_t, x_s, y_s, t_samples=ts)
    if os.environ.get("FST_GRAD_REPORT"):
        print(f"[branch report] {phase}: {sum(int(b.numel()) for b in branches)} synchronised units, flipped (layer, units, |x|/max): {flips}")
    want = {name: {n: p.grad.detach().numpy().copy() for n, p in P.items() if p.requires_grad and p.grad is not None}
            for name, P in js.m.items()}
    return rep_o, want, rep, grads


# Gradient tolerances (of each module's largest gradient), with the oracle on the device run's piece of EVERY ReLU / LeakyReLU
# layer — the MLP heads and the dimension unification (torch ops) and the omni-scale layers (fused into the BatchNorm launches,
# recorded from their outputs) — each imposed branch bounded to a rounding-level pre-activation (FLIP_BOUND).  Measured on the
# MI355X over the steps below and B = 32 (tests/test_gpu_full_size.py); FST_GRAD_REPORT=1 prints them:
#  * exact-f32 MFMA mode: <= 6e-6 in all eleven modules                      -> gate 3e-5
#  * split-bf16 mode:     <= 7e-5 (extractors), <= 2.5e-5 everywhere else    -> gate 2e-4
# This is the gate on the step's LOGIC (which loss reaches which parameter with which coefficient, the double backward of quirk
# Q3, the GRL coefficients) — it caught the critic coefficient being read before the second critic call (3e-2) — and on the
# arithmetic of every kernel in the backward pass.  Round 2's gates were 5e-2 / 1e-2 for the modules with convolutions in front
# of a train-mode BatchNorm, attributed to cancellation in Σ dy·x amplifying the split-bf16 product error; that was wrong: with
# the convolutional ReLUs on the same piece the same gradients agree to 7e-5 at B = 3, 4 and 32 alike — the percent-level
# differences were single ReLU elements of B·C·L taking the other branch (each flip bounded here: |x| <= 6e-6 of the layer's max).
GRAD_TOL = {"f32": {"default": 3e-5},
            "bf16x3": {"default": 2e-4}}


@pytest.fixture(params=["bf16x3", "f32"])
def arithmetic(request):
    from feature_level_style_transfer_for_tsc_amd import ops
    prev, ops.MATH = ops.MATH, request.param
    yield request.param
    ops.MATH = prev


def _check_step(rep_o, want, rep, grads, tr, what, math="bf16x3"):
    for k in LOSSES:
        a, b = float(rep[k]), float(rep_o[k])
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (what, k, a, b)
    for k in ("logit_t", "logit_s", "logit_s2t"):
        close(rep[k], rep_o[k], 1e-4, f"{what} {k}")
    close(rep["feat_s2t"], rep_o["feat_s2t"], 1e-4, f"{what} feat_s2t")
    close(rep["norms_t"], rep_o["norms_t"], 1e-3, f"{what} GradNorm norms_t")
    close(rep["norms_s"], rep_o["norms_s"], 1e-3, f"{what} GradNorm norms_s")
    close(rep["w_t"], rep_o["w_t"], 1e-4, f"{what} w_t")
    close(rep["w_s"], rep_o["w_s"], 1e-4, f"{what} w_s")
    tol, errs = GRAD_TOL[math], {}
    for name in tr.MODULES:
        errs[name] = _grad_err(tr.m[name], want[name], grads[name])
    if os.environ.get("FST_GRAD_REPORT"):
        print(f"[grad report] {what}: " + " ".join(f"{n}={e:.1e}({k})" for n, (e, k) in errs.items()))
    for name, (e, k) in errs.items():
        assert e <= tol.get(name, tol["default"]), f"{what} Q3 {name} grad {k}: {e:.3e} of the module's gradient scale"


def _grad_err(module, want, grads):
    """(largest |got − want| over the module's parameters ÷ the module's largest oracle gradient, the parameter it is at).
    Omni-scale conv weights: the reference's gradient is dense over the Kmax taps (it masks ``weight.data``, OS_CNN.py:67-70,
    not the graph); layers whose masked-tap gradients nobody reads compute only the taps their row groups cover, so a
    masked tap holds either exactly 0 (not computed) or the dense value — compared wherever it is not 0."""
    scale = max(float(np.abs(v).max()) for v in want.values())
    masks = live_masks(module)
    worst = (0.0, "")
    for k, v in want.items():
        assert k in grads and grads[k] is not None, f"{k}: no grad"
        got = grads[k].detach().cpu().numpy().astype(np.float64)
        if k in masks:
            got = np.where((masks[k] == 0) & (got == 0), v, got)
        e = float(np.abs(got - v).max()) / max(scale, 1e-30)
        if e > worst[0]:
            worst = (e, k)
    return worst


@pytest.mark.parametrize("L,B,seed", [(512, 4, 512), (1024, 2, 1024)])
def test_whole_joint_step_with_gradients_vs_oracle(L, B, seed, arithmetic):
    """configs[1] (L=512) and configs[4] (L=1024) geometry: forward, GradNorm and the accumulated gradients of the
    whole step, all eleven modules, against the oracle from identical seeded state."""
    js = R.build_joint_step(L, 1, L, 1, 4, 4, seed=seed, dropout_p=0.0, zero_end=False)
    tr = _trainer_from(js, L, L, 4)
    gen = torch.Generator().manual_seed(seed + 1)
    batch = (_pair(gen, B, 1, L, 4), _pair(gen, B, 1, L, 4))
    _check_step(*_step_both(js, tr, batch, (L // 8, L // 16)), tr, f"L={L} {arithmetic}", math=arithmetic)


def test_config2_four_sources_one_step_each_then_vote():
    """configs[2]: four source domains at len=512.  The reference trains one pipeline per source (main.py:7-11) and
    votes over the saved target-side checkpoints (multi_source_voting.py:265-277,281-424).  Here: four JointTrainers
    (different seeds, i.e. different source domains and initialisations) take one step each — every step checked
    against the oracle incl. gradients — then the four post-step (extractor, classifier) pairs vote on a test set:
    K=4 eval forward + batched vote on the device against the oracle's eval forward of the SAME post-step weights
    (copied back to the CPU: the first RMSprop step of a zero-gradient bias is +-10*lr by the sign of rounding noise,
    DESIGN.md "chaotic trajectory", so post-step weights are compared by what they predict, not bit for bit) fed to
    the restated voting block."""
    L, B, ncls, K = 512, 3, 4, 4
    gen = torch.Generator().manual_seed(2024)
    target = _pair(gen, B, 1, L, ncls)                                     # one target domain, four sources
    models, oracle_params = [], []
    for k in range(K):
        js = R.build_joint_step(L, 1, L, 1, ncls, ncls, seed=100 + k, dropout_p=0.0, zero_end=False)
        tr = _trainer_from(js, L, L, ncls)
        batch = (target, _pair(gen, B, 1, L, ncls))
        _check_step(*_step_both(js, tr, batch, (17 + k, 40 - k)), tr, f"source {k}")
        fe, clf = tr.m["fe_t"], tr.m["clf_t"]
        # one optimisation step leaves the BatchNorm running statistics at 0.9·init + 0.1·batch: eval-mode logits of such a
        # model are in the hundreds, where the reference's own vote — exp(x)/Σexp(x) in float32 (multi_source_voting.py:407)
        # — overflows to NaN.  Let the statistics settle (train-mode forwards, no parameter update) as an epoch would.
        with torch.no_grad():
            for _ in range(40):
                clf(fe(target[0].to(DEV)))
        fe.eval(); clf.eval()
        models.append((fe, clf))
        oracle_params.append(({n: v.detach().cpu() for n, v in fe.state_dict().items()},
                              {n: v.detach().cpu() for n, v in clf.state_dict().items()}))
    mk = lambda n: [_pair(gen, 5, 1, L, ncls) for _ in range(n)]
    train, test = mk(3), mk(2)
    w, scores, pred, acc = fst.multi_source_voting(models, train, test)
    fe_spec, clf_spec = R.train_specs(L, 1)

    def oracle_logits(batches):
        out = [torch.cat([R.classifier(R.feature_extractor(x, Pf, fe_spec, False), Pc, clf_spec, False)[0] for x, _ in batches])
               for Pf, Pc in oracle_params]
        return torch.stack(out).detach().numpy(), torch.cat([y for _, y in batches]).numpy()
    (trl, try_), (tel, tey) = oracle_logits(train), oracle_logits(test)
    got_tel, _ = fst.collect_logits(models, test)
    close(got_tel, tel, 1e-4, "K=4 eval logits")
    w_o, scores_o, pred_o, acc_o = R.multi_source_vote(trl, try_, tel, tey)
    np.testing.assert_allclose(w.cpu().numpy(), w_o, rtol=1e-9, atol=0)
    np.testing.assert_allclose(scores.cpu().numpy(), scores_o, rtol=2e-3)   # 9^w (1+120 e^-H) amplifies the 1e-4 logit tolerance
    assert np.array_equal(pred.cpu().numpy(), pred_o) and abs(acc - acc_o) < 1e-12


def test_full_batch_graph_replay_equals_eager_step():
    """B=256, L=512 (the bench configuration): one replay of the captured hipGraph equals the eager step from the
    same snapshot — nine losses, logits, GradNorm weights, and the post-step state of parameters with real gradients."""
    B, L = 256, 512
    torch.manual_seed(1234)
    tr = fst.JointTrainer(fst.JointConfig(L_t=L, L_s=L, dropout_p=0.0), DEV)  # the bench configuration, dropout off (its masks are drawn per call)
    gen = torch.Generator().manual_seed(7)
    (x_t, y_t), (x_s, y_s) = _pair(gen, B, 1, L, 4), _pair(gen, B, 1, L, 4)
    args = (x_t.to(DEV), y_t.to(DEV), x_s.to(DEV), y_s.to(DEV))
    tr.capture(*args, epoch=0)
    snap = tr.snapshot()
    rep = {k: v.clone() for k, v in tr.replay(*args, (31, 77)).items()}
    after_graph = tr.snapshot()
    # run-to-run: a second replay from the same state reproduces the first bit for bit — every reported tensor and every
    # tensor the step mutates (parameters, BatchNorm buffers, optimiser moments): no float atomics are left on the step's path
    tr.restore(snap)
    rep2 = tr.replay(*args, (31, 77))
    for k, v in rep.items():
        diff = float((rep2[k].double() - v.double()).abs().max())
        if _ops.MATH == "bf16x3":
            assert torch.equal(rep2[k], v), f"two replays differ in {k}: {diff:.3e}"
        else:
            # FST_MATH=f32: RandomLayer's products run on the conv engine's K-split GEMM with float atomics (see below): the CDAN
            # branch — forward value included — moves in the last bits from run to run
            assert diff <= 1e-5 * max(1.0, float(v.double().abs().max())), f"two replays differ in {k}: {diff:.3e}"
    again = tr.snapshot()["t"]
    differing = [k for k, v in after_graph["t"].items() if not torch.equal(again[k], v)]
    # FST_MATH=f32: fst_nt_gemm is a split-bf16 kernel, so RandomLayer's 25600 x 1024 products fall back to the conv engine's K-split
    # GEMM, whose slices are added with float atomics (FST_EPI_ATOMIC): the CDAN branch's data gradient — and every
    # gradient upstream of it — moves in the last bits from run to run, and RMSprop turns last bits of a rounding-noise gradient
    # (conv biases in front of a BatchNorm) into +-lr steps.  The state comparison is the default arithmetic's.
    if _ops.MATH == "bf16x3":
        assert not differing, f"two replays leave different state in {len(differing)} tensors, e.g. {differing[:5]}"
    tr.restore(snap)
    eager = tr.step(*args, epoch=0, t_samples=(31, 77))
    for k in LOSSES:
        a, b = float(rep[k]), float(eager[k])
        assert abs(a - b) <= 1e-6 * max(1.0, abs(b)), (k, a, b)
    # Two runs of the product from the same state: every launch of the step is deterministic (BatchNorm moments, bias-gradient
    # row sums and the CPC loss are fixed-order sums, the K-split GEMMs reduce slabs: tools/determinism_probe.py shows
    # eager/eager and graph/graph bit-identical), and the captured step issues the same launches as the eager one, so the gate
    # is north_star's 1e-4 with a wide margin — measured: 0 on every forward quantity, 1e-7 on parameters after the update
    # (the graph reads the CPC start index / NoiseTransfer ratios from device scalars).
    for k in ("logit_t", "logit_s", "logit_s2t", "feat_t", "feat_s2t", "w_t", "w_s", "norms_t", "norms_s"):
        close(rep[k], eager[k], 1e-5, f"graph vs eager {k}")
    after_eager = tr.snapshot()
    # weights whose gradient is real (not rounding noise in front of a BatchNorm): RMSprop's first-step size is
    # lr*g/sqrt(0.01 g^2) = 10*lr whatever |g|, so equal signs give equal steps
    for k in ("m.fe_t.net_1.net.net.1.conv1d.weight", "m.nf.WN.0.in_layers.3.weight_v", "m.nf.WN.2.res_skip_layers.7.weight_g",
              "m.clf_t.hidden.weight", "m.cpc.Wk.0.weight", "w_s"):
        d = (after_graph["t"][k] - after_eager["t"][k]).abs()
        scale = float(after_eager["t"][k].abs().max())
        assert float((d > 2e-3 * scale).double().mean()) < 0.01, (k, float(d.max()), scale)
