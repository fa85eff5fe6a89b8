"""Train steps whose target and source batch differ in size, and batches of one.  Needs an MI355X.

The reference trains with ``DataLoader(batch_size=20, shuffle=True)`` without ``drop_last`` and pairs batch k of the target loader
with batch k of the source loader (train_and_test.py:135-136, 536-541, and every pre-training phase alike): a target set of 50
series and a source set of 67 end an epoch on the pair (10, 20), a set of 41 series ends on a batch of one.  Every other
comparison of a train step with the oracle in this suite runs ``B_t == B_s``, where
  * the three applications of a WN inside ``WaveGlow.shared_fold()`` (flow on feat_t, flow on feat_s, infer on z_s2t) leave
    equally shaped weight-gradient operands in the ``WNGradPool``,
  * ``NoiseTransfer.forward`` takes its kernel path, never the composition it falls back to for unequal shapes,
  * quirk Q5's two accumulation ratios B_t/N_t and B_s/N_s are the same number.

Geometry S is the joint fixture's (tests/golden/joint_small.npz): L_t = 32, C_in_t = 1, L_s = 24, C_in_s = 2, 3 / 4 classes,
feature width 20, WN n = 16, h = 10, CPC hidden 8 — the time-as-k weight-gradient kernels serve kind 1 at every layer and kind 0
at dilations >= 4, so the pooled path runs in the default arithmetic.  Device trainer and oracle start from the fixture's state;
the batches are drawn here, the CPC start indices pinned (both below T // 2 = 8).

Gates: ``_check_step``'s (1e-4 relative on losses, logits, feat_s2t, GradNorm weights; 1e-3 on the GradNorm norms) and ``GRAD_TOL``
of test_gpu_full_step.py (3e-5 exact-f32, 2e-4 split-bf16, of each module's largest oracle gradient, the oracle on the device run's
ReLU branches, each flip bounded by ``FLIP_BOUND``).  ``GRAD_TOL`` was measured at L = 512 / 1024 with equal batches; the (4, 4)
control of test 1 is its measurement at S (FST_GRAD_REPORT=1 prints the per-module errors), and no uneven pair is gated looser
than that control.  Where B = 1 makes a CPC loss exactly 0 in the oracle, the device value is within 1e-6 absolute of 0.

Measured on the MI355X, joint step at S, error of each module's gradients (of the module's largest oracle gradient):

  split-bf16     (4, 4)   (3, 4)   (4, 3)   (1, 4)   (5, 1)   (7, 2)      exact-f32  (4, 4)   (3, 4)   (4, 3)   (1, 4)   (5, 1)   (7, 2)
  fe_t          1.5e-05  1.9e-05  1.2e-05  1.4e-05  1.2e-05  1.6e-05                1.2e-06  3.7e-07  1.3e-06  9.0e-07  1.3e-06  1.1e-06
  clf_t         7.5e-06  9.8e-06  1.6e-05  1.2e-05  7.7e-06  8.6e-06                3.9e-07  1.6e-07  4.7e-07  3.5e-07  6.9e-07  1.1e-06
  fe_s          1.4e-05  1.8e-05  2.6e-05  1.9e-05  2.8e-05  2.4e-05                4.1e-07  3.9e-07  8.8e-07  8.8e-07  5.9e-07  1.1e-06
  dimunif       8.8e-06  6.8e-06  9.2e-06  9.1e-06  1.9e-05  1.4e-05                6.3e-07  6.1e-07  6.4e-07  6.7e-07  8.1e-07  6.8e-07
  clf_s         3.4e-06  3.6e-06  3.6e-06  3.2e-06  1.6e-06  4.4e-06                1.5e-07  1.5e-07  1.6e-07  1.5e-07  4.5e-08  1.4e-07
  probtransfer  7.9e-06  7.1e-06  3.6e-06  7.5e-06  4.1e-06  8.4e-06                2.4e-07  3.7e-07  3.1e-07  4.2e-07  2.4e-07  2.0e-07
  nf            1.5e-05  1.6e-05  2.0e-05  1.5e-05  1.5e-05  1.0e-05                1.8e-06  7.2e-07  1.7e-06  6.7e-07  5.0e-07  5.0e-07
  noise         2.4e-05  1.4e-05  1.7e-05  1.4e-05  1.2e-05  1.6e-05                7.6e-07  7.9e-07  1.0e-06  5.9e-07  6.4e-07  1.1e-06
  ad_net        9.9e-06  1.8e-05  9.3e-06  1.0e-05  6.1e-06  7.1e-06                8.4e-07  7.4e-07  6.6e-07  5.4e-07  2.7e-07  2.6e-07
  fd_s          9.1e-07  9.1e-07  1.0e-06  9.1e-07  1.7e-06  1.0e-06                3.5e-08  2.2e-08  3.0e-08  2.7e-08  4.5e-08  7.9e-08
  cpc           1.6e-05  1.6e-05  1.6e-05  4.2e-05  1.6e-05  1.2e-05                1.5e-05  9.0e-06  1.5e-05  2.8e-05  9.9e-06  3.6e-06

The control (4, 4) is inside GRAD_TOL (2e-4 / 3e-5), so GRAD_TOL gates every pair.  cpc at (1, 4): the target call has no gradient
(no negatives), so the source call alone sets the module's scale.  cpc in the exact-f32 column: the CPC forward's Gram product
follows the FST_MATH environment variable, not the ``arithmetic`` fixture — it is the split-bf16 one in both of the fixture's
modes, and its lse against the backward's fp32 logits is what shows.  Phases: <= 4.6e-5 split-bf16, <= 2.7e-5 exact-f32 (fe_t,
through the CPC gradient); cpc <= 4.0e-5 / 2.4e-5 at (1, 4).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from feature_level_style_transfer_for_tsc_amd import ops
from oracle import restatement as R
from test_gpu_full_step import (GRAD_TOL, LOSSES, _check_step, _grad_err, _pair, _phase_both, _step_both, _trainer_from,
                                arithmetic)                                        # noqa: F401  (arithmetic: a fixture)
from test_gpu_modules import _joint_trainer, _joint_trainer_untrained, close, load
from test_gpu_phase_graphs import clone, replay_vs_eager
from test_oracle_golden import _joint_from_golden

DEV = "cuda"
TS = (3, 5)                                  # CPC start indices
PAIRS = [(3, 4), (4, 3), (1, 4), (5, 1), (7, 2)]
CONTROL = (4, 4)
PHASES = ("target_pretrain", "source_pretrain", "ssl_with_ce", "ssl", "nf_with_ce", "nf")

_SHARED = {}


def _golden():
    if "g" not in _SHARED:
        _SHARED["g"] = load("joint_small")
    return _SHARED["g"]


def _pool(seed=2718):
    """Seven target and five source series of geometry S with labels, drawn once per seed; every batch is a leading slice."""
    if seed not in _SHARED:
        gen = torch.Generator().manual_seed(seed)
        _SHARED[seed] = (_pair(gen, 7, 1, 32, 3), _pair(gen, 5, 2, 24, 4))
    return _SHARED[seed]


def _batch(B_t, B_s, seed=2718):
    (x_t, y_t), (x_s, y_s) = _pool(seed)
    return (x_t[:B_t].clone(), y_t[:B_t].clone()), (x_s[:B_s].clone(), y_s[:B_s].clone())


def _on_device(batch):
    (x_t, y_t), (x_s, y_s) = batch
    return [x_t.to(DEV), y_t.to(DEV), x_s.to(DEV), y_s.to(DEV)]


def _both():
    """(fresh oracle, fresh device trainer), both in the joint fixture's initial state."""
    g = _golden()
    return _joint_from_golden(g)[0], _joint_trainer(g)


def _zero_at_batch_of_one(rep, rep_o, B_t, B_s, what):
    for key, B in (("sl_t", B_t), ("sl_s", B_s)):
        if B == 1 and key in rep_o:
            assert float(rep_o[key]) == 0.0, (what, key, float(rep_o[key]))
            assert abs(float(rep[key])) <= 1e-6, (what, key, float(rep[key]))


def _same_noise_state(tr, js, what, sums=False):
    n, st = tr.m["noise"], js.noise_state
    assert (n.time, n.cal_num_target, n.cal_num_source) == (st["time"], st["n_t"], st["n_s"]), what
    if sums:
        close(n.target_avg, st["target_avg"], 1e-4, f"{what} target_avg")
        close(n.source_avg, st["source_avg"], 1e-4, f"{what} source_avg")


# ------------------------------------------------------------------ 1. the joint step, with gradients
@pytest.mark.parametrize("B_t,B_s", PAIRS + [CONTROL])
def test_joint_step_vs_oracle(B_t, B_s, arithmetic):
    """One joint step at S from the fixture's state: nine losses, logits, feat_s2t, GradNorm norms and weights, the gradients of
    all eleven modules, NoiseTransfer's counters.  (4, 4) is the control on the same series: the measurement of GRAD_TOL at S."""
    js, tr = _both()
    what = f"S ({B_t}, {B_s}) {arithmetic}"
    rep_o, want, rep, grads = _step_both(js, tr, _batch(B_t, B_s), TS)
    assert all(np.isfinite(float(rep_o[k])) for k in LOSSES), (what, {k: float(rep_o[k]) for k in LOSSES})
    _zero_at_batch_of_one(rep, rep_o, B_t, B_s, what)
    _same_noise_state(tr, js, what)
    _check_step(rep_o, want, rep, grads, tr, what, math=arithmetic)


# ------------------------------------------------------------------ 2. the pre-training phases
def _check_phase(rep_o, want, rep, grads, tr, what, math):
    assert set(rep) == set(rep_o), (what, set(rep) ^ set(rep_o))
    for k, b in rep_o.items():
        a, b = float(rep[k]), float(b)
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (what, k, a, b)
    tol, errs = GRAD_TOL[math], {}
    for name in tr.MODULES:
        assert set(grads[name]) == set(want[name]), (what, name, set(grads[name]) ^ set(want[name]))
        if want[name]:
            errs[name] = _grad_err(tr.m[name], want[name], grads[name])
    assert errs, f"{what}: no module received a gradient"
    print(f"[grad report] {what}: " + " ".join(f"{n}={e:.1e}({k})" for n, (e, k) in errs.items()))
    for name, (e, k) in errs.items():
        assert e <= tol.get(name, tol["default"]), f"{what} {name} grad {k}: {e:.3e} of the module's gradient scale"


@pytest.mark.parametrize("phase,B_t,B_s", [(p, 3, 4) for p in PHASES]
                         + [(p, *pair) for p in ("nf_with_ce", "nf") for pair in ((1, 4), (5, 1))])
def test_phase_step_vs_oracle(phase, B_t, B_s, arithmetic):
    """``phase_step`` against the oracle's from identical state: ``total`` and every reported loss, which modules received
    gradients (exactly), and their values.  The two phases that run the flow — two applications of every WN — also at a batch of one."""
    js, tr = _both()
    what = f"{phase} ({B_t}, {B_s}) {arithmetic}"
    rep_o, want, rep, grads = _phase_both(js, tr, phase, _batch(B_t, B_s), TS)
    _zero_at_batch_of_one(rep, rep_o, B_t, B_s, what)
    _check_phase(rep_o, want, rep, grads, tr, what, arithmetic)


# ------------------------------------------------------------------ 3. the second call's state
def test_second_forward_uses_each_sides_own_ratio():
    """Two ``forward_losses`` calls, (3, 4) then (2, 5), no optimiser in between: the second call's accumulation ratios are
    2/3 (target) and 5/4 (source) — quirk Q5 — so one ratio used for both running sums, or the two swapped, shows in the sums
    and in everything downstream of NoiseTransfer."""
    js, tr = _both()
    for call, (B_t, B_s) in enumerate(((3, 4), (2, 5))):
        batch = _batch(B_t, B_s, seed=2718 + call)
        (x_t, y_t), (x_s, y_s) = batch
        Lo, aux_o = js.forward_losses(x_t, y_t, x_s, y_s, TS)
        ratios = tr.m["noise"].advance(B_t, B_s)
        Lg, aux = tr.forward_losses(*_on_device(batch), TS, noise_ratios=ratios)
        _same_noise_state(tr, js, f"call {call}", sums=True)
    assert ratios == (2 / 3, 5 / 4)
    for k in LOSSES:
        a, b = float(Lg[k]), float(Lo[k])
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (k, a, b)
    close(aux["feat_s2t"], aux_o["feat_s2t"], 1e-4, "second call feat_s2t")


# ------------------------------------------------------------------ 4. a shape change leaves nothing behind
def test_a_batch_of_another_size_leaves_nothing_behind(tmp_path):
    """Trainer A: a step at (4, 4), one at (3, 4), save, a step at (4, 4).  Trainer B (other initial weights, no optimiser state,
    has never seen another shape) loads the file and takes the same last step: anything keyed on shape that outlives a batch of
    another size — plan and table caches, workspaces, a pool's ``pending`` — makes A differ.  Gates: those of
    test_trainer_state_checkpoint_resume_equals_uninterrupted."""
    g = _golden()
    tr = _joint_trainer(g)
    for i, pair in enumerate((CONTROL, (3, 4))):
        tr.step(*_on_device(_batch(*pair)), epoch=0, t_samples=(2 + i, 5 - i))
    path = str(tmp_path / "trainer_state.pt")
    tr.save_state(path)
    last = _on_device(_batch(*CONTROL))
    want = tr.step(*last, epoch=0, t_samples=(4, 1))
    want_params = {k: v.detach().clone() for k, v in tr._state_tensors().items() if k.startswith("m.")}

    torch.manual_seed(999)
    fresh = _joint_trainer_untrained(g)
    fresh.load_state(path)
    got = fresh.step(*last, epoch=0, t_samples=(4, 1))
    for k in LOSSES:
        assert abs(got[k].item() - want[k].item()) <= 2e-5 * max(1.0, abs(want[k].item())), (k, got[k].item(), want[k].item())
    close(got["w_t"], want["w_t"], 1e-5, "w_t"); close(got["w_s"], want["w_s"], 1e-5, "w_s")
    close(got["logit_s2t"], want["logit_s2t"], 1e-4, "logit_s2t")
    got_params = fresh._state_tensors()
    for k in ("m.nf.WN.0.in_layers.3.weight_v", "m.clf_t.hidden.weight", "m.ad_net.ad_layer1.weight", "m.cpc.Wk.0.weight",
              "m.noise.apply_learnable_weight.weight"):
        close(got_params[k], want_params[k], 1e-2 if ".ad_net." in k else 2e-3, "post-step " + k)
    assert fresh.m["noise"].time == tr.m["noise"].time and fresh.m["ad_net"].iter_num == tr.m["ad_net"].iter_num


# ------------------------------------------------------------------ 5. under hipGraph capture
def test_captured_joint_step_at_uneven_batches():
    """``capture`` at (3, 4); one replay equals the eager step from the same snapshot (gates of
    test_hipgraph_replay_matches_eager_step, and feat_s2t at 1e-4: NoiseTransfer's composition for unequal shapes reads the two
    ratio TENSORS the host refreshes, and a ratio baked in at capture — one call earlier — would move it); a replay on another
    batch of the same sizes gives another result; another pair of sizes is refused."""
    tr = _joint_trainer(_golden())
    args = _on_device(_batch(3, 4))
    torch.manual_seed(5)
    tr.capture(*args, epoch=0)
    snap = tr.snapshot()
    rep = clone(tr.replay(*args, TS))
    after_graph = tr.snapshot()
    tr.restore(snap)
    eager = tr.step(*args, epoch=0, t_samples=TS)
    for k in LOSSES:
        assert abs(rep[k].item() - eager[k].item()) <= 1e-4 * max(1.0, abs(eager[k].item())), (k, rep[k].item(), eager[k].item())
    close(rep["logit_s2t"], eager["logit_s2t"], 1e-4, "graph vs eager logit_s2t")
    close(rep["feat_s2t"], eager["feat_s2t"], 1e-4, "graph vs eager feat_s2t")
    close(rep["w_t"], eager["w_t"], 1e-4, "graph vs eager w_t")
    after_eager = tr.snapshot()
    assert after_graph["host"] == after_eager["host"]
    for k in ("m.fe_t.net_1.net.net.1.conv1d.weight", "m.nf.WN.0.in_layers.3.weight_v", "m.cpc.Wk.0.weight", "w_s",
              "noise.target_avg", "noise.source_avg"):
        close(after_graph["t"][k], after_eager["t"][k], 2e-3, "post-step " + k)
    tr.restore(snap)
    other = tr.replay(*_on_device(_batch(3, 4, seed=99)), TS)
    assert float((other["feat_s2t"] - rep["feat_s2t"]).abs().max()) > 1e-3 * float(rep["feat_s2t"].abs().max())
    assert abs(other["nf_s"].item() - rep["nf_s"].item()) > 1e-6 and abs(other["nf_t"].item() - rep["nf_t"].item()) > 1e-6
    with pytest.raises(RuntimeError):
        tr.replay(*_on_device(_batch(4, 4)), TS)


def test_captured_phase_at_uneven_batches():
    tr = _joint_trainer(_golden())
    args = _on_device(_batch(3, 4))
    tr.capture_phase("nf_with_ce", *args)
    rep = clone(replay_vs_eager(tr, "nf_with_ce", args, TS, "nf_with_ce (3, 4)"))
    other = replay_vs_eager(tr, "nf_with_ce", _on_device(_batch(3, 4, seed=99)), TS, "nf_with_ce (3, 4), another batch")
    assert abs(float(other["total"]) - float(rep["total"])) > 1e-4
    with pytest.raises(ValueError):
        tr.replay_phase("nf_with_ce", *_on_device(_batch(4, 4)), t_samples=TS)


# ------------------------------------------------------------------ 7. the metric geometry once
def test_metric_geometry_joint_step_vs_oracle(monkeypatch):
    """L = 512, C_in = 1, 4 classes at (3, 4), default arithmetic: uneven batches through the GRU and CPC kernels at hidden 64,
    ``FixedMatmulFn`` and the time-as-k weight-gradient kernels of both kinds at h = 25 — the shapes the benchmark runs."""
    monkeypatch.setattr(ops, "MATH", "bf16x3")
    L = 512
    js = R.build_joint_step(L, 1, L, 1, 4, 4, seed=3412, dropout_p=0.0, zero_end=False)
    tr = _trainer_from(js, L, L, 4)
    gen = torch.Generator().manual_seed(3413)
    batch = (_pair(gen, 3, 1, L, 4), _pair(gen, 4, 1, L, 4))
    rep_o, want, rep, grads = _step_both(js, tr, batch, (L // 8, L // 16))
    _same_noise_state(tr, js, "L=512 (3, 4)")
    _check_step(rep_o, want, rep, grads, tr, "L=512 (3, 4)", math="bf16x3")
