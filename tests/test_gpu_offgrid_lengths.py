"""Train steps, captures, the anomaly guard and inference at sequence lengths OFF the kernels' fast paths.  The tests marked
``gpu`` need an MI355X; ``test_inputs_are_well_conditioned_for_fp32_torch`` runs on the CPU.

Kernel dispatch depends on the sequence length: the split-bf16 conv kernels and the fused WN kernels need L % 4 == 0, the one-launch
WN stack backward L <= 512 as well, the time-as-k WN weight-gradient kernels (and with them the pooled ``WNGradPool`` path) and the
dense-tap weight gradient L % 32 == 0, RandomLayer's ``nt_gemm`` (C·L_t) % 32 == 0, NoiseTransfer's kernels (C·L_t) % 4 == 0, and
CPC(C, hidden, L_t // 2) leaves the last sample of an odd L_t without a prediction.  Every other whole-step comparison of this
suite runs at L_t = 32, 512 or 1024, where each predicate picks the fast path.

Geometry (``_oracle_pair``): fixture S's construction (oracle/capture_fixtures.py) freed from S's lengths — target kernels 1..7
(L_t >= 28), source kernels 1..5 (L_s >= 20), C_in = 1 / 2, 3 / 4 classes, WN n = 16, CPC hidden 8, RandomLayer / ad_net at
1024; k = 1 gives feature width C = 10 (h = 5; C·L % 4 == 2 at every odd L), k = 2 gives C = 20 (C·L % 4 == 0 always).

Reference: the oracle in DOUBLE precision (``R.joint_step_as``), stepped on the device run's ReLU branches, every flip bounded
by FLIP_BOUND.  Gates: ``_check_step``'s (1e-4 relative on values, 1e-3 on the GradNorm norms) and ``GRAD_TOL`` unchanged
(3e-5 exact-f32, 2e-4 split-bf16).  The control (32, 24) is the measurement at this geometry; no off-grid case is gated looser.

Route tuple asserted per case in split-bf16 mode — (wn_fused_ok, wn_stack_bwd_ok, wn_wgrad_ok kind 0 at dilation 4, wn_wgrad_ok
kind 1, (C·L_t) % 32 == 0 [nt_gemm's arithmetic condition; where it is false RandomLayer pads, see the end], (C·L_t) % 4):

  control (32, 24), and (32, 27)                 (T, T, T, T, T, 0)    kind 0 at dilations 1, 2: only on a tensor with slack
  (36, 44), (100, 28)   L % 4 == 0, % 32 != 0    (T, T, F, F, F, 0)
  (520, 36)             beyond one-launch bwd    (T, F, F, F, F, 0)
  (30, 22)              L % 4 == 2               (F, F, F, F, F, 0)
  (31, 27), (31, 32), (33, 25) at k = 1          (F, F, F, F, F, 2)    NoiseTransfer's composition
  (33, 25) at k = 2                              (F, F, F, F, F, 0)    NoiseTransfer's kernels at an odd length

Condition on the inputs (``test_inputs_are_well_conditioned_for_fp32_torch``, no GPU): for every case and seed used here the
fp32 oracle, stepped on the fp64 oracle's ReLU branches, stays within GRAD_TOL["f32"] / 3 = 1e-5 of the fp64 oracle in every
module — so a device miss of 3e-5 is never the inputs' conditioning.

Seed 5 was rejected for every case: at (31, 27) and (31, 32) with input seed 1 the fp32 oracle is 8.1e-5 / 3.4e-5 off the fp64
one in fe_t (every other module <= 2.8e-6).  Not a flip: no ReLU, LeakyReLU or SELU unit changes branch between the two runs, and
imposing the fp64 branches changes nothing.  Conditioning: seed 5 draws a shortcut-conv weight of 0.003 for one channel, whose
batch variance (1.1e-5) is the size of BatchNorm's eps, and that channel's ``net_1.res.conv1d.weight`` gradient carries the whole
error.  With seed 6 every case is within 8.2e-7.

Measured on the MI355X, one joint step against the fp64 oracle, error of each module's gradients (of the module's largest oracle
gradient); columns are (L_t, L_s), k = 1 and B = (4, 4) unless named:

  split-bf16         32-24      36-44     100-28      30-22      31-27      33-25   33-25-k2      32-27      31-32 31-27-B3-4     520-36
  fe_t             3.3e-05    8.3e-06    1.2e-05    8.3e-06    8.0e-06    9.5e-06    1.1e-05    1.1e-05    5.2e-06    6.5e-06    1.1e-05
  clf_t            7.7e-06    1.6e-05    4.5e-05    3.2e-06    1.7e-05    4.1e-06    5.4e-06    1.2e-05    7.6e-06    4.8e-06    9.7e-06
  fe_s             3.2e-05    1.5e-05    1.4e-05    9.9e-06    8.1e-06    1.2e-05    1.1e-05    2.3e-05    9.4e-06    8.9e-06    2.6e-05
  dimunif          1.2e-05    1.3e-05    6.3e-06    8.8e-06    1.6e-05    4.6e-06    4.2e-06    8.3e-06    4.5e-06    9.8e-06    7.1e-06
  clf_s            2.8e-06    3.1e-06    2.1e-06    3.4e-06    3.0e-06    3.2e-06    1.0e-05    4.0e-06    1.8e-05    2.2e-06    2.5e-06
  probtransfer     7.0e-06    6.2e-06    1.2e-05    7.3e-06    6.6e-06    4.7e-06    8.3e-06    4.3e-06    2.1e-05    3.5e-06    4.7e-06
  nf               2.4e-05    1.3e-05    1.1e-05    5.4e-06    1.3e-05    8.1e-06    7.7e-06    1.2e-05    7.8e-06    7.6e-06    1.1e-05
  noise            2.3e-05    1.1e-05    8.4e-06    9.0e-06    7.0e-06    5.3e-06    4.7e-06    1.2e-05    4.9e-06    7.3e-06    7.9e-06
  ad_net           1.1e-05    1.1e-05    9.6e-06    7.5e-06    7.9e-06    9.7e-06    8.1e-06    8.9e-06    1.2e-05    1.0e-05    1.1e-05
  fd_s             7.7e-07    6.5e-07    7.8e-07    6.0e-07    5.5e-07    1.2e-06    9.4e-07    7.0e-07    7.3e-07    8.7e-07    8.6e-07
  cpc              9.3e-06    1.7e-05    6.8e-06    6.7e-06    8.2e-06    7.6e-06    1.3e-05    9.2e-06    8.3e-06    9.1e-06    1.3e-05

  exact-f32          32-24      36-44     100-28      30-22      31-27      33-25   33-25-k2      32-27      31-32 31-27-B3-4     520-36
  fe_t             1.1e-06    6.2e-07    3.2e-07    1.4e-06    5.5e-07    9.6e-07    9.7e-07    8.2e-07    7.3e-07    6.8e-07    5.4e-07
  clf_t            1.3e-07    2.0e-07    9.9e-07    1.5e-07    8.5e-07    6.1e-07    3.2e-07    5.4e-07    8.5e-07    2.0e-07    7.2e-07
  fe_s             5.8e-07    6.0e-07    5.0e-07    5.1e-07    4.5e-07    5.7e-07    7.0e-07    7.8e-07    4.5e-07    4.2e-07    6.2e-07
  dimunif          2.6e-07    5.1e-07    1.9e-07    5.0e-07    8.2e-07    4.6e-07    3.8e-07    1.8e-07    2.7e-07    7.5e-07    3.8e-07
  clf_s            1.4e-07    1.4e-07    1.2e-07    1.5e-07    2.8e-07    2.6e-07    3.9e-07    2.3e-07    7.5e-07    1.1e-07    6.8e-08
  probtransfer     1.3e-07    2.2e-07    3.5e-07    1.3e-07    1.7e-07    5.0e-08    2.1e-07    9.7e-08    6.9e-07    1.3e-07    1.4e-07
  nf               6.2e-07    4.6e-07    3.1e-07    4.3e-07    4.2e-07    3.4e-07    4.7e-07    3.5e-07    5.3e-07    5.1e-07    4.9e-07
  noise            4.1e-07    5.3e-07    3.7e-07    2.7e-07    3.9e-07    4.0e-07    2.6e-07    2.7e-07    3.4e-07    3.0e-07    3.0e-07
  ad_net           3.8e-07    5.3e-07    3.2e-07    4.3e-07    5.9e-07    5.1e-07    4.2e-07    2.6e-07    4.6e-07    7.1e-07    5.3e-07
  fd_s             2.6e-08    3.7e-08    3.8e-08    3.9e-08    2.5e-08    3.7e-08    2.1e-08    2.3e-08    2.6e-08    3.2e-08    3.6e-08
  cpc              7.3e-06    1.2e-05    4.8e-06    6.7e-06    8.2e-06    7.5e-06    3.3e-06    7.3e-06    8.3e-06    9.1e-06    8.3e-06

Every case is inside GRAD_TOL (2e-4 / 3e-5), the control included, so GRAD_TOL gates all of them.  cpc in the exact-f32 table: see
test_gpu_uneven_batches.py (the CPC forward's Gram product follows FST_MATH, not the fixture).  Off-grid cases worse than the
control in split-bf16 mode — clf_t at (100, 28), (36, 44), (31, 27); clf_s and probtransfer at (31, 32): the exact-f32 table
shows the same modules moving by the same factors (clf_t 1.3e-7 -> 9.9e-7 at (100, 28)), and (32, 27), which runs the control's
target-side routes, moves clf_t as well: it is the case's data (gradient scale and cancellation), not a route.  Phases, worst
module: split-bf16 6.0e-5 control, 5.4e-5 (36, 44), 3.4e-5 (31, 27); exact-f32 1.8e-5, 1.5e-5, 8.8e-6.  Imposed flips: at most one
unit per step, |x| / max|x| <= 3.6e-6.  The control passes against the fp64 oracle, so device and fp32
oracle share no error that the fp32 oracle hid.

Defect found by test d: at (C·L_t) % 32 != 0 RandomLayer left ``nt_gemm`` for the conv engine's K-split product, whose slices are
added with float atomics — two trainers in the same state reported cdan 2.7e-6 apart in the default arithmetic, where every other
step of this suite reproduces its bits.  RandomLayer now zero-pads the feature side to a multiple of 32 and stays on ``nt_gemm``.
``test_random_layer_at_a_width_off_the_gemm_stage`` holds the padded product itself to fp64 and to the same bits twice.
"""
import numpy as np
import pytest
import torch

import feature_level_style_transfer_for_tsc_amd as fst
from feature_level_style_transfer_for_tsc_amd import ops
from oracle import restatement as R
from test_gpu_full_step import (GRAD_TOL, LOSSES, _check_step, _head_unit_branches, _pair, _phase_both, _step_both,
                                arithmetic)                                        # noqa: F401  (arithmetic: a fixture)
from test_gpu_modules import close
from test_gpu_phase_graphs import clone, replay_vs_eager
from test_gpu_uneven_batches import PHASES, _check_phase, _same_noise_state

gpu = pytest.mark.gpu
DEV = "cuda"
TS = (3, 2)                                  # CPC start indices: below (L_t // 2) // 2 at every L_t >= 28
NCLS = (3, 4)
C_IN = (1, 2)
SEED, INPUT_SEED = 6, 1                      # initial state / series and labels
REJECTED = (("every case", 5, "fe_t's shortcut BatchNorm has a channel of batch variance 1.1e-5: conditioning, see above"),)

# id -> (L_t, L_s, B_t, B_s, k, expected route tuple)
T, F_ = True, False
CASES = {
    "control-32-24": (32, 24, 4, 4, 1, (T, T, T, T, T, 0)),
    "36-44": (36, 44, 4, 4, 1, (T, T, F_, F_, F_, 0)),
    "100-28": (100, 28, 4, 4, 1, (T, T, F_, F_, F_, 0)),
    "30-22": (30, 22, 4, 4, 1, (F_, F_, F_, F_, F_, 0)),
    "31-27": (31, 27, 4, 4, 1, (F_, F_, F_, F_, F_, 2)),
    "33-25": (33, 25, 4, 4, 1, (F_, F_, F_, F_, F_, 2)),
    "33-25-k2": (33, 25, 4, 4, 2, (F_, F_, F_, F_, F_, 0)),
    "32-27": (32, 27, 4, 4, 1, (T, T, T, T, T, 0)),
    "31-32": (31, 32, 4, 4, 1, (F_, F_, F_, F_, F_, 2)),
    "31-27-B3-4": (31, 27, 3, 4, 1, (F_, F_, F_, F_, F_, 2)),
    "520-36": (520, 36, 2, 2, 1, (T, F_, F_, F_, F_, 0)),
}
WN_N, WN_LAYERS = 16, 8


def _specs(C_in_t, C_in_s, k):
    fe_t = R.omni_scale_spec(1, 8, [18 * k * C_in_t, 10 * 18 * 3], C_in_t)
    fe_s = R.omni_scale_spec(1, 6, [11 * 2 * C_in_s, 8 * 11 * 3], C_in_s)
    return fe_t, R.respec_first_layer(fe_t, R.feature_width(fe_t)), fe_s


def _oracle32(L_t, C_in_t, L_s, C_in_s, ncls_t, ncls_s, seed, k):
    """The fp32 oracle of the narrow geometry at any pair of lengths, freshly initialised from ``seed``."""
    assert L_t >= 28 and L_s >= 20, "every length is at least 4 x the largest kernel of its side"
    gen = torch.Generator().manual_seed(seed)
    fe_t, clf, fe_s = _specs(C_in_t, C_in_s, k)
    C, C_s = R.feature_width(fe_t), R.feature_width(fe_s)
    assert (C, C_s) == (10 * k, 16)
    mods = {"fe_t": R.init_feature_extractor(fe_t, gen), "clf_t": R.init_classifier(clf, ncls_t, gen),
            "fe_s": R.init_feature_extractor(fe_s, gen), "clf_s": R.init_classifier(clf, ncls_s, gen),
            "nf": R.init_waveglow(3, C, WN_N, gen, zero_end=False), "cpc": R.init_cpc(C, 8, L_t // 2, gen)}
    mods.update(R.init_small_heads(C, C_s, L_t, L_s, gen))
    mats = [torch.randn(C * L_t, 1024, generator=gen), torch.randn(ncls_t, 1024, generator=gen)]
    return R.JointStep(mods, mats, fe_t, clf, fe_s, 3, L_t // 2, dropout_p=0.0)


def _trainer_of(js, L_t, C_in_t, L_s, C_in_s, ncls_t, ncls_s, **kw):
    cfg = fst.JointConfig(L_t=L_t, C_in_t=C_in_t, L_s=L_s, C_in_s=C_in_s, n_class_t=ncls_t, n_class_s=ncls_s, nf_channels=WN_N,
                          cpc_hidden=8, dropout_p=0.0)
    tr = fst.JointTrainer(cfg, DEV, fe_t_spec=js.fe_t_spec, clf_spec=js.clf_spec, fe_s_spec=js.fe_s_spec, **kw)
    tr.load_params({name: {n: t.detach().float() for n, t in P.items()} for name, P in js.m.items()}, [m.float() for m in js.mats])
    return tr


def _oracle_pair(L_t, C_in_t, L_s, C_in_s, ncls_t, ncls_s, seed, k, **kw):
    """(fp64 oracle ``R.JointStep``, ``JointTrainer``) holding the same state: the fp32 draws of ``seed``."""
    js = _oracle32(L_t, C_in_t, L_s, C_in_s, ncls_t, ncls_s, seed, k)
    return R.joint_step_as(js, torch.float64), _trainer_of(js, L_t, C_in_t, L_s, C_in_s, ncls_t, ncls_s, **kw)


def _case_pair(case, **kw):
    L_t, L_s, _, _, k, _ = CASES[case]
    return _oracle_pair(L_t, C_IN[0], L_s, C_IN[1], NCLS[0], NCLS[1], SEED, k, **kw)


def _case_trainer(case, **kw):
    L_t, L_s, _, _, k, _ = CASES[case]
    return _trainer_of(_oracle32(L_t, C_IN[0], L_s, C_IN[1], NCLS[0], NCLS[1], SEED, k), L_t, C_IN[0], L_s, C_IN[1], *NCLS, **kw)


def _batch(case, seed=INPUT_SEED):
    """((x_t, y_t), (x_s, y_s)) drawn as ``_pair`` does: per-row standardised series."""
    L_t, L_s, B_t, B_s, _, _ = CASES[case]
    gen = torch.Generator().manual_seed(seed)
    return _pair(gen, B_t, C_IN[0], L_t, NCLS[0]), _pair(gen, B_s, C_IN[1], L_s, NCLS[1])


def _on_device(batch):
    (x_t, y_t), (x_s, y_s) = batch
    return [x_t.to(DEV), y_t.to(DEV), x_s.to(DEV), y_s.to(DEV)]


def _routes(case):
    """The predicates the trainer's dispatch consults, at the shapes of ``case`` (every WN application runs at L_t)."""
    L_t, _, B_t, B_s, k, _ = CASES[case]
    C = 10 * k
    h, CL = C // 2, C * L_t
    assert TS[0] < (L_t // 2) // 2 and TS[1] < (L_t // 2) // 2
    return (ops.wn_fused_ok(WN_N, h, L_t), ops.wn_stack_bwd_ok(WN_N, h, L_t, WN_LAYERS),
            all(ops.wn_wgrad_ok(0, B, L_t, WN_N, h, 4) for B in (B_t, B_s)),
            all(ops.wn_wgrad_ok(1, B, L_t, WN_N, h, 2 ** i) for B in (B_t, B_s) for i in range(WN_LAYERS)),
            CL % 32 == 0, CL % 4)


def _assert_routes(case, math):
    """The case runs the routes it is there for — so that a later dispatch change cannot silently empty the test."""
    L_t, _, B_t, _, k, want = CASES[case]
    got = _routes(case)
    if math == "bf16x3":
        assert got == want, (case, got, want)
        if want[2]:                                              # the control: kind 0 at dilations 1, 2 needs readable slack
            h = 10 * k // 2
            assert not ops.wn_wgrad_ok(0, B_t, L_t, WN_N, h, 1)
            assert ops.wn_wgrad_ok(0, B_t, L_t, WN_N, h, 1, ops.empty_with_slack(B_t, WN_N, L_t, DEV))
    else:                                                        # exact-f32: no split-bf16 kernel serves anything
        assert (got[0], got[2], got[3]) == (False, False, False) and got[1] == want[1] and got[4:] == want[4:], (case, got, want)


# ------------------------------------------------------------------ 0. the inputs (CPU)
def _recorded_step(js, batch):
    (x_t, y_t), (x_s, y_s) = batch
    branches = []
    with _head_unit_branches(record=branches):
        js.step(x_t, y_t, x_s, y_s, epoch=0, t_samples=TS)
    return branches


def _module_errors(js32, js64):
    out = {}
    for name, P in js64.m.items():
        want = {n: p.grad for n, p in P.items() if p.requires_grad and p.grad is not None}
        scale = max(float(g.abs().max()) for g in want.values())
        out[name] = max(float((js32.m[name][n].grad.double() - g).abs().max()) for n, g in want.items()) / max(scale, 1e-30)
    return out


def _conditioning(case, seed=SEED, input_seed=INPUT_SEED, impose=True):
    L_t, L_s, _, _, k, _ = CASES[case]
    js32 = _oracle32(L_t, C_IN[0], L_s, C_IN[1], NCLS[0], NCLS[1], seed, k)
    js64 = R.joint_step_as(js32, torch.float64)
    batch = _batch(case, input_seed)
    branches = _recorded_step(js64, batch)
    (x_t, y_t), (x_s, y_s) = batch
    flips = []
    if impose:
        with _head_unit_branches(impose=branches, flips=flips):
            js32.step(x_t, y_t, x_s, y_s, epoch=0, t_samples=TS)
    else:
        js32.step(x_t, y_t, x_s, y_s, epoch=0, t_samples=TS)
    return _module_errors(js32, js64), flips


@pytest.mark.parametrize("case", list(CASES))
def test_inputs_are_well_conditioned_for_fp32_torch(case):
    """The fp32 oracle on the fp64 oracle's ReLU branches (imposed and bounded as the device run's are) is within a third of the
    exact-f32 gate of the fp64 oracle, in every module: what the device is held to, plain fp32 torch meets three times over."""
    errs, flips = _conditioning(case)
    print(f"[conditioning] {case}: flips {flips} " + " ".join(f"{n}={e:.1e}" for n, e in errs.items()))
    bound = GRAD_TOL["f32"]["default"] / 3
    for name, e in errs.items():
        assert e <= bound, f"{case}: fp32 torch is {e:.2e} off the fp64 oracle in {name} (bound {bound:.1e})"


# ------------------------------------------------------------------ a. the joint step, every gradient
@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_joint_step_vs_fp64_oracle(case, arithmetic):
    """One joint step against the fp64 oracle from identical state: nine losses, three logit tensors, feat_s2t, GradNorm norms and
    weights, every module's accumulated gradient, NoiseTransfer's counters and running sums."""
    _assert_routes(case, arithmetic)
    js, tr = _case_pair(case)
    what = f"{case} {arithmetic}"
    rep_o, want, rep, grads = _step_both(js, tr, _batch(case), TS)
    assert all(np.isfinite(float(rep_o[k])) for k in LOSSES), (what, {k: float(rep_o[k]) for k in LOSSES})
    _same_noise_state(tr, js, what, sums=True)
    _check_step(rep_o, want, rep, grads, tr, what, math=arithmetic)


# ------------------------------------------------------------------ b. the six pre-training phases
@gpu
@pytest.mark.parametrize("phase", PHASES)
@pytest.mark.parametrize("case", ["31-27", "36-44", "control-32-24"])
def test_phase_step_vs_fp64_oracle(case, phase, arithmetic):
    """``phase_step`` against the fp64 oracle's, a fresh oracle per phase: ``total`` and every reported loss, which modules received
    gradients (exactly), and their values — the gates test_gpu_uneven_batches.py holds the phases to."""
    js, tr = _case_pair(case)
    what = f"{phase} {case} {arithmetic}"
    _check_phase(*_phase_both(js, tr, phase, _batch(case), TS), tr, what, arithmetic)


# ------------------------------------------------------------------ c. graph capture
STATE_KEYS = ("m.fe_t.net_1.net.net.1.conv1d.weight", "m.nf.WN.0.in_layers.3.weight_v", "m.nf.WN.2.res_skip_layers.7.weight_g",
              "m.clf_t.hidden.weight", "m.cpc.Wk.0.weight", "w_s")


@gpu
@pytest.mark.parametrize("case", ["31-27", "36-44"])
def test_captured_joint_step_equals_eager(case):
    """``capture`` + ``replay`` against ``step`` from the same snapshot (the recipe and gates of
    test_full_batch_graph_replay_equals_eager_step), then a second replay — other ``advance`` ratios, B / N_seen — which must move
    NoiseTransfer's running sums exactly as the second eager step does.  At (31, 27) the capture holds NoiseTransfer's composition."""
    _assert_routes(case, ops.MATH)
    tr = _case_trainer(case)
    args, args2 = _on_device(_batch(case)), _on_device(_batch(case, seed=INPUT_SEED + 98))
    torch.manual_seed(5)
    tr.capture(*args, epoch=0)
    snap = tr.snapshot()
    rep = clone(tr.replay(*args, TS))
    after_graph = tr.snapshot()
    rep2 = clone(tr.replay(*args2, (1, 4)))
    sums_graph = (tr.m["noise"].target_avg.clone(), tr.m["noise"].source_avg.clone())
    host_graph = tr.snapshot()["host"]
    tr.restore(snap)
    eager = tr.step(*args, epoch=0, t_samples=TS)
    after_eager = tr.snapshot()
    for k in LOSSES:
        a, b = float(rep[k]), float(eager[k])
        assert abs(a - b) <= 1e-6 * max(1.0, abs(b)), (k, a, b)
    for k in ("logit_t", "logit_s", "logit_s2t", "feat_t", "feat_s2t", "w_t", "w_s", "norms_t", "norms_s"):
        close(rep[k], eager[k], 1e-5, f"graph vs eager {k}")
    assert after_graph["host"] == after_eager["host"]
    for k in ("noise.target_avg", "noise.source_avg"):
        assert torch.equal(after_graph["t"][k], after_eager["t"][k]), f"first replay: {k} differs from the eager step's"
    for k in STATE_KEYS:
        d = (after_graph["t"][k] - after_eager["t"][k]).abs()
        scale = float(after_eager["t"][k].abs().max())
        assert float((d > 2e-3 * scale).double().mean()) < 0.01, (k, float(d.max()), scale)
    # the second call: ratios (B_t / N_t, B_s / N_s) instead of (1, 1).  From the FIRST REPLAY's state, so that both second steps
    # start from the same bits
    tr.restore(after_graph)
    before = (tr.m["noise"].target_avg.clone(), tr.m["noise"].source_avg.clone())
    eager2 = tr.step(*args2, epoch=0, t_samples=(1, 4))
    assert tr.snapshot()["host"] == host_graph
    for name, g, e, b in zip(("target_avg", "source_avg"), sums_graph, (tr.m["noise"].target_avg, tr.m["noise"].source_avg), before):
        assert not torch.equal(e, b), f"the second eager step left {name} where it was"
        assert torch.equal(g, e), f"second replay: {name} is {float((g - e).abs().max()):.3e} off the eager step's"
    for k in ("nf_t", "nf_s", "ce_s2t2s"):
        a, b = float(rep2[k]), float(eager2[k])
        assert abs(a - b) <= 1e-6 * max(1.0, abs(b)), ("second replay", k, a, b)
    close(rep2["feat_s2t"], eager2["feat_s2t"], 1e-5, "second replay feat_s2t")


@gpu
@pytest.mark.parametrize("phase", ["nf", "target_pretrain"])
@pytest.mark.parametrize("case", ["31-27", "36-44"])
def test_captured_phase_equals_eager(case, phase):
    """``capture_phase`` + one replay against the eager ``phase_step`` from the same snapshot (the gates of
    test_phase_replay_equals_eager_step): the flow phase and a classifier phase."""
    tr = _case_trainer(case)
    args = _on_device(_batch(case))
    tr.capture_phase(phase, *args)
    replay_vs_eager(tr, phase, args, TS, f"{phase} {case}")


# ------------------------------------------------------------------ d. the anomaly guard over NoiseTransfer's composition
@gpu
def test_a_nan_batch_leaves_no_trace_with_the_composed_noise_transfer():
    """(31, 27): NoiseTransfer's composition — not the kernels the guard's list of forward-written buffers was written for —
    updates the running sums.  A step on a batch holding a NaN leaves every state tensor bit-identical, the sums included; the
    clean step after it is the step of a twin that never saw the bad batch."""
    from test_gpu_anomaly_guard import NAN, counts_of, follow_host_counters, poisoned, same_step, unchanged
    case = "31-27"
    _assert_routes(case, ops.MATH)
    tr, twin = _case_trainer(case, anomaly_guard=True), _case_trainer(case)
    args, args_b = _on_device(_batch(case)), _on_device(_batch(case, seed=INPUT_SEED + 98))
    # a clean first step: the sums are non-zero when the bad batch arrives
    ra, rb = tr.step(*args, epoch=0, t_samples=TS), twin.step(*args, epoch=0, t_samples=TS)
    same_step(ra, rb, tr.snapshot()["t"], twin.snapshot()["t"], "clean first step")
    before = tr.snapshot()
    assert bool(before["t"]["noise.target_avg"].any()) and bool(before["t"]["noise.source_avg"].any())
    rep = tr.step(*poisoned(args_b, 0, NAN), epoch=0, t_samples=TS)
    assert int(rep["skipped"]) == 1 and counts_of(rep)["fe_t"] > 0 and counts_of(rep)["buffers"] > 0
    after = tr.snapshot()["t"]
    for k in ("noise.target_avg", "noise.source_avg"):
        assert torch.equal(after[k], before["t"][k]), f"the skipped step moved {k}"
    unchanged(before["t"], after, "bad step")
    follow_host_counters(twin, tr, args_b)
    ra, rb = tr.step(*args_b, epoch=0, t_samples=TS), twin.step(*args_b, epoch=0, t_samples=TS)
    assert int(ra["skipped"]) == 0
    same_step(ra, rb, tr.snapshot()["t"], twin.snapshot()["t"], "clean step after a skipped step")


@gpu
@pytest.mark.parametrize("D", [310, 330, 5200, 320])
def test_random_layer_at_a_width_off_the_gemm_stage(D, monkeypatch):
    """RandomLayer at C·L_t = 310, 330, 5200 (no multiple of 32) and 320: value and input gradients against fp64 at 2e-5 (the gate
    test_gpu_kernels.py holds ``nt_gemm`` to), and the same bits twice — the product stays on ``nt_gemm``, on zero-padded operands;
    at a multiple of 32 the operand is the transposed matrix itself, as before."""
    monkeypatch.setattr(ops, "MATH", "bf16x3")
    torch.manual_seed(D)
    rl = fst.RandomLayer([D, 3], 1024).to(DEV)
    assert (rl._rt_k32(0) is rl._rt(0)) == (D % 32 == 0) and rl._rt_k32(0).shape == (1024, -(-D // 32) * 32)
    x0, p0, cot = torch.randn(4, D, device=DEV), torch.softmax(torch.randn(4, 3, device=DEV), 1), torch.randn(4, 1024, device=DEV)

    def run():
        x, p = x0.clone().requires_grad_(True), p0.clone().requires_grad_(True)
        out = rl([x, p])
        return (out.detach(),) + torch.autograd.grad(out, (x, p), cot)
    got, again = run(), run()
    assert ops.wn_last_route()[0] == ops.WN_ROUTE_WGRAD, "the forward product did not run on the time-as-k kernel"
    x, p = x0.double().requires_grad_(True), p0.double().requires_grad_(True)
    R0, R1 = (m.double() for m in rl.random_matrix)
    want = (x @ R0) / 32.0 * (p @ R1)
    for g, w, a, name in zip(got, (want.detach(),) + torch.autograd.grad(want, (x, p), cot.double()), again, ("out", "dx", "dp")):
        assert g.shape == w.shape
        close(g, w, 2e-5, f"RandomLayer D={D} {name}")
        assert torch.equal(g, a), f"RandomLayer D={D}: {name} differs between two runs"


# ------------------------------------------------------------------ e. eval / inference
@gpu
@pytest.mark.parametrize("case", ["31-27", "30-22"])
def test_inference_vs_fp64_oracle(case):
    """Modules in ``eval()`` under ``torch.no_grad()``: ``fe_t`` then ``clf_t`` with BatchNorm folded into the convs against the
    oracle's eval forward, and ``WaveGlow.infer`` (the forward kernels that store no gate halves fall back layer by layer here)
    against ``R.waveglow_infer``; 1e-4 each."""
    _assert_routes(case, ops.MATH)
    L_t, L_s, B, _, k, _ = CASES[case]
    js32 = _oracle32(L_t, C_IN[0], L_s, C_IN[1], NCLS[0], NCLS[1], SEED, k)
    gen = torch.Generator().manual_seed(INPUT_SEED)
    for name in ("fe_t", "clf_t"):                                           # non-trivial running statistics
        for key, v in js32.m[name].items():
            if key.endswith("running_mean"):
                v.copy_(torch.randn(v.shape, generator=gen) * 0.3)
            if key.endswith("running_var"):
                v.copy_(torch.rand(v.shape, generator=gen) + 0.5)
    js = R.joint_step_as(js32, torch.float64)
    tr = _trainer_of(js32, L_t, C_IN[0], L_s, C_IN[1], *NCLS)
    x, _ = _pair(gen, B + 1, C_IN[0], L_t, NCLS[0])
    z = torch.randn(B + 1, 10 * k, L_t, generator=gen)
    fe, clf, nf = tr.m["fe_t"].eval(), tr.m["clf_t"].eval(), tr.m["nf"].eval()
    with torch.no_grad():
        feat = fe(x.to(DEV))
        logits, pooled = clf(feat)
        back = nf.infer(z.to(DEV))
        feat_o = R.feature_extractor(x.double(), js.m["fe_t"], js.fe_t_spec, False)
        logits_o, pooled_o = R.classifier(feat_o, js.m["clf_t"], js.clf_spec, False)
        back_o = R.waveglow_infer(z.double(), js.m["nf"], 3, {})
    close(feat, feat_o, 1e-4, f"{case} folded eval features")
    close(logits, logits_o, 1e-4, f"{case} folded eval logits")
    close(pooled, pooled_o, 1e-4, f"{case} folded eval pooled")
    close(back, back_o, 1e-4, f"{case} WaveGlow.infer")
