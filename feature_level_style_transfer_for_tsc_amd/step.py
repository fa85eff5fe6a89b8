"""Train steps behind the reference's outer loop (train_and_test.py), built from the drop-in modules.

* ``ClassifierTrainer`` — S1: FE → CLF → CE → backward → RMSprop×2 (train_and_test.py:148-171, no CPC term).
* ``JointTrainer``      — S2: one batch of the joint phase incl. GradNorm (train_and_test.py:539-766).

Differences from the reference are mechanical, not numerical:
  - the double ``loss_total.backward()`` (quirk Q3) is reproduced by ONE backward of
    Σ wᵢ·Lᵢ + 2·(a·cdan + b·fd_s + c·sl_t + d·sl_s) — same accumulated gradients, half the work;
  - GradNorm's numpy round-trip (:694-711) stays on the device (same fp32 formulas, no host sync);
  - per-batch ``.cpu()`` prints and feature dumps (:564-644) are not part of the step;
  - during GradNorm's five partial backward passes only the shared OS_block needs weight gradients, so
    every other conv skips its weight-gradient kernels (``ops.partial_backward``).
Data parallelism: ``dist.GradBucket`` all-reduces one flat fp32 gradient bucket over RCCL.

Schedules (schedules.py): ``JointTrainer.make_schedulers`` builds the reference's eleven learning-rate schedulers on the trainer's
optimisers and ``end_epoch`` steps the ones the reference steps.  A captured step follows them only after
``enable_device_hparams()``, which moves the learning rates and the four epoch coefficients into device tensors.

Anomaly guard (``JointTrainer.enable_anomaly_guard()``): instead of the reference's ``torch.autograd.set_detect_anomaly(True)``
(train_and_test.py:24), which cannot run under capture, a step whose update would consume a NaN or an inf is made a no-op on the
trainer's state, decided on the device, in eager and in replayed steps alike.

Gradient norms and clipping (``JointTrainer.enable_grad_clip()``): per-module L2 norms of the gradients the optimisers are about
to read in every report, and caps per module and on the whole that scale those gradients in place — what
``torch.nn.utils.clip_grad_norm_`` does with a host decision — computed and applied on the device, under graph replay too.

Transfer monitor (``JointTrainer.enable_transfer_monitor()``, monitor.py): in place of the feature dumps for t-SNE plots (:564-621,
:792-797), the multi-kernel MMD² between the target, source-to-target and source feature sets and between the source, t2s and
s2t2s hidden vectors in every report, computed on the device, under graph replay too; ``aux`` still hands out the raw tensors.

Weight averaging, gradient accumulation and device-resident input, which both trainers offer, are the mixins of modes.py.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _capture, ops
from .cdan import CDAN, RandomLayer
from .cpc import CPC
from . import dist as _dist
from .dist import GradBucket
from .modes import _enable_from_arg, _Fed, _GradAccumulating, _WeightAveraging, _WindowOpens
from .monitor import _TransferMonitoring
from .optim import (MAX_GROUPS, _capturing, AnomalyGuard, FusedRMSprop, GradClip, SharedStepAdam, accumulate, count_nonfinite, guard_copy,
                    push_lr, push_words, rmsprop_step_many, scale_by_group, sumsq_norms)
from .os_cnn import OS_CNN, OS_CNN_res, build_layer_with_layer_parameter
from .schedules import (EPOCH_SCHEDULERS, PLATEAU, PLATEAU_METRIC, STEP_LR, loss_coefficients, make_schedulers,  # noqa: F401 (re-exported)
                        step_schedulers)
from .structure import generate_layer_parameter_list, layer_parameter_list_input_change, out_channels
from .waveglow import WaveGlow, WaveGlowLoss
from .widgets import (AdversarialNetworkforCDAN, DimensionUnification, FeatureDiscriminatorforSource, NoiseTransfer,
                      ProbTransfer, wgan_loss)

MAX_KERNEL_SIZE = 89                                                          # train_and_test.py:40
_KEEP = object()                                                              # set_grad_clip: "leave this limit as it is"


def specs_for(length: int, in_channel: int):
    """(feature-extractor spec, classifier spec) exactly as train_and_test.py:38-53 derives them."""
    budgets = [8 * 128 * in_channel, 5 * 128 * 256 + 2 * 256 * 128]
    rf = min(int(length / 4), MAX_KERNEL_SIZE)
    fe = generate_layer_parameter_list(1, rf, budgets, in_channel)
    return fe, layer_parameter_list_input_change(fe, out_channels(fe[-1]))


class ClassifierTrainer(_WeightAveraging, _GradAccumulating, _Fed):
    """S1 of the reference.  The anomaly guard (``JointTrainer.enable_anomaly_guard``) is not offered here: a non-finite batch
    reaches this trainer's parameters as it does in the reference.  Weight averaging (``enable_weight_average``) is, over the
    groups "fe" and "clf"; its device words are ``weight_average``.  Gradient accumulation (``enable_grad_accumulation``) too."""

    def __init__(self, length: int, in_channel: int, n_class: int, device, bucket: Optional[GradBucket] = None,
                 sync: str = "ddp", device_hparams: bool = False, weight_average=None, grad_accumulation=None):
        """``weight_average``: ``enable_weight_average()`` at once — True, a decay, or a dict of its keyword arguments.
        ``grad_accumulation``: ``enable_grad_accumulation()`` at once, with that many steps."""
        self.sync, self.device = sync, device
        fe_spec, clf_spec = specs_for(length, in_channel)
        self.fe = OS_CNN_res(fe_spec).to(device)
        self.clf = OS_CNN(clf_spec, n_class).to(device)
        # capturable: the optimisers' step counters live on the device, so the step can be captured into a hipGraph
        self.opt_fe = FusedRMSprop(self.fe.parameters(), lr=0.001)
        self.opt_clf = FusedRMSprop(self.clf.parameters(), lr=0.003)
        self.bucket = bucket
        self.fe.train(); self.clf.train()
        self._graph = None
        self._graph_update = None                                             # gradient accumulation: the update's own graph
        self.device_hparams = False
        if device_hparams:
            self.enable_device_hparams()
        _enable_from_arg(self.enable_weight_average, weight_average, "decay")
        _enable_from_arg(self.enable_grad_accumulation, grad_accumulation, "steps")

    def _ema_modules(self) -> Dict[str, nn.Module]:
        return {"fe": self.fe, "clf": self.clf}

    def _capture_resident(self) -> bool:
        return self._graph is not None

    def enable_device_hparams(self) -> None:
        """Keep both learning rates in device tensors (``optim.push_lr``): ``replay`` then trains at the current ``group["lr"]`` of
        ``opt_fe`` / ``opt_clf`` — what a ``torch.optim.lr_scheduler`` on them has set — instead of the rates of capture day.
        Idempotent; before ``capture`` only (a resident graph holds the launches that take the rates by value)."""
        if self.device_hparams:
            return
        self._refuse_resident("enable_device_hparams()")
        self.opt_fe.enable_lr_on_device(); self.opt_clf.enable_lr_on_device()
        self.device_hparams = True

    def parameters(self) -> List[nn.Parameter]:
        return list(self.fe.parameters()) + list(self.clf.parameters())

    def step(self, x: torch.Tensor, y: torch.Tensor):
        """One batch; with gradient accumulation one micro-batch, whose call updates only if it closes its window.  Returns
        (loss, logits) of this call's batch."""
        self._ema_no_step("step()")
        closing = self._closing
        loss, logits = self._fwd_bwd(x, y)
        if self.grad_accumulation is not None:
            self._accum_fold(self.parameters(), advance=True)
        if closing:
            self._update()
        return loss.detach(), logits.detach()

    def _fwd_bwd(self, x: torch.Tensor, y: torch.Tensor):
        """First half of a step: forward and backward.  With gradient accumulation the gradients of the call before are dropped
        here, not behind the update: they stay alive for the update of a captured window, which is a graph of its own."""
        if self.grad_accumulation is not None:
            self.opt_fe.zero_grad(set_to_none=True); self.opt_clf.zero_grad(set_to_none=True)
        with _dist.global_batch(self.bucket if self.sync == "global" else None):
            with ops.pack_cache():
                logits, _ = self.clf(self.fe(x))
                loss = F.cross_entropy(logits, y)
                loss.backward()
        return loss, logits

    def _update(self) -> None:
        """Second half: the gradient all-reduce, both optimisers, then the weight average."""
        if self.bucket is not None:
            self.bucket.all_reduce(self.parameters())
        rmsprop_step_many([self.opt_fe, self.opt_clf])
        if self.grad_accumulation is None:
            self.opt_fe.zero_grad(set_to_none=True); self.opt_clf.zero_grad(set_to_none=True)
        self._ema_update(("fe", "clf"))

    # ---- single GPU: the whole step as one hipGraph (the eager step is launch-bound: ~300 launches for ~2 ms of GPU work)
    def capture(self, x: torch.Tensor, y: torch.Tensor, warmup: int = 3):
        """Capture one step.  The learning rates are baked into the graph unless ``enable_device_hparams()`` ran before.  With
        gradient accumulation two graphs sharing a pool, the micro-step (forward, backward, fold) and the update, and a warm-up
        of whole windows, so that the capture starts with the window closed."""
        self._ema_no_step("capture()")
        if self.bucket is not None:
            raise RuntimeError("ClassifierTrainer.capture(): single-GPU only (the DP step has an eager all-reduce)")
        self._accum_closed("capture()")
        acc = self.grad_accumulation
        if acc is not None:
            warmup = -(-warmup // acc.steps_host) * acc.steps_host
        self._g_x, self._g_y = x.clone(), y.clone()
        with _capture.warmup_stream(self.device):
            for _ in range(warmup):
                self.step(self._g_x, self._g_y)
        self._graph = torch.cuda.CUDAGraph()
        self._graph_update = None
        if acc is None:
            with _capture.graph(self._graph):
                self._g_out = self.step(self._g_x, self._g_y)
            return
        with _capture.graph(self._graph):
            loss, logits = self._fwd_bwd(self._g_x, self._g_y)
            self._accum_fold(self.parameters(), advance=True)
            self._g_out = (loss.detach(), logits.detach())
        self._graph_update = torch.cuda.CUDAGraph()
        with _capture.graph(self._graph_update, self._graph.pool()):
            self._update()

    def replay(self, x: torch.Tensor, y: torch.Tensor):
        """One captured step on a new batch of the captured shape; returns (loss, logits) in static buffers.  With
        ``device_hparams`` it runs at the optimisers' current ``group["lr"]``, otherwise at the captured rates.  With gradient
        accumulation the micro-step graph, and the update graph behind it on the call that closes a window."""
        self._ema_no_step("replay()")
        if self._graph is None:
            raise RuntimeError("call capture() first")
        self._g_x.copy_(x); self._g_y.copy_(y)
        return self._replay_graphs()

    def _replay_graphs(self):
        """What a replay does once the static inputs hold the batch."""
        if self.device_hparams:
            push_lr((self.opt_fe, self.opt_clf))
        self._graph.replay()
        if self._graph_update is not None:
            closing = self._closing
            self.grad_accumulation.advance_host()
            if closing:
                self._graph_update.replay()
        return self._g_out

    # ---- device-resident input (the methods of _Fed): a target-only EpochFeeder
    def begin_epoch(self) -> int:
        """Plan and upload the attached feeder's next epoch; returns its number of rounds."""
        if self.feeder is not None and len(self.feeder.sets) != 1:
            raise ValueError("ClassifierTrainer.begin_epoch(): a target-only feeder (source=None) is needed")
        return self._fed_begin("classifier")

    def step_fed(self):
        """``step`` on the feeder's current round, drawn into buffers this trainer keeps.  ``StopIteration`` once the epoch is over."""
        self._ema_no_step("step_fed()")
        self._fed_check("classifier", "step_fed()")
        return self.step(*self._fed_eager()["batch"])

    def replay_fed(self):
        """``replay`` on the feeder's current round, drawn straight into the capture's static inputs."""
        self._ema_no_step("replay_fed()")
        if self._graph is None:
            raise RuntimeError("call capture() first")
        self._fed_check("classifier", "replay_fed()")
        self.feeder.feed(self._g_x, self._g_y)
        return self._replay_graphs()

    def make_evaluator(self, data, batch_size: int, **kw):
        """An ``evaluate.Evaluator`` of (``fe``, ``clf``) over the resident ``data``; ``kw`` are its other arguments."""
        from .evaluate import Evaluator
        return Evaluator(self.fe, self.clf, data, batch_size, **kw)


@dataclass
class JointConfig:
    L_t: int = 512
    C_in_t: int = 1
    L_s: int = 512
    C_in_s: int = 1
    n_class_t: int = 4
    n_class_s: int = 4
    nf_flows: int = 3                                                         # WaveGlow(3, C, 120) :71
    nf_channels: int = 120
    cpc_hidden: int = 64                                                      # CPC(C, 64, L//2) :131
    cdan_dim: int = 1024                                                      # :75-77
    ad_hidden: int = 1024
    dropout_p: float = 0.2
    nf_end_std: float = 0.0       # >0: draw WN.end (zero-init in the reference) so the flow is non-degenerate


class JointTrainer(_WeightAveraging, _GradAccumulating, _Fed, _TransferMonitoring):
    MODULES = ("fe_t", "clf_t", "fe_s", "dimunif", "clf_s", "probtransfer", "nf", "noise", "ad_net", "fd_s", "cpc")
    LRS = {"fe_t": 0.001, "clf_t": 0.003, "fe_s": 0.001, "dimunif": 0.001, "clf_s": 0.003, "probtransfer": 0.001,
           "nf": 0.001, "noise": 0.005, "ad_net": 0.001, "fd_s": 0.001}       # train_and_test.py:97-106
    # groups of the anomaly guard's counts: a module's gradients; "gradnorm" = the ten GradNorm scalars and the two weight
    # gradients; "losses" = the step's loss scalars (per rank under data parallelism: reported, never part of the verdict);
    # "buffers" = the BatchNorm running statistics and NoiseTransfer sums the forward pass wrote (decide without a GradBucket only)
    ANOMALY_GROUPS = MODULES + ("gradnorm", "losses", "buffers")
    TRANSFER_AUX = ("feat_s", "pool_s", "tr_t", "tr_s2t")                       # aux entries that reach a report with the transfer monitor on only

    def __init__(self, cfg: JointConfig, device, bucket: Optional[GradBucket] = None, fe_t_spec=None, clf_spec=None,
                 fe_s_spec=None, sync: str = "ddp", device_hparams: bool = False, anomaly_guard: bool = False, grad_clip=None,
                 weight_average=None, grad_accumulation=None, transfer_monitor=None):
        """``sync`` (with a bucket): "ddp" = per-rank batch statistics (SURVEY §8e mode A); "global" = every
        batch-coupled quantity over the samples of all ranks (mode B, eager only) — N ranks reproduce the
        single-process step on the concatenated batch.  ``device_hparams``: ``enable_device_hparams()`` at once;
        ``anomaly_guard``: ``enable_anomaly_guard()`` at once.  ``grad_clip``: ``enable_grad_clip()`` at once — True for norms
        only, a number for ``max_norm``, or a dict of its keyword arguments.  ``weight_average``: ``enable_weight_average()`` at
        once — True, a decay, or a dict of its keyword arguments.  ``grad_accumulation``: ``enable_grad_accumulation()`` at once,
        with that many steps.  ``transfer_monitor``: ``enable_transfer_monitor()`` at once — True, a number of kernels, or a dict of
        its keyword arguments."""
        if sync not in ("ddp", "global"):
            raise ValueError(f"sync must be 'ddp' or 'global', got {sync!r}")
        self.cfg, self.device, self.bucket, self.sync = cfg, device, bucket, sync
        if fe_t_spec is None:
            fe_t_spec, clf_spec = specs_for(cfg.L_t, cfg.C_in_t)
            fe_s_spec, _ = specs_for(cfg.L_s, cfg.C_in_s)
        C, C_s = out_channels(fe_t_spec[-1]), out_channels(fe_s_spec[-1])
        m: Dict[str, nn.Module] = {}
        m["fe_t"] = OS_CNN_res(fe_t_spec)
        m["clf_t"] = OS_CNN(clf_spec, cfg.n_class_t)
        m["fe_s"] = OS_CNN_res(fe_s_spec)
        m["dimunif"] = DimensionUnification(C_s, C, cfg.L_s, cfg.L_t)
        m["clf_s"] = OS_CNN(clf_spec, cfg.n_class_s)
        m["probtransfer"] = ProbTransfer(m["clf_s"].length_before_classification)
        m["nf"] = WaveGlow(cfg.nf_flows, C, cfg.nf_channels)
        if cfg.nf_end_std > 0:
            for wn in m["nf"].WN:
                wn.end.weight.data.normal_(0, cfg.nf_end_std)
                wn.end.bias.data.normal_(0, cfg.nf_end_std)
        m["noise"] = NoiseTransfer(C, cfg.L_t)
        self.random_layer = RandomLayer([C * cfg.L_t, cfg.n_class_t], cfg.cdan_dim)
        m["ad_net"] = AdversarialNetworkforCDAN(cfg.cdan_dim, cfg.ad_hidden)
        m["ad_net"].dropout1.p = m["ad_net"].dropout2.p = cfg.dropout_p
        m["fd_s"] = FeatureDiscriminatorforSource(m["clf_s"].length_before_classification)
        m["cpc"] = CPC(C, cfg.cpc_hidden, cfg.L_t // 2)
        self.m = {k: v.to(device) for k, v in m.items()}
        self.random_layer = self.random_layer.to(device)
        self.nf_loss = WaveGlowLoss()
        # ten RMSprops (one learning rate per module) stepped by the same single-pass multi-tensor launches (optim.FusedRMSprop)
        self.opts = {k: FusedRMSprop(self.m[k].parameters(), lr=lr) for k, lr in self.LRS.items()}
        # CPC = 516 small tensors: torch's capturable Adam spends ~4 k tiny kernels per step on per-parameter step
        # counters; same update with one shared device counter (optim.SharedStepAdam)
        self.opt_cpc = SharedStepAdam(self.m["cpc"].parameters(), lr=0.002)
        self.w_t = nn.Parameter(torch.tensor([2.0, 5.0], device=device))         # :501-505
        self.w_s = nn.Parameter(torch.tensor([2.0, 2.0, 4.0], device=device))
        self.opt_w_t = torch.optim.Adam([self.w_t], lr=0.0002, capturable=True)
        self.opt_w_s = torch.optim.Adam([self.w_s], lr=0.001, capturable=True)
        self.init_t = self.init_s = None
        self.alpha = 3
        self.on_grads_ready = None                                            # test hook: called before the optimisers step
        self._side = torch.cuda.Stream(device=device)                         # launch-bound side chains (CPC)
        self._phase: Dict[str, dict] = {}                                     # captured pre-training phases (capture_phase)
        self._phase_pool = None                                               # their shared graph memory pool
        self._graphs = None                                                   # the captured joint step (capture)
        self.device_hparams = False
        self._coef = None                                                     # device_hparams: (cdan, fd_s, sl_t, sl_s) on the device
        self._coef_host = None                                                # ... and the values it holds
        self.schedulers = None                                                # make_schedulers()
        self._sched_epoch = None                                              # epoch of the coefficients last applied
        self.anomaly_guard = False
        self._guard: Optional[AnomalyGuard] = None                            # anomaly_guard: the verdict words on the device
        self._shadow: Dict[str, torch.Tensor] = {}                            # ... copies of the state rolled back after a bad step
        self._guard_live = None                                               # ... (live, shadow) lists of the step's save
        self._guard_fwd = ()                                                  # ... fp32 buffers the forward writes, of that save
        self._guard_losses = ()                                               # ... loss scalars of a phase step, for the counts
        self._accum_scalars = None                                            # gradient accumulation: accumulators of the 10 GradNorm scalars and the 9 losses
        self.grad_clip = False
        self._clip: Optional[GradClip] = None                                 # grad_clip: limits, norms and factors on the device
        self._clip_max: Optional[float] = None                                # ... the cap on the norm over all modules (None: none)
        self._clip_per: Dict[str, float] = {}                                 # ... the caps per module
        self._clip_masks: Dict[Tuple[str, ...], torch.Tensor] = {}            # ... which report entries a step's modules fill
        for mod in self.m.values():
            mod.train()
        # GradNorm differentiates the shared OS_blocks only: their convs keep weight gradients in partial passes
        for key in ("fe_t", "fe_s"):
            for layer in self.m[key].return_last_layer().layer_list:
                layer.spec.always_weight_grad = True
        if device_hparams:
            self.enable_device_hparams()
        if anomaly_guard:
            self.enable_anomaly_guard()
        _enable_from_arg(self.enable_grad_clip, grad_clip, "max_norm")
        _enable_from_arg(self.enable_weight_average, weight_average, "decay")
        _enable_from_arg(self.enable_grad_accumulation, grad_accumulation, "steps")
        _enable_from_arg(self.enable_transfer_monitor, transfer_monitor, "kernels")

    # ------------------------------------------------------------------ weight averaging (the methods are _WeightAveraging's)
    def _ema_modules(self) -> Dict[str, nn.Module]:
        return {k: self.m[k] for k in self.MODULES}

    def _capture_resident(self) -> bool:
        return self._graphs is not None or bool(self._phase)

    def _ema_caches(self) -> list:
        return list(self.m["nf"].convinv)                                     # Invertible1x1Conv.W_inverse (Q2)

    # ------------------------------------------------------------------ anomaly guard: skip non-finite steps on the device
    def enable_anomaly_guard(self) -> None:
        """From now on a step whose update would consume a non-finite value is a NO-OP on the trainer's state: after it every
        tensor of ``_state_tensors()`` holds the bits it held before.  Decided on the device with no host synchronisation, in
        ``step``, ``capture`` / ``replay``, ``phase_step`` and ``capture_phase`` / ``replay_phase``; a clean step computes the bits
        of the unguarded step.

        The verdict covers exactly what the update consumes: every ``.grad`` the step's optimisers read (after the data-parallel
        all-reduce), and in the joint step the ten GradNorm scalars (after ``mean_scalars``) and the two GradNorm weight
        gradients — all identical on every rank, so every rank decides alike.  Without a ``GradBucket`` the BatchNorm running
        statistics and NoiseTransfer's sums as the forward pass left them decide as well, counted as the group "buffers" — a
        second line: the fused ReLUs propagate NaN as torch's do, so a bad input reaches the gradients of whatever consumes the
        features (in the "nf" phase, whose features are detached, the flow's).  With a bucket those per-rank buffers stay out of
        the verdict (a rank deciding alone would part from the others).  The verdict is taken after ``on_grads_ready`` and before the
        first optimiser.  Parameters and RMSprop / Adam moments are guarded where they are written (``fst_*_multi_guard``, CPC's
        shared counter advances by ``ok``); what the forward pass and the tail of the update mutate in place (BatchNorm buffers,
        NoiseTransfer's sums, the omni-scale conv weights whose masked taps every forward zeroes again (Q1), the GradNorm weights
        with their Adams, the WGAN-clamped ``ad_net`` / ``fd_s`` parameters) is saved
        into shadow buffers at the start of the step and rolled back at its end if the verdict says so — both inside the
        captured region (first and last graph of a data-parallel capture).

        Every report gains ``"skipped"`` (0 or 1) and ``"anomaly"`` (int32 counts of non-finite values per ``ANOMALY_GROUPS``
        entry; "losses" counts the step's loss scalars for the report only, "buffers" is 0 with a bucket); ``skipped_steps`` is the cumulative device counter.
        ``init_t`` / ``init_s`` are created by the first COMPLETED step: that one eager step reads the verdict on the host (one
        synchronisation, once) and leaves them unset if it was skipped; ``capture`` raises if its warm-up ends without them.
        Host-side call counters — NoiseTransfer's ``time`` / ``cal_num_*`` and the GRL ``iter_num`` — count CALLS, skipped or not.
        Works with ``device_hparams`` on or off and with or without a ``GradBucket``.  Idempotent; raises while a joint or phase
        capture is resident, whose launches are the unguarded ones."""
        if self.anomaly_guard:
            return
        self._refuse_resident("enable_anomaly_guard()")
        self._guard = AnomalyGuard(self.device)
        # the GradNorm-weight Adams create their state on their first step; a skipped first step must leave none behind, so it
        # exists from now on, with the values torch would create (capturable: a float32 device step counter)
        for o, w in ((self.opt_w_t, self.w_t), (self.opt_w_s, self.w_s)):
            if len(o.state[w]) == 0:
                o.state[w]["step"] = torch.zeros((), dtype=torch.float32, device=w.device)
                o.state[w]["exp_avg"] = torch.zeros_like(w, memory_format=torch.preserve_format)
                o.state[w]["exp_avg_sq"] = torch.zeros_like(w, memory_format=torch.preserve_format)
        self.anomaly_guard = True

    @property
    def skipped_steps(self) -> Optional[torch.Tensor]:
        """The cumulative number of skipped steps as a device tensor (int32, one element; None with the mode off).  Nothing in
        a step waits for it: read it whenever the host chooses."""
        return None if self._guard is None else self._guard.skipped

    def _guard_save(self) -> None:
        """Start of a guarded step: copy the state that is not guarded at its writer into its shadows.  With gradient
        accumulation only the call that opens a window saves: eagerly a host decision, under capture the copy's own predicate
        on the window's position word, so that a skipped window is rolled back to before its first micro-step."""
        acc = self.grad_accumulation
        capturing = acc is not None and _capturing(acc.words)
        if acc is not None and not capturing and acc.pending != 0:
            return
        live: List[torch.Tensor] = []
        names: List[str] = []
        fwd = []                                                              # fp32 state the forward pass writes
        for k in self.MODULES:
            is_param = {n for n, _ in self.m[k].named_parameters()}
            # Q1: an omni-scale layer re-masks its weight's .data in every forward, after the optimiser has moved the masked taps
            masked = {f"{n}.conv1d.weight" if n else "conv1d.weight" for n, sub in self.m[k].named_modules()
                      if isinstance(sub, build_layer_with_layer_parameter)}
            for n, t in self.m[k].state_dict().items():
                if n not in is_param or n in masked or k in ("ad_net", "fd_s"):   # buffers; parameters the WGAN clamps rewrite
                    names.append(f"m.{k}.{n}"); live.append(t)
                    if n not in is_param and t.dtype == torch.float32:
                        fwd.append(t)
        for k, o, w in (("w_t", self.opt_w_t, self.w_t), ("w_s", self.opt_w_s, self.w_s)):
            names.append(k); live.append(w.data)
            for n, t in o.state[w].items():
                if isinstance(t, torch.Tensor):
                    names.append(f"o.{k}.{n}"); live.append(t)
        names += ["noise.target_avg", "noise.source_avg"]
        live += [self.m["noise"].target_avg, self.m["noise"].source_avg]
        fwd += live[-2:]
        self._guard_fwd = fwd
        shadow = []
        for n, t in zip(names, live):
            sh = self._shadow.get(n)
            if sh is None or sh.shape != t.shape or sh.dtype != t.dtype:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError(f"anomaly guard: no shadow buffer for {n} yet; run one eager step before capturing")
                sh = self._shadow[n] = torch.empty_like(t, memory_format=torch.contiguous_format)
            shadow.append(sh)
        if acc is not None and capturing:
            guard_copy(shadow, live, _WindowOpens(acc), when=False)           # copies where j == 0 when the kernel runs
        else:
            guard_copy(shadow, live)
        self._guard_live = (live, shadow)

    def _guard_scan(self, modules, gradnorm, losses) -> None:
        """The verdict of a step: count the non-finite values of the gradients of ``modules`` (one group each), of the
        ``gradnorm`` tensors and of the ``losses`` scalars; everything but the losses decides."""
        G = self.ANOMALY_GROUPS
        xs, gs = [], []
        for k in modules:
            for p in self.m[k].parameters():
                if p.grad is not None:
                    xs.append(p.grad); gs.append(G.index(k))
        if self.bucket is None:
            # One process: what the forward pass has already written into the state (BatchNorm running statistics, NoiseTransfer's
            # sums) decides too, as the group "buffers" — a second line behind the gradients, which a NaN input reaches now that the
            # fused ReLUs propagate it.  With a GradBucket these buffers are per-rank values and stay out: ranks must decide alike.
            xs += list(self._guard_fwd); gs += [G.index("buffers")] * len(self._guard_fwd)
        xs += list(gradnorm); gs += [G.index("gradnorm")] * len(gradnorm)
        xs += list(losses); gs += [G.index("losses")] * len(losses)
        count_nonfinite(xs, gs, len(G), self._guard, verdict_groups=[i for i, k in enumerate(G) if k != "losses"])

    def _guard_rollback(self) -> None:
        """End of a guarded step: if the verdict is 1, put the shadows of ``_guard_save`` back."""
        live, shadow = self._guard_live
        guard_copy(live, shadow, self._guard, when=True)

    def _mode_report(self, modules, live: bool = False) -> Dict[str, torch.Tensor]:
        """What the enabled modes add to the report of a step over ``modules``: fresh tensors, or with ``live`` the views of the
        device words themselves where an entry is one — ``capture_phase`` copies those into static tensors of its own, and a
        clone would be one more launch in its graph."""
        out = {}
        if self._clip is not None:
            out.update(self._clip_report(modules))
        if self.weight_average is not None:
            out.update(self._ema_report(live))
        if self._guard is not None:
            words = {"skipped": self._guard.verdict[0], "anomaly": self._guard.counts[: len(self.ANOMALY_GROUPS)]}
            out.update(words if live else {k: v.clone() for k, v in words.items()})
        return out

    # ------------------------------------------------------------------ gradient norms and clipping on the device
    def enable_grad_clip(self, max_norm: Optional[float] = None, per_module: Optional[Dict[str, float]] = None) -> None:
        """From now on every step measures the L2 norm of the gradients per module and, where a limit is set, scales them in
        place before the optimisers read them — on the device, with no host decision, in ``step``, ``capture`` / ``replay``,
        ``phase_step`` and ``capture_phase`` / ``replay_phase``.  ``max_norm`` caps the norm over all modules the step updates,
        ``per_module`` ({name in ``MODULES``: cap}) a module's own; None = no limit, so ``enable_grad_clip()`` alone only reports.
        A module's cap is applied first, as ``torch.nn.utils.clip_grad_norm_(module.parameters(), cap)`` would, then ``max_norm``
        to what the module caps leave (``optim.clip_coefficients`` is the arithmetic).

        Groups are ``MODULES`` in order; only the modules the step updates take part (all of them in the joint step,
        ``PHASES[phase]`` in a phase step) and of those the parameters that have a ``.grad``.  The GradNorm weights' gradients are
        neither counted nor clipped.  The norms are taken after ``on_grads_ready`` — after the data-parallel all-reduce and the Q3
        doubling: those of the gradients the optimisers consume, the same on every rank — and before the anomaly guard's scan,
        which therefore sees the clipped gradients.  Unlike torch, a non-finite norm leaves every gradient alone (all factors 1):
        the norms are reported as they came out and the anomaly guard, if on, skips the step.

        Every report gains ``"grad_l2"`` (fp32 [len(MODULES) + 1]: per module, 0 for one the step does not update; last the norm
        over all of them, before clipping) and ``"clip_coef"`` (fp32 [len(MODULES)]: the factor applied, exactly 1 where nothing was
        clipped — those gradients keep their bits).  With no limit set the step computes the bits of the step without the mode.
        ``set_grad_clip`` changes the limits at any time, under resident captures too.  Idempotent (a second call with arguments
        sets those limits); raises while a joint or phase capture is resident, whose launches lack the two kernels."""
        limits = self._clip_limits(max_norm, dict(per_module or {}))
        if not self.grad_clip:
            self._refuse_resident("enable_grad_clip()")
            self._clip = GradClip(self.device)
            for mods in (self.MODULES,) + tuple(self.PHASES.values()):
                self._clip_masks[tuple(mods)] = torch.tensor([k in mods for k in self.MODULES], device=self.device)
            self.grad_clip = True
        elif max_norm is None and per_module is None:
            return
        self._clip_max, self._clip_per = max_norm, dict(per_module or {})
        self._clip.set_limits(limits)

    def set_grad_clip(self, max_norm=_KEEP, per_module=_KEEP) -> bool:
        """Change the limits of ``enable_grad_clip`` (an argument left out keeps its current value, None removes the limit;
        ``per_module`` replaces the whole mapping).  Legal while captures are resident: the host copy is updated and one
        stream-ordered copy goes into the device limits, so a graph replayed afterwards clips by the new values with no re-capture
        (as ``push_lr`` does for learning rates).  Returns whether the device limits changed."""
        if not self.grad_clip:
            raise RuntimeError("set_grad_clip(): call enable_grad_clip() first")
        max_norm = self._clip_max if max_norm is _KEEP else max_norm
        per_module = self._clip_per if per_module is _KEEP else dict(per_module or {})
        limits = self._clip_limits(max_norm, per_module)
        self._clip_max, self._clip_per = max_norm, dict(per_module)
        return self._clip.set_limits(limits)

    def _clip_limits(self, max_norm, per_module) -> List[float]:
        """The 33 limits of the device vector: group g = MODULES[g], the last one the cap on the whole; inf = none."""
        def cap(v, what):
            if v is None:
                return float("inf")
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not float(v) >= 0.0:
                raise ValueError(f"grad clip: {what} must be a non-negative number or None, got {v!r}")
            return float(v)
        limits = [float("inf")] * (MAX_GROUPS + 1)
        for k, v in per_module.items():
            if k not in self.MODULES:
                raise ValueError(f"grad clip: unknown module {k!r}; one of {self.MODULES}")
            limits[self.MODULES.index(k)] = cap(v, f"the cap of {k!r}")
        limits[MAX_GROUPS] = cap(max_norm, "max_norm")
        return limits

    def _clip_grads(self, modules) -> None:
        """Norms of the gradients of ``modules`` (one group each), the factors their limits ask for, and the scaling: one read
        pass, a finalising workgroup, and a second launch series that returns at once where the factor is 1."""
        xs, gs = [], []
        for k in modules:
            for p in self.m[k].parameters():
                if p.grad is not None:
                    if not p.grad.is_contiguous():
                        p.grad = p.grad.contiguous()
                    xs.append(p.grad); gs.append(self.MODULES.index(k))
        from . import _lib
        c = self._clip
        sumsq_norms(xs, gs, c.limits, c.norms, c.coef, c.slots(int(_lib.load().fst_sumsq_slots(len(xs)))))
        scale_by_group(xs, gs, c.coef)

    def _clip_report(self, modules) -> Dict[str, torch.Tensor]:
        c, n = self._clip, len(self.MODULES)
        return {"grad_l2": torch.cat([c.norms[:n], c.norms[MAX_GROUPS:]]),
                "clip_coef": torch.where(self._clip_masks[tuple(modules)], c.coef[:n], torch.ones((), device=self.device))}

    # ------------------------------------------------------------------ schedules under graph replay
    def enable_device_hparams(self) -> None:
        """Move what the reference schedules into device memory, so that captured steps follow it: the learning rates of the ten
        RMSprops and CPC's Adam (``optim.push_lr`` carries ``group["lr"]`` over before every replay) and the four epoch
        coefficients of ``loss_coefficients`` (``replay(..., epoch=)`` refreshes them).  The two GradNorm-weight Adams (never
        scheduled by the reference) and the GRL coefficients (they saturate: quirk Q7) stay as they are.  Idempotent; raises
        while a joint or phase capture is resident, whose launches take the values by value."""
        if self.device_hparams:
            return
        self._refuse_resident("enable_device_hparams()")
        for o in self._scheduled_opts():
            o.enable_lr_on_device()
        self._coef_host = tuple(float(v) for v in loss_coefficients(0))
        self._coef = torch.tensor(self._coef_host, dtype=torch.float32, device=self.device)
        self.device_hparams = True

    def _scheduled_opts(self):
        return list(self.opts.values()) + [self.opt_cpc]

    def _set_epoch(self, epoch: int) -> None:
        """Note the epoch a step runs at (it goes into the checkpoint); with ``device_hparams`` also bring the coefficient
        tensor to ``loss_coefficients(epoch)`` (a stream-ordered copy, no wait)."""
        self._sched_epoch = epoch
        if not self.device_hparams:
            return
        want = tuple(float(v) for v in loss_coefficients(epoch))
        if want != self._coef_host:
            push_words(self._coef, torch.tensor(want, dtype=torch.float32))
            self._coef_host = want

    def make_schedulers(self) -> Dict[str, object]:
        """The reference's eleven schedulers (train_and_test.py:118-134) on this trainer's optimisers, {name: scheduler}; kept as
        ``self.schedulers`` for ``end_epoch`` and the checkpoint."""
        opts = dict(self.opts)
        opts["cpc"] = self.opt_cpc
        self.schedulers = make_schedulers(opts)
        return self.schedulers

    def end_epoch(self, kind: str, report: Dict[str, torch.Tensor]) -> int:
        """After an epoch of ``kind`` (one of the six phase names or "joint"): step the schedulers the reference steps there, the
        plateau ones on the epoch's last batch ``report`` (rank-averaged with a ``GradBucket``), then push the new rates to the
        device (a no-op without ``device_hparams``, where eager steps read ``group["lr"]`` and captured ones keep their rates).
        Returns the number of learning rates pushed."""
        if self.schedulers is None:
            raise RuntimeError("end_epoch(): call make_schedulers() first")
        step_schedulers(self.schedulers, kind, report, self.bucket)
        return push_lr(self._scheduled_opts())

    # ------------------------------------------------------------------ helpers
    def parameters(self) -> List[nn.Parameter]:
        return [p for k in self.MODULES for p in self.m[k].parameters()]

    def load_params(self, mods: Dict[str, Dict[str, torch.Tensor]], mats=None) -> None:
        """Load per-module state (reference state_dict key names) — used by the parity tests."""
        for k, sd in mods.items():
            self.m[k].load_state_dict({n: v.detach().to(self.device) for n, v in sd.items()})
        if mats is not None:
            self.random_layer.random_matrix = [t.to(self.device) for t in mats]
            self.random_layer._transposed = {}

    # ------------------------------------------------------------------ state snapshot (in-place restore keeps addresses)
    def _state_tensors(self):
        out = {}
        for k in self.MODULES:
            for n, t in self.m[k].state_dict().items():
                out[f"m.{k}.{n}"] = t
        opts = dict(self.opts)
        opts.update({"cpc": self.opt_cpc, "w_t": self.opt_w_t, "w_s": self.opt_w_s})
        for k, o in opts.items():
            for gi, group in enumerate(o.param_groups):
                for pi, p in enumerate(group["params"]):
                    for n, t in o.state.get(p, {}).items():
                        if isinstance(t, torch.Tensor):
                            out[f"o.{k}.{gi}.{pi}.{n}"] = t
        out["w_t"], out["w_s"] = self.w_t.data, self.w_s.data
        out["noise.target_avg"], out["noise.source_avg"] = self.m["noise"].target_avg, self.m["noise"].source_avg
        if self.init_t is not None:
            out["init_t"], out["init_s"] = self.init_t, self.init_s
        if self.weight_average is not None:
            for k, d in self._ema_avg.items():
                for n, t in d.items():
                    out[f"ema.{k}.{n}"] = t
            out["ema.count"] = self.weight_average.count
        return out

    def snapshot(self):
        """Copy of every tensor the step mutates (parameters, BN buffers, optimiser moments, GradNorm weights,
        NoiseTransfer sums) plus the host-side counters."""
        self._ema_no_step("snapshot()")
        self._accum_closed("snapshot()")
        host = {"noise": (self.m["noise"].time, self.m["noise"].cal_num_target, self.m["noise"].cal_num_source),
                "ad": self.m["ad_net"].iter_num, "fd": self.m["fd_s"].iter_num}
        return {"t": {k: v.detach().clone() for k, v in self._state_tensors().items()}, "host": host}

    def restore(self, snap, new_to_zero: bool = False) -> None:
        """``new_to_zero``: also return state created since the snapshot (moments an optimiser makes on its first step) to its
        initial value, zero — the trainer then computes what it would have computed had that state never been created."""
        self._ema_no_step("restore()")
        cur = self._state_tensors()
        with torch.no_grad():
            for k, v in snap["t"].items():
                cur[k].copy_(v)
            if new_to_zero:
                for k, t in cur.items():
                    if k not in snap["t"]:
                        t.zero_()
        n = self.m["noise"]
        n.time, n.cal_num_target, n.cal_num_source = snap["host"]["noise"]
        self.m["ad_net"].iter_num, self.m["fd_s"].iter_num = snap["host"]["ad"], snap["host"]["fd"]

    # ------------------------------------------------------------------ trainer-state checkpoint (resume == uninterrupted)
    def state_dict(self) -> dict:
        """Everything one more step depends on, on the CPU: the eleven modules, all thirteen optimisers, the GradNorm
        weights and their reference losses, NoiseTransfer's running sums and counters (Q5), the GRL call counters (Q7),
        the fixed CDAN random matrices and WaveGlow's cached — possibly stale — inverses (Q2).  The reference keeps
        none of this across runs (utils.py:9-25 saves the classification modules only); a captured-graph trainer that
        cannot resume would be a gap of this build, not of the reference.  Once ``make_schedulers()`` has run, also
        "schedules": the eleven schedulers' state, CPC's learning rate (the RMSprops' are in their ``param_groups``), the epoch of
        the last step and its loss coefficients.  With ``enable_grad_clip()`` on, also "grad_clip": its limits; with
        ``enable_weight_average()`` on, also "weight_average": decay, warm-up flag, update counts and the averaged tensors; with
        ``enable_grad_accumulation()`` on, also "grad_accumulation": its steps; with ``enable_transfer_monitor()`` on, also
        "transfer_monitor": its settings, running sums and counts; with a feeder attached (``attach_feeder``), also
        "feeder": the epoch's kind and the feeder's generator state, epoch, cursor and plan, which ``load_state_dict`` puts into
        the feeder attached then (without one the entry is ignored).  Raises while an accumulation window is open: half a window
        is no state a run could resume from."""
        self._ema_no_step("state_dict()")
        self._accum_closed("state_dict()")
        cpu = lambda t: t.detach().cpu().clone()
        cpc = self.opt_cpc
        noise = self.m["noise"]

        def opt_cpu(o):
            # Optimizer.state_dict() aliases the live (device) moment tensors: copy them out, or an in-memory snapshot
            # followed by more steps would restore advanced moments
            sd = o.state_dict()
            return {"state": {i: {n: (cpu(v) if isinstance(v, torch.Tensor) else v) for n, v in st.items()}
                              for i, st in sd["state"].items()},
                    "param_groups": [dict(g) for g in sd["param_groups"]]}
        return {
            "modules": {k: {n: cpu(v) for n, v in self.m[k].state_dict().items()} for k in self.MODULES},
            "opts": {k: opt_cpu(o) for k, o in self.opts.items()},
            "opt_w_t": opt_cpu(self.opt_w_t), "opt_w_s": opt_cpu(self.opt_w_s),
            "opt_cpc": {"step": [cpu(g["step"]) for g in cpc.param_groups],
                        "exp_avg": [[cpu(cpc.state[p]["exp_avg"]) for p in g["params"]] for g in cpc.param_groups],
                        "exp_avg_sq": [[cpu(cpc.state[p]["exp_avg_sq"]) for p in g["params"]] for g in cpc.param_groups]},
            "w_t": cpu(self.w_t), "w_s": cpu(self.w_s),
            "init_t": None if self.init_t is None else cpu(self.init_t),
            "init_s": None if self.init_s is None else cpu(self.init_s),
            "noise": {"target_avg": cpu(noise.target_avg), "source_avg": cpu(noise.source_avg), "time": noise.time,
                      "cal_num_target": noise.cal_num_target, "cal_num_source": noise.cal_num_source},
            "grl": {"ad_net": self.m["ad_net"].iter_num, "fd_s": self.m["fd_s"].iter_num},
            "random_matrix": [cpu(t) for t in self.random_layer.random_matrix],
            "w_inverse": [cpu(c.W_inverse) if hasattr(c, "W_inverse") else None for c in self.m["nf"].convinv],
            **({} if self.schedulers is None else
               {"schedules": {"schedulers": {k: s.state_dict() for k, s in self.schedulers.items()}, "epoch": self._sched_epoch,
                              "cpc_lr": [g["lr"] for g in cpc.param_groups],       # "opts" carry theirs in param_groups
                              "coefficients": None if self._sched_epoch is None else loss_coefficients(self._sched_epoch)}}),
            **({"grad_clip": {"max_norm": self._clip_max, "per_module": dict(self._clip_per)}} if self.grad_clip else {}),
            **({"weight_average": self._ema_state_dict()} if self.weight_average is not None else {}),
            **({"grad_accumulation": {"steps": self.grad_accumulation.steps_host}} if self.grad_accumulation is not None else {}),
            **({"transfer_monitor": self.transfer_monitor.state_dict()} if self.transfer_monitor is not None else {}),
            **self._fed_state_dict(),                                         # "feeder", while one is attached: its plan and position
        }

    def load_state_dict(self, sd: dict) -> None:
        """Inverse of ``state_dict``.  A captured graph holds the old buffers' addresses only for parameters and
        optimiser moments that are restored IN PLACE here, but re-capture after loading anyway (GRL coefficients and,
        unless ``device_hparams`` is on, the learning rates and the epoch's loss coefficients are baked into a capture; with
        it on, the loaded ``group["lr"]`` reach the device with the next ``push_lr`` — every replay does one — and the loaded
        epoch's coefficients are applied here).  A "schedules" entry is loaded into the schedulers of ``make_schedulers()``,
        which is called here if it has not run; a checkpoint without the entry leaves them alone.  The RMSprop moments are NOT restored in place
        (``Optimizer.load_state_dict`` replaces the tensors), so a resident phase graph would update dead moments:
        every phase capture is dropped here and ``replay_phase`` raises until ``capture_phase`` has run again."""
        self._ema_no_step("load_state_dict()")
        self._accum_closed("load_state_dict()")
        self.release_phase()
        dev = self.device
        for k in self.MODULES:
            self.m[k].load_state_dict({n: v.to(dev) for n, v in sd["modules"][k].items()}, strict=True)
        for k, o in self.opts.items():
            o.load_state_dict(sd["opts"][k])
        self.opt_w_t.load_state_dict(sd["opt_w_t"]); self.opt_w_s.load_state_dict(sd["opt_w_s"])
        cpc = self.opt_cpc
        with torch.no_grad():
            for gi, g in enumerate(cpc.param_groups):
                g["step"].copy_(sd["opt_cpc"]["step"][gi])
                for pi, p in enumerate(g["params"]):
                    cpc.state[p]["exp_avg"].copy_(sd["opt_cpc"]["exp_avg"][gi][pi])
                    cpc.state[p]["exp_avg_sq"].copy_(sd["opt_cpc"]["exp_avg_sq"][gi][pi])
            self.w_t.copy_(sd["w_t"]); self.w_s.copy_(sd["w_s"])
            noise = self.m["noise"]
            noise.target_avg.copy_(sd["noise"]["target_avg"]); noise.source_avg.copy_(sd["noise"]["source_avg"])
        noise.time, noise.cal_num_target, noise.cal_num_source = (sd["noise"][k] for k in ("time", "cal_num_target", "cal_num_source"))
        self.init_t = None if sd["init_t"] is None else sd["init_t"].to(dev)
        self.init_s = None if sd["init_s"] is None else sd["init_s"].to(dev)
        self.m["ad_net"].iter_num, self.m["fd_s"].iter_num = sd["grl"]["ad_net"], sd["grl"]["fd_s"]
        self.random_layer.random_matrix = [t.to(dev) for t in sd["random_matrix"]]
        self.random_layer._transposed = {}
        for c, w in zip(self.m["nf"].convinv, sd["w_inverse"]):
            if w is not None:
                c.W_inverse = w.to(dev)
            elif hasattr(c, "W_inverse"):
                del c.W_inverse
        if "schedules" in sd:
            if self.schedulers is None:
                self.make_schedulers()
            for k, s in self.schedulers.items():
                s.load_state_dict(sd["schedules"]["schedulers"][k])
            for g, lr in zip(cpc.param_groups, sd["schedules"]["cpc_lr"]):
                g["lr"] = lr
            if sd["schedules"]["epoch"] is not None:
                self._set_epoch(sd["schedules"]["epoch"])
        push_lr(self._scheduled_opts())
        if "grad_clip" in sd:                                                 # a checkpoint without the entry leaves the mode as it is
            if not self.grad_clip:
                self.enable_grad_clip()
            self.set_grad_clip(max_norm=sd["grad_clip"]["max_norm"], per_module=sd["grad_clip"]["per_module"])
        if "weight_average" in sd:                                            # likewise; restored in place
            self._ema_load_state_dict(sd["weight_average"])
        if "grad_accumulation" in sd:                                         # likewise; under a resident capture a copy into its words
            if self.grad_accumulation is None:
                self.enable_grad_accumulation(sd["grad_accumulation"]["steps"])
            self.set_grad_accumulation(sd["grad_accumulation"]["steps"])
        if "transfer_monitor" in sd:                                          # likewise; sums, counts and bandwidth restored in place
            self._transfer_load_state_dict(sd["transfer_monitor"])
        self._fed_load_state_dict(sd)

    def save_state(self, path: str) -> None:
        self._accum_closed("save_state()")
        torch.save(self.state_dict(), path)

    def load_state(self, path: str) -> None:
        self.load_state_dict(torch.load(path, map_location="cpu", weights_only=False))

    # ------------------------------------------------------------------ forward (train_and_test.py:547-603)
    def forward_losses(self, x_t, y_t, x_s, y_s, t_samples=(None, None), noise_ratios=None):
        m = self.m
        # log|det W| of the flows' 1x1 weights: three single-workgroup launches that depend on the weights only — on the side stream,
        # beside the feature extractors, instead of in the chain of the first flow pass
        self._side.wait_stream(torch.cuda.current_stream())
        m["nf"].prefetch_logdets(self._side)
        feat_t = m["fe_t"](x_t)
        feat_s = m["dimunif"](m["fe_s"](x_s))
        # The two CPC losses are ~3 k tiny launches (MIOpen's GRU runs step by step) that would leave the chip idle in
        # the captured graph's single chain.  Fork them onto a side stream: they (and their backward, which autograd
        # runs on the stream of the forward op) overlap the WaveGlow passes; joined before the losses are summed.
        main = torch.cuda.current_stream()
        self._side.wait_stream(main)
        with torch.cuda.stream(self._side):
            sl_t = m["cpc"](feat_t, t_samples[0])
            sl_s = m["cpc"](feat_s, t_samples[1])
        out_t, out_s = m["nf"](feat_t), m["nf"](feat_s)
        nf_t, nf_s = self.nf_loss(out_t), self.nf_loss(out_s)
        z_s2t = m["noise"](out_t[0], out_s[0], noise_ratios)
        feat_s2t = m["nf"].infer(z_s2t)
        logit_t, pool_t = m["clf_t"](feat_t)
        m["clf_t"].eval()                                                     # :584-586
        logit_s2t, pool_s2t = m["clf_t"](feat_s2t)
        m["clf_t"].train()
        logit_s, pool_s = m["clf_s"](feat_s)
        ce_t, ce_s = F.cross_entropy(logit_t, y_t), F.cross_entropy(logit_s, y_s)
        cdan = CDAN(feat_t, feat_s2t, logit_t, logit_s2t, m["ad_net"], self.random_layer)
        tr_t, tr_s2t = m["probtransfer"](pool_t), m["probtransfer"](pool_s2t)
        ce_s2t2s = F.cross_entropy(ops.linear_act(tr_s2t, m["clf_s"].hidden), y_s)
        fd = wgan_loss(m["fd_s"](tr_t), m["fd_s"](tr_s2t), m["fd_s"](pool_s))
        main.wait_stream(self._side)
        for t in (feat_t, feat_s):                                             # consumed on the side stream too
            t.record_stream(self._side)
        losses = {"nf_t": nf_t, "nf_s": nf_s, "ce_t": ce_t, "sl_t": sl_t, "ce_s": ce_s, "sl_s": sl_s, "cdan": cdan,
                  "ce_s2t2s": ce_s2t2s, "fd_s": fd}
        # with the two feature tensors, the tensors the reference dumps for its t-SNE plots (:564-581, :604-621): what the
        # transfer monitor measures
        aux = {"logit_t": logit_t, "logit_s": logit_s, "logit_s2t": logit_s2t, "feat_t": feat_t, "feat_s2t": feat_s2t, "feat_s": feat_s,
               "pool_s": pool_s, "tr_t": tr_t, "tr_s2t": tr_s2t}
        return losses, aux

    # ------------------------------------------------------------------ pre-training phases (train_and_test.py:141-494)
    PHASES = {                                                                       # phase -> optimisers stepped
        "target_pretrain": ("fe_t", "clf_t", "cpc"),                                 # :143-171  CE_t + CPC_t
        "source_pretrain": ("fe_s", "dimunif", "clf_s"),                             # :183-209  CE_s
        "ssl_with_ce": ("fe_t", "clf_t", "cpc", "fe_s", "dimunif", "clf_s"),         # :232-275  every 50th epoch
        "ssl": ("fe_t", "cpc", "fe_s", "dimunif"),                                   # :296-348
        "nf_with_ce": ("fe_t", "clf_t", "fe_s", "dimunif", "clf_s", "nf", "cpc"),    # :388-431  every 75th epoch
        "nf": ("fe_t", "fe_s", "dimunif", "nf"),                                     # :457-494  features detached
    }

    def phase_losses(self, phase: str, x_t, y_t, x_s, y_s, t_samples=(None, None)):
        """(total, losses) of one batch of a pre-training phase — sub-graphs of the joint step on the same modules.
        "ssl" runs both classifiers in train mode (their BatchNorm running statistics move) although nothing of theirs
        is in the total; "nf" detaches the features, so only the flow receives gradients."""
        if phase not in self.PHASES:
            raise ValueError(f"unknown phase {phase!r}; one of {sorted(self.PHASES)}")
        m, L = self.m, {}
        if phase == "target_pretrain":
            feat_t = m["fe_t"](x_t)
            L["sl_t"] = m["cpc"](feat_t, t_samples[0])
            L["ce_t"] = F.cross_entropy(m["clf_t"](feat_t)[0], y_t)
            return L["ce_t"] + L["sl_t"], L
        if phase == "source_pretrain":
            feat_s = m["dimunif"](m["fe_s"](x_s))
            L["ce_s"] = F.cross_entropy(m["clf_s"](feat_s)[0], y_s)
            return L["ce_s"], L
        feat_t = m["fe_t"](x_t)
        feat_s = m["dimunif"](m["fe_s"](x_s))
        if phase == "nf":
            feat_t, feat_s = feat_t.detach(), feat_s.detach()
        else:
            L["sl_t"] = m["cpc"](feat_t, t_samples[0])
            L["ce_t"] = F.cross_entropy(m["clf_t"](feat_t)[0], y_t)
            L["sl_s"] = m["cpc"](feat_s, t_samples[1])
            L["ce_s"] = F.cross_entropy(m["clf_s"](feat_s)[0], y_s)
        if phase == "ssl_with_ce":
            return L["sl_t"] + L["sl_s"] + 0.8 * L["ce_t"] + 1.2 * L["ce_s"], L
        if phase == "ssl":
            return L["sl_t"] + L["sl_s"], L
        L["nf_t"], L["nf_s"] = self.nf_loss(m["nf"](feat_t)), self.nf_loss(m["nf"](feat_s))
        if phase == "nf_with_ce":
            return L["nf_t"] + L["nf_s"] + 5 * L["ce_t"] + 5 * L["ce_s"] + 3 * L["sl_t"] + 3 * L["sl_s"], L
        return L["nf_t"] + L["nf_s"], L

    def phase_step(self, phase: str, x_t, y_t, x_s, y_s, t_samples=(None, None)):
        """One batch of a pre-training phase: forward, backward, the phase's optimisers, zero_grad (eager; ``capture_phase`` /
        ``replay_phase`` issue the same launches as one hipGraph).  With gradient accumulation one micro-batch of a window: the
        report is this call's own plus "accum_index", and the update, with what it adds to the report, runs on the call that
        closes the window.  Captured phases do not accumulate: ``capture_phase`` / ``replay_phase`` raise at more than one step."""
        self._ema_no_step("phase_step()")
        acc, closing = self.grad_accumulation, self._closing
        report = self._phase_fwd_bwd(phase, x_t, y_t, x_s, y_s, t_samples)
        if acc is not None:                                                   # a micro-step of a window: only its last call updates
            self._accum_fold(self.parameters(), advance=True)
            report["accum_index"] = acc.j[0].clone()
            if not closing:
                return report
        if self.bucket is not None:
            self.bucket.all_reduce(self.parameters())
        self._phase_update(phase)
        report.update(self._mode_report(self.PHASES[phase]))
        return report

    def _phase_fwd_bwd(self, phase: str, x_t, y_t, x_s, y_s, t_samples):
        """First half of a phase step, device-side and shape-static when the CPC indices are device scalars: the losses, zero_grad,
        backward.  Returns the report."""
        if self._guard is not None:
            self._guard_save()
        with _dist.global_batch(self.bucket if self.sync == "global" else None):
            with ops.pack_cache(), self.m["nf"].shared_fold(), self.m["cpc"].shared_stack():
                total, L = self.phase_losses(phase, x_t, y_t, x_s, y_s, t_samples)
                for o in self.opts.values():
                    o.zero_grad(set_to_none=True)
                self.opt_cpc.zero_grad(set_to_none=True)
                total.backward()
        report = {k: v.detach() for k, v in L.items()}
        report["total"] = total.detach()
        if self._guard is not None:
            self._guard_losses = tuple(report.values())
        return report

    def _phase_update(self, phase: str) -> None:
        """Second half (after the gradient all-reduce of a data-parallel step): the phase's optimisers, then the weight average."""
        if self.on_grads_ready is not None:
            self.on_grads_ready()
        if self._clip is not None:
            self._clip_grads(self.PHASES[phase])
        if self._guard is not None:
            self._guard_scan(self.PHASES[phase], (), self._guard_losses)
            self._guard_losses = ()
        rmsprop_step_many([self.opts[k] for k in self.PHASES[phase] if k != "cpc"], self._guard)
        if "cpc" in self.PHASES[phase]:
            self.opt_cpc.step(guard=self._guard)
        if self._guard is not None:
            self._guard_rollback()
        self._ema_update(self.PHASES[phase], self._guard)                     # the last thing a step does

    # ------------------------------------------------------------------ hipGraph for the phases: capture once each, replay per batch
    def capture_phase(self, phase: str, x_t, y_t, x_s, y_s, warmup: int = 2):
        """Capture one batch of a pre-training phase — exactly what ``phase_step`` issues — into a hipGraph that ``replay_phase``
        launches.  The batch and the two CPC start indices (int32 device scalars; unused by "source_pretrain" and "nf") live in
        static device buffers of this phase.  Capturing has no training side effect: the eager warm-up steps (on a side stream;
        they create the RMSprop moments and load every code object) are undone by ``snapshot`` / ``restore``, moments created
        by the warm-up go back to zero, and the ``.grad`` attributes are put back as they were.
        Single GPU: one graph.  With a ``GradBucket`` (mode A): two graphs, forward + backward and update, with the eager
        gradient all-reduce between them — no collective is ever captured; ``sync="global"`` over more than one rank raises as
        ``capture`` does.  Any number of phases may be resident at once, next to the joint capture: the reference alternates
        "ssl" / "ssl_with_ce" and "nf" / "nf_with_ce".  Phase graphs never replay concurrently, so they share one memory pool;
        the reports are copied out of it, so a phase's report stays valid until that phase's next replay.  Capturing a phase
        again replaces its graph.  The learning rates of the phase's optimisers are baked into the graph, unless
        ``enable_device_hparams()`` ran before: then every ``replay_phase`` runs at their current ``group["lr"]``.
        ``on_grads_ready`` is called inside the captured region, as in ``capture``: it fires ONCE, at capture time (on the gradient
        tensors the graph will write), not per replay and not during the warm-up."""
        self._ema_no_step("capture_phase()")
        if phase not in self.PHASES:
            raise ValueError(f"unknown phase {phase!r}; one of {sorted(self.PHASES)}")
        if self.sync == "global" and self.bucket is not None and self.bucket.world > 1:
            raise RuntimeError("sync='global' (mode B) puts collectives inside autograd: run it eagerly with phase_step()")
        if warmup < 1:
            raise ValueError("capture_phase(): at least one warm-up step (it creates the optimiser moments the graph updates)")
        self._accum_phase_graphs("capture_phase()")
        self.release_phase(phase)
        dev = self.device
        gi = {"x_t": x_t.clone(), "y_t": y_t.clone(), "x_s": x_s.clone(), "y_s": y_s.clone(),
              "t": torch.zeros(2, dtype=torch.int32, device=dev)}
        args = self._static_args(gi)
        params = self.parameters()
        grads_before = [p.grad for p in params]
        snap, hook = self.snapshot(), self.on_grads_ready
        self.on_grads_ready = None
        try:
            with _capture.warmup_stream(dev):                                 # eager warm-up on a side stream
                for _ in range(warmup):
                    keys = sorted(self.phase_step(phase, *args))
                self.restore(snap, new_to_zero=True)
        finally:
            self.on_grads_ready = hook
        # static report: the graphs' own outputs live in the shared pool, where a later capture may reuse what this one frees;
        # the modes' entries get static tensors of their own, shaped like the entries themselves
        g_rep = {k: torch.zeros_like(v) for k, v in self._mode_report(self.PHASES[phase], live=True).items()}
        keys = [k for k in keys if k not in g_rep and k != "accum_index"]     # (the eager warm-up's; a captured phase is a whole step)
        out = torch.zeros(len(keys), device=dev)

        def update():
            self._phase_update(phase)
            for k, v in self._mode_report(self.PHASES[phase], live=True).items():
                g_rep[k].copy_(v)

        def fwd_bwd():
            rep = self._phase_fwd_bwd(phase, *args)
            out.copy_(torch.stack([rep[k] for k in keys]))

        if self._phase_pool is None:
            self._phase_pool = torch.cuda.graph_pool_handle()
        try:
            if self.bucket is None:
                graphs = [torch.cuda.CUDAGraph()]
                with _capture.graph(graphs[0], self._phase_pool):
                    fwd_bwd()
                    update()
            else:
                graphs = [torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()]
                with _capture.graph(graphs[0], self._phase_pool):
                    fwd_bwd()
                self.bucket.all_reduce(params)                                # eager, between the graphs
                with _capture.graph(graphs[1], self._phase_pool):
                    update()
            # the gradient tensors the graph writes stay allocated as long as the graph does
            grads = [p.grad for p in params if p.grad is not None]
        finally:
            for p, g in zip(params, grads_before):
                p.grad = g
        self._phase[phase] = {"graphs": graphs, "in": gi, "grads": grads, "report": {**{k: out[i] for i, k in enumerate(keys)}, **g_rep}}
        return self

    def replay_phase(self, phase: str, x_t, y_t, x_s, y_s, t_samples=(0, 0)):
        """One batch of a captured phase on a new batch of the captured shapes; returns the phase's static report (the keys of
        ``phase_step``: its losses and "total"), valid until this phase's next replay.  Nothing here waits for the device.
        ``.grad`` is left alone: the gradients are in the tensors the capture kept."""
        rec = self._replay_phase_begin(phase, "replay_phase()")
        gi = rec["in"]
        batch = (("x_t", x_t), ("y_t", y_t), ("x_s", x_s), ("y_s", y_s))
        for k, v in batch:
            if v.shape != gi[k].shape or v.dtype != gi[k].dtype:
                raise ValueError(f"replay_phase({phase!r}): {k} is {tuple(v.shape)} {v.dtype}, captured "
                                 f"{tuple(gi[k].shape)} {gi[k].dtype}")
        for k, v in batch:
            if v is not gi[k]:
                gi[k].copy_(v, non_blocking=True)
        gi["t"].copy_(torch.tensor([int(t_samples[0]), int(t_samples[1])], dtype=torch.int32), non_blocking=True)
        return self._replay_phase_graphs(rec)

    def _replay_phase_begin(self, phase: str, what: str) -> dict:
        """The checks of a phase replay; returns the phase's capture record."""
        self._ema_no_step(what)
        self._accum_phase_graphs(what)
        rec = self._phase.get(phase)
        if rec is None:
            if phase not in self.PHASES:
                raise ValueError(f"unknown phase {phase!r}; one of {sorted(self.PHASES)}")
            raise RuntimeError(f"phase {phase!r} is not captured: call capture_phase({phase!r}, ...) first "
                               "(load_state_dict drops every phase capture)")
        return rec

    def _replay_phase_graphs(self, rec: dict):
        """What a phase replay does once the static inputs hold the batch and the CPC indices."""
        if self.device_hparams:
            push_lr(self._scheduled_opts())
        rec["graphs"][0].replay()
        if len(rec["graphs"]) == 2:
            self.bucket.all_reduce_grads(rec["grads"])
            rec["graphs"][1].replay()
        return rec["report"]

    # ------------------------------------------------------------------ device-resident input (the methods of _Fed)
    def begin_epoch(self, kind: str = "joint") -> int:
        """Plan and upload the attached feeder's next epoch for ``kind`` — "joint" or a phase name — and return its number of
        rounds.  For a joint epoch the NoiseTransfer ratios of every round are planned here (``NoiseTransfer.planned_ratios``:
        ``advance``'s own arithmetic from a copy of its counters) and ride in the plan; the counters themselves still move one
        ``advance`` per fed joint step, so a checkpoint taken mid-epoch stays right.  The plan assumes that until the epoch is over
        every joint step is a fed one."""
        if kind != "joint" and kind not in self.PHASES:
            raise ValueError(f"unknown kind {kind!r}; 'joint' or one of {sorted(self.PHASES)}")
        f = self.feeder
        if f is not None and len(f.sets) != 2:
            raise ValueError("JointTrainer.begin_epoch(): a feeder with a source set is needed")
        ratios = None
        if kind == "joint" and f is not None:
            ratios = self.m["noise"].planned_ratios(f.rounds, f.batch[0], f.batch[1])
        return self._fed_begin(kind, ratios)

    def step_fed(self, epoch: int = 0):
        """``step`` on the feeder's current round: the batch, the CPC start indices and the ratios drawn into device buffers this
        trainer keeps, the indices and ratios passed on as 0-d device tensors.  ``StopIteration`` once the epoch is over."""
        self._ema_no_step("step_fed()")
        self._fed_check("joint", "step_fed()")
        b = self._fed_eager()
        x_t, y_t, x_s, y_s = b["batch"]
        self._set_epoch(epoch)
        self.m["noise"].advance(x_t.size(0), x_s.size(0))                     # the counters; this round's ratios are in the plan
        return self._step_body(x_t, y_t, x_s, y_s, epoch, (b["t"][0], b["t"][1]), (b["r"][0], b["r"][1]))

    def replay_fed(self, epoch: Optional[int] = None):
        """``replay`` on the feeder's current round, drawn straight into the capture's static inputs (batch, CPC indices, ratios);
        everything behind the inputs is ``replay``'s, the three-graph data-parallel path included."""
        self._fed_check("joint", "replay_fed()")
        self._replay_begin("replay_fed()", epoch)
        gi = self._g_in
        self.feeder.feed(gi["x_t"], gi["y_t"], gi["x_s"], gi["y_s"], t=gi["t"], r=gi["r"])
        self.m["noise"].advance(gi["x_t"].size(0), gi["x_s"].size(0))
        return self._replay_graphs()

    def phase_step_fed(self, phase: str):
        """``phase_step`` on the feeder's current round.  A phase that uses one side only still consumes the round's other side."""
        self._ema_no_step("phase_step_fed()")
        self._fed_check(phase, "phase_step_fed()")
        b = self._fed_eager()
        return self.phase_step(phase, *b["batch"], (b["t"][0], b["t"][1]))

    def replay_phase_fed(self, phase: str):
        """``replay_phase`` on the feeder's current round, drawn straight into the phase capture's static inputs."""
        self._fed_check(phase, "replay_phase_fed()")
        rec = self._replay_phase_begin(phase, "replay_phase_fed()")
        gi = rec["in"]
        self.feeder.feed(gi["x_t"], gi["y_t"], gi["x_s"], gi["y_s"], t=gi["t"])
        return self._replay_phase_graphs(rec)

    def make_evaluator(self, side: str, data, batch_size: int, **kw):
        """An ``evaluate.Evaluator`` over the resident ``data``: ``side="target"`` evaluates (``fe_t``, ``clf_t``), ``side="source"``
        (``fe_s``, ``clf_s``) through ``dimunif``; ``kw`` are its other arguments."""
        from .evaluate import Evaluator
        if side == "target":
            return Evaluator(self.m["fe_t"], self.m["clf_t"], data, batch_size, **kw)
        if side == "source":
            return Evaluator(self.m["fe_s"], self.m["clf_s"], data, batch_size, feature_trans=self.m["dimunif"], **kw)
        raise ValueError(f"make_evaluator(): side must be 'target' or 'source', got {side!r}")

    def _accum_phase_graphs(self, what: str) -> None:
        """A captured phase is one whole step per replay: the phase graphs have no micro-step / update split."""
        self._accum_closed(what)
        if self.grad_accumulation is not None and self.grad_accumulation.steps_host > 1:
            raise RuntimeError(f"{what}: captured phases do not accumulate gradients ({self.grad_accumulation.steps_host} steps per "
                               "window are set); run the phase eagerly with phase_step()")

    def release_phase(self, phase: Optional[str] = None) -> None:
        """Drop the capture of ``phase`` (of every phase if None); a phase that is not captured is left as it is."""
        if phase is None:
            self._phase.clear()
        else:
            self._phase.pop(phase, None)
        if not self._phase:
            self._phase_pool = None

    def captured_phases(self) -> Tuple[str, ...]:
        return tuple(sorted(self._phase))

    # ------------------------------------------------------------------ one optimisation step (:645-766)
    def step(self, x_t, y_t, x_s, y_s, epoch: int = 0, t_samples=(None, None)):
        """Eager step.  ``t_samples``: the two CPC start indices (drawn like the reference if None)."""
        self._ema_no_step("step()")
        self._set_epoch(epoch)
        ratios = self.m["noise"].advance(x_t.size(0), x_s.size(0))
        return self._step_body(x_t, y_t, x_s, y_s, epoch, t_samples, ratios)

    def _step_body(self, x_t, y_t, x_s, y_s, epoch, t_samples, noise_ratios):
        """Everything device-side and shape-static, so it runs eagerly or under hipGraph capture unchanged.
        Three parts with the step's only collectives between them (so a captured step never contains RCCL):
        A1 = forward + the full backward;  [the gradient bucket's all-reduce starts on a side stream]
        A2 = GradNorm's partial backward passes (they never touch ``.grad``: they overlap the all-reduce);
        [wait for the bucket; average the 10 GradNorm scalars]  B = GradNorm weight update + optimisers."""
        closing = self._closing                                               # the collectives and B: on the call that closes a window
        with _dist.global_batch(self.bucket if self.sync == "global" else None), self._step_scope():
            state = self._step_part_a1(x_t, y_t, x_s, y_s, epoch, t_samples, noise_ratios)
            if closing:
                self._reduce_begin()
            mid = self._step_part_a2(state)
        if not closing:
            return self._micro_report(mid)
        self._reduce_end(mid)
        return self._step_part_b(mid)

    @staticmethod
    def _micro_report(mid):
        """What a call that does not close its window returns: this micro-batch's losses and aux entries, and the position."""
        report = dict(mid["report"])
        report["accum_index"] = mid["accum_index"]
        return report

    def _step_scope(self):
        """One scope for forward and every backward pass of a step: weights packed once, the flow's weight-norm fold and the
        CPC predictor stack built once."""
        import contextlib
        st = contextlib.ExitStack()
        st.enter_context(ops.pack_cache())
        st.enter_context(self.m["nf"].shared_fold())
        st.enter_context(self.m["cpc"].shared_stack())
        return st

    def _step_part_a1(self, x_t, y_t, x_s, y_s, epoch, t_samples, noise_ratios):
        if self._guard is not None:
            self._guard_save()
        L, aux = self.forward_losses(x_t, y_t, x_s, y_s, t_samples, noise_ratios)
        lt = torch.stack([L["nf_t"], L["ce_t"]])
        ls = torch.stack([L["nf_s"], L["ce_s"], L["ce_s2t2s"]])
        # device_hparams: 0-dim views of the coefficient tensor (_set_epoch wrote the epoch's values) — same fp32 products
        a, b, c, d = loss_coefficients(epoch) if self._coef is None else self._coef.unbind(0)
        # Q3: first backward + second backward (weights zeroed) == Σ wᵢ∇Lᵢ + 2·(a∇cdan + b∇fd + c∇sl_t + d∇sl_s)
        total = torch.sum(self.w_t.detach() * lt) + torch.sum(self.w_s.detach() * ls) \
            + 2.0 * (a * L["cdan"] + b * L["fd_s"] + c * L["sl_t"] + d * L["sl_s"])
        for o in self.opts.values():
            o.zero_grad(set_to_none=True)
        self.opt_cpc.zero_grad(set_to_none=True)
        total.backward(retain_graph=True)
        if self.grad_accumulation is not None:                                # every .grad of the step is final here: A2 never touches one
            self._accum_fold(self.parameters(), advance=False)
        return {"L": L, "aux": aux, "lt": lt, "ls": ls}

    def _step_part_a2(self, state):
        L, aux, lt, ls = state["L"], state["aux"], state["lt"], state["ls"]
        # GradNorm (:682-690): per-loss gradient norms over the 12 shared tensors
        sh_t = list(self.m["fe_t"].return_last_layer().parameters())
        sh_s = list(self.m["fe_s"].return_last_layer().parameters())
        # Differentiate the loss tensors themselves, not lt[i] / ls[i]: a select of the stacked vector sends a ZERO
        # cotangent down every other loss's graph (autograd does not prune zeros), i.e. 8 WaveGlow backward
        # traversals per step where 4 carry anything (ce_t / ce_s never touch the flow).  Same values, half the work.
        with ops.partial_backward():
            g_t = [torch.autograd.grad(L[k], sh_t, retain_graph=True) for k in ("nf_t", "ce_t")]
            g_s = [torch.autograd.grad(L[k], sh_s, retain_graph=(k != "ce_s2t2s")) for k in ("nf_s", "ce_s", "ce_s2t2s")]
        if _dist.global_batch_active():
            # mode B: the norms are those of the GLOBAL per-loss gradients (mean over ranks), not means of norms
            flat = torch.cat([g.reshape(-1) for gs in g_t + g_s for g in gs])
            flat = flat / _dist.sum_over_ranks_(flat)
            it = iter(torch.split(flat, [g.numel() for gs in g_t + g_s for g in gs]))
            g_t = [[next(it).view_as(g) for g in gs] for gs in g_t]
            g_s = [[next(it).view_as(g) for g in gs] for gs in g_s]
        # Σ_θ ‖∂L_i/∂θ‖₂ per loss (:685-690): all 5 × 12 norms as ONE multi-tensor launch (60 separate reductions before)
        norms = torch.stack(torch._foreach_norm([g for gs in g_t + g_s for g in gs])).view(len(g_t) + len(g_s), -1).sum(dim=1)
        base_t, base_s = norms[: len(g_t)], norms[len(g_t):]
        report = {k: v.detach() for k, v in L.items()}
        # (with the transfer monitor off a report holds the entries it always held: the monitor's four extra tensors stay in aux)
        mine = () if self.transfer_monitor is not None else self.TRANSFER_AUX
        report.update({k: v.detach() for k, v in aux.items() if k not in mine})
        if self.transfer_monitor is not None:                                 # this batch's MMD² for the four pairs; reads only
            report["transfer"] = self._transfer_measure(report)
        # scalars that must be identical on every rank: loss values and gradient-norm bases (10 floats)
        scal = torch.cat([lt.detach(), ls.detach(), base_t, base_s]).contiguous()
        mid = {"report": report, "scal": scal, "loss_keys": tuple(L)}
        acc = self.grad_accumulation
        if acc is not None:
            # the ten scalars and the nine losses are averaged over the window as the gradients are, at the same position: this
            # fold is the one that moves the window on
            losses = torch.stack([L[k].detach().float() for k in L]).contiguous()
            if self._accum_scalars is None:
                if _capturing(scal):
                    raise RuntimeError("gradient accumulation: run one eager window before capturing")
                self._accum_scalars = (torch.empty_like(scal), torch.empty_like(losses))
            accumulate(self._accum_scalars, (scal, losses), acc, advance=True)
            mid["window_losses"], mid["accum_index"] = losses, acc.j[0].clone()
        return mid

    def _step_part_a(self, x_t, y_t, x_s, y_s, epoch, t_samples, noise_ratios):
        with self._step_scope():
            return self._step_part_a2(self._step_part_a1(x_t, y_t, x_s, y_s, epoch, t_samples, noise_ratios))

    def _reduce_begin(self) -> None:
        if self.bucket is not None:
            self.bucket.all_reduce_begin(self.parameters())

    def _reduce_end(self, mid) -> None:
        if self.bucket is None:
            return
        self.bucket.all_reduce_end()
        mid["scal"].copy_(self.bucket.mean_scalars(mid["scal"]))

    def _step_part_b(self, mid):
        scal = mid["scal"]
        lt_v, ls_v, base_t, base_s = scal[0:2], scal[2:5], scal[5:7], scal[7:10]
        guard, first = self._guard, self.init_t is None
        if self.init_t is None:                                               # :658-664
            self.init_t, self.init_s = torch.sigmoid(lt_v).clone(), torch.sigmoid(ls_v).clone()
        # ‖wᵢ·g‖ = |wᵢ|·‖g‖, so the norms are differentiable functions of w alone (:685-715)
        nt, ns = torch.abs(self.w_t) * base_t, torch.abs(self.w_s) * base_s
        ratio_t, ratio_s = torch.sigmoid(lt_v) / self.init_t, torch.sigmoid(ls_v) / self.init_s
        inv_t, inv_s = ratio_t / ratio_t.mean(), ratio_s / ratio_s.mean()
        const_t = (nt.detach().mean() * inv_t ** self.alpha).detach()
        const_s = (ns.detach().mean() * inv_s ** self.alpha).detach()
        g_w_t = torch.autograd.grad(torch.sum(torch.abs(nt - const_t)), self.w_t)[0]
        g_w_s = torch.autograd.grad(torch.sum(torch.abs(ns - const_s)), self.w_s)[0]
        for w, g in ((self.w_t, g_w_t), (self.w_s, g_w_s)):                   # static .grad buffers (graph-safe)
            if w.grad is None:
                w.grad = torch.zeros_like(w)
            w.grad.copy_(g)
        if self.on_grads_ready is not None:
            self.on_grads_ready()
        if self._clip is not None:
            self._clip_grads(self.MODULES)
        if guard is not None:
            losses = [mid["window_losses"]] if "window_losses" in mid else [mid["report"][k] for k in mid["loss_keys"]]
            self._guard_scan(self.MODULES, (scal, self.w_t.grad, self.w_s.grad), losses)
            if first and int(guard.verdict) != 0:                             # the one host read: only a COMPLETED step sets them
                self.init_t = self.init_s = None
        self.opt_w_t.step(); self.opt_w_s.step()
        rmsprop_step_many(list(self.opts.values()), guard)
        self.opt_cpc.step(guard=guard)
        with torch.no_grad():                                                 # :756-766
            self.w_t.clamp_(min=0.0)
            self.w_t.mul_(7 / torch.sum(self.w_t))
            self.w_s.clamp_(min=0.0)
            self.w_s.mul_(8 / torch.sum(self.w_s))
            for p in self.m["ad_net"].parameters():
                p.clamp_(-0.0005, 0.0005)
            for p in self.m["fd_s"].parameters():
                p.clamp_(-0.01, 0.01)
        if guard is not None:
            self._guard_rollback()
        self._ema_update(self.MODULES, guard)                                 # the last thing a step does
        report = dict(mid["report"])
        report.update({"w_t": self.w_t.detach().clone(), "w_s": self.w_s.detach().clone(),
                       "norms_t": nt.detach(), "norms_s": ns.detach()})
        report.update(self._mode_report(self.MODULES))
        if "window_losses" in mid:
            report.update({"accum_index": mid["accum_index"], "window_losses": mid["window_losses"]})
        return report

    # ------------------------------------------------------------------ hipGraph: capture once, replay per step
    def capture(self, x_t, y_t, x_s, y_s, epoch: int = 0, warmup: int = 11):
        """Capture one whole step (≈12 k launches: forward, GradNorm partial backwards, backward, optimisers) into
        hipGraphs.  Per-step inputs live in static device buffers that ``replay`` refreshes: the batch, the two CPC
        start indices and NoiseTransfer's two accumulation ratios.  The GRL coefficients are Python floats baked in
        at capture, so the warm-up runs until their call counters saturate (20 calls = 10 steps — quirk Q7); the
        epoch-dependent loss coefficients and every learning rate are baked too: re-capture when ``loss_coefficients(epoch)``
        or a ``group["lr"]`` changes — a scheduler attached to ``opts[k]`` does NOT reach a replayed step.  After
        ``enable_device_hparams()`` both live on the device instead: every ``replay`` runs at the optimisers' current
        ``group["lr"]`` and ``replay(..., epoch=)`` at that epoch's coefficients, with no re-capture (the GRL coefficients and the
        GradNorm-weight Adams' rates stay baked).
        Single GPU: one graph.  Data parallel: three graphs (A1 forward + backward, A2 GradNorm's partial passes, B update)
        with the eager RCCL collectives between them, the gradient all-reduce overlapping A2 on a side stream.
        With gradient accumulation, single GPU: two graphs sharing a pool — the micro-step (A1, the fold of the gradients, A2, the
        fold of the scalars, which moves the window on) and the update (B) — of which ``replay`` launches the first on every call
        and the second on the calls that close a window; data parallel: the three graphs, the folds at the end of A1 and of A2.
        The warm-up then runs whole windows (``warmup`` rounded up), so that the capture starts with the window closed."""
        self._ema_no_step("capture()")
        self._accum_closed("capture()")
        acc = self.grad_accumulation
        if acc is not None:
            warmup = -(-warmup // acc.steps_host) * acc.steps_host
        if self.sync == "global" and self.bucket is not None and self.bucket.world > 1:
            raise RuntimeError("sync='global' (mode B) puts collectives inside autograd: run it eagerly with step()")
        dev = self.device
        self._g_in = {"x_t": x_t.clone(), "y_t": y_t.clone(), "x_s": x_s.clone(), "y_s": y_s.clone(),
                      "t": torch.zeros(2, dtype=torch.int32, device=dev), "r": torch.ones(2, device=dev)}
        self._g_epoch = epoch
        self._set_epoch(epoch)
        T_half = max(1, (self.cfg.L_t // 2) // 2)
        with _capture.warmup_stream(dev):                                     # eager warm-up on a side stream
            for _ in range(warmup):
                self._replay_inputs(x_t, y_t, x_s, y_s, (int(torch.randint(T_half, (1,))), int(torch.randint(T_half, (1,)))))
                self._graph_body()
        if self.m["ad_net"].iter_num < self.m["ad_net"].max_iter or self.m["fd_s"].iter_num < self.m["fd_s"].max_iter:
            raise RuntimeError("capture(): GRL call counters not saturated yet; increase warmup")
        if self._guard is not None and self.init_t is None:
            raise RuntimeError("capture(): the anomaly guard skipped every warm-up step (non-finite gradients), so the GradNorm "
                               "reference losses init_t / init_s do not exist yet; capture on a batch the step completes on")
        self._replay_inputs(x_t, y_t, x_s, y_s, (0, 0))
        if self.bucket is None and acc is None:
            self._graphs = [torch.cuda.CUDAGraph()]
            with _capture.graph(self._graphs[0]):
                self._g_out = self._graph_body()
        elif self.bucket is None:
            gm, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with _capture.graph(gm):
                self._g_mid = self._step_part_a(*self._static_args(self._g_in, self._g_epoch))
            with _capture.graph(gb, gm.pool()):
                self._g_out = self._step_part_b(self._g_mid)
            self._graphs = [gm, gb]
        else:
            ga1, ga2, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with self._step_scope():                                          # packed weights of A1 are reused by A2
                with _capture.graph(ga1):
                    state = self._step_part_a1(*self._static_args(self._g_in, self._g_epoch))
                pool = ga1.pool()
                self._reduce_begin()                                          # eager, on the bucket's side stream
                with _capture.graph(ga2, pool):
                    self._g_mid = self._step_part_a2(state)
                del state                                                     # the autograd graph of the captured step
            self._reduce_end(self._g_mid)                                     # eager; also fixes the bucket's buffer
            with _capture.graph(gb, pool):
                self._g_out = self._step_part_b(self._g_mid)
            self._graphs = [ga1, ga2, gb]
        if acc is not None:
            self._g_micro = self._micro_report(self._g_mid)
        return self

    def _graph_body(self):
        return self._step_body(*self._static_args(self._g_in, self._g_epoch))

    @staticmethod
    def _static_args(gi: dict, *epoch):
        """The arguments of a step out of a capture's static inputs ``gi``: the batch, ``epoch`` if the step takes one, the two CPC
        indices and, where the capture holds them, NoiseTransfer's two ratios, as 0-d views."""
        pairs = [(gi[k][0], gi[k][1]) for k in ("t", "r") if k in gi]
        return (gi["x_t"], gi["y_t"], gi["x_s"], gi["y_s"], *epoch, *pairs)

    def _replay_inputs(self, x_t, y_t, x_s, y_s, t_samples):
        gi = self._g_in
        for k, v in (("x_t", x_t), ("y_t", y_t), ("x_s", x_s), ("y_s", y_s)):
            if v is not gi[k]:
                gi[k].copy_(v, non_blocking=True)
        ratios = self.m["noise"].advance(x_t.size(0), x_s.size(0))
        host = torch.tensor([float(t_samples[0]), float(t_samples[1]), ratios[0], ratios[1]], dtype=torch.float64)
        dev = host.to(self.device, non_blocking=True)
        gi["t"].copy_(dev[:2])
        gi["r"].copy_(dev[2:])

    def replay(self, x_t, y_t, x_s, y_s, t_samples, epoch: Optional[int] = None):
        """One step through the captured graph(s); returns the (static) report tensors.  With ``device_hparams`` the step runs at
        the optimisers' current ``group["lr"]`` and, when ``epoch`` is given, at ``loss_coefficients(epoch)``; without it, at the
        captured values, and an ``epoch`` other than the captured one raises.  With gradient accumulation a call that does not
        close its window returns the micro-step's report (this batch's losses and aux entries, "accum_index") and launches no
        update; the closing call returns the whole report, with "window_losses"."""
        self._replay_begin("replay()", epoch)
        self._replay_inputs(x_t, y_t, x_s, y_s, t_samples)
        return self._replay_graphs()

    def _replay_begin(self, what: str, epoch: Optional[int]) -> None:
        """The checks of a replay, and with ``device_hparams`` the epoch's coefficients and the learning rates."""
        self._ema_no_step(what)
        if self._graphs is None:
            raise RuntimeError("call capture() first")
        if self.device_hparams:
            if epoch is not None:
                self._set_epoch(epoch)
            push_lr(self._scheduled_opts())
        elif epoch is not None and epoch != self._g_epoch:
            raise ValueError(f"{what[:-1]}epoch={epoch}): the graph was captured at epoch {self._g_epoch} and its loss coefficients "
                             "are baked in; re-capture, or enable_device_hparams() before capturing")

    def _replay_graphs(self):
        """What a replay does once the static inputs hold the batch, the CPC indices and the ratios."""
        acc, closing = self.grad_accumulation, self._closing
        self._graphs[0].replay()
        if len(self._graphs) == 3:
            if closing:
                self._reduce_begin()                                          # the bucket's all-reduce, on its side stream ...
            self._graphs[1].replay()                                          # ... under GradNorm's partial backward passes
        if acc is not None:
            acc.advance_host()                                                # the captured fold of the scalars moved the window on
            if not closing:
                return self._g_micro
        if len(self._graphs) == 3:
            self._reduce_end(self._g_mid)
        if len(self._graphs) > 1:
            self._graphs[-1].replay()
        return self._g_out
