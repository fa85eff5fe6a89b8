"""The reference's schedules (train_and_test.py:118-134, :665-672), on a device-free footing so the tables can be tested.

``make_schedulers`` builds the reference's eleven learning-rate schedulers on a trainer's optimisers and ``step_schedulers`` steps
the ones the reference steps after an epoch (``JointTrainer.end_epoch``); ``loss_coefficients`` are the four epoch coefficients of
the joint step.  A captured step follows them only after ``enable_device_hparams()``, which moves the learning rates and the
coefficients into device tensors.
"""
from __future__ import annotations

import warnings
from typing import Dict, Tuple

import torch


def loss_coefficients(epoch: int) -> Tuple[float, float, float, float]:
    """(cdan, fd_s, sl_t, sl_s) coefficients by epoch (train_and_test.py:665-672)."""
    if epoch < 12:
        return 3, 3, 2, 2
    if epoch < 24:
        return 2, 3, 1.8, 1.5
    if epoch < 50:
        return 1.5, 2, 1.8, 1.8
    return 1.5, 1.5, 2.5, 2.5


# ---- the reference's learning-rate schedules (train_and_test.py:118-134)
STEP_LR = {"fe_t": (25, 0.8), "clf_t": (25, 0.8), "fe_s": (25, 0.8), "dimunif": (25, 0.8), "clf_s": (25, 0.8),
           "cpc": (25, 0.7), "noise": (55, 0.6)}                               # name -> (step_size, gamma)
PLATEAU = ("probtransfer", "nf", "ad_net", "fd_s")                             # ReduceLROnPlateau('min', factor=0.7, min_lr=1e-4)
EPOCH_SCHEDULERS = {                                                           # kind of epoch -> schedulers stepped after it
    "target_pretrain": ("fe_t", "clf_t", "cpc"),                               # :172-174
    "source_pretrain": ("fe_s", "dimunif", "clf_s"),                           # :211-213
    "ssl_with_ce": ("fe_t", "clf_t", "cpc", "fe_s", "dimunif", "clf_s"),       # :275-280
    "ssl": ("fe_t", "cpc", "fe_s", "dimunif"),                                 # :343-348
    "nf_with_ce": ("fe_t", "clf_t", "fe_s", "dimunif", "clf_s", "cpc", "nf"),  # :436-442
    "nf": ("fe_t", "fe_s", "dimunif", "nf"),                                   # :491-494
    "joint": ("fe_t", "clf_t", "cpc", "fe_s", "dimunif", "clf_s", "probtransfer", "nf", "noise", "ad_net", "fd_s"),  # :767-777
}
# The metric a plateau scheduler is given: a key of the epoch's LAST batch report, or None for the constant 0.0 (quirk Q8: the
# reference zeroes cdan_loss.data and feature_discriminator_s_loss.data in place at :739-740 before :776-777 read them)
PLATEAU_METRIC = {
    "nf_with_ce": {"nf": "total"},                                             # :420, :442
    "nf": {"nf": "total"},                                                     # :481, :494
    "joint": {"probtransfer": "ce_s2t2s", "nf": "nf_t", "ad_net": None, "fd_s": None},   # :773-777
}


def make_schedulers(opts: Dict[str, torch.optim.Optimizer]) -> Dict[str, object]:
    """The reference's scheduler for every optimiser of ``opts`` it schedules ({module name: optimiser}, "cpc" for CPC's Adam):
    stock ``torch.optim.lr_scheduler`` objects, {name: scheduler}."""
    sch = torch.optim.lr_scheduler
    out = {}
    for k, o in opts.items():
        if k in STEP_LR:
            out[k] = sch.StepLR(o, step_size=STEP_LR[k][0], gamma=STEP_LR[k][1])
        elif k in PLATEAU:
            out[k] = sch.ReduceLROnPlateau(o, "min", factor=0.7, min_lr=0.0001)
    return out


def step_schedulers(schedulers: Dict[str, object], kind: str, report: Dict[str, torch.Tensor], bucket=None) -> None:
    """Step the schedulers the reference steps after an epoch of ``kind`` (a phase name or "joint"); ``report`` is the epoch's
    last batch report.  With a ``GradBucket`` the plateau metrics are averaged over the ranks first, so that every rank's
    schedulers take the same decisions."""
    if kind not in EPOCH_SCHEDULERS:
        raise ValueError(f"unknown kind of epoch {kind!r}; one of {sorted(EPOCH_SCHEDULERS)}")
    metric_of = PLATEAU_METRIC.get(kind, {})
    keys = [k for k in EPOCH_SCHEDULERS[kind] if metric_of.get(k) is not None]
    values = {}
    if keys:
        vals = torch.stack([report[metric_of[k]].detach().float().reshape(()) for k in keys])
        if bucket is not None:
            vals = bucket.mean_scalars(vals)
        values = dict(zip(keys, vals.tolist()))
    with warnings.catch_warnings():
        # torch warns when a scheduler steps before its optimiser's step() was ever called: the trainers step the optimisers
        # through rmsprop_step_many and graph replays, never through step()
        warnings.filterwarnings("ignore", message="Detected call of `lr_scheduler.step\\(\\)` before", category=UserWarning)
        for k in EPOCH_SCHEDULERS[kind]:
            if k in PLATEAU:
                schedulers[k].step(values.get(k, 0.0))
            else:
                schedulers[k].step()
