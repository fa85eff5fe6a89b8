"""Transfer monitor: how far apart two feature sets are, as a number, on the device and under graph replay.

The reference judges its style transfer by eye: every batch of the joint epoch it copies six tensors to the host and every second
epoch it writes them out for t-SNE plots (train_and_test.py:564-621, :792-797).  Here the same six tensors are compared by the
multi-kernel maximum mean discrepancy of the domain-adaptation literature (the Gaussian bank with the mean-distance bandwidth of
DAN / JAN), per step, with no host read.

The definition (``mmd2_reference``, plain torch fp64, runs anywhere).  For ``x [n, ...]`` and ``y [m, ...]`` flattened to
``[n, D]`` and ``[m, D]``, ``n, m >= 2``:

    Z = [x; y],  N = n + m,  c = column mean of x,  Zc = Z - c,  G = Zc Zc^T
    d2_ij = max(G_ii + G_jj - 2 G_ij, 0),  d2_ii = 0
    bw = sum_{i != j} d2_ij / (N^2 - N)                       (unless ``bandwidth`` is given)
    k_ij = sum_{q < kernels} exp(-d2_ij / (bw mul^(q - kernels // 2)))
    MMD2 = sum_{i != j in x} k / (n (n - 1)) + sum_{i != j in y} k / (m (m - 1)) - 2 sum_{i in x, j in y} k / (n m)

(the unbiased estimator; ``bw == 0``, all rows equal, gives 0).  The centring is part of the definition: in exact arithmetic it
changes nothing (the kernel is translation invariant), in split-bf16 it decides whether ``d2`` survives the cancellation
``G_ii + G_jj - 2 G_ij`` — features behind BatchNorm and ReLU have non-zero means, and two sets 1 % apart at mean 3 have ``d2`` at
1e-5 of ``|z|^2``, the size of the split-bf16 error.

On the device (``mmd2``, ``TransferMonitor``): ``ops.mmd_centre`` (the column mean of the first set), ``ops.mmd_gram`` (the pooled
Gram of up to four sets on the matrix cores, centred while staged; under ``FST_MATH=f32`` ``ops.gemm_f32`` on explicitly centred
copies) and ``ops.mmd_fold`` (distances, bandwidth, kernel bank and estimator per pair of sets, in fp64).  ``JointTrainer.
enable_transfer_monitor()`` runs them after ``forward_losses`` on the six tensors and reports ``"transfer"``.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import ops
from .modes import _Mode

FIELDS = ("mmd2", "bandwidth", "d2_within_x", "d2_within_y", "d2_between")       # the five numbers of a pair, in order
# the trainer's pairs, x|y: target features against source-to-target features (the distance the transfer is meant to close) and
# against the untransferred source features (the distance it started from); in the source classifier's hidden space the source
# against the transformed target (t2s) and against the source sent to the target and back (s2t2s)
PAIRS = ("t|s2t", "t|s", "s|t2s", "s|s2t2s")


def check_settings(kernels, mul, bandwidth) -> Tuple[int, float, Optional[float]]:
    """(kernels, mul, bandwidth) as the kernels take them (``mul`` rounded to fp32), or ValueError."""
    if isinstance(kernels, bool) or not isinstance(kernels, int) or not 1 <= kernels <= ops.MMD_MAX_KERNELS:
        raise ValueError(f"transfer monitor: kernels must be an integer in 1..{ops.MMD_MAX_KERNELS}, got {kernels!r}")
    if isinstance(mul, bool) or not isinstance(mul, (int, float)) or not 0.0 < float(mul) <= 1e30:
        raise ValueError(f"transfer monitor: mul must be a positive number (at most 1e30), got {mul!r}")
    if bandwidth is not None and (isinstance(bandwidth, bool) or not isinstance(bandwidth, (int, float))
                                  or not 0.0 < float(bandwidth) < math.inf):
        raise ValueError(f"transfer monitor: bandwidth must be a positive finite number or None, got {bandwidth!r}")
    mul = float(torch.tensor(float(mul), dtype=torch.float32))                 # (mul crosses the C ABI as fp32 and is widened there)
    return kernels, mul, None if bandwidth is None else float(bandwidth)


def mmd2_from_gram(G: torch.Tensor, n: int, m: int, kernels: int = 5, mul: float = 2.0, bandwidth: Optional[float] = None) -> torch.Tensor:
    """The five numbers (``FIELDS``) from a Gram ``G [n + m, n + m]`` of the pooled rows, x first: the arithmetic of
    ``mmd2_reference`` behind the Gram, and of ``ops.mmd_fold``.  fp64 on ``G``'s device."""
    kernels, mul, bandwidth = check_settings(kernels, mul, bandwidth)
    N = n + m
    if n < 2 or m < 2 or tuple(G.shape) != (N, N):
        raise ValueError(f"mmd2: two sets of at least 2 rows and a [{N}, {N}] Gram, got n = {n}, m = {m}, G {tuple(G.shape)}")
    G = G.double()
    g = G.diagonal()
    d2 = (g[:, None] + g[None, :] - 2.0 * G).clamp(min=0.0)                    # (a NaN stays a NaN)
    d2.fill_diagonal_(0.0)
    xx, yy, xy = d2[:n, :n].sum(), d2[n:, n:].sum(), d2[:n, n:].sum()
    bw = (xx + yy + 2.0 * xy) / (N * N - N) if bandwidth is None else torch.tensor(bandwidth, dtype=torch.float64, device=G.device)
    if float(bw) == 0.0:
        mmd2 = torch.zeros((), dtype=torch.float64, device=G.device)
    else:
        k = torch.zeros_like(d2)
        for q in range(kernels):
            k += torch.exp(-d2 / (bw * mul ** (q - kernels // 2)))
        k.fill_diagonal_(0.0)
        mmd2 = k[:n, :n].sum() / (n * (n - 1)) + k[n:, n:].sum() / (m * (m - 1)) - 2.0 * k[:n, n:].sum() / (n * m)
    return torch.stack([mmd2, bw, xx / (n * (n - 1)), yy / (m * (m - 1)), xy / (n * m)])


def mmd2_reference(x: torch.Tensor, y: torch.Tensor, kernels: int = 5, mul: float = 2.0, bandwidth: Optional[float] = None) -> torch.Tensor:
    """The definition in plain torch fp64 (module docstring): five fp64 numbers, ``FIELDS``."""
    if x.dim() < 1 or y.dim() < 1 or x.size(0) < 2 or y.size(0) < 2:
        raise ValueError(f"mmd2: two sets of at least 2 rows, got {tuple(x.shape)} and {tuple(y.shape)}")
    x, y = x.double().reshape(x.size(0), -1), y.double().reshape(y.size(0), -1)
    if x.size(1) != y.size(1) or x.size(1) < 1:
        raise ValueError(f"mmd2: rows of {x.size(1)} and of {y.size(1)} values")
    Zc = torch.cat([x, y]) - x.mean(dim=0)
    return mmd2_from_gram(Zc @ Zc.t(), x.size(0), y.size(0), kernels, mul, bandwidth)


def as_rows(t: torch.Tensor) -> torch.Tensor:
    """``t [n, ...]`` as the fp32 matrix ``[n, D]`` the kernels take (unit column stride, rows that do not overlap, a 16-byte
    aligned start): a view where it is one, a copy where it is not."""
    if t.dim() < 1 or t.size(0) < 1 or t.numel() == 0:
        raise ValueError(f"transfer monitor: a set needs rows and columns, got {tuple(t.shape)}")
    t = t.detach()
    if t.dtype != torch.float32:
        raise TypeError(f"transfer monitor: fp32 sets, got {t.dtype}")
    r = t if t.dim() == 2 else t.reshape(t.size(0), -1)
    D = r.size(1)
    if (D > 1 and r.stride(1) != 1) or (r.size(0) > 1 and r.stride(0) < D) or r.data_ptr() % 16:
        r = torch.empty(r.shape, device=r.device, dtype=r.dtype).copy_(r)
    return r


@torch.no_grad()
def pooled_gram(sets: Sequence[torch.Tensor]) -> torch.Tensor:
    """The Gram of the pooled rows of ``sets`` (matrices of ``as_rows``) about the column mean of ``sets[0]``: ``ops.mmd_gram``; in
    ``FST_MATH=f32`` the exact-f32 ``ops.gemm_f32`` on explicitly centred copies."""
    c = ops.mmd_centre(sets[0])
    if ops.MATH == "bf16x3":
        return ops.mmd_gram(sets, c)
    Zc = torch.cat([s - c for s in sets])
    return ops.gemm_f32(Zc, False, Zc, False)


@torch.no_grad()
def mmd2(x: torch.Tensor, y: torch.Tensor, kernels: int = 5, mul: float = 2.0, bandwidth: Optional[float] = None) -> torch.Tensor:
    """``mmd2_reference`` on the device for any two fp32 device tensors ``x [n, ...]``, ``y [m, ...]`` (``n + m <= 1024``): three
    launch sets and no host read; the five numbers (``FIELDS``) as a device fp64 tensor."""
    kernels, mul, bandwidth = check_settings(kernels, mul, bandwidth)
    sets = [as_rows(x), as_rows(y)]
    dev = sets[0].device
    out = torch.empty(1, 5, dtype=torch.float64, device=dev)
    word = None if bandwidth is None else torch.tensor([bandwidth], dtype=torch.float64).to(dev, non_blocking=True)
    ops.mmd_fold(pooled_gram(sets), [s.size(0) for s in sets], [(0, 1)], kernels, mul, out, torch.zeros_like(out),
                 torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), bandwidth=word)
    return out[0]


class TransferMonitor:
    """The device words of a trainer's monitor and the launches of one measurement.  ``sums`` fp64 [4, 5] and ``counts`` int32 [4]:
    the running sums per pair of ``PAIRS`` and how many measurements each holds; ``nonfinite`` int32 [1]: measurements whose
    ``mmd2`` was not finite (they are in no sum); ``word`` fp64 [1]: the bandwidth that replaces the mean-distance one while
    positive.  The addresses never change: captured launches name them."""

    def __init__(self, device, kernels: int = 5, mul: float = 2.0, bandwidth: Optional[float] = None):
        self.kernels, self.mul, bandwidth = check_settings(kernels, mul, bandwidth)
        P = len(PAIRS)
        self.sums = torch.zeros(P, 5, dtype=torch.float64, device=device)
        self.counts = torch.zeros(P, dtype=torch.int32, device=device)
        self.nonfinite = torch.zeros(1, dtype=torch.int32, device=device)
        self.word = torch.zeros(1, dtype=torch.float64, device=device)
        self.bandwidth: Optional[float] = None
        self.set_bandwidth(bandwidth)

    def set_bandwidth(self, bandwidth: Optional[float]) -> bool:
        """One stream-ordered copy into the device word (None: back to the mean-distance bandwidth).  Returns whether it changed."""
        _, _, bandwidth = check_settings(self.kernels, self.mul, bandwidth)
        if bandwidth == self.bandwidth:
            return False
        self.bandwidth = bandwidth
        self.word.copy_(torch.tensor([0.0 if bandwidth is None else bandwidth], dtype=torch.float64), non_blocking=True)
        return True

    def reset(self) -> None:
        self.sums.zero_(); self.counts.zero_(); self.nonfinite.zero_()

    def mean(self) -> torch.Tensor:
        """fp64 [4, 5]: the running sums over their counts (NaN for a pair that holds no measurement)."""
        n = self.counts.to(torch.float64)[:, None]
        return torch.where(n > 0, self.sums / n, torch.full_like(self.sums, float("nan")))

    @torch.no_grad()
    def measure(self, feature_sets: Sequence[torch.Tensor], hidden_sets: Sequence[torch.Tensor]) -> torch.Tensor:
        """One measurement: a Gram over (target, source-to-target, source) features and one over the (source, t2s, s2t2s) hidden
        vectors, each about the mean of its first set, and one fold each for its two pairs against that first set.  Returns a
        fresh fp64 [4, 5] tensor, rows in ``PAIRS`` order; the finite pairs join the running sums."""
        out = torch.empty(len(PAIRS), 5, dtype=torch.float64, device=self.sums.device)
        for base, group in ((0, feature_sets), (2, hidden_sets)):
            sets = [as_rows(t) for t in group]
            ops.mmd_fold(pooled_gram(sets), [s.size(0) for s in sets], [(0, 1), (0, 2)], self.kernels, self.mul, out[base: base + 2],
                         self.sums[base: base + 2], self.counts[base: base + 2], self.nonfinite, bandwidth=self.word)
        return out

    def state_dict(self) -> dict:
        return {"kernels": self.kernels, "mul": self.mul, "bandwidth": self.bandwidth, "sums": self.sums.detach().cpu().clone(),
                "counts": self.counts.detach().cpu().clone(), "nonfinite": self.nonfinite.detach().cpu().clone()}

    def load_state_dict(self, sd: dict) -> None:
        """Sums, counts and the bandwidth, in place (``kernels`` and ``mul`` ride by value in the launches: the owner sets them)."""
        self.sums.copy_(sd["sums"]); self.counts.copy_(sd["counts"]); self.nonfinite.copy_(sd["nonfinite"])
        self.set_bandwidth(sd["bandwidth"])


class _TransferMonitoring(_Mode):
    """The transfer monitor of the joint trainer.  The trainer calls ``_transfer_measure`` on the detached tensors of a step's
    report, behind ``forward_losses``."""
    transfer_monitor: Optional[TransferMonitor] = None                        # the device words; None while the mode is off

    def enable_transfer_monitor(self, kernels: int = 5, mul: float = 2.0, bandwidth: Optional[float] = None) -> None:
        """From now on every joint step measures how far the transferred features are from where they should be: the multi-kernel
        MMD² (``monitor.mmd2_reference`` is the definition; ``kernels`` Gaussians whose bandwidths are the mean pairwise squared
        distance times ``mul^(q - kernels // 2)``, or ``bandwidth`` in its place) for the pairs ``monitor.PAIRS`` — in feature space
        ``[B, C·L]`` target against source-to-target and against source features, in the source classifier's hidden space source
        against t2s and against s2t2s vectors.  Two Gram launches and two folds on the detached tensors of ``forward_losses``, on the
        device with no host read, in ``step`` and ``capture`` / ``replay`` (captured into the joint graph); under gradient
        accumulation every micro-step measures its own batch; under data parallelism the values are this rank's (no collective); a
        step the anomaly guard skips still reports, and joins the running sums if its numbers are finite.  ``phase_step`` and
        ``replay_phase`` have no source-to-target features and ignore the mode.  The monitor only reads: losses, gradients and
        weights keep the bits of the mode off.

        Every report gains ``"transfer"``: fp64 [4, 5], rows in ``PAIRS`` order, columns ``monitor.FIELDS``, and the four tensors of
        ``aux`` that only the monitor reads (``TRANSFER_AUX``: ``"feat_s"``, ``"pool_s"``, ``"tr_t"``, ``"tr_s2t"``), detached.  ``transfer_mean()``
        gives the means since ``reset_transfer_monitor()``; ``set_transfer_bandwidth`` steers a resident capture.  Both batches need
        at least 2 rows and three of them at most 1024 together.  A second call sets its arguments; raises while a joint or phase
        capture is resident if that would switch the mode on or change ``kernels`` / ``mul``, which captured launches hold by value."""
        kernels, mul, bandwidth = check_settings(kernels, mul, bandwidth)
        mon = self.transfer_monitor
        if mon is None:
            self._refuse_resident("enable_transfer_monitor()")
            self.transfer_monitor = TransferMonitor(self.device, kernels, mul, bandwidth)
            return
        if (kernels, mul) != (mon.kernels, mon.mul):
            self._refuse_resident("enable_transfer_monitor()")
            mon.kernels, mon.mul = kernels, mul
        mon.set_bandwidth(bandwidth)

    def _transfer_on(self, what: str) -> TransferMonitor:
        if self.transfer_monitor is None:
            raise RuntimeError(f"{what}: call enable_transfer_monitor() first")
        return self.transfer_monitor

    def set_transfer_bandwidth(self, bandwidth: Optional[float]) -> bool:
        """A fixed bandwidth for every pair (None: each pair's own mean pairwise squared distance again).  Legal while captures are
        resident: one stream-ordered copy into the device word that a graph replayed afterwards reads — no re-capture.  Returns
        whether the word changed."""
        return self._transfer_on("set_transfer_bandwidth()").set_bandwidth(bandwidth)

    def transfer_mean(self) -> torch.Tensor:
        """fp64 [4, 5] on the device: the means of the finite measurements since the last ``reset_transfer_monitor()`` (rows
        ``PAIRS``, columns ``FIELDS``; NaN where there is none yet)."""
        return self._transfer_on("transfer_mean()").mean()

    def reset_transfer_monitor(self) -> None:
        self._transfer_on("reset_transfer_monitor()").reset()

    def _transfer_measure(self, rep: Dict[str, torch.Tensor]) -> torch.Tensor:
        return self.transfer_monitor.measure((rep["feat_t"], rep["feat_s2t"], rep["feat_s"]), (rep["pool_s"], rep["tr_t"], rep["tr_s2t"]))

    def _transfer_load_state_dict(self, sd: dict) -> None:
        self.enable_transfer_monitor(sd["kernels"], sd["mul"], sd["bandwidth"])
        self.transfer_monitor.load_state_dict(sd)
