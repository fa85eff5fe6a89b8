"""Input pipeline of the reference without sktime (DataSource.py:9-68, train_and_test.py:134-137).

``load_ts`` parses the UCR/UEA ``.ts`` text format into what ``sktime.datasets.load_from_tsfile(...,
return_data_type="numpy3d")`` hands the reference: a float64 array ``[N, C, L]`` and an array of label strings.
``TrainData`` / ``TestData`` keep the reference's constructor signature, attributes and label-dictionary semantics,
including its quirks: the dictionary is shared and mutated by the training set (labels numbered in order of first
appearance), ``num_class`` counts only the labels THIS dataset added, the test set never adds labels (an unseen one is
reported and its sample gets no label) and its ``num_class`` stays 0.

Parity note: the file format itself is restated from its public description (sktime is not in the image, so the
parser has no reference-generated vectors: "parity unpinned" for ``load_ts``); the dataset classes are pinned by
``tests/golden/datasource_small.npz``, produced by the REFERENCE's classes running on top of this parser.

``DeviceLoader`` is the H2D side: batches are cast to float32, staged in pinned memory and copied on a side stream one
batch ahead, so the step never waits for the host at B=256.

``DeviceDataset`` / ``EpochFeeder`` take the host out of the per-step path altogether: the set is uploaded once, an epoch's
permutations, CPC indices and ratios are planned once and uploaded with one copy, and every batch is gathered on the device
(``ops.feed_batch``, csrc/feed.hip) at a plan position kept in a device word.

``EvalPlan`` is the evaluation's counterpart: one sequential plan over a resident set, built once, whose last batch is padded to
the static shape and comes with its count of valid rows (``evaluate.Evaluator`` serves its captured passes from it).
"""
from __future__ import annotations

import os
from typing import Dict, Iterator, List, Optional, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset


class TsFormatError(ValueError):
    pass


def load_ts(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """Parse an equal-length ``.ts`` file -> (x float64 [N, C, L], y str [N]).  ``?`` is a missing value (NaN).
    Dimensions of a case are separated by ``:``, values by ``,``, the class label is the last ``:`` field."""
    with open(path, "r", encoding="utf-8") as f:
        return parse_ts(f.read(), where=path)


def parse_ts(text: str, where: str = "<string>") -> Tuple[np.ndarray, np.ndarray]:
    has_labels, in_data, timestamps = None, False, False
    cases: List[List[np.ndarray]] = []
    labels: List[str] = []
    for ln, raw in enumerate(text.splitlines(), 1):
        line = raw.strip()
        if not line or line.startswith("#"):
            continue
        if not in_data:
            low = line.lower()
            if low.startswith("@data"):
                in_data = True
                if has_labels is None:
                    raise TsFormatError(f"{where}:{ln}: @data before @classLabel")
            elif low.startswith("@classlabel"):
                tok = line.split()
                if len(tok) < 2 or tok[1].lower() not in ("true", "false"):
                    raise TsFormatError(f"{where}:{ln}: malformed @classLabel")
                has_labels = tok[1].lower() == "true"
            elif low.startswith("@timestamps"):
                timestamps = line.split()[-1].lower() == "true"
            elif not low.startswith("@"):
                raise TsFormatError(f"{where}:{ln}: expected a header line starting with '@'")
            continue
        if timestamps:
            raise TsFormatError(f"{where}: time-stamped .ts files are not supported")
        fields = line.split(":")
        if has_labels:
            if len(fields) < 2:
                raise TsFormatError(f"{where}:{ln}: case without a class label")
            labels.append(fields[-1].strip())
            fields = fields[:-1]
        dims = []
        for d in fields:
            vals = [v.strip() for v in d.split(",")]
            try:
                dims.append(np.array([np.nan if v == "?" else float(v) for v in vals], dtype=np.float64))
            except ValueError as e:
                raise TsFormatError(f"{where}:{ln}: {e}") from None
        cases.append(dims)
    if not in_data or not cases:
        raise TsFormatError(f"{where}: no @data section / no cases")
    C, L = len(cases[0]), len(cases[0][0])
    for i, dims in enumerate(cases):
        if len(dims) != C or any(len(v) != L for v in dims):
            raise TsFormatError(f"{where}: case {i} is not {C} x {L} (numpy3d needs equal dimensions and lengths)")
    x = np.stack([np.stack(dims) for dims in cases])
    return x, np.array(labels if has_labels else [""] * len(cases))


class TrainData(Dataset):
    """DataSource.py:9-36 — ``temp_dict`` is filled in place, in order of first appearance."""

    def __init__(self, file_path_begin, file_path_end, temp_dict: Dict[str, int]):
        super().__init__()
        train_x, train_y = load_ts(os.path.join(file_path_begin, file_path_end))
        self.len = train_x.shape[0]
        self.in_channel = train_x.shape[1]
        self.time_length = train_x.shape[-1]
        self.train_x = torch.from_numpy(train_x)                       # float64 like the reference; cast at use (:151)
        label, class_label = [], 0
        for i in train_y:
            if i not in temp_dict:
                temp_dict[i] = class_label
                class_label += 1
            label.append(temp_dict[i])
        self.num_class = class_label                                   # only the labels added here (reference quirk)
        self.train_y = torch.tensor(label).long()

    def __len__(self):
        return self.len

    def __getitem__(self, idx):
        return self.train_x[idx, :, :], self.train_y[idx]


class TestData(Dataset):
    """DataSource.py:38-64 — never adds labels; an unseen one is reported and skipped; ``num_class`` stays 0."""

    def __init__(self, file_path_begin, file_path_end, temp_dict: Dict[str, int]):
        super().__init__()
        test_x, test_y = load_ts(os.path.join(file_path_begin, file_path_end))
        self.len = test_x.shape[0]
        self.in_channel = test_x.shape[1]
        self.time_length = test_x.shape[-1]
        self.test_x = torch.from_numpy(test_x)
        label = []
        self.unseen_labels: List[str] = []
        for i in test_y:
            if i in temp_dict:
                label.append(temp_dict[i])
            else:
                self.unseen_labels.append(str(i))
                print("label of the test set missing from the training set: stop the training", i)
        self.num_class = 0
        self.test_y = torch.tensor(label).long()

    def __len__(self):
        return self.len

    def __getitem__(self, idx):
        return self.test_x[idx, :, :], self.test_y[idx]


class DeviceLoader:
    """Iterate (x float32 on device, y on device) batches with the next batch's host->device copy in flight:
    float32 cast and pinning on the host, ``non_blocking`` copies on a side stream, an event per batch so the consumer
    stream waits only for its own batch.  Order is the dataset's unless ``generator`` is given (then a permutation
    per epoch, like ``DataLoader(shuffle=True)``)."""

    def __init__(self, x: torch.Tensor, y: torch.Tensor, batch_size: int, device, generator: Optional[torch.Generator] = None,
                 drop_last: bool = False):
        if x.size(0) != y.size(0):
            raise ValueError(f"{x.size(0)} series but {y.size(0)} labels")
        self.device = torch.device(device)
        pin = self.device.type == "cuda"
        self.x = x.to(torch.float32).contiguous()
        self.y = y.contiguous()
        if pin:
            self.x, self.y = self.x.pin_memory(), self.y.pin_memory()
        self.batch_size, self.generator, self.drop_last = batch_size, generator, drop_last
        self._copy = torch.cuda.Stream(self.device) if pin else None

    def __len__(self) -> int:
        n = self.x.size(0)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _stage(self, idx):
        if self._copy is None:
            return self.x[idx], self.y[idx], None
        # gather on the host into fresh pinned buffers (index_select output is not pinned), then async copy
        xb = torch.empty((len(idx),) + tuple(self.x.shape[1:]), dtype=torch.float32).pin_memory()
        yb = torch.empty((len(idx),) + tuple(self.y.shape[1:]), dtype=self.y.dtype).pin_memory()
        torch.index_select(self.x, 0, idx, out=xb)
        torch.index_select(self.y, 0, idx, out=yb)
        with torch.cuda.stream(self._copy):
            xd, yd = xb.to(self.device, non_blocking=True), yb.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._copy)
        return xd, yd, (ev, xb, yb)                                  # keep the pinned buffers alive until consumed

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        n = self.x.size(0)
        order = torch.randperm(n, generator=self.generator) if self.generator is not None else torch.arange(n)
        chunks = [order[i: i + self.batch_size] for i in range(0, n, self.batch_size)]
        if self.drop_last and chunks and len(chunks[-1]) < self.batch_size:
            chunks.pop()
        nxt = self._stage(chunks[0]) if chunks else None
        for i in range(len(chunks)):
            cur = nxt
            nxt = self._stage(chunks[i + 1]) if i + 1 < len(chunks) else None
            xd, yd, hold = cur
            if hold is not None:
                torch.cuda.current_stream(self.device).wait_event(hold[0])
                xd.record_stream(torch.cuda.current_stream(self.device))
                yd.record_stream(torch.cuda.current_stream(self.device))
            yield xd, yd


class DeviceDataset:
    """A whole data set resident on the device: ``x`` [N, C, L] of any float dtype as ONE contiguous fp32 tensor (the reference's
    ``.float()``, train_and_test.py:151, applied once at upload as ``DeviceLoader`` applies it) and ``y`` as int64.  The
    reference's sets are a few MB to a few hundred MB: nothing forces them across PCIe once per step."""

    def __init__(self, x: torch.Tensor, y: torch.Tensor, device):
        if x.size(0) != y.size(0):
            raise ValueError(f"{x.size(0)} series but {y.size(0)} labels")
        if x.size(0) < 1:
            raise ValueError("an empty data set")
        self.device = torch.device(device)
        self.x = x.to(torch.float32).contiguous().to(self.device)
        self.y = y.to(torch.int64).contiguous().to(self.device)

    def __len__(self) -> int:
        return self.x.size(0)

    def batches(self, batch_size: int) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        """Contiguous views in data-set order, the last partial one included: evaluation over a resident set copies nothing."""
        if batch_size < 1:
            raise ValueError(f"batch_size {batch_size}")
        for i in range(0, len(self), batch_size):
            yield self.x[i: i + batch_size], self.y[i: i + batch_size]


class EpochFeeder:
    """Plans a whole epoch on the host, uploads the plan once and then serves every step's batch from device memory
    (``ops.feed_batch``), the plan's current row a device word: per step the host issues one launch pair and touches no tensor.

    ``target`` / ``source``: ``DeviceDataset``s (``source=None``: a target-only feeder, for ``ClassifierTrainer``).  ``batch_size``:
    one int or ``(B_t, B_s)``.  ``begin_epoch`` draws from ``generator`` (the global CPU generator if None) in this fixed order:
    ``randperm(N_t)``; ``randperm(N_s)`` if there is a source; ``randint(cpc_timestep // 2, (rounds, 2))`` if ``cpc_timestep`` (the
    CPC module's ``timestep``, L_t // 2) is given.  With ``shuffle=False`` the orders are ``arange`` and only the CPC indices are
    drawn.  ``rounds = min(N_t // (world·B_t), N_s // (world·B_s))``: full batches only (graph shapes are static), the tail of a
    permutation dropped as ``DeviceLoader(drop_last=True)`` drops it, the number of rounds the reference's ``min``
    (train_and_test.py:538).  Rank ``r`` of ``world`` takes slice ``[r·B, (r+1)·B)`` of every global batch of ``world·B``.
    For the same generator state the batches of an epoch are bit-equal to ``DeviceLoader(x, y, B, device, generator,
    drop_last=True)``'s."""

    SCALARS = 4                                                               # columns of the scalar table: t_t, t_s (int32), r_t, r_s (fp32)

    def __init__(self, target: DeviceDataset, source: Optional[DeviceDataset] = None, batch_size=1,
                 generator: Optional[torch.Generator] = None, shuffle: bool = True, cpc_timestep: Optional[int] = None,
                 rank: int = 0, world: int = 1):
        sizes = tuple(batch_size) if isinstance(batch_size, (tuple, list)) else (batch_size, batch_size)
        if len(sizes) != 2 or any(isinstance(b, bool) or not isinstance(b, int) or b < 1 for b in sizes):
            raise ValueError(f"batch_size must be a positive int or a pair of them, got {batch_size!r}")
        if not 0 <= rank < world:
            raise ValueError(f"rank {rank} of world {world}")
        if source is not None and source.device != target.device:
            raise ValueError(f"the target set lives on {target.device}, the source set on {source.device}")
        if cpc_timestep is not None and cpc_timestep < 1:
            raise ValueError(f"cpc_timestep {cpc_timestep}")
        self.target, self.source, self.device = target, source, target.device
        self.batch = sizes if source is not None else sizes[:1]
        self.generator, self.shuffle, self.cpc_timestep, self.rank, self.world = generator, shuffle, cpc_timestep, rank, world
        self.sets = (target,) if source is None else (target, source)
        self.rounds = min(len(d) // (world * b) for d, b in zip(self.sets, self.batch))
        self.epoch = 0                                                        # epochs begun
        self.cursor = 0                                                       # host mirror of the device cursor
        self.steps = 0                                                        # rows of the current plan (0: no epoch begun)
        self.state = torch.zeros(8, dtype=torch.int32, device=self.device)    # fst_feed_batch's state block
        if self.state.data_ptr() % 16:
            raise RuntimeError("EpochFeeder: the allocator returned a block off a 16-byte boundary")
        self._host: Optional[torch.Tensor] = None                             # the current plan's tables, int32, as uploaded
        self._plan: Optional[torch.Tensor] = None                             # ... on the device
        self._sink = torch.zeros(self.SCALARS, dtype=torch.int32, device=self.device)   # scalars nobody asked for
        self._calls: Dict[tuple, object] = {}

    def _gen(self) -> torch.Generator:
        return torch.default_generator if self.generator is None else self.generator

    def _words(self) -> int:
        return self.rounds * (sum(self.batch) + self.SCALARS)

    def _upload(self, host: torch.Tensor, head: torch.Tensor) -> None:
        """The tables in one host-to-device copy, the state words in a second one of 32 bytes; neither waits for the device."""
        if self.device.type == "cuda":
            host, head = host.pin_memory(), head.pin_memory()
        self._host = host
        if self._plan is None or self._plan.numel() != host.numel():
            self._plan = torch.empty(host.numel(), dtype=torch.int32, device=self.device)
            self._calls = {}
        self._plan.copy_(host, non_blocking=True)
        self.state[: head.numel()].copy_(head, non_blocking=True)

    def _tables(self):
        """Views of the device plan: one index table per data set, then the scalars."""
        out, at = [], 0
        for b in self.batch:
            out.append(self._plan[at: at + self.rounds * b].view(self.rounds, b))
            at += self.rounds * b
        return out, self._plan[at:].view(self.rounds, self.SCALARS)

    def begin_epoch(self, ratios=None) -> int:
        """Plan and upload the next epoch; returns its number of rounds.  ``ratios``: optional ``[rounds, 2]`` NoiseTransfer
        accumulation ratios, rounded to float32 here.  Resets the cursor; the counters ``fed``, ``overrun`` and ``bad_index`` run on."""
        gen, R, W = self._gen(), self.rounds, self.world
        parts = []
        for d, b in zip(self.sets, self.batch):
            order = torch.randperm(len(d), generator=gen) if self.shuffle else torch.arange(len(d))
            parts.append(order[: R * W * b].view(R, W, b)[:, self.rank].to(torch.int32).reshape(-1))
        scal = torch.zeros(R, self.SCALARS, dtype=torch.int32)
        if self.cpc_timestep is not None:
            scal[:, :2] = torch.randint(max(1, self.cpc_timestep // 2), (R, 2), generator=gen).to(torch.int32)
        r32 = torch.ones(R, 2, dtype=torch.float32)
        if ratios is not None:
            r32 = torch.as_tensor(ratios, dtype=torch.float64).reshape(-1, 2).to(torch.float32)
            if r32.size(0) != R:
                raise ValueError(f"begin_epoch(): {r32.size(0)} rows of ratios for {R} rounds")
        scal[:, 2:] = r32.contiguous().view(torch.int32)
        self.epoch += 1
        self.cursor, self.steps = 0, R
        self._upload(torch.cat(parts + [scal.reshape(-1)]), torch.tensor([0, R], dtype=torch.int32))
        return R

    def _need_epoch(self, what: str) -> None:
        if self._plan is None:
            raise RuntimeError(f"{what}: no epoch is planned; call begin_epoch() first")

    def feed(self, *dst: torch.Tensor, t: Optional[torch.Tensor] = None, r: Optional[torch.Tensor] = None) -> None:
        """Serve the current round into ``dst`` — (x_t, y_t) or (x_t, y_t, x_s, y_s), device tensors of the batch shapes — and the
        round's scalars into ``t`` (int32 [2]: the CPC start indices) and ``r`` (fp32 [2]: the ratios) where given; then move on.
        Two launches on the current stream.  Raises ``StopIteration`` before any launch once the epoch is over."""
        self._need_epoch("feed()")
        if self.cursor >= self.steps:
            raise StopIteration
        key = tuple(d.data_ptr() for d in dst) + (None if t is None else t.data_ptr(), None if r is None else r.data_ptr())
        call = self._calls.get(key)
        if call is None:
            from . import ops
            if len(dst) != 2 * len(self.sets):
                raise ValueError(f"feed(): {len(dst)} destinations for {len(self.sets)} data sets (x and y each)")
            for name, v, dt in (("t", t, torch.int32), ("r", r, torch.float32)):
                if v is not None and (v.dtype != dt or v.numel() != 2 or not v.is_contiguous()):
                    raise ValueError(f"feed(): {name} must be two contiguous {dt} words")
            index, scal = self._tables()
            streams = []
            for i, d in enumerate(self.sets):
                streams += [(d.x, dst[2 * i], index[i]), (d.y, dst[2 * i + 1], index[i])]
            words = [self._sink[k: k + 1] for k in range(self.SCALARS)]
            if t is not None:
                words[0], words[1] = t.view(-1)[0:1], t.view(-1)[1:2]
            if r is not None:
                words[2], words[3] = r.view(-1)[0:1], r.view(-1)[1:2]
            call = self._calls[key] = ops.FeedCall(streams, [(scal, w) for w in words], self.state)
        call()
        self.cursor += 1

    def peek(self):
        """Row 0 of the current plan as fresh tensors, nothing moved: (x_t, y_t[, x_s, y_s], t int32 [2], r fp32 [2]) — the batch to
        hand to ``capture(...)``."""
        self._need_epoch("peek()")
        if self.steps < 1:
            raise RuntimeError("peek(): the plan has no rounds")
        index, scal = self._tables()
        out = []
        for d, idx in zip(self.sets, index):
            rows = idx[0].long()
            out += [d.x.index_select(0, rows), d.y.index_select(0, rows)]
        return (*out, scal[0, :2].clone(), scal[0, 2:].view(torch.float32).clone())

    def counters(self) -> torch.Tensor:
        """The state block on the device (``ops.FEED_CURSOR`` ... ``ops.FEED_BAD_INDEX``); no host read."""
        return self.state

    def check(self) -> None:
        """Read the state block once (this waits for the device: for the end of an epoch) and raise if a call ran past the plan's
        end or a row's index fell outside its data set."""
        from . import ops
        words = self.state.cpu()
        over, bad = int(words[ops.FEED_OVERRUN]), int(words[ops.FEED_BAD_INDEX])
        if over or bad:
            raise RuntimeError(f"EpochFeeder: {over} calls past the end of a plan, {bad} rows with an index outside their data set")

    def state_dict(self) -> dict:
        """Generator state, epoch number, cursor and the current plan's tables: a run resumed mid-epoch feeds the same remaining
        batches.  Reads the counters back (waits for the device)."""
        return {"generator": self._gen().get_state().clone(), "epoch": self.epoch, "cursor": self.cursor, "steps": self.steps,
                "batch": tuple(self.batch), "rank": self.rank, "world": self.world,
                "table": None if self._host is None else self._host.clone(), "counters": self.state.cpu().clone()}

    def load_state_dict(self, sd: dict) -> None:
        if tuple(sd["batch"]) != tuple(self.batch) or (sd["rank"], sd["world"]) != (self.rank, self.world):
            raise ValueError(f"EpochFeeder: the checkpoint was planned for batch {tuple(sd['batch'])}, rank {sd['rank']} of "
                             f"{sd['world']}; this feeder has batch {tuple(self.batch)}, rank {self.rank} of {self.world}")
        if sd["table"] is not None and (sd["steps"] != self.rounds or sd["table"].numel() != self._words()):
            raise ValueError("EpochFeeder: the checkpoint's plan does not fit this feeder's data sets")
        self._gen().set_state(sd["generator"])
        self.epoch, self.cursor, self.steps = sd["epoch"], sd["cursor"], sd["steps"]
        head = sd["counters"].to(torch.int32).clone()
        head[0], head[1] = self.cursor, self.steps
        if sd["table"] is None:
            self._host = self._plan = None
            self._calls = {}
            self.state.copy_(head)
        else:
            self._upload(sd["table"].to(torch.int32).clone(), head)


class EvalPlan:
    """A sequential plan over ONE ``DeviceDataset`` for evaluation, built and uploaded once at construction (one host-to-device
    copy), not per epoch: ``rounds = ceil(N / B)`` rows of ``B`` indices holding ``arange(N)``, the last row padded with index
    ``N - 1`` (a valid index: ``bad_index`` stays 0, and the padding rows hold finite data), and one scalar column with each round's
    count of valid rows.  ``feed`` serves the current round through the unchanged ``ops.FeedCall`` (``fst_feed_batch``): ``x`` and
    ``y`` into the caller's static inputs, the count into the word that ``ops.eval_fold`` reads.  ``rewind`` resets the cursor from
    a resident device word: a device-to-device copy of four bytes that a captured graph can hold.  The host keeps no mirror of the
    cursor, so a call past the end is not refused here but counted in ``overrun`` on the device (``check``).

    ``rank`` / ``world`` slicing is out of scope: a data-parallel user evaluates on rank 0."""

    def __init__(self, data: DeviceDataset, batch_size: int):
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
            raise ValueError(f"batch_size must be a positive int, got {batch_size!r}")
        N, B = len(data), batch_size
        self.data, self.device, self.batch, self.n = data, data.device, B, N
        self.rounds = R = (N + B - 1) // B
        if R * B >= 1 << 31:
            raise ValueError(f"EvalPlan: {R} rounds of {B} rows exceed int32 indices")
        host = torch.zeros(16 + R * B + R, dtype=torch.int32)
        host[1] = R                                                           # ops.FEED_STEPS; words 0..7: fst_feed_batch's state block
        host[16: 16 + R * B] = torch.arange(R * B, dtype=torch.int32).clamp_(max=N - 1)      # (words 8..15: the cursor's home, zero)
        host[16 + R * B:] = (N - torch.arange(R, dtype=torch.int64) * B).clamp_(max=B).to(torch.int32)
        if self.device.type == "cuda":
            host = host.pin_memory()
        self._host = host
        self._words = torch.empty(host.numel(), dtype=torch.int32, device=self.device)
        self._words.copy_(host, non_blocking=True)
        self.state = self._words[:8]
        if self.state.data_ptr() % 16:
            raise RuntimeError("EvalPlan: the allocator returned a block off a 16-byte boundary")
        self._home = self._words[8:9]
        self.index = self._words[16: 16 + R * B].view(R, B)
        self.valid = self._words[16 + R * B:].view(R, 1)
        self._calls: Dict[tuple, object] = {}

    def __len__(self) -> int:
        return self.rounds

    def rewind(self) -> None:
        """Back to round 0; the counters ``fed``, ``overrun`` and ``bad_index`` run on.  One four-byte copy within device memory."""
        self.state[:1].copy_(self._home)

    def feed(self, x: torch.Tensor, y: torch.Tensor, valid: torch.Tensor) -> None:
        """Serve the current round into ``x`` [B, ...], ``y`` [B] and the round's count of valid rows into ``valid`` (one int32 word);
        then move on.  Two launches on the current stream."""
        key = (x.data_ptr(), y.data_ptr(), valid.data_ptr())
        call = self._calls.get(key)
        if call is None:
            from . import ops
            if valid.dtype != torch.int32 or valid.numel() != 1:
                raise ValueError("EvalPlan.feed(): valid must be one int32 word")
            call = self._calls[key] = ops.FeedCall([(self.data.x, x, self.index), (self.data.y, y, self.index)],
                                                   [(self.valid, valid.view(-1))], self.state)
        call()

    def counters(self) -> torch.Tensor:
        """The state block on the device (``ops.FEED_CURSOR`` ... ``ops.FEED_BAD_INDEX``); no host read."""
        return self.state

    def check(self) -> None:
        """Read the state block once (this waits for the device) and raise if a call ran past the plan's end or an index fell
        outside the data set."""
        from . import ops
        words = self.state.cpu()
        over, bad = int(words[ops.FEED_OVERRUN]), int(words[ops.FEED_BAD_INDEX])
        if over or bad:
            raise RuntimeError(f"EvalPlan: {over} calls past the end of the plan, {bad} rows with an index outside the data set")
