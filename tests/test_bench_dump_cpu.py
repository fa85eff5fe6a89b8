"""bench.py --dump-outputs: what the timed step returned, written as .npy files of float32 / float64 within the size budget,
with a sample drawn at the same positions every time when the full set would not fit."""
import os

import numpy as np
import torch

import bench


def _reports():
    g = torch.Generator().manual_seed(5)
    return [{"ce_t": torch.tensor(1.25), "w_t": torch.randn(2, generator=g), "feat_t": torch.randn(4, 50, 64, generator=g),
             "n": torch.tensor([3, 4], dtype=torch.int32), "d": torch.randn(3, dtype=torch.float64, generator=g), "host": 7}]


def _sizes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_writes_every_report_tensor_in_full(tmp_path):
    reps = _reports()
    info = bench.dump_outputs(str(tmp_path), reps)
    assert info["arrays"] == 5 and not info["sampled"]
    assert sorted(os.listdir(tmp_path)) == ["ce_t.npy", "d.npy", "feat_t.npy", "n.npy", "w_t.npy"]
    feat = np.load(tmp_path / "feat_t.npy")
    assert feat.dtype == np.float32 and np.array_equal(feat, reps[0]["feat_t"].numpy())
    assert np.load(tmp_path / "n.npy").dtype == np.float64 and np.load(tmp_path / "d.npy").dtype == np.float64
    assert np.array_equal(np.load(tmp_path / "d.npy"), reps[0]["d"].numpy())


def test_dump_samples_the_same_positions_within_the_budget(tmp_path):
    budget = 16_000
    a, b = tmp_path / "a", tmp_path / "b"
    reps = _reports()
    info = bench.dump_outputs(str(a), reps, budget=budget)
    bench.dump_outputs(str(b), [{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in reps[0].items()}], budget=budget)
    assert info["sampled"] and _sizes(a) <= budget
    feat = np.load(a / "feat_t.npy")
    assert feat.ndim == 1 and 0 < feat.size < reps[0]["feat_t"].numel()
    assert np.isin(feat, reps[0]["feat_t"].numpy()).all()
    for f in os.listdir(a):
        assert np.array_equal(np.load(a / f), np.load(b / f)), f


def test_dump_prefixes_each_pipeline(tmp_path):
    bench.dump_outputs(str(tmp_path), _reports() + _reports())
    names = set(os.listdir(tmp_path))
    assert {"src0.feat_t.npy", "src1.feat_t.npy", "src0.ce_t.npy", "src1.ce_t.npy"} <= names and len(names) == 10
