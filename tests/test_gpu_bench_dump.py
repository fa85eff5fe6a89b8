"""bench.py on one GPU at a small shape: --steps sets the number of timed steps, ms_per_step is one of them, a run without
--full carries no extra leg, and --dump-outputs writes the last timed step's report as float32 / float64 .npy files within
64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_steps_and_dump_outputs(tmp_path):
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "16",
           "--length", "128", "--plain", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    # without --full the run stops at the headline: no roofline step, no S1 / north-star / f32 / CPU legs
    assert not {"roofline", "s1_classifier_step", "north_star_extras", "f32_mode", "cpu_baseline", "gpu_over_cpu"} & set(d)
    assert abs(d["value"] - 16 * 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"]
    files = sorted(os.listdir(out_dir))
    assert {"ce_t.npy", "nf_t.npy", "cdan.npy", "w_t.npy", "feat_t.npy", "logit_t.npy"} <= set(files)
    assert d["dumped_outputs"]["arrays"] == len(files) and not d["dumped_outputs"]["sampled"]
    assert sum(os.path.getsize(out_dir / f) for f in files) <= 64_000_000
    for f in files:
        a = np.load(out_dir / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
    assert np.load(out_dir / "feat_t.npy").shape[0] == 16
    assert abs(float(np.load(out_dir / "ce_t.npy")) - d["losses"]["ce_t"]) <= 1e-6 * max(1.0, abs(d["losses"]["ce_t"]))
