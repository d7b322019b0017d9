"""bench.py's --dump-outputs: what the last timed step computed, written so that two builds can be compared file by file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_fixed_sample(tmp_path):
    """Outputs above DUMP_SAMPLE elements are cut to the same sorted positions in every call; smaller ones are written whole."""
    import bench
    big = [torch.arange(3 * bench.DUMP_SAMPLE // 2, dtype=torch.float64), torch.arange(bench.DUMP_SAMPLE, dtype=torch.float64) * -1]
    small = [torch.ones(3, 5), torch.full((7,), 2.5)]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch.tensor(0.75), {"params": big, "grads": small})
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("loss", "params", "grads")}
    b = {n: np.load(tmp_path / "b" / (n + ".npy")) for n in ("loss", "params", "grads")}
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["loss"].tolist() == [0.75]
    assert a["params"].shape == (bench.DUMP_SAMPLE,) and np.array_equal(a["params"], b["params"])
    assert (a["params"] >= 0).any() and (a["params"] < 0).any()  # drawn over the whole concatenation
    assert np.array_equal(a["grads"], np.concatenate([np.ones(15), np.full(7, 2.5)]).astype(np.float32))


@pytest.mark.gpu
def test_bench_plain_run_and_dump_outputs(cuda, tmp_path):
    """A plain run (no --full) times exactly --steps steps and adds no roofline or CPU baseline; two runs with the same arguments
    dump identical outputs (seeded inputs, deterministic kernels), float32, within 64 MB, and loss.npy is the last step's loss."""
    lines, dumps = [], []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8",
                            "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
        files = sorted(os.listdir(tmp_path / d))
        assert files == ["grads.npy", "loss.npy", "params.npy"], files
        assert sum(os.path.getsize(tmp_path / d / f) for f in files) <= 64 << 20
        dumps.append({f: np.load(tmp_path / d / f) for f in files})
    out = lines[0]
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert abs(out["value"] - 8 * 1e3 / out["ms_per_step"]) < 0.01 * out["value"]
    assert out["roofline"] is None and "cpu_baseline" not in out and "other_kernels" not in out
    for f, v in dumps[0].items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), f
        assert np.array_equal(v, dumps[1][f]), f
    assert abs(float(dumps[0]["loss.npy"][0]) - out["loss_last"]) < 1e-5 * abs(out["loss_last"]) + 1e-5
