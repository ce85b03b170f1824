"""bench.py's command line: a plain run prints the headline line only and `--dump-outputs` writes
the last timed step's disparity; the secondary legs (rooflines, parity against the CPU oracle,
CPU baseline) appear with `--full`."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"}
FULL_KEYS = {"roofline", "kernels", "epe_vs_ref", "max_abs_disp_err_vs_ref", "cpu_baseline"}


def _bench(*argv):
    res = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *argv],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout
    return json.loads(lines[0])


def test_dump_outputs_writes_float32_npy(tmp_path):
    import bench
    t = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4).transpose(1, 2)  # non-contiguous
    bench.dump_outputs(argparse.Namespace(dump_outputs=str(tmp_path / "d")), 0, disp=t)
    a = np.load(tmp_path / "d" / "disp.npy")
    assert a.dtype == np.float32 and a.shape == (2, 4, 3)
    assert np.array_equal(a, t.numpy().astype(np.float32))
    bench.dump_outputs(argparse.Namespace(dump_outputs=None), 0, disp=t)  # off: writes nothing
    assert sorted(os.listdir(tmp_path)) == ["d"]


@pytest.mark.gpu
def test_plain_run_prints_headline_only_and_dumps_disparity(tmp_path):
    line = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2",
                  "--dump-outputs", str(tmp_path))
    assert HEADLINE_KEYS <= set(line) and not FULL_KEYS & set(line)
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(2 * 1000.0 / line["ms_per_step"])  # pairs per step / time
    assert os.listdir(tmp_path) == ["disp.npy"]
    disp = np.load(tmp_path / "disp.npy")
    assert disp.dtype == np.float32 and disp.shape == (2, 128, 416)
    assert np.isfinite(disp).all() and disp.min() >= 0 and disp.max() <= 63


@pytest.mark.gpu
def test_full_run_adds_the_secondary_legs():
    line = _bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "1", "--full",
                  "--no-cpu-baseline", "--kernel-iters", "2")
    assert HEADLINE_KEYS <= set(line) and FULL_KEYS - {"cpu_baseline"} <= set(line)
    assert line["max_abs_disp_err_vs_ref"] <= 1e-3  # the hot path's bar against the oracle (smoke())
    assert line["roofline"]["kernel"] in line["kernels"]
