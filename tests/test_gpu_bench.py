"""bench.py's command line: a plain run prints the headline line only, `--dump-outputs`
writes the last timed step's y (the same bits from run to run), `--steps` sets the number
of timed steps.  Small matrices (4096 rows, two replicas): the checks are about the
benchmark's plumbing, not its figures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--rows-per-rank", "4096", "--replicas", "2"]
FULL_ONLY = ("cpu_baseline", "spmm", "rmat", "config5")


def run_bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    out = tmp_path_factory.mktemp("dump")
    line = run_bench("--steps", "7", "--warmup", "2", "--dump-outputs", str(out))
    return line, np.load(out / "y.npy")


def test_plain_line_and_dump(plain):
    line, y = plain
    assert line["metric"] == "CSR SpMV effective HBM GB/s" and line["unit"] == "GB/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 7 and line["warmup"] == 2
    assert line["ms_per_step"] > 0 and line["value"] > 0
    # value is the algorithmic bytes of one step over ms_per_step (both rounded on the line:
    # value to 0.1, ms_per_step to 1e-5 ms)
    rows = cols = 4096
    alg = 8 * 16 * rows + 4 * (rows + 1) + 4 * cols + 8 * rows
    assert line["value"] == pytest.approx(alg / (line["ms_per_step"] * 1e-3) / 1e9, rel=5e-3, abs=0.06)
    for k in FULL_ONLY:   # a plain run measures the headline only
        assert line.get(k) is None, k
    assert line["roofline"]["distribution"] == {}
    assert y.dtype == np.float32 and y.shape == (4096,) and np.isfinite(y).all()
    assert np.abs(y).max() > 0


def test_dump_is_reproducible(plain, tmp_path):
    _, y = plain
    line = run_bench("--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path))
    again = np.load(tmp_path / "y.npy")
    assert np.array_equal(again.view(np.uint32), y.view(np.uint32))
    assert sorted(os.listdir(tmp_path)) == ["y.npy"]
    assert line["steps"] == 7
