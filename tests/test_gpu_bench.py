"""bench.py's plain run: the headline line only, and --dump-outputs writes what the last timed step computed — checked here
against the CPU oracle on the same inputs (the small configs[0] workload: a fresh child process, seconds)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_plain_run_dumps_the_timed_outputs(tmp_path):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--workload", "ks_50x2_T100_N1", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=str(ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["unit"] == "JVPs/s" and line["dtype"] == "f64"
    assert not {"roofline", "sweeps_ms", "output_check", "cpu_baseline", "extra"} & set(line)
    agg, dagg = np.load(tmp_path / "out" / "agg.npy"), np.load(tmp_path / "out" / "dagg.npy")
    P, N = 99, 1
    assert agg.shape == (P,) and dagg.shape == (P, N) and agg.dtype == dagg.dtype == np.float64

    sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
    import bench
    from conftest import ks_paths
    m, ss = bench.load_or_solve_ss(50, 2, 100)
    x, _ = ks_paths(m, ss, "x1", 0.01)
    dx = np.random.default_rng(1000).standard_normal(2 * P * N).reshape((2, P, N), order="F")   # rank 0's tangents
    chk = bench.check_timed_output(m, ss, x, dx, agg, dagg)
    assert chk["oracle_status"] == 0, chk
    assert chk["agg_max_rel_err"] < chk["tolerance"] and chk["dagg_col0_max_rel_err"] < chk["tolerance"], chk
