"""bench.py itself: a plain run times exactly --steps steps and prints the headline without --full's figures;
--dump-outputs writes the last timed step's results, the same for two runs of the same command."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "roofline_extend", "cpu_baseline", "end_to_end", "kernel_ms_per_launch_isolated", "serial_ms_per_step",
             "secondary_cfg2", "secondary_skewed")


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.syspath_prepend(ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7"])
    a = bench.parse_args()
    assert not a.full and a.dump_outputs is None and a.steps == 7 and a.min_seconds == 0      # one block of exactly 7 steps
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse_args()
    assert a.full and a.dump_outputs == "out"


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--reads", "400000", "--species", "12", "--genomes", "4",
           "--genome-size", "200000", "--steps", "3", "--warmup", "1", "--pipeline", "2"]
    lines = []
    for k in range(2):
        r = subprocess.run(cmd + ["--dump-outputs", str(tmp_path / ("d%d" % k))], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        lines.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    line = lines[0]
    assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
    assert line["timed_region"]["blocks"] == 1 and line["timed_region"]["steps_per_block"] == 3 and line["steps"] == 3
    assert line["ms_per_step"] > 0 and line["concordance"]["st_match"]
    names = sorted(os.listdir(tmp_path / "d0"))
    assert names == ["chosen_allele.npy", "consensus.npy", "counters.npy", "locus_first.npy", "locus_len_sum.npy", "st_called.npy"]
    assert names == sorted(os.listdir(tmp_path / "d1"))
    for n in names:
        a, b = np.load(tmp_path / "d0" / n), np.load(tmp_path / "d1" / n)
        assert a.dtype == np.float64 and np.array_equal(a, b, equal_nan=True), n
    st = np.load(tmp_path / "d0" / "st_called.npy")
    assert st.shape == (4,) and np.isfinite(st).all()          # every planted species called
    chosen = np.load(tmp_path / "d0" / "chosen_allele.npy")
    assert (chosen >= 0).sum() >= 4 * 7 and np.load(tmp_path / "d0" / "consensus.npy").size > 0
