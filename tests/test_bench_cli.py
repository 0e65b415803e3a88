"""bench.py's command line: a plain run prints the headline line and nothing that takes work of its own (that is --full),
--steps sets the number of timed steps, and --dump-outputs writes the state of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("reference_pass_order", "c3_literal", "iteration_breakdown_us", "moments_kernel", "roofline", "cpu_baseline")


def test_dump_outputs_writes_float64_files_within_the_limit(tmp_path, monkeypatch):
    T, n = 9, 2
    state = dict(mu=np.arange(T * n, dtype=np.float64).reshape(T, n), D=np.ones((T, n, n)), U=np.ones((T - 1, n, n)),
                 SigD=np.ones((T, n, n)), SigU=np.ones((T - 1, n, n)))
    last = dict(cost_iter=2.5, accepted=True, new_cost=1.5, ntrials=1)
    bench.dump_outputs(str(tmp_path / "all"), state, last)
    for name, a in state.items():
        got = np.load(tmp_path / "all" / (name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, a)
    assert np.array_equal(np.load(tmp_path / "all" / "last_step.npy"), [2.5, 1.5, 1.0, 1.0])
    # over the limit: every s-th block, the smallest s that fits
    monkeypatch.setattr(bench, "DUMP_LIMIT", sum(a[::2].nbytes for a in state.values()))
    bench.dump_outputs(str(tmp_path / "part"), state, last)
    mu = np.load(tmp_path / "part" / "mu.npy")
    assert np.array_equal(mu, state["mu"][::2])
    total = sum(os.path.getsize(tmp_path / "part" / (k + ".npy")) - 128 for k in state)      # .npy header: 128 bytes
    assert total <= bench.DUMP_LIMIT


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
    assert line["steps"] == 7 and line["passes"]["full"] + line["passes"]["cost_only"] >= 7
    assert line["ms_per_step"] > 0 and line["dtype"] == "f64"
    mu = np.load(out / "mu.npy")
    assert mu.dtype == np.float64 and mu.shape == (1025, 6) and np.isfinite(mu).all()
    assert np.load(out / "D.npy").shape == (1025, 6, 6) and np.load(out / "SigU.npy").shape == (1024, 6, 6)
    last = np.load(out / "last_step.npy")
    assert last[1] == line["final_cost"] and last[2] == 1.0
