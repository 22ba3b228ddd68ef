"""bench.py's command line: a plain run times the steps and writes the solution of the last one (--dump-outputs); --full adds the
side measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench

    return bench


def test_dump_outputs_real_and_complex(tmp_path):
    bench = _bench()
    x = np.random.default_rng(1).standard_normal(1000)
    bench.dump_outputs(str(tmp_path / "r"), x)
    assert sorted(os.listdir(tmp_path / "r")) == ["x.npy"]
    y = np.load(tmp_path / "r" / "x.npy")
    assert y.dtype == np.float64 and np.array_equal(y, x)
    z = x + 1j * x[::-1]
    bench.dump_outputs(str(tmp_path / "c"), z)
    assert sorted(os.listdir(tmp_path / "c")) == ["x_imag.npy", "x_real.npy"]
    assert np.array_equal(np.load(tmp_path / "c" / "x_real.npy"), z.real)
    assert np.array_equal(np.load(tmp_path / "c" / "x_imag.npy"), z.imag)


def test_dump_outputs_samples_a_long_solution_within_the_budget(tmp_path):
    """Longer than the budget: the same seeded positions in every run, and the files stay within DUMP_BYTES_MAX."""
    bench = _bench()
    n = bench.DUMP_BYTES_MAX // 16 + 12345
    z = np.arange(n, dtype=np.float64) + 1j * -np.arange(n, dtype=np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), z)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["x_imag.npy", "x_index.npy", "x_real.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_BYTES_MAX
    idx = np.load(tmp_path / "a" / "x_index.npy")
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(np.load(tmp_path / "a" / "x_real.npy"), idx)
    assert np.array_equal(np.load(tmp_path / "a" / "x_imag.npy"), -idx)
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_command_line_has_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def _run(tmp_path, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "poisson3d_32", *args],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_solution(hs, tmp_path):
    out = tmp_path / "out"
    j = _run(tmp_path, "--steps", "2", "--warmup", "1", "--dump-outputs", str(out))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in j
    assert j["steps"] == 2 and j["warmup"] == 1 and j["dtype"] == "f64" and j["higher_is_better"] is False
    assert j["ms_per_step"] == pytest.approx(j["value"] * 1e3)
    for k in ("residual", "roofline", "solve", "oneshot", "metric_workload", "cpu_baseline"):
        assert k not in j, k
    # the dumped solution solves the bench's own (post-ordered) system
    A, b, nd = hs.problems.make_problem("poisson3d_32", rhs="randn")
    nd, nd_loc = hs.symfact(nd)
    perm = hs.postorder(nd)
    Ap, bp = A[perm - 1][:, perm - 1].tocsc(), b[perm - 1]
    x = np.load(out / "x.npy")
    assert x.dtype == np.float64 and x.shape == bp.shape
    assert np.linalg.norm(Ap @ x - bp) / np.linalg.norm(bp) < 1e-10


@pytest.mark.gpu
def test_full_run_adds_the_side_measurements(tmp_path):
    j = _run(tmp_path, "--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline", "--metric-workload", "")
    assert j["steps"] == 1
    assert j["residual"] < 1e-10
    assert "solve" in j and "oneshot" in j
