"""bench.py's command line: a plain run prints the headline line only, `--full` adds the extra measurements and checks,
`--dump-outputs DIR` writes what the last timed solve returned.  The CPU tests cover the argument handling and the dump
format; the GPU test runs the benchmark end to end on a small mesh and compares the dumped z with the committed golden."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "parity", "kernel_bandwidth_probe", "cpu_baseline")


def test_plain_run_is_the_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (3, 2, False, None)
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked(argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def _sol(L=3, nt=4):
    return dict(its=np.arange(L * nt, dtype=np.int64).reshape(L, nt), ts=0.1 * 10.0 ** np.arange(nt),
                c_dot_Dz=np.linspace(1.0, 2.0, nt))


def test_dump_outputs_writes_float64_arrays(tmp_path):
    n = 50
    z = np.arange(2 * n, dtype=np.float64)                    # flat, column-major as AMG.get_z returns it
    sol = _sol()
    bench.dump_outputs(str(tmp_path / "d"), z, n, sol)
    got = {f[:-4]: np.load(str(tmp_path / "d" / f)) for f in os.listdir(str(tmp_path / "d"))}
    assert set(got) == {"z", "its", "ts", "c_dot_Dz"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["z"], z.reshape((n, 2), order="F"))
    for k in ("its", "ts", "c_dot_Dz"):
        assert np.array_equal(got[k], sol[k])


def test_dump_outputs_samples_large_z_reproducibly(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    n = 1000
    z = np.random.default_rng(1).standard_normal(2 * n)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), z, n, _sol())
    assert sum(np.load(str(tmp_path / "a" / f)).nbytes for f in os.listdir(str(tmp_path / "a"))) <= 4096
    rows = np.load(str(tmp_path / "a" / "z_rows.npy"))
    za = np.load(str(tmp_path / "a" / "z.npy"))
    assert np.array_equal(rows, np.load(str(tmp_path / "b" / "z_rows.npy")))
    assert np.array_equal(za, np.load(str(tmp_path / "b" / "z.npy")))
    assert np.all(np.diff(rows) > 0) and za.shape == (rows.size, 2)
    assert np.array_equal(za, z.reshape((n, 2), order="F")[rows.astype(np.int64)])


def _run_bench(args, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_and_full_runs_on_a_small_mesh(gpu_required, tmp_path):
    """fem2d L=3, p=1: the plain line holds the headline fields and none of the --full extras; the dumped z is the golden z
    (tests/golden/fem2d_L3_p1_0.npz) at the suite's solve tolerance, and --full adds its objects."""
    out = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--L", "3", "--dump-outputs", str(tmp_path / "d")], 300)
    assert all(k in out for k in HEADLINE) and not any(k in out for k in FULL_ONLY)
    assert (out["steps"], out["warmup"], out["dtype"], out["higher_is_better"]) == (2, 1, "f64", True)
    assert out["ms_per_step"] > 0 and out["value"] > 0
    gold = np.load(os.path.join(ROOT, "tests", "golden", "fem2d_L3_p1_0.npz"))
    z = np.load(str(tmp_path / "d" / "z.npy"))
    assert z.dtype == np.float64 and z.shape == gold["z"].shape
    assert np.linalg.norm(z - gold["z"]) / np.linalg.norm(gold["z"]) < 1e-10
    assert np.allclose(np.load(str(tmp_path / "d" / "ts.npy")), gold["ts"], rtol=1e-12)
    full = _run_bench(["--gpus", "1", "--steps", "1", "--L", "3", "--full", "--probe-L", "0", "--cpu-budget", "1"], 300)
    assert "roofline" in full and "cpu_baseline" in full
