"""bench.py --gpus N launcher (one process per GPU) exercised on CPU in its gloo
--dry-run mode: N ranks start, see a world of N with distinct local ranks, and exactly one JSON
line is printed (by rank 0)."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args, timeout=240):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]  # gloo logs its own lines
    return lines


@pytest.mark.parametrize("n", [1, 2])
def test_launcher_dry_run(n):
    lines = _run("--gpus", str(n), "--dry-run", "--steps", "3", "--warmup", "1")
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["n_gpus"] == n
    assert out["process_group"]["world_size"] == n
    assert sorted(out["process_group"]["local_ranks"]) == list(range(n))
    assert out["steps"] == 3 and out["warmup"] == 1


def test_dry_run_accepts_full_and_dumps_outputs(tmp_path):
    """--full and --dump-outputs DIR parse on every path; the dump is DIR/<name>.npy in float32 / float64 and the
    same from run to run."""
    import numpy as np
    got = []
    for d in ("a", "b"):
        lines = _run("--gpus", "1", "--dry-run", "--steps", "2", "--warmup", "1", "--full",
                     "--dump-outputs", str(tmp_path / d))
        assert len(lines) == 1 and json.loads(lines[0])["ms_per_step"] > 0
        got.append(np.load(tmp_path / d / "sum.npy"))
    assert got[0].dtype == np.float64 and got[0].shape == (1,)
    assert np.array_equal(got[0], got[1])


def test_dump_outputs_samples_large_arrays(tmp_path):
    """An array above the per-array cap is cut to a fixed sample of its rows; integers are written as float64."""
    import numpy as np
    sys.path.insert(0, REPO)
    import bench
    big = np.arange(3 * (bench.DUMP_ARRAY_BYTES // 4), dtype=np.float32).reshape(-1, 4)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "ints": np.arange(5, dtype=np.int32), "none": None})
    a, rows = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "a" / "big.rows.npy").astype(np.int64)
    assert a.dtype == np.float32 and a.nbytes <= bench.DUMP_ARRAY_BYTES and np.array_equal(a, big[rows])
    assert np.array_equal(a, np.load(tmp_path / "b" / "big.npy"))
    ints = np.load(tmp_path / "a" / "ints.npy")
    assert ints.dtype == np.float64 and np.array_equal(ints, np.arange(5))
    assert not (tmp_path / "a" / "none.npy").exists()


def test_launcher_propagates_failure():
    """A rank that dies must not leave the others waiting in a collective: the parent stops them
    and exits non-zero."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["ECO_BENCH_DRY_FAIL_RANK"] = "1"
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--dry-run"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode != 0
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
