"""bench.py's plain run and ``--dump-outputs``: a plain run carries only the
headline (no --full legs), ``--steps`` sets the timed steps, and the dumped
potentials / accelerations are those of the seeded workload (checked against
the oracle); an output past the 64 MB budget is cut to a fixed sample."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


class _Results:
    def __init__(self, n):
        self.pot = np.arange(n, dtype=np.float64)
        self.acc = np.stack([self.pot, -self.pot, 2.0 * self.pot], axis=1)

    def results(self):
        return self.pot, self.acc


def test_dump_outputs_samples_past_the_budget(tmp_path):
    import bench

    n = 2_100_000  # 67.2 MB of potentials + accelerations
    src = _Results(n)
    info = bench.dump_outputs(str(tmp_path / "a"), src, 0, 1)
    again = bench.dump_outputs(str(tmp_path / "b"), src, 0, 1)
    assert info["sampled"] and info["of"] == n and info["rows"] == again["rows"] < n
    size = sum(f.stat().st_size for f in (tmp_path / "a").iterdir())
    assert size <= bench.DUMP_BYTES_MAX
    pot, acc = np.load(tmp_path / "a" / "pot.npy"), np.load(tmp_path / "a" / "acc.npy")
    assert pot.dtype == np.float64 and acc.dtype == np.float64
    assert pot.shape == (info["rows"],) and acc.shape == (info["rows"], 3)
    # the same rows of both arrays, in particle order, identical from run to run
    assert np.all(np.diff(pot) > 0)
    assert np.array_equal(acc, np.stack([pot, -pot, 2.0 * pot], axis=1))
    assert np.array_equal(pot, np.load(tmp_path / "b" / "pot.npy"))

    small = _Results(1000)
    info = bench.dump_outputs(str(tmp_path / "c"), small, 1, 2)
    assert not info["sampled"] and info["files"] == ["pot_rank1.npy", "acc_rank1.npy"]
    assert np.array_equal(np.load(tmp_path / "c" / "pot_rank1.npy"), small.pot)
    assert np.array_equal(np.load(tmp_path / "c" / "acc_rank1.npy"), small.acc)


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_outputs(gpu, tmp_path):
    from oracle import gravity as og
    from pynbodyext.synthetic import plummer

    n = 10_007  # odd, past parallel.SYM_MIN_N: the headline's symmetric kernel
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--n-per-gpu", str(n), "--dump-outputs",
                        str(tmp_path / "out")], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False
    assert out["ms_per_step"] > 0 and out["unit"] == "pairs/s" and out["dtype"] == "f64"
    assert out["value"] == pytest.approx(n * (n - 1.0) / (out["ms_per_step"] * 1e-3))
    assert out["roofline"]["kernel_ms"] > 0 and "precise_kernel_ms" not in out["roofline"]
    assert "tree" not in out and "profile" not in out
    assert out["cpu_baseline"] is None and out["api_level"] is None

    pot, acc = np.load(tmp_path / "out" / "pot.npy"), np.load(tmp_path / "out" / "acc.npy")
    assert pot.dtype == np.float64 and pot.shape == (n,) and acc.shape == (n, 3)
    pos, mass = plummer(n, seed=out["config"]["seed"])
    pot_ref = og.direct_potentials(pos, mass)
    acc_ref = og.direct_accelerations(pos, mass)
    assert np.max(np.abs(pot - pot_ref) / np.abs(pot_ref)) < 1e-5
    assert np.max(np.linalg.norm(acc - acc_ref, axis=1) / np.linalg.norm(acc_ref, axis=1)) < 1e-5
