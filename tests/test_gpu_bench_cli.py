"""bench.py end to end on a short run (256 rounds per step): a plain run times the headline leg only and reports its step
time; --dump-outputs writes the final state of the timed path, the same from run to run and the same with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

BENCH = os.path.join(REPO, "bench.py")


def bench(*args):
    env = dict(os.environ, NLMC_BENCH_ROUNDS_PER_STEP="256")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", *args], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_plain_and_full_runs_compute_the_same_outputs(tmp_path):
    a = bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a"))
    assert a["steps"] == 3 and a["rounds_timed"] == 3 * 256 and a["full"] is False
    assert a["ms_per_step"] == pytest.approx(a["seconds_timed"] * 1e3 / 3)
    assert a["value"] == pytest.approx(256 * 10_000 * 10 * 3 * 256 / a["seconds_timed"])
    assert a["unit"] == "spin-updates/s" and a["higher_is_better"] is True and a["dtype"].startswith("f64")
    for k in ("fixed_point_f32", "roofline", "cpu_baseline", "value_kernel_loop"):
        assert k not in a
    out = load(tmp_path / "a")
    assert sorted(out) == ["energies", "slots", "spins"]
    assert out["spins"].dtype == np.float32 and out["spins"].shape == (256, 10_000) and set(np.unique(out["spins"])) == {-1.0, 1.0}
    assert out["energies"].dtype == np.float64 and out["energies"].shape == (256,)
    assert np.array_equal(np.sort(out["slots"]), np.arange(256))
    assert out["energies"].min() < -5_000                       # 7680 sweeps: far below a random start (~0)

    b = bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "b"))
    assert all(np.array_equal(out[k], v) for k, v in load(tmp_path / "b").items())

    c = bench("--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "c"))
    assert c["full"] is True and "fixed_point_f32" in c and "roofline" in c and c["tracked_energies_equal_fp64_recomputation"]
    assert all(np.array_equal(out[k], v) for k, v in load(tmp_path / "c").items())
