"""bench.py pieces that need no GPU: the self-launcher of `--gpus N` (the ranks are started as a CHILD
`python -m torch.distributed.run` before anything touches the GPU) and the CPU-baseline worker process."""
import json
import os
import subprocess
import sys

from conftest import REPO

BENCH = os.path.join(REPO, "bench.py")


def run(*args, env=None):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        e.pop(k, None)
    e.update(env or {})
    p = subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, timeout=300, env=e)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_gpus_n_starts_its_own_ranks_as_a_child_launcher():
    d = run("--gpus", "4", "--steps", "3", "--warmup", "1", "--strong", "--dry-run-launch")
    cmd = d["would_run"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=4" in cmd
    i = cmd.index("--master-addr")
    assert cmd[i + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1].isdigit()
    tail = cmd[cmd.index(BENCH) + 1:]
    assert tail[:2] == ["--gpus", "4"] and "--strong" in tail and tail[tail.index("--steps") + 1] == "3"


def test_cpu_baseline_worker_is_a_plain_cpu_process():
    d = run("--cpu-worker", "0.3", "--cpu-chain", "2", env={"HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""})
    assert d["kind"] == "port" and d["cores"] == 1 and d["unit"] == "spin-updates/s" and d["value"] > 1e5


def test_fused_plans_stay_within_the_memory_budget_for_default_arguments():
    """one planning call for a default-length run (10^4 sweeps: 200 windows of 50) would take ~2 GB at N = 10^3 and
    ~16 GB at N = 10^4, times 30 phase launches in NMC.run_restarts; Engine.sweep_philox_windows plans piece by piece."""
    from conftest import load_product
    P = load_product()
    eng = P.engine
    assert eng.fused_window(10000) == 50
    for n, n_long in ((1000, 40), (10000, 400), (11264, 0)):
        per_window = eng.fused_plan_bytes(n, n_long, 50)
        assert 50 * n * 24 < per_window < 50 * (n + n_long) * 90 + 6 * 2 ** 20       # 24 ... 76 bytes per position + padding
        piece = eng.sweeps_per_plan_piece(per_window, 10000, 50, eng.Engine.FUSED_PLAN_BUDGET)
        assert piece % 50 == 0 and 50 <= piece <= 10000
        assert (piece // 50) * per_window <= eng.Engine.FUSED_PLAN_BUDGET
        # strided records: pieces start on recorded sweeps
        assert eng.sweeps_per_plan_piece(per_window, 10000, 50, eng.Engine.FUSED_PLAN_BUDGET, record_stride=4) % 100 == 0
    # a budget below one window still makes progress, one window at a time
    assert eng.sweeps_per_plan_piece(eng.fused_plan_bytes(10000, 0, 50), 10000, 50, 1) == 50


def test_the_launcher_forwards_full_and_dump_outputs(tmp_path):
    d = run("--gpus", "2", "--steps", "2", "--warmup", "0", "--full", "--dump-outputs", str(tmp_path), "--dry-run-launch")
    tail = d["would_run"][d["would_run"].index(BENCH) + 1:]
    assert "--full" in tail and tail[tail.index("--dump-outputs") + 1] == str(tmp_path)


def test_dump_outputs_are_exact_floats_within_the_budget(tmp_path):
    """Spins (int8) as float32, slots (int32) and energies (float64) as float64; past 64 MB a fixed, seeded sample of rows."""
    import numpy as np
    import bench
    rng = np.random.default_rng(5)
    spins = (2 * rng.integers(0, 2, size=(256, 1000)) - 1).astype(np.int8)
    slots = rng.permutation(256).astype(np.int32)
    energies = rng.standard_normal(256) * 1e4
    bench.dump_outputs(str(tmp_path / "a"), {"spins": spins, "energies": energies, "slots": slots})
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in ("spins", "energies", "slots")}
    assert got["spins"].dtype == np.float32 and np.array_equal(got["spins"], spins)
    assert got["slots"].dtype == np.float64 and np.array_equal(got["slots"], slots)
    assert got["energies"].dtype == np.float64 and np.array_equal(got["energies"], energies)
    assert sorted(os.listdir(tmp_path / "a")) == ["energies.npy", "slots.npy", "spins.npy"]

    big = np.ones((8, 256, 10000), np.int8)                     # 80 MB as float32
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"spins": big, "energies": np.arange(2048, dtype=np.int64).reshape(8, 256)})
    files = os.listdir(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in files) <= 64 << 20
    rows = np.load(tmp_path / "b" / "spins_rows.npy")
    assert np.load(tmp_path / "b" / "spins.npy").shape == (rows.size, 10000) and rows.size > 1000
    assert np.array_equal(rows, np.load(tmp_path / "c" / "spins_rows.npy"))
    assert np.array_equal(np.load(tmp_path / "b" / "energies.npy"), np.arange(2048).reshape(8, 256))


def test_steps_must_be_positive():
    p = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--steps" in p.stderr
