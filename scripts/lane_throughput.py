"""Spin-updates/s of Engine.sweep_philox on short and dense instances, one call of 20 sweeps at a time (shared order, no outputs,
both precisions; the per-chain order at one point of the grid), construction of the visiting orders / level schedules included:
wall time around calls that end in a device synchronise, median over REPS calls after one warm-up call of the same shape.

  Wishart-like complete graphs of N = 16 and N = 40, tests/golden/instances/chimera128__001.txt, make_instance(255)
  rows (chains of the call): 64, 256, 1024, 4096, 16384

LANES=force (default) | auto | off selects the route where the engine has set_lane_sweeps; an engine without it (a build of an
earlier commit) is timed as it is, which is the sweep-by-sweep route.  GRID=rng times only N = 40 and Chimera-128 (the two
random-number designs of k_sweep_lanes: run once with NLMC_LANE_RNG=0 and once with NLMC_LANE_RNG=1).  Compare two builds in one
job, alternating them (scripts/README.md)."""
import os, sys, time
import numpy as np
import scipy.sparse as sp
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import load_product
from helpers import make_instance
P = load_product()
S, SEED = 20, 12345
ROWS = (64, 256, 1024, 4096, 16384)
MODE = os.environ.get("LANES", "force")
MIN_TIME, MIN_REPS, MAX_REPS = float(os.environ.get("MIN_TIME", 0.2)), 5, 400


def wishart_like(N, seed, alpha=0.75):
    """Planted Wishart couplings (complete graph): J = -W W^T / N off the diagonal, the columns of W orthogonal to the planted state."""
    r = np.random.default_rng(seed)
    t = r.choice([-1.0, 1.0], size=N)
    W = r.standard_normal((N, max(1, int(alpha * N))))
    W -= np.outer(t, t @ W) / N
    J = -(W @ W.T) / N
    np.fill_diagonal(J, 0.0)
    return J / np.max(np.abs(J)), np.zeros(N)


def chimera128():
    W, h = P.instances.txt_to_A_droplet(os.path.join(REPO, "tests", "golden", "instances", "chimera128__001.txt"))
    J = -sp.csr_matrix(W).astype(np.float64)
    s = np.max(np.abs(J.data))
    return (J / s).tocsr(), -np.asarray(h, dtype=np.float64).ravel() / s


def rate(inst, rows, precision, order="shared"):
    N = inst.n
    spins = np.where(np.random.default_rng(rows).random((rows, N)) < 0.5, -1, 1).astype(np.int8)
    with P.Engine(inst, None, rows) as eng:
        route = "as built"
        if hasattr(eng, "set_lane_sweeps"):
            eng.set_lane_sweeps(MODE)
        eng.set_spins(spins)
        eng.energy()
        times, t_all, k = [], 0.0, 0
        while k < 1 + MIN_REPS or (t_all < MIN_TIME and k < 1 + MAX_REPS):
            t0 = time.perf_counter()
            eng.sweep_philox(S, SEED, sweep0=k * S, beta=1.0, precision=precision, order=order)
            eng.energy_tracked()                       # (synchronises)
            dt = time.perf_counter() - t0
            if k > 0:                                  # call 0 warms up: code objects, buffers
                times.append(dt)
                t_all += dt
            k += 1
        if hasattr(eng, "last_sweep_route"):
            route = eng.last_sweep_route()
    med = float(np.median(times))
    return rows * N * S / med, med * 1e6, min(times) * 1e6, max(times) * 1e6, len(times), route


def main():
    grid = [("Wishart-like complete graph, N = 16", *wishart_like(16, 1)), ("Wishart-like complete graph, N = 40", *wishart_like(40, 2)),
            ("Chimera-128/001", *chimera128()), ("make_instance(255)", *make_instance(255))]
    if os.environ.get("GRID") == "rng":
        grid = grid[1:3]
    print(f"device: {P.device_count()} visible; LANES={MODE}; NLMC_LANE_RNG={os.environ.get('NLMC_LANE_RNG', 'unset')}; "
          f"{S} sweeps per call, shared order unless stated, no outputs", flush=True)
    print(f"{'instance':38s} {'rows':>6s} {'mode':>4s} {'spin-updates/s':>15s} {'us/call median':>15s} {'min':>9s} {'max':>9s} {'calls':>6s}  route", flush=True)
    for name, J, h in grid:
        inst = P.Instance(J, h)
        for rows in ROWS:
            for prec in ("f32", "f64"):
                r = rate(inst, rows, prec)
                print(f"{name:38s} {rows:6d} {prec:>4s} {r[0]:15.3e} {r[1]:15.1f} {r[2]:9.1f} {r[3]:9.1f} {r[4]:6d}  {r[5]}", flush=True)
        if "N = 40" in name:
            for prec in ("f32", "f64"):
                r = rate(inst, 1024, prec, order="per_chain")
                print(f"{name + ', per-chain order':38s} {1024:6d} {prec:>4s} {r[0]:15.3e} {r[1]:15.1f} {r[2]:9.1f} {r[3]:9.1f} {r[4]:6d}  {r[5]}", flush=True)


if __name__ == "__main__":
    main()
