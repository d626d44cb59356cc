"""What the run-long per-round energy log (Engine.elog_begin; LocalTempering(track_energies=True)) costs: time per round with the log
closed and open on the same build, on each of the four rounds routes:

  in launch          N = 10^4 (+-J of degree 6, the instance bench.py times), 256 replicas on one ladder, 10 sweeps per round, f32:
                     the rounds inside k_rounds_fused launches (thread 0 of every chain stores 12 bytes per round)
  launch per round   the same shape with NLMC_NO_PERSISTENT=1 at context creation: a k_elog_update launch behind every sweep launch
  lanes              Wishart N = 10, 1024 ladders of L = 16 (16 384 chains), 10 sweeps per round, f32: the rounds inside k_rounds_lanes
  apt lanes          the same chains as 256 systems of K = 4 sub-replica ladders, Engine.apt_rounds_lanes: inside k_apt_rounds_lanes

The first three time LocalTempering.plan + run_rounds end to end (planning of the chunk and the log's reset included, a device
synchronise at the end); the last one times the one Engine.apt_rounds_lanes call and a synchronise.  Both variants of a workload
alternate in one job and start every run from the same random states.  Median of REPS (default 5) timed runs per variant after one
warm-up run each, with the minimum and maximum.  Both variants leave the same spins and slots, which is asserted."""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import load_product
from helpers import make_instance
from test_gpu_lanes import wishart
P = load_product()
SEED, REPS, T = 0xE106 + (5 << 32), int(os.environ.get("REPS", 5)), 10


def report(name, times, rounds, routes):
    med = [float(np.median(t)) for t in times]
    for v, label in enumerate(("log closed", "log open")):
        print(f"{name:40s} {label:>10s} {med[v] / rounds * 1e6:12.2f} {min(times[v]) / rounds * 1e6:10.2f} "
              f"{max(times[v]) / rounds * 1e6:10.2f}  {routes[v]}", flush=True)
    print(f"{name:40s} {'open/closed':>10s} {med[1] / med[0]:12.4f}", flush=True)


def timed_run(lt, m0, rounds):
    lt.set_spins(m0)
    for e in lt.engs:
        e.pt_set_slots((np.arange(lt.G) % e.ladder_len).astype(np.int32))
        e.energy_tracked()                                      # (synchronises: nothing of the set-up is timed)
    t0 = time.perf_counter()
    lt.plan(rounds * T, rounds)                                 # (track_energies: opens the log for these rounds)
    lt.run_rounds(rounds, T)
    lt.engs[0].energy_tracked()                                 # (synchronises)
    return time.perf_counter() - t0


def measure(name, inst, betas, G, pairs, lanes, rounds, env=None):
    m0 = np.where(np.random.default_rng(G).random((G, inst.n)) < 0.5, -1, 1).astype(np.int8)
    os.environ.update(env or {})                                # (read when the contexts are created)
    try:
        lts = [P.distributed.LocalTempering(inst, betas, G, SEED, pairs, [0], lane_sweeps=lanes, track_energies=on) for on in (False, True)]
    finally:
        for k in (env or {}):
            del os.environ[k]
    try:
        times = [[], []]
        for rep in range(REPS + 1):
            for v, lt in enumerate(lts):
                dt = timed_run(lt, m0, rounds)
                if rep > 0:                                     # run 0 warms up: code objects, buffers
                    times[v].append(dt)
        ends = [(lt.gather_spins(), lt.slots()) for lt in lts]
        assert np.array_equal(ends[0][0], ends[1][0]) and np.array_equal(ends[0][1], ends[1][1]), name
        E, sl = lts[1].energy_log()
        assert E.shape == (rounds, G) and not np.isnan(E).any() and (sl >= 0).all(), name
        report(name, times, rounds, [lt.rounds_routes[0] for lt in lts])
    finally:
        for lt in lts:
            lt.close()


def measure_apt(name, inst, betas, M, K, pairs, rounds):
    L = len(betas)
    G = M * K * L
    m0 = np.where(np.random.default_rng(G).random((G, inst.n)) < 0.5, -1, 1).astype(np.int8)
    with P.Engine(inst, None, G) as eng:
        eng.pt_init(betas)
        eng.apt_systems(M)
        eng.pt_plan(0, rounds, SEED, pairs)
        times, ends = [[], []], [None, None]
        for rep in range(REPS + 1):
            for v in (0, 1):
                eng.set_spins(m0)
                eng.pt_set_slots((np.arange(G) % L).astype(np.int32))
                eng.energy_tracked()
                t0 = time.perf_counter()
                if v:
                    eng.elog_begin(0, rounds)
                ok, _ = eng.apt_rounds_lanes(rounds, T, SEED, 0, 0, pairs)
                assert ok, eng.rounds_fused_refusal
                eng.energy_tracked()
                dt = time.perf_counter() - t0
                if v:
                    eng.elog_end()
                if rep > 0:
                    times[v].append(dt)
                ends[v] = (eng.get_spins(), eng.pt_slots())
        assert np.array_equal(ends[0][0], ends[1][0]) and np.array_equal(ends[0][1], ends[1][1]), name
        E, _ = eng.elog_read()
        assert E.shape == (rounds, G) and not np.isnan(E).any(), name
        report(name, times, rounds, [eng.last_rounds_route()] * 2)


def main():
    print(f"device: {P.device_count()} visible; {T} sweeps per round; {REPS} timed runs per variant, alternating, one warm-up each", flush=True)
    print(f"{'workload':40s} {'variant':>10s} {'us/round med':>12s} {'min':>10s} {'max':>10s}  route", flush=True)
    J, h = make_instance(10_000, seed=20250225)
    inst = P.Instance(J, h)
    betas = np.geomspace(0.05, 4.0, 256)
    measure("N = 10^4, 256 replicas (bench), f32", inst, betas, 256, round(0.3 * 256), "off", 200)
    measure("... with NLMC_NO_PERSISTENT=1", inst, betas, 256, round(0.3 * 256), "off", 200, env={"NLMC_NO_PERSISTENT": "1"})
    Jw, hw, _, _ = wishart(P)
    inst = P.Instance(Jw, hw)
    betas = np.geomspace(0.3, 1.5, 16)
    measure("Wishart N = 10, L = 16 x 1024 ladders", inst, betas, 16 * 1024, 5, "force", 200)
    measure_apt("... as 256 APT systems of K = 4", inst, betas, 256, 4, 5, 200)


if __name__ == "__main__":
    main()
