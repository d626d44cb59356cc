"""APT rounds of short chains: an engine loop shaped like APT_ICM._run_device_resident (planning of the run included, one read-back
of the swap log and a device synchronise at the end), rounds/s of three variants that alternate in one job --

  in launch      pt_plan + Engine.apt_rounds_lanes: all rounds inside k_apt_rounds_lanes launches (info of every round read back)
  lanes by round set_lane_sweeps("force"): a lane sweep call, icm_round_ladders and pt_swap_philox per round, same build
  off            lane mode off: what APT_ICM.run does without the lanes keyword (sweep by sweep, a workgroup per chain)

on Wishart N = 10 (golden), complete graphs of N = 16 and N = 40, Chimera-128/001; K = 10 sub-replicas of L = 6, 16 and 32
temperatures; T = 1, 10, 100 sweeps per round (ROUNDS_OF rounds per timed run); f32 and fp64.  The round-by-round variants read the
cluster sizes back on the class's sample of the rounds.  Median of REPS (default 5) timed runs per variant after one warm-up run
each, with the minimum and maximum.  The three variants leave the same spins and slots, which is asserted."""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests")); sys.path.insert(0, os.path.join(REPO, "scripts"))
from conftest import load_product
from lane_throughput import wishart_like, chimera128
from test_gpu_lanes import wishart
P = load_product()
K, SEED, REPS = 10, 0xA11CE + (7 << 32), int(os.environ.get("REPS", 5))
LADDERS = tuple(int(x) for x in os.environ.get("LADDERS", "6,16,32").split(","))
SWEEPS = tuple(int(x) for x in os.environ.get("SWEEPS", "1,10,100").split(","))
ROUNDS_OF = {1: 100, 10: 30, 100: 4}
VARIANTS = (("in launch", "off"), ("lanes by round", "force"), ("off", "off"))


def timed_run(eng, v, L, T, rounds, prec, m0):
    pairs = L // 3
    eng.set_spins(m0)
    eng.pt_set_slots((np.arange(K * L) % L).astype(np.int32))
    eng.energy_tracked()                                        # (synchronises)
    t0 = time.perf_counter()
    eng.pt_plan(0, rounds, SEED, pairs)
    eng.pt_log_begin(0, rounds, pairs)
    if v == 0:
        ok, _ = eng.apt_rounds_lanes(rounds, T, SEED, 0, 0, pairs, precision=prec, want_info=True)
        assert ok, eng.rounds_fused_refusal
    else:
        planner = P.engine.RoundPlanner(eng, 0, rounds, T, SEED, precision=prec)
        every = max(1, rounds // 16)
        for ii in range(rounds):
            planner.sweep(ii)
            eng.icm_round_ladders(ii, SEED, True, want_info=rounds <= 16 or ii == rounds - 1 or ii % every == 0)
            eng.pt_swap_philox(ii, SEED, pairs, want_log=False)
    eng.pt_log_read()
    eng.energy_tracked()
    return time.perf_counter() - t0


def main():
    Jw, hw, _, _ = wishart(P)
    grid = [("Wishart N = 10 (golden)", Jw, hw), ("complete graph N = 16", *wishart_like(16, 1)), ("complete graph N = 40", *wishart_like(40, 2)),
            ("Chimera-128/001", *chimera128())]
    print(f"device: {P.device_count()} visible; K = {K} sub-replicas, L // 3 pairs per round; {REPS} timed runs per variant, alternating; "
          f"rounds per run: {ROUNDS_OF}", flush=True)
    print(f"{'instance':26s} {'L':>3s} {'T':>4s} {'mode':>4s} {'variant':>15s} {'rounds/s':>11s} {'us/round':>9s} {'ms/run median':>14s} "
          f"{'min':>9s} {'max':>9s}  route", flush=True)
    for name, J, h in grid:
        inst = P.Instance(J, h)
        for L in LADDERS:
            m0 = np.where(np.random.default_rng(L).random((K * L, inst.n)) < 0.5, -1, 1).astype(np.int8)
            engs = [P.Engine(inst, None, K * L) for _ in VARIANTS]
            try:
                for eng, (_, lanes) in zip(engs, VARIANTS):
                    eng.set_lane_sweeps(lanes)
                    eng.pt_init(np.geomspace(0.3, 1.5, L))
                for prec in ("f32", "f64"):
                    for T in SWEEPS:
                        rounds = ROUNDS_OF.get(T, max(2, 400 // T))
                        times = [[] for _ in VARIANTS]
                        for rep in range(REPS + 1):
                            for v, eng in enumerate(engs):
                                dt = timed_run(eng, v, L, T, rounds, prec, m0)
                                if rep > 0:                      # run 0 warms up: code objects, buffers
                                    times[v].append(dt)
                        ends = [(e.get_spins(), e.pt_slots(), e.energy_tracked()) for e in engs]
                        assert all(all(np.array_equal(x, y) for x, y in zip(e, ends[0])) for e in ends[1:]), (name, L, T, prec)
                        for v, eng in enumerate(engs):
                            med = float(np.median(times[v]))
                            route = "apt lanes" if v == 0 else f"{eng.last_sweep_route()} by round"
                            print(f"{name:26s} {L:3d} {T:4d} {prec:>4s} {VARIANTS[v][0]:>15s} {rounds / med:11.1f} {med / rounds * 1e6:9.1f} "
                                  f"{med * 1e3:14.3f} {min(times[v]) * 1e3:9.3f} {max(times[v]) * 1e3:9.3f}  {route}", flush=True)
            finally:
                for eng in engs:
                    eng.close()


if __name__ == "__main__":
    main()
