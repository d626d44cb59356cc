"""APT restarts side by side: the engine loop of scripts/apt_lanes_throughput.py with M = 1, 16, 256 independent systems in one context
(Engine.apt_systems), system-rounds/s of three variants that alternate in one job --

  in launch      pt_plan + Engine.apt_rounds_lanes: all rounds inside k_apt_rounds_lanes launches, a workgroup per system
  lanes by round set_lane_sweeps("force"): a lane sweep call, icm_round_ladders and pt_swap_philox per round
  off            lane mode off: what APT_ICM.run(num_restarts=M) does without the lanes keyword

on Wishart N = 10 (golden), a complete graph of N = 40 and Chimera-128/001; K = 10 sub-replicas of L = 6 temperatures; T = 1 and 10 sweeps
per round; f32 and fp64.  Median of REPS (default 5) timed runs per variant after one warm-up run each, with the minimum and maximum.  The
three variants leave the same spins, slots and energies, which is asserted.  "x loop": M times the one-system run of the same variant
over this run -- what running the one-system loop M times costs against the M systems side by side.  With SYSTEMS=1 the script also runs
on a build without Engine.apt_systems: that is how the parent commit's one-system loop is measured for the baseline."""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests")); sys.path.insert(0, os.path.join(REPO, "scripts"))
from conftest import load_product
from lane_throughput import wishart_like, chimera128
from test_gpu_lanes import wishart
P = load_product()
K, L, SEED, REPS = 10, int(os.environ.get("LADDER", 6)), 0xA11CE + (7 << 32), int(os.environ.get("REPS", 5))
SYSTEMS = tuple(int(x) for x in os.environ.get("SYSTEMS", "1,16,256").split(","))
SWEEPS = tuple(int(x) for x in os.environ.get("SWEEPS", "1,10").split(","))
ROUNDS_OF = {1: 100, 10: 30}
VARIANTS = (("in launch", "off"), ("lanes by round", "force"), ("off", "off"))


def timed_run(eng, v, M, T, rounds, prec, m0):
    pairs = L // 3
    eng.set_spins(m0)
    eng.pt_set_slots((np.arange(M * K * L) % L).astype(np.int32))
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
    grid = [("Wishart N = 10 (golden)", Jw, hw), ("complete graph N = 40", *wishart_like(40, 2)), ("Chimera-128/001", *chimera128())]
    print(f"device: {P.device_count()} visible; K = {K} sub-replicas of L = {L} temperatures, L // 3 pairs per round; {REPS} timed runs per "
          f"variant, alternating; rounds per run: {ROUNDS_OF}", flush=True)
    print(f"{'instance':24s} {'M':>4s} {'T':>3s} {'mode':>4s} {'variant':>15s} {'sys-rounds/s':>13s} {'us/round':>9s} {'ms/run median':>14s} "
          f"{'min':>9s} {'max':>9s} {'x loop':>7s}  route", flush=True)
    for name, J, h in grid:
        inst = P.Instance(J, h)
        one = {}                                                # (T, prec, variant) -> median seconds of the one-system run
        for M in SYSTEMS:
            G = M * K * L
            m0 = np.where(np.random.default_rng(L).random((G, inst.n)) < 0.5, -1, 1).astype(np.int8)
            engs = [P.Engine(inst, None, G) for _ in VARIANTS]
            try:
                for eng, (_, lanes) in zip(engs, VARIANTS):
                    eng.set_lane_sweeps(lanes)
                    eng.pt_init(np.geomspace(0.3, 1.5, L))
                    if M > 1:
                        eng.apt_systems(M)
                for prec in ("f32", "f64"):
                    for T in SWEEPS:
                        rounds = ROUNDS_OF.get(T, max(2, 400 // T))
                        times = [[] for _ in VARIANTS]
                        for rep in range(REPS + 1):
                            for v, eng in enumerate(engs):
                                dt = timed_run(eng, v, M, T, rounds, prec, m0)
                                if rep > 0:                      # run 0 warms up: code objects, buffers
                                    times[v].append(dt)
                        ends = [(e.get_spins(), e.pt_slots(), e.energy_tracked()) for e in engs]
                        assert all(all(np.array_equal(x, y) for x, y in zip(e, ends[0])) for e in ends[1:]), (name, M, T, prec)
                        for v, eng in enumerate(engs):
                            med = float(np.median(times[v]))
                            if M == 1:
                                one[(T, prec, v)] = med
                            loop = f"{M * one[(T, prec, v)] / med:7.2f}" if (T, prec, v) in one else f"{'-':>7s}"
                            route = "apt lanes" if v == 0 else f"{eng.last_sweep_route()} by round"
                            print(f"{name:24s} {M:4d} {T:3d} {prec:>4s} {VARIANTS[v][0]:>15s} {M * rounds / med:13.1f} {med / rounds * 1e6:9.1f} "
                                  f"{med * 1e3:14.3f} {min(times[v]) * 1e3:9.3f} {max(times[v]) * 1e3:9.3f} {loop}  {route}", flush=True)
            finally:
                for eng in engs:
                    eng.close()


if __name__ == "__main__":
    main()
