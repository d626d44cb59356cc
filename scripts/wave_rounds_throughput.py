"""Tempering rounds of short chains as the classes drive them, LocalTempering.plan + run_rounds end to end (planning of the chunk
included, a device synchronise at the end), f32: rounds/s and spin-updates/s of four variants that alternate in one job --

  waves by round   set_wave_sweeps("force"): a wave sweep call and a swap call per round (without set_wave_rounds the rounds entry
                   points do not look at the wave mode)
  off              every mode off: what NPT.run does without a keyword (sweep by sweep, a workgroup per chain)
  in launch        set_lane_sweeps("force"): the chunk inside k_rounds_lanes launches (Engine.pt_rounds_deferred)
  waves in launch  set_wave_sweeps("force") + set_wave_rounds(True): the chunk inside k_rounds_waves launches

on Wishart N = 10 (golden), complete graphs of N = 16 and N = 40, Chimera-128/001; ladders of L = 16, 64 and 1024 of them, and
ladders of L = 64, 16 of them (k_rounds_waves' chains in turn: four chains a wave); T = 1, 10, 1000 sweeps per round.  The shape
and the protocol are scripts/lane_rounds_throughput.py's: median of REPS (default 5) timed runs per variant after one warm-up run
each, with the minimum and maximum.  The four variants leave the same spins and slots, which is asserted.  VARIANTS_OFF (a comma
list of variant names) leaves variants out of a job; LADDERS / LADDERS_64 (comma lists) choose the ladder counts of L = 16 / 64."""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests")); sys.path.insert(0, os.path.join(REPO, "scripts"))
from conftest import load_product, GOLDEN
from lane_throughput import wishart_like, chimera128
import wavefields
P = load_product()
SEED, REPS = 0xA11CE + (3 << 32), int(os.environ.get("REPS", 5))
LADDERS = tuple(int(x) for x in os.environ.get("LADDERS", "64,1024").split(",") if x)
LADDERS_64 = tuple(int(x) for x in os.environ.get("LADDERS_64", "16").split(",") if x)     # ladders of L = 64
SHAPES = [(16, n) for n in LADDERS] + [(64, n) for n in LADDERS_64]
SWEEPS = tuple(int(x) for x in os.environ.get("SWEEPS", "1,10,1000").split(","))
ROUNDS_OF = {1: 200, 10: 50, 1000: 2}
VARIANTS = tuple(v for v in (("waves by round", "off", "force", False), ("off", "off", "off", False), ("in launch", "force", "off", False),
                             ("waves in launch", "off", "force", True))                      # name, lane mode, wave mode, wave rounds
                 if v[0] not in os.environ.get("VARIANTS_OFF", "").split(","))


def timed_run(lt, T, rounds):
    t0 = time.perf_counter()
    lt.plan(rounds * T, rounds)
    lt.run_rounds(rounds, T)
    lt.engs[0].energy_tracked()                             # (synchronises)
    return time.perf_counter() - t0


def main():
    Jw, hw, _, _ = wavefields.wishart(P, GOLDEN)
    grid = [("Wishart N = 10 (golden)", Jw, hw), ("complete graph N = 16", *wishart_like(16, 1)), ("complete graph N = 40", *wishart_like(40, 2)),
            ("Chimera-128/001", *chimera128())]
    print(f"device: {P.device_count()} visible; f32; L // 3 pairs per round; {REPS} timed runs per variant, alternating; "
          f"rounds per run: {ROUNDS_OF}", flush=True)
    print(f"{'instance':26s} {'L':>3s} {'ladders':>7s} {'T':>5s} {'variant':>15s} {'rounds/s':>11s} {'spin-updates/s':>15s} {'ms/run median':>14s} "
          f"{'min':>9s} {'max':>9s}  route", flush=True)
    for name, J, h in grid:
        inst = P.Instance(J, h)
        for L, ladders in SHAPES:
            BETAS, PAIRS = np.geomspace(0.3, 1.5, L), L // 3
            m0 = np.where(np.random.default_rng(ladders).random((L * ladders, inst.n)) < 0.5, -1, 1).astype(np.int8)
            lts = [P.distributed.LocalTempering(inst, BETAS, L * ladders, SEED, PAIRS, [0], lane_sweeps=lanes, wave_sweeps=waves, wave_rounds=wr)
                   for _, lanes, waves, wr in VARIANTS]
            try:
                for lt in lts:
                    lt.set_spins(m0)
                for T in SWEEPS:
                    rounds = ROUNDS_OF.get(T, max(2, 2000 // T))
                    times = [[] for _ in VARIANTS]
                    for rep in range(REPS + 1):
                        for v, lt in enumerate(lts):
                            dt = timed_run(lt, T, rounds)
                            if rep > 0:                      # run 0 warms up: code objects, buffers
                                times[v].append(dt)
                    ends = [(lt.gather_spins(), lt.slots()) for lt in lts]
                    assert all(np.array_equal(e[0], ends[0][0]) and np.array_equal(e[1], ends[0][1]) for e in ends[1:]), (name, L, ladders, T)
                    for v, lt in enumerate(lts):
                        med = float(np.median(times[v]))
                        route = (lt.rounds_routes[0] if getattr(lt, "deferred_rounds", 0) else None) or f"{lt.engs[0].last_sweep_route()} by round"
                        print(f"{name:26s} {L:3d} {ladders:7d} {T:5d} {VARIANTS[v][0]:>15s} {rounds / med:11.1f} "
                              f"{rounds * T * L * ladders * inst.n / med:15.3e} {med * 1e3:14.3f} {min(times[v]) * 1e3:9.3f} {max(times[v]) * 1e3:9.3f}  {route}",
                              flush=True)
            finally:
                for lt in lts:
                    lt.close()


if __name__ == "__main__":
    main()
