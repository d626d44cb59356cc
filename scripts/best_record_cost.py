"""What the run-long best-state record (Engine.best_begin; LocalTempering(track_best=True)) costs: time per round with the record off
and on, LocalTempering.plan + run_rounds end to end (planning of the chunk included, a device synchronise at the end), on

  bench shape   N = 10^4 (+-J of degree 6, the instance bench.py times), 256 replicas on one ladder, 10 sweeps per round, fp64 and fixed
                point: the rounds inside k_rounds_fused launches
  lane rounds   complete graph N = 40 (planted Wishart couplings), ladders of L = 16, 16 384 chains, 10 sweeps per round, f32 and fp64:
                the rounds inside k_rounds_lanes launches

Both variants of a workload alternate in one job and start every run from the same random states with a fresh record -- the first
rounds of a quench are where chains improve most often, the worst case for the record.  Median of REPS (default 7) timed runs per
variant after one warm-up run each, with the minimum and maximum.  Both variants leave the same spins and slots, which is asserted."""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests")); sys.path.insert(0, os.path.join(REPO, "scripts"))
from conftest import load_product
from helpers import make_instance
from lane_throughput import wishart_like
P = load_product()
SEED, REPS, T = 0xBE57 + (5 << 32), int(os.environ.get("REPS", 7)), 10


def timed_run(lt, m0, rounds):
    lt.set_spins(m0)
    for e in lt.engs:
        e.pt_set_slots((np.arange(lt.G) % e.ladder_len).astype(np.int32))
        if lt.track_best:
            e.best_begin(None)
        e.energy_tracked()                                      # (synchronises: nothing of the set-up is timed)
    t0 = time.perf_counter()
    lt.plan(rounds * T, rounds)
    lt.run_rounds(rounds, T)
    lt.engs[0].energy_tracked()                                 # (synchronises)
    return time.perf_counter() - t0


def measure(name, inst, betas, G, pairs, precision, lanes, rounds):
    m0 = np.where(np.random.default_rng(G).random((G, inst.n)) < 0.5, -1, 1).astype(np.int8)
    lts = [P.distributed.LocalTempering(inst, betas, G, SEED, pairs, [0], precision=precision, lane_sweeps=lanes, track_best=on)
           for on in (False, True)]
    try:
        times = [[], []]
        for rep in range(REPS + 1):
            for v, lt in enumerate(lts):
                dt = timed_run(lt, m0, rounds)
                if rep > 0:                                     # run 0 warms up: code objects, buffers
                    times[v].append(dt)
        ends = [(lt.gather_spins(), lt.slots()) for lt in lts]
        assert np.array_equal(ends[0][0], ends[1][0]) and np.array_equal(ends[0][1], ends[1][1]), name
        improved = float(np.mean(lts[1].best()["stamp"] > lts[1].rounds_done - rounds))      # (the last run's first round)
        med = [float(np.median(t)) for t in times]
        for v, label in enumerate(("record off", "record on")):
            print(f"{name:34s} {precision:>4s} {label:>11s} {med[v] / rounds * 1e6:12.2f} {min(times[v]) / rounds * 1e6:10.2f} "
                  f"{max(times[v]) / rounds * 1e6:10.2f}  {lts[v].rounds_routes[0]}", flush=True)
        print(f"{name:34s} {precision:>4s} {'on / off':>11s} {med[1] / med[0]:12.4f}   (chains whose best came after round 0: {improved:.2f})", flush=True)
    finally:
        for lt in lts:
            lt.close()


def main():
    print(f"device: {P.device_count()} visible; {T} sweeps per round; {REPS} timed runs per variant, alternating, one warm-up each", flush=True)
    print(f"{'workload':34s} {'mode':>4s} {'variant':>11s} {'us/round med':>12s} {'min':>10s} {'max':>10s}  route", flush=True)
    J, h = make_instance(10_000, seed=20250225)
    inst = P.Instance(J, h)
    for prec in ("f64", "f32"):
        measure("N = 10^4, 256 replicas (bench)", inst, np.geomspace(0.05, 4.0, 256), 256, round(0.3 * 256), prec, "off", 200)
    Jw, hw = wishart_like(40, 2)
    inst = P.Instance(Jw, hw)
    for prec in ("f32", "f64"):
        measure("complete N = 40, L = 16, 16384 chains", inst, np.geomspace(0.3, 1.5, 16), 16 * 1024, 5, prec, "force", 50)


if __name__ == "__main__":
    main()
