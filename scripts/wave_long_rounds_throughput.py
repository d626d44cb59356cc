"""Tempering rounds of chains of 257 .. 1024 spins as the classes drive them, LocalTempering.plan + run_rounds end to end (planning of
the chunk included, a device synchronise at the end), f32, under wave_sweeps="force", wave_rounds=True, wave_long=True: rounds/s and
spin-updates/s of two variants that alternate in one job --

  call by call   wave_long_rounds=False: a wave sweep call (k_sweep_waves_long, which builds the local fields) and a swap call per round
  in launch      wave_long_rounds=True: the chunk inside k_rounds_waves_long launches, the fields built once per launch

on complete Gaussian graphs of n = 320, 512 and 1024 and one sparse degree-6 graph of 1024 spins (tests/helpers.make_instance); ladders
of L = 8, 16 and 32 temperatures, 16 and 256 of them; T = 1, 10, 100, 1000 sweeps per round.  The ladders are cold at the top (the dense
instances' fields are of order sqrt(n) / 4, so their inverse temperatures are a tenth of the sparse one's): the cold rungs flip a few
percent of their spins per sweep, which is where a field prologue per round weighs most.  The protocol is
scripts/wave_rounds_throughput.py's: median of REPS (default 5) timed runs per variant after one warm-up run each, with the minimum
and maximum.  Both variants leave the same spins and slots, which is asserted.  INSTANCES (comma list of 0 .. 3), LS, LADDERS, SWEEPS
(comma lists) choose a part of the grid, so that a job can give every instance a process and a time limit of its own."""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import load_product
from helpers import make_instance
import wavefields
P = load_product()
SEED, REPS = 0xA11CE + (3 << 32), int(os.environ.get("REPS", 5))


def ints(name, default):
    return tuple(int(x) for x in os.environ.get(name, default).split(",") if x)


INSTANCES, LS, LADDERS, SWEEPS = ints("INSTANCES", "0,1,2,3"), ints("LS", "8,16,32"), ints("LADDERS", "16,256"), ints("SWEEPS", "1,10,100,1000")
ROUNDS_OF = {1: 40, 10: 20, 100: 4, 1000: 2}
VARIANTS = (("call by call", False), ("in launch", True))
GRID = [("complete graph n = 320", lambda: wavefields.dense_instance(320, 320), (0.03, 0.6)),
        ("complete graph n = 512", lambda: wavefields.dense_instance(512, 512), (0.03, 0.6)),
        ("complete graph n = 1024", lambda: wavefields.dense_instance(1024, 1024), (0.03, 0.6)),
        ("sparse degree 6 n = 1024", lambda: make_instance(1024, seed=1024, with_h=True, gaussian=True), (0.3, 6.0))]


def timed_run(lt, T, rounds):
    t0 = time.perf_counter()
    lt.plan(rounds * T, rounds)
    lt.run_rounds(rounds, T)
    lt.engs[0].energy_tracked()                             # (synchronises)
    return time.perf_counter() - t0


def main():
    print(f"device: {P.device_count()} visible; f32; L // 3 pairs per round; {REPS} timed runs per variant, alternating; "
          f"rounds per run: {ROUNDS_OF}", flush=True)
    print(f"{'instance':26s} {'L':>3s} {'ladders':>7s} {'T':>5s} {'variant':>13s} {'rounds/s':>11s} {'spin-updates/s':>15s} {'ms/run median':>14s} "
          f"{'min':>9s} {'max':>9s} {'x call by call':>14s}  route", flush=True)
    for i in INSTANCES:
        name, make, (b_lo, b_hi) = GRID[i]
        J, h = make()
        inst = P.Instance(J, h)
        for L in LS:
            for ladders in LADDERS:
                m0 = np.where(np.random.default_rng(ladders).random((L * ladders, inst.n)) < 0.5, -1, 1).astype(np.int8)
                lts = [P.distributed.LocalTempering(inst, np.geomspace(b_lo, b_hi, L), L * ladders, SEED, L // 3, [0], wave_sweeps="force",
                                                    wave_rounds=True, wave_long=True, wave_long_rounds=on) for _, on in VARIANTS]
                try:
                    for lt in lts:
                        lt.set_spins(m0)
                    for T in SWEEPS:
                        rounds = ROUNDS_OF.get(T, max(2, 2000 // T))
                        times = [[] for _ in VARIANTS]
                        for rep in range(REPS + 1):
                            for v, lt in enumerate(lts):
                                dt = timed_run(lt, T, rounds)
                                if rep > 0:                  # run 0 warms up: code objects, buffers
                                    times[v].append(dt)
                        ends = [(lt.gather_spins(), lt.slots()) for lt in lts]
                        assert np.array_equal(ends[0][0], ends[1][0]) and np.array_equal(ends[0][1], ends[1][1]), (name, L, ladders, T)
                        base = float(np.median(times[0]))
                        for v, lt in enumerate(lts):
                            med = float(np.median(times[v]))
                            print(f"{name:26s} {L:3d} {ladders:7d} {T:5d} {VARIANTS[v][0]:>13s} {rounds / med:11.1f} "
                                  f"{rounds * T * L * ladders * inst.n / med:15.3e} {med * 1e3:14.3f} {min(times[v]) * 1e3:9.3f} "
                                  f"{max(times[v]) * 1e3:9.3f} {med / base:14.2f}  {lt.rounds_routes[0]}", flush=True)
                finally:
                    for lt in lts:
                        lt.close()


if __name__ == "__main__":
    main()
