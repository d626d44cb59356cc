"""The NMC part of a round on dense chains of 257 to 1024 spins: the phases of one round on the marked chains of an engine, between two
device synchronises (host clock; backbone masks installed once, no inference in the timed part), on two routes --

  in launch    Engine.nmc_phases_waves_long: all phases in k_nmc_phases_waves_long launches
  wave loop    set_wave_sweeps("force") + set_wave_long(): per phase adopt_best, set_phase and a long wave sweep call under track_minimum

The method is scripts/wave_nmc_throughput.py's (timed_phases): REPS (default 3) timed repeats per route after one warm-up; median, minimum
and maximum.  Each route prints a checksum of the spins it leaves: the two routes leave the same spins.

Shapes: complete +-J graphs of 320, 512 and 1024 spins; 16 / 256 / 1024 marked chains (ladders of 16 temperatures, every slot marked); 30
phases per round (10 cycles of C, NC, ALL) of S = 1, 4 and 16 sweeps.
ROUTES=loop times the wave loop only: with PRODUCT_TREE=<checkout> on a build of the parent commit, which has no nmc_phases_waves_long;
ROUTES=launch the launch only.  The default of distributed.WAVE_LONG_NMC_IN_LAUNCH is read off the "in launch" rows of this tree against
the "wave loop" rows of the parent commit's build, the two processes run in turn (parent, new, parent, new): the ratio of the medians
per shape, and the spread between the two runs of either."""
import os, sys, time, zlib
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("PRODUCT_TREE", REPO)
sys.path.insert(0, TREE); sys.path.insert(0, os.path.join(TREE, "tests")); sys.path.insert(0, os.path.join(TREE, "scripts"))
from conftest import load_product
P = load_product()
L, SEED, REPS = 16, 0xBEE5 + (9 << 32), int(os.environ.get("REPS", 3))
SIZES = tuple(int(x) for x in os.environ.get("SIZES", "320,512,1024").split(","))
CHAINS = tuple(int(x) for x in os.environ.get("CHAINS", "16,256,1024").split(","))
SWEEPS = tuple(int(x) for x in os.environ.get("SWEEPS", "1,4,16").split(","))
ONLY = os.environ.get("ROUTES", "all")
PHASES = ["C", "NC", "ALL"] * 10
ROUTES = {"loop": ("wave loop",), "launch": ("in launch",)}.get(ONLY, ("in launch", "wave loop"))
BETAS = np.geomspace(0.3, 3.0, L)
TEMP_X = 20.0


def complete(n):
    A = np.triu(np.random.default_rng(n).choice([-1.0, 1.0], size=(n, n)), 1)
    return A + A.T, np.zeros(n)


def timed_phases(eng, S, route, k, gbeta):
    """The phases of one round on the selected (marked) chains, between two synchronises."""
    sweep0 = (1 << 31) + k * len(PHASES) * S
    eng.subset()
    t0 = time.perf_counter()
    if route == "in launch":
        eng.nmc_phases_waves_long(PHASES, S, SEED, sweep0, gbeta, TEMP_X)
    else:
        eng.track_minimum(True)
        for p, kind in enumerate(PHASES):
            if p > 0:
                eng.adopt_best()
            eng.set_phase(kind, TEMP_X)
            eng.sweep_philox(S, SEED, sweep0=sweep0 + p * S, beta=gbeta)
        eng.track_minimum(False)
        eng.set_phase("ALL")
    eng.subset()                                                 # (synchronises the stream the subset's work ran on)
    return time.perf_counter() - t0


def stats(ts):
    return float(np.median(ts)) * 1e3, min(ts) * 1e3, max(ts) * 1e3


def main():
    print(f"device: {P.device_count()} visible; product tree: {'PRODUCT_TREE' if os.environ.get('PRODUCT_TREE') else 'this one'}; "
          f"{len(PHASES)} phases per round on the marked chains; {REPS} timed repeats per route after one warm-up; "
          f"ms: median, min, max", flush=True)
    print(f"{'instance':24s} {'chains':>7s} {'S':>3s} {'route':>12s} {'phases ms':>10s} {'min':>9s} {'max':>9s} {'spins crc':>10s}", flush=True)
    for n in SIZES:
        name, (J, h), gbeta = f"complete +-J N = {n}", complete(n), 2.5 / np.sqrt(n)
        inst = P.Instance(J, h)
        for G in CHAINS:
            m0 = np.where(np.random.default_rng(G).random((G, inst.n)) < 0.5, -1, 1).astype(np.int8)
            mk = np.random.default_rng(7).integers(0, 2, size=(G, inst.n)).astype(np.uint8)
            for S in SWEEPS:
                engs = []
                try:
                    for route in ROUTES:
                        e = P.Engine(inst, None, G)
                        engs.append(e)
                        if route == "wave loop":
                            e.set_wave_sweeps("force")
                            e.set_wave_long()
                        e.pt_init(BETAS)
                        e.set_spins(m0)
                        e.mark_slots(np.ones(L, dtype=bool))
                        e.set_cluster_mask(mk)
                        e.select("marked")
                    times = [[] for _ in ROUTES]
                    for rep in range(REPS + 1):
                        for v, e in enumerate(engs):
                            dt = timed_phases(e, S, ROUTES[v], rep, gbeta)
                            if rep > 0:                          # repeat 0 warms up: code objects, buffers, the dense matrix
                                times[v].append(dt)
                    ends = [e.get_spins() for e in engs]
                    assert all(np.array_equal(x, ends[0]) for x in ends[1:]), (name, G, S)
                    for v, route in enumerate(ROUTES):
                        assert engs[v].last_sweep_route() == "waves"
                        r = stats(times[v])
                        print(f"{name:24s} {G:7d} {S:3d} {route:>12s} {r[0]:10.3f} {r[1]:9.3f} {r[2]:9.3f} {zlib.crc32(ends[v].tobytes()):10d}",
                              flush=True)
                finally:
                    for x in engs:
                        x.close()


if __name__ == "__main__":
    main()
