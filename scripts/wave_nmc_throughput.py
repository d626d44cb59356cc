"""The NMC part of a round on short dense chains: the phases of one round on the marked chains of an engine, between two device
synchronises (host clock; backbone masks installed once, no inference in the timed part), on three routes that alternate in one process --

  in launch    Engine.nmc_phases_waves: all phases in one k_nmc_phases_waves launch
  wave loop    set_wave_sweeps("force"): per phase adopt_best, set_phase and a wave sweep call under track_minimum
  lane launch  Engine.nmc_phases_lanes on the same chains: all phases in one k_nmc_phases_lanes launch

The method is scripts/lane_nmc_throughput.py's (timed_phases): REPS (default 5) timed repeats per route after one warm-up, the routes
alternating; median, minimum and maximum.  The routes leave the same spins, which is asserted.

Shapes: Wishart N = 10 (golden), complete +-J graphs of 40, 128 and 256 spins; 16 / 256 / 4096 marked chains (ladders of 16 temperatures,
every slot marked); 30 phases per round (10 cycles of C, NC, ALL) of S = 1 and S = 4 sweeps.
ROUTES=loop times the wave loop only: with PRODUCT_TREE=<checkout> on a build of an earlier commit, which has no nmc_phases_waves.  The
default of distributed.WAVE_NMC_IN_LAUNCH is read off the "in launch" rows against the "wave loop" rows of the parent commit's build."""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("PRODUCT_TREE", REPO)
sys.path.insert(0, TREE); sys.path.insert(0, os.path.join(TREE, "tests")); sys.path.insert(0, os.path.join(TREE, "scripts"))
from conftest import load_product
from test_gpu_lanes import wishart
P = load_product()
L, SEED, REPS = 16, 0xBEE5 + (9 << 32), int(os.environ.get("REPS", 5))
CHAINS = tuple(int(x) for x in os.environ.get("CHAINS", "16,256,4096").split(","))
SWEEPS = tuple(int(x) for x in os.environ.get("SWEEPS", "1,4").split(","))
ONLY = os.environ.get("ROUTES", "all")
PHASES = ["C", "NC", "ALL"] * 10
ROUTES = ("wave loop",) if ONLY == "loop" else ("in launch", "wave loop", "lane launch")
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
        eng.nmc_phases_waves(PHASES, S, SEED, sweep0, gbeta, TEMP_X)
    elif route == "lane launch":
        eng.nmc_phases_lanes(PHASES, S, SEED, sweep0, gbeta, TEMP_X)
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
    Jw, hw, _, _ = wishart(P)
    grid = [("Wishart N = 10 (golden)", Jw, hw, 2.5)] + [(f"complete +-J N = {n}", *complete(n), 2.5 / np.sqrt(n)) for n in (40, 128, 256)]
    only = os.environ.get("INSTANCES")
    if only:
        grid = [g for i, g in enumerate(grid) if str(i) in only.split(",")]
    print(f"device: {P.device_count()} visible; product tree: {'PRODUCT_TREE' if os.environ.get('PRODUCT_TREE') else 'this one'}; "
          f"{len(PHASES)} phases per round on the marked chains; {REPS} timed repeats per route after one warm-up, alternating; "
          f"ms: median, min, max", flush=True)
    print(f"{'instance':24s} {'chains':>7s} {'S':>3s} {'route':>12s} {'phases ms':>10s} {'min':>9s} {'max':>9s}", flush=True)
    for name, J, h, gbeta in grid:
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
                    if "wave loop" in ROUTES:
                        assert engs[ROUTES.index("wave loop")].last_sweep_route() == "waves"
                    for v, route in enumerate(ROUTES):
                        r = stats(times[v])
                        print(f"{name:24s} {G:7d} {S:3d} {route:>12s} {r[0]:10.3f} {r[1]:9.3f} {r[2]:9.3f}", flush=True)
                finally:
                    for x in engs:
                        x.close()


if __name__ == "__main__":
    main()
