"""Rounds of LocalTempering whose marked slots run NMC cycles, on short chains: time per round of three routes that alternate in one
process --

  in launch       lane_sweeps="force", lane_nmc=True : all phases of a round in one Engine.nmc_phases_lanes call per context
  phase by phase  lane_sweeps="force", lane_nmc=False: per phase adopt_best, set_phase and a lane sweep call
  off             lane mode off: what NPT.run does without the lanes keyword

and, beside it, the phases alone: the same two lane routes on the marked chains of an engine between two device synchronises (host
clock; backbone masks installed once, no inference in the timed part).

Shapes: Wishart N = 10 (golden), a complete graph of N = 40, Chimera-128/001; ladders of 16 temperatures with the 5 coldest marked,
1 / 16 / 256 ladders; 30 phases per round (10 cycles of C, NC, ALL) of S = 1, 4, 34 sweeps, and 30 S plain sweeps per round (the
reference's split: S = ceil(sweeps per swap / 3 / num_cycles)).  REPS (default 5) timed rounds per route after one warm-up round each,
the routes alternating; median, minimum and maximum.  The three routes leave the same spins and slots, which is asserted.
ROUTES=loop times the phase-by-phase route only (a build of an earlier commit, which has no lane_nmc keyword: PRODUCT_TREE=<checkout>
loads the package from there)."""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("PRODUCT_TREE", REPO)
sys.path.insert(0, TREE); sys.path.insert(0, os.path.join(TREE, "tests")); sys.path.insert(0, os.path.join(TREE, "scripts"))
from conftest import load_product
from lane_throughput import wishart_like, chimera128
from test_gpu_lanes import wishart
P = load_product()
L, MARKED, SEED, REPS = 16, 5, 0xBEE5 + (9 << 32), int(os.environ.get("REPS", 5))
LADDERS = tuple(int(x) for x in os.environ.get("LADDERS", "1,16,256").split(","))
SWEEPS = tuple(int(x) for x in os.environ.get("SWEEPS", "1,4,34").split(","))
ONLY = os.environ.get("ROUTES", "all")
PHASES = ["C", "NC", "ALL"] * 10
ROUTES = (("in launch", "force", True), ("phase by phase", "force", False), ("off", "off", False))
if ONLY == "loop":
    ROUTES = (("phase by phase", "force", None),)
BETAS = np.geomspace(0.3, 3.0, L)
PAIRS, GBETA, TEMP_X = L // 3, 2.5, 20.0
EPS = np.finfo(float).eps
MARKS = [False] * (L - MARKED) + [True] * MARKED


def tempering(inst, ladders, lanes, lane_nmc, S):
    kw = {} if lane_nmc is None else {"lane_nmc": lane_nmc}
    lt = P.distributed.LocalTempering(inst, BETAS, L * ladders, SEED, PAIRS, [0], lane_sweeps=lanes, **kw)
    graph = P.lbp.EdgeGraph(inst)
    thr, t = [0.9999], 0.9899
    while t > 0.97:
        thr.append(t)
        t -= 0.01
    lt.configure_nmc(MARKS, PHASES, S, GBETA, TEMP_X, graph.epsilon(inst.h), P.lbp.lambda_list(3.0, 0.05, 0.8), EPS, 100,
                     float(np.tanh(19.06)) - EPS, thr)
    return lt


def timed_round(lt, n_sweeps):
    t0 = time.perf_counter()
    lt.round(n_sweeps)
    lt.engs[0].energy_tracked()                                 # (synchronises)
    return time.perf_counter() - t0


def timed_phases(eng, S, in_launch, k):
    """The phases of one round on the selected (marked) chains, between two synchronises."""
    sweep0 = (1 << 31) + k * len(PHASES) * S
    eng.subset()
    t0 = time.perf_counter()
    if in_launch:
        eng.nmc_phases_lanes(PHASES, S, SEED, sweep0, GBETA, TEMP_X)
    else:
        eng.track_minimum(True)
        for p, kind in enumerate(PHASES):
            if p > 0:
                eng.adopt_best()
            eng.set_phase(kind, TEMP_X)
            eng.sweep_philox(S, SEED, sweep0=sweep0 + p * S, beta=GBETA)
        eng.track_minimum(False)
        eng.set_phase("ALL")
    eng.subset()                                                 # (synchronises the stream the subset's work ran on)
    return time.perf_counter() - t0


def stats(ts):
    return float(np.median(ts)) * 1e3, min(ts) * 1e3, max(ts) * 1e3


def main():
    Jw, hw, _, _ = wishart(P)
    grid = [("Wishart N = 10 (golden)", Jw, hw), ("complete graph N = 40", *wishart_like(40, 2)), ("Chimera-128/001", *chimera128())]
    only = os.environ.get("INSTANCES")
    if only:
        grid = [g for i, g in enumerate(grid) if str(i) in only.split(",")]
    print(f"device: {P.device_count()} visible; product tree: {'PRODUCT_TREE' if os.environ.get('PRODUCT_TREE') else 'this one'}; L = {L}, {MARKED} coldest slots "
          f"marked, {PAIRS} pairs per round, {len(PHASES)} phases per round, 30 S plain sweeps per round; {REPS} timed rounds per route after "
          f"one warm-up round, alternating; ms: median, min, max", flush=True)
    print(f"{'instance':24s} {'ladders':>7s} {'S':>3s} {'route':>15s} {'round ms':>10s} {'min':>9s} {'max':>9s} {'phases ms':>10s} {'min':>9s} {'max':>9s}",
          flush=True)
    for name, J, h in grid:
        inst = P.Instance(J, h)
        for ladders in LADDERS:
            G = L * ladders
            m0 = np.where(np.random.default_rng(ladders).random((G, inst.n)) < 0.5, -1, 1).astype(np.int8)
            mk = np.random.default_rng(7).integers(0, 2, size=(G, inst.n)).astype(np.uint8)
            for S in SWEEPS:
                lts = [tempering(inst, ladders, lanes, ln, S) for _, lanes, ln in ROUTES]
                engs = []
                try:
                    for lt in lts:
                        lt.set_spins(m0)
                    times = [[] for _ in ROUTES]
                    for rep in range(REPS + 1):
                        for v, lt in enumerate(lts):
                            dt = timed_round(lt, 30 * S)
                            if rep > 0:                          # round 0 warms up: code objects, buffers
                                times[v].append(dt)
                    ends = [(lt.gather_spins(), lt.slots()) for lt in lts]
                    assert all(np.array_equal(e[0], ends[0][0]) and np.array_equal(e[1], ends[0][1]) for e in ends[1:]), (name, ladders, S)
                    if ONLY != "loop":
                        assert lts[0].lane_nmc_rounds == REPS + 1 and lts[1].lane_nmc_rounds == 0
                    # the phases alone, on the marked chains of engines of their own
                    lane_routes = [r for r in ROUTES if r[1] == "force"]
                    ptimes = [[] for _ in lane_routes]
                    for _ in lane_routes:
                        e = P.Engine(inst, None, G)
                        engs.append(e)
                        e.set_lane_sweeps("force")
                        e.pt_init(BETAS)
                        e.set_spins(m0)
                        e.mark_slots(MARKS)
                        e.set_cluster_mask(mk)
                        e.select("marked")
                    for rep in range(REPS + 1):
                        for v, e in enumerate(engs):
                            dt = timed_phases(e, S, bool(lane_routes[v][2]), rep)
                            if rep > 0:
                                ptimes[v].append(dt)
                    if len(engs) == 2:
                        assert np.array_equal(engs[0].get_spins(), engs[1].get_spins()), (name, ladders, S, "phases")
                    for v, (route, lanes, _) in enumerate(ROUTES):
                        r = stats(times[v])
                        p = stats(ptimes[v]) if lanes == "force" else None
                        tail = f" {p[0]:10.3f} {p[1]:9.3f} {p[2]:9.3f}" if p else f" {'-':>10s} {'-':>9s} {'-':>9s}"
                        print(f"{name:24s} {ladders:7d} {S:3d} {route:>15s} {r[0]:10.3f} {r[1]:9.3f} {r[2]:9.3f}" + tail, flush=True)
                finally:
                    for x in lts + engs:
                        x.close()


if __name__ == "__main__":
    main()
