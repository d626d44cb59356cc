"""Spin-updates/s of the fp64 mode on real-valued couplings: the fused-window variant (Engine.set_fused_f64_real), the
sweep-by-sweep fp64 kernel, the "f32" mode on fused windows and -- on a +-J instance of the same graph -- the integer-threshold
fp64 kernel.  Two shapes at the C4 round (10 sweeps + one swap round, 256 replicas): Chimera-2048/001 divided by max|J|
(couplings k/75) and a Gaussian instance of N = 10^4.  ROUNDS (default 20) timed rounds after WARMUP (default 2); wall time
over the rounds, planning excluded (the schedules are made before the clock starts, as RoundPlanner does).

The rounds leg (LEGS=rounds alone, LEGS=sweeps without it; default both): the same rounds through Engine.pt_rounds_deferred on its
two routes -- inside k_rounds_fused launches (the real-valued variant) and one launch per round (an engine created with
NLMC_NO_PERSISTENT=1) -- on two engines with the same plans, alternating, REPS (default 11) calls of CALL_ROUNDS (default 50) rounds
each after one warm-up call; microseconds per round: median, minimum and maximum over the calls."""
import os, sys, time
import numpy as np
import scipy.sparse as sp
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import load_product
from helpers import make_instance, init_spins
P = load_product()
R, T, PAIRS, SEED = 256, 10, 77, 12345
ROUNDS, WARMUP = int(os.environ.get("ROUNDS", 20)), int(os.environ.get("WARMUP", 2))


def chimera():
    W, h = P.instances.txt_to_A_droplet(os.path.join(REPO, "tests", "golden", "instances", "chimera2048__001.txt"))
    J = sp.csr_matrix(W).astype(np.float64)
    s = np.max(np.abs(J.data))
    J = (J / s).tocsr()
    J.sort_indices()
    return J, np.asarray(h, dtype=np.float64).ravel() / s


def measure(J, h, precision, fused, real):
    inst = P.Instance(J, h)
    N = inst.n
    n_rounds = WARMUP + ROUNDS
    with P.Engine(inst, None, R) as eng:
        eng.set_fused_f64_real(real)
        eng.set_spins(init_spins(R, N))
        eng.pt_init(np.geomspace(0.05, 4.0, R))
        if fused:
            planned = eng.plan_philox_fused(0, n_rounds, T, SEED)
            assert planned == n_rounds, "no fused plan"
            assert precision == "f32" or precision in eng.fused_modes(T), "the fp64 mode does not run on fused windows here"
        else:
            eng.plan_philox(0, n_rounds * T, SEED, precision=precision)
        eng.pt_plan(0, n_rounds, SEED, PAIRS)
        lv = []
        for r in range(n_rounds):
            if r == WARMUP:
                eng.get_spins()                        # (synchronises)
                t0 = time.perf_counter()
            eng.sweep_philox(T, SEED, sweep0=r * T, beta=None, precision=precision)
            st = eng.last_schedule_stats()
            lv.append(st["levels"] / max(1, st["orders"]))
            eng.pt_swap_philox(r, SEED, PAIRS, want_log=False)
        eng.get_spins()
        dt = time.perf_counter() - t0
    return R * N * T * ROUNDS / dt, dt / ROUNDS * 1e6, float(np.mean(lv))


def rounds_leg(name, J, h):
    reps, k = int(os.environ.get("REPS", 11)), int(os.environ.get("CALL_ROUNDS", 50))
    inst = P.Instance(J, h)
    engs = {}
    try:
        for route in ("in launch", "launch per round"):
            if route == "launch per round":
                os.environ["NLMC_NO_PERSISTENT"] = "1"          # (read when the engine is created)
            try:
                eng = P.Engine(inst, None, R)
            finally:
                os.environ.pop("NLMC_NO_PERSISTENT", None)
            engs[route] = eng
            eng.set_fused_f64_real(True)
            eng.set_spins(init_spins(R, inst.n))
            eng.pt_init(np.geomspace(0.05, 4.0, R))
            assert eng.plan_philox_fused(0, k, T, SEED) == k and "f64" in eng.fused_modes(T), "no fused fp64 plan"
            eng.pt_plan(0, k, SEED, PAIRS)
        times = {route: [] for route in engs}
        forced = False
        for rep in range(reps + 1):
            for route, eng in engs.items():
                t0 = time.perf_counter()
                assert eng.pt_rounds_deferred(k, T, SEED, 0, 0, PAIRS, precision="f64"), eng.rounds_fused_refusal
                if route == "in launch" and eng.last_rounds_route() != route:
                    # (the default keeps a launch per round for real-valued instances: this leg asks for the kernel by name.  The
                    # call above ran the other route; it is not counted)
                    eng.pt_check()
                    forced = True
                    t0 = time.perf_counter()
                    assert eng.pt_rounds_fused(k, T, SEED, 0, 0, PAIRS, precision="f64"), eng.rounds_fused_refusal
                assert eng.last_rounds_route() == route
                eng.pt_check()                             # (synchronises)
                if rep > 0:
                    times[route].append((time.perf_counter() - t0) / k * 1e6)
    finally:
        for eng in engs.values():
            eng.close()
    print(f"{name}: N = {inst.n}, {R} replicas, rounds of {T} sweeps + one swap round ({PAIRS} pairs), fp64 real-valued; "
          f"{reps} calls of {k} rounds per route, alternating" + ("; in launch through pt_rounds_fused" if forced else ""), flush=True)
    for route, v in times.items():
        print(f"  pt_rounds_deferred, {route:18s} median {np.median(v):8.1f}   min {min(v):8.1f}   max {max(v):8.1f} us per round", flush=True)


def report(name, J, h, pmj=None):
    rows = [("fp64 fused, real couplings (new)", J, h, "f64", True, True),
            ("fp64 sweep by sweep", J, h, "f64", False, False),
            ("f32 fused", J, h, "f32", True, False)]
    if pmj is not None:
        rows.append(("fp64 fused, integer thresholds (+-J graph)", pmj[0], pmj[1], "f64", True, False))
    print(f"{name}: N = {J.shape[0]}, {R} replicas, rounds of {T} sweeps + one swap round ({PAIRS} pairs), {ROUNDS} rounds", flush=True)
    for label, Jm, hm, prec, fused, real in rows:
        ups, us, lv = measure(Jm, hm, prec, fused, real)
        print(f"  {label:46s} {ups:.3e} spin-updates/s   {us:9.1f} us per round   {lv:6.2f} levels per sweep", flush=True)


if __name__ == "__main__":
    print(f"device: {P.device_count()} visible", flush=True)
    legs = os.environ.get("LEGS", "sweeps,rounds").split(",")
    Jc, hc = chimera()
    Jg, hg = make_instance(10_000, seed=20250225, with_h=True, gaussian=True)
    if "sweeps" in legs:
        report("Chimera-2048/001 / max|J|", Jc, hc)
        Jp = Jg.copy()
        Jp.data = np.sign(Jp.data)
        report("Gaussian", Jg, hg, pmj=(Jp, np.zeros(Jg.shape[0])))
    if "rounds" in legs:
        rounds_leg("Chimera-2048/001 / max|J|", Jc, hc)
        rounds_leg("Gaussian", Jg, hg)
