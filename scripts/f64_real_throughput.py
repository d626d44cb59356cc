"""Spin-updates/s of the fp64 mode on real-valued couplings: the fused-window variant (Engine.set_fused_f64_real), the
sweep-by-sweep fp64 kernel, the "f32" mode on fused windows and -- on a +-J instance of the same graph -- the integer-threshold
fp64 kernel.  Two shapes at the C4 round (10 sweeps + one swap round, 256 replicas): Chimera-2048/001 divided by max|J|
(couplings k/75) and a Gaussian instance of N = 10^4.  ROUNDS (default 20) timed rounds after WARMUP (default 2); wall time
over the rounds, planning excluded (the schedules are made before the clock starts, as RoundPlanner does)."""
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
    Jc, hc = chimera()
    report("Chimera-2048/001 / max|J|", Jc, hc)
    Jg, hg = make_instance(10_000, seed=20250225, with_h=True, gaussian=True)
    Jp = Jg.copy()
    Jp.data = np.sign(Jp.data)
    report("Gaussian", Jg, hg, pmj=(Jp, np.zeros(Jg.shape[0])))
