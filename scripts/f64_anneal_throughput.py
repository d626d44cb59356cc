"""Spin-updates/s of an fp64 anneal: Engine.sweep_philox_windows(10^3 sweeps, beta = [R, S] table of hostlogic.beta_schedule(S, 2.5,
anneal=True), precision="f64", running minimum + argmin state as NMC.run_restarts asks for them) as fused_route sends it (fused
windows with a temperature per sweep for the integer-threshold variant, sweep by sweep for real-valued instances), the same with
NLMC_NO_FUSED64=1 (sweep by sweep), precision="f32" for scale, and the fp64 call with ONE temperature per chain (beta = 2.5
throughout: the output kernels the anneal shares its code with).  Instances: a +-J graph of N = 10^4 (the integer-threshold variant
with its ring of K tables), Chimera-2048/001 and DCL C8/00 divided by max|J| as run() does (real-valued couplings, the real-valued
option switched on).  64 and 256 chains.  One warm-up call, then REPEATS (default 5)
timed calls at consecutive sweep indices; a call plans its windows, sweeps and returns host arrays, so the clock stops behind the last
launch and planning is included: this is what a caller of the anneal gets.  Median and spread (min .. max) per case."""
import os, statistics, sys, time
import numpy as np
import scipy.sparse as sp
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import load_product
from helpers import make_instance, init_spins
P = load_product()
S, SEED = int(os.environ.get("ANNEAL_SWEEPS", 1000)), 4242
REPEATS = int(os.environ.get("REPEATS", 5))
GOLD = os.path.join(REPO, "tests", "golden", "instances")


def measure(J, h, R, precision, no_fused64, flat=False):
    if no_fused64:
        os.environ["NLMC_NO_FUSED64"] = "1"
    else:
        os.environ.pop("NLMC_NO_FUSED64", None)
    try:
        N = J.shape[0]
        beta = np.full((R, S), 2.5) if flat else np.repeat(P.hostlogic.beta_schedule(S, 2.5, True, 1, 0)[None, :], R, axis=0)
        with P.Engine(P.Instance(J, h), None, R) as eng:
            eng.set_fused_f64_real(True)
            eng.set_spins(init_spins(R, N))
            times, fused = [], []
            for i in range(REPEATS + 1):
                t0 = time.perf_counter()
                eng.sweep_philox_windows(S, SEED, sweep0=i * S, beta=beta, want_min=True, want_state=True, precision=precision)
                times.append(time.perf_counter() - t0)
                fused.append(eng.fused_last_call)
            st = eng.last_schedule_stats()
        ups = sorted(R * N * S / t for t in times[1:])             # (the first call is the warm-up)
        return statistics.median(ups), ups[0], ups[-1], statistics.median(times[1:]) * 1e3, all(fused), st["levels"] / max(1, st["orders"])
    finally:
        os.environ.pop("NLMC_NO_FUSED64", None)


def report(name, J, h):
    print(f"{name}: N = {J.shape[0]}, anneal of {S} sweeps, {REPEATS} repeats", flush=True)
    for R in (64, 256):
        for label, prec, off, flat in (("fp64 anneal", "f64", False, False), ("fp64, NLMC_NO_FUSED64=1", "f64", True, False),
                                       ("f32 anneal", "f32", False, False), ("fp64, one temperature", "f64", False, True)):
            med, lo, hi, ms, fz, lv = measure(J, h, R, prec, off, flat)
            print(f"  R = {R:3d}  {label:24s} {med:.3e} spin-updates/s  (min {lo:.3e} .. max {hi:.3e})  {ms:8.2f} ms per call  "
                  f"{lv:6.1f} levels per sweep  fused: {fz}", flush=True)


def normalised(W, h):
    J = sp.csr_matrix(W).astype(np.float64)
    s = np.max(np.abs(J.data))
    J = (J / s).tocsr()
    J.sort_indices()
    return J, np.asarray(h, dtype=np.float64).ravel() / s


if __name__ == "__main__":
    print(f"device: {P.device_count()} visible", flush=True)
    J, _ = make_instance(10_000, seed=20250225)
    report("+-J, mean degree 6", J, np.zeros(J.shape[0]))
    report("Chimera-2048/001 / max|J|", *normalised(*P.instances.txt_to_A_droplet(os.path.join(GOLD, "chimera2048__001.txt"))))
    report("DCL C8/00 / max|J|", *normalised(*P.instances.txt_to_A_DCL(os.path.join(GOLD, "DCL_C8__00.txt"))))
