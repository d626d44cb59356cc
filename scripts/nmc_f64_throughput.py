"""Spin-updates/s of the NMC phases of NMC.run_restarts in the fp64 mode: NMC(precision="f64") with the phases on fused windows
(k_sweep_fused with phase flags), the same with NLMC_NO_FUSED64=1 (sweep by sweep), and precision="f32" for context.  Instances:
Chimera-2048/001 and DCL C8/00 (run_restarts divides them by max|J|: real-valued couplings, the opt-in real-valued variant) and a
+-J graph of N = 10^4 (the integer-threshold variant).  Device path with one fixed backbone (every tenth spin), no anneal, phases of
S sweeps; one warm-up call of one cycle, a calibration call of two, then a call of as many cycles as fill MIN_SECONDS (default
1.5) of host clock -- the call returns host arrays, so the clock stops behind the last launch.  Launch overheads of run_restarts
(minima read back per phase, hand-off) are included: this is what a user of run_restarts gets."""
import contextlib, io, math, os, sys, time
import numpy as np
import scipy.sparse as sp
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import load_product
from helpers import make_instance
P = load_product()
S, SEED = int(os.environ.get("PHASE_SWEEPS", 50)), 4242
MIN_SECONDS = float(os.environ.get("MIN_SECONDS", 1.5))
GOLD = os.path.join(REPO, "tests", "golden", "instances")


def call(obj, R, cycles, cl):
    with contextlib.redirect_stdout(io.StringIO()):
        t0 = time.perf_counter()
        obj.run_restarts(R, num_sweeps_initial=0, num_sweeps_per_NMC_phase=S, num_NMC_cycles=cycles, temp_x=20, global_beta=2.5,
                         all_clusters=cl)
        return time.perf_counter() - t0


def measure(J, h, R, precision, no_fused64):
    if no_fused64:
        os.environ["NLMC_NO_FUSED64"] = "1"
    else:
        os.environ.pop("NLMC_NO_FUSED64", None)
    try:
        N = J.shape[0]
        cl = np.arange(0, N, 10)
        obj = P.NMC(J, h, rng="philox", seed=SEED, lbp="device", precision=precision)
        seen = []
        eng_cls = P.Engine
        orig = eng_cls.sweep_philox_windows

        def spy(self, *a, **kw):
            o = orig(self, *a, **kw)
            seen.append(self.fused_last_call)
            return o
        eng_cls.sweep_philox_windows = spy
        try:
            call(obj, R, 1, cl)                              # warm-up (engine, plans, kernels' first launches)
            t2 = call(obj, R, 2, cl)                         # calibration: the cost of a cycle once warm
            cycles = max(2, math.ceil(MIN_SECONDS / max(t2 / 2, 1e-4)))
            seen.clear()
            dt = call(obj, R, cycles, cl)
            while dt < MIN_SECONDS:                          # (a call has fixed costs the calibration counted per cycle)
                cycles = math.ceil(cycles * 1.2 * MIN_SECONDS / dt)
                seen.clear()
                dt = call(obj, R, cycles, cl)
        finally:
            eng_cls.sweep_philox_windows = orig
        return R * N * S * 3 * cycles / dt, dt / (3 * cycles) * 1e3, cycles, dt, sum(seen) / max(1, len(seen))
    finally:
        os.environ.pop("NLMC_NO_FUSED64", None)


def report(name, J, h):
    print(f"{name}: N = {J.shape[0]}, phases of {S} sweeps (C, NC, ALL per cycle), backbone = every tenth spin", flush=True)
    for R in (64, 256):
        for label, prec, off in (("fp64, fused phases (new)", "f64", False), ("fp64, NLMC_NO_FUSED64=1", "f64", True),
                                 ("f32, fused", "f32", False)):
            ups, ms, cyc, dt, frac = measure(J, h, R, prec, off)
            print(f"  R = {R:3d}  {label:26s} {ups:.3e} spin-updates/s  {ms:8.3f} ms per phase  ({cyc} cycles in {dt:.2f} s, "
                  f"{frac:4.0%} of phase launches fused)", flush=True)


if __name__ == "__main__":
    print(f"device: {P.device_count()} visible", flush=True)
    W, h = P.instances.txt_to_A_droplet(os.path.join(GOLD, "chimera2048__001.txt"))
    report("Chimera-2048/001 / max|J|", sp.csr_matrix(W).astype(np.float64), np.asarray(h, dtype=np.float64).ravel())
    W, h = P.instances.txt_to_A_DCL(os.path.join(GOLD, "DCL_C8__00.txt"))
    report("DCL C8/00 / max|J|", sp.csr_matrix(W).astype(np.float64), np.asarray(h, dtype=np.float64).ravel())
    J, _ = make_instance(10_000, seed=20250225)
    report("+-J, mean degree 6", J, np.zeros(J.shape[0]))
