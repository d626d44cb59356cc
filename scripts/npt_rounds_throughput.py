"""NPT.run(rng="philox") end to end with its plain rounds handed to the engine in chunks (LocalTempering.run_rounds, the default)
against the round-by-round loop (NLMC_NO_DEFERRED=1): N = 10^4, +-J, 256 replicas, 100 rounds of 10 sweeps, return_trace=None.
The two alternate in one process, REPS (default 7) runs each after one warm-up run each; wall seconds of the whole run() call
(planning, read-out and context set-up included): median, minimum and maximum.  PRECISION: "f32" (default) or "f64"."""
import os, sys, time, contextlib, io
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import load_product
from helpers import make_instance
P = load_product()
N, R, ROUNDS, S = int(os.environ.get("N", 10_000)), 256, 100, 10
REPS, PRECISION = int(os.environ.get("REPS", 7)), os.environ.get("PRECISION", "f32")
J, h = make_instance(N, seed=20250225)
betas = np.geomspace(0.05, 4.0, R)
times, last = {"batched": [], "round by round": []}, {}
for rep in range(REPS + 1):
    for leg in times:
        if leg == "round by round":
            os.environ["NLMC_NO_DEFERRED"] = "1"
        try:
            obj = P.NPT(J, h, rng="philox", seed=5, precision=PRECISION)
            t = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                M, E = obj.run(betas, R, [False] * R, num_sweeps_MCMC=ROUNDS * S, num_sweeps_read=ROUNDS * S, num_swap_attempts=ROUNDS,
                               num_swapping_pairs=77, return_trace=None)
            dt = time.perf_counter() - t
        finally:
            os.environ.pop("NLMC_NO_DEFERRED", None)
        if rep > 0:
            times[leg].append(dt)
        last[leg] = (E, obj.final_slots)
assert np.array_equal(last["batched"][0], last["round by round"][0]) and np.array_equal(last["batched"][1], last["round by round"][1])
print(f"NPT.run, +-J N = {N}, {R} replicas, {ROUNDS} rounds of {S} sweeps, precision {PRECISION}, return_trace=None; {REPS} runs per leg, alternating")
for leg, v in times.items():
    print(f"  {leg:16s} median {np.median(v) * 1e3:8.2f}   min {min(v) * 1e3:8.2f}   max {max(v) * 1e3:8.2f} ms per run   "
          f"({R * N * ROUNDS * S / np.median(v):.3e} spin-updates/s)", flush=True)
