"""Diagnostic build only (NLMC_LIB=.../libnlmc_hip_stamps.so NLMC_STAMP_FILE=...): the level loop of k_rounds_fused against the one of
k_sweep_fused on the same windows (bench shape): cycles per level, work (fetch issue + threshold production + update) and barrier wait,
median over the chains, per wave and over the worker waves.  MODE=rounds: W rounds in one launch of k_rounds_fused; the stamps are those
of its last but one round (carried tables in, the next round's tables made in its tail) and of its last round (carried tables in,
nothing made ahead).  MODE=window: W one-window launches of k_sweep_fused, the stamps are the last one's (window W - 1 in both modes)."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from conftest import load_product
from helpers import make_instance, init_spins
P = load_product()
N, R, T, W = (int(os.environ.get(k, d)) for k, d in (('N', 10000), ('R', 256), ('T', 10), ('W', 6)))
MODE, PREC, PAIRS = os.environ.get("MODE", "rounds"), os.environ.get("PRECISION", "f64"), 77
J, h = make_instance(N)
eng = P.Engine(J, h, R)
eng.set_spins(init_spins(R, N)); eng.pt_init(np.geomspace(0.05, 4.0, R))
assert eng.plan_philox_fused(0, W, T, 7) == W
if MODE == "rounds":
    eng.pt_plan(0, W, 7, PAIRS)
    assert eng.pt_rounds_fused(W, T, 7, 0, 0, PAIRS, precision=PREC), eng.rounds_fused_refusal
else:
    for w in range(W):
        eng.sweep_philox(T, 7, sweep0=w * T, beta=None, precision=PREC)
nl = eng.last_schedule_stats()["levels"]
eng.energy()
eng.close()
d = np.fromfile(os.environ["NLMC_STAMP_FILE"], dtype=np.int64)[:R * 16 * 8].reshape(R, 16, 8)
workers = [w for w in range(16) if np.median(d[:, w, 4]) > 0]


def report(name, j_work, j_bar, j_tot, tot="prologue + loop"):
    m = lambda w, j: np.median(d[:, w, j])
    print(f"{MODE} {PREC} {name}: {nl} levels; cycles per level, median over {R} chains")
    for w in range(16):
        print(f"  wave {w:2d}: work {m(w, j_work) / nl:6.1f}  barrier-wait {m(w, j_bar) / nl:6.1f}  loop {(m(w, j_work) + m(w, j_bar)) / nl:6.1f}")
    loop = np.median([(m(w, j_work) + m(w, j_bar)) / nl for w in range(16)])
    work = np.mean([m(w, j_work) / nl for w in workers])
    print(f"  level loop {loop:6.1f} cycles per level (median over waves), work of the {len(workers)} worker waves {work:6.1f}; "
          f"{tot} {np.median(d[:, 0, j_tot]):9.0f} cycles = {np.median(d[:, 0, j_tot]) / nl:6.1f} per level", flush=True)


if MODE == "rounds":
    report(f"round {W - 2} (tables of the next round made ahead)", 1, 2, 3)
    report(f"round {W - 1} (last of the launch)", 5, 6, 7)
else:
    report(f"window {W - 1}", 5, 6, 7, "whole kernel (spins in, prologue, loop, spins out)")
