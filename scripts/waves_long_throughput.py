"""Time per update of Engine.sweep_philox on dense chains of 257 .. 1024 spins under the routes of one build: every mode off (sweep by
sweep), the chain-per-lane kernels forced, and the wave-per-chain kernels forced with set_wave_long -- the row of the dense matrix
requested on a flip only (NLMC_WAVE_LONG_AHEAD=0) and requested ahead at every update (=1).  The protocol is
scripts/wave_throughput.py's: one f32 call of 20 sweeps at a time, shared order, no outputs, construction of the visiting orders /
level schedules included, wall time around calls that end in a device synchronise, one warm-up call per engine, then the median of
five calls with min .. max.  The variants of a point are engines that take turns call by call, so that they see the same machine.

  complete Gaussian graphs (tests/wavefields.py: dense_instance) of n = 320, 512, 1024, beta = 0.1; make_instance(1024), degree 6
  rows (chains of the call): 16, 256, 1024, 4096

"us/update" is the call's time over its 20 n update steps: what one update of one chain takes while `rows` chains run beside each
other.  Usage: python scripts/waves_long_throughput.py [out.txt] [instance,...] [rows,...]  (instances: k320 k512 k1024 s1024)."""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import load_product
from helpers import make_instance
from wavefields import dense_instance
P = load_product()
S, SEED, REPS = 20, 12345, 5
ROWS = (16, 256, 1024, 4096)
# name, lane mode, wave mode, wave_long, environment at nlmc_create
VARIANTS = (("off", "off", "off", False, {}), ("lanes", "force", "off", False, {}),
            ("waves long", "off", "force", True, {"NLMC_WAVE_LONG_AHEAD": "0"}),
            ("waves long, row ahead", "off", "force", True, {"NLMC_WAVE_LONG_AHEAD": "1"}))


def instances():
    out = {}
    for n in (320, 512, 1024):
        out[f"k{n}"] = (f"complete Gaussian graph, n = {n}", *dense_instance(n, n), 0.1)
    out["s1024"] = ("make_instance(1024), degree 6", *make_instance(1024, seed=7, with_h=True, gaussian=True), 1.0)
    return out


def engines(inst, rows):
    spins = np.where(np.random.default_rng(rows).random((rows, inst.n)) < 0.5, -1, 1).astype(np.int8)
    out = []
    for name, lanes, waves, long_on, env in VARIANTS:
        os.environ.update(env)
        eng = P.Engine(inst, None, rows)
        for k in env:
            del os.environ[k]
        eng.set_lane_sweeps(lanes)
        eng.set_wave_sweeps(waves)
        eng.set_wave_long(long_on)
        eng.set_spins(spins)
        eng.energy()
        out.append(eng)
    return out


def point(inst, rows, beta):
    """{variant: (median us/update, min, max, median ms/call, route)}, the variants' calls interleaved."""
    engs = engines(inst, rows)
    times = [[] for _ in engs]
    try:
        for k in range(1 + REPS):
            for i, eng in enumerate(engs):
                t0 = time.perf_counter()
                eng.sweep_philox(S, SEED, sweep0=k * S, beta=beta, precision="f32")
                eng.energy_tracked()                   # (synchronises)
                if k > 0:                              # call 0 warms up: code objects, buffers, the dense matrix
                    times[i].append(time.perf_counter() - t0)
        routes = [eng.last_sweep_route() for eng in engs]
    finally:
        for eng in engs:
            eng.close()
    per = 1e6 / (S * inst.n)
    return {v[0]: (float(np.median(t)) * per, min(t) * per, max(t) * per, float(np.median(t)) * 1e3, r) for v, t, r in zip(VARIANTS, times, routes)}


def main():
    out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
    names = sys.argv[2].split(",") if len(sys.argv) > 2 else ["k320", "k512", "k1024", "s1024"]
    rows_list = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else ROWS

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    emit(f"{S} f32 sweeps per call, shared order, no outputs; median of {REPS} calls after a warm-up call; variants interleaved")
    emit(f"{'instance':34s} {'rows':>5s} {'variant':>22s} {'us/update':>10s} {'min':>8s} {'max':>8s} {'ms/call':>9s} {'x off':>6s} {'x lanes':>7s}  route")
    all_inst = instances()
    for key in names:
        label, J, h, beta = all_inst[key]
        inst = P.Instance(J, h)
        for rows in rows_list:
            res = point(inst, rows, beta)
            for name, r in res.items():
                emit(f"{label:34s} {rows:5d} {name:>22s} {r[0]:10.3f} {r[1]:8.3f} {r[2]:8.3f} {r[3]:9.2f} {res['off'][0] / r[0]:6.2f} "
                     f"{res['lanes'][0] / r[0]:7.2f}  {r[4]}")


if __name__ == "__main__":
    main()
