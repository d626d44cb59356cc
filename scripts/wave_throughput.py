"""Spin-updates/s of Engine.sweep_philox on short instances under three routes of one build: every mode off (sweep by sweep), the
chain-per-lane kernels forced, the wave-per-chain kernels forced.  The protocol is scripts/lane_throughput.py's: one f32 call of 20
sweeps at a time, shared order, no outputs, construction of the visiting orders / level schedules included, wall time around calls
that end in a device synchronise, median over the calls after one warm-up call per engine.  The three variants of a point are three
engines that take turns call by call, so that they see the same machine.

  Wishart-like complete graphs of N = 16 and N = 40, tests/golden/instances/chimera128__001.txt, make_instance(255)
  rows (chains of the call): 1, 16, 64, 1024, 4096, 16384

and, for the wave route alone: the per-chain order at N = 40 x 1024 rows, NLMC_WAVE_JLDS=0 against the default at N = 40 and
Chimera-128, NLMC_WAVE_WAVES = 1 / 4 / 16 at 1024 rows (both knobs are read when an engine is created).  The last block derives
NLMC_WAVE_AUTO_MAX_ROWS from the table by the rule stated in include/nlmc.h."""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests")); sys.path.insert(0, os.path.join(REPO, "scripts"))
from conftest import load_product
from helpers import make_instance
from lane_throughput import wishart_like, chimera128
P = load_product()
S, SEED = 20, 12345
ROWS = (1, 16, 64, 1024, 4096, 16384)
MIN_TIME, MIN_REPS, MAX_REPS = float(os.environ.get("MIN_TIME", 0.1)), 5, 200
VARIANTS = (("off", "off", "off"), ("lanes", "force", "off"), ("waves", "off", "force"))      # name, lane mode, wave mode


def engines(inst, rows, variants, env=None):
    spins = np.where(np.random.default_rng(rows).random((rows, inst.n)) < 0.5, -1, 1).astype(np.int8)
    out = []
    for name, lanes, waves in variants:
        for k, v in (env or {}).get(name, {}).items():
            os.environ[k] = v
        eng = P.Engine(inst, None, rows)
        for k in (env or {}).get(name, {}):
            del os.environ[k]
        eng.set_lane_sweeps(lanes)
        eng.set_wave_sweeps(waves)
        eng.set_spins(spins)
        eng.energy()
        out.append(eng)
    return out


def rates(inst, rows, variants=VARIANTS, order="shared", env=None):
    """{variant: (spin-updates/s, median us, min us, max us, calls, route)}, the variants' calls interleaved."""
    engs = engines(inst, rows, variants, env)
    times = [[] for _ in engs]
    try:
        k, t_all = 0, 0.0
        while k < 1 + MIN_REPS or (t_all < MIN_TIME * len(engs) and k < 1 + MAX_REPS):
            for i, eng in enumerate(engs):
                t0 = time.perf_counter()
                eng.sweep_philox(S, SEED, sweep0=k * S, beta=1.0, precision="f32", order=order)
                eng.energy_tracked()                   # (synchronises)
                dt = time.perf_counter() - t0
                if k > 0:                              # call 0 warms up: code objects, buffers, the dense matrix
                    times[i].append(dt)
                    t_all += dt
            k += 1
        routes = [eng.last_sweep_route() for eng in engs]
    finally:
        for eng in engs:
            eng.close()
    res = {}
    for (name, _, _), t, route in zip(variants, times, routes):
        med = float(np.median(t))
        res[name] = (rows * inst.n * S / med, med * 1e6, min(t) * 1e6, max(t) * 1e6, len(t), route)
    return res


def show(label, rows, res):
    for name, r in res.items():
        print(f"{label:40s} {rows:6d} {name:>12s} {r[0]:15.3e} {r[1]:15.1f} {r[2]:9.1f} {r[3]:9.1f} {r[4]:6d}  {r[5]}", flush=True)


def main():
    grid = [("Wishart-like complete graph, N = 16", *wishart_like(16, 1)), ("Wishart-like complete graph, N = 40", *wishart_like(40, 2)),
            ("Chimera-128/001", *chimera128()), ("make_instance(255)", *make_instance(255))]
    insts = {name: P.Instance(J, h) for name, J, h in grid}
    print(f"device: {P.device_count()} visible; {S} f32 sweeps per call, shared order unless stated, no outputs; variants interleaved", flush=True)
    print(f"{'instance':40s} {'rows':>6s} {'variant':>12s} {'spin-updates/s':>15s} {'us/call median':>15s} {'min':>9s} {'max':>9s} {'calls':>6s}  route", flush=True)
    ratio = {}
    for name, inst in insts.items():
        for rows in ROWS:
            res = rates(inst, rows)
            show(name, rows, res)
            ratio[(name, rows)] = (res["off"][1] / res["waves"][1], res["lanes"][1] / res["waves"][1])
    n40, chim = "Wishart-like complete graph, N = 40", "Chimera-128/001"
    show(n40 + ", per-chain", 1024, rates(insts[n40], 1024, variants=VARIANTS, order="per_chain"))
    for name in (n40, chim):
        two = (("waves", "off", "force"), ("waves JLDS=0", "off", "force"))
        for rows in (64, 1024):
            show(name, rows, rates(insts[name], rows, variants=two, env={"waves JLDS=0": {"NLMC_WAVE_JLDS": "0"}}))
    for name in (n40, chim):
        three = tuple((f"waves W={w}", "off", "force") for w in (1, 4, 16))
        show(name, 1024, rates(insts[name], 1024, variants=three, env={f"waves W={w}": {"NLMC_WAVE_WAVES": str(w)} for w in (1, 4, 16)}))
    print("\ntime of the route a call takes with every mode off / time of the wave route (and lanes forced / waves):")
    for (name, rows), (a, b) in ratio.items():
        print(f"  {name:40s} {rows:6d}  {a:7.2f}x  {b:7.2f}x")
    top = 0
    for rows in ROWS:                                  # the largest measured row count up to which the margin holds everywhere
        if all(ratio[(name, rows)][0] >= 1.2 for name in insts):
            top = rows
        else:
            break
    if top == ROWS[-1]:
        top = 2 ** 31 - 1
    print(f"NLMC_WAVE_AUTO_MAX_ROWS by the 1.2x rule: {top}")


if __name__ == "__main__":
    main()
