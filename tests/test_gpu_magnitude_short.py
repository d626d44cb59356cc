"""The coupling-magnitude family (tests/scalefamily.py) through every short-chain route: the chain-per-lane kernels (k_sweep_lanes,
k_rounds_lanes, k_nmc_phases_lanes) and the chain-per-wave kernels (k_sweep_waves, k_sweep_waves_long, k_rounds_waves,
k_rounds_waves_long, k_nmc_phases_waves).  Each of them has its own copy of the fixed-point update -- z = scale_cb(cb, qinv) X, the
energy delta (X - Xd) (so - sn) << eshift, the lane route's 24-bit multiply, the wave routes' X += d Jc in int32 registers or LDS --
and their own test files run at order-one couplings (qs 0 or 22, escale 51).  Here: a negative field scale (qs = -29, -18, -7),
eshift = escale - qs at 0, at 29 and between, an instance without couplings, and complete graphs whose local fields start within
1 % of the int32 limit (one chain of every dense case starts from scalefamily.aligned_state, one from the same state with spin 0
against its field: it flips in the first sweep with |X_0| above 2^30, an energy delta whose factor 2 |X_0| is beyond int32).

The only reference is the sequential oracle (oracle/nlo.c, oracle/pt.py; pinned at these magnitudes by test_scale_rule_cpu.py and
test_magnitude_short_cpu.py) -- never another device route.  Every case names the route it ran on, compares the device scales with
the oracle's, and asserts bit-equality of every sweep's spins, the energy trace, the final spins and the tracked energy (rounds: the
slots and the swap log too; NMC: every phase's minimum and argmin and the last best state), that every chain moved, and in the
"f32" mode the integer account tracked_end - tracked_start == exact_efix(end) - exact_efix(start), read as integers.  The case set
and its start states are in tests/magshort.py; test_magnitude_short_cpu.py checks there what the set covers."""
import numpy as np
import pytest

import magshort as mc
import oracle
import scalefamily as sf
from fake_engine import OracleEngine
from test_gpu_lane_nmc import SEED as NMC_SEED, SWEEP0, TEMP_X, masks
from test_gpu_lanes import nmc_flags
from test_gpu_magnitude import exact_start, raw_tracked, units

pytestmark = pytest.mark.gpu
SEED = mc.SEED
S = 3                                    # sweeps of a sweep case, of a round, of a phase
ROUNDS = 4
KINDS = ["C", "NC", "ALL"]


def lanes(eng):
    eng.set_lane_sweeps("force")


def waves(eng):
    eng.set_wave_sweeps("force")


def waves_long(eng):
    eng.set_wave_sweeps("force")
    eng.set_wave_long()


def integer_account(name, n, precision, m0, final, start, end):
    """"f32": no unit of 2^-escale lost between the start and the end of the run, whatever eshift is; on a dyadic member the
    tracked energy IS the quantised model's."""
    if precision != "f32":
        return
    q0, q1 = [mc.exact_efix(name, n, s) for s in m0], [mc.exact_efix(name, n, s) for s in final]
    assert [a - b for a, b in zip(end, start)] == [a - b for a, b in zip(q1, q0)]
    J, h, _, _, (qs, _) = mc.instance(name, n)
    if name in sf.DYADIC:
        assert exact_start(J, h, qs) and end == q1


# ---- sweeps --------------------------------------------------------------------------------------------------------------------------

def sweeps_vs_oracle(product, case, modes, route, flagged=False):
    name, n, precision = case
    J, h, beta, csr, (qs, escale) = mc.instance(name, n)
    f64 = precision == "f64"
    m0 = mc.start_spins(name, n, mc.ROWS)
    flags = nmc_flags(mc.ROWS, csr.n, m0) if flagged else None
    with product.Engine(J, h, mc.ROWS) as eng:
        assert (eng.field_scale, eng.energy_scale) == (qs, escale)
        modes(eng)
        eng.set_spins(m0)
        start = units(eng.energy(), escale)
        if flagged:
            eng.set_flags(flags, TEMP_X)
        o = eng.sweep_philox(S, SEED, beta=beta, precision=precision, record_stride=1, want_energy=True)
        assert eng.last_sweep_route() == route
        tracked, final = eng.energy_tracked(), eng.get_spins()
        eng.set_flags(None)
        end = raw_tracked(eng)
    cb = np.tile(np.array(oracle.cb_pair(beta, TEMP_X if flagged else 1.0, f64)), (S, 1))
    for c in range(mc.ROWS):
        M, s_fin, tr = oracle.sweeps_philox(csr, h, m0[c], cb, SEED, c, flags=None if flags is None else flags[c], escale=escale,
                                            use_f64=f64, efix0=start[c])
        assert np.array_equal(o["spins"][c], M), (case, c)
        assert np.array_equal(o["energy"][c], tr * 2.0 ** -escale), (case, c)
        assert np.array_equal(final[c], s_fin) and tracked[c] == tr[-1] * 2.0 ** -escale and end[c] == int(tr[-1])
        assert not np.array_equal(s_fin, m0[c])                                     # the chain moved
        if mc.is_dense(name) and c == mc.OPPOSED:               # spin 0 flipped in the first sweep with its field at the limit
            assert M[0][0] == -m0[c][0] and mc.field_at_first_visit(name, n, m0[c], M[0]) >= mc.FLIP_FLOOR[name]
    if flagged:
        assert set(np.unique(flags)) == {0, 1, 2, 3} and np.array_equal(final[flags >= 2], m0[flags >= 2])
        assert any(not np.array_equal(final[c][flags[c] == 1], m0[c][flags[c] == 1]) for c in range(mc.ROWS))   # scaled spins moved
    integer_account(name, n, precision, m0, final, start, end)


@pytest.mark.parametrize("case", mc.LANE_SWEEPS, ids=mc.case_id)
def test_lane_sweeps(product, case):
    """k_sweep_lanes in both arithmetics.  flat1024 and flat256h hold the largest |Jq| the 24-bit multiply sees (2^21 and 2^22)."""
    sweeps_vs_oracle(product, case, lanes, "lanes")


def test_lane_sweeps_with_phase_flags(product):
    """x1e9 with scaled and frozen spins, temp_x = 20: the second inverse temperature under qinv = 2^7."""
    assert mc.instance(*mc.LANE_FLAGGED[:2])[4][0] == -7
    sweeps_vs_oracle(product, mc.LANE_FLAGGED, lanes, "lanes", flagged=True)


@pytest.mark.parametrize("case", mc.WAVE_SWEEPS, ids=mc.case_id)
def test_wave_sweeps(product, case):
    """k_sweep_waves: two fields per lane at n = 100, one at n = 50 (no couplings: an empty matrix), four at flat192h (the last
    matrix staged in LDS) and flat256h (rows from global memory)."""
    sweeps_vs_oracle(product, case, waves, "waves")


@pytest.mark.parametrize("case", mc.LONG_SWEEPS, ids=mc.case_id)
def test_long_wave_sweeps(product, case):
    """k_sweep_waves_long: eight fields per lane at n = 300, sixteen at 513 and 1024."""
    sweeps_vs_oracle(product, case, waves_long, "waves")


# ---- tempering rounds in one launch --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", mc.ROUNDS, ids=mc.case_id)
def test_rounds_in_one_launch(product, case):
    """Two ladders of four, four rounds of three sweeps, one pair per round, against the oracle double round by round."""
    entry, name, n, precision = case
    J, h, beta, csr, (qs, escale) = mc.instance(name, n)
    L, G = mc.LADDER, mc.LADDER * mc.LADDERS
    betas = beta * np.linspace(0.9, 1.1, L)
    m0 = mc.start_spins(name, n, G)
    route = {"pt_rounds_lanes": "lanes", "pt_rounds_waves": "waves", "pt_rounds_waves_long": "waves long"}[entry]
    with product.Engine(J, h, G) as eng:
        assert (eng.field_scale, eng.energy_scale) == (qs, escale)
        eng.pt_init(betas)
        eng.set_spins(m0)
        start = units(eng.energy(), escale)
        eng.pt_plan(0, ROUNDS, SEED, 1)
        eng.pt_log_begin(0, ROUNDS, 1)
        assert getattr(eng, entry)(ROUNDS, S, SEED, 0, 0, 1, precision=precision), getattr(eng, "rounds_fused_refusal", "")
        assert eng.last_rounds_route() == route and eng.last_sweep_route() == ("lanes" if route == "lanes" else "waves")
        eng.pt_check()
        pairs, acc = eng.pt_log_read()
        final, slots, tracked = eng.get_spins(), eng.pt_slots(), eng.energy_tracked()
        end = raw_tracked(eng, betas)
        inst = eng.inst
    o = OracleEngine(inst, G, 0, G)
    assert o.esc == escale
    o.pt_init(betas)
    o.set_spins(m0)
    o.efix = np.array(start, dtype=np.int64)                   # the start the device has: rint(its own fp64 energies 2^escale)
    e_pairs, e_acc = [], []
    for r in range(ROUNDS):
        o.sweep_philox(S, SEED, sweep0=r * S, precision=precision)
        p, a = o.pt_swap_philox(r, SEED, 1)
        e_pairs.append(p)
        e_acc.append(a)
    assert np.array_equal(pairs, np.stack(e_pairs)) and np.array_equal(acc, np.stack(e_acc))
    assert np.array_equal(slots, o.pt_slots()) and np.array_equal(final, o.get_spins())
    assert end == [int(x) for x in o.efix] and np.array_equal(tracked, o.energy_tracked())
    assert acc.sum() > 0 and not np.array_equal(slots, np.arange(G) % L)            # swaps were accepted
    assert all(not np.array_equal(final[c], m0[c]) for c in range(G))               # every chain moved
    integer_account(name, n, precision, m0, final, start, end)


# ---- NMC phase cycles in one launch --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", mc.NMC, ids=mc.case_id)
def test_nmc_phase_cycles(product, case):
    """Phases C, NC, ALL of three sweeps, temp_x = 20 (the backbone's inverse temperature under qinv), an empty, a full and random
    backbones: flagged oracle sweeps with the np.argmin hand-off between the phases."""
    entry, name, n, precision = case
    J, h, beta, csr, (qs, escale) = mc.instance(name, n)
    rows = mc.ROWS
    m0, mk = mc.start_spins(name, n, rows), masks(rows, csr.n)
    with product.Engine(J, h, rows) as eng:
        assert (eng.field_scale, eng.energy_scale) == (qs, escale)
        eng.set_spins(m0)
        eng.set_cluster_mask(mk)
        start = units(eng.energy(), escale)
        assert getattr(eng, entry + "_refusal")(S) is None
        out = getattr(eng, entry)(KINDS, S, NMC_SEED, SWEEP0, beta, TEMP_X, precision=precision, want_minima=True, want_last_best=True)
        assert eng.last_sweep_route() == {"nmc_phases_lanes": "lanes", "nmc_phases_waves": "waves"}[entry]
        final, tracked = eng.get_spins(), eng.energy_tracked()
        end = raw_tracked(eng)
    cb = np.tile(np.array(oracle.cb_pair(beta, TEMP_X)), (S, 1))
    inv = 2.0 ** -escale
    for c in range(rows):
        s, e0 = m0[c].copy(), start[c]
        for p, kind in enumerate(KINDS):
            m = mk[c].astype(bool)
            fl = None if kind == "ALL" else (np.where(m, 1, 2) if kind == "C" else np.where(m, 2, 0)).astype(np.uint8)
            M, s_fin, tr = oracle.sweeps_philox(csr, h, s, cb, NMC_SEED, c, sweep0=SWEEP0 + p * S, flags=fl, escale=escale, efix0=e0)
            t = int(np.argmin(tr))                                # first minimum, as np.argmin has it
            assert out["phase_argmin"][c, p] == t and out["phase_min"][c, p] == int(tr[t]) * inv, (case, c, p)
            s, e0 = M[t].copy(), int(tr[t])
        assert np.array_equal(out["last_best"][c], s)
        assert np.array_equal(final[c], s_fin) and tracked[c] == tr[-1] * inv and end[c] == int(tr[-1])
        assert not np.array_equal(s_fin, m0[c])
    integer_account(name, n, precision, m0, final, start, end)
