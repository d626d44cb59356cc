"""The fixed-point scales and the energy bookkeeping of the engine across coupling magnitudes (tests/scalefamily.py: one Gaussian
instance scaled from 1e-20 to 3e15, a hub row, |h| >> |J|, dyadic instances, couplings that all quantise to 0, fields only).  Every
other GPU test runs at qs 0 or 22 and escale 51; here qs goes from -29 to 52, eshift = escale - qs from 0 to 29.

The references are the sequential oracle (oracle/nlo.c, oracle/pt.py; pinned at these magnitudes by test_scale_rule_cpu.py) and the
Python-int / Fraction energies of scalefamily.py -- never another device route.

Tracked energies of the "f32" mode.  The engine starts a chain's tracked energy from the fp64 energy of the REAL (J, h)
(nlmc_set_spins, nlmc_energy: efix = rint(E 2^escale)) and from there adds the exact deltas of the QUANTISED model (DESIGN.md
section 2: "exact for the quantised model, i.e. within 2^-(qs+1) (nnz/2 + n) of the fp64 energy of (J, h) with no drift").  So the
integer identity that holds on every member is
    tracked_end - tracked_start == exact_efix_f32(end) - exact_efix_f32(start)            (no unit lost, whatever eshift is)
and tracked_end == exact_efix_f32(end) itself only where the start's fp64 energy is the quantised one (every J and h a multiple
of 2^-qs: the dyadic members).  The first is asserted on every member together with the bound on the start's offset, the second
where it can hold.  The integers are read as integers (raw_tracked): energy_tracked() returns doubles."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import oracle
import scalefamily as sf
from helpers import init_spins
from oracle.pt import swap_round

pytestmark = pytest.mark.gpu
SEED = 0x5CA1E
R, S, T = 3, 5, 5
LOG2E = 1.4426950408889634


@functools.lru_cache(maxsize=None)
def case(name, n=None):
    J, h, beta = sf.member(name, n)
    csr = oracle.Csr(J)
    return J, h, beta, csr, oracle.field_scale(csr, h)


def efix_of(J, h, spins, qs, escale):
    return [sf.exact_efix_f32(J, h, s, qs, escale) for s in spins]


def units(E, escale):
    """What nlmc_set_spins / nlmc_energy leave as tracked integers: rint(E 2^escale) of the fp64 energies they computed."""
    return [int(round(Fraction(float(x)) * (1 << escale))) for x in E]


def raw_tracked(eng, betas=None):
    """The tracked energies as the int64 the engine holds, by chain (energy_tracked() converts them to double, which drops the low
    bits of an integer above 2^53: at escale 51 an energy of 20 is one).  Read through nlmc_apt_pack, which hands the integers out
    by (ladder, slot); declaring the context a one-block ladder re-keys the random numbers of LATER calls, so this is the last thing
    a test does with an engine (or the first, where no bits are compared with the oracle)."""
    if betas is None:
        betas = np.arange(1.0, eng.n_chains + 1.0)
        eng.pt_init(betas)
    eng.apt_shard(np.asarray(betas, dtype=np.float64), 1, 0)
    e, _, _ = eng.apt_pack(want_configs=False)
    L, slots = eng.ladder_len, eng.pt_slots()
    return [int(e[c // L, slots[c]]) for c in range(eng.n_chains)]


def exact_start(J, h, qs):
    """Is the fp64 energy of (J, h) the energy of the quantised model?  (every value an exact multiple of 2^-qs)"""
    rows, hq = sf.quantise(J, h, qs)
    rf, hf = sf._parts(J, h)
    return (all(sf._scaled(v, qs) == q for r, rq in zip(rf, rows) for (_, v), (_, q) in zip(r, rq))
            and all(sf._scaled(v, qs) == q for v, q in zip(hf, hq)))


# ---- a. the scale rule on the device ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sf.NAMES)
def test_device_scales_are_the_oracles(product, name):
    """nlmc_create's scales (with its one-pass common-power-of-two shortcut, which the oracle does not have) == oracle.field_scale
    == the pinned pair."""
    J, h, _, _, scales = case(name)
    with product.Engine(J, h, 1) as eng:
        assert (eng.field_scale, eng.energy_scale) == scales == sf.PINNED[name]


# ---- b, c. sweeps against the oracle -------------------------------------------------------------------------------------------------

def sweeps_vs_oracle(product, name, precision, fused=False, real=False, n=None, declined=False):
    """R chains, S sweeps at beta_unit with every per-sweep output: spins of every sweep and the energy trace bit-equal to the
    oracle's, spins moved, the tracked energy an exact integer account.  fused: on one planned window of S sweeps (asserted).
    declined: the plan is asked for and must come back empty; the call then runs sweep by sweep (asserted), same bits."""
    J, h, beta, csr, (qs, escale) = case(name, n)
    N = csr.n
    f64 = precision == "f64"
    m0 = init_spins(R, N)
    with product.Engine(J, h, R) as eng:
        if real:
            eng.set_fused_f64_real(True)
        eng.set_spins(m0)
        E0 = eng.energy()
        start = units(E0, escale)
        assert np.array_equal(eng.energy_tracked(), np.array(start, dtype=np.int64) * 2.0 ** -escale)
        if fused or declined:
            assert eng.plan_philox_fused(0, 1, S, SEED) == (0 if declined else 1)
            assert precision in eng.fused_modes(S)
        o = eng.sweep_philox(S, SEED, beta=beta, precision=precision, record_stride=1, want_energy=True)
        assert eng._last_fused() is fused
        tracked = eng.energy_tracked()
        final = eng.get_spins()
        end = raw_tracked(eng)
    cb = np.tile(np.array(oracle.cb_pair(beta, 1.0, f64)), (S, 1))
    for c in range(R):
        M, s_fin, tr = oracle.sweeps_philox(csr, h, m0[c], cb, SEED, c, escale=escale, use_f64=f64, efix0=start[c])
        assert np.array_equal(o["spins"][c], M), (name, c)
        assert np.array_equal(o["energy"][c], tr * 2.0 ** -escale), (name, c)
        assert np.array_equal(final[c], s_fin) and tracked[c] == tr[-1] * 2.0 ** -escale
        assert not np.array_equal(s_fin, m0[c])                  # the chain moved
        assert end[c] == int(tr[-1])
    if not f64:
        q0, q1 = efix_of(J, h, m0, qs, escale), efix_of(J, h, final, qs, escale)
        print(f"{name}: start offset (tracked - quantised, units of 2^-{escale}) {[a - b for a, b in zip(start, q0)]}")
        assert [a - b for a, b in zip(end, start)] == [a - b for a, b in zip(q1, q0)]
        # the start is the real model's fp64 energy: within the quantisation bound of the quantised one, plus its own rounding
        A = sp_nnz(J)
        slack = Fraction(A // 2 + N, 2) * (1 << (escale - qs)) + sf.energy_bound(J, h) * (1 << escale) + 1
        assert all(abs(a - b) <= slack for a, b in zip(start, q0))
        if exact_start(J, h, qs):
            assert end == q1
    return o


def sp_nnz(J):
    import scipy.sparse as sp
    A = sp.csr_matrix(J).copy()
    A.eliminate_zeros()
    return int(A.nnz)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("name", sf.NAMES)
def test_sweep_by_sweep_matches_the_oracle(product, name, precision):
    sweeps_vs_oracle(product, name, precision)


FUSED = tuple(nm for nm in sf.NAMES if sf.SIZES.get(nm, 300) >= 256)


def test_the_field_only_member_is_below_the_fused_kernels(product):
    """n = 50 < 256: the plan is declined (0 windows, not an error), no precision may run fused."""
    J, h, _, _, _ = case("honly")
    with product.Engine(J, h, 1) as eng:
        assert eng.plan_philox_fused(0, 1, S, SEED) == 0 and eng.fused_modes(S) == set()
    assert set(FUSED) == set(sf.NAMES) - {"honly"}


def earlier_neighbours(csr, k, sweep):
    """How many neighbours of spin k come before it in the order of sweep `sweep`: spins sorted by (philox(k, t, 0, ORDER)[0], k)."""
    lo, hi = SEED & 0xFFFFFFFF, SEED >> 32
    key = lambda j: (int(oracle.philox(int(j), sweep, 0, 2, lo, hi)[0]), int(j))      # tag 2: NLMC_TAG_ORDER
    mine = key(k)
    return sum(key(j) < mine for j in csr.indices[csr.indptr[k]:csr.indptr[k + 1]] if j != k)


@pytest.mark.parametrize("name", FUSED)
def test_fused_window_f32_matches_the_oracle(product, name):
    """hub: the fused levelizer counts a spin's unfinished earlier neighbours in eight bits and declines a window in which some
    spin has more than 255 of them (include/nlmc.h: nlmc_plan_philox_fused); the centre of the star has about 1500.  That refusal
    is asserted, and the call behind it, which runs sweep by sweep, against the oracle."""
    if name == "hub":
        csr = case(name)[3]
        assert max(earlier_neighbours(csr, 0, t) for t in range(S)) > 255
        assert max(np.diff(csr.indptr)[1:]) == 1                 # (no other spin comes near the limit)
        sweeps_vs_oracle(product, name, "f32", declined=True)
    else:
        sweeps_vs_oracle(product, name, "f32", fused=True)


@pytest.mark.parametrize("name", sf.DYADIC)
def test_fused_window_f64_on_the_dyadic_members(product, name):
    """The integer-threshold fp64 kernel: cb * (X * 2^-qs) with qs = -7 and 13."""
    J, h, _, _, (qs, _) = case(name)
    assert exact_start(J, h, qs)
    sweeps_vs_oracle(product, name, "f64", fused=True)


@pytest.mark.parametrize("name", ["x1e9", "x1e-9"])
def test_fused_window_f64_real_valued(product, name):
    J, h, _, _, (qs, _) = case(name)
    assert not exact_start(J, h, qs)
    with product.Engine(J, h, 1) as eng:
        assert "f64" not in eng.fused_modes(S)                   # real-valued: opt-in only
    sweeps_vs_oracle(product, name, "f64", fused=True, real=True)


@pytest.mark.parametrize("n,fused", [(300, False), (2000, False), (2200, True)])
def test_f64_anneal_on_the_dyadic_member_follows_the_rule(product, n, fused):
    """pmJ_2m10_h with a temperature per sweep.  The rule (include/nlmc.h: nlmc_fused_modes): such a call runs on fused windows when
    8 (2 xmax + 1) <= n, xmax = max row sum of |Jq| + |hq|.  n = 300: xmax = 116, 1864 > 300, sweep by sweep.  n = 2000: the graph
    of that size has a row of 16 couplings, xmax = 131, 2104 > 2000: sweep by sweep as well.  n = 2200: xmax = 116 again, fused.
    Either way the bits are the oracle's."""
    J, h, beta, csr, (qs, escale) = case("pmJ_2m10_h", n)
    rows, hq = sf.quantise(J, h, qs)
    xmax = max(sum(abs(q) for _, q in r) + abs(x) for r, x in zip(rows, hq))
    assert xmax == {300: 116, 2000: 131, 2200: 116}[n] and (8 * (2 * xmax + 1) <= n) is fused
    S2 = 2 * T
    table = np.stack([np.geomspace(0.2 * (1 + 0.1 * c), 3.0 / (1 + 0.07 * c), S2) for c in range(R)]) * beta
    m0 = init_spins(R, n)
    with product.Engine(J, h, R) as eng:
        assert "f64" in eng.fused_modes(T)
        eng.set_spins(m0)
        start = units(eng.energy(), escale)
        o = eng.sweep_philox_windows(S2, SEED, beta=table, window=T, precision="f64", record_stride=1, want_energy=True)
        assert eng.fused_last_call is fused
        tracked, final = eng.energy_tracked(), eng.get_spins()
        end = raw_tracked(eng)
    for c in range(R):
        cb = np.array([oracle.cb_pair(b, 1.0, True) for b in table[c]])
        M, s_fin, tr = oracle.sweeps_philox(csr, h, m0[c], cb, SEED, c, escale=escale, use_f64=True, efix0=start[c])
        assert np.array_equal(o["spins"][c], M) and np.array_equal(o["energy"][c], tr * 2.0 ** -escale), c
        assert np.array_equal(final[c], s_fin) and tracked[c] == tr[-1] * 2.0 ** -escale
        assert not np.array_equal(s_fin, m0[c])
    assert end == efix_of(J, h, final, qs, escale)      # dyadic: the fp64 account is the quantised one


# ---- d. energy kernels ---------------------------------------------------------------------------------------------------------------

def within(E, J, h, spins, bound):
    for e, s in zip(np.asarray(E).reshape(-1), spins):
        assert abs(Fraction(float(e)) - sf.exact_energy(J, h, s)) <= bound


@pytest.mark.parametrize("name", sf.NAMES)
def test_energy_kernels_within_the_summation_bound(product, name):
    """energy(), energy_of (also of configurations with zeros) and energy_of_recorded against the exact energy, within
    (nnz + n) 2^-53 (sum|J|/2 + sum|h|)."""
    J, h, beta, csr, _ = case(name)
    N = csr.n
    bound = sf.energy_bound(J, h)
    m0 = init_spins(R, N)
    third = m0[0].copy()
    third[::3] = 0
    batch = np.stack([m0[1], third, np.zeros(N, dtype=np.int8), np.ones(N, dtype=np.int8)])
    with product.Engine(J, h, R) as eng:
        eng.set_spins(m0)
        within(eng.energy(), J, h, m0, bound)
        Eb = eng.energy_of(batch)
        within(Eb, J, h, batch, bound)
        assert Eb[2] == 0.0
        o = eng.sweep_philox(3, SEED, beta=beta, record_stride=1)
        Er = eng.energy_of_recorded(2, first=1)
        assert Er.shape == (R, 2)
        within(Er, J, h, o["spins"][:, 1:3].reshape(-1, N), bound)
        assert not np.array_equal(o["spins"][:, 2], m0)
        within(eng.energy(), J, h, o["spins"][:, 2], bound)


def test_energy_of_a_cancelling_configuration(product):
    """x1e9, a configuration whose energy is below 1e-6 of the sum of its terms' sizes: the error stays within the bound relative to
    that sum (0.07 here against terms of 3e11), not relative to |E|."""
    J, h, _, csr, _ = case("x1e9")
    s = sf.cancelling_state(J, h)
    assert abs(sf.exact_energy(J, h, s)) < sf.abs_terms(J, h) / 10 ** 6
    bound = sf.energy_bound(J, h)
    with product.Engine(J, h, 1) as eng:
        within(eng.energy_of(s[None]), J, h, [s], bound)
        eng.set_spins(s[None])
        within(eng.energy(), J, h, [s], bound)
        within(eng.energy_tracked(), J, h, [s], bound + Fraction(1, 2 << eng.energy_scale))


# ---- e. swap rounds with saturated and degenerate acceptance -------------------------------------------------------------------------

def swap_ladder(J, h, csr):
    """Eight configurations (slots 3 and 4 hold the same one) and a ladder whose adjacent pairs start at
    dBeta dE log2(e) = +2000, -2000, 1, 0 (the twins), -1.5, +3000, -3000."""
    m = init_spins(8, csr.n).copy()
    m[4] = m[3]
    E = [sf.exact_energy(J, h, s) for s in m]
    want = [2000.0, -2000.0, 1.0, None, -1.5, 3000.0, -3000.0]
    betas = [0.0]
    for i, z in enumerate(want):
        dE = float(E[i + 1] - E[i])
        betas.append(betas[-1] + (0.5 / max(abs(float(e)) for e in E) if z is None else z / (dE * LOG2E)))
    return m, np.array(betas)


@pytest.mark.parametrize("name", ["x3e15", "x1e-9"])
def test_swap_rounds_saturated_and_degenerate(product, name):
    J, h, _, csr, (_, escale) = case(name)
    m, betas = swap_ladder(J, h, csr)
    L, n_pairs = 8, 3
    seen, sat = set(), set()
    with product.Engine(J, h, L) as eng:
        eng.set_spins(m)
        eng.pt_init(betas)
        slots = eng.pt_slots()
        for rnd in range(6):
            E = eng.energy()
            Et = eng.energy_tracked()
            assert np.all(np.abs(Et - E) <= 2.0 ** -(escale + 1))            # what the kernel reads: the same energies, rounded
            exp_slots, exp_pairs, exp_acc = swap_round(E, slots, betas, L, n_pairs, rnd, SEED)
            assert np.array_equal(exp_acc, swap_round(Et, slots, betas, L, n_pairs, rnd, SEED)[2])
            chain_of = np.argsort(slots)
            for (i, _), a in zip(exp_pairs[0], exp_acc[0]):
                z = ((betas[i + 1] - betas[i]) * (E[chain_of[i + 1]] - E[chain_of[i]])) * LOG2E
                kind = "below" if z < -1100 else "above" if z > 1100 else "zero" if z == 0.0 else "one" if 0.1 < abs(z) < 30 else "other"
                seen.add(kind)
                if kind in ("below", "above"):
                    sat.add((kind, int(a)))
                    assert int(a) == (kind == "above")
                if kind == "zero":
                    assert int(a) == 1
            pairs, acc = eng.pt_swap_philox(rnd, SEED, n_pairs)
            slots = eng.pt_slots()
            assert np.array_equal(pairs, exp_pairs) and np.array_equal(acc, exp_acc) and np.array_equal(slots, exp_slots), rnd
    assert {"below", "above", "zero", "one"} <= seen, seen
    assert sat == {("below", 0), ("above", 1)}
    assert not np.array_equal(slots, np.arange(L))


# ---- f. the iso-cluster move's energy resynchronisation ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["x2p40", "x1e-9"])
def test_icm_round_keeps_the_integer_account(product, name):
    """icm_round_ladders (K = 4 sub-replicas, 2 slots) after a few sweeps: the moves' energy changes enter the tracked energies as
    sh_dE << eshift (eshift = 29 and 0 here).  Integer identity from the start of the run to its end; energy() within the bound."""
    J, h, beta, csr, (qs, escale) = case(name)
    N, K, L = csr.n, 4, 2
    G = K * L
    m0 = init_spins(G, N)
    with product.Engine(J, h, G) as eng:
        eng.set_spins(m0)
        betas = np.array([0.7, 1.0]) * beta
        eng.pt_init(betas)
        start = raw_tracked(eng, betas)
        assert start == units(eng.energy(), escale)
        eng.sweep_philox(3, SEED, beta=None)
        mid_s, mid = eng.get_spins(), raw_tracked(eng, betas)
        info = eng.icm_round_ladders(0, SEED, True, want_info=True)
        end_s, end = eng.get_spins(), raw_tracked(eng, betas)
        assert np.array_equal(eng.energy_tracked(), np.array(end, dtype=np.int64) * 2.0 ** -escale)
        E = eng.energy()
    assert info.shape == (L * (K // 2), 2) and np.all(info[:, 0] > 0) and np.all(info[:, 1] > 0)
    moved = [not np.array_equal(end_s[c], mid_s[c]) for c in range(G)]           # (a cluster above n/2 flips one chain of the pair)
    assert sum(moved) >= len(info) and end != mid
    q0, q1, q2 = (efix_of(J, h, s, qs, escale) for s in (m0, mid_s, end_s))
    assert [a - b for a, b in zip(mid, start)] == [a - b for a, b in zip(q1, q0)]
    assert [a - b for a, b in zip(end, mid)] == [a - b for a, b in zip(q2, q1)]
    within(E, J, h, end_s, sf.energy_bound(J, h))


# ---- g. rounds against the oracle ----------------------------------------------------------------------------------------------------

def host_rounds(J, h, csr, m0, start, betas, L, rounds, Tr, n_pairs, f64, escale):
    """The rounds on the host: every chain's sweeps by the sequential oracle at its slot's beta, then oracle.pt.swap_round on the
    tracked energies.  -> spins, slot map, log pairs [rounds, ladders, n_pairs, 2], log decisions."""
    G = len(m0)
    s, efix = [x.copy() for x in m0], list(start)
    slots = np.arange(G, dtype=np.int32) % L
    lp, la = [], []
    for r in range(rounds):
        for c in range(G):
            cb = np.tile(np.array(oracle.cb_pair(betas[slots[c]], 1.0, f64)), (Tr, 1))
            _, s[c], tr = oracle.sweeps_philox(csr, h, s[c], cb, SEED, c, sweep0=r * Tr, escale=escale, use_f64=f64,
                                               efix0=efix[c], want_M=False)
            efix[c] = int(tr[-1])
        E = np.array([float(Fraction(e, 1 << escale)) for e in efix])
        slots, p, a = swap_round(E, slots, betas, L, n_pairs, r, SEED)
        lp.append(p)
        la.append(a)
    return np.stack(s), slots, np.stack(lp), np.stack(la), efix


@pytest.mark.parametrize("name,precision", [("x1e9", "f32"), ("pmJ_2p7", "f64")])
def test_rounds_in_launch_match_the_host_chain(product, name, precision):
    """pt_rounds_deferred, 4 rounds of 3 sweeps, two ladders of 4, N = 320: the other rounds tests compare device routes with each
    other; this one compares the in-launch route with the oracle (qs = -7 on both members)."""
    J, h, beta, csr, (qs, escale) = case(name, 320)
    L, nl, rounds, Tr, n_pairs = 4, 2, 4, 3, 1
    G = L * nl
    betas = np.linspace(0.9, 1.1, L) * beta
    m0 = init_spins(G, 320)
    with product.Engine(J, h, G) as eng:
        eng.set_spins(m0)
        start = units(eng.energy(), escale)
        eng.pt_init(betas)
        assert eng.plan_philox_fused(0, rounds, Tr, SEED) == rounds
        eng.pt_plan(0, rounds, SEED, n_pairs)
        eng.pt_log_begin(0, rounds, n_pairs)
        assert eng.pt_rounds_deferred(rounds, Tr, SEED, 0, 0, n_pairs, precision=precision), getattr(eng, "rounds_fused_refusal", "")
        assert eng.last_rounds_route() == "in launch"
        lp, la = eng.pt_log_read()
        spins, slots, tracked_f = eng.get_spins(), eng.pt_slots(), eng.energy_tracked()
        tracked = raw_tracked(eng, betas)
    e_spins, e_slots, e_lp, e_la, e_efix = host_rounds(J, h, csr, m0, start, betas, L, rounds, Tr, n_pairs, precision == "f64", escale)
    assert np.array_equal(lp, e_lp) and np.array_equal(la, e_la)
    assert np.array_equal(slots, e_slots) and np.array_equal(spins, e_spins)
    assert tracked == e_efix and np.array_equal(tracked_f, np.array(e_efix, dtype=np.int64) * 2.0 ** -escale)
    assert la.sum() > 0 and not np.array_equal(slots, np.arange(G) % L)          # swaps happened
    assert all(not np.array_equal(spins[c], m0[c]) for c in range(G))
