"""The LAW of the "f32" throughput mode, checked on the CPU against closed forms (no GPU, no reference import).

The product's device-RNG mode is not stream-matched with the reference, so its parity with NMC/nmc.py:86-87 rests on
two facts that are checked here on the oracle's restatement of the spec (the -m gpu tests then require the HIP kernels
to equal that restatement bit for bit):
  1. the acceptance test  z < W(r),  r uniform on 2^32 values, has P(s' = +1) = 1 / (1 + 2^z) = (1 + tanh(beta x)) / 2,
     the reference's heat-bath probability, to ~2e-7 relative, down to probabilities of 2^-33, and is exactly symmetric
     under a global spin flip (the round-1 spec broke that symmetry at cold rungs);
  2. couplings are held in fixed point with a stated, bounded error (exact for +-J instances).
The fp64 mode's law (exp2_spec_f64, the 53-bit uniform and the fma(u, 2^z, u) < 1 test; on fused windows the integer
thresholds count the same uniforms) is checked against 200-bit arithmetic and a closed form.  The calibration checker of
tests/lawcheck.py, which tests/test_gpu_law.py runs on every sweep route's traces, is validated here on the oracle's own
traces: the true law passes, every wrong hypothesis rejects.
"""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import lawcheck
import oracle
from helpers import make_instance, init_spins


def test_threshold_is_antisymmetric():
    r = np.random.default_rng(1).integers(0, 2 ** 32, size=20000, dtype=np.uint64)
    edge = np.array([0, 1, 2, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1], dtype=np.uint64)
    for v in np.concatenate([r, edge]):
        a, b = oracle.threshold(int(v)), oracle.threshold(int(v) ^ 0xFFFFFFFF)
        assert a == -b or (a == 0.0 and b == 0.0)


def test_threshold_matches_the_logit_pointwise():
    rng = np.random.default_rng(2)
    # uniform r, and r concentrated in both tails (small u and small 1 - u)
    rs = np.concatenate([rng.integers(0, 2 ** 32, size=20000, dtype=np.uint64),
                         rng.integers(0, 2 ** 12, size=2000, dtype=np.uint64),
                         2 ** 32 - 1 - rng.integers(0, 2 ** 12, size=2000, dtype=np.uint64)])
    worst = 0.0
    for r in rs:
        u = (float(r) + 0.5) / 2.0 ** 32
        exact = math.log2((1.0 - u) / u)
        worst = max(worst, abs(oracle.threshold(int(r)) - exact) / max(1.0, abs(exact)))
    assert worst < 1.5e-6            # degree-7 fit: 2 x 3.8e-7 + f32 rounding


@pytest.mark.parametrize("z", [-20.0, -2.0, -0.5, 0.0, 0.5, 6.0, 12.0])
def test_acceptance_probability_is_the_heat_bath_law(z):
    """P(z < W(r)) over a 1/256 sample of ALL 2^32 values of r vs 1/(1+2^z) = (1+tanh(beta x))/2 at z = -2 log2(e) beta x
    (NMC/nmc.py:87).  The full enumeration (scripts/law_exhaustive.py) gives <= 2e-7 relative at every z listed."""
    p = oracle.threshold_cdf(z, 256)
    exact = 1.0 / (1.0 + 2.0 ** z)
    # sampling 2^24 points of a deterministic lattice: error <= lattice spacing + fit error
    assert abs(p - exact) <= 3e-7 * max(exact, 1e-3) + 2.0 ** -23


def test_rare_moves_keep_their_probability():
    """beta = 4, |x| = 2 on a +-J instance: true flip probability 1.1e-7.  The round-1 24-bit uniform gave 1.19e-7 one
    way and 5.96e-8 the other; here both directions see the same probability, resolved to 2^-32.  W is decreasing in
    r, so only the first (last) few hundred r can pass the test: they are enumerated one by one."""
    z = 2.0 * oracle.LOG2E * 4.0 * 2.0           # s' = +1 against the field
    edge = 1 << 16
    assert oracle.threshold_count(z, edge, 1 << 32, 4099) == 0             # nothing beyond the tail passes
    n_up = oracle.threshold_count(z, 0, edge)                               # z < W(r)
    n_dn = edge - oracle.threshold_count(-z, (1 << 32) - edge, 1 << 32)    # s' = -1 against the flipped field
    assert oracle.threshold_count(-z, 0, (1 << 32) - edge, 4099) == -(-((1 << 32) - edge) // 4099)
    exact = 2.0 ** 32 / (1.0 + 2.0 ** z)
    assert abs(n_up - exact) <= 2 and abs(n_up - n_dn) <= 1


def test_field_scale_and_quantisation_bound():
    J, h = make_instance(300, seed=5, gaussian=True, with_h=True)
    csr = oracle.Csr(J)
    qs, esc = oracle.field_scale(csr, h)
    q = np.rint(np.ldexp(csr.data, qs))
    assert np.max(np.abs(q)) <= 2 ** 23 - 1 and np.max(np.abs(q)) >= 2 ** 21      # 24-bit multiplier, well used
    assert np.max(np.abs(np.ldexp(q, -qs) - csr.data)) <= 2.0 ** -(qs + 1)
    assert qs <= esc <= qs + 29
    # +-J: exact
    J2, h2 = make_instance(300, seed=6)
    csr2 = oracle.Csr(J2)
    qs2, _ = oracle.field_scale(csr2, h2)
    assert np.array_equal(np.ldexp(np.rint(np.ldexp(csr2.data, qs2)), -qs2), csr2.data)


def test_fixed_point_energy_tracking_is_exact():
    """E_fix after S sweeps == E_fix(start) + exact energy difference of the quantised model, in integers."""
    J, h = make_instance(200, seed=7, gaussian=True, with_h=True)
    csr = oracle.Csr(J)
    qs, esc = oracle.field_scale(csr, h)
    Jq = np.rint(np.ldexp(csr.data, qs)).astype(np.int64)
    hq = np.rint(np.ldexp(h, qs)).astype(np.int64)
    import scipy.sparse as sp
    A = sp.csr_matrix((Jq, csr.indices, csr.indptr), shape=(csr.n, csr.n))

    def e_int(s):
        s = s.astype(np.int64)
        return -(int(s @ (A @ s)) // 2 + int(hq @ s))      # J symmetric, zero diagonal: s^T A s is even

    s0 = np.where(np.random.default_rng(3).random(csr.n) < 0.5, -1, 1).astype(np.int8)
    cb = np.tile(np.array(oracle.cb_pair(0.7)), (12, 1))
    M, s_fin, tr = oracle.sweeps_philox(csr, h, s0, cb, 99, 0, escale=esc, efix0=0)
    for t in (0, 5, 11):
        assert int(tr[t]) == (e_int(M[t]) - e_int(s0)) << (esc - qs)


# ---- the fp64 mode: exp2_spec_f64 and the acceptance count of the 53-bit uniform ------------------------------------------------
def _z_grid():
    rng = np.random.default_rng(64)
    z = np.concatenate([rng.uniform(-1000.0, 1000.0, 2000), rng.uniform(-60.0, 60.0, 2000), rng.uniform(-2.0, 2.0, 2000)])
    edge = [0.0, -0.0, 52.0, -52.0, 53.0, -53.0, 1000.0, -1000.0, 1000.5, -1000.5, 1e4, -1e4, 0.5, -0.5]
    return np.concatenate([z, edge])


def test_fp64_exp2_against_200_bit_arithmetic():
    """exp2_spec_f64 (degree-13 Horner in fma) against mpmath at 200 bits over [-1000, 1000] and at the clamps: relative error
    <= 2^-52 (the Horner rounding bounds it; a sample measured 1.07 ulp of 2^-53)."""
    import mpmath
    mpmath.mp.prec = 200
    worst = 0.0
    for z in _z_grid():
        zc = min(1000.0, max(-1000.0, float(z)))
        exact = mpmath.power(2, mpmath.mpf(zc))
        got = mpmath.mpf(oracle.exp2_f64(float(z)))
        worst = max(worst, float(abs(got - exact) / exact))
    assert worst <= 2.0 ** -52, worst


def test_fp64_acceptance_count_is_the_heat_bath_law():
    """K(z) = #{m < 2^53 : fma(m 2^-53, E, m 2^-53) < 1}, E = exp2_spec_f64(z), found by bisection on the test itself, equals the
    closed form ceil((2^53 - 1/2) / (1 + E)) (the fma result rounds below 1 iff u (1 + E) < 1 - 2^-54; the tie rounds to 1.0);
    K 2^-53 is 1 / (1 + 2^z) = (1 + tanh(beta x)) / 2 (NMC/nmc.py:87) to 2^-53 (ceiling) + 2^-54 (the <= 2^-52 relative error of E
    moves 1 / (1 + E) by at most 2^-52 E / (1 + E)^2 <= 2^-54); and K(z) + K(-z) - 2^53 is 0 or 1 (spin-flip symmetry up to one
    uniform)."""
    from fractions import Fraction
    import mpmath
    mpmath.mp.prec = 200
    two53 = 1 << 53
    worst = 0.0
    for z in _z_grid():
        K = oracle.accept_count_f64(float(z))
        E = Fraction(oracle.exp2_f64(float(z)))
        X = (Fraction(two53) - Fraction(1, 2)) / (1 + E)
        closed = -((-X.numerator) // X.denominator)             # ceil
        assert K == closed, (z, K, closed)
        zc = min(1000.0, max(-1000.0, float(z)))
        p = 1 / (1 + mpmath.power(2, mpmath.mpf(zc)))
        err = float(abs(mpmath.mpf(K) / two53 - p))
        worst = max(worst, err)
        assert err <= 2.0 ** -53 + 2.0 ** -54, (z, err)
        assert K + oracle.accept_count_f64(-float(z)) - two53 in (0, 1), z
    assert worst > 0.0


# ---- the law checker (tests/lawcheck.py) on the oracle's own traces ---------------------------------------------------------------
LAW_SEED = 0x1A3C0DE5 + (3 << 32)


def test_lawcheck_philox_and_orders_restate_the_oracle():
    rng = np.random.default_rng(8)
    for _ in range(50):
        c = [int(v) for v in rng.integers(0, 2 ** 32, 6, dtype=np.uint64)]
        assert [int(w) for w in lawcheck.philox(*c)] == [int(w) for w in oracle.philox(*c)]
    # a sweep's order: spins sorted by (philox(k, t, group, ORDER)[0], k), shared (group 0) or per chain
    n, t, g = 300, 11, 5
    pos = lawcheck.order_positions(n, t, LAW_SEED, np.array([0, g]))
    for row, grp in zip(pos, (0, g)):
        keys = [(int(oracle.philox(k, t, grp, 2, LAW_SEED & 0xFFFFFFFF, LAW_SEED >> 32)[0]), k) for k in range(n)]
        assert np.array_equal(np.argsort(row), [k for _, k in sorted(keys)])
    assert np.array_equal(lawcheck.order_positions(n, t, LAW_SEED), pos[0])


def hub_diag_instance(N, seed):
    """Gaussian couplings and fields, hub rows of 9-40 entries, a real diagonal."""
    rng = np.random.default_rng(seed)
    Jb, h = make_instance(N, seed=seed, with_h=True, gaussian=True)
    A = sp.lil_matrix(sp.csr_matrix(Jb))
    for hub, deg in enumerate((9, 12, 16, 17, 40)):
        for j in rng.choice(np.arange(64, N), size=deg, replace=False):
            A[hub, j] = A[j, hub] = float(rng.standard_normal() * 0.7)
    A = (sp.csr_matrix(A) + sp.diags(rng.standard_normal(N) * 0.4)).tocsr()
    A.sort_indices()
    return A, h


def oracle_trace(J, h, s0, beta, use_f64, flags=None, temp_x=1.0, per_chain=False):
    """[R, S, N] trace of the sequential spec (oracle/nlo.c) at beta [R, S]."""
    csr = oracle.Csr(J)
    R, S = beta.shape
    M = np.empty((R, S, csr.n), np.int8)
    for c in range(R):
        cb = np.array([oracle.cb_pair(b, temp_x, use_f64) for b in beta[c]])
        M[c] = oracle.sweeps_philox(csr, h, s0[c], cb, LAW_SEED, c, order_group=(c + 1 if per_chain else 0),
                                    flags=None if flags is None else flags[c], use_f64=use_f64)[0]
    return M


def assert_law(inst, s0, M, beta, pos, wrong, flags=None, temp_x=1.0, quant=None):
    """The true law passes with delta* <= 1e-2; beta (1 + delta*), the Jacobi reading and every hypothesis in `wrong` reject."""
    hyp = {"true": {}, "jacobi": {"reading": "jacobi"}}
    hyp.update(wrong)
    res = lawcheck.check(inst, s0, M, beta, pos, flags=flags, temp_x=temp_x, hypotheses=hyp, quant=quant)
    ds = res["true"]["delta_star"]
    print(lawcheck.summary(res))
    tr = res["true"]
    assert tr["ok"], tr
    assert ds <= 1e-2
    if quant is not None:
        assert tr["quant_ok"]
    for name, r in res.items():
        if name != "true":
            assert not r["ok"], name
    return res


def test_checker_pmj_fp64_anneal_per_sweep_temperatures():
    """+-J, fp64, a temperature per sweep that differs between chains (coarse steps): the true law passes; beta (1 + delta*),
    the Jacobi reading, the order read backwards and every update at the previous sweep's beta reject."""
    N, R, S = 3000, 32, 76
    J, h = make_instance(N, seed=71)
    s0 = init_spins(R, N)
    beta = np.stack([np.concatenate([np.geomspace(0.25 * (1 + 0.02 * c), 1.3, S // 2)] * 2) for c in range(R)])
    M = oracle_trace(J, h, s0, beta, True)
    prev = np.concatenate([beta[:, :1], beta[:, :-1]], axis=1)
    assert_law(lawcheck.Instance(J, h), s0, M, beta, lambda t: lawcheck.order_positions(N, t, LAW_SEED),
               {"reversed": {"reading": "reversed"}, "previous_sweep_beta": {"beta": prev}})


def test_checker_gaussian_fields_diagonal_f32_quantised():
    """Gaussian couplings, fields, hub rows and a diagonal in the "f32" mode (24-bit fixed-point couplings): every bin's summed
    quantisation shift stays under its standard deviation, the true law passes with the true J, the wrong ones (the order read
    backwards, the beta of the neighbouring ladder slot: x1.033) reject."""
    N, R, S = 3000, 48, 50
    J, h = hub_diag_instance(N, 72)
    s0 = init_spins(R, N)
    beta = np.repeat(np.geomspace(0.35, 1.6, R)[:, None], S, axis=1)
    M = oracle_trace(J, h, s0, beta, False)
    inst = lawcheck.Instance(J, h)
    qs = oracle.field_scale(oracle.Csr(J), h)[0]
    slot = np.arange(R)                                     # the ladder: chain r on slot r; the neighbouring slot's beta is wrong
    neighbour = beta[np.where(slot < R - 1, slot + 1, R - 2)]
    assert_law(inst, s0, M, beta, lambda t: lawcheck.order_positions(N, t, LAW_SEED),
               {"reversed": {"reading": "reversed"}, "neighbour_slot_beta": {"beta": neighbour}},
               quant=lawcheck.quantisation_bound(inst, qs))


def test_checker_phase_flags_fp64_gaussian():
    """NMC phase flags: frozen rows (2, 3) never change and are no samples, scaled rows (1) run at beta / temp_x: the true law
    passes; scaled rows at full beta reject, as do beta (1 + delta*) and the Jacobi reading."""
    N, R, S, tx = 3000, 40, 100, 2.0
    J, h = hub_diag_instance(N, 73)
    s0 = init_spins(R, N)
    flags = np.random.default_rng(74).choice([0, 0, 0, 0, 1, 1, 2, 3], size=(R, N)).astype(np.uint8)
    beta = np.repeat(np.geomspace(0.4, 2.0, R)[:, None], S, axis=1)
    M = oracle_trace(J, h, s0, beta, True, flags=flags, temp_x=tx)
    assert np.array_equal(M[:, -1][flags >= 2], s0[flags >= 2])
    assert_law(lawcheck.Instance(J, h), s0, M, beta, lambda t: lawcheck.order_positions(N, t, LAW_SEED),
               {"scaled_rows_at_full_beta": {"scaled_rows_at_full_beta": True}}, flags=flags, temp_x=tx)
    # a frozen row that moved is caught on its own
    M2 = M.copy()
    k = int(np.nonzero(flags[0] >= 2)[0][0])
    M2[0, 3:, k] = -s0[0, k]
    r = lawcheck.check(lawcheck.Instance(J, h), s0, M2, beta, lambda t: lawcheck.order_positions(N, t, LAW_SEED), flags=flags,
                       temp_x=tx, power=False)["true"]
    assert r["frozen_changed"] == 1 and not r["ok"]


def test_checker_per_chain_orders_f32_pmj():
    """order="per_chain" (order group chain + 1): the true law passes with the per-chain orders; the SHARED order's reading rejects."""
    N, R, S = 2000, 48, 72
    J, h = make_instance(N, seed=75)
    h = np.random.default_rng(75).integers(-1, 2, N).astype(np.float64)
    s0 = init_spins(R, N)
    beta = np.repeat(np.geomspace(0.3, 1.3, R)[:, None], S, axis=1)
    M = oracle_trace(J, h, s0, beta, False, per_chain=True)
    groups = np.arange(R) + 1
    inst = lawcheck.Instance(J, h)
    assert_law(inst, s0, M, beta, lambda t: lawcheck.order_positions(N, t, LAW_SEED, groups), {},
               quant=lawcheck.quantisation_bound(inst, oracle.field_scale(oracle.Csr(J), h)[0]))
    shared = lawcheck.check(inst, s0, M, beta, lambda t: lawcheck.order_positions(N, t, LAW_SEED), power=False)["true"]
    assert not shared["ok"], shared["max_z"]


def test_swap_calibration_on_the_oracle_swap_rounds():
    """Replica-exchange decisions of the sequential spec (oracle.pt.swap_round: 10 pairs per round on a 32-slot ladder, two
    fp64 sweeps between rounds) against min(1, exp(dBeta dE)) with the energies recomputed exactly (integers on +-J): the
    calibration passes; with the sign of dBeta dE flipped it rejects."""
    from oracle import pt
    N, R, PAIRS, ROUNDS, T = 200, 32, 10, 70, 2
    J, h = make_instance(N, seed=77)
    csr = oracle.Csr(J)
    ladder = np.geomspace(0.1, 1.5, R)
    s = init_spins(R, N)
    slots = np.arange(R, dtype=np.int32)
    dbde, acc_all = [], []
    for rnd in range(ROUNDS):
        for c in range(R):
            cb = np.tile(np.array(oracle.cb_pair(ladder[slots[c]], 1.0, True)), (T, 1))
            s[c] = oracle.sweeps_philox(csr, h, s[c], cb, LAW_SEED, c, sweep0=rnd * T, use_f64=True, want_M=False)[1]
        E = np.array([oracle.energy(csr, h, s[c]) for c in range(R)])
        assert np.array_equal(E, np.rint(E))
        chain_of = np.empty(R, np.int64)
        chain_of[slots] = np.arange(R)
        slots, pairs, acc = pt.swap_round(E, slots, ladder, R, PAIRS, rnd, LAW_SEED)
        i = pairs[0, :, 0]
        dbde.append((ladder[i + 1] - ladder[i]) * (E[chain_of[i + 1]] - E[chain_of[i]]))
        acc_all.append(acc[0].astype(bool))
    dbde, acc_all = np.concatenate(dbde), np.concatenate(acc_all)
    r = lawcheck.check_swaps(dbde, acc_all)
    assert r["ok"] and r["z_pool"] is not None and np.count_nonzero(dbde < 0) > 200, r
    assert not lawcheck.check_swaps(-dbde, acc_all)["ok"]


def test_swap_calibration_rejects_a_flipped_sign():
    """The swap calibration on decisions drawn from the exact law passes; with the sign of dBeta dE flipped it rejects."""
    rng = np.random.default_rng(76)
    a = rng.normal(-0.5, 1.5, 4000)
    acc = rng.random(a.size) < np.minimum(1.0, np.exp(a))
    r = lawcheck.check_swaps(a, acc)
    assert r["ok"] and r["z_pool"] is not None, r
    assert not lawcheck.check_swaps(-a, acc)["ok"]
