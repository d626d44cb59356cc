"""The dense members of tests/scalefamily.py (complete graphs whose rows sit within 1 % of the int32 row-sum limit) and the case set
of tests/test_gpu_magnitude_short.py (tests/magshort.py), without a GPU: the oracle's scales against the numpy and Fraction
restatements and the pinned pairs, the numpy energy against the Fraction one, the aligned state, and the coverage conditions of the
case set computed from the oracle's scales alone -- so that the GPU file compares the short-chain routes with an oracle that is
itself pinned at these magnitudes, on cases that are known to reach them."""
import numpy as np
import pytest

import magshort as mc
import oracle
import scalefamily as sf
from helpers import init_spins

LIMIT = 1 << 31
SEED = 0x5CA1E


@pytest.mark.parametrize("name", sf.DENSE)
def test_dense_scales_are_the_restated_rule_and_the_pinned_pair(name):
    J, h, _, csr, got = mc.instance(name)
    assert got == sf.dense_scale_rule(J, h) == sf.DENSE_PINNED[name]
    if csr.n <= 513:
        assert got == sf.scale_rule(J, h)


@pytest.mark.parametrize("n,with_h", [(40, False), (40, True), (41, True)])
def test_numpy_scale_rule_is_the_fraction_one_on_small_cuts(n, with_h):
    """... and on members of the sparse family, whose branches (a negative qs, everything quantised to 0, a common power of two,
    fields only) the flat construction does not take."""
    J, h = sf.flat(n, with_h)
    assert sf.dense_scale_rule(J, h) == sf.scale_rule(J, h) == oracle.field_scale(oracle.Csr(J), h)
    for name in ("x3e15", "x1e-20", "pmJ_2m10_h", "bigh", "honly"):
        Js, hs, _ = sf.member(name, None if name == "honly" else 40)
        assert sf.dense_scale_rule(Js, hs) == sf.scale_rule(Js, hs), name


@pytest.mark.parametrize("which", ["flat256h", "cut40", "x1e9"])
def test_numpy_energy_is_the_fraction_one(which):
    if which == "flat256h":
        J, h, _, csr, (qs, escale) = mc.instance(which)
    else:
        J, h = sf.flat(40, True) if which == "cut40" else sf.member("x1e9", 40)[:2]
        csr = oracle.Csr(J)
        qs, escale = oracle.field_scale(csr, h)
    states = list(init_spins(2, csr.n)) + [sf.aligned_state(J, h), np.ones(csr.n, dtype=np.int8)]
    third = states[0].copy()
    third[::3] = 0
    for s in states + [third]:
        assert sf.dense_exact_efix_f32(J, h, s, qs, escale) == sf.exact_efix_f32(J, h, s, qs, escale)
    rows, hq = sf.quantise(J, h, qs)
    Jq, hq2 = sf.dense_quantise(J, h, qs)
    assert all(int(Jq[k, c]) == q for k, row in enumerate(rows) for c, q in row) and [int(x) for x in hq2] == hq
    assert int(np.count_nonzero(Jq)) == sum(1 for row in rows for _, q in row if q)


@pytest.mark.parametrize("name", sf.DENSE)
def test_dense_rows_are_at_the_int32_limit(name):
    """Every invariant of the header, the largest row sum in [0.99, 1) 2^31, and the aligned state's X_0 the whole sum of row 0 (in
    Python ints)."""
    J, h, _, csr, (qs, escale) = mc.instance(name)
    Jq, hq = sf.dense_quantise(J, h, qs)
    sums = sf.dense_row_sums(J, h, qs)
    assert int(np.max(np.abs(Jq))) <= (1 << 23) - 1 and qs <= escale <= qs + 29
    assert 0.99 * LIMIT <= int(sums.max()) <= LIMIT - 1
    assert int(np.max(np.abs(Jq))) >= (1 << 21)                # the couplings the 24-bit multiply sees: its top bits are in use
    s = sf.aligned_state(J, h)
    x0 = int(hq[0]) + sum(int(q) * int(x) for q, x in zip(Jq[0], s))
    assert x0 == int(sums[0]) >= 0.99 * LIMIT and int(Jq[0, 0]) == 0
    print(f"{name}: qs {qs}, escale {escale}, largest row sum {int(sums.max())} = {int(sums.max()) / LIMIT:.4f} 2^31, "
          f"X_0 of the aligned state {x0} = {x0 / LIMIT:.4f} 2^31, max |Jq| {int(np.max(np.abs(Jq)))}")


def test_aligned_state_under_a_negative_field():
    J, h = sf.flat(40, True)
    qs, _ = oracle.field_scale(oracle.Csr(J), h)
    Jq, hq = sf.dense_quantise(J, h, qs)
    assert h[1] < 0
    s = sf.aligned_state(J, h, 1)
    assert int(hq[1] + Jq[1] @ s.astype(np.int64)) == -int(sf.dense_row_sums(J, h, qs)[1]) and s[1] == -1


def test_the_staged_cut_stays_near_the_limit():
    """flat192h, the largest matrix the wave kernels stage in LDS: its rows reach 0.7 2^31 at least."""
    J, h, _, csr, (qs, escale) = mc.instance(mc.FLAT192H)
    assert csr.n == 192 and (qs, escale) == sf.dense_scale_rule(J, h) == sf.scale_rule(J, h)
    x = mc.start_fields(mc.FLAT192H, None, mc.ROWS)
    assert 0.7 * LIMIT <= abs(int(x[mc.ALIGNED, 0])) == int(sf.dense_row_sums(J, h, qs)[0]) < LIMIT


@pytest.mark.parametrize("name", sf.DENSE)
def test_f32_oracle_trace_is_the_exact_quantised_energy_on_dense_members(name):
    """Three sweeps from the aligned state, efix0 = its exact quantised energy: the trace ends on the exact quantised energy of the end."""
    J, h, beta, csr, (qs, escale) = mc.instance(name)
    m0 = sf.aligned_state(J, h)
    cb = np.tile(np.array(oracle.cb_pair(beta, 1.0, False)), (3, 1))
    _, s_fin, tr = oracle.sweeps_philox(csr, h, m0, cb, SEED, 0, escale=escale, efix0=sf.dense_exact_efix_f32(J, h, m0, qs, escale))
    assert not np.array_equal(s_fin, m0)
    assert int(tr[-1]) == sf.dense_exact_efix_f32(J, h, s_fin, qs, escale)


# ---- the coverage conditions of the GPU file's case set -----------------------------------------------------------------------------

def scales_of(group):
    return {(qs, escale - qs) for qs, escale in (mc.instance(nm, n)[4] for nm, n, _ in mc.GROUPS[group])}


@pytest.mark.parametrize("group", list(mc.GROUPS))
def test_every_group_of_routes_sees_both_ends_of_the_shift_and_a_negative_scale(group):
    got = scales_of(group)
    print(f"{group}: (qs, eshift) {sorted(got)}")
    assert any(qs <= -18 for qs, _ in got)
    assert (52, 0) in got
    assert any(sh == 29 for _, sh in got)
    assert any(0 < sh < 29 for _, sh in got)


def test_scales_the_issue_lists():
    want = {("x3e15", 48): (-29, 29), ("x3e15", 100): (-29, 29), ("x2p40", 48): (-18, 29), ("x2p40", 100): (-18, 29),
            ("x1e9", 48): (-7, 29), ("x1e9", 100): (-7, 29), ("x1e-9", 48): (52, 0), ("x1e-9", 100): (52, 0), ("x1e-20", 48): (52, 0),
            ("x1e-20", 100): (52, 0), ("bigh", 48): (21, 25), ("bigh", 100): (21, 24), ("honly", 50): (8, 29), ("bigh", 300): (21, 22),
            ("x1e9", 300): (-7, 28), ("flat513", None): (22, 21), ("flat256h", None): (22, 21), ("flat1024", None): (21, 20)}
    for (nm, n), (qs, sh) in want.items():
        q, e = mc.instance(nm, n)[4]
        assert (q, e - q) == (qs, sh), (nm, n)


@pytest.mark.parametrize("group", list(mc.DENSE_GROUPS))
def test_every_dense_route_starts_a_chain_at_the_int32_limit(group):
    best = 0
    for nm, n, prec in mc.DENSE_GROUPS[group]:
        if prec == "f32" and mc.is_dense(nm):
            rows = mc.LADDER * mc.LADDERS if "rounds" in group else mc.ROWS
            best = max(best, abs(int(mc.start_fields(nm, n, rows)[mc.ALIGNED, 0])))
    assert 0.99 * LIMIT <= best < LIMIT


@pytest.mark.parametrize("name", sf.DENSE + (mc.FLAT192H,))
@pytest.mark.parametrize("ladder", [False, True], ids=["sweeps", "rounds"])
def test_the_opposed_chain_flips_spin_0_at_the_limit(name, ladder):
    """Chain OPPOSED of a dense case (spin 0 against a local field of the whole row sum): under the oracle spin 0 flips in the first
    sweep, and after what moved before it |X_0| was still above 2^30 then -- an energy delta of 2 |X_0| 2^eshift whose factor
    2 |X_0| no longer fits int32.  In rounds the chain sits on the fourth rung."""
    J, h, beta, csr, (qs, escale) = mc.instance(name)
    m0 = mc.start_spins(name, None, mc.ROWS)[mc.OPPOSED]
    b = beta * np.linspace(0.9, 1.1, mc.LADDER)[mc.OPPOSED] if ladder else beta
    M, _, _ = oracle.sweeps_philox(csr, h, m0, np.array([oracle.cb_pair(b, 1.0, False)]), mc.SEED, mc.OPPOSED, escale=escale)
    bound = mc.field_at_first_visit(name, None, m0, M[0])
    print(f"{name}: spin 0 flipped with |X_0| = {bound} = {bound / LIMIT:.4f} 2^31")
    assert M[0][0] == -m0[0] and mc.FLIP_FLOOR[name] <= bound < LIMIT


def test_largest_start_fields_by_group():
    """The figures of the case set: per group the (qs, eshift) pairs and the largest |X| over the start states (all inside int32)."""
    for group, cases in mc.GROUPS.items():
        top = max((int(np.max(np.abs(mc.start_fields(nm, n, rows)))), mc.case_id((nm, n))) for nm, n, rows in cases)
        assert top[0] < LIMIT
        print(f"{group}: largest |X| {top[0]} = {top[0] / LIMIT:.4f} 2^31 on {top[1]}; (qs, eshift) {sorted(scales_of(group))}")
