"""The fixed-point scales (qs, escale) and the oracle's energy bookkeeping over the magnitude family of scalefamily.py: couplings
from 1e-20 to 3e15, a hub row, |h| >> |J|, dyadic instances, couplings that all quantise to 0, fields only.  No GPU: the oracle
(oracle/nlo.c) against plain Python-int / Fraction restatements, so that the GPU tests of test_gpu_magnitude.py compare the device
with an oracle that is itself pinned at these magnitudes."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import oracle
import scalefamily as sf
from helpers import init_spins

SEED = 0x5CA1E
S = 6


@functools.lru_cache(maxsize=None)
def case(name):
    J, h, beta = sf.member(name)
    csr = oracle.Csr(J)
    return J, h, beta, csr, oracle.field_scale(csr, h)


@pytest.mark.parametrize("name", sf.NAMES)
def test_scale_is_the_stated_rule_and_the_pinned_pair(name):
    J, h, _, _, got = case(name)
    assert got == sf.scale_rule(J, h)
    assert got == sf.PINNED[name]


@pytest.mark.parametrize("name", sf.NAMES)
def test_invariants_of_the_header(name):
    """|Jq| <= 2^23 - 1, every row sum <= 2^31 - 1, qs <= escale <= qs + 29, (sum|J|/2 + sum|h|) 2^escale < 2^60."""
    J, h, _, _, (qs, escale) = case(name)
    rows, hq = sf.quantise(J, h, qs)
    assert all(abs(q) <= (1 << 23) - 1 for row in rows for _, q in row)
    sums = [sum(abs(q) for _, q in row) + abs(x) for row, x in zip(rows, hq)]
    assert max(sums) <= (1 << 31) - 1
    assert qs <= escale <= qs + 29
    assert sf.abs_terms(J, h) * (1 << escale) < (1 << 60)
    # what the family is there for (the facts the issue states about single members)
    if name == "x1e-20":
        assert not any(q for row in rows for _, q in row) and not any(hq)
    if name == "pmJ_2p7":
        assert {q for row in rows for _, q in row} == {-1, 1}
    if name == "pmJ_2m10_h":
        assert max(sums) == 116
    if name == "hub":
        assert max(sums) == 1569193912
    if name == "bigh":
        assert max(sums) == 1995757741 and max(abs(q) for row in rows for _, q in row) < (1 << 22)   # |h| forces the scale, not |J|
    if name in sf.DYADIC:
        assert all(Fraction(q, 1) == sf._scaled(Fraction(float(v)), qs) for (_, q), v in
                   zip((e for row in rows for e in row), oracle.Csr(J).data))
        assert max(sums) <= 4095


@pytest.mark.parametrize("name", sf.NAMES)
def test_f32_oracle_trace_is_the_exact_quantised_energy(name):
    """Six sweeps from efix0 = the exact quantised energy of the start: the trace ends on the exact quantised energy of the end."""
    J, h, beta, csr, (qs, escale) = case(name)
    m0 = init_spins(1, csr.n)[0]
    cb = np.tile(np.array(oracle.cb_pair(beta, 1.0, False)), (S, 1))
    M, s_fin, tr = oracle.sweeps_philox(csr, h, m0, cb, SEED, 0, escale=escale, efix0=sf.exact_efix_f32(J, h, m0, qs, escale))
    assert not np.array_equal(s_fin, m0)
    assert int(tr[-1]) == sf.exact_efix_f32(J, h, s_fin, qs, escale)


@pytest.mark.parametrize("name", sf.NAMES)
def test_f64_oracle_trace_stays_within_its_rounding_bound(name):
    J, h, beta, csr, (qs, escale) = case(name)
    m0 = init_spins(1, csr.n)[0]
    cb = np.tile(np.array(oracle.cb_pair(beta, 1.0, True)), (S, 1))
    e0 = int(round(sf.exact_energy(J, h, m0) * (1 << escale)))
    M, s_fin, tr = oracle.sweeps_philox(csr, h, m0, cb, SEED, 0, escale=escale, use_f64=True, efix0=e0)
    assert not np.array_equal(s_fin, m0)
    flips = int(np.count_nonzero(np.diff(np.concatenate([m0[None], M]).astype(np.int32), axis=0)))
    err = abs(int(tr[-1]) - sf.exact_energy(J, h, s_fin) * (1 << escale))
    bound = sf.f64_trace_bound(J, h, flips, escale)
    print(f"{name}: fp64 trace error {float(err):.3g} units of 2^-{escale}, bound {float(bound):.3g}, {flips} flips")
    assert err <= bound


@pytest.mark.parametrize("name", sf.NAMES)
def test_oracle_energy_within_the_summation_bound(name):
    J, h, _, csr, _ = case(name)
    bound = sf.energy_bound(J, h)
    for s in (init_spins(1, csr.n)[0], np.ones(csr.n, dtype=np.int8)):
        assert abs(Fraction(oracle.energy(csr, h, s)) - sf.exact_energy(J, h, s)) <= bound
