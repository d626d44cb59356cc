"""The yardstick of test_gpu_icm_shapes.py, checked without a GPU: every builder of tests/icmshapes.py keeps its promises, the
SciPy component search equals oracle.clusters (C code, oracle/nlo.c) on every shape, and the move reference equals
fake_engine.OracleEngine.icm_round_ladders on a small ladder."""
import numpy as np
import pytest

import oracle
import icmshapes as ics
from fake_engine import OracleEngine

TAG_ICM = 5


def small_shapes():
    out = []
    for n in (1, 2, 63, 64, 65):
        for order in ("ascending", "descending", "permuted"):
            out.append(ics.path(n, order))
    out += [ics.path(65, "permuted", agree=(20,)), ics.path(64, "descending", agree=(0, 31, 32, 63))]
    for n in (2, 17, 18, 65):
        out += [ics.star(n, 0), ics.star(n, n - 1)]
    out += [ics.complete(96), ics.complete(3), ics.grid(7, 9), ics.grid(1, 5), ics.grid(8, 8)]
    for n in (6, 7, 64, 65):
        out += [ics.halves(n, False), ics.halves(n, True), ics.halves(n, True, order="ascending")]
    for n in (2, 63, 64):
        out += [ics.many(n), ics.many(n, edges=False)]
    for n in (8, 63, 64):
        out += [ics.zero_bridge(n, False), ics.zero_bridge(n, True)]
    return out


SHAPES = small_shapes()
IDS = [f"{s.name}-{s.n}" for s in SHAPES]


def oracle_csr(shape):
    return oracle.Csr.from_parts(*ics.csr_parts(shape))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_builders_keep_their_promises(shape):
    J = shape.J
    assert (abs(J - J.T)).nnz == 0 and J.has_sorted_indices
    assert shape.s_a.dtype == np.int8 and set(np.unique(shape.s_a)) <= {-1, 1} and set(np.unique(shape.s_b)) <= {-1, 1}
    if shape.integer:
        assert set(np.unique(J.data)) <= {-1.0, 1.0} and set(np.unique(shape.h)) <= {-1.0, 0.0, 1.0} and shape.h.any()
    labels, comps, sizes = ics.components(J, shape.s_a, shape.s_b)
    assert len(comps) == shape.ncomp
    assert sorted(sizes.tolist(), reverse=True) == shape.sizes
    assert ics.diameter_of_largest(J, shape.s_a, shape.s_b) == shape.diameter
    # labels: smallest member, ascending-label order of the list, -1 exactly where the spins agree
    assert np.array_equal(labels == -1, shape.s_a == shape.s_b)
    assert [int(c[0]) for c in comps] == sorted(int(c[0]) for c in comps)
    for c in comps:
        assert np.all(labels[c] == c[0]) and np.all(np.diff(c) > 0)


def test_shape_specific_promises():
    n = 65
    assert np.diff(ics.star(n, 0).J.indptr)[0] == n - 1 and np.diff(ics.star(n, n - 1).J.indptr)[n - 1] == n - 1
    assert np.all(np.diff(ics.complete(96).J.indptr) == 95)
    assert np.max(np.diff(ics.grid(7, 9).J.indptr)) == 4
    for m in (64, 65, 4096, 4097):
        u, o = ics.halves(m, False), ics.halves(m, True)
        assert u.sizes == [m // 2, m // 2 - 1] and not u.sizes[0] > m // 2
        assert o.sizes == [m // 2 + 1, m - m // 2 - 2] and o.sizes[0] > m // 2
    mm = ics.many(64)
    d = mm.s_a != mm.s_b
    A = mm.J.tocoo()
    assert np.all(np.diff(mm.J.indptr) == 1) and np.all(d[A.row] != d[A.col])           # one end of every edge
    assert ics.many(64, edges=False).J.nnz == 0
    for tiny in (False, True):
        z = ics.zero_bridge(64, tiny)
        i, j = z.facts["bridge"]
        assert z.J[i, j] == (1e-13 if tiny else 0.0) and z.J[j, i] == z.J[i, j]
        stored = z.J.indices[z.J.indptr[i]:z.J.indptr[i + 1]]
        assert j in stored and (z.J.data == 0.0).any() and z.J.diagonal().any()
        # without the bridge the two paths are separate
        cut = z.J.copy()
        cut.data[(cut.data != 0) & (np.abs(cut.data) < 1e-12)] = 0.0
        assert len(ics.components(cut, z.s_a, z.s_b)[1]) == 2


def test_degenerate_pairs():
    for base in (ics.grid(7, 9), ics.many(64), ics.zero_bridge(64, False), ics.path(65, "permuted", agree=(20,))):
        same, opp = ics.identical(base), ics.opposite(base)
        labels, comps, _ = ics.components(base.J, same.s_a, same.s_b)
        assert not comps and np.all(labels == -1)
        assert ics.move(base.J, same.s_a, same.s_b, 3, True)[2] == (0, 0)
        _, comps, sizes = ics.components(base.J, opp.s_a, opp.s_b)
        from scipy.sparse.csgraph import connected_components
        A = base.J.copy()
        A.eliminate_zeros()
        assert len(comps) == connected_components(A, directed=False)[0] and sizes.sum() == base.n


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_scipy_reference_equals_oracle_clusters(shape):
    csr = oracle_csr(shape)
    for s in (shape, ics.identical(shape), ics.opposite(shape)):
        _, comps, _ = ics.components(shape.J, s.s_a, s.s_b)
        cl = oracle.clusters(csr, s.s_a, s.s_b)
        assert len(cl) == len(comps)
        for x, y in zip(cl, comps):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("katz", [True, False])
@pytest.mark.parametrize("shape", [s for s in SHAPES if s.n >= 6 and s.n in (6, 7, 8, 63, 64, 65, 96)][::3], ids=lambda s: f"{s.name}-{s.n}")
def test_move_reference_equals_the_oracle_engine(shape, katz):
    """A ladder of 2 slots x 4 sub-replicas whose chains hold the shape's states: OracleEngine pairs them and moves them with
    oracle.clusters; the same pairs moved by icmshapes.move give the same states, info and energies."""
    R, K, seed, rnd = 2, 4, 424242, 3
    inst = ics.HostInstance(shape)
    csr = oracle_csr(shape)
    r = np.random.default_rng(5)
    states = ics.ladder_states(shape, r)
    eng = OracleEngine(inst, R * K, 0, R * K)
    eng.pt_init(np.array([0.5, 1.0]))
    eng.set_spins(states)
    info = eng.icm_round_ladders(rnd, seed, katzgraber=katz, want_info=True)
    exp, exp_info = expected_ladder_round(shape, states, R, K, rnd, seed, katz)
    assert np.array_equal(eng.get_spins(), exp)
    assert np.array_equal(info, exp_info)
    esc = oracle.field_scale(csr, shape.h)[1]
    E = np.array([np.rint(oracle.energy(csr, shape.h, s) * 2.0 ** esc) * 2.0 ** -esc for s in exp])
    assert np.array_equal(eng.energy_tracked(), E)
    assert info[:, 0].max() > 0                                  # some pair did move


def expected_ladder_round(shape, states, R, K, rnd, seed, katz, slots=None):
    """nlmc_icm_round_ladders restated with icmshapes.move: per slot the K ladders are ordered by their keys philox(j, round, slot,
    ICM_PAIR) and paired; the pick of a pair is keyed by its two chain ids."""
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    exp = states.copy()
    info = []
    for slot in range(R):
        keys = [int(oracle.philox(j, rnd, slot, 6, lo, hi)[0]) for j in range(K)]
        sh = sorted(range(K), key=lambda j: (keys[j], j))
        for q in range(K // 2):
            a, b = sh[2 * q] * R + slot, sh[2 * q + 1] * R + slot
            ncomp = len(ics.components(shape.J, exp[a], exp[b])[1])
            pick = (int(oracle.philox(a, rnd, b, TAG_ICM, lo, hi)[0]) * ncomp) >> 32 if ncomp else 0
            exp[a], exp[b], i = ics.move(shape.J, exp[a], exp[b], pick, katz)
            info.append(i)
    return exp, np.array(info, np.int32).reshape(-1, 2)
