"""Iso-cluster kernels (k_icm_components, k_icm_move, k_icm_round and their global-memory twins) on the graphs and sizes where a
lock-free union-find, the pick scan and the energy bookkeeping can go wrong: deep paths in three labellings, hubs whose row runs past
the 16-entry adjacency table, a dense graph, a lattice, clusters on either side of n / 2, thousands of one-spin components, a stored
coupling of exactly zero -- at sizes around one wave, around the switch to 1024 threads (n = 4096), at the largest LDS size and the
first size of the `_big` kernels, and once more at a small size with NLMC_FORCE_BIG.

Reference: tests/icmshapes.py (SciPy component search, the move rule of NPT/apt_ICM.py:232-246), shown equal to oracle.clusters and
to fake_engine.OracleEngine in test_icm_shapes_cpu.py.  Integer instances compare for equality in spins, labels, info and energies;
the real-valued zero_bridge instances use energy_tolerance of test_gpu_apt_lanes.py with no updates.

Every case asserts on the reference that the branch it is there for was taken.

complete() is pinned at n = 96 (rows of 95 entries, six times the table): at n = 4097 its 16.8 million stored couplings take 2.4 s
to build on the host and 1.7 s for every component search of the reference, of which a round test makes ten, so long rows cross the
thread-count switch through star(), whose hub row is as long as a row can be.

Found by these tests: k_icm_round was refused ("instance too large for the LDS-resident kernels") from n = 20 221 to 24 576, sizes
every other call accepts; such chains now take k_icm_round_big (ROUND_LDS_N below pins both sides of that switch).  And on
path-descending-24577 the round once reported a giant cluster of 24 571 spins: the final labelling pass of both round kernels let a
halving store of another thread put an inner node back over a root just written; that pass no longer stores while it walks."""
import numpy as np
import pytest

import oracle
import icmshapes as ics
from fake_engine import OracleEngine
from test_gpu_apt_lanes import energy_tolerance

pytestmark = pytest.mark.gpu
TAG_ICM = 5
LDS_N = 24576                      # _abi.LDS_N (asserted below)
ROUND_LDS_N = 20220                # the longest chain whose k_icm_round state (8 bytes a spin + alignment) fits the 158 KiB of dynamic LDS:
                                   # 4 n + 2 (n rounded up to 8) + 2 (n rounded up to 16) + 16 = 161 792 there; from 20 221 on the round takes
                                   # k_icm_round_big while components and moves by index stay in LDS up to LDS_N
SEED = 0x5EED00000000 + 20250917    # both halves of the Philox key in use


def _cases():
    c = []

    def add(name, build, big=False):
        c.append(pytest.param((name, build, big), id=name + ("-forcebig" if big else "")))
    # around one wave; every shape once more on the global-memory kernels at a small size
    for n in (63, 64, 65):
        order = {63: "ascending", 64: "descending", 65: "permuted"}[n]
        add(f"path-{order}-{n}", lambda n=n, order=order: ics.path(n, order))
        add(f"star-hub0-{n}", lambda n=n: ics.star(n, 0))
        add(f"star-hublast-{n}", lambda n=n: ics.star(n, n - 1))
        add(f"halves-under-{n}", lambda n=n: ics.halves(n, False))
        add(f"halves-over-{n}", lambda n=n: ics.halves(n, True))
        add(f"many-matching-{n}", lambda n=n: ics.many(n))
        add(f"zero-bridge-{'tiny' if n == 64 else 'zero'}-{n}", lambda n=n: ics.zero_bridge(n, n == 64))
    add("path-1", lambda: ics.path(1, "ascending"))
    add("path-cut-65", lambda: ics.path(65, "permuted", agree=(20,)))
    add("grid-7x9", lambda: ics.grid(7, 9))
    add("grid-8x8", lambda: ics.grid(8, 8))
    add("grid-5x13", lambda: ics.grid(5, 13))
    add("many-edgeless-64", lambda: ics.many(64, edges=False))
    add("complete-96", lambda: ics.complete(96))
    for order in ("ascending", "descending", "permuted"):
        add(f"path-{order}-65", lambda order=order: ics.path(65, order), big=True)
    add("path-cut-65", lambda: ics.path(65, "permuted", agree=(20,)), big=True)
    add("star-hub0-65", lambda: ics.star(65, 0), big=True)
    add("star-hublast-65", lambda: ics.star(65, 64), big=True)
    add("complete-96", lambda: ics.complete(96), big=True)
    add("grid-7x9", lambda: ics.grid(7, 9), big=True)
    add("halves-under-64", lambda: ics.halves(64, False), big=True)
    add("halves-under-65", lambda: ics.halves(65, False), big=True)
    add("halves-over-64", lambda: ics.halves(64, True), big=True)
    add("halves-over-65", lambda: ics.halves(65, True), big=True)
    add("many-matching-64", lambda: ics.many(64), big=True)
    add("many-edgeless-65", lambda: ics.many(65, edges=False), big=True)
    add("zero-bridge-zero-64", lambda: ics.zero_bridge(64, False), big=True)
    add("zero-bridge-tiny-65", lambda: ics.zero_bridge(65, True), big=True)
    # the switch from 256 to 1024 threads
    for n in (4095, 4096, 4097):
        add(f"path-permuted-{n}", lambda n=n: ics.path(n, "permuted"))
        add(f"halves-under-{n}", lambda n=n: ics.halves(n, False))
        add(f"halves-over-{n}", lambda n=n: ics.halves(n, True))
    add("path-ascending-4097", lambda: ics.path(4097, "ascending"))
    add("path-descending-4097", lambda: ics.path(4097, "descending"))
    add("path-cut-4097", lambda: ics.path(4097, "permuted", agree=(1000, 3000)))
    add("star-hub0-4097", lambda: ics.star(4097, 0))
    add("star-hublast-4097", lambda: ics.star(4097, 4096))
    add("grid-17x241", lambda: ics.grid(17, 241))                    # 4097 spins
    add("many-matching-4097", lambda: ics.many(4097))
    add("many-edgeless-4097", lambda: ics.many(4097, edges=False))
    add("zero-bridge-zero-4097", lambda: ics.zero_bridge(4097, False))
    add("zero-bridge-tiny-4097", lambda: ics.zero_bridge(4097, True))
    # the last size of the LDS round kernel and the first that takes the global-memory one
    for n in (ROUND_LDS_N, ROUND_LDS_N + 1):
        add(f"path-permuted-{n}", lambda n=n: ics.path(n, "permuted"))
        add(f"star-hublast-{n}", lambda n=n: ics.star(n, n - 1))
        add(f"halves-over-{n}", lambda n=n: ics.halves(n, True))
    # the largest LDS size and the first size of the global-memory kernels
    for n in (LDS_N, LDS_N + 1):
        add(f"path-permuted-{n}", lambda n=n: ics.path(n, "permuted"))
        add(f"path-{'ascending' if n == LDS_N else 'descending'}-{n}", lambda n=n: ics.path(n, "ascending" if n == LDS_N else "descending"))
        add(f"star-hub0-{n}", lambda n=n: ics.star(n, 0))
        add(f"star-hublast-{n}", lambda n=n: ics.star(n, n - 1))
        add(f"halves-under-{n}", lambda n=n: ics.halves(n, False))
        add(f"halves-over-{n}", lambda n=n: ics.halves(n, True))
    add(f"many-matching-{LDS_N}", lambda: ics.many(LDS_N))
    add(f"many-edgeless-{LDS_N + 1}", lambda: ics.many(LDS_N + 1, edges=False))
    return c


CASES = _cases()
_BUILT = {}


@pytest.fixture
def case(request, product, monkeypatch):
    """-> (shape, product.Instance, oracle.Csr); the knob NLMC_FORCE_BIG is read when a context is created."""
    name, build, big = request.param
    assert product._abi.LDS_N == LDS_N
    if big:
        monkeypatch.setenv("NLMC_FORCE_BIG", "1")
    else:
        monkeypatch.delenv("NLMC_FORCE_BIG", raising=False)
    if name not in _BUILT:
        sh = build()
        _BUILT[name] = (sh, oracle.Csr.from_parts(*ics.csr_parts(sh)))
    sh, csr = _BUILT[name]
    check_intent(name, sh, big)
    return sh, ics.engine_instance(product, sh), csr


def check_intent(name, sh, big):
    """The shape is what the case is there for (facts of the instance; the branch a move takes is asserted where it is taken)."""
    deg = np.diff(sh.J.indptr)
    if name.startswith("star") or name.startswith("complete"):
        assert deg.max() > 16                                         # the hub's row runs past the adjacency table into the CSR tail
    if name.startswith("zero-bridge"):
        assert (sh.J.data == 0.0).any() and sh.J.diagonal().any()      # a stored zero: the kernels read the CSR entries
        assert sh.ncomp == (1 if "tiny" in name else 2)
    else:
        assert not (sh.J.data == 0.0).any()
    if name.startswith("many") and sh.n >= 4097:
        assert sh.ncomp > 1024                                        # more roots than threads: every chunk of the pick scan holds some
    if name.startswith("halves"):
        assert len(sh.sizes) == 2 and (sh.sizes[0] > sh.n // 2) == ("over" in name)
        if "under" in name:
            assert sh.sizes[0] == sh.n // 2
    if name.endswith(str(LDS_N + 1)):
        assert sh.n > LDS_N


def energies(csr, sh, states):
    return np.array([oracle.energy(csr, sh.h, s) for s in states])


def assert_energy(sh, inst, eng, got, want):
    if sh.integer:
        assert np.array_equal(got, want)
    else:
        assert np.max(np.abs(got - want)) <= energy_tolerance(inst, eng.field_scale, eng.energy_scale, False, 0)


def philox_pick(a, b, rnd, ncomp):
    w = int(oracle.philox(a, rnd, b, TAG_ICM, SEED & 0xFFFFFFFF, SEED >> 32)[0])
    return (w * ncomp) >> 32


@pytest.mark.parametrize("case", CASES, indirect=True)
def test_components_and_labels(product, case):
    sh, inst, _ = case
    states = np.stack([sh.s_a, sh.s_b, sh.s_a, -sh.s_a])
    with product.Engine(inst, None, 4) as eng:
        eng.set_spins(states)
        for a, b in ((0, 1), (1, 0), (0, 2), (0, 3)):                 # the pair, the pair reversed, identical, opposite
            labels, comps, _ = ics.components(sh.J, states[a], states[b])
            assert eng.icm_components(a, b) == len(comps)
            assert np.array_equal(eng.icm_labels(), labels)
            if (a, b) == (0, 1):
                assert len(comps) == sh.ncomp
            if (a, b) == (0, 2):
                assert len(comps) == 0
            if (a, b) == (0, 3):
                assert sum(len(c) for c in comps) == sh.n
        assert np.array_equal(eng.get_spins(), states)


@pytest.mark.parametrize("katz", [True, False])
@pytest.mark.parametrize("case", CASES, indirect=True)
def test_move_by_index(product, case, katz):
    sh, inst, csr = case
    _, comps, sizes = ics.components(sh.J, sh.s_a, sh.s_b)
    nc = len(comps)
    picks = sorted({0, nc - 1, nc // 2, nc + 1, int(np.argmax(sizes))})        # first, last, middle, one past the count, the largest
    giant = set()
    with product.Engine(inst, None, 2) as eng:
        for pick in picks:
            eng.set_spins(np.stack([sh.s_a, sh.s_b]))
            info = eng.icm_move(0, 1, pick, katzgraber=katz)
            ea, eb, einfo = ics.move(sh.J, sh.s_a, sh.s_b, pick, katz)
            got = eng.get_spins()
            assert info == einfo
            assert np.array_equal(got[0], ea) and np.array_equal(got[1], eb)
            assert_energy(sh, inst, eng, eng.energy(), energies(csr, sh, [ea, eb]))
            if einfo[1] > sh.n // 2:
                giant.add(pick % nc)
    assert len(giant) == int(sh.sizes[0] > sh.n // 2)               # exactly the giant cluster is above n / 2 ...
    if "largest" in sh.facts:
        assert sh.facts["largest"] in (sh.n // 2, sh.n // 2 + 1)     # ... and halves() sits on either side of the boundary


ROUND_PAIRS = np.array([[0, 1], [3, 2], [4, 5], [7, 6]], np.int32)     # the shape's pair, identical, opposite, against a random state
ROUND_BASE, ROUND_GLOBAL, ROUND_CHAINS = 4, 16, 10


def round_states(sh):
    r = np.random.default_rng(77)
    x, y, z = (r.choice(np.array([-1, 1], np.int8), sh.n) for _ in range(3))
    return np.stack([sh.s_a, sh.s_b, sh.s_a, sh.s_a, x, -x, sh.s_b, y, z, sh.s_a])       # chains 8 and 9 are in no pair


@pytest.mark.parametrize("katz", [True, False])
@pytest.mark.parametrize("case", CASES, indirect=True)
def test_round_philox(product, case, katz):
    sh, inst, csr = case
    states = round_states(sh)
    _, comps, sizes = ics.components(sh.J, sh.s_a, sh.s_b)
    # a round whose pick for the shape's pair is its largest component: the one that flips (or, on the boundary, must not)
    rnd = next(r for r in range(256) if sizes[philox_pick(ROUND_BASE + 0, ROUND_BASE + 1, r, len(comps))] == sizes.max())

    def run():
        with product.Engine(inst, None, ROUND_CHAINS, chain_base=ROUND_BASE, n_chains_global=ROUND_GLOBAL) as eng:
            eng.set_spins(states)
            info = eng.icm_round_philox(ROUND_PAIRS, rnd, SEED, katzgraber=katz, want_info=True)
            tracked = eng.energy_tracked()
            return eng.get_spins(), info, tracked, eng.energy(), eng.field_scale, eng.energy_scale

    got, info, tracked, E, qs, esc = run()
    exp, exp_info = states.copy(), []
    for a, b in ROUND_PAIRS:
        nc = len(ics.components(sh.J, states[a], states[b])[1])
        pick = philox_pick(ROUND_BASE + a, ROUND_BASE + b, rnd, nc) if nc else 0
        exp[a], exp[b], i = ics.move(sh.J, states[a], states[b], pick, katz)
        exp_info.append(i)
    exp_info = np.array(exp_info, np.int32)
    assert exp_info[0, 1] == sh.sizes[0] and exp_info[0, 0] == sh.ncomp
    if sh.sizes[0] > sh.n // 2 and katz:
        assert np.array_equal(exp[0], -states[0]) and np.array_equal(exp[1], states[1])          # the global flip ...
        assert sh.h @ states[0].astype(float) != 0 or sh.n == 1      # ... whose energy change 2 h.s does not vanish
    else:
        assert np.array_equal(exp[0] != states[0], exp[1] != states[1]) and (exp[0] != states[0]).sum() == sh.sizes[0]   # the exchange
    assert tuple(exp_info[1]) == (0, 0) and exp_info[2, 0] >= 1 and np.array_equal(exp[[2, 3]], states[[2, 3]])
    assert np.array_equal(info, exp_info)
    assert np.array_equal(got, exp)
    assert np.array_equal(got[8:], states[8:])                       # chains that are in no pair
    want = energies(csr, sh, exp)
    if sh.integer:
        assert np.array_equal(tracked, E) and np.array_equal(E, want)
    else:
        tol = energy_tolerance(inst, qs, esc, False, 0)
        assert np.max(np.abs(tracked - E)) <= tol and np.max(np.abs(E - want)) <= tol
    again = run()
    for x, y in zip((got, info, tracked, E), again):
        assert np.array_equal(x, y)


def ladder_order(rnd, slot, K):
    """The K ladders of a slot in the order of their keys philox(ladder, round, slot, ICM_PAIR): neighbours are paired."""
    keys = [int(oracle.philox(j, rnd, slot, 6, SEED & 0xFFFFFFFF, SEED >> 32)[0]) for j in range(K)]
    return sorted(range(K), key=lambda j: (keys[j], j))


@pytest.mark.parametrize("katz", [True, False])
@pytest.mark.parametrize("case", CASES, indirect=True)
def test_round_ladders(product, case, katz):
    """2 temperature slots x 4 sub-replicas holding the shape's states (icmshapes.ladder_states), paired on the device."""
    sh, inst, csr = case
    R, K = 2, 4
    states = ics.ladder_states(sh, np.random.default_rng(5))
    # a round that pairs an s_a with an s_b on slot 0 (ladders 0 and 2 hold s_a there, 1 and 3 s_b): the shape's own pair is moved
    rnd = next(r for r in range(64) if ladder_order(r, 0, K)[0] % 2 != ladder_order(r, 0, K)[1] % 2)
    ref = OracleEngine(ics.HostInstance(sh), R * K, 0, R * K)
    ref.pt_init(np.array([0.5, 1.0]))
    ref.set_spins(states)
    exp_info = ref.icm_round_ladders(rnd, SEED, katzgraber=katz, want_info=True)
    exp = ref.get_spins()

    def run():
        with product.Engine(inst, None, R * K) as eng:
            eng.set_spins(states)
            eng.pt_init(np.array([0.5, 1.0]))
            info = eng.icm_round_ladders(rnd, SEED, katzgraber=katz, want_info=True)
            tracked = eng.energy_tracked()
            return eng.get_spins(), info, tracked, eng.energy(), eng.field_scale, eng.energy_scale

    got, info, tracked, E, qs, esc = run()
    assert exp_info[0, 0] == sh.ncomp and exp_info[1, 0] == sh.ncomp                 # slot 0: the shape's pair, twice
    assert not np.array_equal(exp, states)
    assert np.array_equal(info, exp_info)
    assert np.array_equal(got, exp)
    want = energies(csr, sh, exp)
    if sh.integer:
        assert np.array_equal(tracked, ref.energy_tracked()) and np.array_equal(tracked, E) and np.array_equal(E, want)
    else:
        tol = energy_tolerance(inst, qs, esc, False, 0)
        assert max(np.max(np.abs(tracked - ref.energy_tracked())), np.max(np.abs(tracked - E)), np.max(np.abs(E - want))) <= tol
    again = run()
    for x, y in zip((got, info, tracked, E), again):
        assert np.array_equal(x, y)
