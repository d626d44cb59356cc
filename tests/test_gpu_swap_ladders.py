"""Swap pair selection (pt_select_pairs, used by k_pt_swap and k_pt_select) on ladders longer than one 64-bit word of pairs.

A lane holds the availability of 64 adjacent pairs; a pick is located by a wave prefix sum over the lanes' popcounts and nth_set_bit,
and clears its neighbours i +- 1, which may sit in another lane's word.  With ladders of at most 32 temperatures lane 0 holds
everything.  Here: L in {2, 3, 64, 65, 66, 128, 129, 130, 1000, 4096} (L - 1 pairs: 63 fill a word less one bit, 64 fill it, 65 start
a second one; the same around two words; the host's limit), one pair per round and the most that can never exhaust, (L + 1) // 3.

The instance is tiny (N = 16, +-J, integer field): the kernel's cost does not depend on N.  Chains keep their start configurations
(helpers.init_spins, no sweeps), so the whole reference -- oracle.pt.swap_round from oracle.energy -- is known without a GPU, and
ROUNDS holds, per case, round numbers for which that reference alone meets the conditions of `conditions` below: they are asserted
on the reference before anything is compared.  Three routes -- selection inside the swap kernel, planned selections (k_pt_select),
energies handed in on the device and from the host -- must equal the reference round by round in pairs, decisions and slots.

L = 65 has 64 pairs, exactly one word: no pick of it has a neighbour in another word, so the cross-word conditions start at L = 66."""
import numpy as np
import pytest

import oracle
from oracle import pt as opt
from helpers import make_instance, init_spins, DeviceBuffer

pytestmark = pytest.mark.gpu
N, SEED = 16, 0x0B5E55ED00000000 + 4242
LADDERS = (2, 3, 64, 65, 66, 128, 129, 130, 1000, 4096)

# (L, n_pairs) -> the rounds run, found with tools of this file alone (find_rounds): the smallest set of round numbers, taken in
# ascending order from 0, after which every condition that applies to L holds and both decisions have occurred
ROUNDS = {
    (2, 1): (0, 1), (3, 1): (0, 1), (64, 1): (0, 1), (64, 21): (0, 1), (65, 1): (0, 1), (65, 22): (0, 1),
    (66, 1): (0, 7), (66, 22): (0, 1), (128, 1): (4, 82), (128, 43): (0, 1), (129, 1): (0, 1, 4, 9), (129, 43): (0, 1),
    (130, 1): (0, 4, 7), (130, 43): (0, 1), (1000, 1): (0, 1, 2, 3, 4, 44, 57), (1000, 333): (0, 1),
    (4096, 1): (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 38, 72), (4096, 1365): (0, 1),
}


def n_ladders(L):
    return 3 if L <= 130 else 1


def betas_of(L):
    return np.geomspace(0.05, 50.0 if L <= 130 else 2000.0, L)


_SETUP = {}


def setup(L):
    """(J, h, start spins [G, N], their energies): integers."""
    if L not in _SETUP:
        J, _ = make_instance(N, seed=31)
        h = np.random.default_rng(32).integers(-1, 2, N).astype(float)
        assert h.any()
        G = L * n_ladders(L)
        m0 = init_spins(G, N)
        csr = oracle.Csr(J)
        E = np.array([oracle.energy(csr, h, s) for s in m0])
        assert np.array_equal(E, np.rint(E))
        _SETUP[L] = (J, h, m0, E)
    return _SETUP[L]


def selection_trace(L, n_pairs, rnd, ladder):
    """oracle.pt.swap_round's selection of one (round, ladder), restated to see the availability at every pick:
    -> [(pick i, set of pairs available before it)]."""
    lo, hi = SEED & 0xFFFFFFFF, SEED >> 32
    avail, out = list(range(L - 1)), []
    for p in range(n_pairs):
        if not avail:
            raise ValueError("Cannot find non-overlapping pairs.")
        r = int(oracle.philox(p, rnd, ladder, opt.TAG_PAIR, lo, hi)[0])
        i = avail[(r * len(avail)) >> 32]
        out.append((i, avail))
        avail = [q for q in avail if abs(q - i) > 1]
    return out


def conditions(L, trace):
    """Which parts of pt_select_pairs a selection exercised:
    up    a pick on the last bit of a word while pair i + 1 (first bit of the next lane's word) was still available;
    down  a pick on the first bit of a word above the first while pair i - 1 (last bit of the previous lane's word) was available;
    rank  (L >= 129) a pick in a word above the first that is not the first available bit of its word: nth_set_bit behind a prefix."""
    got = set()
    for i, avail in trace:
        s = set(avail)
        if i % 64 == 63 and i + 1 in s:
            got.add("up")
        if i % 64 == 0 and i > 0 and i - 1 in s:
            got.add("down")
        if i >= 64 and any(q // 64 == i // 64 and q < i for q in avail):
            got.add("rank")
    return got


def wanted(L):
    return set() if L < 66 else ({"up", "down"} | ({"rank"} if L >= 129 else set()))


def reference_rounds(L, n_pairs, rounds):
    """-> per round (slots after, pairs, decisions), conditions met, decisions seen."""
    _, _, _, E = setup(L)
    nl, betas = n_ladders(L), betas_of(L)
    slots = (np.arange(L * nl) % L).astype(np.int32)
    out, met, seen = [], set(), set()
    for rnd in rounds:
        slots, pairs, acc = opt.swap_round(E, slots, betas, L, n_pairs, rnd, SEED)
        for g in range(nl):
            tr = selection_trace(L, n_pairs, rnd, g)
            assert [i for i, _ in tr] == pairs[g, :, 0].tolist()             # the restated selection is the reference's
            met |= conditions(L, tr)
        seen |= set(acc.ravel().tolist())
        out.append((slots, pairs, acc))
    return out, met, seen


def find_rounds(L, n_pairs, limit=4000):
    """The committed ROUNDS entry of a case (CPU only): scan rounds 0, 1, ... and keep one when its selection adds a condition still
    missing; then add rounds until both decisions have occurred and there are at least two."""
    need, rounds = wanted(L), []
    for rnd in range(limit):
        if not need:
            break
        got = set()
        for g in range(n_ladders(L)):
            got |= conditions(L, selection_trace(L, n_pairs, rnd, g))
        if got & need:
            need -= got
            rounds.append(rnd)
    assert not need, (L, n_pairs, need)
    rnd = 0
    while len(rounds) < 2 or reference_rounds(L, n_pairs, sorted(rounds))[2] != {0, 1}:
        while rnd in rounds:
            rnd += 1
        rounds.append(rnd)
        assert len(rounds) <= 16
    return tuple(sorted(rounds))


CASES = [(L, p) for L in LADDERS for p in sorted({1, (L + 1) // 3})]


def run_route(product, route, L, n_pairs, rounds):
    """-> [(slots, pairs, decisions)] of one fresh context."""
    J, h, m0, E = setup(L)
    out = []
    with product.Engine(J, h, len(m0)) as eng:
        eng.set_spins(m0)
        eng.pt_init(betas_of(L))
        assert np.array_equal(eng.energy_tracked(), E)
        buf = DeviceBuffer(E) if route == "device" else None
        for rnd in rounds:
            if route == "planned":
                eng.pt_plan(rnd, 1, SEED, n_pairs)
            if route == "host":
                pairs, acc = eng.pt_swap_philox_host(rnd, SEED, n_pairs, E, want_log=True)
            else:
                pairs, acc = eng.pt_swap_philox(rnd, SEED, n_pairs, energies_all_dev=buf.ptr.value if buf else None)
            out.append((eng.pt_slots(), pairs, acc))
        if buf:
            buf.free()
        assert np.array_equal(eng.get_spins(), m0)
    return out


@pytest.mark.parametrize("L,n_pairs", CASES)
def test_swap_rounds_equal_the_reference_on_every_route(product, L, n_pairs):
    rounds = ROUNDS[(L, n_pairs)]
    ref, met, seen = reference_rounds(L, n_pairs, rounds)
    assert met >= wanted(L)                                    # cross-word clearing both ways, nth_set_bit behind a prefix
    assert seen == {0, 1}                                      # the reference accepted some pairs and refused others
    G = L * n_ladders(L)
    assert not np.array_equal(ref[-1][0], np.arange(G) % L)
    for route in ("kernel", "planned", "device", "host"):
        got = run_route(product, route, L, n_pairs, rounds)
        for k, ((slots, pairs, acc), (eslots, epairs, eacc)) in enumerate(zip(got, ref)):
            assert np.array_equal(pairs, epairs), (route, rounds[k])
            assert np.array_equal(acc, eacc), (route, rounds[k])
            assert np.array_equal(slots, eslots), (route, rounds[k])


@pytest.mark.parametrize("L,n_pairs", [(2, 2), (3, 2)])
def test_a_selection_that_runs_out_of_pairs_raises_like_the_reference(product, L, n_pairs):
    """Two pairs out of ladders of 2 and 3 temperatures: whichever pair is picked first, none is left for the second (L = 2 is refused
    by the host's argument check, L = 3 by the kernel's count of available pairs)."""
    J, h, m0, E = setup(L)
    rnd = 0
    with pytest.raises(ValueError, match="non-overlapping"):
        opt.swap_round(E, np.arange(len(m0)) % L, betas_of(L), L, n_pairs, rnd, SEED)
    for route in ("kernel", "planned", "device", "host"):
        with product.Engine(J, h, len(m0)) as eng:
            eng.set_spins(m0)
            eng.pt_init(betas_of(L))
            buf = DeviceBuffer(E)
            with pytest.raises(ValueError, match="non-overlapping"):
                if route == "planned":
                    eng.pt_plan(rnd, 1, SEED, n_pairs)
                elif route == "host":
                    eng.pt_swap_philox_host(rnd, SEED, n_pairs, E, want_log=True)
                else:
                    eng.pt_swap_philox(rnd, SEED, n_pairs, energies_all_dev=buf.ptr.value if route == "device" else None)
            assert np.array_equal(eng.pt_slots(), np.arange(len(m0)) % L)
            buf.free()


def test_the_ladder_length_limit_is_refused_on_both_entries(product):
    """4096 temperatures are the most a wave's 64 words hold (4095 pairs): 4096 runs (above), 4097 is refused, with nothing changed."""
    L = 4097
    J, h, _, _ = setup(2)
    m0 = init_spins(L, N)
    with product.Engine(J, h, L) as eng:
        eng.set_spins(m0)
        eng.pt_init(betas_of(L))
        E = eng.energy_tracked()
        with pytest.raises(NotImplementedError, match="nlmc_pt_plan: ladder_len > 4096"):
            eng.pt_plan(0, 2, SEED, 1)
        with pytest.raises(NotImplementedError, match="nlmc_pt_swap_philox: ladder_len > 4096"):
            eng.pt_swap_philox(0, SEED, 1)
        with pytest.raises(NotImplementedError, match="nlmc_pt_swap_philox: ladder_len > 4096"):
            eng.pt_swap_philox_host(0, SEED, 1, E, want_log=True)
        assert np.array_equal(eng.pt_slots(), np.arange(L))
        assert np.array_equal(eng.get_spins(), m0) and np.array_equal(eng.energy_tracked(), E)


def test_whole_ladders_split_over_two_contexts(product):
    """Four ladders of 130 temperatures, two per context (chain_base, n_chains_global): each context decides its own ladders from its
    own energies with the Philox keys of their GLOBAL ladder index, and equals the single context and the reference (ladder0)."""
    L, nl, n_pairs = 130, 4, 43
    rounds = (0, 1, 2)
    G = L * nl
    J, h, _, _ = setup(2)
    m0 = init_spins(G, N)
    csr = oracle.Csr(J)
    E = np.array([oracle.energy(csr, h, s) for s in m0])
    betas = betas_of(L)
    met = set()
    for rnd in rounds:
        for g in range(nl):
            met |= conditions(L, selection_trace(L, n_pairs, rnd, g))
    assert met >= wanted(L)

    def run(base, cnt):
        out = []
        with product.Engine(J, h, cnt, chain_base=base, n_chains_global=G) as eng:
            eng.set_spins(m0[base:base + cnt])
            eng.pt_init(betas)
            for rnd in rounds:
                pairs, acc = eng.pt_swap_philox(rnd, SEED, n_pairs)
                out.append((eng.pt_slots(), pairs, acc))
        return out

    whole = run(0, G)
    slots = (np.arange(G) % L).astype(np.int32)
    for k, rnd in enumerate(rounds):                           # the single context against the reference
        slots, pairs, acc = opt.swap_round(E, slots, betas, L, n_pairs, rnd, SEED)
        assert np.array_equal(whole[k][0], slots) and np.array_equal(whole[k][1], pairs) and np.array_equal(whole[k][2], acc)
    assert set(np.concatenate([w[2].ravel() for w in whole]).tolist()) == {0, 1}
    half = G // 2
    for base in (0, half):
        part = run(base, half)
        l0, sl = base // L, slice(base, base + half)
        own = (np.arange(G) % L).astype(np.int32)[sl]
        for k, rnd in enumerate(rounds):
            own, pairs, acc = opt.swap_round(E[sl], own, betas, L, n_pairs, rnd, SEED, ladder0=l0)
            assert np.array_equal(part[k][0][sl], own) and np.array_equal(part[k][0][sl], whole[k][0][sl])
            assert np.array_equal(part[k][1][l0:l0 + nl // 2], pairs) and np.array_equal(part[k][2][l0:l0 + nl // 2], acc)
            assert np.array_equal(part[k][1][l0:l0 + nl // 2], whole[k][1][l0:l0 + nl // 2])
