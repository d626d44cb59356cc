"""tests/exactlaw.py itself, the sequential spec against the exact Boltzmann law at reduced sample sizes, and mutant drivers.

Three parts.  (1) The helper: enumeration against brute force, the sampler's own chi-square, pi K = pi for the exact heat-bath sweep
matrix of several visiting orders and for a Houdayer exchange -- the maths the stationarity tests rest on.  (2) The spec alone stays
within the rule of exactlaw (family-wise ALPHA = 1e-4, Bonferroni): oracle.sweeps_philox over consecutive calls, rounds with
oracle.pt.swap_round, the drivers of distributed.py over the OracleEngine double.  (3) Mutants -- drivers written here around the
oracle, never product code -- fall outside it: a sweep counter that does not advance, a swap round index that does not advance, the
wrong sign of dBeta dE, a Houdayer exchange of half a component, sweeps at beta (1 + 2 delta*), one chain's random numbers used for
two chains.  Seeds are fixed: every result is reproducible."""
import itertools
import types

import numpy as np
import pytest

import exactlaw as xl
import oracle
from oracle import pt as opt

SEED = 0xE8AC7000 + (11 << 32)


# ---- drivers around the oracle ------------------------------------------------------------------------------------------------------
def sweep_calls(bi, m0, beta_of_chain, calls, T, use_f64=False, order="shared", advance=True, chain_id=lambda c: c, beta_scale=1.0,
                sweep0=0):
    """`calls` calls of T sweeps for every chain; advance=False is the mutant that hands every call the same sweep0."""
    csr = oracle.Csr(bi.J)
    out = np.array(m0, np.int8)
    for c in range(out.shape[0]):
        cb = np.tile(np.array(oracle.cb_pair(beta_of_chain[c] * beta_scale, 1.0, use_f64)), (T, 1))
        cid = chain_id(c)
        for k in range(calls):
            out[c] = oracle.sweeps_philox(csr, bi.h, out[c], cb, SEED, cid, order_group=(cid + 1 if order == "per_chain" else 0),
                                          sweep0=sweep0 + (k * T if advance else 0), use_f64=use_f64, want_M=False)[1]
    return out


def pt_rounds(bi, m0, betas, T, rounds, n_pairs, use_f64=False, advance_round=True, sign=1.0):
    """Rounds of T sweeps at the slot temperatures + oracle.pt.swap_round.  -> (spins, slots, pairs [rounds, nl, P, 2], acc)."""
    L, G = len(betas), m0.shape[0]
    slots = (np.arange(G) % L).astype(np.int32)
    spins = np.array(m0, np.int8)
    log_p, log_a = [], []
    for r in range(rounds):
        spins = sweep_calls(bi, spins, np.asarray(betas)[slots], 1, T, use_f64=use_f64, sweep0=r * T)
        E = bi.block_energy(bi.state_index(spins)).sum(axis=1)
        slots, p, a = opt.swap_round(E, slots, sign * np.asarray(betas), L, n_pairs, r if advance_round else 0, SEED)
        log_p.append(p)
        log_a.append(a)
    return spins, slots, np.array(log_p), np.array(log_a)


def judge_slots(route, bi, conf_by_slot, betas, extra=None):
    v = xl.Verdict(route)
    for i, b in enumerate(betas):
        v.add_slot(f"slot{i}", bi, conf_by_slot[i], b)
    if extra:
        extra(v)
    v.finish()
    if not extra:
        print(v.summary())
    return v


# ---- (1) the helper -----------------------------------------------------------------------------------------------------------------
def test_species_are_dyadic_frustrated_and_without_diagonal():
    for spc in (xl.K6, xl.RING2):
        assert spc.dyadic and xl.is_frustrated(spc) and not np.any(np.diag(spc.J))
        assert np.count_nonzero(np.triu(spc.J, 1)) == (15 if spc is xl.K6 else 8)
    assert not xl.GAUSS.dyadic and not np.any(np.diag(xl.GAUSS.J))


def test_enumeration_against_brute_force_on_three_spins():
    """A 3-spin block enumerated by hand (8 states), and the 6-spin law of the instance energy oracle.energy returns."""
    J = np.array([[0, 1, -0.5], [1, 0, 0.75], [-0.5, 0.75, 0]])
    h = np.array([0.25, -0.125, 0.5])
    beta, Z, w = 0.7, 0.0, {}
    for s in itertools.product((-1, 1), repeat=3):
        e = -(J[0, 1] * s[0] * s[1] + J[0, 2] * s[0] * s[2] + J[1, 2] * s[1] * s[2] + h @ np.array(s))
        w[s] = np.exp(-beta * e)
        Z += w[s]
    big = np.zeros((6, 6))
    big[:3, :3] = J
    spc = xl.Species("three", big, np.concatenate([h, np.zeros(3)]), True)
    law = xl.Law(spc, beta)
    for k in range(64):
        s = tuple(int(x) for x in xl.STATES[k, :3])
        assert abs(law.p[k] - w[s] / Z / 8) < 1e-15                   # the three free spins: a factor 1/8
    for spc in (xl.K6, xl.RING2, xl.GAUSS):
        bi = xl.BlockInstance(spc, 3, "strided")
        J6, h6 = bi.J, bi.h
        csr = oracle.Csr(J6)
        st = np.array([5, 40, 63])
        assert abs(oracle.energy(csr, h6, bi.spins_of(st)) - bi.block_energy(st).sum()) < 1e-12
        law = xl.Law(spc, 0.9)
        assert abs(law.p.sum() - 1) < 1e-15
        assert abs(law.mean - law.p @ spc.energy) < 1e-13 and abs(law.var - (law.p @ spc.energy ** 2 - law.mean ** 2)) < 1e-12


@pytest.mark.parametrize("layout", ["contiguous", "strided"])
def test_layouts_and_state_round_trip(layout):
    bi = xl.BlockInstance([xl.K6, xl.RING2], 7, layout)
    J, h, idx = xl.block_instance([xl.K6, xl.RING2], 7, layout)
    assert (J != bi.J).nnz == 0 and np.array_equal(h, bi.h) and np.array_equal(idx, bi.idx)
    assert sorted(idx.ravel()) == list(range(42))
    assert idx[3, 2] == (3 * 6 + 2 if layout == "contiguous" else 3 + 7 * 2)
    A = J.toarray()
    assert np.array_equal(A, A.T) and not np.any(np.diag(A))
    for b in range(7):
        assert np.array_equal(A[np.ix_(idx[b], idx[b])], bi.species[b % 2].J) and np.array_equal(h[idx[b]], bi.species[b % 2].h)
    outside = A.copy()
    for b in range(7):
        outside[np.ix_(idx[b], idx[b])] = 0
    assert not np.any(outside)                                           # blocks are disjoint
    st = np.random.default_rng(1).integers(0, 64, (5, 7))
    assert np.array_equal(bi.state_index(bi.spins_of(st)), st)


def test_the_samplers_own_chi_square_and_a_wrong_temperature():
    bi = xl.BlockInstance([xl.K6, xl.RING2], 40, "contiguous")
    m0 = xl.equilibrium_start(np.random.default_rng(5), bi, np.repeat([0.4, 1.2], 500))
    v = judge_slots("sampler", bi, [m0[:500], m0[500:]], [0.4, 1.2])
    assert v.ok() and v.wrong_rejected(), v.summary()
    assert max(v.pooled) <= 0.05


def sweep_matrix(spc, beta, order):
    """Exact 64 x 64 transition matrix of one heat-bath sweep of a block in the given visiting order."""
    K = np.eye(64)
    s = xl.STATES.astype(float)
    for i in order:
        x = s @ spc.J[i] + spc.h[i]
        up = 1.0 / (1.0 + np.exp(-2.0 * beta * x))                          # P(s_i' = +1 | the others)
        Ki = np.zeros((64, 64))
        k = np.arange(64)
        Ki[k, k | (1 << i)] += up
        Ki[k, k & ~(1 << i)] += 1.0 - up
        K = K @ Ki
    return K


def test_heat_bath_sweeps_leave_the_law_invariant():
    for spc, beta in ((xl.K6, 0.8), (xl.RING2, 1.2), (xl.GAUSS, 0.5)):
        pi = xl.Law(spc, beta).p
        for order in ([0, 1, 2, 3, 4, 5], [5, 3, 1, 0, 2, 4], [2, 2, 0, 5, 1, 4, 3]):
            K = sweep_matrix(spc, beta, order)
            assert np.max(np.abs(K.sum(axis=1) - 1)) < 1e-14
            assert np.max(np.abs(pi @ K - pi)) < 1e-14
        assert np.max(np.abs(xl.Law(spc, beta * 1.05).p @ sweep_matrix(spc, beta, range(6)) - xl.Law(spc, beta * 1.05).p)) > 1e-4


def components(A, diff):
    """Connected components of the sites where diff is set, in the graph of A (lists of sites, by smallest member)."""
    n, seen, out = len(diff), set(), []
    for a in range(n):
        if diff[a] and a not in seen:
            comp, todo = [], [a]
            seen.add(a)
            while todo:
                x = todo.pop()
                comp.append(x)
                for y in np.nonzero(A[x])[0]:
                    if diff[y] and y not in seen:
                        seen.add(y)
                        todo.append(y)
            out.append(sorted(comp))
    return out


def test_a_houdayer_exchange_leaves_the_product_law_invariant():
    """Two replicas at one beta on two disjoint 3-spin blocks with fields: pick one of the components of the sites where they differ
    uniformly and exchange it.  pi x pi is invariant (4096 joint states); exchanging half a component is not."""
    n, beta = 6, 0.9
    A = np.zeros((n, n))
    for (i, j), v in {(0, 1): 1.0, (1, 2): -0.75, (0, 2): 0.5, (3, 4): -1.0, (4, 5): 0.25}.items():
        A[i, j] = A[j, i] = v
    h = np.array([1, -2, 3, 0, -1, 2]) / 8
    S = np.array([[1 if (k >> i) & 1 else -1 for i in range(n)] for k in range(1 << n)], float)
    e = -(0.5 * np.einsum("ki,ij,kj->k", S, A, S) + S @ h)
    p = np.exp(-beta * e)
    p /= p.sum()
    joint = np.outer(p, p).ravel()
    for half in (False, True):
        out = np.zeros_like(joint)
        for a in range(1 << n):
            for b in range(1 << n):
                cl = components(A, [(a >> i) & 1 != (b >> i) & 1 for i in range(n)])
                if not cl:
                    out[a * 64 + b] += joint[a * 64 + b]
                    continue
                for c in cl:
                    c = c[:max(1, len(c) // 2)] if half else c
                    m = sum(1 << i for i in c)
                    a2, b2 = (a & ~m) | (b & m), (b & ~m) | (a & m)
                    out[a2 * 64 + b2] += joint[a * 64 + b] / len(cl)
        err = np.max(np.abs(out - joint))
        assert (err > 1e-4) if half else (err < 1e-14)


def test_acceptance_expectation_against_direct_enumeration():
    """Two chains of two blocks each (4096 joint block states per chain pair side): E[min(1, exp(dBeta dE))] summed state by state."""
    bi = xl.BlockInstance([xl.K6, xl.RING2], 2, "contiguous")
    ba, bb = 0.5, 0.9
    pa = np.outer(xl.Law(xl.K6, ba).p, xl.Law(xl.RING2, ba).p).ravel()
    pb = np.outer(xl.Law(xl.K6, bb).p, xl.Law(xl.RING2, bb).p).ravel()
    E = (xl.K6.energy[:, None] + xl.RING2.energy[None, :]).ravel()
    for sign in (1.0, -1.0):
        direct = np.sum(np.outer(pa, pb) * np.minimum(1.0, np.exp(sign * (bb - ba) * (E[None, :] - E[:, None]))))
        got = xl.acceptance(xl.chain_energy_pmf(bi, ba), xl.chain_energy_pmf(bi, bb), ba, bb, sign=sign)
        assert abs(got - direct) < 1e-12
    lo, pmf = xl.chain_energy_pmf(bi, ba)
    assert abs(pmf.sum() - 1) < 1e-14 and abs((lo + np.arange(len(pmf))) @ pmf / xl.UNIT - (xl.Law(xl.K6, ba).mean + xl.Law(xl.RING2, ba).mean)) < 1e-12


# ---- (2) the spec passes, (3) mutants reject: sweeps -------------------------------------------------------------------------------
COPIES, CHAINS, BETAS = 44, 300, (0.4, 1.2)


def sweep_case(layout, seed):
    bi = xl.BlockInstance([xl.K6, xl.RING2], COPIES, layout)
    beta = np.repeat(BETAS, CHAINS)
    return bi, beta, xl.equilibrium_start(np.random.default_rng(seed), bi, beta)


@pytest.mark.parametrize("use_f64,order,layout", [(False, "shared", "contiguous"), (True, "per_chain", "strided"),
                                                  (True, "shared", "contiguous"), (False, "per_chain", "strided")])
def test_spec_sweeps_over_consecutive_calls(use_f64, order, layout):
    bi, beta, m0 = sweep_case(layout, 21)
    out = sweep_calls(bi, m0, beta, 4, 2, use_f64=use_f64, order=order)
    assert not np.array_equal(out, m0)
    v = judge_slots(f"spec sweeps f64={use_f64} {order} {layout}", bi, [out[:CHAINS], out[CHAINS:]], BETAS)
    assert v.ok() and v.wrong_rejected(), v.summary()


def test_mutant_sweep_counter_not_advanced():
    bi, beta, m0 = sweep_case("contiguous", 22)
    out = sweep_calls(bi, m0, beta, 8, 1, advance=False)
    v = judge_slots("mutant sweep0 fixed", bi, [out[:CHAINS], out[CHAINS:]], BETAS)
    assert not v.ok(), v.summary()


def test_mutant_sweeps_at_a_wrong_temperature():
    """Sweeps at beta (1 + 2 delta*), delta* that of this sample size: statistic (ii) sees it once the chains have relaxed."""
    bi, beta, m0 = sweep_case("strided", 23)
    ok = judge_slots("wrong temperature: the sample size", bi, [m0[:CHAINS], m0[CHAINS:]], BETAS)
    out = sweep_calls(bi, m0, beta, 1, 12, beta_scale=1 + 2 * max(ok.delta))
    v = judge_slots("mutant beta(1+2delta*)", bi, [out[:CHAINS], out[CHAINS:]], BETAS)
    assert ok.ok() and not v.ok(), v.summary()


def test_mutant_one_chains_random_numbers_used_for_two_chains():
    """Chains 2j and 2j + 1 run with the chain id 2j.  Each chain alone still has the exact law -- (i)-(iii) pass -- but the two are
    no longer independent: the overlap histogram (iv) rejects, and passes for the true spec."""
    bi, beta, m0 = sweep_case("contiguous", 24)
    for mutant in (False, True):
        out = sweep_calls(bi, m0, beta, 3, 2, chain_id=(lambda c: c - c % 2) if mutant else (lambda c: c))
        v = xl.Verdict(f"{'mutant shared chain id' if mutant else 'spec'} overlaps")
        for i, b in enumerate(BETAS):
            rows = out[i * CHAINS:(i + 1) * CHAINS]
            if not mutant:
                v.add_slot(f"slot{i}", bi, rows, b)
            for k, spc in enumerate(bi.species):
                v.add(f"slot{i} overlap {spc.name}", xl.chi2_overlap(rows[0::2], rows[1::2], bi, k, xl.Law(spc, b)))
        v.finish()
        print(v.summary())
        assert v.ok() != mutant, v.summary()


# ---- rounds with replica exchange -------------------------------------------------------------------------------------------------
PT_BETAS, PT_COPIES, PT_LADDERS = (0.5, 0.62, 0.74, 0.86), 20, 400


def pt_case(seed, betas=PT_BETAS, copies=PT_COPIES, ladders=PT_LADDERS):
    bi = xl.BlockInstance([xl.K6, xl.RING2], copies, "strided")
    L = len(betas)
    return bi, L, xl.equilibrium_start(np.random.default_rng(seed), bi, np.tile(betas, ladders))


def judge_pt(route, bi, L, spins, slots, pairs, acc, betas=PT_BETAS):
    v = judge_slots(route, bi, xl.by_slot(spins, slots, L), betas, extra=lambda v: v.add_acceptance(bi, betas, pairs, acc))
    print(v.summary())
    return v


@pytest.mark.parametrize("use_f64", [False, True])
def test_spec_rounds_with_swaps(use_f64):
    bi, L, m0 = pt_case(31)
    spins, slots, pairs, acc = pt_rounds(bi, m0, PT_BETAS, 2, 6, 1, use_f64=use_f64)
    assert acc.sum() > 0 and not np.array_equal(slots, np.arange(len(slots)) % L)
    v = judge_pt(f"spec rounds f64={use_f64}", bi, L, spins, slots, pairs, acc)
    assert v.ok() and v.wrong_rejected(), v.summary()


def test_mutant_wrong_sign_of_the_swap_test():
    bi, L, m0 = pt_case(32)
    v = judge_pt("mutant swap sign", bi, L, *pt_rounds(bi, m0, PT_BETAS, 2, 6, 1, sign=-1.0))
    assert not v.ok(), v.summary()


def test_mutant_swap_round_index_not_advanced():
    """Every round tries the same pair with the same uniform u: a ladder swaps back and forth while u < min(r, 1 / r) and otherwise
    settles in its more probable arrangement.  Where nothing moves between the rounds, the less probable arrangement is held with
    probability m^2 / (1 + m) instead of m / (1 + m) after an even number of rounds (m = min(r, 1 / r)), and later attempts are
    accepted less often than the exact expectation: statistic (v) sees it.  Sweeps between the rounds wash that memory out, so the
    mutant runs where one sweep moves a block little (cold two-slot ladders, eight rounds of one sweep)."""
    betas = (2.5, 4.0)
    bi, L, m0 = pt_case(33, betas, 6, 2000)
    v = judge_pt("mutant swap round fixed", bi, L, *pt_rounds(bi, m0, betas, 1, 8, 1, advance_round=False), betas=betas)
    assert not v.ok(), v.summary()


# ---- the host drivers over the oracle double ---------------------------------------------------------------------------------------
def as_instance(bi):
    """What the engine double reads of a product Instance."""
    csr = oracle.Csr(bi.J)
    return types.SimpleNamespace(n=csr.n, indptr=csr.indptr, indices=csr.indices, data=csr.data, h=np.ascontiguousarray(bi.h, dtype=np.float64))


@pytest.mark.parametrize("contexts", [1, 2])
def test_spec_local_tempering_driver(contexts):
    """distributed.LocalTempering (plan + run_rounds + round) over the double, as test_local_run_rounds_cpu.py drives it: the
    driver's own sweep and round counters."""
    from conftest import load_product
    from fake_engine import OracleEngine
    P = load_product()

    class Logging(OracleEngine):
        def pt_swap_philox(self, *a, **k):
            out = super().pt_swap_philox(*a, **k)
            self.__dict__.setdefault("log", []).append(out)
            return out

    bi, L, m0 = pt_case(41)
    lt = P.distributed.LocalTempering(as_instance(bi), np.array(PT_BETAS), m0.shape[0], SEED, 1, [0] * contexts,
                                      engine_factory=lambda i, n, b, g: Logging(i, n, b, g))
    lt.set_spins(m0)
    lt.plan(6 * 2, 6, chunk_rounds=4)
    lt.run_rounds(4, 2)
    lt.round(2)
    lt.run_rounds(1, 2)
    assert lt.rounds_done == 6 and lt.sweeps_done == 12
    spins, slots = lt.gather_spins(), lt.slots()
    pairs = np.concatenate([np.stack([p for p, _ in e.log]) for e in lt.engs], axis=1)
    acc = np.concatenate([np.stack([a for _, a in e.log]) for e in lt.engs], axis=1)
    assert pairs.shape == (6, PT_LADDERS, 1, 2) and acc.sum() > 0
    v = judge_pt(f"spec LocalTempering contexts={contexts}", bi, L, spins, slots, pairs, acc)
    assert v.ok() and v.wrong_rejected(), v.summary()


APT_K = 300


@pytest.mark.parametrize("shards", [1, 2])
def test_spec_apt_protocol(shards):
    """distributed.SlotShardedAPT over the double: sweeps, Houdayer moves between the sub-replicas of a slot, swaps -- with one
    block of slots and with two (accepted boundary pairs move configurations).  (i)-(iii) by slot, and the overlaps (iv) between
    the two halves of a slot's sub-replicas."""
    from conftest import load_product
    from fake_engine import OracleEngine
    P = load_product()
    bi = xl.BlockInstance([xl.K6, xl.RING2], PT_COPIES, "contiguous")
    R = len(PT_BETAS)
    start = xl.equilibrium_start(np.random.default_rng(51), bi, np.tile(PT_BETAS, APT_K)).reshape(APT_K, R, bi.n)
    apt = P.distributed.SlotShardedAPT(lambda i, n, b, g, dev=None: OracleEngine(i, n, b, g), as_instance(bi), np.array(PT_BETAS), APT_K,
                                       SEED, 1, device="cpu", device_ids=None if shards == 1 else [0] * shards)
    apt.set_spins_by_slot(start)
    moved, accepted, boundary = 0, 0, 0
    for _ in range(5):
        (pairs, acc), info = apt.round(2, want_log=True, want_info=True)
        info = np.concatenate(info)
        assert info[:, 1].max() <= bi.n // 2                        # no global flip: not an invariant move when h != 0
        moved += int((info[:, 1] > 0).sum())
        accepted += int(acc.sum())
        boundary += int((acc.astype(bool) & (pairs[..., 1] % (R // shards) == 0)).sum())
    cfg, _ = apt.gather_by_slot()
    apt.check()
    apt.close()
    assert moved > 0 and accepted > 0 and (shards == 1 or boundary > 0)
    v = xl.Verdict(f"spec APT shards={shards}")
    for r, b in enumerate(PT_BETAS):
        v.add_slot(f"slot{r}", bi, cfg[:, r], b)
        for k, spc in enumerate(bi.species):
            v.add(f"slot{r} overlap {spc.name}", xl.chi2_overlap(cfg[:APT_K // 2, r], cfg[APT_K // 2:, r], bi, k, xl.Law(spc, b)))
    v.finish()
    print(v.summary())
    assert v.ok() and v.wrong_rejected(), v.summary()


def houdayer_rounds(bi, spins, rounds, rng, half):
    """Random pairs of chains; one of the components of the sites where a pair differs, picked uniformly, is exchanged -- or, the
    mutant, a random half of it."""
    csr = oracle.Csr(bi.J)
    s = np.array(spins, np.int8)
    for _ in range(rounds):
        order = rng.permutation(len(s))
        for a, b in zip(order[0::2], order[1::2]):
            cl = oracle.clusters(csr, s[a], s[b])
            if not cl:
                continue
            c = cl[rng.integers(len(cl))]
            if half:
                c = c[rng.random(len(c)) < 0.5]
            s[a, c], s[b, c] = s[b, c].copy(), s[a, c].copy()
    return s


@pytest.mark.parametrize("half", [False, True])
def test_houdayer_exchange_and_its_mutant(half):
    """Whole components keep the law (that is oracle.clusters and the move of the engine double); half components do not."""
    bi = xl.BlockInstance([xl.K6, xl.RING2], 6, "contiguous")
    beta, R = 1.2, 1500
    m0 = xl.equilibrium_start(np.random.default_rng(61), bi, np.full(R, beta))
    out = houdayer_rounds(bi, m0, 12, np.random.default_rng(62), half)
    assert not np.array_equal(out, m0)
    v = judge_slots(f"houdayer half={half}", bi, [out], [beta])
    assert v.ok() != half, v.summary()
