"""distributed.LocalTempering.run_rounds on the CPU double: plain rounds handed to the engine a planned chunk at a time
(Engine.pt_rounds_deferred) must leave what round() called once per round leaves -- spins, slots, counters -- and everything that
does not qualify must fall back to exactly that."""
import numpy as np
import pytest

from conftest import load_product
from fake_engine import OracleEngine
from helpers import make_instance, init_spins

N, SEED, S, ROUNDS, PAIRS = 96, 0xB0B0CAFE, 4, 7, 1
LQ, NLQ = 4, 4
G = LQ * NLQ


class BatchingEngine(OracleEngine):
    """The double with a pt_rounds_deferred of its own: it runs the k rounds itself (a sweep call and a swap call each), or refuses
    (`refuse_from`: from that call on) like a context that does not qualify."""
    refuse_from = None

    def __init__(self, *a):
        super().__init__(*a)
        self.batched, self.asked, self.single_sweeps = [], 0, 0

    def sweep_philox(self, *a, **k):
        if not getattr(self, "_in_batch", False):
            self.single_sweeps += 1
        return super().sweep_philox(*a, **k)

    def pt_rounds_deferred(self, n_rounds, sweeps_per_round, seed, sweep0, round0, n_pairs, precision="f32"):
        self.asked += 1
        if self.refuse_from is not None and self.asked > self.refuse_from:
            self.rounds_fused_refusal = "refused by the test"
            return False
        self._in_batch = True
        for r in range(n_rounds):
            self.sweep_philox(sweeps_per_round, seed, sweep0=sweep0 + r * sweeps_per_round, precision=precision)
            self.pt_swap_philox(round0 + r, seed, n_pairs)
        self._in_batch = False
        self.batched.append((int(round0), int(n_rounds)))
        return True

    def last_rounds_route(self):
        return "launch per round" if self.batched else None


@pytest.fixture(scope="module")
def case():
    P = load_product()
    J, h = make_instance(N, seed=3, with_h=True, gaussian=True)
    inst = P.Instance(J, h)
    betas = np.geomspace(0.3, 2.5, LQ)
    m0 = init_spins(G, N)
    ref = drive(P, inst, betas, m0, 1, OracleEngine, batched=False)
    assert not np.array_equal(ref[1], np.arange(G) % LQ)               # swaps happened
    for x in ref[:2]:
        x.setflags(write=False)
    return P, inst, betas, m0, ref


def drive(P, inst, betas, m0, k, cls, batched=True, chunk=None, prepare=None, pieces=None):
    lt = P.distributed.LocalTempering(inst, betas, G, SEED, PAIRS, [0] * k, engine_factory=lambda i, n, b, g: cls(i, n, b, g))
    if prepare:
        prepare(lt)
    lt.set_spins(m0)
    lt.plan(ROUNDS * S, ROUNDS, chunk_rounds=chunk)
    if batched:
        for n in (pieces or [ROUNDS]):
            lt.run_rounds(n, S)
    else:
        for _ in range(ROUNDS):
            lt.round(S)
    out = lt.gather_spins(), lt.slots().copy(), lt
    assert lt.sweeps_done == ROUNDS * S and lt.rounds_done == ROUNDS
    return out


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("chunk", [None, 3])
def test_run_rounds_equals_round_by_round(case, k, chunk):
    """Contexts of whole ladders; one chunk for all rounds, or chunks of 3 (7 rounds = 3 + 3 + 1 batched calls per context)."""
    P, inst, betas, m0, ref = case
    spins, slots, lt = drive(P, inst, betas, m0, k, BatchingEngine, chunk=chunk)
    assert np.array_equal(spins, ref[0]) and np.array_equal(slots, ref[1])
    want = [(0, 7)] if chunk is None else [(0, 3), (3, 3), (6, 1)]
    for e in lt.engs:
        assert e.batched == want and e.single_sweeps == 0
    assert lt.deferred_rounds == ROUNDS and lt.deferred_calls == len(want) * k
    assert lt.rounds_routes == ["launch per round"] * k


def test_calls_in_pieces_keep_the_counters(case):
    """run_rounds(3) + run_rounds(4) over chunks of 5: batched calls of 3, 2 and 2 rounds."""
    P, inst, betas, m0, ref = case
    spins, slots, lt = drive(P, inst, betas, m0, 2, BatchingEngine, chunk=5, pieces=[3, 4])
    assert np.array_equal(spins, ref[0]) and np.array_equal(slots, ref[1])
    assert all(e.batched == [(0, 3), (3, 2), (5, 2)] for e in lt.engs)
    assert lt.deferred_rounds == ROUNDS


@pytest.mark.parametrize("refuse_from", [0, 1])
def test_a_refusal_falls_back_and_is_not_repeated(case, refuse_from):
    """Context 1 of 2 refuses its first / its second batched call (chunks of 3): it runs those rounds and all later ones one by
    one and is not asked again, context 0 goes on batching; the same bits."""
    P, inst, betas, m0, ref = case

    def prepare(lt):
        lt.engs[1].refuse_from = refuse_from
    spins, slots, lt = drive(P, inst, betas, m0, 2, BatchingEngine, chunk=3, prepare=prepare)
    assert np.array_equal(spins, ref[0]) and np.array_equal(slots, ref[1])
    a, b = lt.engs
    assert a.batched == [(0, 3), (3, 3), (6, 1)] and a.single_sweeps == 0
    assert b.asked == refuse_from + 1 and b.batched == [(0, 3)][:refuse_from] and b.single_sweeps == ROUNDS - 3 * refuse_from
    assert lt.deferred_rounds == 3 * refuse_from


def test_every_context_refusing_ends_in_round(case):
    P, inst, betas, m0, ref = case

    def prepare(lt):
        for e in lt.engs:
            e.refuse_from = 0
    spins, slots, lt = drive(P, inst, betas, m0, 2, BatchingEngine, prepare=prepare)
    assert np.array_equal(spins, ref[0]) and np.array_equal(slots, ref[1])
    assert all(e.asked == 1 and not e.batched and e.single_sweeps == ROUNDS for e in lt.engs)
    assert lt.deferred_rounds == 0 and lt.rounds_routes == [None, None]


def test_the_plain_double_falls_back(case):
    """An engine without pt_rounds_deferred: round by round."""
    P, inst, betas, m0, ref = case
    spins, slots, lt = drive(P, inst, betas, m0, 2, OracleEngine)
    assert np.array_equal(spins, ref[0]) and np.array_equal(slots, ref[1])
    assert lt.deferred_rounds == 0 and lt.deferred_calls == 0


def test_cut_ladders_fall_back(case):
    """8 contexts over 4 ladders of 4: every ladder is cut in two, the energies pass through the host every round."""
    P, inst, betas, m0, ref = case
    spins, slots, lt = drive(P, inst, betas, m0, 8, BatchingEngine)
    assert not lt.whole_ladders
    assert np.array_equal(spins, ref[0]) and np.array_equal(slots, ref[1])
    assert all(e.asked == 0 and e.single_sweeps == ROUNDS for e in lt.engs) and lt.deferred_rounds == 0


def test_no_deferred_switch_and_other_round_lengths(case, monkeypatch):
    """NLMC_NO_DEFERRED: nothing is batched.  Rounds of another length than the planned one: nothing is batched either."""
    P, inst, betas, m0, ref = case
    monkeypatch.setenv("NLMC_NO_DEFERRED", "1")
    spins, slots, lt = drive(P, inst, betas, m0, 2, BatchingEngine)
    assert np.array_equal(spins, ref[0]) and np.array_equal(slots, ref[1])
    assert all(e.asked == 0 for e in lt.engs)
    monkeypatch.delenv("NLMC_NO_DEFERRED")
    lt = P.distributed.LocalTempering(inst, betas, G, SEED, PAIRS, [0], engine_factory=lambda i, n, b, g: BatchingEngine(i, n, b, g))
    lt.set_spins(m0)
    lt.plan(ROUNDS * S, ROUNDS)
    lt.run_rounds(2, S + 1)
    assert lt.engs[0].asked == 0 and lt.rounds_done == 2 and lt.sweeps_done == 2 * (S + 1)
