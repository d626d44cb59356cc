"""distributed.ShardedTempering.run_rounds on the CPU double (one process, no collective): the counterpart of
test_local_run_rounds_cpu.py for the driver bench.py times.  Chunks handed to the engine's batched call -- pt_rounds_deferred, or
pt_rounds_fused by name with persistent=True -- must leave what round() called once per round leaves, and everything that does not
qualify must fall back to exactly that."""
import numpy as np
import pytest

from conftest import load_product
from fake_engine import OracleEngine
from helpers import make_instance, init_spins
from test_local_run_rounds_cpu import BatchingEngine

N, SEED, S, ROUNDS, PAIRS = 96, 0xB0B0CAFE, 4, 7, 1
LQ, NLQ = 4, 4
G = LQ * NLQ


class NamedEngine(BatchingEngine):
    """BatchingEngine with a pt_rounds_fused that counts the calls by name and forwards them."""

    def __init__(self, *a):
        super().__init__(*a)
        self.by_name = 0

    def pt_rounds_fused(self, *a, **k):
        self.by_name += 1
        return self.pt_rounds_deferred(*a, **k)


class WaveRoundsEngine(NamedEngine):
    """A context whose sweeps go one chain per wave, with wave rounds on: no fused window is needed for a chunk to be batched."""
    wave_rounds = True

    def waves_take(self, rows=None, precision="f32"):
        return True


def drive(P, inst, betas, m0, cls, n_sweeps=S, batched=True, chunk=None, persistent=False, refuse_from=None, run_sweeps=None):
    made = []

    def mk(i, n, b, g):
        made.append(cls(i, n, b, g))
        made[0].refuse_from = refuse_from
        return made[0]
    st = P.distributed.ShardedTempering(mk, inst, betas, G, SEED, PAIRS)
    st.set_spins(m0)
    st.plan(ROUNDS * n_sweeps, ROUNDS, chunk_rounds=chunk)
    if batched:
        st.run_rounds(ROUNDS, n_sweeps if run_sweeps is None else run_sweeps, persistent=persistent)
    else:
        for _ in range(ROUNDS):
            st.round(n_sweeps)
    assert st.rounds_done == ROUNDS and st.sweeps_done == ROUNDS * (n_sweeps if run_sweeps is None else run_sweeps)
    return st.gather_spins(), st.eng.pt_slots().copy(), st


@pytest.fixture(scope="module")
def case():
    P = load_product()
    J, h = make_instance(N, seed=3, with_h=True, gaussian=True)
    inst = P.Instance(J, h)
    betas = np.geomspace(0.3, 2.5, LQ)
    m0 = init_spins(G, N)
    refs = {}
    for n_sweeps in (S, 1, S + 1):
        ref = drive(P, inst, betas, m0, OracleEngine, n_sweeps=n_sweeps, batched=False)[:2]
        for x in ref:
            x.setflags(write=False)
        refs[n_sweeps] = ref
    assert not np.array_equal(refs[S][1], np.arange(G) % LQ)               # swaps happened
    return P, inst, betas, m0, refs


def rounds_counters(st):
    return getattr(st, "deferred_rounds", 0), getattr(st, "persistent_rounds", 0)


@pytest.mark.parametrize("persistent", [False, True])
@pytest.mark.parametrize("chunk, refuse_from, batched, asked, single, counter", [
    (None, None, [(0, 7)], 1, 0, 7),
    (None, 0, [], 1, 7, 0),
    (3, None, [(0, 3), (3, 3), (6, 1)], 3, 0, 7),
    (3, 1, [(0, 3)], 2, 4, 3),
])
def test_run_rounds_equals_round_by_round(case, persistent, chunk, refuse_from, batched, asked, single, counter):
    """One chunk for all rounds or chunks of 3, accepted or refused at the first / second call: a refused engine runs those rounds
    and all later ones one by one and is not asked again; the same bits.  persistent: the calls go by name and are counted apart."""
    P, inst, betas, m0, refs = case
    spins, slots, st = drive(P, inst, betas, m0, NamedEngine, chunk=chunk, persistent=persistent, refuse_from=refuse_from)
    assert np.array_equal(spins, refs[S][0]) and np.array_equal(slots, refs[S][1])
    e = st.eng
    assert e.batched == batched and e.asked == asked and e.single_sweeps == single
    assert e.by_name == (asked if persistent else 0)
    assert rounds_counters(st) == ((0, counter) if persistent else (counter, 0))
    if refuse_from is not None:
        assert e.rounds_fused_refusal == "refused by the test"


@pytest.mark.parametrize("persistent", [False, True])
def test_other_round_lengths_batch_nothing(case, persistent):
    P, inst, betas, m0, refs = case
    spins, slots, st = drive(P, inst, betas, m0, NamedEngine, persistent=persistent, run_sweeps=S + 1)
    assert np.array_equal(spins, refs[S + 1][0]) and np.array_equal(slots, refs[S + 1][1])
    assert st.eng.asked == 0 and st.eng.single_sweeps == ROUNDS and rounds_counters(st) == (0, 0)


def test_no_deferred_switch_batches_nothing(case, monkeypatch):
    P, inst, betas, m0, refs = case
    monkeypatch.setenv("NLMC_NO_DEFERRED", "1")
    spins, slots, st = drive(P, inst, betas, m0, NamedEngine)
    assert np.array_equal(spins, refs[S][0]) and np.array_equal(slots, refs[S][1])
    assert st.eng.asked == 0 and st.eng.single_sweeps == ROUNDS and rounds_counters(st) == (0, 0)


def test_the_plain_double_falls_back(case):
    """An engine without pt_rounds_fused / pt_rounds_deferred: round by round."""
    P, inst, betas, m0, refs = case
    spins, slots, st = drive(P, inst, betas, m0, OracleEngine)
    assert np.array_equal(spins, refs[S][0]) and np.array_equal(slots, refs[S][1])
    assert rounds_counters(st) == (0, 0)


def test_persistent_switch_in_the_environment(case, monkeypatch):
    """NLMC_PERSISTENT is the default of `persistent`."""
    P, inst, betas, m0, refs = case
    monkeypatch.setenv("NLMC_PERSISTENT", "1")
    spins, slots, st = drive(P, inst, betas, m0, NamedEngine, persistent=None)
    assert np.array_equal(spins, refs[S][0]) and np.array_equal(slots, refs[S][1])
    assert st.eng.by_name == 1 and rounds_counters(st) == (0, ROUNDS)


def test_wave_rounds_batch_whatever_the_round_length(case):
    """Sweeps one chain per wave with wave rounds on, rounds of ONE sweep (no fused window exists): every chunk goes to the batched
    call, as under LocalTempering -- the rule does not look at fused_window(S) on this route.  By name nothing is asked:
    pt_rounds_fused takes fused windows only."""
    P, inst, betas, m0, refs = case
    spins, slots, st = drive(P, inst, betas, m0, WaveRoundsEngine, n_sweeps=1)
    assert np.array_equal(spins, refs[1][0]) and np.array_equal(slots, refs[1][1])
    assert st.eng.batched == [(0, 7)] and st.eng.single_sweeps == 0 and rounds_counters(st) == (ROUNDS, 0)
    spins, slots, st = drive(P, inst, betas, m0, WaveRoundsEngine, n_sweeps=1, persistent=True)
    assert np.array_equal(spins, refs[1][0]) and np.array_equal(slots, refs[1][1])
    assert st.eng.asked == 0 and st.eng.by_name == 0 and st.eng.single_sweeps == ROUNDS and rounds_counters(st) == (0, 0)
