"""Tempering rounds of short chains in one launch (csrc/nlmc_lane_rounds.h: k_rounds_lanes, a chain per lane and a ladder per wave).

Every case starts three runs from one fixed state and compares them bit for bit -- spins, tracked energies, slots and the device-side
swap log: (a) the rounds in k_rounds_lanes launches, (b) the same engine with the lane sweeps forced, round by round (sweep_philox +
pt_swap_philox), (c) the lane mode off, round by round, with the pair selections made inside the swap kernel.  Run (a) is repeated
without a device log.  Named ladders are also driven by the oracle double.  Shapes: the smallest that reach every path of the kernel
-- idle lanes, a last wave with fewer ladders, full waves, one ladder per wave, two-lane ladders, the diagonal branch, a chain shorter
than a Philox block, a chain base, permuted slots, cut calls, several launches per call."""
import contextlib
import io

import numpy as np
import pytest

from fake_engine import OracleEngine
from helpers import make_instance, init_spins
from test_gpu_lanes import dense_instance, wishart, nmc_flags

pytestmark = pytest.mark.gpu
SEED = 0xC3C30000 + (11 << 32)          # high bits set
FUSED_PLAN_MESSAGE = "no fused-window plan of one window per round covers these sweeps"


def ladder_betas(L):
    return np.geomspace(0.3, 1.5, L)


def n_pairs_of(L):
    return max(1, L // 3)                # greedy selection never runs out: a pick removes at most 3 of the L - 1 pairs


def state(eng):
    p, a = eng.pt_log_read()
    return {"spins": eng.get_spins(), "energy": eng.energy_tracked(), "slots": eng.pt_slots(), "pairs": p, "acc": a}


def assert_same(a, b, what, log=True):
    for k in ("spins", "energy", "slots") + (("pairs", "acc") if log else ()):
        assert np.array_equal(a[k], b[k]), (what, k)


def three_runs(product, J, h, L, ladders, T, rounds, precision, chain_base=0, G=None, slots0=None, cuts=None, entry="pt_rounds_lanes",
               mode_a="off", oracle_ladders=(0,), seed=SEED):
    """-> (a), the engine's instance.  Asserts (a) == (a without a log) == (b) == (c) and the oracle on `oracle_ladders`."""
    N, GL = J.shape[0], L * ladders
    G = GL if G is None else G
    betas, pairs = ladder_betas(L), n_pairs_of(L)
    m0 = init_spins(GL, N)
    start = (np.arange(G) % L).astype(np.int32) if slots0 is None else np.asarray(slots0, np.int32)
    cuts = cuts or [rounds]
    with product.Engine(J, h, GL, chain_base=chain_base, n_chains_global=G) as eng:
        eng.pt_init(betas)

        def begin(mode, log=True, plan=True):
            eng.set_lane_sweeps(mode)
            eng.set_spins(m0)
            eng.pt_set_slots(start)
            eng.pt_plan(0, rounds if plan else 0, seed, pairs)
            eng.pt_log_begin(0, rounds if log else 0, pairs)

        def in_launch(log):
            begin(mode_a, log=log)
            at = 0
            for k in cuts:
                assert getattr(eng, entry)(k, T, seed, at * T, at, pairs, precision=precision), getattr(eng, "rounds_fused_refusal", "")
                assert eng.last_rounds_route() == "lanes" and eng.last_sweep_route() == "lanes"
                assert eng.last_schedule_stats() == {"orders": k * T, "levels": 0} and not eng._last_fused()
                at += k
            eng.pt_check()
            if not log:
                return {"spins": eng.get_spins(), "energy": eng.energy_tracked(), "slots": eng.pt_slots()}
            return state(eng)

        def by_round(mode, route, plan):
            begin(mode, plan=plan)
            for r in range(rounds):
                eng.sweep_philox(T, seed, sweep0=r * T, beta=None, precision=precision)
                assert eng.last_sweep_route() == route
                eng.pt_swap_philox(r, seed, pairs, want_log=False)
            eng.pt_check()
            return state(eng)

        a = in_launch(True)
        assert_same(a, in_launch(False), "without a device log", log=False)
        b = by_round("force", "lanes", True)
        assert_same(a, b, "lane sweeps round by round")
        c = by_round("off", "stepwise", False)
        assert_same(a, c, "lane mode off")
        inst = eng.inst
    # no case is vacuous: swaps were accepted, the slots and the spins moved, every selected pair was logged
    assert a["acc"].mean() > 0 and not np.array_equal(a["slots"], start) and not np.array_equal(a["spins"], m0)
    lo, hi = chain_base // L, chain_base // L + ladders
    assert (a["pairs"][:, lo:hi] >= 0).all() and (a["pairs"][:, lo:hi, :, 1] == a["pairs"][:, lo:hi, :, 0] + 1).all()
    assert np.array_equal(a["slots"][:chain_base], start[:chain_base]) and np.array_equal(a["slots"][chain_base + GL:], start[chain_base + GL:])
    for g in oracle_ladders:
        o = OracleEngine(inst, L, chain_base + g * L, G)
        o.pt_init(betas)
        o.pt_set_slots(start)
        o.set_spins(m0[g * L:(g + 1) * L])
        for r in range(rounds):
            o.sweep_philox(T, seed, sweep0=r * T, precision=precision)
            o.pt_swap_philox(r, seed, pairs)
        rows = slice(g * L, (g + 1) * L)
        assert np.array_equal(a["spins"][rows], o.get_spins()), f"oracle: spins of ladder {g}"
        assert np.array_equal(a["slots"][chain_base + g * L:chain_base + (g + 1) * L], o.pt_slots()[chain_base + g * L:chain_base + (g + 1) * L]), g
    return a


@pytest.fixture(scope="module")
def five():
    return make_instance(37, seed=9, with_h=True, gaussian=True)


@pytest.mark.parametrize("precision,rng", [("f32", None), ("f64", None), ("f32", "0"), ("f32", "1"), ("f64", "0"), ("f64", "1")],
                         ids=["f32", "f64", "f32-rng0", "f32-rng1", "f64-rng0", "f64-rng1"])
def test_twelve_ladders_a_wave_with_idle_lanes_and_a_short_last_wave(product, five, precision, rng, monkeypatch):
    """L = 5: 12 ladders per wave leave 4 idle lanes; 27 ladders make the last wave hold 3.  rng: NLMC_LANE_RNG (read when the engine is
    created) -- the Philox call per update, or the table per sweep; None leaves the default."""
    if rng is not None:
        monkeypatch.setenv("NLMC_LANE_RNG", rng)
    three_runs(product, *five, 5, 27, 3, 6, precision, oracle_ladders=(0, 11, 12, 26))


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_full_waves_of_one_ladder_on_real_couplings(product, precision):
    """L = 64 on the golden Wishart N = 10 instance as run() normalises it: every lane of a wave is one rung."""
    J, h, _, _ = wishart(product)
    three_runs(product, J, h, 64, 2, 3, 5, precision, oracle_ladders=(1,))


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_one_ladder_per_wave_with_idle_lanes_and_a_diagonal(product, precision):
    """L = 33: one ladder and 31 idle lanes per wave; the instance has diagonal entries (left out of the energy deltas)."""
    J, h = dense_instance(12, seed=4, diag=True)
    three_runs(product, J, h, 33, 3, 3, 5, precision, oracle_ladders=(2,))


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_two_lane_ladders_of_a_chain_shorter_than_a_philox_block(product, precision):
    """L = 2, n = 2: 32 ladders per wave, 70 ladders, one pair."""
    J, h = dense_instance(2, seed=6)
    three_runs(product, J, h, 2, 70, 2, 8, precision, oracle_ladders=(0, 31, 32, 69))


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_chain_base_keys_and_maps_are_global(product, five, precision):
    """A context that owns ladders 2 .. 28 of 29: Philox keys by global ladder and chain, chain_of_slot rows by global ladder."""
    L, ladders = 5, 27
    three_runs(product, *five, L, ladders, 3, 6, precision, chain_base=2 * L, G=L * ladders + 2 * L, oracle_ladders=(0, 26))


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_permuted_start(product, five, precision):
    L, ladders = 5, 27
    r = np.random.default_rng(17)
    slots0 = np.concatenate([r.permutation(L) for _ in range(ladders)])
    assert not np.array_equal(slots0, np.arange(L * ladders) % L)
    three_runs(product, *five, L, ladders, 3, 6, precision, slots0=slots0, oracle_ladders=(0, 13, 26))


@pytest.mark.parametrize("cuts", [[1, 5], [2, 1, 3]])
def test_cut_calls(product, five, cuts):
    whole = three_runs(product, *five, 5, 27, 3, 6, "f32", oracle_ladders=())
    assert_same(whole, three_runs(product, *five, 5, 27, 3, 6, "f32", cuts=cuts, oracle_ladders=()), cuts)


def test_several_launches_per_call_and_a_round_too_large_for_the_scratch(product, five, monkeypatch):
    """NLMC_LANE_SCRATCH (read when the engine is created) of two rounds' visiting orders: a call of 6 rounds is 3 launches; the same
    bits, and again with one round's worth, 6 launches.  The order buffer holds the orders of one launch only and every launch reads
    it from its start, so a call that was not cut at whole rounds -- or a launch with a wrong first sweep, first round, plan row or
    log row -- cannot give the bits of the uncut call.  Below one round's worth the call is refused."""
    J, h = five
    T, N, L = 3, J.shape[0], 5
    whole = three_runs(product, J, h, L, 27, T, 6, "f64", oracle_ladders=())
    monkeypatch.setenv("NLMC_LANE_SCRATCH", str(2 * T * N * 2))
    assert_same(whole, three_runs(product, J, h, L, 27, T, 6, "f64", oracle_ladders=()), "three launches")
    monkeypatch.setenv("NLMC_LANE_SCRATCH", str(T * N * 2))
    assert_same(whole, three_runs(product, J, h, L, 27, T, 6, "f64", oracle_ladders=()), "six launches")
    monkeypatch.setenv("NLMC_LANE_SCRATCH", str(T * N * 2 - 1))
    with product.Engine(J, h, L * 27) as eng:
        refused(eng, L, T, "NLMC_LANE_SCRATCH", init_spins(L * 27, N))


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_forced_lanes_come_before_fused_windows(product, precision):
    """n = 300 would admit fused windows: under "force" pt_rounds_deferred takes the lane rounds, and asks for no plan."""
    J, h = make_instance(300, seed=12)
    three_runs(product, J, h, 8, 9, 2, 4, precision, entry="pt_rounds_deferred", mode_a="force", oracle_ladders=(8,))


def refused(eng, L, T, why, m0, prepare=None, plan=True, rounds=3):
    """pt_rounds_lanes answers False with a reason, runs nothing and leaves the rounds route as it was."""
    pairs = n_pairs_of(L)
    eng.pt_init(ladder_betas(L))
    eng.set_spins(m0)
    if plan:
        eng.pt_plan(0, rounds, SEED, pairs)
    if prepare:
        prepare(eng)
    before = (eng.get_spins(), eng.energy_tracked(), eng.pt_slots(), eng.last_rounds_route())
    eng.rounds_fused_refusal = None
    assert eng.pt_rounds_lanes(rounds, T, SEED, 0, 0, pairs) is False
    assert why in eng.rounds_fused_refusal, eng.rounds_fused_refusal
    after = (eng.get_spins(), eng.energy_tracked(), eng.pt_slots(), eng.last_rounds_route())
    assert all(np.array_equal(x, y) for x, y in zip(before[:3], after[:3])) and before[3] == after[3] is None


def test_refusals(product, five):
    J, h = five
    N = J.shape[0]
    with product.Engine(J, h, 65) as eng:
        refused(eng, 65, 2, "64 temperatures", init_spins(65, N))
    m0 = init_spins(10, N)
    with product.Engine(J, h, 10) as eng:
        refused(eng, 5, 2, "phase flags", m0, prepare=lambda e: e.set_flags(nmc_flags(10, N, m0)))
    with product.Engine(J, h, 10) as eng:
        def subset(e):
            e.mark_slots(np.arange(5) == 1)
            e.select("marked")
        refused(eng, 5, 2, "chain subset", m0, prepare=subset)
    with product.Engine(J, h, 10) as eng:
        refused(eng, 5, 2, "not planned", m0, plan=False)
    J2, h2 = make_instance(1025, seed=3)
    with product.Engine(J2, h2, 10) as eng:
        refused(eng, 5, 1, "NLMC_LANE_N", init_spins(10, 1025))


def test_lane_mode_off_keeps_deferred_as_it_was(product, five):
    """n = 37 with the lane mode off: pt_rounds_deferred is refused for want of a fused plan, as ever; pt_rounds_lanes still runs."""
    J, h = five
    L, T, rounds, pairs = 5, 3, 4, n_pairs_of(5)
    m0 = init_spins(2 * L, 37)
    with product.Engine(J, h, 2 * L) as eng:
        eng.pt_init(ladder_betas(L))
        eng.set_spins(m0)
        eng.pt_plan(0, rounds, SEED, pairs)
        assert eng.pt_rounds_deferred(rounds, T, SEED, 0, 0, pairs) is False
        assert eng.rounds_fused_refusal == "nlmc_pt_rounds_deferred: " + FUSED_PLAN_MESSAGE
        assert eng.last_rounds_route() is None and np.array_equal(eng.get_spins(), m0)
        assert eng.pt_rounds_lanes(rounds, T, SEED, 0, 0, pairs) is True
        assert eng.last_rounds_route() == "lanes" and not np.array_equal(eng.get_spins(), m0)


def test_npt_lanes_keyword(product, monkeypatch):
    """NPT(lanes="force") on the Wishart N = 10 instance, 9 restarts of a 6-rung ladder: the results of lanes="off", with rounds
    0 .. 6 of 8 inside k_rounds_lanes launches."""
    calls = []
    orig = product.engine.Engine.pt_rounds_deferred

    def wrapped(self, n_rounds, *a, **k):
        ok = orig(self, n_rounds, *a, **k)
        calls.append((int(n_rounds), bool(ok), self.last_rounds_route() if ok else None, self.last_sweep_route()))
        return ok
    monkeypatch.setattr(product.engine.Engine, "pt_rounds_deferred", wrapped)
    Jn, _, nf, _ = wishart(product)
    J = Jn * nf                                # as the example hands it over: run() normalises

    def run(lanes):
        obj = product.NPT(J, np.zeros(J.shape[0]), rng="philox", seed=0x9E370001 + (5 << 32), lanes=lanes)
        with contextlib.redirect_stdout(io.StringIO()):
            M, E = obj.run(np.geomspace(0.4, 1.6, 6), 6, [False] * 6, num_sweeps_MCMC=40, num_sweeps_read=40, num_swap_attempts=8,
                           num_swapping_pairs=2, num_restarts=9, return_trace="int8")
        return {"M": M, "Energy": E, "restart_energies": obj.restart_energies, "swap_pairs": obj.swap_pairs,
                "swap_accepted": obj.swap_accepted, "final_slots": obj.final_slots}
    got = run("force")
    assert calls and sum(n for n, _, _, _ in calls) == 7 and all(c[1:] == (True, "lanes", "lanes") for c in calls)
    del calls[:]
    ref = run("off")
    assert not any(ok for _, ok, _, _ in calls)              # n = 10 has no fused windows: round by round, as before
    for k in got:
        assert np.array_equal(got[k], ref[k]), k
    assert got["M"].dtype == np.int8 and got["M"].shape == (6 * 10, 5)
    assert got["swap_accepted"].sum() > 0 and not np.array_equal(got["final_slots"], np.arange(54) % 6)
