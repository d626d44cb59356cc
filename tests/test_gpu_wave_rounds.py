"""Tempering rounds inside a wave launch (csrc/nlmc_wave_rounds.h: k_rounds_waves, a chain per wave and whole ladders per workgroup).

Every case starts four runs from one fixed state and compares them bit for bit -- spins, tracked energies, slots and the device-side
swap log: (a) the rounds in k_rounds_waves launches, (a') the same without a device log, (b) the same engine with the wave sweeps
forced, round by round (sweep_philox + pt_swap_philox), (c) every mode off, round by round, with the pair selections made inside the
swap kernel.  Named ladders are also driven by the oracle double.  Shapes: the smallest that reach every path of the kernel -- several
ladders per workgroup and a short last workgroup whose idle waves must meet the barriers, sixteen full waves, waves that run two, three
and four chains in turn with their state parked in LDS, a chain shorter than a Philox block, the register-count boundaries R = 1 / 2 /
4, the staged matrix and global rows, a chain base, permuted slots, cut calls, several launches per call, both observers."""
import numpy as np
import pytest

from fake_engine import OracleEngine
from helpers import make_instance, init_spins
from test_gpu_lanes import dense_instance, wishart, nmc_flags
from test_gpu_lane_rounds import ladder_betas, n_pairs_of, state, assert_same, FUSED_PLAN_MESSAGE

pytestmark = pytest.mark.gpu
SEED = 0xC3C30000 + (11 << 32)          # high bits set
BOUNDARY_SEED = {40: 2, 63: 5, 64: 1, 65: 1, 128: 1, 129: 3, 192: 4, 193: 3, 256: 14}


def four_runs(product, J, h, L, ladders, T, rounds, chain_base=0, G=None, slots0=None, cuts=None, entry="pt_rounds_waves", oracle_ladders=(0,),
              seed=SEED, by_round=True):
    """-> (a).  Asserts (a) == (a without a log) == (b) == (c) and the oracle on `oracle_ladders`.  entry = "pt_rounds_deferred": (a)
    runs under set_wave_sweeps("force") + set_wave_rounds(True)."""
    N, GL = J.shape[0], L * ladders
    G = GL if G is None else G
    betas, pairs = ladder_betas(L), n_pairs_of(L)
    m0 = init_spins(GL, N)
    start = (np.arange(G) % L).astype(np.int32) if slots0 is None else np.asarray(slots0, np.int32)
    cuts = cuts or [rounds]
    deferred = entry == "pt_rounds_deferred"
    with product.Engine(J, h, GL, chain_base=chain_base, n_chains_global=G) as eng:
        eng.pt_init(betas)

        def begin(mode, wave_rounds=False, log=True, plan=True):
            eng.set_wave_sweeps(mode)
            eng.set_wave_rounds(wave_rounds)
            eng.set_spins(m0)
            eng.pt_set_slots(start)
            eng.pt_plan(0, rounds if plan else 0, seed, pairs)
            eng.pt_log_begin(0, rounds if log else 0, pairs)

        def in_launch(log):
            begin("force" if deferred else "off", wave_rounds=deferred, log=log)
            at = 0
            for k in cuts:
                assert getattr(eng, entry)(k, T, seed, at * T, at, pairs, precision="f32"), getattr(eng, "rounds_fused_refusal", "")
                assert eng.last_rounds_route() == "waves" and eng.last_sweep_route() == "waves"
                assert eng.last_schedule_stats() == {"orders": k * T, "levels": 0} and not eng._last_fused()
                at += k
            eng.pt_check()
            if not log:
                return {"spins": eng.get_spins(), "energy": eng.energy_tracked(), "slots": eng.pt_slots()}
            return state(eng)

        def round_by_round(mode, route, plan):
            begin(mode, plan=plan)
            for r in range(rounds):
                eng.sweep_philox(T, seed, sweep0=r * T, beta=None, precision="f32")
                assert eng.last_sweep_route() == route
                eng.pt_swap_philox(r, seed, pairs, want_log=False)
            eng.pt_check()
            return state(eng)

        a = in_launch(True)
        assert_same(a, in_launch(False), "without a device log", log=False)
        if by_round:
            assert_same(a, round_by_round("force", "waves", True), "wave sweeps round by round")
            assert_same(a, round_by_round("off", "stepwise", False), "every mode off")
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
            o.sweep_philox(T, seed, sweep0=r * T, precision="f32")
            o.pt_swap_philox(r, seed, pairs)
        rows = slice(g * L, (g + 1) * L)
        assert np.array_equal(a["spins"][rows], o.get_spins()), f"oracle: spins of ladder {g}"
        assert np.array_equal(a["slots"][chain_base + g * L:chain_base + (g + 1) * L], o.pt_slots()[chain_base + g * L:chain_base + (g + 1) * L]), g
    return a


@pytest.fixture(scope="module")
def five():
    return make_instance(37, seed=9, with_h=True, gaussian=True)


@pytest.mark.parametrize("knob", [None, "1", "3"], ids=["rule", "ladders1", "ladders3"])
def test_three_ladders_a_workgroup_and_a_short_last_workgroup(product, five, knob, monkeypatch):
    """L = 5, 7 ladders.  NLMC_WAVE_ROUNDS_LADDERS = 3 (read when the engine is created): 15 waves per workgroup, and the last
    workgroup holds one ladder -- its ten waves without a chain must still meet every barrier.  = 1: a ladder per workgroup.  The
    results do not depend on it."""
    if knob is not None:
        monkeypatch.setenv("NLMC_WAVE_ROUNDS_LADDERS", knob)
    four_runs(product, *five, 5, 7, 3, 6, oracle_ladders=(0, 2, 3, 6))


def test_sixteen_full_waves_on_real_couplings(product):
    """L = 16 on the golden Wishart N = 10 instance as run() normalises it: one ladder per workgroup, every wave one rung."""
    J, h, _, _ = wishart(product)
    four_runs(product, J, h, 16, 2, 3, 5, oracle_ladders=(1,))


@pytest.mark.parametrize("L", [17, 33, 64])
def test_chains_in_turn_with_parked_state_and_a_diagonal(product, L):
    """L = 17: two chains a wave on nine waves, the last wave with a single chain that stays in registers; L = 33: three (uneven
    turns); L = 64: four.  The instance has diagonal entries (left out of the energy deltas, not of the fields)."""
    J, h = dense_instance(12, seed=4, diag=True)
    four_runs(product, J, h, L, 2, 3, 5, oracle_ladders=(1,))


def test_eight_two_rung_ladders_a_workgroup_of_a_chain_shorter_than_a_philox_block(product, monkeypatch):
    """L = 2, n = 2, 20 ladders, eight per workgroup (16 waves), the last workgroup four."""
    monkeypatch.setenv("NLMC_WAVE_ROUNDS_LADDERS", "8")
    J, h = dense_instance(2, seed=6)
    four_runs(product, J, h, 2, 20, 2, 8, oracle_ladders=(0, 7, 8, 19))


@pytest.mark.parametrize("n,jlds", [(63, None), (64, None), (65, None), (128, None), (129, None), (192, None), (193, None), (256, None),
                                    (40, "0"), (129, "0")])
def test_register_count_and_staging_boundaries(product, n, jlds, monkeypatch):
    """R = 1 / 2 / 4 fields per lane at n = 64 | 65 and 128 | 129, the matrix staged in LDS up to n = 192 and read from global memory
    from 193 on; NLMC_WAVE_JLDS=0: global rows at every n."""
    if jlds is not None:
        monkeypatch.setenv("NLMC_WAVE_JLDS", jlds)
    J, h = make_instance(n)
    # six swap decisions per case: the seed of each size is the first after SEED at which the oracle accepts one and the slots move
    four_runs(product, J, h, 3, 2, 2, 3, oracle_ladders=(1,), seed=SEED + BOUNDARY_SEED[n])


def test_a_matrix_that_leaves_no_room_for_the_parked_state(product):
    """n = 192, L = 64: matrix (144 KB) + parked fields and spins of 64 chains exceed the LDS ceiling, so the launch shape drops the
    staging and reads global rows."""
    J, h = make_instance(192)
    four_runs(product, J, h, 64, 1, 1, 3, oracle_ladders=())


def test_chain_base_keys_and_maps_are_global(product, five):
    """A context that owns ladders 2 .. 8 of 9: Philox keys by global ladder and chain, chain_of_slot rows by global ladder."""
    L, ladders = 5, 7
    four_runs(product, *five, L, ladders, 3, 6, chain_base=2 * L, G=L * ladders + 2 * L, oracle_ladders=(0, 6))


def test_permuted_start(product, five):
    L, ladders = 5, 7
    r = np.random.default_rng(17)
    slots0 = np.concatenate([r.permutation(L) for _ in range(ladders)])
    assert not np.array_equal(slots0, np.arange(L * ladders) % L)
    four_runs(product, *five, L, ladders, 3, 6, slots0=slots0, oracle_ladders=(0, 3, 6))


@pytest.mark.parametrize("cuts", [[1, 5], [2, 1, 3]])
def test_cut_calls(product, five, cuts):
    whole = four_runs(product, *five, 5, 7, 3, 6, oracle_ladders=(), by_round=False)
    assert_same(whole, four_runs(product, *five, 5, 7, 3, 6, cuts=cuts, oracle_ladders=(), by_round=False), cuts)


def refused(eng, L, T, why, m0, prepare=None, plan=True, rounds=3, precision="f32"):
    """pt_rounds_waves answers False with a reason, runs nothing and leaves the rounds route as it was."""
    pairs = n_pairs_of(L)
    eng.pt_init(ladder_betas(L))
    eng.set_spins(m0)
    if plan:
        eng.pt_plan(0, rounds, SEED, pairs)
    if prepare:
        prepare(eng)
    before = (eng.get_spins(), eng.energy_tracked(), eng.pt_slots(), eng.last_rounds_route())
    eng.rounds_fused_refusal = None
    assert eng.pt_rounds_waves(rounds, T, SEED, 0, 0, pairs, precision=precision) is False
    assert why in eng.rounds_fused_refusal, eng.rounds_fused_refusal
    assert eng.rounds_fused_refusal.startswith("nlmc_pt_rounds_waves: ")
    after = (eng.get_spins(), eng.energy_tracked(), eng.pt_slots(), eng.last_rounds_route())
    assert all(np.array_equal(x, y) for x, y in zip(before[:3], after[:3])) and before[3] == after[3] is None


def test_several_launches_per_call_and_a_round_too_large_for_the_scratch(product, five, monkeypatch):
    """NLMC_LANE_SCRATCH (read when the engine is created) of two rounds' visiting orders: a call of 6 rounds is 3 launches; the same
    bits, and again with one round's worth, 6 launches: every launch pays the prologue again and takes the maps, energies and spins
    the previous one left.  One byte below one round's worth the call is refused."""
    J, h = five
    T, N, L = 3, J.shape[0], 5
    whole = four_runs(product, J, h, L, 7, T, 6, oracle_ladders=(), by_round=False)
    monkeypatch.setenv("NLMC_LANE_SCRATCH", str(2 * T * N * 2))
    assert_same(whole, four_runs(product, J, h, L, 7, T, 6, oracle_ladders=(), by_round=False), "three launches")
    monkeypatch.setenv("NLMC_LANE_SCRATCH", str(T * N * 2))
    assert_same(whole, four_runs(product, J, h, L, 7, T, 6, oracle_ladders=(), by_round=False), "six launches")
    monkeypatch.setenv("NLMC_LANE_SCRATCH", str(T * N * 2 - 1))
    with product.Engine(J, h, L * 7) as eng:
        refused(eng, L, T, "NLMC_LANE_SCRATCH", init_spins(L * 7, N))


def test_wave_rounds_come_before_fused_windows_and_off_changes_nothing(product):
    """n = 256 admits fused windows.  With the wave sweeps forced and set_wave_rounds(True) pt_rounds_deferred takes the wave rounds and
    asks for no plan; with set_wave_rounds(False) the same call is what it was: refused for want of a fused plan, nothing run."""
    J, h = make_instance(256)
    L, ladders, T, rounds = 8, 3, 3, 4
    four_runs(product, J, h, L, ladders, T, rounds, entry="pt_rounds_deferred", oracle_ladders=(2,))
    pairs, m0 = n_pairs_of(L), init_spins(L * ladders, 256)
    with product.Engine(J, h, L * ladders) as eng:
        eng.pt_init(ladder_betas(L))
        eng.set_spins(m0)
        eng.pt_plan(0, rounds, SEED, pairs)
        eng.set_wave_sweeps("force")
        assert eng.wave_rounds is False
        assert eng.pt_rounds_deferred(rounds, T, SEED, 0, 0, pairs) is False
        assert eng.rounds_fused_refusal == "nlmc_pt_rounds_deferred: " + FUSED_PLAN_MESSAGE
        assert eng.last_rounds_route() is None and np.array_equal(eng.get_spins(), m0)
        # with a plan the call runs, and not on the wave rounds
        assert eng.plan_philox_fused(0, rounds, T, SEED) == rounds
        assert eng.pt_rounds_deferred(rounds, T, SEED, 0, 0, pairs) is True
        assert eng.last_rounds_route() in ("in launch", "launch per round")
        eng.set_wave_rounds(True)
        assert eng.wave_rounds is True
        eng.set_spins(m0)
        eng.pt_set_slots((np.arange(L * ladders) % L).astype(np.int32))
        assert eng.pt_rounds_deferred(rounds, T, SEED, 0, 0, pairs) is True
        assert eng.last_rounds_route() == "waves"


def test_refusals(product, five):
    J, h = five
    N = J.shape[0]
    with product.Engine(J, h, 65) as eng:
        refused(eng, 65, 2, "64 temperatures", init_spins(65, N))
    m0 = init_spins(10, N)
    with product.Engine(J, h, 10) as eng:
        refused(eng, 5, 2, "NLMC_F32", m0, precision="f64")
    with product.Engine(J, h, 10) as eng:
        refused(eng, 5, 2, "phase flags", m0, prepare=lambda e: e.set_flags(nmc_flags(10, N, m0)))
    with product.Engine(J, h, 10) as eng:
        def subset(e):
            e.mark_slots(np.arange(5) == 1)
            e.select("marked")
        refused(eng, 5, 2, "chain subset", m0, prepare=subset)
    with product.Engine(J, h, 10) as eng:
        refused(eng, 5, 2, "not planned", m0, plan=False)
    J2, h2 = make_instance(257, seed=3)
    with product.Engine(J2, h2, 10) as eng:
        refused(eng, 5, 1, "NLMC_WAVE_N", init_spins(10, 257))


@pytest.mark.parametrize("shape", ["L5", "L17"])
@pytest.mark.parametrize("cuts", [[6], [2, 4]])
def test_observers(product, five, shape, cuts):
    """The best-state record (with a target) and the energy log open together: pt_rounds_waves equals the round-by-round drive with
    best_update / elog_update in every field -- a wave with one chain (L = 5) and waves that run chains in turn (L = 17)."""
    if shape == "L5":
        (J, h), L, ladders, T = five, 5, 7, 3
    else:
        (J, h), L, ladders, T = dense_instance(12, seed=4, diag=True), 17, 2, 3
    rounds, pairs, GL = 6, n_pairs_of(L), L * ladders
    m0 = init_spins(GL, J.shape[0])
    with product.Engine(J, h, GL) as eng:
        eng.pt_init(ladder_betas(L))

        def begin(target):
            eng.set_spins(m0)
            eng.pt_set_slots((np.arange(GL) % L).astype(np.int32))
            eng.pt_plan(0, rounds, SEED, pairs)
            eng.pt_log_begin(0, rounds, pairs)
            eng.best_begin(target)
            eng.elog_begin(0, rounds)

        def read():
            out = dict(state(eng))
            out.update({"best_" + k: v for k, v in eng.best_read().items()})
            out["elog_energy"], out["elog_slot"] = eng.elog_read()
            return out

        def explicit(target):
            begin(target)
            for r in range(rounds):
                eng.sweep_philox(T, SEED, sweep0=r * T, beta=None)
                eng.best_update(r)
                eng.elog_update(r)
                eng.pt_swap_philox(r, SEED, pairs, want_log=False)
            return read()

        # a target some chains reach and others do not, in some round after the first (from a free run: it depends on the RNG only)
        free = explicit(None)
        target = float(np.median(free["elog_energy"][rounds // 2]))
        want = explicit(target)
        assert (want["best_first_hit"] >= 0).any() and (want["best_first_hit"] < 0).any() and (want["best_stamp"] > 0).any()
        begin(target)
        at = 0
        for k in cuts:
            assert eng.pt_rounds_waves(k, T, SEED, at * T, at, pairs), eng.rounds_fused_refusal
            at += k
        got = read()
        eng.best_end()
        eng.elog_end()
    for k in want:
        assert np.array_equal(got[k], want[k]), k
