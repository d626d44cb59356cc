"""Tempering rounds of chains of 257 .. 1024 spins inside a wave launch (csrc/nlmc_wave_long_rounds.h: k_rounds_waves_long, the local
fields built once per launch and resident in LDS across the swap rounds).

Every case starts four runs from one fixed state and compares them bit for bit -- spins, tracked energies, slots and the device-side
swap log: (a) the rounds in k_rounds_waves_long launches, (a') the same without a device log, (b) pt_rounds_deferred with the wave
sweeps forced, set_wave_rounds and set_wave_long on and set_wave_long_rounds off -- a wave sweep call and a swap call per round --, (c)
every mode off, round by round, with the pair selections made inside the swap kernel.  Named ladders are also driven by the oracle
double.  Shapes: the smallest that reach every path of the kernel -- three ladders a workgroup and a short last workgroup whose idle
waves must meet the barriers, both register counts at their boundary, sixteen regions of 1024 spins (the LDS cap with a chain per
wave), waves that run two and three chains in turn, a chain base, permuted slots, cut calls, several launches per call, slot-keyed
random numbers, both observers, the refusals, the deferred route with the option on and off, and two drivers."""
import numpy as np
import pytest

from fake_engine import OracleEngine
from helpers import make_instance, init_spins
from test_gpu_lane_rounds import n_pairs_of, state, assert_same, FUSED_PLAN_MESSAGE
from test_gpu_waves_drivers import quiet
from wavefields import dense_instance, phase_flags

pytestmark = pytest.mark.gpu
SEED = 0xC3C30000 + (11 << 32)          # high bits set


def sparse_betas(L):
    """Close rungs on a sparse Gaussian instance of a few hundred spins: swaps are accepted."""
    return np.linspace(0.30, 0.30 + 0.02 * (L - 1), L)


def dense_betas(L):
    """Inverse temperatures of a dense instance's scale (fields of order sqrt(n)), close rungs: the chains move, swaps are accepted."""
    return np.linspace(0.05, 0.05 + 0.002 * (L - 1), L)


def set_modes(eng, waves="off", wave_rounds=False, wave_long=False, wave_long_rounds=False):
    eng.set_wave_sweeps(waves)
    eng.set_wave_rounds(wave_rounds)
    eng.set_wave_long(wave_long)
    eng.set_wave_long_rounds(wave_long_rounds)


ALL_ON = dict(waves="force", wave_rounds=True, wave_long=True, wave_long_rounds=True)
CALL_BY_CALL = dict(ALL_ON, wave_long_rounds=False)


def four_runs(product, J, h, L, ladders, T, rounds, betas, chain_base=0, G=None, slots0=None, cuts=None, entry="pt_rounds_waves_long",
              oracle_ladders=(0,), seed=SEED, by_round=True, after_init=None):
    """-> (a).  Asserts (a) == (a without a log) == (b) == (c) and the oracle on `oracle_ladders`.  entry = "pt_rounds_deferred": (a)
    runs with every option on.  after_init(eng): once, after pt_init."""
    N, GL = J.shape[0], L * ladders
    G = GL if G is None else G
    pairs = n_pairs_of(L)
    m0 = init_spins(GL, N)
    start = (np.arange(G) % L).astype(np.int32) if slots0 is None else np.asarray(slots0, np.int32)
    cuts = cuts or [rounds]
    with product.Engine(J, h, GL, chain_base=chain_base, n_chains_global=G) as eng:
        eng.pt_init(betas)
        if after_init:
            after_init(eng)

        def begin(modes, log=True, plan=True):
            set_modes(eng, **modes)
            eng.set_spins(m0)
            eng.pt_set_slots(start)
            eng.pt_plan(0, rounds if plan else 0, seed, pairs)
            eng.pt_log_begin(0, rounds if log else 0, pairs)

        def batched(call, modes, route, log=True):
            begin(modes, log=log)
            at = 0
            for k in cuts:
                assert getattr(eng, call)(k, T, seed, at * T, at, pairs, precision="f32"), getattr(eng, "rounds_fused_refusal", "")
                assert eng.last_rounds_route() == route and eng.last_sweep_route() == "waves"
                if route == "waves long":
                    assert eng.last_schedule_stats() == {"orders": k * T, "levels": 0} and not eng._last_fused()
                at += k
            eng.pt_check()
            if not log:
                return {"spins": eng.get_spins(), "energy": eng.energy_tracked(), "slots": eng.pt_slots()}
            return state(eng)

        def round_by_round():
            begin({}, plan=False)
            for r in range(rounds):
                eng.sweep_philox(T, seed, sweep0=r * T, beta=None, precision="f32")
                assert eng.last_sweep_route() == "stepwise"
                eng.pt_swap_philox(r, seed, pairs, want_log=False)
            eng.pt_check()
            return state(eng)

        modes_a = ALL_ON if entry == "pt_rounds_deferred" else {}
        a = batched(entry, modes_a, "waves long")
        assert_same(a, batched(entry, modes_a, "waves long", log=False), "without a device log", log=False)
        assert_same(a, batched("pt_rounds_deferred", CALL_BY_CALL, "launch per round"), "a wave sweep call and a swap call per round")
        if by_round:
            assert_same(a, round_by_round(), "every mode off")
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
def sparse257():
    """n = 257 (n_pad = 272), sparse Gaussian couplings and fields."""
    return make_instance(257, seed=9, with_h=True, gaussian=True)


@pytest.fixture(scope="module")
def dense300():
    """n = 300 (n_pad = 304), a complete graph with diagonal entries (left out of the energy deltas, not of the fields)."""
    return dense_instance(300, seed=4, diag=True)


@pytest.mark.parametrize("knob", [None, "1", "3"], ids=["rule", "ladders1", "ladders3"])
def test_three_ladders_a_workgroup_and_a_short_last_workgroup(product, sparse257, knob, monkeypatch):
    """L = 5, 7 ladders.  NLMC_WAVE_ROUNDS_LADDERS = 3 (read when the engine is created): 15 waves per workgroup, and the last
    workgroup holds one ladder -- its ten waves without a chain must still meet every barrier.  = 1: a ladder per workgroup.  The
    results do not depend on it."""
    if knob is not None:
        monkeypatch.setenv("NLMC_WAVE_ROUNDS_LADDERS", knob)
    four_runs(product, *sparse257, 5, 7, 3, 6, sparse_betas(5), oracle_ladders=(0, 3, 6))


@pytest.mark.parametrize("n", [512, 513])
def test_register_count_boundary(product, n):
    """Eight fields per lane up to n = 512, sixteen beyond (n_pad = 512 | 528)."""
    J, h = make_instance(n, seed=100 + n, with_h=True, gaussian=True)
    four_runs(product, J, h, 4, 3, 2, 4, sparse_betas(4), oracle_ladders=(1,))


def test_sixteen_regions_of_1024_spins_on_a_complete_graph(product):
    """n = 1024, L = 16, one ladder: sixteen waves with a chain each, 147616 bytes of LDS -- the most a chain per wave asks for."""
    J, h = dense_instance(1024, seed=1224)
    four_runs(product, J, h, 16, 1, 1, 3, dense_betas(16), oracle_ladders=(0,))


@pytest.mark.parametrize("L", [17, 33])
def test_chains_in_turn_and_a_diagonal(product, dense300, L):
    """L = 17: two chains a wave on nine waves, the last wave with a single chain; L = 33: three on eleven waves (uneven turns).  A
    wave takes the fields of the chain whose turn it is from the chain's region."""
    four_runs(product, *dense300, L, 2, 2, 4, dense_betas(L), oracle_ladders=(1,))


def test_chain_base_keys_and_maps_are_global_and_a_permuted_start(product, sparse257):
    """A context that owns ladders 2 .. 8 of 9, from permuted slots: Philox keys by global ladder and chain, chain_of_slot rows by
    global ladder."""
    L, ladders = 5, 7
    G = L * ladders + 2 * L
    r = np.random.default_rng(17)
    slots0 = np.concatenate([r.permutation(L) for _ in range(G // L)])
    assert not np.array_equal(slots0, np.arange(G) % L)
    four_runs(product, *sparse257, L, ladders, 3, 6, sparse_betas(L), chain_base=2 * L, G=G, slots0=slots0, oracle_ladders=(0, 6))


def test_cut_calls_continue_sweep_and_round_counters(product, sparse257):
    b = sparse_betas(5)
    whole = four_runs(product, *sparse257, 5, 7, 3, 6, b, oracle_ladders=(), by_round=False)
    assert_same(whole, four_runs(product, *sparse257, 5, 7, 3, 6, b, cuts=[2, 4], oracle_ladders=(), by_round=False), [2, 4])


def refused(eng, betas, T, why, m0, prepare=None, plan=True, rounds=3, precision="f32"):
    """pt_rounds_waves_long answers False with a reason, runs nothing and leaves the rounds route as it was."""
    pairs = n_pairs_of(len(betas))
    eng.pt_init(betas)
    eng.set_spins(m0)
    if plan:
        eng.pt_plan(0, rounds, SEED, pairs)
    if prepare:
        prepare(eng)
    before = (eng.get_spins(), eng.energy_tracked(), eng.pt_slots(), eng.last_rounds_route())
    eng.rounds_fused_refusal = None
    assert eng.pt_rounds_waves_long(rounds, T, SEED, 0, 0, pairs, precision=precision) is False
    assert why in eng.rounds_fused_refusal, eng.rounds_fused_refusal
    assert eng.rounds_fused_refusal.startswith("nlmc_pt_rounds_waves_long: ")
    after = (eng.get_spins(), eng.energy_tracked(), eng.pt_slots(), eng.last_rounds_route())
    assert all(np.array_equal(x, y) for x, y in zip(before[:3], after[:3])) and before[3] == after[3] is None


def test_several_launches_per_call_and_a_round_too_large_for_the_scratch(product, sparse257, monkeypatch):
    """NLMC_LANE_SCRATCH (read when the engine is created) of two rounds' visiting orders: a call of 6 rounds is 3 launches, each of
    which builds the fields again from the spins the previous one left; the same bits.  One byte below one round's worth the call is
    refused."""
    J, h = sparse257
    T, N, L = 3, J.shape[0], 5
    b = sparse_betas(L)
    whole = four_runs(product, J, h, L, 7, T, 6, b, oracle_ladders=(), by_round=False)
    monkeypatch.setenv("NLMC_LANE_SCRATCH", str(2 * T * N * 2))
    assert_same(whole, four_runs(product, J, h, L, 7, T, 6, b, oracle_ladders=(), by_round=False), "three launches")
    monkeypatch.setenv("NLMC_LANE_SCRATCH", str(T * N * 2 - 1))
    with product.Engine(J, h, L * 7) as eng:
        refused(eng, b, T, "NLMC_LANE_SCRATCH", init_spins(L * 7, N))


def test_slot_keyed_random_numbers(product, sparse257):
    """apt_shard(world = 1): the Philox key of a chain follows its slot, so a chain whose slot moved in a swap round takes another key
    from the next round on."""
    L = 5
    b = sparse_betas(L)
    four_runs(product, *sparse257, L, 7, 3, 6, b, oracle_ladders=(), after_init=lambda e: e.apt_shard(b, 1, 0))


def test_refusals(product, sparse257):
    J, h = sparse257
    N, b = J.shape[0], sparse_betas(5)
    m0 = init_spins(10, N)
    for n, why in ((256, "more than NLMC_WAVE_N"), (1025, "at most NLMC_WAVE_LONG_N")):
        Jn, hn = make_instance(n, seed=3)
        with product.Engine(Jn, hn, 10) as eng:
            refused(eng, b, 1, why, init_spins(10, n))
    with product.Engine(J, h, 10) as eng:
        refused(eng, b, 2, "NLMC_F32", m0, precision="f64")
    with product.Engine(J, h, 10) as eng:
        refused(eng, b, 2, "phase flags", m0, prepare=lambda e: e.set_flags(phase_flags(10, N, m0)))
    with product.Engine(J, h, 10) as eng:
        def subset(e):
            e.mark_slots(np.arange(5) == 1)
            e.select("marked")
        refused(eng, b, 2, "chain subset", m0, prepare=subset)
    with product.Engine(J, h, 10) as eng:
        refused(eng, b, 2, "not planned", m0, plan=False)
    J2, h2 = make_instance(1024, seed=3)
    with product.Engine(J2, h2, 64) as eng:
        refused(eng, sparse_betas(64), 1, "the ladders of a workgroup do not fit its LDS", init_spins(64, 1024), rounds=1)


@pytest.mark.parametrize("shape", ["L5", "L17"])
@pytest.mark.parametrize("cuts", [[6], [2, 4]])
def test_observers(product, sparse257, dense300, shape, cuts):
    """The best-state record (with a target) and the energy log open together: pt_rounds_waves_long equals the round-by-round drive
    with best_update / elog_update in every field -- a wave with one chain (L = 5) and waves that run chains in turn (L = 17)."""
    if shape == "L5":
        (J, h), L, ladders, T, betas = sparse257, 5, 7, 3, sparse_betas(5)
    else:
        (J, h), L, ladders, T, betas = dense300, 17, 2, 2, dense_betas(17)
    rounds, pairs, GL = 6, n_pairs_of(L), L * ladders
    m0 = init_spins(GL, J.shape[0])
    with product.Engine(J, h, GL) as eng:
        eng.pt_init(betas)

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
            assert eng.pt_rounds_waves_long(k, T, SEED, at * T, at, pairs), eng.rounds_fused_refusal
            assert eng.last_rounds_route() == "waves long"
            at += k
        got = read()
        eng.best_end()
        eng.elog_end()
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_deferred_takes_the_kernel_only_with_all_three_options(product, dense300):
    """n = 300: with set_wave_rounds, set_wave_long and set_wave_long_rounds on pt_rounds_deferred runs inside k_rounds_waves_long; with
    the new option off it says "launch per round" (run (b) of four_runs) -- the same bits."""
    four_runs(product, *dense300, 4, 2, 2, 4, dense_betas(4), entry="pt_rounds_deferred", oracle_ladders=(1,))
    J, h = dense300
    L, G, T, rounds, pairs = 4, 8, 2, 2, 1
    with product.Engine(J, h, G) as eng:
        eng.pt_init(dense_betas(L))
        eng.set_spins(init_spins(G, 300))
        eng.pt_plan(0, rounds, SEED, pairs)
        assert eng.wave_long_rounds is False
        for missing in ("wave_rounds", "wave_long"):               # the new option without one of the other two changes nothing:
            set_modes(eng, **dict(ALL_ON, **{missing: False}))     # no short-chain route takes the call, and no fused plan was made
            assert eng.pt_rounds_deferred(rounds, T, SEED, 0, 0, pairs) is False
            assert eng.rounds_fused_refusal == "nlmc_pt_rounds_deferred: " + FUSED_PLAN_MESSAGE and eng.last_rounds_route() is None


def test_a_shape_the_kernel_refuses_still_completes_call_by_call(product):
    """n = 1024, L = 64: the ladder's regions do not fit a workgroup's LDS, so with every option on pt_rounds_deferred runs a sweep
    call and a swap call per round, as with the option off."""
    J, h = make_instance(1024, seed=3, with_h=True, gaussian=True)
    L, T, rounds = 64, 1, 1
    pairs, betas, m0 = n_pairs_of(L), np.linspace(0.30, 0.40, L), init_spins(L, 1024)
    with product.Engine(J, h, L) as eng:
        eng.pt_init(betas)

        def run(modes, plan):
            set_modes(eng, **modes)
            eng.set_spins(m0)
            eng.pt_set_slots(np.arange(L, dtype=np.int32))
            eng.pt_plan(0, rounds if plan else 0, SEED, pairs)
            eng.pt_log_begin(0, rounds, pairs)
            if plan:
                assert eng.pt_rounds_deferred(rounds, T, SEED, 0, 0, pairs) is True, eng.rounds_fused_refusal
                assert eng.last_rounds_route() == "launch per round" and eng.last_sweep_route() == "waves"
            else:
                eng.sweep_philox(T, SEED, sweep0=0, beta=None)
                assert eng.last_sweep_route() == "stepwise"
                eng.pt_swap_philox(0, SEED, pairs, want_log=False)
            return state(eng)
        a, b, c = run(ALL_ON, True), run(CALL_BY_CALL, True), run({}, False)
    assert_same(a, b, "the option off")
    assert_same(a, c, "every mode off")
    assert not np.array_equal(a["spins"], m0) and a["acc"].sum() > 0


def tempering(product, J, h, wave_long_rounds):
    L, ladders, rounds, S, pairs = 6, 2, 4, 2, 2
    lt = product.distributed.LocalTempering(product.Instance(J, h), sparse_betas(L), L * ladders, SEED, pairs, [0], wave_sweeps="force",
                                            wave_rounds=True, wave_long=True, wave_long_rounds=wave_long_rounds, track_best=True,
                                            track_energies=True)
    try:
        assert lt.engs[0].wave_long_rounds is wave_long_rounds
        lt.set_spins(init_spins(L * ladders, J.shape[0]))
        lt.plan(rounds * S, rounds)
        lt.log_begin(rounds)
        lt.run_rounds(rounds, S)
        lt.check()
        return {"spins": lt.gather_spins(), "slots": lt.slots(), "log": lt.swap_log(), "tracked": lt.engs[0].energy_tracked(),
                "routes": lt.rounds_routes, "deferred": lt.deferred_rounds, "best": lt.best(), "elog": lt.energy_log()}
    finally:
        lt.close()


def test_local_tempering_run_rounds(product, sparse257):
    """LocalTempering with all four keywords: run_rounds' chunk runs inside k_rounds_waves_long, which keeps the best-state record and
    the energy log itself; the results of wave_long_rounds=False."""
    a, b = tempering(product, *sparse257, False), tempering(product, *sparse257, True)
    assert a["routes"] == ["launch per round"] and b["routes"] == ["waves long"] and a["deferred"] == b["deferred"] == 4
    assert np.array_equal(a["spins"], b["spins"]) and np.array_equal(a["slots"], b["slots"]) and np.array_equal(a["tracked"], b["tracked"])
    assert np.array_equal(a["log"][0], b["log"][0]) and np.array_equal(a["log"][1], b["log"][1]) and a["log"][1].any()
    for k in ("energy", "stamp", "first_hit", "state"):
        assert np.array_equal(a["best"][k], b["best"][k]), k
    assert np.array_equal(a["elog"][0], b["elog"][0]) and np.array_equal(a["elog"][1], b["elog"][1])
    assert np.isfinite(b["elog"][0]).all() and (b["best"]["stamp"] >= 0).all()


def test_npt_run(product, monkeypatch):
    """NPT.run with all four keywords against NPT.run with none: n = 300, 6 replicas, 2 restarts, 3 rounds."""
    J, h = make_instance(300, seed=14, with_h=True, gaussian=True)
    J = J.toarray()
    R, S, rounds = 6, 2, 3
    betas = np.geomspace(0.3, 2.0, R)
    calls = []
    orig = product.engine.Engine.pt_rounds_deferred

    def wrapped(self, n_rounds, *a, **k):
        ok = orig(self, n_rounds, *a, **k)
        calls.append((int(n_rounds), bool(ok), self.last_rounds_route() if ok else None))
        return ok
    monkeypatch.setattr(product.engine.Engine, "pt_rounds_deferred", wrapped)

    def run(**kw):
        obj = product.NPT(J, h, rng="philox", seed=4242, **kw)
        with quiet():
            M, E = obj.run(betas, R, [False] * R, num_sweeps_MCMC=S * rounds, num_sweeps_read=S * rounds, num_swap_attempts=rounds,
                           num_swapping_pairs=2, num_restarts=2, return_trace="int8")
        return M, E, obj.restart_energies
    want = run()
    assert not any(route == "waves long" for _, _, route in calls)
    del calls[:]
    got = run(waves="force", wave_rounds=True, wave_long=True, wave_long_rounds=True)
    assert calls and all(c[1:] == (True, "waves long") for c in calls)
    for x, y in zip(want, got):
        assert np.array_equal(x, y)
    assert want[0].any()
