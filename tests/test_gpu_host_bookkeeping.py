"""Host-side bookkeeping of the launch layer (csrc/nlmc.hip), which no kernel test sees: the timing counters behind
nlmc_last_timing / nlmc_timing_total (bench.py reads them), and the edges of the two round windows -- the device-side swap log
(nlmc_pt_log_begin) and the planned pair selections (nlmc_pt_plan) -- as the swap launchers and the rounds entry points apply them;
and the end of a context that holds every family of buffers, beside one that lives on."""
import functools

import numpy as np
import pytest

from helpers import make_instance, init_spins

pytestmark = pytest.mark.gpu
SEED = 0x5EED0019
IN_LAUNCH, PER_ROUND = "in launch", "launch per round"
# +-J at the smallest size with 4-wave fused workgroups; 2 ladders of 8 chains, rounds of 3 sweeps, 3 pairs per round
N, L, NL, T, PAIRS = 512, 8, 2, 3, 3
G = L * NL
BETAS = np.geomspace(0.1, 3.0, L)


@functools.lru_cache(maxsize=None)
def instance(product):
    J, h = make_instance(N, seed=19)
    return product.Instance(J, h), init_spins(G, N)


def engine(product):
    inst, m0 = instance(product)
    eng = product.Engine(inst, None, G)
    eng.set_spins(m0)
    eng.pt_init(BETAS)
    return eng


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_timing_counters(product, precision, monkeypatch):
    W, K = 7, 6

    def deltas(eng, before):
        tm = eng.timing_total()
        return tm["launches_sweep"] - before["launches_sweep"], tm["launches_timed"] - before["launches_timed"]

    with engine(product) as eng:
        # 1. events around every launch
        eng.timing_reset(True, every=1)
        eng.sweep_philox(T, SEED, sweep0=0, beta=None, precision=precision)            # no plan: sweep by sweep, one window
        assert not eng._last_fused()
        tm = eng.timing_total()
        assert (tm["launches_sweep"], tm["launches_timed"]) == (1, 1) and tm["ms_levelize"] > 0 and tm["ms_sweep"] > 0
        lt = eng.last_timing()
        assert lt["launches_sweep"] == 1 and lt["ms_levelize"] > 0 and lt["ms_sweep"] > 0
        assert eng.plan_philox_fused(T, W, T, SEED) == W                               # planning: levelize time, no launch counted
        tp = eng.timing_total()
        assert (tp["launches_sweep"], tp["launches_timed"]) == (1, 1)
        assert tp["ms_levelize"] > tm["ms_levelize"] and tp["ms_sweep"] == tm["ms_sweep"]
        eng.sweep_philox(W * T, SEED, sweep0=T, beta=None, precision=precision)
        assert eng._last_fused()
        assert deltas(eng, tp) == (W, W)
        assert eng.last_timing()["launches_sweep"] == W                                # the last call's launches only
        # 2. events around every third fused window: launches 0, 3 and 6 (the counter restarts at the reset)
        eng.timing_reset(True, every=3)
        eng.sweep_philox(W * T, SEED, sweep0=T, beta=None, precision=precision)
        tm = eng.timing_total()
        assert (tm["launches_sweep"], tm["launches_timed"]) == (W, 3) and tm["ms_sweep"] > 0
        # 3. rounds inside k_rounds_fused launches: every launch is timed and counts for its rounds, whatever `every` is
        eng.pt_plan(0, K, SEED, PAIRS)
        assert eng.pt_rounds_deferred(K, T, SEED, T, 0, PAIRS, precision=precision), getattr(eng, "rounds_fused_refusal", "")
        assert eng.last_rounds_route() == IN_LAUNCH
        assert deltas(eng, tm) == (K, K)
        assert eng.last_timing()["launches_sweep"] == K
        # 5. not accumulating: no times, the launch counts still advance
        eng.timing_reset(False)
        eng.sweep_philox(W * T, SEED, sweep0=T, beta=None, precision=precision)
        assert eng.pt_rounds_deferred(K, T, SEED, T, 0, PAIRS, precision=precision), getattr(eng, "rounds_fused_refusal", "")
        lt, tm = eng.last_timing(), eng.timing_total()
        assert (lt["ms_levelize"], lt["ms_sweep"], lt["launches_sweep"]) == (0, 0, K)
        assert (tm["ms_levelize"], tm["ms_sweep"], tm["launches_sweep"], tm["launches_timed"]) == (0, 0, W + K, 0)

    # 4. a launch per round: the sweep launches count and follow the `every` rule, the closing swap launch is not counted
    monkeypatch.setenv("NLMC_NO_PERSISTENT", "1")
    with engine(product) as eng:
        assert eng.plan_philox_fused(0, 2 * K, T, SEED) == 2 * K
        eng.pt_plan(0, 2 * K, SEED, PAIRS)
        eng.timing_reset(True, every=4)
        zero = eng.timing_total()
        assert eng.pt_rounds_deferred(K, T, SEED, 0, 0, PAIRS, precision=precision), getattr(eng, "rounds_fused_refusal", "")
        assert eng.last_rounds_route() == PER_ROUND
        assert deltas(eng, zero) == (K, 2)                                             # launches 0 and 4 of 0..5
        assert eng.last_timing()["launches_sweep"] == K
        assert eng.pt_rounds_deferred(K, T, SEED, K * T, K, PAIRS, precision=precision), getattr(eng, "rounds_fused_refusal", "")
        assert deltas(eng, zero) == (2 * K, 3)                                         # ... and launch 8 of 6..11
        assert eng.last_timing()["launches_sweep"] == K
        eng.timing_reset(False)
        assert eng.pt_rounds_deferred(K, T, SEED, 0, 0, PAIRS, precision=precision), getattr(eng, "rounds_fused_refusal", "")
        lt, tm = eng.last_timing(), eng.timing_total()
        assert (lt["ms_levelize"], lt["ms_sweep"], lt["launches_sweep"]) == (0, 0, K)
        assert (tm["ms_levelize"], tm["ms_sweep"], tm["launches_sweep"], tm["launches_timed"]) == (0, 0, K, 0)


@pytest.mark.parametrize("route", ["lanes", "waves"])
def test_timing_counters_short_routes(product, route, monkeypatch):
    """The short-chain routes cut a per-chain-order call into windows against the order scratch: every window is one counted launch,
    timed whenever timings accumulate (`every` thins the events of fused windows only), with the k_lane_orders launch as its
    levelize half; the schedule statistics are the visiting orders of the call, no levels."""
    n, R, S = 37, 9, 7
    J, h = make_instance(n, seed=9, with_h=True, gaussian=True)
    tab = np.linspace(0.1, 2.0, R)[:, None] * np.linspace(0.5, 1.5, S)[None, :]
    monkeypatch.setenv("NLMC_LANE_SCRATCH", str(2 * R * n * 3))                        # the orders of three sweeps: windows of 3, 3, 1
    with product.Engine(J, h, R) as eng:
        eng.set_spins(init_spins(R, n))
        (eng.set_lane_sweeps if route == "lanes" else eng.set_wave_sweeps)("force")

        def call():
            eng.sweep_philox(S, SEED, sweep0=11, beta=tab, precision="f32", order="per_chain", record_stride=2, want_energy=True,
                             want_min=True, want_state=True)
            assert eng.last_sweep_route() == route

        eng.timing_reset(True, every=1)
        call()
        tm = eng.timing_total()
        assert (tm["launches_sweep"], tm["launches_timed"]) == (3, 3) and tm["ms_levelize"] > 0 and tm["ms_sweep"] > 0
        assert eng.last_timing()["launches_sweep"] == 3
        assert eng.last_schedule_stats() == {"orders": R * S, "levels": 0}
        eng.timing_reset(True, every=3)
        call()
        tm = eng.timing_total()
        assert (tm["launches_sweep"], tm["launches_timed"]) == (3, 3)
        eng.timing_reset(False)
        call()
        lt, tm = eng.last_timing(), eng.timing_total()
        assert (lt["ms_levelize"], lt["ms_sweep"], lt["launches_sweep"]) == (0, 0, 3)
        assert (tm["ms_levelize"], tm["ms_sweep"], tm["launches_sweep"], tm["launches_timed"]) == (0, 0, 3, 0)


ROUNDS, A, B = 9, 2, 6            # rounds of a run; the window [A, B) of rounds that is logged / planned


def run_rounds(product, precision, log, cuts=None, route=None):
    """ROUNDS rounds from the common start with the swap log over the window `log` = (round0, rounds): one by one (cuts None: a
    sweep launch and a swap launch per round), or through nlmc_pt_rounds_deferred cut as `cuts` says on `route`.  -> spins,
    tracked energies, slot map, log pairs, log decisions."""
    with engine(product) as eng:
        assert eng.plan_philox_fused(0, ROUNDS, T, SEED) == ROUNDS
        eng.pt_plan(0, ROUNDS, SEED, PAIRS)
        eng.pt_log_begin(log[0], log[1], PAIRS)
        at = 0
        for k in (cuts or [1] * ROUNDS):
            if cuts is None:
                eng.sweep_philox(T, SEED, sweep0=at * T, beta=None, precision=precision)
                eng.pt_swap_philox(at, SEED, PAIRS, want_log=False)
            else:
                assert eng.pt_rounds_deferred(k, T, SEED, at * T, at, PAIRS, precision=precision), getattr(eng, "rounds_fused_refusal", "")
                assert eng.last_rounds_route() == route
            at += k
        p, a = eng.pt_log_read()
        return eng.get_spins(), eng.energy(), eng.pt_slots(), p, a


@functools.lru_cache(maxsize=None)
def reference(product, precision):
    """The launch-per-round run with every round logged, computed once."""
    ref = run_rounds(product, precision, (0, ROUNDS))
    for x in ref:
        x.setflags(write=False)
    return ref


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_round_window_edges(product, precision, monkeypatch):
    """The log holds the rows of its window alone (pt_log_read returns B - A rows), so "nothing outside the window is written" shows as:
    the rows read are those of rounds A .. B - 1 and the run's final state is the reference's."""
    ref = reference(product, precision)
    m0 = instance(product)[1]
    assert ref[4].sum() > 0 and not np.array_equal(ref[2], np.arange(G) % L)            # swaps happened

    def check(got, filled, what):
        for name, x, y in zip(("spins", "energies", "slots"), got, ref):
            assert np.array_equal(x, y), (what, name)
        p, a = got[3], got[4]
        assert p.shape == (B - A, NL, PAIRS, 2) and a.shape == (B - A, NL, PAIRS)
        for r in range(A, B):
            if r in filled:
                assert np.array_equal(p[r - A], ref[3][r]) and np.array_equal(a[r - A], ref[4][r]), (what, "round", r)
            else:
                assert np.all(p[r - A].view(np.uint8) == 0xFF) and not a[r - A].any(), (what, "round", r, "not empty")

    window = range(A, B)
    check(run_rounds(product, precision, (A, B - A)), window, "one by one")
    for route in (IN_LAUNCH, PER_ROUND):
        if route == PER_ROUND:
            monkeypatch.setenv("NLMC_NO_PERSISTENT", "1")                               # (read when an engine is created)
        # the middle call lies exactly inside the window
        check(run_rounds(product, precision, (A, B - A), [A, B - A, ROUNDS - B], route), window, (route, "cut at the window"))
        # today's rule: a call the window does not cover is not logged at all
        check(run_rounds(product, precision, (A, B - A), [ROUNDS], route), (), (route, "one call"))
    monkeypatch.delenv("NLMC_NO_PERSISTENT")

    # the window of planned pair selections, through the batch entry
    with engine(product) as eng:
        assert eng.plan_philox_fused(0, ROUNDS, T, SEED) == ROUNDS
        eng.pt_plan(A, B - A, SEED, PAIRS)
        for r0, k in ((A - 1, B - A + 1), (A, B - A + 1)):                              # one round early, one round late
            assert not eng.pt_rounds_fused(k, T, SEED, r0 * T, r0, PAIRS, precision=precision)
            assert "not planned" in eng.rounds_fused_refusal
            assert np.array_equal(eng.get_spins(), m0) and np.array_equal(eng.pt_slots(), np.arange(G) % L)      # nothing has run
        assert eng.pt_rounds_fused(B - A, T, SEED, A * T, A, PAIRS, precision=precision), getattr(eng, "rounds_fused_refusal", "")
        assert eng.last_rounds_route() == IN_LAUNCH
        got = eng.get_spins(), eng.energy(), eng.pt_slots()
    with engine(product) as eng:                        # the same rounds one by one, their selections at other rows of another plan
        eng.pt_plan(0, ROUNDS, SEED, PAIRS)
        for r in range(A, B):
            eng.sweep_philox(T, SEED, sweep0=r * T, beta=None, precision=precision)
            eng.pt_swap_philox(r, SEED, PAIRS, want_log=False)
        for name, x, y in zip(("spins", "energies", "slots"), got, (eng.get_spins(), eng.energy(), eng.pt_slots())):
            assert np.array_equal(x, y), ("planned window", name)
        assert not np.array_equal(got[0], m0)


# ---- context lifetime ---------------------------------------------------------------------------------------------------------------

NA, NA2, LA, RA = 48, 256, 4, 8  # engine A: 2 ladders of 4 chains of 48 spins; A2: the same at 256 spins, where fused windows exist
NB, RB, SB = 96, 4, 4            # engine B: 4 chains of 96 spins, one call of 4 sweeps


@functools.lru_cache(maxsize=None)
def lifetime_case(product):
    """Instances of the engines, and B's sweep on a fresh engine with nothing beside it: (spins, energies)."""
    A = product.Instance(*make_instance(NA, seed=23))
    A2 = product.Instance(*make_instance(NA2, seed=23))
    B = product.Instance(*make_instance(NB, seed=29, with_h=True, gaussian=True))
    with product.Engine(B, None, RB) as eng:
        ref = sweep_b(eng)
    for x in ref:
        x.setflags(write=False)
    return A, A2, B, ref


def sweep_b(eng):
    eng.set_spins(init_spins(RB, NB))
    eng.sweep_philox(SB, SEED, sweep0=5, beta=0.7)
    return eng.get_spins(), eng.energy()


def every_buffer_family(product, inst):
    """An engine on `inst` after one call of every kind that makes buffers: a sweep call on each route, tempering, a plan and two
    rounds, the best-state record, the energy log, an ICM round, a loopy-BP batch.  Fused windows exist from 256 spins on: below,
    the plan call declines, the sweeps stay sweep by sweep, and the rounds run where such chains' rounds run, inside a lane launch."""
    n, fused = inst.n, inst.n >= 256
    a = product.Engine(inst, None, RA)
    a.set_spins(init_spins(RA, n))
    a.pt_init(np.geomspace(0.2, 2.0, LA))
    a.sweep_philox(3, SEED, sweep0=0, beta=None)                                       # sweep by sweep
    assert a.last_sweep_route() == "stepwise"
    assert a.plan_philox_fused(3, 1, 3, SEED) == int(fused)                            # one fused window of 3
    a.sweep_philox(3, SEED, sweep0=3, beta=None)
    assert a._last_fused() == fused
    for setter, route in ((a.set_lane_sweeps, "lanes"), (a.set_wave_sweeps, "waves")):
        setter("force")
        a.sweep_philox(3, SEED, sweep0=6, beta=None, order="per_chain")
        assert a.last_sweep_route() == route
        setter("off")
    a.best_begin()
    a.elog_begin(0, 2)
    assert a.plan_philox_fused(9, 2, 3, SEED) == 2 * int(fused)
    if not fused:
        a.set_lane_sweeps("force")
    a.pt_plan(0, 2, SEED, 1)
    assert a.pt_rounds_deferred(2, 3, SEED, 9, 0, 1), getattr(a, "rounds_fused_refusal", "")
    assert a.last_rounds_route() == (IN_LAUNCH if fused else "lanes")
    best = a.best_read()
    assert best["state"].shape == (RA, n) and np.all(np.isfinite(best["energy"]))
    e, slot = a.elog_read()
    assert e.shape == (2, RA) and np.all(np.isfinite(e)) and np.all((slot >= 0) & (slot < LA))
    assert a.icm_round_ladders(0, SEED, True, want_info=True).shape == (LA * (RA // LA // 2), 2)
    o = a.lbp_convexified(np.ones((1, n)), product.lbp.EdgeGraph(inst).epsilon(inst.h), [0.5, 0.45], 2.5, np.finfo(float).eps, 20,
                          np.tanh(19.06) - np.finfo(float).eps)
    assert o["mag"].shape == (1, n) and np.all(np.abs(o["mag"]) <= 1.0)
    return a


def test_every_buffer_family_goes_with_its_context(product):
    """Contexts that have made every family of their buffers exist (sweep schedules of each route, fused plans, lane orders, the wave
    matrix, tempering, plans and logs of rounds, the best-state record, the energy log, the ICM and loopy-BP buffers) are closed
    while another context on the device lives: the other's next sweep is that of a fresh engine, bit for bit, and closing twice is
    harmless.  Three cycles in one process.  Results and clean returns only: free device memory is not this test's to read."""
    inst_a, inst_a2, inst_b, ref = lifetime_case(product)
    for cycle in range(3):
        a, a2 = every_buffer_family(product, inst_a), every_buffer_family(product, inst_a2)
        b = product.Engine(inst_b, None, RB)                                           # created while A lives
        a.close()
        a2.close()
        got = sweep_b(b)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), cycle
        b.close()
        b.close()                                                                      # a second close does nothing
        a.close()
