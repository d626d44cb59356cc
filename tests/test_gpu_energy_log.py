"""The run-long per-round energy log (include/nlmc.h: nlmc_elog_begin ... nlmc_elog_end) on every rounds route.

The yardstick is a host loop on the same build with no log open.  Per round: sweep_philox(beta = None); for APT cases the Houdayer call
icm_round_ladders; energy_tracked() and pt_slots(); pt_swap_philox.  It collects (E[r], slot[r]): what the swap decision of round r
sees.  With the log open every route must return exactly these doubles and integers (== on the arrays, no tolerance), and must leave
final spins, tracked energies, slots and the swap log identical to the yardstick's -- and to the same route run without a log.

Random +-1 starts (helpers.init_spins), a geometric ladder 0.2 -> 2.0, SEED below for every case.  No case is vacuous: on the
yardstick's own history some swap is accepted (slots move between rounds) and energies differ from round to round (checked in
yardstick())."""

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import make_instance, init_spins
from test_gpu_lanes import wishart

pytestmark = pytest.mark.gpu
SEED = 0xE1060000 + (11 << 32)


def betas_of(L):
    return np.geomspace(0.2, 2.0, L)


def n_pairs_of(L):
    """2 pairs on the short ladders (L = 5: whichever pair the greedy selection picks first, a disjoint one is left), L // 3 on long ones."""
    return 2 if L < 9 else L // 3


def regular3(n=256, seed=8, gaussian=False):
    """Random 3-regular graph (configuration model, redrawn until simple), couplings +-1 -- or, on the SAME graph, Gaussian couplings
    scaled to max |J| = 1 with Gaussian fields."""
    r = np.random.default_rng(seed)
    while True:
        stubs = r.permutation(np.repeat(np.arange(n), 3))
        a, b = np.minimum(stubs[0::2], stubs[1::2]), np.maximum(stubs[0::2], stubs[1::2])
        if (a != b).all() and len(set(zip(a.tolist(), b.tolist()))) == len(a):
            break
    w = r.choice([-1.0, 1.0], size=len(a))
    h = np.zeros(n)
    if gaussian:
        g = np.random.default_rng(seed + 1)
        w = g.standard_normal(len(a))
        w /= np.max(np.abs(w))
        h = 0.3 * g.standard_normal(n)
    J = sp.coo_matrix((np.concatenate([w, w]), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(n, n)).tocsr()
    J.sort_indices()
    return J, h


def final_state(eng):
    out = {"spins": eng.get_spins(), "tracked": eng.energy_tracked(), "slots": eng.pt_slots()}
    out["pairs"], out["acc"] = eng.pt_log_read()
    return out


_YARD = {}


def yardstick(product, key, J, h, L, ladders, T, rounds, precision, real=False, katz=None, systems=1, seed=SEED):
    """Round by round on an engine of its own, no log: -> dict(E [rounds, G], slot [rounds, G], final, m0, pairs, houdayer).  `katz`
    not None: an APT round (the Houdayer step of icm_round_ladders between the sweeps and the observation).  Computed once per key."""
    if key in _YARD:
        return _YARD[key]
    G, N = L * ladders, J.shape[0]
    m0, pairs = init_spins(G, N), n_pairs_of(L)
    E, sl = np.empty((rounds, G)), np.empty((rounds, G), np.int32)
    houdayer = 0
    with product.Engine(J, h, G) as eng:
        eng.set_fused_f64_real(real)
        eng.set_spins(m0)
        eng.pt_init(betas_of(L))
        if systems > 1:
            eng.apt_systems(systems)
        eng.pt_log_begin(0, rounds, pairs)
        for r in range(rounds):
            eng.sweep_philox(T, seed, sweep0=r * T, beta=None, precision=precision)
            if katz is not None:
                before = eng.energy_tracked()
                eng.icm_round_ladders(r, seed, katz)
                houdayer += int((eng.energy_tracked() != before).sum())
            E[r], sl[r] = eng.energy_tracked(), eng.pt_slots()
            eng.pt_swap_philox(r, seed, pairs, want_log=False)
        eng.pt_check()
        fin = final_state(eng)
    print(f"yardstick {key}: swaps accepted {fin['acc'].mean():.2f}, energies changed by the Houdayer step {houdayer}")
    assert fin["acc"].any() and (sl[1:] != sl[:-1]).any() and (E[1:] != E[:-1]).any() and not np.isnan(E).any()
    y = {"E": E, "slot": sl, "final": fin, "m0": m0, "pairs": pairs, "houdayer": houdayer, "L": L, "T": T, "rounds": rounds}
    for v in (E, sl, m0, *fin.values()):
        v.setflags(write=False)
    _YARD[key] = y
    return y


def same_final(got, want, what):
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k)


def same_log(got, y, what, lo=0, hi=None):
    hi = y["rounds"] if hi is None else hi
    e, s = got
    assert e.dtype == np.float64 and s.dtype == np.int32 and e.shape == s.shape == (hi - lo, y["E"].shape[1]), what
    assert np.array_equal(e, y["E"][lo:hi]), (what, "energy")
    assert np.array_equal(s, y["slot"][lo:hi]), (what, "slot")


def start(eng, y, window):
    """The yardstick's start; `window` = (round0, n_rounds) of the log, or None: no log open."""
    eng.set_spins(y["m0"])
    eng.pt_set_slots((np.arange(len(y["m0"])) % y["L"]).astype(np.int32))
    eng.pt_log_begin(0, y["rounds"], y["pairs"])
    if window is None:
        eng.elog_end()
    else:
        eng.elog_begin(*window)


def batched(eng, y, precision, entry, route, cuts=None, window=(0, None), seed=SEED, **kw):
    """The yardstick's rounds through Engine.<entry>, cut into calls of `cuts` rounds -> (log or None, final state)."""
    rounds, T = y["rounds"], y["T"]
    if window is not None and window[1] is None:
        window = (window[0], rounds)
    start(eng, y, window)
    at = 0
    for k in (cuts or [rounds]):
        ok = getattr(eng, entry)(k, T, seed, at * T, at, y["pairs"], precision=precision, **kw)
        assert (ok[0] if isinstance(ok, tuple) else ok), getattr(eng, "rounds_fused_refusal", "")
        assert eng.last_rounds_route() == route
        at += k
    eng.pt_check()
    return (eng.elog_read() if window is not None else None), final_state(eng)


def check_route(eng, y, precision, entry, route, cut_sets, what, **kw):
    for cuts in cut_sets:
        log, fin = batched(eng, y, precision, entry, route, cuts, **kw)
        same_log(log, y, (what, cuts))
        same_final(fin, y["final"], (what, cuts))
    _, off = batched(eng, y, precision, entry, route, window=None, **kw)          # the same route without a log
    same_final(off, y["final"], (what, "log off"))


# ---- 1. / 2. the rounds inside k_rounds_fused, and a launch per round ------------------------------------------------------------------
FL, FLAD, FT, FROUNDS = 5, 2, 3, 7


def fused_case(product, arith, rounds=FROUNDS):
    J, h = regular3(gaussian=arith == "r64")
    prec = "f32" if arith == "f32" else "f64"
    return J, h, prec, yardstick(product, ("fused", arith, rounds), J, h, FL, FLAD, FT, rounds, prec, real=arith == "r64")


def fused_engine(product, J, h, arith, rounds=FROUNDS):
    eng = product.Engine(J, h, FL * FLAD)
    eng.set_fused_f64_real(arith == "r64")
    eng.pt_init(betas_of(FL))
    assert eng.plan_philox_fused(0, rounds, FT, SEED) == rounds
    eng.pt_plan(0, rounds, SEED, n_pairs_of(FL))
    return eng


@pytest.mark.parametrize("arith", ["f32", "f64", "r64"])
def test_rounds_inside_k_rounds_fused(product, arith):
    """n = 256 random 3-regular, 2 ladders x L = 5, T = 3, 2 pairs, 7 rounds: fixed point, the fp64 mode's integer thresholds (+-J is
    dyadic) and the real-valued fp64 variant on Gaussian couplings of the same graph; one call, and rounds 0..2 + 3..6 under one log."""
    J, h, prec, y = fused_case(product, arith)
    with fused_engine(product, J, h, arith) as eng:
        check_route(eng, y, prec, "pt_rounds_fused", "in launch", ([7], [3, 4]), arith)


def test_row_index_crosses_a_k_rounds_fused_launch_boundary(product):
    """1030 rounds > NLMC_ROUNDS_PER_LAUNCH = 1024: the row of a round is round0 + r of the CALL, not of the launch."""
    rounds = 1030
    J, h, prec, y = fused_case(product, "f32", rounds)
    with fused_engine(product, J, h, "f32", rounds) as eng:
        log, fin = batched(eng, y, prec, "pt_rounds_fused", "in launch")
        same_log(log, y, "1030 rounds")
        same_final(fin, y["final"], "1030 rounds")


@pytest.mark.parametrize("arith", ["f32", "f64", "r64"])
def test_launch_per_round_route_of_pt_rounds_deferred(product, arith, monkeypatch):
    """The same shape with NLMC_NO_PERSISTENT=1 (read at context creation): a k_elog_update behind every sweep launch."""
    monkeypatch.setenv("NLMC_NO_PERSISTENT", "1")
    J, h, prec, y = fused_case(product, arith)
    with fused_engine(product, J, h, arith) as eng:
        check_route(eng, y, prec, "pt_rounds_deferred", "launch per round", ([7], [3, 4]), arith)


def test_in_launch_route_of_pt_rounds_deferred(product):
    J, h, prec, y = fused_case(product, "f32")
    with fused_engine(product, J, h, "f32") as eng:
        check_route(eng, y, prec, "pt_rounds_deferred", "in launch", ([7],), "deferred")


# ---- 3. the rounds inside k_rounds_lanes ---------------------------------------------------------------------------------------------
LANE_T, LANE_ROUNDS = 2, 9


def lanes_case(product, L, ladders, precision, rounds=LANE_ROUNDS):
    J, h, _, _ = wishart(product)
    return J, h, yardstick(product, ("lanes", L, ladders, precision, rounds), J, h, L, ladders, LANE_T, rounds, precision)


def lanes_engine(product, J, h, L, ladders, rounds=LANE_ROUNDS):
    eng = product.Engine(J, h, L * ladders)
    eng.pt_init(betas_of(L))
    eng.pt_plan(0, rounds, SEED, n_pairs_of(L))
    return eng


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("L, ladders", [(6, 10), (64, 2), (5, 13)])
def test_rounds_inside_k_rounds_lanes(product, L, ladders, precision):
    """Wishart N = 10.  L = 6 x 10 ladders: one wave, 4 tail lanes.  L = 64 x 2: full waves.  L = 5 x 13: a second, partly filled
    wave.  One call, and rounds 0..4 + 5..8 in two calls under one log."""
    J, h, y = lanes_case(product, L, ladders, precision)
    with lanes_engine(product, J, h, L, ladders) as eng:
        check_route(eng, y, precision, "pt_rounds_lanes", "lanes", ([9], [5, 4]), (L, ladders, precision))
        assert eng.last_sweep_route() == "lanes"


# ---- 4. the APT rounds inside k_apt_rounds_lanes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("katz", [True, False])
@pytest.mark.parametrize("systems", [1, 3])
def test_rounds_inside_k_apt_rounds_lanes(product, systems, katz):
    """K = 4 sub-replica ladders of L = 6 on the Wishart N = 10 instance, M = 1 and M = 3 systems, Katzgraber on and off, 6 rounds of 2
    sweeps.  The yardstick observes behind icm_round_ladders, and at least one Houdayer move of its run changes an energy: a log
    stored before the step could not pass."""
    J, h, _, _ = wishart(product)
    K, L, T, rounds = 4, 6, 2, 6
    y = yardstick(product, ("apt", systems, katz), J, h, L, K * systems, T, rounds, "f32", katz=katz, systems=systems)
    assert y["houdayer"] > 0
    with product.Engine(J, h, L * K * systems) as eng:
        eng.pt_init(betas_of(L))
        if systems > 1:
            eng.apt_systems(systems)
        eng.pt_plan(0, rounds, SEED, y["pairs"])
        check_route(eng, y, "f32", "apt_rounds_lanes", "apt lanes", ([6], [2, 4]), (systems, katz), katzgraber=katz)
        # it keeps refusing while a best-state record is open, log or no log
        start(eng, y, (0, rounds))
        eng.best_begin(None)
        queued, _ = eng.apt_rounds_lanes(rounds, T, SEED, 0, 0, y["pairs"], katzgraber=katz)
        assert not queued and "record" in eng.rounds_fused_refusal
        eng.best_end()
        assert np.isnan(eng.elog_read()[0]).all()


def test_apt_rounds_lanes_f64(product):
    J, h, _, _ = wishart(product)
    K, L, T, rounds = 4, 6, 2, 6
    y = yardstick(product, ("apt", "f64"), J, h, L, K, T, rounds, "f64", katz=True)
    assert y["houdayer"] > 0
    with product.Engine(J, h, L * K) as eng:
        eng.pt_init(betas_of(L))
        eng.pt_plan(0, rounds, SEED, y["pairs"])
        check_route(eng, y, "f64", "apt_rounds_lanes", "apt lanes", ([6],), "f64", katzgraber=True)


# ---- 5. explicit updates: the stepwise sweeps, and chains too long for LDS -----------------------------------------------------------
def explicit(eng, y, precision, seed=SEED):
    start(eng, y, (0, y["rounds"]))
    for r in range(y["rounds"]):
        eng.sweep_philox(y["T"], seed, sweep0=r * y["T"], beta=None, precision=precision)
        eng.elog_update(r)
        eng.pt_swap_philox(r, seed, y["pairs"], want_log=False)
    eng.pt_check()
    return eng.elog_read(), final_state(eng)


def test_explicit_updates_round_by_round(product):
    J, h = make_instance(301, seed=21)
    L, ladders, T, rounds = 5, 2, 3, 7
    y = yardstick(product, "pmj301", J, h, L, ladders, T, rounds, "f32")
    with product.Engine(J, h, L * ladders) as eng:
        eng.pt_init(betas_of(L))
        log, fin = explicit(eng, y, "f32")
        same_log(log, y, "explicit")
        same_final(fin, y["final"], "explicit")
        e_s, c_s = eng.elog_read(by="slot")
        assert e_s.shape == c_s.shape == (rounds, ladders, L)
        for r in range(rounds):
            for c in range(L * ladders):
                assert c_s[r, c // L, y["slot"][r, c]] == c and e_s[r, c // L, y["slot"][r, c]] == y["E"][r, c]
        with pytest.raises(ValueError):
            eng.elog_read(by="ladder")


def test_explicit_updates_on_a_long_chain_pair(product):
    """n = 24 592 > NLMC_LDS_N: two chains of the global-memory kernels, 3 rounds of 1 sweep; k_elog_update reads the state arrays."""
    J, h = make_instance(24592, seed=5)
    L, T, rounds = 2, 1, 3
    G, m0 = L, init_spins(L, 24592)
    E, sl = np.empty((rounds, G)), np.empty((rounds, G), np.int32)
    with product.Engine(J, h, G) as eng:
        eng.pt_init(betas_of(L))
        for logged in (False, True):
            eng.set_spins(m0)
            eng.pt_set_slots(np.arange(G, dtype=np.int32))
            if logged:
                eng.elog_begin(0, rounds)
            for r in range(rounds):
                eng.sweep_philox(T, SEED, sweep0=r * T, beta=None)
                if logged:
                    eng.elog_update(r)
                else:
                    E[r], sl[r] = eng.energy_tracked(), eng.pt_slots()
                eng.pt_swap_philox(r, SEED, 1, want_log=False)
        got_e, got_s = eng.elog_read()
    assert np.array_equal(got_e, E) and np.array_equal(got_s, sl) and (E[1:] != E[:-1]).all()


# ---- 6. window and overwrite rules, on the lanes shape ---------------------------------------------------------------------------------
def test_window_inside_and_past_the_run(product):
    """A log over rounds [2, 5) of a 7-round run: rows as the yardstick's rounds 2-4, whether the run is one call or cut inside the
    window.  A window [4, 10) reaching past the run: rows of rounds 4-6, then NaN / -1.  A window the run never reaches stays empty.
    Reads after elog_end return the same rows."""
    L, ladders, rounds = 6, 10, 7
    J, h, y = lanes_case(product, L, ladders, "f32", rounds)
    with lanes_engine(product, J, h, L, ladders, rounds) as eng:
        for cuts in ([7], [3, 4], [1, 1, 5]):
            log, fin = batched(eng, y, "f32", "pt_rounds_lanes", "lanes", cuts, window=(2, 3))
            same_log(log, y, ("[2, 5)", cuts), 2, 5)
            same_final(fin, y["final"], ("[2, 5)", cuts))
        (e, s), _ = batched(eng, y, "f32", "pt_rounds_lanes", "lanes", window=(4, 6))
        same_log((e[:3], s[:3]), y, "[4, 10)", 4, 7)
        assert np.isnan(e[3:]).all() and (s[3:] == -1).all()
        eng.elog_end()
        e2, s2 = eng.elog_read()
        assert np.array_equal(e, e2, equal_nan=True) and np.array_equal(s, s2)
        (e, s), fin = batched(eng, y, "f32", "pt_rounds_lanes", "lanes", window=(7, 4))
        assert e.shape == (4, L * ladders) and np.isnan(e).all() and (s == -1).all()
        same_final(fin, y["final"], "window behind the run")
        # the same windows through explicit updates
        start(eng, y, (2, 3))
        for r in range(rounds):
            eng.sweep_philox(LANE_T, SEED, sweep0=r * LANE_T, beta=None)
            eng.elog_update(r)                       # rounds outside the window are not logged and are no error
            eng.pt_swap_philox(r, SEED, y["pairs"], want_log=False)
        same_log(eng.elog_read(), y, "explicit [2, 5)", 2, 5)


def test_a_second_observation_of_a_round_overwrites_the_first(product):
    L, ladders = 6, 10
    J, h, y = lanes_case(product, L, ladders, "f32", 7)
    with lanes_engine(product, J, h, L, ladders, 7) as eng:
        start(eng, y, (0, 2))
        eng.sweep_philox(LANE_T, SEED, sweep0=0, beta=None)
        eng.elog_update(1)
        first = eng.energy_tracked()
        eng.sweep_philox(LANE_T, SEED, sweep0=LANE_T, beta=None)
        eng.elog_update(1)
        second = eng.energy_tracked()
        e, s = eng.elog_read()
        assert (first != second).any() and np.array_equal(e[1], second) and np.array_equal(s[1], eng.pt_slots())
        assert np.isnan(e[0]).all() and (s[0] == -1).all()


# ---- 7. both records open ----------------------------------------------------------------------------------------------------------
KEYS = ("energy", "stamp", "first_hit", "state")


@pytest.mark.parametrize("route", ["fused", "lanes"])
def test_best_record_and_energy_log_together(product, route):
    """best_begin and elog_begin on one run: the log is the yardstick's, the record is the one a run with the record alone leaves."""
    if route == "fused":
        J, h, prec, y = fused_case(product, "f32")
        eng, entry, name = fused_engine(product, J, h, "f32"), "pt_rounds_fused", "in launch"
    else:
        J, h, y = lanes_case(product, 5, 13, "f32")
        eng, entry, name, prec = lanes_engine(product, J, h, 5, 13), "pt_rounds_lanes", "lanes", "f32"
    target = float(np.median(y["E"].min(axis=0)))
    with eng:
        eng.best_begin(target)
        _, fin = batched(eng, y, prec, entry, name, window=None)
        alone = eng.best_read()
        same_final(fin, y["final"], "record alone")
        eng.best_begin(target)
        log, fin = batched(eng, y, prec, entry, name)
        both = eng.best_read()
        eng.best_end()
    same_log(log, y, "both open")
    same_final(fin, y["final"], "both open")
    for k in KEYS:
        assert np.array_equal(alone[k], both[k]), k
    assert np.array_equal(both["energy"], y["E"].min(axis=0)) and (both["first_hit"] >= 0).any()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(product):
    J, h = make_instance(301, seed=21)
    with product.Engine(J, h, 8) as eng:
        with pytest.raises(RuntimeError, match="nlmc_pt_init"):
            eng.elog_update(0)
        with pytest.raises(RuntimeError, match="nlmc_pt_init"):
            eng.elog_begin(0, 4)
        eng.pt_init(betas_of(4))
        eng.set_spins(init_spins(8, 301))
        with pytest.raises(RuntimeError, match="no log is open"):
            eng.elog_update(0)
        eng.elog_begin(0, 2)
        eng.mark_slots([0, 0, 1, 1])
        eng.select("marked")
        with pytest.raises(NotImplementedError, match="subset"):
            eng.elog_update(0)
        eng.select("all")
        eng.elog_update(0)
        e, s = eng.elog_read()
        assert np.array_equal(e[0], eng.energy_tracked()) and np.array_equal(s[0], np.arange(8) % 4) and np.isnan(e[1]).all()
    # a context created with chain_base != 0 that holds half a ladder: the log takes contexts of whole ladders
    with product.Engine(J, h, 4, chain_base=2, n_chains_global=8) as eng:
        eng.pt_init(betas_of(4))
        with pytest.raises(NotImplementedError, match="cut ladder"):
            eng.elog_begin(0, 2)
