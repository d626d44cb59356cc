"""The run-long best-state record (include/nlmc.h: nlmc_best_begin ... nlmc_best_end) on every rounds route.

The specification is written here: the same rounds one at a time with the calls that existed before the record -- sweep_philox(beta =
None), get_spins + energy_tracked, pt_swap_philox -- and on the host the strict running minimum of every chain, the round that first
reached it, the state at that round and the first round at or below a target.  Every route must reproduce all four: energies with ==
on the doubles, stamps, first-passage stamps, states byte for byte.  Each case names the route it took.

Random +-1 starts, a geometric ladder 0.2 -> 2.0.  The target of every case is the median over chains of the specification's best
energy.  No case is vacuous: on the specification's own history at least a quarter of the chains have their best round strictly
before the last one, at least two chains improve three or more times, and some chains reach the target while others never do
(checked in spec(); the long-chain pair is exempt and says why).  Seeds: SEED below for every case; the starts are helpers.init_spins'."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN
from helpers import make_instance, init_spins
from test_gpu_lanes import dense_instance

pytestmark = pytest.mark.gpu
SEED = 0xBE570000 + (7 << 32)
KEYS = ("energy", "stamp", "first_hit", "state")


def betas_of(L):
    return np.geomspace(0.2, 2.0, L)


def n_pairs_of(L):
    return max(1, L // 3)                # greedy selection never runs out: a pick removes at most 3 of the L - 1 pairs


def final_state(eng, log=True):
    out = {"spins": eng.get_spins(), "tracked": eng.energy_tracked(), "slots": eng.pt_slots()}
    if log:
        out["pairs"], out["acc"] = eng.pt_log_read()
    return out


def spec(product, J, h, L, ladders, T, rounds, precision, seed=SEED, vacuity=True):
    """Round by round on an engine of its own, no record: -> dict(energy, stamp, first_hit, state, target, hist [rounds, G], final)."""
    G, N = L * ladders, J.shape[0]
    m0, pairs = init_spins(G, N), n_pairs_of(L)
    hist, states = np.empty((rounds, G)), np.empty((rounds, G, N), np.int8)
    with product.Engine(J, h, G) as eng:
        eng.set_spins(m0)
        eng.pt_init(betas_of(L))
        eng.pt_log_begin(0, rounds, pairs)
        for r in range(rounds):
            eng.sweep_philox(T, seed, sweep0=r * T, beta=None, precision=precision)
            states[r], hist[r] = eng.get_spins(), eng.energy_tracked()
            eng.pt_swap_philox(r, seed, pairs, want_log=False)
        eng.pt_check()
        fin = final_state(eng)
    best, stamp, improved = np.full(G, np.inf), np.full(G, -1, np.int32), np.zeros(G, int)
    state = np.zeros((G, N), np.int8)
    for r in range(rounds):
        imp = hist[r] < best                                   # strict: the first attainment is kept
        best[imp], stamp[imp], state[imp] = hist[r][imp], r, states[r][imp]
        improved += imp
    target = float(np.median(best))
    below = hist <= target
    first_hit = np.where(below.any(axis=0), below.argmax(axis=0), -1).astype(np.int32)
    print(f"spec: best before the last round {np.mean(stamp < rounds - 1):.2f}, chains with >= 3 improvements {(improved >= 3).sum()}, "
          f"hit the target {np.mean(first_hit >= 0):.2f}, swaps accepted {fin['acc'].mean():.2f}")
    if vacuity:
        assert np.mean(stamp < rounds - 1) >= 0.25
        assert (improved >= 3).sum() >= 2
        assert (first_hit >= 0).any() and (first_hit < 0).any()
    s = {"energy": best, "stamp": stamp, "first_hit": first_hit, "state": state, "target": target, "hist": hist, "final": fin, "m0": m0}
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def same_record(got, want, what):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


def same_final(got, want, what):
    for k in got:
        assert np.array_equal(got[k], want[k]), (what, k)


def start(eng, s, L, rounds, record=True):
    eng.set_spins(s["m0"])
    eng.pt_set_slots((np.arange(len(s["m0"])) % L).astype(np.int32))
    eng.pt_log_begin(0, rounds, n_pairs_of(L))
    if record:
        eng.best_begin(s["target"])
    else:
        eng.best_end()


def explicit(eng, s, L, T, rounds, precision, route=None, seed=SEED):
    start(eng, s, L, rounds)
    for r in range(rounds):
        eng.sweep_philox(T, seed, sweep0=r * T, beta=None, precision=precision)
        if route:
            assert eng.last_sweep_route() == route
        eng.best_update(r)
        eng.pt_swap_philox(r, seed, n_pairs_of(L), want_log=False)
    eng.pt_check()
    return eng.best_read(), final_state(eng)


def batched(eng, s, L, T, rounds, precision, entry, route, cuts=None, record=True, seed=SEED):
    """The rounds through Engine.<entry>, cut into calls of `cuts` rounds; plans made by the caller."""
    start(eng, s, L, rounds, record=record)
    at = 0
    for k in (cuts or [rounds]):
        assert getattr(eng, entry)(k, T, seed, at * T, at, n_pairs_of(L), precision=precision), getattr(eng, "rounds_fused_refusal", "")
        assert eng.last_rounds_route() == route
        at += k
    eng.pt_check()
    return (eng.best_read() if record else None), final_state(eng)


def pm_j(n=301):
    return make_instance(n, seed=21)


def gauss_on_graph(n=301):
    return make_instance(n, seed=21, with_h=True, gaussian=True)


def chimera128(product):
    W, h = product.instances.txt_to_A_droplet(os.path.join(GOLDEN, "instances", "chimera128__001.txt"))
    J = -sp.csr_matrix(W).astype(np.float64)
    sc = np.max(np.abs(J.data))
    return (J / sc).tocsr(), -np.asarray(h, dtype=np.float64).ravel() / sc


# ---- 1. explicit updates, round by round ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["complete10", "pmj301"])
def test_explicit_updates_round_by_round(product, name):
    """n = 10 complete Gaussian; n = 301 +-J of degree 6 (n_pad = 304 != n: the padded rows of the state copy)."""
    J, h = dense_instance(10, seed=3) if name == "complete10" else pm_j()
    L, ladders, T, rounds = 8, 2, 3, 12
    s = spec(product, J, h, L, ladders, T, rounds, "f32")
    with product.Engine(J, h, L * ladders) as eng:
        eng.pt_init(betas_of(L))
        rec, fin = explicit(eng, s, L, T, rounds, "f32", route="stepwise")
        same_record(rec, s, name)
        same_final(fin, s["final"], name)
        # a second begin resets the record: nothing observed, no state; a read after end still returns it
        eng.best_begin(None)
        eng.best_end()
        empty = eng.best_read()
        assert np.isinf(empty["energy"]).all() and (empty["stamp"] == -1).all() and (empty["first_hit"] == -1).all() and not empty["state"].any()


def test_explicit_updates_on_a_long_chain_pair(product):
    """n = 24 592 > NLMC_LDS_N: two chains of the global-memory kernels, 3 rounds of 1 sweep.  Two chains and three rounds cannot meet
    the conditions of the other cases together (both chains improving three times means both bests in the last round), so this case
    asks only that the record moved and holds a state that differs from the start."""
    J, h = make_instance(24592, seed=5)
    L, T, rounds = 2, 1, 3
    s = spec(product, J, h, L, 1, T, rounds, "f32", vacuity=False)
    assert (s["stamp"] >= 0).all() and not np.array_equal(s["state"], s["m0"])
    with product.Engine(J, h, L) as eng:
        eng.pt_init(betas_of(L))
        rec, fin = explicit(eng, s, L, T, rounds, "f32")
        same_record(rec, s, "long chains")
        same_final(fin, s["final"], "long chains")


# ---- 2. / 3. the rounds inside k_rounds_fused, and a launch per round ----------------------------------------------------------------
FL, FLAD, FT, FROUNDS = 8, 2, 3, 12


def fused_case(product, arith):
    J, h = gauss_on_graph() if arith == "r64" else pm_j()
    prec = "f32" if arith == "f32" else "f64"
    return J, h, prec, spec(product, J, h, FL, FLAD, FT, FROUNDS, prec)


def fused_engine(product, J, h, arith, rounds=FROUNDS, G=FL * FLAD, L=FL, T=FT):
    eng = product.Engine(J, h, G)
    eng.set_fused_f64_real(arith == "r64")
    eng.pt_init(betas_of(L))
    assert eng.plan_philox_fused(0, rounds, T, SEED) == rounds
    eng.pt_plan(0, rounds, SEED, n_pairs_of(L))
    return eng


@pytest.mark.parametrize("arith", ["f32", "f64", "r64"])
def test_rounds_inside_k_rounds_fused(product, arith):
    """Fixed point, the fp64 mode's integer thresholds (+-J is dyadic) and the real-valued fp64 variant on Gaussian couplings of the
    same graph; one call, and rounds 0..5 + 6..11 in two calls (the record carries over)."""
    J, h, prec, s = fused_case(product, arith)
    with fused_engine(product, J, h, arith) as eng:
        for cuts in ([12], [6, 6]):
            rec, fin = batched(eng, s, FL, FT, FROUNDS, prec, "pt_rounds_fused", "in launch", cuts)
            same_record(rec, s, (arith, cuts))
            same_final(fin, s["final"], (arith, cuts))
        _, off = batched(eng, s, FL, FT, FROUNDS, prec, "pt_rounds_fused", "in launch", record=False)      # observation only
        same_final(off, s["final"], (arith, "record off"))


@pytest.mark.parametrize("arith", ["r64", "f32"])
def test_launch_per_round_route_of_pt_rounds_deferred(product, arith, monkeypatch):
    """The real-valued fp64 instance keeps a launch per round by default; f32 takes it with NLMC_NO_PERSISTENT=1 (read at creation)."""
    if arith == "f32":
        monkeypatch.setenv("NLMC_NO_PERSISTENT", "1")
    J, h, prec, s = fused_case(product, arith)
    with fused_engine(product, J, h, arith) as eng:
        for cuts in ([12], [5, 7]):
            rec, fin = batched(eng, s, FL, FT, FROUNDS, prec, "pt_rounds_deferred", "launch per round", cuts)
            same_record(rec, s, (arith, cuts))
            same_final(fin, s["final"], (arith, cuts))
        _, off = batched(eng, s, FL, FT, FROUNDS, prec, "pt_rounds_deferred", "launch per round", record=False)
        same_final(off, s["final"], (arith, "record off"))


# ---- 4. the rounds inside k_rounds_lanes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("name, L, ladders", [("complete10", 16, 5), ("complete10", 5, 13), ("chimera128", 16, 5), ("chimera128", 5, 13)])
def test_rounds_inside_k_rounds_lanes(product, name, L, ladders, precision):
    """L = 16 with 5 ladders: four ladders a wave, a partial last wave.  L = 5 with 13 ladders: 12 ladders a wave leave four tail
    lanes, the last wave holds one ladder."""
    J, h = dense_instance(10, seed=3) if name == "complete10" else chimera128(product)
    T, rounds = 3, 12
    s = spec(product, J, h, L, ladders, T, rounds, precision)
    with product.Engine(J, h, L * ladders) as eng:
        eng.pt_init(betas_of(L))
        eng.pt_plan(0, rounds, SEED, n_pairs_of(L))
        for cuts in ([12], [6, 6]):
            rec, fin = batched(eng, s, L, T, rounds, precision, "pt_rounds_lanes", "lanes", cuts)
            assert eng.last_sweep_route() == "lanes"
            same_record(rec, s, (name, L, cuts))
            same_final(fin, s["final"], (name, L, cuts))
        _, off = batched(eng, s, L, T, rounds, precision, "pt_rounds_lanes", "lanes", record=False)
        same_final(off, s["final"], (name, L, "record off"))


# ---- 5. continuity across launches -------------------------------------------------------------------------------------------------------
def test_more_rounds_than_one_k_rounds_fused_launch_holds(product):
    """1030 rounds of 3 sweeps, n = 301, 16 chains: the call is cut after NLMC_ROUNDS_PER_LAUNCH = 1024 rounds."""
    J, h = pm_j()
    rounds = 1030
    s = spec(product, J, h, FL, FLAD, FT, rounds, "f32")
    with fused_engine(product, J, h, "f32", rounds=rounds) as eng:
        rec, fin = batched(eng, s, FL, FT, rounds, "f32", "pt_rounds_fused", "in launch")
        same_record(rec, s, "1030 rounds")
        same_final(fin, s["final"], "1030 rounds")


def test_more_rounds_than_one_k_rounds_lanes_launch_holds(product, monkeypatch):
    """1030 rounds on the lane route at n = 10, the order scratch cut to 100 rounds' visiting orders: eleven launches."""
    J, h = dense_instance(10, seed=3)
    L, ladders, T, rounds = 16, 5, 3, 1030
    monkeypatch.setenv("NLMC_LANE_SCRATCH", str(100 * T * 10 * 2))
    s = spec(product, J, h, L, ladders, T, rounds, "f32")
    with product.Engine(J, h, L * ladders) as eng:
        eng.pt_init(betas_of(L))
        eng.pt_plan(0, rounds, SEED, n_pairs_of(L))
        rec, fin = batched(eng, s, L, T, rounds, "f32", "pt_rounds_lanes", "lanes")
        assert eng.last_schedule_stats()["orders"] == rounds * T
        same_record(rec, s, "1030 rounds in lanes")
        same_final(fin, s["final"], "1030 rounds in lanes")


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_apt_rounds_lanes_refuses_while_a_record_is_open(product):
    J, h = dense_instance(10, seed=3)
    L, K, T, rounds = 4, 4, 2, 3
    m0 = init_spins(L * K, 10)
    with product.Engine(J, h, L * K) as eng:
        eng.pt_init(betas_of(L))
        eng.pt_plan(0, rounds, SEED, 1)
        eng.set_spins(m0)
        eng.best_begin(None)
        queued, _ = eng.apt_rounds_lanes(rounds, T, SEED, 0, 0, 1)
        assert not queued and "record" in eng.rounds_fused_refusal
        with pytest.raises(NotImplementedError, match="record"):
            product._abi.check(eng._L.nlmc_apt_rounds_lanes(eng._ctx, 0, rounds, T, 0, 0, SEED, 1, 1, None), eng._ctx)
        assert np.array_equal(eng.get_spins(), m0) and np.array_equal(eng.pt_slots(), np.arange(L * K) % L)
        assert np.isinf(eng.best_read()["energy"]).all()
        eng.best_end()
        queued, _ = eng.apt_rounds_lanes(rounds, T, SEED, 0, 0, 1)
        assert queued and eng.last_rounds_route() == "apt lanes"


def test_best_update_needs_all_chains_and_an_open_record(product):
    J, h = pm_j()
    with product.Engine(J, h, 8) as eng:
        eng.pt_init(betas_of(4))
        eng.set_spins(init_spins(8, 301))
        with pytest.raises(RuntimeError, match="no record is open"):
            eng.best_update(0)
        eng.best_begin(None)
        eng.mark_slots([0, 0, 1, 1])
        eng.select("marked")
        with pytest.raises(NotImplementedError, match="subset"):
            eng.best_update(0)
        eng.select("all")
        eng.best_update(0)
        assert (eng.best_read()["stamp"] == 0).all()
