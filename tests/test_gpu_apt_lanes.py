"""APT rounds of short chains in one launch (csrc/nlmc_lane_apt.h: k_apt_rounds_lanes, one system per workgroup, a Houdayer pair per
lane).

Every case starts four runs from one fixed state and compares them bit for bit -- spins, tracked energies, slots, the device-side swap
log and the {components, picked size} of every Houdayer pair of every round: (a) the rounds in k_apt_rounds_lanes launches, (a') the
same without a device log and without info, (b) the same engine with the lane sweeps forced, round by round (sweep_philox +
icm_round_ladders + pt_swap_philox), (c) the lane mode off, round by round.  The first cases are also driven whole by the oracle
double.  After every run the tracked energies are compared with a recomputation from the final states.  The cases are run once and
kept: the last test asserts over the whole set that none of the paths stayed unvisited."""
import contextlib
import io

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
import scalefamily as sf
from fake_engine import OracleEngine
from helpers import make_instance, init_spins
from test_gpu_lanes import dense_instance, wishart, nmc_flags

pytestmark = pytest.mark.gpu
SEED = 0xA97C0000 + (13 << 32)          # high bits set


def n_pairs_of(L):
    return max(1, L // 3)                # greedy selection never runs out: a pick removes at most 3 of the L - 1 pairs


def chimera128(product):
    import os
    from conftest import GOLDEN
    W, h = product.instances.txt_to_A_droplet(os.path.join(GOLDEN, "instances", "chimera128__001.txt"))
    J = -sp.csr_matrix(W).astype(np.float64)
    s = np.max(np.abs(J.data))
    return (J / s).tocsr(), -np.asarray(h, dtype=np.float64).ravel() / s


def permuted_ring(n, seed):
    """A ring of n spins numbered by a random permutation, couplings +-1: the smallest index of a component travels a few spins per
    label pass."""
    r = np.random.default_rng(seed)
    p = r.permutation(n)
    a, b = p, np.roll(p, -1)
    w = r.choice([-1.0, 1.0], size=n)
    J = sp.coo_matrix((np.concatenate([w, w]), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(n, n)).tocsr()
    J.sort_indices()
    return J, np.zeros(n)


def diag_and_zero(product):
    """Gaussian couplings on 30 spins with diagonal entries, one stored coupling of exactly zero (both directions) and one so small
    that its fixed-point value is zero while its fp64 value is not: no edge and an edge of the disagreement graph."""
    J, h = make_instance(30, seed=14, with_h=True, gaussian=True)
    J = J.tolil()
    J.setdiag(0.25 * np.random.default_rng(3).standard_normal(30))
    J = J.tocsr()
    J.sort_indices()
    inst = product.Instance(J, h)
    rows = np.repeat(np.arange(30), np.diff(inst.indptr))
    off = np.nonzero(rows < inst.indices)[0]

    def both(e, v):
        k, j = rows[e], inst.indices[e]
        back = inst.indptr[j] + int(np.where(inst.indices[inst.indptr[j]:inst.indptr[j + 1]] == k)[0][0])
        inst.data[e] = inst.data[back] = v
    both(off[5], 0.0)
    both(off[17], 1e-13)
    return inst


def energy_tolerance(inst, qs, esc, exact, updates):
    """|tracked - recomputed|.  Exact instances (every J, h a multiple of 2^-qs): 0.  Otherwise the tracked energy is the exact start
    energy rounded to 2^-esc plus deltas of the fixed-point model, whose couplings and fields differ from the true ones by at most
    2^-(qs+1) each: the model's energy differs from the true one by at most B = (nnz / 2 + n) 2^-(qs+1) at the start and at the end;
    the fp64 sweeps round every flip's delta to 2^-esc (half a unit per update), the recomputation rounds once more."""
    if exact:
        return 0.0
    return 2.0 * (inst.nnz / 2 + inst.n) * 2.0 ** -(qs + 1) + (updates + 2) * 2.0 ** -esc


_KEPT = {}


def four_runs(product, J, h, K, L, T, rounds, precision, katz=True, pairs=None, slots0=None, cuts=None, oracle_run=False, exact=False,
              betas=None, seed=SEED):
    """-> dict of run (a) with info [rounds, L (K // 2), 2] and `cross`: a moved pair of round 0 joined columns of two waves."""
    inst = J if isinstance(J, product.Instance) else product.Instance(J, h)
    N, G = inst.n, K * L
    betas = np.geomspace(0.3, 1.5, L) if betas is None else np.asarray(betas, float)
    pairs = n_pairs_of(L) if pairs is None else pairs
    m0 = init_spins(G, N)
    start = (np.arange(G) % L).astype(np.int32) if slots0 is None else np.asarray(slots0, np.int32)
    cuts = cuts or [rounds]
    NP = L * (K // 2)
    with product.Engine(inst, None, G) as eng:
        eng.pt_init(betas)
        tol = energy_tolerance(inst, eng.field_scale, eng.energy_scale, exact, rounds * (T + 1) * N)

        def begin(mode, log=True, plan=True):
            eng.set_lane_sweeps(mode)
            eng.set_spins(m0)
            eng.pt_set_slots(start)
            if pairs > 0:
                eng.pt_plan(0, rounds if plan else 0, seed, pairs)
                eng.pt_log_begin(0, rounds if log else 0, pairs)

        def state(info, log=True):
            s = {"spins": eng.get_spins(), "energy": eng.energy_tracked(), "slots": eng.pt_slots(), "info": info}
            if log and pairs > 0:
                s["pairs"], s["acc"] = eng.pt_log_read()
            err = np.max(np.abs(s["energy"] - eng.energy()))
            assert err <= tol, ("tracked energies against a recomputation", err, tol)
            return s

        def in_launch(log):
            begin("off", log=log)
            at, infos = 0, []
            for k in cuts:
                ok, info = eng.apt_rounds_lanes(k, T, seed, at * T, at, pairs, katzgraber=katz, precision=precision, want_info=log)
                assert ok, getattr(eng, "rounds_fused_refusal", "")
                assert eng.last_rounds_route() == "apt lanes" and eng.last_sweep_route() == "lanes"
                assert eng.last_schedule_stats() == {"orders": k * T, "levels": 0} and not eng._last_fused()
                assert (info is None) == (not log)
                infos.append(info)
                at += k
            if pairs > 0:
                eng.pt_check()
            return state(np.concatenate(infos) if log else None, log)

        def by_round(mode, route, plan):
            begin(mode, plan=plan)
            infos = []
            for r in range(rounds):
                eng.sweep_philox(T, seed, sweep0=r * T, beta=None, precision=precision)
                assert eng.last_sweep_route() == route
                infos.append(eng.icm_round_ladders(r, seed, katz, want_info=True))
                if pairs > 0:
                    eng.pt_swap_philox(r, seed, pairs, want_log=False)
            if pairs > 0:
                eng.pt_check()
            return state(np.stack(infos).reshape(rounds, NP, 2))

        def same(x, y, what, keys):
            for k in keys:
                assert np.array_equal(x[k], y[k]), (what, k)

        keys = ("spins", "energy", "slots", "info") + (("pairs", "acc") if pairs > 0 else ())
        a = in_launch(True)
        assert a["info"].shape == (rounds, NP, 2)
        same(a, in_launch(False), "without a device log and without info", ("spins", "energy", "slots"))
        same(a, by_round("force", "lanes", True), "lane sweeps round by round", keys)
        same(a, by_round("off", "stepwise", False), "lane mode off", keys)
    assert not np.array_equal(a["spins"], m0)
    if pairs > 0:
        assert (a["pairs"] >= 0).all() and (a["pairs"][..., 1] == a["pairs"][..., 0] + 1).all()
    if oracle_run:
        o = OracleEngine(inst, G, 0, G)
        o.pt_init(betas)
        o.pt_set_slots(start)
        o.set_spins(m0)
        infos = []
        for r in range(rounds):
            o.sweep_philox(T, seed, sweep0=r * T, precision=precision)
            infos.append(o.icm_round_ladders(r, seed, katz, want_info=True))
            if pairs > 0:
                o.pt_swap_philox(r, seed, pairs)
        assert np.array_equal(a["info"], np.stack(infos).reshape(rounds, NP, 2)), "oracle: components and picked sizes"
        assert np.array_equal(a["spins"], o.get_spins()), "oracle: spins"
        assert np.array_equal(a["slots"], o.pt_slots()), "oracle: slots"
    # round 0's pairing on the host (the rule of k_icm_pair_ladders): did a pair that moved join two waves?
    P, half, lo, hi = 64 // L, K // 2, int(seed) & 0xFFFFFFFF, int(seed) >> 32
    cross = False
    for r in range(L if half else 0):
        key = [int(oracle.philox(j, 0, r, 6, lo, hi)[0]) for j in range(K)]
        sh = sorted(range(K), key=lambda j: (key[j], j))
        for i in range(half):
            cross |= bool(sh[2 * i] // P != sh[2 * i + 1] // P and a["info"][0, r * half + i, 1] > 0)
    a["cross"], a["n"], a["katz"], a["start"] = cross, N, katz, start
    return a


# name -> (arguments of four_runs after `product`, as a function of product), both precisions unless the name ends in a precision
def _wishart(p):
    J, h, _, _ = wishart(p)
    return J, h


def _fields16(p):
    return dense_instance(16, seed=8)


def _perm_slots(K, L):
    r = np.random.default_rng(17)
    return np.concatenate([r.permutation(L) for _ in range(K)])


CASES = {
    "wishart10_K10_L4": lambda p, prec: dict(a=(*_wishart(p), 10, 4, 2, 6, prec), k=dict(oracle_run=True)),
    "complete16_K10_L16_katz": lambda p, prec: dict(a=(*_fields16(p), 10, 16, 2, 4, prec), k=dict(oracle_run=True, katz=True)),
    "complete16_K10_L16_plain": lambda p, prec: dict(a=(*_fields16(p), 10, 16, 2, 4, prec), k=dict(katz=False)),
    "chimera128_K10_L8": lambda p, prec: dict(a=(*chimera128(p), 10, 8, 2, 3, prec), k=dict(betas=np.geomspace(1.0, 3.0, 8))),
    "ring33_K4_L2": lambda p, prec: dict(a=(*permuted_ring(33, 5), 4, 2, 1, 4, prec), k=dict(exact=True, betas=[0.4, 0.9])),
    "K3_L5": lambda p, prec: dict(a=(*dense_instance(12, seed=4), 3, 5, 2, 4, prec), k={}),
    "K2_L5": lambda p, prec: dict(a=(*dense_instance(12, seed=4), 2, 5, 2, 4, prec), k={}),
    "K1_L5": lambda p, prec: dict(a=(*dense_instance(12, seed=4), 1, 5, 2, 4, prec), k={}),
    "wishart10_K10_L64": lambda p, prec: dict(a=(*_wishart(p), 10, 64, 1, 3, prec), k={}),
    "diag_and_zero_K6_L5": lambda p, prec: dict(a=(diag_and_zero(p), None, 6, 5, 2, 4, prec), k={}),
    "permuted_start_K10_L4": lambda p, prec: dict(a=(*_wishart(p), 10, 4, 2, 6, prec), k=dict(slots0=_perm_slots(10, 4))),
    "no_swaps_K10_L4": lambda p, prec: dict(a=(*_wishart(p), 10, 4, 2, 5, prec), k=dict(pairs=0)),
    "shifted_delta_K6_L6": lambda p, prec: dict(a=(*sf.member("pmJ_2m10_h", 40)[:2], 6, 6, 2, 4, prec),
                                                k=dict(exact=True, betas=sf.member("pmJ_2m10_h", 40)[2] * np.geomspace(0.4, 1.6, 6))),
    "negative_scale_K6_L6": lambda p, prec: dict(a=(*sf.member("x1e9", 40)[:2], 6, 6, 2, 4, prec),
                                                 k=dict(betas=sf.member("x1e9", 40)[2] * np.geomspace(0.4, 1.6, 6))),
}
PARAMS = [(name, prec) for name in CASES for prec in ("f32", "f64")]


def run_case(product, name, prec):
    if (name, prec) not in _KEPT:
        c = CASES[name](product, prec)
        _KEPT[(name, prec)] = four_runs(product, *c["a"], **c["k"])
    return _KEPT[(name, prec)]


@pytest.mark.parametrize("name,prec", PARAMS)
def test_case(product, name, prec):
    """wishart10_K10_L4: one wave with tail lanes.  complete16_K10_L16: three waves, the last partly filled, with and without the
    Katzgraber flip.  chimera128: sparse, many components, the pick matters.  ring33: several label passes, n no multiple of 4.
    K = 3 leaves a ladder unpaired per slot, K = 1 has no Houdayer pair.  L = 64: ten waves of one ladder.  shifted_delta: couplings
    of 2^-10 (scalefamily pmJ_2m10_h: qs 13, escale 42), the energy deltas are shifted by escale - qs = 29 bits.  negative_scale:
    Gaussian couplings of 1e9 (scalefamily x1e9: qs = -7), not exact, under energy_tolerance."""
    a = run_case(product, name, prec)
    if name == "negative_scale_K6_L6":
        csr = oracle.Csr(sf.member("x1e9", 40)[0])
        assert oracle.field_scale(csr, sf.member("x1e9", 40)[1])[0] == -7
    if name == "shifted_delta_K6_L6":
        assert sf.PINNED["pmJ_2m10_h"][1] - sf.PINNED["pmJ_2m10_h"][0] > 0
    if name == "permuted_start_K10_L4":
        assert not np.array_equal(a["start"], np.arange(40) % 4)
    if name == "K1_L5":
        assert a["info"].shape == (4, 0, 2)


@pytest.mark.parametrize("rng", ["0", "1"])
def test_chimera_with_and_without_the_random_number_table(product, monkeypatch, rng):
    """NLMC_LANE_RNG (read when the engine is created): the Philox call per update, or the table per sweep that shares its bytes with
    the label plane."""
    monkeypatch.setenv("NLMC_LANE_RNG", rng)
    c = CASES["chimera128_K10_L8"](product, "f32")
    got = four_runs(product, *c["a"], **c["k"])                # (not kept: the engine of this run read the variable)
    ref = run_case(product, "chimera128_K10_L8", "f32")
    for k in ("spins", "energy", "slots", "info", "acc"):
        assert np.array_equal(got[k], ref[k]), k


def test_cut_calls_and_several_launches_per_call(product, monkeypatch):
    """Rounds 4 + 3 in two calls; then NLMC_LANE_SCRATCH of two rounds' visiting orders: the call of 7 rounds is 4 launches.  The order
    buffer holds one launch's orders, so a launch with a wrong first sweep, first round, plan row, log row or info row cannot give
    the bits of the uncut call."""
    J, h = dense_instance(16, seed=8)
    T, N = 2, 16
    whole = four_runs(product, J, h, 10, 16, T, 7, "f32")
    keys = ("spins", "energy", "slots", "info", "pairs", "acc")
    cut = four_runs(product, J, h, 10, 16, T, 7, "f32", cuts=[4, 3])
    for k in keys:
        assert np.array_equal(whole[k], cut[k]), ("cut", k)
    monkeypatch.setenv("NLMC_LANE_SCRATCH", str(2 * T * N * 2))
    small = four_runs(product, J, h, 10, 16, T, 7, "f32")
    for k in keys:
        assert np.array_equal(whole[k], small[k]), ("four launches", k)


def test_no_path_stayed_unvisited(product):
    """Over the case set: moves happened, some pair had several components, Katzgraber flips and exchanges both happened, swaps
    were accepted, and a Houdayer pair that moved joined columns of two different waves."""
    runs = {(n, p): run_case(product, n, p) for n, p in PARAMS}
    info = {k: v["info"].reshape(-1, 2) for k, v in runs.items()}
    assert sum(int((i[:, 1] > 0).sum()) for i in info.values()) > len(info)
    assert any((i[:, 0] > 1).any() for i in info.values())
    assert (info[("chimera128_K10_L8", "f32")][:, 0] > 3).any()                     # many components: the pick matters
    flips = sum(int((i[:, 1] > runs[k]["n"] // 2).sum()) for k, i in info.items() if runs[k]["katz"])
    exchanges = sum(int(((i[:, 1] > 0) & (i[:, 1] <= runs[k]["n"] // 2)).sum()) for k, i in info.items())
    unflipped = int((info[("complete16_K10_L16_plain", "f32")][:, 1] > 8).sum())   # large clusters exchanged where katzgraber is off
    assert flips > 0 and exchanges > 0 and unflipped > 0, (flips, exchanges, unflipped)
    assert sum(int(v["acc"].sum()) for v in runs.values() if "acc" in v) > len(runs)
    assert any(not np.array_equal(v["slots"], v["start"]) for v in runs.values())
    assert runs[("complete16_K10_L16_katz", "f32")]["cross"] and runs[("wishart10_K10_L64", "f32")]["cross"]
    assert not runs[("wishart10_K10_L4", "f32")]["cross"]                          # one wave: nothing to cross


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def refused(eng, L, T, why, m0, prepare=None, pairs=None, rounds=3):
    """apt_rounds_lanes answers (False, None) with a reason, runs nothing and leaves the rounds route as it was."""
    pairs = n_pairs_of(L) if pairs is None else pairs
    eng.pt_init(np.geomspace(0.3, 1.5, L))
    eng.set_spins(m0)
    if pairs > 0:
        eng.pt_plan(0, rounds, SEED, pairs)
    if prepare:
        prepare(eng)
    before = (eng.get_spins(), eng.energy_tracked(), eng.pt_slots(), eng.last_rounds_route())
    eng.rounds_fused_refusal = None
    assert eng.apt_rounds_lanes(rounds, T, SEED, 0, 0, pairs, want_info=True) == (False, None)
    assert eng.rounds_fused_refusal.startswith("nlmc_apt_rounds_lanes: ") and why in eng.rounds_fused_refusal, eng.rounds_fused_refusal
    after = (eng.get_spins(), eng.energy_tracked(), eng.pt_slots(), eng.last_rounds_route())
    assert all(np.array_equal(x, y) for x, y in zip(before[:3], after[:3])) and before[3] == after[3] is None


def test_refusals(product):
    J, h = make_instance(37, seed=9, with_h=True, gaussian=True)
    N = 37
    m0 = init_spins(10, N)
    J2, h2 = make_instance(1025, seed=3)
    with product.Engine(J2, h2, 10) as eng:
        refused(eng, 5, 1, "NLMC_LANE_N", init_spins(10, 1025))
    with product.Engine(J, h, 10) as eng:
        refused(eng, 5, 2, "phase flags", m0, prepare=lambda e: e.set_flags(nmc_flags(10, N, m0)))
    with product.Engine(J, h, 10) as eng:
        def subset(e):
            e.mark_slots(np.arange(5) == 1)
            e.select("marked")
        refused(eng, 5, 2, "chain subset", m0, prepare=subset)
    with product.Engine(J, h, 10) as eng:
        refused(eng, 5, 2, "tracked minimum", m0, prepare=lambda e: e.track_minimum(True))
    with product.Engine(J, h, 10, chain_base=5, n_chains_global=15) as eng:
        refused(eng, 5, 2, "one context", m0)
    with product.Engine(J, h, 10) as eng:
        refused(eng, 5, 2, "temperature slot", m0, prepare=lambda e: e.apt_shard(np.geomspace(0.3, 1.5, 5), 1, 0))
    with product.Engine(J, h, 40 * 33) as eng:
        refused(eng, 33, 1, "16 waves", init_spins(40 * 33, N))
    J3, h3 = make_instance(1000, seed=4)
    with product.Engine(J3, h3, 160) as eng:
        refused(eng, 16, 1, "LDS", init_spins(160, 1000))
    with product.Engine(J, h, 10) as eng:                      # not planned: refused as by pt_rounds_lanes; without swaps nothing to plan
        eng.pt_init(np.geomspace(0.3, 1.5, 5))
        eng.set_spins(m0)
        assert eng.apt_rounds_lanes(2, 1, SEED, 0, 0, 1) == (False, None) and "not planned" in eng.rounds_fused_refusal
        assert eng.apt_rounds_lanes(2, 1, SEED, 0, 0, 0)[0] is True


# ---- the class -------------------------------------------------------------------------------------------------------------------------
def test_apt_icm_lanes_keyword(product, monkeypatch):
    """APT_ICM(lanes="force") on the Wishart N = 10 instance, 10 sub-replicas of a 6-rung ladder: the results of lanes="off", with
    rounds 0 .. 6 of 8 in one apt_rounds_lanes call."""
    calls = []
    orig = product.engine.Engine.apt_rounds_lanes

    def wrapped(self, n_rounds, *a, **k):
        ok, info = orig(self, n_rounds, *a, **k)
        calls.append((int(n_rounds), bool(ok), self.last_rounds_route() if ok else None))
        return ok, info
    monkeypatch.setattr(product.engine.Engine, "apt_rounds_lanes", wrapped)
    monkeypatch.setattr(product.engine, "APT_LANES_IN_LAUNCH", True)       # the route under test, whatever the measured default is
    Jn, h, _, _ = wishart(product)

    def run(lanes):
        obj = product.APT_ICM(Jn, h, rng="philox", seed=0x9E370001 + (5 << 32), lanes=lanes)
        with contextlib.redirect_stdout(io.StringIO()):
            M, E = obj.run(np.geomspace(0.4, 1.6, 6), 6, num_sweeps_MCMC=24, num_sweeps_read=24, num_swap_attempts=8,
                           num_swapping_pairs=2, icm_feedback=True, return_trace="int8")
        return {"M": M, "Energy": E, "swap_accepted": obj.swap_accepted, "icm_cluster_sizes": obj.icm_cluster_sizes,
                "final_slots": obj.final_slots, "final_energies": obj.final_energies}
    got = run("force")
    assert calls == [(7, True, "apt lanes")]
    del calls[:]
    ref = run("off")
    assert not calls
    for k in got:
        assert np.array_equal(got[k], ref[k]), k
    assert got["swap_accepted"].sum() > 0 and (got["icm_cluster_sizes"] > 0).any()
    assert not np.array_equal(got["final_slots"], np.arange(60) % 6)
