"""Many independent APT systems in one context and launch (include/nlmc.h: nlmc_apt_systems): a context of M K ladders whose Houdayer
pairing stays inside each system of K ladders.

Round by round (sweep_philox + icm_round_ladders + pt_swap_philox) against the helper tests/aptsystems.py -- spins, tracked energies,
slots, the {components, picked size} of every pair and the swap log, bit for bit; system 0 against a one-system engine; the pairing kernel
for K above a workgroup's threads; the global-memory kernel; the rounds inside k_apt_rounds_lanes launches, a workgroup per system,
against the round-by-round route; APT_ICM(num_restarts=...); the refusals.  States start from init_spins, the seed has high bits set,
pairs = max(1, L // 3).

So that no equality holds vacuously every equality case asserts aptsystems.conditions on what the device returned: every system has a
pair with n_components > 0 over the rounds, a swap is accepted (where the case has swaps), a moved pair is not a global flip."""
import contextlib
import io

import numpy as np
import pytest

import aptsystems as aps
from aptsystems import SEED, SWEEPS, n_pairs_of
from helpers import init_spins
from test_gpu_apt_lanes import energy_tolerance

pytestmark = pytest.mark.gpu
KEYS = ("spins", "energy", "slots", "info", "pairs", "acc")
_KEPT = {}


def setup_case(product, case):
    name, M, K, L, rounds, prec = case
    J, h, betas = aps.instance(product, name)
    inst = product.Instance(J, h)
    return inst, betas(L), init_spins(M * K * L, inst.n)


def begin(eng, M, betas, m0, rounds, pairs, mode="off"):
    eng.set_lane_sweeps(mode)
    eng.pt_init(betas)
    eng.apt_systems(M)
    eng.set_spins(m0)
    if pairs > 0:
        eng.pt_plan(0, rounds, SEED, pairs)
        eng.pt_log_begin(0, rounds, pairs)


def state(eng, info, pairs, tol=None):
    s = {"spins": eng.get_spins(), "energy": eng.energy_tracked(), "slots": eng.pt_slots(), "info": info, "pairs": None, "acc": None}
    if pairs > 0:
        eng.pt_check()
        s["pairs"], s["acc"] = eng.pt_log_read()
    if tol is not None:
        err = float(np.max(np.abs(s["energy"] - eng.energy())))
        print("tracked energies against a recomputation:", err, "tolerance", tol)
        assert err <= tol, (err, tol)
    return s


def by_round(product, case, mode="off", pairs=None, M=None, chains=None):
    """The round-by-round route of a case -> state; M / chains: another division of (the first chains of) the same start."""
    name, M0, K, L, rounds, prec = case
    inst, betas, m0 = setup_case(product, case)
    M = M0 if M is None else M
    G = M * K * L if chains is None else chains
    pairs = n_pairs_of(L) if pairs is None else pairs
    with product.Engine(inst, None, G) as eng:
        begin(eng, M, betas, m0[:G], rounds, pairs, mode)
        efix0 = np.rint(eng.energy_tracked() * 2.0 ** eng.energy_scale).astype(np.int64)    # (exact: a rounded fp64 energy)
        infos = []
        for r in range(rounds):
            eng.sweep_philox(SWEEPS, SEED, sweep0=r * SWEEPS, beta=None, precision=prec)
            assert (eng.last_sweep_route() == "lanes") == (mode == "force")
            infos.append(eng.icm_round_ladders(r, SEED, True, want_info=True))
            if pairs > 0:
                eng.pt_swap_philox(r, SEED, pairs, want_log=False)
        s = state(eng, np.stack(infos), pairs)
    s["efix0"] = efix0
    assert s["info"].shape == (rounds, M * L * (K // 2), 2)
    return s


def kept(product, case):
    if case not in _KEPT:
        _KEPT[case] = by_round(product, case)
    return _KEPT[case]


def same(x, y, what, keys=KEYS):
    for k in keys:
        assert (x[k] is None) == (y[k] is None), (what, k)
        assert x[k] is None or np.array_equal(x[k], y[k]), (what, k)


def meets(s, case, n, swaps=True):
    bad = aps.conditions(s["info"], s["acc"], case[1], n)
    assert [b for b in bad if swaps or b != "no swap accepted"] == [], bad


# ---- round by round against the helper -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(aps.ORACLE_CASES))
def test_round_by_round_against_the_helper(product, name):
    """Wishart N = 10 with (M, K, L) = (3, 4, 3) in both precisions and (2, 5, 6), odd K; Chimera-128 with (2, 4, 3); and (2, 258, 2):
    K above the 256 threads of k_icm_round's workgroup, the pairing is made by k_icm_pair_ladders (one round)."""
    case = aps.ORACLE_CASES[name]
    got = kept(product, case)
    ref = aps.oracle_case(product, case, efix0=got["efix0"])  # (the helper starts from the engine's own start energies)
    for k in KEYS:
        print(name, k, "entries that differ:", int(np.sum(np.asarray(got[k]) != np.asarray(ref[k]))), "of", np.asarray(got[k]).size)
    same(got, ref, name)
    meets(got, case, ref["n"])


def test_system_zero_equals_a_one_system_engine(product):
    """Same instance and seed, G = K L chains: every array of system 0 is equal (no oracle in this check), and system 1 is another run."""
    case = aps.ORACLE_CASES["wishart10_M3_K4_L3_f32"]
    _, M, K, L, rounds, _ = case
    many = kept(product, case)
    one = by_round(product, case, M=1, chains=K * L)
    G1, NP1 = K * L, L * (K // 2)
    for k in ("spins", "energy", "slots"):
        assert np.array_equal(many[k][:G1], one[k]), k
    assert np.array_equal(many["info"][:, :NP1], one["info"])
    assert np.array_equal(many["pairs"][:, :K], one["pairs"]) and np.array_equal(many["acc"][:, :K], one["acc"])
    assert not np.array_equal(many["spins"][G1:2 * G1], one["spins"])
    meets(many, case, 10)
    meets(one, (None, 1), 10)


def test_global_memory_kernel_equals_the_lds_kernel(product, monkeypatch):
    """NLMC_FORCE_BIG (read when the context is created): k_icm_round_big pairs by system as k_icm_round does."""
    case = aps.ORACLE_CASES["wishart10_M3_K4_L3_f32"]
    ref = kept(product, case)
    monkeypatch.setenv("NLMC_FORCE_BIG", "1")
    got = by_round(product, case)
    same(got, ref, "global-memory kernel")
    meets(got, case, 10)


# ---- the rounds in one launch, a workgroup per system ----------------------------------------------------------------------------------
def in_launch(product, case, cuts=None, pairs=None):
    name, M, K, L, rounds, prec = case
    inst, betas, m0 = setup_case(product, case)
    pairs = n_pairs_of(L) if pairs is None else pairs
    with product.Engine(inst, None, M * K * L) as eng:
        begin(eng, M, betas, m0, rounds, pairs)
        tol = energy_tolerance(inst, eng.field_scale, eng.energy_scale, False, rounds * (SWEEPS + 1) * inst.n)
        at, infos = 0, []
        for k in cuts or [rounds]:
            ok, info = eng.apt_rounds_lanes(k, SWEEPS, SEED, at * SWEEPS, at, pairs, precision=prec, want_info=True)
            assert ok, getattr(eng, "rounds_fused_refusal", "")
            assert eng.last_rounds_route() == "apt lanes" and eng.last_sweep_route() == "lanes"
            assert info.shape == (k, M * L * (K // 2), 2)
            infos.append(info)
            at += k
        return state(eng, np.concatenate(infos), pairs, tol=tol)


@pytest.mark.parametrize("name", list(aps.LAUNCH_CASES))
def test_in_launch_equals_round_by_round(product, name):
    """(3, 4, 3); (2, 12, 6): two waves per system, the second with tail lanes; (300, 2, 3): more workgroups than compute units.  The
    tracked energies of the launch are also compared with eng.energy() (tolerance of test_gpu_apt_lanes.energy_tolerance)."""
    case = aps.LAUNCH_CASES[name]
    got, ref = in_launch(product, case), kept(product, case)
    same(got, ref, name)
    meets(got, case, 10)
    if name == "wishart10_M2_K12_L6":
        assert 64 // 6 < 12 <= 2 * (64 // 6) and (12 - 64 // 6) * 6 < 64


def test_a_call_cut_into_two_launches(product):
    """cuts = [1, 3]: the second launch starts at round 1 -- its first sweep, round, plan row, log row and info row."""
    case = aps.LAUNCH_CASES["wishart10_M3_K4_L3"]
    got = in_launch(product, case, cuts=[1, 3])
    same(got, kept(product, case), "cut")
    meets(got, case, 10)


def test_in_launch_without_swaps(product):
    """n_pairs = 0 (no swap can be accepted: the other two conditions hold)."""
    case = aps.LAUNCH_CASES["wishart10_M3_K4_L3"]
    got, ref = in_launch(product, case, pairs=0), by_round(product, case, pairs=0)
    same(got, ref, "no swaps")
    assert got["acc"] is None and np.array_equal(got["slots"], np.arange(36) % 3)
    meets(got, case, 10, swaps=False)


# ---- the class -------------------------------------------------------------------------------------------------------------------------
def run_api(product, restarts, lanes="off", **kw):
    J, h, _ = aps.instance(product, "wishart10")
    obj = product.APT_ICM(J, h, rng="philox", seed=SEED, lanes=lanes)
    with contextlib.redirect_stdout(io.StringIO()):
        M, E = obj.run(np.geomspace(0.4, 1.6, 6), 6, num_sweeps_MCMC=12, num_sweeps_read=12, num_swap_attempts=6, num_swapping_pairs=2,
                       icm_feedback=True, return_trace="int8", **({} if restarts is None else dict(num_restarts=restarts)), **kw)
    return obj, M, E


def test_apt_icm_num_restarts(product, monkeypatch):
    """Restart 0 of num_restarts = 3 equals num_restarts = 1 in M and Energy; the shapes of every attribute; each restart's best
    energy is the minimum over its chains; lanes="force" with the in-launch route gives the same bits."""
    K, R, N, rounds, S = product.APT_ICM.num_subreplicas, 6, 10, 6, 2
    G1 = K * R
    o1, M1, E1 = run_api(product, None)
    o3, M3, E3 = run_api(product, 3)
    assert M1.shape == (N * R, S * K) and M1.any() and np.array_equal(M1, M3) and np.array_equal(E1, E3)
    assert o1.restart_energies.shape == (1, R) and o3.restart_energies.shape == (3, R)
    assert np.array_equal(o3.restart_energies[0], E3) and len({tuple(r) for r in o3.restart_energies}) > 1
    assert o3.final_energies.shape == o3.final_slots.shape == (3 * G1,)
    assert o3.swap_accepted.shape == (rounds * 3 * K * 2,) and o3.icm_cluster_sizes.shape == (rounds * 3 * R * (K // 2),)
    assert np.array_equal(o3.final_slots[:G1], o1.final_slots) and np.array_equal(o3.final_energies[:G1], o1.final_energies)
    assert np.array_equal(o3.swap_accepted.reshape(rounds, 3 * K, 2)[:, :K].reshape(-1), o1.swap_accepted)
    assert np.array_equal(o3.icm_cluster_sizes.reshape(rounds, 3, -1)[:, 0].reshape(-1), o1.icm_cluster_sizes)
    assert o3.swap_accepted.sum() > 0 and all((o3.icm_cluster_sizes.reshape(rounds, 3, -1)[:, s] > 0).any() for s in range(3))

    target = float(np.sort(o3.final_energies)[len(o3.final_energies) // 2])
    ob, Mb, Eb = run_api(product, 3, track_best=True, target_energy=target)
    assert np.array_equal(Mb, M3) and np.array_equal(Eb, E3)
    assert ob.best_energy.shape == ob.best_round.shape == ob.first_hit_round.shape == (3 * G1,) and ob.best_state.shape == (3 * G1, N)
    assert ob.restart_best_energy.shape == ob.restart_first_hit_round.shape == (3,)
    for s in range(3):
        blk = slice(s * G1, (s + 1) * G1)
        assert ob.restart_best_energy[s] == ob.best_energy[blk].min()
        hits = ob.first_hit_round[blk][ob.first_hit_round[blk] >= 0]
        assert ob.restart_first_hit_round[s] == (hits.min() if hits.size else -1)
    assert (ob.restart_first_hit_round >= 0).any()

    calls = []
    orig = product.engine.Engine.apt_rounds_lanes

    def wrapped(self, n_rounds, *a, **k):
        ok, info = orig(self, n_rounds, *a, **k)
        calls.append((int(n_rounds), bool(ok), self.n_systems))
        return ok, info
    monkeypatch.setattr(product.engine.Engine, "apt_rounds_lanes", wrapped)
    monkeypatch.setattr(product.engine, "APT_LANES_IN_LAUNCH", True)       # the route under test, whatever the measured default is
    of, Mf, Ef = run_api(product, 3, lanes="force")
    assert calls == [(rounds - 1, True, 3)]
    assert np.array_equal(Mf, M3) and np.array_equal(Ef, E3) and np.array_equal(of.restart_energies, o3.restart_energies)
    for k in ("final_energies", "final_slots", "swap_accepted", "icm_cluster_sizes"):
        assert np.array_equal(getattr(of, k), getattr(o3, k)), k


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(product):
    J, h, _ = aps.instance(product, "wishart10")
    betas = np.geomspace(0.3, 1.5, 3)
    with product.Engine(J, h, 12) as eng:
        with pytest.raises(RuntimeError, match="nlmc_pt_init first"):
            eng.apt_systems(2)
        eng.pt_init(betas)
        for bad in (0, -2, 3, 8):                             # 4 ladders
            with pytest.raises(ValueError, match="divide the number of ladders"):
                eng.apt_systems(bad)
        assert eng.n_systems == 1
        eng.apt_systems(2)
        with pytest.raises(NotImplementedError, match="several systems"):
            eng.apt_shard(betas, 1, 0)
        eng.pt_init(betas)                                    # resets to one system: the shard is taken, and then refuses systems
        assert eng.n_systems == 1
        eng.apt_shard(betas, 1, 0)
        with pytest.raises(NotImplementedError, match="temperature slot"):
            eng.apt_systems(2)
        eng.apt_systems(1)
        assert eng.icm_round_ladders(0, SEED, want_info=True).shape == (3 * 2, 2)
