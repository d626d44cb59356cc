"""Many independent APT systems in one context (include/nlmc.h: nlmc_apt_systems), the parts that need no GPU: the helper
tests/aptsystems.py against the single-system oracle double and against the definition, the seed of the GPU cases, APT_ICM's
num_restarts over the helper through the engine_factory seam, the keyword's refusals, and the export."""
import contextlib
import ctypes
import functools
import io
import re

import numpy as np
import pytest

import aptsystems as aps
from conftest import load_product
from fake_engine import OracleEngine
from helpers import make_instance, init_spins
from test_lanes_cpu import header

SEED = aps.SEED


def _pair(cls, inst, G, L, M=None):
    e = cls(inst, G, 0, G)
    e.pt_init(np.geomspace(0.4, 1.4, L))
    if M is not None:
        e.apt_systems(M)
    e.set_spins(init_spins(G, inst.n))
    return e


def test_one_system_is_the_single_system_double():
    """M = 1: the helper's Houdayer step equals OracleEngine.icm_round_ladders bit for bit, rounds of sweeps and swaps in between.
    Couplings +-1 and fields that are multiples of 1/8: the fixed-point model is exact there, so the double's recomputed energies and
    the helper's integer deltas are the same numbers (on other instances the helper follows the kernels, the double the true J)."""
    P = load_product()
    J, h = make_instance(14, seed=6, with_h=True)
    h = np.rint(8 * h) / 8
    assert h.any()
    inst = P.Instance(J, h)
    K, L = 5, 3
    a, b = _pair(OracleEngine, inst, K * L, L), _pair(aps.SystemsOracleEngine, inst, K * L, L, M=1)
    moved = 0
    for r in range(4):
        for e in (a, b):
            e.sweep_philox(2, SEED, sweep0=2 * r)
        ia, ib = a.icm_round_ladders(r, SEED, True, want_info=True), b.icm_round_ladders(r, SEED, True, want_info=True)
        assert np.array_equal(ia, ib) and ia.shape == (L * (K // 2), 2)
        moved += int((ia[:, 1] > 0).sum())
        for e in (a, b):
            e.pt_swap_philox(r, SEED, 1)
        assert np.array_equal(a.spins, b.spins) and np.array_equal(a.efix, b.efix) and np.array_equal(a.slots, b.slots)
    assert moved > 0 and not np.array_equal(a.slots, np.arange(K * L) % L)


def test_pairs_stay_inside_their_system():
    """M = 3, K = 5, L = 3: no pair crosses a system, every chain is in at most one pair, exactly one ladder per (system, slot) sits
    out; the rows come in the order (system, slot, i); after swaps the pair is still the two holders of one slot."""
    P = load_product()
    J, h = make_instance(14, seed=6, with_h=True)
    M, K, L = 3, 5, 3
    e = _pair(aps.SystemsOracleEngine, P.Instance(J, h), M * K * L, L, M=M)
    for r in range(3):
        e.sweep_philox(1, SEED, sweep0=r)
        rows = e.pairing(r, SEED)
        assert [(s, sl, i) for s, sl, i, _, _ in rows] == [(s, sl, i) for s in range(M) for sl in range(L) for i in range(K // 2)]
        chains = [c for row in rows for c in row[3:]]
        assert len(set(chains)) == len(chains) == M * L * 2 * (K // 2)
        for s, sl, _, ca, cb in rows:
            assert ca // (K * L) == cb // (K * L) == s and ca // L != cb // L
            assert e.slots[ca] == e.slots[cb] == sl
        for s in range(M):
            for sl in range(L):
                holders = {c // L for c in range(s * K * L, (s + 1) * K * L) if e.slots[c] == sl}
                paired = {c // L for row in rows if row[0] == s and row[1] == sl for c in row[3:]}
                assert len(holders) == K and len(holders - paired) == 1
        e.icm_round_ladders(r, SEED)
        e.pt_swap_philox(r, SEED, 1)
    assert not np.array_equal(e.slots, np.arange(M * K * L) % L)


def test_system_zero_of_the_helper_is_a_one_system_run():
    P = load_product()
    case = aps.ORACLE_CASES["wishart10_M3_K4_L3_f32"]
    name, M, K, L, rounds, prec = case
    many, one = aps.oracle_case(P, case), aps.oracle_case(P, (name, 1, K, L, rounds, prec))
    G1, NP1 = K * L, L * (K // 2)
    assert np.array_equal(many["spins"][:G1], one["spins"]) and np.array_equal(many["efix"][:G1], one["efix"])
    assert np.array_equal(many["slots"][:G1], one["slots"]) and np.array_equal(many["info"][:, :NP1], one["info"])
    assert np.array_equal(many["acc"][:, :K], one["acc"]) and np.array_equal(many["pairs"][:, :K], one["pairs"])
    assert not np.array_equal(many["spins"][G1:2 * G1], one["spins"])


@pytest.mark.parametrize("name", list(aps.ORACLE_CASES) + list(aps.LAUNCH_CASES))
def test_the_seed_meets_the_conditions_on_the_helper_alone(name):
    """Every equality case of tests/test_gpu_apt_systems.py: every system has a pair with components over the rounds, a swap is
    accepted, a moved pair is not a global flip."""
    P = load_product()
    assert aps.SEED >> 32
    case = aps.ORACLE_CASES.get(name) or aps.LAUNCH_CASES[name]
    o = aps.oracle_case(P, case)
    assert o["info"].shape == (case[4], case[1] * case[3] * (case[2] // 2), 2)
    assert aps.conditions(o["info"], o["acc"], case[1], o["n"]) == []


# ---- APT_ICM(num_restarts=...) over the helper -----------------------------------------------------------------------------------------
def run_class(P, monkeypatch, restarts, rounds=4, **kw):
    N, R, S = 12, 3, 2
    J, h = make_instance(N, seed=5, with_h=True)
    obj = P.APT_ICM(J, h, rng="philox", seed=SEED)
    obj.num_subreplicas = 4                                    # (the class attribute is 10: four keep the oracle's run short)
    monkeypatch.setattr(obj, "_run_device_resident", functools.partial(obj._run_device_resident, engine_factory=aps.RunEngine))
    del aps.RunEngine.made[:]
    with contextlib.redirect_stdout(io.StringIO()):
        M, E = obj.run(np.geomspace(0.4, 1.4, R), R, num_sweeps_MCMC=S * rounds, num_sweeps_read=S * rounds, num_swap_attempts=rounds,
                       num_swapping_pairs=1, icm_feedback=True, **({} if restarts is None else dict(num_restarts=restarts)), **kw)
    (eng,) = aps.RunEngine.made
    return obj, M, E, eng


def test_restart_zero_does_not_depend_on_the_number_of_restarts(monkeypatch):
    P = load_product()
    o1, M1, E1, e1 = run_class(P, monkeypatch, None)
    o3, M3, E3, e3 = run_class(P, monkeypatch, 3)
    K, R, G1 = 4, 3, 12
    assert e1.n_systems == 1 and e1.n_chains == G1 and e3.n_systems == 3 and e3.n_chains == 3 * G1
    assert M1.any() and np.array_equal(M1, M3) and np.array_equal(E1, E3)
    assert o1.restart_energies.shape == (1, R) and np.array_equal(o1.restart_energies[0], E1)
    assert o3.restart_energies.shape == (3, R) and np.array_equal(o3.restart_energies[0], E3)
    assert len({tuple(row) for row in o3.restart_energies}) > 1                    # the other restarts are other runs
    assert o3.final_energies.shape == o3.final_slots.shape == (3 * G1,)
    assert np.array_equal(o3.final_slots[:G1], o1.final_slots) and np.array_equal(o3.final_energies[:G1], o1.final_energies)
    rounds = 4
    assert o3.swap_accepted.shape == (rounds * 3 * K,) and o3.icm_cluster_sizes.shape == (rounds * 3 * R * (K // 2),)
    assert np.array_equal(o3.swap_accepted.reshape(rounds, 3 * K)[:, :K].reshape(-1), o1.swap_accepted) and o1.swap_accepted.sum() > 0
    assert np.array_equal(o3.icm_cluster_sizes.reshape(rounds, 3, -1)[:, 0].reshape(-1), o1.icm_cluster_sizes)
    assert (o1.icm_cluster_sizes > 0).any()
    # chain id = (s K + j) R + holder: the start states of restart s are rows s K R .. of the one (G, N) draw
    draw = 2 * np.random.default_rng(SEED).integers(0, 2, size=(3 * G1, 12), dtype=np.int8) - 1
    assert np.array_equal(draw[:G1], 2 * np.random.default_rng(SEED).integers(0, 2, size=(G1, 12), dtype=np.int8) - 1)


def test_num_restarts_is_refused_off_the_device_resident_path():
    P = load_product()
    J, h = make_instance(16, seed=2)
    kw = dict(num_sweeps_MCMC=4, num_sweeps_read=4, num_swap_attempts=2)
    b = np.linspace(0.5, 1.0, 3)
    with pytest.raises(ValueError, match="num_restarts"):
        P.APT_ICM(J, h, rng="numpy").run(b, 3, num_restarts=2, **kw)
    obj = P.APT_ICM(J, h, rng="philox", seed=1)
    with pytest.raises(ValueError, match="num_restarts"):
        obj.run(b, 3, icm_feedback=False, num_restarts=2, **kw)
    with pytest.raises(ValueError, match="num_restarts"):
        obj.run(b, 3, icm_feedback=True, device_ids=[0], num_restarts=2, **kw)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="num_restarts"):
            obj.run(b, 3, icm_feedback=True, num_restarts=bad, **kw)


# ---- header, binding, exports --------------------------------------------------------------------------------------------------------
def test_the_export_is_in_the_header_the_library_and_the_binding():
    P = load_product()
    L = P._abi.lib()
    assert re.search(r"int\s+nlmc_apt_systems\s*\(\s*nlmc_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", header())
    assert "nlmc_apt_systems" in P._abi.EXPORTS and hasattr(L, "nlmc_apt_systems")
    f = L.nlmc_apt_systems
    assert f.restype is ctypes.c_int and f.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert f(None, 2) == P._abi.ERR_ARG                       # a NULL context: before any device work
    assert hasattr(P.Engine, "apt_systems") and P.Engine.n_systems == 1
