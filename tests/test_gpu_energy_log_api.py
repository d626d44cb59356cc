"""track_energies through the classes: NPT.run and APT_ICM.run keep, for every round, every chain's tracked energy and temperature
slot as that round's swap decision sees them, without a synchronisation inside the run.

The yardstick is the same run without the keyword, driven round by round (NLMC_NO_DEFERRED=1: LocalTempering.run_rounds falls back to
round(); APT_ICM with lanes="off" runs a call per step anyway) with read-backs: a spy on Engine.pt_swap_philox reads energy_tracked()
and pt_slots() right before every swap call.  round_energies / round_slots must equal it exactly; (M, Energy), the swap log and every
other attribute must equal the run without the keyword."""
import contextlib
import io

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import golden
from helpers import make_instance
from test_gpu_lanes import wishart

pytestmark = pytest.mark.gpu


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def golden_instance(name):
    g = golden(name)
    J = sp.csr_matrix((g["data"], g["indices"], g["indptr"]), shape=(int(g["N"]),) * 2).toarray()
    return J, np.asarray(g["h"], dtype=np.float64).reshape(-1)


@contextlib.contextmanager
def read_backs(product, seen):
    """Every Engine.pt_swap_philox call first appends (round, tracked energies, slots of the context's chains) to `seen`."""
    orig = product.engine.Engine.pt_swap_philox

    def spy(self, round_idx, *a, **k):
        seen.append((int(round_idx), self.energy_tracked(), self.pt_slots()[self.chain_base:self.chain_base + self.n_chains]))
        return orig(self, round_idx, *a, **k)
    product.engine.Engine.pt_swap_philox = spy
    try:
        yield
    finally:
        product.engine.Engine.pt_swap_philox = orig


@contextlib.contextmanager
def rounds_calls(product, calls):
    orig = product.engine.Engine.pt_rounds_deferred

    def spy(self, n_rounds, *a, **k):
        ok = orig(self, n_rounds, *a, **k)
        calls.append((int(n_rounds), self.last_rounds_route() if ok else None))
        return ok
    product.engine.Engine.pt_rounds_deferred = spy
    try:
        yield
    finally:
        product.engine.Engine.pt_rounds_deferred = orig


def stacked(seen, rounds):
    assert [r for r, _, _ in seen] == list(range(rounds))
    return np.stack([e for _, e, _ in seen]), np.stack([s for _, _, s in seen]).astype(np.int32)


NPT_ATTRS = ("swap_pairs", "swap_accepted", "final_slots", "restart_energies")


def npt_three_runs(product, monkeypatch, J, h, betas, doNMC, run_kw, lanes="off", seed=77):
    """-> (yardstick (E, slots), plain run, tracked run, batched calls of the tracked run); each run = (obj, M, Energy)."""
    R = len(betas)

    def run(**kw):
        obj = product.NPT(J, h, rng="philox", seed=seed, lanes=lanes)
        with quiet():
            M, Energy = obj.run(betas, R, list(doNMC), **run_kw, **kw)
        return obj, M, Energy
    seen = []
    monkeypatch.setenv("NLMC_NO_DEFERRED", "1")
    with read_backs(product, seen):
        run()
    monkeypatch.delenv("NLMC_NO_DEFERRED")
    plain = run()
    calls = []
    with rounds_calls(product, calls):
        tracked = run(track_energies=True)
    return stacked(seen, run_kw["num_swap_attempts"]), plain, tracked, calls


def same_npt_run(plain, tracked):
    assert np.array_equal(plain[1], tracked[1]) and np.array_equal(plain[2], tracked[2])
    for a in NPT_ATTRS:
        assert np.array_equal(getattr(plain[0], a), getattr(tracked[0], a)), a
    for x, y in zip(plain[0].swap_log_all, tracked[0].swap_log_all):
        assert np.array_equal(x, y)
    assert not hasattr(plain[0], "round_energies")


def check_report(obj, betas, rounds, n_reports, L):
    assert len(obj.ladder_report) == n_reports
    for rep in obj.ladder_report:
        assert rep["mean_energy"].shape == rep["sigma_energy"].shape == (L,) and rep["acceptance"].shape == (L - 1,)
        assert rep["n_rounds"] == rounds and (rep["swap_attempts"] == rounds - 1).all() and (rep["sigma_energy"] >= 0).all()
        assert np.array_equal(rep["beta"], betas)


@pytest.mark.parametrize("case", ["pmj40", "pmj301", "wishart10-lanes"])
def test_npt_run_track_energies_equals_round_by_round_read_backs(product, monkeypatch, case):
    """6 replicas x 2 restarts, 8 rounds of 6 sweeps.  pmj40: the fixture instance (40 spins, +-J with fields), lanes="off" -- too short
    for fused windows, so run_rounds runs every round on its call-per-step fallback with an explicit update.  pmj301: +-J of 301 spins,
    rounds 0..6 in one pt_rounds_deferred call (inside k_rounds_fused, or a launch per round), the last one through round().
    wishart10-lanes: Wishart N = 10 under lanes="force", the 7 rounds inside k_rounds_lanes."""
    lanes = "force" if case == "wishart10-lanes" else "off"
    if case == "pmj40":
        J, h = golden_instance("npt_run_pmj40_plain")
    elif case == "pmj301":
        J, h = make_instance(301, seed=21)
    else:
        J, h, _, _ = wishart(product)
    betas, rounds, S, restarts = np.linspace(0.5, 2.0, 6), 8, 6, 2
    kw = dict(num_sweeps_MCMC=S * rounds, num_sweeps_read=S * rounds, num_swap_attempts=rounds, num_swapping_pairs=2, num_restarts=restarts)
    (E, sl), plain, tracked, calls = npt_three_runs(product, monkeypatch, J, h, betas, [False] * 6, kw, lanes=lanes)
    if case == "pmj40":
        assert calls == []
    else:
        assert len(calls) == 1 and calls[0][0] == rounds - 1 and calls[0][1] in (("lanes",) if lanes == "force" else ("in launch", "launch per round"))
    obj = tracked[0]
    assert obj.round_energies.shape == obj.round_slots.shape == (rounds, 12) and obj.round_slots.dtype == np.int32
    assert np.array_equal(obj.round_energies, E) and np.array_equal(obj.round_slots, sl)
    assert (sl[1:] != sl[:-1]).any()
    same_npt_run(plain, tracked)
    check_report(obj, betas, rounds, restarts, 6)
    # the last row's slots and the run's last swap give the final slots: the log stops BEFORE the last swap
    moved = obj.final_slots != obj.round_slots[-1]
    assert moved.sum() == 2 * obj.swap_log_all[1][-1].sum()
    new = product.hostlogic.suggest_ladder(obj.ladder_report[0], betas)
    assert new[0] == betas[0] and (np.diff(new) > 0).all()


def test_npt_run_track_energies_with_an_nmc_slot(product, monkeypatch):
    """The gsparse30 fixture instance, 4 replicas x 2 restarts, the coldest slot runs NMC cycles: every round goes through round(), and
    a row is the state BEHIND the NMC phases (what the swap decision sees)."""
    J, h = golden_instance("npt_run_gsparse30_mixed")
    betas, rounds = np.linspace(0.5, 2.0, 4), 4
    kw = dict(num_sweeps_MCMC=40, num_sweeps_read=20, num_swap_attempts=rounds, num_swapping_pairs=1, num_cycles=1, global_beta=2.5,
              lambda_start=3.0, lambda_end=0.05, lambda_reduction_factor=0.8, threshold_initial=0.9999, threshold_cutoff=0.97,
              num_restarts=2)
    (E, sl), plain, tracked, calls = npt_three_runs(product, monkeypatch, J, h, betas, [False, False, False, True], kw)
    obj = tracked[0]
    assert not calls
    assert np.array_equal(obj.round_energies, E) and np.array_equal(obj.round_slots, sl) and E.shape == (rounds, 8)
    same_npt_run(plain, tracked)
    check_report(obj, betas, rounds, 2, 4)


APT_ATTRS = ("final_energies", "final_slots", "swap_accepted", "icm_cluster_sizes", "restart_energies")


@pytest.mark.parametrize("lanes", ["off", "force"])
def test_apt_icm_track_energies(product, monkeypatch, lanes):
    """Wishart N = 10, 10 sub-replicas of a 6-rung ladder, 2 restarts, 6 rounds of 3 sweeps.  The yardstick: the call-per-step run
    (lanes="off") without the keyword, read back before every swap -- behind icm_round_ladders.  lanes="force": rounds 0..4 inside
    k_apt_rounds_lanes.  Restart 0's rows equal a num_restarts=1 run."""
    monkeypatch.setattr(product.engine, "APT_LANES_IN_LAUNCH", True)       # the route under test, whatever the measured default is
    J, h, _, _ = wishart(product)
    betas, rounds, S = np.geomspace(0.2, 2.0, 6), 6, 3
    kw = dict(num_replicas=6, num_sweeps_MCMC=S * rounds, num_sweeps_read=S * rounds, num_swap_attempts=rounds, num_swapping_pairs=2,
              icm_feedback=True)

    def run(lanes_, **k):
        obj = product.APT_ICM(J, h, rng="philox", seed=5, lanes=lanes_)
        with quiet():
            M, Energy = obj.run(betas, **kw, **k)
        return obj, M, Energy
    seen = []
    with read_backs(product, seen):
        run("off", num_restarts=2)
    E, sl = stacked(seen, rounds)
    plain = run(lanes, num_restarts=2)
    routes = []
    orig = product.engine.Engine.apt_rounds_lanes

    def spy(self, n_rounds, *a, **k):
        out = orig(self, n_rounds, *a, **k)
        routes.append((int(n_rounds), out[0]))
        return out
    product.engine.Engine.apt_rounds_lanes = spy
    try:
        tracked = run(lanes, num_restarts=2, track_energies=True)
    finally:
        product.engine.Engine.apt_rounds_lanes = orig
    assert routes == ([(rounds - 1, True)] if lanes == "force" else [])
    obj = tracked[0]
    G1 = 10 * 6
    assert obj.round_energies.shape == (rounds, 2 * G1)
    assert np.array_equal(obj.round_energies, E) and np.array_equal(obj.round_slots, sl)
    assert np.array_equal(plain[1], tracked[1]) and np.array_equal(plain[2], tracked[2])
    for a in APT_ATTRS:
        assert np.array_equal(getattr(plain[0], a), getattr(obj, a)), a
    one = run(lanes, num_restarts=1, track_energies=True)[0]
    assert np.array_equal(one.round_energies, obj.round_energies[:, :G1]) and np.array_equal(one.round_slots, obj.round_slots[:, :G1])
    assert len(obj.ladder_report) == 2 and len(one.ladder_report) == 1
    for k in ("mean_energy", "sigma_energy", "swap_accepts", "round_trips"):
        assert np.array_equal(one.ladder_report[0][k], obj.ladder_report[0][k]), k
    assert obj.ladder_report[0]["round_trips"].shape == (G1,) and (obj.ladder_report[0]["swap_attempts"] == 10 * (rounds - 1)).all()


def test_track_energies_is_refused_off_the_device_resident_paths(product):
    J, h = make_instance(40, seed=2)
    kw = dict(num_sweeps_MCMC=4, num_sweeps_read=4, num_swap_attempts=2, track_energies=True)
    with pytest.raises(ValueError, match="track_energies"):
        product.NPT(J, h).run(np.array([0.5, 1.0]), 2, [False, False], **kw)
    with pytest.raises(ValueError, match="track_energies"):
        product.NPT(J, h, rng="philox", seed=1).run(np.array([0.5, 1.0]), 2, [False, False], device_ids=[0, 0], **kw)
    with pytest.raises(ValueError, match="track_energies"):
        product.APT_ICM(J.toarray(), h).run(np.array([0.5, 1.0]), 2, **kw)
    with pytest.raises(ValueError, match="track_energies"):
        product.APT_ICM(J.toarray(), h, rng="philox", seed=1).run(np.array([0.5, 1.0]), 2, icm_feedback=True, device_ids=[0, 0], **kw)
