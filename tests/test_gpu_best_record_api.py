"""track_best through the classes: NPT.run and APT_ICM.run keep every chain's lowest-energy state over ALL rounds (the return value
Energy looks at the last round only).  NPT's attributes equal the engine-level specification of tests/test_gpu_best_record.py run
with the run's seed, start and normalisation; energy_of(best_state) gives best_energy back (exactly on +-J, within the tracked
energies' stated tolerance -- DESIGN.md section 2 -- on real couplings); the Wishart ground state is found and recorded."""
import contextlib
import io
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, golden
from helpers import make_instance

pytestmark = pytest.mark.gpu
INST = os.path.join(GOLDEN, "instances")
R = 8


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def tracked_tolerance(inst, qs, esc):
    """|tracked - fp64 energy of (J, h)|: the tracked energy is the fp64 start energy rounded to 2^-esc plus exact
    deltas of the quantised model, whose energy is within (nnz / 2 + n) 2^-(qs + 1) of the true one at the start and at the end."""
    return 2.0 * (inst.nnz / 2 + inst.n) * 2.0 ** -(qs + 1) + 2.0 * 2.0 ** -esc


def npt_spec(product, Jn, hn, betas, restarts, S, rounds, pairs, seed, target):
    """NPT.run's device-resident protocol at engine level, round by round, no record: start default_rng(seed) bits, sweeps r S ..,
    swap round r.  -> best energy / round / state and first-passage round per global chain."""
    L, N = len(betas), Jn.shape[0]
    G = L * restarts
    m0 = (2 * np.random.default_rng(seed).integers(0, 2, size=(G, N), dtype=np.int8) - 1).astype(np.int8)
    best, stamp, hit = np.full(G, np.inf), np.full(G, -1, np.int32), np.full(G, -1, np.int32)
    state = np.zeros((G, N), np.int8)
    with product.Engine(Jn, hn, G) as eng:
        eng.set_spins(m0)
        eng.pt_init(betas)
        for r in range(rounds):
            eng.sweep_philox(S, seed, sweep0=r * S, beta=None)
            s, E = eng.get_spins(), eng.energy_tracked()
            imp = E < best
            best[imp], stamp[imp], state[imp] = E[imp], r, s[imp]
            if target is not None:
                hit[(hit < 0) & (E <= target)] = r
            eng.pt_swap_philox(r, seed, pairs, want_log=False)
        eng.pt_check()
    return best, stamp, state, hit


@pytest.mark.parametrize("lanes", ["off", "force"])
def test_npt_run_track_best_equals_the_engine_level_specification(product, lanes):
    """+-J, n = 301, 2 restarts of 8 replicas, 10 rounds of 4 sweeps: 9 rounds in batched calls (inside k_rounds_fused, or inside
    k_rounds_lanes under lanes="force"), the last one round by round with its explicit update."""
    J, h = make_instance(301, seed=21)
    betas, seed, S, rounds, pairs, restarts = np.geomspace(0.2, 2.0, R), 4242, 4, 10, 2, 2
    calls = []
    orig = product.engine.Engine.pt_rounds_deferred

    def spy(self, n_rounds, *a, **k):
        ok = orig(self, n_rounds, *a, **k)
        calls.append((int(n_rounds), self.last_rounds_route() if ok else None))
        return ok
    free = npt_spec(product, J, h, betas, restarts, S, rounds, pairs, seed, None)
    target = float(np.median(free[0]))
    want = npt_spec(product, J, h, betas, restarts, S, rounds, pairs, seed, target)
    assert (want[3] >= 0).any() and (want[3] < 0).any() and np.mean(want[1] < rounds - 1) >= 0.25
    obj = product.NPT(J, h, rng="philox", seed=seed, lanes=lanes)
    product.engine.Engine.pt_rounds_deferred = spy
    try:
        with quiet():
            _, Energy = obj.run(betas, R, [False] * R, num_sweeps_MCMC=S * rounds, num_sweeps_read=S * rounds, num_swap_attempts=rounds,
                                num_swapping_pairs=pairs, num_restarts=restarts, track_best=True, target_energy=target)
    finally:
        product.engine.Engine.pt_rounds_deferred = orig
    assert calls == [(rounds - 1, "lanes" if lanes == "force" else "in launch")]
    assert np.array_equal(obj.best_energy, want[0]) and np.array_equal(obj.best_round, want[1])
    assert np.array_equal(obj.best_state, want[2]) and np.array_equal(obj.first_hit_round, want[3])
    assert obj.best_state.dtype == np.int8 and obj.best_state.shape == (restarts * R, 301)
    # +-J: the tracked energy IS the energy
    with product.Engine(J, h, 1) as eng:
        assert np.array_equal(eng.energy_of(obj.best_state), obj.best_energy)
    # the run-long record is at least as good as the last-round read-out of restart 0, slot by slot
    assert obj.best_energy[:R].min() <= Energy.min()


def test_npt_run_track_best_on_real_couplings(product):
    J, h = make_instance(301, seed=21, with_h=True, gaussian=True)
    betas, rounds, S = np.geomspace(0.2, 2.0, R), 6, 4
    obj = product.NPT(J, h, rng="philox", seed=9)
    with quiet():
        obj.run(betas, R, [False] * R, num_sweeps_MCMC=S * rounds, num_sweeps_read=S * rounds, num_swap_attempts=rounds, num_swapping_pairs=2,
                track_best=True)
    assert (obj.first_hit_round == -1).all() and (obj.best_round >= 0).all()
    nf = np.max(np.abs(J))
    inst = product.Instance(J / nf, h / nf)
    with product.Engine(inst, None, 1) as eng:
        err = np.abs(eng.energy_of(obj.best_state) - obj.best_energy)
        assert err.max() <= tracked_tolerance(inst, eng.field_scale, eng.energy_scale), err.max()


def test_npt_run_track_best_with_nmc_slots(product):
    """The n = 60 sparse fixture instance, 4 replicas, the two coldest slots run NMC cycles: the run completes, every chain was
    observed every round (after its NMC chains were handed back), and the recorded states carry the recorded energies."""
    g = golden("nmc_run_gsparse60")
    J = sp.csr_matrix((g["data"], g["indices"], g["indptr"]), shape=(int(g["N"]),) * 2).toarray()
    h = np.asarray(g["h"], dtype=np.float64).reshape(-1)
    rounds = 3
    obj = product.NPT(J, h, rng="philox", seed=5)
    with quiet():
        obj.run(np.geomspace(0.2, 2.0, 4), 4, [False, False, True, True], num_sweeps_MCMC=60, num_sweeps_read=30, num_swap_attempts=rounds,
                num_swapping_pairs=1, num_cycles=1, global_beta=2.5, lambda_start=3.0, lambda_end=0.05, lambda_reduction_factor=0.8,
                threshold_initial=0.9999, threshold_cutoff=0.97, track_best=True)
    assert obj.best_energy.shape == (4,) and ((obj.best_round >= 0) & (obj.best_round < rounds)).all()
    nf = np.max(np.abs(J))
    inst = product.Instance(J / nf, h / nf)
    with product.Engine(inst, None, 1) as eng:
        err = np.abs(eng.energy_of(obj.best_state) - obj.best_energy)
        assert err.max() <= tracked_tolerance(inst, eng.field_scale, eng.energy_scale), err.max()


def test_track_best_is_refused_off_the_device_resident_paths(product):
    J, h = make_instance(40, seed=2)
    with pytest.raises(ValueError, match="track_best"):
        product.NPT(J, h).run(np.array([0.5, 1.0]), 2, [False, False], num_sweeps_MCMC=4, num_sweeps_read=4, num_swap_attempts=2,
                              track_best=True)
    with pytest.raises(ValueError, match="track_best"):
        product.APT_ICM(J.toarray(), h).run(np.array([0.5, 1.0]), 2, num_sweeps_MCMC=4, num_sweeps_read=4, num_swap_attempts=2, track_best=True)


def test_apt_icm_track_best_sees_the_houdayer_step(product, monkeypatch):
    """pmj-12 (the +-J fixture of 12 spins), 10 sub-replicas of a 6-rung ladder.  best_energy <= final_energies chain by chain; and at
    least one chain's best state is none of the states the chains had after that round's sweeps: it was recorded by the observation
    behind the Houdayer step.  Seed 3: of the seeds 1 .. 24, 3 and 18 have such a chain (12 spins leave few states that no chain of 60
    holds after its sweeps); every one of them has 13 to 26 chains whose best state differs from their OWN post-sweep state."""
    g = golden("apt_icm_run_pmj12_S5")
    J = sp.csr_matrix((g["data"], g["indices"], g["indptr"]), shape=(int(g["N"]),) * 2).toarray()
    N, Rr, rounds, S = J.shape[0], 6, 8, 3
    post_sweep = {}
    orig = product.engine.Engine.best_update

    def spy(self, stamp):
        post_sweep.setdefault(int(stamp), self.get_spins())          # the first observation of a round: the states after its sweeps
        return orig(self, stamp)
    monkeypatch.setattr(product.engine.Engine, "best_update", spy)
    obj = product.APT_ICM(J, np.zeros(N), rng="philox", seed=3)
    with quiet():
        obj.run(np.geomspace(0.2, 2.0, Rr), num_replicas=Rr, num_sweeps_MCMC=S * rounds, num_sweeps_read=S * rounds, num_swap_attempts=rounds,
                num_swapping_pairs=2, icm_feedback=True, track_best=True)
    G = 10 * Rr
    assert obj.best_energy.shape == (G,) and obj.best_state.shape == (G, N) and sorted(post_sweep) == list(range(rounds))
    assert (obj.best_energy <= obj.final_energies).all()
    with product.Engine(J, np.zeros(N), 1) as eng:
        assert np.array_equal(eng.energy_of(obj.best_state), obj.best_energy)
    after_houdayer = [c for c in range(G) if not (post_sweep[int(obj.best_round[c])] == obj.best_state[c]).all(axis=1).any()]
    assert after_houdayer, "no chain's best state came from the observation behind the Houdayer step"


def test_wishart_ground_state_is_recorded(product):
    """Wishart N = 10, instance 1: 64 chains (8 restarts of 8 replicas), 50 rounds of 10 sweeps; the record's minimum times max|J| is
    the file's ground-state energy."""
    fn = "wishart_planting_N_10_alpha_0.50_inst_1.txt"
    W, _ = product.instances.txt_to_A_wishart(os.path.join(INST, "wishart_N10_a0.50__" + fn))
    J = (-W).toarray()
    gs = {l.split()[0]: float(l.split()[1]) for l in open(os.path.join(INST, "wishart_N10_a0.50__gs_energies.txt"))}[fn]
    nf = float(np.max(np.abs(J)))
    obj = product.NPT(J, np.zeros(10), rng="philox", seed=31)
    with quiet():
        obj.run(np.geomspace(0.2, 2.0, R), R, [False] * R, num_sweeps_MCMC=500, num_sweeps_read=500, num_swap_attempts=50,
                num_swapping_pairs=2, num_restarts=8, track_best=True, target_energy=gs / nf + 1e-9)
    assert obj.best_energy.shape == (64,)
    inst = product.Instance(J / nf, np.zeros(10))
    with product.Engine(inst, None, 1) as eng:
        tol = tracked_tolerance(inst, eng.field_scale, eng.energy_scale)
        assert abs(obj.best_energy.min() * nf - gs) <= tol * nf
        c = int(np.argmin(obj.best_energy))
        assert abs(eng.energy_of(obj.best_state[c:c + 1])[0] * nf - gs) < 1e-9
    assert (obj.first_hit_round[obj.best_energy <= gs / nf + 1e-9] >= 0).all()
