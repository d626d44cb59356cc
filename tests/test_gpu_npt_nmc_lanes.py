"""NPT(lanes=...) with doNMC slots: the plain chains and the NMC phases on the chain-per-lane route, the rounds without output with all
phases of a round in one launch per context (lane_nmc; Engine.nmc_phases_lanes).  Same bits as lanes="off" and as the phase loop on the
lane kernels: M, Energy, every restart's energies, the best-state record and the energy log."""
import contextlib
import io
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
INST = os.path.join(GOLDEN, "instances")
LBP = dict(lambda_start=3.0, lambda_end=0.05, lambda_reduction_factor=0.8, threshold_initial=0.9999, threshold_cutoff=0.97)


def wishart(P):
    W, _ = P.instances.txt_to_A_wishart(os.path.join(INST, "wishart_N10_a0.50__wishart_planting_N_10_alpha_0.50_inst_1.txt"))
    J = (-W).toarray()                         # NMC/examples/wishart_example.py: J = -W, h = 0
    return J, np.zeros(J.shape[0])


def run(P, J, h, betas, doNMC, seed=41, **kw):
    ctor = {k: kw.pop(k) for k in ("lanes", "lane_nmc") if k in kw}
    obj = P.NPT(J, h, rng="philox", seed=seed, **ctor)
    with contextlib.redirect_stdout(io.StringIO()):
        M, E = obj.run(betas, len(betas), doNMC, **kw)
    return obj, M, E


@pytest.mark.parametrize("num_restarts", [1, 3])
def test_wishart_rounds_with_nmc_slots_on_the_lane_route(product, num_restarts):
    P = product
    J, h = wishart(P)
    R, rounds = 8, 3
    betas = np.geomspace(0.3, 3.0, R)
    doNMC = [False] * 5 + [True] * 3
    args = dict(num_sweeps_MCMC=60, num_sweeps_read=30, num_swap_attempts=rounds, num_swapping_pairs=3, num_cycles=2, global_beta=2.5,
                num_restarts=num_restarts, return_trace="int8", track_best=True, track_energies=True, **LBP)
    a, Ma, Ea = run(P, J, h, betas, doNMC, lanes="force", lane_nmc=True, **args)
    b, Mb, Eb = run(P, J, h, betas, doNMC, lanes="force", lane_nmc=False, **args)
    c, Mc, Ec = run(P, J, h, betas, doNMC, lanes="off", **args)
    assert Ma.shape == (R * 10, 20) and not np.all(Ma == Ma[:, :1])
    for o, M, E in ((b, Mb, Eb), (c, Mc, Ec)):
        assert np.array_equal(Ma, M) and np.array_equal(Ea, E)
        assert np.array_equal(a.restart_energies, o.restart_energies)
        assert np.array_equal(a.swap_accepted, o.swap_accepted) and np.array_equal(a.swap_pairs, o.swap_pairs)
        for k in ("best_energy", "best_state", "best_round", "first_hit_round", "round_energies", "round_slots"):
            assert np.array_equal(getattr(a, k), getattr(o, k)), k
    assert a.restart_energies.shape == (num_restarts, R)
    # the contexts ran on the lane route; rounds 0 .. rounds - 2 took the in-launch call, the last one (it returns the trace) the loop
    assert a.sweep_routes == ["lanes"] and b.sweep_routes == ["lanes"] and c.sweep_routes != ["lanes"]
    assert a.lane_nmc_rounds == rounds - 1 and b.lane_nmc_rounds == 0 and c.lane_nmc_rounds == 0


def test_the_default_follows_the_module_constant_on_the_lane_route_only(product):
    """LocalTempering(lane_nmc=None): the one-launch call where LANE_NMC_IN_LAUNCH says so AND the engine's sweeps run one chain per
    lane; with the lane mode off the phase loop and its fused-window planner stay, whatever the constant.  NPT without the keyword
    keeps refusing lanes with doNMC slots."""
    P = product
    J, h = wishart(P)
    J = J / np.max(np.abs(J))
    inst = P.Instance(J, h)
    betas, marks, eps = np.geomspace(0.3, 3.0, 8), [False] * 5 + [True] * 3, np.finfo(float).eps
    thr = [0.9999, 0.9899, 0.9799]
    ends = []
    for lanes in ("force", "off"):
        lt = P.distributed.LocalTempering(inst, betas, 16, 41, 3, [0], lane_sweeps=lanes)
        try:
            lt.configure_nmc(marks, ["C", "NC", "ALL"], 4, 2.5, 20.0, P.lbp.EdgeGraph(inst).epsilon(inst.h), P.lbp.lambda_list(3.0, 0.05, 0.8),
                             eps, 100, float(np.tanh(19.06)) - eps, thr)
            lt.set_spins((2 * np.random.default_rng(2).integers(0, 2, size=(16, 10), dtype=np.int8) - 1).astype(np.int8))
            lt.plan(3 * 20, 3)
            for _ in range(3):
                lt.round(20)
            lt.check()
            want = 3 if (lanes == "force" and P.distributed.LANE_NMC_IN_LAUNCH) else 0
            assert lt.lane_nmc_rounds == want and (lt._nmc_planners is None) == (want == 3)
            ends.append((lt.gather_spins(), lt.slots()))
        finally:
            lt.close()
    assert np.array_equal(ends[0][0], ends[1][0]) and np.array_equal(ends[0][1], ends[1][1])
    obj = P.NPT(J, h, rng="philox", seed=1, lanes="force")
    with pytest.raises(ValueError, match="lane_nmc"):
        obj.run(betas, 8, marks, num_sweeps_MCMC=60, num_sweeps_read=30, num_swap_attempts=3, num_swapping_pairs=3, num_cycles=2)


def test_chimera128_one_ladder_without_a_trace(product):
    """No trace comes back; the last round still reads its per-sweep energies (the read-out takes their minimum), so it keeps the phase
    loop and rounds 0 .. rounds - 2 run in launch."""
    P = product
    W, hh = P.instances.txt_to_A_droplet(os.path.join(INST, "chimera128__001.txt"))
    J, h = -W, -np.asarray(hh, dtype=np.float64).reshape(-1)      # NMC/examples/chimera_example.py: J = -W, h = -h
    R, rounds = 8, 4
    betas = np.geomspace(0.3, 5.0, R)
    doNMC = [False] * 5 + [True] * 3
    args = dict(num_sweeps_MCMC=40, num_sweeps_read=40, num_swap_attempts=rounds, num_swapping_pairs=2, num_cycles=1, global_beta=10.0,
                temp_x=20, return_trace=None, **LBP)
    a, Ma, Ea = run(P, J, h, betas, doNMC, seed=8, lanes="force", lane_nmc=True, **args)
    c, Mc, Ec = run(P, J, h, betas, doNMC, seed=8, lanes="off", **args)
    assert Ma is None and Mc is None
    assert np.array_equal(Ea, Ec) and np.array_equal(a.restart_energies, c.restart_energies)
    assert np.array_equal(a.swap_accepted, c.swap_accepted)
    assert a.sweep_routes == ["lanes"] and a.lane_nmc_rounds == rounds - 1
