"""NPT(waves=...) with doNMC slots: the rounds without output run all NMC phases of a round in one k_nmc_phases_waves launch per context
(wave_nmc; Engine.nmc_phases_waves).  Same bits as waves="off" and as the phase loop on the wave kernels: M, Energy, every restart's
energies, the swap log, the best-state record and the energy log.  Wishart N = 10, a ladder of 6 with 3 doNMC slots, 2 restarts."""
import contextlib
import io

import numpy as np
import pytest

from test_gpu_npt_nmc_lanes import LBP, wishart

pytestmark = pytest.mark.gpu
R, ROUNDS = 6, 4
DONMC = [False] * 3 + [True] * 3
ARGS = dict(num_sweeps_MCMC=40, num_sweeps_read=20, num_swap_attempts=ROUNDS, num_swapping_pairs=2, num_cycles=2, global_beta=2.5,
            num_restarts=2, **LBP)


def run(P, J, h, betas, seed=41, **kw):
    ctor = {k: kw.pop(k) for k in ("waves", "wave_nmc") if k in kw}
    obj = P.NPT(J, h, rng="philox", seed=seed, **ctor)
    with contextlib.redirect_stdout(io.StringIO()):
        M, E = obj.run(betas, len(betas), DONMC, **kw)
    return obj, M, E


@pytest.mark.parametrize("records", [False, True])
def test_wishart_rounds_with_nmc_slots_on_the_wave_route(product, records):
    P = product
    J, h = wishart(P)
    betas = np.geomspace(0.3, 3.0, R)
    args = dict(ARGS, return_trace="int8", track_best=records, track_energies=records)
    a, Ma, Ea = run(P, J, h, betas, waves="force", wave_nmc=True, **args)
    b, Mb, Eb = run(P, J, h, betas, waves="force", wave_nmc=False, **args)
    c, Mc, Ec = run(P, J, h, betas, waves="off", **args)
    assert Ma.shape[0] == R * 10 and not np.all(Ma == Ma[:, :1])
    for o, M, E in ((b, Mb, Eb), (c, Mc, Ec)):
        assert np.array_equal(Ma, M) and np.array_equal(Ea, E)
        assert np.array_equal(a.restart_energies, o.restart_energies)
        assert np.array_equal(a.swap_accepted, o.swap_accepted) and np.array_equal(a.swap_pairs, o.swap_pairs)
        for k in (("best_energy", "best_state", "best_round", "first_hit_round", "round_energies", "round_slots") if records else ()):
            assert np.array_equal(getattr(a, k), getattr(o, k)), k
    assert a.restart_energies.shape == (2, R)
    # the contexts ran on the wave route; rounds 0 .. rounds - 2 took the in-launch call, the last one (it returns the trace) the loop
    assert a.sweep_routes == ["waves"] and b.sweep_routes == ["waves"] and c.sweep_routes != ["waves"]
    assert a.wave_nmc_rounds == ROUNDS - 1 and b.wave_nmc_rounds == 0 and c.wave_nmc_rounds == 0
    assert a.lane_nmc_rounds == 0


def _local(P, inst, betas, **kw):
    eps = np.finfo(float).eps
    lt = P.distributed.LocalTempering(inst, betas, 2 * R, 41, 2, [0], **kw)
    lt.configure_nmc(DONMC, ["C", "NC", "ALL"], 4, 2.5, 20.0, P.lbp.EdgeGraph(inst).epsilon(inst.h), P.lbp.lambda_list(3.0, 0.05, 0.8),
                     eps, 100, float(np.tanh(19.06)) - eps, [0.9999, 0.9899, 0.9799])
    lt.set_spins((2 * np.random.default_rng(2).integers(0, 2, size=(2 * R, 10), dtype=np.int8) - 1).astype(np.int8))
    return lt


def test_the_knob_makes_local_tempering_fall_back_once(product, monkeypatch):
    """NLMC_NO_WAVE_NMC=1: the engine refuses when asked, the phase loop and its planner stay, the bits are those of wave_nmc=False."""
    P = product
    J, h = wishart(P)
    inst = P.Instance(J / np.max(np.abs(J)), h)
    betas = np.geomspace(0.3, 3.0, R)
    ends = []
    for knob, wave_nmc in ((True, True), (False, True), (False, False)):
        if knob:
            monkeypatch.setenv("NLMC_NO_WAVE_NMC", "1")
        else:
            monkeypatch.delenv("NLMC_NO_WAVE_NMC", raising=False)
        lt = _local(P, inst, betas, wave_sweeps="force", wave_nmc=wave_nmc)
        try:
            lt.plan(3 * 20, 3)
            for _ in range(3):
                lt.round(20)
            lt.check()
            took = wave_nmc and not knob
            assert lt.wave_nmc_rounds == (3 if took else 0) and (lt._nmc_planners is None) == took
            assert lt.nmc_routes["waves"].refused == ({0} if knob else set())
            assert lt.engs[0].last_sweep_route() == "waves"
            ends.append((lt.gather_spins(), lt.slots()))
        finally:
            lt.close()
    for e in ends[1:]:
        assert np.array_equal(ends[0][0], e[0]) and np.array_equal(ends[0][1], e[1])


def test_the_default_follows_the_module_constant_on_the_wave_route_only(product):
    P = product
    J, h = wishart(P)
    inst = P.Instance(J / np.max(np.abs(J)), h)
    betas = np.geomspace(0.3, 3.0, R)
    ends = []
    for waves in ("force", "off"):
        lt = _local(P, inst, betas, wave_sweeps=waves)
        try:
            for _ in range(3):
                lt.round(20)
            lt.check()
            assert lt.wave_nmc_rounds == (3 if (waves == "force" and P.distributed.WAVE_NMC_IN_LAUNCH) else 0)
            ends.append((lt.gather_spins(), lt.slots()))
        finally:
            lt.close()
    assert np.array_equal(ends[0][0], ends[1][0]) and np.array_equal(ends[0][1], ends[1][1])
