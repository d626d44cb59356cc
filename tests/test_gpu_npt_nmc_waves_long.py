"""NPT(waves=..., wave_long=True) with doNMC slots on a complete graph of 257 spins: the rounds without output run all NMC phases of a
round in one k_nmc_phases_waves_long launch per context (wave_long_nmc; Engine.nmc_phases_waves_long).  Same bits as the phase loop on
the long wave kernels and as waves="off": M, Energy, every restart's energies, the swap log.  A ladder of 4 with 2 doNMC slots, 3 rounds,
2 restarts."""
import contextlib
import io

import numpy as np
import pytest

from test_gpu_npt_nmc_lanes import LBP

pytestmark = pytest.mark.gpu
N, R, ROUNDS = 257, 4, 3
DONMC = [False] * 2 + [True] * 2
GBETA = 2.5 / np.sqrt(N)
ARGS = dict(num_sweeps_MCMC=8, num_sweeps_read=4, num_swap_attempts=ROUNDS, num_swapping_pairs=1, num_cycles=2, global_beta=GBETA,
            num_restarts=2, return_trace="int8", **LBP)


def complete():
    A = np.triu(np.random.default_rng(N).choice([-1.0, 1.0], size=(N, N)), 1)
    return A + A.T, np.zeros(N)


def run(P, J, h, betas, seed=41, **kw):
    ctor = {k: kw.pop(k) for k in ("waves", "wave_long", "wave_long_nmc") if k in kw}
    obj = P.NPT(J, h, rng="philox", seed=seed, **ctor)
    with contextlib.redirect_stdout(io.StringIO()):
        M, E = obj.run(betas, len(betas), DONMC, **kw)
    return obj, M, E


def test_rounds_with_nmc_slots_on_the_long_wave_route(product):
    P = product
    J, h = complete()
    betas = np.geomspace(0.5, 2.0, R) * GBETA
    a, Ma, Ea = run(P, J, h, betas, waves="force", wave_long=True, wave_long_nmc=True, **ARGS)
    b, Mb, Eb = run(P, J, h, betas, waves="force", wave_long=True, wave_long_nmc=False, **ARGS)
    c, Mc, Ec = run(P, J, h, betas, waves="off", **ARGS)
    assert Ma.shape[0] == R * N and not np.all(Ma == Ma[:, :1])
    for o, M, E in ((b, Mb, Eb), (c, Mc, Ec)):
        assert np.array_equal(Ma, M) and np.array_equal(Ea, E)
        assert np.array_equal(a.restart_energies, o.restart_energies)
        assert np.array_equal(a.swap_accepted, o.swap_accepted) and np.array_equal(a.swap_pairs, o.swap_pairs)
    assert a.restart_energies.shape == (2, R)
    # the contexts ran on the wave route; rounds 0 .. rounds - 2 took the in-launch call, the last one (it returns the trace) the loop
    assert a.sweep_routes == ["waves"] and b.sweep_routes == ["waves"] and c.sweep_routes != ["waves"]
    assert a.wave_long_nmc_rounds == ROUNDS - 1 and b.wave_long_nmc_rounds == 0 and c.wave_long_nmc_rounds == 0
    assert a.wave_nmc_rounds == 0 and a.lane_nmc_rounds == 0


def _local(P, inst, betas, **kw):
    eps = np.finfo(float).eps
    lt = P.distributed.LocalTempering(inst, betas, 2 * R, 41, 1, [0], **kw)
    lt.configure_nmc(DONMC, ["C", "NC", "ALL"], 2, GBETA, 20.0, P.lbp.EdgeGraph(inst).epsilon(inst.h), P.lbp.lambda_list(3.0, 0.05, 0.8),
                     eps, 100, float(np.tanh(19.06)) - eps, [0.9999, 0.9899, 0.9799])
    lt.set_spins((2 * np.random.default_rng(2).integers(0, 2, size=(2 * R, N), dtype=np.int8) - 1).astype(np.int8))
    return lt


def test_the_knob_makes_local_tempering_fall_back_once(product, monkeypatch):
    """NLMC_NO_WAVE_LONG_NMC=1: the engine refuses when asked, the phase loop and its planner stay, the bits are those of
    wave_long_nmc=False."""
    P = product
    J, h = complete()
    inst = P.Instance(J, h)
    betas = np.geomspace(0.5, 2.0, R) * GBETA
    ends = []
    for knob, given in ((True, True), (False, True), (False, False)):
        if knob:
            monkeypatch.setenv("NLMC_NO_WAVE_LONG_NMC", "1")
        else:
            monkeypatch.delenv("NLMC_NO_WAVE_LONG_NMC", raising=False)
        lt = _local(P, inst, betas, wave_sweeps="force", wave_long=True, wave_long_nmc=given)
        try:
            lt.plan(3 * 6, 3)
            for _ in range(3):
                lt.round(6)
            lt.check()
            took = given and not knob
            assert lt.wave_long_nmc_rounds == (3 if took else 0) and (lt._nmc_planners is None) == took
            assert lt.nmc_routes["waves_long"].refused == ({0} if knob else set())
            assert lt.wave_nmc_rounds == 0 and lt.engs[0].last_sweep_route() == "waves"
            ends.append((lt.gather_spins(), lt.slots()))
        finally:
            lt.close()
    for e in ends[1:]:
        assert np.array_equal(ends[0][0], e[0]) and np.array_equal(ends[0][1], e[1])
