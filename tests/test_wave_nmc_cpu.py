"""NMC phase cycles inside one wave launch (include/nlmc.h: nlmc_nmc_phases_waves), the parts that need no GPU: LocalTempering's route
rule over the CPU double -- rounds with wave_nmc=True against rounds with the phase loop, state for state; a round with outputs keeps the
loop; a refusing engine is asked once; the wave call is asked before the lane call; no fused-window planner for the phases where every
context takes the call; wave_nmc=None takes effect only where the engine's sweeps run on the wave kernels -- and the keyword checks of
NPT.  The double is the one of tests/test_lane_nmc_cpu.py with nmc_phases_waves beside it: the same specification in NumPy (the two
entry points compute the same thing), counted apart."""
import numpy as np
import pytest

from conftest import load_product
from helpers import make_instance
from test_lane_nmc_cpu import G, GBETA, L, MARKS, N, PAIRS, PHASES, S, S_NMC, SEED, TEMP_X, NmcEngine, _instance, _state


class WaveNmcEngine(NmcEngine):
    """NmcEngine with the wave mode of the engine (set_wave_sweeps, waves_take) and nmc_phases_waves; `order` records which of the two
    entry points LocalTempering asked, in order."""
    refuse_waves = False
    wave_sweeps = "off"
    lane_sweeps = "off"

    def __init__(self, *a):
        super().__init__(*a)
        self.wave_calls = self.wave_asked = 0
        self.order = []

    def set_wave_sweeps(self, mode):
        self.wave_sweeps = mode

    def set_lane_sweeps(self, mode):
        self.lane_sweeps = mode

    def waves_take(self, rows=None, precision="f32"):
        return self.wave_sweeps == "force"

    def lanes_take(self, rows=None):
        return self.lane_sweeps == "force"

    def nmc_phases_lanes_refusal(self, sweeps_per_phase):
        self.order.append("lanes")
        return super().nmc_phases_lanes_refusal(sweeps_per_phase)

    def nmc_phases_waves_refusal(self, sweeps_per_phase):
        self.wave_asked += 1
        self.order.append("waves")
        return "refused by the test" if (self.refuse_waves and self.has_query) else None

    def nmc_phases_waves(self, kinds, sweeps_per_phase, seed, sweep0, beta, temp_x, min_stride=1, precision="f32", want_minima=False,
                         want_last_best=False):
        """The specification of nmc_phases_lanes (NmcEngine), f32 only."""
        if self.refuse_waves or precision != "f32":
            raise NotImplementedError("refused by the test")
        lane_calls = self.lane_calls
        super().nmc_phases_lanes(kinds, sweeps_per_phase, seed, sweep0, beta, temp_x, min_stride=min_stride, precision=precision)
        self.lane_calls = lane_calls
        self.wave_calls += 1


def _tempering(P, wave_nmc, engine=WaveNmcEngine, m_skip=1, lane_nmc=False, **kw):
    betas = np.geomspace(0.3, 2.0, L)
    lt = P.distributed.LocalTempering(_instance(P), betas, G, SEED, PAIRS, [0], engine_factory=engine, lane_nmc=lane_nmc,
                                      wave_nmc=wave_nmc, **kw)
    lt.configure_nmc(MARKS, PHASES, S_NMC, GBETA, TEMP_X, np.zeros(N), [1.0], 1e-9, 10, 0.99, [0.9], M_skip=m_skip)
    lt.set_spins((2 * np.random.default_rng(3).integers(0, 2, size=(G, N), dtype=np.int8) - 1).astype(np.int8))
    return lt


@pytest.mark.parametrize("m_skip", [1, 2])
def test_rounds_in_launch_equal_the_phase_loop_state_for_state(m_skip):
    P = load_product()
    a, b = _tempering(P, True, m_skip=m_skip), _tempering(P, False, m_skip=m_skip)
    for r in range(4):
        a.round(S)
        b.round(S)
        for x, y in zip(_state(a), _state(b)):
            assert np.array_equal(x, y), f"round {r}"
        assert (a.sweeps_done, a.nmc_sweeps_done) == (b.sweeps_done, b.nmc_sweeps_done) == ((r + 1) * S, (r + 1) * len(PHASES) * S_NMC)
    assert not np.array_equal(a.slots(), np.arange(G) % L)            # swaps moved chains: the marked subset is not the first one's
    ea, eb = a.engs[0], b.engs[0]
    assert (ea.wave_calls, ea.lane_calls, ea.phase_sweeps, ea.adopted) == (4, 0, 0, 0)
    assert (a.wave_nmc_rounds, a.wave_nmc_calls, a.lane_nmc_rounds, a.lane_nmc_calls) == (4, 4, 0, 0)
    assert (eb.wave_calls, eb.phase_sweeps, eb.adopted) == (0, 4 * len(PHASES), 4 * (len(PHASES) - 1)) and b.wave_nmc_rounds == 0
    assert ea.wave_asked == 1 and eb.wave_asked == 0                   # the engine is asked once, not every round


def test_a_round_that_wants_outputs_keeps_the_phase_loop():
    P = load_product()
    a, b = _tempering(P, True), _tempering(P, False)
    a.round(S)
    b.round(S)
    oa, ob = a.round(S, want_energy=True)[0], b.round(S, want_energy=True)[0]
    assert a.engs[0].wave_calls == 1 and a.engs[0].phase_sweeps == len(PHASES) and a.wave_nmc_rounds == 1
    assert len(oa["nmc"]) == len(PHASES)
    for x, y in zip(oa["nmc"], ob["nmc"]):
        assert np.array_equal(x["energy"], y["energy"])
    for x, y in zip(_state(a), _state(b)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("has_query", [True, False])
def test_a_refusing_engine_is_asked_once(has_query):
    """With the query the refusal costs no call; without it the first call raises, nothing was run, and the loop takes over for good."""
    P = load_product()

    class Refusing(WaveNmcEngine):
        refuse_waves = True
    Refusing.has_query = has_query
    a, b = _tempering(P, True, engine=Refusing), _tempering(P, False)
    for _ in range(3):
        a.round(S)
        b.round(S)
    e = a.engs[0]
    assert e.wave_asked == 1 and e.wave_calls == 0 and e.phase_sweeps == 3 * len(PHASES) and a.wave_nmc_rounds == 0
    assert a.nmc_routes["waves"].refused == {0}
    for x, y in zip(_state(a), _state(b)):
        assert np.array_equal(x, y)


def test_the_wave_call_is_asked_before_the_lane_call():
    P = load_product()
    a = _tempering(P, True, lane_nmc=True)
    a.round(S)
    e = a.engs[0]
    assert e.order == ["waves"] and (e.wave_calls, e.lane_calls) == (1, 0)         # taken by the waves: the lanes are never asked

    class Refusing(WaveNmcEngine):
        refuse_waves = True
    b, c = _tempering(P, True, engine=Refusing, lane_nmc=True), _tempering(P, False)
    for _ in range(2):
        b.round(S)
        c.round(S)
    e = b.engs[0]
    assert e.order == ["waves", "lanes"] and (e.wave_calls, e.lane_calls, e.phase_sweeps) == (0, 2, 0)
    assert (b.wave_nmc_rounds, b.lane_nmc_rounds) == (0, 2)
    for x, y in zip(_state(b), _state(c)):
        assert np.array_equal(x, y)


def test_no_phase_planner_where_every_context_takes_the_call():
    P = load_product()
    a, b = _tempering(P, True), _tempering(P, False)
    a.plan(3 * S, 3)
    b.plan(3 * S, 3)
    assert a._planners is not None and a._nmc_planners is None
    assert b._nmc_planners is not None and b._nmc_planners[0].slot == 1

    class Refusing(WaveNmcEngine):
        refuse_waves = True
    c = _tempering(P, True, engine=Refusing)
    c.plan(3 * S, 3)
    assert c._nmc_planners is not None                                 # a context that keeps the loop keeps its planner


@pytest.mark.parametrize("waves", ["off", "force"])
def test_the_default_takes_effect_only_on_the_wave_route(waves):
    P = load_product()
    lt = _tempering(P, None, wave_sweeps=waves)
    assert lt.wave_nmc is P.distributed.WAVE_NMC_IN_LAUNCH
    assert lt.engs[0].wave_sweeps == waves
    for _ in range(2):
        lt.round(S)
    want = 2 if (waves == "force" and P.distributed.WAVE_NMC_IN_LAUNCH) else 0
    e = lt.engs[0]
    assert (lt.wave_nmc_rounds, e.wave_calls) == (want, want) and e.phase_sweeps == (2 - want) * len(PHASES)
    assert e.wave_asked == (1 if want else 0)                          # off the wave route the engine is not even asked


def test_npt_keywords():
    P = load_product()
    J, h = make_instance(16, seed=2)
    assert P.NPT(J, h, rng="philox").wave_nmc is None
    assert P.NPT(J, h, rng="philox", waves="force").wave_nmc is None
    for given in (True, False):
        with pytest.raises(ValueError, match="wave_nmc needs"):
            P.NPT(J, h, rng="philox", wave_nmc=given)
        with pytest.raises(ValueError, match="wave_nmc needs"):
            P.NPT(J, h, rng="philox", lanes="force", wave_nmc=given)
    seen = []

    def device_resident(*a, **k):
        seen.append(a[4])
        return None, np.zeros(3)
    run = dict(num_sweeps_MCMC=4, num_sweeps_read=4, num_swap_attempts=2)
    for mode, given in (("force", True), ("auto", True), ("force", False), ("force", None)):
        obj = P.NPT(J, h, rng="philox", seed=1, waves=mode, wave_nmc=given)
        assert obj.wave_nmc is given
        obj._run_device_resident = device_resident
        obj.run(np.linspace(0.5, 1.0, 3), 3, [False, True, False], **run)
    assert len(seen) == 4 and all(s is not None for s in seen)          # waves + doNMC runs device-resident, with or without the keyword
    obj = P.NPT(J, h, rng="philox", seed=1, waves="force", wave_rounds=True, wave_nmc=True)
    obj._run_device_resident = device_resident
    with pytest.raises(ValueError, match="wave_rounds runs plain replicas only"):     # the rounds kernels have no phase flags: as before
        obj.run(np.linspace(0.5, 1.0, 3), 3, [False, True, False], **run)
    with pytest.raises(ValueError, match="f32"):
        P.NPT(J, h, rng="philox", precision="f64", waves="force", wave_nmc=True)


def test_binding_and_engine_wrapper():
    import ctypes
    import re
    P = load_product()
    lib = P._abi.lib()
    hdr = open(P._abi.os.path.join(P._abi.os.path.dirname(P._abi._PKG), "include", "nlmc.h")).read()
    assert re.search(r"int\s+nlmc_nmc_phases_waves\s*\(\s*nlmc_ctx\s*\*", hdr)
    assert {"nlmc_nmc_phases_waves", "nlmc_nmc_phases_waves_refusal"} <= set(P._abi.EXPORTS)
    assert lib.nlmc_nmc_phases_waves.argtypes == lib.nlmc_nmc_phases_lanes.argtypes
    assert lib.nlmc_nmc_phases_waves(None, P._abi.F32, None, 1, 1, 0, 1, 1.0, 20.0, 1, None, None, None) == P._abi.ERR_ARG
    assert lib.nlmc_nmc_phases_waves_refusal(None, 1) == b"no context"
    assert lib.nlmc_abi_version() == 3

    class FakeLib:
        calls = []

        def nlmc_subset_count(self, ctx):
            return 2

        def nlmc_nmc_phases_waves(self, ctx, prec, kinds, P_, S_, sweep0, seed, beta, temp_x, stride, pmin, parg, best):
            k = np.ctypeslib.as_array(ctypes.cast(kinds, ctypes.POINTER(ctypes.c_int32)), (P_,)).tolist()
            self.calls.append((prec, k, S_, sweep0, seed, beta, temp_x, stride, pmin is not None, parg is not None, best is not None))
            if pmin is not None:
                np.ctypeslib.as_array(ctypes.cast(pmin, ctypes.POINTER(ctypes.c_int64)), (2 * P_,))[:] = np.arange(2 * P_) << 4
            return 0

        def nlmc_nmc_phases_waves_refusal(self, ctx, S_):
            return b"too long" if S_ > 4 else None
    eng = P.Engine.__new__(P.Engine)
    eng._L, eng._ctx, eng.n, eng.energy_scale = FakeLib(), None, 5, 4
    assert eng.nmc_phases_waves(["C", "NC", "ALL"], 4, SEED, (1 << 32) | 7, 2.5, 20.0, min_stride=2) is None
    assert eng._L.calls[-1] == (P._abi.F32, [1, 2, 0], 4, 7, SEED, 2.5, 20.0, 2, False, False, False)
    out = eng.nmc_phases_waves(["C", "ALL"], 1, SEED, 0, 1.0, 20.0, want_minima=True, want_last_best=True)
    assert eng._L.calls[-1][-3:] == (True, True, True)
    assert out["phase_min"].shape == (2, 2) and np.array_equal(out["phase_min"], np.arange(4.0).reshape(2, 2))
    assert out["phase_argmin"].shape == (2, 2) and out["last_best"].shape == (2, 5)
    assert eng.nmc_phases_waves_refusal(4) is None and eng.nmc_phases_waves_refusal(5) == "too long"
    with pytest.raises(KeyError):
        eng.nmc_phases_waves(["X"], 1, SEED, 0, 1.0, 20.0)
