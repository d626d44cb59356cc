"""NMC phase cycles of long chains inside one wave launch (include/nlmc.h: nlmc_nmc_phases_waves_long), the parts that need no GPU: the
premise of the kernel in NumPy int64 (fields carried through the flips and copied at the argmin equal the fields rebuilt from the
adopted spins); LocalTempering's route rule over the CPU double of tests/test_wave_nmc_cpu.py with nmc_phases_waves_long beside the
other two entry points -- the order of asking, a refusal remembered, rounds with outputs on the loop, the default where the sweeps run on
the wave kernels only, the counters; the keyword checks of NPT and LocalTempering; the binding."""
import numpy as np
import pytest

from conftest import load_product
from helpers import make_instance
from test_lane_nmc_cpu import G, L, PHASES, S, _state
from test_wave_nmc_cpu import WaveNmcEngine, _tempering


@pytest.mark.parametrize("n", [257, 513])
def test_fields_carried_and_copied_equal_fields_rebuilt(n):
    """X_j = h_j + sum_i J_ji s_i in integers.  Three phases of three sweeps with a random decision per visit: X is carried through the
    flips (X += (s_new - s_old) J[k]), copied beside the spins where the energy improves, and adopted with them at the hand-off: at
    every hand-off and at the end both copies equal the fields rebuilt from their spins, so the rebuild is never needed."""
    r = np.random.default_rng(n)
    A = np.triu(r.choice([-1, 1], size=(n, n)), 1).astype(np.int64)
    J = (A + A.T) << 20                                       # fixed-point couplings; no diagonal
    h = np.zeros(n, np.int64)
    s = r.choice([-1, 1], size=n).astype(np.int64)
    X = h + J @ s
    E = -(s @ (J @ s)) // 2
    sb, Xb = s.copy(), X.copy()
    for p in range(3):
        if p > 0:
            s, X, E = sb.copy(), Xb.copy(), Emin              # the hand-off: a copy, no rebuild
            assert np.array_equal(X, h + J @ s) and E == -(s @ (J @ s)) // 2
        Emin = np.iinfo(np.int64).max
        improved = 0
        for t in range(3):
            for k in r.permutation(n):
                sn = 1 if r.random() < 1.0 / (1.0 + np.exp(np.clip(-2.5 / np.sqrt(n) * X[k] / (1 << 20), -50, 50))) else -1
                if sn != s[k]:
                    E += X[k] * (s[k] - sn)
                    X += (sn - s[k]) * J[k]
                    s[k] = sn
            if E < Emin:
                Emin, sb, Xb = E, s.copy(), X.copy()
                improved += 1
        assert improved >= 1                                  # sweep 0 of a phase always improves: the copy is whole before it is read
        assert np.array_equal(Xb, h + J @ sb) and np.array_equal(X, h + J @ s)
        assert Emin == -(sb @ (J @ sb)) // 2
    assert np.all(np.abs(X) < 2 ** 31)                        # ... and they are int32 on the device


class LongNmcEngine(WaveNmcEngine):
    """WaveNmcEngine as a context of long chains: nmc_phases_waves refuses (as the library does beyond 256 spins), and
    nmc_phases_waves_long stands beside it -- the same specification in NumPy, counted apart."""
    refuse_waves = True
    refuse_long = False
    has_query = True

    def __init__(self, *a):
        super().__init__(*a)
        self.long_calls = self.long_asked = 0
        self.wave_long = False

    def set_wave_long(self, on=True):
        self.wave_long = bool(on)

    def nmc_phases_waves_long_refusal(self, sweeps_per_phase):
        self.long_asked += 1
        self.order.append("waves_long")
        return "refused by the test" if (self.refuse_long and self.has_query) else None

    def nmc_phases_waves_long(self, kinds, sweeps_per_phase, seed, sweep0, beta, temp_x, min_stride=1, precision="f32",
                              want_minima=False, want_last_best=False):
        if self.refuse_long or precision != "f32":
            raise NotImplementedError("refused by the test")
        refuse, self.refuse_waves = self.refuse_waves, False
        try:
            wave_calls = self.wave_calls
            super().nmc_phases_waves(kinds, sweeps_per_phase, seed, sweep0, beta, temp_x, min_stride=min_stride, precision=precision)
            self.wave_calls = wave_calls
        finally:
            self.refuse_waves = refuse
        self.long_calls += 1


class RefusingLong(LongNmcEngine):
    refuse_long = True


def _long(P, wave_long_nmc, engine=LongNmcEngine, wave_nmc=True, **kw):
    kw.setdefault("wave_sweeps", "force")
    kw.setdefault("wave_long", True)
    return _tempering(P, wave_nmc, engine=engine, wave_long_nmc=wave_long_nmc, **kw)


@pytest.mark.parametrize("m_skip", [1, 2])
def test_rounds_in_launch_equal_the_phase_loop_state_for_state(m_skip):
    P = load_product()
    a, b = _long(P, True, m_skip=m_skip), _long(P, False, m_skip=m_skip)
    for r in range(4):
        a.round(S)
        b.round(S)
        for x, y in zip(_state(a), _state(b)):
            assert np.array_equal(x, y), f"round {r}"
    assert not np.array_equal(a.slots(), np.arange(G) % L)
    ea, eb = a.engs[0], b.engs[0]
    assert (ea.long_calls, ea.wave_calls, ea.lane_calls, ea.phase_sweeps, ea.adopted) == (4, 0, 0, 0, 0)
    assert (a.wave_long_nmc_rounds, a.wave_long_nmc_calls) == (4, 4)
    assert (a.wave_nmc_rounds, a.wave_nmc_calls, a.lane_nmc_rounds, a.lane_nmc_calls) == (0, 0, 0, 0)
    assert (eb.long_calls, eb.phase_sweeps, eb.adopted) == (0, 4 * len(PHASES), 4 * (len(PHASES) - 1)) and b.wave_long_nmc_rounds == 0
    assert ea.long_asked == 1 and eb.long_asked == 0                   # the engine is asked once, not every round


def test_the_order_of_asking_is_waves_then_waves_long_then_lanes():
    P = load_product()
    a = _long(P, True, lane_nmc=True)
    a.round(S)
    e = a.engs[0]
    assert e.order == ["waves", "waves_long"] and (e.wave_calls, e.long_calls, e.lane_calls) == (0, 1, 0)
    assert a.nmc_routes["waves"].refused == {0} and a.nmc_routes["waves_long"].refused == set()

    b, c = _long(P, True, engine=RefusingLong, lane_nmc=True), _long(P, False)
    for _ in range(2):
        b.round(S)
        c.round(S)
    e = b.engs[0]
    assert e.order == ["waves", "waves_long", "lanes"] and (e.wave_calls, e.long_calls, e.lane_calls, e.phase_sweeps) == (0, 0, 2, 0)
    assert (b.wave_nmc_rounds, b.wave_long_nmc_rounds, b.lane_nmc_rounds) == (0, 0, 2)
    for x, y in zip(_state(b), _state(c)):
        assert np.array_equal(x, y)

    class Short(LongNmcEngine):                                        # a context of short chains takes the first call: the long one is not asked
        refuse_waves = False
    d = _long(P, True, engine=Short)
    d.round(S)
    assert d.engs[0].order == ["waves"] and (d.wave_nmc_rounds, d.wave_long_nmc_rounds) == (1, 0)


@pytest.mark.parametrize("has_query", [True, False])
def test_a_refusal_is_remembered(has_query):
    """With the query the refusal costs no call; without it the first call raises, nothing was run, and the loop takes over for good."""
    P = load_product()

    class Refusing(RefusingLong):
        pass
    Refusing.has_query = has_query
    a, b = _long(P, True, engine=Refusing), _long(P, False)
    for _ in range(3):
        a.round(S)
        b.round(S)
    e = a.engs[0]
    assert e.long_asked == 1 and e.long_calls == 0 and e.phase_sweeps == 3 * len(PHASES) and a.wave_long_nmc_rounds == 0
    assert a.nmc_routes["waves_long"].refused == {0}
    for x, y in zip(_state(a), _state(b)):
        assert np.array_equal(x, y)


def test_a_round_that_wants_outputs_keeps_the_phase_loop():
    P = load_product()
    a, b = _long(P, True), _long(P, False)
    a.round(S)
    b.round(S)
    oa, ob = a.round(S, want_energy=True)[0], b.round(S, want_energy=True)[0]
    assert a.engs[0].long_calls == 1 and a.engs[0].phase_sweeps == len(PHASES) and a.wave_long_nmc_rounds == 1
    assert len(oa["nmc"]) == len(PHASES)
    for x, y in zip(oa["nmc"], ob["nmc"]):
        assert np.array_equal(x["energy"], y["energy"])
    for x, y in zip(_state(a), _state(b)):
        assert np.array_equal(x, y)


def test_no_phase_planner_where_every_context_takes_the_call():
    P = load_product()
    a, b, c = _long(P, True), _long(P, False), _long(P, True, engine=RefusingLong)
    for lt in (a, b, c):
        lt.plan(3 * S, 3)
    assert a._planners is not None and a._nmc_planners is None
    assert b._nmc_planners is not None and c._nmc_planners is not None      # a context that keeps the loop keeps its planner


@pytest.mark.parametrize("waves", ["off", "force"])
def test_the_default_takes_effect_only_on_the_wave_route(waves, monkeypatch):
    """wave_long_nmc=None is the module constant, and -- whatever its value -- applies only where waves_take() holds."""
    P = load_product()
    for constant in (True, False):
        monkeypatch.setattr(P.distributed, "WAVE_LONG_NMC_IN_LAUNCH", constant)
        lt = _tempering(P, False, engine=LongNmcEngine, wave_sweeps=waves)       # (wave_long_nmc left out: None)
        assert lt.wave_long_nmc is constant
        for _ in range(2):
            lt.round(S)
        want = 2 if (waves == "force" and constant) else 0
        e = lt.engs[0]
        assert (lt.wave_long_nmc_rounds, lt.wave_long_nmc_calls, e.long_calls) == (want, want, want)
        assert e.phase_sweeps == (2 - want) * len(PHASES)
        assert e.long_asked == (1 if want else 0)                      # off the wave route the engine is not even asked
    assert isinstance(P.distributed.WAVE_LONG_NMC_IN_LAUNCH, bool)


def test_keywords_need_wave_long():
    P = load_product()
    J, h = make_instance(16, seed=2)
    assert P.NPT(J, h, rng="philox").wave_long_nmc is None
    assert P.NPT(J, h, rng="philox", waves="force", wave_long=True).wave_long_nmc is None
    for given in (True, False):
        with pytest.raises(ValueError, match="wave_long_nmc needs wave_long"):
            P.NPT(J, h, rng="philox", wave_long_nmc=given)
        with pytest.raises(ValueError, match="wave_long_nmc needs wave_long"):
            P.NPT(J, h, rng="philox", waves="force", wave_long_nmc=given)
        assert P.NPT(J, h, rng="philox", waves="force", wave_long=True, wave_long_nmc=given).wave_long_nmc is given
        with pytest.raises(ValueError, match="wave_long_nmc needs wave_long"):
            _tempering(P, None, engine=LongNmcEngine, wave_sweeps="force", wave_long_nmc=given)
        with pytest.raises(ValueError, match="wave_long_nmc needs wave_long"):
            P.hostlogic.check_wave_long_nmc(given, False)
        P.hostlogic.check_wave_long_nmc(given, True)
    P.hostlogic.check_wave_long_nmc(None, False)
    seen = []

    def device_resident(*a, **k):
        seen.append(a[4])
        return None, np.zeros(3)
    obj = P.NPT(J, h, rng="philox", seed=1, waves="force", wave_long=True, wave_long_nmc=True)
    obj._run_device_resident = device_resident
    obj.run(np.linspace(0.5, 1.0, 3), 3, [False, True, False], num_sweeps_MCMC=4, num_sweeps_read=4, num_swap_attempts=2)
    assert len(seen) == 1 and seen[0] is not None                      # waves + doNMC runs device-resident


def test_binding_and_engine_wrapper():
    import ctypes
    import re
    P = load_product()
    lib = P._abi.lib()
    hdr = open(P._abi.os.path.join(P._abi.os.path.dirname(P._abi._PKG), "include", "nlmc.h")).read()
    assert re.search(r"int\s+nlmc_nmc_phases_waves_long\s*\(\s*nlmc_ctx\s*\*", hdr)
    assert re.search(r"const\s+char\s*\*\s*nlmc_nmc_phases_waves_long_refusal\s*\(\s*const\s+nlmc_ctx\s*\*", hdr)
    assert {"nlmc_nmc_phases_waves_long", "nlmc_nmc_phases_waves_long_refusal"} <= set(P._abi.EXPORTS)
    assert lib.nlmc_nmc_phases_waves_long.argtypes == lib.nlmc_nmc_phases_waves.argtypes
    assert lib.nlmc_nmc_phases_waves_long_refusal.argtypes == lib.nlmc_nmc_phases_waves_refusal.argtypes
    assert lib.nlmc_nmc_phases_waves_long_refusal.restype == lib.nlmc_nmc_phases_waves_refusal.restype
    assert lib.nlmc_nmc_phases_waves_long(None, P._abi.F32, None, 1, 1, 0, 1, 1.0, 20.0, 1, None, None, None) == P._abi.ERR_ARG
    assert lib.nlmc_nmc_phases_waves_long_refusal(None, 1) == b"no context"

    class FakeLib:
        calls = []

        def nlmc_subset_count(self, ctx):
            return 2

        def nlmc_nmc_phases_waves_long(self, ctx, prec, kinds, P_, S_, sweep0, seed, beta, temp_x, stride, pmin, parg, best):
            k = np.ctypeslib.as_array(ctypes.cast(kinds, ctypes.POINTER(ctypes.c_int32)), (P_,)).tolist()
            self.calls.append((prec, k, S_, sweep0, seed, beta, temp_x, stride, pmin is not None, parg is not None, best is not None))
            return 0

        def nlmc_nmc_phases_waves_long_refusal(self, ctx, S_):
            return b"too long" if S_ > 4 else None
    eng = P.Engine.__new__(P.Engine)
    eng._L, eng._ctx, eng.n, eng.energy_scale = FakeLib(), None, 300, 4
    assert eng.nmc_phases_waves_long(["C", "NC", "ALL"], 4, 77, (1 << 32) | 7, 2.5, 20.0, min_stride=2) is None
    assert eng._L.calls[-1] == (P._abi.F32, [1, 2, 0], 4, 7, 77, 2.5, 20.0, 2, False, False, False)
    out = eng.nmc_phases_waves_long(["C", "ALL"], 1, 77, 0, 1.0, 20.0, want_minima=True, want_last_best=True)
    assert eng._L.calls[-1][-3:] == (True, True, True)
    assert out["phase_min"].shape == (2, 2) and out["phase_argmin"].shape == (2, 2) and out["last_best"].shape == (2, 300)
    assert eng.nmc_phases_waves_long_refusal(4) is None and eng.nmc_phases_waves_long_refusal(5) == "too long"
