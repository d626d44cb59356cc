"""Tempering rounds of short chains in one launch (include/nlmc.h: nlmc_pt_rounds_lanes), the parts that need no GPU: the header and its
binding, LocalTempering.run_rounds over the CPU double when the engine runs its sweeps one chain per lane (a chunk then needs only its
pair selections planned and still goes to the batched call), and the validation of NPT(lanes=...)."""
import re

import numpy as np
import pytest

from conftest import load_product
from fake_engine import OracleEngine
from helpers import make_instance, init_spins
from test_lanes_cpu import header

N, SEED, S, ROUNDS, PAIRS = 40, 0xFACE0000 + (3 << 32), 4, 7, 1
LQ, NLQ = 4, 4
G = LQ * NLQ
ROUNDS_ARGS = r"\(\s*nlmc_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint64_t\s+\w+\s*,\s*int\s+\w+\s*\)\s*;"


def test_binding_carries_the_headers_signature():
    import ctypes
    P = load_product()
    L = P._abi.lib()
    hdr = header()
    assert re.search(r"int\s+nlmc_pt_rounds_lanes\s*" + ROUNDS_ARGS, hdr)
    assert re.search(r"int\s+nlmc_pt_rounds_deferred\s*" + ROUNDS_ARGS, hdr)          # (the pattern fits the sibling it was modelled on)
    assert "nlmc_pt_rounds_lanes" in P._abi.EXPORTS
    f = L.nlmc_pt_rounds_lanes
    assert f.restype is ctypes.c_int
    assert f.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64,
                          ctypes.c_int] == L.nlmc_pt_rounds_deferred.argtypes
    assert f(None, P._abi.F32, 1, 1, 0, 0, 1, 1) == P._abi.ERR_ARG                 # a NULL context: before any device work
    consts = {k: int(v) for k, v in re.findall(r"#define\s+NLMC_ROUNDS_(\w+)\s+(\d+)", hdr)}
    assert consts == {"IN_LAUNCH": 1, "LAUNCH_PER_ROUND": 2, "LANES": 3}
    assert (P._abi.ROUNDS_IN_LAUNCH, P._abi.ROUNDS_LAUNCH_PER_ROUND, P._abi.ROUNDS_LANES) == (1, 2, 3)
    assert L.nlmc_abi_version() == 3


class FakeLib:
    """nlmc_pt_rounds_route / nlmc_pt_rounds_lanes of a library that answers what the test tells it to."""
    def __init__(self):
        self.route, self.rc, self.calls = 0, 0, []

    def nlmc_pt_rounds_route(self, ctx):
        return self.route

    def nlmc_pt_rounds_lanes(self, ctx, *a):
        self.calls.append(a)
        return self.rc


def test_engine_names_the_route_and_reports_a_refusal(monkeypatch):
    P = load_product()
    eng = P.Engine.__new__(P.Engine)          # no device: the methods under test only talk to the library handle
    eng._L, eng._ctx = FakeLib(), None
    for code, name in [(0, None), (1, "in launch"), (2, "launch per round"), (3, "lanes")]:
        eng._L.route = code
        assert eng.last_rounds_route() == name
    assert eng.pt_rounds_lanes(5, 3, SEED, 1 << 32 | 9, 2, 1, precision="f64") is True
    assert eng._L.calls == [(P._abi.F64, 5, 3, 9, 2, SEED, 1)]
    eng._L.rc = P._abi.ERR_UNSUPPORTED

    class Err:
        @staticmethod
        def nlmc_last_error(ctx):
            return b"refused by the test"
    monkeypatch.setattr(P._abi, "lib", lambda: Err)
    assert eng.pt_rounds_lanes(5, 3, SEED, 0, 0, 1) is False and eng.rounds_fused_refusal == "refused by the test"


# ---- LocalTempering.run_rounds over the double ---------------------------------------------------------------------------------------
class LaneEngine(OracleEngine):
    """The double as a context with n < 256 presents itself: no fused-window plan (plan_philox_fused answers 0), lanes_take by the
    switch `lane`, a pt_rounds_deferred that records its calls and runs the rounds itself, every planning call counted."""
    lane = True
    refuse = False

    def __init__(self, *a):
        super().__init__(*a)
        self.batched, self.asked, self.single_sweeps, self.pair_plans, self.fused_asked, self.planned_plain = [], 0, 0, [], 0, 0

    def lanes_take(self, rows=None):
        return self.lane

    def plan_philox_fused(self, sweep0, n_windows, window, seed):
        self.fused_asked += 1
        return 0

    def pt_plan(self, round0, n_rounds, seed, n_pairs):
        self.pair_plans.append((int(round0), int(n_rounds)))

    def sweep_philox(self, *a, **k):
        if not getattr(self, "_in_batch", False):
            self.single_sweeps += 1
        return super().sweep_philox(*a, **k)

    def pt_rounds_deferred(self, n_rounds, sweeps_per_round, seed, sweep0, round0, n_pairs, precision="f32"):
        self.asked += 1
        if self.refuse:
            self.rounds_fused_refusal = "refused by the test"
            return False
        p0, pn = self.pair_plans[-1]                          # the chunk's pair selections are planned before it is handed over
        assert p0 <= round0 and round0 + n_rounds <= p0 + pn
        self._in_batch = True
        for r in range(n_rounds):
            self.sweep_philox(sweeps_per_round, seed, sweep0=sweep0 + r * sweeps_per_round, precision=precision)
            self.pt_swap_philox(round0 + r, seed, n_pairs)
        self._in_batch = False
        self.batched.append((int(round0), int(n_rounds)))
        return True

    def last_rounds_route(self):
        return "lanes" if self.batched else None


class NoLaneEngine(LaneEngine):
    lane = False


def drive(P, inst, betas, m0, k, cls, chunk=None, pieces=None, by_round=False, prepare=None):
    lt = P.distributed.LocalTempering(inst, betas, G, SEED, PAIRS, [0] * k, engine_factory=lambda i, n, b, g: cls(i, n, b, g))
    if prepare:
        prepare(lt)
    lt.set_spins(m0)
    lt.plan(ROUNDS * S, ROUNDS, chunk_rounds=chunk)
    trail = []
    if by_round:
        for _ in range(ROUNDS):
            lt.round(S)
            trail.append((lt.gather_spins(), lt.slots().copy()))
    else:
        for n in (pieces or [ROUNDS]):
            lt.run_rounds(n, S)
            trail.append((lt.gather_spins(), lt.slots().copy()))
    assert lt.sweeps_done == ROUNDS * S and lt.rounds_done == ROUNDS
    return trail, lt


@pytest.fixture(scope="module")
def case():
    P = load_product()
    J, h = make_instance(N, seed=5, with_h=True, gaussian=True)
    inst = P.Instance(J, h)
    betas = np.geomspace(0.3, 1.5, LQ)
    m0 = init_spins(G, N)
    ref, _ = drive(P, inst, betas, m0, 1, OracleEngine, by_round=True)           # the state after every round
    assert not np.array_equal(ref[-1][1], np.arange(G) % LQ) and not np.array_equal(ref[-1][0], m0)
    for sp, sl in ref:
        sp.setflags(write=False)
        sl.setflags(write=False)
    return P, inst, betas, m0, ref


@pytest.mark.parametrize("k", [1, 2])
def test_lane_chunks_are_batched_round_by_round_equal(case, k):
    """run_rounds cut after every round: spins and slots equal the round-by-round reference after each of them, every round went
    through the batched call, and nothing but the pair selections was planned."""
    P, inst, betas, m0, ref = case
    trail, lt = drive(P, inst, betas, m0, k, LaneEngine, pieces=[1] * ROUNDS)
    for r, (got, want) in enumerate(zip(trail, ref)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"round {r}"
    for e in lt.engs:
        assert e.batched == [(r, 1) for r in range(ROUNDS)] and e.single_sweeps == 0
        assert e.fused_asked == 0 and e.planned_plain == 0 and e.pair_plans == [(0, ROUNDS)]
    assert lt.deferred_rounds == ROUNDS and lt.deferred_calls == ROUNDS * k and lt.rounds_routes == ["lanes"] * k


@pytest.mark.parametrize("chunk,want", [(None, [(0, 7)]), (3, [(0, 3), (3, 3), (6, 1)])])
def test_lane_chunks_follow_the_planners_chunks(case, chunk, want):
    P, inst, betas, m0, ref = case
    trail, lt = drive(P, inst, betas, m0, 2, LaneEngine, chunk=chunk)
    assert np.array_equal(trail[-1][0], ref[-1][0]) and np.array_equal(trail[-1][1], ref[-1][1])
    for e in lt.engs:
        assert e.batched == want == e.pair_plans and e.single_sweeps == 0 and e.fused_asked == 0 and e.planned_plain == 0
    assert lt.deferred_rounds == ROUNDS and lt.deferred_calls == 2 * len(want)


def test_a_refused_lane_chunk_falls_back_without_a_schedule(case):
    """The engine refuses: the rounds run one by one -- on the lane sweeps, so still nothing but pair selections is planned -- and it
    is not asked again."""
    P, inst, betas, m0, ref = case

    def prepare(lt):
        lt.engs[1].refuse = True
    trail, lt = drive(P, inst, betas, m0, 2, LaneEngine, chunk=3, prepare=prepare)
    assert np.array_equal(trail[-1][0], ref[-1][0]) and np.array_equal(trail[-1][1], ref[-1][1])
    a, b = lt.engs
    assert a.batched == [(0, 3), (3, 3), (6, 1)] and a.single_sweeps == 0
    assert b.asked == 1 and not b.batched and b.single_sweeps == ROUNDS and b.fused_asked == 0 and b.planned_plain == 0
    assert lt.deferred_rounds == 0 and lt.rounds_routes == ["lanes", None]


def test_without_the_lane_route_nothing_changes(case):
    """lanes_take false on a context without fused windows: the fused plan is asked for once and refused, the plain schedule is
    planned, no batched call is made, every round is round()'s -- what such a context did before there was a lane route."""
    P, inst, betas, m0, ref = case
    trail, lt = drive(P, inst, betas, m0, 2, NoLaneEngine, chunk=3)
    assert np.array_equal(trail[-1][0], ref[-1][0]) and np.array_equal(trail[-1][1], ref[-1][1])
    for e in lt.engs:
        assert e.asked == 0 and not e.batched and e.single_sweeps == ROUNDS
        assert e.fused_asked == 1 and e.planned_plain >= 1
    assert lt.deferred_rounds == 0 and lt.deferred_calls == 0 and lt.rounds_routes == [None, None]


def test_lane_sweeps_keyword_reaches_every_engine_made(case):
    P, inst, betas, m0, ref = case
    seen = []

    class Recording(LaneEngine):
        def set_lane_sweeps(self, mode):
            assert not hasattr(self, "betas")                 # before pt_init, like every other setting of a fresh engine
            seen.append(mode)
    mk = lambda i, n, b, g: Recording(i, n, b, g)           # noqa: E731
    P.distributed.LocalTempering(inst, betas, G, SEED, PAIRS, [0, 0], engine_factory=mk, lane_sweeps="force")
    assert seen == ["force", "force"]
    P.distributed.LocalTempering(inst, betas, G, SEED, PAIRS, [0, 0], engine_factory=mk)
    assert seen == ["force", "force"]                         # "off", the default: the engines are left as they were made


# ---- NPT(lanes=...) ------------------------------------------------------------------------------------------------------------------
def test_npt_validates_lanes():
    P = load_product()
    J, h = make_instance(16, seed=2)
    with pytest.raises(ValueError, match="lanes"):
        P.NPT(J, h, rng="philox", lanes="bad")
    with pytest.raises(ValueError, match="lanes"):
        P.NPT(J, h, rng="numpy", lanes="force")
    assert P.NPT(J, h, rng="philox").lanes == "off"
    obj = P.NPT(J, h, rng="philox", seed=1, lanes="force")
    with pytest.raises(ValueError, match="lanes"):
        obj.run(np.linspace(0.5, 1.0, 3), 3, [False, True, False], num_sweeps_MCMC=4, num_sweeps_read=4, num_swap_attempts=2)
