"""engine.RoundPlanner over a stub engine that records its calls: the route the planner names, what it plans on each route, how
many rounds it reports ready for the batched rounds call, and which routes may be batched -- one case per route."""
import pytest

from conftest import load_product

SEED, SWEEP0, ROUND0, ROUNDS, CHUNK = 5, 100, 10, 7, 3        # chunks of rounds [0, 3), [3, 6), [6, 7)


class Stub:
    n = 16

    def __init__(self, lanes=False, waves=False, wave_rounds=False, fused_ok=True):
        self._lanes, self._waves, self.wave_rounds, self.fused_ok = lanes, waves, wave_rounds, fused_ok
        self.calls = []

    def lanes_take(self, rows=None):
        return self._lanes

    def waves_take(self, rows=None, precision="f32"):
        return self._waves

    def pt_plan(self, round0, n_rounds, seed, n_pairs):
        self.calls.append(("pt_plan", round0, n_rounds))

    def plan_slot(self, slot):
        self.calls.append(("plan_slot", slot))

    def plan_philox_fused(self, sweep0, n_windows, window, seed):
        self.calls.append(("plan_philox_fused", sweep0, n_windows, window))
        return n_windows if self.fused_ok else 0

    def plan_philox(self, sweep0, n_sweeps, seed, precision="f32"):
        self.calls.append(("plan_philox", sweep0, n_sweeps))

    def sweep_philox(self, n_sweeps, seed, sweep0=0, beta=None, precision="f32", **outputs):
        self.calls.append(("sweep", sweep0, n_sweeps))

    def taken(self):
        out, self.calls = self.calls, []
        return out


def planner(S=4, **stub):
    eng = Stub(**stub)
    pl = load_product().engine.RoundPlanner(eng, SWEEP0, ROUNDS, S, SEED, chunk_rounds=CHUNK, pt_pairs=1, pt_round0=ROUND0)
    return pl, eng


@pytest.mark.parametrize("route, stub", [("lanes", dict(lanes=True)), ("lanes", dict(lanes=True, waves=True, wave_rounds=True)),
                                         ("wave rounds", dict(waves=True, wave_rounds=True))])
def test_short_chain_routes_with_whole_rounds_plan_pair_selections_only(route, stub):
    pl, eng = planner(**stub)
    assert pl.route() == route
    assert pl.batchable(4) and not pl.batchable(4, by_name=True) and not pl.batchable(5)
    assert pl.rounds_ready(0) == 3 and eng.taken() == [("pt_plan", ROUND0, 3)]              # the first round
    assert pl.rounds_ready(1) == 2 and pl.rounds_ready(2) == 1 and eng.taken() == []        # inside the chunk
    assert pl.rounds_ready(3) == 3 and eng.taken() == [("pt_plan", ROUND0 + 3, 3)]          # the chunk's edge
    assert pl.rounds_ready(6) == 1 and eng.taken() == [("pt_plan", ROUND0 + 6, 1)]
    assert pl.rounds_ready(7) == 0 and pl.rounds_ready(-1) == 0 and eng.taken() == []       # past the end
    assert pl.rounds_ready(6, by_name=True) == 0
    pl.sweep(6)
    assert eng.taken() == [("sweep", SWEEP0 + 24, 4)]
    assert not pl.fused_covers(6) and pl.window == 4                                       # no window was planned or turned down


def test_waves_round_by_round_are_not_batched():
    pl, eng = planner(waves=True)
    assert pl.route() == "waves"
    assert not pl.batchable(4) and not pl.batchable(4, by_name=True)
    assert [pl.rounds_ready(ii) for ii in (0, 1, 3, 7)] == [0, 0, 0, 0] and eng.taken() == []
    pl.sweep(0)
    assert eng.taken() == [("pt_plan", ROUND0, 3), ("sweep", SWEEP0, 4)]
    pl.sweep(1)
    assert eng.taken() == [("sweep", SWEEP0 + 4, 4)]
    pl.sweep(3)
    assert eng.taken() == [("pt_plan", ROUND0 + 3, 3), ("sweep", SWEEP0 + 12, 4)]
    assert not pl.fused_covers(3)


def test_windows_accepted():
    pl, eng = planner()
    assert pl.route() == "windows" and pl.window == 4
    assert pl.batchable(4) and pl.batchable(4, by_name=True) and not pl.batchable(5) and not pl.batchable(5, by_name=True)
    assert pl.rounds_ready(0) == 3
    assert eng.taken() == [("pt_plan", ROUND0, 3), ("plan_slot", 0), ("plan_philox_fused", SWEEP0, 3, 4)]
    assert [pl.fused_covers(ii) for ii in (0, 2, 3)] == [True, True, False]
    assert pl.rounds_ready(1, by_name=True) == 2 and pl.rounds_ready(2) == 1 and eng.taken() == []
    assert pl.rounds_ready(3, by_name=True) == 3
    assert eng.taken() == [("pt_plan", ROUND0 + 3, 3), ("plan_slot", 0), ("plan_philox_fused", SWEEP0 + 12, 3, 4)]
    assert pl.rounds_ready(7) == 0 and eng.taken() == []
    pl.sweep(6)
    assert eng.taken() == [("pt_plan", ROUND0 + 6, 1), ("plan_slot", 0), ("plan_philox_fused", SWEEP0 + 24, 1, 4), ("sweep", SWEEP0 + 24, 4)]
    pl.prepare(6)
    assert pl.fused_covers(6) and eng.taken() == []


def test_rounds_of_several_windows_are_not_batched():
    pl, eng = planner(S=128)
    assert pl.route() == "windows" and pl.window == 64
    assert not pl.batchable(128) and not pl.batchable(128, by_name=True) and pl.rounds_ready(0) == 0 and eng.taken() == []
    pl.sweep(0)
    assert eng.taken() == [("pt_plan", ROUND0, 3), ("plan_slot", 0), ("plan_philox_fused", SWEEP0, 6, 64), ("sweep", SWEEP0, 128)]


def test_windows_refused_by_the_engine():
    pl, eng = planner(fused_ok=False)
    assert pl.route() == "windows" and pl.batchable(4)
    assert pl.rounds_ready(0) == 0
    assert eng.taken() == [("pt_plan", ROUND0, 3), ("plan_slot", 0), ("plan_philox_fused", SWEEP0, 3, 4), ("plan_philox", SWEEP0, 12)]
    assert pl.window == 0 and pl.route() == "plain"                                        # ... and from then on
    assert not pl.batchable(4) and not pl.batchable(4, by_name=True)
    assert [pl.rounds_ready(ii) for ii in (0, 1, 3, 7)] == [0, 0, 0, 0] and eng.taken() == []
    pl.sweep(1)
    assert eng.taken() == [("sweep", SWEEP0 + 4, 4)]
    pl.sweep(3)
    assert eng.taken() == [("pt_plan", ROUND0 + 3, 3), ("plan_philox", SWEEP0 + 12, 12), ("sweep", SWEEP0 + 12, 4)]
    assert not pl.fused_covers(3)


def test_plain():
    pl, eng = planner(S=2)                                                                 # no divisor in 3 .. 64: no window
    assert pl.route() == "plain" and pl.window == 0
    assert not pl.batchable(2) and not pl.batchable(2, by_name=True)
    assert [pl.rounds_ready(ii) for ii in (0, 1, 3, 7)] == [0, 0, 0, 0] and eng.taken() == []
    pl.sweep(0)
    assert eng.taken() == [("pt_plan", ROUND0, 3), ("plan_philox", SWEEP0, 6), ("sweep", SWEEP0, 2)]
    pl.sweep(2)
    assert eng.taken() == [("sweep", SWEEP0 + 4, 2)]
    pl.sweep(1, want_energy=True)                                                          # outputs: no planning either way
    assert eng.taken() == [("sweep", SWEEP0 + 2, 2)]
