"""APT rounds of short chains in one launch (include/nlmc.h: nlmc_apt_rounds_lanes), the parts that need no GPU: the keyword of
APT_ICM, the header and its binding, APT_ICM._run_device_resident over a CPU double whose engine takes the in-launch call, refuses it,
or has no lane route at all, and the host check of the lane code for disagreement components (scripts/lane_icm_check.cpp)."""
import contextlib
import ctypes
import functools
import io
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from conftest import REPO, load_product
from fake_engine import OracleEngine
from helpers import make_instance
from test_lanes_cpu import header

SEED = 0xA17C0000 + (9 << 32)


# ---- APT_ICM(lanes=...) --------------------------------------------------------------------------------------------------------------
def test_apt_icm_validates_lanes():
    P = load_product()
    J, h = make_instance(16, seed=2)
    with pytest.raises(ValueError, match="lanes must be 'off', 'auto' or 'force'"):
        P.APT_ICM(J, h, rng="philox", lanes="bad")
    with pytest.raises(ValueError, match="lanes applies to rng='philox'"):
        P.APT_ICM(J, h, rng="numpy", lanes="force")
    assert P.APT_ICM(J, h, rng="philox").lanes == "off"
    obj = P.APT_ICM(J, h, rng="philox", seed=1, lanes="force")
    kw = dict(num_sweeps_MCMC=4, num_sweeps_read=4, num_swap_attempts=2)
    with pytest.raises(ValueError, match="lanes"):
        obj.run(np.linspace(0.5, 1.0, 3), 3, icm_feedback=False, **kw)
    with pytest.raises(ValueError, match="lanes"):
        obj.run(np.linspace(0.5, 1.0, 3), 3, icm_feedback=True, device_ids=[0], **kw)


# ---- header, binding, exports --------------------------------------------------------------------------------------------------------
APT_ARGS = (r"\(\s*nlmc_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,"
            r"\s*uint64_t\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int32_t\s*\*\s*\w+\s*\)\s*;")


def test_binding_carries_the_headers_signature():
    P = load_product()
    L = P._abi.lib()
    hdr = header()
    assert re.search(r"int\s+nlmc_apt_rounds_lanes\s*" + APT_ARGS, hdr)
    assert "nlmc_apt_rounds_lanes" in P._abi.EXPORTS and hasattr(L, "nlmc_apt_rounds_lanes")
    f = L.nlmc_apt_rounds_lanes
    assert f.restype is ctypes.c_int
    assert f.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64,
                          ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    assert f(None, P._abi.F32, 1, 1, 0, 0, 1, 1, 1, None) == P._abi.ERR_ARG          # a NULL context: before any device work
    assert re.search(r"#define\s+NLMC_ROUNDS_APT_LANES\s+\(\s*NLMC_ROUNDS_LANES\s*\+\s*1\s*\)", hdr)
    assert int(re.search(r"#define\s+NLMC_ROUNDS_LANES\s+(\d+)", hdr).group(1)) + 1 == P._abi.ROUNDS_APT_LANES == 4


class FakeLib:
    def __init__(self):
        self.route, self.rc, self.calls = 0, 0, []

    def nlmc_pt_rounds_route(self, ctx):
        return self.route

    def nlmc_apt_rounds_lanes(self, ctx, *a):
        self.calls.append(a)
        return self.rc


def test_engine_names_the_route_and_reports_a_refusal(monkeypatch):
    P = load_product()
    eng = P.Engine.__new__(P.Engine)          # no device: the methods under test only talk to the library handle
    eng._L, eng._ctx, eng.ladder_len, eng.n_chains_global = FakeLib(), None, 4, 12
    eng._L.route = 4
    assert eng.last_rounds_route() == "apt lanes"
    ok, info = eng.apt_rounds_lanes(5, 3, SEED, 1 << 32 | 9, 2, 1, katzgraber=False, precision="f64")
    assert ok is True and info is None
    assert eng._L.calls == [(P._abi.F64, 5, 3, 9, 2, SEED, 1, 0, None)]
    ok, info = eng.apt_rounds_lanes(5, 3, SEED, 0, 0, 0, want_info=True)
    assert ok is True and info.shape == (5, 4 * 1, 2) and info.dtype == np.int32
    eng._L.rc = P._abi.ERR_UNSUPPORTED

    class Err:
        @staticmethod
        def nlmc_last_error(ctx):
            return b"refused by the test"
    monkeypatch.setattr(P._abi, "lib", lambda: Err)
    assert eng.apt_rounds_lanes(5, 3, SEED, 0, 0, 1, want_info=True) == (False, None)
    assert eng.rounds_fused_refusal == "refused by the test"


# ---- APT_ICM._run_device_resident over the double ------------------------------------------------------------------------------------
class AptEngine(OracleEngine):
    """The double as APT_ICM's device-resident run drives an engine: the oracle's sweeps, Houdayer step and swap round, a recorded trace,
    a swap log kept until it is read, the lane switch -- and an apt_rounds_lanes that loops the three oracle calls."""
    lane = True
    refuse = False
    made = []

    def __init__(self, inst, betas, n_chains, device=0):
        super().__init__(inst, n_chains, 0, n_chains)
        self.inst = inst
        self.lane_modes, self.in_launch, self.asked, self.single_sweeps, self.pair_plans = [], [], 0, 0, []
        self.fused_calls = self.planned_plain = 0
        self.log = []
        AptEngine.made.append(self)

    def set_lane_sweeps(self, mode):
        assert not hasattr(self, "betas")                     # before pt_init, like every other setting of a fresh engine
        self.lane_modes.append(mode)

    def lanes_take(self, rows=None):
        return self.lane and bool(self.lane_modes) and self.lane_modes[-1] != "off"

    def pt_plan(self, round0, n_rounds, seed, n_pairs):
        self.pair_plans.append((int(round0), int(n_rounds)))

    def pt_log_begin(self, round0, n_rounds, n_pairs):
        self.log = []

    def pt_log_read(self):
        return (np.stack([p for p, _ in self.log]), np.stack([a for _, a in self.log]))

    def pt_swap_philox(self, rnd, seed, n_pairs, want_log=True):
        out = super().pt_swap_philox(rnd, seed, n_pairs)
        self.log.append(out)
        return out

    def sweep_philox(self, n_sweeps, seed, sweep0=0, beta=None, precision="f32", record_stride=0):
        if not getattr(self, "_in_batch", False):
            self.single_sweeps += 1
        rec = []
        for t in range(n_sweeps):
            super().sweep_philox(1, seed, sweep0=sweep0 + t, precision=precision)
            rec.append(self.spins.copy())
        self.recorded = np.stack(rec, axis=1) if rec else np.zeros((self.n_chains, 0, self.n), np.int8)
        return {"spins": self.recorded} if record_stride else {}

    def energy_of_recorded(self, n_rec):
        return np.array([[oracle.energy(self.csr, self.h, s) for s in row] for row in self.recorded])

    def energy(self):
        return np.array([oracle.energy(self.csr, self.h, s) for s in self.spins])

    def apt_rounds_lanes(self, n_rounds, sweeps_per_round, seed, sweep0, round0, n_pairs, katzgraber=True, precision="f32", want_info=False):
        self.asked += 1
        if self.refuse:
            self.rounds_fused_refusal = "refused by the test"
            return False, None
        if n_pairs > 0:                                       # the pair selections are planned before the rounds are handed over
            p0, pn = self.pair_plans[-1]
            assert p0 <= round0 and round0 + n_rounds <= p0 + pn
        self._in_batch = True
        info = []
        for r in range(n_rounds):
            self.sweep_philox(sweeps_per_round, seed, sweep0=sweep0 + r * sweeps_per_round, precision=precision)
            info.append(self.icm_round_ladders(round0 + r, seed, katzgraber, want_info=True))
            if n_pairs > 0:
                self.pt_swap_philox(round0 + r, seed, n_pairs, want_log=False)
        self._in_batch = False
        self.in_launch.append((int(round0), int(n_rounds)))
        return True, (np.stack(info) if want_info else None)


class RefusingEngine(AptEngine):
    refuse = True


class NoLaneEngine(AptEngine):
    lane = False


def run_class(P, monkeypatch, cls, lanes, rounds, in_launch=True, pairs=1):
    N, R, S = 12, 3, 2
    J, h = make_instance(N, seed=5, with_h=True)
    monkeypatch.setattr(P.engine, "APT_LANES_IN_LAUNCH", in_launch)
    obj = P.APT_ICM(J, h, rng="philox", seed=SEED, lanes=lanes)
    monkeypatch.setattr(obj, "_run_device_resident", functools.partial(obj._run_device_resident, engine_factory=cls))
    del AptEngine.made[:]
    with contextlib.redirect_stdout(io.StringIO()):
        M, E = obj.run(np.geomspace(0.4, 1.4, R), R, num_sweeps_MCMC=S * rounds, num_sweeps_read=S * rounds, num_swap_attempts=rounds,
                       num_swapping_pairs=pairs, icm_feedback=True)
    (eng,) = AptEngine.made
    out = {"M": M, "Energy": E, "swap_accepted": obj.swap_accepted, "icm_cluster_sizes": obj.icm_cluster_sizes,
           "final_slots": obj.final_slots}
    return out, eng


@pytest.mark.parametrize("rounds", [5, 34])
def test_in_launch_rounds_give_the_round_by_round_run(monkeypatch, rounds):
    """rounds = 34: the cluster sizes are sampled every second round, and the sample is cut from the in-launch call's rows."""
    P = load_product()
    ref, e0 = run_class(P, monkeypatch, NoLaneEngine, "force", rounds)
    assert not e0.in_launch and e0.asked == 0 and e0.single_sweeps == rounds and e0.lane_modes == ["force"]
    assert ref["swap_accepted"].sum() > 0 and (ref["icm_cluster_sizes"] > 0).any() and ref["M"].any()
    assert not np.array_equal(ref["final_slots"], np.arange(30) % 3)
    assert len(ref["icm_cluster_sizes"]) == 3 * 5 * (rounds if rounds <= 16 else 18)

    got, e1 = run_class(P, monkeypatch, AptEngine, "force", rounds)
    assert e1.in_launch == [(0, rounds - 1)] and e1.asked == 1 and e1.single_sweeps == 1      # the last round keeps its three calls
    assert e1.fused_calls == 0 and e1.planned_plain == 0 and e1.pair_plans == [(0, rounds)]  # no window planned, only the pairs
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k

    got, e2 = run_class(P, monkeypatch, RefusingEngine, "force", rounds)
    assert e2.asked == 1 and not e2.in_launch and e2.single_sweeps == rounds and e2.fused_calls == 0 and e2.planned_plain == 0
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k


def test_the_constant_and_the_keyword_gate_the_in_launch_call(monkeypatch):
    P = load_product()
    assert isinstance(P.engine.APT_LANES_IN_LAUNCH, bool)
    ref, _ = run_class(P, monkeypatch, NoLaneEngine, "force", 4, pairs=0)
    assert ref["swap_accepted"].size == 0
    got, e = run_class(P, monkeypatch, AptEngine, "force", 4, in_launch=False, pairs=0)
    assert e.asked == 0 and e.single_sweeps == 4 and e.lane_modes == ["force"]
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k
    got, e = run_class(P, monkeypatch, AptEngine, "force", 4, pairs=0)                         # rounds without swaps are handed over too
    assert e.in_launch == [(0, 3)] and not e.pair_plans
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k
    got, e = run_class(P, monkeypatch, AptEngine, "off", 4, pairs=0)                           # "off": the engine is left as it was made
    assert e.asked == 0 and e.lane_modes == [] and e.single_sweeps == 4
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k


# ---- the lane code for disagreement components on the host -------------------------------------------------------------------------------
def test_lane_icm_check_builds_and_passes(tmp_path):
    exe = str(tmp_path / "lane_icm_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(REPO, "scripts", "lane_icm_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"75 cases of 64 pairs, 0 wrong", r.stdout), r.stdout
