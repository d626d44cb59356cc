"""No GPU needed: the bindings and switches of the tempering rounds inside a wave launch (k_rounds_waves), the drivers' handling of
the wave_rounds keyword on the oracle double, and the workgroup's data flow (tests/waverounds.py: chains in turn with parked fields,
the two byte maps, wave 0's lane-to-pair assignment) held against the oracle double round by round."""
import re

import numpy as np
import pytest

import waverounds
import wavefields
from conftest import GOLDEN, REPO, load_product
from fake_engine import OracleEngine
from helpers import make_instance, init_spins

SEED = 0xC3C30000 + (11 << 32)          # high bits set


def header():
    import os
    text = open(os.path.join(REPO, "include", "nlmc.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_bindings_carry_the_headers_signatures():
    import ctypes
    P = load_product()
    L = P._abi.lib()
    hdr = header()
    assert re.search(r"int\s+nlmc_pt_rounds_waves\s*\(\s*nlmc_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*uint32_t\s+\w+\s*,"
                     r"\s*uint32_t\s+\w+\s*,\s*uint64_t\s+\w+\s*,\s*int\s+\w+\s*\)\s*;", hdr)
    assert re.search(r"int\s+nlmc_set_wave_rounds\s*\(\s*nlmc_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", hdr)
    assert "nlmc_pt_rounds_waves" in P._abi.EXPORTS and "nlmc_set_wave_rounds" in P._abi.EXPORTS
    i, u32, u64, vp = ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    assert L.nlmc_pt_rounds_waves.restype is i and L.nlmc_pt_rounds_waves.argtypes == [vp, i, i, i, u32, u32, u64, i]
    assert L.nlmc_pt_rounds_waves.argtypes == L.nlmc_pt_rounds_lanes.argtypes
    assert L.nlmc_set_wave_rounds.restype is i and L.nlmc_set_wave_rounds.argtypes == [vp, i]
    assert L.nlmc_pt_rounds_waves(None, 0, 1, 1, 0, 0, 0, 1) == P._abi.ERR_ARG        # a NULL context: an argument error, before any device work
    assert L.nlmc_set_wave_rounds(None, 1) == P._abi.ERR_ARG
    lanes = int(re.search(r"#define\s+NLMC_ROUNDS_LANES\s+(\d+)", hdr).group(1))
    more = int(re.search(r"#define\s+NLMC_ROUNDS_WAVES\s+\(\s*NLMC_ROUNDS_LANES\s*\+\s*(\d+)\s*\)", hdr).group(1))
    assert lanes + more == P._abi.ROUNDS_WAVES == 5
    assert len(set((P._abi.ROUNDS_IN_LAUNCH, P._abi.ROUNDS_LAUNCH_PER_ROUND, P._abi.ROUNDS_LANES, P._abi.ROUNDS_APT_LANES, P._abi.ROUNDS_WAVES))) == 5


class FakeLib:
    def __init__(self):
        self.calls, self.route, self.rc, self.on = [], 0, 0, []

    def nlmc_pt_rounds_waves(self, ctx, *a):
        self.calls.append(a)
        return self.rc

    def nlmc_set_wave_rounds(self, ctx, on):
        self.on.append(on)
        return 0

    def nlmc_pt_rounds_route(self, ctx):
        return self.route


def test_engine_names_the_route_and_reports_a_refusal(monkeypatch):
    P = load_product()
    eng = P.Engine.__new__(P.Engine)          # no device: the methods under test only talk to the library handle
    eng._L, eng._ctx, eng.wave_rounds = FakeLib(), None, False
    for on in (True, False, 1):
        eng.set_wave_rounds(on)
        assert eng.wave_rounds is bool(on)
    assert eng._L.on == [1, 0, 1]
    for code, name in ((0, None), (1, "in launch"), (2, "launch per round"), (3, "lanes"), (4, "apt lanes"), (5, "waves")):
        eng._L.route = code
        assert eng.last_rounds_route() == name
    assert eng.pt_rounds_waves(4, 3, SEED, 6, 2, 1) is True
    assert eng._L.calls == [(P._abi.F32, 4, 3, 6, 2, SEED, 1)]
    eng._L.rc = P._abi.ERR_UNSUPPORTED

    class Lib:
        @staticmethod
        def nlmc_last_error(ctx):
            return b"nlmc_pt_rounds_waves: no swap pairs"
    monkeypatch.setattr(P._abi, "lib", lambda: Lib)
    assert eng.pt_rounds_waves(4, 3, SEED, 6, 2, 1, precision="f64") is False
    assert eng.rounds_fused_refusal == "nlmc_pt_rounds_waves: no swap pairs" and eng._L.calls[-1][0] == P._abi.F64
    eng._ctx = None                            # (nothing for __del__ to destroy)


class WaveEngine(OracleEngine):
    """The oracle double with the switches of an engine whose sweeps run one chain per wave, and a batched rounds call that counts
    its calls and runs the rounds one by one on the oracle (or refuses)."""
    n_made = 0

    def __init__(self, *a):
        super().__init__(*a)
        self.wave_sweeps, self.wave_rounds, self.deferred, self.refuse = "off", False, [], False
        self.fused_ok = False
        WaveEngine.n_made += 1

    def set_wave_sweeps(self, mode):
        self.wave_sweeps = mode

    def set_wave_rounds(self, on):
        self.wave_rounds = bool(on)

    def waves_take(self, rows=None, precision="f32"):
        return self.wave_sweeps == "force" and precision == "f32"

    def lanes_take(self, rows=None):
        return False

    def pt_rounds_deferred(self, n_rounds, T, seed, sweep0, round0, n_pairs, precision="f32"):
        self.deferred.append((n_rounds, T, sweep0, round0))
        if self.refuse or not (self.wave_rounds and self.waves_take(precision=precision)):
            self.rounds_fused_refusal = "refused"
            return False
        for r in range(n_rounds):
            self.sweep_philox(T, seed, sweep0=sweep0 + r * T, precision=precision)
            self.pt_swap_philox(round0 + r, seed, n_pairs)
        return True

    def last_rounds_route(self):
        return "waves"


def drive(P, wave_rounds, chunk=None, refuse=False, parts=None, wave_sweeps="force"):
    J, h = wavefields.dense_instance(8, seed=2)
    inst = P.Instance(J, h)
    L, ladders, rounds, S, pairs = 4, 2, 7, 2, 1
    G = L * ladders
    parts = parts or [(0, G)]
    lt = P.distributed.LocalTempering(inst, np.geomspace(0.3, 1.5, L), G, SEED, pairs, list(range(len(parts))), parts=parts,
                                      engine_factory=WaveEngine, wave_sweeps=wave_sweeps, wave_rounds=wave_rounds)
    for e in lt.engs:
        e.refuse = refuse
    lt.set_spins(init_spins(G, 8))
    lt.plan(rounds * S, rounds, **({"chunk_rounds": chunk} if chunk else {}))
    lt.run_rounds(rounds, S)
    out = {"spins": lt.gather_spins(), "slots": lt.slots(), "calls": [e.deferred for e in lt.engs], "routes": lt.rounds_routes,
           "deferred_rounds": lt.deferred_rounds, "planned_plain": [getattr(e, "planned_plain", 0) for e in lt.engs],
           "fused_calls": [getattr(e, "fused_calls", 0) for e in lt.engs], "wave_rounds": [e.wave_rounds for e in lt.engs]}
    lt.close()
    return out


def test_driver_chunks_follow_the_planners_chunks():
    P = load_product()
    ref = drive(P, False)
    assert ref["calls"] == [[]] and ref["routes"] == [None] and ref["deferred_rounds"] == 0      # off: no batched call is ever made
    assert not np.array_equal(ref["slots"], np.arange(8) % 4)
    one = drive(P, True)
    assert one["calls"] == [[(7, 2, 0, 0)]] and one["routes"] == ["waves"] and one["deferred_rounds"] == 7
    cut = drive(P, True, chunk=3)
    assert cut["calls"] == [[(3, 2, 0, 0), (3, 2, 6, 3), (1, 2, 12, 6)]] and cut["deferred_rounds"] == 7
    for got in (one, cut):
        assert np.array_equal(got["spins"], ref["spins"]) and np.array_equal(got["slots"], ref["slots"])
        assert got["planned_plain"] == [0] and got["fused_calls"] == [0]                         # no level schedule, no window asked for


def test_a_refused_chunk_falls_back_without_a_schedule():
    P = load_product()
    ref, got = drive(P, False), drive(P, True, chunk=3, refuse=True)
    assert got["calls"] == [[(3, 2, 0, 0)]] and got["routes"] == [None] and got["deferred_rounds"] == 0      # asked once, not again
    assert np.array_equal(got["spins"], ref["spins"]) and np.array_equal(got["slots"], ref["slots"])
    assert got["planned_plain"] == [0] and got["fused_calls"] == [0]


def test_the_keyword_reaches_every_engine_and_needs_the_wave_sweeps():
    P = load_product()
    got = drive(P, True, parts=[(0, 4), (4, 4)])
    assert got["wave_rounds"] == [True, True] and got["calls"] == [[(7, 2, 0, 0)], [(7, 2, 0, 0)]] and got["routes"] == ["waves", "waves"]
    ref = drive(P, False, parts=[(0, 4), (4, 4)])
    assert ref["wave_rounds"] == [False, False] and ref["calls"] == [[], []]
    assert np.array_equal(got["spins"], ref["spins"]) and np.array_equal(got["slots"], ref["slots"])
    with pytest.raises(ValueError, match="wave_rounds needs wave_sweeps"):
        drive(P, True, wave_sweeps="off")
    J, h = wavefields.dense_instance(8)
    assert P.NPT(J, h, rng="philox", seed=1, waves="force", wave_rounds=True).wave_rounds is True
    assert P.NPT(J, h, rng="philox", seed=1, waves="force").wave_rounds is False
    with pytest.raises(ValueError, match="wave_rounds needs waves"):
        P.NPT(J, h, rng="philox", seed=1, wave_rounds=True)
    with pytest.raises(ValueError):
        P.NPT(J, h, rng="philox", seed=1, precision="f64", waves="force", wave_rounds=True)


@pytest.mark.parametrize("L,P_,instance", [(5, 3, "sparse"), (17, 1, "dense")], ids=["L5-three-ladders", "L17-chains-in-turn"])
def test_workgroup_data_flow_against_the_oracle_round_by_round(L, P_, instance):
    """L = 5, three ladders on 15 waves with a chain each; L = 17, one ladder on nine waves, eight of them with two chains in turn and
    parked fields.  A workgroup in the middle of the chain set: ladder0 = 2, so keys and chains are global."""
    P = load_product()
    if instance == "sparse":
        Js, h = make_instance(37, seed=9, with_h=True, gaussian=True)
        J = Js.toarray()
    else:
        J, h = wavefields.dense_instance(12, seed=4, diag=True)
    n = J.shape[0]
    Q, C, W = waverounds.launch_shape(L, P_)
    assert (Q, C, W) == ((15, 1, 15) if L == 5 else (17, 2, 9))
    ladder0, rounds, T, pairs = 2, 4, 2, max(1, L // 3)
    chain0, G = ladder0 * L, (ladder0 + P_ + 1) * L
    betas = np.geomspace(0.3, 1.5, L)
    r = np.random.default_rng(5)
    slots0 = np.concatenate([r.permutation(L) for _ in range(G // L)]).astype(np.int32)
    m0 = init_spins(Q, n)
    o = OracleEngine(P.Instance(J, h), Q, chain0, G)
    o.pt_init(betas)
    o.pt_set_slots(slots0)
    o.set_spins(m0)
    flow = waverounds.workgroup_rounds(J, h, m0, slots0[chain0:chain0 + Q], o.efix.copy(), betas, L, P_, ladder0, chain0, rounds, T, pairs,
                                       SEED, sweep0=3, round0=1)
    accepted = 0
    for rr, (s, slots, efix, prs, acc) in enumerate(flow):
        o.sweep_philox(T, SEED, sweep0=3 + rr * T)
        e_before = o.efix.copy()
        po, ao = o.pt_swap_philox(1 + rr, SEED, pairs)
        assert np.array_equal(s, o.get_spins()), rr
        assert np.array_equal(efix, e_before), rr
        assert np.array_equal(slots, o.pt_slots()[chain0:chain0 + Q]), rr
        assert np.array_equal(prs, po) and np.array_equal(acc, ao), rr
        accepted += int(acc.sum())
    assert rr == rounds - 1 and accepted > 0 and not np.array_equal(o.get_spins(), m0)
