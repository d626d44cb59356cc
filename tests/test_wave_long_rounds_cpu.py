"""No GPU needed: the bindings and switches of the tempering rounds of long chains inside a wave launch (k_rounds_waves_long), the
drivers' handling of the wave_long_rounds keyword on the oracle double, the launch-shape rule restated in Python against a table, and
the workgroup's data flow (tests/wavelongrounds.py: fields built once and kept in the chains' regions, chains in turn, the two byte
maps, wave 0's lane-to-pair assignment) held against the oracle double round by round."""
import re

import numpy as np
import pytest

import wavefields
import wavelongrounds
from conftest import load_product
from fake_engine import OracleEngine
from helpers import init_spins
from test_wave_rounds_cpu import SEED, WaveEngine, header


def test_bindings_carry_the_headers_signatures():
    import ctypes
    P = load_product()
    L = P._abi.lib()
    hdr = header()
    assert re.search(r"int\s+nlmc_pt_rounds_waves_long\s*\(\s*nlmc_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*uint32_t\s+\w+\s*,"
                     r"\s*uint32_t\s+\w+\s*,\s*uint64_t\s+\w+\s*,\s*int\s+\w+\s*\)\s*;", hdr)
    assert re.search(r"int\s+nlmc_set_wave_long_rounds\s*\(\s*nlmc_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", hdr)
    assert "nlmc_pt_rounds_waves_long" in P._abi.EXPORTS and "nlmc_set_wave_long_rounds" in P._abi.EXPORTS
    i, vp = ctypes.c_int, ctypes.c_void_p
    assert L.nlmc_pt_rounds_waves_long.restype is i and L.nlmc_pt_rounds_waves_long.argtypes == L.nlmc_pt_rounds_waves.argtypes
    assert L.nlmc_set_wave_long_rounds.restype is i and L.nlmc_set_wave_long_rounds.argtypes == [vp, i]
    assert L.nlmc_pt_rounds_waves_long(None, 0, 1, 1, 0, 0, 0, 1) == P._abi.ERR_ARG   # a NULL context: an argument error, before any device work
    assert L.nlmc_set_wave_long_rounds(None, 1) == P._abi.ERR_ARG
    lanes = int(re.search(r"#define\s+NLMC_ROUNDS_LANES\s+(\d+)", hdr).group(1))
    more = int(re.search(r"#define\s+NLMC_ROUNDS_WAVES_LONG\s+\(\s*NLMC_ROUNDS_LANES\s*\+\s*(\d+)\s*\)", hdr).group(1))
    assert lanes + more == P._abi.ROUNDS_WAVES_LONG == 6
    assert len(set((P._abi.ROUNDS_IN_LAUNCH, P._abi.ROUNDS_LAUNCH_PER_ROUND, P._abi.ROUNDS_LANES, P._abi.ROUNDS_APT_LANES, P._abi.ROUNDS_WAVES,
                    P._abi.ROUNDS_WAVES_LONG))) == 6
    assert P._abi.ABI_VERSION == L.nlmc_abi_version() == 3


class FakeLib:
    def __init__(self):
        self.calls, self.route, self.rc, self.on = [], 0, 0, []

    def nlmc_pt_rounds_waves_long(self, ctx, *a):
        self.calls.append(a)
        return self.rc

    def nlmc_set_wave_long_rounds(self, ctx, on):
        self.on.append(on)
        return 0

    def nlmc_pt_rounds_route(self, ctx):
        return self.route


def test_engine_names_the_route_and_reports_a_refusal(monkeypatch):
    P = load_product()
    eng = P.Engine.__new__(P.Engine)          # no device: the methods under test only talk to the library handle
    eng._L, eng._ctx, eng.wave_long_rounds = FakeLib(), None, False
    eng.set_wave_long_rounds()
    assert eng.wave_long_rounds is True
    for on in (False, 1):
        eng.set_wave_long_rounds(on)
        assert eng.wave_long_rounds is bool(on)
    assert eng._L.on == [1, 0, 1]
    for code, name in ((0, None), (1, "in launch"), (2, "launch per round"), (3, "lanes"), (4, "apt lanes"), (5, "waves"), (6, "waves long")):
        eng._L.route = code
        assert eng.last_rounds_route() == name
    assert eng.pt_rounds_waves_long(4, 3, SEED, 6, 2, 1) is True
    assert eng._L.calls == [(P._abi.F32, 4, 3, 6, 2, SEED, 1)]
    eng._L.rc = P._abi.ERR_UNSUPPORTED

    class Lib:
        @staticmethod
        def nlmc_last_error(ctx):
            return b"nlmc_pt_rounds_waves_long: the ladders of a workgroup do not fit its LDS"
    monkeypatch.setattr(P._abi, "lib", lambda: Lib)
    assert eng.pt_rounds_waves_long(4, 3, SEED, 6, 2, 1, precision="f64") is False
    assert eng.rounds_fused_refusal == "nlmc_pt_rounds_waves_long: the ladders of a workgroup do not fit its LDS" and eng._L.calls[-1][0] == P._abi.F64
    eng._ctx = None                            # (nothing for __del__ to destroy)


class LongWaveEngine(WaveEngine):
    """WaveEngine with the two long-chain switches; its batched rounds call says "waves long" when all of them are on."""

    def __init__(self, *a):
        super().__init__(*a)
        self.wave_long, self.wave_long_rounds = False, False

    def set_wave_long(self, on=True):
        self.wave_long = bool(on)

    def set_wave_long_rounds(self, on=True):
        self.wave_long_rounds = bool(on)

    def last_rounds_route(self):
        return "waves long" if self.wave_rounds and self.wave_long and self.wave_long_rounds else "launch per round"


def drive(P, parts=None, **kw):
    J, h = wavefields.dense_instance(8, seed=2)
    L, ladders, rounds, S, pairs = 4, 2, 7, 2, 1
    G = L * ladders
    parts = parts or [(0, G)]
    lt = P.distributed.LocalTempering(P.Instance(J, h), np.geomspace(0.3, 1.5, L), G, SEED, pairs, list(range(len(parts))), parts=parts,
                                      engine_factory=LongWaveEngine, **kw)
    lt.set_spins(init_spins(G, 8))
    lt.plan(rounds * S, rounds)
    lt.run_rounds(rounds, S)
    out = {"spins": lt.gather_spins(), "slots": lt.slots(), "calls": [e.deferred for e in lt.engs], "routes": lt.rounds_routes,
           "switches": [(e.wave_rounds, e.wave_long, e.wave_long_rounds) for e in lt.engs]}
    lt.close()
    return out


def test_the_keyword_reaches_every_engine_and_needs_both_wave_rounds_and_wave_long():
    P = load_product()
    parts = [(0, 4), (4, 4)]
    on = dict(wave_sweeps="force", wave_rounds=True, wave_long=True)
    got = drive(P, parts, wave_long_rounds=True, **on)
    assert got["switches"] == [(True, True, True)] * 2 and got["routes"] == ["waves long"] * 2 and got["calls"] == [[(7, 2, 0, 0)]] * 2
    ref = drive(P, parts, **on)
    assert ref["switches"] == [(True, True, False)] * 2 and ref["routes"] == ["launch per round"] * 2
    assert np.array_equal(got["spins"], ref["spins"]) and np.array_equal(got["slots"], ref["slots"])
    assert not np.array_equal(got["slots"], np.arange(8) % 4)
    for missing in ("wave_rounds", "wave_long"):
        kw = dict(on, wave_long_rounds=True)
        kw[missing] = False
        with pytest.raises(ValueError, match="wave_long_rounds needs wave_rounds=True and wave_long=True"):
            drive(P, parts, **kw)
        with pytest.raises(ValueError, match="wave_long_rounds needs"):
            P.hostlogic.check_route_keywords(waves="force", rng="philox", wave_long_rounds=True,
                                             **{k: v for k, v in kw.items() if k in ("wave_rounds", "wave_long")})
        with pytest.raises(ValueError, match="wave_long_rounds needs"):
            P.hostlogic.set_route_modes(LongWaveEngine(P.Instance(*wavefields.dense_instance(8)), 4, 0, 4), waves="force", wave_long_rounds=True,
                                        **{k: v for k, v in kw.items() if k in ("wave_rounds", "wave_long")})
    P.hostlogic.check_route_keywords(waves="force", wave_rounds=True, wave_long=True, rng="philox", wave_long_rounds=True)
    J, h = wavefields.dense_instance(8)
    all_on = dict(rng="philox", seed=1, waves="force", wave_rounds=True, wave_long=True)
    assert P.NPT(J, h, wave_long_rounds=True, **all_on).wave_long_rounds is True
    assert P.NPT(J, h, **all_on).wave_long_rounds is False
    for missing in ("wave_rounds", "wave_long"):
        with pytest.raises(ValueError, match="wave_long_rounds needs"):
            P.NPT(J, h, wave_long_rounds=True, **dict(all_on, **{missing: False}))
    # doNMC slots stay refused, as with wave_rounds alone
    obj = P.NPT(J, h, wave_long_rounds=True, **all_on)
    with pytest.raises(ValueError, match="wave_rounds runs plain replicas only"):
        obj.run(np.geomspace(0.3, 2.0, 4), 4, [False, True, False, False], num_sweeps_MCMC=4, num_sweeps_read=4, num_swap_attempts=2,
                num_swapping_pairs=1)
    assert P.engine.WAVE_LONG_ROUNDS_IN_LAUNCH in (True, False)


# (n, L, ladders, n_cu, knob) -> (R, P, C, W, blocks), or None: refused.  Worked out by hand from the rule and the region sizes: a chain
# is 2048 + n_pad bytes at n <= 512 and 4096 + n_pad beyond, a wave's thresholds 16 ceil(n / 4), then 8 Q + 2 Q bytes rounded up to 16.
SHAPES = [
    ((257, 5, 7, 256, 3), (8, 3, 1, 15, 3)),             # three ladders a workgroup, the last workgroup holds one
    ((257, 5, 7, 256, 0), (8, 1, 1, 5, 7)),              # the compute units first: a ladder per workgroup
    ((257, 5, 7, 2, 0), (8, 3, 1, 15, 3)),               # two compute units: ceil(7 / 2) = 4 ladders asked, three fit 16 waves
    ((512, 4, 3, 256, 0), (8, 1, 1, 4, 3)),              # the register boundary: 8 fields per lane ..
    ((513, 4, 3, 256, 0), (16, 1, 1, 4, 3)),             # .. and 16
    ((1024, 16, 1, 256, 0), (16, 1, 1, 16, 1)),          # sixteen regions of 9216 bytes + tables: 147616 bytes
    ((1024, 64, 1, 256, 0), None),                       # the field copies alone are 256 KB
    ((1024, 22, 1, 256, 0), (16, 1, 2, 11, 1)),          # 22 x 5120 + 11 x 4096 + 176 + 48 = 157920 <= 161792
    ((1024, 23, 1, 256, 0), None),                       # 23 x 5120 + 12 x 4096 = 166912
    ((300, 17, 2, 256, 0), (8, 1, 2, 9, 2)),             # a ladder of 17: two chains in turn on nine waves
    ((300, 33, 2, 256, 0), (8, 1, 3, 11, 2)),            # uneven turns
    ((300, 64, 1, 256, 0), None),                        # 64 x 2352 + 16 x 1200 = 169728
    ((1024, 5, 40, 256, 8), (16, 4, 2, 10, 10)),         # the knob asks for 8 ladders, 64 / 5 allows 12: the LDS holds 4 (20 chains)
    ((1024, 4, 40, 256, 99), (16, 5, 2, 10, 8)),         # likewise: 16 by the knob's cap, 5 by the LDS
    ((256, 5, 7, 256, 0), None), ((1025, 5, 7, 256, 0), None), ((300, 65, 1, 256, 0), None), ((300, 0, 1, 256, 0), None),
    ((300, 5, 0, 256, 0), None),
]


@pytest.mark.parametrize("case,want", SHAPES, ids=[str(c) for c, _ in SHAPES])
def test_launch_shape_rule(case, want):
    n, L, ladders, n_cu, knob = case
    n_pad = (n + 15) // 16 * 16
    s = wavelongrounds.launch_shape(n, n_pad, L, ladders, n_cu, knob)
    if want is None:
        assert s is None
        return
    assert (s["R"], s["P"], s["C"], s["W"], s["blocks"]) == want
    Q = s["P"] * L
    assert s["lds"] <= wavelongrounds.LDS_MAX and s["W"] <= 16 and Q <= 64 and s["blocks"] * s["P"] >= ladders > (s["blocks"] - 1) * s["P"]
    owned = sorted(w + t * s["W"] for w in range(s["W"]) for t in range(s["C"]) if w + t * s["W"] < Q)
    assert owned == list(range(Q))                                                   # every chain has exactly one wave
    g = wavelongrounds.layout(n, n_pad, Q, s["W"])
    assert all(g[k] % 16 == 0 for k in g) and g["chain_bytes"] >= 256 * s["R"] + n_pad and g["w_bytes"] >= 4 * n
    assert g["w_off"] == Q * g["chain_bytes"] and g["e_off"] >= g["w_off"] + s["W"] * g["w_bytes"] and g["map_off"] >= g["e_off"] + 8 * Q
    assert g["total"] >= g["map_off"] + 2 * Q and g["total"] == s["lds"]
    if case == (1024, 16, 1, 256, 0):
        assert s["lds"] == 147616


def test_the_header_and_the_restatement_agree_on_the_layout_constants():
    """What the Python rule assumes of csrc/nlmc_wave_shape.h, read from its text: the LDS ceiling and the chain-length limits."""
    import os
    from conftest import REPO
    text = open(os.path.join(REPO, "nonlocal-monte-carlo_amd", "csrc", "nlmc_wave_shape.h")).read()
    assert re.search(r"#define\s+NLMC_WAVE_LONG_LDS_MAX\s+\(\(size_t\)158\s*\*\s*1024\)", text)
    assert re.search(r"#define\s+NLMC_WAVE_LONG_MIN_N\s+257", text) and re.search(r"#define\s+NLMC_WAVE_LONG_MAX_N\s+1024", text)
    assert "nlmc_wave_long_rounds_shape(int n, int n_pad, int L, int ladders, int n_cu, int knob_ladders)" in text
    assert "nlmc_wave_long_rounds_layout" in open(os.path.join(REPO, "nonlocal-monte-carlo_amd", "csrc", "nlmc_wave_long_rounds.h")).read()


@pytest.mark.parametrize("L,P_", [(5, 3), (17, 1)], ids=["L5-three-ladders", "L17-chains-in-turn"])
def test_workgroup_data_flow_against_the_oracle_round_by_round(L, P_):
    """n = 260 dense with a diagonal.  L = 5, three ladders on 15 waves with a chain each; L = 17, one ladder on nine waves, eight of
    them with two chains in turn.  A workgroup in the middle of the chain set: ladder0 = 2, so keys and chains are global.  The
    fields are built once per chain, whatever the number of rounds."""
    P = load_product()
    n = 260
    J, h = wavefields.dense_instance(n, seed=4, diag=True)
    Q = L * P_
    s = wavelongrounds.launch_shape(n, 272, L, P_, 1, P_)
    assert (s["P"], s["C"], s["W"]) == ((3, 1, 15) if L == 5 else (1, 2, 9))
    ladder0, rounds, T, pairs = 2, 3, 2, max(1, L // 3)
    chain0, G = ladder0 * L, (ladder0 + P_ + 1) * L
    betas = np.linspace(0.05, 0.05 + 0.002 * (L - 1), L)          # a dense instance's scale, close rungs: chains move, swaps are accepted
    r = np.random.default_rng(5)
    slots0 = np.concatenate([r.permutation(L) for _ in range(G // L)]).astype(np.int32)
    m0 = init_spins(Q, n)
    o = OracleEngine(P.Instance(J, h), Q, chain0, G)
    o.pt_init(betas)
    o.pt_set_slots(slots0)
    o.set_spins(m0)
    flow = wavelongrounds.workgroup_rounds(J, h, m0, slots0[chain0:chain0 + Q], o.efix.copy(), betas, L, P_, ladder0, chain0, rounds, T, pairs,
                                           SEED, sweep0=3, round0=1)
    accepted = 0
    for rr, (s_, slots, efix, prs, acc, builds) in enumerate(flow):
        o.sweep_philox(T, SEED, sweep0=3 + rr * T)
        e_before = o.efix.copy()
        po, ao = o.pt_swap_philox(1 + rr, SEED, pairs)
        assert np.array_equal(s_, o.get_spins()), rr
        assert np.array_equal(efix, e_before), rr
        assert np.array_equal(slots, o.pt_slots()[chain0:chain0 + Q]), rr
        assert np.array_equal(prs, po) and np.array_equal(acc, ao), rr
        assert builds == Q
        accepted += int(acc.sum())
    assert rr == rounds - 1 and accepted > 0 and not np.array_equal(o.get_spins(), m0)
    assert not np.array_equal(o.pt_slots()[chain0:chain0 + Q], slots0[chain0:chain0 + Q])
