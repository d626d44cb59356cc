"""No GPU needed: the wave-per-chain route's bindings and switches, its premise -- resident integer fields corrected on flips give the
spec's bits -- under the oracle alone, and the premise of its known-answer GPU test."""
import re

import numpy as np
import pytest

import oracle
import wavefields
from conftest import GOLDEN, REPO, load_product
from helpers import make_instance, init_spins

SEED = 0xA5A50000 + (7 << 32)          # high bits set


def header():
    import os
    text = open(os.path.join(REPO, "include", "nlmc.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_bindings_carry_the_headers_signatures():
    import ctypes
    P = load_product()
    L = P._abi.lib()
    hdr = header()
    assert re.search(r"int\s+nlmc_set_wave_sweeps\s*\(\s*nlmc_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", hdr)
    assert "nlmc_set_wave_sweeps" in P._abi.EXPORTS
    assert L.nlmc_set_wave_sweeps.restype is ctypes.c_int and L.nlmc_set_wave_sweeps.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert L.nlmc_set_wave_sweeps(None, 1) == P._abi.ERR_ARG           # a NULL context: an argument error, before any device work
    assert int(re.search(r"#define\s+NLMC_WAVE_N\s+(\d+)", hdr).group(1)) == P._abi.WAVE_N == 256
    assert int(re.search(r"#define\s+NLMC_WAVE_AUTO_MAX_ROWS\s+(\d+)", hdr).group(1)) == P._abi.WAVE_AUTO_MAX_ROWS
    tail = re.search(r"NLMC_ROUTE_LANES\s*=\s*(\d+)\s*,\s*NLMC_ROUTE_WAVES\s*=\s*(\d+)\s*}", hdr)
    assert tuple(map(int, tail.groups())) == (P._abi.ROUTE_LANES, P._abi.ROUTE_WAVES) == (3, 4)
    assert (P._abi.WAVES_OFF, P._abi.WAVES_AUTO, P._abi.WAVES_FORCE) == (0, 1, 2)
    assert L.nlmc_abi_version() == 3


class FakeLib:
    def __init__(self):
        self.modes, self.route = [], 0

    def nlmc_set_wave_sweeps(self, ctx, mode):
        self.modes.append(mode)
        return 0

    def nlmc_last_sweep_route(self, ctx):
        return self.route

    def nlmc_subset_count(self, ctx):
        return 7


def test_engine_maps_the_three_modes_and_the_routes():
    P = load_product()
    eng = P.Engine.__new__(P.Engine)          # no device: the methods under test only talk to the library handle
    eng._L, eng._ctx, eng.n, eng.lane_sweeps, eng.wave_sweeps = FakeLib(), None, 40, "off", "off"
    assert not eng.waves_take() and not eng.waves_take(1)              # off: never
    for mode in ("off", "auto", "force"):
        eng.set_wave_sweeps(mode)
        assert eng.wave_sweeps == mode
    assert eng._L.modes == [P._abi.WAVES_OFF, P._abi.WAVES_AUTO, P._abi.WAVES_FORCE] == [0, 1, 2]
    for bad in ("on", "", None, 1):
        with pytest.raises(ValueError):
            eng.set_wave_sweeps(bad)
    assert eng._L.modes == [0, 1, 2] and eng.wave_sweeps == "force"
    for code, name in ((0, None), (1, "stepwise"), (2, "fused"), (3, "lanes"), (4, "waves")):
        eng._L.route = code
        assert eng.last_sweep_route() == name
    assert P.Engine.ROUTES[4] == "waves"
    # the rule sweep_philox_windows asks before lanes_take and before it plans fused windows (nlmc_set_wave_sweeps)
    assert eng.waves_take() and eng.waves_take(10 ** 6)
    assert not eng.waves_take(precision="f64")
    eng.n = 256
    assert eng.waves_take()
    eng.n = 257
    assert not eng.waves_take()
    eng.n, eng.wave_sweeps = 40, "auto"
    top = P._abi.WAVE_AUTO_MAX_ROWS            # auto: up to that many rows (2^31 - 1: every int row count)
    assert eng.waves_take(top) and (top == 2 ** 31 - 1 or not eng.waves_take(top + 1))
    assert not eng.waves_take(top, precision="f64")
    eng.n = 257
    assert not eng.waves_take(top)
    eng.n = 40
    eng.wave_sweeps = "off"
    assert not eng.waves_take(1)
    assert not eng.lanes_take()                # the lane switch is its own
    eng._ctx = None                            # (nothing for __del__ to destroy)


def test_keywords_of_the_classes():
    """waves="off" | "auto" | "force", rng="philox" only, and not with NPT's precision="f64"."""
    P = load_product()
    J, h = wavefields.dense_instance(8)
    for cls in (P.NPT, P.APT_ICM, P.APT_preprocessor):
        assert cls(J, h, rng="philox", seed=1).waves == "off"
        assert cls(J, h, rng="philox", seed=1, waves="force").waves == "force"
        with pytest.raises(ValueError, match="waves must be"):
            cls(J, h, rng="philox", seed=1, waves="on")
        with pytest.raises(ValueError, match="waves applies to rng='philox'"):
            cls(J, h, rng="numpy", seed=1, waves="force")
    with pytest.raises(ValueError, match="waves applies to precision='f32'"):
        P.NPT(J, h, rng="philox", seed=1, precision="f64", waves="force")


def against_oracle(J, h, m0, cb, seed, chain, group, sweep0=0, flags=None):
    csr = oracle.Csr(J)
    esc = oracle.field_scale(csr, h)[1]
    M, s_fin, tr = oracle.sweeps_philox(csr, h, m0, cb, seed, chain, order_group=group, sweep0=sweep0, flags=flags, escale=esc,
                                        use_f64=False, efix0=12345)
    Mw, sw, trw = wavefields.sweeps(J, h, m0, cb, seed, chain, order_group=group, sweep0=sweep0, flags=flags, escale=esc, efix0=12345)
    assert np.array_equal(M, Mw) and np.array_equal(s_fin, sw) and np.array_equal(tr, trw)
    return M


@pytest.mark.parametrize("per_chain", [False, True], ids=["shared", "per_chain"])
def test_resident_fields_give_the_specs_bits_dense_with_diagonal(per_chain):
    J, h = wavefields.dense_instance(12, diag=True)
    S, chain = 6, 5
    cb = np.tile(np.array(oracle.cb_pair(1.1)), (S, 1))
    M = against_oracle(J, h, init_spins(8, 12)[chain], cb, SEED, chain, chain + 1 if per_chain else 0, sweep0=5)
    assert len({M[t].tobytes() for t in range(S)}) > 1         # the chain moves


@pytest.mark.parametrize("per_chain", [False, True], ids=["shared", "per_chain"])
def test_resident_fields_give_the_specs_bits_with_phase_flags(per_chain):
    N, R, S = 70, 4, 4
    J, h = make_instance(N, seed=3, with_h=True)
    m0 = init_spins(R, N)
    flags = wavefields.phase_flags(R, N, m0)
    assert set(np.unique(flags)) == {0, 1, 2, 3}
    cb = np.tile(np.array(oracle.cb_pair(2.0, 20.0)), (S, 1))
    for c in range(R):                                         # (the last chain has all its spins frozen)
        M = against_oracle(J.toarray(), h, m0[c], cb, SEED, c, c + 1 if per_chain else 0, sweep0=7, flags=flags[c])
        frozen = flags[c] >= 2
        assert np.array_equal(M[-1][frozen], m0[c][frozen])
    assert np.array_equal(M[-1], m0[R - 1])


@pytest.mark.parametrize("per_chain", [False, True], ids=["shared", "per_chain"])
def test_resident_fields_give_the_specs_bits_wishart(per_chain):
    J, h, _, _ = wavefields.wishart(load_product(), GOLDEN)
    S, chain = 8, 3
    cb = np.tile(np.array(oracle.cb_pair(3.0)), (S, 1))
    against_oracle(J, h, init_spins(8, 10)[chain], cb, SEED, chain, chain + 1 if per_chain else 0, sweep0=2)


@pytest.mark.parametrize("per_chain", [False, True], ids=["shared", "per_chain"])
def test_known_answer_premise_under_the_oracle_alone(per_chain):
    """tests/test_gpu_waves.py::test_known_answer_wishart_ground_state: Wishart N = 10 instance 1 divided by max |J|, 64 chains from
    init_spins, 20 f32 sweeps at the example's beta = 3, seed 5 -- the oracle's chains reach the listed ground-state energy."""
    J, h, nf, e_gs = wavefields.wishart(load_product(), GOLDEN)
    csr = oracle.Csr(J)
    esc = oracle.field_scale(csr, h)[1]
    m0 = init_spins(64, 10)
    cb = np.tile(np.array(oracle.cb_pair(3.0)), (20, 1))
    best = np.inf
    for c in range(64):
        M, _, _ = oracle.sweeps_philox(csr, h, m0[c], cb, 5, c, order_group=c + 1 if per_chain else 0, escale=esc, use_f64=False)
        best = min(best, min(oracle.energy(csr, h, M[t]) for t in range(20)))
    assert abs(best * nf - e_gs) < 1e-9
