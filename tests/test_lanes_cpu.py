"""No GPU needed: the chain-per-lane route's bindings and switches, and the premise of its known-answer GPU test."""
import os
import re

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, REPO, load_product
from helpers import init_spins

INST = os.path.join(GOLDEN, "instances")


def header():
    text = open(os.path.join(REPO, "include", "nlmc.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_bindings_carry_the_headers_signatures():
    import ctypes
    P = load_product()
    L = P._abi.lib()
    hdr = header()
    assert re.search(r"int\s+nlmc_set_lane_sweeps\s*\(\s*nlmc_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", hdr)
    assert re.search(r"int\s+nlmc_last_sweep_route\s*\(\s*const\s+nlmc_ctx\s*\*\s*\w+\s*\)\s*;", hdr)
    assert {"nlmc_set_lane_sweeps", "nlmc_last_sweep_route"} <= set(P._abi.EXPORTS)
    assert L.nlmc_set_lane_sweeps.restype is ctypes.c_int and L.nlmc_set_lane_sweeps.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert L.nlmc_last_sweep_route.restype is ctypes.c_int and L.nlmc_last_sweep_route.argtypes == [ctypes.c_void_p]
    # a NULL context: an argument error / no route, before any device work
    assert L.nlmc_set_lane_sweeps(None, 1) == P._abi.ERR_ARG
    assert L.nlmc_last_sweep_route(None) == P._abi.ROUTE_NONE == 0
    # the constants the binding mirrors
    assert int(re.search(r"#define\s+NLMC_LANE_N\s+(\d+)", hdr).group(1)) == P._abi.LANE_N == 1024
    assert int(re.search(r"#define\s+NLMC_LANE_AUTO_ROWS\s+(\d+)", hdr).group(1)) == P._abi.LANE_AUTO_ROWS
    routes = re.search(r"NLMC_ROUTE_NONE\s*=\s*(\d+)\s*,\s*NLMC_ROUTE_STEPWISE\s*=\s*(\d+)\s*,\s*NLMC_ROUTE_FUSED\s*=\s*(\d+)\s*,\s*NLMC_ROUTE_LANES\s*=\s*(\d+)", hdr)
    assert tuple(map(int, routes.groups())) == (P._abi.ROUTE_NONE, P._abi.ROUTE_STEPWISE, P._abi.ROUTE_FUSED, P._abi.ROUTE_LANES) == (0, 1, 2, 3)
    assert L.nlmc_abi_version() == 3


class FakeLib:
    def __init__(self):
        self.modes, self.route = [], 0

    def nlmc_set_lane_sweeps(self, ctx, mode):
        self.modes.append(mode)
        return 0

    def nlmc_last_sweep_route(self, ctx):
        return self.route

    def nlmc_subset_count(self, ctx):
        return 7


def test_engine_maps_the_three_modes_and_the_routes():
    P = load_product()
    eng = P.Engine.__new__(P.Engine)          # no device: the methods under test only talk to the library handle
    eng._L, eng._ctx, eng.n, eng.lane_sweeps = FakeLib(), None, 40, "off"
    for mode in ("off", "auto", "force"):
        eng.set_lane_sweeps(mode)
        assert eng.lane_sweeps == mode
    assert eng._L.modes == [P._abi.LANES_OFF, P._abi.LANES_AUTO, P._abi.LANES_FORCE] == [0, 1, 2]
    for bad in ("on", "", None, 1):
        with pytest.raises(ValueError):
            eng.set_lane_sweeps(bad)
    assert eng._L.modes == [0, 1, 2] and eng.lane_sweeps == "force"
    for code, name in ((0, None), (1, "stepwise"), (2, "fused"), (3, "lanes")):
        eng._L.route = code
        assert eng.last_sweep_route() == name
    # the rule sweep_philox_windows asks before it plans fused windows (nlmc_set_lane_sweeps)
    assert eng.lanes_take()
    eng.n = 1024
    assert eng.lanes_take()
    eng.n = 1025
    assert not eng.lanes_take()
    eng.n, eng.lane_sweeps = 40, "off"
    assert not eng.lanes_take(10 ** 6)
    eng.lane_sweeps = "auto"
    assert eng.lanes_take(P._abi.LANE_AUTO_ROWS) and not eng.lanes_take(P._abi.LANE_AUTO_ROWS - 1)
    eng.n = 256
    assert not eng.lanes_take(P._abi.LANE_AUTO_ROWS)
    eng._ctx = None                            # (nothing for __del__ to destroy)


def test_known_answer_premise_under_the_oracle_alone():
    """tests/test_gpu_lanes.py::test_known_answer_wishart_ground_state: Wishart N = 10 instance 1 divided by max |J|, 64 chains from
    init_spins, 20 fp64 sweeps at the example's beta = 3, seed 5 -- the oracle's chains reach the listed ground-state energy."""
    P = load_product()
    fn = "wishart_planting_N_10_alpha_0.50_inst_1.txt"
    W, _ = P.instances.txt_to_A_wishart(os.path.join(INST, "wishart_N10_a0.50__" + fn))
    J = (-W).toarray()
    nf = float(np.max(np.abs(J)))
    J = J / nf
    h = np.zeros(10)
    e_gs = {l.split()[0]: float(l.split()[1]) for l in open(os.path.join(INST, "wishart_N10_a0.50__gs_energies.txt"))}[fn]
    csr = oracle.Csr(J)
    esc = oracle.field_scale(csr, h)[1]
    m0 = init_spins(64, 10)
    cb = np.tile(np.array(oracle.cb_pair(3.0, 1.0, True)), (20, 1))
    best = np.inf
    for c in range(64):
        M, _, _ = oracle.sweeps_philox(csr, h, m0[c], cb, 5, c, escale=esc, use_f64=True)
        best = min(best, min(oracle.energy(csr, h, M[t]) for t in range(20)))
    assert abs(best * nf - e_gs) < 1e-9
