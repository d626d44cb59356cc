"""No GPU needed: the long-chain option of the wave-per-chain route (include/nlmc.h: nlmc_set_wave_long; csrc/nlmc_waves_long.h) --
its binding and constant, Engine.waves_take with the option on and off, the keyword refusals, the launch-shape rule of
csrc/nlmc_wave_shape.h restated in Python against a table, and the resident-field premise on a dense chain of 300 spins."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle
import wavefields
from conftest import REPO, load_product
from helpers import init_spins

SEED = 0xA5A50000 + (7 << 32)          # high bits set
LDS_MAX = 158 * 1024                   # dynamic LDS a workgroup may ask for


def header():
    text = open(os.path.join(REPO, "include", "nlmc.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_binding_and_constant():
    P = load_product()
    L = P._abi.lib()
    hdr = header()
    assert re.search(r"int\s+nlmc_set_wave_long\s*\(\s*nlmc_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", hdr)
    assert "nlmc_set_wave_long" in P._abi.EXPORTS
    assert L.nlmc_set_wave_long.restype is ctypes.c_int and L.nlmc_set_wave_long.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert L.nlmc_set_wave_long(None, 1) == P._abi.ERR_ARG            # a NULL context: an argument error, before any device work
    assert int(re.search(r"#define\s+NLMC_WAVE_LONG_N\s+(\d+)", hdr).group(1)) == P._abi.WAVE_LONG_N == 1024
    assert int(re.search(r"#define\s+NLMC_WAVE_N\s+(\d+)", hdr).group(1)) == P._abi.WAVE_N == 256      # additive: the old limit stays
    assert L.nlmc_abi_version() == P._abi.ABI_VERSION == 3
    shape = open(os.path.join(REPO, "nonlocal-monte-carlo_amd", "csrc", "nlmc_wave_shape.h")).read()
    assert int(re.search(r"#define\s+NLMC_WAVE_LONG_MAX_N\s+(\d+)", shape).group(1)) == 1024
    assert int(re.search(r"#define\s+NLMC_WAVE_LONG_MIN_N\s+(\d+)", shape).group(1)) == 257


class FakeLib:
    def __init__(self):
        self.long = []

    def nlmc_set_wave_long(self, ctx, on):
        self.long.append(on)
        return 0

    def nlmc_subset_count(self, ctx):
        return 7


def test_waves_take_with_the_option_on_and_off():
    P = load_product()
    eng = P.Engine.__new__(P.Engine)          # no device: the methods under test only talk to the library handle
    eng._L, eng._ctx, eng.lane_sweeps, eng.wave_sweeps, eng.wave_long = FakeLib(), None, "off", "force", False
    def takes():
        out = []
        for n in (256, 257, 1024, 1025):
            eng.n = n
            out.append(eng.waves_take())
        return out
    assert takes() == [True, False, False, False]                     # as before the option existed
    eng.set_wave_long()
    assert eng.wave_long is True and eng._L.long == [1]
    assert takes() == [True, True, True, False]
    eng.n = 300
    assert eng.waves_take(10 ** 6) and not eng.waves_take(precision="f64")
    eng.wave_sweeps = "auto"                  # auto keeps its row rule (NLMC_WAVE_AUTO_MAX_ROWS = 0: never)
    top = P._abi.WAVE_AUTO_MAX_ROWS
    assert eng.waves_take(top) and (top == 2 ** 31 - 1 or not eng.waves_take(top + 1))
    eng.wave_sweeps = "off"
    assert takes() == [False] * 4
    eng.wave_sweeps = "force"
    eng.set_wave_long(False)
    assert eng.wave_long is False and eng._L.long == [1, 0]
    assert takes() == [True, False, False, False]
    del eng.wave_long                          # an engine double without the attribute answers as with the option off
    assert takes() == [True, False, False, False]
    eng._ctx = None


def test_keyword_refusals():
    P = load_product()
    ck = P.hostlogic.check_route_keywords
    ck(waves="force", wave_long=True, rng="philox")
    ck(waves="auto", wave_long=True, wave_rounds=True, rng="philox")           # together with wave_rounds: allowed
    ck(waves="force", wave_long=True)                                          # rng unknown yet: the mode values only
    ck(rng="numpy")
    with pytest.raises(ValueError, match="wave_long needs waves="):
        ck(wave_long=True, rng="philox")
    with pytest.raises(ValueError, match="rng='philox'"):
        ck(waves="force", wave_long=True, rng="numpy")
    with pytest.raises(ValueError, match="wave_long"):
        ck(wave_long=True, rng="numpy")
    with pytest.raises(ValueError, match="precision='f32'"):
        ck(waves="force", wave_long=True, rng="philox", precision="f64")

    class Eng:
        calls = []

        def set_wave_sweeps(self, m):
            self.calls.append(("waves", m))

        def set_wave_rounds(self, on):
            self.calls.append(("rounds", on))

        def set_wave_long(self, on):
            self.calls.append(("long", on))
    P.hostlogic.set_route_modes(Eng(), waves="force")
    assert Eng.calls == [("waves", "force")]
    P.hostlogic.set_route_modes(Eng(), waves="force", wave_rounds=True, wave_long=True)
    assert Eng.calls[1:] == [("waves", "force"), ("rounds", True), ("long", True)]


def test_keywords_of_the_classes():
    P = load_product()
    J, h = wavefields.dense_instance(8)
    for cls in (P.NPT, P.APT_ICM, P.APT_preprocessor):
        assert cls(J, h, rng="philox", seed=1).wave_long is False
        assert cls(J, h, rng="philox", seed=1, waves="force", wave_long=True).wave_long is True
        with pytest.raises(ValueError, match="wave_long needs"):
            cls(J, h, rng="philox", seed=1, wave_long=True)
        with pytest.raises(ValueError, match="rng='philox'"):
            cls(J, h, rng="numpy", seed=1, waves="force", wave_long=True)
    with pytest.raises(ValueError, match="precision='f32'"):
        P.NPT(J, h, rng="philox", seed=1, precision="f64", waves="force", wave_long=True)
    assert P.NPT(J, h, rng="philox", seed=1, waves="force", wave_rounds=True, wave_long=True).wave_rounds is True
    with pytest.raises(ValueError, match="wave_long needs wave_sweeps"):
        P.distributed.LocalTempering(None, [1.0], 1, 1, 0, [], wave_long=True)


def long_shape(n, n_pad, rows, n_cu, knob):
    """csrc/nlmc_wave_shape.h: nlmc_wave_long_shape, restated.  (R, W, workgroups, LDS bytes of the launch); R = 0: refused."""
    if n < 257 or n > 1024 or n_pad < n or rows < 1:
        return (0, 1, 0, 0)
    R = 8 if n <= 512 else 16
    if n_pad > 64 * R:
        return (0, 1, 0, 0)
    a16 = lambda x: (x + 15) // 16 * 16
    region = 256 * R + 16 * ((n + 3) // 4) + 2 * a16(n_pad)           # X, a word per lane and register | thresholds | spins | flags
    cu = n_cu if n_cu > 0 else 1
    w = knob if knob > 0 else (rows + cu - 1) // cu
    w = max(1, min(w, LDS_MAX // region, 16))
    return (R, w, (rows + w - 1) // w, w * region)


SHAPE_TABLE = [
    # n, n_pad, rows, n_cu, knob -> R, W, workgroups, LDS bytes
    ((257, 272, 1, 256, 0), (8, 1, 1, 3632)),
    ((257, 272, 17, 256, 1), (8, 1, 17, 3632)),
    ((300, 304, 100, 256, 0), (8, 1, 100, 3856)),
    ((512, 512, 4096, 256, 0), (8, 16, 256, 16 * 5120)),
    ((512, 512, 17, 256, 16), (8, 16, 2, 16 * 5120)),
    ((513, 528, 3, 256, 0), (16, 1, 3, 7216)),
    ((1023, 1024, 1024, 256, 0), (16, 4, 256, 4 * 10240)),
    ((1024, 1024, 4096, 256, 0), (16, 15, 274, 15 * 10240)),          # sixteen regions of 10 KB exceed a workgroup's LDS
    ((1024, 1024, 17, 256, 16), (16, 15, 2, 15 * 10240)),
    ((1024, 1024, 17, 256, 99), (16, 15, 2, 15 * 10240)),
    ((1024, 1024, 3, 0, 0), (16, 3, 1, 3 * 10240)),
    ((256, 256, 1, 256, 0), (0, 1, 0, 0)),
    ((1025, 1040, 1, 256, 0), (0, 1, 0, 0)),
    ((500, 528, 1, 256, 0), (0, 1, 0, 0)),
    ((300, 304, 0, 256, 0), (0, 1, 0, 0)),
]


@pytest.mark.parametrize("args,want", SHAPE_TABLE, ids=[f"n{a[0]}-r{a[2]}-k{a[4]}" for a, _ in SHAPE_TABLE])
def test_launch_shape_rule(args, want):
    n, n_pad = args[:2]
    got = long_shape(*args)
    assert got[:3] == want[:3]
    if want[0]:
        region = 256 * got[0] + 16 * ((n + 3) // 4) + 2 * n_pad       # (n_pad is a multiple of 16 in every row of the table)
        assert got[3] == got[1] * region <= LDS_MAX and 1 <= got[1] <= 16
        assert got[3] == want[3]
        assert (got[2] - 1) * got[1] < args[2] <= got[2] * got[1]


def test_shape_rule_matches_the_header_text():
    """The constants the restatement uses are the header's own."""
    shape = open(os.path.join(REPO, "nonlocal-monte-carlo_amd", "csrc", "nlmc_wave_shape.h")).read()
    assert re.search(r"#define\s+NLMC_WAVE_LONG_LDS_MAX\s+\(\(size_t\)158 \* 1024\)", shape)
    assert "n <= 512 ? 8 : 16" in shape


@pytest.mark.parametrize("per_chain", [False, True], ids=["shared", "per_chain"])
def test_resident_fields_give_the_specs_bits_dense_300(per_chain):
    """The premise of the route at a length the existing CPU test does not reach: fields kept resident over 300 spins of a complete
    graph with a diagonal, corrected row by row on every flip, give oracle.sweeps_philox's bits."""
    n, S, chain = 300, 2, 3
    J, h = wavefields.dense_instance(n, 17, diag=True)
    m0 = init_spins(4, n)[chain]
    cb = np.tile(np.array(oracle.cb_pair(0.15)), (S, 1))
    csr = oracle.Csr(J)
    esc = oracle.field_scale(csr, h)[1]
    group = chain + 1 if per_chain else 0
    M, s_fin, tr = oracle.sweeps_philox(csr, h, m0, cb, SEED, chain, order_group=group, sweep0=5, escale=esc, use_f64=False, efix0=12345)
    Mw, sw, trw = wavefields.sweeps(J, h, m0, cb, SEED, chain, order_group=group, sweep0=5, escale=esc, efix0=12345)
    assert np.array_equal(M, Mw) and np.array_equal(s_fin, sw) and np.array_equal(tr, trw)
    assert len({M[t].tobytes() for t in range(S)}) > 1 and not np.array_equal(M[0], m0)          # the chain moves
