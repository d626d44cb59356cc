"""Head stream of a fused-window plan (k_levelize_fused writes it beside head[]; fused_levels<.., HS> reads it; include/nlmc.h:
nlmc_plan_get_head_stream, nlmc_last_head_path; NLMC_NO_HEAD_STREAM=1 keeps the per-level head loads in the same build).

The stream holds head.x of every item once more, wave-major: int4 number (l // 4 * workers + w) * 64 + lane, component l % 4, is
the head of the item lane `lane` of worker wave w executes in published level l.  A plain fused launch of an instance without a
field term reads one such int4 per four levels instead of an 8-byte head per level.  The stream is a second copy of bytes the plan
already has, so every expectation is an equality: with head[] re-indexed on the CPU, with the same build under
NLMC_NO_HEAD_STREAM=1, with the sequential fp64 / fixed-point oracle.

Shapes (T = 3 or 4 sweeps per window, at most 16 chains).  The fused path takes chains of 256 spins or more (fused_supported), so
the edgeless graph has n = 258, not fewer.  Such a workgroup has 3 worker waves, a cap of 192 positions a level, so a sweep of 258
independent updates takes two levels and a window of T = 3 sweeps has 4 to 6 levels (5 measured): the shortest windows there are
-- a window of fewer than four levels does not exist on this path -- one whole quad and a partly used one.
The path graph of test_gpu_schedules.py along the order of sweep S0 has nl = n + 6 in window 0 at these sizes (computed here with
schedcheck.reference_levels before the device is asked; the cap of 192 positions is never reached by a path, so the count is
exact): n = 270 .. 273 give nl = 276 .. 279, all four residues of nl mod 4.  The degree-6 +-J graph at n = 1000 (4-wave
workgroups: 3 worker waves whatever NLMC_FUSED_WORKERS says) and at n = 5504 with NLMC_FUSED_WORKERS=8 (16-wave workgroups, where
the knob counts); a star whose hub has 40 neighbours (a lane quad plus a CSR tail)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
import schedcheck as sc
import test_gpu_schedules as tg
from helpers import make_instance, init_spins

pytestmark = pytest.mark.gpu
SEED, S0 = tg.SEED, tg.S0
R = 4
W = 2
PATH_NL = {270: 276, 271: 277, 272: 278, 273: 279}
CASES = ["edgeless", "path270", "path271", "path272", "path273", "deg6", "star", "deg6_w8", "deg6_5504_w8"]


@functools.lru_cache(maxsize=None)
def instance(case):
    """-> (J, T, knobs)."""
    if case == "edgeless":
        return sp.csr_matrix((258, 258), dtype=np.float64), 3, {}
    if case.startswith("path"):
        return tg.path(int(case[4:])), 3, {}
    if case == "star":
        return tg.star(300, 40, True), 3, {}
    if case == "deg6_5504_w8":
        return make_instance(5504, seed=55)[0], 3, {"NLMC_FUSED_WORKERS": 8}
    return make_instance(1000, seed=1000)[0], 4, ({"NLMC_FUSED_WORKERS": 8} if case == "deg6_w8" else {})


def make_engine(product, monkeypatch, J, h, knobs, stream, chains=R, betas=None):
    """The knobs are read when an engine is created."""
    monkeypatch.delenv("NLMC_FUSED_WORKERS", raising=False)
    monkeypatch.delenv("NLMC_NO_HEAD_STREAM", raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))
    if not stream:
        monkeypatch.setenv("NLMC_NO_HEAD_STREAM", "1")
    n = J.shape[0]
    eng = product.Engine(product.Instance(J, h), None, chains)
    eng.set_spins(init_spins(chains, n))
    eng.pt_init(np.linspace(0.36, 0.9, chains) if betas is None else betas)
    return eng


@pytest.mark.parametrize("case", CASES)
def test_stream_is_head_x_reindexed(product, monkeypatch, case):
    """Every real chunk of two windows: hs[l // 4, w, :, l % 4] == head[64 (loff[l] + w) : +64, 0]."""
    J, T, knobs = instance(case)
    n = J.shape[0]
    if case.startswith("path"):
        ref = sc.reference_levels(sc.csr_of(J), sc.window_orders(n, S0, T, 0, SEED))
        assert int(ref.max()) == PATH_NL[n]
    residues = set()
    with make_engine(product, monkeypatch, J, np.zeros(n), knobs, True) as eng:
        assert eng.plan_philox_fused(S0, W, T, SEED) == W
        for w in range(W):
            plan = eng.plan_items(w)
            hs, workers = plan["head_stream"]["hs"], plan["head_stream"]["workers"]
            nl, loff, head = plan["nlev"], plan["loff"], plan["head"]
            assert workers == plan["workers"] and hs.shape == ((nl + 3) // 4, workers, 64, 4)
            if case == "deg6_5504_w8":
                assert workers == 8
            if case.startswith("path") and w == 0:
                assert nl == PATH_NL[n]
                residues.add(nl % 4)
            if case == "edgeless":
                assert T < nl <= 2 * T                               # a sweep of 258 updates overflows the cap of 192 once
            if case == "star":
                assert (sc.decode_heads(plan)[1] == 3).any()          # kind TAIL: the hub's quad reads on from the CSR arrays
            chunks = 0
            for l in range(nl):
                c = int(loff[l + 1] - loff[l])
                assert 1 <= c <= workers
                want = head[64 * loff[l]:64 * loff[l + 1], 0].reshape(c, 64)
                assert np.array_equal(hs[l // 4, :c, :, l % 4], want), (w, l)
                chunks += c
            assert chunks * 64 == plan["npos"]
    print(f"{case}: levels mod 4 of window 0 {sorted(residues)}")


def test_path_sizes_cover_every_residue():
    """(CPU arithmetic only, but it belongs with the cases above.)"""
    assert sorted(v % 4 for v in PATH_NL.values()) == [0, 1, 2, 3]


def run_windows(product, monkeypatch, case, prec, stream):
    J, T, knobs = instance(case)
    n = J.shape[0]
    with make_engine(product, monkeypatch, J, np.zeros(n), knobs, stream) as eng:
        E0 = eng.energy()
        assert eng.plan_philox_fused(S0, W, T, SEED) == W
        for w in range(W):
            eng.sweep_philox(T, SEED, sweep0=S0 + w * T, beta=None, precision=prec)
            assert eng._last_fused() and eng.last_head_path() == ("stream" if stream else "loads")
        return dict(spins=eng.get_spins(), E=eng.energy_tracked(), E0=E0, esc=eng.energy_scale)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("case", CASES)
def test_same_bits_one_window_per_launch(product, monkeypatch, case, prec):
    """k_sweep_fused, a window per launch: spins and tracked energies with the stream equal those with the head loads and the
    sequential oracle's."""
    J, T, _ = instance(case)
    n = J.shape[0]
    a = run_windows(product, monkeypatch, case, prec, True)
    b = run_windows(product, monkeypatch, case, prec, False)
    assert np.array_equal(a["spins"], b["spins"]) and np.array_equal(a["E"], b["E"])
    m0, csr, f64 = init_spins(R, n), oracle.Csr(J), prec == "f64"
    assert not np.array_equal(a["spins"], m0)
    betas = np.linspace(0.36, 0.9, R)
    for c in (0, R - 1):
        cb = np.tile(np.array(oracle.cb_pair(betas[c], 1.0, f64)), (W * T, 1))
        _, s_fin, tr = oracle.sweeps_philox(csr, np.zeros(n), m0[c], cb, SEED, c, sweep0=S0, escale=a["esc"], use_f64=f64,
                                            efix0=int(np.rint(a["E0"][c] * 2.0 ** a["esc"])), want_M=False)
        assert np.array_equal(a["spins"][c], s_fin), c
        assert a["E"][c] == tr[-1] * 2.0 ** -a["esc"], c


def run_rounds(product, monkeypatch, J, h, stream, prec, rounds=5, T=4, chains=16, pairs=3):
    betas = np.geomspace(0.3, 1.5, chains)
    with make_engine(product, monkeypatch, J, h, {}, stream, chains=chains, betas=betas) as eng:
        assert eng.plan_philox_fused(0, rounds, T, SEED) == rounds
        eng.pt_plan(0, rounds, SEED, pairs)
        eng.pt_log_begin(0, rounds, pairs)
        assert eng.pt_rounds_fused(rounds, T, SEED, 0, 0, pairs, precision=prec), getattr(eng, "rounds_fused_refusal", "")
        p, acc = eng.pt_log_read()
        return (eng.get_spins(), eng.energy_tracked(), eng.pt_slots(), p, acc), eng.last_rounds_route(), eng.last_rounds_route(heads=True)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_same_bits_rounds_in_one_launch(product, monkeypatch, prec):
    """k_rounds_fused, 5 rounds of a ladder of 16 in one launch, 3 swap pairs a round: spins, energies, slot table and swap log
    equal the run with head loads; the route record names the head path."""
    J = instance("deg6")[0]
    h = np.zeros(J.shape[0])
    a, route, detail = run_rounds(product, monkeypatch, J, h, True, prec)
    assert route == "in launch" and detail == "in launch, head stream"
    b, route, detail = run_rounds(product, monkeypatch, J, h, False, prec)
    assert route == "in launch" and detail == "in launch, head loads"
    for name, x, y in zip(("spins", "energies", "slots", "pairs", "accepted"), a, b):
        assert np.array_equal(x, y), name
    assert not np.array_equal(a[0], init_spins(16, J.shape[0]))


def test_wide_format_takes_the_head_loads(product, monkeypatch):
    """Gaussian couplings without a field: the plan has 8-byte entries, whose kernels keep the per-level head loads (four plane
    sets of four planes do not fit their registers).  The route says so and the bits are the knob-off run's."""
    J = make_instance(1000, seed=1001, gaussian=True)[0]
    h = np.zeros(J.shape[0])
    a, route, detail = run_rounds(product, monkeypatch, J, h, True, "f32")
    assert route == "in launch" and detail == "in launch, head loads"
    b, _, _ = run_rounds(product, monkeypatch, J, h, False, "f32")
    for name, x, y in zip(("spins", "energies", "slots", "pairs", "accepted"), a, b):
        assert np.array_equal(x, y), name
    with make_engine(product, monkeypatch, J, h, {}, True) as eng:
        assert eng.plan_philox_fused(0, 1, 4, SEED) == 1
        plan = eng.plan_items(0)
        assert plan["fmt"] == 0 and plan["head_stream"] is None       # (such a plan neither reserves nor builds a stream)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_field_takes_the_head_loads(product, monkeypatch, prec):
    """The same graph with a field in {-1, 0, 1}: head.y matters, so the launches load head[] whatever the knob says -- the route
    record says so -- and the bits are those of the knob-off run."""
    J = instance("deg6")[0]
    h = np.random.default_rng(7).integers(-1, 2, J.shape[0]).astype(np.float64)
    assert h.any()
    a, route, detail = run_rounds(product, monkeypatch, J, h, True, prec)
    assert route == "in launch" and detail == "in launch, head loads"
    b, _, detail = run_rounds(product, monkeypatch, J, h, False, prec)
    assert detail == "in launch, head loads"
    for name, x, y in zip(("spins", "energies", "slots", "pairs", "accepted"), a, b):
        assert np.array_equal(x, y), name
    # a window per launch as well
    n = J.shape[0]
    res = []
    for stream in (True, False):
        with make_engine(product, monkeypatch, J, h, {}, stream) as eng:
            assert eng.plan_philox_fused(0, 1, 4, SEED) == 1
            eng.sweep_philox(4, SEED, sweep0=0, beta=None, precision=prec)
            assert eng._last_fused() and eng.last_head_path() == "loads"
            assert eng.plan_items(0)["head_stream"] is None           # no launch could read it: not reserved, not built
            res.append((eng.get_spins(), eng.energy_tracked()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert not np.array_equal(res[0][0], init_spins(R, n))
