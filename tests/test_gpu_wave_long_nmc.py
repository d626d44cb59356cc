"""All phases of an NMC cycle of dense chains of 257 to 1024 spins in one wave launch (include/nlmc.h: nlmc_nmc_phases_waves_long;
csrc/nlmc_wave_long_nmc.h) against the call sequence it replaces, bit for bit: on a second engine with the same start under
set_wave_sweeps("force") + set_wave_long(), track_minimum(True, stride), then per phase adopt_best (from the second on), set_phase and
sweep_philox(S, want_min, want_state) -- and, once, on the default route.  Compared: final spins, tracked energies, every phase's minimum
and argmin, the last phase's best state, the chains outside the subset (untouched).  The masks come from set_cluster_mask: no inference
runs.  Shapes are the smallest where the code changes path: complete +-1 graphs of 257 spins (the first long chain, R = 8, n_pad = 272),
512 (the last with R = 8), 513 (the first with R = 16, n_pad = 528) and 1024 (the largest, n_pad = n); a sparse graph of degree 6 with
fields, where most visited spins do not flip; a stored diagonal; one row, workgroups of four waves whose last waves have no row, more
rows than a workgroup's LDS holds regions; both row-request variants; a marked subset after swaps (a chain list that is not contiguous);
empty, full and random masks (masks() of tests/test_gpu_lane_nmc.py); calls cut into several launches."""
import numpy as np
import pytest

import oracle
from helpers import init_spins
from test_gpu_lane_nmc import FIVE, SEED, SIX, SWEEP0, TEMP_X, masks
from test_gpu_wave_nmc import sequence

pytestmark = pytest.mark.gpu


def instance(P, name):
    """-> (J, h, beta of the phases)"""
    if name.startswith("k"):                                   # complete +-1 graph: k129's rule of tests/test_gpu_wave_nmc.py
        n = int(name[1:])
        A = np.triu(np.random.default_rng(n).choice([-1.0, 1.0], size=(n, n)), 1)
        return A + A.T, np.zeros(n), 2.5 / np.sqrt(n)
    r = np.random.default_rng(sum(map(ord, name)))
    if name == "sparse300":                                    # a ring with chords 1, 2, 3: degree 6, +-1 couplings, fields
        n = 300
        J = np.zeros((n, n))
        for d in (1, 2, 3):
            i = np.arange(n)
            J[i, (i + d) % n] = r.choice([-1.0, 1.0], size=n)
        J = J + J.T
        return J, 0.5 * r.standard_normal(n), 1.0
    if name == "diag260":                                      # diag12's rule of tests/test_gpu_lane_nmc.py
        n = 260
        A = np.triu(r.standard_normal((n, n)), 1)
        J = A + A.T
        J[np.arange(n), np.arange(n)] = r.standard_normal(n)
        return J / np.max(np.abs(J)), 0.3 * r.standard_normal(n), 2.5 / np.sqrt(n)
    raise KeyError(name)


_REFERENCE = {}


def reference(P, name, rows, kinds, S, stride, waves):
    """The call sequence's results, computed once per shape and shared (read-only) among the cases that need them."""
    key = (name, rows, tuple(kinds), S, stride, waves)
    if key not in _REFERENCE:
        J, h, beta = instance(P, name)
        n = J.shape[0]
        with P.Engine(J, h, rows) as ref:
            if waves:
                ref.set_wave_sweeps("force")
                ref.set_wave_long()
            ref.set_spins(init_spins(rows, n))
            ref.set_cluster_mask(masks(rows, n))
            want = sequence(ref, kinds, S, beta, stride, "waves" if waves else None)
            _REFERENCE[key] = want + (ref.get_spins(), ref.energy_tracked())
        for a in _REFERENCE[key]:
            a.setflags(write=False)
    return _REFERENCE[key]


def compare(P, name, rows, kinds, S, stride=1, read_back=True, new_env=None, monkeypatch=None, waves=True):
    J, h, beta = instance(P, name)
    n = J.shape[0]
    m0, mk = init_spins(rows, n), masks(rows, n)
    want = reference(P, name, rows, kinds, S, stride, waves)
    for k, v in (new_env or {}).items():
        monkeypatch.setenv(k, str(v))
    with P.Engine(J, h, rows) as eng:                     # (no wave mode is set: the entry is reached by name)
        eng.set_spins(m0)
        eng.set_cluster_mask(mk)
        assert eng.nmc_phases_waves_long_refusal(S) is None
        out = eng.nmc_phases_waves_long(kinds, S, SEED, SWEEP0, beta, TEMP_X, min_stride=stride, want_minima=read_back,
                                        want_last_best=read_back)
        assert eng.last_sweep_route() == "waves"
        stats = eng.last_schedule_stats()
        got_final, got_E = eng.get_spins(), eng.energy_tracked()
    assert np.array_equal(got_final, want[3])
    assert np.array_equal(got_E, want[4])
    assert not np.array_equal(got_final, m0)
    if read_back:
        assert np.array_equal(out["phase_min"], want[0])
        assert np.array_equal(out["phase_argmin"], want[1])
        assert np.array_equal(out["last_best"], want[2])
    else:
        assert out is None
    assert stats["orders"] == len(kinds) * S and stats["levels"] == 0
    return out


@pytest.mark.parametrize("name", ["k257", "k512", "k513", "k1024", "sparse300", "diag260"])
def test_instances_against_the_long_wave_phase_loop(product, name):
    compare(product, name, 5, SIX, 3)


def test_against_the_phase_loop_on_the_default_route(product):
    """"The bits of the call sequence on ANY route": the sequence with every route mode off."""
    compare(product, "k257", 5, SIX, 3, waves=False)


@pytest.mark.parametrize("rows", [1, 4, 5, 9])
def test_workgroups_of_four_waves(product, monkeypatch, rows):
    """NLMC_WAVE_WAVES=4: one wave with a row and three without, a full workgroup, a second workgroup with one row, a third."""
    compare(product, "k257", rows, SIX, 3, new_env={"NLMC_WAVE_WAVES": 4}, monkeypatch=monkeypatch)


def test_more_rows_than_a_workgroup_holds_regions(product, monkeypatch):
    """20 rows of 1024 spins with 16 waves asked for: the LDS holds 13 regions of 12 KB, so the launch has two workgroups of 13 waves."""
    compare(product, "k1024", 20, SIX, 3, new_env={"NLMC_WAVE_WAVES": 16}, monkeypatch=monkeypatch)


def test_rows_by_the_shape_rule(product):
    compare(product, "k1024", 20, SIX, 3)


@pytest.mark.parametrize("ahead", [0, 1])
def test_both_row_request_variants(product, monkeypatch, ahead):
    compare(product, "k513", 5, SIX, 3, new_env={"NLMC_WAVE_LONG_AHEAD": ahead}, monkeypatch=monkeypatch)


@pytest.mark.parametrize("kinds", [["C"], ["NC"], ["ALL"], SIX, FIVE], ids=lambda k: "-".join(k))
def test_phase_kinds(product, kinds):
    compare(product, "k257", 5, kinds, 3)


@pytest.mark.parametrize("S", [1, 3, 4])
def test_sweeps_per_phase(product, S):
    compare(product, "k257", 5, FIVE, S)


@pytest.mark.parametrize("stride", [1, 2])
def test_minimum_stride(product, stride):
    out = compare(product, "k257", 32, FIVE, 4, stride=stride)
    assert np.all(out["phase_argmin"] % stride == 0)
    if stride == 1:
        assert np.any(out["phase_argmin"] % 2 == 1)           # (so that the stride of 2 is seen to bind)


def test_without_read_backs(product):
    compare(product, "k257", 5, SIX, 3, read_back=False)


@pytest.mark.parametrize("name", ["k257", "k1024"])
def test_launches_of_two_phases_give_the_same_bits(product, monkeypatch, name):
    """NLMC_LANE_SCRATCH holds the orders of two phases: a call of six is cut into three launches of two, and every later launch starts
    from the context's best state and minimum with the fields built again."""
    S, n = 3, instance(product, name)[0].shape[0]
    compare(product, name, 5, SIX, S, new_env={"NLMC_LANE_SCRATCH": 2 * S * n * 2 + 2}, monkeypatch=monkeypatch)


def test_more_phases_than_one_launch_holds(product):
    """130 phases of one sweep: the kinds of 128 travel in the kernel arguments, the call takes a second launch."""
    compare(product, "k257", 5, (["C", "NC", "ALL"] * 44)[:130], 1)


def _fresh(P, name, rows, mask=True, **kw):
    J, h, beta = instance(P, name)
    eng = P.Engine(J, h, rows, **kw)
    eng.set_spins(init_spins(rows, J.shape[0]))
    if mask:
        eng.set_cluster_mask(masks(rows, J.shape[0]))
    return eng, beta


def _unchanged(eng, rows, n):
    return np.array_equal(eng.get_spins(), init_spins(rows, n))


def test_a_scratch_below_one_phase_is_refused(product, monkeypatch):
    monkeypatch.setenv("NLMC_LANE_SCRATCH", str(3 * 257 * 2 - 1))
    eng, beta = _fresh(product, "k257", 4)
    with eng:
        E = eng.energy_tracked()
        assert "NLMC_LANE_SCRATCH" in eng.nmc_phases_waves_long_refusal(3)
        with pytest.raises(NotImplementedError, match="NLMC_LANE_SCRATCH"):
            eng.nmc_phases_waves_long(SIX, 3, SEED, SWEEP0, beta, TEMP_X)
        assert eng.nmc_phases_waves_long_refusal(2) is None
        assert _unchanged(eng, 4, 257) and np.array_equal(E, eng.energy_tracked())


def test_the_knob_refuses(product, monkeypatch):
    monkeypatch.setenv("NLMC_NO_WAVE_LONG_NMC", "1")
    eng, beta = _fresh(product, "k257", 4)
    with eng:
        E = eng.energy_tracked()
        assert "NLMC_NO_WAVE_LONG_NMC" in eng.nmc_phases_waves_long_refusal(3)
        with pytest.raises(NotImplementedError, match="NLMC_NO_WAVE_LONG_NMC"):
            eng.nmc_phases_waves_long(SIX, 3, SEED, SWEEP0, beta, TEMP_X)
        assert _unchanged(eng, 4, 257) and np.array_equal(E, eng.energy_tracked())


def test_short_chains_are_refused(product):
    """256 spins belong to nmc_phases_waves; the long entry names its lower bound."""
    eng, beta = _fresh(product, "k256", 4)
    with eng:
        eng.set_wave_sweeps("force")
        eng.set_wave_long()
        E = eng.energy_tracked()
        assert "NLMC_WAVE_LONG" in eng.nmc_phases_waves_long_refusal(3)
        with pytest.raises(NotImplementedError, match="NLMC_WAVE_LONG"):
            eng.nmc_phases_waves_long(SIX, 3, SEED, SWEEP0, beta, TEMP_X)
        assert eng.nmc_phases_waves_refusal(3) is None
        assert _unchanged(eng, 4, 256) and np.array_equal(E, eng.energy_tracked())


def test_f64_is_refused(product):
    eng, beta = _fresh(product, "k257", 4)
    with eng:
        E = eng.energy_tracked()
        with pytest.raises(NotImplementedError, match="f32"):
            eng.nmc_phases_waves_long(SIX, 3, SEED, SWEEP0, beta, TEMP_X, precision="f64")
        assert _unchanged(eng, 4, 257) and np.array_equal(E, eng.energy_tracked())


def test_slot_keyed_random_numbers_are_refused(product):
    eng, beta = _fresh(product, "k257", 10)
    with eng:
        eng.pt_init(np.geomspace(0.3, 1.5, 5))
        eng.apt_shard(np.geomspace(0.3, 1.5, 5), 1, 0)
        eng.set_spins(init_spins(10, 257))
        E = eng.energy_tracked()
        assert "temperature slot" in eng.nmc_phases_waves_long_refusal(3)
        with pytest.raises(NotImplementedError, match="temperature slot"):
            eng.nmc_phases_waves_long(SIX, 3, SEED, SWEEP0, beta, TEMP_X)
        assert _unchanged(eng, 10, 257) and np.array_equal(E, eng.energy_tracked())


def test_errors_run_nothing(product):
    eng, beta = _fresh(product, "k257", 4, mask=False)
    with eng:
        E = eng.energy_tracked()
        with pytest.raises(RuntimeError, match="backbone"):               # no mask yet: a state error, as set_phase reports it
            eng.nmc_phases_waves_long(SIX, 3, SEED, SWEEP0, beta, TEMP_X)
        eng.set_cluster_mask(masks(4, 257))
        with pytest.raises(ValueError):
            eng.nmc_phases_waves_long(SIX, 0, SEED, SWEEP0, beta, TEMP_X)      # S = 0
        with pytest.raises(ValueError):
            eng.nmc_phases_waves_long([], 3, SEED, SWEEP0, beta, TEMP_X)       # P = 0
        with pytest.raises(ValueError):
            eng.nmc_phases_waves_long(SIX, 3, SEED, SWEEP0, beta, TEMP_X, min_stride=0)
        with pytest.raises(ValueError, match="temp_x"):
            eng.nmc_phases_waves_long(SIX, 3, SEED, SWEEP0, beta, 0.0)
        eng.track_minimum(True)
        with pytest.raises(RuntimeError, match="track"):
            eng.nmc_phases_waves_long(SIX, 3, SEED, SWEEP0, beta, TEMP_X)
        eng.track_minimum(False)
        assert _unchanged(eng, 4, 257) and np.array_equal(E, eng.energy_tracked())


def test_the_marked_subset_of_a_ladder_after_swaps(product):
    """Rows = the chains on the marked slots of 5 ladders of 8 after four swap rounds: a chain list that is not contiguous.  The chains
    outside the subset keep their state."""
    P = product
    J, h, beta = instance(P, "k257")
    n, L, nl, S = J.shape[0], 8, 5, 3
    G = L * nl
    betas = np.linspace(0.9, 1.1, L) * beta
    marks = np.array([False] * 5 + [True] * 3)
    m0, mk = init_spins(G, n), masks(G, n, seed=4)
    res = []
    for new in (False, True):
        with P.Engine(J, h, G) as eng:
            eng.set_wave_sweeps("force")
            eng.set_wave_long()
            eng.pt_init(betas)
            eng.set_spins(m0)
            eng.mark_slots(marks)
            for r in range(4):
                eng.sweep_philox(2, SEED, sweep0=2 * r, beta=None)
                eng.pt_swap_philox(r, SEED, 3)
            eng.set_cluster_mask(mk)
            before = eng.get_spins()
            eng.select("marked")
            sub = eng.subset()
            assert len(sub) == 15 and not np.array_equal(sub, np.arange(sub[0], sub[0] + 15))
            if new:
                out = eng.nmc_phases_waves_long(SIX, S, SEED, SWEEP0, beta, TEMP_X, want_minima=True, want_last_best=True)
                got = (out["phase_min"], out["phase_argmin"], out["last_best"])
            else:
                got = sequence(eng, SIX, S, beta, 1, "waves")
            eng.select("all")
            after = eng.get_spins()
            rest = np.setdiff1d(np.arange(G), sub)
            assert np.array_equal(after[rest], before[rest]) and not np.array_equal(after[sub], before[sub])
            res.append((sub, after, eng.energy_tracked()) + tuple(got))
    for x, y in zip(*res):
        assert np.array_equal(x, y)


def test_against_the_oracle(product):
    """Directly against the sequential specification: flagged sweeps and the np.argmin hand-off (tests/test_gpu_npt_nmc.py)."""
    P = product
    J, h, beta = instance(P, "k257")
    n, rows, S = 257, 4, 3
    csr = oracle.Csr(J)
    m0, mk = init_spins(rows, n), masks(rows, n)
    with P.Engine(J, h, rows) as eng:
        eng.set_spins(m0)
        eng.set_cluster_mask(mk)
        esc = eng.energy_scale
        E0 = eng.energy_tracked()
        out = eng.nmc_phases_waves_long(FIVE, S, SEED, SWEEP0, beta, TEMP_X, want_minima=True, want_last_best=True)
        final, E = eng.get_spins(), eng.energy_tracked()
    cb = np.tile(np.array(oracle.cb_pair(beta, TEMP_X)), (S, 1))
    for c in range(rows):
        s, e0 = m0[c].copy(), int(np.rint(E0[c] * 2.0 ** esc))
        for p, kind in enumerate(FIVE):
            m = mk[c].astype(bool)
            fl = None if kind == "ALL" else (np.where(m, 1, 2) if kind == "C" else np.where(m, 2, 0)).astype(np.uint8)
            M, s_fin, tr = oracle.sweeps_philox(csr, h, s, cb, SEED, c, sweep0=SWEEP0 + p * S, flags=fl, escale=esc, efix0=e0)
            t = int(np.argmin(tr))                                # first minimum: np.argmin (NPT/npt.py:436)
            assert out["phase_argmin"][c, p] == t and out["phase_min"][c, p] == tr[t] * 2.0 ** -esc, (c, p)
            s, e0 = M[t].copy(), int(tr[t])
        assert np.array_equal(out["last_best"][c], s)
        assert np.array_equal(final[c], s_fin) and E[c] == tr[-1] * 2.0 ** -esc
