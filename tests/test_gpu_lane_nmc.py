"""All phases of an NMC cycle in one lane launch (include/nlmc.h: nlmc_nmc_phases_lanes; csrc/nlmc_lane_nmc.h) against the call sequence
it replaces, bit for bit: on a second engine with the same start, track_minimum(True, stride), then per phase adopt_best (from the
second on), set_phase and sweep_philox(S, want_min, want_state) under set_lane_sweeps("force").  Compared: final spins, tracked
energies, every phase's minimum and argmin, the last phase's best state, the chains outside the subset (untouched).  The masks come from
set_cluster_mask: no inference runs.  Shapes are the smallest where the code changes path: n < 64 with n_pad = 16, a complete graph of
40, of 65 (the second block of the 64-entry order hand-out), sparse Chimera-128 with fields (no random-number table in LDS), a stored
diagonal, a sparse graph of 256 spins (the best state stays in global memory); 1 / 63 / 64 / 65 / 130 rows (tail lanes, several waves),
a marked subset after swaps (a chain list that is not contiguous); empty, full and random masks."""
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN
from helpers import make_instance, init_spins

pytestmark = pytest.mark.gpu
SEED = 0x5EED0000 + (11 << 32)          # high bits set
SWEEP0 = (1 << 31) + 12                  # the phases' own range of sweep indices
INST = os.path.join(GOLDEN, "instances")
SIX = ["C", "NC", "ALL"] * 2
FIVE = ["C", "NC", "C", "NC", "ALL"]     # full_update_frequency = 2
TEMP_X = 20.0


def instance(P, name):
    """-> (J, h, beta of the phases)"""
    r = np.random.default_rng(sum(map(ord, name)))
    if name == "wishart10":
        W, _ = P.instances.txt_to_A_wishart(os.path.join(INST, "wishart_N10_a0.50__wishart_planting_N_10_alpha_0.50_inst_1.txt"))
        J = (-W).toarray()
        return J / float(np.max(np.abs(J))), np.zeros(J.shape[0]), 2.5
    if name in ("k40", "k65"):
        n = int(name[1:])
        A = np.triu(r.choice([-1.0, 1.0], size=(n, n)), 1)
        return A + A.T, np.zeros(n), 0.4
    if name == "chimera128":
        W, h = P.instances.txt_to_A_droplet(os.path.join(INST, "chimera128__001.txt"))
        J = -W
        s = float(abs(J).max())
        return J / s, -np.asarray(h, dtype=np.float64).ravel() / s, 1.5
    if name == "diag12":
        n = 12
        A = np.triu(r.standard_normal((n, n)), 1)
        J = A + A.T
        J[np.arange(n), np.arange(n)] = r.standard_normal(n)
        return J / np.max(np.abs(J)), 0.3 * r.standard_normal(n), 1.5
    if name == "sparse256":
        J, h = make_instance(256, seed=12, with_h=True)
        return J, h, 1.0
    raise KeyError(name)


def masks(rows, n, seed=1):
    m = np.random.default_rng(seed).integers(0, 2, size=(rows, n)).astype(np.uint8)
    m[0] = 0                             # an empty backbone ...
    if rows > 1:
        m[1] = 1                         # ... a full one, every other chain its own random one
    return m


def sequence(eng, kinds, S, beta, stride, precision):
    """The call sequence nmc_phases_lanes replaces, on the selected chains -> per-phase minima, argmins, the last best state."""
    eng.track_minimum(True, stride=stride)
    pmin, parg, best = [], [], None
    for p, kind in enumerate(kinds):
        if p > 0:
            eng.adopt_best()
        eng.set_phase(kind, TEMP_X)
        o = eng.sweep_philox(S, SEED, sweep0=SWEEP0 + p * S, beta=beta, precision=precision, want_min=True, want_state=True)
        assert eng.last_sweep_route() == "lanes"
        pmin.append(o["min_energy"])
        parg.append(o["argmin"])
        best = o["argmin_state"]
    eng.track_minimum(False)
    eng.set_phase("ALL")
    return np.stack(pmin, axis=1), np.stack(parg, axis=1), best


def compare(P, name, rows, kinds, S, stride=1, precision="f32", read_back=True, new_env=None, monkeypatch=None):
    J, h, beta = instance(P, name)
    n = J.shape[0]
    m0, mk = init_spins(rows, n), masks(rows, n)
    with P.Engine(J, h, rows) as ref:
        ref.set_lane_sweeps("force")
        ref.set_spins(m0)
        ref.set_cluster_mask(mk)
        want = sequence(ref, kinds, S, beta, stride, precision)
        want_final, want_E = ref.get_spins(), ref.energy_tracked()
    for k, v in (new_env or {}).items():
        monkeypatch.setenv(k, str(v))
    with P.Engine(J, h, rows) as eng:                     # (the lane mode stays off: the entry is reached by name)
        eng.set_spins(m0)
        eng.set_cluster_mask(mk)
        assert eng.nmc_phases_lanes_refusal(S) is None
        out = eng.nmc_phases_lanes(kinds, S, SEED, SWEEP0, beta, TEMP_X, min_stride=stride, precision=precision,
                                   want_minima=read_back, want_last_best=read_back)
        assert eng.last_sweep_route() == "lanes"
        stats = eng.last_schedule_stats()
        got_final, got_E = eng.get_spins(), eng.energy_tracked()
    assert np.array_equal(got_final, want_final)
    assert np.array_equal(got_E, want_E)
    assert not np.array_equal(got_final, m0)
    if read_back:
        assert np.array_equal(out["phase_min"], want[0])
        assert np.array_equal(out["phase_argmin"], want[1])
        assert np.array_equal(out["last_best"], want[2])
    else:
        assert out is None
    assert stats["orders"] == len(kinds) * S and stats["levels"] == 0
    return out


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("name", ["wishart10", "k40", "k65", "chimera128", "diag12", "sparse256"])
def test_instances_in_both_arithmetics(product, name, precision):
    compare(product, name, 65, SIX, 3, precision=precision)


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 130])
def test_rows_tail_lanes_and_several_waves(product, rows):
    compare(product, "wishart10", rows, FIVE, 1)


@pytest.mark.parametrize("kind", ["C", "NC", "ALL"])
def test_a_single_phase(product, kind):
    compare(product, "k40", 65, [kind], 3)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("stride", [1, 2])
def test_minimum_stride(product, stride, precision):
    out = compare(product, "k40", 64, FIVE, 4, stride=stride, precision=precision)
    assert np.all(out["phase_argmin"] % stride == 0)
    if stride == 1:
        assert np.any(out["phase_argmin"] % 2 == 1)           # (so that the stride of 2 is seen to bind)


def test_without_read_backs(product):
    compare(product, "k40", 65, SIX, 3, read_back=False)


@pytest.mark.parametrize("name", ["k40", "sparse256"])
def test_launches_of_two_phases_give_the_same_bits(product, monkeypatch, name):
    """NLMC_LANE_SCRATCH holds the orders of two phases: the call is cut into launches of whole phases, the state carried over by the
    context's arrays (k40: best state in LDS within a launch; sparse256: in global memory)."""
    S, n = 3, instance(product, name)[0].shape[0]
    compare(product, name, 65, FIVE, S, new_env={"NLMC_LANE_SCRATCH": 2 * S * n * 2 + 2}, monkeypatch=monkeypatch)


def _fresh(P, name, rows, mask=True):
    J, h, beta = instance(P, name)
    eng = P.Engine(J, h, rows)
    eng.set_spins(init_spins(rows, J.shape[0]))
    if mask:
        eng.set_cluster_mask(masks(rows, J.shape[0]))
    return eng, beta


def _unchanged(eng, rows, n):
    return np.array_equal(eng.get_spins(), init_spins(rows, n))


def test_a_scratch_below_one_phase_is_refused(product, monkeypatch):
    monkeypatch.setenv("NLMC_LANE_SCRATCH", str(3 * 40 * 2 - 1))
    eng, beta = _fresh(product, "k40", 8)
    with eng:
        E = eng.energy_tracked()
        assert "NLMC_LANE_SCRATCH" in eng.nmc_phases_lanes_refusal(3)
        with pytest.raises(NotImplementedError, match="NLMC_LANE_SCRATCH"):
            eng.nmc_phases_lanes(SIX, 3, SEED, SWEEP0, beta, TEMP_X)
        assert eng.nmc_phases_lanes_refusal(2) is None
        assert _unchanged(eng, 8, 40) and np.array_equal(E, eng.energy_tracked())


def test_the_knob_refuses(product, monkeypatch):
    monkeypatch.setenv("NLMC_NO_LANE_NMC", "1")
    eng, beta = _fresh(product, "k40", 8)
    with eng:
        with pytest.raises(NotImplementedError, match="NLMC_NO_LANE_NMC"):
            eng.nmc_phases_lanes(SIX, 3, SEED, SWEEP0, beta, TEMP_X)
        assert _unchanged(eng, 8, 40)


def test_errors_run_nothing(product):
    eng, beta = _fresh(product, "k40", 8, mask=False)
    with eng:
        E = eng.energy_tracked()
        with pytest.raises(RuntimeError, match="backbone"):               # no mask yet: a state error, as set_phase reports it
            eng.nmc_phases_lanes(SIX, 3, SEED, SWEEP0, beta, TEMP_X)
        eng.set_cluster_mask(masks(8, 40))
        with pytest.raises(ValueError):
            eng.nmc_phases_lanes(SIX, 0, SEED, SWEEP0, beta, TEMP_X)      # S = 0
        with pytest.raises(ValueError):
            eng.nmc_phases_lanes([], 3, SEED, SWEEP0, beta, TEMP_X)       # P = 0
        with pytest.raises(ValueError, match="temp_x"):
            eng.nmc_phases_lanes(SIX, 3, SEED, SWEEP0, beta, 0.0)
        eng.track_minimum(True)
        with pytest.raises(RuntimeError, match="track"):
            eng.nmc_phases_lanes(SIX, 3, SEED, SWEEP0, beta, TEMP_X)
        eng.track_minimum(False)
        assert _unchanged(eng, 8, 40) and np.array_equal(E, eng.energy_tracked())


@pytest.mark.parametrize("name", ["wishart10", "chimera128"])
def test_the_marked_subset_of_a_ladder_after_swaps(product, name):
    """Rows = the chains on the marked slots of 5 ladders of 8 after a few swap rounds: a chain list that is not contiguous (and a tail:
    15 rows).  The chains outside the subset keep their state."""
    P = product
    J, h, beta = instance(P, name)
    n, L, nl, S = J.shape[0], 8, 5, 3
    G = L * nl
    betas = np.geomspace(0.05, 0.4, L) if name == "wishart10" else np.linspace(1.0, 1.1, L)
    marks = np.array([False] * 5 + [True] * 3)
    m0, mk = init_spins(G, n), masks(G, n, seed=4)
    res = []
    for new in (False, True):
        with P.Engine(J, h, G) as eng:
            eng.set_lane_sweeps("force")
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
                out = eng.nmc_phases_lanes(SIX, S, SEED, SWEEP0, beta, TEMP_X, want_minima=True, want_last_best=True)
                got = (out["phase_min"], out["phase_argmin"], out["last_best"])
            else:
                got = sequence(eng, SIX, S, beta, 1, "f32")
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
    J, h, beta = instance(P, "k40")
    n, rows, S = 40, 6, 5
    csr = oracle.Csr(J)
    m0, mk = init_spins(rows, n), masks(rows, n)
    with P.Engine(J, h, rows) as eng:
        eng.set_spins(m0)
        eng.set_cluster_mask(mk)
        esc = eng.energy_scale
        E0 = eng.energy_tracked()
        out = eng.nmc_phases_lanes(FIVE, S, SEED, SWEEP0, beta, TEMP_X, want_minima=True, want_last_best=True)
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
