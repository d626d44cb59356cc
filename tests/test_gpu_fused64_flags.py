"""The fp64 mode on fused windows with NMC phase flags in force (k_sweep_fused<.., FLAGS, .., F64> and its real-valued variant).

Spec: oracle/nlo.c nlo_sweeps_philox(use_f64=1, flags): a scaled row (flag 1) takes cb_run[2t+1], a frozen one (flags 2 and 3)
keeps its spin and adds no energy.  Every case checks (i) that the fused kernel ran -- fewer levels per sweep than the same call with
NLMC_NO_FUSED64=1 -- and (ii) that spins, tracked energies and per-sweep outputs are the sweep-by-sweep kernel's and the sequential
fp64 oracle's bits."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
from helpers import make_instance, init_spins

pytestmark = pytest.mark.gpu
SEED = 0x5EED0F64
INST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instances")
OUT_KEYS = ("spins", "energy", "min_energy", "argmin", "argmin_state")


def hub_instance(N, seed):
    """Gaussian couplings, hub rows of 9-40 entries (lane pairs, the CSR tail), real fields and a real diagonal."""
    rng = np.random.default_rng(seed)
    Jb, h = make_instance(N, seed=seed, with_h=True, gaussian=True)
    A = sp.lil_matrix(sp.csr_matrix(Jb))
    for hub, deg in enumerate((9, 12, 16, 17, 40)):
        for j in rng.choice(np.arange(64, N), size=deg, replace=False):
            A[hub, j] = A[j, hub] = float(rng.standard_normal() * 0.7)
    A = (sp.csr_matrix(A) + sp.diags(rng.standard_normal(N) * 0.4)).tocsr()
    A.sort_indices()
    return A, h


def chimera_normalised():
    import nlmc_amd as P
    W, h = P.instances.txt_to_A_droplet(os.path.join(INST, "chimera2048__001.txt"))
    J = sp.csr_matrix(W).astype(np.float64)
    s = np.max(np.abs(J.data))
    J = (J / s).tocsr()
    J.sort_indices()
    return J, np.asarray(h, dtype=np.float64).ravel() / s


def sweep(product, inst, R, T, W, betas, flags, temp_x, m0, real, outputs=False):
    """W calls of T sweeps (one planned window each) at the ladder temperatures with `flags` [R, N] in force."""
    with product.Engine(inst, None, R) as eng:
        eng.set_fused_f64_real(real)
        eng.set_spins(m0)
        E0 = eng.energy()
        eng.pt_init(betas)
        eng.set_flags(flags, temp_x)
        planned = eng.plan_philox_fused(0, W, T, SEED)
        lv, outs = [], []
        for w in range(W):
            kw = dict(record_stride=2, want_energy=True, want_min=True, want_state=True) if outputs else {}
            outs.append(eng.sweep_philox(T, SEED, sweep0=w * T, beta=None, precision="f64", **kw))
            st = eng.last_schedule_stats()
            lv.append(st["levels"] / max(1, st["orders"]))
        return {"spins": eng.get_spins(), "E": eng.energy_tracked(), "planned": planned, "lv": lv, "outs": outs,
                "esc": eng.energy_scale, "E0": E0}


def both(product, inst, R, T, W, betas, flags, temp_x, m0, real, monkeypatch, outputs=False):
    f = sweep(product, inst, R, T, W, betas, flags, temp_x, m0, real, outputs)
    monkeypatch.setenv("NLMC_NO_FUSED64", "1")
    p = sweep(product, inst, R, T, W, betas, flags, temp_x, m0, real, outputs)
    monkeypatch.delenv("NLMC_NO_FUSED64")
    assert f["planned"] == W
    assert max(f["lv"]) < min(p["lv"])                        # the fused kernel ran (fewer levels per sweep)
    assert np.array_equal(f["spins"], p["spins"]) and np.array_equal(f["E"], p["E"])
    for of, op in zip(f["outs"], p["outs"]):
        for k in OUT_KEYS:
            assert (of[k] is None and op[k] is None) or np.array_equal(of[k], op[k]), k
    return f


def check_oracle(J, h, m0, betas, flags, temp_x, chains, res, T, W, outputs=False):
    csr = oracle.Csr(J)
    esc = res["esc"]
    for c in chains:
        cb = np.tile(np.array(oracle.cb_pair(betas[c], temp_x, True)), (T * W, 1))
        M, s_fin, tr = oracle.sweeps_philox(csr, h, m0[c], cb, SEED, c, flags=flags[c], escale=esc, use_f64=True,
                                            efix0=int(np.rint(res["E0"][c] * 2.0 ** esc)))
        assert np.array_equal(res["spins"][c], s_fin), f"chain {c}"
        assert res["E"][c] == tr[-1] * 2.0 ** -esc, f"chain {c}"
        if outputs:
            for w, o in enumerate(res["outs"]):
                t = slice(w * T, (w + 1) * T)
                assert np.array_equal(o["energy"][c], tr[t] * 2.0 ** -esc), f"chain {c} window {w}"
                assert np.array_equal(o["spins"][c], M[t][::2]), f"chain {c} window {w}"
                am = int(np.argmin(tr[t]))
                assert o["argmin"][c] == am and o["min_energy"][c] == tr[t][am] * 2.0 ** -esc
                assert np.array_equal(o["argmin_state"][c], M[t][am])


def test_pmj_random_flags_two_threshold_tables(product, monkeypatch):
    """+-J couplings and integer fields (integer-threshold variant): every chain a random mix of flags 0-3, so that both K
    tables (plain and scaled rows) and frozen rows meet in every level; plain launches and per-sweep outputs."""
    N, R, T, W, tx = 3000, 6, 5, 2, 4.0
    J, _ = make_instance(N, seed=61)
    h = np.random.default_rng(61).integers(-2, 3, N).astype(np.float64)
    inst = product.Instance(J, h)
    betas = np.geomspace(0.2, 3.0, R)
    m0 = init_spins(R, N)
    flags = np.random.default_rng(62).integers(0, 4, (R, N)).astype(np.uint8)
    with product.Engine(inst, None, R) as eng:
        assert eng.fused_modes(T) == {"f32", "f64"}            # the integer-threshold variant, whatever the real-valued option says
    f = both(product, inst, R, T, W, betas, flags, tx, m0, False, monkeypatch)
    check_oracle(J, h, m0, betas, flags, tx, (0, 3, R - 1), f, T, W)
    f = both(product, inst, R, T, W, betas, flags, tx, m0, False, monkeypatch, outputs=True)
    check_oracle(J, h, m0, betas, flags, tx, (1, R - 1), f, T, W, outputs=True)


def test_hub_rows_real_diagonal_r64(product, monkeypatch):
    """Gaussian couplings with hub rows and a real diagonal (real-valued variant, opt-in): random flags 0-3."""
    N, R, T, W, tx = 2600, 4, 6, 2, 7.5
    J, h = hub_instance(N, 71)
    inst = product.Instance(J, h)
    betas = np.geomspace(0.2, 2.5, R)
    m0 = init_spins(R, N)
    flags = np.random.default_rng(72).integers(0, 4, (R, N)).astype(np.uint8)
    flags[:, :5] = 1                                          # the hub rows scaled
    f = both(product, inst, R, T, W, betas, flags, tx, m0, True, monkeypatch)
    check_oracle(J, h, m0, betas, flags, tx, (0, R - 1), f, T, W)
    f = both(product, inst, R, T, W, betas, flags, tx, m0, True, monkeypatch, outputs=True)
    check_oracle(J, h, m0, betas, flags, tx, (2,), f, T, W, outputs=True)


@pytest.mark.parametrize("kind", ["C", "NC"])
def test_chimera_nmc_mask(product, monkeypatch, kind):
    """Chimera-2048 divided by max|J| (couplings k/75): the flags of an NMC phase (hostlogic.phase_flags) for a backbone of
    about a tenth of the spins, per chain."""
    import nlmc_amd as P
    J, h = chimera_normalised()
    N, R, T, W, tx = J.shape[0], 16, 5, 3, 20.0
    inst = product.Instance(J, h)
    betas = np.full(R, 2.5)
    m0 = init_spins(R, N)
    rng = np.random.default_rng(81)
    flags = np.stack([P.hostlogic.phase_flags(N, m0[c], rng.choice(N, N // 10, replace=False), kind) for c in range(R)])
    f = both(product, inst, R, T, W, betas, flags, tx, m0, True, monkeypatch, outputs=True)
    check_oracle(J, h, m0, betas, flags, tx, (0, R - 1), f, T, W, outputs=True)


def subset_phase(product, inst, m0, betas, mask, T, W, real):
    """Marked temperature slots only (select("marked")), flags from the cluster masks (set_phase("C")), a running minimum over
    every second sweep, then the argmin state adopted."""
    L = len(betas)
    with product.Engine(inst, None, L) as eng:
        eng.set_fused_f64_real(real)
        eng.set_spins(m0)
        eng.pt_init(betas)
        eng.mark_slots(np.arange(L) % 2 == 1)
        eng.select("marked")
        eng.set_cluster_mask(mask)
        eng.set_phase("C", 20.0)
        eng.track_minimum(True, stride=2)
        assert eng.plan_philox_fused(0, W, T, SEED) == W
        lv, outs = [], []
        for w in range(W):
            outs.append(eng.sweep_philox(T, SEED, sweep0=w * T, beta=None, precision="f64", want_min=True, want_state=True))
            st = eng.last_schedule_stats()
            lv.append(st["levels"] / max(1, st["orders"]))
        before = eng.get_spins()
        eng.adopt_best()
        eng.track_minimum(False)
        eng.select("all")
        eng.set_phase("ALL")
        return {"before": before, "after": eng.get_spins(), "E": eng.energy_tracked(), "lv": lv, "outs": outs}


@pytest.mark.parametrize("real", [False, True])
def test_chain_subset_strided_minimum_adopt_best(product, monkeypatch, real):
    if real:
        J, h = hub_instance(2048, 91)
    else:
        J, _ = make_instance(2048, seed=91)
        h = np.zeros(2048)
    inst = product.Instance(J, h)
    N, L, T, W = 2048, 8, 6, 2
    betas = np.geomspace(0.3, 3.0, L)
    m0 = init_spins(L, N)
    mask = (np.random.default_rng(92).random((L, N)) < 0.15).astype(np.uint8)
    f = subset_phase(product, inst, m0, betas, mask, T, W, real)
    monkeypatch.setenv("NLMC_NO_FUSED64", "1")
    p = subset_phase(product, inst, m0, betas, mask, T, W, real)
    monkeypatch.delenv("NLMC_NO_FUSED64")
    assert max(f["lv"]) < min(p["lv"])
    for k in ("before", "after", "E"):
        assert np.array_equal(f[k], p[k]), k
    for of, op in zip(f["outs"], p["outs"]):
        for k in ("min_energy", "argmin", "argmin_state"):
            assert np.array_equal(of[k], op[k]), k
    marked = np.arange(1, L, 2)
    assert np.array_equal(f["before"][::2], m0[::2])              # unmarked chains untouched
    # the oracle: chain c (on slot c) with the phase flags of its mask, the minimum over sweeps 0, 2, 4, ... of each call
    import nlmc_amd as P
    csr = oracle.Csr(J)
    with product.Engine(inst, None, 1) as e1:
        esc = e1.energy_scale
    for c in marked[[0, -1]]:
        fl = P.hostlogic.phase_flags(N, m0[c], np.nonzero(mask[c])[0], "C")
        cb = np.tile(np.array(oracle.cb_pair(betas[c], 20.0, True)), (T * W, 1))
        E0 = oracle.energy(csr, h, m0[c])
        M, s_fin, tr = oracle.sweeps_philox(csr, h, m0[c], cb, SEED, int(c), flags=fl, escale=esc, use_f64=True,
                                            efix0=int(np.rint(E0 * 2.0 ** esc)))
        assert np.array_equal(f["before"][c], s_fin)
        row = 0 if c == marked[0] else len(marked) - 1
        t = slice((W - 1) * T, W * T, 2)                          # the last call's strided minimum
        am = int(np.argmin(tr[t])) * 2
        assert f["outs"][-1]["argmin"][row] == am
        assert np.array_equal(f["outs"][-1]["argmin_state"][row], M[(W - 1) * T + am])


def test_two_table_layout_too_big_falls_back(product, monkeypatch):
    """An integer instance whose field range (xmax) leaves room for one K table but not for two plus the flags: the plain fp64
    call runs on the fused windows, the flagged one sweep by sweep -- the same bits, and fused_last_call says so."""
    N, R, S, tx = 8192, 3, 10, 3.0
    Jb, _ = make_instance(N, seed=101)
    rng = np.random.default_rng(101)
    U = sp.triu(Jb, 1).tocsr()
    U.data = U.data * rng.integers(1, 300, U.nnz)
    J = (U + U.T).tocsr()
    J.sort_indices()
    h = rng.integers(-3, 4, N).astype(np.float64)
    inst = product.Instance(J, h)
    betas = np.geomspace(0.002, 0.02, R)
    m0 = init_spins(R, N)
    flags = np.random.default_rng(102).integers(0, 4, (R, N)).astype(np.uint8)

    def go(fl):
        with product.Engine(inst, None, R) as eng:
            qs = eng.field_scale
            xmax = np.max(np.abs(np.rint(np.ldexp(h, qs))) + np.asarray(abs(J * 2.0 ** qs).sum(axis=1)).ravel())
            assert 1200 < xmax < 3300                                 # one table fits at N = 8192, two do not
            modes = eng.fused_modes(5)
            eng.set_spins(m0)
            eng.pt_init(betas)
            eng.set_flags(fl, tx)
            o = eng.sweep_philox_windows(S, SEED, beta=None, window=5, precision="f64", want_energy=True)
            st = eng.last_schedule_stats()
            return eng.fused_last_call, st["levels"] / st["orders"], eng.get_spins(), eng.energy_tracked(), o["energy"], modes

    plain_fused, plain_lv, *_, modes = go(None)
    assert "f64" in modes
    fused_flag, lv1, s1, e1, t1, _ = go(flags)
    monkeypatch.setenv("NLMC_NO_FUSED64", "1")
    off, lv2, s2, e2, t2, _ = go(flags)
    monkeypatch.delenv("NLMC_NO_FUSED64")
    assert plain_fused and not fused_flag and not off
    assert plain_lv < lv1 == lv2                                  # the flagged call took the sweep-by-sweep path
    assert np.array_equal(s1, s2) and np.array_equal(e1, e2) and np.array_equal(t1, t2)


def test_fused_last_call_with_flags(product):
    """Engine.fused_last_call for fp64 calls with flags in force: True where the flagged kernel runs (fewer levels per sweep than a
    call with a temperature per sweep, which runs sweep by sweep and reports False)."""
    N, R, S = 2048, 2, 10
    J, _ = make_instance(N, seed=111)
    inst = product.Instance(J, np.zeros(N))
    with product.Engine(inst, None, R) as eng:
        eng.set_spins(init_spins(R, N))
        eng.set_flags(np.random.default_rng(112).integers(0, 4, (R, N)).astype(np.uint8), 5.0)
        eng.sweep_philox_windows(S, SEED, beta=1.5, window=5, precision="f64")
        assert eng.fused_last_call
        st = eng.last_schedule_stats()
        lv_fused = st["levels"] / st["orders"]
        eng.sweep_philox_windows(S, SEED, sweep0=S, beta=np.tile(np.linspace(0.5, 2.0, S), (R, 1)), window=5, precision="f64")
        assert not eng.fused_last_call
        st = eng.last_schedule_stats()
        assert lv_fused < st["levels"] / st["orders"]
        eng.set_phase("ALL")
        eng.sweep_philox_windows(S, SEED, sweep0=2 * S, beta=1.5, window=5, precision="f64")
        assert eng.fused_last_call
