"""The fp64 mode on fused windows for REAL couplings and fields (k_sweep_fused<.., R64>, opt-in: Engine.set_fused_f64_real,
include/nlmc.h: nlmc_set_fused_f64_real).

The field is summed with fma in CSR order from the plan's fp64 value plane, z = cb x, and the spec's test fma(u, 2^z, u) < 1
(NMC/nmc.py:86-87) is decided from the 27 high bits of u where they decide, from all 53 otherwise.  The kernel must give the
sweep-by-sweep fp64 kernel's bits and the sequential fp64 oracle's: spins, tracked energies, per-sweep outputs, swap decisions."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
from helpers import make_instance, init_spins

pytestmark = pytest.mark.gpu
SEED = 0xA5A50000
INST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instances")


def real_instance(N, seed, hub_degs=(9, 12, 16, 17, 40), diag=False):
    """Gaussian couplings on a degree-6 graph, hub rows of the given degrees (lane pairs, the CSR tail), real fields, optional
    real diagonal: nothing is a multiple of a power of two."""
    rng = np.random.default_rng(seed)
    Jb, h = make_instance(N, seed=seed, with_h=True, gaussian=True)
    A = sp.lil_matrix(sp.csr_matrix(Jb))
    for hub, deg in enumerate(hub_degs):
        for j in rng.choice(np.arange(64, N), size=deg, replace=False):
            A[hub, j] = A[j, hub] = float(rng.standard_normal() * 0.7)
    A = sp.csr_matrix(A)
    if diag:
        A = (A + sp.diags(rng.standard_normal(N) * 0.4)).tocsr()
    A.sort_indices()
    return A, h


def normalised(kind):
    """A reference instance divided by max|J| as run() does (couplings k/75 for Chimera, k/7 for DCL after rounding)."""
    import nlmc_amd as P
    if kind == "chimera":
        W, h = P.instances.txt_to_A_droplet(os.path.join(INST, "chimera2048__001.txt"))
    else:
        W, h = P.instances.txt_to_A_DCL(os.path.join(INST, "DCL_C8__00.txt"))
    J = sp.csr_matrix(W).astype(np.float64)
    s = np.max(np.abs(J.data))
    J = (J / s).tocsr()
    J.sort_indices()
    return J, np.asarray(h, dtype=np.float64).ravel() / s


def run(product, inst, R, T, W, betas, fused, real, precision="f64", swaps=0, m0=None, outputs=False):
    with product.Engine(inst, None, R) as eng:
        eng.set_fused_f64_real(real)
        eng.set_spins(m0)
        E0 = eng.energy()
        eng.pt_init(betas)
        planned = eng.plan_philox_fused(0, W, T, SEED) if fused else 0
        if swaps:
            eng.pt_plan(0, W, SEED, swaps)
        lv, outs = [], []
        for w in range(W):
            kw = dict(record_stride=2, want_energy=True, want_min=True, want_state=True) if outputs else {}
            outs.append(eng.sweep_philox(T, SEED, sweep0=w * T, beta=None, precision=precision, **kw))
            st = eng.last_schedule_stats()
            lv.append(st["levels"] / max(1, st["orders"]))
            if swaps:
                eng.pt_swap_philox(w, SEED, swaps, want_log=False)
        return {"spins": eng.get_spins(), "E": eng.energy(), "slots": eng.pt_slots(), "planned": planned, "lv": lv,
                "esc": eng.energy_scale, "E0": E0, "outs": outs, "modes": eng.fused_modes(T)}


def check_oracle(J, h, m0, betas, chains, res, S):
    csr = oracle.Csr(J)
    for c in chains:
        cb = np.tile(np.array(oracle.cb_pair(betas[c], 1.0, True)), (S, 1))
        _, s_fin, _ = oracle.sweeps_philox(csr, h, m0[c], cb, SEED, c, escale=res["esc"], use_f64=True,
                                           efix0=int(np.rint(res["E0"][c] * 2.0 ** res["esc"])), want_M=False)
        assert np.array_equal(res["spins"][c], s_fin), f"chain {c}"


def same(a, b, keys=("spins", "E", "slots")):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def test_gaussian_couplings_and_fields(product):
    N, R, T, W = 4000, 4, 5, 3
    J, h = make_instance(N, seed=41, with_h=True, gaussian=True)
    inst = product.Instance(J, h)
    betas = np.geomspace(0.1, 3.0, R)
    m0 = init_spins(R, N)
    f = run(product, inst, R, T, W, betas, True, True, m0=m0)
    p = run(product, inst, R, T, W, betas, True, False, m0=m0)
    assert f["modes"] == {"f32", "f64"} and p["modes"] == {"f32"}
    assert f["planned"] == W
    assert max(f["lv"]) < min(p["lv"])                  # the fused kernel really ran (fewer levels per sweep)
    same(f, p)
    check_oracle(J, h, m0, betas, (0, 1, R - 1), f, T * W)


def test_long_rows_diagonal_and_fields(product):
    """Hub rows of 9-40 entries (the lane pair hands its partial sum on; the CSR tail continues it), a real diagonal, real
    fields: fused == sweep by sweep == oracle."""
    N, R, T, W = 3000, 4, 6, 2
    J, h = real_instance(N, 7, diag=True)
    inst = product.Instance(J, h)
    betas = np.geomspace(0.1, 2.5, R)
    m0 = init_spins(R, N)
    f = run(product, inst, R, T, W, betas, True, True, m0=m0)
    p = run(product, inst, R, T, W, betas, True, False, m0=m0)
    assert "f64" in f["modes"] and f["planned"] == W and max(f["lv"]) < min(p["lv"])
    same(f, p)
    check_oracle(J, h, m0, betas, (0, R - 1), f, T * W)
    check_oracle(J, h, m0, betas, (0, R - 1), p, T * W)


def test_exact_path_of_undecided_high_words(product, monkeypatch):
    """NLMC_F64_TIE_MASK widens the interval of u the high word leaves open (0: every update takes the exact path, one Philox
    call for the low 26 bits): same bits."""
    N, R, T, W = 2500, 3, 7, 2
    J, h = real_instance(N, 11)
    inst = product.Instance(J, h)
    betas = np.geomspace(0.2, 3.0, R)
    m0 = init_spins(R, N)
    a = run(product, inst, R, T, W, betas, True, True, m0=m0)
    monkeypatch.setenv("NLMC_F64_TIE_MASK", "0xFFFF0000")
    b = run(product, inst, R, T, W, betas, True, True, m0=m0)
    monkeypatch.setenv("NLMC_F64_TIE_MASK", "0")
    c = run(product, inst, R, T, W, betas, True, True, m0=m0)
    monkeypatch.delenv("NLMC_F64_TIE_MASK")
    p = run(product, inst, R, T, W, betas, True, False, m0=m0)
    assert a["planned"] == b["planned"] == c["planned"] == W and max(c["lv"]) < min(p["lv"])
    same(a, p)
    same(a, b)
    same(a, c)
    check_oracle(J, h, m0, betas, (1,), c, T * W)


def test_per_sweep_outputs(product):
    """Energy trace, running minimum, argmin, argmin state and recorded configurations == sweep by sweep."""
    N, R, T, W = 2600, 4, 6, 2
    J, h = real_instance(N, 21, diag=True)
    inst = product.Instance(J, h)
    betas = np.geomspace(0.3, 2.0, R)
    m0 = init_spins(R, N)
    f = run(product, inst, R, T, W, betas, True, True, m0=m0, outputs=True)
    p = run(product, inst, R, T, W, betas, True, False, m0=m0, outputs=True)
    assert f["planned"] == W and max(f["lv"]) < min(p["lv"])
    for of, op in zip(f["outs"], p["outs"]):
        for k in ("spins", "energy", "min_energy", "argmin", "argmin_state"):
            assert np.array_equal(of[k], op[k]), k
    same(f, p)


def drive(product, inst, G, L, T, rounds, pairs, real, deferred, m0):
    betas = np.geomspace(0.1, 3.0, L)
    with product.Engine(inst, None, G) as eng:
        eng.set_fused_f64_real(real)
        eng.set_spins(m0)
        eng.pt_init(betas)
        assert eng.plan_philox_fused(0, rounds, T, SEED) == rounds
        eng.pt_plan(0, rounds, SEED, pairs)
        eng.pt_log_begin(0, rounds, pairs)
        if deferred:
            ok = eng.pt_rounds_deferred(rounds, T, SEED, 0, 0, pairs, precision="f64")
            if not ok:
                return None
        else:
            for r in range(rounds):
                eng.sweep_philox(T, SEED, sweep0=r * T, beta=None, precision="f64")
                eng.pt_swap_philox(r, SEED, pairs, want_log=False)
        p, a = eng.pt_log_read()
        return {"spins": eng.get_spins(), "E": eng.energy(), "slots": eng.pt_slots(), "pairs": p, "acc": a}


def test_deferred_rounds_with_swaps(product):
    N, L, T, rounds, pairs = 2048, 8, 5, 4, 3
    G = 2 * L
    J, h = real_instance(N, 31)
    inst = product.Instance(J, h)
    m0 = init_spins(G, N)
    assert drive(product, inst, G, L, T, rounds, pairs, False, True, m0) is None       # option off: refused, nothing run
    d = drive(product, inst, G, L, T, rounds, pairs, True, True, m0)
    o = drive(product, inst, G, L, T, rounds, pairs, True, False, m0)
    assert d is not None
    same(d, o, ("spins", "E", "slots", "pairs", "acc"))
    assert not np.array_equal(d["slots"], np.arange(G) % L)


@pytest.mark.parametrize("kind", ["chimera", "DCL"])
def test_reference_instances(product, kind):
    """Chimera-2048 (couplings k/75) and DCL C8 (k/7) divided by max|J|: 256 replicas, windows with swaps in between."""
    J, h = normalised(kind)
    N, R, T, W = J.shape[0], 256, 5, 3
    inst = product.Instance(J, h)
    betas = np.geomspace(0.1, 4.0, R)
    m0 = init_spins(R, N)
    f = run(product, inst, R, T, W, betas, True, True, m0=m0, swaps=60)
    p = run(product, inst, R, T, W, betas, True, False, m0=m0, swaps=60)
    assert "f64" in f["modes"] and f["planned"] == W and max(f["lv"]) < min(p["lv"])
    same(f, p)


def test_pmj_instance_keeps_the_integer_threshold_kernel(product):
    N, R, T, W = 3000, 4, 5, 2
    J, h = make_instance(N, seed=13)
    inst = product.Instance(J, h)
    betas = np.geomspace(0.1, 3.0, R)
    m0 = init_spins(R, N)
    on = run(product, inst, R, T, W, betas, True, True, m0=m0)
    off = run(product, inst, R, T, W, betas, True, False, m0=m0)
    assert on["modes"] == off["modes"] == {"f32", "f64"}
    same(on, off)
    assert on["lv"] == off["lv"]


def test_dropin_npt_precision_f64(product, monkeypatch):
    """NPT(J, h, rng="philox", precision="f64") on Chimera-2048: the same M / Energy with the fused fp64 kernels switched off."""
    NPT = product.NPT
    W, h = product.instances.txt_to_A_droplet(os.path.join(INST, "chimera2048__001.txt"))
    R = 8
    betas = list(np.geomspace(0.2, 3.0, R))

    def go():
        npt = NPT(W, h, rng="philox", seed=5, precision="f64")
        return npt.run(betas, R, [False] * R, num_sweeps_MCMC=30, num_sweeps_read=30, num_swap_attempts=3,
                       num_swapping_pairs=2)

    M1, E1 = go()
    monkeypatch.setenv("NLMC_NO_FUSED64", "1")
    M2, E2 = go()
    assert np.array_equal(M1, M2) and np.array_equal(E1, E2)
    with pytest.raises(ValueError):
        NPT(W, h, rng="philox", seed=5, precision="f64").run(betas, R, [True] + [False] * (R - 1), num_sweeps_MCMC=10,
                                                            num_sweeps_read=10, num_swap_attempts=1, num_swapping_pairs=1)
