"""Every sweep route's updates against the exact heat-bath law (tests/lawcheck.py), not against another kernel.

The rest of the GPU suite ties the sweep kernels to each other and to the sequential spec (oracle/nlo.c) bit for bit; this module
ties them to the reference's dynamics (NMC/nmc.py:62-89): with record_stride=1 a call returns every sweep's configuration, the
shared order of a sweep is a pure function of (seed, sweep, order group), so the field each update saw is known exactly and its
outcome is a Bernoulli draw with probability (1 + tanh(beta x)) / 2.  Each test first asserts that the route it is meant for ran
(a route that silently falls back fails), reproduces a chain or two with the oracle bit for bit (that guards the order
reconstruction), then calibrates every update of the run: the true law passes; a temperature error of delta* = 2 t / sqrt(I)
<= 1e-2, the Jacobi reading (every neighbour at its pre-sweep value) and the route's own wrong hypothesis reject.

Routes without per-sweep outputs stay covered by the parity tests that tie them to the routes checked here: the plain and
deferred fused kernels and k_rounds_fused (test_gpu_fused.py::test_fused_equals_oracle_and_plain,
test_gpu_fused.py::test_fused_with_swaps_and_sharded_contexts, test_gpu_fused64.py::test_fused_f64_equals_plain_f64_and_the_oracle_pmj,
test_gpu_fused64.py::test_c4_size_f64_fused_oracle_sample_and_energy, test_gpu_fused64_real.py::test_deferred_rounds_with_swaps,
test_gpu_persistent.py::test_persistent_rounds_equal_rounds_launched_one_by_one).

Each test prints one LAW line: route, updates, k, t, delta*, max |z| under the true law, smallest max |z| of the wrong hypotheses."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import lawcheck
import oracle
from helpers import make_instance, init_spins

pytestmark = pytest.mark.gpu
SEED = 0x1A5EED00 + (7 << 32)
INST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instances")
MAX_DELTA = 1e-2


# ---- instances ------------------------------------------------------------------------------------------------------------------
def integer_instance(N, seed, wmax=3, diag=False, h_step=0.0):
    """Degree-6 graph with couplings in +-{1..wmax}, hub rows of 9-40 entries, optional integer diagonal, fields in multiples of h_step."""
    rng = np.random.default_rng(seed)
    Jb, _ = make_instance(N, seed=seed)
    A = sp.lil_matrix(sp.csr_matrix(Jb))
    for hub, deg in enumerate((9, 12, 16, 17, 40)):
        for j in rng.choice(np.arange(64, N), size=deg, replace=False):
            A[hub, j] = A[j, hub] = float(rng.choice([-1.0, 1.0]))
    A = sp.csr_matrix(A)
    U = sp.triu(A, 1).tocoo()
    w = U.data * rng.integers(1, wmax + 1, U.nnz)
    A = sp.coo_matrix((np.concatenate([w, w]), (np.concatenate([U.row, U.col]), np.concatenate([U.col, U.row]))), shape=(N, N)).tocsr()
    if diag:
        A = (A + sp.diags(rng.integers(-2, 3, N).astype(float))).tocsr()
    h = rng.integers(-3, 4, N) * h_step if h_step else np.zeros(N)
    A.sort_indices()
    return A, h


def hub_instance(N, seed):
    """Gaussian couplings, hub rows of 9-40 entries, real fields and a real diagonal."""
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


def ring_instance(n, seed):
    """+-J ring with random chords (mean degree ~6), integer fields: a chain too long for LDS."""
    r = np.random.default_rng(seed)
    i = np.concatenate([np.arange(n), r.integers(0, n, 2 * n)])
    j = np.concatenate([(np.arange(n) + 1) % n, r.integers(0, n, 2 * n)])
    keep = i != j
    A = sp.coo_matrix((np.ones(keep.sum()), (i[keep], j[keep])), shape=(n, n)).tocsr()
    A = sp.triu(((A + A.T) > 0).astype(np.float64), 1).tocsr()
    A.data = r.choice([-1.0, 1.0], A.nnz)
    A = (A + A.T).tocsr()
    A.sort_indices()
    return A, r.integers(-1, 2, n).astype(float)


# ---- runs -----------------------------------------------------------------------------------------------------------------------
def traced(product, J, h, m0, T, W, precision, beta=None, ladder=None, fused=True, flags=None, temp_x=1.0, real=False,
           order="shared"):
    """W calls of T sweeps each (one planned fused window per call when `fused`) with every configuration recorded.
    beta [R, W T] a table, or ladder: the PT ladder (beta=None calls: chain c runs at ladder[slot of c]).
    Returns (M [R, W T, N], beta [R, W T] as run, {"fused": per call, "planned", "modes"})."""
    R = m0.shape[0]
    with product.Engine(product.Instance(J, h), None, R) as eng:
        eng.set_fused_f64_real(real)
        eng.set_spins(m0)
        if ladder is not None:
            eng.pt_init(ladder)
            beta = np.repeat(np.asarray(ladder)[eng.pt_slots()][:, None], T * W, axis=1)
        if flags is not None:
            eng.set_flags(flags, temp_x)
        planned = eng.plan_philox_fused(0, W, T, SEED) if fused else 0
        Ms, ran = [], []
        for w in range(W):
            o = eng.sweep_philox(T, SEED, sweep0=w * T, beta=None if ladder is not None else beta[:, w * T:(w + 1) * T],
                                 precision=precision, order=order, record_stride=1)
            ran.append(eng._last_fused())
            Ms.append(o["spins"])
        route = {"fused": ran, "planned": planned, "modes": eng.fused_modes(T)}
    return np.concatenate(Ms, axis=1), beta, route


def oracle_chain(J, h, m0, beta, c, use_f64, flags=None, temp_x=1.0, order_group=0):
    cb = np.array([oracle.cb_pair(b, temp_x, use_f64) for b in beta[c]])
    return oracle.sweeps_philox(oracle.Csr(J), h, m0[c], cb, SEED, c, order_group=order_group,
                                flags=None if flags is None else flags[c], use_f64=use_f64)[0]


def assert_law(route, J, h, m0, M, beta, wrong, flags=None, temp_x=1.0, quant_qs=None, order_groups=None):
    """The calibration: true law passes with delta* <= 1e-2; beta (1 + delta*), the Jacobi reading and `wrong` reject."""
    inst = lawcheck.Instance(J, h)
    N = inst.n
    if order_groups is None:
        pos = lambda t: lawcheck.order_positions(N, t, SEED)             # noqa: E731
    else:
        pos = lambda t: lawcheck.order_positions(N, t, SEED, order_groups)  # noqa: E731
    hyp = {"true": {}, "jacobi": {"reading": "jacobi"}}
    hyp.update(wrong)
    quant = None if quant_qs is None else lawcheck.quantisation_bound(inst, quant_qs)
    res = lawcheck.check(inst, m0, M, beta, pos, flags=flags, temp_x=temp_x, hypotheses=hyp, quant=quant)
    print(lawcheck.summary(res))
    tr = res["true"]
    others = {k: v for k, v in res.items() if k != "true"}
    print(f"LAW {route}: updates={tr['n']} k={tr['k']} t={tr['t']:.2f} delta*={tr['delta_star']:.4f} max|z|={tr['max_z']:.2f} "
          f"min wrong max|z|={min(v['max_z'] for v in others.values()):.1f}")
    assert tr["ok"], lawcheck.summary({"true": tr})
    assert tr["delta_star"] <= MAX_DELTA
    if quant is not None:
        assert tr["quant_ok"]
    for name, r in others.items():
        assert not r["ok"], name
    return res


# ---- (a) "f32" fused windows with per-sweep outputs -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pmj", "gauss_hubs_diag"])
def test_f32_fused(product, kind):
    """+-J, and Gaussian couplings with fields, hub rows of 9-40 entries and a diagonal (checked with the true J: the 24-bit
    fixed-point couplings shift no bin by more than a standard deviation)."""
    N, T = 4096, 5
    if kind == "pmj":
        J, h = make_instance(N, seed=201)
        R, W, lo, hi = 48, 8, 0.3, 1.2
    else:
        J, h = hub_instance(N, 202)
        R, W, lo, hi = 48, 8, 0.35, 1.6
    m0 = init_spins(R, N)
    beta = np.repeat(np.geomspace(lo, hi, R)[:, None], T * W, axis=1)
    M, beta, rt = traced(product, J, h, m0, T, W, "f32", beta=beta)
    assert rt["planned"] == W and all(rt["fused"])
    assert np.array_equal(M[R - 1], oracle_chain(J, h, m0, beta, R - 1, False))
    qs = oracle.field_scale(oracle.Csr(J), h)[0]
    assert_law(f"f32 fused {kind}", J, h, m0, M, beta, {}, quant_qs=qs)


# ---- (b) fp64 integer-threshold fused windows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tie_mask", [None, "0"])
def test_f64_integer_threshold_fused(product, monkeypatch, tie_mask):
    """Integer couplings (hub rows included), quarter-integer fields; NLMC_F64_TIE_MASK=0 sends every update down the exact path."""
    if tie_mask is not None:
        monkeypatch.setenv("NLMC_F64_TIE_MASK", tie_mask)
    N, R, T, W = 4096, 48, 5, 8
    J, h = integer_instance(N, 203, wmax=3, h_step=0.25)
    m0 = init_spins(R, N)
    M, beta, rt = traced(product, J, h, m0, T, W, "f64", ladder=np.geomspace(0.1, 0.5, R))
    assert "f64" in rt["modes"] and rt["planned"] == W and all(rt["fused"])
    assert np.array_equal(M[0], oracle_chain(J, h, m0, beta, 0, True))
    assert_law(f"f64 integer fused tie_mask={tie_mask}", J, h, m0, M, beta, {})


# ---- (c) fp64 real-valued fused windows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gauss_hubs_diag", "chimera2048"])
def test_f64_real_valued_fused(product, kind):
    """set_fused_f64_real: Gaussian couplings with fields, hubs and a diagonal; Chimera-2048/001 divided by max|J|."""
    T = 5
    if kind == "chimera2048":
        J, h = chimera_normalised()
        R, W, lo, hi = 96, 9, 0.6, 3.0
    else:
        J, h = hub_instance(4096, 204)
        R, W, lo, hi = 48, 8, 0.35, 1.6
    N = J.shape[0]
    m0 = init_spins(R, N)
    M, beta, rt = traced(product, J, h, m0, T, W, "f64", ladder=np.geomspace(lo, hi, R), real=True)
    assert "f64" in rt["modes"] and rt["planned"] == W and all(rt["fused"])
    assert np.array_equal(M[R - 1], oracle_chain(J, h, m0, beta, R - 1, True))
    assert_law(f"f64 real fused {kind}", J, h, m0, M, beta, {})


# ---- (d) fp64 anneal on fused windows -------------------------------------------------------------------------------------------
def test_f64_anneal_fused(product):
    """+-J, an [R, S] table that changes at every sweep (20 sweeps from 0.2 to 3.0, rows that differ between chains): every
    update at the PREVIOUS sweep's beta -- a mix-up of the ring of K tables -- must reject (one step, x1.15, exceeds delta*)."""
    N, R, T, W, S = 4096, 128, 5, 4, 20
    J, h = make_instance(N, seed=205)
    m0 = init_spins(R, N)
    beta = np.stack([np.geomspace(0.2 * (1 + 0.002 * c), 3.0 / (1 + 0.001 * c), S) for c in range(R)])
    M, beta, rt = traced(product, J, h, m0, T, W, "f64", beta=beta)
    assert rt["planned"] == W and all(rt["fused"])
    assert np.array_equal(M[0], oracle_chain(J, h, m0, beta, 0, True))
    prev = np.concatenate([beta[:, :1], beta[:, :-1]], axis=1)
    res = assert_law("f64 anneal fused", J, h, m0, M, beta, {"previous_sweep_beta": {"beta": prev}})
    assert np.min(beta[:, 1:] / beta[:, :-1]) - 1 > res["true"]["delta_star"]          # every step exceeds delta*


# ---- (e) NMC phase flags ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f64_integer", "f64_real", "f32"])
def test_phase_flags(product, kind):
    """Flags 0-3 mixed in every chain: frozen rows bit-identical from start to end, scaled rows at beta / temp_x; the scaled rows
    at FULL beta must reject."""
    N, R, T, W, tx = 4096, 48, 5, (13 if kind == "f64_real" else 9), 3.0
    if kind == "f64_integer":
        J, h = integer_instance(N, 206, wmax=2, h_step=0.25)
        ladder = np.geomspace(0.15, 0.8, R)
    elif kind == "f64_real":
        J, h = hub_instance(N, 207)
        ladder = np.geomspace(0.35, 1.8, R)
    else:
        J, h = make_instance(N, seed=208)
        ladder = np.geomspace(0.3, 1.4, R)
    m0 = init_spins(R, N)
    flags = np.random.default_rng(209).choice([0, 0, 0, 0, 1, 1, 2, 3], size=(R, N)).astype(np.uint8)
    prec = "f32" if kind == "f32" else "f64"
    M, beta, rt = traced(product, J, h, m0, T, W, prec, ladder=ladder, flags=flags, temp_x=tx, real=(kind == "f64_real"))
    assert rt["planned"] == W and all(rt["fused"])
    if prec == "f64":
        assert "f64" in rt["modes"]
    frozen = flags >= 2
    assert not np.any((M != m0[:, None, :]) & frozen[:, None, :])             # frozen rows: the same bits at every sweep
    assert np.array_equal(M[1], oracle_chain(J, h, m0, beta, 1, prec == "f64", flags=flags, temp_x=tx))
    qs = oracle.field_scale(oracle.Csr(J), h)[0] if prec == "f32" else None
    assert_law(f"phase flags {kind}", J, h, m0, M, beta, {"scaled_rows_at_full_beta": {"scaled_rows_at_full_beta": True}},
               flags=flags, temp_x=tx, quant_qs=qs)


# ---- (f) sweep-by-sweep kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,precision", [("shared", "f64"), ("per_chain", "f32")])
def test_sweep_by_sweep(product, monkeypatch, order, precision):
    """No fused plan (and NLMC_NO_FUSED64=1): the sweep-by-sweep kernels, a shared order and an order per chain
    (order group chain + 1)."""
    monkeypatch.setenv("NLMC_NO_FUSED64", "1")
    N, R, T, W = 4096, 48, 5, (7 if order == "per_chain" else 8)
    J, _ = make_instance(N, seed=210)
    h = np.random.default_rng(210).integers(-1, 2, N).astype(np.float64)
    m0 = init_spins(R, N)
    beta = np.repeat(np.geomspace(0.3, 1.2, R)[:, None], T * W, axis=1)
    M, beta, rt = traced(product, J, h, m0, T, W, precision, beta=beta, fused=False, order=order)
    assert rt["planned"] == 0 and not any(rt["fused"])
    groups = np.arange(R) + 1 if order == "per_chain" else None
    assert np.array_equal(M[2], oracle_chain(J, h, m0, beta, 2, precision == "f64", order_group=0 if groups is None else 3))
    qs = oracle.field_scale(oracle.Csr(J), h)[0] if precision == "f32" else None
    assert_law(f"sweep by sweep {order} {precision}", J, h, m0, M, beta, {}, quant_qs=qs, order_groups=groups)


# ---- (g) global-memory kernels --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_global_memory_kernels(product, precision):
    """N = 30 000 > LDS_N: every sweep runs the global-memory kernels (csrc/nlmc_big.h)."""
    N, R, T, W = 30_000, 8, 5, 8
    assert N > product._abi.LDS_N
    J, h = ring_instance(N, 211)
    m0 = init_spins(R, N)
    beta = np.repeat(np.geomspace(0.3, 1.2, R)[:, None], T * W, axis=1)
    M, beta, rt = traced(product, J, h, m0, T, W, precision, beta=beta, fused=False)
    assert not any(rt["fused"])
    assert np.array_equal(M[R - 1], oracle_chain(J, h, m0, beta, R - 1, precision == "f64"))
    qs = oracle.field_scale(oracle.Csr(J), h)[0] if precision == "f32" else None
    assert_law(f"global memory {precision}", J, h, m0, M, beta, {}, quant_qs=qs)


# ---- (h) the bench shape: fp64 fused windows with replica exchange ------------------------------------------------------------
def test_bench_shape_windows_and_swaps(product):
    """N = 10^4, 256 replicas, beta = geomspace(0.05, 4), windows of 10 fp64 sweeps on fused windows, 77-pair swap rounds between
    them: each window's beta per chain from pt_slots() before it.  Wrong: the beta of the neighbouring ladder slot (ratio 1.017).
    The swap decisions are calibrated against min(1, exp(dBeta dE)) with the energies recomputed exactly (integers); the same
    decisions with the sign of dBeta dE flipped must reject."""
    N, R, T, W, PAIRS = 10_000, 256, 10, 4, 77
    J, h = make_instance(N)
    ladder = np.geomspace(0.05, 4.0, R)
    m0 = init_spins(R, N)
    A = sp.csr_matrix(J)
    Ms, betas, nb, dbde, acc_all = [], [], [], [], []
    with product.Engine(product.Instance(J, h), None, R) as eng:
        eng.set_spins(m0)
        eng.pt_init(ladder)
        assert eng.plan_philox_fused(0, W, T, SEED) == W and "f64" in eng.fused_modes(T)
        eng.pt_plan(0, W, SEED, PAIRS)
        for w in range(W):
            slots = eng.pt_slots()
            betas.append(np.repeat(ladder[slots][:, None], T, axis=1))
            nb.append(np.repeat(ladder[np.where(slots < R - 1, slots + 1, R - 2)][:, None], T, axis=1))
            o = eng.sweep_philox(T, SEED, sweep0=w * T, beta=None, precision="f64", record_stride=1)
            assert eng._last_fused(), f"window {w} did not run on fused windows"
            Ms.append(o["spins"])
            s = o["spins"][:, -1].astype(np.float64)
            E = -(np.einsum("rn,rn->r", s, (A @ s.T).T) / 2 + s @ h)
            assert np.array_equal(eng.energy_tracked(), E)
            pairs, acc = eng.pt_swap_philox(w, SEED, PAIRS, want_log=True)
            chain_of = np.empty(R, np.int64)
            chain_of[slots] = np.arange(R)
            i = pairs[0, :, 0]
            assert np.array_equal(pairs[0, :, 1], i + 1)
            ca, cb = chain_of[i], chain_of[i + 1]
            dbde.append((ladder[i + 1] - ladder[i]) * (E[cb] - E[ca]))
            acc_all.append(acc[0].astype(bool))
            after = slots.copy()
            after[ca[acc[0] == 1]], after[cb[acc[0] == 1]] = i[acc[0] == 1] + 1, i[acc[0] == 1]
            assert np.array_equal(eng.pt_slots(), after)
    M = np.concatenate(Ms, axis=1)
    beta = np.concatenate(betas, axis=1)
    assert np.array_equal(Ms[0][0], oracle_chain(J, h, m0, beta[:, :T], 0, True))        # chain 0, first window
    assert_law("bench shape fp64 fused + swaps", J, h, m0, M, beta, {"neighbour_slot_beta": {"beta": np.concatenate(nb, axis=1)}})
    dbde, acc_all = np.concatenate(dbde), np.concatenate(acc_all)
    sw = lawcheck.check_swaps(dbde, acc_all)
    flip = lawcheck.check_swaps(-dbde, acc_all)
    print(f"LAW swaps: decisions={dbde.size} k={sw['k']} t={sw['t']:.2f} max|z|={sw['max_z']:.2f} z_pool={sw['z_pool']:.2f} "
          f"tail={sw['tail_n']}/{sw['tail_max']} (p=1: {sw['n_tail']}); flipped: ok={flip['ok']} max|z|={flip['max_z']:.1f} "
          f"tail={flip['tail_n']}/{flip['tail_max']}")
    assert sw["ok"]
    assert not flip["ok"]
