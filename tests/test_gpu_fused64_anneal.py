"""The fp64 mode on fused windows with a temperature per sweep (an anneal): k_sweep_fused's output variant, integer thresholds, with
a ring of three K tables, one per threshold slot, rebuilt at every sweep's cb.  Unflagged chains only.  The real-valued variant
(Engine.set_fused_f64_real) keeps such a call sweep by sweep: its anneal measured slower there than the sweep-by-sweep kernel
(measured and rejected), so its cases here assert that route (fused_last_call False) and the same bits.
APT_ICM.MCMC sweeps at one fixed beta in the "f32" arithmetic and never makes such a call; NMC is the drop-in that does.

Every comparison is bit for bit: fused == the same call with NLMC_NO_FUSED64=1 (sweep by sweep) == the sequential fp64 oracle with a
coefficient pair per sweep.

`PYTHONPATH=. python tests/test_gpu_fused64_anneal.py` from the repository root, with the library of the commit BEFORE this feature
(NLMC_LIB names a library built from it) on the GPU, rewrites tests/golden/fused64_anneal_parent.npz, the recorded outputs
test_nothing_moved compares with: that is how the committed file was made."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
from helpers import make_instance, init_spins

pytestmark = pytest.mark.gpu
SEED = 0xA11EA1
HERE = os.path.dirname(os.path.abspath(__file__))
INST = os.path.join(HERE, "golden", "instances")
PARENT = os.path.join(HERE, "golden", "fused64_anneal_parent.npz")
OUT_KEYS = ("spins", "energy", "min_energy", "argmin", "argmin_state")
LBP = dict(lambda_start=3.0, lambda_end=0.3, lambda_reduction_factor=0.8, threshold_initial=0.9999, threshold_cutoff=0.97,
           max_iterations=100)


def pmj2048():
    J, _ = make_instance(2048, seed=111)
    return J, np.zeros(2048)


def chimera_normalised():
    import nlmc_amd as P
    W, h = P.instances.txt_to_A_droplet(os.path.join(INST, "chimera2048__001.txt"))
    J = sp.csr_matrix(W).astype(np.float64)
    s = np.max(np.abs(J.data))
    J = (J / s).tocsr()
    J.sort_indices()
    return J, np.asarray(h, dtype=np.float64).ravel() / s


def table(R, S, lo=0.05, hi=4.0):
    """[R, S] inverse temperatures, cold start to hot end, a different value at every sweep and rows that differ between chains."""
    return np.stack([np.geomspace(lo * (1 + 0.1 * c), hi / (1 + 0.07 * c), S) for c in range(R)])


def call(product, J, h, m0, beta, T, real=False, budget=None, precision="f64", stride=1):
    """One sweep_philox_windows call of beta.shape[1] sweeps with every per-sweep output."""
    R, S = beta.shape
    with product.Engine(product.Instance(J, h), None, R) as eng:
        eng.set_fused_f64_real(real)
        eng.set_spins(m0)
        E0 = eng.energy()
        o = eng.sweep_philox_windows(S, SEED, beta=beta, window=T, budget_bytes=budget, precision=precision, record_stride=stride,
                                     want_energy=True, want_min=True, want_state=True)
        st = eng.last_schedule_stats()
        return {"o": o, "fused": eng.fused_last_call, "lv": st["levels"] / max(1, st["orders"]), "final": eng.get_spins(),
                "E": eng.energy_tracked(), "E0": E0, "esc": eng.energy_scale}


def same(a, b):
    for k in OUT_KEYS:
        assert np.array_equal(a["o"][k], b["o"][k]), k
    assert np.array_equal(a["final"], b["final"]) and np.array_equal(a["E"], b["E"])


def pair(product, monkeypatch, J, h, m0, beta, T, real=False, budget=None):
    """The call, and the same call on an engine created under NLMC_NO_FUSED64=1: the same bits, fewer levels per sweep."""
    f = call(product, J, h, m0, beta, T, real, budget)
    monkeypatch.setenv("NLMC_NO_FUSED64", "1")
    p = call(product, J, h, m0, beta, T, real, budget)
    monkeypatch.delenv("NLMC_NO_FUSED64")
    assert not p["fused"]
    same(f, p)
    return f, p


def check_oracle(J, h, m0, beta, res, chains):
    csr = oracle.Csr(J)
    esc, o = res["esc"], res["o"]
    for c in chains:
        cb = np.array([oracle.cb_pair(b, 1.0, True) for b in beta[c]])
        M, s_fin, tr = oracle.sweeps_philox(csr, h, m0[c], cb, SEED, c, escale=esc, use_f64=True,
                                            efix0=int(np.rint(res["E0"][c] * 2.0 ** esc)))
        assert np.array_equal(o["spins"][c], M), f"chain {c}"
        assert np.array_equal(o["energy"][c], tr * 2.0 ** -esc), f"chain {c}"
        am = int(np.argmin(tr))
        assert o["argmin"][c] == am and o["min_energy"][c] == tr[am] * 2.0 ** -esc, f"chain {c}"
        assert np.array_equal(o["argmin_state"][c], M[am]), f"chain {c}"
        assert np.array_equal(res["final"][c], s_fin) and res["E"][c] == tr[-1] * 2.0 ** -esc, f"chain {c}"


def test_pmj_anneal_runs_on_fused_windows(product, monkeypatch):
    """+-J, h = 0, four chains, no flags, a [R, 20] table whose rows differ: the integer-threshold variant with its ring of K tables."""
    J, h = pmj2048()
    R, S, T = 4, 20, 5
    m0, beta = init_spins(R, 2048), table(R, S)
    f, p = pair(product, monkeypatch, J, h, m0, beta, T)
    assert f["fused"] is True
    assert f["lv"] < p["lv"]
    check_oracle(J, h, m0, beta, f, range(R))


@pytest.mark.parametrize("kind", ["chimera", "gaussian"])
def test_real_valued_anneal(product, monkeypatch, kind):
    """Real couplings (Chimera-2048 / max|J|: k / 75; Gaussian couplings and fields) with the real-valued variant switched on: a
    temperature per sweep stays sweep by sweep there (measured and rejected), with the option off as well."""
    J, h = chimera_normalised() if kind == "chimera" else make_instance(3000, seed=41, with_h=True, gaussian=True)
    R, S, T = 4, 20, 5
    m0, beta = init_spins(R, J.shape[0]), table(R, S)
    f, p = pair(product, monkeypatch, J, h, m0, beta, T, real=True)
    assert f["fused"] is False and f["lv"] == p["lv"]
    check_oracle(J, h, m0, beta, f, range(R))
    q = call(product, J, h, m0, beta, T, real=False)        # option off, not dyadic: sweep by sweep, the same bits
    assert q["fused"] is False and q["lv"] == p["lv"]
    same(q, f)


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("mask", ["0", "0x7800000"])
def test_tie_path_takes_the_sweeps_own_threshold(product, monkeypatch, real, mask):
    """NLMC_F64_TIE_MASK = 0 sends every update through the exact 53-bit comparison; 0x7800000 keeps the top four of the high word's
    27 bits, which sends about one update in sixteen of the integer-threshold variant there (some 10^4 of the call's 1.6e5) and
    widens the real-valued variant's interval of u to a sixteenth: a K table taken from the wrong sweep shows there.  The real-valued
    call runs sweep by sweep, where the mask has nothing to widen: the same bits."""
    J, h = chimera_normalised() if real else pmj2048()
    R, S, T = 4, 20, 5
    m0, beta = init_spins(R, 2048), table(R, S)
    ref = call(product, J, h, m0, beta, T, real)
    monkeypatch.setenv("NLMC_F64_TIE_MASK", mask)
    t = call(product, J, h, m0, beta, T, real)
    monkeypatch.delenv("NLMC_F64_TIE_MASK")
    assert ref["fused"] is (not real) and t["fused"] is (not real)
    same(t, ref)
    check_oracle(J, h, m0, beta, t, range(R))


def stretch_table(R, S):
    """Chain 0 changes at every sweep; the others hold one temperature over the first third of the call and change from there on."""
    b = table(R, S)
    for c in range(1, R):
        b[c, :S // 3] = b[c, 0]
    return b


@pytest.mark.parametrize("T", [3, 5, 20])
@pytest.mark.parametrize("mult", [3, 7])
def test_window_seams_and_lengths(product, monkeypatch, T, mult):
    """S = 3 T and 7 T: every window starts with the K tables of its own first two sweeps.  Integer thresholds on every shape; the
    real-valued instance on the same shapes, sweep by sweep."""
    R, S = 3, mult * T
    m0 = init_spins(R, 2048)
    for real, (J, h) in ((False, pmj2048()), (True, chimera_normalised())):
        for beta in (table(R, S), stretch_table(R, S)):
            f, p = pair(product, monkeypatch, J, h, m0, beta, T, real)
            assert f["fused"] is (not real) and (f["lv"] < p["lv"]) == (not real)
            check_oracle(J, h, m0, beta, f, range(R))


@pytest.mark.parametrize("real", [False, True])
def test_pieces_cut_the_table(product, monkeypatch, real):
    """A small plan budget cuts the call into several pieces, each planned and swept on its own columns of the table; in the first
    piece every chain holds one temperature (its launches take the plain rule), the later ones change at every sweep.  Real-valued:
    the first piece runs on fused windows, the others sweep by sweep, so the call as a whole reports False."""
    J, h = chimera_normalised() if real else pmj2048()
    R, T, S = 3, 5, 40
    m0, beta = init_spins(R, 2048), table(R, S)
    with product.Engine(product.Instance(J, h), None, R) as eng:
        eng.set_fused_f64_real(real)
        budget = 2 * eng.fused_plan_bytes(T)                      # two windows per piece: four pieces
    beta[:, :2 * T] = beta[:, :1]
    f, p = pair(product, monkeypatch, J, h, m0, beta, T, real, budget=budget)
    assert f["fused"] is (not real) and (f["lv"] < p["lv"]) == (not real)      # (lv: the last piece's)
    one = call(product, J, h, m0, beta, T, real)
    same(f, one)
    check_oracle(J, h, m0, beta, f, range(R))


def integer_instance(N, wmax, seed):
    """+-J graph with integer weights in [1, wmax) and small integer fields: the field range grows with wmax."""
    Jb, _ = make_instance(N, seed=seed)
    rng = np.random.default_rng(seed)
    U = sp.triu(Jb, 1).tocsr()
    U.data = U.data * rng.integers(1, wmax, U.nnz)
    J = (U + U.T).tocsr()
    J.sort_indices()
    return J, rng.integers(-3, 4, N).astype(np.float64)


@pytest.mark.parametrize("wmax,fused", [(40, True), (300, False)])
def test_field_range_and_the_lds_rule(product, monkeypatch, wmax, fused):
    """The rule of fused_route for a temperature per sweep: three tables of 2 xmax + 1 entries fit in LDS and 8 (2 xmax + 1) <= n.
    Weights below 40 at N = 8192 (several table entries per producing thread) pass it, weights below 300 do not and run sweep by sweep;
    the bits are the same, and fused_last_call tells which kernel ran."""
    N, R, S, T = 8192, 3, 10, 5
    J, h = integer_instance(N, wmax, 101)
    with product.Engine(product.Instance(J, h), None, 1) as eng:
        qs = eng.field_scale
    xmax = int(np.max(np.abs(np.rint(np.ldexp(h, qs))) + np.asarray(abs(J * 2.0 ** qs).sum(axis=1)).ravel()))
    assert (8 * (2 * xmax + 1) <= N) == fused and (fused or xmax <= 4095)     # the case is on the side of the rule it is meant for
    m0, beta = init_spins(R, N), table(R, S, lo=0.05 / wmax, hi=4.0 / wmax)
    f, p = pair(product, monkeypatch, J, h, m0, beta, T)
    assert f["fused"] is fused
    assert (f["lv"] < p["lv"]) == f["fused"] and (f["fused"] or f["lv"] == p["lv"])
    if fused:
        check_oracle(J, h, m0, beta, f, range(R))


@pytest.mark.parametrize("real", [False, True])
def test_diagonal(product, monkeypatch, real):
    """J with a diagonal (the field of the energy delta leaves it out): the integer-threshold variant on fused windows, the
    real-valued instance sweep by sweep."""
    N, R, S, T = 2600, 3, 15, 5
    rng = np.random.default_rng(131)
    if real:
        J, h = make_instance(N, seed=131, with_h=True, gaussian=True)
        J = (J + sp.diags(rng.standard_normal(N) * 0.4)).tocsr()
    else:
        J, _ = make_instance(N, seed=131)
        J = (J + sp.diags(rng.integers(-2, 3, N).astype(np.float64))).tocsr()
        h = rng.integers(-1, 2, N).astype(np.float64)
    J.sort_indices()
    m0, beta = init_spins(R, N), table(R, S)
    f, p = pair(product, monkeypatch, J, h, m0, beta, T, real)
    assert f["fused"] is (not real) and (f["lv"] < p["lv"]) == (not real)
    check_oracle(J, h, m0, beta, f, range(R))


@pytest.fixture
def fused_calls(product, monkeypatch):
    """(phase flags in force, fused_last_call, the beta table changes along the sweeps) of every Engine.sweep_philox_windows call
    with precision="f64"."""
    seen = []
    orig = product.Engine.sweep_philox_windows

    def spy(self, *a, **kw):
        o = orig(self, *a, **kw)
        if kw.get("precision") == "f64":
            b = np.asarray(kw.get("beta", 0.0), dtype=np.float64)
            seen.append((self._flags_on, self.fused_last_call, bool(b.ndim == 2 and (b != b[:, :1]).any())))
        return o

    monkeypatch.setattr(product.Engine, "sweep_philox_windows", spy)
    return seen


def dropin_instance(kind):
    if kind == "chimera":
        return chimera_normalised()
    J, _ = make_instance(2000, seed=211)
    return J, np.random.default_rng(211).integers(-1, 2, 2000).astype(np.float64)


@pytest.mark.parametrize("kind", ["chimera", "pmj"])
def test_dropin_anneals(product, monkeypatch, fused_calls, kind):
    """NMC(rng="philox", precision="f64"): MCMC(anneal=True), run and run_restarts with an anneal of 60 sweeps in front equal the same
    calls with the fused fp64 kernels off, the anneal is an unflagged fp64 call with a temperature per sweep that ran on fused windows
    on the +-J instance (integer thresholds) and sweep by sweep on Chimera-2048 / max|J| (real-valued), and MCMC(anneal=True) is the
    oracle's fp64 sweep on the same beta_schedule."""
    import nlmc_amd as P
    J, h = dropin_instance(kind)
    N = J.shape[0]
    m0 = np.sign(2 * np.random.default_rng(5).random(N) - 1)

    def go():
        with contextlib.redirect_stdout(io.StringIO()):
            obj = product.NMC(J, h, rng="philox", seed=31, lbp="host", precision="f64")
            t0 = obj._sweep_counter
            M = obj.MCMC(60, m0, 2.5, J, h, anneal=True)
            r = product.NMC(J, h, rng="philox", seed=32, lbp="host", precision="f64").run(
                num_sweeps_initial=60, num_sweeps_per_NMC_phase=20, num_NMC_cycles=1, **LBP)
            rr = product.NMC(J, h, rng="philox", seed=33, lbp="device", precision="f64").run_restarts(
                6, num_sweeps_initial=60, num_sweeps_per_NMC_phase=12, num_NMC_cycles=1, temp_x=20, global_beta=2.5,
                all_clusters=np.arange(0, N, 7))
        return M, r, rr, t0

    M1, r1, rr1, t0 = go()
    anneals = [(fl, fz) for fl, fz, per_sweep in fused_calls if per_sweep]
    assert anneals == [(False, kind == "pmj")] * 3, fused_calls     # MCMC, run, run_restarts: one anneal each, no flags in force
    assert any(fl and fz for fl, fz, _ in fused_calls)              # (the phases with flags ran on fused windows as before)
    fused_calls.clear()
    monkeypatch.setenv("NLMC_NO_FUSED64", "1")
    M2, r2, rr2, _ = go()
    monkeypatch.delenv("NLMC_NO_FUSED64")
    assert not any(fz for _, fz, _ in fused_calls)
    assert np.array_equal(M1, M2)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]) and r1[2] == r2[2]
    for a, b in zip(rr1, rr2):
        assert np.array_equal(a, b)
    sched = P.hostlogic.beta_schedule(60, 2.5, True, 1, 0)
    cb = np.array([oracle.cb_pair(b, 1.0, True) for b in sched])
    Mo, _, _ = oracle.sweeps_philox(oracle.Csr(J), h, m0.astype(np.int8), cb, 31, 0, sweep0=t0, use_f64=True)
    assert np.array_equal(M1.T, Mo)


def parent_cases(product):
    """What this feature must leave alone, on the instance of the first test: an fp64 call with one temperature per chain and an
    f32 call with a table per sweep (both with per-sweep outputs, both on fused windows before and after)."""
    J, h = pmj2048()
    R, S, T = 4, 20, 5
    m0 = init_spins(R, 2048)
    flat = np.repeat(np.geomspace(0.3, 3.0, R)[:, None], S, axis=1)
    out = {}
    for name, beta, prec in (("f64_flat", flat, "f64"), ("f32_table", table(R, S), "f32")):
        r = call(product, J, h, m0, beta, T, precision=prec)
        for k in OUT_KEYS:
            out[f"{name}.{k}"] = r["o"][k]
        out[f"{name}.final"], out[f"{name}.E"], out[f"{name}.fused"] = r["final"], r["E"], np.array(r["fused"])
    return out


def test_nothing_moved(product):
    """The bits and the route recorded from the commit before this feature (see the module docstring)."""
    want = np.load(PARENT)
    got = parent_cases(product)
    assert sorted(want.files) == sorted(got)
    for k in want.files:
        assert np.array_equal(want[k], got[k]), k
    assert bool(want["f64_flat.fused"]) and bool(want["f32_table.fused"])


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    from conftest import load_product
    np.savez_compressed(PARENT, **parent_cases(load_product()))
    print("wrote", PARENT)
