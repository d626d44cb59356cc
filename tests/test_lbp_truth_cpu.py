"""The oracle of tests/test_gpu_lbp_exact.py, checked without a GPU (tests/lbptruth.py):
  * the long-double fixed point IS the exact Boltzmann marginal wherever that can be enumerated;
  * the reference (lbp.loopy_bp, bit-exact against the reference's goldens) converges on every input the GPU tests use, so no GPU
    assertion depends on where a limit cycle begins;
  * how far the reference's own float64 arithmetic lies from the truth: E_zoo (absolute, on graphs) and C_grid (in units of
    eps (1 + kappa), on single messages).  Both are printed (pytest -s) and asserted as upper bounds against the constants the GPU
    tests take their tolerances from;
  * a copy of the host restatement broken in each of the ways a kernel could be broken fails the assertions the GPU tests make."""
import numpy as np
import pytest

import lbptruth as T
from conftest import load_product

EPS = T.EPS


@pytest.fixture(scope="module")
def P():
    return load_product()


@pytest.mark.parametrize("diag", [False, True])
@pytest.mark.parametrize("beta", [0.5, 1.0])
def test_truth_is_the_exact_boltzmann_marginal_on_small_components(diag, beta):
    J, h, comps = T.shape_zoo(diag, trees=6)
    eps = T.epsilon_of(J, h)
    h_lam = T.h_lambda(h, 0.25, T.seeds(1, J.shape[0])[0], eps)
    m = T.truth_marginals(J, h_lam, beta)
    small = [c for c in comps if len(c) <= 12]
    assert len(small) >= 6 + 3 + 3 + 5                    # trees, isolated spins, short paths, stars up to degree 9
    worst = max(float(np.max(np.abs(m[c] - T.brute_marginals(J, h_lam, beta, c)))) for c in small)
    assert worst < 1e-17, worst


def test_zoo_has_the_rows_the_kernels_change_path_on():
    for diag in (False, True):
        J, h, comps = T.shape_zoo(diag)
        n, indptr, src, dst, _, _ = T.edge_list(J)
        assert n == 647 and sum(len(c) for c in comps) == n
        deg = np.bincount(src[src != dst], minlength=n)
        assert {0, 1, 2, 7, 8, 9, 15, 16, 17, 40} <= set(deg.tolist())
        assert deg[0] == 0 and deg[n - 1] == 0
        assert bool(np.any(src == dst)) == diag
        if diag:
            rows = np.diff(indptr)
            assert np.any((rows == 1) & (deg == 0)) and np.any((rows == 9) & (deg == 8)) and np.any((rows == 8) & (deg == 7))
    a, b = T.shape_zoo(False), T.shape_zoo(True)
    off = b[0].copy()
    off.setdiag(0)
    off.eliminate_zeros()
    assert (off != a[0]).nnz == 0 and np.array_equal(a[1], b[1])


def test_truth_raises_when_it_does_not_settle():
    J, h, _ = T.shape_zoo(False, trees=1)
    with pytest.raises(RuntimeError, match="not settled"):
        T.truth_marginals(J, h, 1.0, cap=5)


def test_reference_converges_on_every_gpu_input_and_its_distance_from_the_truth(P):
    """`it < max_iterations - 1` at every lambda of every seed, and E_zoo."""
    worst = {}
    for name in T.CONVERGING_CASES:
        c = T.case(name)
        for o in c.host(P):
            assert o["status"] == 0 and o["n_lambdas"] == len(c.lams), name
            assert np.all(o["iters"] < c.max_iterations - 1), (name, o["iters"])
        worst[name] = max(float(np.max(np.abs(o["mag_all"] - t))) for o, t in zip(c.host(P), c.truth()))
    for name, e in worst.items():
        print(f"host restatement vs truth, {name}: {e:.3g} = {e / EPS:.2f} eps")
    e_zoo = max(worst.values())
    print(f"E_zoo = {e_zoo:.3g} = {e_zoo / EPS:.2f} eps (recorded: {T.E_ZOO / EPS:g} eps; zoo tolerance {T.ZOO_TOL:.3g})")
    assert e_zoo <= T.E_ZOO
    assert max(int(np.max(o["iters"])) for o in T.case("zoo-diag-1.0").host(P)) <= 40


def test_batch_case_diverges_for_the_unbiased_seeds_only(P):
    c = T.case("batch")
    o = c.host(P)
    assert [q["status"] for q in o] == [0, 0, 0, 0, 1, 1]
    for q in o[:4]:
        assert q["n_lambdas"] == 2 and np.all(q["iters"] <= c.max_iterations - 1 - 3), q["iters"]     # the device may differ by +-2
    hundred = T.Case("batch100", c.J, c.h, c.beta, 2, lams=c.lams, ms=c.ms[4:])
    for q in hundred.host(P):
        assert q["status"] == 0 and q["iters"][0] >= c.max_iterations - 1 + 3, q["iters"]
    # the iteration budgets 0 and 1 (zoo-diag-1.0 with max_iterations replaced): nothing to converge
    z = T.case("zoo-diag-1.0")
    for budget, status in ((0, 0), (1, 1)):
        for m in z.ms:
            assert T.host_run(P, z.J, z.h, z.eps, m, z.lams, z.beta, budget)["status"] == status


def test_grid_holds_both_classes_and_the_reference_is_accurate_on_it(P):
    """C_grid; at least 100 interior pairs and 16 clipped ones; the reference converges."""
    g = T.message_grid(2.5)
    n = g["J"].shape[0]
    assert n <= 2048 and g["J"].nnz <= 6144                  # one instance, on either route
    assert int(np.sum(~g["clipped"])) >= 100 and int(np.sum(g["clipped"])) >= 16
    assert np.all(g["kappa"][g["clipped"]] == 0) and np.max(g["kappa"]) <= 500
    for small in (1e-12, 1e-6):                              # the k == 0 branch of the device's logarithm, both signs
        assert np.sum(np.abs(g["Y"]) == small) >= 4
    o = T.host_run(P, g["J"], g["h"], np.zeros(n), np.ones(n), [0.5], 2.5)
    assert o["status"] == 0 and o["iters"][0] < 98
    truth = T.truth_marginals(g["J"], g["h"], 2.5).astype(np.float64)
    assert np.max(np.abs(truth[g["recv"]] - np.tanh(T.GRID_OFFSET))) < 1e-15      # the null measurement: every receiver at tanh(0.1)
    err = np.abs(o["mag_all"][0] - truth)[g["recv"]]
    c_grid = float(np.max(err / (EPS * (1 + g["kappa"]))))
    print(f"C_grid = {c_grid:.3g} (recorded: {T.C_GRID:g}); largest receiver error {err.max():.3g}; {T.grid_report(err, g)}")
    assert c_grid <= T.C_GRID


# ---- sensitivity: what "would fail if the kernel were subtly wrong" means here ---------------------------------------------------
def copy_errors(mutate):
    """(zoo error, grid errors [pairs]) of the float64 copy of the host restatement, broken as `mutate` says (None: intact)."""
    c = T.case("zoo-diag-1.0")
    bp, start = T.bp_copy(c.J, c.beta, mutate=mutate)
    zoo = 0.0
    for m, t in zip(c.ms, c.truth()):
        o = T.run_lambdas(bp, c.h, c.eps, m, c.lams, start(m), c.max_iterations)
        k = o["n_lambdas"]
        zoo = max(zoo, float(np.max(np.abs(o["mag_all"][:k] - t[:k]))) if k else np.inf)
    g = T.message_grid(2.5)
    n = g["J"].shape[0]
    bp, start = T.bp_copy(g["J"], 2.5, mutate=mutate)
    o = T.run_lambdas(bp, g["h"], np.zeros(n), np.ones(n), [0.5], start(np.ones(n)), 100)
    truth = T.truth_marginals(g["J"], g["h"], 2.5).astype(np.float64)
    return zoo, np.abs(o["mag_all"][0] - truth)[g["recv"]], g


def test_the_intact_copy_passes_both_assertions():
    zoo, err, g = copy_errors(None)
    assert zoo <= T.ZOO_TOL and np.all(err <= T.grid_tol(g["kappa"])), (zoo, T.grid_report(err, g))


@pytest.mark.parametrize("mutate,zoo_fails,grid_fails", [
    ("scale", True, "interior"),        # a message formula wrong by 1e-11 relative
    ("clamp", False, "clipped"),        # a clamp one ulp off: seen by the clipped class alone (no zoo message saturates)
    ("row8", True, None),               # a row sum that drops its ninth term
    ("diag", True, None),               # the diagonal's h_msgs kept
])
def test_a_broken_copy_fails_the_assertions_of_the_gpu_tests(mutate, zoo_fails, grid_fails):
    zoo, err, g = copy_errors(mutate)
    bad = err > T.grid_tol(g["kappa"])
    print(f"{mutate}: zoo error {zoo:.3g} (bound {T.ZOO_TOL:.3g}); grid: {T.grid_report(err, g)}")
    assert (zoo > T.ZOO_TOL) == zoo_fails
    if grid_fails == "interior":
        assert np.sum(bad & ~g["clipped"]) >= 50
    elif grid_fails == "clipped":
        assert np.all(bad[g["clipped"]]) and not np.any(bad[~g["clipped"]])
    else:
        assert not np.any(bad)          # (pairs have one neighbour and no diagonal)
