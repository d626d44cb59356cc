"""Device loopy BP (k_lbp in global memory, k_lbp_lds in LDS; csrc/nlmc_lbp.h) against HIGH-PRECISION fixed points (tests/lbptruth.py).

tests/test_gpu_lbp.py compares with the reference at beta = 2.5 on loopy graphs, where the lambda at which the iteration runs out is a
coin toss and 1e-10 is all that can be asked.  Here every input is chosen, and checked on the CPU (tests/test_lbp_truth_cpu.py), so
that the reference converges at every lambda; the expected value is the fixed point of the same map iterated in long doubles (on a
forest: the exact Boltzmann marginal), and the tolerance is the reference's own measured distance from it:
  graphs    |mag_all - truth| <= max(4 E_zoo, 8 eps) = 8 eps = 1.8e-15, E_zoo = 1.88 eps = 4.2e-16 measured on the host restatement
            (recorded as 2 eps).  The factor 4: the device adds a row sequentially where NumPy adds pairwise, plus one more ulp in each
            of its two transcendental steps.
  messages  a receiver of the null-measurement grid within max(2 C_grid, 4) eps (1 + kappa) = 4 eps (1 + kappa), C_grid = 0.75 measured
            (recorded as 1); kappa = |x*| / (1 - x*^2) is the factor by which atanh amplifies the rounding of its argument.
Largest device errors seen on an MI355X (the two routes gave the same bits): zoo 2.31 eps, boundary graphs and K_12 0.5 eps, tiny
forests 1.27 eps, interior receivers 0.81 eps (1 + kappa), clipped receivers 0.75 eps ("Loopy BP against
high-precision fixed points").  No test here found a defect in the kernels.

Every case runs on both routes (NLMC_LBP_GLOBAL is read when an engine is created).  What the shapes pin: HAS_DIAG (J_ii != 0 on a
third of the spins, stored rows of 8 and 9 entries one of which is the diagonal), rows of degree 0, 7, 8, 9, 15-17 and 40 (the tail of
k_lbp_lds's row sum), n < 512 and n < group (empty node slots, workgroups that own nothing), the routing boundary n <= 2048 && nnz <=
6144 at equality and one past it, a complete graph (the non-edge rule switched off), a diverging problem beside converging ones."""
import numpy as np
import pytest

import lbptruth as T

pytestmark = pytest.mark.gpu
EPS = T.EPS
ROUTES = ("lds", "global")
_results = {}


def device(product, monkeypatch, c, route, group=None, ms=None, max_iterations=None, key=None):
    """One engine, one call of nlmc_lbp_convexified on the case's seeds (or `ms`); results are kept per (case, route, group)."""
    k = (c.name, route, group, key)
    if k in _results:
        return _results[k]
    if route == "global":
        monkeypatch.setenv("NLMC_LBP_GLOBAL", "1")
    else:
        monkeypatch.delenv("NLMC_LBP_GLOBAL", raising=False)
    if group is None:
        monkeypatch.delenv("NLMC_LBP_GROUP", raising=False)
    else:
        monkeypatch.setenv("NLMC_LBP_GROUP", str(group))
    with product.Engine(product.Instance(c.J, c.h), None, 1) as eng:
        o = eng.lbp_convexified(c.ms if ms is None else ms, c.eps, list(c.lams), c.beta, EPS,
                                c.max_iterations if max_iterations is None else max_iterations, T.SAT, want_all=True)
    if key is not False:
        _results[k] = o
    return o


def same_bits(a, b, keys=("mag", "mag_all", "iters", "n_lambdas", "status")):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def check_against_truth(product, c, o, what):
    """status 0, every lambda processed, marginals within the zoo tolerance of the truth, iteration counts within 2 of the reference's."""
    L = len(c.lams)
    assert np.all(o["status"] == 0) and np.all(o["n_lambdas"] == L), (what, o["status"], o["n_lambdas"])
    err = float(np.max(np.abs(o["mag_all"] - c.truth())))
    host = np.array([q["iters"] for q in c.host(product)])
    print(f"{what}: device vs truth {err:.3g} = {err / EPS:.2f} eps (bound {T.ZOO_TOL / EPS:g} eps); iterations {o['iters'].tolist()} "
          f"(reference {host.tolist()})")
    assert err <= T.ZOO_TOL, (what, err)
    assert np.array_equal(o["mag"], o["mag_all"][:, L - 1])
    assert np.max(np.abs(o["iters"].astype(np.int64) - host)) <= 2, (what, o["iters"], host)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", T.ZOO_CASES)
def test_zoo_marginals_are_the_exact_ones(product, monkeypatch, name, route):
    """647-spin forest, with and without a diagonal, beta 0.5 and 1, three seeds, four lambdas, the real epsilon, tolerance = machine
    epsilon: the exact Boltzmann marginals to 8 eps (this replaces 1e-10 for these inputs)."""
    c = T.case(name)
    check_against_truth(product, c, device(product, monkeypatch, c, route), f"{name} {route}")


@pytest.mark.parametrize("name", T.ZOO_CASES)
def test_zoo_lds_route_equals_global_route(product, monkeypatch, name):
    """The same operations in the same order: the same bits -- on HAS_DIAG, on rows of degree 0 / 7 / 8 / 9 / 40 and at n < 512."""
    c = T.case(name)
    same_bits(device(product, monkeypatch, c, "lds"), device(product, monkeypatch, c, "global"))


@pytest.mark.parametrize("route", ROUTES)
def test_single_messages_on_the_null_measurement_grid(product, monkeypatch, route):
    """lbp_message_w one message at a time (tests/lbptruth.py: message_grid): beta = 2.5, zero epsilon, one lambda.  The receiver of a
    pair shows tanh(0.1 + beta (u_device - u_expected)): an error of the message u(tanh K, Y) at full resolution.  Interior pairs
    (1 - |x*| >= 1e-3) and clipped ones (the result is usat whatever x rounds to) are reported separately.  ONLY RECEIVERS are
    asserted: a sender's field is h_j plus one message, which puts tanh(K) tanh(beta h_msgs) of the returning message anywhere,
    also into the zone the grid leaves out, where the reference's own formula is noise."""
    g = T.message_grid(2.5)
    n = g["J"].shape[0]
    c = T.Case("grid", g["J"], g["h"], 2.5, 1, lams=(0.5,), ms=np.ones((1, n)))
    c.eps = np.zeros(n)
    o = device(product, monkeypatch, c, route)
    assert o["status"][0] == 0 and o["n_lambdas"][0] == 1 and o["iters"][0, 0] < 98
    truth = T.truth_marginals(g["J"], g["h"], 2.5).astype(np.float64)
    err = np.abs(o["mag_all"][0, 0] - truth)[g["recv"]]
    report = T.grid_report(err, g)
    print(f"grid {route}: {report}")
    assert np.all(err <= T.grid_tol(g["kappa"])), report


@pytest.mark.parametrize("name", T.BOUNDARY_CASES)
def test_routing_boundary(product, monkeypatch, name):
    """(n, nnz) = (2048, 6144) and (2047, 6142) take k_lbp_lds with every edge slot / all but two in use, (2048, 6146) and (2049, 6144)
    are one coupling / one spin past it.  Loopy graphs at |J| <= 0.3, beta = 0.5: a contraction, the truth is its fixed point."""
    c = T.case(name)
    a, b = device(product, monkeypatch, c, "lds"), device(product, monkeypatch, c, "global")
    check_against_truth(product, c, a, f"{name} lds")
    check_against_truth(product, c, b, f"{name} global")
    same_bits(a, b)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["k12", "k12iso"])
def test_complete_graph_switches_the_non_edge_rule_off(product, monkeypatch, name, route):
    """K_12: no row of the dense h_msgs has a non-edge entry, so no node total enters dh; with one isolated spin added every row has."""
    c = T.case(name)
    check_against_truth(product, c, device(product, monkeypatch, c, route), f"{name} {route}")


@pytest.mark.parametrize("name", T.TINY_CASES)
def test_tiny_problems_on_the_group_barrier(product, monkeypatch, name):
    """n = 2, 5, 20 on 2 and 8 workgroups: most of them own no node and no edge and still arrive at every barrier.  (A tree plus an
    isolated spin; n = 2 is the single coupling: two isolated spins exchange no message, and the reference's du is then 0 / 0.)  The
    poll budget is left alone."""
    c = T.case(name)
    one = device(product, monkeypatch, c, "lds")
    check_against_truth(product, c, one, f"{name} lds")
    same_bits(one, device(product, monkeypatch, c, "global"))
    for group in (2, 8):
        same_bits(one, device(product, monkeypatch, c, "global", group=group))


@pytest.mark.parametrize("route", ROUTES)
def test_a_diverging_problem_leaves_its_neighbours_alone(product, monkeypatch, route):
    """Six problems in one launch (tests/lbptruth.py: case "batch"): two strongly biased seeds (|m*| = 8), the same two once more, and two
    seeds of +-1 that run out of the 16 iterations at the first lambda -- convergence speed is a property of the seed, the reference
    needs 6-9 iterations for the former and 22-29 for the latter.  The diverged problems report status 1, no lambda and marginals of
    zero; the others are right, repeat each other bit for bit, and every problem equals the same problem run alone."""
    c = T.case("batch")
    o = device(product, monkeypatch, c, route)
    assert o["status"].tolist() == [0, 0, 0, 0, 1, 1] and o["n_lambdas"].tolist() == [2, 2, 2, 2, 0, 0]
    assert not np.any(o["mag"][4:])
    err = float(np.max(np.abs(o["mag_all"][:4] - c.truth()[:4])))
    print(f"batch {route}: device vs truth {err:.3g} = {err / EPS:.2f} eps; iterations {o['iters'].tolist()}")
    assert err <= T.ZOO_TOL
    host = np.array([q["iters"] for q in c.host(product)])
    assert np.max(np.abs(o["iters"][:4].astype(np.int64) - host[:4])) <= 2
    assert np.all(o["iters"][4:, 0] == c.max_iterations - 1)
    for k in ("mag", "mag_all", "iters"):
        assert np.array_equal(o[k][0:2], o[k][2:4]), k
    for p in range(6):
        alone = device(product, monkeypatch, c, route, ms=c.ms[p:p + 1], key=False)
        assert alone["status"][0] == o["status"][p] and alone["n_lambdas"][0] == o["n_lambdas"][p]
        assert np.array_equal(alone["mag"][0], o["mag"][p]) and np.array_equal(alone["iters"][0, :1], o["iters"][p, :1])
        m = int(o["n_lambdas"][p])
        assert np.array_equal(alone["mag_all"][0, :m], o["mag_all"][p, :m]) and np.array_equal(alone["iters"][0, :m], o["iters"][p, :m])


@pytest.mark.parametrize("route", ROUTES)
def test_degenerate_budgets(product, monkeypatch, route):
    """max_iterations = 0: no iteration, every lambda reports the marginals of the INITIAL messages u = J m* (it = 0 is not
    max_iterations - 1); max_iterations = 1: iteration 0 is the last one, so every problem diverges; a lambda list of one entry."""
    c = T.case("zoo-diag-1.0")
    o = device(product, monkeypatch, c, route, max_iterations=0, key="budget0")
    assert np.all(o["status"] == 0) and np.all(o["n_lambdas"] == len(c.lams)) and not np.any(o["iters"])
    host = np.array([T.host_run(product, c.J, c.h, c.eps, m, c.lams, c.beta, 0)["mag_all"] for m in c.ms])
    err = float(np.max(np.abs(o["mag_all"] - host)))
    print(f"max_iterations = 0, {route}: device vs host restatement {err:.3g} = {err / EPS:.2f} eps")
    assert err <= T.ZOO_TOL and np.array_equal(o["mag"], o["mag_all"][:, -1])
    o = device(product, monkeypatch, c, route, max_iterations=1, key="budget1")
    assert np.all(o["status"] == 1) and not np.any(o["n_lambdas"]) and not np.any(o["mag"]) and not np.any(o["iters"])
    s = T.case("single")
    check_against_truth(product, s, device(product, monkeypatch, s, route), f"single lambda {route}")


def test_degenerate_budgets_are_the_same_bits_on_both_routes(product, monkeypatch):
    c = T.case("zoo-diag-1.0")
    for budget in (0, 1):
        same_bits(device(product, monkeypatch, c, "lds", max_iterations=budget, key=f"budget{budget}"),
                  device(product, monkeypatch, c, "global", max_iterations=budget, key=f"budget{budget}"),
                  keys=("mag", "iters", "n_lambdas", "status") + (("mag_all",) if budget == 0 else ()))
    same_bits(device(product, monkeypatch, T.case("single"), "lds"), device(product, monkeypatch, T.case("single"), "global"))
    same_bits(device(product, monkeypatch, T.case("batch"), "lds"), device(product, monkeypatch, T.case("batch"), "global"),
              keys=("mag", "iters", "n_lambdas", "status"))
