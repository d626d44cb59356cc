"""Device loopy BP (include/nlmc.h: nlmc_lbp_convexified) against the reference's golden
marginals and against the oracle's dense restatement (oracle/refport.py) on larger graphs.

Tolerance: the device sums each node's incoming messages sequentially and uses the GPU's fp64 tanh/atanh, the
reference uses NumPy's pairwise association and NumPy's own SIMD tanh/arctanh -> agreement to rounding.  A fixed
point of the message map is reached to ~1 ulp by both, so marginals agree to 1e-10 absolute where both visit the same
lambdas; the lambda at which the iteration budget runs out is a knife-edge (convergence is tested against machine
epsilon: it is a 1-ulp limit cycle), so the tests compare every lambda both sides converged on and compare clusters
only when both stopped at the same lambda.  The sharp bound (8 eps against high-precision fixed points, on inputs where
the reference converges at every lambda) is in tests/test_gpu_lbp_exact.py.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import golden, golden_names
from helpers import make_instance

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
TOL = 1e-10


def inst_of(product, g):
    A = sp.csr_matrix((g["data"], g["indices"], g["indptr"]), shape=(int(g["N"]),) * 2)
    return product.Instance(A, g["h"])


@pytest.mark.parametrize("name", golden_names("lbp_"))
def test_device_lbp_matches_reference_golden(product, name):
    g = golden(name)
    inst = inst_of(product, g)
    graph = product.lbp.EdgeGraph(inst)
    eps = graph.epsilon(inst.h)
    with product.Engine(inst, None, 1) as eng:
        cls, margs = product.lbp.lbp_convexified_device(
            eng, graph, float(g["lambda_start"]), float(g["lambda_end"]), float(g["lambda_reduction_factor"]),
            g["m_star"].astype(float)[None], eps, EPS, int(g["max_iterations"]), float(g["threshold_initial"]),
            float(g["threshold_cutoff"]), float(g["global_beta"]), want_marginals=True)
    lam = np.array(sorted(margs[0].keys(), reverse=True))
    n_ref, n_dev = len(g["lambdas"]), len(lam)
    m = min(n_ref, n_dev)
    assert np.array_equal(lam[:m], g["lambdas"][:m])
    # The lambda loop stops where an LBP call runs out of iterations.  With tolerance = machine epsilon that happens
    # when the iteration falls into a 1-ulp limit cycle (the reference does at lambda = 0.45 on chimera128: du stays at
    # 3.3e-16 for 75 iterations), which depends on the last bit of every sum: the stop may differ, the marginals of
    # every lambda both sides converged on may not.  (The entry AT the stop is a copy of the previous one.)
    k = m if n_ref == n_dev else m - 1
    assert k >= 10
    got = np.array([margs[0][l] for l in lam[:k]])
    assert np.max(np.abs(got - g["marginals"][:k])) < TOL
    if n_ref == n_dev:
        cl = cls[0]
        assert np.array_equal(np.array([len(c) for c in cl], dtype=np.int64), g["cluster_sizes"])
        cat = np.concatenate(cl).astype(np.int64) if cl else np.zeros(0, np.int64)
        assert np.array_equal(cat, g["clusters_concat"])


def low_energy_states(J, h, P, seed, beta=3.0, sweeps=200):
    import oracle
    csr = oracle.Csr(J)
    out = []
    for p in range(P):
        s = np.where(np.random.default_rng(seed + p).random(csr.n) < 0.5, -1, 1).astype(np.int8)
        cb = np.tile(np.array(oracle.cb_pair(beta)), (sweeps, 1))
        _, s, _ = oracle.sweeps_philox(csr, h, s, cb, 77, p, want_M=False)
        out.append(s.astype(np.float64))
    return np.stack(out)


def test_device_lbp_batch_vs_oracle(product):
    """Three seeds at once on a 300-spin graph against the oracle's dense line-by-line restatement of the reference."""
    from oracle import refport
    J, h = make_instance(300, seed=11)
    inst = product.Instance(J, h)
    graph = product.lbp.EdgeGraph(inst)
    eps = graph.epsilon(inst.h)
    ms = low_energy_states(J, h, 3, seed=5)
    args = (0.5, 0.01, 0.9)
    with product.Engine(inst, None, 1) as eng:
        cls, margs = product.lbp.lbp_convexified_device(eng, graph, *args, ms, eps, EPS, 100, 0.999999, 0.99999, 2.5,
                                                        want_marginals=True)
    Jd = np.asarray(J.todense()) if sp.issparse(J) else np.asarray(J)
    for p in range(3):
        rc, rm = refport.lbp_convexified(Jd, np.asarray(h, float).reshape(-1), *args, ms[p].copy(), eps, EPS, 100,
                                         0.999999, 0.99999, 2.5, want_marginals=True)
        lam_ref = sorted(rm.keys(), reverse=True)
        lam_dev = sorted(margs[p].keys(), reverse=True)
        m = min(len(lam_ref), len(lam_dev))
        common = lam_dev[:m if len(lam_ref) == len(lam_dev) else m - 1]
        assert lam_ref[:m] == lam_dev[:m] and len(common) >= 1
        for l in common:
            assert np.max(np.abs(margs[p][l] - np.asarray(rm[l]).reshape(-1))) < TOL
        if len(lam_ref) == len(lam_dev):
            assert [sorted(map(int, c)) for c in cls[p]] == [sorted(map(int, c)) for c in rc]


def test_device_lbp_divergence(product):
    """Error behaviour: ValueError when the first lambda exhausts the iterations (NMC/nmc.py:142-144).  (A J whose
    pattern is not symmetric is refused by Engine() before it can reach nlmc_lbp_convexified's own check.)"""
    J, h = make_instance(120, seed=2)
    inst = product.Instance(J, h)
    graph = product.lbp.EdgeGraph(inst)
    eps = graph.epsilon(inst.h)
    ms = np.where(np.random.default_rng(0).random((1, 120)) < 0.5, -1.0, 1.0)
    with product.Engine(inst, None, 1) as eng:
        with pytest.raises(ValueError, match="LBP diverged at initial lambda"):
            product.lbp.lbp_convexified_device(eng, graph, 0.5, 0.01, 0.9, ms, eps, EPS, 3, 0.999999, 0.99999, 2.5)


def test_device_lbp_bench_size(product):
    """N = 10^4, 8 seeds in one launch: finishes, marginals in [-1, 1], consistent with the host restatement (lbp.py,
    itself bit-exact against the reference's goldens) on the lambdas both visit."""
    J, h = make_instance(10_000, seed=3)
    inst = product.Instance(J, h)
    graph = product.lbp.EdgeGraph(inst)
    eps = graph.epsilon(inst.h)
    ms = low_energy_states(J, h, 2, seed=9, sweeps=100)
    ms = np.concatenate([ms] * 4)
    with product.Engine(inst, None, 1) as eng:
        cls, margs = product.lbp.lbp_convexified_device(eng, graph, 0.5, 0.01, 0.9, ms, eps, EPS, 100, 0.999999, 0.99999,
                                                        2.5, want_marginals=True)
    for p in range(2):
        assert [sorted(margs[p + 2 * k].keys()) for k in range(4)] == [sorted(margs[p].keys())] * 4   # deterministic
        hc, hm = product.lbp.lbp_convexified(inst, 0.5, 0.01, 0.9, ms[p].copy(), eps, EPS, 100, 0.999999, 0.99999, 2.5,
                                             graph=graph, want_marginals=True)
        lam_h, lam_d = sorted(hm.keys(), reverse=True), sorted(margs[p].keys(), reverse=True)
        m = min(len(lam_h), len(lam_d))
        assert m >= 2 and lam_h[:m] == lam_d[:m]
        for l in lam_d[:m if len(lam_h) == len(lam_d) else m - 1]:
            assert np.max(np.abs(margs[p][l] - hm[l])) < 1e-9
            assert np.all(np.abs(margs[p][l]) <= 1.0)


def test_device_lbp_does_not_depend_on_workgroups_per_problem(product, monkeypatch):
    """A problem may be spread over 1, 2, 4 or 8 workgroups (one group barrier per BP iteration): row sums stay
    sequential and maxima are order-independent, so marginals, iteration counts and the stopping lambda are the same
    bits for every grouping."""
    J, h = make_instance(3000, seed=19, with_h=True, gaussian=True)
    inst = product.Instance(J, h)
    graph = product.lbp.EdgeGraph(inst)
    eps = graph.epsilon(inst.h)
    ms = low_energy_states(J, h, 3, seed=2, sweeps=60)
    lams = product.lbp.lambda_list(0.5, 0.01, 0.9)
    res = {}
    for grp in (1, 2, 4, 8):
        monkeypatch.setenv("NLMC_LBP_GROUP", str(grp))
        with product.Engine(inst, None, 1) as eng:
            res[grp] = eng.lbp_convexified(ms, eps, lams, 2.5, EPS, 60, float(np.tanh(19.06)) - EPS, want_all=True)
    for grp in (2, 4, 8):
        for k in ("mag", "n_lambdas", "iters", "status", "mag_all"):
            assert np.array_equal(res[grp][k], res[1][k]), (grp, k)
    assert res[1]["n_lambdas"].min() >= 2


@pytest.mark.parametrize("N,P", [(300, 3), (1000, 16), (1500, 5)])
def test_lds_resident_kernel_equals_the_global_memory_kernel(product, N, P, monkeypatch):
    """k_lbp_lds (small instances: messages in LDS, a thread's edges in registers) does the operations of k_lbp in the same
    order: marginals, lambda counts and iteration counts are the same bits.  This is also the test of k_lbp_lds's exact-cycle
    exit (it leaves a lambda whose message array has started to repeat; k_lbp has no such exit and runs every lambda to
    max_iterations): nearly every seed ends its lambda loop on an exhausted lambda, and all outputs must still be equal."""
    J, h = make_instance(N, seed=N, with_h=True)
    inst = product.Instance(J, h)
    graph = product.lbp.EdgeGraph(inst)
    eps = graph.epsilon(inst.h)
    ms = low_energy_states(J, h, P, seed=3, sweeps=60).astype(np.float64)
    lams = product.lbp.lambda_list(3.0, 0.05, 0.85)
    sat = float(np.tanh(19.06)) - EPS
    with product.Engine(inst, None, 1) as eng:
        a = eng.lbp_convexified(ms, eps, lams, 2.5, EPS, 100, sat, want_all=True)
    monkeypatch.setenv("NLMC_LBP_GLOBAL", "1")                # (read when an engine is created)
    with product.Engine(inst, None, 1) as eng:
        b = eng.lbp_convexified(ms, eps, lams, 2.5, EPS, 100, sat, want_all=True)
    for k in ("mag", "n_lambdas", "status"):
        assert np.array_equal(a[k], b[k]), k
    assert a["n_lambdas"].min() >= 3
    assert sum(int(a["iters"][q, int(a["n_lambdas"][q]) - 1]) == 99 for q in range(P)) >= 1      # exhausted lambdas were seen
    for q in range(P):                        # (rows behind the last processed lambda are not written)
        m = int(a["n_lambdas"][q])
        assert np.array_equal(a["iters"][q, :m], b["iters"][q, :m])
        assert np.array_equal(a["mag_all"][q, :m], b["mag_all"][q, :m])


def test_group_barrier_timeout_falls_back_to_one_workgroup_per_problem(product, monkeypatch):
    """the workgroups that share one inference poll each other with a bounded budget and give up when they are
    not all resident (another context on the GPU); the call then runs once more with one workgroup per problem instead of
    failing.  Provoked here with a poll budget of ONE poll; the result must equal the undisturbed call bit for bit."""
    N = 9000
    J, h = make_instance(N, seed=5)
    inst = product.Instance(J, h)
    graph = product.lbp.EdgeGraph(inst)
    eps = graph.epsilon(inst.h)
    ms = low_energy_states(J, h, 1, seed=2, sweeps=40).astype(np.float64)
    lams = product.lbp.lambda_list(3.0, 0.5, 0.7)
    sat = float(np.tanh(19.06)) - EPS
    monkeypatch.setenv("NLMC_LBP_GROUP", "4")                 # (knobs are read when an engine is created)
    with product.Engine(inst, None, 1) as eng:
        a = eng.lbp_convexified(ms, eps, lams, 2.5, EPS, 60, sat)
    monkeypatch.setenv("NLMC_LBP_POLL_BUDGET", "1")
    with product.Engine(inst, None, 1) as eng:
        b = eng.lbp_convexified(ms, eps, lams, 2.5, EPS, 60, sat)
    assert a["status"][0] == 0 and b["status"][0] == 0
    assert np.array_equal(a["mag"], b["mag"]) and np.array_equal(a["n_lambdas"], b["n_lambdas"])


def test_lambda_continuation_stops_where_the_reference_stops_on_average(product):
    """Where LBP_convexified ends its lambda loop (NMC/nmc.py:139-150) is decided by rounding noise: the tolerance is machine
    epsilon, the loop ends at the first lambda whose messages do not become bit-stable in max_iterations.  Seed by seed that is
    a coin toss between any two arithmetics (std of the difference ~4 lambdas), but its MEAN is a property of the arithmetic:
    a message formula that skips the reference's intermediate roundings (tanh(beta h) and tanh(beta J) * tanh(beta h) as
    doubles) ran 2.8 lambdas deeper on these 64 seeds (5 sigma) and handed weaker-bias marginals to the cluster search.
    Fixture: the reference itself on 64 C3-shape seeds (tools/make_golden.py lbpstat; mean 33.3 lambdas).  Bound: 3 sigma."""
    g = golden("stats_lbp_lambdas_c3")
    J, h = make_instance(1000)
    inst = product.Instance(J, h)
    graph = product.lbp.EdgeGraph(inst)
    eps = graph.epsilon(inst.h)
    ms = g["m_star"].astype(np.float64)
    lams = product.lbp.lambda_list(float(g["lambda_start"]), float(g["lambda_end"]), float(g["lambda_reduction_factor"]))
    with product.Engine(inst, None, ms.shape[0]) as eng:
        o = eng.lbp_convexified(ms, eps, lams, float(g["global_beta"]), EPS, int(g["max_iterations"]), float(np.tanh(19.06)) - EPS)
    assert np.all(o["status"] == 0)
    ref = g["n_lambdas_reference"].astype(np.int64)
    dev = o["n_lambdas"].astype(np.int64)
    d = dev - ref
    assert abs(d.mean()) <= 3.0 * d.std() / np.sqrt(len(d)) + 0.25, (dev.mean(), ref.mean(), d.std())
    assert abs(d.mean()) <= 1.7
