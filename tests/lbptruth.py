"""High-precision fixed points of the loopy-BP message map (csrc/nlmc_lbp.h, lbp.py), and the inputs on which they are sharp.

On a forest the fixed point of belief propagation is the exact Boltzmann marginal, and at weak coupling on any graph the map is a
contraction: iterating the SAME map in 80-bit long doubles reaches its fixed point to ~1e-19.  That is the expected value of every
test built on this module -- never the device's or the host restatement's own output.  The truth clips the argument of atanh where
the reference does (NMC/nmc.py:230-255: +-(tanh(19.06) - eps)) and nowhere else, ignores the diagonal of J (the reference zeroes
h_msgs[i, i], so J_ii enters the very first node total only and no fixed point), and raises when it does not settle.

Three families of inputs:
  shape_zoo      a forest whose rows pin the degrees at which the kernels change path (0, 7, 8, 9, 15-17, 40), long and short paths,
                 random trees, isolated spins, an optional diagonal;
  message_grid   disjoint pairs that read ONE message u(a = tanh(K), y = Y) through a null measurement on the receiver;
  loopy_graph / complete_graph / tiny_forest   weakly coupled graphs for the routing boundary, the non-edge rule and the barrier.
`bp_copy` is a float64 copy of the host restatement (lbp.loopy_bp) with switches that break it on purpose: the CPU tests show that
each break fails the assertions the GPU tests make.  CPU only; the product package is passed in where it is needed.  No test in here."""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
EPS = np.finfo(float).eps
SAT = float(np.tanh(19.06)) - EPS                 # clip bound of atanh_saturated as the library is handed it
LAMBDAS = (0.5, 0.25, 0.125, 0.0625)              # powers of two: lam * m_star * epsilon is exact for m_star = +-2^k
if not np.finfo(LD).eps < 2e-19:                  # (x86 long double; a platform without it needs an mpmath truth instead)
    raise ImportError("lbptruth needs an extended-precision numpy.longdouble")

# Measured by tests/test_lbp_truth_cpu.py (it prints them and asserts them as upper bounds), used by tests/test_gpu_lbp_exact.py:
#   E_ZOO   largest |host restatement - truth| over the zoo, the boundary graphs, K_12 and the tiny forests (absolute; measured
#           4.16e-16 = 1.88 eps on the zoo at beta = 1, at most 2.3e-16 elsewhere; recorded as the next whole multiple of eps)
#   C_GRID  largest err / (eps (1 + kappa)) over the receivers of the message grid (measured 0.75 at beta = 2.5; recorded as 1)
# so the zoo bound is 8 eps = 1.8e-15 absolute, and a receiver's is 4 eps (1 + kappa): the floors of both rules.
E_ZOO = 2 * EPS
C_GRID = 1.0
ZOO_TOL = max(4 * E_ZOO, 8 * EPS)


def grid_tol(kappa):
    return max(2 * C_GRID, 4.0) * EPS * (1.0 + np.asarray(kappa))


# ---- graphs ----------------------------------------------------------------------------------------------------------------------
def edge_list(J):
    """(n, indptr, src, dst, val, rev) of a symmetric-pattern matrix, entries in CSR order; rev[e] is the position of the
    transposed entry (as lbp.EdgeGraph: the entries sorted by (dst, src) enumerate the reverses in CSR order)."""
    A = sp.csr_matrix(J).astype(np.float64).copy()
    A.eliminate_zeros()
    A.sort_indices()
    n = A.shape[0]
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr))
    dst = A.indices.astype(np.int64)
    rev = np.lexsort((src, dst))
    assert np.array_equal(src[rev], dst) and np.array_equal(dst[rev], src), "pattern not symmetric"
    return n, A.indptr.astype(np.int64), src, dst, A.data.copy(), rev


def _assemble(n, edges, vals, diag_vals=None):
    i, j = np.array(edges, dtype=np.int64).reshape(-1, 2).T
    rows, cols, data = np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([vals, vals])
    if diag_vals is not None:
        k = np.nonzero(diag_vals)[0]
        rows, cols, data = np.concatenate([rows, k]), np.concatenate([cols, k]), np.concatenate([data, diag_vals[k]])
    J = sp.csr_matrix((data, (rows, cols)), shape=(n, n))
    J.sort_indices()
    return J


def _couplings(r, m, lo, hi):
    return np.where(r.random(m) < 0.5, -1.0, 1.0) * r.uniform(lo, hi, m)


STAR_DEGREES = (1, 2, 7, 8, 9, 15, 16, 17, 40)
PATH_LENGTHS = (2, 3, 5, 30)


def shape_zoo(diag, trees=40, seed=1):
    """(J csr, h, components): stars of degree 1, 2, 7, 8, 9, 15, 16, 17 and 40, paths of 2, 3, 5 and 30 spins, `trees` random 12-spin
    trees (the size parameter; 40 gives 647 spins), three isolated spins; |J| in [0.2, 1], h ~ 0.5 N(0, 1).  Spins are relabelled
    by a random permutation (a row's neighbours are scattered over the index range), except that isolated spins sit at index 0 and
    n - 1.  diag: a non-zero J_ii on every third spin and on the centres of the stars of degree 7 and 8 -- drawn in either case, so
    that the off-diagonal part and h are the same."""
    r = np.random.default_rng(seed)
    edges, comps, n = [], [], 0

    def add(k, local):
        nonlocal n
        comps.append(np.arange(n, n + k))
        edges.extend((n + a, n + b) for a, b in local)
        n += k

    for d in STAR_DEGREES:
        add(d + 1, [(0, k) for k in range(1, d + 1)])
    for length in PATH_LENGTHS:
        add(length, [(k, k + 1) for k in range(length - 1)])
    for _ in range(trees):
        add(12, [(int(r.integers(0, k)), k) for k in range(1, 12)])
    for _ in range(3):
        add(1, [])
    perm = r.permutation(n)
    for end, iso in ((0, n - 1), (n - 1, n - 2)):                  # two of the isolated spins to the ends of the index range
        a, b = int(np.nonzero(perm == end)[0][0]), iso
        perm[[a, b]] = perm[[b, a]]
    vals = _couplings(r, len(edges), 0.2, 1.0)
    h = 0.5 * r.standard_normal(n)
    on_diag = np.arange(n) % 3 == 0
    for c, d in zip(comps, STAR_DEGREES):                          # ... and the centres of the stars of degree 7 and 8: stored rows
        if d in (7, 8):                                            # of 8 and 9 entries, one of them the diagonal
            on_diag[perm[c[0]]] = True
    dvals = np.where(on_diag, _couplings(r, n, 0.2, 1.0), 0.0)
    J = _assemble(n, [(perm[a], perm[b]) for a, b in edges], vals, dvals if diag else None)
    return J, h, [np.sort(perm[c]) for c in comps]


def loopy_graph(n, nnz, seed):
    """Ring of n spins plus random chords up to nnz stored entries (nnz / 2 couplings); |J| in [0.1, 0.3], h ~ 0.5 N(0, 1)."""
    assert nnz % 2 == 0 and nnz // 2 >= n
    r = np.random.default_rng(seed)
    have = {(k, (k + 1) % n) if k + 1 < n else (0, k) for k in range(n)}
    while len(have) < nnz // 2:
        a, b = sorted(int(v) for v in r.integers(0, n, 2))
        if a != b:
            have.add((a, b))
    edges = sorted(have)
    return _assemble(n, edges, _couplings(r, len(edges), 0.1, 0.3)), 0.5 * r.standard_normal(n)


def complete_graph(k, isolated, seed=3):
    """K_k with |J| in [0.05, 0.1] (no non-edge in any row: the reference's dh takes no node total), optionally plus one isolated
    spin at the end (then every row has a non-edge)."""
    r = np.random.default_rng(seed)
    edges = [(a, b) for a in range(k) for b in range(a + 1, k)]
    n = k + (1 if isolated else 0)
    return _assemble(n, edges, _couplings(r, len(edges), 0.05, 0.1)), 0.5 * r.standard_normal(n)


def tiny_forest(n, seed=7):
    """A random tree on the spins 0 .. n - 2 and spin n - 1 isolated; n = 2: the single coupling 0 - 1 (with an isolated spin there
    is no message left, and the reference's convergence test is then 0 / 0: it reports divergence)."""
    r = np.random.default_rng(seed + n)
    m = n if n == 2 else n - 1
    edges = [(int(r.integers(0, k)), k) for k in range(1, m)]
    return _assemble(n, edges, _couplings(r, len(edges), 0.2, 1.0)), 0.5 * r.standard_normal(n)


def seeds(P, n, seed=5):
    return np.where(np.random.default_rng(seed).random((P, n)) < 0.5, -1.0, 1.0)


def epsilon_of(J, h):
    """|h| + sum_j |J_ij| (NMC/nmc.py:353), diagonal included.  (The tests hand the SAME array to the device, the host restatement
    and the truth, so its own rounding is no part of any comparison.)"""
    return np.abs(h) + np.asarray(abs(sp.csr_matrix(J)).sum(axis=1)).reshape(-1)


def h_lambda(h, lam, m_star, eps):
    """h + lam (m_star epsilon) in float64, as the device and the reference form it: an INPUT of the fixed point."""
    return h + lam * m_star * eps


# ---- the truth -------------------------------------------------------------------------------------------------------------------
def truth_marginals(J, h_lam, beta, sat=SAT, cap=3000, settle=1e-18):
    """Marginals tanh(beta (h_lam_i + sum_k u_ki)) at the fixed point of synchronous BP
        u_ij <- atanh(clip(tanh(beta J_ij) tanh(beta (h_lam_i + sum_{k != j} u_ki)), +-sat)) / beta
    in long doubles, from u = 0, until no message changes by `settle` or more; raises after `cap` iterations.  J_ii is ignored."""
    n, _, src, dst, val, rev = edge_list(J)
    keep = src != dst
    pos = np.cumsum(keep) - 1
    src, dst, val, rev = src[keep], dst[keep], val[keep], pos[rev[keep]]
    b, s = LD(beta), LD(sat)
    h = np.asarray(h_lam, dtype=np.float64).reshape(-1).astype(LD)
    tJ = np.tanh(b * val.astype(LD))
    u = np.zeros(src.shape[0], dtype=LD)

    def totals(u):
        t = h.copy()
        np.add.at(t, src, u[rev])
        return t

    for _ in range(cap):
        un = np.arctanh(np.clip(tJ * np.tanh(b * (totals(u)[src] - u[rev])), -s, s)) / b
        d = np.max(np.abs(un - u)) if u.size else LD(0)
        u = un
        if d < settle:
            return np.tanh(b * totals(u))
    raise RuntimeError(f"truth_marginals: not settled after {cap} iterations (last change {float(d):.3g})")


def brute_marginals(J, h, beta, comp):
    """<s_i> of the component `comp` (at most 12 spins) under exp(-beta E), E = -(sum_{i<j} J_ij s_i s_j + h . s), by enumeration in
    long doubles (J_ii s_i^2 is a constant)."""
    comp = np.asarray(comp)
    k = comp.shape[0]
    assert k <= 12
    Jc = np.asarray(sp.csr_matrix(J)[comp][:, comp].todense()).astype(LD)
    Jc[np.arange(k), np.arange(k)] = 0
    S = np.array([[1 if (q >> i) & 1 else -1 for i in range(k)] for q in range(1 << k)], dtype=LD)
    mE = LD(0.5) * np.einsum("qi,ij,qj->q", S, Jc, S) + S @ np.asarray(h, dtype=np.float64)[comp].astype(LD)
    w = np.exp(LD(beta) * (mE - np.max(mE)))
    return (w @ S) / np.sum(w)


# ---- the host restatement under the device's calling convention -----------------------------------------------------------------
def run_lambdas(bp, h, eps, m_star, lams, state, max_iterations):
    """The lambda loop as the kernels run it (k_lbp: one launch, all lambdas): bp(h_lam, state) -> (mag, it, state).  Returns
    dict(mag_all [L, n], iters [L], n_lambdas, status) with the library's meaning: a lambda is exhausted when it == max_iterations - 1;
    exhausted at the first one: status 1, nothing written; at a later one: the previous marginals once more, then stop."""
    n, L = h.shape[0], len(lams)
    out = {"mag_all": np.zeros((L, n)), "iters": np.zeros(L, np.int64), "n_lambdas": 0, "status": 0, "mag": np.zeros(n)}
    for l, lam in enumerate(lams):
        mag, it, state = bp(h_lambda(h, lam, m_star, eps), state)
        out["iters"][l] = it
        exhausted = it == max_iterations - 1
        if exhausted and l == 0:
            out["status"] = 1
            break
        if not exhausted:
            out["mag"] = mag
        out["mag_all"][l] = out["mag"]
        out["n_lambdas"] = l + 1
        if exhausted:
            break
    return out


def host_run(product, J, h, eps, m_star, lams, beta, max_iterations=100, tol=EPS):
    """lbp.loopy_bp (bit-exact against the reference's goldens, tests/test_host_lbp.py) over a lambda list, one seed."""
    inst = product.Instance(J, h)
    g = product.lbp.EdgeGraph(inst)
    m_star = np.asarray(m_star, dtype=np.float64)
    state = (np.zeros(g.val.shape[0]), g.val * m_star[g.dst], np.zeros(g.n))
    return run_lambdas(lambda hl, st: product.lbp.loopy_bp(g, hl, beta, st, tol, max_iterations), inst.h, eps, m_star, lams, state,
                       max_iterations)


MUTATIONS = ("scale", "clamp", "row8", "diag")


def bp_copy(J, beta, sat=SAT, tol=EPS, max_iterations=100, mutate=None):
    """A float64 copy of lbp.loopy_bp on the edge list, row sums sequential in ascending neighbour index as in the kernels, as a
    function bp(h_lam, state) for run_lambdas (`start` builds the initial state).  mutate breaks it the way a kernel could be broken:
      "scale"  every message wrong by 1e-11 relative (an ln2 split without its low word is of that size)
      "clamp"  the argument of atanh clipped one ulp above sat
      "row8"   a row sum that stops after 8 terms
      "diag"   h_msgs[i, i] kept instead of zeroed."""
    assert mutate is None or mutate in MUTATIONS
    n, indptr, src, dst, val, rev = edge_list(J)
    tJ = np.tanh(beta * val)
    not_diag = src != dst
    non_nbr = np.bincount(src[not_diag], minlength=n) < n - 1
    take = (np.arange(src.shape[0]) - indptr[src] < 8) if mutate == "row8" else np.ones(src.shape[0], bool)
    clip = float(np.nextafter(sat, 1.0)) if mutate == "clamp" else sat

    def rowsum(u):
        return np.bincount(src[take], weights=u[rev][take], minlength=n)

    def bp(h_lam, state):
        hm, u, tot = state
        it = 0
        for it in range(max_iterations):
            hm_old, u_old, tot_old = hm, u, tot
            tot = h_lam + rowsum(u)
            hm = tot[src] - u[rev]
            if mutate != "diag":
                hm = np.where(not_diag, hm, 0.0)
            u = (1.0 / beta) * np.arctanh(np.clip(tJ * np.tanh(beta * hm), -clip, clip))
            if mutate == "scale":
                u = u * (1.0 + 1e-11)
            with np.errstate(invalid="ignore", divide="ignore"):
                du = np.max(np.abs(u - u_old)) / np.max(np.abs(u) + np.abs(u_old)) if u.size else np.nan
                num = max(np.max(np.abs(hm - hm_old), initial=0.0), np.max(np.abs(tot - tot_old)[non_nbr], initial=0.0))
                den = max(np.max(np.abs(hm) + np.abs(hm_old), initial=0.0), np.max((np.abs(tot) + np.abs(tot_old))[non_nbr], initial=0.0))
                dh = np.float64(num) / np.float64(den)
            if du < tol and dh < tol:
                break
        return np.tanh(beta * (h_lam + rowsum(u))), it, (hm, u, tot)

    def start(m_star):
        return (np.zeros(src.shape[0]), val * np.asarray(m_star, dtype=np.float64)[dst], np.zeros(n))

    return bp, start


# ---- the inputs of tests/test_gpu_lbp_exact.py (tests/test_lbp_truth_cpu.py checks on the CPU that the reference converges on all) ---
class Case:
    """One engine call: instance, real epsilon, seeds [P, n], lambda list, beta, iteration budget -- and, computed once and shared,
    the truth [P, L, n] and the host restatement's result per seed."""

    def __init__(self, name, J, h, beta, P, lams=LAMBDAS, max_iterations=100, ms=None):
        self.name, self.J, self.h, self.beta, self.lams, self.max_iterations = name, J, h, beta, tuple(lams), max_iterations
        self.n = J.shape[0]
        self.eps = epsilon_of(J, h)
        self.ms = seeds(P, self.n) if ms is None else ms
        self._truth, self._host = None, None

    def truth(self):
        if self._truth is None:
            self._truth = np.array([[truth_marginals(self.J, h_lambda(self.h, lam, m, self.eps), self.beta).astype(np.float64)
                                     for lam in self.lams] for m in self.ms])
            self._truth.setflags(write=False)
        return self._truth

    def host(self, product):
        if self._host is None:
            self._host = [host_run(product, self.J, self.h, self.eps, m, self.lams, self.beta, self.max_iterations) for m in self.ms]
        return self._host


BOUNDARY_SIZES = ((2048, 6144), (2048, 6146), (2049, 6144), (2047, 6142))      # (n, nnz) around k_lbp_lds's n <= 2048 && nnz <= 6144
TINY_SIZES = (2, 5, 20)
BATCH_BIAS = 8.0
_cases = {}


def case(name):
    """zoo-<diag>-<beta> (647 spins) | zoo407-<diag>-<beta> (20 trees: n < 512) | boundary-<n>-<nnz> | k12 | k12iso | tiny-<n> | batch | single"""
    if name in _cases:
        return _cases[name]
    kind, *arg = name.split("-")
    if kind in ("zoo", "zoo407"):
        J, h, _ = shape_zoo(arg[0] == "diag", trees=40 if kind == "zoo" else 20)
        c = Case(name, J, h, float(arg[1]), 3)
    elif kind == "boundary":
        n, nnz = int(arg[0]), int(arg[1])
        c = Case(name, *loopy_graph(n, nnz, seed=n + nnz), 0.5, 2)
    elif kind in ("k12", "k12iso"):
        c = Case(name, *complete_graph(12, kind == "k12iso"), 0.5, 3)
    elif kind == "tiny":
        c = Case(name, *tiny_forest(int(arg[0])), 1.0, 2)
    elif kind == "batch":
        # How fast a problem converges is a property of its seed: the bias lam m* epsilon pins the cavity fields, and a perturbation
        # dies within a few hops instead of crossing the 30-spin path.  At beta = 1 the host restatement needs 6 and 8-9 iterations
        # for the two lambdas with |m*| = 8 and 22-29 at the first lambda with |m*| = 1: a budget of 16 lies >= 6 from either.
        J, h, _ = shape_zoo(True)
        s = seeds(3, J.shape[0], seed=11)
        ms = np.stack([BATCH_BIAS * s[0], BATCH_BIAS * s[1], BATCH_BIAS * s[0], BATCH_BIAS * s[1], s[0], s[2]])
        c = Case(name, J, h, 1.0, 6, lams=LAMBDAS[:2], max_iterations=16, ms=ms)
    elif kind == "single":
        J, h, _ = shape_zoo(True)
        c = Case(name, J, h, 1.0, 3, lams=LAMBDAS[:1])
    else:
        raise KeyError(name)
    _cases[name] = c
    return c


ZOO_CASES = tuple(f"zoo-{d}-{b}" for d in ("plain", "diag") for b in ("0.5", "1.0")) + ("zoo407-diag-1.0",)
BOUNDARY_CASES = tuple(f"boundary-{n}-{nnz}" for n, nnz in BOUNDARY_SIZES)
TINY_CASES = tuple(f"tiny-{n}" for n in TINY_SIZES)
CONVERGING_CASES = ZOO_CASES + BOUNDARY_CASES + ("k12", "k12iso") + TINY_CASES + ("single",)


# ---- single messages through a null measurement ----------------------------------------------------------------------------------
GRID_Y = (1e-12, 1e-6, 1e-3, 0.05, 0.3, 0.55, 0.7, 1, 2, 5, 8, 19, 19.06, 19.5, 30, 700)
GRID_K = (1e-9, 1e-3, 0.2, 1, 3, 8, 19.06, 19.5, 40)
GRID_OFFSET = 0.1


def message_grid(beta):
    """Disjoint pairs (receiver i = 2 q, sender j = 2 q + 1) with h_j = +-Y / beta, J_ij = +-K / beta and
    h_i = -u_expected + 0.1 / beta, for zero epsilon: at the fixed point the cavity field of j is h_j, its message to i is
    u = atanh(clip(tanh(K) tanh(Y))) / beta, and m_i = tanh(0.1 + beta (u - u_expected)) -- an error of that ONE message shows at the
    full resolution of a double instead of being flattened by tanh.  Y, K over GRID_Y x GRID_K, both signs of each, kept when
      interior   1 - |x*| >= 1e-3, x* = tanh(K) tanh(Y): the rounding of x to a double is amplified by kappa = |x*| / (1 - x*^2) <= 500;
      clipped    Y >= 19.5 and K >= 19.5: x* lies beyond the clip bound, the message is atanh(sat) / beta whatever x rounds to (kappa = 0).
    Everything between is left out by construction: there kappa reaches 1e13 and the reference's own formula is noise (1e-3 relative at
    a = 1, y = 18).  The SENDER of a pair sits in that zone by design (its field is h_j plus one message): only receivers are looked at.
    All pairs fit one instance (|J| from 4e-10 to 16, |h| up to 280: the engine takes that range, there is nothing to split).
    Returns dict(J, h, recv, send, clipped [bool], kappa, Y, K) with Y, K signed."""
    b = LD(beta)
    sat = LD(SAT)
    rows = []
    for Y in GRID_Y:
        for K in GRID_K:
            for sy in (1.0, -1.0):
                for sk in (1.0, -1.0):
                    hj, Jij = sy * Y / beta, sk * K / beta                       # the doubles the instance holds
                    x = np.tanh(b * LD(Jij)) * np.tanh(b * LD(hj))
                    clipped = Y >= 19.5 and K >= 19.5
                    if not (clipped or 1 - abs(x) >= 1e-3):
                        continue
                    assert (abs(x) > sat) == clipped
                    u = float(np.arctanh(np.clip(x, -sat, sat)) / b)
                    kappa = 0.0 if clipped else float(abs(x) / (1 - x * x))
                    rows.append((-u + GRID_OFFSET / beta, hj, Jij, clipped, kappa, sy * Y, sk * K))
    hi, hj, Jij, clipped, kappa, Y, K = (np.array(c) for c in zip(*rows))
    q = np.arange(len(rows))
    h = np.empty(2 * len(rows))
    h[2 * q], h[2 * q + 1] = hi, hj
    J = _assemble(2 * len(rows), list(zip(2 * q, 2 * q + 1)), Jij)
    return {"J": J, "h": h, "recv": 2 * q, "send": 2 * q + 1, "clipped": clipped.astype(bool), "kappa": kappa, "Y": Y, "K": K}


def grid_report(err, grid):
    """Failure message: the worst receiver of either class, in units of eps (1 + kappa)."""
    ratio = err / (EPS * (1.0 + grid["kappa"]))
    out = []
    for name, m in (("interior", ~grid["clipped"]), ("clipped", grid["clipped"])):
        k = np.nonzero(m)[0][np.argmax(ratio[m])]
        out.append(f"{name}: worst {ratio[k]:.2f} eps(1+kappa) at Y={grid['Y'][k]:g} K={grid['K'][k]:g} kappa={grid['kappa'][k]:.3g} "
                   f"err={err[k]:.3g} ({int(np.sum(ratio[m] > max(2 * C_GRID, 4.0)))} of {int(m.sum())} over the bound)")
    return "; ".join(out)
