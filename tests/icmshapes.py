"""Worst-case inputs of the iso-cluster kernels and a host reference that shares no code with them or with oracle/nlo.c.

Builders return a `Shape`: the instance (J as CSR that may STORE zeros, h), a pair of states and the facts the builder promises about
the disagreement graph (number of components, their sizes, diameter of the largest).  Couplings are +-1 and the field is an
integer in {-1, 0, 1} that is not all zero unless stated otherwise, so every energy is an exact integer.

Reference: scipy.sparse.csgraph.connected_components on the sub-graph induced by {k : s_a[k] s_b[k] = -1} over the stored entries
with `val != 0` (NPT/apt_ICM.py:116-143), components numbered by smallest member; the move is the rule of NPT/apt_ICM.py:232-246 as
restated in tests/fake_engine.py.  Pure NumPy / SciPy: nothing here touches a GPU."""
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components, shortest_path


@dataclass
class Shape:
    name: str
    J: sp.csr_matrix          # both triangles, sorted columns; explicit zeros are part of the instance (zero_bridge)
    h: np.ndarray
    s_a: np.ndarray
    s_b: np.ndarray
    ncomp: int                # promised: components of the disagreement graph
    sizes: list               # promised: their sizes, descending
    diameter: int             # promised: diameter of the largest one
    integer: bool = True      # every J and h an integer: energies compare for equality
    facts: dict = field(default_factory=dict)

    def __post_init__(self):             # shared between tests: nobody writes into a shape
        for a in (self.J.data, self.J.indices, self.J.indptr, self.h, self.s_a, self.s_b):
            a.flags.writeable = False

    @property
    def n(self):
        return self.J.shape[0]

    def with_states(self, s_a, s_b):
        return Shape(self.name, self.J, self.h, np.asarray(s_a, np.int8), np.asarray(s_b, np.int8), -1, [], -1, self.integer)


# ---- reference ----------------------------------------------------------------------------------------------------------------
def components(J, s_a, s_b):
    """-> (labels [n]: smallest member of the spin's component, -1 where the spins agree; components as sorted index arrays in
    ascending-label order; their sizes)."""
    n = J.shape[0]
    d = (np.asarray(s_a, int) * np.asarray(s_b, int)) == -1
    A = sp.csr_matrix(J)
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    keep = (A.data != 0) & d[rows] & d[A.indices]
    G = sp.csr_matrix((np.ones(int(keep.sum())), (rows[keep], A.indices[keep])), shape=(n, n))
    _, comp = connected_components(G, directed=False)
    idx = np.nonzero(d)[0]
    labels = np.full(n, -1, np.int64)
    if idx.size == 0:
        return labels.astype(np.int32), [], np.zeros(0, int)
    smallest = np.full(n, n, np.int64)
    np.minimum.at(smallest, comp[idx], idx)
    labels[idx] = smallest[comp[idx]]
    order = idx[np.argsort(labels[idx], kind="stable")]                 # by label, members ascending inside a component
    cuts = np.nonzero(np.diff(labels[order]))[0] + 1
    comps = np.split(order, cuts)
    return labels.astype(np.int32), comps, np.array([len(c) for c in comps])


def move(J, s_a, s_b, pick, katz):
    """The move on component number `pick` (taken modulo their count) -> (s_a', s_b', (n_components, picked size))."""
    n = J.shape[0]
    _, comps, _ = components(J, s_a, s_b)
    a, b = np.array(s_a, np.int8), np.array(s_b, np.int8)
    if not comps:
        return a, b, (0, 0)
    c = comps[int(pick) % len(comps)]
    if katz and len(c) > n // 2:
        a = (-a).astype(np.int8)
    else:
        a[c], b[c] = np.asarray(s_b, np.int8)[c], np.asarray(s_a, np.int8)[c]
    return a, b, (len(comps), len(c))


def diameter_of_largest(J, s_a, s_b):
    """Longest shortest path inside the largest component (dense all-pairs search: small n only)."""
    _, comps, sizes = components(J, s_a, s_b)
    if not comps:
        return 0
    c = comps[int(np.argmax(sizes))]
    A = sp.csr_matrix(J)
    B = sp.csr_matrix((np.where(A.data != 0, 1.0, 0.0), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    B.eliminate_zeros()
    B = B[c][:, c]
    B.setdiag(0)
    B.eliminate_zeros()
    D = shortest_path(B, directed=False, unweighted=True)
    return int(np.max(D[np.isfinite(D)]))


def csr_parts(shape):
    """(n, indptr, indices, data) with the stored zeros kept: oracle.Csr.from_parts / fake_engine.OracleEngine take these."""
    A = shape.J
    return A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


class HostInstance:
    """What tests/fake_engine.OracleEngine reads of an instance."""

    def __init__(self, shape):
        self.n, self.indptr, self.indices, self.data = csr_parts(shape)
        self.h = np.asarray(shape.h, float)


def engine_instance(product, shape):
    """product.Instance of the shape.  Instance drops explicit zeros, so it is built on the pattern and the values set afterwards
    (as diag_and_zero of tests/test_gpu_apt_lanes.py does)."""
    A = shape.J
    pattern = sp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
    inst = product.Instance(pattern, shape.h)
    assert np.array_equal(inst.indptr, A.indptr) and np.array_equal(inst.indices, A.indices)
    inst.data[:] = A.data
    return inst


# ---- builders -----------------------------------------------------------------------------------------------------------------
def _field(n, r):
    h = r.integers(-1, 2, n).astype(float)
    if not h.any():
        h[n // 2] = 1.0
    return h


def _sym(n, i, j, w):
    """CSR of the undirected edges (i, j) with weights w (both triangles; weights of exactly zero stay stored)."""
    i, j, w = np.asarray(i, np.int64), np.asarray(j, np.int64), np.asarray(w, float)
    off = i != j                                                        # a diagonal entry is stored once
    rows, cols, vals = np.concatenate([i, j[off]]), np.concatenate([j, i[off]]), np.concatenate([w, w[off]])
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    assert not np.any((rows[1:] == rows[:-1]) & (cols[1:] == cols[:-1])), "duplicate edge"
    indptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    return sp.csr_matrix((vals, cols.astype(np.int32), indptr), shape=(n, n))


def _states(n, disagree, r):
    s_a = r.choice(np.array([-1, 1], np.int8), n)
    s_b = s_a.copy()
    s_b[disagree] = -s_b[disagree]
    return s_a, s_b


def _relabel(n, order, r):
    if order == "ascending":
        return np.arange(n)
    if order == "descending":
        return np.arange(n)[::-1].copy()
    if order == "permuted":
        return r.permutation(n)
    raise ValueError(order)


def _path_edges(lab, r):
    return lab[:-1], lab[1:], r.choice([-1.0, 1.0], max(len(lab) - 1, 0))


def path(n, order, agree=(), seed=11):
    """A path through all n spins in the given labelling; every spin disagrees except those at the path POSITIONS `agree`, which
    cut it into runs."""
    r = np.random.default_rng(seed)
    lab = _relabel(n, order, r)
    J = _sym(n, *_path_edges(lab, r))
    mask = np.ones(n, bool)
    mask[list(agree)] = False
    s_a, s_b = _states(n, lab[mask], r)
    runs, cur = [], 0
    for k in range(n):
        if mask[k]:
            cur += 1
        else:
            runs.append(cur)
            cur = 0
    runs.append(cur)
    runs = sorted([x for x in runs if x], reverse=True)
    return Shape(f"path-{order}" + ("-cut" if len(agree) else ""), J, _field(n, r), s_a, s_b, len(runs), runs, (runs[0] - 1) if runs else 0)


def star(n, hub, seed=12):
    """Every spin is joined to `hub` (0 or n - 1) and to nothing else; all disagree."""
    assert hub in (0, n - 1)
    r = np.random.default_rng(seed)
    leaves = np.array([k for k in range(n) if k != hub], np.int64)
    J = _sym(n, np.full(len(leaves), hub), leaves, r.choice([-1.0, 1.0], len(leaves)))
    s_a, s_b = _states(n, np.arange(n), r)
    return Shape(f"star-hub{'0' if hub == 0 else 'last'}", J, _field(n, r), s_a, s_b, 1, [n], min(n - 1, 2))


def complete(n, seed=13):
    r = np.random.default_rng(seed)
    i, j = np.triu_indices(n, 1)
    J = _sym(n, i, j, r.choice([-1.0, 1.0], len(i)))
    s_a, s_b = _states(n, np.arange(n), r)
    return Shape("complete", J, _field(n, r), s_a, s_b, 1, [n], 1 if n > 1 else 0)


def grid(a, b, seed=14):
    """a x b square lattice with open boundaries, all disagreeing."""
    r = np.random.default_rng(seed)
    n = a * b
    k = np.arange(n).reshape(a, b)
    i = np.concatenate([k[:, :-1].ravel(), k[:-1, :].ravel()])
    j = np.concatenate([k[:, 1:].ravel(), k[1:, :].ravel()])
    J = _sym(n, i, j, r.choice([-1.0, 1.0], len(i)))
    s_a, s_b = _states(n, np.arange(n), r)
    return Shape("grid", J, _field(n, r), s_a, s_b, 1, [n], a + b - 2)


def halves(n, over, order="permuted", seed=15):
    """A path through all spins whose disagreeing spins form exactly two runs, one at each end.
    over=False: sizes n // 2 and n // 2 - 1: the larger is NOT above n / 2 and must be exchanged.
    over=True : sizes n // 2 + 1 and n - n // 2 - 2: the larger flips the whole state under katz and is exchanged without."""
    big, small = (n // 2 + 1, n - n // 2 - 2) if over else (n // 2, n // 2 - 1)
    assert small >= 1 and big + small < n
    s = path(n, order, agree=range(big, n - small), seed=seed)
    assert s.sizes == [big, small]
    s.name = f"halves-{'over' if over else 'under'}"
    s.facts["largest"] = big
    return s


def many(n, edges=True, seed=16):
    """edges=True : a perfect matching (an odd n leaves one spin out) and exactly one end of every edge disagrees: n // 2 components
    of one spin.  edges=False: no coupling at all and about two spins in three disagree: each is its own component."""
    r = np.random.default_rng(seed)
    if edges:
        p = r.permutation(n)[:n - n % 2].reshape(-1, 2)
        J = _sym(n, p[:, 0], p[:, 1], r.choice([-1.0, 1.0], len(p)))
        dis = p[np.arange(len(p)), r.integers(0, 2, len(p))]
    else:
        J = sp.csr_matrix((n, n))
        dis = np.nonzero(r.random(n) < 2.0 / 3.0)[0]
        if dis.size == 0:
            dis = np.array([0])
    s_a, s_b = _states(n, dis, r)
    return Shape("many-matching" if edges else "many-edgeless", J, _field(n, r), s_a, s_b, len(dis), [1] * len(dis), 0)


def zero_bridge(n, tiny, seed=17):
    """Two paths (spins 0 .. m-1 and m .. n-1, all disagreeing) joined only by the stored coupling (m-1, m): exactly 0.0 -- no edge, two
    components -- or, tiny=True, 1e-13 -- zero in fixed point, an edge for `val != 0`: one component.  Both variants also store a zero
    between spins 0 and 2 (already joined through 1), so a context built on either reads neighbours from the CSR entries, and a few
    non-zero diagonal entries.  Couplings and fields are real-valued."""
    assert n >= 8
    r = np.random.default_rng(seed)
    m = n // 2 + 1
    i = np.concatenate([np.arange(0, m - 1), np.arange(m, n - 1)])
    w = r.choice([-1.0, 1.0], len(i)) * (0.1 + 0.9 * r.random(len(i)))
    dg = np.unique(r.integers(0, n, 4))
    i_all = np.concatenate([i, [m - 1, 0], dg])
    j_all = np.concatenate([i + 1, [m, 2], dg])
    w_all = np.concatenate([w, [1e-13 if tiny else 0.0, 0.0], 0.25 * r.standard_normal(len(dg))])
    J = _sym(n, i_all, j_all, w_all)
    s_a, s_b = _states(n, np.arange(n), r)
    sizes = [n] if tiny else sorted([m, n - m], reverse=True)
    s = Shape("zero-bridge-tiny" if tiny else "zero-bridge-zero", J, 0.3 * r.standard_normal(n), s_a, s_b, len(sizes), sizes, sizes[0] - 1,
              integer=False)
    s.facts["bridge"] = (m - 1, m)
    return s


def identical(shape):
    """s_b = s_a: no disagreement, info (0, 0), nothing moves."""
    return shape.with_states(shape.s_a, shape.s_a.copy())


def opposite(shape):
    """s_b = -s_a: every spin disagrees, the components are those of the graph."""
    return shape.with_states(shape.s_a, -shape.s_a)


def ladder_states(shape, r):
    """Chain j R + slot: slot 0 of the four ladders holds (s_a, s_b, s_a, s_b), slot 1 (s_a, -s_a, random, s_b)."""
    rand = r.choice(np.array([-1, 1], np.int8), shape.n)
    s = np.empty((8, shape.n), np.int8)
    s[0::2] = [shape.s_a, shape.s_b, shape.s_a, shape.s_b]
    s[1::2] = [shape.s_a, -shape.s_a, rand, shape.s_b]
    return s
