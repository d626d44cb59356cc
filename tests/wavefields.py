"""The data flow of the wave-per-chain sweeps (csrc/nlmc_waves.h) restated in NumPy, for ONE chain: a dense fixed-point matrix, local
fields that stay resident and are corrected when a neighbour flips, and from the field on the operations of the spec.  It shares
with the oracle only its leaf functions (oracle.philox, oracle.threshold, oracle.field_scale); the sweep itself -- the order, the
fields, the decision, the energy delta -- is written out here, so that tests/test_waves_cpu.py can hold it against
oracle.sweeps_philox without a GPU.  No test in here."""
import numpy as np
import scipy.sparse as sp

import oracle

TAG_UNIFORM, TAG_ORDER = 1, 2


def dense_instance(n, seed=1, diag=False):
    """Complete graph: symmetric Gaussian couplings scaled to max |J| = 1, Gaussian fields (optionally a non-zero diagonal)."""
    r = np.random.default_rng(seed)
    A = r.standard_normal((n, n))
    J = np.triu(A, 1)
    J = J + J.T
    if diag:
        J[np.arange(n), np.arange(n)] = r.standard_normal(n)
    J /= np.max(np.abs(J))
    return J, 0.3 * r.standard_normal(n)


def wishart(P, golden, i=1):
    """(J, h, norm factor, listed ground-state energy) of the Wishart N = 10 golden instance i, divided by max |J| as run() does."""
    import os
    inst = os.path.join(golden, "instances")
    fn = f"wishart_planting_N_10_alpha_0.50_inst_{i}.txt"
    W, _ = P.instances.txt_to_A_wishart(os.path.join(inst, "wishart_N10_a0.50__" + fn))
    J = (-W).toarray()
    nf = float(np.max(np.abs(J)))
    gs = {l.split()[0]: float(l.split()[1]) for l in open(os.path.join(inst, "wishart_N10_a0.50__gs_energies.txt"))}
    return J / nf, np.zeros(J.shape[0]), nf, gs[fn]


def phase_flags(R, N, m0, seed=1):
    """Phase flags 0 / 1 / 2 / 3 per (chain, spin): even chains scale clusters and freeze the rest at its start value, odd chains
    freeze the clusters; the last chain has all its spins frozen."""
    r = np.random.default_rng(seed)
    flags = np.zeros((R, N), np.uint8)
    for c in range(R):
        cl = r.random(N) < 0.2
        if c % 2 == 0:
            flags[c, cl] = 1
            flags[c, ~cl] = np.where(m0[c, ~cl] > 0, 2, 3)
        else:
            flags[c, cl] = np.where(m0[c, cl] > 0, 2, 3)
    flags[R - 1] = np.where(m0[R - 1] > 0, 2, 3)
    return flags


def dense_matrix(J, h, qs):
    """(Jd [n, n] int64 with Jq = rint(J 2^qs) of every stored entry, diagonal included and equal columns of a row added up;
    hq [n] int64)."""
    A = sp.csr_matrix(J)
    n = A.shape[0]
    Jd = np.zeros((n, n), dtype=np.int64)
    for k in range(n):
        for e in range(A.indptr[k], A.indptr[k + 1]):
            Jd[k, A.indices[e]] += int(np.rint(np.ldexp(float(A.data[e]), qs)))
    hq = np.rint(np.ldexp(np.asarray(h, dtype=np.float64).reshape(-1), qs)).astype(np.int64)
    return Jd, hq


def visiting_order(n, t, group, seed):
    """Spins in ascending order of (philox(k, t, group, ORDER)[0], k)."""
    lo, hi = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    keys = [int(oracle.philox(k, t, group, TAG_ORDER, lo, hi)[0]) for k in range(n)]
    return sorted(range(n), key=lambda k: (keys[k], k))


def sweeps(J, h, s_start, cb_run, seed, chain_id, order_group=0, sweep0=0, flags=None, escale=None, efix0=0):
    """(M [S, n] int8 spins after every sweep, final spins, energy trace [S] int64) of the fixed-point mode with resident fields.
    cb_run: [S, 2] (normal, scaled) as oracle.cb_pair gives them."""
    csr = oracle.Csr(J)
    qs, es = oracle.field_scale(csr, h)
    escale = es if escale is None else int(escale)
    Jd, hq = dense_matrix(J, h, qs)
    n = Jd.shape[0]
    # the matrix is used by rows (row k corrects the fields when k flips) and, in the prologue, by columns: J == J^T
    assert np.array_equal(Jd, Jd.T)
    s = np.asarray(s_start, dtype=np.int64).reshape(-1).copy()
    fl = np.zeros(n, dtype=np.int64) if flags is None else np.asarray(flags, dtype=np.int64).reshape(-1)
    cb_run = np.asarray(cb_run, dtype=np.float64).reshape(-1, 2)
    lo, hi = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    X = hq.copy()                                              # prologue: X_j = hq_j + sum_i Jd[i][j] s_i, row by row
    for i in range(n):
        X += Jd[i] * s[i]
    assert np.all(np.abs(X) < 2 ** 31)
    S = cb_run.shape[0]
    M, tr, E = np.empty((S, n), dtype=np.int8), np.empty(S, dtype=np.int64), int(efix0)
    for t in range(S):
        tt = (int(sweep0) + t) & 0xFFFFFFFF
        W = np.empty(4 * ((n + 3) // 4), dtype=np.float32)     # four thresholds per Philox block, one call per block and sweep
        for b in range((n + 3) // 4):
            r = oracle.philox(b, tt, chain_id, TAG_UNIFORM, lo, hi)
            W[4 * b:4 * b + 4] = [oracle.threshold(int(r[q])) for q in range(4)]
        for k in visiting_order(n, tt, order_group, seed):
            if fl[k] >= 2:                                     # frozen: keeps its value and adds nothing
                continue
            cbq = np.float32(np.ldexp(np.float32(cb_run[t, 1 if fl[k] == 1 else 0]), -qs))
            z = np.float32(cbq * np.float32(int(X[k])))
            so, sn = int(s[k]), (1 if z < W[k] else -1)
            if sn != so:
                E += (int(X[k]) - int(Jd[k, k]) * so) * ((so - sn) << (escale - qs))      # the diagonal term left out
                s[k] = sn
                X += (sn - so) * Jd[k]                         # ... but not out of the field: lane k's own entry included
                assert np.all(np.abs(X) < 2 ** 31)
        M[t], tr[t] = s, E
    return M, s.astype(np.int8), tr
