"""Calibration of recorded heat-bath sweeps against the exact law (plain NumPy / SciPy; imports nothing of the product or oracle).

The reference's update (NMC/nmc.py:86-87) sets s' = +1 with probability p = (1 + tanh(beta x)) / 2 = expit(2 beta x), where x is
the field the spin sees when its turn comes in a sweep whose order is a random permutation.  In the throughput mode that order is
shared by the chains of a sweep (or drawn per chain), a pure function of (seed, sweep, order group): spins sorted by
(philox(k, sweep, order_group, TAG_ORDER)[0], k).  Given the start states and every sweep's recorded configuration, the field of
every update is therefore known exactly, and its outcome is one Bernoulli draw with a known probability.  Millions of updates
make a calibration test whose power comes from their number, not from a reference sample:

  - score statistic of a temperature-scale error   Z_beta = sum (sigma - th) a / sqrt(I),  I = sum (1 - th^2) a^2,
    a = beta x, th = tanh(a), sigma = +-1 the outcome;
  - calibration by log-odds: bins of width 0.5 in ln(p / (1 - p)), adjacent bins merged until V = sum p (1 - p) >= 100,
    z_b = (O_b - E_b) / sqrt(V_b);
  - tail pool: updates with min(p, 1 - p) < 1e-9; the number of outcomes against the field must not exceed the upper 1e-7
    Poisson quantile of sum min(p, 1 - p);
  - every |z| < t = Phi^-1(1 - 1e-6 / (2 k)), k the number of z statistics.

Every update counts, in exactly one bin or in the tail pool.  Rows with phase flag 2 or 3 never change and are no samples; rows
with flag 1 run at beta / temp_x.  The power of a run is delta* = 2 t / sqrt(I): a temperature error of that relative size is
resolved with margin.
"""
import math

import numpy as np
import scipy.sparse as sp
from scipy import special, stats

TAG_ORDER = 2
BIN_WIDTH = 0.5
TAIL_P = 1e-9
FAMILY_ALPHA = 1e-6
TAIL_ALPHA = 1e-7
MIN_BIN_VAR = 100.0

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_LO32 = np.uint64(0xFFFFFFFF)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11), vectorised over the counter words (broadcast); returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _LO32 for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = _M0 * c0
        p1 = _M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _LO32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _LO32
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def order_positions(n, sweep, seed, order_group=0):
    """Position of every spin in the order of sweep `sweep`: spins sorted by (philox(k, sweep, group, TAG_ORDER)[0], k).
    order_group: 0 (shared order) -> [n]; an array of groups (order="per_chain": chain_base + chain + 1) -> [len, n]."""
    g = np.asarray(order_group, dtype=np.uint64)
    k = np.arange(n, dtype=np.uint64)
    key = philox(k[None, :], np.uint64(sweep & 0xFFFFFFFF), g.reshape(-1, 1), TAG_ORDER, seed & 0xFFFFFFFF, seed >> 32)[0]
    order = np.sort((key << np.uint64(32)) | k[None, :], axis=1) & _LO32   # by key, ties by the spin index
    pos = np.empty(order.shape, dtype=np.int64)
    np.put_along_axis(pos, order.astype(np.int64), np.broadcast_to(np.arange(n), order.shape), axis=1)
    return pos[0] if g.ndim == 0 else pos


class Instance:
    """CSR J (both triangles, a diagonal allowed) and h, as the checker reads them."""

    def __init__(self, J, h):
        A = sp.csr_matrix(J).astype(np.float64).copy()
        A.eliminate_zeros()
        A.sort_indices()
        self.n = A.shape[0]
        self.A = A
        self.h = np.asarray(h, dtype=np.float64).reshape(-1)
        self.rows = np.repeat(np.arange(self.n), np.diff(A.indptr))
        self.cols = A.indices.astype(np.int64)
        self.ind = sp.csr_matrix((np.ones(A.nnz), np.arange(A.nnz), A.indptr), shape=(self.n, A.nnz))
        v = np.concatenate([A.data, self.h])
        self.grain = None                                   # 2^q: every field an exact multiple of 2^-q (dyadic instances)
        for q in range(9):
            if np.all(np.ldexp(v, q) == np.rint(np.ldexp(v, q))) and np.sum(np.abs(np.ldexp(v, q))) < 2.0 ** 50:
                self.grain = 2.0 ** q
                break

    def jacobi(self, s):
        """x [n, R] with every neighbour at s [n, R] (float64)."""
        return self.A @ s + self.h[:, None]

    def moved(self, pos, d, before=True):
        """sum over the neighbours j updated before (after) k in the order of the change d = new - old [n, R]: what turns the
        Jacobi field into the sequential one (the diagonal term stays at the old s_k: it is neither before nor after)."""
        if pos.ndim == 1:
            m = (pos[self.cols] < pos[self.rows]) if before else (pos[self.cols] > pos[self.rows])
            return sp.csr_matrix((self.A.data * m, self.A.indices, self.A.indptr), shape=self.A.shape) @ d
        pT = np.ascontiguousarray(pos.T)                        # [n, R]: contiguous rows to gather
        pc, pr = pT[self.cols], pT[self.rows]
        vals = d[self.cols] * ((pc < pr) if before else (pc > pr))
        vals *= self.A.data[:, None]
        return self.ind @ vals


class Tally:
    """Accumulates updates given in groups of equal probability: log-odds lo = ln(p / (1 - p)), n_up outcomes s' = +1 (or swaps
    accepted) out of n_tot, and optionally d, the summed bound on how far the group's probabilities may sit from p (the "f32"
    mode's quantised couplings)."""

    NB = 2 * int(math.ceil(math.log(1.0 / TAIL_P) / BIN_WIDTH)) + 4
    TAIL_LO = math.log((1.0 - TAIL_P) / TAIL_P)           # min(p, 1 - p) < 1e-9  <=>  |lo| > TAIL_LO

    def __init__(self, score=True, pooled=False):
        self.score, self.pooled = score, pooled
        self.O, self.E, self.V, self.D, self.cnt = (np.zeros(self.NB) for _ in range(5))
        self.tail_n, self.tail_mu, self.n_tail = 0, 0.0, 0
        self.num, self.info, self.n = 0.0, 0.0, 0
        self.frozen_changed = 0

    def add(self, lo, n_up, n_tot=None, d=None):
        """n_tot None: one update per entry (n_up its outcome, 0 or 1)."""
        lo = np.asarray(lo, dtype=np.float64).ravel()
        n_up = np.asarray(n_up, dtype=np.float64).ravel()
        if lo.size == 0:
            return
        ones = n_tot is None
        n_tot = np.ones_like(lo) if ones else np.asarray(n_tot, dtype=np.float64).ravel()
        self.n += lo.size if ones else int(round(n_tot.sum()))
        al = np.abs(lo)
        m = special.expit(-al)                                  # against the field: min(p, 1 - p), relative accuracy kept
        v = m * (1.0 - m)                                       # p (1 - p)
        tail = al > self.TAIL_LO
        if tail.any():
            lt, ut, nt = lo[tail], n_up[tail], n_tot[tail]
            self.tail_n += int(round(np.sum(np.where(lt > 0, nt - ut, ut))))       # outcomes against the field
            self.tail_mu += float(np.sum(nt * m[tail]))
            self.n_tail += int(round(nt.sum()))
        if self.score:
            a = 0.5 * lo
            th = np.copysign(1.0 - 2.0 * m, lo)                   # tanh(a)
            self.num += float(np.sum((2.0 * n_up - n_tot * (1.0 + th)) * a))
            self.info += 4.0 * float(np.sum(n_tot * v * (a * a)))  # 1 - tanh(a)^2 = 4 p (1 - p)
        if tail.any():
            body = ~tail
            lo, n_up, n_tot, m, v = lo[body], n_up[body], n_tot[body], m[body], v[body]
            d = None if d is None else np.asarray(d, dtype=np.float64).ravel()[body]
        p = np.where(lo > 0, 1.0 - m, m)
        b = np.floor(lo * (1.0 / BIN_WIDTH)).astype(np.int64) + self.NB // 2
        self.O += np.bincount(b, weights=n_up, minlength=self.NB)
        if ones:
            self.E += np.bincount(b, weights=p, minlength=self.NB)
            self.V += np.bincount(b, weights=v, minlength=self.NB)
            self.cnt += np.bincount(b, minlength=self.NB)
        else:
            self.E += np.bincount(b, weights=n_tot * p, minlength=self.NB)
            self.V += np.bincount(b, weights=n_tot * v, minlength=self.NB)
            self.cnt += np.bincount(b, weights=n_tot, minlength=self.NB)
        if d is not None:
            self.D += np.bincount(b, weights=d, minlength=self.NB)

    def bins(self):
        """Adjacent fine bins merged left to right until V >= 100 (a remainder joins the last bin): [(O, E, V, D, count)]."""
        out, cur = [], np.zeros(5)
        for i in range(self.NB):
            if self.cnt[i] == 0:
                continue
            cur += (self.O[i], self.E[i], self.V[i], self.D[i], self.cnt[i])
            if cur[2] >= MIN_BIN_VAR:
                out.append(cur)
                cur = np.zeros(5)
        if cur[4]:
            if out:
                out[-1] = out[-1] + cur
            else:
                out.append(cur)
        return out

    def result(self):
        bins = self.bins()
        zb = np.array([(o - e) / math.sqrt(v) if v > 0 else (0.0 if o == e else math.inf) for o, e, v, _, _ in bins])
        zs = list(zb)
        z_beta = self.num / math.sqrt(self.info) if (self.score and self.info > 0) else None
        if z_beta is not None:
            zs.append(z_beta)
        z_pool = None
        if self.pooled:
            V = sum(b[2] for b in bins)
            z_pool = (sum(b[0] for b in bins) - sum(b[1] for b in bins)) / math.sqrt(V) if V > 0 else 0.0
            zs.append(z_pool)
        k = max(1, len(zs))
        t = float(stats.norm.isf(FAMILY_ALPHA / (2 * k)))
        tail_max = int(stats.poisson.isf(TAIL_ALPHA, self.tail_mu)) if self.tail_mu > 0 else 0
        max_z = float(np.max(np.abs(zs))) if zs else 0.0
        return {
            "n": self.n, "k": k, "t": t, "z_bins": zb, "z_beta": z_beta, "z_pool": z_pool, "max_z": max_z,
            "info": self.info, "delta_star": (2.0 * t / math.sqrt(self.info)) if self.info > 0 else math.inf,
            "tail_n": self.tail_n, "tail_mu": self.tail_mu, "tail_max": tail_max, "n_tail": self.n_tail,
            "frozen_changed": self.frozen_changed,
            "quant_ok": all(b[3] <= math.sqrt(b[2]) for b in bins),
            "ok": max_z < t and self.tail_n <= tail_max and self.frozen_changed == 0,
        }


def quantisation_bound(inst, qs):
    """d_k / beta = sum_j |J_kj - rint(J_kj 2^qs) 2^-qs| / 2 + |h_k - rint(h_k 2^qs) 2^-qs| / 2 : how far the "f32" mode's
    fixed-point couplings can move P(s' = +1) of row k, per unit of beta (|dp/dx| <= beta / 2)."""
    dJ = np.abs(inst.A.data - np.ldexp(np.rint(np.ldexp(inst.A.data, qs)), -qs))
    dh = np.abs(inst.h - np.ldexp(np.rint(np.ldexp(inst.h, qs)), -qs))
    return 0.5 * (np.bincount(inst.rows, weights=dJ, minlength=inst.n) + dh)


def _group(x, up, cls, quant, n_cls, grain):
    """Updates of one sweep -> groups of equal (class, field): class = 2 chain + scaled, so that any hypothesis that only changes
    the inverse temperatures gives every member of a group the same probability.  Dyadic instances (every field an exact
    multiple of 1 / grain, grain <= 2^8) collapse to a few groups per chain; other fields stay one update per group (n_tot None)."""
    if grain is not None:
        xi = (x * grain).astype(np.int64)                      # exact
        off = int(xi.min())
        K = int(xi.max()) - off + 1
        key = cls * K + (xi - off)
        nt = np.bincount(key, minlength=n_cls * K)
        keep = np.nonzero(nt)[0]
        nu = np.bincount(key, weights=up, minlength=n_cls * K)[keep]
        qd = None if quant is None else np.bincount(key, weights=quant, minlength=n_cls * K)[keep]
        return keep // K, ((keep % K) + off) / grain, nu, nt[keep].astype(np.float64), qd
    return cls, x, up, None, quant


def check(inst, s0, M, beta, pos, flags=None, temp_x=1.0, hypotheses=None, quant=None, power=True):
    """Calibrate recorded sweeps against the heat-bath law under one or more hypotheses, in one pass over the trace.

    inst      Instance(J, h)
    s0        [R, n] states before the first recorded sweep;  M [R, S, n] the state after every sweep
    beta      [R, S] the inverse temperature chain r ran at in sweep t
    pos       callable t -> order positions of sweep t ([n] shared or [R, n] per chain; order_positions)
    flags     optional [R, n] phase flags (0 normal, 1 scaled: beta / temp_x, 2 / 3 frozen: never change, no samples)
    quant     optional [n] quantisation_bound (per unit of beta) of the "f32" mode
    hypotheses  {name: dict(reading="sequential" | "jacobi" | "reversed", beta=[R, S] override, scale=float,
                 scaled_rows_at_full_beta=bool)};  default {"true": {}}
    power     also evaluate "beta(1+d*)": every temperature scaled by 1 + delta*, delta* = 2 t / sqrt(I) of the hypothesis
              named "true" (which must then be given)
    Returns {name: Tally.result()}."""
    hypotheses = {"true": {}} if hypotheses is None else dict(hypotheses)
    s0 = np.asarray(s0, dtype=np.int8)
    M = np.asarray(M, dtype=np.int8)
    R, S, n = M.shape
    beta = np.asarray(beta, dtype=np.float64).reshape(R, S)
    # everything per update is laid out [n, R] (spin-major), the layout of the sparse products
    flT = np.zeros((n, R), np.uint8) if flags is None else np.ascontiguousarray(np.asarray(flags, dtype=np.uint8).reshape(R, n).T)
    sample = flT < 2
    every = bool(sample.all())
    pick = (lambda a: a.ravel()) if every else (lambda a: a[sample])          # noqa: E731
    cls = pick(2 * np.arange(R)[None, :] + (flT == 1))
    qk = None if quant is None else pick(np.repeat(np.asarray(quant, dtype=np.float64)[:, None], R, axis=1))
    tallies = {name: Tally() for name in hypotheses}
    readings = {hyp.get("reading", "sequential") for hyp in hypotheses.values()} | ({"sequential"} if power else set())
    kept = []                                              # the true law's groups, for the power hypothesis
    frozen = 0
    old = np.ascontiguousarray(s0.T, dtype=np.float64)
    xj = inst.jacobi(old)
    for t in range(S):
        new = np.ascontiguousarray(M[:, t].T, dtype=np.float64)
        d = new - old
        if not every:
            frozen += int(np.count_nonzero(d[~sample]))
        p = pos(t)
        up = pick(new > 0).astype(np.float64)
        xs = {"jacobi": xj}
        for rd in readings - {"jacobi"}:
            xs[rd] = xj + inst.moved(p, d, before=(rd == "sequential"))
        for rd in sorted(readings):
            g = _group(pick(xs[rd]), up, cls, qk, 2 * R, inst.grain)
            if rd == "sequential" and power:
                kept.append((t, g))
            for name, hyp in hypotheses.items():
                if hyp.get("reading", "sequential") == rd:
                    _add(tallies[name], g, t, hyp, beta, temp_x)
        old = new
        if t + 1 < S:
            xj = inst.jacobi(old)
    for tl in tallies.values():
        tl.frozen_changed = frozen
    res = {name: tl.result() for name, tl in tallies.items()}
    if power:
        ds = res["true"]["delta_star"]
        tl = Tally()
        for t, g in kept:
            _add(tl, g, t, {"scale": 1.0 + ds}, beta, temp_x)
        tl.frozen_changed = frozen
        res["beta(1+d*)"] = tl.result()
    return res


def _add(tally, g, t, hyp, beta, temp_x):
    c, x, nu, nt, qd = g
    b = np.asarray(hyp.get("beta", beta), dtype=np.float64)[:, t] * hyp.get("scale", 1.0)
    if not hyp.get("scaled_rows_at_full_beta", False):
        b = np.stack([b, b / temp_x], axis=1).ravel()             # indexed by class = 2 chain + scaled
    else:
        b = np.repeat(b, 2)
    bb = b[c]
    tally.add(2.0 * bb * x, nu, nt, None if qd is None else bb * qd)


def swap_log_odds(dbeta_de):
    """ln(p / (1 - p)) of a replica-exchange decision p = min(1, exp(dBeta dE)): +inf where p = 1."""
    a = np.asarray(dbeta_de, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(a >= 0, np.inf, a - np.log(-np.expm1(np.minimum(a, -1e-300))))


def check_swaps(dbeta_de, accepted):
    """Calibration of swap decisions (same bins, tail pool and threshold as the sweeps, plus one pooled z)."""
    tl = Tally(score=False, pooled=True)
    lo = swap_log_odds(dbeta_de)
    tl.add(np.where(np.isinf(lo), 1e300, lo), np.asarray(accepted, dtype=np.float64))
    return tl.result()


def summary(res):
    """One line per hypothesis (for the test log)."""
    out = []
    for name, r in res.items():
        out.append(f"{name}: n={r['n']} k={r['k']} t={r['t']:.2f} delta*={r['delta_star']:.4g} max|z|={r['max_z']:.2f} "
                   f"z_beta={r['z_beta'] if r['z_beta'] is None else round(r['z_beta'], 2)} tail={r['tail_n']}/{r['tail_max']} "
                   f"ok={r['ok']}")
    return "\n".join(out)
