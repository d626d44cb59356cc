"""Instances whose couplings span forty orders of magnitude, and exact references for what the engine derives from them.

Every other GPU test instance has couplings of order one, so the fixed-point machinery of the "f32" throughput mode runs at one
operating point (qs 0 or 22, escale 51).  family() scales one Gaussian instance from 1e-20 to 3e15 and adds the shapes that take
the remaining branches of the scale rule (csrc/nlmc_instance.h; restated in oracle/nlo.c:nlo_field_scale): a hub row and |h| >> |J| (the
int32 row-sum limit decides), dyadic instances (the common power of two is dropped), couplings that all quantise to 0, fields only.

The references are plain Python: int and fractions.Fraction, no floating point except math.frexp for an exponent.
  scale_rule        (qs, escale) from the rule as include/nlmc.h and the comment in csrc/nlmc_instance.h state it -- not the code's loops
  quantise          Jq, hq = rint(J 2^qs), rint(h 2^qs) as Python ints
  exact_efix_f32    energy of the quantised model in units of 2^-escale, an int
  exact_energy      energy of the real (J, h), a Fraction
A second, separate group (DENSE, dense_member): complete graphs whose rows sit within 1 % of the int32 row-sum limit, for the
short-chain routes that keep a whole chain's local fields resident; aligned_state puts one local field at that limit; the dense_*
functions restate quantise, the scale rule and exact_efix_f32 in numpy int64 (exact at these sizes, and fast at 10^6 entries).
No GPU, no test in here (test_scale_rule_cpu.py, test_gpu_magnitude.py, test_magnitude_short_cpu.py, test_gpu_magnitude_short.py)."""
import functools
import math
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

from helpers import make_instance

# (qs, escale) per member: what oracle.field_scale returned when the family was written.  A change is a finding, not a number to
# update (tests/test_scale_rule_cpu.py compares the oracle and scale_rule with these, tests/test_instance_prep_cpu.py the shipped
# rule of csrc/nlmc_instance.h, tests/test_gpu_magnitude.py nlmc_create on the GPU).
PINNED = {
    "x1": (22, 51), "x1e9": (-7, 21), "x2p40": (-18, 11), "x3e15": (-29, 0), "x1e-9": (52, 52), "x2m30": (52, 52),
    "x1e-20": (52, 52), "pmJ_2p7": (-7, 22), "pmJ_2m10_h": (13, 42), "wide": (23, 52), "hub": (19, 48), "bigh": (21, 43),
    "honly": (8, 37),
}
NAMES = tuple(PINNED)
DYADIC = ("pmJ_2p7", "pmJ_2m10_h")        # every J and h an exact multiple of 2^-qs with a small field range
SIZES = {"hub": 3000, "honly": 50}        # every other member: 300 unless asked otherwise


def _sym(U):
    J = (U + U.T).tocsr()
    J.sort_indices()
    return J


@functools.lru_cache(maxsize=None)
def member(name, n=None):
    """(J csr, h, beta_unit) of one member; n: another size where the construction has one (the star and the field-only member
    keep theirs).  beta_unit = 0.8 / max|J| (max|h| without couplings): chains move at it.  Treat the result as read-only."""
    n = SIZES.get(name, 300) if n is None else int(n)
    if name in ("hub", "honly") and n != SIZES[name]:
        raise ValueError(f"{name} has one size")
    GJ, Gh = make_instance(n, seed=1, with_h=True, gaussian=True) if name not in ("hub", "honly") else (None, None)
    scaled = {"x1": 1.0, "x1e9": 1e9, "x2p40": 2.0 ** 40, "x3e15": 3e15, "x1e-9": 1e-9, "x2m30": 2.0 ** -30, "x1e-20": 1e-20}
    if name in scaled:
        J, h = (GJ * scaled[name]).tocsr(), Gh * scaled[name]
    elif name == "pmJ_2p7":
        J, h = (make_instance(n, seed=2)[0] * 128.0).tocsr(), np.zeros(n)
    elif name == "pmJ_2m10_h":
        J, h = (make_instance(n, seed=2)[0] * 2.0 ** -10).tocsr(), np.rint(8.0 * Gh) / 8.0 * 2.0 ** -10
    elif name == "wide":
        U = sp.triu(GJ, 1).tocsr()
        U.sort_indices()
        keep = np.arange(U.nnz) % 7 == 0            # every 7th stored value keeps its size, the others are a million times smaller
        U.data = np.where(keep, U.data, U.data * 1e-6)
        J, h = _sym(U), Gh * 1e-6
    elif name == "hub":
        j = np.arange(1, n)
        w = 1.0 - 1e-3 * (j % 5)
        J = _sym(sp.coo_matrix((w, (np.zeros(n - 1, dtype=np.int64), j)), shape=(n, n)).tocsr())
        h = np.zeros(n)
    elif name == "bigh":
        J, h = (GJ * 1e-3).tocsr(), Gh * 1e3
    elif name == "honly":
        J, h = sp.csr_matrix((n, n)), np.linspace(-3e4, 3e4, n)
    else:
        raise KeyError(name)
    J.sort_indices()
    ref = float(np.max(np.abs(J.data))) if J.nnz else float(np.max(np.abs(h)))
    h = np.ascontiguousarray(h, dtype=np.float64)
    h.setflags(write=False)
    return J, h, 0.8 / ref


def family():
    """(name, J, h, beta_unit) of every member at its own size."""
    for name in NAMES:
        yield (name,) + member(name)


# ---- dense members: local fields at the int32 limit ---------------------------------------------------------------------------------
# Complete graphs with near-uniform, non-dyadic weights: the int32 row-sum limit decides qs (or leaves its cap just standing) and the
# common power of two drops nothing, so sum|Jq| + |hq| of EVERY row is within 1 % of 2^31.  A group of its own, not in NAMES / PINNED:
# those parametrise GPU tests at n = 300 and are walked with Fraction arithmetic, too slow at 10^6 entries -- the dense members have
# the numpy int64 restatements below (exact: |Jq| < 2^23, n <= 1024, so every sum stays far below 2^63).
# name -> (n, with a field, (qs, escale) as oracle.field_scale returned them when the group was written, beta_unit)
DENSE_SPEC = {
    "flat513": (513, False, (22, 43), 0.05),         # the first n past k_sweep_waves_long's n <= 512 register compare
    "flat1024": (1024, False, (21, 41), 0.05),
    "flat256h": (256, True, (22, 43), 0.8 / 254),    # n <= 256: J alone cannot reach the row-sum limit, the field supplies the rest
}
DENSE = tuple(DENSE_SPEC)
DENSE_PINNED = {k: v[2] for k, v in DENSE_SPEC.items()}


@functools.lru_cache(maxsize=None)
def flat(n, with_h=False):
    """(J csr, h) of the flat construction on n spins: the complete graph with J_ij = sign_ij (1 - 1e-3 ((i + j) % 5)), signs from
    default_rng(3); h = 0 or 254 (+1, -1, ..)_k (1 - 1e-3 (k % 3)).  Treat the result as read-only."""
    n = int(n)
    i, j = np.triu_indices(n, 1)
    U = np.zeros((n, n))
    U[i, j] = np.random.default_rng(3).choice([-1, 1], size=len(i)) * (1.0 - 1e-3 * ((i + j) % 5))
    J = sp.csr_matrix(U + U.T)
    J.sort_indices()
    k = np.arange(n)
    h = 254.0 * np.where(k % 2 == 0, 1.0, -1.0) * (1.0 - 1e-3 * (k % 3)) if with_h else np.zeros(n)
    h = np.ascontiguousarray(h, dtype=np.float64)
    h.setflags(write=False)
    return J, h


def dense_member(name):
    """(J csr, h, beta_unit) of a dense member.  beta_unit: 0.05 without a field (the inverse temperature of a dense instance's
    scale, fields of order sqrt(n)), 0.8 / 254 with one: test inputs at which the chains move (the tests assert that they do)."""
    n, with_h, _, beta = DENSE_SPEC[name]
    return flat(n, with_h) + (beta,)


def aligned_state(J, h, k=0, opposed=False):
    """The +-1 configuration in which the local field of spin k, h_k + sum_j J_kj s_j, is the whole row sum |h_k| + sum_j |J_kj| in
    size: s_j = sign(J_kj) for j != k (+1 where there is no coupling), all reversed where h_k < 0; s_k = sign(h_k), +1 where h_k = 0.
    There spin k sits in its field and stays.  opposed: s_k reversed -- the field is the same (it does not depend on s_k), the spin
    stands against it and flips at its first visit at any temperature at which 2 beta |X_k| is large: an energy delta of
    2 |X_k| 2^eshift with |X_k| at the limit."""
    row = np.asarray(sp.csr_matrix(J)[k].todense()).reshape(-1)
    hk = float(np.asarray(h).reshape(-1)[k])
    sk = -1 if hk < 0 else 1
    s = np.where(row < 0, -sk, sk).astype(np.int8)
    s[k] = -sk if opposed else sk
    return s


def dense_quantise(J, h, qs):
    """(Jq [n, n] int64, hq [n] int64) = rint(J 2^qs), rint(h 2^qs), ties to even: the scaling by a power of two is exact in fp64."""
    Jd = np.asarray(sp.csr_matrix(J).todense(), dtype=np.float64)
    return (np.rint(np.ldexp(Jd, qs)).astype(np.int64),
            np.rint(np.ldexp(np.asarray(h, dtype=np.float64).reshape(-1), qs)).astype(np.int64))


def dense_row_sums(J, h, qs):
    """sum_j |Jq_kj| + |hq_k| of every row, int64."""
    Jq, hq = dense_quantise(J, h, qs)
    return np.abs(Jq).sum(axis=1) + np.abs(hq)


def _abs_sum(x):
    """sum|x| of fp64 values as a Fraction (exact: every distinct value once, times its count)."""
    v, cnt = np.unique(np.abs(np.asarray(x, dtype=np.float64)).reshape(-1), return_counts=True)
    return sum((Fraction(float(a)) * int(c) for a, c in zip(v, cnt)), Fraction(0))


def dense_scale_rule(J, h):
    """scale_rule in numpy int64 for matrices whose quantised rows stay inside int64 (the same statement, not the code's loops)."""
    Jd = np.asarray(sp.csr_matrix(J).todense(), dtype=np.float64)
    hv = np.asarray(h, dtype=np.float64).reshape(-1)
    B = _abs_sum(Jd) / 2 + _abs_sum(hv)
    ex = int(max(B, Fraction(1)).__floor__()).bit_length()
    escale0 = max(0, min(52, 60 - ex))
    maxj = float(np.max(np.abs(Jd))) if Jd.size else 0.0
    ref = maxj if maxj > 0 else float(np.max(np.abs(hv), initial=0.0))
    if ref == 0:
        return 0, min(escale0, 29)
    top = min(23 - math.frexp(ref)[1], escale0)

    def fits(q):
        if max(np.max(np.abs(np.ldexp(Jd, q))), np.max(np.abs(np.ldexp(hv, q)))) >= 2.0 ** 50:       # (far outside, and int64 stays exact)
            return False
        Jq, hq = dense_quantise(Jd, hv, q)
        return bool(np.max(np.abs(Jq)) <= (1 << 23) - 1 and np.max(np.abs(Jq).sum(axis=1) + np.abs(hq)) <= (1 << 31) - 1)

    lo, hi = top - 128, top
    assert fits(lo)
    if not fits(hi):
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if fits(mid) else (lo, mid)
        hi = lo
    qs = hi
    Jq, hq = dense_quantise(Jd, hv, qs)
    common = int(np.bitwise_or.reduce(np.abs(Jq).reshape(-1))) | int(np.bitwise_or.reduce(np.abs(hq)))
    if common:
        qs -= (common & -common).bit_length() - 1
    return qs, min(escale0, qs + 29)


def dense_exact_efix_f32(J, h, s, qs, escale):
    """exact_efix_f32 in numpy int64 (|pair sum| <= n 2^31 < 2^42), returned as a Python int."""
    Jq, hq = dense_quantise(J, h, qs)
    np.fill_diagonal(Jq, 0)
    s = np.asarray(s).reshape(-1).astype(np.int64)
    pair = int(s @ (Jq @ s))
    assert pair % 2 == 0, "J is not symmetric after quantisation"
    assert escale >= qs
    return -(pair // 2 + int(hq @ s)) * (1 << (escale - qs))


# ---- exact references ------------------------------------------------------------------------------------------------------------

def _parts(J, h):
    """Rows of J as lists of (column, Fraction) without explicit zeros, h as Fractions."""
    A = sp.csr_matrix(J).copy()
    A.eliminate_zeros()
    A.sort_indices()
    n = A.shape[0]
    rows = [[(int(A.indices[e]), Fraction(float(A.data[e]))) for e in range(A.indptr[k], A.indptr[k + 1])] for k in range(n)]
    return rows, [Fraction(float(x)) for x in np.asarray(h, dtype=np.float64).reshape(-1)]


def _rint(x):
    """Nearest integer of a Fraction, ties to even (the default rounding of llrint)."""
    return int(round(x))


def _scaled(x, q):
    return x * (1 << q) if q >= 0 else x / (1 << -q)


def quantise(J, h, qs):
    """(rows of (column, Jq), hq) with Jq = rint(J 2^qs), hq = rint(h 2^qs) as Python ints."""
    rows, hf = _parts(J, h)
    return [[(c, _rint(_scaled(v, qs))) for c, v in row] for row in rows], [_rint(_scaled(v, qs)) for v in hf]


def scale_rule(J, h):
    """(qs, escale) as the interface states them (include/nlmc.h: nlmc_field_scale, nlmc_energy_scale; the comment on the
    fixed-point scales in csrc/nlmc_instance.h):
      energies are integers in units of 2^-escale with |E| <= B = sum|J|/2 + sum|h|:  escale0 = 60 - ex clamped to [0, 52], where
      2^ex is the first power of two above max(B, 1);
      qs is the largest exponent, at most escale0 and at most 23 - (exponent of the largest |J|; of the largest |h| where there
      is no coupling), such that every |Jq| <= 2^23 - 1 and every row sum  sum|Jq| + |hq| <= 2^31 - 1;
      then lowered by the number of trailing zero bits common to every non-zero Jq and hq;
      escale = min(escale0, qs + 29)."""
    rows, hf = _parts(J, h)
    B = sum((abs(v) for row in rows for _, v in row), Fraction(0)) / 2 + sum((abs(v) for v in hf), Fraction(0))
    ex = int(max(B, Fraction(1)).__floor__()).bit_length()        # 2^(ex-1) <= floor(B) <= B < floor(B) + 1 <= 2^ex
    escale0 = max(0, min(52, 60 - ex))
    maxj = max((abs(v) for row in rows for _, v in row), default=Fraction(0))
    ref = maxj if maxj > 0 else max((abs(v) for v in hf), default=Fraction(0))
    if ref == 0:
        return 0, min(escale0, 29)
    top = min(23 - math.frexp(float(ref))[1], escale0)             # ref is a double: the conversion is exact

    def fits(q):
        for row, hk in zip(rows, hf):
            jq = [abs(_rint(_scaled(v, q))) for _, v in row]
            if any(x > (1 << 23) - 1 for x in jq) or sum(jq) + abs(_rint(_scaled(hk, q))) > (1 << 31) - 1:
                return False
        return True

    lo, hi = top - 128, top                  # fits() is monotone in q (every |value 2^q| shrinks with q) and holds at lo: bisect
    assert fits(lo)
    if not fits(hi):
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if fits(mid) else (lo, mid)
        hi = lo
    qs = hi
    ints = [abs(_rint(_scaled(v, qs))) for row in rows for _, v in row] + [abs(_rint(_scaled(v, qs))) for v in hf]
    common = 0
    for x in ints:
        common |= x
    if common:
        qs -= (common & -common).bit_length() - 1
    return qs, min(escale0, qs + 29)


def exact_efix_f32(J, h, s, qs, escale):
    """-(1/2 sum_{k != c} Jq_kc s_k s_c + sum_k hq_k s_k) 2^(escale - qs), the energy of the quantised model in units of
    2^-escale, as a Python int.  The diagonal is left out (it is a constant of the +-1 states and the kernels' deltas skip it);
    s may hold zeros."""
    rows, hq = quantise(J, h, qs)
    s = [int(x) for x in np.asarray(s).reshape(-1)]
    pair = sum(q * s[k] * s[c] for k, row in enumerate(rows) for c, q in row if c != k)
    assert pair % 2 == 0, "J is not symmetric after quantisation"
    assert escale >= qs
    return -(pair // 2 + sum(q * x for q, x in zip(hq, s))) * (1 << (escale - qs))


def exact_energy(J, h, s):
    """E = -(s^T J s / 2 + s^T h) of the real (J, h) as a Fraction (what nlmc_energy computes in fp64, diagonal included)."""
    rows, hf = _parts(J, h)
    s = [int(x) for x in np.asarray(s).reshape(-1)]
    pair = sum((v * (s[k] * s[c]) for k, row in enumerate(rows) for c, v in row), Fraction(0))
    return -(pair / 2 + sum((v * x for v, x in zip(hf, s)), Fraction(0)))


def abs_terms(J, h):
    """sum|J|/2 + sum|h| as a Fraction: the size every rounding bound of an energy is relative to."""
    rows, hf = _parts(J, h)
    return sum((abs(v) for row in rows for _, v in row), Fraction(0)) / 2 + sum((abs(v) for v in hf), Fraction(0))


def energy_bound(J, h):
    """Bound on |fp64 energy - exact energy| for any order of summation: m 2^-53 (sum|J|/2 + sum|h|) with m = nnz + n terms
    (each of the m products is exact -- s is 0 or +-1 --, a sum of m terms in any association is within (m - 1) u sum|terms| to
    first order, u = 2^-53; the halving is exact)."""
    A = sp.csr_matrix(J)
    return (A.nnz + A.shape[0]) * abs_terms(J, h) / (1 << 53)


def row_stats(J, h):
    """(deg_max, rowabs_max): the longest row and the largest sum|J_row| + |h| (a Fraction)."""
    rows, hf = _parts(J, h)
    return max(len(r) for r in rows), max(sum((abs(v) for _, v in r), Fraction(0)) + abs(hk) for r, hk in zip(rows, hf))


def f64_trace_bound(J, h, flips, escale):
    """Bound on |fp64 trace - exact energy 2^escale| after `flips` spin flips from a start of round(exact 2^escale): the start's
    rounding, then per flip the llrint (1/2) and the fp64 row sum of up to deg_max + 1 terms, doubled by (s' - s) = +-2."""
    deg, rowabs = row_stats(J, h)
    return Fraction(1, 2) + flips * (Fraction(1, 2) + 2 * (deg + 1) * rowabs * (1 << escale) / (1 << 53))


def cancelling_state(J, h, rel=Fraction(1, 10 ** 6), seed=0):
    """A +-1 configuration whose exact energy is below rel * (sum|J|/2 + sum|h|) in size: from a random start, flip the spin that
    brings |E| closest to 0; where no flip helps, flip a random spin and go on (an energy of that size is all cancellation)."""
    rows, hf = _parts(J, h)
    n = len(hf)
    den = max([v.denominator for row in rows for _, v in row] + [v.denominator for v in hf])     # powers of two: the largest is common
    ri = [[(c, int(v * den)) for c, v in row if c != k] for k, row in enumerate(rows)]
    hi = [int(v * den) for v in hf]
    rng = np.random.default_rng(seed)
    s = [int(x) for x in np.where(rng.random(n) < 0.5, -1, 1)]
    target = rel * abs_terms(J, h) * den
    E = int(exact_energy(J, h, s) * den)
    for _ in range(50 * n):
        if abs(E) < target:
            break
        d = [2 * s[k] * (sum(v * s[c] for c, v in ri[k]) + hi[k]) for k in range(n)]       # what flipping k adds to E
        k = min(range(n), key=lambda i: abs(E + d[i]))
        if abs(E + d[k]) >= abs(E):
            k = int(rng.integers(n))
        s[k] = -s[k]
        E += d[k]
    assert abs(E) < target and Fraction(E, den) == exact_energy(J, h, s)
    return np.array(s, dtype=np.int8)
