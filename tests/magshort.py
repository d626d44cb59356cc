"""The cases of tests/test_gpu_magnitude_short.py: which member of the coupling-magnitude family (tests/scalefamily.py) runs on which
short-chain route, at which size, from which start states.  Kept apart from the GPU file so that tests/test_magnitude_short_cpu.py
can check, from the oracle's scales alone and without a GPU, that the case set covers what it is there for (a negative field scale,
both ends of escale - qs and a value between them on every group of routes, a local field within 1 % of the int32 limit on every
dense route) -- the GPU file cannot go vacuous unnoticed.  No test in here."""
import functools

import numpy as np

import oracle
import scalefamily as sf
import wavefields
from helpers import init_spins

SEED = 0x5CA1E000 + (9 << 32)            # of the sweep and rounds cases; high bits set
ROWS = 5                                 # chains of a sweep or NMC case
ALIGNED = 2                              # on a dense member this chain starts from sf.aligned_state: |X_0| is the whole row sum
OPPOSED = 3                              # ... and this one from the same state with spin 0 reversed: it flips with |X_0| at the limit
LADDER, LADDERS = 4, 2                   # rounds: two ladders of four
# what |X_0| is at least when spin 0 of chain OPPOSED flips (field_at_first_visit): above 2^30, where twice the field leaves int32
FLIP_FLOOR = {"flat513": 1 << 30, "flat1024": 1 << 30, "flat256h": 1 << 30, "flat192h": 0.6 * (1 << 31)}
FLAT192H = "flat192h"                    # the flat construction cut to 192 spins, flat256h's field rule: the last matrix staged in LDS


def is_dense(name):
    return name in sf.DENSE or name == FLAT192H


@functools.lru_cache(maxsize=None)
def instance(name, n=None):
    """(J, h, beta_unit, oracle.Csr, (qs, escale) of the oracle) -- read-only, computed once per (member, size)."""
    if name == FLAT192H:
        J, h, beta = sf.flat(192, True) + (0.8 / 254,)
    elif name in sf.DENSE:
        J, h, beta = sf.dense_member(name)
    else:
        J, h, beta = sf.member(name, n)
    csr = oracle.Csr(J)
    return J, h, beta, csr, oracle.field_scale(csr, h)


def start_spins(name, n, rows):
    """init_spins; on a dense member chain ALIGNED (the third rung of the first ladder, in rounds) starts from the aligned state and
    chain OPPOSED from the aligned state with spin 0 reversed."""
    J, h, _, csr, _ = instance(name, n)
    m0 = init_spins(rows, csr.n).copy()
    if is_dense(name):
        m0[ALIGNED] = sf.aligned_state(J, h)
        m0[OPPOSED] = sf.aligned_state(J, h, opposed=True)
    return m0


def field_at_first_visit(name, n, m0_row, after_first_sweep, seed=SEED, sweep0=0):
    """X_0 of a chain of a dense member at spin 0's visit in its first sweep (shared visiting order), exactly: every spin is
    visited once, so the spins that moved before the visit are those ahead of spin 0 in the order that the sweep changed."""
    J, h, _, csr, (qs, _) = instance(name, n)
    Jq, hq = sf.dense_quantise(J, h, qs)
    order = wavefields.visiting_order(csr.n, sweep0, 0, seed)
    s = np.asarray(m0_row, dtype=np.int64).copy()
    ahead = np.array(order[:order.index(0)], dtype=np.int64)
    s[ahead] = np.asarray(after_first_sweep, dtype=np.int64)[ahead]
    return abs(int(hq[0] + Jq[0] @ s))


def exact_efix(name, n, s):
    """Energy of the quantised model in units of 2^-escale, a Python int (numpy int64 on dense members, Fractions otherwise)."""
    J, h, _, _, (qs, escale) = instance(name, n)
    return (sf.dense_exact_efix_f32 if is_dense(name) else sf.exact_efix_f32)(J, h, s, qs, escale)


def start_fields(name, n, rows):
    """X_k = hq_k + sum_j Jq_kj s_j of every (chain, spin) of the start states, int64 [rows, n] (diagonal included, as the kernels'
    field build has it)."""
    J, h, _, csr, (qs, _) = instance(name, n)
    m0 = start_spins(name, n, rows).astype(np.int64)
    if is_dense(name):
        Jq, hq = sf.dense_quantise(J, h, qs)
    else:
        rows_q, hq = sf.quantise(J, h, qs)
        Jq = np.zeros((csr.n, csr.n), dtype=np.int64)
        for k, row in enumerate(rows_q):
            for c, q in row:
                Jq[k, c] += q
        hq = np.array(hq, dtype=np.int64)
    return m0 @ Jq.T + hq[None, :]


# ---- the cases: (member, n or None for the member's own size, precision) -------------------------------------------------------------
SPARSE_48 = ("x3e15", "x1e9", "x1e-9", "x1e-20", "bigh", "wide", "pmJ_2p7")
LANE_SWEEPS = ([(nm, 48, p) for nm in SPARSE_48 for p in ("f32", "f64")] + [("honly", 50, p) for p in ("f32", "f64")]
               + [("flat256h", None, "f32"), ("flat1024", None, "f32")])
LANE_FLAGGED = ("x1e9", 48, "f32")       # phase flags with temp_x = 20: the flagged spins' cb1 under qinv = 2^7
WAVE_SWEEPS = [(nm, 100, "f32") for nm in ("x3e15", "x1e9", "bigh", "x1e-20")] + [("honly", 50, "f32"), ("flat256h", None, "f32"),
                                                                                    (FLAT192H, None, "f32")]
# x1e-9: the issue's list for this group has no member with qs = 52; its coverage conditions ask for one
LONG_SWEEPS = [("flat513", None, "f32"), ("flat1024", None, "f32"), ("x3e15", 300, "f32"), ("bigh", 300, "f32"), ("x1e-9", 300, "f32")]
ROUNDS = ([("pt_rounds_lanes", nm, 48, p) for nm in ("x1e9", "x1e-9") for p in ("f32", "f64")]
          + [("pt_rounds_waves", "x3e15", 100, "f32"), ("pt_rounds_waves", "flat256h", None, "f32"),
             ("pt_rounds_waves_long", "flat513", None, "f32"), ("pt_rounds_waves_long", "x2p40", 300, "f32")])
NMC = [("nmc_phases_lanes", "x1e9", 48, "f32"), ("nmc_phases_lanes", "x1e-9", 48, "f32"),
       ("nmc_phases_waves", "x3e15", 100, "f32"), ("nmc_phases_waves", "flat256h", None, "f32")]

# group -> its f32 cases as (member, n, rows of the start states): what the coverage conditions are computed over
GROUPS = {
    "lane sweeps": [(nm, n, ROWS) for nm, n, p in LANE_SWEEPS + [LANE_FLAGGED] if p == "f32"],
    "wave sweeps": [(nm, n, ROWS) for nm, n, p in WAVE_SWEEPS],
    "long wave sweeps": [(nm, n, ROWS) for nm, n, p in LONG_SWEEPS],
    "rounds": [(nm, n, LADDER * LADDERS) for _, nm, n, p in ROUNDS if p == "f32"],
    "nmc": [(nm, n, ROWS) for _, nm, n, p in NMC],
}
# the groups (and, within the mixed ones, the entries) whose kernels keep the fields of a whole chain resident or feed |Jq| near 2^23
# into the 24-bit multiply: each holds a dense member whose aligned chain starts with |X_0| >= 0.99 2^31
DENSE_GROUPS = {
    "lane sweeps": LANE_SWEEPS, "wave sweeps": WAVE_SWEEPS, "long wave sweeps": LONG_SWEEPS,
    "wave rounds": [(nm, n, p) for e, nm, n, p in ROUNDS if e == "pt_rounds_waves"],
    "long wave rounds": [(nm, n, p) for e, nm, n, p in ROUNDS if e == "pt_rounds_waves_long"],
    "wave nmc": [(nm, n, p) for e, nm, n, p in NMC if e == "nmc_phases_waves"],
}


def case_id(case):
    return "-".join(str(x) for x in case if x is not None)
