"""The instance preparation that ships (csrc/nlmc_instance.h: nlmc_instance_prepare, what nlmc_create runs before it asks for a
device) through the host program scripts/instance_prep_check.cpp: scales, quantisation, format facts and refusals against exact
restatements (Python int / Fraction) over the magnitude family of scalefamily.py, the smallest shapes that take each remaining
branch, and malformed inputs.  No GPU.  The program is built plainly here; NLMC_KEEP_INSTANCE_INPUTS=dir keeps the input files for
the run under the sanitizers that the program's header describes."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
import scalefamily as sf

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -3
MAX_N = 16777216
FZ_W = 8


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """Path of the built program, and the directory the cases' input files go to."""
    out = tmp_path_factory.mktemp("instance_prep")
    exe = str(out / "instance_prep_check")
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    tried = []
    for cxx in ("g++", "clang++", rocm_clang):
        if not (shutil.which(cxx) or os.path.exists(cxx)):
            tried.append(f"{cxx}: not found")
            continue
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", os.path.join(REPO, "scripts", "instance_prep_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
        if r.returncode == 0:
            break
        tried.append(f"{cxx}: {r.stderr[-2000:]}")
    else:
        pytest.fail("no host compiler built scripts/instance_prep_check.cpp:\n" + "\n".join(tried))
    keep = os.environ.get("NLMC_KEEP_INSTANCE_INPUTS")
    if keep:
        os.makedirs(keep, exist_ok=True)
    return exe, keep or str(out)


def run(program, name, n, rowptr, colidx, vals, h, nnz=None, chains=(1, 0, 1), null=()):
    """Writes the case `name` and runs the program on it -> {key: int | [int] | str}.  nnz: what the call claims (default: the
    length of vals); null: names among out, rowptr, colidx, vals, h that are handed over as NULL."""
    exe, where = program
    rowptr, colidx = np.asarray(rowptr, dtype=np.int32), np.asarray(colidx, dtype=np.int32)
    vals, h = np.asarray(vals, dtype=np.float64), np.asarray(h, dtype=np.float64)
    mask = sum(1 << ("out", "rowptr", "colidx", "vals", "h").index(x) for x in null)
    head = np.array([mask, n, len(vals) if nnz is None else nnz, *chains, len(rowptr), len(colidx), len(vals), len(h)], dtype=np.int64)
    path = os.path.join(where, name + ".bin")
    with open(path, "wb") as f:
        for a in (head, rowptr, colidx, vals, h):
            f.write(a.tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        key, _, rest = line.partition(" ")
        out[key] = rest if key == "err" else [int(x) for x in rest.split()] if key in ("col", "Jq", "hq") else int(rest)
    return out


def expected(n, rowptr, colidx, vals, h):
    """Every fact of a well-formed instance, restated: the scales by scalefamily.scale_rule, the rest in ints and Fractions."""
    rowptr, colidx = [int(x) for x in rowptr], [int(x) for x in colidx]
    vf, hf = [Fraction(float(v)) for v in vals], [Fraction(float(v)) for v in h]
    J = sp.csr_matrix((np.asarray(vals, dtype=np.float64), np.asarray(colidx, dtype=np.int32), np.asarray(rowptr, dtype=np.int32)), shape=(n, n))
    qs, escale = sf.scale_rule(J, np.asarray(h, dtype=np.float64))
    Jq, hq = [sf._rint(sf._scaled(v, qs)) for v in vf], [sf._rint(sf._scaled(v, qs)) for v in hf]
    deg = [rowptr[k + 1] - rowptr[k] for k in range(n)]
    rows = [range(rowptr[k], rowptr[k + 1]) for k in range(n)]
    return {
        "rc": 0, "err": "", "qs": qs, "escale": escale, "col": colidx, "Jq": Jq, "hq": hq,
        "has_diag": int(any(colidx[e] == k and vf[e] != 0 for k in range(n) for e in rows[k])),
        "has_zero_vals": int(any(v == 0 for v in vf)),
        "max_deg": max(deg), "n_gt1": sum(d > FZ_W for d in deg), "n_gt2": sum(d > 2 * FZ_W for d in deg),
        "fits16": int(n <= 65535 and all(-32768 <= q <= 32767 for q in Jq)),
        "pm1": int(all(abs(q) == 1 for q in Jq)),
        "exact_q": int(all(sf._scaled(v, qs) == q for v, q in zip(vf, Jq))),
        "exact_h": int(all(sf._scaled(v, qs) == q for v, q in zip(hf, hq))),
        "xmax": max(sum(abs(Jq[e]) for e in rows[k]) + abs(hq[k]) for k in range(n)),
    }


# ---- the magnitude family ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sf.NAMES)
def test_family_scales_quantisation_and_flags(program, name):
    J, h, _ = sf.member(name)
    n = J.shape[0]
    assert n == sf.SIZES.get(name, 300)
    got = run(program, "family_" + name, n, J.indptr, J.indices, J.data, h)
    assert got["rc"] == 0 and got["err"] == ""
    # scales: the shipped rule == the pinned pair == the oracle == the stated rule
    pair = (got["qs"], got["escale"])
    assert pair == sf.PINNED[name] == oracle.field_scale(oracle.Csr(J), h) == sf.scale_rule(J, h)
    # quantisation, entry for entry
    rows, hq = sf.quantise(J, h, pair[0])
    assert sum(len(r) for r in rows) == J.nnz                      # (no member stores a zero: quantise() would drop it)
    assert got["col"] == [c for r in rows for c, _ in r] and got["Jq"] == [q for r in rows for _, q in r] and got["hq"] == hq
    assert got["xmax"] == max(sum(abs(q) for _, q in r) + abs(x) for r, x in zip(rows, hq))
    # every fact, format flags included, against the restatement above
    assert got == expected(n, J.indptr, J.indices, J.data, h)
    if name == "pmJ_2p7":
        assert (got["pm1"], got["exact_q"], got["exact_h"], got["fits16"]) == (1, 1, 1, 1)
    if name == "x1":
        assert (got["pm1"], got["exact_q"], got["exact_h"]) == (0, 0, 0)


# ---- the smallest shapes that take each remaining branch ----------------------------------------------------------------------------

def pair_graph(v, h=(0.0, 0.0)):
    """Two spins coupled by v."""
    return 2, [0, 1, 2], [1, 0], [v, v], list(h)


def long_rows():
    """Rows of 8, 9, 16 and 17 entries of +-1 (then empty rows): the two long-row counts of the fused plans."""
    deg = [8, 9, 16, 17, 0, 0]
    n = 18
    rowptr = np.concatenate([[0], np.cumsum(deg + [0] * (n - len(deg)))])
    colidx = np.concatenate([np.arange(n - d, n) for d in deg])
    return n, rowptr, colidx, np.where(np.arange(len(colidx)) % 3 == 0, -1.0, 1.0), np.zeros(n)


SHAPES = {
    "one_spin_nothing": (1, [0, 0], [], [], [0.0]),
    "one_spin_diagonal": (1, [0, 1], [0], [1.5], [0.0]),
    "stored_zero": (2, [0, 2, 3], [0, 1, 0], [0.0, 1.0, 1.0], [0.0, 0.0]),                  # the zero sits on the diagonal: no has_diag
    "empty_65535": (65535, np.zeros(65536), [], [], np.zeros(65535)),
    "empty_65536": (65536, np.zeros(65537), [], [], np.zeros(65536)),
    "jq_32767": pair_graph(32767.0, (1.0, 0.0)),
    "jq_32768": pair_graph(32768.0, (1.0, 0.0)),
    "jq_m32768": pair_graph(-32768.0, (1.0, 0.0)),
    "long_rows": long_rows(),
    # 4 and 4 (1 + 2^-40): at the fitted scale (qs = 20) the second is no integer, so the one-pass scan stands down; both round to
    # 2^22, and the per-bit loop lowers qs by 22
    "per_bit_loop": pair_graph(4.0)[:3] + ([4.0, 4.0 * (1 + 2.0 ** -40)], [0.0, 0.0]),
}
FACTS = {      # what each shape is there for (the rest is compared with expected() like every other fact)
    "one_spin_nothing": {"qs": 0, "escale": 29, "has_diag": 0, "has_zero_vals": 0, "max_deg": 0, "xmax": 0},
    "one_spin_diagonal": {"has_diag": 1},
    "stored_zero": {"has_zero_vals": 1, "has_diag": 0},
    "empty_65535": {"fits16": 1},
    "empty_65536": {"fits16": 0},
    "jq_32767": {"fits16": 1, "qs": 0, "Jq": [32767, 32767]},
    "jq_32768": {"fits16": 0, "qs": 0, "Jq": [32768, 32768]},
    "jq_m32768": {"fits16": 1, "qs": 0, "Jq": [-32768, -32768]},
    "long_rows": {"max_deg": 17, "n_gt1": 3, "n_gt2": 1, "pm1": 1},
    "per_bit_loop": {"qs": -2, "Jq": [1, 1], "exact_q": 0, "pm1": 1},
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_smallest_shapes(program, name):
    n, rowptr, colidx, vals, h = SHAPES[name]
    got = run(program, "shape_" + name, n, rowptr, colidx, vals, h)
    assert got == expected(n, rowptr, colidx, vals, h)
    assert {k: got[k] for k in FACTS[name]} == FACTS[name]
    if name == "per_bit_loop":                  # the premise: a value that is no multiple of 2^-20, the scale the fit loop ends on
        assert any(sf._scaled(Fraction(float(v)), 20).denominator != 1 for v in vals)


# ---- malformed inputs: the codes and texts of nlmc_create -----------------------------------------------------------------------------

OK2 = dict(n=2, rowptr=[0, 1, 2], colidx=[1, 0], vals=[1.0, 1.0], h=[0.0, 0.0])
BAD_SIZES = (ERR_ARG, "nlmc_create: bad sizes or NULL arrays")
NOT_MONOTONE = (ERR_ARG, "nlmc_create: rowptr not monotone")
BAD_COLUMN = (ERR_ARG, "nlmc_create: column index out of range")
BAD_ENDS = (ERR_ARG, "nlmc_create: rowptr[0] != 0 or rowptr[n] != nnz")
MALFORMED = {
    "null_out": (dict(OK2, null=("out",)), (ERR_ARG, "nlmc_create: out is NULL")),
    "null_out_comes_first": (dict(OK2, n=0, null=("out", "rowptr")), (ERR_ARG, "nlmc_create: out is NULL")),
    "null_rowptr": (dict(OK2, null=("rowptr",)), BAD_SIZES),
    "null_colidx": (dict(OK2, null=("colidx",)), BAD_SIZES),
    "null_vals": (dict(OK2, null=("vals",)), BAD_SIZES),
    "null_h": (dict(OK2, null=("h",)), BAD_SIZES),
    "n_zero": (dict(OK2, n=0), BAD_SIZES),
    "nnz_negative": (dict(OK2, nnz=-1), BAD_SIZES),
    "chains_negative": (dict(OK2, chains=(-1, 0, 1)), BAD_SIZES),
    "chain_base_negative": (dict(OK2, chains=(1, -1, 1)), BAD_SIZES),
    "chains_beyond_global": (dict(OK2, chains=(2, 3, 4)), BAD_SIZES),
    "n_above_max": (dict(OK2, n=MAX_N + 1), (ERR_UNSUPPORTED, "nlmc_create: n exceeds NLMC_MAX_N")),
    "rowptr_first_not_zero": (dict(OK2, rowptr=[1, 1, 2]), BAD_ENDS),
    "rowptr_last_not_nnz": (dict(OK2, rowptr=[0, 1, 1]), BAD_ENDS),
    "rowptr_decreasing": (dict(n=3, rowptr=[0, 2, 1, 2], colidx=[1, 2], vals=[1.0, 1.0], h=[0.0] * 3), NOT_MONOTONE),
    # passes the check of the two ends; row 0 would run over entries 2..4 of two-entry arrays
    "rowptr_beyond_nnz": (dict(OK2, rowptr=[0, 5, 2]), NOT_MONOTONE),
    "column_negative": (dict(OK2, colidx=[-1, 0]), BAD_COLUMN),
    "column_n": (dict(OK2, colidx=[1, 2]), BAD_COLUMN),
}


@pytest.mark.parametrize("name", list(MALFORMED))
def test_malformed_inputs(program, name):
    kw, (code, text) = MALFORMED[name]
    got = run(program, "malformed_" + name, **kw)
    assert got == {"rc": code, "err": text}


def test_null_arrays_of_an_instance_without_entries_are_taken(program):
    got = run(program, "shape_no_entries_null_arrays", 2, [0, 0, 0], [], [], [1.0, -1.0], null=("colidx", "vals"))
    assert got == expected(2, [0, 0, 0], [], [], [1.0, -1.0])
