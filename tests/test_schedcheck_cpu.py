"""No GPU needed: the schedule checker (tests/schedcheck.py) accepts the reference scheduler's output, packed into the read-back
layout by the small packer below, and rejects array-level mutations of it under the rule each one breaks.

The packer writes what include/nlmc.h documents for nlmc_plan_get_items / nlmc_plan_get_order; it is the only code that knows the
layout besides the checker's decoder and the kernels, and shares nothing with either."""
import copy

import numpy as np
import pytest
import scipy.sparse as sp

import schedcheck as sc
from schedcheck import FMT_ADDR, FMT_COMPACT, FMT_WIDE

SEED = 0xA5A50000


# ------------------------------------------------------------------------------------------------------------------------
# graphs
# ------------------------------------------------------------------------------------------------------------------------
def sym(n, i, j, v):
    U = sp.coo_matrix((v, (np.minimum(i, j), np.maximum(i, j))), shape=(n, n)).tocsr()
    U.sum_duplicates()
    J = (U + U.T).tocsr()
    J.sort_indices()
    return J


def mixed_graph(n=300, couplings="pmj", diag=False, seed=3):
    """Spins 0..199: random degree-6 graph with hubs of 12, 20 and 40 entries; 200..259: a perfect matching; 260..279: a path;
    280..: isolated."""
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(200), 3)
    j = rng.integers(0, 200, size=600)
    hub_i = np.concatenate([np.full(12, 5), np.full(20, 17), np.full(40, 33)])
    hub_j = np.concatenate([rng.choice(np.arange(40, 200), d, replace=False) for d in (12, 20, 40)])
    i, j = np.concatenate([i, hub_i, np.arange(200, 260, 2), np.arange(260, 279)]), np.concatenate([j, hub_j, np.arange(201, 260, 2), np.arange(261, 280)])
    keep = i != j
    i, j = i[keep], j[keep]
    A = sym(n, i, j, np.ones(i.size))
    A.data[:] = 1.0
    U = sp.triu(A, 1).tocsr()
    if couplings == "pmj":
        U.data = rng.choice([-1.0, 1.0], size=U.nnz)
    elif couplings == "int3":
        U.data = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], size=U.nnz)
    else:
        U.data = rng.normal(size=U.nnz)
    J = (U + U.T).tolil()
    if diag:
        J[7, 7] = 1.0 if couplings != "gauss" else 0.375
        J[250, 250] = -1.0 if couplings != "gauss" else -1.25
    J = J.tocsr()
    J.sort_indices()
    h = np.zeros(n) if couplings == "pmj" else rng.integers(-1, 2, n).astype(np.float64) if couplings == "int3" else rng.normal(size=n)
    return J, h


# ------------------------------------------------------------------------------------------------------------------------
# packer: reference levels -> the read-back layout
# ------------------------------------------------------------------------------------------------------------------------
def pack_fused(J, h, window=0, T=4, sweep0=7, seed=SEED, workers=3, quads=1, fmt=FMT_ADDR, bank_aware=0, with_val=False, scale=1.0):
    A = sc.csr_of(J)
    n = A.shape[0]
    n_pad = (n + 15) // 16 * 16
    plan = dict(fmt=fmt, T=T, sweep0=sweep0, seed=seed, workers=workers, quads=quads, bank_aware=bank_aware, n_pad=n_pad, k_dummy=n_pad,
                k_zero=n_pad + 8, neg_off=n_pad + 16, tab_words=n_pad, val=None)
    cap = 64 * workers
    pos = sc.window_orders(n, sweep0, T, window, seed)
    ref = sc.reference_levels(A, pos)
    deg = np.diff(A.indptr)
    lanes_k, kind_k = sc.lanes_of(deg, quads)
    rng = np.random.default_rng(11)
    items = []                       # (k, t, lane) per position, k = -1 for a dummy
    loff, run, himax = [], 0, 0
    for lv in range(1, int(ref.max()) + 1):
        t_, k_ = np.nonzero(ref == lv)
        here = []
        for L in (4, 2, 1):
            for t, k in zip(t_[lanes_k[k_] == L], k_[lanes_k[k_] == L]):
                here += [(k, t, p) for p in range(L)]
        grouped = sum(1 for it in here if lanes_k[it[0]] > 1)
        himax = max(himax, (grouped + 63) // 64)
        for p in range(0, len(here), cap):
            loff.append((run + p) // 64)
        here += [(-1, 0, 0)] * (-len(here) % 64)
        items += here
        run += len(here)
    loff.append(run // 64)
    npos = run
    loff = np.array(loff, dtype=np.int32)
    head = np.zeros((npos, 2), dtype=np.int64)
    col, jq, pad = np.zeros((npos, 8), dtype=np.int64), np.zeros((npos, 8), dtype=np.int64), np.ones((npos, 8), dtype=bool)
    val = np.zeros((npos, 9))
    send = np.zeros(T, dtype=np.int32)
    for p, (k, t, lane) in enumerate(items):
        if k < 0:
            head[p] = (plan["k_dummy"] | ((3 * n_pad) << 16), 0)
            continue
        level = np.searchsorted(loff, p // 64, side="right") - 1
        send[t] = max(send[t], level)
        head[p] = (k | (kind_k[k] << 14) | (((t % 3) * n_pad + k) << 16), 0 if lane else int(np.rint(h[k] * scale)))
        e = np.arange(A.indptr[k] + 8 * lane, min(A.indptr[k + 1], A.indptr[k] + 8 * lane + 8))
        slots = rng.permutation(8)[:e.size] if bank_aware else np.arange(e.size)
        col[p, slots], pad[p, slots] = A.indices[e], False
        jq[p, slots] = np.sign(A.data[e]) if fmt == FMT_ADDR else np.rint(A.data[e] * scale)
        val[p, slots] = np.abs(A.data[e]) if fmt == FMT_ADDR else A.data[e]
        val[p, 8] = h[k]
    plan.update(head=head.astype(np.uint32).view(np.int32).reshape(npos, 2).copy(), loff=loff, send=send, nlev=len(loff) - 1, npos=npos,
                hi_max=min(himax, workers), pstride=npos + 64)
    plan["head"][:, 1] = head[:, 1].astype(np.int32)
    plan["ell"] = sc.encode_entries(plan, col, jq, pad)
    if with_val:
        plan["val"] = np.concatenate([val[:, 2 * q:2 * q + 2].reshape(-1) for q in range(4)] + [val[:, 8]])
    return plan, pos, ref


def pack_order(J, pos, cap=0, big=False):
    A = sc.csr_of(J)
    n = A.shape[0]
    deg = np.diff(A.indptr)
    ref = sc.reference_levels(A, pos[None, :])[0] - 1
    order, off, hm = [], [], 0
    for lv in range(int(ref.max()) + 1):
        ks = np.flatnonzero(ref == lv)
        if not big:
            ks = np.concatenate([ks[deg[ks] > 8], ks[deg[ks] <= 8][::-1]])
            hm = max(hm, int((deg[ks] > 8).sum()))
        off += list(range(len(order), len(order) + ks.size, cap if cap else n))
        order += [(k if big else k | (deg[k] << 16), A.indptr[k]) for k in ks]
    off.append(n)
    return dict(order=np.array(order, dtype=np.int64).astype(np.uint32).view(np.int32).reshape(n, 2), lvl_off=np.array(off, dtype=np.int32),
                nlev=len(off) - 1, hi_max=n if big else hm, big=big, cap=cap)


# ------------------------------------------------------------------------------------------------------------------------
# array-level mutations
# ------------------------------------------------------------------------------------------------------------------------
def rejects(plan, J, h, rule, **kw):
    with pytest.raises(sc.ScheduleError) as e:
        sc.check_fused(plan, J, h, 0, **kw)
    assert e.value.rule == rule, str(e.value)
    return str(e.value)


# ------------------------------------------------------------------------------------------------------------------------
# the checker accepts the reference scheduler's output
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("couplings,fmt,scale", [("pmj", FMT_ADDR, 1.0), ("int3", FMT_COMPACT, 1.0), ("gauss", FMT_WIDE, 2.0 ** 20)])
@pytest.mark.parametrize("quads,bank_aware,with_val", [(1, 1, False), (0, 0, False), (1, 0, True)])
def test_reference_schedule_passes(couplings, fmt, scale, quads, bank_aware, with_val):
    J, h = mixed_graph(couplings=couplings, diag=True)
    plan, pos, ref = pack_fused(J, h, fmt=fmt, quads=quads, bank_aware=bank_aware, with_val=with_val, scale=scale, sweep0=0x80000003)
    r = sc.check_fused(plan, J, h, 0, nofill=True)
    assert r["exact"] and r["depth"] == int(ref.max()) and r["scale"] == scale
    kinds = set(sc.decode_heads(plan)[1].tolist())
    assert kinds == ({0, 1, 2, 3} if quads else {0, 1, 3})


def test_reference_schedule_without_groups_and_second_window():
    J = mixed_graph()[0]
    long_rows = np.flatnonzero(np.diff(J.indptr) > 8)
    J = J.tolil()
    J[long_rows, :] = 0
    J[:, long_rows] = 0
    J = J.tocsr()
    J.eliminate_zeros()
    h = np.zeros(300)
    plan, _, _ = pack_fused(J, h, window=1)
    assert set(sc.decode_heads(plan)[1].tolist()) == {0} and plan["hi_max"] == 0
    sc.check_fused(plan, J, h, 1, nofill=True)
    with pytest.raises(sc.ScheduleError):                   # the orders of window 0 are other orders
        sc.check_fused(plan, J, h, 0, nofill=True)


@pytest.mark.parametrize("shape", ["complete", "edgeless", "star_first", "star_last", "bipartite", "matchings", "path"])
def test_worst_case_shapes_at_reduced_size(shape):
    """The shapes of tests/test_gpu_schedules.py, smaller: a cap that splits levels (edgeless, matchings), TAIL rows (complete,
    star, bipartite), depth n (path)."""
    rng = np.random.default_rng(5)
    n, T, s0 = 96, 3, 0x80000000
    p0 = sc.window_orders(n, s0, T, 0, SEED)[0]
    by = np.argsort(p0)
    if shape == "complete":
        n = 40
        i, j = np.triu_indices(n, 1)
    elif shape == "edgeless":
        n = 200
        i = j = np.zeros(0, dtype=np.int64)
    elif shape.startswith("star"):
        hub = by[0] if shape == "star_first" else by[-1]
        j = np.setdiff1d(np.arange(n), [hub])[:50]
        i = np.full(50, hub)
    elif shape == "bipartite":
        i, j = np.meshgrid(np.arange(6), np.arange(6, n), indexing="ij")
        i, j = i.reshape(-1), j.reshape(-1)
    elif shape == "matchings":
        n = 400
        pr = [rng.permutation(n) for _ in range(9)]
        i, j = np.concatenate([p[0::2] for p in pr]), np.concatenate([p[1::2] for p in pr])
    else:
        i, j = by[:-1], by[1:]
    J = sym(n, i, j, np.ones(len(i)))
    J.data[:] = rng.choice([-1.0, 1.0], size=J.nnz)
    J = sp.triu(J, 1).tocsr()
    J = (J + J.T).tocsr()
    plan, pos, ref = pack_fused(J, np.zeros(n), T=T, sweep0=s0, workers=1)
    r = sc.check_fused(plan, J, np.zeros(n), 0, nofill=True, pos=pos, ref=ref)
    if shape == "complete":
        assert ref.max(axis=1).tolist() == [40, 80, 120] and r["levels"] == 120
    if shape == "path":
        assert ref[0].max() == n
    if shape in ("edgeless", "matchings"):
        assert r["levels"] > r["depth"]                     # the cap of 64 splits levels
    for t in range(T):                                       # the per-sweep rule on the same orders, capped and not, both forms
        sc.check_order(pack_order(J, pos[t]), J, pos[t])
        sc.check_order(pack_order(J, pos[t], cap=7), J, pos[t])
        sc.check_order(pack_order(J, pos[t], big=True), J, pos[t])


# ------------------------------------------------------------------------------------------------------------------------
# per-sweep mutations
# ------------------------------------------------------------------------------------------------------------------------
def order_rejects(plan, J, pos, rule):
    with pytest.raises(sc.ScheduleError) as e:
        sc.check_order(plan, J, pos)
    assert e.value.rule == rule, str(e.value)


def test_order_mutations():
    J, _ = mixed_graph()
    A = sc.csr_of(J)
    pos = sc.window_orders(300, 5, 1, 0, SEED)[0]
    good = pack_order(J, pos)
    sc.check_order(good, J, pos)
    k = good["order"][:, 0] & 0xFFFF
    at = np.empty(300, dtype=np.int64)
    at[k] = np.arange(300)
    # two spins swapped across a dependent pair
    ek, ej = sc._edges(A)
    e = np.flatnonzero(pos[ej] < pos[ek])[0]
    m = copy.deepcopy(good)
    m["order"][[at[ek[e]], at[ej[e]]]] = m["order"][[at[ej[e]], at[ek[e]]]]
    order_rejects(m, J, pos, "P3")
    # an offset moved by one: level 1 loses its first spin to level 0, where one of its earlier neighbours stands
    m = copy.deepcopy(good)
    m["lvl_off"][1] += 1
    order_rejects(m, J, pos, "P3")
    # ... between two sub-levels of one earliest level nothing depends on it: the cut is in the wrong place
    J0 = sp.csr_matrix((300, 300))
    capped = pack_order(J0, pos, cap=64)
    sc.check_order(capped, J0, pos)
    m = copy.deepcopy(capped)
    assert np.diff(capped["lvl_off"]).tolist() == [64, 64, 64, 64, 44]
    m["lvl_off"][4] -= 1
    order_rejects(m, J0, pos, "P4")
    m = copy.deepcopy(capped)
    m["lvl_off"] = np.delete(m["lvl_off"], 1)
    m["nlev"] -= 1
    order_rejects(m, J0, pos, "P2")                          # a level wider than the cap
    # a long row behind a short one
    deg = np.diff(A.indptr)
    lv = np.searchsorted(good["lvl_off"], np.arange(300), side="right") - 1
    p_long = next(p for p in range(300) if deg[k[p]] > 8 and (deg[k[lv == lv[p]]] <= 8).any())
    p_short = np.flatnonzero((lv == lv[p_long]) & (deg[k] <= 8))[0]
    m = copy.deepcopy(good)
    m["order"][[p_long, p_short]] = m["order"][[p_short, p_long]]
    order_rejects(m, J, pos, "P5")
    m = copy.deepcopy(good)
    m["hi_max"] += 1
    order_rejects(m, J, pos, "P5")
    # a spin twice, a wrong degree, a wrong row start
    m = copy.deepcopy(good)
    m["order"][3] = m["order"][4]
    order_rejects(m, J, pos, "P1")
    m = copy.deepcopy(good)
    m["order"][3, 0] += 1 << 16
    order_rejects(m, J, pos, "P1")
    m = copy.deepcopy(good)
    m["order"][3, 1] += 1
    order_rejects(m, J, pos, "P1")
    # the global-memory form carries no degree and reports hi_max = n
    b = pack_order(J, pos, big=True)
    sc.check_order(b, J, pos)
    b["hi_max"] = 3
    order_rejects(b, J, pos, "P5")


# ------------------------------------------------------------------------------------------------------------------------
# fused mutations
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    """+-J mixed graph with the value plane (ADDR entries in row order), and what the checker says about it."""
    J, h = mixed_graph()
    plan, pos, ref = pack_fused(J, h, with_val=True)
    r = sc.check_fused(plan, J, h, 0, nofill=True, pos=pos, ref=ref)
    return J, h, plan, pos, ref, r


def fresh(base):
    J, h, plan, pos, ref, r = base
    return J, h, copy.deepcopy(plan), dict(nofill=False, pos=pos, ref=ref), r


def test_level_mutations(base):
    J, h, plan, kw, r = fresh(base)
    lev, at, pos = r["lev"], r["at"], kw["pos"]
    A = sc.csr_of(J)
    deg = np.diff(A.indptr)
    # one item into its predecessor's level (a dummy stands behind the level's items, so the occurrences keep their order)
    t, k = next((t, k) for t in range(1, 4) for k in range(300) if deg[k] <= 8 and sc.dummy_in_level(plan, lev[t - 1, k]) is not None)
    m = copy.deepcopy(plan)
    sc.swap_positions(m, at[t, k], sc.dummy_in_level(m, lev[t - 1, k]))
    rejects(m, J, h, "F3", **kw)
    # anti-dependency: k's only neighbour j comes later in sweep 1; (1, k) moves into the level of (0, j)
    ek, ej = sc._edges(A)
    e = next(e for e in range(ek.size) if deg[ek[e]] == 1 and pos[1][ej[e]] > pos[1][ek[e]] and lev[0, ej[e]] > lev[0, ek[e]]
             and sc.dummy_in_level(plan, lev[0, ej[e]]) is not None)
    m = copy.deepcopy(plan)
    sc.swap_positions(m, at[1, ek[e]], sc.dummy_in_level(m, lev[0, ej[e]]))
    assert "anti-dependency" in rejects(m, J, h, "F4", **kw)
    # a plain dependency, for comparison: j precedes k in sweep 0 and k moves into j's level
    e = next(e for e in range(ek.size) if deg[ek[e]] == 1 and pos[0][ej[e]] < pos[0][ek[e]] and sc.dummy_in_level(plan, lev[0, ej[e]]) is not None)
    m = copy.deepcopy(plan)
    sc.swap_positions(m, at[0, ek[e]], sc.dummy_in_level(m, lev[0, ej[e]]))
    assert "anti-dependency" not in rejects(m, J, h, "F4", **kw)
    # an isolated spin's sweep-2 update in front of the end of sweep 0 (behind its own sweep-1 update: only the floor holds it)
    k = 290
    assert deg[k] == 0 and lev[1, k] + 1 < r["lev"][0].max()
    m = copy.deepcopy(plan)
    sc.swap_positions(m, at[2, k], sc.dummy_in_level(m, lev[1, k] + 1))
    rejects(m, J, h, "F5", **kw)


def test_item_mutations(base):
    J, h, plan, kw, r = fresh(base)
    at = r["at"]
    k_, kind, thr, dummy, level = sc.decode_heads(plan)
    d = int(np.flatnonzero(dummy)[-1])
    m = copy.deepcopy(plan)                                 # two items of different sweeps of one spin exchanged
    sc.swap_positions(m, at[1, 100], at[2, 100])
    rejects(m, J, h, "F2", **kw)
    m = copy.deepcopy(plan)                                 # an item dropped
    sc.copy_position(m, d, at[1, 100])
    rejects(m, J, h, "F1", **kw)
    m = copy.deepcopy(plan)                                 # an item duplicated
    sc.copy_position(m, at[1, 100], d)
    rejects(m, J, h, "F1", **kw)
    deg = np.diff(sc.csr_of(J).indptr)
    pair = next(int(p) for p in at[1, (deg > 8) & (deg <= 16)] if level[p + 2] == level[p])
    assert kind[pair] == sc.KIND_PAIR and pair % 2 == 0
    m = copy.deepcopy(plan)                                 # a pair moved to an odd start
    sc.swap_positions(m, pair + 1, pair + 2)
    sc.swap_positions(m, pair, pair + 1)
    rejects(m, J, h, "F1", **kw)
    m = copy.deepcopy(plan)                                 # a group split over two chunks
    sc.swap_positions(m, pair + 1, pair + 1 + 64 if level[min(pair + 65, plan["npos"] - 1)] == level[pair] else pair + 1 - 64)
    rejects(m, J, h, "F1", **kw)
    m = copy.deepcopy(plan)                                 # a threshold word of the wrong table slot
    m["head"][at[1, 100], 0] += plan["tab_words"] << 16
    rejects(m, J, h, "F2", **kw)


def test_publication_mutations():
    n = 300
    J, h = sp.csr_matrix((n, n)), np.zeros(n)
    plan, pos, ref = pack_fused(J, h, T=3)
    sc.check_fused(plan, J, h, 0, nofill=True, pos=pos, ref=ref)
    assert np.diff(plan["loff"]).tolist() == [3, 2] * 3      # 192 + 108 positions per sweep at a cap of 192
    m = copy.deepcopy(plan)                                 # a level over the cap: it takes the first chunk of the next one
    m["loff"][1] += 1
    rejects(m, J, h, "F6", pos=pos, ref=ref)
    for t in range(3):                                      # send[t] off by one, either way
        for d in (-1, 1):
            m = copy.deepcopy(plan)
            m["send"][t] += d
            rejects(m, J, h, "F5", pos=pos, ref=ref)
    m = copy.deepcopy(plan)
    m["hi_max"] = 0
    sc.check_fused(m, J, h, 0, pos=pos, ref=ref)             # no groups: nothing to hold
    m["nlev"] += 1
    rejects(m, J, h, "F1", pos=pos, ref=ref)


@pytest.mark.parametrize("couplings,fmt", [("pmj", FMT_ADDR), ("int3", FMT_COMPACT), ("gauss", FMT_WIDE)])
@pytest.mark.parametrize("bank_aware", [0, 1])
def test_row_entry_mutations(couplings, fmt, bank_aware):
    J, h = mixed_graph(couplings=couplings, diag=True)
    plan, pos, ref = pack_fused(J, h, fmt=fmt, bank_aware=bank_aware, scale=1.0 if fmt != FMT_WIDE else 2.0 ** 16)
    kw = dict(pos=pos, ref=ref)
    at = sc.check_fused(plan, J, h, 0, **kw)["at"]
    p = int(at[1, 100])
    col, jq, pad = sc.decode_entries(plan)
    real, free = int(np.flatnonzero(~pad[p])[0]), int(np.flatnonzero(pad[p])[0])

    def drop(c, q, d):
        d[real] = True

    def dup(c, q, d):
        c[free], q[free], d[free] = c[real], q[real], False

    def flip(c, q, d):
        q[real] = -q[real]

    def on_dummy(c, q, d):
        c[0], q[0], d[0] = 3, 1, False

    for fn in (drop, dup) + ((flip,) if fmt == FMT_ADDR else ()):
        m = copy.deepcopy(plan)
        sc.rewrite_entries(m, p, fn)
        rejects(m, J, h, "F8", **kw)
    m = copy.deepcopy(plan)
    sc.rewrite_entries(m, int(np.flatnonzero(sc.decode_heads(plan)[3])[0]), on_dummy)
    rejects(m, J, h, "F8", **kw)
    m = copy.deepcopy(plan)                                 # the stored diagonal of spin 7 is a row entry like any other
    pd = int(at[0, 7])
    assert 7 in col[pd][~pad[pd]].tolist()
    sc.rewrite_entries(m, pd, lambda c, q, d: d.__setitem__(int(np.flatnonzero(~d & (c == 7))[0]), True))
    rejects(m, J, h, "F8", **kw)
    if fmt != FMT_ADDR:                                     # one coupling at another scale
        m = copy.deepcopy(plan)
        sc.rewrite_entries(m, p, lambda c, q, d: q.__setitem__(real, 4 * q[real]))
        rejects(m, J, h, "F8", **kw)


def test_value_plane_and_head_mutations(base):
    J, h, plan, kw, r = fresh(base)
    at, npos = r["at"], plan["npos"]
    p = int(at[1, 100])
    col, jq, pad = sc.decode_entries(plan)
    assert not pad[p, 0] and pad[p, 7]
    m = copy.deepcopy(plan)                                 # an entry in the wrong slot: slots 0 and 7 of plane pairs 0 / 3
    v = m["val"][:8 * npos].reshape(4, npos, 2)
    v[0, p, 0], v[3, p, 1] = v[3, p, 1], v[0, p, 0]
    rejects(m, J, h, "F9", **kw)
    m = copy.deepcopy(plan)
    m["val"][8 * npos + p] += 1.0                           # the field
    rejects(m, J, h, "F9", **kw)
    m = copy.deepcopy(plan)
    m["val"][8 * npos + int(np.flatnonzero(sc.decode_heads(plan)[3])[0])] = 1.0
    rejects(m, J, h, "F9", **kw)
    m = copy.deepcopy(plan)
    deg = np.diff(sc.csr_of(J).indptr)
    m["head"][at[2, np.flatnonzero(deg > 8)[0]] + 1, 1] = 1  # head.y on the second lane of a group
    rejects(m, J, h, "F9", **kw)
    m = copy.deepcopy(plan)
    m["head"][at[2, 100], 1] += 1                           # one value per spin
    rejects(m, J, h, "F9", **kw)


def test_depth_rule():
    """F7: a plan with level fill may be deeper than the reference, never shallower; where no level overflows it is the reference."""
    n = 300
    J, h = sp.csr_matrix((n, n)), np.zeros(n)
    plan, pos, ref = pack_fused(J, h, T=3)
    r = sc.check_fused(plan, J, h, 0, pos=pos, ref=ref)
    assert not r["exact"] and r["levels"] == 6 and r["depth"] == 3
    J2, h2 = mixed_graph()
    plan, pos, ref = pack_fused(J2, h2)
    r = sc.check_fused(plan, J2, h2, 0, pos=pos, ref=ref)
    assert r["exact"]
    m = copy.deepcopy(plan)                                 # a single row one level late, nothing depends on it: legal only as level fill
    k = 295
    lvl = sc.decode_heads(m)[4]
    end = int(np.flatnonzero(~sc.decode_heads(m)[3] & (lvl == r["lev"][3, k]))[-1])     # last item of its level: no gap stays behind
    sc.swap_positions(m, r["at"][3, k], end)
    sc.swap_positions(m, end, sc.dummy_in_level(m, r["lev"][3, k] + 1))
    with pytest.raises(sc.ScheduleError) as e:
        sc.check_fused(m, J2, h2, 0, pos=pos, ref=ref)
    assert e.value.rule == "F7"
