"""Level schedules checked item by item against the dependency rules (plain NumPy / SciPy; no test in here; imports nothing of the
product or of oracle/ -- visiting orders come from lawcheck.order_positions, which restates Philox on its own).

A level schedule reorders the updates of one sweep (per-sweep plans: k_levelize, k_blv_*) or of T consecutive sweeps (fused
windows: k_levelize_fused) so that every level holds independent updates only.  The rules are the ones the kernels' comments
state; nothing below shares code with the kernels that build or pack a plan.

Reference scheduler (sequential): for sweep t, in visiting order,

    level(t, k) = 1 + max(level(t-1, k), last level of sweep t-2,
                          level(t, j) for the neighbours j that precede k in sweep t, level(t-1, j) for the other neighbours j)

self-couplings are no neighbours, missing terms count 0.  With T = 1 this is the per-sweep rule (zero-based there).

check_order(plan, J, pos)        rules P1-P5, a per-sweep plan as Engine.plan_order returns it
check_fused(plan, J, h, window)  rules F1-F9, one window of a fused plan as Engine.plan_items returns it

A broken rule raises ScheduleError; its .rule is the rule's name ("P3", "F4", ...), the message names the window, the positions and
the spins involved."""
import numpy as np
import scipy.sparse as sp

import lawcheck

LCAP = 1024                      # level offsets the sweep kernels keep: a fused plan has at most LCAP - 1 levels
FZ_W = 8                         # row entries per schedule position of a fused plan
FMT_WIDE, FMT_COMPACT, FMT_ADDR = 0, 1, 2
KIND_SINGLE, KIND_PAIR, KIND_QUAD, KIND_TAIL = 0, 1, 2, 3
PLANES = {FMT_WIDE: 4, FMT_COMPACT: 2, FMT_ADDR: 1}      # 16-byte entry planes per position


class ScheduleError(AssertionError):
    def __init__(self, rule, msg):
        super().__init__(f"{rule}: {msg}")
        self.rule = rule


def _need(ok, rule, msg):
    if not ok:
        raise ScheduleError(rule, msg() if callable(msg) else msg)


def _some(a, limit=8):
    a = np.asarray(a).reshape(-1)
    return f"{a[:limit].tolist()}{' ...' if a.size > limit else ''} ({a.size})"


def csr_of(J):
    """CSR with sorted columns and every stored entry kept (a stored diagonal stays: the planners see it as a row entry)."""
    A = sp.csr_matrix(J).astype(np.float64).copy()
    A.sort_indices()
    return A


def window_orders(n, sweep0, T, window, seed):
    """pos[t][k]: position of spin k in the order of sweep t of window `window` (sweep sweep0 + window T + t, 32-bit wrap)."""
    return np.stack([lawcheck.order_positions(n, (sweep0 + window * T + t) & 0xFFFFFFFF, seed) for t in range(T)])


def reference_levels(A, pos, floor=True):
    """The reference scheduler.  A: CSR; pos [T, n] visiting positions.  -> levels [T, n], 1-based."""
    pos = np.atleast_2d(pos)
    T, n = pos.shape
    ip, ix = A.indptr, A.indices
    lev = np.zeros((T, n), dtype=np.int64)
    prev = np.zeros(n, dtype=np.int64)
    last = []                                       # last level of every finished sweep
    for t in range(T):
        cur = np.zeros(n, dtype=np.int64)
        fl = last[t - 2] if (floor and t >= 2) else 0
        p = pos[t]
        for k in np.argsort(p, kind="stable"):
            nb = ix[ip[k]:ip[k + 1]]
            nb = nb[nb != k]
            m = max(int(prev[k]), fl)
            if nb.size:
                before = p[nb] < p[k]
                m = max(m, int(np.where(before, cur[nb], prev[nb]).max()))
            cur[k] = m + 1
        lev[t] = cur
        prev = cur
        last.append(int(cur.max()) if n else 0)
    return lev


def _edges(A):
    """Stored off-diagonal entries (k, j)."""
    k = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    j = A.indices.astype(np.int64)
    keep = k != j
    return k[keep], j[keep]


# ------------------------------------------------------------------------------------------------------------------------
# per-sweep plans
# ------------------------------------------------------------------------------------------------------------------------
def check_order(plan, J, pos, name="order"):
    """plan: dict with order [n, 2] int32, lvl_off [nlev + 1], nlev, hi_max, big (built by the global-memory levelizer), cap (widest
    published level; 0: no cap in force).  pos [n]: visiting position of every spin."""
    A = csr_of(J)
    n = A.shape[0]
    deg = np.diff(A.indptr).astype(np.int64)
    order = np.asarray(plan["order"]).astype(np.int64).reshape(n, 2)
    off = np.asarray(plan["lvl_off"]).astype(np.int64)
    nlev, big, cap = int(plan["nlev"]), bool(plan["big"]), int(plan["cap"])
    w0 = order[:, 0] & 0xFFFFFFFF
    k = w0 if big else (w0 & 0xFFFF)
    # P1
    _need(np.array_equal(np.sort(k), np.arange(n)), "P1", lambda: f"{name}: not every spin exactly once; missing "
          f"{_some(np.setdiff1d(np.arange(n), k))}, twice {_some(np.unique(k[np.argsort(k)][1:][np.diff(np.sort(k)) == 0]))}")
    if not big:
        bad = np.flatnonzero((w0 >> 16) != deg[k])
        _need(bad.size == 0, "P1", lambda: f"{name}: degree field differs from the CSR degree at positions {_some(bad)}, spins {_some(k[bad])}")
    bad = np.flatnonzero(order[:, 1] != A.indptr[k])
    _need(bad.size == 0, "P1", lambda: f"{name}: second word is not rowptr[k] at positions {_some(bad)}, spins {_some(k[bad])}")
    # P2
    _need(off.size == nlev + 1 and nlev >= (1 if n else 0), "P2", f"{name}: {off.size} offsets for {nlev} levels")
    _need(off[0] == 0 and off[-1] == n, "P2", f"{name}: offsets run from {off[0]} to {off[-1]}, not 0 to {n}")
    bad = np.flatnonzero(np.diff(off) <= 0)
    _need(bad.size == 0, "P2", lambda: f"{name}: offsets not strictly increasing at levels {_some(bad)}")
    if cap > 0:
        bad = np.flatnonzero(np.diff(off) > cap)
        _need(bad.size == 0, "P2", lambda: f"{name}: levels {_some(bad)} wider than the cap {cap}: {_some(np.diff(off)[bad])}")
    # P3
    plev = np.empty(n, dtype=np.int64)
    plev[k] = np.searchsorted(off, np.arange(n), side="right") - 1
    ek, ej = _edges(A)
    bad = np.flatnonzero((pos[ej] < pos[ek]) & (plev[ej] >= plev[ek]))
    _need(bad.size == 0, "P3", lambda: f"{name}: spins {_some(ek[bad])} not behind their earlier neighbours {_some(ej[bad])}: levels "
          f"{_some(plev[ek[bad]])} against {_some(plev[ej[bad]])}")
    # P4
    ref = reference_levels(A, pos[None, :])[0] - 1
    width = np.bincount(ref, minlength=int(ref.max()) + 1 if n else 0)
    c = cap if cap > 0 else max(n, 1)
    start = np.concatenate([[0], np.cumsum(width)])
    exp = np.concatenate([np.arange(start[l], start[l + 1], c) for l in range(width.size)] + [[n]]).astype(np.int64)
    count = int(np.sum((width + c - 1) // c))
    _need(nlev == count, "P4", f"{name}: {nlev} published levels, the reference has {count} (earliest levels {width.size}, cap {cap})")
    for l in range(width.size):
        got, want = np.sort(k[start[l]:start[l + 1]]), np.flatnonzero(ref == l)
        _need(np.array_equal(got, want), "P4", lambda: f"{name}: earliest level {l} (positions {start[l]}..{start[l + 1] - 1}) holds spins "
              f"{_some(np.setdiff1d(got, want))} that the reference has elsewhere, and lacks {_some(np.setdiff1d(want, got))}")
    _need(np.array_equal(off, exp), "P4", lambda: f"{name}: offsets differ from the reference's levels cut at the cap, first at level "
          f"{int(np.flatnonzero(off != exp)[0])}")
    # P5
    if big:
        _need(int(plan["hi_max"]) == n, "P5", f"{name}: hi_max {plan['hi_max']} of a global-memory plan, not n = {n}")
    else:
        long_row = deg[k] > 8
        hm = 0
        for l in range(width.size):
            lr = long_row[start[l]:start[l + 1]]
            nl_ = int(lr.sum())
            hm = max(hm, nl_)
            _need(bool(lr[:nl_].all()), "P5", lambda: f"{name}: earliest level {l}: a long row (spins {_some(k[start[l]:start[l + 1]][lr])}) stands "
                  f"behind a short one, positions {start[l]}..{start[l + 1] - 1}")
        _need(int(plan["hi_max"]) == hm, "P5", f"{name}: hi_max {plan['hi_max']}, the largest number of long rows in a level is {hm}")
    return {"levels": nlev, "earliest": int(width.size)}


# ------------------------------------------------------------------------------------------------------------------------
# fused windows
# ------------------------------------------------------------------------------------------------------------------------
def decode_heads(plan):
    """-> k, kind, thr (unsigned), dummy mask, level of every position below npos."""
    x = np.asarray(plan["head"]).reshape(-1, 2)[:, 0].astype(np.int64) & 0xFFFFFFFF
    k, kind, thr = x & 0x3FFF, (x >> 14) & 3, x >> 16
    dummy = (k == plan["k_dummy"]) & (thr == 3 * plan["tab_words"])
    loff = np.asarray(plan["loff"]).astype(np.int64)
    level = np.searchsorted(loff, np.arange(x.size) // 64, side="right") - 1
    return k, kind, thr, dummy, level


def decode_entries(plan):
    """-> col [npos, 8], jq [npos, 8] (ADDR: the sign, +-1), pad [npos, 8] (bool), from the entry planes by the plan's format."""
    fmt, npos = plan["fmt"], int(plan["npos"])
    ell = np.asarray(plan["ell"]).reshape(PLANES[fmt], npos, 4)
    if fmt == FMT_ADDR:
        w = ell[0].astype(np.int64) & 0xFFFFFFFF                                    # [npos, 4] words, two addresses each
        ad = np.stack([w & 0xFFFF, w >> 16], axis=2).reshape(npos, 8)
        pad = ad == plan["k_zero"]
        neg = ad >= plan["neg_off"]
        return np.where(neg, ad - plan["neg_off"], ad), np.where(neg, -1, 1), pad
    if fmt == FMT_COMPACT:
        v = np.concatenate([ell[0], ell[1]], axis=1).astype(np.int64) & 0xFFFFFFFF  # [npos, 8]
        col, jq = v >> 16, ((v & 0xFFFF) ^ 0x8000) - 0x8000
        return col, jq, (col == plan["k_dummy"]) & (jq == 0)
    e = np.concatenate([ell[q] for q in range(4)], axis=1).astype(np.int64)        # [npos, 8 words]: col, jq, col, jq ...
    col, jq = e[:, 0::2], e[:, 1::2]
    return col, jq, (col == plan["k_dummy"]) & (jq == 0)


def decode_values(plan):
    """-> v [npos, 8] (value of every entry slot), hval [npos]."""
    npos = int(plan["npos"])
    val = np.asarray(plan["val"], dtype=np.float64)
    v = val[:8 * npos].reshape(4, npos, 2)
    return np.concatenate([v[q] for q in range(4)], axis=1), val[8 * npos:9 * npos]


def lanes_of(deg, quads):
    """Schedule positions a row of `deg` stored entries takes, and the kind its lanes carry."""
    deg = np.asarray(deg)
    lanes = np.where(deg <= FZ_W, 1, np.where((deg <= 2 * FZ_W) | (not quads), 2, 4))
    kind = np.where(deg <= FZ_W, KIND_SINGLE, np.where(deg <= 2 * FZ_W, KIND_PAIR,
                    np.where(bool(quads) & (deg <= 4 * FZ_W), KIND_QUAD, KIND_TAIL)))
    return lanes, kind


def check_fused(plan, J, h, window, nofill=False, pos=None, ref=None):
    """One window of a fused plan (the dict of Engine.plan_items) against F1-F9.  J, h: the instance; nofill: the plan was built
    with NLMC_NO_LEVEL_FILL=1.  pos [T, n] / ref [T, n]: the visiting orders / the reference scheduler's levels where the caller
    has them already (they are computed otherwise).  -> dict of figures (levels, reference depth, exact)."""
    A = csr_of(J)
    n, T = A.shape[0], int(plan["T"])
    W = f"window {window}"
    deg = np.diff(A.indptr).astype(np.int64)
    npos, nlev, cap = int(plan["npos"]), int(plan["nlev"]), 64 * int(plan["workers"])
    loff, send = np.asarray(plan["loff"]).astype(np.int64), np.asarray(plan["send"]).astype(np.int64)
    if pos is None:
        pos = window_orders(n, int(plan["sweep0"]), T, window, int(plan["seed"]))
    k, kind, thr, dummy, level = decode_heads(plan)
    real = ~dummy
    P = np.arange(npos)

    # F1 coverage and groups
    _need(npos % 64 == 0 and k.size == npos, "F1", f"{W}: npos {npos} is no multiple of 64 (or {k.size} heads)")
    _need(loff.size == nlev + 1 and loff[0] == 0 and loff[-1] * 64 == npos and np.all(np.diff(loff) > 0), "F1",
          lambda: f"{W}: level offsets do not cover chunks 0..{npos // 64} in strictly increasing steps: {_some(loff)}")
    bad = P[real & (k >= n)]
    _need(bad.size == 0, "F1", lambda: f"{W}: positions {_some(bad)} are neither dummies nor spins below n: k {_some(k[bad])}, thr {_some(thr[bad])}")
    lanes_k, kind_k = lanes_of(deg, plan["quads"])
    rp = P[real]
    L = lanes_k[k[rp]]
    bad = rp[kind[rp] != kind_k[k[rp]]]
    _need(bad.size == 0, "F1", lambda: f"{W}: kind of positions {_some(bad)} (spins {_some(k[bad])}) does not match the row length: "
          f"{_some(kind[bad])} for {_some(deg[k[bad]])} entries")
    base = rp - rp % L                                      # a group is aligned to its size: first lane of the group of every position
    for i in range(4):
        m = i < L
        q = base[m] + i
        ok = (q < npos)
        ok[ok] &= real[q[ok]] & (k[q[ok]] == k[rp[m]][ok]) & (kind[q[ok]] == kind[rp[m]][ok]) & (q[ok] // 64 == rp[m][ok] // 64)
        bad = rp[m][~ok]
        _need(bad.size == 0, "F1", lambda: f"{W}: positions {_some(bad)} (spins {_some(k[bad])}) are not part of an aligned group of "
              f"{_some(lanes_k[k[bad]])} lanes with one spin and kind in one chunk")
    lane = rp - base                                        # part of the row this position holds
    first = rp[lane == 0]
    cnt = np.bincount(k[first], minlength=n)[:n]
    bad = np.flatnonzero(cnt != T)
    _need(bad.size == 0, "F1", lambda: f"{W}: spins {_some(bad)} occur {_some(cnt[bad])} times, not T = {T}: positions "
          f"{_some(first[np.isin(k[first], bad[:4])])}")
    srt = np.lexsort((first, level[first], k[first]))       # occurrence i of spin k in level order is its update of sweep i
    first = first[srt]
    item_t = np.tile(np.arange(T), n)
    item_k = k[first]
    lev = np.empty((T, n), dtype=np.int64)                  # published level (0-based) of update (t, k)
    lev[item_t, item_k] = level[first]
    at = np.empty((T, n), dtype=np.int64)
    at[item_t, item_k] = first

    # F2 threshold word
    t_of = np.empty(npos, dtype=np.int64)
    t_of[first] = item_t
    bad = np.flatnonzero(thr[base] != ((t_of[base] % 3) * plan["tab_words"] + k[rp]))
    _need(bad.size == 0, "F2", lambda: f"{W}: threshold word of positions {_some(rp[bad])} (spins {_some(k[rp[bad]])}, sweeps "
          f"{_some(t_of[base[bad]])}) is {_some(thr[rp[bad]])}, not (t % 3) tab_words + k")
    bad = np.flatnonzero(thr[rp] != thr[base])
    _need(bad.size == 0, "F2", lambda: f"{W}: lanes of one group differ in their threshold word at positions {_some(rp[bad])}")

    # F3 own order
    if T > 1:
        tt, kk = np.nonzero(lev[1:] <= lev[:-1])
        _need(tt.size == 0, "F3", lambda: f"{W}: updates (t, k) {_some(np.stack([tt + 1, kk], 1))} not behind the spin's update of the sweep "
              f"before: positions {_some(at[tt + 1, kk])} / {_some(at[tt, kk])}, levels {_some(lev[tt + 1, kk])} / {_some(lev[tt, kk])}")

    # F4 neighbours
    ek, ej = _edges(A)
    for t in range(T):
        before = pos[t][ej] < pos[t][ek]
        bad = np.flatnonzero(before & (lev[t][ej] >= lev[t][ek]))
        _need(bad.size == 0, "F4", lambda: f"{W}: sweep {t}: spins {_some(ek[bad])} (positions {_some(at[t][ek[bad]])}) not behind their earlier "
              f"neighbours {_some(ej[bad])} (positions {_some(at[t][ej[bad]])})")
        if t:
            bad = np.flatnonzero(~before & (lev[t - 1][ej] >= lev[t][ek]))
            _need(bad.size == 0, "F4", lambda: f"{W}: sweep {t}: spins {_some(ek[bad])} (positions {_some(at[t][ek[bad]])}) not behind the "
                  f"sweep-{t - 1} update of their later neighbours {_some(ej[bad])} (positions {_some(at[t - 1][ej[bad]])}): anti-dependency")

    # F5 three tables
    last = lev.max(axis=1)
    for t in range(2, T):
        bad = np.flatnonzero(lev[t] <= last[t - 2])
        _need(bad.size == 0, "F5", lambda: f"{W}: sweep-{t} updates of spins {_some(bad)} (positions {_some(at[t][bad])}, levels "
              f"{_some(lev[t][bad])}) not behind the last level of sweep {t - 2} ({last[t - 2]})")
    _need(send.size == T and np.array_equal(send, last), "F5", lambda: f"{W}: send {_some(send)} is not the last level of every sweep {_some(last)}")
    _need(bool(np.all(np.diff(send) > 0)), "F5", lambda: f"{W}: send not strictly increasing: {_some(send)}")

    # F6 width and layout
    width = np.diff(loff) * 64
    bad = np.flatnonzero(width > cap)
    _need(bad.size == 0, "F6", lambda: f"{W}: levels {_some(bad)} wider than the cap of {cap} positions: {_some(width[bad])}")
    _need(nlev <= LCAP - 1, "F6", f"{W}: {nlev} levels, the sweep kernels keep {LCAP - 1}")
    cls = np.zeros(npos, dtype=np.int64)                    # 4 / 2 / 1 lanes, 0 for a dummy
    cls[rp] = L
    bad = np.flatnonzero((level[1:] == level[:-1]) & (cls[1:] > cls[:-1])) + 1
    _need(bad.size == 0, "F6", lambda: f"{W}: positions {_some(bad)} (spins {_some(k[bad])}): inside a level quads stand first, then pairs, "
          f"then single rows, then padding")
    grp = rp[L > 1]
    bad = grp[grp // 64 - loff[level[grp]] >= int(plan["hi_max"])]
    _need(bad.size == 0, "F6", lambda: f"{W}: groups at positions {_some(bad)} lie behind the first hi_max = {plan['hi_max']} chunks of their level")

    # F7 depth
    if ref is None:
        ref = reference_levels(A, pos)
    depth = int(ref.max())
    occupied = int(T * lanes_k.sum())
    _need(nlev >= depth, "F7", f"{W}: {nlev} levels, the reference scheduler needs {depth}")
    _need(nlev >= -(-occupied // cap), "F7", f"{W}: {nlev} levels cannot hold {occupied} positions at {cap} a level")
    rw = np.zeros(depth + 1, dtype=np.int64)                # positions of every earliest level of the reference
    np.add.at(rw, ref.reshape(-1), np.tile(lanes_k, T))
    exact = bool(nofill or rw.max() <= cap)
    if exact:
        sub = (rw[1:] + cap - 1) // cap                     # published levels per earliest level
        _need(nlev == int(sub.sum()), "F7", f"{W}: {nlev} levels, the reference's earliest levels cut at the cap give {int(sub.sum())}")
        early = np.repeat(np.arange(1, depth + 1), sub)     # earliest level of every published level
        bad_t, bad_k = np.nonzero(early[lev] != ref)
        _need(bad_t.size == 0, "F7", lambda: f"{W}: updates (t, k) {_some(np.stack([bad_t, bad_k], 1))} at positions {_some(at[bad_t, bad_k])} are "
              f"not in their earliest level: {_some(early[lev[bad_t, bad_k]])} against the reference's {_some(ref[bad_t, bad_k])}")
        want = np.concatenate([np.minimum(cap, rw[l] - cap * np.arange(sub[l - 1])) for l in range(1, depth + 1)])
        got = np.bincount(level[rp], minlength=nlev)
        _need(np.array_equal(got, want), "F7", lambda: f"{W}: occupied positions per level differ from the earliest levels cut at the cap, first at "
              f"level {int(np.flatnonzero(got != want)[0])}")

    # F8 row entries
    col, jq, pad = decode_entries(plan)
    dp = P[dummy]
    bad = dp[~pad[dp].all(axis=1)]
    _need(bad.size == 0, "F8", lambda: f"{W}: dummies at positions {_some(bad)} hold row entries")
    e0 = A.indptr[k[rp]] + lane * FZ_W                      # this lane's entries: [e0, e0 + 8) of the row, as far as the row goes
    nreal = np.clip(deg[k[rp]] - lane * FZ_W, 0, FZ_W)
    slot = np.arange(FZ_W)[None, :]
    have = slot < nreal[:, None]
    eidx = np.where(have, e0[:, None] + slot, 0)
    a_col, a_val = np.append(A.indices, 0), np.append(A.data, 0.0)      # (an edgeless graph has no entry to point at)
    wcol = np.where(have, a_col[eidx], -1)                  # -1: padding
    wJ = np.where(have, a_val[eidx], 0.0)
    gcol = np.where(pad[rp], -1, col[rp])
    if plan["bank_aware"]:                                  # any order: compare as multisets (a row's columns are distinct)
        o_got, o_want = np.argsort(gcol, axis=1, kind="stable"), np.argsort(wcol, axis=1, kind="stable")
    else:
        o_got = o_want = np.broadcast_to(slot, gcol.shape)
    gs, ws = np.take_along_axis(gcol, o_got, 1), np.take_along_axis(wcol, o_want, 1)
    bad = np.flatnonzero((gs != ws).any(axis=1))
    _need(bad.size == 0, "F8", lambda: f"{W}: positions {_some(rp[bad])} (spins {_some(k[rp[bad]])}, lanes {_some(lane[bad])}) do not hold entries "
          f"[8 lane, 8 lane + 8) of the row{'' if plan['bank_aware'] else ' in row order'}: columns {gs[bad[0]].tolist()} against {ws[bad[0]].tolist()}")
    gq, wj = np.take_along_axis(np.where(pad[rp], 0, jq[rp]), o_got, 1), np.take_along_axis(wJ, o_want, 1)
    m = ws >= 0
    if plan["fmt"] == FMT_ADDR:
        bad = np.flatnonzero((m & (gq != np.sign(wj))).any(axis=1))
        _need(bad.size == 0, "F8", lambda: f"{W}: positions {_some(rp[bad])} (spins {_some(k[rp[bad]])}): the sign of an address entry is not the "
              f"sign of J")
        scale = 1.0
    elif m.any():
        # Jq / J is one constant: the fixed-point scale, a power of two; a coupling that is no multiple of the grain is rounded to
        # the nearest one, so |Jq - scale J| <= 1/2 (and 0 where the instance is integer or dyadic)
        big_ = np.unravel_index(np.argmax(np.abs(wj) * m), wj.shape)
        scale = 2.0 ** np.rint(np.log2(abs(gq[big_] / wj[big_]))) if gq[big_] != 0 else 0.0
        bad = np.flatnonzero((m & (np.abs(gq - scale * wj) > 0.5)).any(axis=1))
        _need(bad.size == 0 and scale > 0, "F8", lambda: f"{W}: positions {_some(rp[bad])} (spins {_some(k[rp[bad]])}): Jq is not {scale} J")
    else:
        scale = 1.0

    # F9 head.y and the value plane
    hy = np.asarray(plan["head"]).reshape(-1, 2)[:, 1].astype(np.int64)
    bad = P[(hy != 0) & (dummy | np.isin(P, rp[lane != 0]))]
    _need(bad.size == 0, "F9", lambda: f"{W}: head.y is not 0 at dummies / later lanes of a group: positions {_some(bad)}")
    hq = hy[at]                                             # [T, n]
    tt, kk = np.nonzero(hq != hq[0][None, :])
    _need(tt.size == 0, "F9", lambda: f"{W}: head.y differs between the occurrences of spins {_some(kk)}: positions {_some(at[tt, kk])}")
    if plan.get("val") is not None:
        v, hv = decode_values(plan)
        bad = dp[(v[dp] != 0).any(axis=1) | (hv[dp] != 0)]
        _need(bad.size == 0, "F9", lambda: f"{W}: value plane of the dummies at positions {_some(bad)} is not 0")
        wv = np.abs(wJ) if plan["fmt"] == FMT_ADDR else wJ   # row order: the plan was built without bank-aware placement
        bad = np.flatnonzero((v[rp] != wv).any(axis=1))
        _need(bad.size == 0, "F9", lambda: f"{W}: value plane of positions {_some(rp[bad])} (spins {_some(k[rp[bad]])}) is not the row's couplings "
              f"in row order: {v[rp[bad[0]]].tolist()} against {wv[bad[0]].tolist()}")
        hh = np.asarray(h, dtype=np.float64).reshape(-1)
        bad = np.flatnonzero(hv[rp] != hh[k[rp]])
        _need(bad.size == 0, "F9", lambda: f"{W}: last value plane of positions {_some(rp[bad])} is not h_k of spins {_some(k[rp[bad]])}")
    return {"levels": nlev, "depth": depth, "exact": exact, "occupied": occupied, "scale": scale, "lev": lev, "at": at, "ref": ref}


# ------------------------------------------------------------------------------------------------------------------------
# the encoder of the entry planes and array-level edits of a read-back plan: what the tests build their mutations from
# ------------------------------------------------------------------------------------------------------------------------
def encode_entries(plan, col, jq, pad):
    """[m, 8] columns / fixed-point couplings (ADDR: signs) / padding mask -> [planes, m, 4] int32."""
    m = col.shape[0]
    col, jq = col.astype(np.int64), jq.astype(np.int64)
    if plan["fmt"] == FMT_ADDR:
        ad = np.where(pad, plan["k_zero"], col + np.where(jq < 0, plan["neg_off"], 0))
        w = ad[:, 0::2] | (ad[:, 1::2] << 16)
        return w.astype(np.uint32).view(np.int32).reshape(1, m, 4)
    if plan["fmt"] == FMT_COMPACT:
        v = np.where(pad, plan["k_dummy"] << 16, (col << 16) | (jq & 0xFFFF)).astype(np.uint32).view(np.int32)
        return np.stack([v[:, :4], v[:, 4:]])
    e = np.empty((m, 16), dtype=np.int64)
    e[:, 0::2], e[:, 1::2] = np.where(pad, plan["k_dummy"], col), np.where(pad, 0, jq)
    return np.stack([e[:, 4 * q:4 * q + 4] for q in range(4)]).astype(np.int32)


def swap_positions(plan, p, q):
    """Exchange everything two schedule positions hold."""
    npos = plan["npos"]
    plan["head"][[p, q]] = plan["head"][[q, p]]
    plan["ell"][:, [p, q]] = plan["ell"][:, [q, p]]
    if plan["val"] is not None:
        v = plan["val"][:8 * npos].reshape(4, npos, 2)
        v[:, [p, q]] = v[:, [q, p]]
        hv = plan["val"][8 * npos:]
        hv[[p, q]] = hv[[q, p]]


def copy_position(plan, src, dst):
    npos = plan["npos"]
    plan["head"][dst] = plan["head"][src]
    plan["ell"][:, dst] = plan["ell"][:, src]
    if plan["val"] is not None:
        v = plan["val"][:8 * npos].reshape(4, npos, 2)
        v[:, dst] = v[:, src]
        plan["val"][8 * npos + dst] = plan["val"][8 * npos + src]


def dummy_in_level(plan, level):
    k, kind, thr, dummy, lvl = decode_heads(plan)
    d = np.flatnonzero(dummy & (lvl == level))
    return int(d[0]) if d.size else None


def rewrite_entries(plan, p, fn):
    """Decode the eight entries of position p, let fn(col, jq, pad) change them in place, encode them again."""
    col, jq, pad = decode_entries(plan)
    c, q, d = col[p:p + 1].copy(), jq[p:p + 1].copy(), pad[p:p + 1].copy()
    fn(c[0], q[0], d[0])
    plan["ell"][:, p] = encode_entries(plan, c, q, d)[:, 0]
