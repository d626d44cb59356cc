"""Planned level schedules read back (Engine.plan_items / plan_order; include/nlmc.h: nlmc_plan_get_items, nlmc_plan_get_order) and
checked item by item against the dependency rules (tests/schedcheck.py): k_levelize_fused, k_levelize and k_blv_* on worst-case
graphs built from the visiting orders themselves, each on one of the levelizers' limits.

Every case: plan (a fused plan three times, on a fresh engine each -- the planner's claims race, one plan is one sample), read back,
check every window / order; three mutations of the read-back copy must be rejected (the decode is live on the device's own bytes);
then the planned sweeps run once on 64 chains at beta about 0.4 and are compared with the sequential oracle (4 chains) and with
the route that does not use the plan (all chains).

The boundary sizes were found with the reference scheduler alone (schedcheck.reference_levels, SEED, sweep0 = 0x80000000): the path
along the order of sweep 0x80000000 has last levels 1016 / 1018 / 1023 over three sweeps at n = 1016 and 1017 / 1019 / 1024 at
n = 1017; the last spin of a complete graph's order has n - 1 earlier neighbours, 255 at K256 and 256 at K257.  Every test
asserts its numbers on the reference before it asks the device."""

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
import schedcheck as sc
from helpers import init_spins

pytestmark = pytest.mark.gpu
SEED = 0xA5A50000
S0 = 0x80000000                      # bit 31 set: the sweep index is an unsigned 32-bit counter word
R = 64
KNOBS = ("NLMC_NO_LEVEL_FILL", "NLMC_NO_QUADS", "NLMC_NO_BANK_AWARE", "NLMC_FUSED_WORKERS", "NLMC_FORCE_BIG", "NLMC_BIG_PER_LEVEL",
         "NLMC_SWEEP_NT", "NLMC_NO_FUSED")
PATH_PLANNED, PATH_REFUSED = 1016, 1017


def set_knobs(monkeypatch, env):
    """The knobs are read when an engine is created."""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, str(v))


def betas(chains):
    return np.linspace(0.36, 0.44, chains)


# ------------------------------------------------------------------------------------------------------------------------
# graphs (+-J unless said otherwise)
# ------------------------------------------------------------------------------------------------------------------------
def sym(n, i, j, rng=None, values=None):
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    keep = i != j
    A = sp.coo_matrix((np.ones(int(keep.sum())), (np.minimum(i, j)[keep], np.maximum(i, j)[keep])), shape=(n, n)).tocsr()
    U = sp.triu(A, 1).tocsr()
    U.sum_duplicates()
    rng = rng or np.random.default_rng(n)
    U.data = rng.choice([-1.0, 1.0], size=U.nnz) if values is None else values(rng, U.nnz)
    J = (U + U.T).tocsr()
    J.sort_indices()
    return J


def visit_order(n, sweep):
    """Spins in the order sweep `sweep` visits them."""
    return np.argsort(sc.window_orders(n, sweep, 1, 0, SEED)[0])


def complete(n):
    i, j = np.triu_indices(n, 1)
    return sym(n, i, j)


def path(n, sweep=S0):
    by = visit_order(n, sweep)
    return sym(n, by[:-1], by[1:])


def star(n, degree, hub_first, sweep=S0):
    by = visit_order(n, sweep)
    hub = by[0] if hub_first else by[-1]
    leaves = np.setdiff1d(np.arange(n), [hub])[:degree]
    return sym(n, np.full(degree, hub), leaves)


def bipartite(a, b):
    i, j = np.meshgrid(np.arange(a), np.arange(a, a + b), indexing="ij")
    return sym(a + b, i.reshape(-1), j.reshape(-1))


def matchings_and_hubs(n=512):
    """Nine random perfect matchings (rows of 9 entries: lane pairs) and 10 hubs of 19 entries (quads; pairs with a CSR tail under
    NLMC_NO_QUADS)."""
    rng = np.random.default_rng(512)
    pr = [rng.permutation(n) for _ in range(9)]
    i, j = np.concatenate([p[0::2] for p in pr]), np.concatenate([p[1::2] for p in pr])
    J = sym(n, i, j, rng)
    hubs = rng.choice(n, 10, replace=False)
    A = J.tolil()
    for hb in hubs:
        free = np.setdiff1d(np.arange(n), np.concatenate([[hb], hubs, A.rows[hb]]))
        for q in rng.choice(free, 19 - len(A.rows[hb]), replace=False):
            A[hb, q] = A[q, hb] = rng.choice([-1.0, 1.0])
    J = A.tocsr()
    J.sort_indices()
    deg = np.diff(J.indptr)
    assert (deg[hubs] == 19).all() and (deg > 8).mean() > 0.9 and deg.max() == 19
    return J


def degree6(n, couplings):
    """Degree-6 random graph with two stored diagonals; Gaussian fields with Gaussian couplings (nothing a multiple of a power of
    two: an fp64-real plan carries the value plane), fields in {-1, 0, 1} otherwise (the 2- and 4-byte entry formats need the
    instance's fixed-point scale small, which a real field rules out)."""
    rng = np.random.default_rng(300)
    values = {"pmj": None, "int3": lambda g, m: g.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], size=m), "gauss": lambda g, m: g.normal(size=m)}[couplings]
    J = sym(n, np.repeat(np.arange(n), 3), rng.integers(0, n, 3 * n), rng, values).tolil()
    J[11, 11], J[200, 200] = (1.0, -1.0) if couplings != "gauss" else (0.375, -1.3)
    J = J.tocsr()
    J.sort_indices()
    return J, rng.normal(size=n) if couplings == "gauss" else rng.integers(-1, 2, n).astype(np.float64)


def max_preceding(A, pos):
    """Largest number of neighbours that precede a spin in one of the orders pos [T, n]."""
    ek, ej = sc._edges(A)
    return max(int(np.bincount(ek[p[ej] < p[ek]], minlength=A.shape[0]).max()) if ek.size else 0 for p in pos)


# ------------------------------------------------------------------------------------------------------------------------
# fused windows
# ------------------------------------------------------------------------------------------------------------------------
def mutations_rejected(plan, J, h, w, kw):
    """One level move, one dropped entry (one dropped item where the graph has no entry), one send error on the read-back copy."""
    import copy
    res = sc.check_fused(plan, J, h, w, **kw)
    lev, at = res["lev"], res["at"]
    A = sc.csr_of(J)
    lanes = sc.lanes_of(np.diff(A.indptr), plan["quads"])[0]
    # level move: the group of (1, k) changes places with a group of the level of (0, k) -- (0, k) itself where it stands alone
    k = 0
    same = np.flatnonzero((lev[0] == lev[0, k]) & (lanes == lanes[k]) & (np.arange(A.shape[0]) != k))
    k2 = int(same[0]) if same.size else k
    m = copy.deepcopy(plan)
    for lane in range(int(lanes[k])):
        sc.swap_positions(m, at[1, k] + lane, at[0, k2] + lane)
    with pytest.raises(sc.ScheduleError) as e:
        sc.check_fused(m, J, h, w, **kw)
    assert e.value.rule in ("F2", "F3", "F4", "F5"), str(e.value)
    # dropped entry
    m = copy.deepcopy(plan)
    if A.nnz:
        col, jq, pad = sc.decode_entries(plan)
        p = int(np.flatnonzero(~pad.all(axis=1))[0])
        sc.rewrite_entries(m, p, lambda c, q, d: d.__setitem__(int(np.flatnonzero(~d)[0]), True))
        rule = "F8"
    else:
        sc.copy_position(m, int(np.flatnonzero(sc.decode_heads(plan)[3])[0]) if sc.decode_heads(plan)[3].any() else int(at[0, 1]), int(at[0, 0]))
        rule = "F1"
    with pytest.raises(sc.ScheduleError) as e:
        sc.check_fused(m, J, h, w, **kw)
    assert e.value.rule == rule, str(e.value)
    # send error
    m = copy.deepcopy(plan)
    m["send"][1] += 1
    with pytest.raises(sc.ScheduleError) as e:
        sc.check_fused(m, J, h, w, **kw)
    assert e.value.rule == "F5", str(e.value)


def fused_case(product, monkeypatch, J, h, T, env=None, sweep0=S0, W=2, real64=False, expect=None):
    """Plans W windows three times and checks each; runs them once.  expect: windows that get a schedule (default: derived from the
    reference -- depth at most 1023 levels, at most 255 earlier neighbours); -> figures of the last plan's checks."""
    env = dict(env or {})
    A = sc.csr_of(J)
    n = A.shape[0]
    h = np.zeros(n) if h is None else h
    inst = product.Instance(J, h)
    nofill = "NLMC_NO_LEVEL_FILL" in env
    pos = [sc.window_orders(n, sweep0, T, w, SEED) for w in range(W)]
    ref = [sc.reference_levels(A, p) for p in pos]
    want = [bool(r.max() <= sc.LCAP - 1 and max_preceding(A, p) <= 255) for p, r in zip(pos, ref)]
    assert expect is None or want == list(expect), (want, [int(r.max()) for r in ref], [max_preceding(A, p) for p in pos])
    m0 = init_spins(R, n)
    prec = "f64" if real64 else "f32"
    figures, got = [], None
    set_knobs(monkeypatch, env)
    for rep in range(3):
        with product.Engine(inst, None, R) as eng:
            if real64:
                eng.set_fused_f64_real(True)
            eng.set_spins(m0)
            E0 = eng.energy()
            eng.pt_init(betas(R))
            assert eng.plan_philox_fused(sweep0, W, T, SEED) == sum(want)
            for w in range(W):
                plan = eng.plan_items(w)
                assert (plan["nlev"] > 0) == want[w], (w, plan["nlev"])
                if not want[w]:
                    continue
                assert plan["T"] == T and plan["sweep0"] == sweep0 and plan["seed"] == SEED and plan["has_val"] == int(real64)
                assert plan["quads"] == int("NLMC_NO_QUADS" not in env) and plan["level_fill"] == int(not nofill)
                assert plan["bank_aware"] == int("NLMC_NO_BANK_AWARE" not in env and not real64)
                kw = dict(nofill=nofill, pos=pos[w], ref=ref[w])
                r = sc.check_fused(plan, J, h, w, **kw)
                figures.append({k: r[k] for k in ("levels", "depth", "exact", "occupied")} | {"cap": 64 * plan["workers"], "fmt": plan["fmt"]})
                if rep == 0 and (w == 0 or not want[0]):
                    mutations_rejected(plan, J, h, w, kw)
            if rep == 0:
                for w in range(W):
                    eng.sweep_philox(T, SEED, sweep0=sweep0 + w * T, beta=None, precision=prec)
                    assert eng._last_fused() is want[w], w
                got = (eng.get_spins(), eng.energy() if real64 else eng.energy_tracked(), E0, eng.energy_scale)
    set_knobs(monkeypatch, {"NLMC_NO_FUSED": 1})
    with product.Engine(inst, None, R) as eng:
        eng.set_spins(m0)
        eng.pt_init(betas(R))
        eng.sweep_philox(W * T, SEED, sweep0=sweep0, beta=None, precision=prec)
        assert not eng._last_fused()
        assert np.array_equal(eng.get_spins(), got[0])
        assert np.array_equal(eng.energy() if real64 else eng.energy_tracked(), got[1])
    assert not np.array_equal(got[0], m0)
    csr = oracle.Csr(J)
    for c in (0, 1, R // 2, R - 1):
        cb = np.tile(np.array(oracle.cb_pair(betas(R)[c], 1.0, real64)), (W * T, 1))
        _, s_fin, tr = oracle.sweeps_philox(csr, h, m0[c], cb, SEED, c, sweep0=sweep0, escale=got[3], use_f64=real64,
                                            efix0=int(np.rint(got[2][c] * 2.0 ** got[3])), want_M=False)
        assert np.array_equal(got[0][c], s_fin), f"chain {c}"
        if not real64:
            assert got[1][c] == tr[-1] * 2.0 ** -got[3], f"chain {c}"
    print(figures[-W:] if figures else "nothing planned")
    return figures


BANK = pytest.mark.parametrize("bank", [{}, {"NLMC_NO_BANK_AWARE": 1}], ids=["bank-aware", "row-order"])


@BANK
def test_complete_graph_255_earlier_neighbours(product, monkeypatch, bank):
    """K256, T = 3: every row a quad with a CSR tail; the last spin of every order waits for 255 neighbours (the 8-bit counter at its
    maximum); 768 levels of one item, last levels 256 / 512 / 768."""
    J = complete(256)
    pos = sc.window_orders(256, S0, 3, 0, SEED)
    assert max_preceding(sc.csr_of(J), pos) == 255
    assert sc.reference_levels(sc.csr_of(J), pos).max(axis=1).tolist() == [256, 512, 768]
    f = fused_case(product, monkeypatch, J, None, 3, bank, expect=(True, True))
    assert all(x["levels"] == 768 and x["exact"] for x in f)


@BANK
@pytest.mark.parametrize("n,T", [(256, 4), (257, 3)])
def test_complete_graph_refused(product, monkeypatch, bank, n, T):
    """K256 with T = 4 is 1024 levels deep, K257 has a spin with 256 earlier neighbours: nothing is planned, and the sweeps equal
    the oracle sweep by sweep."""
    J = complete(n)
    pos = sc.window_orders(n, S0, T, 0, SEED)
    assert max_preceding(sc.csr_of(J), pos) == n - 1 and sc.reference_levels(sc.csr_of(J), pos).max() == n * T
    assert fused_case(product, monkeypatch, J, None, T, bank, expect=(False, False)) == []


# Behind the end of the path's sweep (level n) the whole third sweep becomes ready within seven levels, up to 390 positions in one:
# at the default workgroup of four waves (cap 192) level fill moves updates back and the depth depends on the race.  Twelve waves
# (cap 704) hold every level of the reference, so the plan is the reference's level for level and the boundary is exact.
WIDE_WG = {"NLMC_SWEEP_NT": 768}


@BANK
def test_path_along_the_order_1023_levels(product, monkeypatch, bank):
    """n = 1016: the first window is exactly 1023 levels deep and planned, level for level the reference's."""
    J = path(PATH_PLANNED)
    ref = sc.reference_levels(sc.csr_of(J), sc.window_orders(PATH_PLANNED, S0, 3, 0, SEED))
    assert ref.max(axis=1).tolist() == [1016, 1018, 1023]
    f = fused_case(product, monkeypatch, J, None, 3, {**bank, **WIDE_WG}, expect=(True, True))
    assert f[-2]["levels"] == 1023 and f[-2]["cap"] == 704 and f[-2]["exact"] and f[-1]["exact"]


@BANK
def test_path_along_the_order_1024_levels(product, monkeypatch, bank):
    """n = 1017: 1024 levels, the first window is refused; the second one (another order: a dozen levels) is planned."""
    J = path(PATH_REFUSED)
    ref = sc.reference_levels(sc.csr_of(J), sc.window_orders(PATH_REFUSED, S0, 3, 0, SEED))
    assert ref.max(axis=1).tolist() == [1017, 1019, 1024]
    fused_case(product, monkeypatch, J, None, 3, {**bank, **WIDE_WG}, expect=(False, True))


@BANK
@pytest.mark.parametrize("n", [1024, 256])
@pytest.mark.parametrize("fill", [{}, {"NLMC_NO_LEVEL_FILL": 1}], ids=["fill", "no-fill"])
def test_edgeless(product, monkeypatch, bank, n, fill):
    """No entry at all: every update of a sweep is ready at once and claims room in one level (add and undo at its worst); the
    levels of the split are exactly at the cap, and only the spin's own order and the three tables order anything.  With level fill a
    sweep's last level takes updates of the next sweep and a claim may be turned away from a level that had room, so the count is
    bounded by the positions only."""
    J = sp.csr_matrix((n, n))
    f = fused_case(product, monkeypatch, J, None, 3, {**bank, **fill}, expect=(True, True))
    for x in f:
        assert x["cap"] == 192 and x["depth"] == 3 and x["levels"] >= -(-3 * n // 192)
        assert not fill or x["levels"] == 3 * -(-n // 192)


@BANK
@pytest.mark.parametrize("degree,hub_first", [(200, True), (200, False), (255, True), (255, False), (256, False)])
def test_star(product, monkeypatch, bank, degree, hub_first):
    """n = 512: a TAIL row.  Hub first: every leaf is ready in one pass behind it; hub last: it waits for every leaf, 255 of them at
    the counter's maximum -- and with 256 the window of that sweep is refused."""
    J = star(512, degree, hub_first)
    fused_case(product, monkeypatch, J, None, 3, bank, expect=None if degree < 256 else (False, True))


def test_complete_bipartite(product, monkeypatch):
    """K16,240: TAIL rows of 240 entries against pairs of 16; two-level sweeps of maximal width."""
    fused_case(product, monkeypatch, bipartite(16, 240), None, 3, expect=(True, True))


@pytest.mark.parametrize("quads", [{}, {"NLMC_NO_QUADS": 1}], ids=["quads", "no-quads"])
def test_matchings_and_hubs_overflow_the_cap(product, monkeypatch, quads):
    """n = 512: nearly every item a pair, more than 1000 positions per sweep.  A workgroup of four waves has three workers whatever
    NLMC_FUSED_WORKERS says (8 is the least the knob takes), a cap of 192; the reference's widest level holds 106 positions at this
    size, so nothing overflows and the plan is the reference's level for level (the pairs that do overflow: the next test)."""
    f = fused_case(product, monkeypatch, matchings_and_hubs(), None, 3, {"NLMC_FUSED_WORKERS": 8, **quads}, expect=(True, True))
    assert all(x["cap"] == 192 and x["exact"] for x in f)


@pytest.mark.parametrize("fill", [{}, {"NLMC_NO_LEVEL_FILL": 1}], ids=["fill", "no-fill"])
def test_pairs_overflow_the_cap(product, monkeypatch, fill):
    """K9,255 with the nine hubs first in the order of sweep S0: behind them 255 rows of nine entries are ready at once, 510 positions
    of lane pairs claimed two at a time against a cap of 192 (and every hub has at most 255 earlier neighbours in the other sweeps)."""
    n = 264
    by = visit_order(n, S0)
    i, j = np.meshgrid(by[:9], by[9:], indexing="ij")
    J = sym(n, i.reshape(-1), j.reshape(-1))
    f = fused_case(product, monkeypatch, J, None, 3, fill, expect=(True, True))
    assert not f[-2]["exact"] or fill


@pytest.mark.parametrize("couplings,fmt,real64", [("gauss", sc.FMT_WIDE, False), ("gauss", sc.FMT_WIDE, True), ("pmj", sc.FMT_ADDR, False),
                                                  ("int3", sc.FMT_COMPACT, False)])
def test_entry_formats_diagonal_and_value_plane(product, monkeypatch, couplings, fmt, real64):
    """n = 300, two stored diagonals: the three entry formats, and the fp64-real plan with its value plane (entries in row order).
    The value plane only ever comes with 8-byte entries: a plan carries it when the couplings or fields are no multiples of the
    fixed-point grain, and the scale such an instance gets leaves no coupling in 16 bits."""
    J, h = degree6(300, couplings)
    f = fused_case(product, monkeypatch, J, h, 4, real64=real64, expect=(True, True))
    assert all(x["fmt"] == fmt for x in f)


def test_read_back_errors(product, monkeypatch):
    set_knobs(monkeypatch, {})
    J, h = degree6(300, "pmj")
    with product.Engine(J, h, 2) as eng:
        with pytest.raises(RuntimeError, match="no such planned"):
            eng.plan_items(0)
        with pytest.raises(RuntimeError, match="no such planned"):
            eng.plan_order(0)
        assert eng.plan_philox_fused(0, 2, 3, SEED) == 2
        eng.plan_philox(0, 2, SEED)
        for bad in (-1, 2):
            with pytest.raises(RuntimeError, match="no such planned"):
                eng.plan_items(bad)
            with pytest.raises(RuntimeError, match="no such planned"):
                eng.plan_order(bad)
        import ctypes
        info = np.zeros(24, dtype=np.int64)
        small = np.zeros((64, 4), dtype=np.int32)
        rc = eng._L.nlmc_plan_get_items(eng._ctx, 0, product._abi.ptr(info), product._abi.ptr(small), product._abi.ptr(small), None,
                                        product._abi.ptr(np.zeros(1025, np.int32)), product._abi.ptr(np.zeros(64, np.int32)), ctypes.c_int64(64))
        assert rc == product._abi.ERR_ARG and info[14] > 64
        rc = eng._L.nlmc_plan_get_order(eng._ctx, 0, product._abi.ptr(info), product._abi.ptr(small), product._abi.ptr(small), ctypes.c_int64(64))
        assert rc == product._abi.ERR_ARG


# ------------------------------------------------------------------------------------------------------------------------
# per-sweep plans
# ------------------------------------------------------------------------------------------------------------------------
LDS, BIG = {}, {"NLMC_FORCE_BIG": 1, "NLMC_BIG_PER_LEVEL": 0}
LEVELIZER = pytest.mark.parametrize("lev", [LDS, BIG], ids=["lds", "global"])


def order_case(product, monkeypatch, J, env, chains=R, sweeps=3, sweep0=S0, orders=3, cap=None):
    A = sc.csr_of(J)
    n = A.shape[0]
    h = np.zeros(n)
    inst = product.Instance(J, h)
    m0 = init_spins(chains, n)
    big = "NLMC_FORCE_BIG" in env
    set_knobs(monkeypatch, env)
    figures = []
    with product.Engine(inst, None, chains) as eng:
        eng.set_spins(m0)
        E0 = eng.energy()
        eng.pt_init(betas(chains))
        eng.plan_philox(sweep0, orders, SEED)
        for o in range(orders):
            plan = eng.plan_order(o)
            assert plan["big"] is big and plan["orders"] == orders and plan["sweep0"] == sweep0
            if cap is not None:
                assert plan["cap"] == (0 if big else cap)
            pos = sc.window_orders(n, sweep0, 1, o, SEED)[0]
            figures.append(sc.check_order(plan, J, pos, name=f"order {o}"))
            if o == 0:
                import copy
                m = copy.deepcopy(plan)
                m["order"][0] = m["order"][n - 1]            # one spin twice, one missing
                with pytest.raises(sc.ScheduleError) as e:
                    sc.check_order(m, J, pos)
                assert e.value.rule == "P1", str(e.value)
                ek, ej = sc._edges(A)
                dep = np.flatnonzero(pos[ej] < pos[ek])
                if dep.size:                                 # two spins exchanged across a dependent pair
                    spin = plan["order"][:, 0].astype(np.int64) & (0xFFFFFFFF if big else 0xFFFF)
                    a, b = int(np.flatnonzero(spin == ek[dep[0]])[0]), int(np.flatnonzero(spin == ej[dep[0]])[0])
                    m = copy.deepcopy(plan)
                    m["order"][[a, b]] = m["order"][[b, a]]
                    with pytest.raises(sc.ScheduleError) as e:
                        sc.check_order(m, J, pos)
                    assert e.value.rule == "P3", str(e.value)
        eng.sweep_philox(sweeps, SEED, sweep0=sweep0, beta=None)
        got, Et, esc = eng.get_spins(), eng.energy_tracked(), eng.energy_scale
    with product.Engine(inst, None, chains) as eng:          # no plan: the call builds its own schedule
        eng.set_spins(m0)
        eng.pt_init(betas(chains))
        eng.sweep_philox(sweeps, SEED, sweep0=sweep0, beta=None)
        assert np.array_equal(eng.get_spins(), got) and np.array_equal(eng.energy_tracked(), Et)
    csr = oracle.Csr(J)
    for c in sorted({0, 1, chains // 2, chains - 1}):
        cb = np.tile(np.array(oracle.cb_pair(betas(chains)[c])), (sweeps, 1))
        _, s_fin, tr = oracle.sweeps_philox(csr, h, m0[c], cb, SEED, c, sweep0=sweep0, escale=esc, efix0=int(np.rint(E0[c] * 2.0 ** esc)), want_M=False)
        assert np.array_equal(got[c], s_fin) and Et[c] == tr[-1] * 2.0 ** -esc, f"chain {c}"
    print(figures)
    return figures


def test_order_path_depth_n(product, monkeypatch):
    """Path along the order, n = 300: the LDS levelizer's relaxation runs to its last iteration."""
    f = order_case(product, monkeypatch, path(300), LDS)
    assert f[0]["levels"] == 300


@LEVELIZER
@pytest.mark.parametrize("n", [2047, 2048, 2049])
def test_order_path_at_the_histogram_edge(product, monkeypatch, lev, n):
    """Depth n around the 2048 LDS bins of k_blv_hist / k_blv_place (and the same on the LDS levelizer); 8 chains, 1 sweep."""
    f = order_case(product, monkeypatch, path(n), lev, chains=8, sweeps=1)
    assert f[0]["levels"] == n


@LEVELIZER
def test_order_edgeless_small_cap(product, monkeypatch, lev):
    """n = 5000 without an entry, sweep workgroups of 64 threads: one level cut into 79 (the global-memory form publishes it whole)."""
    f = order_case(product, monkeypatch, sp.csr_matrix((5000, 5000)), {**lev, "NLMC_SWEEP_NT": 64}, cap=64)
    assert all(x["earliest"] == 1 and x["levels"] == (1 if lev else 79) for x in f)


@LEVELIZER
def test_order_matchings_and_hubs(product, monkeypatch, lev):
    """Long rows at the front of their levels on the LDS form; hi_max == n on the global-memory form."""
    order_case(product, monkeypatch, matchings_and_hubs(), lev)


def test_order_star_second_tile(product, monkeypatch):
    """n = 4097 under NLMC_FORCE_BIG: k_blv_hist / k_blv_place run a second tile of one spin; the hub, last in the order, stands alone
    in the last level."""
    J = star(4097, 4096, False)
    f = order_case(product, monkeypatch, J, BIG)
    assert f[0] == {"levels": 2, "earliest": 2}
