"""Rows of more than 8 entries in the fused windows: lane pairs (9-16 entries), lane quads (17-32) and the CSR tail beyond 32.

A graph of 512 spins -- sparse random base of mean degree 4 -- with hub rows of exactly 8, 9, 16, 17, 24, 31, 32, 33 and 40 entries
(every boundary of the 1 / 2 / 4 positions a row takes, and a tail of 1 and of 8 entries), two of the hubs adjacent.  Every case
runs on the fused windows (quads, the default), on the fused windows with NLMC_NO_QUADS=1 (a pair plus the CSR tail beyond 16) and
sweep by sweep (NLMC_NO_FUSED=1: k_sweep_philox); the three must give the same bits.  The sums are integer sums in the fixed-point
and integer-threshold modes and keep the row order in the real-valued fp64 mode, so there is no tolerance anywhere."""
import numpy as np
import pytest
import scipy.sparse as sp

from helpers import init_spins

pytestmark = pytest.mark.gpu
SEED = 0x5EED10A6
N, R, W = 512, 8, 2
HUB_DEG = (8, 9, 16, 17, 24, 31, 32, 33, 40)            # vertex v < 9 is a hub with HUB_DEG[v] neighbours
H17, H24 = 3, 4                                         # the two adjacent hubs
OUT_KEYS = ("spins", "energy", "min_energy", "argmin", "argmin_state")
BETAS = np.geomspace(0.2, 2.5, R)
# (couplings, precision, real-valued fp64 variant): address format, compact format, wide format in the f32 mode, R64
ARITH = {"pm1-f32": ("pm1", "f32", False), "pm1-f64": ("pm1", "f64", False), "int-f32": ("int", "f32", False),
         "int-f64": ("int", "f64", False), "gauss-f32": ("gauss", "f32", False), "gauss-r64": ("gauss", "f64", True)}


def hub_graph(kind, field=False, self_coupling=False):
    rng = np.random.default_rng(20251019)
    nh = len(HUB_DEG)
    edges = {(H17, H24)}
    while len(edges) < 1 + 2 * (N - nh):
        i, j = (int(x) for x in rng.integers(nh, N, 2))
        if i != j:
            edges.add((min(i, j), max(i, j)))
    for v, d in enumerate(HUB_DEG):
        for j in rng.choice(np.arange(nh, N), size=d - (1 if v in (H17, H24) else 0), replace=False):
            edges.add((v, int(j)))
    e = np.array(sorted(edges), dtype=np.int64)
    m = len(e)
    w = {"pm1": lambda: rng.choice([-1.0, 1.0], m), "int": lambda: rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], m),
         "gauss": lambda: rng.standard_normal(m)}[kind]()
    J = sp.coo_matrix((np.concatenate([w, w]), (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))), shape=(N, N))
    if self_coupling:                                   # one more entry in the row of the degree-17 hub: the DIAG kernels
        d = np.zeros(N)
        d[H17] = {"pm1": -1.0, "int": 2.0, "gauss": 0.37}[kind]
        J = J + sp.diags(d)
    J = sp.csr_matrix(J)
    J.eliminate_zeros()
    J.sort_indices()
    rows = np.diff(J.indptr)
    assert tuple(rows[:nh] - (np.arange(nh) == H17) * int(self_coupling)) == HUB_DEG and J[H17, H24] != 0
    if not field:
        h = np.zeros(N)
    elif kind == "gauss":
        h = rng.standard_normal(N) * 0.3
    else:
        h = rng.integers(-2, 3, N).astype(np.float64)
    return J, h


def positions(J, quads):
    """Schedule positions the rows of one sweep take: 1, 2 or 4 each."""
    rows = np.diff(J.indptr)
    return int(np.sum(np.where(rows > 16, 4 if quads else 2, np.where(rows > 8, 2, 1))))


def sweeps(product, J, h, T, prec, real, flags=None, outputs=False):
    """W calls of T sweeps at the ladder temperatures, a planned window each where the engine plans any."""
    with product.Engine(product.Instance(J, h), None, R) as eng:
        eng.set_fused_f64_real(real)
        eng.set_spins(init_spins(R, N))
        eng.pt_init(BETAS)
        if flags is not None:
            eng.set_flags(flags, 3.0)
        planned = eng.plan_philox_fused(0, W, T, SEED)
        kw = dict(record_stride=2, want_energy=True, want_min=True, want_state=True) if outputs else {}
        outs, lv = [], []
        for w in range(W):
            outs.append(eng.sweep_philox(T, SEED, sweep0=w * T, beta=None, precision=prec, **kw))
            st = eng.last_schedule_stats()
            lv.append(st["levels"] / max(1, st["orders"]))
        chunks = [eng.plan_levels(w) for w in range(planned)]
        return {"spins": eng.get_spins(), "E": eng.energy_tracked(), "planned": planned, "lv": lv, "outs": outs, "chunks": chunks}


def three_ways(product, monkeypatch, J, h, T, prec, real, flags=None, outputs=False):
    """Quads, NLMC_NO_QUADS=1 and sweep by sweep: the same bits."""
    q = sweeps(product, J, h, T, prec, real, flags, outputs)
    monkeypatch.setenv("NLMC_NO_QUADS", "1")
    p = sweeps(product, J, h, T, prec, real, flags, outputs)
    monkeypatch.delenv("NLMC_NO_QUADS")
    monkeypatch.setenv("NLMC_NO_FUSED", "1")
    ref = sweeps(product, J, h, T, prec, real, flags, outputs)
    monkeypatch.delenv("NLMC_NO_FUSED")
    assert q["planned"] == W and p["planned"] == W and ref["planned"] == 0
    assert max(q["lv"] + p["lv"]) < min(ref["lv"])              # the fused kernels ran (fewer levels per sweep)
    for name, got in (("quads", q), ("NLMC_NO_QUADS", p)):
        what = (name, T, prec, "outputs" if outputs else "plain")
        assert np.array_equal(got["spins"], ref["spins"]), what
        assert np.array_equal(got["E"], ref["E"]), what
        for og, orf in zip(got["outs"], ref["outs"]):
            for k in OUT_KEYS:
                assert (og[k] is None and orf[k] is None) or np.array_equal(og[k], orf[k]), what + (k,)
    return q, p


@pytest.mark.parametrize("field", [False, True], ids=["h0", "h"])
@pytest.mark.parametrize("arith", list(ARITH))
def test_hub_rows_equal_sweep_by_sweep(product, monkeypatch, arith, field):
    """All three entry formats, the f32 mode, the integer-threshold and the real-valued fp64 mode; windows of 3 and of 5 sweeps;
    plain launches (final spins, tracked energies) and per-sweep outputs (energy trace, running minimum, argmin state)."""
    kind, prec, real = ARITH[arith]
    J, h = hub_graph(kind, field)
    for T in (3, 5):
        for outputs in (False, True):
            three_ways(product, monkeypatch, J, h, T, prec, real, outputs=outputs)


@pytest.mark.parametrize("arith", ["pm1-f64", "int-f32", "gauss-f32", "gauss-r64"])
def test_self_coupling_on_a_quad(product, monkeypatch, arith):
    """A self-coupling in the row of the degree-17 hub (18 entries then): the diagonal entry sits in one lane of the quad, the
    energy must leave it out of the whole row's field."""
    kind, prec, real = ARITH[arith]
    J, h = hub_graph(kind, True, self_coupling=True)
    for T in (3, 5):
        for outputs in (False, True):
            three_ways(product, monkeypatch, J, h, T, prec, real, outputs=outputs)


@pytest.mark.parametrize("arith", ["pm1-f32", "pm1-f64", "int-f64", "gauss-f32", "gauss-r64"])
def test_phase_flags_on_the_hubs(product, monkeypatch, arith):
    """NMC phase flags in force: every hub is plain, scaled, frozen up or frozen down in some chain (a frozen group keeps its
    spin in every lane, a scaled one takes the second coefficient in every lane); the other rows a random mix."""
    kind, prec, real = ARITH[arith]
    J, h = hub_graph(kind, True)
    flags = np.random.default_rng(7).choice([0, 0, 0, 1, 2, 3], (R, N)).astype(np.uint8)
    flags[:, :len(HUB_DEG)] = (np.arange(R)[:, None] + np.arange(len(HUB_DEG))[None, :]) % 4
    for T in (3, 5):
        for outputs in (False, True):
            three_ways(product, monkeypatch, J, h, T, prec, real, flags=flags, outputs=outputs)


def rounds(product, J, h, T, n_rounds, pairs, prec, entry):
    """entry None: a sweep call and a swap call per round; "fused" / "deferred": the rounds through that entry point.
    -> spins, tracked energies, slot map, log pairs, log decisions, route."""
    with product.Engine(product.Instance(J, h), None, R) as eng:
        eng.set_spins(init_spins(R, N))
        eng.pt_init(np.linspace(0.95, 1.05, R))                 # a ladder on which swaps are accepted
        planned = eng.plan_philox_fused(0, n_rounds, T, SEED)
        eng.pt_plan(0, n_rounds, SEED, pairs)
        eng.pt_log_begin(0, n_rounds, pairs)
        if entry is None:
            for r in range(n_rounds):
                eng.sweep_philox(T, SEED, sweep0=r * T, beta=None, precision=prec)
                eng.pt_swap_philox(r, SEED, pairs, want_log=False)
        else:
            batch = eng.pt_rounds_fused if entry == "fused" else eng.pt_rounds_deferred
            assert batch(n_rounds, T, SEED, 0, 0, pairs, precision=prec), getattr(eng, "rounds_fused_refusal", "")
        lp, la = eng.pt_log_read()
        return (eng.get_spins(), eng.energy_tracked(), eng.pt_slots(), lp, la), planned, eng.last_rounds_route()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_rounds_routes(product, monkeypatch, prec):
    """4 rounds of 5 sweeps with 2 pairs selected per round on the +-1 hub graph: the rounds inside one launch (quads, and
    NLMC_NO_QUADS=1) and with a launch per round against sweep-by-sweep rounds: spins, tracked energies, slot map and swap log."""
    T, n_rounds, pairs = 5, 4, 2
    J, h = hub_graph("pm1")
    monkeypatch.setenv("NLMC_NO_FUSED", "1")
    ref, planned, _ = rounds(product, J, h, T, n_rounds, pairs, prec, None)
    monkeypatch.delenv("NLMC_NO_FUSED")
    assert planned == 0
    assert ref[4].sum() > 0 and not np.array_equal(ref[2], np.arange(R))       # swaps happened

    def same(got, what):
        for name, x, y in zip(("spins", "tracked energies", "slots", "log pairs", "log decisions"), got, ref):
            assert np.array_equal(x, y), (what, name)

    got, planned, route = rounds(product, J, h, T, n_rounds, pairs, prec, "fused")
    assert planned == n_rounds and route == "in launch"
    same(got, "in launch")
    monkeypatch.setenv("NLMC_NO_QUADS", "1")
    got, planned, route = rounds(product, J, h, T, n_rounds, pairs, prec, "fused")
    monkeypatch.delenv("NLMC_NO_QUADS")
    assert planned == n_rounds and route == "in launch"
    same(got, "in launch, NLMC_NO_QUADS")
    monkeypatch.setenv("NLMC_NO_PERSISTENT", "1")
    got, planned, route = rounds(product, J, h, T, n_rounds, pairs, prec, "deferred")
    monkeypatch.delenv("NLMC_NO_PERSISTENT")
    assert planned == n_rounds and route == "launch per round"
    same(got, "launch per round")


@pytest.mark.parametrize("T", [3, 5])
def test_plan_positions_and_depth(product, monkeypatch, T):
    """The plan's size: a window holds T x (sum over the rows of 1, 2 or 4 positions) real items, every level padded to a chunk
    of 64; moving the rows beyond 16 entries from pairs to quads changes the number of levels by at most two (the level fill
    turns a claim away only where a level is full, and which claims meet a full level depends on their order)."""
    J, h = hub_graph("pm1")
    q, p = three_ways(product, monkeypatch, J, h, T, "f64", False)
    for got, quads in ((q, True), (p, False)):
        for chunks in got["chunks"]:
            real = T * positions(J, quads)
            assert real <= 64 * int(chunks.sum()) < real + 64 * len(chunks)
    assert positions(J, True) == positions(J, False) + 2 * 6            # six hubs beyond 16 entries
    for cq, cp in zip(q["chunks"], p["chunks"]):
        assert abs(len(cq) - len(cp)) <= 2
