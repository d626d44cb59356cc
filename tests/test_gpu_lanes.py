"""Chain-per-lane sweeps (include/nlmc.h: nlmc_set_lane_sweeps; csrc/nlmc_lanes.h) against the sweep-by-sweep route and the oracle.

Every case runs the same call twice on one engine, set_lane_sweeps("off") then ("force"), from the same start state: every output
(recorded spins, energy trace, min_energy, argmin, argmin_state, final spins, energy_tracked()) is equal bit for bit, and
last_sweep_route() says "stepwise", then "lanes".  Named chains are also compared with oracle.sweeps_philox, as
test_gpu_sweep.test_philox_mode_bit_exact_vs_oracle does.  The shapes are the smallest at which the lane kernel can go wrong: a
lane tail and several blocks, chains shorter than a Philox block of four, a complete graph, diagonal entries, the size limit with
flags in LDS, every temperature source, every output, chain subsets, more than one window of visiting orders."""
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN
from helpers import make_instance, init_spins, DeviceBuffer

pytestmark = pytest.mark.gpu
SEED = 0xA5A50000 + (7 << 32)          # high bits set
OUT_KEYS = ("spins", "energy", "min_energy", "argmin", "argmin_state")
ALL_OUT = dict(record_stride=1, want_energy=True, want_min=True, want_state=True)
INST = os.path.join(GOLDEN, "instances")


def dense_instance(n, seed, diag=False):
    """Complete graph: symmetric Gaussian couplings scaled to max |J| = 1, Gaussian fields (optionally a non-zero diagonal)."""
    r = np.random.default_rng(seed)
    A = r.standard_normal((n, n))
    J = np.triu(A, 1)
    J = J + J.T
    if diag:
        J[np.arange(n), np.arange(n)] = r.standard_normal(n)
    J /= np.max(np.abs(J))
    return J, 0.3 * r.standard_normal(n)


def wishart(P, i=1):
    fn = f"wishart_planting_N_10_alpha_0.50_inst_{i}.txt"
    W, _ = P.instances.txt_to_A_wishart(os.path.join(INST, "wishart_N10_a0.50__" + fn))
    J = (-W).toarray()                         # NMC/examples/wishart_example.py: J = -W, h = 0
    nf = float(np.max(np.abs(J)))              # ... and run() divides by max |J|
    gs = {l.split()[0]: float(l.split()[1]) for l in open(os.path.join(INST, "wishart_N10_a0.50__gs_energies.txt"))}
    return J / nf, np.zeros(J.shape[0]), nf, gs[fn]


def run_both(eng, m0, call, prepare=None, modes=("off", "force")):
    """`call(eng)` under each lane mode from the same start state (spins, re-synchronised energies, whatever `prepare` sets)."""
    res = []
    for mode in modes:
        eng.set_lane_sweeps(mode)
        eng.set_spins(m0)
        E0 = eng.energy()
        if prepare:
            prepare(eng)
        o = call(eng)
        res.append({"o": o, "route": eng.last_sweep_route(), "final": eng.get_spins(), "tracked": eng.energy_tracked(), "E0": E0,
                    "fused": eng._last_fused(), "stats": eng.last_schedule_stats()})
    return res


def assert_same(a, b, routes=("stepwise", "lanes")):
    assert (a["route"], b["route"]) == routes
    for k in OUT_KEYS:
        if a["o"][k] is None:
            assert b["o"][k] is None
        else:
            assert np.array_equal(a["o"][k], b["o"][k]), k
    assert np.array_equal(a["final"], b["final"])
    assert np.array_equal(a["tracked"], b["tracked"])
    if b["route"] == "lanes":
        assert not b["fused"] and b["stats"]["levels"] == 0 and b["stats"]["orders"] > 0


def assert_oracle(J, h, m0, res, chains, beta_of, S, esc, f64, order, sweep0=0, chain_base=0, flags=None, temp_x=1.0, seed=SEED):
    """res: one run with all outputs; beta_of(c) -> [S] inverse temperatures of chain c."""
    csr = oracle.Csr(J)
    o = res["o"]
    for c in chains:
        gc = c + chain_base
        cb = np.array([oracle.cb_pair(b, temp_x, f64) for b in beta_of(c)])
        ef0 = int(np.rint(res["E0"][c] * 2.0 ** esc))
        M, s_fin, tr = oracle.sweeps_philox(csr, h, m0[c], cb, seed, gc, order_group=(gc + 1 if order == "per_chain" else 0), sweep0=sweep0,
                                            flags=None if flags is None else flags[c], escale=esc, use_f64=f64, efix0=ef0)
        assert np.array_equal(o["spins"][c], M), f"chain {c}"
        assert np.array_equal(res["final"][c], s_fin)
        assert np.array_equal(o["energy"][c], tr.astype(np.float64) * 2.0 ** -esc)
        am = int(np.argmin(tr))
        assert o["argmin"][c] == am and o["min_energy"][c] == tr[am] * 2.0 ** -esc
        assert np.array_equal(o["argmin_state"][c], M[am])
        assert res["tracked"][c] == tr[-1] * 2.0 ** -esc


@pytest.mark.parametrize("order", ["shared", "per_chain"])
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("rows,rng", [(1, None), (63, None), (65, None), (130, None), (65, "0"), (65, "1")],
                         ids=["1", "63", "65", "130", "65-rng0", "65-rng1"])
def test_lane_tail_and_blocks(product, rows, rng, precision, order, monkeypatch):
    """rng: NLMC_LANE_RNG (read when the engine is created) -- the Philox call per update, or the table per sweep; None: the default."""
    if rng is not None:
        monkeypatch.setenv("NLMC_LANE_RNG", rng)
    J, h = make_instance(37, seed=9, with_h=True, gaussian=True)
    S, N, f64 = 5, 37, precision == "f64"
    m0 = init_spins(rows, N)
    betas = np.linspace(0.2, 3.0, rows)
    with product.Engine(J, h, rows, chain_base=3, n_chains_global=rows + 3) as eng:
        esc = eng.energy_scale
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, sweep0=5, beta=np.repeat(betas[:, None], S, axis=1),
                                                          precision=precision, order=order, **ALL_OUT))
    assert_same(a, b)
    assert b["stats"]["orders"] == (S * rows if order == "per_chain" else S)
    assert_oracle(J, h, m0, b, [c for c in (0, 62, 64, 129) if c < rows], lambda c: np.full(S, betas[c]), S, esc, f64, order, sweep0=5,
                  chain_base=3)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n", [2, 5, 10])
def test_chains_shorter_than_a_philox_block(product, n, precision):
    J, h = dense_instance(n, 40 + n)
    R, S, f64 = 70, 5, precision == "f64"
    m0 = init_spins(R, n)
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=0.9, precision=precision, **ALL_OUT))
    assert_same(a, b)
    assert_oracle(J, h, m0, b, (0, 3, 69), lambda c: np.full(S, 0.9), S, esc, f64, "shared")


@pytest.mark.parametrize("order", ["shared", "per_chain"])
def test_complete_graph_of_the_reference(product, order):
    J, h, _, _ = wishart(product, 1)
    R, S = 128, 6
    m0 = init_spins(R, 10)
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=3.0, precision="f64", order=order, **ALL_OUT))
    assert_same(a, b)
    assert_oracle(J, h, m0, b, (0, 64, 127), lambda c: np.full(S, 3.0), S, esc, True, order)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_diagonal_entries(product, precision):
    J, h = dense_instance(24, 77, diag=True)
    R, S, f64 = 66, 6, precision == "f64"
    m0 = init_spins(R, 24)
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=1.1, precision=precision, **ALL_OUT))
        eng.set_spins(b["final"])
        E_exact = eng.energy()
    assert_same(a, b)
    assert_oracle(J, h, m0, b, (0, 65), lambda c: np.full(S, 1.1), S, esc, f64, "shared")
    # the tracked energies leave the diagonal out of every delta: they stay with the recomputed ones (test_gpu_sweep.py's bound)
    assert np.all(np.abs(b["tracked"] - E_exact) <= (1e-4 if not f64 else 1e-9) * np.maximum(1.0, np.abs(E_exact)))


def nmc_flags(R, N, m0, seed=1):
    r = np.random.default_rng(seed)
    flags = np.zeros((R, N), np.uint8)
    for c in range(R):
        cl = r.random(N) < 0.2
        if c % 2 == 0:          # phase C: clusters scaled, the rest frozen at its start value
            flags[c, cl] = 1
            flags[c, ~cl] = np.where(m0[c, ~cl] > 0, 2, 3)
        else:                   # phase NC: clusters frozen
            flags[c, cl] = np.where(m0[c, cl] > 0, 2, 3)
    return flags


def test_size_limit_with_flags(product):
    N, R, S = 1024, 66, 3
    J, h = make_instance(N, seed=21, with_h=True)
    m0 = init_spins(R, N)
    flags = nmc_flags(R, N, m0)
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=2.0, **ALL_OUT), prepare=lambda e: e.set_flags(flags, 20.0))
    assert_same(a, b)
    assert_oracle(J, h, m0, b, (0, 65), lambda c: np.full(S, 2.0), S, esc, False, "shared", flags=flags, temp_x=20.0)
    frozen = flags >= 2
    assert np.array_equal(b["final"][frozen], m0[frozen])


def test_one_spin_past_the_size_limit_runs_as_before(product):
    N, R, S = 1025, 3, 3
    J, h = make_instance(N, seed=22)
    m0 = init_spins(R, N)
    with product.Engine(J, h, R) as eng:
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=1.5, **ALL_OUT))
    assert_same(a, b, routes=("stepwise", "stepwise"))


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_phase_flags(product, precision):
    N, R, S, f64 = 96, 70, 6, precision == "f64"
    J, h = make_instance(N, seed=3, with_h=True)
    m0 = init_spins(R, N)
    flags = nmc_flags(R, N, m0)
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, 99, beta=2.0, precision=precision, **ALL_OUT),
                        prepare=lambda e: e.set_flags(flags, 20.0))
    assert_same(a, b)
    assert_oracle(J, h, m0, b, (0, 1, 68, 69), lambda c: np.full(S, 2.0), S, esc, f64, "shared", flags=flags, temp_x=20.0, seed=99)
    frozen = flags >= 2
    assert np.array_equal(b["final"][frozen], m0[frozen])


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_temperature_per_sweep(product, precision):
    N, R, S, f64 = 40, 70, 6, precision == "f64"
    J, h = dense_instance(N, 5)
    m0 = init_spins(R, N)
    tab = np.linspace(0.1, 2.0, R)[:, None] * np.linspace(0.5, 1.5, S)[None, :]        # distinct columns
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=tab, precision=precision, **ALL_OUT))
    assert_same(a, b)
    assert_oracle(J, h, m0, b, (0, 69), lambda c: tab[c], S, esc, f64, "shared")


@pytest.mark.parametrize("order", ["shared", "per_chain"])
def test_ladder_temperatures(product, order):
    N, R, S = 40, 70, 5
    J, h = dense_instance(N, 6)
    m0 = init_spins(R, N)
    betas = np.geomspace(0.1, 3.0, R)
    slots = np.random.default_rng(4).permutation(R).astype(np.int32)                   # chain c sits on slot slots[c]
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        eng.pt_init(betas)
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=None, order=order, **ALL_OUT), prepare=lambda e: e.pt_set_slots(slots))
    assert_same(a, b)
    assert not np.array_equal(slots, np.arange(R))
    assert_oracle(J, h, m0, b, (0, 1, 69), lambda c: np.full(S, betas[slots[c]]), S, esc, False, order)


@pytest.mark.parametrize("record_stride", [1, 3])
def test_outputs(product, record_stride):
    J, h = make_instance(128, seed=12, with_h=True, gaussian=True)
    N, R, S = 128, 70, 7
    m0 = init_spins(R, N)
    betas = np.repeat(np.linspace(0.3, 2.5, R)[:, None], S, axis=1)
    with product.Engine(J, h, R) as eng:
        buf = DeviceBuffer(np.zeros(R))
        eng.set_energy_sink(buf.ptr.value)
        sinks = []

        def call(e):
            o = e.sweep_philox(S, SEED, beta=betas, record_stride=record_stride, want_energy=True, want_min=True, want_state=True)
            sinks.append(buf.read(R))
            return o
        a, b = run_both(eng, m0, call)
        assert_same(a, b)
        assert b["o"]["spins"].shape == (R, (S + record_stride - 1) // record_stride, N)
        assert np.array_equal(sinks[0], a["tracked"]) and np.array_equal(sinks[1], b["tracked"])
        assert np.array_equal(b["o"]["energy"][:, -1], b["tracked"])
        assert np.array_equal(b["o"]["min_energy"], b["o"]["energy"].min(axis=1))
        assert np.array_equal(b["o"]["argmin"], b["o"]["energy"].argmin(axis=1))
        # only the minimum and its state, nothing per sweep handed back
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=betas, want_min=True, want_state=True))
        assert_same(a, b)
        # running minimum kept on the device over sweeps 0, 2, 4, ...; the argmin state adopted afterwards
        def tracked_call(e):
            e.track_minimum(True, stride=2)
            o = e.sweep_philox(S, SEED, beta=betas, want_energy=True, want_min=True, want_state=True)
            e.adopt_best()
            e.track_minimum(False)
            return o
        a, b = run_both(eng, m0, tracked_call)
        assert_same(a, b)
        ev = b["o"]["energy"][:, ::2]
        assert np.array_equal(b["o"]["argmin"], 2 * ev.argmin(axis=1)) and np.array_equal(b["o"]["min_energy"], ev.min(axis=1))
        assert np.array_equal(b["final"], b["o"]["argmin_state"])
        eng.set_energy_sink(None)
        buf.free()


def test_chain_subsets(product):
    N, L, S = 40, 70, 5
    J, h = dense_instance(N, 8)
    m0 = init_spins(L, N)
    betas = np.geomspace(0.2, 3.0, L)
    marks = np.arange(L) % 3 == 1
    with product.Engine(J, h, L) as eng:
        eng.pt_init(betas)
        eng.mark_slots(marks)
        for which in ("marked", "unmarked"):
            def call(e):
                e.select(which)
                o = e.sweep_philox(S, SEED, beta=None, **ALL_OUT)
                e.select("all")
                return o
            a, b = run_both(eng, m0, call)
            assert_same(a, b)
            sel = marks if which == "marked" else ~marks
            assert b["o"]["spins"].shape[0] == int(sel.sum())
            assert np.array_equal(b["final"][~sel], m0[~sel])                  # untouched chains unchanged
            assert not np.array_equal(b["final"][sel], m0[sel])
        # per-chain orders over a subset are refused on every route
        for mode in ("off", "force"):
            eng.set_lane_sweeps(mode)
            eng.select("marked")
            with pytest.raises(NotImplementedError, match="shared-order"):
                eng.sweep_philox(S, SEED, beta=None, order="per_chain")
            eng.select("all")


def test_windows_of_visiting_orders(product, monkeypatch):
    """A per-chain-order call whose orders exceed the scratch bound runs in several windows (NLMC_LANE_SCRATCH, read at nlmc_create:
    the bound run_sweeps_stepwise keeps is 256 MiB): same bits as one window."""
    J, h = make_instance(37, seed=9, with_h=True, gaussian=True)
    N, R, S = 37, 65, 7
    m0 = init_spins(R, N)
    tab = np.linspace(0.1, 2.0, R)[:, None] * np.linspace(0.5, 1.5, S)[None, :]

    def go(launches):
        with product.Engine(J, h, R) as eng:
            a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, sweep0=11, beta=tab, precision="f64", order="per_chain",
                                                              record_stride=2, want_energy=True, want_min=True, want_state=True))
            assert eng.last_timing()["launches_sweep"] == launches
        assert_same(a, b)
        return b
    one = go(1)
    monkeypatch.setenv("NLMC_LANE_SCRATCH", str(2 * R * N * 3))           # room for the orders of three sweeps
    many = go(3)
    for k in OUT_KEYS:
        assert np.array_equal(one["o"][k], many["o"][k]), k
    assert np.array_equal(one["final"], many["final"]) and np.array_equal(one["tracked"], many["tracked"])


def test_windows_helper_does_not_plan_for_a_lane_call(product):
    """sweep_philox_windows asks the route first: under "force" a chain of 300 spins runs one chain per lane (no fused plan), with the
    bits of the fused windows it takes otherwise."""
    N, R, S = 300, 5, 6
    J, h = make_instance(N, seed=31)
    m0 = init_spins(R, N)
    with product.Engine(J, h, R) as eng:
        a, b = run_both(eng, m0, lambda e: e.sweep_philox_windows(S, SEED, beta=1.2, window=3, **ALL_OUT))
        assert eng.fused_last_call is False
    assert_same(a, b, routes=("fused", "lanes"))


def test_known_answer_wishart_ground_state(product):
    J, h, nf, e_gs = wishart(product, 1)
    R = 64
    m0 = init_spins(R, 10)
    with product.Engine(J, h, R) as eng:
        eng.set_lane_sweeps("force")
        eng.set_spins(m0)
        eng.energy()
        o = eng.sweep_philox(20, 5, beta=3.0, precision="f64", want_min=True)
        assert eng.last_sweep_route() == "lanes"
    assert abs(o["min_energy"].min() * nf - e_gs) < 1e-9
