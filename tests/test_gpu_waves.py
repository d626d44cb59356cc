"""Wave-per-chain sweeps with resident local fields (include/nlmc.h: nlmc_set_wave_sweeps; csrc/nlmc_waves.h) against the
sweep-by-sweep route and the oracle.

Every case runs the same call twice on one engine, set_wave_sweeps("off") then ("force"), from the same start state: every output
(recorded spins, energy trace, min_energy, argmin, argmin_state, final spins, energy_tracked()) is equal bit for bit, and
last_sweep_route() says "stepwise", then "waves".  Named chains are also compared with oracle.sweeps_philox.  The shapes are the
smallest at which the wave kernel can go wrong: one row and a partly filled last workgroup, 1 and 16 waves per workgroup, chains
shorter than a Philox block, every register count (n = 64 | 65, 128 | 129, 256) and the matrix in LDS or in global memory
(n = 192 | 193), diagonal entries, phase flags with a wholly frozen chain, every temperature source, every output, chain subsets,
more than one window of visiting orders, both ends of escale - qs, and the calls the route leaves to the others (fp64, n = 257)."""
import numpy as np
import pytest

import oracle
import scalefamily
import wavefields
from wavefields import dense_instance
from conftest import GOLDEN
from helpers import make_instance, init_spins, DeviceBuffer

pytestmark = pytest.mark.gpu
SEED = 0xA5A50000 + (7 << 32)          # high bits set
OUT_KEYS = ("spins", "energy", "min_energy", "argmin", "argmin_state")
ALL_OUT = dict(record_stride=1, want_energy=True, want_min=True, want_state=True)


def run_both(eng, m0, call, prepare=None, modes=("off", "force")):
    """`call(eng)` under each wave mode from the same start state (spins, re-synchronised energies, whatever `prepare` sets)."""
    res = []
    for mode in modes:
        eng.set_wave_sweeps(mode)
        eng.set_spins(m0)
        E0 = eng.energy()
        if prepare:
            prepare(eng)
        o = call(eng)
        res.append({"o": o, "route": eng.last_sweep_route(), "final": eng.get_spins(), "tracked": eng.energy_tracked(), "E0": E0,
                    "fused": eng._last_fused(), "stats": eng.last_schedule_stats()})
    return res


def assert_same(a, b, routes=("stepwise", "waves")):
    assert (a["route"], b["route"]) == routes
    for k in OUT_KEYS:
        if a["o"][k] is None:
            assert b["o"][k] is None
        else:
            assert np.array_equal(a["o"][k], b["o"][k]), k
    assert np.array_equal(a["final"], b["final"])
    assert np.array_equal(a["tracked"], b["tracked"])
    if b["route"] == "waves":
        assert not b["fused"] and b["stats"]["levels"] == 0 and b["stats"]["orders"] > 0


def assert_oracle(J, h, m0, res, chains, beta_of, S, esc, order, sweep0=0, chain_base=0, flags=None, temp_x=1.0, seed=SEED):
    """res: one f32 run with all outputs; beta_of(c) -> [S] inverse temperatures of chain c."""
    csr = oracle.Csr(J)
    o = res["o"]
    for c in chains:
        gc = c + chain_base
        cb = np.array([oracle.cb_pair(b, temp_x, False) for b in beta_of(c)])
        ef0 = int(np.rint(res["E0"][c] * 2.0 ** esc))
        M, s_fin, tr = oracle.sweeps_philox(csr, h, m0[c], cb, seed, gc, order_group=(gc + 1 if order == "per_chain" else 0), sweep0=sweep0,
                                            flags=None if flags is None else flags[c], escale=esc, use_f64=False, efix0=ef0)
        assert np.array_equal(o["spins"][c], M), f"chain {c}"
        assert np.array_equal(res["final"][c], s_fin)
        assert np.array_equal(o["energy"][c], tr.astype(np.float64) * 2.0 ** -esc)
        am = int(np.argmin(tr))
        assert o["argmin"][c] == am and o["min_energy"][c] == tr[am] * 2.0 ** -esc
        assert np.array_equal(o["argmin_state"][c], M[am])
        assert res["tracked"][c] == tr[-1] * 2.0 ** -esc


@pytest.mark.parametrize("order", ["shared", "per_chain"])
@pytest.mark.parametrize("waves", [None, "1", "16"], ids=["w-unset", "w1", "w16"])
@pytest.mark.parametrize("rows", [1, 3, 17, 70])
def test_rows_workgroup_shapes_and_keys(product, rows, waves, order, monkeypatch):
    """waves: NLMC_WAVE_WAVES (read when the engine is created), the waves = chains of a workgroup; None: chosen by row count."""
    if waves is not None:
        monkeypatch.setenv("NLMC_WAVE_WAVES", waves)
    J, h = make_instance(37, seed=9, with_h=True, gaussian=True)
    S, N = 5, 37
    m0 = init_spins(rows, N)
    betas = np.linspace(0.2, 3.0, rows)
    with product.Engine(J, h, rows, chain_base=3, n_chains_global=rows + 3) as eng:
        esc = eng.energy_scale
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, sweep0=5, beta=np.repeat(betas[:, None], S, axis=1), order=order,
                                                          **ALL_OUT))
    assert_same(a, b)
    assert b["stats"]["orders"] == (S * rows if order == "per_chain" else S)
    assert_oracle(J, h, m0, b, [c for c in (0, 2, 16, 69) if c < rows], lambda c: np.full(S, betas[c]), S, esc, order, sweep0=5,
                  chain_base=3)


@pytest.mark.parametrize("n", [2, 5, 10])
def test_chains_shorter_than_a_philox_block(product, n):
    J, h = dense_instance(n, 40 + n)
    R, S = 19, 5
    m0 = init_spins(R, n)
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=0.9, **ALL_OUT))
    assert_same(a, b)
    assert_oracle(J, h, m0, b, (0, 3, 18), lambda c: np.full(S, 0.9), S, esc, "shared")


def boundary_case(product, J, h, N, order="shared"):
    R, S = 5, 3
    m0 = init_spins(R, N)
    betas = np.linspace(0.3, 2.0, R)
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, sweep0=2, beta=np.repeat(betas[:, None], S, axis=1), order=order,
                                                          **ALL_OUT))
    assert_same(a, b)
    assert_oracle(J, h, m0, b, (0, 4), lambda c: np.full(S, betas[c]), S, esc, order, sweep0=2)


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129, 192, 193, 255, 256])
def test_register_and_matrix_boundaries_sparse(product, n):
    """One, two and four fields per lane (n <= 64, 128, 256); the matrix in LDS up to n = 192, in global memory beyond."""
    J, h = make_instance(n, seed=100 + n, with_h=True, gaussian=True)
    boundary_case(product, J, h, n, order="per_chain" if n % 2 else "shared")


@pytest.mark.parametrize("n", [65, 193])
def test_register_and_matrix_boundaries_dense(product, n):
    J, h = dense_instance(n, 200 + n)
    boundary_case(product, J, h, n)


@pytest.mark.parametrize("n", [40, 129])
def test_matrix_rows_from_global_memory(product, n, monkeypatch):
    """NLMC_WAVE_JLDS=0 (read when the engine is created): the rows come from global memory at a size that stages them otherwise."""
    monkeypatch.setenv("NLMC_WAVE_JLDS", "0")
    J, h = dense_instance(n, 300 + n) if n == 40 else make_instance(n, seed=300 + n, with_h=True, gaussian=True)
    boundary_case(product, J, h, n)


def test_one_spin_past_the_size_limit_runs_as_before(product):
    N, R, S = 257, 3, 3
    J, h = make_instance(N, seed=22)
    m0 = init_spins(R, N)
    with product.Engine(J, h, R) as eng:
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=1.5, **ALL_OUT))
    assert_same(a, b, routes=("stepwise", "stepwise"))


def test_diagonal_entries(product):
    J, h = dense_instance(20, 77, diag=True)
    R, S = 9, 6
    m0 = init_spins(R, 20)
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=1.1, **ALL_OUT))
        eng.set_spins(b["final"])
        E_exact = eng.energy()
    assert_same(a, b)
    assert_oracle(J, h, m0, b, (0, 8), lambda c: np.full(S, 1.1), S, esc, "shared")
    # the tracked energies leave the diagonal out of every delta: they stay with the recomputed ones (test_gpu_sweep.py's bound)
    assert np.all(np.abs(b["tracked"] - E_exact) <= 1e-4 * np.maximum(1.0, np.abs(E_exact)))


def test_phase_flags(product):
    N, R, S = 70, 6, 6
    J, h = make_instance(N, seed=3, with_h=True)
    m0 = init_spins(R, N)
    flags = wavefields.phase_flags(R, N, m0)
    assert set(np.unique(flags)) == {0, 1, 2, 3} and np.all(flags[R - 1] >= 2)
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, 99, beta=2.0, **ALL_OUT), prepare=lambda e: e.set_flags(flags, 20.0))
    assert_same(a, b)
    assert_oracle(J, h, m0, b, range(R), lambda c: np.full(S, 2.0), S, esc, "shared", flags=flags, temp_x=20.0, seed=99)
    frozen = flags >= 2
    assert np.array_equal(b["final"][frozen], m0[frozen])
    assert np.array_equal(b["final"][R - 1], m0[R - 1])         # the chain with every spin frozen


@pytest.mark.parametrize("source", ["scalar", "per_chain", "per_sweep", "slots"])
def test_every_temperature_source(product, source):
    N, R, S = 40, 7, 5
    J, h = dense_instance(N, 5)
    m0 = init_spins(R, N)
    betas = np.geomspace(0.1, 3.0, R)
    tab = np.linspace(0.1, 2.0, R)[:, None] * np.linspace(0.5, 1.5, S)[None, :]        # distinct columns
    slots = np.random.default_rng(4).permutation(R).astype(np.int32)                   # chain c sits on slot slots[c]
    assert not np.array_equal(slots, np.arange(R))
    beta = {"scalar": 0.7, "per_chain": np.repeat(betas[:, None], S, axis=1), "per_sweep": tab, "slots": None}[source]
    beta_of = {"scalar": lambda c: np.full(S, 0.7), "per_chain": lambda c: np.full(S, betas[c]), "per_sweep": lambda c: tab[c],
               "slots": lambda c: np.full(S, betas[slots[c]])}[source]
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        if source == "slots":
            eng.pt_init(betas)
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=beta, **ALL_OUT),
                        prepare=(lambda e: e.pt_set_slots(slots)) if source == "slots" else None)
    assert_same(a, b)
    assert_oracle(J, h, m0, b, (0, 1, 6), beta_of, S, esc, "shared")


def test_every_output_on_its_own_and_strided(product):
    J, h = make_instance(70, seed=12, with_h=True, gaussian=True)
    N, R, S = 70, 6, 7
    m0 = init_spins(R, N)
    betas = np.repeat(np.linspace(0.3, 2.5, R)[:, None], S, axis=1)
    with product.Engine(J, h, R) as eng:
        buf = DeviceBuffer(np.zeros(R))
        eng.set_energy_sink(buf.ptr.value)
        sinks = []

        def call(e):
            o = e.sweep_philox(S, SEED, beta=betas, record_stride=3, want_energy=True, want_min=True, want_state=True)
            sinks.append(buf.read(R))
            return o
        a, b = run_both(eng, m0, call)
        assert_same(a, b)
        assert b["o"]["spins"].shape == (R, (S + 2) // 3, N)
        assert np.array_equal(sinks[0], a["tracked"]) and np.array_equal(sinks[1], b["tracked"])
        assert np.array_equal(b["o"]["energy"][:, -1], b["tracked"])
        assert np.array_equal(b["o"]["min_energy"], b["o"]["energy"].min(axis=1))
        assert np.array_equal(b["o"]["argmin"], b["o"]["energy"].argmin(axis=1))
        for outs in (dict(record_stride=1), dict(want_energy=True), dict(want_min=True), dict(want_min=True, want_state=True), dict()):
            a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=betas, **outs))
            assert_same(a, b)

        def tracked_call(e):                   # running minimum kept on the device over sweeps 0, 2, 4, ...; its state adopted afterwards
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
    N, L, S = 40, 10, 5
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
        for mode in ("off", "force"):          # per-chain orders over a subset are refused on every route
            eng.set_wave_sweeps(mode)
            eng.select("marked")
            with pytest.raises(NotImplementedError, match="shared-order"):
                eng.sweep_philox(S, SEED, beta=None, order="per_chain")
            eng.select("all")


def test_windows_of_visiting_orders(product, monkeypatch):
    """A per-chain-order call whose orders exceed the scratch bound runs in several windows (NLMC_LANE_SCRATCH, read at nlmc_create):
    same bits as one window."""
    J, h = make_instance(37, seed=9, with_h=True, gaussian=True)
    N, R, S = 37, 9, 7
    m0 = init_spins(R, N)
    tab = np.linspace(0.1, 2.0, R)[:, None] * np.linspace(0.5, 1.5, S)[None, :]

    def go(launches):
        with product.Engine(J, h, R) as eng:
            a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, sweep0=11, beta=tab, order="per_chain", record_stride=2,
                                                              want_energy=True, want_min=True, want_state=True))
            assert eng.last_timing()["launches_sweep"] == launches
        assert_same(a, b)
        return b
    one = go(1)
    monkeypatch.setenv("NLMC_LANE_SCRATCH", str(2 * R * N * 3))           # room for the orders of three sweeps
    many = go(3)
    for k in OUT_KEYS:
        assert np.array_equal(one["o"][k], many["o"][k]), k
    assert np.array_equal(one["final"], many["final"]) and np.array_equal(one["tracked"], many["tracked"])


def test_fp64_calls_go_on_to_the_other_routes(product):
    """precision="f64" under "force": not the wave route, the bits of off; with the lane mode forced too, f32 -> waves, f64 -> lanes."""
    N, R, S = 40, 6, 4
    J, h = dense_instance(N, 6)
    m0 = init_spins(R, N)
    with product.Engine(J, h, R) as eng:
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=1.3, precision="f64", **ALL_OUT))
        assert_same(a, b, routes=("stepwise", "stepwise"))
        eng.set_lane_sweeps("force")
        c, d = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=1.3, precision="f64", **ALL_OUT))
        assert_same(c, d, routes=("lanes", "lanes"))
        assert_same(a, d, routes=("stepwise", "lanes"))
        e32, f32 = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=1.3, **ALL_OUT))
        assert_same(e32, f32, routes=("lanes", "waves"))
        eng.set_lane_sweeps("off")
        g32, _ = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=1.3, **ALL_OUT))
        assert_same(g32, f32)


def test_windows_helper_does_not_plan_for_a_wave_call(product):
    """sweep_philox_windows asks the route first: under "force" a chain of 256 spins runs one chain per wave (no fused plan), with the
    bits of the fused windows it takes otherwise."""
    N, R, S = 256, 5, 6
    J, h = make_instance(N, seed=31)
    m0 = init_spins(R, N)
    with product.Engine(J, h, R) as eng:
        a, b = run_both(eng, m0, lambda e: e.sweep_philox_windows(S, SEED, beta=1.2, window=3, **ALL_OUT))
        assert eng.fused_last_call is False
    assert_same(a, b, routes=("fused", "waves"))


@pytest.mark.parametrize("order", ["shared", "per_chain"])
def test_known_answer_wishart_ground_state(product, order):
    """The premise is tests/test_waves_cpu.py::test_known_answer_premise_under_the_oracle_alone."""
    J, h, nf, e_gs = wavefields.wishart(product, GOLDEN)
    R, S = 64, 20
    m0 = init_spins(R, 10)
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        eng.set_wave_sweeps("force")
        eng.set_spins(m0)
        E0 = eng.energy()
        o = eng.sweep_philox(S, 5, beta=3.0, order=order, **ALL_OUT)
        assert eng.last_sweep_route() == "waves"
        res = {"o": o, "final": eng.get_spins(), "tracked": eng.energy_tracked(), "E0": E0}
    csr = oracle.Csr(J)                         # (the tracked energies are those of the fixed-point model: the states' own energy)
    best = min(oracle.energy(csr, h, o["spins"][c, t]) for c in range(R) for t in range(S))
    assert abs(best * nf - e_gs) < 1e-9
    assert_oracle(J, h, m0, res, range(R), lambda c: np.full(S, 3.0), S, esc, order, seed=5)


@pytest.mark.parametrize("name", ["x1e-9", "x1"])
def test_magnitudes(product, name):
    """The two ends of escale - qs: 0 (x1e-9: qs = escale = 52) and 29 (x1)."""
    J, h, beta_unit = scalefamily.member(name, 100)
    qs, esc_pinned = oracle.field_scale(oracle.Csr(J), h)
    assert esc_pinned - qs == {"x1e-9": 0, "x1": 29}[name]
    R, S = 5, 4
    m0 = init_spins(R, 100)
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        assert (eng.field_scale, esc) == (qs, esc_pinned)
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=beta_unit, **ALL_OUT))
    assert_same(a, b)
    assert_oracle(J, h, m0, b, (0, 4), lambda c: np.full(S, beta_unit), S, esc, "shared")
