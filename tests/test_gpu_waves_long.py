"""Wave-per-chain sweeps of dense chains of 257 .. 1024 spins (include/nlmc.h: nlmc_set_wave_long; csrc/nlmc_waves_long.h) against the
sweep-by-sweep route and the oracle.

Every case runs the same call twice on one engine under set_wave_sweeps("force"), set_wave_long(False) then (True), from the same
start state: every output (recorded spins, energy trace, min_energy, argmin, argmin_state, final spins, energy_tracked()) is equal
bit for bit, and last_sweep_route() says "stepwise", then "waves".  Named chains are also compared with oracle.sweeps_philox.  The
shapes are the smallest at which the kernel can go wrong: both register counts and their boundaries (n = 257, 511 | 512 | 513,
1023 | 1024), n_pad != n, one row and a partly filled last workgroup, 1 wave and as many waves per workgroup as the LDS holds,
diagonal entries, phase flags with a wholly frozen chain, a temperature per sweep, every output with strides, chain subsets, more
than one window of visiting orders, both ends of escale - qs, the calls the route leaves to the others (n = 1025, fp64, the option
off), tempering rounds under set_wave_rounds, and the keyword through two drivers."""
import contextlib
import io

import numpy as np
import pytest

import oracle
import scalefamily
import wavefields
from wavefields import dense_instance
from helpers import make_instance, init_spins

pytestmark = pytest.mark.gpu
SEED = 0xA5A50000 + (7 << 32)          # high bits set
OUT_KEYS = ("spins", "energy", "min_energy", "argmin", "argmin_state")
ALL_OUT = dict(record_stride=1, want_energy=True, want_min=True, want_state=True)


def run_both(eng, m0, call, prepare=None, longs=(False, True), waves="force"):
    """`call(eng)` with the long-chain option off, then on, from the same start state (spins, re-synchronised energies, whatever
    `prepare` sets)."""
    res = []
    eng.set_wave_sweeps(waves)
    for on in longs:
        eng.set_wave_long(on)
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


def boundary_case(product, J, h, N, R=5, S=3, order="shared", beta_hi=2.0):
    m0 = init_spins(R, N)
    betas = np.linspace(0.3, beta_hi, R)
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, sweep0=2, beta=np.repeat(betas[:, None], S, axis=1), order=order,
                                                          **ALL_OUT))
    assert_same(a, b)
    assert not np.array_equal(b["final"], m0)
    assert_oracle(J, h, m0, b, (0, R - 1), lambda c: np.full(S, betas[c]), S, esc, order, sweep0=2)


@pytest.mark.parametrize("n", [257, 272, 511, 512, 513, 1023, 1024])
def test_register_and_region_boundaries_sparse(product, n):
    """Eight fields per lane up to n = 512, sixteen beyond; n_pad = n at 272, 512 and 1024 only."""
    J, h = make_instance(n, seed=100 + n, with_h=True, gaussian=True)
    boundary_case(product, J, h, n, order="per_chain" if n % 2 else "shared")


@pytest.mark.parametrize("n", [257, 513, 1024])
def test_register_and_region_boundaries_dense(product, n):
    """Complete graphs: every row of the matrix is full.  (Inverse temperatures of a dense instance's scale: the chains move.)"""
    J, h = dense_instance(n, 200 + n)
    big = n == 1024
    boundary_case(product, J, h, n, R=2 if big else 5, S=2 if big else 3, beta_hi=0.2)


def largest_w(n):
    """The most waves the shape function gives a workgroup at n spins (csrc/nlmc_wave_shape.h)."""
    n_pad = (n + 15) // 16 * 16
    return min(16, 158 * 1024 // (256 * (8 if n <= 512 else 16) + 16 * ((n + 3) // 4) + 2 * n_pad))


@pytest.mark.parametrize("order", ["shared", "per_chain"])
@pytest.mark.parametrize("waves", [None, "1", "max"], ids=["w-unset", "w1", "wmax"])
@pytest.mark.parametrize("rows", [1, 3, 17])
def test_rows_workgroup_shapes_and_keys(product, rows, waves, order, monkeypatch):
    """waves: NLMC_WAVE_WAVES (read when the engine is created), the waves = chains of a workgroup; None: chosen by row count.  17
    rows on 16 waves: a second workgroup with one wave at work.  chain_base = 3: the keys are those of the global chain."""
    N, S = 300, 3
    if waves is not None:
        monkeypatch.setenv("NLMC_WAVE_WAVES", "1" if waves == "1" else str(largest_w(N)))
    J, h = make_instance(N, seed=9, with_h=True, gaussian=True)
    m0 = init_spins(rows, N)
    betas = np.linspace(0.2, 3.0, rows)
    with product.Engine(J, h, rows, chain_base=3, n_chains_global=rows + 3) as eng:
        esc = eng.energy_scale
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, sweep0=5, beta=np.repeat(betas[:, None], S, axis=1), order=order,
                                                          **ALL_OUT))
    assert_same(a, b)
    assert b["stats"]["orders"] == (S * rows if order == "per_chain" else S)
    assert_oracle(J, h, m0, b, [c for c in (0, 2, 16) if c < rows], lambda c: np.full(S, betas[c]), S, esc, order, sweep0=5, chain_base=3)


def test_fifteen_waves_share_the_lds_at_1024_spins(product, monkeypatch):
    """NLMC_WAVE_WAVES = 16 at n = 1024: sixteen regions of 10 KB exceed a workgroup's LDS, the shape function gives 15; 17 rows
    leave two waves at work in the second workgroup."""
    assert largest_w(1024) == 15 and largest_w(512) == 16
    monkeypatch.setenv("NLMC_WAVE_WAVES", "16")
    N, R, S = 1024, 17, 2
    J, h = make_instance(N, seed=41, with_h=True, gaussian=True)
    m0 = init_spins(R, N)
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=1.1, **ALL_OUT))
    assert_same(a, b)
    assert_oracle(J, h, m0, b, (14, 15, 16), lambda c: np.full(S, 1.1), S, esc, "shared")


def test_a_temperature_per_sweep(product):
    N, R, S = 300, 7, 3
    J, h = dense_instance(N, 5)
    m0 = init_spins(R, N)
    tab = np.linspace(0.02, 0.2, R)[:, None] * np.linspace(0.5, 1.5, S)[None, :]        # distinct columns
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=tab, **ALL_OUT))
    assert_same(a, b)
    assert_oracle(J, h, m0, b, (0, 6), lambda c: tab[c], S, esc, "shared")


def test_diagonal_entries(product):
    N, R, S = 300, 5, 3
    J, h = dense_instance(N, 77, diag=True)
    m0 = init_spins(R, N)
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=0.1, **ALL_OUT))
        eng.set_spins(b["final"])
        E_exact = eng.energy()
    assert_same(a, b)
    assert_oracle(J, h, m0, b, (0, 4), lambda c: np.full(S, 0.1), S, esc, "shared")
    # the tracked energies leave the diagonal out of every delta: they stay with the recomputed ones (test_gpu_sweep.py's bound)
    assert np.all(np.abs(b["tracked"] - E_exact) <= 1e-4 * np.maximum(1.0, np.abs(E_exact)))


def test_phase_flags(product):
    N, R, S = 300, 6, 3
    J, h = make_instance(N, seed=3, with_h=True)
    m0 = init_spins(R, N)
    flags = wavefields.phase_flags(R, N, m0)
    assert set(np.unique(flags)) == {0, 1, 2, 3} and np.all(flags[R - 1] >= 2)
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, 99, beta=2.0, **ALL_OUT), prepare=lambda e: e.set_flags(flags, 20.0))
    assert_same(a, b)
    assert_oracle(J, h, m0, b, (0, 1, R - 1), lambda c: np.full(S, 2.0), S, esc, "shared", flags=flags, temp_x=20.0, seed=99)
    frozen = flags >= 2
    assert np.array_equal(b["final"][frozen], m0[frozen])
    assert np.array_equal(b["final"][R - 1], m0[R - 1])         # the chain with every spin frozen


def test_chain_subsets(product):
    N, L, S = 300, 10, 3
    J, h = make_instance(N, seed=8, with_h=True, gaussian=True)
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


def test_strided_outputs(product):
    """record_stride = 3, and the running minimum over sweeps 0, 2, 4, .. kept on the device with its state adopted afterwards."""
    N, R, S = 300, 4, 5
    J, h = make_instance(N, seed=12, with_h=True, gaussian=True)
    m0 = init_spins(R, N)
    betas = np.repeat(np.linspace(0.3, 2.5, R)[:, None], S, axis=1)
    with product.Engine(J, h, R) as eng:
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=betas, record_stride=3, want_energy=True, want_min=True, want_state=True))
        assert_same(a, b)
        assert b["o"]["spins"].shape == (R, (S + 2) // 3, N)
        assert np.array_equal(b["o"]["energy"][:, -1], b["tracked"])
        for outs in (dict(record_stride=2), dict(want_min=True, want_state=True), dict()):
            a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=betas, **outs))
            assert_same(a, b)

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


def test_windows_of_visiting_orders(product, monkeypatch):
    """A per-chain-order call whose orders exceed the scratch bound runs in several windows (NLMC_LANE_SCRATCH, read at nlmc_create):
    same bits as one window; the fields are rebuilt from the spins at every launch."""
    N, R, S = 300, 3, 5
    J, h = make_instance(N, seed=9, with_h=True, gaussian=True)
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
    monkeypatch.setenv("NLMC_LANE_SCRATCH", str(2 * R * N * 2))           # room for the orders of two sweeps
    many = go(3)
    for k in OUT_KEYS:
        assert np.array_equal(one["o"][k], many["o"][k]), k
    assert np.array_equal(one["final"], many["final"]) and np.array_equal(one["tracked"], many["tracked"])


@pytest.mark.parametrize("name", ["x1e-9", "x1"])
def test_magnitudes(product, name):
    """The two ends of escale - qs: 0 (x1e-9: qs = escale = 52) and 29 (x1)."""
    J, h, beta_unit = scalefamily.member(name, 300)
    qs, esc_pinned = oracle.field_scale(oracle.Csr(J), h)
    assert esc_pinned - qs == {"x1e-9": 0, "x1": 29}[name]
    R, S = 3, 3
    m0 = init_spins(R, 300)
    with product.Engine(J, h, R) as eng:
        esc = eng.energy_scale
        assert (eng.field_scale, esc) == (qs, esc_pinned)
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=beta_unit, **ALL_OUT))
    assert_same(a, b)
    assert_oracle(J, h, m0, b, (0, 2), lambda c: np.full(S, beta_unit), S, esc, "shared")


def test_the_prefetching_variant(product, monkeypatch):
    """NLMC_WAVE_LONG_AHEAD=1 (read when the engine is created): the next visited spin's row requested at every update."""
    monkeypatch.setenv("NLMC_WAVE_LONG_AHEAD", "1")
    J, h = dense_instance(513, 31, diag=True)
    boundary_case(product, J, h, 513, R=3, S=2, beta_hi=0.2)


def test_one_spin_past_the_size_limit_runs_as_before(product):
    N, R, S = 1025, 2, 2
    J, h = make_instance(N, seed=22)
    m0 = init_spins(R, N)
    with product.Engine(J, h, R) as eng:
        assert not eng.waves_take()
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=1.5, **ALL_OUT))
    assert a["route"] == b["route"] != "waves"
    assert_same(a, b, routes=(a["route"], a["route"]))


def test_fp64_calls_go_on_to_the_other_routes(product):
    """precision="f64" under "force" with the option on: not the wave route; with the lane mode forced too, f32 -> waves, f64 -> lanes."""
    N, R, S = 300, 3, 2
    J, h = make_instance(N, seed=6, with_h=True, gaussian=True)
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


def test_with_the_option_off_257_spins_leave_the_wave_route(product):
    """The setter's default, and set_wave_long(False) after (True); "off" and "auto" wave modes do not take the route with the option on."""
    N, R, S = 257, 3, 2
    J, h = make_instance(N, seed=22)
    m0 = init_spins(R, N)
    with product.Engine(J, h, R) as eng:
        assert eng.wave_long is False
        eng.set_wave_sweeps("force")
        assert not eng.waves_take()
        eng.set_spins(m0)
        eng.sweep_philox(S, SEED, beta=1.5)
        assert eng.last_sweep_route() == "stepwise"
        a, b = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=1.5, **ALL_OUT), longs=(True, False))
        assert_same(b, a)
        for mode in ("off", "auto"):
            c, d = run_both(eng, m0, lambda e: e.sweep_philox(S, SEED, beta=1.5, **ALL_OUT), waves=mode)
            assert_same(c, d, routes=("stepwise", "stepwise"))
            assert_same(c, a)


def test_rounds_fall_through_to_a_sweep_and_a_swap_call_per_round(product):
    """n = 300, L = 4, two ladders.  With set_wave_rounds(True) and the option on, pt_rounds_deferred runs the rounds as sweep and swap
    calls, the sweeps on the wave route: the bits of the round-by-round drive with every mode off.  pt_rounds_waves keeps its limit."""
    N, L, ladders, T, rounds, pairs = 300, 4, 2, 2, 4, 1
    J, h = make_instance(N, seed=5, with_h=True, gaussian=True)
    G = L * ladders
    betas = np.linspace(0.30, 0.36, L)                             # close temperatures: swaps are accepted
    m0 = init_spins(G, N)

    def state(e):
        p, acc = e.pt_log_read()
        return {"spins": e.get_spins(), "energy": e.energy_tracked(), "slots": e.pt_slots(), "pairs": p, "acc": acc}

    with product.Engine(J, h, G) as eng:
        eng.pt_init(betas)

        def begin(mode, long_on, wave_rounds):
            eng.set_wave_sweeps(mode)
            eng.set_wave_long(long_on)
            eng.set_wave_rounds(wave_rounds)
            eng.set_spins(m0)
            eng.pt_set_slots((np.arange(G) % L).astype(np.int32))
            eng.pt_plan(0, rounds, SEED, pairs)
            eng.pt_log_begin(0, rounds, pairs)

        begin("force", True, True)
        assert eng.pt_rounds_waves(rounds, T, SEED, 0, 0, pairs) is False
        assert "at most NLMC_WAVE_N spins" in eng.rounds_fused_refusal
        assert np.array_equal(eng.get_spins(), m0)
        at = 0
        for k in (1, 3):                                           # two calls: the second starts where the first ended
            assert eng.pt_rounds_deferred(k, T, SEED, at * T, at, pairs) is True, eng.rounds_fused_refusal
            assert eng.last_sweep_route() == "waves" and eng.last_rounds_route() == "launch per round"
            at += k
        eng.pt_check()
        a = state(eng)

        begin("off", False, False)
        for r in range(rounds):
            eng.sweep_philox(T, SEED, sweep0=r * T, beta=None)
            assert eng.last_sweep_route() == "stepwise"
            eng.pt_swap_philox(r, SEED, pairs, want_log=False)
        eng.pt_check()
        b = state(eng)

        begin("force", False, True)                                # the option off: as before it existed, no route for these rounds
        assert eng.pt_rounds_deferred(rounds, T, SEED, 0, 0, pairs) is False
        assert np.array_equal(eng.get_spins(), m0)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["acc"].mean() > 0 and not np.array_equal(a["spins"], m0) and not np.array_equal(a["slots"], np.arange(G) % L)


@contextlib.contextmanager
def quiet():
    with contextlib.redirect_stdout(io.StringIO()):
        yield


def spy_routes(product, monkeypatch):
    """The routes of every sweep_philox call made while the patch is in place."""
    seen = []
    orig = product.engine.Engine.sweep_philox

    def spy(self, *a, **k):
        o = orig(self, *a, **k)
        seen.append(self.last_sweep_route())
        return o
    monkeypatch.setattr(product.engine.Engine, "sweep_philox", spy)
    return seen


def test_npt_run(product, monkeypatch):
    J, h = make_instance(300, seed=14, with_h=True, gaussian=True)
    J = J.toarray()
    R, S, rounds = 6, 2, 3
    betas = np.geomspace(0.3, 2.0, R)

    def run(**kw):
        obj = product.NPT(J, h, rng="philox", seed=4242, **kw)
        with quiet():
            M, E = obj.run(betas, R, [False] * R, num_sweeps_MCMC=S * rounds, num_sweeps_read=S * rounds, num_swap_attempts=rounds,
                           num_swapping_pairs=2, num_restarts=2, return_trace="int8")
        return M, E, obj.restart_energies
    want = run()
    seen = spy_routes(product, monkeypatch)
    got = run(waves="force", wave_long=True)
    assert seen and set(seen) == {"waves"}
    for x, y in zip(want, got):
        assert np.array_equal(x, y)
    assert want[0].any()


def test_apt_preprocessor_run(product, monkeypatch, tmp_path):
    J, h = make_instance(300, seed=15, with_h=True, gaussian=True)
    J = J.toarray()
    monkeypatch.chdir(tmp_path)

    def run(**kw):
        obj = product.APT_preprocessor(J.copy(), h.copy(), rng="philox", seed=11, **kw)
        with quiet():
            return obj.run(num_sweeps_MCMC=6, num_sweeps_read=4, num_rng=4, beta_start=0.5, alpha=1.25, sigma_E_val=1000, beta_max=2,
                           use_hash_table=0, num_cores=1)
    beta0, sigma0 = run()
    seen = spy_routes(product, monkeypatch)
    beta1, sigma1 = run(waves="force", wave_long=True)
    assert seen and set(seen) == {"waves"}
    assert len(beta0) > 1 and beta0 == beta1 and sigma0 == sigma1
