"""The tempering rounds inside k_rounds_waves launches through the drivers: LocalTempering(wave_sweeps="force", wave_rounds=True) hands
run_rounds' chunks to the kernel and gives what wave_rounds=False gives round by round -- spins, slots, swap log, tracked energies; once
more with the best-state record and the energy log, which the kernel then keeps itself -- and NPT(waves="force", wave_rounds=True).run
returns what NPT().run returns."""
import numpy as np
import pytest

import wavefields
from conftest import GOLDEN
from helpers import init_spins
from test_gpu_waves_drivers import SEED, quiet

pytestmark = pytest.mark.gpu


def tempering(product, wave_rounds, observed):
    J, h, _, _ = wavefields.wishart(product, GOLDEN)
    inst = product.Instance(J, h)
    L, ladders, rounds, S, pairs = 6, 2, 8, 3, 2
    betas = np.geomspace(0.3, 2.0, L)
    lt = product.distributed.LocalTempering(inst, betas, L * ladders, SEED, pairs, [0], wave_sweeps="force", wave_rounds=wave_rounds,
                                            track_best=observed, track_energies=observed)
    try:
        assert lt.engs[0].wave_rounds is wave_rounds
        lt.set_spins(init_spins(L * ladders, 10))
        lt.plan(rounds * S, rounds)
        lt.log_begin(rounds)
        lt.run_rounds(rounds, S)
        lt.check()
        out = {"spins": lt.gather_spins(), "slots": lt.slots(), "log": lt.swap_log(), "tracked": lt.engs[0].energy_tracked(),
               "routes": lt.rounds_routes, "deferred": lt.deferred_rounds, "sweep_route": lt.engs[0].last_sweep_route()}
        if observed:
            out["best"], out["elog"] = lt.best(), lt.energy_log()
    finally:
        lt.close()
    return out


@pytest.mark.parametrize("observed", [False, True], ids=["plain", "track_best+track_energies"])
def test_local_tempering_run_rounds(product, observed):
    """Wishart N = 10, L = 6, 2 ladders, 8 rounds of 3 sweeps."""
    a, b = tempering(product, False, observed), tempering(product, True, observed)
    assert a["routes"] == [None] and a["deferred"] == 0 and a["sweep_route"] == "waves"      # round by round, as ever
    assert b["routes"] == ["waves"] and b["deferred"] == 8 and b["sweep_route"] == "waves"
    assert np.array_equal(a["spins"], b["spins"]) and np.array_equal(a["slots"], b["slots"]) and np.array_equal(a["tracked"], b["tracked"])
    assert np.array_equal(a["log"][0], b["log"][0]) and np.array_equal(a["log"][1], b["log"][1]) and a["log"][1].any()
    assert not np.array_equal(a["slots"], np.arange(12) % 6)
    if observed:
        for k in ("energy", "stamp", "first_hit", "state"):
            assert np.array_equal(a["best"][k], b["best"][k]), k
        assert np.array_equal(a["elog"][0], b["elog"][0]) and np.array_equal(a["elog"][1], b["elog"][1])
        assert np.isfinite(b["elog"][0]).all() and (b["best"]["stamp"] >= 0).all()


def test_npt_run(product, monkeypatch):
    """Wishart N = 10, R = 6, 2 restarts: rounds 0 .. 4 of 6 in one pt_rounds_deferred call that takes the wave rounds."""
    J, h, _, _ = wavefields.wishart(product, GOLDEN)
    R, S, rounds = 6, 3, 6
    betas = np.geomspace(0.3, 2.0, R)
    calls = []
    orig = product.engine.Engine.pt_rounds_deferred

    def wrapped(self, n_rounds, *a, **k):
        ok = orig(self, n_rounds, *a, **k)
        calls.append((int(n_rounds), bool(ok), self.last_rounds_route() if ok else None))
        return ok
    monkeypatch.setattr(product.engine.Engine, "pt_rounds_deferred", wrapped)

    def run(**kw):
        obj = product.NPT(J, h, rng="philox", seed=4242, **kw)
        with quiet():
            M, E = obj.run(betas, R, [False] * R, num_sweeps_MCMC=S * rounds, num_sweeps_read=S * rounds, num_swap_attempts=rounds,
                           num_swapping_pairs=2, num_restarts=2, return_trace="int8")
        return M, E, obj.restart_energies
    want = run()
    assert not any(ok for _, ok, _ in calls)
    del calls[:]
    got = run(waves="force", wave_rounds=True)
    assert calls and sum(n for n, _, _ in calls) == rounds - 1 and all(c[1:] == (True, "waves") for c in calls)
    for x, y in zip(want, got):
        assert np.array_equal(x, y)
    assert want[0].any()


def test_value_errors(product):
    J, h, _, _ = wavefields.wishart(product, GOLDEN)
    with pytest.raises(ValueError, match="wave_rounds needs waves"):
        product.NPT(J, h, rng="philox", seed=1, wave_rounds=True)
    with pytest.raises(ValueError, match="precision='f32'"):
        product.NPT(J, h, rng="philox", seed=1, precision="f64", waves="force", wave_rounds=True)
    obj = product.NPT(J, h, rng="philox", seed=1, waves="force", wave_rounds=True)
    with pytest.raises(ValueError, match="wave_rounds runs plain replicas only"):
        with quiet():
            obj.run(np.geomspace(0.3, 2.0, 4), 4, [False, True, False, False], num_sweeps_MCMC=4, num_sweeps_read=4, num_swap_attempts=2,
                    num_swapping_pairs=1)
    with pytest.raises(ValueError, match="wave_rounds needs wave_sweeps"):
        product.distributed.LocalTempering(product.Instance(J, h), np.geomspace(0.3, 2.0, 4), 4, 1, 1, [0], wave_rounds=True)
