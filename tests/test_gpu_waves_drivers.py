"""The wave-per-chain route through the drivers: off and "force" give the same results -- LocalTempering round by round (spins,
slots, swap log, tracked energies; once more with the best-state record and the energy log, which observe the state arrays),
NPT.run, APT_ICM.run(icm_feedback=True), APT_preprocessor.run -- and the sweeps do run one chain per wave."""
import contextlib
import io

import numpy as np
import pytest

import wavefields
from conftest import GOLDEN
from helpers import init_spins

pytestmark = pytest.mark.gpu
SEED = 0xA5A50000 + (7 << 32)


@contextlib.contextmanager
def quiet():
    with contextlib.redirect_stdout(io.StringIO()):
        yield


def tempering(product, waves, observed):
    J, h, _, _ = wavefields.wishart(product, GOLDEN)
    inst = product.Instance(J, h)
    L, ladders, rounds, S, pairs = 6, 2, 8, 3, 2
    betas = np.geomspace(0.3, 2.0, L)
    lt = product.distributed.LocalTempering(inst, betas, L * ladders, SEED, pairs, [0], wave_sweeps=waves, track_best=observed,
                                            track_energies=observed)
    try:
        lt.set_spins(init_spins(L * ladders, 10))
        lt.plan(rounds * S, rounds)
        lt.log_begin(rounds)
        routes = set()
        for _ in range(rounds):
            lt.round(S)
            routes.add(lt.engs[0].last_sweep_route())
        lt.check()
        out = {"spins": lt.gather_spins(), "slots": lt.slots(), "log": lt.swap_log(), "tracked": lt.engs[0].energy_tracked(),
               "routes": routes}
        if observed:
            out["best"], out["elog"] = lt.best(), lt.energy_log()
    finally:
        lt.close()
    return out


@pytest.mark.parametrize("observed", [False, True], ids=["plain", "track_best+track_energies"])
def test_local_tempering_round_by_round(product, observed):
    """Wishart N = 10, L = 6, 2 ladders, 8 rounds of 3 sweeps."""
    a, b = tempering(product, "off", observed), tempering(product, "force", observed)
    assert a["routes"] == {"stepwise"} and b["routes"] == {"waves"}
    assert np.array_equal(a["spins"], b["spins"]) and np.array_equal(a["slots"], b["slots"]) and np.array_equal(a["tracked"], b["tracked"])
    assert np.array_equal(a["log"][0], b["log"][0]) and np.array_equal(a["log"][1], b["log"][1]) and a["log"][1].any()
    assert not np.array_equal(a["slots"], np.arange(12) % 6)
    if observed:
        for k in ("energy", "stamp", "first_hit", "state"):
            assert np.array_equal(a["best"][k], b["best"][k]), k
        assert np.array_equal(a["elog"][0], b["elog"][0]) and np.array_equal(a["elog"][1], b["elog"][1])
        assert np.isfinite(b["elog"][0]).all() and (b["best"]["stamp"] >= 0).all()


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
    J, h, _, _ = wavefields.wishart(product, GOLDEN)
    R, S, rounds = 6, 3, 6
    betas = np.geomspace(0.3, 2.0, R)

    def run(**kw):
        obj = product.NPT(J, h, rng="philox", seed=4242, **kw)
        with quiet():
            M, E = obj.run(betas, R, [False] * R, num_sweeps_MCMC=S * rounds, num_sweeps_read=S * rounds, num_swap_attempts=rounds,
                           num_swapping_pairs=2, num_restarts=2, return_trace="int8")
        return M, E, obj.restart_energies
    want = run()
    seen = spy_routes(product, monkeypatch)
    got = run(waves="force")
    assert seen and set(seen) == {"waves"}
    for x, y in zip(want, got):
        assert np.array_equal(x, y)
    assert want[0].any()
    with pytest.raises(ValueError, match="waves applies to precision='f32'"):
        product.NPT(J, h, rng="philox", seed=1, precision="f64", waves="force")


def test_apt_icm_run(product, monkeypatch):
    J, h, _, _ = wavefields.wishart(product, GOLDEN)

    def run(**kw):
        obj = product.APT_ICM(J, h, rng="philox", seed=77, **kw)
        with quiet():
            M, E = obj.run(np.geomspace(0.4, 1.6, 6), 6, num_sweeps_MCMC=12, num_sweeps_read=12, num_swap_attempts=6, num_swapping_pairs=2,
                           icm_feedback=True, return_trace="int8")
        return M, E, obj.final_energies, obj.final_slots, obj.swap_accepted, obj.icm_cluster_sizes
    want = run()
    seen = spy_routes(product, monkeypatch)
    got = run(waves="force")
    assert seen and set(seen) == {"waves"}
    for x, y in zip(want, got):
        assert np.array_equal(x, y)
    assert want[0].any() and want[4].sum() > 0


def test_apt_preprocessor_run(product, monkeypatch, tmp_path):
    J, h, _, _ = wavefields.wishart(product, GOLDEN)
    monkeypatch.chdir(tmp_path)

    def run(**kw):
        obj = product.APT_preprocessor(J.copy(), h.copy(), rng="philox", seed=11, **kw)
        with quiet():
            return obj.run(num_sweeps_MCMC=12, num_sweeps_read=8, num_rng=8, beta_start=0.5, alpha=1.25, sigma_E_val=1000, beta_max=4,
                           use_hash_table=0, num_cores=1)
    beta0, sigma0 = run()
    seen = spy_routes(product, monkeypatch)
    beta1, sigma1 = run(waves="force")
    assert seen and set(seen) == {"waves"}
    assert len(beta0) > 1 and beta0 == beta1 and sigma0 == sigma1
