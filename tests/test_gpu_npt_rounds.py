"""NPT.run(rng="philox") hands its plain rounds 0 .. rounds - 2 to the engine a planned chunk at a time
(distributed.LocalTempering.run_rounds -> Engine.pt_rounds_deferred -> k_rounds_fused where the context qualifies); the last
round, which has outputs, stays a call of its own.  Every run is compared with the same run under NLMC_NO_DEFERRED=1, the
round-by-round loop: M, Energy, swap log, final slots and restart energies must be the same bits.  A spy on
Engine.pt_rounds_deferred shows which route ran."""
import contextlib
import io
import os

import numpy as np
import pytest

from helpers import make_instance

pytestmark = pytest.mark.gpu
INST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instances")
R = 8


@pytest.fixture
def spy(product, monkeypatch):
    """Batched calls of the run: (rounds, queued?, last_rounds_route() after the call)."""
    calls = []
    orig = product.engine.Engine.pt_rounds_deferred

    def wrapped(self, n_rounds, *a, **k):
        ok = orig(self, n_rounds, *a, **k)
        calls.append((int(n_rounds), bool(ok), self.last_rounds_route() if ok else None))
        return ok
    monkeypatch.setattr(product.engine.Engine, "pt_rounds_deferred", wrapped)
    return calls


def run(product, J, h, precision="f32", doNMC=None, **kw):
    args = dict(num_sweeps_MCMC=40, num_sweeps_read=40, num_swap_attempts=8, num_swapping_pairs=3, num_restarts=2)
    args.update(kw)
    obj = product.NPT(J, h, rng="philox", seed=77, precision=precision)
    with contextlib.redirect_stdout(io.StringIO()):
        M, E = obj.run(np.linspace(0.9, 1.1, R), R, doNMC or [False] * R, **args)
    return {"M": M, "Energy": E, "swap_pairs": obj.swap_pairs, "swap_accepted": obj.swap_accepted, "final_slots": obj.final_slots,
            "restart_energies": obj.restart_energies}


def same(a, b):
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert np.array_equal(a[k], b[k]), k


def both(product, monkeypatch, spy, J, h, **kw):
    """The run by default and under NLMC_NO_DEFERRED=1 -> (default result, its batched calls); the two must agree."""
    got = run(product, J, h, **kw)
    calls = list(spy)
    del spy[:]
    monkeypatch.setenv("NLMC_NO_DEFERRED", "1")
    ref = run(product, J, h, **kw)
    monkeypatch.delenv("NLMC_NO_DEFERRED")
    assert spy == []                                       # the round-by-round loop makes no batched call
    same(got, ref)
    return got, calls


@pytest.fixture(scope="module")
def pmj():
    return make_instance(2000, seed=19)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_plain_rounds_are_batched(product, monkeypatch, spy, pmj, precision):
    """+-J, 2 restarts of 8 replicas, 8 rounds of 5 sweeps: 7 rounds in batched calls inside k_rounds_fused launches."""
    got, calls = both(product, monkeypatch, spy, *pmj, precision=precision)
    assert calls and all(ok for _, ok, _ in calls) and sum(n for n, _, _ in calls) == 7
    assert all(route == "in launch" for _, _, route in calls)
    assert got["swap_accepted"].sum() > 0 and not np.array_equal(got["final_slots"], np.arange(2 * R) % R)
    assert got["M"].shape == (R * 2000, 5)


def test_chimera_f64_takes_the_real_valued_route(product, monkeypatch, spy):
    """Chimera-2048 / max|J| (couplings k/75) in the fp64 mode: batched rounds on the real-valued kernels."""
    W, h = product.instances.txt_to_A_droplet(os.path.join(INST, "chimera2048__001.txt"))
    _, calls = both(product, monkeypatch, spy, W, h, precision="f64", num_restarts=1)
    assert calls and all(ok for _, ok, _ in calls) and sum(n for n, _, _ in calls) == 7
    from test_gpu_rounds_real import DEFERRED_DEFAULT_REAL
    assert all(route == DEFERRED_DEFAULT_REAL for _, _, route in calls)


@pytest.mark.parametrize("return_trace", ["int8", None])
def test_other_read_outs(product, monkeypatch, spy, pmj, return_trace):
    got, calls = both(product, monkeypatch, spy, *pmj, return_trace=return_trace)
    assert sum(n for n, _, _ in calls) == 7
    assert (got["M"] is None) == (return_trace is None)


def test_two_contexts_give_the_bits_of_one(product, monkeypatch, spy, pmj):
    one = run(product, *pmj)
    del spy[:]
    two, calls = both(product, monkeypatch, spy, *pmj, device_ids=[0, 0])
    same(one, two)
    assert len(calls) >= 2 and sum(n for n, _, _ in calls) == 2 * 7 and all(ok for _, ok, _ in calls)


@pytest.mark.parametrize("case", ["one_round", "two_sweeps"])
def test_nothing_to_batch(product, monkeypatch, spy, pmj, case):
    """num_swap_attempts = 1: the only round has outputs.  Rounds of 2 sweeps: no fused window."""
    kw = dict(num_swap_attempts=1, num_sweeps_MCMC=5, num_sweeps_read=5) if case == "one_round" else \
        dict(num_swap_attempts=8, num_sweeps_MCMC=16, num_sweeps_read=16)
    _, calls = both(product, monkeypatch, spy, *pmj, **kw)
    assert calls == []


def test_nmc_slot_keeps_the_round_by_round_loop(product, monkeypatch, spy):
    J, h = make_instance(400, seed=4)
    kw = dict(doNMC=[False] * (R - 1) + [True], num_sweeps_MCMC=60, num_sweeps_read=30, num_swap_attempts=3, num_cycles=1,
              global_beta=2.5, lambda_start=3.0, lambda_end=0.05, lambda_reduction_factor=0.8, threshold_initial=0.9999,
              threshold_cutoff=0.97, num_restarts=1)
    _, calls = both(product, monkeypatch, spy, J, h, **kw)
    assert calls == []
