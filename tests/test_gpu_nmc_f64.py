"""NMC(J, h, rng="philox", precision="f64"): the reference's arithmetic (fp64 field, 53-bit uniform) with the device RNG for every
sweep of NMC.run / NMC_subroutine / run_restarts, the NMC phases on fused windows (k_sweep_fused with phase flags in the fp64
mode).  Same results as with the fused fp64 kernels switched off (NLMC_NO_FUSED64=1), and one cycle restated with the oracle."""
import contextlib
import io
import os

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
from helpers import make_instance

pytestmark = pytest.mark.gpu
INST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instances")
LBP = dict(lambda_start=3.0, lambda_end=0.3, lambda_reduction_factor=0.8, threshold_initial=0.9999, threshold_cutoff=0.97,
           max_iterations=100)


def chimera():
    import nlmc_amd as P
    W, h = P.instances.txt_to_A_droplet(os.path.join(INST, "chimera2048__001.txt"))
    return sp.csr_matrix(W).astype(np.float64), np.asarray(h, dtype=np.float64).ravel()


def pmj(N=2000):
    J, _ = make_instance(N, seed=211)
    return J, np.random.default_rng(211).integers(-1, 2, N).astype(np.float64)


@pytest.fixture
def fused_calls(product, monkeypatch):
    """(phase flags in force, fused_last_call) of every Engine.sweep_philox_windows call with precision="f64"."""
    seen = []
    orig = product.Engine.sweep_philox_windows

    def spy(self, *a, **kw):
        o = orig(self, *a, **kw)
        if kw.get("precision") == "f64":
            seen.append((self._flags_on, self.fused_last_call))
        return o

    monkeypatch.setattr(product.Engine, "sweep_philox_windows", spy)
    return seen


@pytest.mark.parametrize("kind", ["chimera", "pmj"])
def test_run_equals_sweep_by_sweep(product, monkeypatch, fused_calls, kind):
    J, h = chimera() if kind == "chimera" else pmj()

    def go():
        obj = product.NMC(J, h, rng="philox", seed=31, lbp="host", precision="f64")
        with contextlib.redirect_stdout(io.StringIO()):
            return obj.run(num_sweeps_initial=30, num_sweeps_per_NMC_phase=20, num_NMC_cycles=2, **LBP)

    M1, E1, m1 = go()
    assert any(fl and fz for fl, fz in fused_calls)             # phases with flags ran on the fused fp64 kernel
    fused_calls.clear()
    monkeypatch.setenv("NLMC_NO_FUSED64", "1")
    M2, E2, m2 = go()
    assert not any(fz for _, fz in fused_calls)
    assert M1.shape == (J.shape[0], 2 * 3 * 20)
    assert np.array_equal(M1, M2) and np.array_equal(E1, E2) and m1 == m2


def test_one_cycle_restated_with_the_oracle(product, fused_calls):
    """NMC_subroutine for one cycle (C, NC, ALL) on Chimera-2048 divided by max|J|: every recorded column is the oracle's fp64
    sweep with the phase's flags at the run's sweep indices, every hand-off the first argmin of the oracle's energies."""
    import nlmc_amd as P
    W, h = chimera()
    s = np.max(np.abs(W.data))
    J, h = (W / s).tocsr(), h / s
    N, S, beta, tx, seed = J.shape[0], 12, 2.5, 20.0, 47
    obj = product.NMC(J, h, rng="philox", seed=seed, lbp="host", precision="f64")
    m_star = np.sign(2 * np.random.default_rng(5).random(N) - 1)
    cl = np.sort(np.random.default_rng(6).choice(N, N // 8, replace=False))
    t0 = obj._sweep_counter
    with contextlib.redirect_stdout(io.StringIO()):
        M, E, emin, _ = obj.NMC_subroutine(m_star, 1, S, 1, 1, beta, tx, all_clusters=cl, tolerance=np.finfo(float).eps, **LBP)
    assert sum(1 for fl, fz in fused_calls if fl and fz) == 2     # phases C and NC on the fused fp64 kernel
    csr = oracle.Csr(J)
    cb = np.tile(np.array(oracle.cb_pair(beta, tx, True)), (S, 1))
    m = m_star.astype(np.int8)
    for k, phase in enumerate(("C", "NC", "ALL")):
        fl = P.hostlogic.phase_flags(N, m, cl, phase)
        Mo, _, _ = oracle.sweeps_philox(csr, h, m, cb, seed, 0, sweep0=t0, flags=None if phase == "ALL" else fl, use_f64=True)
        assert np.array_equal(M[:, k * S:(k + 1) * S].T, Mo), phase
        en = np.array([oracle.energy(csr, h, Mo[t]) for t in range(S)])
        assert np.allclose(E[k * S:(k + 1) * S], en, rtol=0, atol=1e-9), phase
        m = Mo[int(np.argmin(en))].copy()
        t0 += S
    assert obj._sweep_counter == t0
    assert emin == np.min(E)


@pytest.mark.parametrize("kind,given", [("pmj", False), ("pmj", True), ("chimera", True)])
def test_run_restarts_device_host_and_sweep_by_sweep(product, monkeypatch, fused_calls, kind, given):
    J, h = (chimera() if kind == "chimera" else pmj(600))
    N, R = J.shape[0], 6
    kw = dict(num_sweeps_initial=20, num_sweeps_per_NMC_phase=12, num_NMC_cycles=2, temp_x=20, global_beta=2.5,
              all_clusters=np.arange(0, N, 7) if given else None, lambda_start=3.0, lambda_end=0.05, lambda_reduction_factor=0.8,
              threshold_initial=0.9999, threshold_cutoff=0.97)
    res = []
    for force_host, off in ((False, False), (True, False), (False, True)):
        if off:
            monkeypatch.setenv("NLMC_NO_FUSED64", "1")
        fused_calls.clear()
        obj = product.NMC(J, h, rng="philox", seed=9, lbp="device", precision="f64")
        with contextlib.redirect_stdout(io.StringIO()):
            res.append(obj.run_restarts(R, _force_host=force_host, **kw))
        assert any(fl and fz for fl, fz in fused_calls) != off
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert np.array_equal(a, b)
    assert res[0][2].shape == (R, 1 + 2 * 3)


def test_precision_argument_checks(product):
    J, h = make_instance(300, seed=3)
    with pytest.raises(ValueError):
        product.NMC(J, h, rng="numpy", precision="f64")
    with pytest.raises(ValueError):
        product.NMC(J, h, rng="philox", precision="f16")
    assert product.NMC(J, h, rng="philox", precision="f64").precision == "f64"
    assert product.NMC(J, h, rng="philox").precision == "f32"
