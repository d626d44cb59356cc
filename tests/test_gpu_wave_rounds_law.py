"""The exact Boltzmann law under tempering rounds inside k_rounds_waves launches (csrc/nlmc_wave_rounds.h), judged as
tests/test_gpu_lane_rounds_law.py judges the lane rounds: chains start in equilibrium at their slot's temperature, run 15 rounds of T
sweeps + a swap round of L // 3 pairs through Engine.pt_rounds_waves -- cut into three calls, so the law is that of a composition of
launches, each with its own field prologue and slot maps -- and every slot must still show its exact law: state histogram, mean
energy, adjacent correlation and the swap acceptance rates, under test_gpu_stationarity's thresholds, the rejection of the deliberately
wrong laws included.  Block instance DYADIC x 42 copies (N = 252, just inside the wave kernels' limit of 256 spins: four fields per
lane); the number of ladders comes from the exact variances by that file's rule (chains_per_slot), so the resolution is the same."""
import numpy as np
import pytest

import exactlaw as xl
from test_gpu_stationarity import DYADIC, PT_BETAS, ROUNDS_M, case_seeds, chains_per_slot, judge_rounds, oracle_ladder

pytestmark = pytest.mark.gpu
COPIES = 42


def test_rounds_in_wave_launches_keep_the_law(product):
    L, T, rounds, cuts = len(PT_BETAS), 4, 15, (4, 1, 10)
    pairs, nl = L // 3, max(1024, chains_per_slot(DYADIC, PT_BETAS, COPIES, ROUNDS_M))
    G = nl * L
    name = f"rounds waves f32 contiguous ladders={nl}"
    start_seed, seed = case_seeds(name)
    bi = xl.BlockInstance(DYADIC, COPIES, "contiguous")
    assert bi.J.shape[0] == 252
    inst = product.Instance(bi.J, bi.h)
    m0 = xl.equilibrium_start(np.random.default_rng(start_seed), bi, np.tile(PT_BETAS, nl))
    with product.Engine(inst, None, G) as eng:
        eng.set_spins(m0)
        eng.pt_init(PT_BETAS)
        eng.pt_plan(0, rounds, seed, pairs)
        eng.pt_log_begin(0, rounds, pairs)
        at = 0
        for k in cuts:
            assert eng.pt_rounds_waves(k, T, seed, at * T, at, pairs), getattr(eng, "rounds_fused_refusal", "")
            assert eng.last_rounds_route() == "waves" and eng.last_sweep_route() == "waves"
            at += k
        eng.pt_check()
        p, a = eng.pt_log_read()
        spins, slots = eng.get_spins(), eng.pt_slots()
    for g in (1, nl - 1):
        s, sl = oracle_ladder(bi, inst, m0, g, G, T, rounds, pairs, "f32", seed)
        assert np.array_equal(spins[g * L:(g + 1) * L], s) and np.array_equal(slots[g * L:(g + 1) * L], sl), f"ladder {g}"
    judge_rounds(name, bi, spins, slots, p, a)
