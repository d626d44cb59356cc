"""The exact Boltzmann law under tempering rounds inside k_rounds_lanes launches (csrc/nlmc_lane_rounds.h), judged as
tests/test_gpu_stationarity.py judges the other rounds routes (rounds_case): chains start in equilibrium at their slot's temperature,
run 15 rounds of T sweeps + a swap round of L // 3 pairs through Engine.pt_rounds_lanes, and every slot must still show its exact
law -- state histogram, mean energy, adjacent correlation, and the swap acceptance rates -- under that file's thresholds, the
rejection of the deliberately wrong laws included.  Block instance DYADIC x 170 copies (N = 1020, just inside the lane kernels'
limit of 1024 spins), all ladders in ONE context: this route has no residency condition, so nothing is batched by 64 ladders."""
import numpy as np
import pytest

import exactlaw as xl
from test_gpu_stationarity import COPIES, DYADIC, PT_BETAS, case_seeds, judge_rounds, oracle_ladder, pt_ladders

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("precision,layout", [("f32", "contiguous"), ("f64", "strided")])
def test_rounds_in_lane_launches_keep_the_law(product, precision, layout):
    L, T, rounds = len(PT_BETAS), 4 if precision == "f32" else 3, 15
    pairs, nl = L // 3, pt_ladders()
    G = nl * L
    name = f"rounds lanes {precision} {layout} ladders={nl}"
    start_seed, seed = case_seeds(name)
    bi = xl.BlockInstance(DYADIC, COPIES, layout)
    assert bi.J.shape[0] == 1020
    inst = product.Instance(bi.J, bi.h)
    m0 = xl.equilibrium_start(np.random.default_rng(start_seed), bi, np.tile(PT_BETAS, nl))
    with product.Engine(inst, None, G) as eng:
        eng.set_spins(m0)
        eng.pt_init(PT_BETAS)
        eng.pt_plan(0, rounds, seed, pairs)
        eng.pt_log_begin(0, rounds, pairs)
        assert eng.pt_rounds_lanes(rounds, T, seed, 0, 0, pairs, precision=precision), getattr(eng, "rounds_fused_refusal", "")
        assert eng.last_rounds_route() == "lanes" and eng.last_sweep_route() == "lanes"
        eng.pt_check()
        p, a = eng.pt_log_read()
        spins, slots = eng.get_spins(), eng.pt_slots()
    for g in (1, nl - 1):
        s, sl = oracle_ladder(bi, inst, m0, g, G, T, rounds, pairs, precision, seed)
        assert np.array_equal(spins[g * L:(g + 1) * L], s) and np.array_equal(slots[g * L:(g + 1) * L], sl), f"ladder {g}"
    judge_rounds(name, bi, spins, slots, p, a)
