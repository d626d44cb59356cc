"""The exact Boltzmann law under APT rounds inside k_apt_rounds_lanes launches (csrc/nlmc_lane_apt.h), judged as
tests/test_gpu_stationarity.py::test_apt_rounds judges the round-by-round route: the same block instance (DYADIC x 170 copies,
N = 1020), K = 8 sub-replicas x 8 temperatures, 10 rounds of 3 sweeps + Houdayer moves + swaps of L // 3 pairs, the same number of
independent runs of 64 chains (a fresh seed each, one engine), equilibrium starts, and that file's Verdict with its thresholds
unchanged, the rejection of the deliberately wrong laws included.  katzgraber=True stays and no picked cluster may exceed N / 2 (the
global flip is not an invariant move when h != 0; blocks of 6 spins never get there).  The first run is reproduced whole by the
protocol over the oracle double.  N = 1020 with K = L = 8 is the largest system of one wave: 64 KB of spins + 64 KB of labels."""
import numpy as np
import pytest

import exactlaw as xl
from fake_engine import OracleEngine
from test_gpu_stationarity import APT_M, COPIES, DYADIC, PT_BETAS, case_seeds, chains_per_slot, conclude

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("precision,layout", [("f32", "contiguous"), ("f64", "strided")])
def test_apt_rounds_in_lane_launches_keep_the_law(product, precision, layout):
    K, R, T, rounds = 8, len(PT_BETAS), 3, 10
    pairs, G = R // 3, K * R
    runs = -(-max(1024, chains_per_slot(DYADIC, PT_BETAS, COPIES, APT_M)) // K)
    bi = xl.BlockInstance(DYADIC, COPIES, layout)
    assert bi.n == 1020
    inst = product.Instance(bi.J, bi.h)
    name = f"APT lanes {precision} {layout} runs={runs}"
    start_seed, seed0 = case_seeds(name)
    start = xl.equilibrium_start(np.random.default_rng(start_seed), bi, np.tile(PT_BETAS, runs * K)).reshape(runs, G, bi.n)
    identity = (np.arange(G) % R).astype(np.int32)

    def by_slot(spins, slots):
        cfg = np.empty((K, R, bi.n), np.int8)
        cfg[np.arange(G) // R, slots] = spins
        return cfg

    out, moved, accepted = [], 0, 0
    with product.Engine(inst, None, G) as eng:
        eng.pt_init(PT_BETAS)
        for r in range(runs):
            seed = seed0 + (r << 20)
            eng.set_spins(start[r])
            eng.pt_set_slots(identity)
            eng.pt_plan(0, rounds, seed, pairs)
            eng.pt_log_begin(0, rounds, pairs)
            ok, info = eng.apt_rounds_lanes(rounds, T, seed, 0, 0, pairs, katzgraber=True, precision=precision, want_info=True)
            assert ok, getattr(eng, "rounds_fused_refusal", "")
            assert eng.last_rounds_route() == "apt lanes" and eng.last_sweep_route() == "lanes"
            assert info[:, :, 1].max() <= bi.n // 2
            eng.pt_check()
            moved += int((info[:, :, 1] > 0).sum())
            accepted += int(eng.pt_log_read()[1].sum())
            out.append(by_slot(eng.get_spins(), eng.pt_slots()))
    assert moved > runs and accepted > runs
    o = OracleEngine(inst, G, 0, G)
    o.pt_init(PT_BETAS)
    o.set_spins(start[0])
    for rnd in range(rounds):
        o.sweep_philox(T, seed0, sweep0=rnd * T, precision=precision)
        o.icm_round_ladders(rnd, seed0, True)
        o.pt_swap_philox(rnd, seed0, pairs)
    assert np.array_equal(out[0], by_slot(o.get_spins(), o.pt_slots()))
    cfg = np.stack(out)                                                             # [runs, K, R, n]
    v = xl.Verdict(name)
    for r, b in enumerate(PT_BETAS):
        v.add_slot(f"slot{r}", bi, cfg[:, :, r].reshape(runs * K, -1), b)
        for k, spc in enumerate(bi.species):
            v.add(f"slot{r} overlap {spc.name}", xl.chi2_overlap(cfg[:, :K // 2, r], cfg[:, K // 2:, r], bi, k, xl.Law(spc, b)))
    assert v.m == APT_M
    conclude(v)
