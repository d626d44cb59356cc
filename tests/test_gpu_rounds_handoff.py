"""Rounds inside k_rounds_fused launches with the pairwise energy hand-off (include/nlmc.h: nlmc_pt_rounds_fused, and
nlmc_pt_rounds_deferred where it takes that route): a chain publishes its energy per round and slot, waits for its swap partner's
record alone, carries the next round's first two uniform tables over from this round's tail and keeps its K tables while its slot
stays.  Every case against the same rounds driven with a sweep launch and a swap launch each: spins, tracked energies, slot maps
and the swap log must be the same bits."""
import functools

import numpy as np
import pytest

from helpers import make_instance, init_spins
from test_gpu_fused64 import integer_instance

pytestmark = pytest.mark.gpu
SEED = 0x5EED0017
IN_LAUNCH, PER_ROUND = "in launch", "launch per round"


def drive(product, inst, G, L, T, rounds, pairs, precision, m0, entry=None, split=None, route=None, betas=None, slot_keys=False):
    """entry None: sweep launch + swap launch per round; "fused" / "deferred": the rounds through that entry point, cut as `split`
    says, on the route `route`.  slot_keys: the chains' RNG keys follow their slots.  -> spins, tracked energies, slot map, log
    pairs, log decisions."""
    betas = np.geomspace(0.1, 3.0, L) if betas is None else betas
    with product.Engine(inst, None, G) as eng:
        eng.set_spins(m0)
        eng.pt_init(betas)
        if slot_keys:
            eng.apt_shard(betas, 1, 0)      # one block of the ladder: random numbers keyed by (ladder, slot) instead of the chain
        # fused windows hold at least three sweeps (the ring of three uniform tables): shorter rounds have no such plan
        assert eng.plan_philox_fused(0, rounds, T, SEED) == (rounds if T >= 3 else 0)
        eng.pt_plan(0, rounds, SEED, pairs)
        eng.pt_log_begin(0, rounds, pairs)

        def one_by_one(r0, k):
            for r in range(r0, r0 + k):
                eng.sweep_philox(T, SEED, sweep0=r * T, beta=None, precision=precision)
                eng.pt_swap_philox(r, SEED, pairs, want_log=False)

        if entry is None:
            one_by_one(0, rounds)
        else:
            assert eng.last_rounds_route() is None
            batch = eng.pt_rounds_fused if entry == "fused" else eng.pt_rounds_deferred
            at = 0
            for k in (split or [rounds]):
                ran = batch(k, T, SEED, at * T, at, pairs, precision=precision)
                if T >= 3:
                    assert ran, getattr(eng, "rounds_fused_refusal", "")
                    assert eng.last_rounds_route() == route
                else:
                    # refused before anything ran; the caller drives the rounds one by one (include/nlmc.h)
                    assert not ran and "plan" in eng.rounds_fused_refusal and eng.last_rounds_route() is None
                    one_by_one(at, k)
                at += k
        p, a = eng.pt_log_read()
        return eng.get_spins(), eng.energy(), eng.pt_slots(), p, a


def same(got, ref, what):
    for name, x, y in zip(("spins", "energies", "slots", "log pairs", "log decisions"), got, ref):
        assert np.array_equal(x, y), (what, name)


# ---- window lengths: +-J, 3 ladders of 8, 3 pairs per round; 9 rounds ----------------------------------------------------------
WN, WL, WNL, WROUNDS, WPAIRS = 2000, 8, 3, 9, 3


@functools.lru_cache(maxsize=None)
def window_case(product, T, precision):
    """Instance, start and the launch-per-round reference of one (T, precision), computed once."""
    J, h = make_instance(WN, seed=17)
    inst = product.Instance(J, h)
    m0 = init_spins(WL * WNL, WN)
    ref = drive(product, inst, WL * WNL, WL, T, WROUNDS, WPAIRS, precision, m0)
    for x in ref:
        x.setflags(write=False)
    return inst, m0, ref


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
def test_window_lengths_and_launch_cuts(product, T, precision):
    """T = 1, 2: rounds too short for a fused window, so nothing can be carried either: both entry points refuse, nothing has run,
    and the rounds driven one by one behind the refusals give the reference.  T = 3, 4, 5: the three residues of T mod 3, i.e. the
    three ways the carried tables are moved to ring slots 0 and 1.  [9]: first and last round of one launch;
    [4, 5]: carried tables end with a launch; [1, 1, 7]: launches of one round."""
    inst, m0, ref = window_case(product, T, precision)
    G = WL * WNL
    assert ref[4].sum() > 0 and not np.array_equal(ref[2], np.arange(G) % WL)          # swaps happened
    for split in ([9], [4, 5], [1, 1, 7]):
        got = drive(product, inst, G, WL, T, WROUNDS, WPAIRS, precision, m0, "deferred", split, IN_LAUNCH)
        same(got, ref, ("deferred", split))
    same(drive(product, inst, G, WL, T, WROUNDS, WPAIRS, precision, m0, "fused", [9], IN_LAUNCH), ref, "fused")


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_same_call_twice_same_bits(product, precision):
    inst, m0, ref = window_case(product, 4, precision)
    G = WL * WNL
    a = drive(product, inst, G, WL, 4, WROUNDS, WPAIRS, precision, m0, "deferred", [9], IN_LAUNCH)
    b = drive(product, inst, G, WL, 4, WROUNDS, WPAIRS, precision, m0, "deferred", [9], IN_LAUNCH)
    same(a, b, "twice")
    same(a, ref, "reference")


@pytest.mark.parametrize("case", ["integer_diag", "gaussian"])
def test_other_entry_formats(product, case):
    """Compact entries + diagonal + fields + hub rows (fp64 mode), Gaussian couplings (wide entries, f32 mode), T = 4."""
    N, L, nl, T, rounds, pairs = 3000, 6, 2, 4, 4, 2
    if case == "integer_diag":
        J, h = integer_instance(N, 4, wmax=2, diag=True, h_step=0.25)
        precision = "f64"
    else:
        J, h = make_instance(N, seed=9, with_h=True, gaussian=True)
        precision = "f32"
    inst = product.Instance(J, h)
    G = L * nl
    m0 = init_spins(G, N)
    ref = drive(product, inst, G, L, T, rounds, pairs, precision, m0)
    for split in ([4], [1, 3]):
        same(drive(product, inst, G, L, T, rounds, pairs, precision, m0, "deferred", split, IN_LAUNCH), ref, split)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_single_pair_most_chains_never_wait(product, precision):
    """n_pairs = 1: two chains of a ladder meet per round, the others run on without waiting for anybody.  (A narrow ladder, so that
    some of the 18 decisions are acceptances and slots do change.)"""
    N, L, nl, T, rounds = 2000, 8, 2, 4, 9
    J, h = make_instance(N, seed=23)
    inst = product.Instance(J, h)
    G = L * nl
    m0 = init_spins(G, N)
    betas = np.linspace(0.95, 1.05, L)
    ref = drive(product, inst, G, L, T, rounds, 1, precision, m0, betas=betas)
    assert ref[4].sum() > 0
    for split in ([9], [2, 7]):
        same(drive(product, inst, G, L, T, rounds, 1, precision, m0, "deferred", split, IN_LAUNCH, betas=betas), ref, split)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_route_selection(product, precision, monkeypatch):
    """Default: the rounds run in launch.  NLMC_NO_PERSISTENT=1 (read when the engine is created): a launch per round
    (k_sweep_fused<.., DEFER>) -- the same bits -- and nlmc_pt_rounds_fused refuses."""
    T = 4
    inst, m0, ref = window_case(product, T, precision)
    G = WL * WNL
    same(drive(product, inst, G, WL, T, WROUNDS, WPAIRS, precision, m0, "deferred", [4, 5], IN_LAUNCH), ref, "default")
    monkeypatch.setenv("NLMC_NO_PERSISTENT", "1")
    same(drive(product, inst, G, WL, T, WROUNDS, WPAIRS, precision, m0, "deferred", [4, 5], PER_ROUND), ref, "NLMC_NO_PERSISTENT")
    with product.Engine(inst, None, G) as eng:
        eng.set_spins(m0)
        eng.pt_init(np.geomspace(0.1, 3.0, WL))
        assert eng.plan_philox_fused(0, 2, T, SEED) == 2
        eng.pt_plan(0, 2, SEED, WPAIRS)
        assert not eng.pt_rounds_fused(2, T, SEED, 0, 0, WPAIRS, precision=precision) and "NLMC_NO_PERSISTENT" in eng.rounds_fused_refusal
        assert eng.last_rounds_route() is None


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_rng_keys_that_follow_the_slot(product, precision):
    """A context whose random numbers are keyed by (ladder, slot): a swap changes the chain's key, so no uniform tables are carried
    from round to round (the K tables are still kept while the slot stays).  A narrow ladder: slots do change."""
    N, L, nl, T, rounds, pairs = 2000, 8, 2, 4, 9, 3
    J, h = make_instance(N, seed=29)
    inst = product.Instance(J, h)
    G = L * nl
    m0 = init_spins(G, N)
    betas = np.linspace(0.9, 1.1, L)
    ref = drive(product, inst, G, L, T, rounds, pairs, precision, m0, betas=betas, slot_keys=True)
    assert ref[4].sum() > 0 and not np.array_equal(ref[2], np.arange(G) % L)
    plain = drive(product, inst, G, L, T, rounds, pairs, precision, m0, betas=betas)
    assert not np.array_equal(plain[0], ref[0])                                      # the keys do differ
    for split in ([9], [4, 5]):
        same(drive(product, inst, G, L, T, rounds, pairs, precision, m0, "deferred", split, IN_LAUNCH, betas=betas, slot_keys=True), ref, split)


def test_call_longer_than_a_launch_holds(product):
    """1100 rounds in one call: the host cuts it into launches of 1024 and 76 rounds (the rows of the record array), each with its own
    windows, pair selections and log rows."""
    N, L, T, rounds, pairs = 300, 4, 3, 1100, 1
    J, h = make_instance(N, seed=31)
    inst = product.Instance(J, h)
    m0 = init_spins(L, N)
    betas = np.linspace(0.95, 1.05, L)
    ref = drive(product, inst, L, L, T, rounds, pairs, "f64", m0, betas=betas)
    assert ref[4][1024:].sum() > 0
    same(drive(product, inst, L, L, T, rounds, pairs, "f64", m0, "deferred", [rounds], IN_LAUNCH, betas=betas), ref, "1100")
