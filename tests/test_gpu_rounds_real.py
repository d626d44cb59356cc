"""Real-valued fp64 rounds inside k_rounds_fused launches (k_rounds_fused<.., R64>; include/nlmc.h: nlmc_pt_rounds_fused with
nlmc_set_fused_f64_real on): the chains stay in LDS from round to round, take their couplings and fields from the windows' fp64
value plane, and carry the next round's first two uniform tables over from this round's tail.  Every case against the same rounds
driven with one sweep launch and one swap launch per round on an engine set up the same way: spins, recomputed and tracked
energies, slot maps, log pairs and log decisions must be the same bits."""
import functools

import numpy as np
import pytest

import oracle
from helpers import make_instance, init_spins
from test_gpu_fused64_real import real_instance, normalised

pytestmark = pytest.mark.gpu
SEED = 0x5EED0A07
IN_LAUNCH, PER_ROUND = "in launch", "launch per round"
# Which route nlmc_pt_rounds_deferred takes by default for a real-valued instance (include/nlmc.h)
DEFERRED_DEFAULT_REAL = PER_ROUND
NARROW = functools.partial(np.linspace, 0.95, 1.05)          # a ladder on which swaps are accepted


def drive(product, inst, G, L, T, rounds, pairs, m0, entry=None, split=None, route=None, betas=None, slot_keys=False, real=True):
    """entry None: sweep launch + swap launch per round; "fused" / "deferred": the rounds through that entry point, cut as `split`
    says, on the route `route`.  slot_keys: the chains' RNG keys follow their slots.  -> spins, recomputed energies, tracked
    energies, slot map, log pairs, log decisions."""
    betas = np.geomspace(0.1, 3.0, L) if betas is None else betas
    with product.Engine(inst, None, G) as eng:
        eng.set_fused_f64_real(real)
        eng.set_spins(m0)
        eng.pt_init(betas)
        if slot_keys:
            eng.apt_shard(betas, 1, 0)
        assert eng.plan_philox_fused(0, rounds, T, SEED) == rounds
        eng.pt_plan(0, rounds, SEED, pairs)
        eng.pt_log_begin(0, rounds, pairs)
        if entry is None:
            for r in range(rounds):
                eng.sweep_philox(T, SEED, sweep0=r * T, beta=None, precision="f64")
                eng.pt_swap_philox(r, SEED, pairs, want_log=False)
        else:
            assert eng.last_rounds_route() is None
            batch = eng.pt_rounds_fused if entry == "fused" else eng.pt_rounds_deferred
            at = 0
            for k in (split or [rounds]):
                assert batch(k, T, SEED, at * T, at, pairs, precision="f64"), getattr(eng, "rounds_fused_refusal", "")
                assert eng.last_rounds_route() == route
                at += k
        p, a = eng.pt_log_read()
        return eng.get_spins(), eng.energy(), eng.energy_tracked(), eng.pt_slots(), p, a


def same(got, ref, what):
    for name, x, y in zip(("spins", "energies", "tracked energies", "slots", "log pairs", "log decisions"), got, ref):
        assert np.array_equal(x, y), (what, name)


def swaps_happened(ref, G, L):
    return ref[5].sum() > 0 and not np.array_equal(ref[3], np.arange(G) % L)


def frozen(ref):
    for x in ref:
        x.setflags(write=False)
    return ref


# ---- window lengths: Gaussian couplings + hub rows (lane pairs), 2 ladders of 8, 3 pairs per round, 9 rounds ---------------------
WN, WL, WNL, WROUNDS, WPAIRS = 2048, 8, 2, 9, 3


@functools.lru_cache(maxsize=None)
def window_case(product, T):
    """Instance, start and the launch-per-round reference of one T, computed once."""
    J, h = real_instance(WN, 31)
    inst = product.Instance(J, h)
    m0 = init_spins(WL * WNL, WN)
    return inst, m0, frozen(drive(product, inst, WL * WNL, WL, T, WROUNDS, WPAIRS, m0, betas=NARROW(WL)))


@pytest.mark.parametrize("T", [3, 4, 5])
def test_window_lengths_and_launch_cuts(product, T):
    """The three residues of T mod 3 = the three ways the carried tables are moved to ring slots 0 and 1.  [9]: first and last round
    of one launch; [4, 5]: carried tables end with a launch; [1, 1, 7]: launches of one round."""
    inst, m0, ref = window_case(product, T)
    G = WL * WNL
    assert swaps_happened(ref, G, WL)
    for split in ([9], [4, 5], [1, 1, 7]):
        same(drive(product, inst, G, WL, T, WROUNDS, WPAIRS, m0, "fused", split, IN_LAUNCH, betas=NARROW(WL)), ref, split)


def test_real_diagonal(product):
    """A real diagonal: the DIAG variant of the kernel."""
    N, L, nl, T, rounds, pairs = 2048, 6, 2, 4, 4, 2
    J, h = real_instance(N, 7, diag=True)
    inst = product.Instance(J, h)
    G = L * nl
    m0 = init_spins(G, N)
    ref = drive(product, inst, G, L, T, rounds, pairs, m0)
    for split in ([4], [1, 3]):
        same(drive(product, inst, G, L, T, rounds, pairs, m0, "fused", split, IN_LAUNCH), ref, split)


def test_rng_keys_that_follow_the_slot(product):
    """Random numbers keyed by (ladder, slot): a swap changes the chain's key, so nothing is carried from round to round."""
    T = 4
    inst, m0, plain = window_case(product, T)
    G = WL * WNL
    ref = drive(product, inst, G, WL, T, WROUNDS, WPAIRS, m0, betas=NARROW(WL), slot_keys=True)
    assert swaps_happened(ref, G, WL)
    assert not np.array_equal(plain[0], ref[0])                                      # the keys do differ
    for split in ([9], [4, 5]):
        same(drive(product, inst, G, WL, T, WROUNDS, WPAIRS, m0, "fused", split, IN_LAUNCH, betas=NARROW(WL), slot_keys=True), ref, split)


def test_single_pair_most_chains_never_wait(product):
    """n_pairs = 1: two chains of a ladder meet per round, the others run on without waiting for anybody."""
    T = 4
    inst, m0, _ = window_case(product, T)
    G = WL * WNL
    ref = drive(product, inst, G, WL, T, WROUNDS, 1, m0, betas=NARROW(WL))
    assert swaps_happened(ref, G, WL)
    for split in ([9], [2, 7]):
        same(drive(product, inst, G, WL, T, WROUNDS, 1, m0, "fused", split, IN_LAUNCH, betas=NARROW(WL)), ref, split)


def test_no_pairs_against_the_fp64_oracle(product):
    """n_pairs = 0: four chains at fixed temperatures, 4 rounds of 5 sweeps in one launch == the sequential fp64 oracle's 20 sweeps."""
    N, L, T, rounds = 2048, 4, 5, 4
    J, h = real_instance(N, 31)
    inst = product.Instance(J, h)
    m0 = init_spins(L, N)
    betas = np.geomspace(0.1, 3.0, L)
    with product.Engine(inst, None, L) as eng:
        eng.set_fused_f64_real(True)
        eng.set_spins(m0)
        E0, esc = eng.energy(), eng.energy_scale
        eng.pt_init(betas)
        assert eng.plan_philox_fused(0, rounds, T, SEED) == rounds
        assert eng.pt_rounds_fused(rounds, T, SEED, 0, 0, 0, precision="f64"), getattr(eng, "rounds_fused_refusal", "")
        assert eng.last_rounds_route() == IN_LAUNCH
        got, slots = eng.get_spins(), eng.pt_slots()
    assert np.array_equal(slots, np.arange(L))
    csr = oracle.Csr(J)
    for c in (0, 1, L - 1):
        cb = np.tile(np.array(oracle.cb_pair(betas[c], 1.0, True)), (rounds * T, 1))
        _, s_fin, _ = oracle.sweeps_philox(csr, h, m0[c], cb, SEED, c, escale=esc, use_f64=True,
                                           efix0=int(np.rint(E0[c] * 2.0 ** esc)), want_M=False)
        assert np.array_equal(got[c], s_fin), f"chain {c}"


@pytest.mark.parametrize("kind", ["chimera", "DCL"])
def test_reference_instances(product, kind):
    """Chimera-2048 (couplings k/75) and DCL C8 (k/7) divided by max|J|: one ladder of 32, 4 rounds of 5 sweeps, 10 pairs."""
    J, h = normalised(kind)
    N, L, T, rounds, pairs = J.shape[0], 32, 5, 4, 10
    inst = product.Instance(J, h)
    m0 = init_spins(L, N)
    betas = np.geomspace(0.1, 4.0, L)
    ref = drive(product, inst, L, L, T, rounds, pairs, m0, betas=betas)
    same(drive(product, inst, L, L, T, rounds, pairs, m0, "fused", [rounds], IN_LAUNCH, betas=betas), ref, kind)


def test_call_longer_than_a_launch_holds(product):
    """1100 rounds in one call: launches of 1024 and 76 rounds, each with its own windows, value planes, pair selections, log rows."""
    N, L, T, rounds, pairs = 300, 4, 3, 1100, 1
    J, h = make_instance(N, seed=31, with_h=True, gaussian=True)
    inst = product.Instance(J, h)
    m0 = init_spins(L, N)
    ref = drive(product, inst, L, L, T, rounds, pairs, m0, betas=NARROW(L))
    assert ref[5][1024:].sum() > 0
    same(drive(product, inst, L, L, T, rounds, pairs, m0, "fused", [rounds], IN_LAUNCH, betas=NARROW(L)), ref, "1100")


def test_same_call_twice_same_bits(product):
    inst, m0, ref = window_case(product, 4)
    G = WL * WNL
    a = drive(product, inst, G, WL, 4, WROUNDS, WPAIRS, m0, "fused", [9], IN_LAUNCH, betas=NARROW(WL))
    b = drive(product, inst, G, WL, 4, WROUNDS, WPAIRS, m0, "fused", [9], IN_LAUNCH, betas=NARROW(WL))
    same(a, b, "twice")
    same(a, ref, "reference")


def test_option_off_refuses(product):
    """Without nlmc_set_fused_f64_real the entry point refuses a real-valued instance, names the fp64 mode and runs nothing."""
    inst, m0, _ = window_case(product, 4)
    G = WL * WNL
    with product.Engine(inst, None, G) as eng:
        eng.set_spins(m0)
        eng.pt_init(NARROW(WL))
        assert eng.plan_philox_fused(0, 2, 4, SEED) == 2
        eng.pt_plan(0, 2, SEED, WPAIRS)
        assert not eng.pt_rounds_fused(2, 4, SEED, 0, 0, WPAIRS, precision="f64")
        assert "fp64" in eng.rounds_fused_refusal and eng.last_rounds_route() is None
        assert np.array_equal(eng.get_spins(), m0) and np.array_equal(eng.pt_slots(), np.arange(G) % WL)


def test_pmj_instance_keeps_the_integer_threshold_kernel(product):
    """A +-J instance with the option on: the plans carry a value plane, the rounds stay on the integer-threshold kernel."""
    N, L, nl, T, rounds, pairs = 2000, 8, 2, 4, 4, 3
    J, h = make_instance(N, seed=13)
    inst = product.Instance(J, h)
    G = L * nl
    m0 = init_spins(G, N)
    ref = drive(product, inst, G, L, T, rounds, pairs, m0, betas=NARROW(L), real=False)
    off = drive(product, inst, G, L, T, rounds, pairs, m0, "fused", [rounds], IN_LAUNCH, betas=NARROW(L), real=False)
    on = drive(product, inst, G, L, T, rounds, pairs, m0, "fused", [rounds], IN_LAUNCH, betas=NARROW(L), real=True)
    same(off, ref, "option off")
    same(on, off, "option on")


def test_deferred_route(product, monkeypatch):
    """nlmc_pt_rounds_deferred on a real-valued instance: the documented default route, and a launch per round with
    NLMC_NO_PERSISTENT=1 (read when the engine is created) -- the same bits either way."""
    T = 4
    inst, m0, ref = window_case(product, T)
    G = WL * WNL
    same(drive(product, inst, G, WL, T, WROUNDS, WPAIRS, m0, "deferred", [4, 5], DEFERRED_DEFAULT_REAL, betas=NARROW(WL)), ref, "default")
    monkeypatch.setenv("NLMC_NO_PERSISTENT", "1")
    same(drive(product, inst, G, WL, T, WROUNDS, WPAIRS, m0, "deferred", [4, 5], PER_ROUND, betas=NARROW(WL)), ref, "NLMC_NO_PERSISTENT")
