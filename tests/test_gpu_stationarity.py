"""Sweeps, swaps and cluster moves as they are composed by the kernels and the host drivers keep the exact Boltzmann law.

The rest of the GPU suite ties every kernel to the sequential spec bit for bit, and test_gpu_law.py ties each single update to the
heat-bath law given the field it saw.  Neither notices a mistake that spec and kernels share, or one made by a driver: a counter
used twice, a tag collision, a round index that does not advance, a hand-off that reuses a uniform table.  Here the instance is a
disjoint union of 6-spin blocks (tests/exactlaw.py): the block laws are known by enumeration, every chain starts from an exact
equilibrium sample at its slot's temperature, and every correct transition leaves that law invariant -- so after any number of
windows or rounds the block states are exact independent samples of a known finite distribution.

Every case asserts the route it is meant for ran (a silent fallback fails), reproduces named chains with the oracle bit for bit
(that guards "did nothing" and the start-state plumbing), then applies the rule of exactlaw per temperature slot, with the
configurations read by slot: family-wise ALPHA = 1e-4 with Bonferroni over the m statistics of the case; delta* <= 1e-2 at every
slot (the sample sizes are computed from the exact variances to meet it); pooled chi-square cells hold <= 5 % of the exact mass;
the same sample against beta (1 + 2 delta*) -- and, where swaps run, the acceptance counts against the expectation with the sign of
dBeta dE flipped -- must reject.  No number here is measured against the code under test.

Shapes: N = 1020 (170 blocks: below the lane limit 1024, above the fused minimum 256) in a contiguous and a strided block layout
(the Philox calls of four spins, the fused schedule, the lane kernel and the LDS chunks cut the index range differently), windows
of 3-5 sweeps, 10-15 rounds, >= 1024 ladders of 8 slots where swaps run.

NMC cycles as a whole are non-equilibrium by design (a backbone inferred from the chain's own state, phases restarted from the
argmin) and stay out of scope; their phase flags alone are case (g).

Each test prints one STAT line: route, m, n, dof, chi2, smallest p, delta*, the weakest p among the wrong hypotheses."""

import zlib

import numpy as np
import pytest

import exactlaw as xl
import oracle
from fake_engine import OracleEngine

pytestmark = pytest.mark.gpu
SEED = 0x57A71C00 + (5 << 32)
MAX_DELTA = 1e-2                       # tests/test_gpu_law.py: MAX_DELTA
COPIES = 170                           # N = 1020
DYADIC = [xl.K6, xl.RING2]
LAYOUTS = ["contiguous", "strided"]
SWEEP_BETAS = np.geomspace(0.3, 1.2, 4)
PT_BETAS = 0.8 + 0.02 * (np.arange(8) - 3.5)          # chain energy deviation ~ 25: dBeta dE of order one
IN_LAUNCH, PER_ROUND = "in launch", "launch per round"


def case_seeds(name):
    """(seed of the start states, Philox seed) of a case, from its name: every case is an independent sample -- also the cases whose
    routes give the same bits from the same start (the dyadic species in the two arithmetics)."""
    k = zlib.crc32(name.encode())
    return k, SEED + (k & 0xFFFFF)


def chains_per_slot(species, betas, copies, m):
    """From the exact variances alone: chains per slot that give delta* <= MAX_DELTA at every slot with m statistics (+ 3 %)."""
    return int(np.ceil(1.03 * xl.blocks_needed(species, betas, copies, MAX_DELTA, m)))


def conclude(v):
    v.finish()
    print(v.summary())
    assert v.ok(), v.summary()
    assert max(v.delta) <= MAX_DELTA, v.summary()
    assert max(v.pooled) <= 0.05, v.summary()
    assert v.wrong and v.wrong_rejected(), (v.summary(), v.wrong)
    return v


def oracle_final(bi, m0, c, beta, S, use_f64, seed, order="shared", flags=None, temp_x=1.0):
    cb = np.tile(np.array(oracle.cb_pair(beta, temp_x, use_f64)), (S, 1))
    return oracle.sweeps_philox(oracle.Csr(bi.J), bi.h, m0[c], cb, seed, c, order_group=(c + 1 if order == "per_chain" else 0),
                                flags=None if flags is None else flags[c], use_f64=use_f64, want_M=False)[1]


# ---- (a) (b) (c) (h): sweep routes --------------------------------------------------------------------------------------------------
def sweep_case(product, route, species, layout, precision, T, W, betas=SWEEP_BETAS, order="shared", plan=False, ladder=False,
               real=False, lanes=False, copies=COPIES, chains=None, expect_route=None):
    """W calls of T sweeps; chain c sits on slot c % L.  ladder: the temperatures come from pt_init (beta=None), else from a table."""
    L = len(betas)
    n_species = len(species)
    m = L * (n_species + 2)
    per_slot = chains_per_slot(species, betas, copies, m) if chains is None else chains
    R = L * per_slot
    bi = xl.BlockInstance(species, copies, layout)
    beta_of = np.asarray(betas)[np.arange(R) % L]
    start_seed, seed = case_seeds(f"{route} {layout}")
    m0 = xl.equilibrium_start(np.random.default_rng(start_seed), bi, beta_of)
    with product.Engine(product.Instance(bi.J, bi.h), None, R) as eng:
        eng.set_fused_f64_real(real)
        eng.set_lane_sweeps("force" if lanes else "off")
        eng.set_spins(m0)
        if ladder:
            eng.pt_init(betas)
        planned = eng.plan_philox_fused(0, W, T, seed) if plan else 0
        assert planned == (W if plan else 0)
        if plan and precision == "f64":
            assert "f64" in eng.fused_modes(T)
        for w in range(W):
            eng.sweep_philox(T, seed, sweep0=w * T, beta=None if ladder else np.repeat(beta_of[:, None], T, axis=1),
                             precision=precision, order=order)
            assert eng.last_sweep_route() == expect_route, (w, eng.last_sweep_route())
            assert eng._last_fused() == (expect_route == "fused")
        out = eng.get_spins()
    for c in (1, R - 2):
        assert np.array_equal(out[c], oracle_final(bi, m0, c, beta_of[c], T * W, precision == "f64", seed, order)), f"chain {c}"
    assert not np.array_equal(out, m0)
    v = xl.Verdict(f"{route} {layout} R={R}")
    for i, b in enumerate(betas):
        v.add_slot(f"slot{i}", bi, out[i::L], b)
    conclude(v)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("precision,order", [("f32", "shared"), ("f64", "per_chain")])
def test_sweep_by_sweep(product, monkeypatch, precision, order, layout):
    """(a) No plan, NLMC_NO_FUSED64=1: the sweep-by-sweep kernels over consecutive calls."""
    monkeypatch.setenv("NLMC_NO_FUSED64", "1")
    sweep_case(product, f"sweep by sweep {precision} {order}", DYADIC, layout, precision, 4, 3, order=order, expect_route="stepwise")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["f32", "f64_integer", "f64_real"])
def test_fused_windows(product, kind, layout):
    """(b) Several planned fused windows at the ladder temperatures: f32, fp64 integer thresholds, and the real-valued fp64 route
    on the Gaussian species (set_fused_f64_real)."""
    T = {"f32": 5, "f64_integer": 4, "f64_real": 3}[kind]
    sweep_case(product, f"fused windows {kind}", [xl.GAUSS] if kind == "f64_real" else DYADIC, layout, "f32" if kind == "f32" else "f64",
               T, 3, plan=True, ladder=True, real=(kind == "f64_real"), expect_route="fused")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_lane_kernel(product, precision, layout):
    """(c) set_lane_sweeps("force"): a chain per lane."""
    sweep_case(product, f"lanes {precision}", DYADIC, layout, precision, 3, 4, lanes=True, expect_route="lanes")


def test_global_memory_kernels(product):
    """(h) N = 24 600 just above LDS_N: 4100 blocks, 64 chains on two slots, f32, contiguous layout."""
    copies = 4100
    # the library picks the global-memory kernels by n > NLMC_LDS_N alone (csrc/nlmc.hip: nlmc_create sets `big`), and reports
    # their sweeps as "stepwise" too: n is the route indicator there is
    assert 6 * (copies - 4) <= product._abi.LDS_N < 6 * copies
    sweep_case(product, "global memory f32", DYADIC, "contiguous", "f32", 4, 3, betas=np.array([0.8, 1.2]), copies=copies, chains=32,
               expect_route="stepwise")


# ---- (d) rounds in one launch, (e) the host drivers ---------------------------------------------------------------------------------
ROUNDS_M = 8 * 4 + 7                                    # statistics of a swap case: (i) x 2, (ii), (iii) per slot, (v) per pair


def pt_ladders():
    return max(1024, chains_per_slot(DYADIC, PT_BETAS, COPIES, ROUNDS_M))


def oracle_ladder(bi, inst, m0, g, G, T, rounds, pairs, precision, seed):
    """Ladder g (chains g L .. g L + L - 1) driven by the oracle double -> (spins [L, n], slots [L])."""
    L = len(PT_BETAS)
    o = OracleEngine(inst, L, g * L, G)
    o.pt_init(PT_BETAS)
    o.set_spins(m0[g * L:(g + 1) * L])
    for r in range(rounds):
        o.sweep_philox(T, seed, sweep0=r * T, precision=precision)
        o.pt_swap_philox(r, seed, pairs)
    return o.get_spins(), o.pt_slots()[g * L:(g + 1) * L]


def judge_rounds(route, bi, spins, slots, pairs, acc):
    L = len(PT_BETAS)
    assert acc.mean() > 0.2 and not np.array_equal(slots, np.arange(len(slots)) % L)          # swaps are accepted often
    conf = xl.by_slot(spins, slots, L)
    v = xl.Verdict(route)
    for i, b in enumerate(PT_BETAS):
        v.add_slot(f"slot{i}", bi, conf[i], b)
    v.add_acceptance(bi, PT_BETAS, pairs, acc)
    assert v.m == ROUNDS_M
    conclude(v)


def rounds_case(product, entry, precision, layout, cut, per_round):
    L, T, rounds = len(PT_BETAS), 4 if precision == "f32" else 3, 15
    pairs = L // 3
    nl = pt_ladders()
    batch = nl if per_round else 64
    nl = -(-nl // batch) * batch
    name = f"rounds {entry} {precision} {layout} cut={cut} route={'per round' if per_round else 'in launch'} ladders={nl}"
    start_seed, seed0 = case_seeds(name)
    bi = xl.BlockInstance(DYADIC, COPIES, layout)
    inst = product.Instance(bi.J, bi.h)
    m0 = xl.equilibrium_start(np.random.default_rng(start_seed), bi, np.tile(PT_BETAS, nl))
    spins, slots, lp, la = [], [], [], []
    for b in range(nl // batch):
        seed, G = seed0 + (b << 20), batch * L
        mb = m0[b * G:(b + 1) * G]
        with product.Engine(inst, None, G) as eng:
            eng.set_spins(mb)
            eng.pt_init(PT_BETAS)
            assert eng.plan_philox_fused(0, rounds, T, seed) == rounds
            eng.pt_plan(0, rounds, seed, pairs)
            eng.pt_log_begin(0, rounds, pairs)
            run = eng.pt_rounds_fused if entry == "fused" else eng.pt_rounds_deferred
            at = 0
            for k in ([rounds] if cut == "all" else [1, rounds - 1]):
                assert run(k, T, seed, at * T, at, pairs, precision=precision), getattr(eng, "rounds_fused_refusal", "")
                assert eng.last_rounds_route() == (PER_ROUND if per_round else IN_LAUNCH)
                at += k
            eng.pt_check()
            p, a = eng.pt_log_read()
            spins.append(eng.get_spins())
            slots.append(eng.pt_slots())
            lp.append(p)
            la.append(a)
        if b == 0:
            for g in (1, batch - 1):
                s, sl = oracle_ladder(bi, inst, mb, g, G, T, rounds, pairs, precision, seed)
                assert np.array_equal(spins[0][g * L:(g + 1) * L], s) and np.array_equal(slots[0][g * L:(g + 1) * L], sl), f"ladder {g}"
    judge_rounds(name, bi, np.concatenate(spins), np.concatenate(slots), np.concatenate(lp, axis=1), np.concatenate(la, axis=1))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cut", ["all", "one_rest"])
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("entry", ["fused", "deferred"])
def test_rounds_in_one_launch(product, entry, precision, cut, layout):
    """(d) pt_rounds_fused / pt_rounds_deferred inside k_rounds_fused launches: T sweeps + a swap round of L // 3 pairs, 15 rounds,
    launches cut [all] and [1, rest].  The kernel needs every chain resident at once, so the ladders run in batches of 64
    (512 chains) with a seed each."""
    rounds_case(product, entry, precision, layout, cut, False)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("precision,cut", [("f64", "all"), ("f32", "one_rest")])
def test_rounds_deferred_launch_per_round(product, monkeypatch, precision, cut, layout):
    """NLMC_NO_PERSISTENT=1 sends pt_rounds_deferred down its other route -- a sweep launch per round that decides the previous
    round's swap in its prologue -- with all ladders in one context."""
    monkeypatch.setenv("NLMC_NO_PERSISTENT", "1")
    rounds_case(product, "deferred", precision, layout, cut, True)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("device_ids", [[0], [0, 0]])
def test_local_tempering_driver(product, device_ids, precision, layout):
    """(e) LocalTempering.plan + run_rounds + round(): the driver's own sweep and round counters, over one and two contexts.
    A context holds 8192 or 4096 chains of 256 threads each -- more workgroups than the device keeps resident at once (at most
    2048 threads per compute unit) -- so its batched calls take the launch-per-round route; the in-launch route is case (d)."""
    L, T, rounds = len(PT_BETAS), 3, 12
    pairs = L // 3
    nl = -(-pt_ladders() // 2) * 2
    G = nl * L
    bi = xl.BlockInstance(DYADIC, COPIES, layout)
    inst = product.Instance(bi.J, bi.h)
    name = f"LocalTempering {precision} {layout} contexts={len(device_ids)} route=per round ladders={nl}"
    start_seed, seed = case_seeds(name)
    m0 = xl.equilibrium_start(np.random.default_rng(start_seed), bi, np.tile(PT_BETAS, nl))
    lt = product.distributed.LocalTempering(inst, PT_BETAS, G, seed, pairs, device_ids, precision=precision)
    try:
        lt.set_spins(m0)
        lt.plan(rounds * T, rounds, chunk_rounds=5)
        lt.log_begin(rounds)
        lt.run_rounds(7, T)
        for _ in range(2):
            lt.round(T)
        lt.run_rounds(3, T)
        assert lt.rounds_done == rounds and lt.sweeps_done == rounds * T
        assert lt.deferred_rounds == 10 and lt.rounds_routes == [PER_ROUND] * len(device_ids), lt.rounds_routes
        lt.check()
        spins, slots = lt.gather_spins(), lt.slots()
        p, a = lt.swap_log()
    finally:
        lt.close()
    for g in (0, nl - 1):
        s, sl = oracle_ladder(bi, inst, m0, g, G, T, rounds, pairs, precision, seed)
        assert np.array_equal(spins[g * L:(g + 1) * L], s) and np.array_equal(slots[g * L:(g + 1) * L], sl), f"ladder {g}"
    judge_rounds(name, bi, spins, slots, p, a)


# ---- (g) phase flags ----------------------------------------------------------------------------------------------------------------
FLAG_PATTERN = np.array([1, 1, 1, 1, 1, 1, 0, 2, 3], np.uint8)       # by block index mod 9: both species meet every flag


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_phase_flags(product, precision, layout):
    """Whole blocks flagged 0 (beta), 1 (beta / temp_x) and frozen (2, 3), temp_x = 3, fused windows.  Flag-1 blocks start at
    beta / temp_x and must stay there, flag-0 blocks at beta, frozen blocks keep their bits.  Wrong: flag-1 blocks at the full beta."""
    betas, tx, T, W = np.array([0.7, 1.1]), 3.0, 4, 3
    L = len(betas)
    bi = xl.BlockInstance(DYADIC, COPIES, layout)
    bflag = FLAG_PATTERN[np.arange(COPIES) % len(FLAG_PATTERN)]
    groups = {f: np.nonzero(bflag == f)[0] for f in (0, 1)}
    m = L * 2 * 4
    need = 0
    for f, blocks in groups.items():
        for b in betas / (tx if f else 1.0):
            var_chain = sum(xl.Law(DYADIC[k], b).var * np.sum(bi.kind[blocks] == k) for k in range(2))
            need = max(need, int(np.ceil(1.03 * (xl.z_threshold(m) / (b * MAX_DELTA)) ** 2 / var_chain)))
    R = L * need
    beta_of = betas[np.arange(R) % L]
    name = f"phase flags {precision} {layout} R={R}"
    start_seed, seed = case_seeds(name)
    hot = xl.equilibrium_start(np.random.default_rng(start_seed), bi, beta_of / tx)
    m0 = xl.equilibrium_start(np.random.default_rng(start_seed + 1), bi, beta_of)
    m0[:, bi.idx[groups[1]].ravel()] = hot[:, bi.idx[groups[1]].ravel()]
    flags = np.empty((R, bi.n), np.uint8)
    flags[:, bi.idx] = bflag[None, :, None]
    with product.Engine(product.Instance(bi.J, bi.h), None, R) as eng:
        eng.set_spins(m0)
        eng.pt_init(betas)
        eng.set_flags(flags, tx)
        assert eng.plan_philox_fused(0, W, T, seed) == W
        if precision == "f64":
            assert "f64" in eng.fused_modes(T)
        for w in range(W):
            eng.sweep_philox(T, seed, sweep0=w * T, beta=None, precision=precision)
            assert eng._last_fused() and eng.last_sweep_route() == "fused"
        out = eng.get_spins()
    frozen = flags >= 2
    assert np.array_equal(out[frozen], m0[frozen]) and not np.array_equal(out, m0)
    for c in (0, R - 1):
        assert np.array_equal(out[c], oracle_final(bi, m0, c, beta_of[c], T * W, precision == "f64", seed, flags=flags, temp_x=tx)), c
    v = xl.Verdict(name)
    for i, b in enumerate(betas):
        v.add_slot(f"slot{i} flag0", bi, out[i::L], b, blocks=groups[0])
        v.add_slot(f"slot{i} flag1", bi, out[i::L], b / tx, blocks=groups[1])
        full = xl.slot_statistics(bi, out[i::L], b, correlation=False, blocks=groups[1])
        v.add_wrong(f"slot{i} flag1 at full beta", min(r["p"] for r in full.values()))
    assert v.m == m
    conclude(v)


# ---- (f) APT rounds: sweeps, Houdayer moves, swaps ----------------------------------------------------------------------------------
APT_M = 8 * 4 + 8 * 2                                   # (i) x 2, (ii), (iii) and the two overlap histograms (iv) per slot


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("W", [1, 2])
def test_apt_rounds(product, W, precision, layout):
    """SlotShardedAPT: K = 8 sub-replicas x 8 temperatures, fused windows of 3 sweeps, Houdayer moves between the sub-replicas of a
    slot (k_icm_round), swaps of L // 3 pairs; W = 2 cuts the ladder into two slot blocks on one device, so accepted boundary pairs
    run k_apt_pack / k_apt_adopt.  katzgraber=True stays, and no picked cluster may exceed N / 2: the global flip is not an invariant
    move when h != 0 (blocks of 6 spins never get there).  Independent runs of 64 chains, a seed each, make up the sample;
    (iv) is taken between sub-replicas 0-3 and 4-7 of a slot.  The first run is reproduced whole by the protocol over the oracle
    double."""
    K, R, T, rounds = 8, len(PT_BETAS), 3, 10
    pairs = R // 3
    runs = -(-max(1024, chains_per_slot(DYADIC, PT_BETAS, COPIES, APT_M)) // K)
    bi = xl.BlockInstance(DYADIC, COPIES, layout)
    inst = product.Instance(bi.J, bi.h)
    name = f"APT W={W} {precision} {layout} runs={runs}"
    start_seed, seed0 = case_seeds(name)
    start = xl.equilibrium_start(np.random.default_rng(start_seed), bi, np.tile(PT_BETAS, runs * K)).reshape(runs, K, R, bi.n)

    def drive(make, seed, spins, plan):
        apt = product.distributed.SlotShardedAPT(make, inst, PT_BETAS, K, seed, pairs, precision=precision, katzgraber=True,
                                                 device_ids=None if W == 1 else [0] * W)
        try:
            apt.set_spins_by_slot(spins)
            if plan:
                apt.plan(rounds, T, chunk_rounds=rounds)
            moved = accepted = boundary = 0
            for _ in range(rounds):
                (p, a), info = apt.round(T, want_log=True, want_info=True)
                if plan:
                    assert all(e._last_fused() and e.last_sweep_route() == "fused" for e in apt.engs)
                info = np.concatenate(info)
                assert info[:, 1].max() <= bi.n // 2
                moved += int((info[:, 1] > 0).sum())
                accepted += int(a.sum())
                boundary += int((a.astype(bool) & (p[..., 1] % (R // W) == 0)).sum())
            cfg, _ = apt.gather_by_slot()
            apt.check()
        finally:
            apt.close()
        return cfg, moved, accepted, boundary

    def gpu(i, n, b, g, dev=0):
        return product.Engine(i, None, n, device=0, chain_base=b, n_chains_global=g, own_stream=W > 1)

    out, moved, accepted, boundary = [], 0, 0, 0
    for r in range(runs):
        cfg, mv, ac, bd = drive(gpu, seed0 + (r << 20), start[r], True)
        out.append(cfg)
        moved, accepted, boundary = moved + mv, accepted + ac, boundary + bd
    assert moved > runs and accepted > runs and (W == 1 or boundary > 0)
    ref = drive(lambda i, n, b, g, dev=None: OracleEngine(i, n, b, g), seed0, start[0], False)[0]
    assert np.array_equal(out[0], ref)
    cfg = np.stack(out)                                                             # [runs, K, R, n]
    v = xl.Verdict(name)
    for r, b in enumerate(PT_BETAS):
        v.add_slot(f"slot{r}", bi, cfg[:, :, r].reshape(runs * K, -1), b)
        for k, spc in enumerate(bi.species):
            v.add(f"slot{r} overlap {spc.name}", xl.chi2_overlap(cfg[:, :K // 2, r], cfg[:, K // 2:, r], bi, k, xl.Law(spc, b)))
    assert v.m == APT_M
    conclude(v)
