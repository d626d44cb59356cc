"""The per-round energy log without a device: the interface (header, binding, library) names the four entry points alike;
hostlogic.ladder_report and suggest_ladder on hand-built logs with known answers; distributed.LocalTempering(track_energies=True) on
the CPU double observes once per round between the round's last state-changing step and its swap; the ValueError paths of the classes
that need no device."""
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_product
from fake_engine import OracleEngine
from helpers import make_instance, init_spins

NEW = ("nlmc_elog_begin", "nlmc_elog_update", "nlmc_elog_read", "nlmc_elog_end")
N, SEED, S, ROUNDS, PAIRS = 48, 0xE106CAFE, 3, 6, 1
LQ, NLQ = 4, 2
G = LQ * NLQ


def test_header_binding_and_library_name_the_log_alike():
    P = load_product()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "nlmc.h")).read(), flags=re.S)
    decl = set(re.findall(r"\b(nlmc_[a-z0-9_]+)\s*\(", text))
    L = P._abi.lib()
    for name in NEW:
        assert name in decl and name in P._abi.EXPORTS and hasattr(L, name), name
    assert sorted(P._abi.EXPORTS) == sorted(decl)
    assert re.search(r"int\s+nlmc_elog_begin\s*\(\s*nlmc_ctx\s*\*\s*\w*\s*,\s*uint32_t\s+\w+\s*,\s*int\s+\w+\s*\)", text)
    assert re.search(r"int\s+nlmc_elog_update\s*\(\s*nlmc_ctx\s*\*\s*\w*\s*,\s*uint32_t\s+\w+\s*\)", text)
    assert re.search(r"int\s+nlmc_elog_read\s*\(\s*nlmc_ctx\s*\*\s*\w*\s*,\s*double\s*\*\s*\w+[^,]*,\s*int32_t\s*\*\s*\w+[^)]*\)", text)
    assert L.nlmc_elog_begin.argtypes[1] is P._abi._u32 and L.nlmc_elog_begin.argtypes[2] is P._abi._i
    assert L.nlmc_elog_update.argtypes[1] is P._abi._u32 and len(L.nlmc_elog_read.argtypes) == 3 and len(L.nlmc_elog_end.argtypes) == 1
    assert L.nlmc_abi_version() == P._abi.ABI_VERSION == 3
    for m in ("elog_begin", "elog_update", "elog_read", "elog_end"):
        assert callable(getattr(P.Engine, m))


# ---- ladder_report on logs written out by hand ----------------------------------------------------------------------------------------
# One ladder of three slots, ten rounds.  slot of chain 0, 1, 2 per round:
HIST = np.array([[0, 1, 2],      # r0
                 [1, 0, 2],      # r1: pair (0, 1) exchanged
                 [2, 0, 1],      # r2: pair (1, 2) exchanged               chain 0 reaches the top
                 [1, 0, 2],      # r3: pair (1, 2)
                 [0, 1, 2],      # r4: pair (0, 1)                         chain 0 back at the bottom: trip 1
                 [0, 1, 2],      # r5: nothing
                 [1, 0, 2],      # r6: pair (0, 1)
                 [2, 0, 1],      # r7: pair (1, 2)
                 [1, 0, 2],      # r8: pair (1, 2)
                 [0, 1, 2]],     # r9: pair (0, 1)                         trip 2
                dtype=np.int32)


def test_ladder_report_on_a_hand_written_slot_history():
    """Nine transitions; pair (0, 1) exchanged at r1, r4, r6, r9, pair (1, 2) at r2, r3, r7, r8.  Chain 0 makes exactly two round
    trips 0 -> 2 -> 0; chain 1 never reaches the top, chain 2 never the bottom.  The energy on slot s in round r is 10 s + (r mod 2):
    per slot a two-valued sequence with five rounds each, whose population std is exactly 0.5."""
    P = load_product()
    rounds = HIST.shape[0]
    E = 10.0 * HIST + (np.arange(rounds) % 2)[:, None]
    rep, = P.hostlogic.ladder_report(E, HIST, [0.5, 1.0, 2.0])
    assert np.array_equal(rep["swap_attempts"], [9, 9]) and np.array_equal(rep["swap_accepts"], [4, 4])
    assert np.array_equal(rep["acceptance"], [4 / 9, 4 / 9])
    assert np.array_equal(rep["round_trips"], [2, 0, 0])
    assert rep["tau_round_trip"] == 10 * 3 / 2 and rep["n_rounds"] == 10
    assert np.array_equal(rep["mean_energy"], [0.5, 10.5, 20.5]) and np.array_equal(rep["sigma_energy"], [0.5, 0.5, 0.5])
    # by slot: the chain that held each slot
    e_s, c_s = P.hostlogic.log_by_slot(E, HIST, 3)
    assert e_s.shape == c_s.shape == (rounds, 1, 3)
    assert np.array_equal(c_s[2, 0], [1, 2, 0]) and np.array_equal(e_s[2, 0], [0.0, 10.0, 20.0])


def test_ladder_report_constant_energies_no_trips_and_unobserved_rows():
    """Constant energies: sigma = 0.  Nobody moves: no accepts, no trips, tau = inf.  Rows NaN / -1 (rounds that did not run) are left
    out, and a transition across such a row is no attempt.  Two ladders give two reports."""
    P = load_product()
    rounds, L = 6, 4
    slots = np.tile(np.arange(2 * L, dtype=np.int32) % L, (rounds, 1))
    E = np.tile(-3.0 * np.arange(2 * L), (rounds, 1)).astype(np.float64)
    slots[3], E[3] = -1, np.nan
    reps = P.hostlogic.ladder_report(E, slots, np.linspace(0.5, 2.0, L))
    assert len(reps) == 2
    for g, rep in enumerate(reps):
        assert np.array_equal(rep["sigma_energy"], np.zeros(L)) and np.array_equal(rep["mean_energy"], -3.0 * (g * L + np.arange(L)))
        assert rep["n_rounds"] == 5 and np.array_equal(rep["swap_attempts"], [3, 3, 3]) and not rep["swap_accepts"].any()
        assert not rep["round_trips"].any() and rep["tau_round_trip"] == float("inf")
    pooled = P.hostlogic.pool_reports(reps)
    assert np.array_equal(pooled["swap_attempts"], [6, 6, 6]) and pooled["round_trips"].shape == (2 * L,)


def test_suggest_ladder():
    P = load_product()
    betas = np.array([0.5, 1.0, 2.0])
    flat = {"sigma_energy": np.array([2.5, 2.5, 2.5])}
    # sigma constant: the arithmetic ladder beta_0 + k alpha / sigma, up to the first value above beta_max (where the preprocessor stops)
    out = P.hostlogic.suggest_ladder(flat, betas, alpha=1.25, beta_max=3.0)
    assert np.array_equal(out, 0.5 + 0.5 * np.arange(len(out))) and out[-2] <= 3.0 < out[-1] and len(out) == 7
    # default beta_max: the largest measured beta
    out = P.hostlogic.suggest_ladder(flat, betas)
    assert np.array_equal(out, [0.5, 1.0, 1.5, 2.0, 2.5])
    # a falling sigma, interpolated linearly in beta: steps grow, the ladder is strictly increasing, the first step is alpha / sigma_0
    fall = {"sigma_energy": np.array([4.0, 2.0, 1.0])}
    out = P.hostlogic.suggest_ladder(fall, betas, alpha=1.0, beta_max=10.0)
    assert (np.diff(out) > 0).all() and out[0] == 0.5 and out[1] == 0.75 and out[2] == 0.75 + 1.0 / 3.0
    assert (out[:-1] <= 10.0).all() and out[-1] > 10.0
    assert np.allclose(np.diff(out)[out[:-1] >= 2.0], 1.0, rtol=0, atol=1e-12) and (out[:-1] >= 2.0).sum() >= 5   # sigma = 1 held beyond the last slot
    # freeze-out: sigma at or below sigma_min ends the ladder
    out = P.hostlogic.suggest_ladder(fall, betas, alpha=1.0, beta_max=10.0, sigma_min=1.0)
    assert out[-1] >= 2.0 and len(out) < 8 and (np.diff(out) > 0).all()
    assert np.array_equal(P.hostlogic.suggest_ladder({"sigma_energy": np.zeros(3)}, betas), [0.5])
    with pytest.raises(ValueError):
        P.hostlogic.suggest_ladder(flat, betas[:2])


# ---- LocalTempering on the CPU double --------------------------------------------------------------------------------------------------
class LoggingEngine(OracleEngine):
    """The double with the log's four methods in NumPy (include/nlmc.h: nlmc_elog_begin) and a journal of the calls it gets."""

    def __init__(self, *a):
        super().__init__(*a)
        self.journal = []
        self.log_on = False

    def sweep_philox(self, *a, **k):
        self.journal.append(("sweep",))
        return super().sweep_philox(*a, **k)

    def pt_swap_philox(self, rnd, *a, **k):
        self.journal.append(("swap", int(rnd)))
        return super().pt_swap_philox(rnd, *a, **k)

    def elog_begin(self, round0, n_rounds):
        self.journal.append(("begin", int(round0), int(n_rounds)))
        self.log_on, self.l_round0 = True, int(round0)
        self.l_e = np.full((n_rounds, self.n_chains), np.nan)
        self.l_s = np.full((n_rounds, self.n_chains), -1, np.int32)

    def elog_update(self, rnd):
        assert self.log_on
        self.journal.append(("update", int(rnd)))
        row = int(rnd) - self.l_round0
        if 0 <= row < len(self.l_e):
            self.l_e[row] = self.efix.astype(np.float64) * 2.0 ** -self.esc
            self.l_s[row] = self.pt_slots()[self.chain_base:self.chain_base + self.n_chains]

    def elog_read(self, by="chain"):
        return self.l_e.copy(), self.l_s.copy()

    def elog_end(self):
        self.log_on = False


class BatchingLoggingEngine(LoggingEngine):
    """... and a batched rounds call that observes each of its rounds itself, as the library's rounds entry points do."""

    def pt_rounds_deferred(self, n_rounds, sweeps_per_round, seed, sweep0, round0, n_pairs, precision="f32"):
        for r in range(n_rounds):
            self.sweep_philox(sweeps_per_round, seed, sweep0=sweep0 + r * sweeps_per_round, precision=precision)
            if self.log_on:
                self.elog_update(round0 + r)
            self.pt_swap_philox(round0 + r, seed, n_pairs)
        return True

    def last_rounds_route(self):
        return "launch per round"


@pytest.fixture(scope="module")
def case():
    P = load_product()
    J, h = make_instance(N, seed=5, with_h=True, gaussian=True)
    return P, P.Instance(J, h), np.geomspace(0.2, 2.0, LQ), init_spins(G, N)


def drive(case, k, cls, how, **kw):
    P, inst, betas, m0 = case
    lt = P.distributed.LocalTempering(inst, betas, G, SEED, PAIRS, [0] * k, engine_factory=lambda i, n, b, g: cls(i, n, b, g), **kw)
    lt.set_spins(m0)
    lt.plan(ROUNDS * S, ROUNDS)
    if how == "round":
        for _ in range(ROUNDS):
            lt.round(S)
    else:
        lt.run_rounds(ROUNDS, S)
    assert lt.rounds_done == ROUNDS
    return lt


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("how, cls", [("round", LoggingEngine), ("run_rounds", LoggingEngine), ("run_rounds", BatchingLoggingEngine)])
def test_local_tempering_observes_once_per_round_before_the_swap(case, k, how, cls):
    """Per context the journal reads begin(0, ROUNDS), then (sweep, update r, swap r) for every round; energy_log() lays the contexts'
    logs out by global chain id; a row holds the slots the swap of that round decided on (the slots BEFORE it)."""
    P = case[0]
    lt = drive(case, k, cls, how, track_energies=True)
    for e in lt.engs:
        assert e.journal[0] == ("begin", 0, ROUNDS)
        assert e.journal[1:] == [x for r in range(ROUNDS) for x in (("sweep",), ("update", r), ("swap", r))]
    E, sl = lt.energy_log()
    assert E.shape == sl.shape == (ROUNDS, G) and E.dtype == np.float64 and sl.dtype == np.int32
    ref_E, ref_s = drive(case, 1, LoggingEngine, "round", track_energies=True).energy_log()
    assert np.array_equal(E, ref_E) and np.array_equal(sl, ref_s)
    assert np.array_equal(sl[0], np.arange(G) % LQ) and not np.isnan(E).any()
    assert np.array_equal(np.sort(sl.reshape(ROUNDS, NLQ, LQ), axis=2), np.tile(np.arange(LQ), (ROUNDS, NLQ, 1)))
    reps = P.hostlogic.ladder_report(E, sl, case[2])
    assert len(reps) == NLQ and all(np.array_equal(r["swap_attempts"], [ROUNDS - 1] * (LQ - 1)) for r in reps)


def test_log_off_calls_none_of_the_new_methods(case):
    lt = drive(case, 2, OracleEngine, "round")
    on = drive(case, 2, LoggingEngine, "round", track_energies=True)
    assert np.array_equal(lt.gather_spins(), on.gather_spins()) and np.array_equal(lt.slots(), on.slots())
    with pytest.raises(ValueError, match="track_energies"):
        lt.energy_log()
    with pytest.raises(ValueError, match="track_energies"):
        lt.energy_log_begin(3)


def test_track_energies_needs_whole_ladders_per_context(case):
    P, inst, betas, _ = case
    with pytest.raises(ValueError, match="track_energies"):
        P.distributed.LocalTempering(inst, betas, G, SEED, PAIRS, [0, 0, 0, 0], track_energies=True,
                                     parts=[(0, 2), (2, 2), (4, 2), (6, 2)], engine_factory=lambda i, n, b, g: LoggingEngine(i, n, b, g))


def test_track_energies_is_refused_off_the_device_resident_paths():
    """rng="numpy" (the default: the reference's own stream order), device_ids that cut a ladder (NPT) or any device_ids (APT_ICM): the
    ValueError comes before any device work."""
    P = load_product()
    J, h = make_instance(40, seed=2)
    kw = dict(num_sweeps_MCMC=4, num_sweeps_read=4, num_swap_attempts=2, track_energies=True)
    with pytest.raises(ValueError, match="track_energies"):
        P.NPT(J, h).run(np.array([0.5, 1.0]), 2, [False, False], **kw)
    with pytest.raises(ValueError, match="track_energies"):
        P.NPT(J, h, rng="philox", seed=1).run(np.array([0.5, 1.0]), 2, [False, False], device_ids=[0, 0], **kw)
    with pytest.raises(ValueError, match="track_energies"):
        P.APT_ICM(J.toarray(), h).run(np.array([0.5, 1.0]), 2, **kw)
    with pytest.raises(ValueError, match="track_energies"):
        P.APT_ICM(J.toarray(), h, rng="philox", seed=1).run(np.array([0.5, 1.0]), 2, icm_feedback=True, device_ids=[0, 0], **kw)
