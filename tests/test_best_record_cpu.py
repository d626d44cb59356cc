"""The best-state record on the CPU double: distributed.LocalTempering(track_best=True) issues exactly one observation per round,
stamped with the round, between the round's sweeps and its swap -- on round() and on everything run_rounds() falls back to -- and
calls none of the record's methods when it is off.  The interface (header, binding, library) names the four entry points alike."""
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_product
from fake_engine import OracleEngine
from helpers import make_instance, init_spins

N, SEED, S, ROUNDS, PAIRS = 48, 0xBE57CAFE, 3, 6, 1
LQ, NLQ = 4, 2
G = LQ * NLQ
NEW = ("nlmc_best_begin", "nlmc_best_update", "nlmc_best_read", "nlmc_best_end")


class RecordingEngine(OracleEngine):
    """The double with the record's four methods in NumPy (include/nlmc.h: nlmc_best_begin) and a journal of the calls it gets."""

    def __init__(self, *a):
        super().__init__(*a)
        self.journal = []
        self.rec_on = False

    def sweep_philox(self, *a, **k):
        self.journal.append(("sweep",))
        return super().sweep_philox(*a, **k)

    def pt_swap_philox(self, rnd, *a, **k):
        self.journal.append(("swap", int(rnd)))
        return super().pt_swap_philox(rnd, *a, **k)

    def best_begin(self, target=None):
        self.journal.append(("begin", target))
        self.rec_on, self.target = True, target
        self.b_efix = np.full(self.n_chains, np.iinfo(np.int64).max, np.int64)
        self.b_stamp = np.full(self.n_chains, -1, np.int32)
        self.b_hit = np.full(self.n_chains, -1, np.int32)
        self.b_state = np.zeros((self.n_chains, self.n), np.int8)

    def best_update(self, stamp):
        assert self.rec_on
        self.journal.append(("update", int(stamp)))
        E = self.efix.astype(np.float64) * 2.0 ** -self.esc
        if self.target is not None:
            self.b_hit[(self.b_hit < 0) & (E <= self.target)] = stamp
        imp = self.efix.astype(np.float64) < self.b_efix.astype(np.float64)
        self.b_efix[imp], self.b_stamp[imp], self.b_state[imp] = self.efix[imp], stamp, self.spins[imp]

    def best_read(self, want_state=True):
        return {"energy": self.b_efix.astype(np.float64) * 2.0 ** -self.esc, "stamp": self.b_stamp.copy(), "first_hit": self.b_hit.copy(),
                "state": self.b_state.copy() if want_state else None}

    def best_end(self):
        self.journal.append(("end",))
        self.rec_on = False


class BatchingRecordingEngine(RecordingEngine):
    """... and a batched rounds call that observes each of its rounds itself, as the library's rounds entry points do."""

    def pt_rounds_deferred(self, n_rounds, sweeps_per_round, seed, sweep0, round0, n_pairs, precision="f32"):
        for r in range(n_rounds):
            self.sweep_philox(sweeps_per_round, seed, sweep0=sweep0 + r * sweeps_per_round, precision=precision)
            if self.rec_on:
                self.best_update(round0 + r)
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
@pytest.mark.parametrize("how, cls", [("round", RecordingEngine), ("run_rounds", RecordingEngine), ("run_rounds", BatchingRecordingEngine)])
def test_one_observation_per_round_between_sweeps_and_swap(case, k, how, cls):
    """round(), run_rounds() falling back to it (the double has no batched call) and run_rounds() on batched calls: per context the
    journal reads begin, then (sweep, update r, swap r) for r = 0 .. ROUNDS - 1; the records of all three agree."""
    lt = drive(case, k, cls, how, track_best=True, target_energy=-20.0)
    for e in lt.engs:
        assert e.journal[0] == ("begin", -20.0)
        assert e.journal[1:] == [x for r in range(ROUNDS) for x in (("sweep",), ("update", r), ("swap", r))]
    b = lt.best()
    assert b["energy"].shape == (G,) and b["state"].shape == (G, N) and b["stamp"].shape == b["first_hit"].shape == (G,)
    ref = drive(case, 1, RecordingEngine, "round", track_best=True, target_energy=-20.0).best()
    for key in ("energy", "stamp", "first_hit", "state"):
        assert np.array_equal(b[key], ref[key]), key
    assert (b["stamp"] >= 0).all() and (b["stamp"] < ROUNDS).all()
    # the record is the strict running minimum: no chain ends below it, and a chain that hit the target did so no later than its best
    fin = np.concatenate([e.energy_tracked() for e in lt.engs])
    assert (b["energy"] <= fin).all()
    hit = b["first_hit"] >= 0
    assert np.array_equal(hit, b["energy"] <= -20.0) and (b["first_hit"][hit] <= b["stamp"][hit]).all()


@pytest.mark.parametrize("how", ["round", "run_rounds"])
def test_record_off_calls_none_of_the_new_methods(case, how):
    """The plain double of tests/fake_engine.py has none of the four methods: with track_best off nothing asks for them, and the
    trajectory is the one a tracked run leaves."""
    lt = drive(case, 2, OracleEngine, how)
    on = drive(case, 2, RecordingEngine, how, track_best=True)
    assert np.array_equal(lt.gather_spins(), on.gather_spins()) and np.array_equal(lt.slots(), on.slots())
    with pytest.raises(ValueError, match="track_best"):
        lt.best()
    off = drive(case, 1, RecordingEngine, how)
    assert not [x for x in off.engs[0].journal if x[0] in ("begin", "update", "end")]


def test_header_binding_and_library_name_the_record_alike():
    P = load_product()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "nlmc.h")).read(), flags=re.S)
    decl = set(re.findall(r"\b(nlmc_[a-z0-9_]+)\s*\(", text))
    L = P._abi.lib()
    for name in NEW:
        assert name in decl and name in P._abi.EXPORTS and hasattr(L, name), name
    assert sorted(P._abi.EXPORTS) == sorted(decl)
    assert re.search(r"int\s+nlmc_best_begin\s*\(\s*nlmc_ctx\s*\*\s*\w*\s*,\s*double\s+\w+\s*\)", text)
    assert re.search(r"int\s+nlmc_best_update\s*\(\s*nlmc_ctx\s*\*\s*\w*\s*,\s*uint32_t\s+\w+\s*\)", text)
    assert L.nlmc_best_begin.argtypes[1] is P._abi._dbl and L.nlmc_best_update.argtypes[1] is P._abi._u32
    assert len(L.nlmc_best_read.argtypes) == 5
    assert L.nlmc_abi_version() == P._abi.ABI_VERSION == 3
    for m in ("best_begin", "best_update", "best_read", "best_end"):
        assert callable(getattr(P.Engine, m))
