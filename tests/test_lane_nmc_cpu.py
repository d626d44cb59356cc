"""NMC phase cycles inside one lane launch (include/nlmc.h: nlmc_nmc_phases_lanes), the parts that need no GPU: LocalTempering's route
rule over the CPU double -- rounds with lane_nmc=True against rounds with the phase loop, state for state; a round with outputs keeps the
loop; a refusing engine falls back once; no fused-window planner for the phases where every context takes the call -- and the keyword
checks of NPT.  The double supplies the NMC calls of the engine through the oracle, and nmc_phases_lanes as its specification written
out once in NumPy (adopt, reset, sweeps with the flag computed from the mask, strict running minimum on the strided sweeps)."""
import numpy as np
import pytest

import oracle
from conftest import load_product
from fake_engine import OracleEngine
from helpers import make_instance

N, SEED, S, PAIRS = 24, 0xA11CE000 + (5 << 32), 3, 2
L, NL = 6, 2
G = L * NL
MARKS = [False, False, False, True, True, True]
PHASES, S_NMC, GBETA, TEMP_X = ["C", "NC", "C", "NC", "ALL"], 4, 2.5, 20.0
I64_MAX = np.iinfo(np.int64).max


class NmcEngine(OracleEngine):
    """The double with the NMC calls LocalTempering.round makes: marked slots and chain subsets, a backbone inference that installs a
    fixed mask, the tracked minimum, phase flags, the argmin hand-off, flagged sweeps with one beta -- and nmc_phases_lanes."""
    refuse = False
    has_query = True

    def __init__(self, *a):
        super().__init__(*a)
        self.sel, self.kind, self.temp_x, self.track = "all", "ALL", 1.0, 0
        self.mask = None
        self.fixed_mask = np.random.default_rng(77).integers(0, 2, size=(self.n_chains, self.n)).astype(np.uint8)
        self.fixed_mask[0] = 0                      # an empty and a full backbone among them
        self.fixed_mask[-1] = 1
        self.emin = np.full(self.n_chains, I64_MAX, np.int64)
        self.argmin = np.zeros(self.n_chains, np.int32)
        self.best = np.zeros((self.n_chains, self.n), np.int8)
        self.phase_sweeps = self.lane_calls = self.asked = self.adopted = 0

    def mark_slots(self, marks):
        self.marks = np.asarray(marks, bool)

    def overlap_subsets(self, on=True):
        pass

    def select(self, which):
        self.sel = which

    def subset(self):
        c = np.arange(self.n_chains)
        if self.sel == "all":
            return c.astype(np.int32)
        m = self.marks[self.slots[self.chain_base + c]]
        return c[m if self.sel == "marked" else ~m].astype(np.int32)

    def rows(self):
        return len(self.subset())

    def backbone_clusters(self, *a):
        if self.mask is None:
            self.mask = np.zeros((self.n_chains, self.n), np.uint8)
        for c in self.subset():
            self.mask[c] = self.fixed_mask[c]

    def backbone_check(self):
        pass

    def track_minimum(self, on=True, stride=1):
        self.track = max(1, int(stride)) if on else 0

    def set_phase(self, kind, temp_x=1.0):
        self.kind = kind
        if kind != "ALL":
            self.temp_x = float(temp_x)

    def adopt_best(self):
        self.adopted += 1
        for c in self.subset():
            self.spins[c], self.efix[c] = self.best[c], self.emin[c]

    @staticmethod
    def _flags(mask, kind):
        if kind == "ALL":
            return None
        m = mask.astype(bool)
        return np.where(m, 1, 2).astype(np.uint8) if kind == "C" else np.where(m, 2, 0).astype(np.uint8)

    def sweep_philox(self, n_sweeps, seed, sweep0=0, beta=None, precision="f32", record_stride=0, want_energy=False, want_min=False,
                     want_state=False):
        f64 = precision == "f64"
        rows = self.subset()
        if self.sel == "marked":
            self.phase_sweeps += 1
        energy = np.empty((len(rows), n_sweeps)) if want_energy else None
        for j, c in enumerate(rows):
            b = self.betas[self.slots[self.chain_base + c]] if beta is None else float(beta)
            fl = self._flags(self.mask[c], self.kind) if self.kind != "ALL" else None
            cb = np.tile(np.array(oracle.cb_pair(b, self.temp_x if fl is not None else 1.0, f64)), (n_sweeps, 1))
            M, s, tr = oracle.sweeps_philox(self.csr, self.h, self.spins[c], cb, seed, self._rng_id(c), sweep0=sweep0, flags=fl,
                                            escale=self.esc, use_f64=f64, efix0=int(self.efix[c]))
            if self.track and n_sweeps:
                cols = np.arange(0, n_sweeps, self.track)
                t = int(cols[np.argmin(tr[cols])])                       # the first minimum over the strided sweeps
                self.emin[c], self.argmin[c], self.best[c] = tr[t], t, M[t]
            self.spins[c] = s
            if n_sweeps:
                self.efix[c] = tr[-1]
            if want_energy:
                energy[j] = tr * 2.0 ** -self.esc
        return {"spins": None, "energy": energy, "min_energy": None, "argmin": None, "argmin_state": None}

    def nmc_phases_lanes_refusal(self, sweeps_per_phase):
        self.asked += 1
        return "refused by the test" if (self.refuse and self.has_query) else None

    def nmc_phases_lanes(self, kinds, sweeps_per_phase, seed, sweep0, beta, temp_x, min_stride=1, precision="f32", want_minima=False,
                         want_last_best=False):
        """Section 1 of the kernel's specification, a chain at a time."""
        if self.refuse:
            raise NotImplementedError("refused by the test")
        assert self.mask is not None and self.track == 0
        self.lane_calls += 1
        f64, Sp = precision == "f64", int(sweeps_per_phase)
        cb = np.array(oracle.cb_pair(float(beta), float(temp_x), f64)).reshape(1, 2)
        for c in self.subset():
            s, E = self.spins[c].copy(), int(self.efix[c])
            Emin, amin, best = I64_MAX, 0, s.copy()
            for p, kind in enumerate(kinds):
                if p > 0:
                    s, E = best.copy(), Emin                              # 1. adopt the previous phase's minimum
                Emin, amin = I64_MAX, 0                                   # 2. reset the running minimum
                fl = self._flags(self.mask[c], kind)                      # 3. the flag of a spin from its mask byte
                for t in range(Sp):
                    _, s, tr = oracle.sweeps_philox(self.csr, self.h, s, cb, seed, self._rng_id(c), sweep0=sweep0 + p * Sp + t, flags=fl,
                                                    escale=self.esc, use_f64=f64, efix0=E, want_M=False)
                    E = int(tr[-1])
                    if E < Emin and t % min_stride == 0:                  # 4. strict: the first argmin
                        Emin, amin, best = E, t, s.copy()
            self.spins[c], self.efix[c], self.emin[c], self.argmin[c], self.best[c] = s, E, Emin, amin, best


def _instance(P):
    J, h = make_instance(N, seed=9)
    return P.Instance(J, h)


def _tempering(P, lane_nmc, engine=NmcEngine, m_skip=1, **kw):
    inst = _instance(P)
    betas = np.geomspace(0.3, 2.0, L)
    lt = P.distributed.LocalTempering(inst, betas, G, SEED, PAIRS, [0], engine_factory=engine, lane_nmc=lane_nmc, **kw)
    lt.configure_nmc(MARKS, PHASES, S_NMC, GBETA, TEMP_X, np.zeros(N), [1.0], 1e-9, 10, 0.99, [0.9], M_skip=m_skip)
    lt.set_spins((2 * np.random.default_rng(3).integers(0, 2, size=(G, N), dtype=np.int8) - 1).astype(np.int8))
    return lt


def _state(lt):
    e = lt.engs[0]
    return lt.gather_spins(), lt.slots(), e.efix.copy(), e.emin.copy(), e.argmin.copy(), e.best.copy()


@pytest.mark.parametrize("m_skip", [1, 2])
def test_rounds_in_launch_equal_the_phase_loop_state_for_state(m_skip):
    P = load_product()
    a, b = _tempering(P, True, m_skip=m_skip), _tempering(P, False, m_skip=m_skip)
    for r in range(4):
        a.round(S)
        b.round(S)
        for x, y in zip(_state(a), _state(b)):
            assert np.array_equal(x, y), f"round {r}"
        assert (a.sweeps_done, a.nmc_sweeps_done) == (b.sweeps_done, b.nmc_sweeps_done) == ((r + 1) * S, (r + 1) * len(PHASES) * S_NMC)
    assert not np.array_equal(a.slots(), np.arange(G) % L)            # swaps moved chains: the marked subset is not the first one's
    ea, eb = a.engs[0], b.engs[0]
    assert (ea.lane_calls, ea.phase_sweeps, ea.adopted) == (4, 0, 0) and (a.lane_nmc_rounds, a.lane_nmc_calls) == (4, 4)
    assert (eb.lane_calls, eb.phase_sweeps, eb.adopted) == (0, 4 * len(PHASES), 4 * (len(PHASES) - 1)) and b.lane_nmc_rounds == 0
    assert ea.asked == 1                                               # the engine is asked once, not every round


def test_the_default_is_the_module_constant():
    P = load_product()
    lt = _tempering(P, None)
    assert lt.lane_nmc is P.distributed.LANE_NMC_IN_LAUNCH


def test_a_round_that_wants_outputs_keeps_the_phase_loop():
    P = load_product()
    a, b = _tempering(P, True), _tempering(P, False)
    a.round(S)
    b.round(S)
    oa, ob = a.round(S, want_energy=True)[0], b.round(S, want_energy=True)[0]
    assert a.engs[0].lane_calls == 1 and a.engs[0].phase_sweeps == len(PHASES) and a.lane_nmc_rounds == 1
    assert len(oa["nmc"]) == len(PHASES)
    for x, y in zip(oa["nmc"], ob["nmc"]):
        assert np.array_equal(x["energy"], y["energy"])
    assert np.array_equal(oa["nmc_chains"], ob["nmc_chains"])
    for x, y in zip(_state(a), _state(b)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("has_query", [True, False])
def test_a_refusing_engine_falls_back_once_and_is_not_asked_again(has_query):
    P = load_product()

    class Refusing(NmcEngine):
        refuse = True
    Refusing.has_query = has_query
    a, b = _tempering(P, True, engine=Refusing), _tempering(P, False)
    for _ in range(3):
        a.round(S)
        b.round(S)
    e = a.engs[0]
    assert e.asked == 1 and e.lane_calls == 0 and e.phase_sweeps == 3 * len(PHASES) and a.lane_nmc_rounds == 0
    assert a.nmc_routes["lanes"].refused == {0}
    for x, y in zip(_state(a), _state(b)):
        assert np.array_equal(x, y)


def test_no_phase_planner_where_every_context_takes_the_call():
    P = load_product()
    a, b = _tempering(P, True), _tempering(P, False)
    a.plan(3 * S, 3)
    b.plan(3 * S, 3)
    assert a._planners is not None and a._nmc_planners is None
    assert b._nmc_planners is not None and b._nmc_planners[0].slot == 1

    class Refusing(NmcEngine):
        refuse = True
    c = _tempering(P, True, engine=Refusing)
    c.plan(3 * S, 3)
    assert c._nmc_planners is not None                                 # a context that keeps the loop keeps its planner


def test_npt_keywords():
    P = load_product()
    J, h = make_instance(16, seed=2)
    assert P.NPT(J, h, rng="philox").lane_nmc is None
    seen = []

    def device_resident(*a, **k):
        seen.append(a[4])
        return None, np.zeros(3)
    for lanes in ("force", "auto"):
        obj = P.NPT(J, h, rng="philox", seed=1, lanes=lanes, lane_nmc=True)
        assert obj.lane_nmc is True
        obj._run_device_resident = device_resident
        obj.run(np.linspace(0.5, 1.0, 3), 3, [False, True, False], num_sweeps_MCMC=4, num_sweeps_read=4, num_swap_attempts=2)
    assert len(seen) == 2 and all(s is not None for s in seen)          # lanes + doNMC is accepted once lane_nmc says how
    obj = P.NPT(J, h, rng="philox", seed=1, lanes="force", lane_nmc=False)
    obj._run_device_resident = device_resident
    obj.run(np.linspace(0.5, 1.0, 3), 3, [False, True, False], num_sweeps_MCMC=4, num_sweeps_read=4, num_swap_attempts=2)
    assert len(seen) == 3
    obj = P.NPT(J, h, rng="philox", seed=1, lanes="force")              # without the keyword: the refusal of before, unchanged
    obj._run_device_resident = device_resident
    with pytest.raises(ValueError, match="lanes runs plain replicas only"):
        obj.run(np.linspace(0.5, 1.0, 3), 3, [False, True, False], num_sweeps_MCMC=4, num_sweeps_read=4, num_swap_attempts=2)
    obj.run(np.linspace(0.5, 1.0, 3), 3, [False, False, False], num_sweeps_MCMC=4, num_sweeps_read=4, num_swap_attempts=2)
    assert len(seen) == 4 and seen[-1] is None
    obj = P.NPT(J, h, rng="philox", seed=1, precision="f64", lanes="force")
    with pytest.raises(ValueError, match="f64"):
        obj.run(np.linspace(0.5, 1.0, 3), 3, [False, True, False], num_sweeps_MCMC=4, num_sweeps_read=4, num_swap_attempts=2)


def test_binding_and_engine_wrapper():
    import ctypes
    import re
    P = load_product()
    lib = P._abi.lib()
    hdr = open(P._abi.os.path.join(P._abi.os.path.dirname(P._abi._PKG), "include", "nlmc.h")).read()
    assert re.search(r"int\s+nlmc_nmc_phases_lanes\s*\(\s*nlmc_ctx\s*\*", hdr)
    assert {"nlmc_nmc_phases_lanes", "nlmc_nmc_phases_lanes_refusal"} <= set(P._abi.EXPORTS)
    i, vp = ctypes.c_int, ctypes.c_void_p
    assert lib.nlmc_nmc_phases_lanes.argtypes == [vp, i, vp, i, i, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double, ctypes.c_double, i,
                                                  vp, vp, vp]
    assert lib.nlmc_nmc_phases_lanes(None, P._abi.F32, None, 1, 1, 0, 1, 1.0, 20.0, 1, None, None, None) == P._abi.ERR_ARG
    assert lib.nlmc_abi_version() == 3

    class FakeLib:
        calls = []

        def nlmc_subset_count(self, ctx):
            return 2

        def nlmc_nmc_phases_lanes(self, ctx, prec, kinds, P_, S_, sweep0, seed, beta, temp_x, stride, pmin, parg, best):
            k = np.ctypeslib.as_array(ctypes.cast(kinds, ctypes.POINTER(ctypes.c_int32)), (P_,)).tolist()
            self.calls.append((prec, k, S_, sweep0, seed, beta, temp_x, stride, pmin is not None, parg is not None, best is not None))
            if pmin is not None:
                np.ctypeslib.as_array(ctypes.cast(pmin, ctypes.POINTER(ctypes.c_int64)), (2 * P_,))[:] = np.arange(2 * P_) << 4
            return 0
    eng = P.Engine.__new__(P.Engine)
    eng._L, eng._ctx, eng.n, eng.energy_scale = FakeLib(), None, 5, 4
    assert eng.nmc_phases_lanes(["C", "NC", "ALL"], 4, SEED, (1 << 32) | 7, 2.5, 20.0, min_stride=2, precision="f64") is None
    assert eng._L.calls[-1] == (P._abi.F64, [1, 2, 0], 4, 7, SEED, 2.5, 20.0, 2, False, False, False)
    out = eng.nmc_phases_lanes(["C", "ALL"], 1, SEED, 0, 1.0, 20.0, want_minima=True, want_last_best=True)
    assert eng._L.calls[-1][-3:] == (True, True, True)
    assert out["phase_min"].shape == (2, 2) and np.array_equal(out["phase_min"], np.arange(4.0).reshape(2, 2))
    assert out["phase_argmin"].shape == (2, 2) and out["last_best"].shape == (2, 5)
    with pytest.raises(KeyError):
        eng.nmc_phases_lanes(["X"], 1, SEED, 0, 1.0, 20.0)
