"""Host-side handle on the HIP engine (one context = one instance (J,h) x a batch of chains on one GPU).

Everything that touches spins runs in the HIP kernels behind the C-ABI (include/nlmc.h).  This module only
marshals NumPy arrays; it contains no CPU implementation of the sweep and never imports `oracle`.
"""
import ctypes

import numpy as np
import scipy.sparse as sp

from . import _abi


class Instance:
    """(J, h) as the engine wants it: CSR, both triangles, sorted columns, explicit zeros dropped -- the matrix
    `scipy.sparse.csr_matrix(J)` the reference builds at NMC/nmc.py:53 -- without ever densifying a sparse input."""

    def __init__(self, J, h):
        A = sp.csr_matrix(J).astype(np.float64).copy()
        if A.shape[0] != A.shape[1]:
            raise ValueError("J must be square")
        A.eliminate_zeros()
        A.sort_indices()
        self.n = int(A.shape[0])
        self.indptr = np.ascontiguousarray(A.indptr, dtype=np.int32)
        self.indices = np.ascontiguousarray(A.indices, dtype=np.int32)
        self.data = np.ascontiguousarray(A.data, dtype=np.float64)
        self.h = np.ascontiguousarray(np.asarray(h, dtype=np.float64).reshape(-1))
        if self.h.shape[0] != self.n:
            raise ValueError("h must have one entry per spin")
        self.csr = A
        d = A - A.T
        self.symmetric = (d.nnz == 0) or (np.max(np.abs(d.data)) <= 1e-12 * max(1.0, float(np.max(np.abs(A.data)))
                                                                                  if A.nnz else 1.0))

    @property
    def nnz(self):
        return int(self.data.shape[0])


def _beta_table(beta, R, S):
    """beta: scalar | [R] | [S] (anneal schedule, only if R != S or flagged by shape) | [R,S] -> (array, cs, ss)."""
    b = np.asarray(beta, dtype=np.float64)
    if b.ndim == 0:
        return np.ascontiguousarray(b.reshape(1)), 0, 0
    if b.ndim == 2:
        if b.shape != (R, S):
            raise ValueError("beta table must be [n_chains, n_sweeps]")
        if S > 1 and (b == b[:, :1]).all():         # one temperature per chain: the kernels' plain variants (stride 0 over sweeps)
            return np.ascontiguousarray(b[:, 0]), 1, 0
        return np.ascontiguousarray(b), S, 1
    raise ValueError("pass a scalar or a 2-D table; use per_chain()/per_sweep() helpers for 1-D inputs")


def _precision(precision):
    """ "f32" / "f64" -> the library's NLMC_F32 / NLMC_F64 (KeyError for anything else)."""
    return {"f32": _abi.F32, "f64": _abi.F64}[precision]


class Engine:
    n_systems = 1            # independent APT systems the ladders are divided into (apt_systems; pt_init resets it)

    def __init__(self, J, h, n_chains, device=0, stream=None, chain_base=0, n_chains_global=None, own_stream=False):
        self.inst = J if isinstance(J, Instance) else Instance(J, h)
        if not self.inst.symmetric:
            raise ValueError("J must be symmetric: the heat-bath field and the incremental energy assume J == J^T")
        self.n = self.inst.n
        self.n_chains = int(n_chains)
        self.chain_base = int(chain_base)
        self.n_chains_global = int(n_chains_global if n_chains_global is not None else n_chains)
        self._L = _abi.lib()
        h_ = ctypes.c_void_p()
        rc = self._L.nlmc_create(ctypes.byref(h_), int(device), ctypes.c_void_p(stream) if stream else None, self.n,
                                 self.inst.nnz, _abi.ptr(self.inst.indptr), _abi.ptr(self.inst.indices),
                                 _abi.ptr(self.inst.data), _abi.ptr(self.inst.h), self.n_chains, self.chain_base,
                                 self.n_chains_global)
        _abi.check(rc, None)
        self._ctx = h_
        if own_stream:                # several contexts on one device: a stream each, or they execute one after the other
            self._ck(self._L.nlmc_own_stream(self._ctx))
        self.ladder_len = 0
        self._ahead = None
        self.fused_f64_real = False
        self._flags_on = False           # phase flags in force (set_flags / set_phase)
        self.lane_sweeps = "off"         # set_lane_sweeps
        self.wave_sweeps = "off"         # set_wave_sweeps
        self.wave_rounds = False         # set_wave_rounds
        self.wave_long = False           # set_wave_long
        self.wave_long_rounds = False    # set_wave_long_rounds
        self.energy_scale = int(self._L.nlmc_energy_scale(self._ctx))
        self.field_scale = int(self._L.nlmc_field_scale(self._ctx))      # qs of the "f32" path: Jq = rint(J 2^qs)

    # -- lifetime ---------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            self._L.nlmc_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
        return False

    def _ck(self, rc):
        _abi.check(rc, self._ctx)

    # -- state ------------------------------------------------------------------------------------------
    def set_spins(self, spins):
        s = _abi.as_c(spins, np.int8).reshape(self.n_chains, self.n)
        self._ck(self._L.nlmc_set_spins(self._ctx, _abi.ptr(s)))

    def get_spins(self):
        s = np.empty((self.n_chains, self.n), dtype=np.int8)
        self._ck(self._L.nlmc_get_spins(self._ctx, _abi.ptr(s)))
        return s

    def set_flags(self, flags, temp_x=1.0):
        if flags is None:
            self._ck(self._L.nlmc_set_flags(self._ctx, None, 1.0))
            self._flags_on = False
            return
        f = _abi.as_c(flags, np.uint8).reshape(self.n_chains, self.n)
        self._ck(self._L.nlmc_set_flags(self._ctx, _abi.ptr(f), float(temp_x)))
        self._flags_on = True

    def energy(self):
        out = np.empty(self.n_chains, dtype=np.float64)
        self._ck(self._L.nlmc_energy(self._ctx, _abi.ptr(out)))
        return out

    def energy_tracked(self):
        """The incrementally tracked energies (no recomputation)."""
        out = np.empty(self.n_chains, dtype=np.float64)
        self._ck(self._L.nlmc_energy_tracked(self._ctx, _abi.ptr(out)))
        return out

    def set_energy_sink(self, dev_ptr):
        """Later sweep calls also write the tracked energies of their final states to this device buffer (None: off)."""
        self._ck(self._L.nlmc_set_energy_sink(self._ctx, ctypes.c_void_p(int(dev_ptr)) if dev_ptr else None))

    def energy_dev(self, dev_ptr):
        self._ck(self._L.nlmc_energy_dev(self._ctx, ctypes.c_void_p(int(dev_ptr))))

    def energy_of(self, configs):
        c = _abi.as_c(configs, np.int8).reshape(-1, self.n)
        out = np.empty(c.shape[0], dtype=np.float64)
        self._ck(self._L.nlmc_energy_of(self._ctx, _abi.ptr(c), c.shape[0], _abi.ptr(out)))
        return out

    def energy_of_recorded(self, count, first=0):
        """fp64 energies of recorded configurations first .. first+count-1 of every chain of the most recent sweep call
        (`record_stride` > 0), taken from the device copy of its trace -> [rows of that call, count]."""
        out = np.empty((getattr(self, "_last_rows", self.n_chains), int(count)), dtype=np.float64)
        self._ck(self._L.nlmc_energy_of_recorded(self._ctx, int(first), int(count), _abi.ptr(out)))
        return out

    # -- sweeps -----------------------------------------------------------------------------------------
    def rows(self):
        """Chains a sweep call acts on: all of them, or the selected subset (select())."""
        return int(self._L.nlmc_subset_count(self._ctx))

    def _outputs(self, S, record_stride, want_energy, want_min, want_state):
        R, n = self.rows(), self.n
        self._last_rows = R
        o = {}
        o["spins"] = np.empty((R, (S + record_stride - 1) // record_stride, n), np.int8) if record_stride else None
        o["energy"] = np.empty((R, S), np.float64) if want_energy else None
        o["min_energy"] = np.empty(R, np.float64) if want_min else None
        o["argmin"] = np.empty(R, np.int32) if want_min else None
        o["argmin_state"] = np.empty((R, n), np.int8) if want_state else None
        return o

    STREAM_CHUNK_BYTES = 384 << 20      # staged permutation + uniforms + schedule per C-ABI call

    def sweep_stream(self, perm, u, beta, record_stride=0, want_energy=False, want_min=False, want_state=False):
        """Reference-stream sweeps (NMC/nmc.py:28-91).  perm,u: [R,S,N]; beta: scalar or [R,S] table.
        Long runs are cut into several C-ABI calls so that the staged stream stays bounded; the pieces are stitched
        back together (trace, energies, first-argmin bookkeeping) exactly as one call would return them."""
        R, n = self.n_chains, self.n
        perm = np.asarray(perm).reshape(R, -1, n)
        S = perm.shape[1]
        u = np.asarray(u).reshape(R, S, n)
        per_sweep = R * n * 36                         # 12 B of stream + ~24 B of per-chain schedule per spin
        chunk = max(1, self.STREAM_CHUNK_BYTES // max(1, per_sweep))
        if record_stride > 1:
            chunk = max(record_stride, chunk // record_stride * record_stride)
        if S > chunk:
            b = np.asarray(beta, dtype=np.float64)
            outs = []
            for t0 in range(0, S, chunk):
                t1 = min(S, t0 + chunk)
                outs.append(self.sweep_stream(perm[:, t0:t1], u[:, t0:t1], b if b.ndim == 0 else b[:, t0:t1], record_stride,
                                              want_energy, want_min, want_state))
            return _stitch_outputs(outs, chunk, record_stride, want_energy, want_min, want_state)
        perm = _abi.as_c(perm, np.int32)
        u = _abi.as_c(u, np.float64)
        tab, cs, ss = _beta_table(beta, R, S)
        o = self._outputs(S, record_stride, want_energy, want_min, want_state)
        self._ck(self._L.nlmc_sweep_stream(self._ctx, S, _abi.ptr(perm), _abi.ptr(u), _abi.ptr(tab), cs, ss,
                                           max(1, record_stride), _abi.ptr(o["spins"]), _abi.ptr(o["energy"]),
                                           _abi.ptr(o["min_energy"]), _abi.ptr(o["argmin"]),
                                           _abi.ptr(o["argmin_state"])))
        return o

    def sweep_philox(self, n_sweeps, seed, sweep0=0, beta=None, precision="f32", order="shared", record_stride=0,
                     want_energy=False, want_min=False, want_state=False):
        """Throughput sweeps (device Philox).  beta: scalar | [R,S] table | None (= PT ladder)."""
        R = self.rows()
        S = int(n_sweeps)
        if beta is None:
            tabp, cs, ss = None, 0, 0
        else:
            tab, cs, ss = _beta_table(beta, R, S)
            tabp = _abi.ptr(tab)
        o = self._outputs(S, record_stride, want_energy, want_min, want_state)
        prec = _precision(precision)
        om = {"shared": _abi.ORDER_SHARED, "per_chain": _abi.ORDER_PER_CHAIN}[order]
        self._ck(self._L.nlmc_sweep_philox(self._ctx, prec, om, S, int(sweep0) & 0xFFFFFFFF, int(seed), tabp, cs, ss,
                                           max(1, record_stride), _abi.ptr(o["spins"]), _abi.ptr(o["energy"]),
                                           _abi.ptr(o["min_energy"]), _abi.ptr(o["argmin"]),
                                           _abi.ptr(o["argmin_state"])))
        return o

    FUSED_PLAN_BUDGET = 1 << 30        # bytes of fused-window plan one sweep_philox_windows piece may hold

    def fused_plan_bytes(self, window):
        rows = np.diff(self.inst.indptr)
        return fused_plan_bytes(self.n, int(np.count_nonzero(rows > 8) + 2 * np.count_nonzero(rows > 16)), window,
                                value_plane=self.fused_f64_real)

    def set_fused_f64_real(self, on=True):
        """Opt-in: the fp64 mode runs on fused windows for real couplings and fields too (include/nlmc.h:
        nlmc_set_fused_f64_real) -- same bits as sweep by sweep.  Plans made while it is on carry an fp64 value plane (72 more
        bytes per schedule position).  sweep_philox, pt_rounds_deferred and pt_rounds_fused all take such instances then.  Changing
        the setting drops the current fused plans."""
        self._ck(self._L.nlmc_set_fused_f64_real(self._ctx, 1 if on else 0))
        self.fused_f64_real = bool(on)

    LANE_MODES = {"off": _abi.LANES_OFF, "auto": _abi.LANES_AUTO, "force": _abi.LANES_FORCE}
    WAVE_MODES = {"off": _abi.WAVES_OFF, "auto": _abi.WAVES_AUTO, "force": _abi.WAVES_FORCE}
    ROUTES = {_abi.ROUTE_STEPWISE: "stepwise", _abi.ROUTE_FUSED: "fused", _abi.ROUTE_LANES: "lanes", _abi.ROUTE_WAVES: "waves"}

    def set_lane_sweeps(self, mode):
        """Chain-per-lane sweeps for short chains (include/nlmc.h: nlmc_set_lane_sweeps): "off" (the default), "auto" (sweep_philox
        calls with n < 256 over at least NLMC_LANE_AUTO_ROWS rows), "force" (every sweep_philox call with n <= 1024).  The results
        are the same bits on every route; last_sweep_route() tells which one a call took."""
        if mode not in self.LANE_MODES:
            raise ValueError(f"set_lane_sweeps: mode must be one of {sorted(self.LANE_MODES)}, got {mode!r}")
        self._ck(self._L.nlmc_set_lane_sweeps(self._ctx, self.LANE_MODES[mode]))
        self.lane_sweeps = mode

    def set_wave_sweeps(self, mode):
        """Wave-per-chain sweeps with resident local fields for short chains (include/nlmc.h: nlmc_set_wave_sweeps): "off" (the
        default), "auto" (f32 sweep_philox calls with n <= 256 over at most NLMC_WAVE_AUTO_MAX_ROWS rows), "force" (every f32
        sweep_philox call with n <= 256).  Calls the route does not take (f64, longer chains) run as before.  The results are the
        same bits on every route; last_sweep_route() tells which one a call took."""
        if mode not in self.WAVE_MODES:
            raise ValueError(f"set_wave_sweeps: mode must be one of {sorted(self.WAVE_MODES)}, got {mode!r}")
        self._ck(self._L.nlmc_set_wave_sweeps(self._ctx, self.WAVE_MODES[mode]))
        self.wave_sweeps = mode

    def set_wave_rounds(self, on):
        """Whether pt_rounds_deferred runs its rounds inside k_rounds_waves launches (include/nlmc.h: nlmc_set_wave_rounds) where the
        context's sweeps go to the wave kernels (waves_take) and pt_rounds_waves' conditions hold: asked before the lane rule and
        before any fused-window plan.  Default off: nothing changes for any caller.  Same bits either way."""
        self._ck(self._L.nlmc_set_wave_rounds(self._ctx, 1 if on else 0))
        self.wave_rounds = bool(on)

    def set_wave_long(self, on=True):
        """Whether the wave route takes chains of up to 1024 spins instead of 256 (include/nlmc.h: nlmc_set_wave_long): dense chains of
        257..1024 spins then sweep one per wave in k_sweep_waves_long, fields in registers and in LDS, under the mode rules of
        set_wave_sweeps.  The rounds inside a wave launch keep their limit of 256 spins: with set_wave_rounds, pt_rounds_deferred runs
        a longer chain's rounds as a sweep call and a swap call each, unless set_wave_long_rounds hands them to k_rounds_waves_long.
        Default off: nothing changes for any caller.  Same bits either
        way."""
        self._ck(self._L.nlmc_set_wave_long(self._ctx, 1 if on else 0))
        self.wave_long = bool(on)

    def set_wave_long_rounds(self, on=True):
        """Whether pt_rounds_deferred runs the rounds of chains of 257..1024 spins inside k_rounds_waves_long launches (include/nlmc.h:
        nlmc_set_wave_long_rounds): the local fields are built once per chunk of rounds and stay in LDS across the swap rounds.  Takes
        effect with set_wave_rounds and set_wave_long both on, where the context's sweeps go to the wave kernels (waves_take) and
        pt_rounds_waves_long's conditions hold; otherwise such rounds stay a sweep call and a swap call each.  Default off: nothing
        changes for any caller.  Same bits either way."""
        self._ck(self._L.nlmc_set_wave_long_rounds(self._ctx, 1 if on else 0))
        self.wave_long_rounds = bool(on)

    def waves_take(self, rows=None, precision="f32"):
        """Whether the context routes a sweep_philox call over `rows` rows (default: the selected chains) in `precision` to the
        wave-per-chain kernels -- the rule of nlmc_set_wave_sweeps (chains of up to 1024 spins under set_wave_long, 256 otherwise),
        asked before lanes_take.  Such a call needs no fused-window plan."""
        mode = getattr(self, "wave_sweeps", "off")
        if mode == "off" or precision != "f32" or self.n > (_abi.WAVE_LONG_N if getattr(self, "wave_long", False) else _abi.WAVE_N):
            return False
        if mode == "force":
            return True
        rows = self.rows() if rows is None else int(rows)
        return rows <= _abi.WAVE_AUTO_MAX_ROWS

    def last_sweep_route(self):
        """Route of the most recent sweep_philox call: "stepwise", "fused", "lanes", "waves", or None before any (nlmc_last_sweep_route)."""
        return self.ROUTES.get(int(self._L.nlmc_last_sweep_route(self._ctx)))

    def lanes_take(self, rows=None):
        """Whether the context routes a sweep_philox call over `rows` rows (default: the selected chains) to the chain-per-lane
        kernels -- the rule of nlmc_set_lane_sweeps.  Such a call needs no fused-window plan."""
        if self.lane_sweeps == "force":
            return self.n <= _abi.LANE_N
        rows = self.rows() if rows is None else int(rows)
        return self.lane_sweeps == "auto" and self.n < 256 and rows >= _abi.LANE_AUTO_ROWS

    def _last_fused(self):
        """Whether every launch of the most recent sweep call ran on fused windows (nlmc_last_sweep_fused)."""
        return bool(self._L.nlmc_last_sweep_fused(self._ctx))

    def sweep_philox_windows(self, n_sweeps, seed, sweep0=0, beta=None, window=None, budget_bytes=None, record_stride=0,
                             want_energy=False, want_min=False, want_state=False, want_recorded_energy=False, precision="f32"):
        """sweep_philox on fused windows planned piece by piece against a memory budget (one planning call for a
        whole run of 10^4 sweeps takes 23 GB at N = 10^3, 230 GB at N = 10^4): the call is cut into pieces of at most
        budget_bytes / fused_plan_bytes windows, each planned, swept and dropped; pieces whose plan is refused (instance or
        window outside what the fused kernels take) run sweep by sweep -- same bits.  Outputs are stitched together exactly
        as one call would return them (trace, energies, first argmin).  want_recorded_energy: o["energy_recorded"] = fp64
        energies of the recorded configurations [rows, n_recorded], computed on the device copy of each piece's trace.
        precision: "f32" or "f64" (the fp64 mode takes the fused windows where fused_modes says so -- with an [R, S] table, a
        temperature per sweep, when no phase flags are in force and the instance is dyadic -- and runs sweep by sweep otherwise; fused_last_call tells)."""
        S = int(n_sweeps)
        T = fused_window(S) if window is None else int(window)
        budget = self.FUSED_PLAN_BUDGET if budget_bytes is None else int(budget_bytes)
        rec_e = bool(want_recorded_energy and record_stride)
        if S > 0 and (self.waves_take(precision=precision) or self.lanes_take()):   # the context runs this call one chain per wave or per lane: no windows to plan
            o = self.sweep_philox(S, seed, sweep0=sweep0, beta=beta, record_stride=record_stride, want_energy=want_energy,
                                  want_min=want_min, want_state=want_state, precision=precision)
            self.fused_last_call = False
            if rec_e:
                o["energy_recorded"] = self.energy_of_recorded(o["spins"].shape[1])
            return o
        a = getattr(self, "_ahead", None)
        if (a is not None and window is None and a.window and S == a.S and int(seed) == a.seed and (int(sweep0) - a.sweep0) % max(1, S) == 0
                and 0 <= (int(sweep0) - a.sweep0) // max(1, S) < a.R
                and sweeps_per_plan_piece(self.fused_plan_bytes(a.window), S, a.window, budget, record_stride) == S):
            ii = (int(sweep0) - a.sweep0) // S          # launch ii of the run announced with plan_ahead: its windows are (or get)
            a.prepare(ii)                                # planned together with those of the launches that follow
            if a.fused_covers(ii):
                o = self.sweep_philox(S, seed, sweep0=sweep0, beta=beta, record_stride=record_stride, want_energy=want_energy,
                                      want_min=want_min, want_state=want_state, precision=precision)
                self.fused_last_call = self._last_fused()
                if rec_e:
                    o["energy_recorded"] = self.energy_of_recorded(o["spins"].shape[1])
                return o
        if not T or S % T or S == 0:
            o = self.sweep_philox(S, seed, sweep0=sweep0, beta=beta, record_stride=record_stride, want_energy=want_energy,
                                  want_min=want_min, want_state=want_state, precision=precision)
            self.fused_last_call = S > 0 and self._last_fused()
            if rec_e and S > 0:
                o["energy_recorded"] = self.energy_of_recorded(o["spins"].shape[1])
            return o
        per_piece = sweeps_per_plan_piece(self.fused_plan_bytes(T), S, T, budget, record_stride)
        b = None if beta is None else np.asarray(beta, dtype=np.float64)
        outs, fused, ran_fused = [], True, True
        if a is not None:                    # this call plans into the slot the announced run's windows live in: they are gone
            a.drop_windows()
            self.plan_slot(a.slot)
        for t0 in range(0, S, per_piece):
            t1 = min(S, t0 + per_piece)
            if fused:
                fused = self.plan_philox_fused(sweep0 + t0, (t1 - t0) // T, T, seed) == (t1 - t0) // T     # refused once: stop asking
            outs.append(self.sweep_philox(t1 - t0, seed, sweep0=sweep0 + t0, beta=b if (b is None or b.ndim < 2) else b[:, t0:t1],
                                          record_stride=record_stride, want_energy=want_energy, want_min=want_min,
                                          want_state=want_state, precision=precision))
            ran_fused = ran_fused and self._last_fused()
            if rec_e:
                outs[-1]["energy_recorded"] = self.energy_of_recorded(outs[-1]["spins"].shape[1])
        self.fused_last_call = ran_fused
        o = outs[0] if len(outs) == 1 else _stitch_outputs(outs, per_piece, record_stride, want_energy, want_min, want_state)
        if rec_e and len(outs) > 1:
            o["energy_recorded"] = np.concatenate([p["energy_recorded"] for p in outs], axis=1)
        return o

    def plan_ahead(self, sweep0, n_launches, sweeps_per_launch, seed, budget_bytes=None, precision="f32"):
        """Announce `n_launches` sweep_philox_windows calls of `sweeps_per_launch` sweeps each at consecutive sweep indices from
        `sweep0` (the phases of an NMC run): their fused windows depend on the RNG only and are planned a budget's worth of
        LAUNCHES at a time instead of one launch at a time -- a planning launch is latency-bound (~1.5 ms whether it builds 9
        windows or 200; per phase launch that was 27 % of C2 through NMC.run_restarts).  plan_ahead(None) ends it.
        precision: that of the announced calls ("f32" / "f64")."""
        if sweep0 is None or n_launches <= 0 or sweeps_per_launch <= 0:
            self._ahead = None
            return
        self._ahead = RoundPlanner(self, sweep0, n_launches, sweeps_per_launch, seed, precision=precision,
                                   budget_bytes=self.FUSED_PLAN_BUDGET if budget_bytes is None else budget_bytes, slot=0,
                                   fused_outputs=True)

    def plan_philox(self, sweep0, n_sweeps, seed, precision="f32"):
        self._ck(self._L.nlmc_plan_philox(self._ctx, _precision(precision), _abi.ORDER_SHARED, int(sweep0), int(n_sweeps), int(seed)))

    def plan_philox_fused(self, sweep0, n_windows, window, seed):
        """Fused-window schedules for `n_windows` launches of exactly `window` sweeps (include/nlmc.h).  Returns the
        number of windows planned (0: the instance does not qualify; calls then take the sweep-by-sweep path)."""
        k = ctypes.c_int32(0)
        self._ck(self._L.nlmc_plan_philox_fused(self._ctx, int(sweep0) & 0xFFFFFFFF, int(n_windows), int(window), int(seed),
                                                ctypes.byref(k)))
        return int(k.value)

    def fused_modes(self, window):
        """Precisions that may run on fused windows of `window` sweeps here: subset of {"f32", "f64"} (nlmc_fused_modes)."""
        m = int(self._L.nlmc_fused_modes(self._ctx, int(window)))
        return {p for bit, p in ((1, "f32"), (2, "f64")) if m & bit}

    def plan_slot(self, slot):
        """Fused-window plans live in two slots (include/nlmc.h: nlmc_plan_slot); planning calls write to the selected one."""
        self._ck(self._L.nlmc_plan_slot(self._ctx, int(slot)))

    def plan_levels(self, window):
        """Chunks (64 schedule positions) per level of a planned fused window of the selected plan slot (diagnostic)."""
        off = np.zeros(1025, dtype=np.int32)
        nl = ctypes.c_int32(0)
        self._ck(self._L.nlmc_plan_get_levels(self._ctx, int(window), _abi.ptr(off), 1025, ctypes.byref(nl)))
        return np.diff(off[:nl.value + 1])

    PLAN_INFO = ("fmt", "pstride", "T", "sweep0", "seed", "workers", "quads", "bank_aware", "n_pad", "k_dummy", "k_zero", "neg_off",
                 "tab_words", "nlev", "npos", "hi_max", "has_val", "level_fill", "planes")

    def plan_items(self, window):
        """Read-back of a planned fused window of the selected plan slot (include/nlmc.h: nlmc_plan_get_items; diagnostic): the
        constants of PLAN_INFO as ints and the raw arrays head [npos, 2], ell [planes, npos, 4] (int32), val (float64
        [9 npos]: four planes of [npos, 2], then the field plane; None without a value plane), loff [nlev + 1], send [T].
        nlev == 0: the window got no fused schedule, and there are no arrays."""
        info = np.zeros(24, dtype=np.int64)
        self._ck(self._L.nlmc_plan_get_items(self._ctx, int(window), _abi.ptr(info), None, None, None, None, None, 0))
        d = {k: int(v) for k, v in zip(self.PLAN_INFO, info)}
        d["seed"] &= 0xFFFFFFFFFFFFFFFF
        d["val"] = None
        if d["nlev"] == 0:
            return d
        npos = d["npos"]
        head, ell = np.zeros((npos, 2), dtype=np.int32), np.zeros((d["planes"], npos, 4), dtype=np.int32)
        val = np.zeros(9 * npos, dtype=np.float64) if d["has_val"] else None
        loff, send = np.zeros(1025, dtype=np.int32), np.zeros(64, dtype=np.int32)
        self._ck(self._L.nlmc_plan_get_items(self._ctx, int(window), _abi.ptr(info), _abi.ptr(head), _abi.ptr(ell), _abi.ptr(val),
                                             _abi.ptr(loff), _abi.ptr(send), npos))
        d.update(head=head, ell=ell, val=val, loff=loff[:d["nlev"] + 1].copy(), send=send[:d["T"]].copy())
        # the window's head stream (include/nlmc.h: nlmc_plan_get_head_stream): [ceil(nlev / 4), workers, 64, 4] int32, element
        # [l // 4, w, lane, l % 4] = head[64 * (loff[l] + w) + lane, 0] for every chunk w the level has (other elements undefined)
        # None: the plan carries no stream (info word 19: a field term, 8-byte entries, or NLMC_NO_HEAD_STREAM at creation)
        d["head_stream"] = None
        if int(info[19]):
            hs = np.zeros(((d["nlev"] + 3) // 4, d["workers"], 64, 4), dtype=np.int32)
            self._ck(self._L.nlmc_plan_get_head_stream(self._ctx, int(window), _abi.ptr(hs), hs.size))
            d["head_stream"] = dict(hs=hs, workers=d["workers"])
        return d

    def plan_order(self, order):
        """Read-back of order `order` of the per-sweep plan (plan_philox; include/nlmc.h: nlmc_plan_get_order; diagnostic):
        order [n, 2] int32, lvl_off [nlev + 1], nlev, hi_max, big (the global-memory levelizer built it), cap (widest published
        level, 0: none), orders, sweep0."""
        info = np.zeros(8, dtype=np.int64)
        self._ck(self._L.nlmc_plan_get_order(self._ctx, int(order), _abi.ptr(info), None, None, 0))
        n, nlev = int(info[0]), int(info[1])
        items, off = np.zeros((n, 2), dtype=np.int32), np.zeros(n + 1, dtype=np.int32)
        self._ck(self._L.nlmc_plan_get_order(self._ctx, int(order), _abi.ptr(info), _abi.ptr(items), _abi.ptr(off), n))
        return dict(order=items, lvl_off=off[:nlev + 1].copy(), nlev=nlev, hi_max=int(info[2]), big=bool(info[3]), cap=int(info[4]),
                    orders=int(info[5]), sweep0=int(info[6]))

    def plan_reserve_fused(self, n_windows, window):
        """Allocate the fused-window plan buffers for up to n_windows windows (no schedule is built)."""
        self._ck(self._L.nlmc_plan_reserve_fused(self._ctx, int(n_windows), int(window)))

    # -- replica exchange -------------------------------------------------------------------------------
    def pt_init(self, beta_list):
        b = _abi.as_c(beta_list, np.float64).reshape(-1)
        self._ck(self._L.nlmc_pt_init(self._ctx, b.shape[0], _abi.ptr(b)))
        self.ladder_len = int(b.shape[0])
        self.n_systems = 1

    def pt_slots(self):
        s = np.empty(self.n_chains_global, dtype=np.int32)
        self._ck(self._L.nlmc_pt_get_slots(self._ctx, _abi.ptr(s)))
        return s

    def pt_set_slots(self, slots):
        s = _abi.as_c(slots, np.int32).reshape(self.n_chains_global)
        self._ck(self._L.nlmc_pt_set_slots(self._ctx, _abi.ptr(s)))

    def pt_apply_swap(self, ladder, slot_a, slot_b):
        self._ck(self._L.nlmc_pt_apply_swap(self._ctx, int(ladder), int(slot_a), int(slot_b)))

    def pt_swap_philox(self, round_idx, seed, n_pairs, energies_all_dev=None, want_log=True):
        nl = self.n_chains_global // self.ladder_len
        pairs = np.empty((nl, n_pairs, 2), np.int32) if want_log else None
        acc = np.empty((nl, n_pairs), np.uint8) if want_log else None
        dev = ctypes.c_void_p(int(energies_all_dev)) if energies_all_dev else None
        self._ck(self._L.nlmc_pt_swap_philox(self._ctx, int(round_idx), int(seed), int(n_pairs), dev, _abi.ptr(pairs),
                                             _abi.ptr(acc)))
        return pairs, acc

    def pt_swap_philox_host(self, round_idx, seed, n_pairs, energies_all, want_log=False):
        """Swap round of a sharded context with the all-gathered energies in host memory."""
        nl = self.n_chains_global // self.ladder_len
        pairs = np.empty((nl, n_pairs, 2), np.int32) if want_log else None
        acc = np.empty((nl, n_pairs), np.uint8) if want_log else None
        e = _abi.as_c(energies_all, np.float64).reshape(self.n_chains_global)
        self._ck(self._L.nlmc_pt_swap_philox_host(self._ctx, int(round_idx), int(seed), int(n_pairs), _abi.ptr(e),
                                                  _abi.ptr(pairs), _abi.ptr(acc)))
        return pairs, acc

    # -- sharded ladders: the per-round all-gather issued by the library (include/nlmc.h: nlmc_comm_init) -------------
    @staticmethod
    def comm_unique_id():
        out = np.zeros(128, dtype=np.uint8)
        _abi.check(_abi.lib().nlmc_comm_unique_id(_abi.ptr(out)), None)
        return out

    def comm_init(self, unique_id, world, rank):
        uid = _abi.as_c(unique_id, np.uint8).reshape(128)
        self._ck(self._L.nlmc_comm_init(self._ctx, _abi.ptr(uid), int(world), int(rank)))

    def pt_swap_philox_collective(self, round_idx, seed, n_pairs, refresh_energies=False, want_log=False):
        nl = self.n_chains_global // self.ladder_len
        pairs = np.empty((nl, n_pairs, 2), np.int32) if want_log else None
        acc = np.empty((nl, n_pairs), np.uint8) if want_log else None
        self._ck(self._L.nlmc_pt_swap_philox_collective(self._ctx, int(round_idx), int(seed), int(n_pairs), int(bool(refresh_energies)),
                                                        _abi.ptr(pairs), _abi.ptr(acc)))
        return pairs, acc

    @staticmethod
    def comm_probe():
        """True when this process can load librccl (nlmc_comm_probe); every rank asks before comm_init and the ranks agree."""
        return _abi.lib().nlmc_comm_probe() == _abi.OK

    def comm_check(self, timeout_ms=-1):
        """RCCL asynchronous error flag, and with timeout_ms >= 0 a bounded wait for the collectives queued on the context's stream;
        RuntimeError after aborting the communicator (include/nlmc.h: nlmc_comm_check)."""
        self._ck(self._L.nlmc_comm_check(self._ctx, int(timeout_ms)))

    # -- APT run cut into temperature-slot blocks over ranks (include/nlmc.h: nlmc_apt_shard) -------------------------------
    def apt_shard(self, beta_global, world, rank):
        b = _abi.as_c(beta_global, np.float64).reshape(-1)
        self._ck(self._L.nlmc_apt_shard(self._ctx, b.shape[0], int(world), int(rank), _abi.ptr(b)))
        self.apt_world, self.apt_rank, self.apt_R = int(world), int(rank), int(b.shape[0])

    def apt_systems(self, n_systems):
        """Divide the context's n_ladders = M K ladders into M = n_systems independent APT systems of K ladders (include/nlmc.h:
        nlmc_apt_systems): icm_round_ladders and apt_rounds_lanes then pair the ladders of each system among themselves and list
        their info rows in the order (system, slot, pair); everything else stays keyed by global chain and ladder ids, so system 0
        has the bits of a one-system context of K L chains.  After pt_init (which resets it to 1); not together with apt_shard."""
        self._ck(self._L.nlmc_apt_systems(self._ctx, int(n_systems)))
        self.n_systems = int(n_systems)

    def _icm_rows(self):
        """Houdayer pairs of one round: M systems x L slots x (K // 2), K the ladders of a system."""
        R, M = self.ladder_len, self.n_systems
        return M * R * ((self.n_chains_global // R // M) // 2) if R else 0

    def apt_pack(self, want_configs=True):
        """(tracked energies [K, Rw] int64 in units of 2^-energy_scale by (ladder, local slot), configurations on local slot 0
        [K, n], on local slot Rw - 1 [K, n])."""
        K = self.n_chains // self.ladder_len
        e = np.empty((K, self.ladder_len), np.int64)
        lo = np.empty((K, self.n), np.int8) if want_configs else None
        hi = np.empty((K, self.n), np.int8) if want_configs else None
        self._ck(self._L.nlmc_apt_pack(self._ctx, _abi.ptr(e), _abi.ptr(lo), _abi.ptr(hi)))
        return e, lo, hi

    def _apt_log(self, n_pairs, want_log):
        K = self.n_chains // self.ladder_len
        return (np.empty((K, n_pairs, 2), np.int32), np.empty((K, n_pairs), np.uint8)) if want_log else (None, None)

    def apt_swap_host(self, round_idx, seed, n_pairs, efix_all, recv_lo, recv_hi, want_log=False):
        pairs, acc = self._apt_log(n_pairs, want_log)
        e = _abi.as_c(efix_all, np.int64).reshape(self.apt_world, -1, self.ladder_len)
        lo = None if recv_lo is None else _abi.as_c(recv_lo, np.int8).reshape(-1, self.n)
        hi = None if recv_hi is None else _abi.as_c(recv_hi, np.int8).reshape(-1, self.n)
        self._ck(self._L.nlmc_apt_swap_host(self._ctx, int(round_idx), int(seed), int(n_pairs), _abi.ptr(e), _abi.ptr(lo), _abi.ptr(hi),
                                            _abi.ptr(pairs), _abi.ptr(acc)))
        return pairs, acc

    def apt_selftest_exchange(self):
        """(recv_lo, recv_hi) [K, n] of the collective path's neighbour exchange run with this rank as its own neighbour."""
        K = self.n_chains // self.ladder_len
        lo, hi = np.empty((K, self.n), np.int8), np.empty((K, self.n), np.int8)
        self._ck(self._L.nlmc_apt_selftest_exchange(self._ctx, _abi.ptr(lo), _abi.ptr(hi)))
        return lo, hi

    def apt_swap_collective(self, round_idx, seed, n_pairs, want_log=False):
        pairs, acc = self._apt_log(n_pairs, want_log)
        self._ck(self._L.nlmc_apt_swap_collective(self._ctx, int(round_idx), int(seed), int(n_pairs), _abi.ptr(pairs), _abi.ptr(acc)))
        return pairs, acc

    def pt_plan(self, round0, n_rounds, seed, n_pairs):
        self._ck(self._L.nlmc_pt_plan(self._ctx, int(round0), int(n_rounds), int(seed), int(n_pairs)))

    def _rounds_call(self, fn, n_rounds, sweeps_per_round, seed, sweep0, round0, n_pairs, precision, *more):
        """One call of a rounds entry point of the library (they share their leading arguments; `more`: what follows them).  True when
        the rounds were queued; False, with the library's reason in rounds_fused_refusal, when it answers NLMC_ERR_UNSUPPORTED."""
        rc = fn(self._ctx, _precision(precision), int(n_rounds), int(sweeps_per_round), int(sweep0) & 0xFFFFFFFF,
                int(round0) & 0xFFFFFFFF, int(seed), int(n_pairs), *more)
        if rc == _abi.ERR_UNSUPPORTED:
            self.rounds_fused_refusal = _abi.lib().nlmc_last_error(self._ctx).decode()
            return False
        self._ck(rc)
        return True

    def pt_rounds_fused(self, n_rounds, sweeps_per_round, seed, sweep0, round0, n_pairs, precision="f32"):
        """n_rounds whole rounds (sweeps + swap round) inside cooperative launches (include/nlmc.h: nlmc_pt_rounds_fused), in any of the
        three arithmetics: "f32", "f64" on dyadic instances, "f64" on real-valued ones with set_fused_f64_real on.  True when the
        rounds were queued, False when the context / plans do not qualify (nothing was run: drive the rounds one by one; the reason
        is in rounds_fused_refusal)."""
        return self._rounds_call(self._L.nlmc_pt_rounds_fused, n_rounds, sweeps_per_round, seed, sweep0, round0, n_pairs, precision)

    def pt_rounds_deferred(self, n_rounds, sweeps_per_round, seed, sweep0, round0, n_pairs, precision="f32"):
        """n_rounds rounds on the route that fits (include/nlmc.h: nlmc_pt_rounds_deferred): inside k_rounds_fused launches where all
        chains are resident at once, otherwise n_rounds sweep launches (each decides the previous round's swap in its prologue) + one
        swap launch; last_rounds_route() tells which.  Real-valued "f64" instances (set_fused_f64_real) keep the launch per round
        by default (include/nlmc.h says why); pt_rounds_fused asks for their k_rounds_fused variant by name.  True when queued, False
        when the context / plans do not qualify.  What LocalTempering.run_rounds and ShardedTempering.run_rounds call."""
        return self._rounds_call(self._L.nlmc_pt_rounds_deferred, n_rounds, sweeps_per_round, seed, sweep0, round0, n_pairs, precision)

    def pt_rounds_lanes(self, n_rounds, sweeps_per_round, seed, sweep0, round0, n_pairs, precision="f32"):
        """n_rounds whole rounds of short chains inside k_rounds_lanes launches, whatever the lane mode is (include/nlmc.h:
        nlmc_pt_rounds_lanes): a chain per lane, a ladder of at most 64 temperatures inside one wave, n <= 1024, pair selections planned
        (pt_plan), no fused-window plan.  True when the rounds were queued, False when the context does not qualify (nothing was run;
        the reason is in rounds_fused_refusal).  pt_rounds_deferred takes this route by itself under set_lane_sweeps("force")."""
        return self._rounds_call(self._L.nlmc_pt_rounds_lanes, n_rounds, sweeps_per_round, seed, sweep0, round0, n_pairs, precision)

    def pt_rounds_waves(self, n_rounds, sweeps_per_round, seed, sweep0, round0, n_pairs, precision="f32"):
        """n_rounds whole rounds of short chains inside k_rounds_waves launches, whatever the wave mode is (include/nlmc.h:
        nlmc_pt_rounds_waves): a chain per wave with resident local fields, whole ladders of at most 64 temperatures per workgroup,
        f32 only, n <= 256, pair selections planned (pt_plan), no fused-window plan.  True when the rounds were queued, False when
        the context does not qualify (nothing was run; the reason is in rounds_fused_refusal).  pt_rounds_deferred takes this route
        by itself under set_wave_sweeps("force") with set_wave_rounds(True)."""
        return self._rounds_call(self._L.nlmc_pt_rounds_waves, n_rounds, sweeps_per_round, seed, sweep0, round0, n_pairs, precision)

    def pt_rounds_waves_long(self, n_rounds, sweeps_per_round, seed, sweep0, round0, n_pairs, precision="f32"):
        """n_rounds whole rounds of dense chains of 257..1024 spins inside k_rounds_waves_long launches, whatever the wave mode is
        (include/nlmc.h: nlmc_pt_rounds_waves_long): a chain per wave, its local fields built once per launch and resident in LDS
        across the swap rounds, whole ladders of at most 64 temperatures per workgroup as far as its LDS holds their regions, f32 only,
        pair selections planned (pt_plan), no fused-window plan.  True when the rounds were queued, False when the context does not
        qualify (nothing was run; the reason is in rounds_fused_refusal).  pt_rounds_deferred takes this route by itself under
        set_wave_sweeps("force") with set_wave_rounds, set_wave_long and set_wave_long_rounds on."""
        return self._rounds_call(self._L.nlmc_pt_rounds_waves_long, n_rounds, sweeps_per_round, seed, sweep0, round0, n_pairs, precision)

    def apt_rounds_lanes(self, n_rounds, sweeps_per_round, seed, sweep0, round0, n_pairs, katzgraber=True, precision="f32",
                         want_info=False):
        """n_rounds whole APT rounds of short chains -- sweeps, the Houdayer step of icm_round_ladders, the swap round -- inside
        k_apt_rounds_lanes launches (include/nlmc.h: nlmc_apt_rounds_lanes): the whole system of K sub-replica ladders in one
        workgroup, a chain per lane, a Houdayer pair per lane.  n_pairs = 0: rounds without swaps; otherwise the pair selections are
        planned (pt_plan).  Returns (queued, info): queued False when the context does not qualify (nothing was run; the reason is in
        rounds_fused_refusal); info [n_rounds, L * (K // 2), 2] = {n_components, picked size} with want_info (a read-back: it
        synchronises the stream), else None.  Same bits as sweep_philox(beta=None) + icm_round_ladders + pt_swap_philox round by round.
        Under apt_systems(M): a workgroup per system, K the ladders of one system, info [n_rounds, M * L * (K // 2), 2]."""
        info = np.zeros((int(n_rounds), self._icm_rows(), 2), np.int32) if want_info else None
        queued = self._rounds_call(self._L.nlmc_apt_rounds_lanes, n_rounds, sweeps_per_round, seed, sweep0, round0, n_pairs, precision,
                                   int(bool(katzgraber)), _abi.ptr(info))
        return queued, (info if queued else None)

    def last_rounds_route(self, heads=False):
        """The route the last pt_rounds_fused / pt_rounds_deferred / pt_rounds_lanes / pt_rounds_waves / pt_rounds_waves_long /
        apt_rounds_lanes call that ran took: "in launch" (the rounds inside k_rounds_fused launches), "launch per round", "lanes"
        (inside k_rounds_lanes launches), "apt lanes" (inside k_apt_rounds_lanes launches), "waves" (inside k_rounds_waves launches),
        "waves long" (inside k_rounds_waves_long launches), or None before any such call (include/nlmc.h: nlmc_pt_rounds_route).
        heads=True: a route on fused windows also names where its launches read the item heads, "in launch, head stream" or
        "in launch, head loads" (last_head_path)."""
        route = {_abi.ROUNDS_IN_LAUNCH: "in launch", _abi.ROUNDS_LAUNCH_PER_ROUND: "launch per round",
                 _abi.ROUNDS_LANES: "lanes", _abi.ROUNDS_APT_LANES: "apt lanes", _abi.ROUNDS_WAVES: "waves",
                 _abi.ROUNDS_WAVES_LONG: "waves long"}.get(self._L.nlmc_pt_rounds_route(self._ctx))
        if heads and route in ("in launch", "launch per round") and self.last_head_path() and self._last_fused():
            route += ", head " + self.last_head_path()
        return route

    def last_head_path(self):
        """Where the most recent launch on fused windows read its item heads: "stream" (the plan's head stream: an instance without a
        field term, no per-sweep outputs), "loads" (a load per level), or None before any such launch (include/nlmc.h:
        nlmc_last_head_path; NLMC_NO_HEAD_STREAM=1 at creation keeps the loads)."""
        return {_abi.HEADS_LOADS: "loads", _abi.HEADS_STREAM: "stream"}.get(self._L.nlmc_last_head_path(self._ctx))

    def pt_log_begin(self, round0, n_rounds, n_pairs):
        """Keep the swap log of the next rounds on the device (rounds called with want_log=False)."""
        self._ck(self._L.nlmc_pt_log_begin(self._ctx, int(round0), int(n_rounds), int(n_pairs)))
        self._pt_log_shape = (int(n_rounds), self.n_chains_global // self.ladder_len, int(n_pairs))

    def pt_log_read(self):
        r, nl, p = self._pt_log_shape
        pairs, acc = np.empty((r, nl, p, 2), np.int32), np.empty((r, nl, p), np.uint8)
        if r * nl * p:
            self._ck(self._L.nlmc_pt_log_read(self._ctx, _abi.ptr(pairs), _abi.ptr(acc)))
        return pairs, acc

    def pt_check(self):
        """ValueError("Cannot find non-overlapping pairs.") if a device-decided swap round ran out of pairs (NPT/npt.py:526)."""
        self._ck(self._L.nlmc_pt_check(self._ctx))

    # -- rounds whose marked temperature slots run NMC cycles (include/nlmc.h) -----------------------------
    def mark_slots(self, marks):
        m = None if marks is None else _abi.as_c(np.asarray(marks).astype(bool), np.uint8).reshape(self.ladder_len)
        self._ck(self._L.nlmc_pt_mark_slots(self._ctx, _abi.ptr(m)))

    def select(self, which):
        """Later sweep_philox / adopt_best / backbone_clusters / set_phase calls act on: "all" chains, or the local chains
        currently on "unmarked" / "marked" temperature slots."""
        w = {"all": _abi.CHAINS_ALL, "unmarked": _abi.CHAINS_UNMARKED, "marked": _abi.CHAINS_MARKED}[which]
        self._ck(self._L.nlmc_select_chains(self._ctx, w))

    def overlap_subsets(self, on=True):
        """Queue the marked subset's work on a second stream beside the unmarked chains' sweeps (nlmc_overlap_subsets)."""
        self._ck(self._L.nlmc_overlap_subsets(self._ctx, int(bool(on))))

    def subset(self):
        out = np.empty(self.rows(), dtype=np.int32)
        self._ck(self._L.nlmc_get_subset(self._ctx, _abi.ptr(out)))
        return out

    def track_minimum(self, on=True, stride=1):
        """Sweep calls keep the running minimum + argmin state on the device; `stride` > 1: over sweeps 0, stride, 2 stride, ... only."""
        self._ck(self._L.nlmc_track_minimum(self._ctx, (max(1, int(stride)) if on else 0)))

    # -- run-long best-state record (include/nlmc.h: nlmc_best_begin) -------------------------------------------------------
    def best_begin(self, target=None):
        """Open (or reset) the record of every chain's lowest-energy state.  target: energy whose first passage is stamped
        (None: no first-passage stamp).  While it is open pt_rounds_fused / pt_rounds_deferred / pt_rounds_lanes observe every
        chain once per round (stamp = round index); round-by-round drivers call best_update."""
        self._ck(self._L.nlmc_best_begin(self._ctx, float("nan") if target is None else float(target)))

    def best_update(self, stamp):
        """One observation of every local chain's current state (asynchronous; all chains must be selected)."""
        self._ck(self._L.nlmc_best_update(self._ctx, int(stamp) & 0xFFFFFFFF))

    def best_read(self, want_state=True):
        """dict(energy [n_chains] as energy_tracked reports (+inf: never observed), stamp [n_chains] of the first attainment,
        first_hit [n_chains] (-1: the target was never reached), state [n_chains, n] int8 or None)."""
        e = np.empty(self.n_chains, np.float64)
        st, fh = np.empty(self.n_chains, np.int32), np.empty(self.n_chains, np.int32)
        s = np.empty((self.n_chains, self.n), np.int8) if want_state else None
        self._ck(self._L.nlmc_best_read(self._ctx, _abi.ptr(e), _abi.ptr(st), _abi.ptr(fh), _abi.ptr(s)))
        return {"energy": e, "stamp": st, "first_hit": fh, "state": s}

    def best_end(self):
        """Close the record (best_read still returns it); the rounds routes behave as before."""
        self._ck(self._L.nlmc_best_end(self._ctx))

    # -- run-long per-round energy log (include/nlmc.h: nlmc_elog_begin) -----------------------------------------------------
    def elog_begin(self, round0, n_rounds):
        """Open (or reset) the log of rounds [round0, round0 + n_rounds): per round and local chain the tracked energy and the
        temperature slot as that round's swap decision sees them.  While it is open pt_rounds_fused / pt_rounds_deferred /
        pt_rounds_lanes / apt_rounds_lanes observe every chain once per round; round-by-round drivers call elog_update between the
        last state-changing step and the swap.  Rounds outside the window are not logged.  After pt_init; NotImplementedError for a
        context with a communicator or a cut ladder."""
        self._ck(self._L.nlmc_elog_begin(self._ctx, int(round0) & 0xFFFFFFFF, int(n_rounds)))
        self._elog_rounds = int(n_rounds)

    def elog_update(self, round_idx):
        """One observation of every local chain's tracked energy and slot as round `round_idx` (asynchronous; all chains must be
        selected).  A second observation of a round overwrites the first."""
        self._ck(self._L.nlmc_elog_update(self._ctx, int(round_idx) & 0xFFFFFFFF))

    def elog_read(self, by="chain"):
        """by="chain": (energy [n_rounds, n_chains] float64, slot [n_rounds, n_chains] int32) by local chain; a row no observation
        reached reads NaN / -1.  by="slot": (energy [n_rounds, n_ladders, L], chain [n_rounds, n_ladders, L]) -- the energy on every
        temperature slot of every local ladder and the local chain that held the slot.  One synchronisation; also after elog_end."""
        if by not in ("chain", "slot"):
            raise ValueError('elog_read: by must be "chain" or "slot"')
        R = getattr(self, "_elog_rounds", None)
        if R is None:
            raise RuntimeError("elog_read: no log was begun (elog_begin)")
        e, s = np.empty((R, self.n_chains), np.float64), np.empty((R, self.n_chains), np.int32)
        if e.size:
            self._ck(self._L.nlmc_elog_read(self._ctx, _abi.ptr(e), _abi.ptr(s)))
        if by == "chain":
            return e, s
        from .hostlogic import log_by_slot
        return log_by_slot(e, s, self.ladder_len)

    def elog_end(self):
        """Close the log (elog_read still returns it); the rounds routes behave as before."""
        self._ck(self._L.nlmc_elog_end(self._ctx))

    def backbone_seed(self, snapshot=True):
        """snapshot=True: later backbone_clusters calls are seeded with the configurations as they are NOW; False: with the current ones."""
        self._ck(self._L.nlmc_backbone_seed(self._ctx, 1 if snapshot else 0))

    def adopt_best(self):
        self._ck(self._L.nlmc_adopt_best(self._ctx))

    def backbone_clusters(self, epsilon, lambdas, beta, tolerance, max_iterations, sat, thresholds):
        eps = _abi.as_c(epsilon, np.float64).reshape(self.n)
        lam = _abi.as_c(lambdas, np.float64).reshape(-1)
        thr = _abi.as_c(thresholds, np.float64).reshape(-1)
        self._ck(self._L.nlmc_backbone_clusters(self._ctx, _abi.ptr(eps), _abi.ptr(lam), lam.shape[0], float(beta), float(tolerance),
                                                int(max_iterations), float(sat), _abi.ptr(thr), thr.shape[0]))

    def backbone_check(self):
        self._ck(self._L.nlmc_backbone_check(self._ctx))

    def cluster_mask(self):
        out = np.empty((self.n_chains, self.n), dtype=np.uint8)
        self._ck(self._L.nlmc_get_cluster_mask(self._ctx, _abi.ptr(out)))
        return out

    def set_cluster_mask(self, mask):
        m = _abi.as_c(np.asarray(mask).astype(bool), np.uint8).reshape(self.n_chains, self.n)
        self._ck(self._L.nlmc_set_cluster_mask(self._ctx, _abi.ptr(m)))

    def set_phase(self, kind, temp_x=1.0):
        k = {"ALL": _abi.PHASE_ALL, "C": _abi.PHASE_BACKBONE_HOT, "NC": _abi.PHASE_BACKBONE_FROZEN}[kind]
        self._ck(self._L.nlmc_set_phase(self._ctx, k, float(temp_x)))
        self._flags_on = kind != "ALL"

    PHASES = {"ALL": _abi.PHASE_ALL, "C": _abi.PHASE_BACKBONE_HOT, "NC": _abi.PHASE_BACKBONE_FROZEN}

    def nmc_phases_lanes(self, kinds, sweeps_per_phase, seed, sweep0, beta, temp_x, min_stride=1, precision="f32",
                         want_minima=False, want_last_best=False):
        """All phases `kinds` ("C" / "NC" / "ALL") of an NMC cycle of the selected chains inside k_nmc_phases_lanes launches, a chain
        per lane (include/nlmc.h: nlmc_nmc_phases_lanes): per phase adopt_best (from the second on), set_phase(kind, temp_x) and
        sweep_philox(sweeps_per_phase, seed, sweep0 + p * sweeps_per_phase, beta) under track_minimum(True, min_stride) -- same bits
        as that call sequence, in one launch per call (or per chunk of phases the order scratch holds).  The backbone masks are those of
        the last backbone_clusters / set_cluster_mask; track_minimum must be off; set_phase's setting is left alone.  Returns None, or
        with want_minima / want_last_best (read-backs: they synchronise the stream) a dict: phase_min [rows, P] float64 as
        energy_tracked reports and phase_argmin [rows, P] int32 (sweep within the phase), last_best [rows, n] int8.
        NotImplementedError when the context does not qualify (nothing was run; nmc_phases_lanes_refusal asks beforehand)."""
        return self._nmc_phases(self._L.nlmc_nmc_phases_lanes, kinds, sweeps_per_phase, seed, sweep0, beta, temp_x, min_stride, precision,
                                want_minima, want_last_best)

    def _nmc_phases(self, call, kinds, sweeps_per_phase, seed, sweep0, beta, temp_x, min_stride, precision, want_minima, want_last_best):
        """nmc_phases_lanes / nmc_phases_waves / nmc_phases_waves_long: the library call `call` and its read-backs."""
        k = _abi.as_c([self.PHASES[x] for x in kinds], np.int32)
        R, P = self.rows(), int(k.shape[0])
        pmin = np.empty((R, P), np.int64) if want_minima else None
        parg = np.empty((R, P), np.int32) if want_minima else None
        best = np.empty((R, self.n), np.int8) if want_last_best else None
        self._ck(call(self._ctx, _precision(precision), _abi.ptr(k), P, int(sweeps_per_phase), int(sweep0) & 0xFFFFFFFF, int(seed),
                      float(beta), float(temp_x), int(min_stride), _abi.ptr(pmin), _abi.ptr(parg), _abi.ptr(best)))
        if not (want_minima or want_last_best):
            return None
        return {"phase_min": None if pmin is None else pmin.astype(np.float64) * 2.0 ** -self.energy_scale,
                "phase_argmin": parg, "last_best": best}

    def _nmc_refusal(self, route, S):
        """nmc_phases_<route>_refusal: the library's reason, or None."""
        why = getattr(self._L, f"nlmc_nmc_phases_{route}_refusal")(self._ctx, int(S))
        return why.decode() if why else None

    def nmc_phases_lanes_refusal(self, sweeps_per_phase):
        """Why nmc_phases_lanes would refuse phases of `sweeps_per_phase` sweeps on this context (the library's reason), or None."""
        return self._nmc_refusal("lanes", sweeps_per_phase)

    def nmc_phases_waves(self, kinds, sweeps_per_phase, seed, sweep0, beta, temp_x, min_stride=1, precision="f32",
                         want_minima=False, want_last_best=False):
        """nmc_phases_lanes' call inside k_nmc_phases_waves launches, a chain per wave in the wave sweeps' launch shape
        (include/nlmc.h: nlmc_nmc_phases_waves): spins, mask, the exact local fields and the best state's fields stay in registers
        across the phases, so the hand-off between two phases is a register copy.  Same arguments, same returns, same bits as the
        call sequence on any route; reached by name (set_wave_sweeps is not looked at).  NotImplementedError when the context does not
        qualify -- chains of more than 256 spins (with set_wave_long too), precision "f64", apt_shard contexts, ... -- and nothing
        was run; nmc_phases_waves_refusal asks beforehand."""
        return self._nmc_phases(self._L.nlmc_nmc_phases_waves, kinds, sweeps_per_phase, seed, sweep0, beta, temp_x, min_stride, precision,
                                want_minima, want_last_best)

    def nmc_phases_waves_refusal(self, sweeps_per_phase):
        """Why nmc_phases_waves would refuse f32 phases of `sweeps_per_phase` sweeps on this context (the library's reason), or None."""
        return self._nmc_refusal("waves", sweeps_per_phase)

    def nmc_phases_waves_long(self, kinds, sweeps_per_phase, seed, sweep0, beta, temp_x, min_stride=1, precision="f32",
                              want_minima=False, want_last_best=False):
        """nmc_phases_waves' call for dense chains of 257 to 1024 spins, inside k_nmc_phases_waves_long launches in the long wave sweeps'
        launch shape (include/nlmc.h: nlmc_nmc_phases_waves_long): the exact local fields stay resident across the phases (registers
        plus the wave's LDS copy), the best state's fields in registers and its spins in the wave's LDS, so the fields are built once
        per launch and the hand-off between two phases stays inside the wave.  Same arguments, same returns, same bits as the call
        sequence on any route; reached by name (set_wave_sweeps / set_wave_long are not looked at).  NotImplementedError when the
        context does not qualify -- chains of at most 256 or more than 1024 spins, precision "f64", apt_shard contexts, ... -- and
        nothing was run; nmc_phases_waves_long_refusal asks beforehand."""
        return self._nmc_phases(self._L.nlmc_nmc_phases_waves_long, kinds, sweeps_per_phase, seed, sweep0, beta, temp_x, min_stride,
                                precision, want_minima, want_last_best)

    def nmc_phases_waves_long_refusal(self, sweeps_per_phase):
        """Why nmc_phases_waves_long would refuse f32 phases of `sweeps_per_phase` sweeps on this context (the library's reason), or
        None."""
        return self._nmc_refusal("waves_long", sweeps_per_phase)

    # -- iso-cluster move -------------------------------------------------------------------------------
    def icm_components(self, chain_a, chain_b):
        out = ctypes.c_int32(0)
        self._ck(self._L.nlmc_icm_components(self._ctx, int(chain_a), int(chain_b), ctypes.byref(out)))
        return int(out.value)

    def icm_move(self, chain_a, chain_b, pick_index, katzgraber=True):
        info = np.zeros(2, np.int32)
        self._ck(self._L.nlmc_icm_move(self._ctx, int(chain_a), int(chain_b), int(pick_index), int(bool(katzgraber)),
                                       _abi.ptr(info)))
        return int(info[0]), int(info[1])

    def icm_labels(self):
        out = np.empty(self.n, dtype=np.int32)
        self._ck(self._L.nlmc_icm_get_labels(self._ctx, _abi.ptr(out)))
        return out

    def icm_round_philox(self, pairs, round_idx, seed, katzgraber=True, want_info=False):
        p = _abi.as_c(pairs, np.int32).reshape(-1, 2)
        info = np.zeros((p.shape[0], 2), np.int32) if want_info else None
        self._ck(self._L.nlmc_icm_round_philox(self._ctx, _abi.ptr(p), p.shape[0], int(round_idx), int(seed),
                                               int(bool(katzgraber)), _abi.ptr(info)))
        return info

    def icm_round_ladders(self, round_idx, seed, katzgraber=True, want_info=False):
        """Houdayer step of one APT round with the pairing decided on the device (include/nlmc.h); info [M * L * (K // 2), 2] in the
        order (system, slot, pair) under apt_systems(M), K the ladders of one system."""
        npairs = ctypes.c_int32(0)
        info = np.zeros((self._icm_rows(), 2), np.int32) if want_info else None
        self._ck(self._L.nlmc_icm_round_ladders(self._ctx, int(round_idx), int(seed), int(bool(katzgraber)),
                                                ctypes.byref(npairs), _abi.ptr(info)))
        return info

    # -- backbone inference (loopy BP on the device) -------------------------------------------------------
    def lbp_convexified(self, m_star, epsilon, lambdas, beta, tolerance, max_iterations, sat, want_all=False):
        """Batched lambda loop of LBP_convexified (include/nlmc.h: nlmc_lbp_convexified).  m_star [P, n] float64.
        Returns dict(mag [P, n], n_lambdas [P], iters [P, L], status [P], mag_all [P, L, n] or None)."""
        ms = _abi.as_c(np.atleast_2d(m_star), np.float64)
        P, L = ms.shape[0], len(lambdas)
        if ms.shape[1] != self.n:
            raise ValueError("m_star must be [n_problems, n]")
        eps = _abi.as_c(epsilon, np.float64).reshape(-1)
        lam = _abi.as_c(lambdas, np.float64).reshape(-1)
        mag = np.zeros((P, self.n))
        mag_all = np.zeros((P, L, self.n)) if want_all else None
        nl, it, st = np.zeros(P, np.int32), np.zeros((P, L), np.int32), np.zeros(P, np.int32)
        self._ck(self._L.nlmc_lbp_convexified(self._ctx, P, _abi.ptr(ms), _abi.ptr(eps), _abi.ptr(lam), L, float(beta),
                                              float(tolerance), int(max_iterations), float(sat), _abi.ptr(mag),
                                              _abi.ptr(mag_all), _abi.ptr(nl), _abi.ptr(it), _abi.ptr(st)))
        return {"mag": mag, "n_lambdas": nl, "iters": it, "status": st, "mag_all": mag_all}

    # -- measurement ------------------------------------------------------------------------------------
    def last_timing(self):
        a, b, c = ctypes.c_float(0), ctypes.c_float(0), ctypes.c_int32(0)
        self._ck(self._L.nlmc_last_timing(self._ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"ms_levelize": a.value, "ms_sweep": b.value, "launches_sweep": c.value}

    def timing_reset(self, enable=True, every=1):
        """Accumulate HIP-event timings of the sweep calls from now on (`every` > 1: events around every `every`-th
        fused-window launch only), or stop accumulating."""
        self._ck(self._L.nlmc_timing_reset(self._ctx, max(1, int(every)) if enable else 0))

    def timing_total(self):
        a, b, c, d = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._ck(self._L.nlmc_timing_total(self._ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
        return {"ms_levelize": a.value, "ms_sweep": b.value, "launches_sweep": c.value, "launches_timed": d.value}

    def probe_level_round(self, waves=16, conflict_free=True, rounds=20000, n_workgroups=256):
        """ns per level-synchronous round (barrier + 8 LDS byte gathers + write) on this device (nlmc_probe_level_round)."""
        out = ctypes.c_double(0)
        self._ck(self._L.nlmc_probe_level_round(self._ctx, int(waves), int(bool(conflict_free)), int(rounds), int(n_workgroups),
                                                ctypes.byref(out)))
        return out.value

    def last_schedule_stats(self):
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        self._ck(self._L.nlmc_last_schedule_stats(self._ctx, ctypes.byref(a), ctypes.byref(b)))
        return {"orders": a.value, "levels": b.value}


def trace_layout(spins, dst_block=None, n_dst_blocks=None, dtype=np.float64, n_threads=0, dst_col=None, row_len=None,
                 out=None):
    """Recorded traces [blocks, S, N] int8 -> the reference's M layout [n_dst_blocks * N, row_len] (`M[r*N:(r+1)*N, :] =
    MCMC(...)`, NPT/npt.py:641; NPT/apt_ICM.py:207 with a column group per sub-replica): block b goes to the rows of block
    dst_block[b], columns dst_col[b] .. dst_col[b]+S-1; int8 or float64; compiled host routine (nlmc_trace_layout), one
    thread per core.  `out`: write into this C-contiguous [n_dst_blocks * N, row_len] array instead of a new one."""
    spins = np.ascontiguousarray(spins, dtype=np.int8)
    B, S, N = spins.shape
    nd = B if n_dst_blocks is None else int(n_dst_blocks)
    rl = S if row_len is None else int(row_len)
    dt = np.dtype(dtype) if out is None else out.dtype
    if dt not in (np.dtype(np.int8), np.dtype(np.float64)):
        raise ValueError("trace_layout: dtype must be int8 or float64")
    db = None if dst_block is None else np.ascontiguousarray(dst_block, dtype=np.int32)
    dc = None if dst_col is None else np.ascontiguousarray(dst_col, dtype=np.int32)
    for x in (db, dc):
        if x is not None and x.shape != (B,):
            raise ValueError("trace_layout: dst_block / dst_col must have one entry per block")
    if out is not None:
        if out.shape != (nd * N, rl) or not out.flags["C_CONTIGUOUS"] or not out.flags["WRITEABLE"]:
            raise ValueError("trace_layout: out must be a writeable C-contiguous [n_dst_blocks * N, row_len] array")
        M = out
    else:
        full = B * S == nd * rl                  # distinct destinations (checked by the routine) then cover all of M
        M = np.empty((nd * N, rl), dtype=dt) if full else np.zeros((nd * N, rl), dtype=dt)
    _abi.check(_abi.lib().nlmc_trace_layout(_abi.ptr(spins), B, S, N, _abi.ptr(db), _abi.ptr(dc), nd, rl, _abi.ptr(M),
                                            dt.itemsize, int(n_threads)), None)
    return M


def _stitch_outputs(outs, chunk, record_stride, want_energy, want_min, want_state):
    """Outputs of consecutive pieces of one logical sweep call (pieces of `chunk` sweeps) -> what one call would return."""
    R = outs[0]["spins"].shape[0] if record_stride else (outs[0]["energy"].shape[0] if want_energy else len(outs[0]["min_energy"]))
    o = {"spins": np.concatenate([p["spins"] for p in outs], axis=1) if record_stride else None,
         "energy": np.concatenate([p["energy"] for p in outs], axis=1) if want_energy else None,
         "min_energy": None, "argmin": None, "argmin_state": None}
    if want_min:
        mins = np.stack([p["min_energy"] for p in outs])           # [pieces, R]
        first = np.argmin(mins, axis=0)                            # np.argmin: first piece holding the minimum
        o["min_energy"] = mins[first, np.arange(R)]
        o["argmin"] = np.array([outs[first[r]]["argmin"][r] + first[r] * chunk for r in range(R)], dtype=np.int32)
        if want_state:
            o["argmin_state"] = np.stack([outs[first[r]]["argmin_state"][r] for r in range(R)])
    return o


def prefault_async(arr, n_threads=0):
    """Touch every page of a freshly allocated array from a background thread (nlmc_host_prefault; the call releases the GIL).
    Returns the thread: join() it before the array is filled."""
    import threading
    a = arr
    t = threading.Thread(target=lambda: _abi.lib().nlmc_host_prefault(_abi.ptr(a), int(a.nbytes), int(n_threads)), daemon=True)
    t.start()
    return t


def device_count():
    return int(_abi.lib().nlmc_device_count())


def fused_plan_bytes(n, n_long, window, value_plane=False):
    """Upper estimate of the device memory one planned window of `window` sweeps takes (head 8 + row planes <= 64 + item ids
    4 bytes per schedule position, 2 bytes per update of level scratch): what nlmc_plan_philox_fused allocates per window
    (csrc/nlmc.hip: reserve_fused_plan, fused_pstride).  n_long: positions a sweep takes beyond one per row -- one more for a
    row longer than 8 entries (a lane pair), three more for one longer than 16 (a lane quad).
    value_plane: plans of the real-valued fp64 variant (Engine.set_fused_f64_real) add 9 doubles per position."""
    pstride = -(-int(window) * (int(n) + int(n_long)) // 64) * 64 + 64 * 1024
    return pstride * (76 + (72 if value_plane else 0)) + int(window) * int(n) * 2 + 8192


def sweeps_per_plan_piece(bytes_per_window, n_sweeps, window, budget_bytes, record_stride=0):
    """Sweeps one piece of Engine.sweep_philox_windows covers: as many whole windows as fit the budget (at least one),
    starting on a recorded sweep when configurations are recorded with a stride."""
    per_piece = max(1, int(budget_bytes) // int(bytes_per_window)) * int(window)
    if record_stride > 1:
        L = int(np.lcm(int(window), int(record_stride)))
        per_piece = per_piece // L * L or int(n_sweeps)
    return min(per_piece, int(n_sweeps))


def fused_window(n_sweeps, lo=3, hi=64):
    """Largest divisor of n_sweeps in [lo, hi] (the launch length of the fused-window schedule), or 0."""
    for t in range(min(hi, n_sweeps), lo - 1, -1):
        if n_sweeps % t == 0:
            return t
    return 0


# Whether APT_ICM(lanes=...) hands its rounds to Engine.apt_rounds_lanes where the engine's sweeps go to the lane kernels.  The rule is
# that of ROUNDS_LANES_IN_LAUNCH (csrc/nlmc.hip): True only if the in-launch median time per run is not above that of lane sweeps
# round by round on the same build by more than the run-to-run spread at any shape of scripts/apt_lanes_throughput.py.  Measured
# (profiles/apt_lanes_throughput.txt): above it at 69 of 72 shapes, 1.1-1.2x at T = 1 on n = 10 up to 7-10x on n = 40
# and Chimera-128.  So the class keeps a call per step, and Engine.apt_rounds_lanes reaches the kernel by name.
APT_LANES_IN_LAUNCH = False

# What the documents recommend for wave_rounds where the wave sweeps are on (the default of every wave_rounds keyword stays False
# whatever this says; nothing in the package reads it).  The rule is that of ROUNDS_LANES_IN_LAUNCH: True only if the in-launch median
# time per run is not above that of wave sweeps round by round on the same build by more than the run-to-run spread at any shape of
# scripts/wave_rounds_throughput.py.  Measured (profiles/wave_rounds_in_launch_throughput.txt): below it at every
# shape with T = 1 and L = 16 (1.3-2.7x), level at T = 10, but above it at T = 1000 with 64 ladders of 16 (1.2-1.35x: a ladder per
# workgroup leaves three quarters of the compute units idle) and at every shape with L = 64 (1.2-5.3x: four chains a wave, in turn).
WAVE_ROUNDS_IN_LAUNCH = False

# What the documents recommend for wave_long_rounds where wave_rounds and wave_long are on (the default of every wave_long_rounds
# keyword stays False whatever this says; nothing in the package reads it).  The same rule: True only if the in-launch median time per
# run is not above that of a sweep call and a swap call per round on the same build (set_wave_long_rounds(False)) by more than the
# run-to-run spread at any shape of scripts/wave_long_rounds_throughput.py.  Measured (DESIGN.md section 6,
# profiles/wave_long_rounds_throughput.txt): below it at every shape with T = 1 and at most 16 temperatures (1.2-4.9x), and 2.0-2.4x
# below it at every T on 256 ladders of 16 at n = 1024 (4096 chains: call by call runs 15 chains a workgroup, more workgroups than
# compute units), but above it at T >= 10 on 16 ladders (up to 1.4x: a ladder per workgroup uses 16 of the compute units, sixteen waves
# each, where call by call spreads the chains a wave per compute unit) and at every T on 16 ladders of 32 (1.5-2.6x: two chains a wave,
# in turn).  Recommended: a swap every sweep or two, or at least as many ladders as compute units, with L <= 16.
WAVE_LONG_ROUNDS_IN_LAUNCH = False


class RoundPlanner:
    """Level schedules planned ahead for `n_rounds` rounds of `sweeps_per_round` sweeps each (they depend on the RNG
    only), a bounded number of rounds at a time.  Rounds whose sweeps need no per-sweep output run on the fused-window
    schedule when the instance qualifies (one or more launches of `window` sweeps), everything else on the
    sweep-by-sweep schedule; the results are the same bits either way.  With `pt_pairs` > 0 the pair selections of the
    swap rounds `pt_round0 + ii` (they depend on the RNG only, too) are planned with every chunk.  The planner is also the one place
    that says which route its rounds take (route) and whether a chunk of them may go to the engine's batched rounds call (batchable,
    rounds_ready); its planned ranges are private."""

    BYTES_PER_UPDATE = 140              # packed schedule: head 8 + row window 128 + scratch

    def __init__(self, eng, sweep0, n_rounds, sweeps_per_round, seed, precision="f32", budget_bytes=1 << 30,
                 chunk_rounds=None, pt_pairs=0, pt_round0=0, slot=0, beta=None, fused_outputs=False):
        """`slot`: fused-plan slot of the engine this planner owns; `beta`: None = the ladder temperatures, or one inverse
        temperature for every chain; `fused_outputs`: rounds with per-sweep outputs also run on fused windows (the
        output variant of the kernel) when the plan covers them."""
        self.eng, self.sweep0, self.R, self.S, self.seed, self.precision = eng, int(sweep0), int(n_rounds), int(sweeps_per_round), int(seed), precision
        self.slot, self.beta, self.fused_outputs = int(slot), beta, bool(fused_outputs)
        self.window = fused_window(self.S)
        if self.window and precision != "f32" and (not hasattr(eng, "fused_modes") or precision not in eng.fused_modes(self.window)):
            self.window = 0              # fp64 mode: fused windows only where the field is an exact integer (nlmc_fused_modes)
        per_round = max(1, self.S * eng.n * self.BYTES_PER_UPDATE)
        self.chunk = max(1, min(self.R, int(budget_bytes // per_round)))
        if chunk_rounds:
            self.chunk = max(1, min(self.chunk, int(chunk_rounds)))
        self.pt_pairs, self.pt_round0 = int(pt_pairs), int(pt_round0)
        # planned round ranges [from, to): fused windows, the sweep-by-sweep schedule, and -- on the short-chain routes, which need no
        # level schedule -- the pair selections alone
        self._fused = self._plain = self._pairs = (0, 0)
        self.chunks_planned = 0

    SHORT_CHAIN = ("lanes", "wave rounds", "waves")

    def route(self):
        """The route this planner's rounds take, decided here and nowhere else: "lanes" (the engine runs the sweeps one chain per lane,
        Engine.lanes_take), "wave rounds" (one chain per wave, Engine.waves_take, with the engine's wave_rounds on), "waves" (one chain
        per wave, round by round through the sweep calls), "windows" (fused windows of `window` sweeps) or "plain" (the sweep-by-sweep
        schedule; also what "windows" becomes once the engine has turned a window plan down).  The three short-chain routes need no
        level schedule: a chunk is planned once its pair selections are."""
        e = self.eng
        if hasattr(e, "lanes_take") and e.lanes_take():
            return "lanes"
        if hasattr(e, "waves_take") and e.waves_take(precision=self.precision):
            return "wave rounds" if getattr(e, "wave_rounds", False) else "waves"
        return "windows" if self.window else "plain"

    def _batchable(self, route, n_sweeps, by_name):
        if int(n_sweeps) != self.S:
            return False
        return (route == "windows" and self.window == self.S) or (not by_name and route in ("lanes", "wave rounds"))

    def batchable(self, n_sweeps, by_name=False):
        """Whether a chunk of rounds of `n_sweeps` sweeps may go to the engine's batched rounds call (Engine.pt_rounds_deferred): rounds
        of the planned length on one fused window each, or on a short-chain route the engine runs whole rounds on (k_rounds_lanes,
        k_rounds_waves).  `by_name`: the caller asks for Engine.pt_rounds_fused, which takes the fused-window route only."""
        return self._batchable(self.route(), n_sweeps, by_name)

    def _planned(self, ii, route):
        a, b = self._pairs if route in self.SHORT_CHAIN else self._fused if route == "windows" else self._plain
        return a <= ii < b

    def rounds_ready(self, ii, by_name=False):
        """Plan the chunk that holds round ii unless it is planned, and return how many rounds from ii on are ready for the batched
        rounds call: 0 when the planner's rounds are not batchable(), when ii lies outside the planned rounds, and once the engine has
        turned fused windows down."""
        route = self.route()
        if not (0 <= ii < self.R) or not self._batchable(route, self.S, by_name):
            return 0
        if not self._planned(ii, route):
            self._plan(ii, route)
        return (self._pairs if route in self.SHORT_CHAIN else self._fused)[1] - ii if self._planned(ii, route) else 0

    def prepare(self, ii):
        """Plan the chunk that starts at round ii unless round ii is planned: its pair selections and the level schedules the route
        needs -- none on a short-chain route; fused windows on "windows", and if the engine turns them down the sweep-by-sweep
        schedule, now and from then on; the sweep-by-sweep schedule on "plain"."""
        route = self.route()
        if not self._planned(ii, route):
            self._plan(ii, route)

    def fused_covers(self, ii):
        """Whether fused windows are planned for round ii."""
        return self._fused[0] <= ii < self._fused[1]

    def drop_windows(self):
        """The planned fused windows are gone (another planning call wrote to the engine's plan slot)."""
        self._fused = (0, 0)

    def _plan(self, ii, route):
        r0, r1 = ii, min(self.R, ii + self.chunk)
        self.chunks_planned += 1
        if self.pt_pairs > 0 and hasattr(self.eng, "pt_plan"):
            self.eng.pt_plan(self.pt_round0 + r0, r1 - r0, self.seed, self.pt_pairs)
        if route in self.SHORT_CHAIN:    # a chain per lane or per wave: nothing to plan but the chunk's pair selections
            self._pairs = (r0, r1)
            return
        if route == "windows":
            if hasattr(self.eng, "plan_slot"):
                self.eng.plan_slot(self.slot)
            k = self.eng.plan_philox_fused(self.sweep0 + r0 * self.S, (r1 - r0) * (self.S // self.window), self.window, self.seed)
            if k == (r1 - r0) * (self.S // self.window):
                self._fused = (r0, r1)
                return
            self.window = 0              # the instance does not qualify: stop asking
        self.eng.plan_philox(self.sweep0 + r0 * self.S, (r1 - r0) * self.S, self.seed, precision=self.precision)
        self._plain = (r0, r1)

    def sweep(self, ii, **outputs):
        """The sweeps of round ii at the PT ladder temperatures.  `outputs`: record_stride / want_* of sweep_philox."""
        needs_plain = bool(outputs) and not self.fused_outputs and any(outputs.get(k) for k in ("record_stride", "want_energy", "want_min", "want_state"))
        if self.S == 0:
            return self.eng.sweep_philox(0, self.seed, sweep0=self.sweep0, beta=self.beta, precision=self.precision, **outputs)
        route = self.route()
        if (not needs_plain or route in self.SHORT_CHAIN) and not self._planned(ii, route):
            self._plan(ii, route)
        # (a round with outputs outside the planned range builds its schedule inside the call; one call either way: on fused windows
        # the library walks the windows of the round)
        return self.eng.sweep_philox(self.S, self.seed, sweep0=self.sweep0 + ii * self.S, beta=self.beta, precision=self.precision,
                                     **outputs)
