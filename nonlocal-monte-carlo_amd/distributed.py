"""Replica-sharded parallel tempering across the GPUs of one node: one process per GPU (`torch.distributed`,
backend "nccl" = RCCL over xGMI; "gloo" for CPU rehearsal with an injected engine).

Sharding: the global set of chains is cut into contiguous blocks, one per rank; a swap round
needs only the scalar energies, so the single collective is ONE all-gather of `n_local` float64 per rank and round.
Every rank then evaluates the identical Philox-keyed swap decision on the full energy vector and updates its replica of
the (tiny) slot table -- swaps are label exchanges, no configuration ever crosses a link.  Because every random
number is a pure function of (seed, global chain id, sweep, spin), the trajectory is bit-identical for any number
of ranks.
"""
import collections
import os
import sys

import numpy as np

from . import hostlogic
from .engine import Engine, RoundPlanner


# Sweep indices (Philox counters) of the NMC phases that marked slots run inside a round: a range of their own, disjoint from the
# plain sweeps' whatever the number of rounds -- so rounds driven with and without a plan draw the same numbers (the
# unplanned fallback used to reuse the next round's plain indices).
NMC_SWEEP_SPACE = 1 << 31

# Whether LocalTempering runs the NMC phases of a round without outputs inside one k_nmc_phases_lanes launch per context
# (Engine.nmc_phases_lanes) where the engine takes them, when the caller does not say (lane_nmc=None).  Set from
# scripts/lane_nmc_throughput.py (profiles/lane_nmc_throughput.txt).
LANE_NMC_IN_LAUNCH = True

# The same for one k_nmc_phases_waves launch per context (Engine.nmc_phases_waves) where the engine's sweeps run one chain per wave
# (wave_nmc=None).  Set from scripts/wave_nmc_throughput.py (profiles/wave_nmc_throughput.txt).
WAVE_NMC_IN_LAUNCH = True

# The same for one k_nmc_phases_waves_long launch per context (Engine.nmc_phases_waves_long) where the engine's sweeps run one chain
# of 257 to 1024 spins per wave (wave_long_nmc=None).  Set from scripts/wave_long_nmc_throughput.py (DESIGN.md section 6,
# profiles/wave_long_nmc_throughput.txt).
WAVE_LONG_NMC_IN_LAUNCH = True

# The one-launch NMC routes in the order a round asks them (the wave calls first, as the wave route is asked before the lane route): per
# route the engine call (`call`, with `call` + "_refusal" beside it), LocalTempering's option keyword, the module constant above that is
# the option's default (read when a LocalTempering is made) and the Engine method that says whether the context's sweeps take that route
# anyway.
NmcRouteSpec = collections.namedtuple("NmcRouteSpec", "call option default take")
NMC_ROUTES = {"waves": NmcRouteSpec("nmc_phases_waves", "wave_nmc", "WAVE_NMC_IN_LAUNCH", "waves_take"),
              "waves_long": NmcRouteSpec("nmc_phases_waves_long", "wave_long_nmc", "WAVE_LONG_NMC_IN_LAUNCH", "waves_take"),
              "lanes": NmcRouteSpec("nmc_phases_lanes", "lane_nmc", "LANE_NMC_IN_LAUNCH", "lanes_take")}


class NmcRouteState:
    """What a LocalTempering keeps per route of NMC_ROUTES: the option (`on`; `by_default`: left to the module constant, and then applied
    only where the context's sweeps take the route anyway), the contexts (by index) whose engine was `asked` and those whose engine
    `refused`, and the counters: `rounds` in which every context took the call, `calls` that ran."""

    def __init__(self, option, default):
        self.on, self.by_default = (default if option is None else bool(option)), option is None
        self.refused, self.asked = set(), set()
        self.rounds = self.calls = 0


def block_partition(n_global, world, rank):
    """Contiguous block of chains owned by `rank` (first `n_global % world` ranks get one extra)."""
    q, r = divmod(int(n_global), int(world))
    count = q + (1 if rank < r else 0)
    base = rank * q + min(rank, r)
    return base, count


def run_round_chunks(drv, engs, planners, n_rounds, n_sweeps, eligible, by_name=False, observe=None):
    """The loop of ShardedTempering.run_rounds and LocalTempering.run_rounds: `n_rounds` rounds of driver `drv` over its contexts
    `engs` (each owns whole ladders and decides their swaps by itself) and their RoundPlanners, the rest of a planned chunk at a
    time through the engines' batched rounds call -- pt_rounds_deferred, or pt_rounds_fused with `by_name` -- and through
    drv.round(), round by round, wherever that does not apply.  It applies where the driver says so (`eligible`), there are swap
    pairs and planners, every engine has the call, NLMC_NO_DEFERRED is unset (it does not bind calls by name) and every planner's
    rounds may be batched (RoundPlanner.batchable: the one place that knows which routes may).  Per chunk: every planner still asked
    plans it and says how many rounds are ready; the smallest number goes to every such engine before any is waited for (the calls
    are asynchronous); an engine that refuses -- or whose planner has nothing ready -- is not asked again (drv._rounds_refused; the
    reason is in its rounds_fused_refusal) and runs the same rounds one by one: the planner's sweep, `observe(engine, round)` where
    given, the swap.  Keeps drv.deferred_calls and drv.rounds_routes (per context: last_rounds_route() after its last batched
    call, or None), advances drv.sweeps_done / rounds_done and returns the rounds that every context took in batched calls."""
    call = "pt_rounds_fused" if by_name else "pt_rounds_deferred"
    if not hasattr(drv, "_rounds_refused"):
        drv.deferred_calls, drv.rounds_routes, drv._rounds_refused = 0, [None] * len(engs), [False] * len(engs)
    refused = drv._rounds_refused
    eligible = bool(eligible and planners and drv.n_pairs > 0 and (by_name or not os.environ.get("NLMC_NO_DEFERRED"))
                    and all(hasattr(e, call) for e in engs) and all(pl.batchable(n_sweeps, by_name) for pl in planners))
    done = batched = 0
    while done < n_rounds:
        ii = drv.rounds_done - (drv._planner_round0 if planners else 0)
        if not eligible or not (0 <= ii < planners[0].R) or all(refused):
            drv.round(n_sweeps)
            done += 1
            continue
        # this chunk's schedules and pair selections (inside whatever the caller times), the same chunk for every context
        k = n_rounds - done
        for j, pl in enumerate(planners):
            if not refused[j]:
                ready = pl.rounds_ready(ii, by_name)
                if ready:
                    k = min(k, ready)
                else:
                    refused[j] = True                # (the instance does not take fused windows after all)
        if all(refused):
            continue
        one_by_one = []
        for j, e in enumerate(engs):
            if not refused[j] and getattr(e, call)(k, n_sweeps, drv.seed, drv.sweeps_done, drv.rounds_done, drv.n_pairs,
                                                   precision=drv.precision):
                drv.rounds_routes[j] = e.last_rounds_route() if hasattr(e, "last_rounds_route") else None
                drv.deferred_calls += 1
            else:
                refused[j] = True
                one_by_one.append(j)
        for j in one_by_one:                         # the same k rounds of a context that was refused: round()'s calls
            for r in range(k):
                planners[j].sweep(ii + r)
                if observe is not None:
                    observe(engs[j], drv.rounds_done + r)
                engs[j].pt_swap_philox(drv.rounds_done + r, drv.seed, drv.n_pairs, want_log=False)
        if not one_by_one:
            batched += k
        drv.sweeps_done += k * n_sweeps
        drv.rounds_done += k
        done += k
    return batched


class ShardedTempering:
    """Drives sweep rounds + swap rounds of a sharded ladder set.

    make_engine(inst, n_chains, chain_base, n_chains_global) -> object with the Engine interface used below;
    `dist` is torch.distributed (already initialised) or None for a single process; `torch` the torch module."""

    def __init__(self, make_engine, inst, beta_list, n_chains_global, seed, n_pairs, torch=None, dist=None,
                 device=None, precision="f32"):
        self.torch, self.dist = torch, dist
        self.world = dist.get_world_size() if dist is not None else 1
        self.rank = dist.get_rank() if dist is not None else 0
        self.G = int(n_chains_global)
        self.base, self.count = block_partition(self.G, self.world, self.rank)
        if self.G % self.world != 0 and self.world > 1:
            raise ValueError("all_gather_into_tensor needs equal shards: n_chains_global % world_size != 0")
        self.seed, self.n_pairs, self.precision = int(seed), int(n_pairs), precision
        self.eng = make_engine(inst, self.count, self.base, self.G)
        self.eng_betas = np.asarray(beta_list, dtype=np.float64)
        self.eng.pt_init(self.eng_betas)
        self._lt = None
        self.sweeps_done = 0
        self.rounds_done = 0
        self.collective = dist is not None          # also with a single rank: the launcher path stays exercised
        self.lib_collective = False
        if self.collective:
            # The all-gather of a round is issued by the LIBRARY (ncclAllGather from libnlmc_hip.so on the stream its kernels run on:
            # no hand-over between c10d's collective stream and the kernels' stream, ~10 us per round).  Every rank probes librccl
            # and the ranks agree before anybody enters ncclCommInitRank; the unique id travels through the process group.
            self.lib_collective = agree_on_library_collectives(self.eng, torch, dist, device, want=self.n_pairs > 0)
        self._check_every = int(os.environ.get("NLMC_COMM_CHECK_EVERY", "256"))
        self._timeout_ms = int(float(os.environ.get("NLMC_COMM_TIMEOUT_S", "120")) * 1000)
        # a gloo process group (rehearsals with several ranks on one GPU, which RCCL refuses): collectives on host tensors, the
        # energies staged through the host every round
        self._host_stage = (self.collective and not self.lib_collective and dist.get_backend() == "gloo"
                            and str(device) != "cpu" and device is not None)
        if self.collective and not self.lib_collective:
            self.e_local = torch.empty(self.count, dtype=torch.float64, device=device)
            self.e_all = torch.empty(self.G, dtype=torch.float64, device=device)
            if self._host_stage:
                self.e_local_h = torch.empty(self.count, dtype=torch.float64)
                self.e_all_h = torch.empty(self.G, dtype=torch.float64)
            # the sweep kernels write their chains' energies straight into the all-gather's send buffer
            self._sink = hasattr(self.eng, "set_energy_sink")
            if self._sink:
                self.eng.set_energy_sink(self.e_local.data_ptr())

    def set_spins(self, spins_global):
        self.eng.set_spins(np.asarray(spins_global)[self.base:self.base + self.count])

    def plan(self, n_sweeps, n_rounds=0, chunk_rounds=None, lazy=False, reserve_rounds=0):
        """Level schedules of the next n_sweeps sweeps and pair selections of the next n_rounds swap rounds (both depend
        on the RNG only).  They are built a bounded chunk of rounds at a time (`chunk_rounds`, and a memory budget);
        with `lazy` nothing is built here: every chunk, the first one included, is planned by the round() that first
        needs it, so that the planning work lies inside whatever the caller times (the reference draws its permutation
        inside the sweep loop, NMC/nmc.py:62-71).  `reserve_rounds`: allocate (only allocate) plan buffers for chunks of
        that many rounds now."""
        self._planner = None
        if self._lt is not None:
            self._lt.sweeps_done, self._lt.rounds_done = self.sweeps_done, self.rounds_done
            self._lt.plan(n_sweeps, n_rounds, chunk_rounds=chunk_rounds)
            return
        if n_rounds > 0 and n_sweeps % n_rounds == 0 and hasattr(self.eng, "plan_philox_fused"):
            # rounds of equal length: fused-window level lists where the instance qualifies (same bits, fuller levels)
            self._planner = RoundPlanner(self.eng, self.sweeps_done, n_rounds, n_sweeps // n_rounds, self.seed,
                                         precision=self.precision, budget_bytes=16 << 30, chunk_rounds=chunk_rounds,
                                         pt_pairs=self.n_pairs, pt_round0=self.rounds_done)
            self._planner_round0 = self.rounds_done
            if reserve_rounds and self._planner.window and hasattr(self.eng, "plan_reserve_fused"):
                self.eng.plan_reserve_fused(int(reserve_rounds) * (self._planner.S // self._planner.window), self._planner.window)
            if not lazy:
                self._planner.prepare(0)
            return
        self.eng.plan_philox(self.sweeps_done, n_sweeps, self.seed, precision=self.precision)
        if n_rounds > 0 and self.n_pairs > 0 and hasattr(self.eng, "pt_plan"):
            self.eng.pt_plan(self.rounds_done, n_rounds, self.seed, self.n_pairs)

    def configure_nmc(self, *args, **kw):
        """NMC_task slots (NPT/npt.py:622-647) under the one-process-per-GPU driver: every rank must own WHOLE ladders (restarts
        sharded over the ranks) -- the chains on marked slots are then a fixed number per rank, each rank decides its own ladders'
        swaps on the device (same Philox keys as one context holding everything) and a round needs no collective at all.  The
        rounds are driven by a LocalTempering over this rank's engine: same bits as LocalTempering over all contexts in one process."""
        L = self.eng.ladder_len
        if self.base % L or self.count % L:
            raise NotImplementedError("NMC slots under a ladder that is cut across ranks: shard whole ladders (restarts % ranks == 0)")
        self._lt = LocalTempering(None, self.eng_betas, self.G, self.seed, self.n_pairs, [0], precision=self.precision,
                                  engines=[self.eng], parts=[(self.base, self.count)])
        self._lt.sweeps_done, self._lt.rounds_done = self.sweeps_done, self.rounds_done
        self._lt.configure_nmc(*args, **kw)

    def round(self, n_sweeps, want_log=False, **outputs):
        """`n_sweeps` sweeps of every local chain at its ladder temperature, then one swap attempt round.  `outputs` (record_stride /
        want_* of sweep_philox): the sweeps' outputs are left in self.last_outputs."""
        if getattr(self, "_lt", None) is not None:           # rounds with NMC slots (whole ladders per rank): no collective
            self.last_outputs = self._lt.round(n_sweeps, **outputs)[0]
            self.sweeps_done, self.rounds_done = self._lt.sweeps_done, self._lt.rounds_done
            return None
        pl = getattr(self, "_planner", None)
        if pl is not None and n_sweeps == pl.S and 0 <= self.rounds_done - self._planner_round0 < pl.R:
            self.last_outputs = pl.sweep(self.rounds_done - self._planner_round0, **outputs)
        else:
            self.last_outputs = self.eng.sweep_philox(n_sweeps, self.seed, sweep0=self.sweeps_done, beta=None, precision=self.precision, **outputs)
        self.sweeps_done += n_sweeps
        log = None
        if self.n_pairs > 0:
            if self.lib_collective:
                log = self.eng.pt_swap_philox_collective(self.rounds_done, self.seed, self.n_pairs, refresh_energies=n_sweeps == 0,
                                                         want_log=want_log)
                if self._check_every and (self.rounds_done + 1) % self._check_every == 0:
                    self.eng.comm_check(self._timeout_ms)            # RCCL async error or a lost rank: abort, RuntimeError (never a hang)
            elif self.collective:
                if not self._sink or n_sweeps == 0:
                    self.eng.energy_dev(self.e_local.data_ptr())       # tracked energies -> device/host buffer
                if self._host_stage:
                    self.e_local_h.copy_(self.e_local)
                    self.dist.all_gather_into_tensor(self.e_all_h, self.e_local_h)
                    self.e_all.copy_(self.e_all_h)
                else:
                    self.dist.all_gather_into_tensor(self.e_all, self.e_local)   # the ONE collective of the round
                log = self.eng.pt_swap_philox(self.rounds_done, self.seed, self.n_pairs,
                                              energies_all_dev=self.e_all.data_ptr(), want_log=want_log)
            else:
                log = self.eng.pt_swap_philox(self.rounds_done, self.seed, self.n_pairs, want_log=want_log)
        self.rounds_done += 1
        return log

    def run_rounds(self, n_rounds, n_sweeps, persistent=None):
        """`n_rounds` rounds of `n_sweeps` sweeps + one swap round each -- same bits as round() called n_rounds times, which is what
        everything that does not qualify falls back to.  A context that owns whole ladders and needs no collective hands a planned
        chunk of rounds to the engine at a time (pt_rounds_deferred; NLMC_NO_DEFERRED switches that off), which runs them inside
        launches of k_rounds_fused where the device holds all chains at once: the chains stay in LDS between the rounds, a chain
        publishes its energy per round and waits for its swap partner's alone, the next round's first two uniform tables are made in
        this round's tail (include/nlmc.h: nlmc_pt_rounds_deferred; measured at the bench shape: 109.6 against 113.9 us per round,
        DESIGN.md section 5).  Otherwise, or with NLMC_NO_PERSISTENT=1 when the engine is created, the engine runs a sweep launch per
        round that decides the previous round's swap in its prologue; eng.last_rounds_route() tells which.  `persistent` (default: the
        environment variable NLMC_PERSISTENT) asks for k_rounds_fused by name (pt_rounds_fused: a refusal instead of the launch per
        round) and counts the rounds in persistent_rounds instead of deferred_rounds.  Sweeps that run one chain per lane, or per wave
        with wave_rounds, need no window: the engine runs such chunks inside k_rounds_lanes / k_rounds_waves, for any round length
        (not by name: pt_rounds_fused would refuse them and is not asked).  The loop and the rule: run_round_chunks."""
        if persistent is None:
            persistent = bool(os.environ.get("NLMC_PERSISTENT"))
        pl = getattr(self, "_planner", None)
        k = run_round_chunks(self, [self.eng], [pl] if pl is not None else None, n_rounds, n_sweeps,
                             self._lt is None and not self.collective, by_name=persistent)
        if persistent:
            self.persistent_rounds = getattr(self, "persistent_rounds", 0) + k
        else:
            self.deferred_rounds = getattr(self, "deferred_rounds", 0) + k

    def gather_spins(self):
        """All chains' configurations on every rank (read-out only; not part of a round)."""
        loc = self.eng.get_spins()
        if not self.collective:
            return loc
        dev = self.torch.device("cuda", self.torch.cuda.current_device()) if self.lib_collective else self.e_all.device
        if self._host_stage:
            dev = "cpu"
        t = self.torch.from_numpy(loc.astype(np.int8)).to(dev)
        out = self.torch.empty((self.G, loc.shape[1]), dtype=self.torch.int8, device=dev)
        self.dist.all_gather_into_tensor(out, t)
        return out.cpu().numpy()

    def close(self):
        try:
            if self.lib_collective:
                self.eng.comm_check(self._timeout_ms)
            if self._lt is not None:
                self._lt.check()
            elif self.n_pairs > 0 and hasattr(self.eng, "pt_check"):
                self.eng.pt_check()          # a swap round whose pair selection ran out raises here at the latest
        finally:
            self.eng.close()


class LocalTempering:
    """The same sharded tempering driven by ONE process over several contexts -- one per entry of `device_ids`
    (NPT.run(device_ids=...), APT_ICM.run(device_ids=...); the reference's knob is num_cores, NPT/npt.py:535-539,616).
    Chains are cut into contiguous blocks like ShardedTempering.  Blocks of whole ladders (restarts >= contexts) decide their
    own ladders' swaps on the device and never meet: the contexts run out of step, which is also how `device_ids=[0] * k`
    shortens a round whose cost is its slowest chain (NMC slots: the backbone inference).  Blocks that cut a ladder pass the
    tracked energies through host memory every round (G float64) and every context takes the identical Philox-keyed
    decision.  Either way the trajectory equals the single-context one bit for bit.  For one GPU per process over RCCL use
    ShardedTempering."""

    def __init__(self, inst, beta_list, n_chains_global, seed, n_pairs, device_ids, precision="f32", engine_factory=None,
                 engines=None, parts=None, lane_sweeps="off", track_best=False, target_energy=None, track_energies=False,
                 wave_sweeps="off", wave_rounds=False, lane_nmc=None, wave_long=False, wave_long_rounds=False, wave_nmc=None,
                 wave_long_nmc=None):
        """`parts` (optional): the blocks [(chain_base, count)] this process drives instead of an even cut over device_ids -- one
        rank's share under a launcher; `engines`: contexts that exist already (they must have had pt_init; not closed here... they
        ARE closed by close(): hand over ownership); `lane_sweeps`: Engine.set_lane_sweeps of every engine created here ("off",
        "auto", "force": short chains one per lane, and run_rounds' chunks inside k_rounds_lanes -- same bits); `wave_sweeps`:
        Engine.set_wave_sweeps of every engine created here ("off", "auto", "force": f32 sweeps of chains of at most 256 spins one per
        wave with resident local fields, round by round through the sweep calls -- same bits); `wave_rounds`:
        Engine.set_wave_rounds of every engine created here (needs wave_sweeps != "off", ValueError otherwise): run_rounds' chunks of
        such chains run inside k_rounds_waves -- same bits); `wave_long`: Engine.set_wave_long of every engine created here (needs
        wave_sweeps != "off", ValueError otherwise): the wave route takes chains of up to 1024 spins, and with `wave_rounds` those of
        more than 256 run a sweep call and a swap call per round -- same bits); `wave_long_rounds`: Engine.set_wave_long_rounds of every
        engine created here (needs `wave_rounds` and `wave_long`, ValueError otherwise): run_rounds' chunks of chains of 257..1024 spins
        run inside k_rounds_waves_long, the local fields resident across the swap rounds -- same bits); `track_best`: every
        context keeps the record of its chains' lowest-energy states (Engine.best_begin; `target_energy`: the energy whose first
        passage is stamped, in the engine's units) -- one observation per round, stamp = round index, after the round's sweeps (and
        NMC cycles) and before its swap; best() reads it.  The record only observes: the trajectory is the same bits.
        `track_energies`: every context keeps a per-round log of its chains' tracked energies and temperature slots as the round's
        swap decision sees them (Engine.elog_begin) -- opened by plan() for the rounds it plans, or by energy_log_begin(); one
        observation per round at the same place; energy_log() reads it.  Needs whole ladders per context (ValueError otherwise).
        `lane_nmc` (None: LANE_NMC_IN_LAUNCH where the engine's sweeps run one chain per lane, Engine.lanes_take; True, False): with NMC slots (configure_nmc), a round that wants no per-sweep output runs
        the marked chains' phases in one Engine.nmc_phases_lanes call per context instead of the phase loop -- same bits.  A context
        whose engine refuses (long chains, ...) keeps the phase loop and is not asked again.  Counters: lane_nmc_rounds (rounds in
        which every context took the call), lane_nmc_calls (calls that ran).
        `wave_nmc` (None: WAVE_NMC_IN_LAUNCH where the engine's sweeps run one chain per wave, Engine.waves_take; True, False): the same
        through Engine.nmc_phases_waves, one k_nmc_phases_waves launch per context -- same bits.  Asked before `lane_nmc`, as the wave
        route is asked before the lane route; a context whose engine refuses (chains of more than 256 spins, ...) goes on to
        `wave_long_nmc`, the lane rule and the phase loop and is not asked again.  Counters: wave_nmc_rounds, wave_nmc_calls.
        `wave_long_nmc` (None: WAVE_LONG_NMC_IN_LAUNCH where the engine's sweeps run one chain per wave; True, False; given, it needs
        `wave_long`, ValueError otherwise): the same for chains of 257 to 1024 spins through Engine.nmc_phases_waves_long, one
        k_nmc_phases_waves_long launch per context -- same bits.  Asked after `wave_nmc` and before `lane_nmc`; a context whose engine
        refuses goes on and is not asked again.  Counters: wave_long_nmc_rounds, wave_long_nmc_calls."""
        hostlogic.check_wave_rounds(wave_rounds, wave_sweeps, needs="wave_sweeps 'auto' or 'force'")
        hostlogic.check_wave_long(wave_long, wave_sweeps, needs="wave_sweeps 'auto' or 'force'")
        hostlogic.check_wave_long_rounds(wave_long_rounds, wave_rounds, wave_long)
        hostlogic.check_wave_long_nmc(wave_long_nmc, wave_long)
        self.G, self.seed, self.n_pairs, self.precision = int(n_chains_global), int(seed), int(n_pairs), precision
        devs = list(device_ids)
        self.parts = list(parts) if parts is not None else [block_partition(self.G, len(devs), r) for r in range(len(devs))]
        L = len(np.asarray(beta_list).reshape(-1))
        # every context owns whole ladders: each decides its own ladders' swaps from its own tracked energies (same Philox keys
        # as one context holding everything), nothing passes through the host and the contexts run out of step with each other
        self.whole_ladders = all(base % L == 0 and count % L == 0 for base, count in self.parts)
        self.engs = list(engines) if engines is not None else []
        self.nmc_sweeps_done = 0
        try:
            for d, (base, count) in (zip(devs, self.parts) if engines is None else []):
                if engine_factory is not None:           # (tests: the CPU double of tests/fake_engine.py)
                    e = engine_factory(inst, count, base, self.G)
                else:
                    e = Engine(inst, None, count, device=int(d), chain_base=base, n_chains_global=self.G,
                               own_stream=len(devs) > 1)
                hostlogic.set_route_modes(e, lane_sweeps, wave_sweeps, wave_rounds, wave_long, wave_long_rounds)
                e.pt_init(np.asarray(beta_list, dtype=np.float64))
                self.engs.append(e)
        except Exception:
            self.close()
            raise
        self.sweeps_done = self.rounds_done = 0
        self._planners = None
        self.nmc = None
        self._nmc_planners = None
        options = dict(lane_nmc=lane_nmc, wave_nmc=wave_nmc, wave_long_nmc=wave_long_nmc)
        self.nmc_routes = {route: NmcRouteState(options[spec.option], globals()[spec.default]) for route, spec in NMC_ROUTES.items()}
        self.track_best = bool(track_best)
        self.track_energies, self._elog_open = bool(track_energies), False
        if self.track_energies and not self.whole_ladders:
            self.close()
            raise ValueError("track_energies needs every ladder inside one context (whole ladders per block)")
        if self.track_best:
            for e in self.engs:
                e.best_begin(target_energy)

    def set_spins(self, spins_global):
        for e, (base, count) in zip(self.engs, self.parts):
            e.set_spins(np.asarray(spins_global)[base:base + count])

    def configure_nmc(self, doNMC, phases, sweeps_per_phase, global_beta, temp_x, epsilon, lambdas, tolerance, max_iterations,
                      sat, thresholds, M_skip=1):
        """Temperature slots with doNMC run NMC_task instead of MCMC_task every round (NPT/npt.py:622-647): backbone inference
        seeded with the chain's state, then `phases` ("C" / "NC" / "ALL") of `sweeps_per_phase` sweeps at `global_beta`,
        each starting from the argmin-energy configuration of the one before (NPT/npt.py:357-477).  Everything stays on the
        device (include/nlmc.h: nlmc_pt_mark_slots ... nlmc_set_phase)."""
        marks = np.asarray(doNMC).astype(bool)
        if not marks.any():
            self.nmc = None
            return
        for e in self.engs:
            e.mark_slots(marks)
            e.overlap_subsets(not os.environ.get("NLMC_NO_OVERLAP"))      # plain chains' sweeps beside the NMC chains' work
        self.nmc = dict(phases=list(phases), S=int(sweeps_per_phase), beta=float(global_beta), temp_x=float(temp_x),
                        epsilon=np.asarray(epsilon, dtype=np.float64), lambdas=np.asarray(lambdas, dtype=np.float64),
                        tol=float(tolerance), max_it=int(max_iterations), sat=float(sat),
                        thresholds=np.asarray(thresholds, dtype=np.float64), M_skip=max(1, int(M_skip)))
        # M_skip > 1 (NPT/npt.py:434-437: M = M[:, ::M_skip] before the energies and the argmin): the phases' running minimum looks at
        # every M_skip-th sweep only (nlmc_track_minimum(M_skip)), their recorded traces are strided the same way

    # the options and counters of nmc_routes under the names the keywords and NPT have for them
    lane_nmc = property(lambda self: self.nmc_routes["lanes"].on)
    lane_nmc_rounds = property(lambda self: self.nmc_routes["lanes"].rounds)
    lane_nmc_calls = property(lambda self: self.nmc_routes["lanes"].calls)
    wave_nmc = property(lambda self: self.nmc_routes["waves"].on)
    wave_nmc_rounds = property(lambda self: self.nmc_routes["waves"].rounds)
    wave_nmc_calls = property(lambda self: self.nmc_routes["waves"].calls)
    wave_long_nmc = property(lambda self: self.nmc_routes["waves_long"].on)
    wave_long_nmc_rounds = property(lambda self: self.nmc_routes["waves_long"].rounds)
    wave_long_nmc_calls = property(lambda self: self.nmc_routes["waves_long"].calls)

    def _nmc_takes(self, route, k):
        """Whether context k's NMC phases go to the engine call of `route` (a key of NMC_ROUTES): the option is on, and the engine has
        not refused (asked once per context: a refusal is remembered).  An option left to its default applies only where the context's
        sweeps take that route anyway (Engine.waves_take / lanes_take)."""
        spec, st = NMC_ROUTES[route], self.nmc_routes[route]
        if not (self.nmc and st.on) or k in st.refused:
            return False
        if k in st.asked:
            return True
        e = self.engs[k]
        st.asked.add(k)
        on_route = hasattr(e, spec.take) and getattr(e, spec.take)()
        if not hasattr(e, spec.call) or (st.by_default and not on_route) or \
                (hasattr(e, spec.call + "_refusal") and getattr(e, spec.call + "_refusal")(self.nmc["S"])):
            st.refused.add(k)
            return False
        return True

    def sweeps_per_round(self, n_sweeps):
        """Plain sweep indices (RNG counters) one round of `n_sweeps` sweeps consumes.  The NMC phases of the marked slots draw from
        a range of their own (NMC_SWEEP_SPACE + nmc_sweeps_done, advanced by phases x sweeps_per_phase per round)."""
        return n_sweeps

    def plan(self, n_sweeps, n_rounds, chunk_rounds=None):
        S = n_sweeps // max(1, n_rounds)
        self._planners = [RoundPlanner(e, self.sweeps_done, n_rounds, S, self.seed,
                                       precision=self.precision, budget_bytes=8 << 30, chunk_rounds=chunk_rounds,
                                       pt_pairs=self.n_pairs, pt_round0=self.rounds_done, slot=0, fused_outputs=True) for e in self.engs]
        self._planner_round0 = self.rounds_done
        self._nmc_planners = None
        if self.nmc and not all(any(self._nmc_takes(route, k) for route in NMC_ROUTES) for k in range(len(self.engs))):
            # (where every context runs its phases inside nmc_phases_waves / nmc_phases_waves_long / nmc_phases_lanes launches there is nothing to plan for
            # them: the rounds with outputs run their phases on the wave or lane kernels, which need no level schedule)
            # the NMC phases draw from their own range of sweep indices, behind the plain sweeps of all planned rounds: both
            # ranges are contiguous over the rounds, so each is served by one fused-window plan (slots 0 and 1)
            n_ph = len(self.nmc["phases"])
            self._nmc_sweep0 = NMC_SWEEP_SPACE + self.nmc_sweeps_done
            self._nmc_planners = [RoundPlanner(e, self._nmc_sweep0, n_rounds * n_ph, self.nmc["S"], self.seed,
                                               precision=self.precision, budget_bytes=4 << 30,
                                               chunk_rounds=None if chunk_rounds is None else chunk_rounds * n_ph,
                                               slot=1, beta=self.nmc["beta"], fused_outputs=True) for e in self.engs]
            self._planned_rounds = n_rounds
        if self.track_energies:
            self.energy_log_begin(n_rounds)

    def energy_log_begin(self, n_rounds):
        """Open (or reset) every context's energy log for rounds [rounds_done, rounds_done + n_rounds) (track_energies)."""
        if not self.track_energies:
            raise ValueError("LocalTempering.energy_log_begin: created without track_energies")
        for e in self.engs:
            e.elog_begin(self.rounds_done, n_rounds)
        self._elog_open = True

    def log_begin(self, n_rounds):
        for e in self.engs:
            e.pt_log_begin(self.rounds_done, n_rounds, self.n_pairs)

    def _observe(self, e, round_idx):
        """Round `round_idx` of context e as its swap decision will see it, for the records that are open (track_best, track_energies)."""
        if self.track_best:
            e.best_update(round_idx)
        if self._elog_open:
            e.elog_update(round_idx)

    def round(self, n_sweeps, energy_columns=0, **outputs):
        """Sweeps of every block (launched back to back: the devices work concurrently), then one swap round.  Returns
        the per-context sweep outputs; with NMC slots configured (configure_nmc) every entry is a dict
        {"plain": outputs of the chains on plain slots, "plain_chains": their local ids, "nmc": [outputs per phase],
        "nmc_chains": ids, "plain_energy_columns": fp64 energies of the first `energy_columns` recorded columns}."""
        ii = self.rounds_done - (self._planner_round0 if self._planners else 0)
        outs = []
        in_launch = dict.fromkeys(NMC_ROUTES, 0)
        wants = any(outputs.get(k) for k in ("record_stride", "want_energy", "want_min", "want_state"))
        for k, e in enumerate(self.engs):
            if self.nmc:
                e.set_phase("ALL")                   # (not set_flags(None): temp_x stays, so do the uploaded temperature tables)
                e.select("unmarked")
            if self._planners and 0 <= ii < self._planners[k].R and n_sweeps == self._planners[k].S:
                o = self._planners[k].sweep(ii, **outputs)
            else:
                o = e.sweep_philox(n_sweeps, self.seed, sweep0=self.sweeps_done, beta=None, precision=self.precision, **outputs)
            if not self.nmc:
                self._observe(e, self.rounds_done)
                outs.append(o)
                continue
            rec = dict(plain=o, nmc=[])
            if wants:
                rec["plain_chains"] = e.subset()
                if energy_columns and outputs.get("record_stride"):
                    rec["plain_energy_columns"] = e.energy_of_recorded(energy_columns)
            q = self.nmc
            e.select("marked")
            if wants:
                rec["nmc_chains"] = e.subset()
            e.backbone_clusters(q["epsilon"], q["lambdas"], q["beta"], q["tol"], q["max_it"], q["sat"], q["thresholds"])
            took = False
            for route in NMC_ROUTES:                 # all phases in one launch (same bits as the loop below): the wave calls asked first
                if wants or took or not self._nmc_takes(route, k):
                    continue
                try:
                    getattr(e, NMC_ROUTES[route].call)(q["phases"], q["S"], self.seed, NMC_SWEEP_SPACE + self.nmc_sweeps_done, q["beta"],
                                                       q["temp_x"], min_stride=q["M_skip"], precision=self.precision)
                    took = True
                    in_launch[route] += 1
                except NotImplementedError:          # nothing was run: the next route or the phase loop, now and from here on
                    self.nmc_routes[route].refused.add(k)
            if took:
                e.set_phase("ALL")
                e.select("all")
                self._observe(e, self.rounds_done)
                outs.append(rec)
                continue
            e.track_minimum(True, stride=q["M_skip"])
            n_ph = len(q["phases"])
            out_nmc = dict(outputs, record_stride=q["M_skip"]) if outputs.get("record_stride") else outputs
            planned = self._nmc_planners is not None and 0 <= ii < self._planned_rounds
            for p, kind in enumerate(q["phases"]):
                if p > 0:
                    e.adopt_best()                   # NPT/npt.py:436-437,454-455: the next phase starts from the argmin column
                e.set_phase(kind, q["temp_x"])
                if planned:
                    rec["nmc"].append(self._nmc_planners[k].sweep(ii * n_ph + p, **out_nmc))
                else:
                    rec["nmc"].append(e.sweep_philox(q["S"], self.seed, sweep0=NMC_SWEEP_SPACE + self.nmc_sweeps_done + p * q["S"],
                                                     beta=q["beta"], precision=self.precision, **out_nmc))
            e.track_minimum(False)
            e.set_phase("ALL")
            e.select("all")
            self._observe(e, self.rounds_done)      # (all chains selected again, the NMC chains in the state they carry on; before the swap)
            outs.append(rec)
        self.sweeps_done += n_sweeps
        for route, st in self.nmc_routes.items():
            st.calls += in_launch[route]
            if in_launch[route] and in_launch[route] == len(self.engs):
                st.rounds += 1
        if self.nmc:
            self.nmc_sweeps_done += len(self.nmc["phases"]) * self.nmc["S"]
        if self.n_pairs > 0:
            if len(self.engs) == 1 or self.whole_ladders:
                for e in self.engs:
                    e.pt_swap_philox(self.rounds_done, self.seed, self.n_pairs, want_log=False)
            else:
                E = np.concatenate([e.energy_tracked() for e in self.engs])
                for e in self.engs:
                    e.pt_swap_philox_host(self.rounds_done, self.seed, self.n_pairs, E)
        self.rounds_done += 1
        return outs

    def run_rounds(self, n_rounds, n_sweeps):
        """`n_rounds` rounds of `n_sweeps` sweeps + one swap round each, without outputs -- same bits as round(n_sweeps) called
        n_rounds times, which is what everything that does not qualify falls back to.  ShardedTempering.run_rounds' loop and rule
        (run_round_chunks) over contexts without NMC slots that own whole ladders: one fused window per round -- or sweeps that run
        one chain per lane (lane_sweeps: such a chunk needs only its pair selections planned, and the engine runs it inside
        k_rounds_lanes) or one chain per wave with wave_rounds (likewise, inside k_rounds_waves); the engine picks the route
        (Engine.pt_rounds_deferred).  A context whose engine refuses is not asked again and runs its rounds one by one from then on
        (whole ladders: the contexts never meet).  Counters: deferred_rounds (rounds every context took in batched calls),
        deferred_calls, and rounds_routes (per context: last_rounds_route() after its last batched call, or None)."""
        self.deferred_rounds = getattr(self, "deferred_rounds", 0) + run_round_chunks(
            self, self.engs, self._planners, int(n_rounds), int(n_sweeps), not self.nmc and self.whole_ladders, observe=self._observe)

    def slots(self):
        if len(self.engs) == 1 or not self.whole_ladders:
            return self.engs[0].pt_slots()
        return np.concatenate([e.pt_slots()[base:base + count] for e, (base, count) in zip(self.engs, self.parts)])

    def swap_log(self):
        if len(self.engs) == 1 or not self.whole_ladders:
            return self.engs[0].pt_log_read()
        L = self.engs[0].ladder_len
        pairs, acc = self.engs[0].pt_log_read()
        for e, (base, count) in list(zip(self.engs, self.parts))[1:]:          # every context logged its own ladders' rows
            p, a = e.pt_log_read()
            pairs[:, base // L:(base + count) // L] = p[:, base // L:(base + count) // L]
            acc[:, base // L:(base + count) // L] = a[:, base // L:(base + count) // L]
        return pairs, acc

    def gather_spins(self):
        return np.concatenate([e.get_spins() for e in self.engs])

    def best(self, want_state=True):
        """The contexts' best-state records by global chain id (track_best): dict(energy [G], stamp [G] = round of the first
        attainment, first_hit [G] = first round at or below target_energy or -1, state [G, n] int8 or None)."""
        if not self.track_best:
            raise ValueError("LocalTempering.best: created without track_best")
        order = np.argsort([base for base, _ in self.parts], kind="stable")
        recs = [self.engs[j].best_read(want_state=want_state) for j in order]
        return {k: (np.concatenate([r[k] for r in recs]) if recs[0][k] is not None else None)
                for k in ("energy", "stamp", "first_hit", "state")}

    def energy_log(self):
        """The contexts' per-round energy logs by global chain id (track_energies): (energies [n_rounds, G] float64, slots
        [n_rounds, G] int32) of the window most recently opened; NaN / -1 in rounds that did not run."""
        if not self.track_energies:
            raise ValueError("LocalTempering.energy_log: created without track_energies")
        if not self._elog_open:
            raise ValueError("LocalTempering.energy_log: no log was opened (plan() or energy_log_begin())")
        order = np.argsort([base for base, _ in self.parts], kind="stable")
        logs = [self.engs[j].elog_read() for j in order]
        return np.concatenate([l[0] for l in logs], axis=1), np.concatenate([l[1] for l in logs], axis=1)

    def check(self):
        if self.n_pairs > 0:
            for e in self.engs:
                e.pt_check()
        if self.nmc:
            for e in self.engs:
                e.backbone_check()      # ValueError('LBP diverged at initial lambda ...') of NPT/npt.py:178-180

    def close(self):
        for e in self.engs:
            e.close()
        self.engs = []


def agree_on_library_collectives(eng, torch, dist, device, want):
    """Every rank probes librccl (nlmc_comm_probe) and the ranks agree -- an all-reduce(MIN) of the answers over the process group
    that is already up -- BEFORE anybody calls nlmc_comm_init: a rank that cannot load the library must not leave the others
    waiting inside ncclCommInitRank.  Returns True when the library-issued collectives are on for ALL ranks; the
    communicator's unique id then travels through the same process group."""
    ok = bool(want) and hasattr(eng, "comm_init") and dist.get_backend() == "nccl" and not os.environ.get("NLMC_TORCH_COLLECTIVE")
    if ok:
        try:
            ok = bool(type(eng).comm_probe())
        except Exception as ex:  # noqa: BLE001
            print(f"[nlmc] librccl probe failed ({ex})", file=sys.stderr)
            ok = False
    if dist.get_backend() == "gloo":
        device = "cpu"                              # (the flags below are host tensors for a gloo group)
    flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=device)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if int(flag.item()) != 1:
        if want and dist.get_rank() == 0 and dist.get_backend() == "nccl" and not os.environ.get("NLMC_TORCH_COLLECTIVE"):
            print("[nlmc] library-issued collectives unavailable on some rank; using torch.distributed", file=sys.stderr)
        return False
    uid = torch.zeros(129, dtype=torch.uint8, device=device)           # [128] = 1: rank 0 could create an id
    if dist.get_rank() == 0:
        try:
            uid[:128].copy_(torch.from_numpy(type(eng).comm_unique_id()))
            uid[128] = 1
        except (NotImplementedError, RuntimeError) as ex:
            print(f"[nlmc] ncclGetUniqueId failed ({ex}); using torch.distributed", file=sys.stderr)
    dist.broadcast(uid, 0)
    if int(uid[128].item()) != 1:
        return False
    # comm_init itself may still fail on one rank (out of memory, ...): agree once more, and drop the communicator everywhere if so
    err = None
    try:
        eng.comm_init(uid[:128].cpu().numpy(), dist.get_world_size(), dist.get_rank())
    except Exception as ex:  # noqa: BLE001
        err = ex
    flag = torch.tensor([0 if err else 1], dtype=torch.int32, device=device)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if int(flag.item()) != 1:
        raise RuntimeError(f"nlmc_comm_init failed on some rank ({err}); aborting the job") from err
    return True


class SlotShardedAPT:
    """APT + iso-cluster moves (NPT/apt_ICM.py:195-285) with the temperature ladder cut into slot blocks (SURVEY.md section 8e:
    all sub-replicas of a temperature on one GPU; include/nlmc.h: nlmc_apt_shard, csrc/nlmc_apt.h).

    R temperatures x K sub-replicas; shard w of W owns the slots [w R/W, (w+1) R/W) of all K sub-replica ladders.  Per round:
    sweeps at the slots' temperatures -> Houdayer moves between the randomly paired sub-replicas of every local slot (k_icm_round,
    nothing leaves the GPU) -> swap round: ONE all-gather of K R/W tracked energies per shard + ONE exchange of the K boundary
    configurations with each neighbour shard; every shard takes the identical Philox-keyed decision; pairs inside a block are label
    exchanges, accepted pairs across a block boundary move the two configurations.  Random numbers are keyed by (sub-replica,
    global slot): the states on every (sub-replica, slot) are bit-identical for any W.

    Three transports, one protocol:
      * `dist` (torch.distributed, one process per GPU): the library issues the collectives itself over RCCL on the kernels'
        stream (apt_swap_collective) when every rank can; otherwise torch.distributed moves the same buffers (gloo on CPUs);
      * `device_ids` (one process, W = len(device_ids) contexts): the same data through host memory;
      * neither: one context, W = 1.
    make_engine(inst, n_chains, chain_base, n_chains_global) as for ShardedTempering (tests inject the oracle-backed double)."""

    def __init__(self, make_engine, inst, beta_list, n_subreplicas, seed, n_pairs, torch=None, dist=None, device=None,
                 precision="f32", katzgraber=True, device_ids=None):
        self.torch, self.dist, self.device = torch, dist, device
        self.betas = np.asarray(beta_list, dtype=np.float64).reshape(-1)
        self.R, self.K = int(self.betas.shape[0]), int(n_subreplicas)
        self.seed, self.n_pairs, self.precision, self.katz = int(seed), int(n_pairs), precision, bool(katzgraber)
        if dist is not None:
            self.W, ranks = dist.get_world_size(), [dist.get_rank()]
        else:
            self.W = len(device_ids) if device_ids else 1
            ranks = list(range(self.W))
        if self.R % self.W:
            raise ValueError(f"{self.R} temperatures do not split evenly over {self.W} shards")
        self.Rw = self.R // self.W
        self.ranks, self.engs = ranks, []
        try:
            for i, w in enumerate(ranks):
                e = make_engine(inst, self.K * self.Rw, 0, self.K * self.Rw) if dist is not None or not device_ids else \
                    make_engine(inst, self.K * self.Rw, 0, self.K * self.Rw, device_ids[i])
                self.engs.append(e)
                e.pt_init(self.betas[w * self.Rw:(w + 1) * self.Rw])
                e.apt_shard(self.betas, self.W, w)
        except Exception:
            self.close()
            raise
        self.sweeps_done = self.rounds_done = 0
        self._planners = None
        self.lib_collective = False
        if dist is not None and self.W > 1:
            self.lib_collective = agree_on_library_collectives(self.engs[0], torch, dist, device, want=self.n_pairs > 0)
        self._check_every = int(os.environ.get("NLMC_COMM_CHECK_EVERY", "256"))
        self._timeout_ms = int(float(os.environ.get("NLMC_COMM_TIMEOUT_S", "120")) * 1000)

    # -- states by (sub-replica, global slot) -------------------------------------------------------------------------------
    def set_spins_by_slot(self, spins):
        """spins [K, R, N]: the configuration on (sub-replica j, temperature slot r).  Slots are reset to the identity."""
        s = np.asarray(spins, dtype=np.int8).reshape(self.K, self.R, -1)
        for e, w in zip(self.engs, self.ranks):
            e.pt_set_slots((np.arange(self.K * self.Rw) % self.Rw).astype(np.int32))
            e.set_spins(np.ascontiguousarray(s[:, w * self.Rw:(w + 1) * self.Rw]).reshape(self.K * self.Rw, -1))

    def _local_by_slot(self, e):
        cfg, slots = e.get_spins(), e.pt_slots()
        out = np.empty((self.K, self.Rw, cfg.shape[1]), np.int8)
        out[np.arange(self.K * self.Rw) // self.Rw, slots] = cfg
        en = np.empty((self.K, self.Rw))
        en[np.arange(self.K * self.Rw) // self.Rw, slots] = e.energy_tracked()
        return out, en

    def gather_by_slot(self):
        """(configurations [K, R, N], tracked energies [K, R]) by (sub-replica, global slot), on every process (read-out only)."""
        loc = [self._local_by_slot(e) for e in self.engs]
        if self.dist is None or self.W == 1:
            return np.concatenate([x[0] for x in loc], axis=1), np.concatenate([x[1] for x in loc], axis=1)
        t, dev = self.torch, self.device
        cfg = t.from_numpy(loc[0][0]).to(dev)
        en = t.from_numpy(loc[0][1]).to(dev)
        cfgs = [t.empty_like(cfg) for _ in range(self.W)]
        ens = [t.empty_like(en) for _ in range(self.W)]
        self.dist.all_gather(cfgs, cfg)
        self.dist.all_gather(ens, en)
        return np.concatenate([x.cpu().numpy() for x in cfgs], axis=1), np.concatenate([x.cpu().numpy() for x in ens], axis=1)

    # -- rounds -----------------------------------------------------------------------------------------------------------
    def plan(self, n_rounds, sweeps_per_round, chunk_rounds=None, budget_bytes=8 << 30):
        """Level schedules and pair selections of the next rounds (RNG only), built a chunk of rounds at a time by the round that
        first needs them (RoundPlanner)."""
        self._planners = [RoundPlanner(e, self.sweeps_done, n_rounds, sweeps_per_round, self.seed, precision=self.precision,
                                       budget_bytes=budget_bytes, chunk_rounds=chunk_rounds, pt_pairs=self.n_pairs,
                                       pt_round0=self.rounds_done) for e in self.engs]
        self._planner_round0 = self.rounds_done

    def _swap_torch(self, want_log):
        """The round's exchange through torch.distributed (gloo on CPUs, or RCCL when the library cannot issue it itself): the same
        buffers as the library path -- K Rw int64 per rank all-gathered, K configurations to and from each neighbour."""
        t, dist, dev, e, w = self.torch, self.dist, self.device, self.engs[0], self.ranks[0]
        ef, lo, hi = e.apt_pack()
        mine = t.from_numpy(ef.reshape(-1)).to(dev)
        parts = [t.empty_like(mine) for _ in range(self.W)]
        dist.all_gather(parts, mine)
        recv_lo = t.empty((self.K, e.n), dtype=t.int8, device=dev) if w > 0 else None
        recv_hi = t.empty((self.K, e.n), dtype=t.int8, device=dev) if w + 1 < self.W else None
        ops = []
        if w > 0:
            ops += [dist.P2POp(dist.isend, t.from_numpy(lo).to(dev), w - 1), dist.P2POp(dist.irecv, recv_lo, w - 1)]
        if w + 1 < self.W:
            ops += [dist.P2POp(dist.isend, t.from_numpy(hi).to(dev), w + 1), dist.P2POp(dist.irecv, recv_hi, w + 1)]
        for req in (dist.batch_isend_irecv(ops) if ops else []):
            req.wait()
        ef_all = np.stack([p.cpu().numpy() for p in parts])
        return e.apt_swap_host(self.rounds_done, self.seed, self.n_pairs, ef_all,
                               None if recv_lo is None else recv_lo.cpu().numpy(), None if recv_hi is None else recv_hi.cpu().numpy(),
                               want_log=want_log)

    def round(self, n_sweeps, want_log=False, want_info=False, **outputs):
        """Sweeps, Houdayer moves, swap round of every local shard.  Returns (swap log or None, cluster info of the local shards or
        None).  `outputs` (record_stride / want_* of sweep_philox): the sweeps' outputs per local shard are left in
        self.last_outputs, with the slots the chains sat on during those sweeps in self.last_slots."""
        ii = self.rounds_done - (self._planner_round0 if self._planners else 0)
        self.last_outputs, self.last_slots = [], []
        for k, e in enumerate(self.engs):
            pl = self._planners[k] if self._planners else None
            if outputs:
                self.last_slots.append(e.pt_slots())
            if pl is not None and 0 <= ii < pl.R and n_sweeps == pl.S:
                o = pl.sweep(ii, **outputs)
            else:
                o = e.sweep_philox(n_sweeps, self.seed, sweep0=self.sweeps_done, beta=None, precision=self.precision, **outputs)
            self.last_outputs.append(o)
        self.sweeps_done += n_sweeps
        info = [e.icm_round_ladders(self.rounds_done, self.seed, self.katz, want_info=want_info) for e in self.engs]
        log = None
        if self.n_pairs > 0:
            if self.lib_collective:
                log = self.engs[0].apt_swap_collective(self.rounds_done, self.seed, self.n_pairs, want_log=want_log)
                if self._check_every and (self.rounds_done + 1) % self._check_every == 0:
                    self.engs[0].comm_check(self._timeout_ms)            # async error / lost rank -> abort, RuntimeError
            elif self.dist is not None and self.W > 1:
                log = self._swap_torch(want_log)
            elif self.W == 1:
                log = self.engs[0].apt_swap_collective(self.rounds_done, self.seed, self.n_pairs, want_log=want_log)
            else:
                packs = [e.apt_pack() for e in self.engs]
                ef_all = np.stack([p[0] for p in packs])
                for w, e in enumerate(self.engs):
                    log = e.apt_swap_host(self.rounds_done, self.seed, self.n_pairs, ef_all, packs[w - 1][2] if w > 0 else None,
                                          packs[w + 1][1] if w + 1 < self.W else None, want_log=want_log)
        self.rounds_done += 1
        return log, (info if want_info else None)

    def check(self):
        for e in self.engs:
            if self.n_pairs > 0 and hasattr(e, "pt_check"):
                e.pt_check()
        if self.lib_collective:
            self.engs[0].comm_check(self._timeout_ms)

    def close(self):
        for e in self.engs:
            e.close()
        self.engs = []


class ShardedAsLocal:
    """The slice of the LocalTempering interface NPT.run drives, over a ShardedTempering (one process per GPU, a ladder cut across
    the ranks: ONE all-gather of the energies per round).  `gather(x)`: rows of every rank's local array, in chain order."""

    def __init__(self, st):
        self.st, self.G, self.engs, self.parts, self.nmc = st, st.G, [st.eng], [(st.base, st.count)], None
        self.nmc_sweeps_done = 0

    sweeps_done = property(lambda self: self.st.sweeps_done, lambda self, v: setattr(self.st, "sweeps_done", v))
    rounds_done = property(lambda self: self.st.rounds_done)

    def configure_nmc(self, *a, **k):
        raise NotImplementedError("NMC slots under a ladder that is cut across ranks: shard whole ladders (num_restarts % ranks == 0)")

    def set_spins(self, spins_global):
        self.st.set_spins(spins_global)

    def sweeps_per_round(self, n_sweeps):
        return n_sweeps

    def plan(self, n_sweeps, n_rounds, chunk_rounds=None):
        self.st.plan(n_sweeps, n_rounds, chunk_rounds=chunk_rounds)

    def log_begin(self, n_rounds):
        self.st.eng.pt_log_begin(self.st.rounds_done, n_rounds, self.st.n_pairs)

    def round(self, n_sweeps, energy_columns=0, **outputs):
        self.st.round(n_sweeps, **outputs)
        return [self.st.last_outputs]

    def slots(self):
        return self.st.eng.pt_slots()              # the replicated table: every rank applied every decision

    def swap_log(self):
        return self.st.eng.pt_log_read()

    def gather(self, x):
        t, dist = self.st.torch, self.st.dist
        dev = "cpu" if dist.get_backend() == "gloo" else t.device("cuda", t.cuda.current_device())
        loc = t.from_numpy(np.ascontiguousarray(x)).to(dev)
        out = t.empty((self.st.world * loc.shape[0],) + tuple(loc.shape[1:]), dtype=loc.dtype, device=dev)
        dist.all_gather_into_tensor(out, loc)
        return out.cpu().numpy()

    def check(self):
        if self.st.n_pairs > 0:
            self.st.eng.pt_check()
        if self.st.lib_collective:
            self.st.eng.comm_check(self.st._timeout_ms)

    def close(self):
        self.st.eng.close()


def launcher_context():
    """(torch, torch.distributed, world, rank, local_rank) when this process is one rank of a `torch.distributed.run` job (RANK /
    WORLD_SIZE in the environment; a job of ONE rank counts: it takes the same path), else None.  The process group (backend "nccl"
    = RCCL) is brought up here if the caller has not done so; call this -- i.e. NPT.run -- before other GPU work of the process
    where possible."""
    try:
        world = int(os.environ.get("WORLD_SIZE", "1"))
    except ValueError:
        return None
    if world < 1 or "RANK" not in os.environ:
        return None
    import torch
    import torch.distributed as dist
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    return torch, dist, dist.get_world_size(), dist.get_rank(), local_rank


def all_reduce_np(torch, dist, arr):
    """Sum of a NumPy array over the ranks (read-out bookkeeping of NPT.run under a launcher); the tensor lives where the process
    group's backend wants it."""
    dev = "cpu" if dist.get_backend() == "gloo" else torch.device("cuda", torch.cuda.current_device())
    t = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
    dist.all_reduce(t)
    return t.cpu().numpy()
