/*
 * nlmc.h -- C-ABI of the MI355X-native heat-bath sweep + replica-exchange engine (libnlmc_hip.so).
 *
 * The reference (usra-riacs/Nonlocal-Monte-Carlo) is pure Python/NumPy and has NO FFI boundary of its own;
 * its boundary is the Python class surface NMC(J,h).run / NPT(J,h).run / APT_ICM(J,h).run.  The entry points
 * below are what a ctypes binding inside those classes needs to replace the reference's inner loops.  Each
 * one names the reference lines it replaces (paths relative to the reference checkout).  Plain pointers and
 * sizes only; no torch types.  All calls are blocking with respect to their host-pointer outputs and are
 * stream-ordered on the HIP stream given at creation.  One context per host thread.
 *
 * Ownership: the caller owns every host buffer for the duration of the call only; the library owns all
 * device memory until nlmc_destroy.  Errors: 0 = ok, negative = failure (text via nlmc_last_error).
 * There is NO CPU fallback: without a HIP device every compute entry point fails with NLMC_ERR_HIP.
 */
#ifndef NLMC_H
#define NLMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nlmc_ctx nlmc_ctx;

enum {
    NLMC_OK = 0,
    NLMC_ERR_ARG = -1,         /* bad argument (ValueError on the Python side) */
    NLMC_ERR_HIP = -2,         /* HIP runtime failure / no device (RuntimeError) */
    NLMC_ERR_UNSUPPORTED = -3, /* size outside what this build handles */
    NLMC_ERR_STATE = -4        /* call order violated (e.g. PT call before nlmc_pt_init) */
};

/* arithmetic of the local field in philox mode.  NLMC_F32 (4-byte couplings): J and h are held in 24-bit fixed point,
 * Jq = rint(J 2^qs) (nlmc_field_scale), the field is an exact int32 sum and the acceptance is one f32 compare with a
 * logistic threshold drawn from 32 random bits -- the chain samples the Boltzmann law of (Jq, hq) 2^-qs exactly, with
 * |Jq 2^-qs - J| <= 2^-(qs+1) (nothing is lost for +-J / integer instances).  NLMC_F64: fp64 field in the reference's
 * summation order (NMC/nmc.py:86), base-2 logistic test on a 53-bit uniform. */
enum { NLMC_F32 = 0, NLMC_F64 = 1 };
enum { NLMC_ORDER_SHARED = 0, NLMC_ORDER_PER_CHAIN = 1 }; /* one permutation per sweep for all chains | per chain */

/* phase flags, one byte per (chain, spin): caller contract of NMC/nmc.py:377-381,398-401 */
enum { NLMC_SPIN_NORMAL = 0, NLMC_SPIN_SCALED = 1, NLMC_SPIN_FROZEN_UP = 2, NLMC_SPIN_FROZEN_DOWN = 3 };

#define NLMC_LDS_N 24576    /* up to here a chain's spins live in LDS (the fast kernels); longer chains keep them in global memory:
                             * sweeps (all three modes), energies, traces, replica exchange, the Houdayer move and the backbone
                             * inference work at any size with the same results spin for spin (csrc/nlmc_big.h); only the
                             * fused windows stay with the LDS kernels (nlmc_fused_modes reports 0, sweeps run order by order) */
#define NLMC_MAX_N 16777216 /* spins per chain (32-bit positions of the schedules, counters of the level histogram) */

/* Version of this interface; nlmc_abi_version() returns the value the library was built with and the binding refuses a
 * library whose value differs.  2 (round 3): nlmc_timing_total has a fifth out-pointer and nlmc_timing_reset's argument is
 * a sampling period (both since round 2), NLMC_F32 means 24-bit fixed-point couplings + logistic thresholds, chain
 * subsets / plan slots / device-side NMC hand-offs were added. */
#define NLMC_ABI_VERSION 3

int nlmc_abi_version(void);
int nlmc_device_count(void);

/* Build a context: uploads J (CSR, both triangles, sorted columns -- what scipy.sparse.csr_matrix(J) holds at
 * NMC/nmc.py:53) and h, allocates n_chains replicas.  chain_base / n_chains_global describe this rank's shard of
 * a replica set spread over several GPUs (single GPU: 0 / n_chains).  hip_stream may be NULL (default stream).
 * Replaces: the per-call `csr_matrix(J)` + process-pool pickling of self (NMC/nmc.py:53, NPT/npt.py:616-640). */
int nlmc_create(nlmc_ctx **out, int device, void *hip_stream, int n, int64_t nnz, const int32_t *rowptr,
                const int32_t *colidx, const double *vals, const double *h, int n_chains, int chain_base,
                int n_chains_global);
void nlmc_destroy(nlmc_ctx *ctx);
const char *nlmc_last_error(const nlmc_ctx *ctx); /* ctx may be NULL: error of the last failed nlmc_create */

/* Replica state, int8 +-1 (0 allowed), layout [n_chains][n].  Replaces m_start / M[:, -1] hand-offs
 * (NMC/nmc.py:50, NPT/npt.py:612,647). */
int nlmc_set_spins(nlmc_ctx *ctx, const int8_t *spins);
int nlmc_get_spins(nlmc_ctx *ctx, int8_t *spins);

/* Phase parameterisation (NMC/nmc.py:377-381,398-401; NPT/npt.py:406-414,425,441): flags [n_chains][n] or NULL
 * to clear.  SCALED spins see (J_k,: , h_k)/temp_x, FROZEN_UP/DOWN spins see h_k = +-10000. */
int nlmc_set_flags(nlmc_ctx *ctx, const uint8_t *flags, double temp_x);

/* E = -(m^T J m/2 + m^T h) of the current state of every local chain, fp64 (NMC/nmc.py:386, NPT/npt.py:31-45,
 * 657-658).  Also re-synchronises the engine's incremental fixed-point energies. */
int nlmc_energy(nlmc_ctx *ctx, double *out /*[n_chains]*/);
/* Same, result left in device memory (for an RCCL all-gather issued by the caller). */
int nlmc_energy_dev(nlmc_ctx *ctx, double *dev_out /*[n_chains], device pointer*/);
/* The incrementally tracked energies of the current states (no recomputation), to the host. */
int nlmc_energy_tracked(nlmc_ctx *ctx, double *out /*[n_chains]*/);
/* Persistent variant: every later sweep call also stores the tracked energies of its final states there (the send
 * buffer of the per-round all-gather, NPT/npt.py:657-658 energies) -- no extra launch.  NULL switches it off. */
int nlmc_set_energy_sink(nlmc_ctx *ctx, double *dev_out /*[n_chains], device pointer or NULL*/);

/* log2 of the fixed-point scale of the incrementally tracked energies (E_tracked = integer * 2^-scale). */
int nlmc_energy_scale(const nlmc_ctx *ctx);
/* qs of the NLMC_F32 path: couplings are held as rint(J 2^qs), |Jq| < 2^23, row sums < 2^31; qs <= energy scale <= qs+29. */
int nlmc_field_scale(const nlmc_ctx *ctx);

/* Energies of an arbitrary batch of configurations (trace read-out, NPT/npt.py:685-692). */
int nlmc_energy_of(nlmc_ctx *ctx, const int8_t *spins /*[count][n]*/, int64_t count, double *out /*[count]*/);
/* fp64 energies of the configurations the most recent sweep call recorded (out_spins), computed where they still lie on
 * the device: configurations first .. first+count-1 of every chain -> out [n_chains][count].  Replaces the per-replica
 * `replica_energy(M[...], k)` loop of NPT/npt.py:685-692 without sending the trace back.  NLMC_ERR_STATE when the last
 * call recorded fewer. */
int nlmc_energy_of_recorded(nlmc_ctx *ctx, int first, int count, double *out);

/* Outputs shared by both sweep entry points (every pointer nullable):
 *   out_spins  [n_chains][ceil(n_sweeps/record_stride)][n]  state after sweeps 0, record_stride, 2*record_stride, ...
 *                                                     (M[:, ::M_skip], NMC/nmc.py:89,390)
 *   out_energy [n_chains][n_sweeps]                   energy after every sweep (NMC/nmc.py:386-387)
 *   out_min_energy [n_chains], out_argmin [n_chains]  min / first argmin over this call's sweeps (NMC/nmc.py:394)
 *   out_argmin_state [n_chains][n]                    the argmin column (NMC/nmc.py:395)
 */

/* STREAM mode: random-permutation sequential heat-bath sweeps consuming a pre-drawn legacy stream
 * (np.random.permutation(N) + N x np.random.rand() per sweep, NMC/nmc.py:71,87), fp64, update rule
 * m_k = sign(tanh(beta x_k) - 2u + 1).  Replaces MCMC(): NMC/nmc.py:28-91 == NPT/npt.py:47-110,
 * NPT/apt_ICM.py:52-93, NPT/apt_preprocessor.py:33-74.
 *   perm, u   : [n_chains][n_sweeps][n]  (i-th visited spin, i-th uniform)
 *   beta      : table of inverse temperatures, element (c, t) at beta[c*chain_stride + t*sweep_stride] */
int nlmc_sweep_stream(nlmc_ctx *ctx, int n_sweeps, const int32_t *perm, const double *u, const double *beta,
                      int chain_stride, int sweep_stride, int record_stride, int8_t *out_spins, double *out_energy,
                      double *out_min_energy, int32_t *out_argmin, int8_t *out_argmin_state);

/* PHILOX mode (throughput): same Markov kernel, counter-based RNG generated on the device.  Sweep t of the run
 * (global index sweep0 + t) visits spins in ascending order of philox(k, t, group, ORDER) and spin k of chain c
 * draws one word of philox(k>>2, t, c, UNIFORM) (f32: 32 bits -> logistic threshold; f64: its high 27 bits + the high 26 bits of the same word of philox(k>>2, t, c, UNIFORM_LO) -> 53-bit uniform); results are a pure function of (seed, global chain id, sweep index, spin) and
 * therefore independent of how chains are sharded over GPUs.
 *   beta : as above, or NULL to take each chain's beta from the PT ladder (nlmc_pt_init).
 * Four routes compute a call, with the same bits: sweep by sweep (a level schedule per order, one workgroup per chain), fused
 * windows (nlmc_plan_philox_fused; n >= 256), for chains of at most NLMC_LANE_N spins one chain per lane (nlmc_set_lane_sweeps)
 * and, for chains of at most NLMC_WAVE_N spins in NLMC_F32, one chain per wave (nlmc_set_wave_sweeps).  nlmc_last_sweep_route
 * tells which one the most recent call took. */
int nlmc_sweep_philox(nlmc_ctx *ctx, int precision, int order_mode, int n_sweeps, uint32_t sweep0, uint64_t seed,
                      const double *beta, int chain_stride, int sweep_stride, int record_stride, int8_t *out_spins,
                      double *out_energy, double *out_min_energy, int32_t *out_argmin, int8_t *out_argmin_state);

/* Chain-per-lane sweeps (csrc/nlmc_lanes.h): a wave runs 64 chains, one per lane, through the same sequential sweep in lock step, the
 * spins transposed in LDS -- no level schedule, no barrier.  Made for many chains of a short or dense instance (complete graphs of
 * 8..40 spins, Chimera-128: below the fused windows' floor, and one spin per level on a complete graph), where a workgroup per chain
 * leaves most of a compute unit idle.  mode: 0 off (the default); 1 auto -- nlmc_sweep_philox calls with n < 256 over at least
 * NLMC_LANE_AUTO_ROWS rows (chains of the call) take it; 2 force -- every nlmc_sweep_philox call with n <= NLMC_LANE_N takes it
 * (longer chains run as before: never an error).  Everything nlmc_sweep_philox accepts runs there: both precisions, both order
 * modes, phase flags, a temperature per sweep, ladder temperatures, chain subsets (shared order), the running minimum, every
 * output.  Results are bit-identical to the other routes.  nlmc_last_sweep_fused is 0 after such a call, nlmc_last_schedule_stats
 * reports the visiting orders built and 0 levels, the timings count the order kernel as the levelize half. */
#define NLMC_LANE_N 1024
/* Rows from which `auto` takes the lane route.  A measured constant: the smallest row count from which the
 * route is at least 1.2 times the sweep-by-sweep route on every instance of the measured grid in both precisions; 2147483647
 * (never) while no row count qualifies. */
#define NLMC_LANE_AUTO_ROWS 2147483647
int nlmc_set_lane_sweeps(nlmc_ctx *ctx, int mode);
/* Route of the most recent nlmc_sweep_philox call: NLMC_ROUTE_NONE before any, a call whose launches mixed routes reports
 * NLMC_ROUTE_STEPWISE. */
enum { NLMC_ROUTE_NONE = 0, NLMC_ROUTE_STEPWISE = 1, NLMC_ROUTE_FUSED = 2, NLMC_ROUTE_LANES = 3, NLMC_ROUTE_WAVES = 4 };
int nlmc_last_sweep_route(const nlmc_ctx *ctx);

/* Wave-per-chain sweeps (csrc/nlmc_waves.h): a wave owns ONE chain and keeps its local fields resident.  In NLMC_F32 the field of a
 * spin is an exact int32 whatever the order of the sum, so lane l holds the fields and spins l, l + 64, .. in registers, the decision
 * for the visited spin is a v_readlane and one compare, and a flip corrects every field by one multiply-add on a row of a dense
 * fixed-point matrix (built once per context on the first such call, freed with it; staged in LDS up to n = 192) -- no level
 * schedule, no barrier, no atomic, and the per-chain visiting order costs what the shared one costs.  Made for tens to a few
 * thousand chains of a short instance (complete graphs of 8..40 spins, Chimera-128), where a workgroup per chain runs one lane per
 * barrier round and a lane per chain walks three dependent loads per update.  mode: 0 off (the default); 1 auto --
 * nlmc_sweep_philox calls in NLMC_F32 with n <= NLMC_WAVE_N over at most NLMC_WAVE_AUTO_MAX_ROWS rows (chains of the call) take it;
 * 2 force -- every nlmc_sweep_philox call in NLMC_F32 with n <= NLMC_WAVE_N takes it.  A call it does not take (NLMC_F64, stream
 * mode, a longer chain) goes on to the lane rule and the other routes as before: never an error.  The route is asked before the
 * lane one.  Everything such a call accepts runs there: both order modes, phase flags, a temperature per sweep, ladder
 * temperatures, chain subsets (shared order), the running minimum, every output.  Results are bit-identical to the other routes.
 * nlmc_last_sweep_route is NLMC_ROUTE_WAVES and nlmc_last_sweep_fused is 0 after such a call, nlmc_last_schedule_stats reports the
 * visiting orders built and 0 levels, the timings count the order kernel as the levelize half.  The rounds entry points
 * (nlmc_pt_rounds_deferred / _lanes / _fused, nlmc_apt_rounds_lanes) do not look at this mode: rounds driven call by call get the
 * route through their sweep calls.  Environment, read at nlmc_create: NLMC_WAVE_WAVES fixes the waves (chains) per workgroup
 * (1..16; no result depends on it), NLMC_WAVE_JLDS=0 reads the matrix rows from global memory at every n. */
#define NLMC_WAVE_N 256
/* Rows up to which `auto` takes the wave route.  A measured constant: the largest measured row count such
 * that at every measured row count up to it the route is at least 1.2 times the route the call takes with every mode off, on every
 * instance of the measured grid; 0 (never) if that holds nowhere, 2147483647 if it holds at every measured row count. */
#define NLMC_WAVE_AUTO_MAX_ROWS 0
int nlmc_set_wave_sweeps(nlmc_ctx *ctx, int mode);
/* Long chains on the wave route (csrc/nlmc_waves_long.h: k_sweep_waves_long).  on != 0: the rule of nlmc_set_wave_sweeps takes chains
 * of up to NLMC_WAVE_LONG_N spins instead of NLMC_WAVE_N, the mode rules unchanged (force: every such NLMC_F32 call; auto: never while
 * NLMC_WAVE_AUTO_MAX_ROWS is 0; NLMC_F64 and stream-mode calls go on to the other routes).  For NLMC_WAVE_N < n <= NLMC_WAVE_LONG_N a
 * lane holds 8 (n <= 512) or 16 fields in registers and writes them through to a copy in LDS the wave keeps to itself beside the spins,
 * the phase flags and the sweep's thresholds (10 bytes a spin; at n = 1024 fifteen waves share a workgroup's LDS): an update is four
 * broadcast LDS reads and a compare, a flip 8 or 16 adds per lane on a row of the dense matrix, which is up to 4 MB per context
 * (n 64 R ints) and read from global memory.  Made for dense instances (complete graphs, Wishart) of a few hundred spins, where the
 * fused windows plan nothing and the other routes walk a row of n entries per update; DESIGN.md section 6 says where it pays.
 * Everything a wave call accepts runs there, bit-identical to the other routes; nlmc_last_sweep_route is NLMC_ROUTE_WAVES.  The rounds
 * inside a wave launch (nlmc_pt_rounds_waves) keep their limit of NLMC_WAVE_N spins: under nlmc_set_wave_rounds,
 * nlmc_pt_rounds_deferred runs such a context's rounds as a sweep call and a swap call each (nlmc_pt_rounds_route:
 * NLMC_ROUNDS_LAUNCH_PER_ROUND) unless nlmc_set_wave_long_rounds hands them to k_rounds_waves_long.  Default: off, and then nothing changes for any caller.  Environment, read at nlmc_create:
 * NLMC_WAVE_WAVES applies (capped by the LDS), NLMC_WAVE_LONG_AHEAD=1 requests the next visited spin's row at every update instead
 * of a row per flip (no result depends on either). */
#define NLMC_WAVE_LONG_N 1024
int nlmc_set_wave_long(nlmc_ctx *ctx, int on);

/* Optional: build and cache the level schedules of sweeps [sweep0, sweep0+n_sweeps) ahead of time (shared-order
 * philox mode).  Later nlmc_sweep_philox calls inside that range with the same seed and precision skip their
 * schedule pass. */
int nlmc_plan_philox(nlmc_ctx *ctx, int precision, int order_mode, uint32_t sweep0, int n_sweeps, uint64_t seed);
/* Fused-window schedules for n_windows consecutive launches of exactly `window` sweeps each (sweeps sweep0 + w*window
 * ...): all sweeps of a launch share one level list in which the tail of sweep t overlaps the head of sweep t+1
 * (DESIGN.md section 3).  A later nlmc_sweep_philox call with F32, shared order, n_sweeps a multiple of window, a planned
 * sweep0 (a whole number of planned windows) runs on it -- with per-sweep outputs or a temperature per sweep when the
 * snapshot slots of that variant fit in LDS; every other call takes the sweep-by-sweep path.  Results are bit-identical either way.  out_planned: number of windows that got a
 * fused schedule (0 when the instance does not qualify: n < 256 or n > 11264,
 * window < 3 or > 64, or the three threshold tables do not fit in LDS next to the spins and the flags -- 14 bytes per spin, n rounded
 * up to a multiple of 16, plus 64 within 150 KB: that bound bites first, the largest n that gets a fused schedule is 10960, and
 * 11264 is only what the planner itself could hold; a window is also left out when its
 * schedule is deeper than 1023 levels or when, in one of its sweeps, a spin has more than 255 neighbours that come before it in the
 * order -- a hub row: the levelizer counts them in eight bits).
 * A level holds at most 64 positions per worker wave of the sweep workgroup.  An update whose earliest level is full goes to the
 * next level with room (level fill; NLMC_NO_LEVEL_FILL=1, read at nlmc_create: every update keeps its earliest level and a wider
 * level is cut into consecutive levels of that width instead, which moves everything behind it one level back).  Which updates
 * are moved depends on the order in which the planner's threads reach a level, so two plans of the same window may differ by a
 * level or two in depth, as they always could in the positions inside a level; the sweeps' results depend on neither.
 * A row of up to 8 entries takes one schedule position, one of 9-16 entries two (a lane pair of the sweep kernel), one of 17-32
 * entries four (a lane quad); only what a row holds beyond 32 entries is read from the CSR arrays while the sweeps run.
 * NLMC_NO_QUADS=1, read at nlmc_create: two positions for every row beyond 8 entries, the CSR arrays beyond 16 -- same results. */
int nlmc_plan_philox_fused(nlmc_ctx *ctx, uint32_t sweep0, int n_windows, int window, uint64_t seed, int32_t *out_planned);
/* Which precisions may run on fused windows of `window` sweeps on this context: bit 0 = NLMC_F32, bit 1 = NLMC_F64.  The fp64
 * mode (the reference's arithmetic, NMC/nmc.py:86-87: fp64 field, 53-bit uniform) qualifies when every coupling AND every field
 * is an exact multiple of 2^-qs (+-J, integer and dyadic instances) with max_k (sum|Jq| + |hq|) <= 4095: its field is then the
 * exact integer X times 2^-qs, z = -2 log2(e) beta x takes one value per X, and the test fma(u, 2^z, u) < 1 of the fp64 spec is
 * monotone in the 53-bit integer of u -- one exact integer threshold per (chain, X), built in the kernel's prologue by bisection on
 * the spec's own test.  A plan is shared by both precisions.  An fp64 call with a temperature per sweep (an anneal) and no phase
 * flags in force runs on it too: the thresholds of a sweep sit in a ring of three tables, one per threshold slot, each rebuilt at
 * its next sweep's temperature, when the three tables fit in LDS and 8 (2 max_k (sum|Jq| + |hq|) + 1) <= n (the rebuilding stays
 * small next to a sweep).  With flags in force, and on real-valued instances (nlmc_set_fused_f64_real: measured slower there than
 * sweep by sweep), such a call runs sweep by sweep.  Phase flags are a property of the call, not of this answer: with flags in force the scaled rows take
 * a second threshold table at cb1, frozen rows keep their spin; where the two tables and the flags do not fit in LDS (large max_k
 * sum |Jq| + |hq| at large n) such a call runs sweep by sweep.  Bit-identical to the sweep-by-sweep fp64 kernel either way.  The
 * answer comes from the same rule the sweep and round calls follow; whether a given call ran on fused windows: nlmc_last_sweep_fused. */
int nlmc_fused_modes(nlmc_ctx *ctx, int window);
/* 1 when every launch of the most recent sweep call (nlmc_sweep_philox, nlmc_sweep_stream, nlmc_pt_rounds_fused,
 * nlmc_pt_rounds_deferred) ran on fused windows, 0 otherwise (sweep by sweep, or no such call yet). */
int nlmc_last_sweep_fused(const nlmc_ctx *ctx);
/* Opt-in (default off): the fp64 mode also runs on fused windows for REAL couplings and fields (instances that are not dyadic,
 * e.g. couplings k/75 or Gaussian ones; dyadic instances keep the integer-threshold kernel whatever this says).  Plans made while
 * it is on carry an fp64 value plane beside the entry planes, in row order; the kernel is update_spin<double> operation for
 * operation (fp64 field summed with fma in CSR order, z = cb x, fma(u, 2^z, u) < 1 decided from the 27 high bits of u where they
 * decide, from all 53 otherwise), bit-identical to the sweep-by-sweep fp64 kernel.  nlmc_fused_modes then reports bit 1 for such
 * instances; nlmc_sweep_philox(NLMC_F64) runs on it (one temperature per chain, phase flags in force or not: z = cb1 x on scaled
 * rows, frozen rows unchanged; a call with a temperature per sweep stays sweep by sweep), and so do nlmc_pt_rounds_deferred(NLMC_F64)
 * and nlmc_pt_rounds_fused(NLMC_F64) (no phase flags; the real-valued variant of k_rounds_fused reads the windows' value planes).
 * NLMC_NO_FUSED64 switches it off.  Changing the setting drops the current fused plans. */
int nlmc_set_fused_f64_real(nlmc_ctx *ctx, int on);
/* Only allocates the plan buffers for up to n_windows windows of `window` sweeps (a later nlmc_plan_philox_fused of at
 * most that size then allocates nothing).  Drops the current fused plan. */
int nlmc_plan_reserve_fused(nlmc_ctx *ctx, int n_windows, int window);

/* Measurement: the floor of ONE level-synchronous step on this device -- workgroup barrier, 8 byte gathers per lane from LDS (all in
 * flight together), sum, one LDS write, barrier: the dependent chain every level of the sweep kernels contains -- in nanoseconds per
 * round, from HIP events around `rounds` rounds of n_workgroups workgroups of `waves` waves (csrc/nlmc_probe.h).  conflict_free = 1:
 * bank-conflict-free gather addresses (the best any placement of row entries could reach), 0: random addresses as in a sweep.
 * bench.py prices the sweep kernel's levels per second against the conflict-free round. */
int nlmc_probe_level_round(nlmc_ctx *ctx, int waves, int conflict_free, int rounds, int n_workgroups, double *out_ns_per_round);

/* Diagnostic: the level list of planned window `window` of the selected plan slot, as chunk offsets (a chunk = 64 schedule
 * positions = one wave's items of one level): level l holds chunks [out[l], out[l+1]); out_n_levels levels (0: the window got
 * no fused schedule).  capacity = entries of the caller's array (>= levels + 1; 1025 always suffices). */
int nlmc_plan_get_levels(nlmc_ctx *ctx, int window, int32_t *out_level_chunk_offsets, int32_t capacity, int32_t *out_n_levels);

/* Diagnostic read-back of planned window `window` of the selected plan slot, byte for byte as the planner left it: copies on the
 * context's stream and a synchronisation, no kernel, no change of the plan (tests/schedcheck.py decodes and checks it).
 * out_info[NLMC_PLAN_INFO_WORDS] is always filled:
 *   [0] fmt (0 wide: entries { col, Jq } of 8 bytes, 4 planes; 1 compact: col << 16 | Jq & 0xFFFF, 2 planes; 2 address: 16-bit LDS
 *   addresses, 1 plane)  [1] pstride  [2] T  [3] sweep0  [4] seed  [5] workers (a level holds at most 64 workers positions)
 *   [6] quads  [7] bank_aware  [8] n_pad  [9] k_dummy  [10] k_zero  [11] neg_off  [12] tab_words  [13] nlev (0: the window got
 *   no fused schedule -- nothing else is copied then)  [14] npos  [15] hi_max  [16] has_val  [17] level_fill  [18] entry planes
 *   [19] 1 when the plan carries a head stream (nlmc_plan_get_head_stream).
 * With out_head != NULL the arrays follow, the first npos positions of each (capacity = positions the caller's arrays hold):
 *   out_head [npos][2]               { k | kind << 14 | threshold word << 16, hq_k }
 *   out_ell  [planes][npos][4]       the 16-byte entry planes, position-minor (eight row entries per position)
 *   out_val  [4][npos][2] + [npos]   the fp64 value plane and the field plane (has_val only; may be NULL otherwise)
 *   out_loff [nlev + 1]              level offsets in chunks of 64 positions (the caller's array holds 1025)
 *   out_send [T]                     published index of the last level that holds an update of sweep t (the caller's holds 64)
 * NLMC_ERR_STATE: no valid plan in the slot or no such window; NLMC_ERR_ARG: capacity < npos. */
#define NLMC_PLAN_INFO_WORDS 24
int nlmc_plan_get_items(nlmc_ctx *ctx, int window, int64_t *out_info, int32_t *out_head, int32_t *out_ell, double *out_val,
                        int32_t *out_loff, int32_t *out_send, int64_t capacity);
/* The head stream of the same window, in the plans that carry one (out_info[19]; NLMC_ERR_STATE otherwise): the plans of a context
 * whose launches can read it -- an instance without a field term, 2- or 4-byte entries, NLMC_NO_HEAD_STREAM unset; no other context
 * reserves its memory (ceil(1024 / 4) x workers KB per window) or has the planner write it.  There the planner writes the first head word of every item a second time, in the order the worker
 * waves of the sweep workgroup read it.  out_hs [ceil(nlev / 4)][workers][64][4] int32 (workers = out_info[5] of
 * nlmc_plan_get_items): element [l / 4][w][lane][l % 4] is head.x of the item that lane `lane` of worker wave w executes in published
 * level l, i.e. of schedule position 64 (loff[l] + w) + lane.  Elements of chunks a level does not have (w >= loff[l + 1] - loff[l])
 * and of levels >= nlev are not defined.  capacity: int32 elements out_hs holds.  A plain fused launch (no per-sweep outputs, not the
 * real-valued fp64 variant) of an instance without a field term -- every h rounds to 0 on the fixed-point grid -- whose plan has 2-
 * or 4-byte entries (fmt 1 or 2) reads its heads from this stream: one 16-byte load per four levels instead of an 8-byte load per level.  NLMC_NO_HEAD_STREAM=1, read at nlmc_create,
 * keeps the per-level loads (same results; for A/B measurements and tests). */
int nlmc_plan_get_head_stream(nlmc_ctx *ctx, int window, int32_t *out_hs, int64_t capacity);
/* Where the most recent launch on fused windows (nlmc_sweep_philox on a plan, nlmc_pt_rounds_fused, nlmc_pt_rounds_deferred) read its
 * item heads: NLMC_HEADS_LOADS (head[], a load per level), NLMC_HEADS_STREAM (the head stream), or 0 (no such launch yet). */
#define NLMC_HEADS_LOADS 1
#define NLMC_HEADS_STREAM 2
int nlmc_last_head_path(nlmc_ctx *ctx);
/* The same for order `order` of the per-sweep plan (nlmc_plan_philox).  out_info[8]: [0] n  [1] nlev  [2] hi_max  [3] 1 when the
 * global-memory levelizer built the plan (items { k, row start }; { k | degree << 16, row start } otherwise)  [4] the widest level
 * the planner publishes (0: no cap in force)  [5] orders planned  [6] sweep0.  out_order [n][2], out_lvl_off [nlev + 1 <= n + 1];
 * capacity = spins the caller's arrays hold (out_lvl_off: capacity + 1 entries).  Errors as above (NLMC_ERR_ARG: capacity < n). */
int nlmc_plan_get_order(nlmc_ctx *ctx, int order, int64_t *out_info, int32_t *out_order, int32_t *out_lvl_off, int64_t capacity);

/* Is librccl loadable in this process (NLMC_OK), or why not (NLMC_ERR_UNSUPPORTED + nlmc_last_error(NULL))?  Every rank asks
 * BEFORE nlmc_comm_init and the ranks agree on the answer over the process group that is already up, so that no rank waits in
 * ncclCommInitRank for one that could not load the library. */
int nlmc_comm_probe(void);
/* Asynchronous failures of the library-issued collectives: ncclCommGetAsyncError, then (timeout_ms >= 0) a BOUNDED wait for the work
 * queued on the context's stream.  On an error or a timeout (a lost rank leaves the others inside a collective for ever) the
 * communicator is aborted with ncclCommAbort, the context drops it, and the call returns NLMC_ERR_HIP: the caller exits non-zero
 * ("RCCL async error -> abort").  timeout_ms < 0: the error flag only, no wait.  NLMC_OK without a communicator. */
int nlmc_comm_check(nlmc_ctx *ctx, int timeout_ms);

/* ---- APT + iso-cluster moves with the temperature ladder cut into SLOT blocks, one per GPU (NPT/apt_ICM.py:215-285; SURVEY.md
 * section 8e: "keep all sub-replicas of a beta on the same GPU").  Rank w of `world` creates a SELF-CONTAINED context of K ladders
 * (sub-replicas) x Rw local slots (chain_base 0, n_chains_global == n_chains = K Rw, nlmc_pt_init with ITS block
 * beta_global[w Rw .. (w+1) Rw)) and declares it shard w of a global ladder of R_global = world Rw slots:
 *   - random numbers of the sweeps, of the Houdayer pairing and of the cluster pick are keyed by (ladder, GLOBAL slot) instead of by
 *     chain, so exchanging two chains' labels and exchanging their configurations are the same step of the Markov chain;
 *   - nlmc_pt_plan plans the pair selections of the GLOBAL ladder (every rank the same ones);
 *   - nlmc_sweep_philox(beta = NULL), nlmc_icm_round_ladders work on the block as on any context;
 *   - the swap round is nlmc_apt_swap_collective (one process per GPU: the library issues ONE ncclAllGather of K Rw int64 tracked
 *     energies per rank and ONE grouped ncclSend/ncclRecv of the K boundary configurations with each neighbour, on the kernels'
 *     stream) or nlmc_apt_pack + nlmc_apt_swap_host (one process driving several contexts; the same data through host memory):
 *     pairs inside a block are label exchanges, an accepted pair across a block boundary moves the two configurations.
 * The states on every (ladder, global slot) are bit-identical for any `world` (world = 1 included). */
int nlmc_apt_shard(nlmc_ctx *ctx, int R_global, int world, int rank, const double *beta_global /*[R_global]*/);
/* Tracked energies by (ladder, local slot) in units of 2^-escale -> out_slot_efix [K][Rw]; the configurations on local slot 0 /
 * Rw - 1 of every ladder -> out_lo / out_hi [K][n] (any of the three may be NULL). */
int nlmc_apt_pack(nlmc_ctx *ctx, int64_t *out_slot_efix, int8_t *out_lo, int8_t *out_hi);
/* efix_all [world][K][Rw]: every rank's nlmc_apt_pack energies; recv_lo = rank - 1's out_hi, recv_hi = rank + 1's out_lo (NULL at the
 * ends of the ladder).  out_pairs [K][n_pairs][2] GLOBAL slots, out_accepted [K][n_pairs]: the full log, identical on every rank. */
int nlmc_apt_swap_host(nlmc_ctx *ctx, uint32_t round, uint64_t seed, int n_pairs, const int64_t *efix_all, const int8_t *recv_lo,
                       const int8_t *recv_hi, int32_t *out_pairs, uint8_t *out_accepted);
int nlmc_apt_swap_collective(nlmc_ctx *ctx, uint32_t round, uint64_t seed, int n_pairs, int32_t *out_pairs, uint8_t *out_accepted);
/* Rehearsal of the collective path's neighbour exchange with ONE rank: the same grouped ncclSend / ncclRecv pair with this rank as its
 * own lower and upper neighbour; out_recv_lo [K][n] must then equal the packed top-slot configurations (nlmc_apt_pack: out_hi),
 * out_recv_hi the bottom-slot ones.  (N > 1 ranks on one GPU are refused by RCCL: this is what a one-GPU box can execute of it.) */
int nlmc_apt_selftest_exchange(nlmc_ctx *ctx, int8_t *out_recv_lo, int8_t *out_recv_hi);

/* Replica exchange (NPT/npt.py:602-683).  Chains are grouped into ladders of ladder_len consecutive global
 * chain ids; slot r of a ladder runs at beta_list[r].  Accepted swaps exchange the beta slots of two chains
 * (label exchange) -- equivalent to the reference's exchange of the two N-blocks of m_start (NPT/npt.py:677-678). */
int nlmc_pt_init(nlmc_ctx *ctx, int ladder_len, const double *beta_list /*[ladder_len]*/);
int nlmc_pt_get_slots(nlmc_ctx *ctx, int32_t *slot_of_chain /*[n_chains_global]*/);
int nlmc_pt_set_slots(nlmc_ctx *ctx, const int32_t *slot_of_chain /*[n_chains_global]*/);
/* Host-decided swaps (numpy-stream mode: select_non_overlapping_pairs + np.random.rand() stay in Python,
 * NPT/npt.py:514-533,668-671): exchange slots a and b (0-based) of ladder `ladder`. */
int nlmc_pt_apply_swap(nlmc_ctx *ctx, int ladder, int slot_a, int slot_b);
/* Device-decided round: pair selection with the law of NPT/npt.py:514-533 and Metropolis acceptance
 * u < min(1, exp(dBeta*dE)) (NPT/npt.py:668-671), Philox-keyed by (seed, round, ladder).
 *   energies_all_dev: device pointer [n_chains_global] (after the caller's all-gather) or NULL = this context's
 *   own current energies: the single-GPU case, and any context whose block of chains consists of WHOLE ladders -- it then
 *   decides its own ladders only (same keys, same bits as the context that holds every chain), other ladders' rows of the log
 *   read "no pair" (-1, not accepted) and its copy of their slot maps is not advanced.  A block that cuts a ladder needs the
 *   gathered energies.  out_pairs [n_ladders][n_pairs][2] slots, out_accepted [n_ladders][n_pairs]. */
int nlmc_pt_swap_philox(nlmc_ctx *ctx, uint32_t round, uint64_t seed, int n_pairs, const double *energies_all_dev,
                        int32_t *out_pairs, uint8_t *out_accepted);
/* Same round with the all-gathered energies handed over in HOST memory (several contexts driven by one process,
 * NPT.run(device_ids=...): no device-to-device path is assumed between them). */
int nlmc_pt_swap_philox_host(nlmc_ctx *ctx, uint32_t round, uint64_t seed, int n_pairs, const double *energies_all_host,
                             int32_t *out_pairs, uint8_t *out_accepted);
/* Replica-sharded ladders, one process per GPU (NPT/npt.py:616-640 hands one task per replica to a process pool): the ONE
 * collective of a round -- an all-gather of every rank's chain energies -- issued BY THE LIBRARY with RCCL on the stream its
 * kernels run on (librccl is bound at run time; the copy the process already holds is reused).  With a communicator in place
 * the sweep kernels write their chains' energies straight into this rank's block of the gathered vector.
 *   nlmc_comm_unique_id   rank 0 creates the id (128 bytes) and hands it to the others over whatever channel the launcher
 *                         has (torch.distributed broadcast in distributed.ShardedTempering)
 *   nlmc_comm_init        every rank; the context must own block `rank` of `world` equal blocks of chains
 *   nlmc_pt_swap_philox_collective   all-gather + the device-decided swap round of nlmc_pt_swap_philox on the gathered
 *                         energies (identical decision on every rank).  refresh_energies != 0: publish the tracked energies
 *                         first (needed when the states changed other than through a sweep call since the last round). */
int nlmc_comm_unique_id(uint8_t *out_id /*[128]*/);
int nlmc_comm_init(nlmc_ctx *ctx, const uint8_t *id /*[128]*/, int world, int rank);
int nlmc_pt_swap_philox_collective(nlmc_ctx *ctx, uint32_t round, uint64_t seed, int n_pairs, int refresh_energies,
                                   int32_t *out_pairs, uint8_t *out_accepted);
/* Optional: the pair selection depends on the RNG only, so the selections of rounds [round0, round0+n_rounds) can be
 * computed ahead of time (one wave per round and ladder).  Later nlmc_pt_swap_philox calls in that range with the same
 * seed and n_pairs are left with the parallel acceptance test.  Results are identical with or without a plan. */
int nlmc_pt_plan(nlmc_ctx *ctx, uint32_t round0, int n_rounds, uint64_t seed, int n_pairs);
/* n_rounds whole rounds -- sweeps_per_round sweeps of every chain at its ladder temperature, then the swap round of
 * nlmc_pt_swap_philox -- in cooperative launches of k_rounds_fused (one per 1024 rounds): the chains stay in LDS from round to
 * round; between two rounds every chain publishes its tracked energy in a record of (round, ladder, slot), a chain whose slot is in
 * a selected pair waits for the partner slot's record of the same round (bounded wait) and both take the identical decision, a
 * chain in no pair waits for nobody; the slot maps are written at the end of a launch.  Bit-identical to nlmc_sweep_philox(beta =
 * NULL) + nlmc_pt_swap_philox round by round (the rounds' decisions go to the device-side swap log when one is open); what a launch
 * per round pays again and again (kernel launches, spins HBM -> LDS -> HBM, the random tables of a round's first two sweeps, the
 * fp64 mode's threshold tables of a chain that kept its slot) is paid once per launch.  Needs: a fused-window plan of ONE window per
 * round covering sweeps [sweep0, sweep0 + n_rounds sweeps_per_round) (nlmc_plan_philox_fused, window == sweeps_per_round), the pair
 * selections of rounds [round0, round0 + n_rounds) planned (nlmc_pt_plan, same seed and n_pairs), a context of whole ladders without
 * a communicator, no phase flags / chain subset, one workgroup per chain resident at once (n_chains <= CUs for large n).  All three
 * arithmetics: fixed point, the fp64 mode's integer thresholds (dyadic instances) and, with nlmc_set_fused_f64_real on and plans made
 * since, the fp64 mode on real couplings and fields (no K tables: the launch's LDS is the fixed-point mode's; without the option such
 * an instance is refused: the fp64 mode does not run on fused windows for it).
 * NLMC_ERR_UNSUPPORTED (nothing was run) when a condition is not met: the caller runs the rounds one by one.  Asynchronous: a wait
 * that times out is reported by nlmc_pt_check / nlmc_pt_log_read (NLMC_ERR_HIP). */
int nlmc_pt_rounds_fused(nlmc_ctx *ctx, int precision, int n_rounds, int sweeps_per_round, uint32_t sweep0, uint32_t round0,
                         uint64_t seed, int n_pairs);
/* The same n_rounds rounds on the route that fits the context (n_pairs >= 1, no tracked minimum; otherwise nlmc_pt_rounds_fused's
 * conditions and NLMC_ERR_UNSUPPORTED convention, residency apart).  Where k_rounds_fused can hold all chains at once the rounds run
 * inside its launches as above (NLMC_NO_PERSISTENT=1 at nlmc_create switches that off) -- except for real-valued fp64 instances
 * (nlmc_set_fused_f64_real), which keep a launch per round here by default: the in-launch route is taken by default only where it was measured faster beyond the
 * run-to-run spread, and for the real-valued variant that measurement is still open; nlmc_pt_rounds_fused reaches the
 * kernel.  Otherwise n_rounds sweep launches + ONE
 * swap launch: the sweep launch of round i decides the swap of round i - 1 in its prologue (every chain looks up its pair, reads its
 * partner's energy as the previous launch published it, takes k_pt_swap's decision and updates its own entries of the slot maps;
 * wave 0 does it while the other waves load the spins), the last round's swap is the ordinary kernel.  Bit-identical to
 * nlmc_sweep_philox + nlmc_pt_swap_philox round by round on either route. */
int nlmc_pt_rounds_deferred(nlmc_ctx *ctx, int precision, int n_rounds, int sweeps_per_round, uint32_t sweep0, uint32_t round0,
                            uint64_t seed, int n_pairs);
/* The same n_rounds rounds of short chains in launches of k_rounds_lanes (csrc/nlmc_lane_rounds.h), whatever the lane mode is: a lane
 * owns a chain as in the chain-per-lane sweeps, a wave holds 64 / ladder_len whole ladders, the spins stay transposed in LDS for the
 * whole launch, and a swap round stays inside the wave -- lane p of a ladder decides selected pair p from the two energies the wave
 * shuffles to it, chains keep their lanes and two byte maps in LDS exchange entries.  No wave waits for another one (no barrier, no
 * atomic, no cooperative launch, no residency condition).  Bit-identical to nlmc_sweep_philox(beta = NULL, shared order) +
 * nlmc_pt_swap_philox round by round on any route; the rounds' decisions go to the device-side swap log when one covers them.  Needs:
 * n <= NLMC_LANE_N, ladder_len <= 64, a context of whole ladders without a communicator, no phase flags / chain subset / second stream /
 * tracked minimum, n_pairs >= 1 with the pair selections of rounds [round0, round0 + n_rounds) planned (nlmc_pt_plan, same seed and
 * n_pairs); no fused-window plan.  The visiting orders of as many rounds as the order scratch holds are built per launch (a call is
 * cut into launches of whole rounds; one round's orders must fit).  NLMC_ERR_UNSUPPORTED (nothing was run, the reason in
 * nlmc_last_error) when a condition is not met.  nlmc_pt_rounds_deferred takes this route first, before it asks for a fused plan,
 * when nlmc_set_lane_sweeps routes the context's sweeps to the lane kernels (today: mode 2, force) and the conditions hold; with
 * the lane mode off it behaves as it always did.  nlmc_last_sweep_route is NLMC_ROUTE_LANES after such a call, nlmc_last_schedule_stats
 * reports the visiting orders built, the timings count the order kernel as the levelize half. */
int nlmc_pt_rounds_lanes(nlmc_ctx *ctx, int precision, int n_rounds, int sweeps_per_round, uint32_t sweep0, uint32_t round0,
                         uint64_t seed, int n_pairs);
/* n_rounds whole rounds of short chains in launches of k_rounds_waves (csrc/nlmc_wave_rounds.h), whatever the wave mode is: a chain
 * per wave with its exact int32 local fields resident in registers (k_sweep_waves' update), a workgroup of up to 16 waves holding
 * whole ladders (up to 64 chains: a wave then runs up to four chains in turn, their state parked in LDS between turns), the field
 * prologue and the staging of the coupling matrix into LDS paid once per launch, the swap round decided by the workgroup's first wave
 * from energies in LDS between two workgroup barriers.  No workgroup waits for another one (no atomic, no cooperative launch, no
 * residency condition).  Bit-identical to nlmc_sweep_philox(beta = NULL, shared order) + nlmc_pt_swap_philox round by round on any
 * route; the rounds' decisions go to the device-side swap log when one covers them, an open best-state record and energy log observe
 * every chain once per round.  Needs: precision NLMC_F32, n <= NLMC_WAVE_N, ladder_len <= 64, a context of whole ladders without a
 * communicator, no phase flags / chain subset / second stream / tracked minimum, n_pairs >= 1 with the pair selections of rounds
 * [round0, round0 + n_rounds) planned (nlmc_pt_plan, same seed and n_pairs); no fused-window plan.  A call is cut into launches of
 * whole rounds against the order scratch as nlmc_pt_rounds_lanes' is.  NLMC_ERR_UNSUPPORTED (nothing was run, the reason in
 * nlmc_last_error) when a condition is not met.  NLMC_WAVE_ROUNDS_LADDERS (read at nlmc_create) fixes the ladders per workgroup; no
 * result depends on it.  nlmc_last_sweep_route is NLMC_ROUTE_WAVES after such a call, nlmc_pt_rounds_route NLMC_ROUNDS_WAVES,
 * nlmc_last_schedule_stats reports the visiting orders built. */
int nlmc_pt_rounds_waves(nlmc_ctx *ctx, int precision, int n_rounds, int sweeps_per_round, uint32_t sweep0, uint32_t round0,
                         uint64_t seed, int n_pairs);
/* on != 0: nlmc_pt_rounds_deferred takes k_rounds_waves first -- before the lane rule and before it asks for a fused plan -- when
 * nlmc_set_wave_sweeps routes the context's sweeps to the wave kernels and nlmc_pt_rounds_waves' conditions hold; where they do not
 * the call goes on as with the option off.  Default: off, and then nothing changes for any caller. */
int nlmc_set_wave_rounds(nlmc_ctx *ctx, int on);
/* n_rounds whole rounds of dense chains of NLMC_WAVE_N < n <= NLMC_WAVE_LONG_N spins in launches of k_rounds_waves_long
 * (csrc/nlmc_wave_long_rounds.h), whatever the wave mode is: the frame of k_rounds_waves around the update of k_sweep_waves_long.  A
 * chain's int32 local fields are built once per launch and stay in LDS across the swap rounds (a swap is a label exchange: the spins
 * never move), where a sweep call and a swap call per round rebuild them from n rows of the dense matrix every round.  A workgroup of
 * up to 16 waves holds whole ladders, as many as have their regions (4 KB of fields at n > 512, 2 KB below, and n_pad bytes of spins a
 * chain; the thresholds of a sweep a wave) in its LDS; a ladder of more than 16 temperatures has the workgroup to itself and its waves
 * run chains in turn.  No workgroup waits for another one.  Bit-identical to nlmc_sweep_philox(beta = NULL, shared order) +
 * nlmc_pt_swap_philox round by round on any route; swap log, best-state record and energy log as in nlmc_pt_rounds_waves.  Needs what
 * nlmc_pt_rounds_waves needs with NLMC_WAVE_N < n <= NLMC_WAVE_LONG_N in place of n <= NLMC_WAVE_N, and one ladder's regions inside
 * a workgroup's LDS (n = 1024: up to 22 temperatures; n = 513: 28; n = 512: 52; n = 300: 60).  NLMC_ERR_UNSUPPORTED (nothing was run,
 * the reason in nlmc_last_error) when a condition is not met.  NLMC_WAVE_ROUNDS_LADDERS applies as it does there, capped by the LDS; no
 * result depends on it.  nlmc_last_sweep_route is NLMC_ROUTE_WAVES after such a call, nlmc_pt_rounds_route NLMC_ROUNDS_WAVES_LONG,
 * nlmc_last_schedule_stats reports the visiting orders built. */
int nlmc_pt_rounds_waves_long(nlmc_ctx *ctx, int precision, int n_rounds, int sweeps_per_round, uint32_t sweep0, uint32_t round0,
                              uint64_t seed, int n_pairs);
/* on != 0: with nlmc_set_wave_rounds and nlmc_set_wave_long both on, nlmc_pt_rounds_deferred takes k_rounds_waves_long for chains of
 * more than NLMC_WAVE_N spins where nlmc_set_wave_sweeps routes the context's sweeps to the wave kernels and
 * nlmc_pt_rounds_waves_long's conditions hold; where they do not the call goes on as with the option off (a sweep call and a swap call
 * per round).  Default: off, and then nothing changes for any caller. */
int nlmc_set_wave_long_rounds(nlmc_ctx *ctx, int on);
/* The route the most recent nlmc_pt_rounds_fused / nlmc_pt_rounds_deferred / nlmc_pt_rounds_lanes / nlmc_pt_rounds_waves /
 * nlmc_pt_rounds_waves_long call that ran took: NLMC_ROUNDS_IN_LAUNCH (the rounds inside k_rounds_fused launches),
 * NLMC_ROUNDS_LAUNCH_PER_ROUND, NLMC_ROUNDS_LANES (inside k_rounds_lanes launches), NLMC_ROUNDS_APT_LANES (nlmc_apt_rounds_lanes),
 * NLMC_ROUNDS_WAVES (inside k_rounds_waves launches), NLMC_ROUNDS_WAVES_LONG (inside k_rounds_waves_long launches), or 0 (no such
 * call yet). */
#define NLMC_ROUNDS_IN_LAUNCH 1
#define NLMC_ROUNDS_LAUNCH_PER_ROUND 2
#define NLMC_ROUNDS_LANES 3
#define NLMC_ROUNDS_APT_LANES (NLMC_ROUNDS_LANES + 1) /* 4 */
#define NLMC_ROUNDS_WAVES (NLMC_ROUNDS_LANES + 2) /* 5 */
#define NLMC_ROUNDS_WAVES_LONG (NLMC_ROUNDS_LANES + 3) /* 6 */
int nlmc_pt_rounds_route(nlmc_ctx *ctx);
/* n_rounds APT rounds of short chains -- sweeps_per_round sweeps at the slot temperatures, the Houdayer step of
 * nlmc_icm_round_ladders, the swap round of nlmc_pt_swap_philox -- in launches of k_apt_rounds_lanes (csrc/nlmc_lane_apt.h): the whole
 * system, K = n_chains / ladder_len sub-replica ladders, in ONE workgroup (nlmc_apt_systems(M): M systems of K = n_ladders / M, a
 * workgroup each, out_info [n_rounds][M][ladder_len * (K / 2)][2]).  A lane owns a chain, wave w holds ladders w P .. w P + P - 1
 * (P = 64 / ladder_len) transposed in a region of LDS of its own, sweeps and swaps stay inside the wave as in k_rounds_lanes; around the
 * Houdayer step the waves meet at a barrier, every chain ranks its ladder among the pairing keys of its slot, and a lane owns a PAIR:
 * components of the disagreement graph by label passes over wave-uniform rows (csrc/nlmc_lane_icm.h, labels in LDS, no atomic), the pick,
 * the Katzgraber flip or the exchange, and k_icm_round's integer energy deltas.  Round r of the call uses sweeps sweep0 + r
 * sweeps_per_round .., Houdayer round round0 + r and swap round round0 + r.  Bit-identical to nlmc_sweep_philox(beta = NULL, shared
 * order) + nlmc_icm_round_ladders + nlmc_pt_swap_philox round by round on any route; swap decisions go to the device-side log when one
 * covers the rounds.  out_info [n_rounds][ladder_len * (K / 2)][2] = {n_components, picked size} per round and pair ({0, 0} where nothing
 * disagrees), nullable; reading it back synchronises the stream and reports a component search that did not converge (NLMC_ERR_STATE),
 * as nlmc_icm_round_ladders does.  Needs nlmc_pt_rounds_lanes' conditions, except that n_pairs = 0 (rounds without swaps) is taken, and:
 * the context holds the whole system (chain_base = 0, all chains), random numbers are keyed by chain (no nlmc_apt_shard), the system fits
 * 16 waves (ceil(K / P) <= 16), and spins + maps + labels fit 150 KB of LDS (64 n_pad bytes per wave + 2 n ladder_len (K / 2) bytes of
 * labels + under 2 KB; the waves' random-number tables share the labels' bytes where they fit too, NLMC_LANE_RNG = 0 leaves them out).
 * NLMC_ERR_UNSUPPORTED (nothing was run, the reason in nlmc_last_error) otherwise.  Afterwards nlmc_last_sweep_route is
 * NLMC_ROUTE_LANES, nlmc_pt_rounds_route NLMC_ROUNDS_APT_LANES, nlmc_last_schedule_stats reports the visiting orders built (as many
 * rounds' orders per launch as the order scratch holds: a call is cut into launches of whole rounds). */
int nlmc_apt_rounds_lanes(nlmc_ctx *ctx, int precision, int n_rounds, int sweeps_per_round, uint32_t sweep0, uint32_t round0,
                          uint64_t seed, int n_pairs, int katzgraber, int32_t *out_info);
/* A context of n_ladders = M K ladders (nlmc_pt_init) as M = n_systems independent APT systems -- restarts side by side.  System s owns
 * ladders s K .. s K + K - 1, hence chains s K L .. (s + 1) K L - 1.  Only the Houdayer pairing changes: per system s and slot r the K
 * ladders of THAT system are ordered by the keys philox(j, round, r, ICM_PAIR), j the global ladder id, ties to the smaller j; ranks 2 i
 * and 2 i + 1 form pair i, an odd K leaves the last rank out.  Pairs and info rows are listed in the order (system, slot, i): M L (K / 2)
 * rows where the calls below say ladder_len * (K / 2).  Sweeps, the pick of a pair and the energy deltas stay keyed by global chain ids,
 * pair selections and swap decisions by global ladder, the visiting order is shared: system 0 has exactly the bits of a one-system
 * context of K L chains with the same seed, the other systems are independent runs.  nlmc_icm_round_ladders pairs by system on all of
 * its kernels; nlmc_apt_rounds_lanes launches a workgroup per system (its 16-wave and 150 KB limits are those of ONE system; no
 * workgroup reads what another writes, so M may exceed the number of compute units).  NLMC_ERR_STATE before nlmc_pt_init; NLMC_ERR_ARG
 * for n_systems < 1 or n_ladders % n_systems != 0; NLMC_ERR_UNSUPPORTED for n_systems > 1 on a context of nlmc_apt_shard (slot-keyed
 * random numbers), as nlmc_apt_shard is on a context of several systems.  nlmc_pt_init resets it to 1. */
int nlmc_apt_systems(nlmc_ctx *ctx, int n_systems);
/* Device-side swap log of rounds [round0, round0 + n_rounds): rounds of nlmc_pt_swap_philox(_host) called WITHOUT host
 * output pointers keep their pairs and decisions on the device; nlmc_pt_log_read copies the whole log in one go
 * (out_pairs [n_rounds][n_ladders][n_pairs][2], -1 where a round did not run; out_accepted [n_rounds][n_ladders][n_pairs])
 * and reports pair exhaustion like nlmc_pt_check.  Replaces the reference's per-round prints (NPT/npt.py:662-674). */
int nlmc_pt_log_begin(nlmc_ctx *ctx, uint32_t round0, int n_rounds, int n_pairs);
int nlmc_pt_log_read(nlmc_ctx *ctx, int32_t *out_pairs, uint8_t *out_accepted);
/* NLMC_ERR_ARG ("Cannot find non-overlapping pairs.", the reference's ValueError of NPT/npt.py:526) if the greedy
 * selection of any device-decided round since the last check ran out of pairs; such a round attempts no swap.  Rounds
 * that return their log, and planned rounds (at nlmc_pt_plan time), report it themselves; call this after a run of
 * unplanned rounds without logs.  One stream synchronisation. */
int nlmc_pt_check(nlmc_ctx *ctx);

/* ---- replica-exchange rounds whose marked temperature slots run NMC cycles, device-resident -------------------------
 * NPT.run submits NMC_task (NPT/npt.py:479-512 -> NMC_subroutine :357-477) instead of MCMC_task for the replicas whose
 * doNMC entry is set (NPT/npt.py:622-647); doNMC belongs to the temperature SLOT.  With label-exchange swaps the chains
 * that sit on marked slots change from round to round, so a round is driven on chain SUBSETS:
 *   nlmc_pt_mark_slots(marks)             marks [ladder_len] = doNMC; every ladder must lie inside one context
 *   nlmc_select_chains(UNMARKED | MARKED) later nlmc_sweep_philox / nlmc_adopt_best / nlmc_backbone_clusters /
 *                                         nlmc_set_phase calls act on the local chains currently on such slots (ascending
 *                                         chain id; the list is rebuilt on the device after every swap round); sweep
 *                                         outputs then have one row per chain of the subset (nlmc_subset_count,
 *                                         nlmc_get_subset), per-chain beta tables are refused (ladder or one beta)
 * One NMC_task of all marked chains at once, without a host round trip:
 *   nlmc_backbone_clusters   LBP_convexified (NPT/npt.py:397-403, :129-202) seeded with each chain's current state, then the
 *                            union of find_clusters' clusters (NPT/npt.py:294-355) as a per-chain mask: thresholds[0] =
 *                            threshold_initial selects the seeds, every further entry is one growth step (the host's
 *                            `current_threshold -= threshold_step` values above threshold_cutoff)
 *   nlmc_set_phase(kind, temp_x)   per-spin flags of the subset from its masks: BACKBONE_HOT = cluster rows / temp_x, the
 *                            rest frozen (NPT/npt.py:406-414,425); BACKBONE_FROZEN = cluster spins frozen (:441); ALL =
 *                            plain (:460)
 *   nlmc_track_minimum(1)    sweep calls keep the running minimum + argmin configuration of every chain on the device
 *   nlmc_adopt_best          the argmin configuration becomes the current state, its energy the tracked energy
 *                            (NPT/npt.py:436-437,454-455,469-470: `m_init = M[:, min_energy_idx]`)
 *   nlmc_backbone_check      NLMC_ERR_ARG with the reference's message if an inference since the last check diverged at its
 *                            first lambda (NPT/npt.py:178-180 raises ValueError at once; here it surfaces at the check).
 * nlmc_get_cluster_mask: [n_chains][n] masks of the most recent inference of every chain (tests, diagnostics). */
enum { NLMC_CHAINS_ALL = 0, NLMC_CHAINS_UNMARKED = 1, NLMC_CHAINS_MARKED = 2 };
enum { NLMC_PHASE_ALL = 0, NLMC_PHASE_BACKBONE_HOT = 1, NLMC_PHASE_BACKBONE_FROZEN = 2 };
int nlmc_pt_mark_slots(nlmc_ctx *ctx, const uint8_t *marks /*[ladder_len] or NULL*/);
int nlmc_select_chains(nlmc_ctx *ctx, int which);
/* on != 0: the work of the MARKED subset (inference, phases, hand-offs) is queued on a second HIP stream of the context, forked
 * from the context's stream where a round first selects a subset and joined where it selects all chains again, so that the
 * unmarked chains' sweeps (select UNMARKED first) run beside it -- the reference's pool runs MCMC_task and NMC_task side by
 * side too (NPT/npt.py:616-640).  Same results either way. */
int nlmc_overlap_subsets(nlmc_ctx *ctx, int on);
/* From now on the context queues its work on a non-blocking HIP stream of its own (created here, destroyed with the context)
 * instead of the stream given at creation.  For several contexts on ONE device driven by one process (distributed.LocalTempering
 * with repeated device ids): contexts that were all created on the NULL stream execute one after the other; with a stream each
 * they share the chip -- the reference's knob for this is the pool of num_cores workers, NPT/npt.py:616-640.  Call it right
 * after nlmc_create (pending work of the old stream is waited for), before nlmc_comm_init. */
int nlmc_own_stream(nlmc_ctx *ctx);
int nlmc_subset_count(const nlmc_ctx *ctx);
int nlmc_get_subset(nlmc_ctx *ctx, int32_t *out_chains /*[nlmc_subset_count] local chain ids*/);
/* on = 0: off; 1: the running minimum looks at every sweep of a call; k > 1: at sweeps 0, k, 2k, ... only -- the reference takes its
 * argmin over the recorded columns M[:, ::M_skip] (NMC/nmc.py:390-395 == NPT/npt.py:434-437). */
int nlmc_track_minimum(nlmc_ctx *ctx, int on);
/* ---- run-long best-state record: the lowest-energy configuration every chain visited, and when -------------------------------
 * nlmc_track_minimum is a per-call minimum (the NMC phase hand-off); NPT.run's read-out looks at the last round only.  This record
 * lasts from nlmc_best_begin to nlmc_best_end, over any number of calls, and only observes: no call's results change while it is open.
 * Per local chain: the lowest tracked energy seen (an integer of 2^-nlmc_energy_scale), the stamp of the observation that FIRST reached
 * it and the chain's spins at that observation, and the stamp of the first observation whose energy was <= target (first passage).
 * One observation of chain c at stamp s with tracked energy E: E < best (strict) replaces energy, stamp and state; first_hit < 0 and
 * E <= target sets first_hit = s.  Both compares are made on the energies as nlmc_energy_tracked reports them ((double) integer 2^-scale:
 * the integer compare while |integer| < 2^53), so a host that keeps its own running minimum over nlmc_energy_tracked sees the same
 * record; it is a function of the observed (state, energy) pairs and has the same bits on every route.
 *   nlmc_best_begin(target)  opens or resets the record (energy: none, stamps -1); target = NaN: no first-passage stamp.  The device
 *                            buffers (8 + 4 + 4 + n bytes per chain) are allocated at the first begin and kept.
 *   nlmc_best_update(stamp)  one observation of every local chain's CURRENT state (k_best_update: a workgroup per chain on the state
 *                            arrays, any n), queued on the context's stream, asynchronous.  stamp < 2^31.  Needs all chains selected
 *                            (NLMC_ERR_UNSUPPORTED under a chain subset).  For drivers that run a round call by call: after the
 *                            sweeps, before the swap round (APT: again after nlmc_icm_round_ladders, which lowers one partner's energy).
 *   nlmc_best_read           energies as nlmc_energy_tracked reports them (+inf for a chain never observed), stamps, first-passage
 *                            stamps (-1: never), states [n_chains][n]; every pointer nullable; one stream synchronisation.  Also after
 *                            nlmc_best_end.
 *   nlmc_best_end            closes the record: the routes behave as before; the buffers stay for the next begin and for reads.
 * While a record is open the rounds entry points observe every chain once per round, stamp = round0 + r, after that round's sweeps and
 * before its swap decision: nlmc_pt_rounds_fused and the in-launch route of nlmc_pt_rounds_deferred inside k_rounds_fused (wave 0
 * copies the spins from LDS after the chain's hand-off record is out; instantiations of their own, the kernels without a record are
 * unchanged), the launch-per-round route of nlmc_pt_rounds_deferred by a k_best_update behind every sweep launch, nlmc_pt_rounds_lanes
 * inside k_rounds_lanes (a lane compares its own energy, improved lanes' columns are written a chain at a time).  The record lives in
 * global memory and carries over from launch to launch and from call to call.  nlmc_apt_rounds_lanes returns NLMC_ERR_UNSUPPORTED
 * (nothing was run) while a record is open: its kernel keeps none.  nlmc_sweep_philox / nlmc_sweep_stream, nlmc_set_spins, nlmc_energy,
 * the Houdayer and swap entry points do not observe and leave the record alone.  The unit is the round: fused windows overlap a round's
 * sweeps, there is no consistent state between them. */
int nlmc_best_begin(nlmc_ctx *ctx, double target);
int nlmc_best_update(nlmc_ctx *ctx, uint32_t stamp);
int nlmc_best_read(nlmc_ctx *ctx, double *out_energy /*[n_chains]*/, int32_t *out_stamp /*[n_chains]*/,
                   int32_t *out_first_hit /*[n_chains]*/, int8_t *out_state /*[n_chains][n]*/);
int nlmc_best_end(nlmc_ctx *ctx);
/* ---- run-long per-round energy log: what energy sat on which temperature in every round ------------------------------------------
 * The swap log says which swaps happened, the best-state record which state a chain reached; this log keeps, for every round of a window
 * [round0, round0 + n_rounds) and every local chain, the tracked energy and the temperature slot AS THE SWAP DECISION OF THAT ROUND SEES
 * THEM: after the round's sweeps, after the Houdayer step or the NMC phases where the round has them.  It lasts from nlmc_elog_begin to
 * nlmc_elog_end, over any number of calls, and only observes: no call's results change while it is open.  energy [n_rounds][n_chains]
 * double = (double) tracked integer 2^-nlmc_energy_scale (nlmc_energy_tracked's conversion), slot [n_rounds][n_chains] int32, by LOCAL
 * chain; a row no observation reached reads NaN / -1; rounds outside the window are not logged and are no error; a second observation
 * of a round overwrites the first.  12 bytes per chain and round of device memory.
 *   nlmc_elog_begin(round0, n_rounds)  opens or resets the log (all rows NaN / -1).  After nlmc_pt_init (NLMC_ERR_STATE before).  The
 *                            buffers are allocated at the first begin and kept (a larger window grows them).  NLMC_ERR_UNSUPPORTED for
 *                            a context with a communicator (nlmc_comm_init) or a cut ladder (nlmc_apt_shard over several ranks, a
 *                            chain block that is not whole ladders).
 *   nlmc_elog_update(round)  one observation of every local chain from the state arrays (k_elog_update: any n), queued on the
 *                            context's stream, asynchronous.  NLMC_ERR_STATE before nlmc_pt_init or with no log open,
 *                            NLMC_ERR_UNSUPPORTED under a chain subset.  For drivers that run a round call by call: between the last
 *                            state-changing step and the swap round.
 *   nlmc_elog_read           the rows of the window most recently begun; both pointers nullable; one stream synchronisation.  Also
 *                            after nlmc_elog_end.
 *   nlmc_elog_end            closes the log: the routes behave as before; the buffers stay for the next begin and for reads.
 * While a log is open the rounds entry points observe every chain once per round, row = round0 + r of the call: nlmc_pt_rounds_fused
 * and the in-launch route of nlmc_pt_rounds_deferred inside k_rounds_fused (thread 0 stores what it publishes for the hand-off; the
 * observing instantiations are those of the best-state record, which test which record is present: the kernels without an observer are
 * unchanged), the launch-per-round route by a k_elog_update behind every sweep launch, nlmc_pt_rounds_lanes inside k_rounds_lanes (every
 * live lane stores its energy and slot), nlmc_apt_rounds_lanes inside k_apt_rounds_lanes<.., ELOG> behind the Houdayer step's energy
 * deltas (it still refuses while a best-state record is open).  nlmc_sweep_*, nlmc_set_spins, nlmc_energy, the Houdayer and swap entry
 * points do not observe. */
int nlmc_elog_begin(nlmc_ctx *ctx, uint32_t round0, int n_rounds);
int nlmc_elog_update(nlmc_ctx *ctx, uint32_t round);
int nlmc_elog_read(nlmc_ctx *ctx, double *out_energy /*[n_rounds][n_chains]*/, int32_t *out_slot /*[n_rounds][n_chains]*/);
int nlmc_elog_end(nlmc_ctx *ctx);
/* mode 1: copy the chains' CURRENT configurations aside; later nlmc_backbone_clusters calls are seeded with that copy instead of the
 * states they find (the m_star of a cycle without a plain phase is the state after the last plain phase, NMC/nmc.py:368-373,433:
 * full_update_frequency != 1).  mode 0: seed with the current states again. */
int nlmc_backbone_seed(nlmc_ctx *ctx, int mode);
int nlmc_adopt_best(nlmc_ctx *ctx);
int nlmc_backbone_clusters(nlmc_ctx *ctx, const double *epsilon /*[n]*/, const double *lambdas, int n_lambdas, double beta,
                           double tolerance, int max_iterations, double sat, const double *thresholds, int n_thresholds);
int nlmc_backbone_check(nlmc_ctx *ctx);
int nlmc_get_cluster_mask(nlmc_ctx *ctx, uint8_t *out /*[n_chains][n]*/);
/* Caller-provided backbones instead of an inference (NMC_subroutine's `all_clusters` argument, NPT/npt.py:357-359): 1 = in a cluster. */
int nlmc_set_cluster_mask(nlmc_ctx *ctx, const uint8_t *mask /*[n_chains][n]*/);
int nlmc_set_phase(nlmc_ctx *ctx, int kind, double temp_x);
/* All phases of an NMC cycle of short chains in launches of k_nmc_phases_lanes (csrc/nlmc_lane_nmc.h), a chain per lane, on the selected
 * chains: for phase p of kind kinds[p] (NLMC_PHASE_*) -- p > 0: nlmc_adopt_best -- nlmc_set_phase(kinds[p], temp_x) and
 * nlmc_sweep_philox(shared order, sweeps_per_phase sweeps from sweep0 + p sweeps_per_phase, one beta) under
 * nlmc_track_minimum(min_stride), with spins, backbone mask and (where it fits) the best state in LDS across the hand-offs: the flag
 * of a spin is computed from its mask byte, the context's flags array and nlmc_set_phase's setting are neither read nor changed.  Same
 * bits as that call sequence on any route: spins, tracked energies, energy sink, minimum, argmin and best state are left as its last
 * sweep call leaves them.  Reached by name: nlmc_set_lane_sweeps is not looked at.
 * Optional read-backs (each nullable; any of them synchronises the stream): out_phase_min [rows][n_phases], the minimum of every phase
 * in the fixed point of the tracked energies (times 2^-nlmc_energy_scale), out_phase_argmin [rows][n_phases] (sweep of the first
 * attainment, counted from 0 within the phase), out_last_best [rows][n], the best state of the last phase; rows = nlmc_subset_count.
 * Without them the call is asynchronous on the stream the subset's sweeps use (nlmc_overlap_subsets), with visiting orders of its own.
 * The orders come from one k_lane_orders launch per launch: a call whose orders exceed the order scratch (NLMC_LANE_SCRATCH), or of
 * more than 128 phases, is cut into launches of whole phases, the state carried over by the context's arrays.
 * NLMC_ERR_ARG: n_phases < 1, sweeps_per_phase < 1, min_stride < 1, a bad kind or precision, temp_x = 0.  NLMC_ERR_STATE: no backbone
 * mask yet (nlmc_backbone_clusters / nlmc_set_cluster_mask), or nlmc_track_minimum is on (the call keeps the minimum itself).
 * NLMC_ERR_UNSUPPORTED (nothing was run, the reason in nlmc_last_error; nlmc_nmc_phases_lanes_refusal asks without a call): n >
 * NLMC_LANE_N or the global-memory kernels (NLMC_FORCE_BIG); one phase's orders exceed the order scratch; random numbers keyed by
 * temperature slot (nlmc_apt_shard); spins + mask exceed a workgroup's LDS; NLMC_NO_LANE_NMC=1 at nlmc_create (test knob).  Afterwards
 * nlmc_last_sweep_route is NLMC_ROUTE_LANES, nlmc_last_schedule_stats reports the visiting orders built, the launch counters count a
 * phase each, the timings count the order kernel as the levelize half. */
int nlmc_nmc_phases_lanes(nlmc_ctx *ctx, int precision, const int32_t *kinds, int n_phases, int sweeps_per_phase, uint32_t sweep0,
                          uint64_t seed, double beta, double temp_x, int min_stride, int64_t *out_phase_min, int32_t *out_phase_argmin,
                          int8_t *out_last_best);
/* NULL when nlmc_nmc_phases_lanes would take phases of sweeps_per_phase sweeps on this context, else the reason of its
 * NLMC_ERR_UNSUPPORTED (a static string). */
const char *nlmc_nmc_phases_lanes_refusal(const nlmc_ctx *ctx, int sweeps_per_phase);
/* The same call in launches of k_nmc_phases_waves (csrc/nlmc_wave_nmc.h), a chain per wave in k_sweep_waves' launch shape: signature,
 * call sequence replaced, read-backs, launch cuts (NLMC_LANE_SCRATCH, 128 phases), order buffer, stream and error codes of
 * nlmc_nmc_phases_lanes.  Spins, backbone mask, the exact int32 local fields and -- beside the best state's spins -- the best state's
 * fields stay in registers across the phases: the argmin hand-off is a register copy, the fields are built once per launch (a launch
 * that continues a call builds them from the context's best state).  Same bits as the call sequence on any route.  Reached by name:
 * nlmc_set_wave_sweeps is not looked at; the dense matrix is built on demand as by the wave sweeps.
 * NLMC_ERR_UNSUPPORTED (nothing was run; nlmc_nmc_phases_waves_refusal asks without a call): n > NLMC_WAVE_N, under nlmc_set_wave_long
 * too (long chains have nlmc_nmc_phases_waves_long); the global-memory kernels (NLMC_FORCE_BIG); precision NLMC_F64; random numbers keyed by
 * temperature slot (nlmc_apt_shard); one phase's orders exceed the order scratch; NLMC_NO_WAVE_NMC=1 at nlmc_create (test knob).
 * Afterwards nlmc_last_sweep_route is NLMC_ROUTE_WAVES, nlmc_last_schedule_stats reports the visiting orders built and no levels, the
 * launch counters count a phase each. */
int nlmc_nmc_phases_waves(nlmc_ctx *ctx, int precision, const int32_t *kinds, int n_phases, int sweeps_per_phase, uint32_t sweep0,
                          uint64_t seed, double beta, double temp_x, int min_stride, int64_t *out_phase_min, int32_t *out_phase_argmin,
                          int8_t *out_last_best);
/* NULL when nlmc_nmc_phases_waves would take f32 phases of sweeps_per_phase sweeps on this context, else the reason of its
 * NLMC_ERR_UNSUPPORTED (a static string). */
const char *nlmc_nmc_phases_waves_refusal(const nlmc_ctx *ctx, int sweeps_per_phase);
/* The same call for dense chains of NLMC_WAVE_N + 1 .. NLMC_WAVE_LONG_N spins in launches of k_nmc_phases_waves_long
 * (csrc/nlmc_wave_long_nmc.h), a chain per wave in k_sweep_waves_long's launch shape: signature, call sequence replaced, read-backs,
 * launch cuts, order buffer, stream and error codes of nlmc_nmc_phases_lanes.  The exact int32 local fields stay in registers with a
 * copy in the wave's LDS region, the best state's fields in registers, spins, flags, best spins and backbone mask in byte planes of the
 * region (nlmc_wave_long_nmc_region): the fields are built once per launch, the argmin hand-off stays inside the wave, and nothing goes
 * to global memory inside the phase loop but the phase minima.  Same bits as the call sequence on any route.  Reached by name: neither
 * nlmc_set_wave_sweeps nor nlmc_set_wave_long is looked at; the dense matrix is built on demand as by the wave sweeps.
 * NLMC_ERR_UNSUPPORTED (nothing was run; nlmc_nmc_phases_waves_long_refusal asks without a call): n <= NLMC_WAVE_N or n >
 * NLMC_WAVE_LONG_N; the global-memory kernels (NLMC_FORCE_BIG); precision NLMC_F64; random numbers keyed by temperature slot
 * (nlmc_apt_shard); one phase's orders exceed the order scratch; a padded chain longer than a matrix row; NLMC_NO_WAVE_LONG_NMC=1 at
 * nlmc_create (test knob).  Afterwards nlmc_last_sweep_route is NLMC_ROUTE_WAVES, nlmc_last_schedule_stats reports the visiting orders
 * built and no levels, the launch counters count a phase each. */
int nlmc_nmc_phases_waves_long(nlmc_ctx *ctx, int precision, const int32_t *kinds, int n_phases, int sweeps_per_phase, uint32_t sweep0,
                               uint64_t seed, double beta, double temp_x, int min_stride, int64_t *out_phase_min,
                               int32_t *out_phase_argmin, int8_t *out_last_best);
/* NULL when nlmc_nmc_phases_waves_long would take f32 phases of sweeps_per_phase sweeps on this context, else the reason of its
 * NLMC_ERR_UNSUPPORTED (a static string). */
const char *nlmc_nmc_phases_waves_long_refusal(const nlmc_ctx *ctx, int sweeps_per_phase);
/* Fused-window plans live in two slots; nlmc_plan_philox_fused / nlmc_plan_reserve_fused write to the selected one, sweep
 * calls use whichever slot covers their sweeps (a round sweeps its plain chains on windows of num_sweeps_MCMC_per_swap and
 * its NMC phases on windows of num_sweeps_per_NMC_phase_per_swap, NPT/npt.py:577-580). */
int nlmc_plan_slot(nlmc_ctx *ctx, int slot /*0 or 1*/);

/* Houdayer iso-cluster move (NPT/apt_ICM.py:116-143, 215-246) between the current states of local chains a and
 * b: connected components of the disagreement sub-graph, pick component number `pick_index mod n_components`
 * (list ordered by ascending smallest member); if its size > n/2 and katzgraber: state a := -state a, else
 * exchange the component between the two states.  out_info = {n_components, picked size}. */
int nlmc_icm_components(nlmc_ctx *ctx, int chain_a, int chain_b, int32_t *out_n_components);
int nlmc_icm_move(nlmc_ctx *ctx, int chain_a, int chain_b, int64_t pick_index, int katzgraber, int32_t *out_info);
/* Component label (= smallest member index) of every spin for the pair of the most recent nlmc_icm_components /
 * nlmc_icm_move call; -1 where the two states agree.  Backs find_disagreement_clusters (NPT/apt_ICM.py:116-143). */
int nlmc_icm_get_labels(nlmc_ctx *ctx, int32_t *out /*[n]*/);
/* Device-decided batch: pairs [n_pairs][2] local chain ids, pick = philox(pair, round, ., ICM) */
int nlmc_icm_round_philox(nlmc_ctx *ctx, const int32_t *pairs, int n_pairs, uint32_t round, uint64_t seed,
                          int katzgraber, int32_t *out_info /*[n_pairs][2] nullable*/);
/* The Houdayer step of one APT round decided entirely on the device (NPT/apt_ICM.py:216-246 for every temperature):
 * chains are K = n_chains_global / ladder_len ladders (sub-replicas) of ladder_len temperature slots (nlmc_pt_init);
 * per slot the ladders are shuffled (Philox(ladder, round, slot, ICM_PAIR) keys) and paired, each pair gets one
 * iso-cluster move with a Philox-picked cluster, tracked energies are resynchronised.  No host round trip.
 * out_n_pairs = ladder_len * (K / 2); out_info (nullable) [n_pairs][2] = {n_components, picked size}, slot-major.
 * Under nlmc_apt_systems(M): K = n_ladders / M, every system pairs its own ladders, out_n_pairs = M ladder_len (K / 2), system-major. */
int nlmc_icm_round_ladders(nlmc_ctx *ctx, uint32_t round, uint64_t seed, int katzgraber, int32_t *out_n_pairs,
                           int32_t *out_info /*nullable*/);

/* Convexified loopy belief propagation (backbone inference), batched: replaces the lambda loop of LBP_convexified
 * (NMC/nmc.py:126-160) together with LoopyBeliefPropagation (NMC/nmc.py:168-228) for n_problems seeds m_star on the
 * context's (J, h).  Host arrays in, host arrays out; messages stay on the device.
 *   h_lambda = h + lambda * m_star * epsilon; messages start at h_msgs = 0, u_msgs = J * m_star (NMC/nmc.py:128-129) and
 *   are carried from one lambda to the next; each lambda iterates until both relative max-norm changes are below
 *   `tolerance` or max_iterations is reached.  Exhausting the iterations at the first lambda sets status 1 (the
 *   reference raises ValueError there); at a later lambda the previous marginals are kept and the loop stops.
 *   lambdas: the host-computed list (lambda *= factor until < lambda_end or round(lambda, 6) == 0).
 *   sat: clip bound of atanh_saturated (tanh(19.06) - eps, NMC/nmc.py:230-255).
 * out_mag [n_problems][n]: marginals after the last processed lambda; out_mag_all (nullable)
 * [n_problems][n_lambdas][n]: one row per processed lambda; out_n_lambdas [n_problems]; out_iters
 * [n_problems][n_lambdas]: last iteration index per lambda; out_status [n_problems].
 * fp64, row sums in ascending neighbour order: equal to the reference to rounding, not bit for bit.
 * NLMC_ERR_ARG when the sparsity pattern of J is not symmetric. */
int nlmc_lbp_convexified(nlmc_ctx *ctx, int n_problems, const double *m_star, const double *epsilon, const double *lambdas,
                         int n_lambdas, double beta, double tolerance, int max_iterations, double sat,
                         double *out_mag, double *out_mag_all, int32_t *out_n_lambdas, int32_t *out_iters,
                         int32_t *out_status);

/* Cluster growth of find_clusters (NMC/nmc.py:257-318) on the CSR neighbour lists -- host-side graph logic (no context,
 * no device work; irregular and sequential by definition: seeds are served in ascending order and claim exclusively).
 * out_members: clusters concatenated in creation order (capacity members_capacity >= n suffices when J has no
 * diagonal), out_sizes [<= n], out_n_clusters.  Errors are reported through nlmc_last_error(NULL). */
int nlmc_find_clusters(int n, const int32_t *rowptr, const int32_t *colidx, const double *vals, const double *mag,
                       double threshold_initial, double threshold_cutoff, double threshold_step, int32_t *out_members,
                       int64_t members_capacity, int32_t *out_sizes, int32_t *out_n_clusters);

/* Host routine (no device work): lays a recorded trace out as the reference's M blocks.  src [n_blocks][n_sweeps][n]
 * int8 (out_spins of the sweep calls) -> dst [n_dst_blocks][n][row_len]; block b goes to block dst_block[b] (NULL:
 * identity), columns dst_col[b] .. dst_col[b]+n_sweeps-1 (NULL: 0; a multiple of n_sweeps), as int8 (elem_bytes 1) or
 * float64 (elem_bytes 8) -- `M[r*N:(r+1)*N, :] = MCMC(...)` of NPT/npt.py:641 and the sub-replica column groups of
 * NPT/apt_ICM.py:207 for every chain at once, filled by n_threads host threads (<= 0: one per core, at most 32).
 * Elements of dst that no block maps to are left untouched. */
int nlmc_trace_layout(const int8_t *src, int64_t n_blocks, int64_t n_sweeps, int64_t n, const int32_t *dst_block,
                      const int32_t *dst_col, int64_t n_dst_blocks, int64_t row_len, void *dst, int elem_bytes, int n_threads);

/* Host routine: writes one zero byte into every 4 KB page of a freshly allocated buffer from n_threads threads (<= 0: one per
 * core, at most 32) -- the first-touch page faults of the reference-shaped float64 M (205 MB at the C4 shape: 14 of the 47 ms of
 * an NPT.run call) are taken while the GPU is still sweeping instead of after it. */
int nlmc_host_prefault(void *ptr, int64_t bytes, int n_threads);

/* Timing of the most recent sweep call, measured with HIP events on the context's stream -- zero unless event timing
 * was switched on with nlmc_timing_reset (the plain product path records no events). */
int nlmc_last_timing(nlmc_ctx *ctx, float *ms_levelize, float *ms_sweep, int32_t *launches_sweep);
/* Accumulated HIP-event timing of the sweep calls since nlmc_timing_reset (one synchronisation, at read time).
 * enable = 0: off; 1: events around every kernel launch; k > 1: around every k-th fused-window launch only (an event
 * record is a stream command of its own: at one launch per 130 us the two records of a launch are a measurable part of
 * the gap between launches).  While accumulation is on, sweep calls do not recycle their events.
 * nlmc_timing_total: ms_sweep = summed duration of the `launches_timed` launches that had events (of `launches_sweep`
 * launches in all); ms_levelize = summed duration of every schedule construction. */
int nlmc_timing_reset(nlmc_ctx *ctx, int enable);
int nlmc_timing_total(nlmc_ctx *ctx, double *ms_levelize, double *ms_sweep, int64_t *launches_sweep, int64_t *launches_timed);
/* Level-schedule statistics of the most recent sweep call: total levels and total spins over its orders. */
int nlmc_last_schedule_stats(nlmc_ctx *ctx, int64_t *n_orders, int64_t *n_levels);

#ifdef __cplusplus
}
#endif
#endif /* NLMC_H */
