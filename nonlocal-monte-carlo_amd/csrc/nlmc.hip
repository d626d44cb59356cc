// nlmc.hip -- context management, kernel launchers and the C-ABI of include/nlmc.h (gfx950 only).
#include "../../include/nlmc.h"
#include "nlmc_kernels.h"
#include "nlmc_pt_icm.h"
#include "nlmc_apt.h"
#include "nlmc_lbp.h"
#include "nlmc_nmc.h"
#include "nlmc_probe.h"
#include "nlmc_big.h"
#include "nlmc_lanes.h"
#include "nlmc_lane_rounds.h"
#include "nlmc_lane_apt.h"
#include "nlmc_lane_nmc.h"
#include "nlmc_waves.h"
#include "nlmc_waves_long.h"
#include "nlmc_wave_rounds.h"
#include "nlmc_wave_long_rounds.h"
#include "nlmc_wave_nmc.h"
#include "nlmc_wave_long_nmc.h"
#include "nlmc_wave_shape.h"
#include "nlmc_host.h"

#include <dlfcn.h>

#include <algorithm>
#include <cassert>
#include <chrono>
#include <thread>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

namespace {

constexpr double LOG2E = 1.4426950408889634;
std::string g_create_error;

// A device buffer that owns its memory: freed when the buffer goes (for a context's buffers, at `delete c` in nlmc_destroy, with the
// context's device current) unless it is borrowed.  Not copyable and not movable: every buffer is a member of nlmc_ctx, built in place.
template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;   // elements
    bool borrowed = false;      // p points into the context's arena (nlmc_create): not freed here
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    hipError_t reserve(size_t n)
    {
        if (n <= cap) return hipSuccess;
        if (p && !borrowed) { hipError_t e = hipFree(p); if (e != hipSuccess) { p = nullptr; cap = 0; return e; } }
        p = nullptr; cap = 0; borrowed = false;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), std::max<size_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) cap = n;
        return e;
    }
    void borrow(void *base, size_t &offset, size_t n)     // n elements at the next 256-byte boundary of the arena
    {
        offset = (offset + 255) & ~(size_t)255;
        p = reinterpret_cast<T *>(static_cast<char *>(base) + offset);
        cap = n; borrowed = true;
        offset += std::max<size_t>(n, 1) * sizeof(T);
    }
    static size_t arena_bytes(size_t n) { return ((std::max<size_t>(n, 1) * sizeof(T)) + 255 + 255) & ~(size_t)255; }   // covers what borrow takes
    void release() { if (p && !borrowed) (void)hipFree(p); p = nullptr; cap = 0; borrowed = false; }   // early give-back (nlmc_plan_philox_fused)
};
static_assert(!std::is_copy_constructible_v<DevBuf<int>> && !std::is_move_constructible_v<DevBuf<int>>, "DevBuf owns device memory");

// Every NLMC_* environment variable of the library: tuning, test and diagnostic switches.  read_knobs() reads them when a context is
// created (nlmc_create); they hold for the context's life, and setting a variable later does not reach a context that exists.
struct Knobs {
    bool force_big = false;          // NLMC_FORCE_BIG: every chain runs the global-memory kernels (tests compare both sets at one size)
    bool no_compact = false;         // NLMC_NO_COMPACT: fused-window schedules never use 4-byte entries
    bool no_pack64 = false;          // NLMC_NO_PACK64: the fp64 schedule window never holds 16-bit columns
    bool no_signfmt = false;         // NLMC_NO_SIGNFMT: fused-window schedules never use 2-byte entries
    int sweep_nt = -1;               // NLMC_SWEEP_NT: threads of a sweep workgroup (64..1024, multiple of 64; -1: unset, 0: invalid)
    int fused_workers = 0;           // NLMC_FUSED_WORKERS: worker waves of a 16-wave fused workgroup (8..16; 0: the default)
    int fused_gen0 = -1;             // NLMC_FUSED_GEN0: first wave that produces thresholds (-1: the default)
    bool no_fused = false;           // NLMC_NO_FUSED: nothing runs on fused windows
    bool no_fused64 = false;         // NLMC_NO_FUSED64: the fp64 mode never runs on fused windows
    bool no_fused_out = false;       // NLMC_NO_FUSED_OUT: calls with per-sweep outputs or temperatures run sweep by sweep
    bool no_warm = false;            // NLMC_NO_WARM: a fused launch does not pull the next window's schedule towards the chip
    bool no_prio = false;            // NLMC_FUSED_NOPRIO: the producing waves of a fused launch keep the default issue priority
    bool no_dbuf = false;            // NLMC_NO_DBUF: sweep-by-sweep kernels keep one copy of the per-sweep uniforms in LDS
    int big_per_level = -1;          // NLMC_BIG_PER_LEVEL: long chains run one launch per level (1) / per window (0); -1: by count
    bool no_bank_aware = false;      // NLMC_NO_BANK_AWARE: the fused planner does not place items by LDS bank
    bool no_quads = false;           // NLMC_NO_QUADS: a row of more than 16 entries takes a lane pair and its CSR tail, not a lane quad
    bool no_level_fill = false;      // NLMC_NO_LEVEL_FILL: the fused planner gives every update its earliest level and splits full levels
    bool no_head_stream = false;     // NLMC_NO_HEAD_STREAM: fused level loops load an item head per level, never the plan's head stream (A/B, tests)
    bool fz_stats = false;           // NLMC_FZ_STATS: the fused planner prints the phase cycle counts of window 0 on stderr
    unsigned tie_mask = 0xFFFFFFFFu; // NLMC_F64_TIE_MASK: high-word mask of the fp64 fused kernels' exact-path test (test knob)
    bool no_persistent = false;      // NLMC_NO_PERSISTENT: nlmc_pt_rounds_fused refuses, nlmc_pt_rounds_deferred launches per round
    bool no_deferred = false;        // NLMC_NO_DEFERRED: nlmc_pt_rounds_deferred refuses
    int lbp_group = 0;               // NLMC_LBP_GROUP: workgroups per loopy-BP problem (1..8; 0: by size)
    int lbp_poll_budget = 0;         // NLMC_LBP_POLL_BUDGET: polls of the loopy-BP group barrier (0: the default; test knob)
    bool lbp_global = false;         // NLMC_LBP_GLOBAL: loopy BP never takes the LDS-resident kernel
    size_t lane_scratch = (size_t)256 << 20;   // NLMC_LANE_SCRATCH: bytes of visiting orders one window of chain-per-lane sweeps may hold (test knob)
    int lane_rng = -1;               // NLMC_LANE_RNG: chain-per-lane sweeps make the Philox call per update (0) / keep a table per sweep in LDS
                                     // where it fits (1); -1: the default
    bool no_lane_nmc = false;        // NLMC_NO_LANE_NMC: nlmc_nmc_phases_lanes refuses (test knob)
    bool no_wave_nmc = false;        // NLMC_NO_WAVE_NMC: nlmc_nmc_phases_waves refuses (test knob)
    bool no_wave_long_nmc = false;   // NLMC_NO_WAVE_LONG_NMC: nlmc_nmc_phases_waves_long refuses (test knob)
    int wave_waves = 0;              // NLMC_WAVE_WAVES: waves (chains) per workgroup of the wave-per-chain sweeps (1..16; 0: by row count)
    bool wave_jlds = true;           // NLMC_WAVE_JLDS=0: the wave-per-chain sweeps read the matrix rows from global memory at every n
    bool wave_long_ahead = NLMC_WAVE_LONG_AHEAD_DEFAULT;   // NLMC_WAVE_LONG_AHEAD: k_sweep_waves_long requests the next visited spin's row at every update (1) or a row on a flip only (0)
    int wave_rounds_ladders = 0;     // NLMC_WAVE_ROUNDS_LADDERS: ladders per workgroup of the rounds inside a wave launch (0: by the rule)
    int dbg_flags = 0;               // NLMC_DBG_FLAGS: timing experiments of NLMC_DEBUG_KNOBS builds
    std::string stamp_file;          // NLMC_STAMP_FILE: NLMC_STAMPS builds dump the last launch's per-wave cycle sums here
};

Knobs read_knobs()
{
    auto on = [](const char *name) { return getenv(name) != nullptr; };
    auto num = [](const char *name, int unset) { const char *s = getenv(name); return s ? atoi(s) : unset; };
    Knobs k;
    k.force_big = on("NLMC_FORCE_BIG"); k.no_compact = on("NLMC_NO_COMPACT"); k.no_pack64 = on("NLMC_NO_PACK64"); k.no_signfmt = on("NLMC_NO_SIGNFMT");
    k.sweep_nt = on("NLMC_SWEEP_NT") ? std::max(0, num("NLMC_SWEEP_NT", 0)) : -1;
    k.fused_workers = num("NLMC_FUSED_WORKERS", 0);
    if (k.fused_workers < 8 || k.fused_workers > 16) k.fused_workers = 0;
    k.fused_gen0 = num("NLMC_FUSED_GEN0", -1);
    k.no_fused = on("NLMC_NO_FUSED"); k.no_fused64 = on("NLMC_NO_FUSED64"); k.no_fused_out = on("NLMC_NO_FUSED_OUT");
    k.no_warm = on("NLMC_NO_WARM"); k.no_prio = on("NLMC_FUSED_NOPRIO"); k.no_dbuf = on("NLMC_NO_DBUF");
    k.big_per_level = on("NLMC_BIG_PER_LEVEL") ? num("NLMC_BIG_PER_LEVEL", 0) != 0 : -1;
    k.no_bank_aware = on("NLMC_NO_BANK_AWARE"); k.no_level_fill = on("NLMC_NO_LEVEL_FILL"); k.fz_stats = on("NLMC_FZ_STATS"); k.no_quads = on("NLMC_NO_QUADS");
    k.no_head_stream = num("NLMC_NO_HEAD_STREAM", 0) != 0;
    if (const char *s = getenv("NLMC_F64_TIE_MASK")) k.tie_mask = (unsigned)strtoul(s, nullptr, 0);
    k.no_persistent = on("NLMC_NO_PERSISTENT"); k.no_deferred = on("NLMC_NO_DEFERRED");
    k.lbp_group = num("NLMC_LBP_GROUP", 0); k.lbp_poll_budget = num("NLMC_LBP_POLL_BUDGET", 0); k.lbp_global = on("NLMC_LBP_GLOBAL");
    if (const char *s = getenv("NLMC_LANE_SCRATCH")) k.lane_scratch = std::max<size_t>(1, (size_t)strtoull(s, nullptr, 0));
    k.lane_rng = on("NLMC_LANE_RNG") ? (num("NLMC_LANE_RNG", 0) != 0) : -1;
    k.no_lane_nmc = num("NLMC_NO_LANE_NMC", 0) != 0;
    k.no_wave_nmc = num("NLMC_NO_WAVE_NMC", 0) != 0;
    k.no_wave_long_nmc = num("NLMC_NO_WAVE_LONG_NMC", 0) != 0;
    k.wave_waves = std::min(16, std::max(0, num("NLMC_WAVE_WAVES", 0)));
    k.wave_jlds = num("NLMC_WAVE_JLDS", 1) != 0;
    k.wave_long_ahead = num("NLMC_WAVE_LONG_AHEAD", NLMC_WAVE_LONG_AHEAD_DEFAULT) != 0;
    k.wave_rounds_ladders = std::min(64, std::max(0, num("NLMC_WAVE_ROUNDS_LADDERS", 0)));
    k.dbg_flags = num("NLMC_DBG_FLAGS", 0);
    if (const char *s = getenv("NLMC_STAMP_FILE")) k.stamp_file = s;
    return k;
}

}  // namespace

struct nlmc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;             // nlmc_own_stream: `stream` was created by the library
    DevBuf<unsigned char> arena;          // ONE allocation behind the fixed-size buffers of nlmc_create (13 hipMalloc + 7 blocking
                                          // memsets + 6 blocking copies were 6 of the 29 ms of an NPT.run call at the C4 shape);
                                          // declared before the buffers that borrow from it, so it is freed after they are gone
    // Work on the MARKED chain subset may run on a second stream beside the unmarked chains' sweeps (nlmc_overlap_subsets):
    // `cur` is the stream the subset-aware launches go to, forked from / joined to `stream` by nlmc_select_chains.
    hipStream_t aux = nullptr, cur = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool overlap = false, forked = false;
    int n = 0, n_pad = 0;
    int64_t nnz = 0;
    int n_chains = 0, chain_base = 0, n_chains_global = 0;
    int escale = 32;
    bool compact16 = false;            // every Jq fits 16 bits: fused-window schedules use 4-byte entries
    bool f64_pack16 = false;           // ... and every J equals Jq 2^-qs exactly: the fp64 schedule window holds 16-bit columns / Jq
    bool sign8 = false;                // every Jq is +-1: fused-window schedules may use 2-byte entries (NLMC_FMT_ADDR)
    bool f64_exact = false;            // every J AND every h is an exact multiple of 2^-qs: the fp64 field is the integer field times
                                       // 2^-qs, the fp64 mode may run on fused windows (k_sweep_fused<.., F64>)
    int xmax = 0;                      // max over rows of sum |Jq| + |hq|: the range of the integer field
    bool no_field = false;             // every hq is 0: plain fused launches read the item heads from the plan's head stream
    bool f64_real = false;             // nlmc_set_fused_f64_real: the fp64 mode runs on fused windows for real couplings / fields too
                                       // (k_sweep_fused<.., R64>; plans then carry the fp64 value plane)
    Knobs knobs;                       // the environment switches, read at nlmc_create
    int ev_every = 1;                  // fused-window launches: events around every ev_every-th one (nlmc_timing_reset)
    long long launches_timed = 0;      // launches that contributed to the event sums since nlmc_timing_reset
    int qs = 0;                        // field scale of the fixed-point ("f32") path: Jq = rint(J 2^qs)
    double *energy_sink = nullptr;     // device buffer the sweep kernels also write the tracked energies to
    double temp_x = 1.0;
    bool has_flags = false;
    bool has_diag = false;
    bool has_zero_vals = false;   // a stored entry is 0.0 (or underflows to 0 in fp32)
    std::vector<std::pair<const void *, size_t>> lds_granted;   // dynamic-LDS opt-in already granted: (kernel, bytes) (ensure_lds)

    DevBuf<int32_t> rowptr, col;
    DevBuf<double> val64, h64;
    DevBuf<EdgeQ> edge32;
    DevBuf<int32_t> hq;
    DevBuf<int8_t> spins, best;
    DevBuf<uint8_t> flags;
    DevBuf<long long> efix, emin, etrace, dbg;
    DevBuf<int32_t> argmin;
    DevBuf<double> energy, tab, ustream, etrace_d;
    DevBuf<uint32_t> keys;
    DevBuf<int32_t> perm_raw;          // stream mode: the caller's permutations / uniforms as drawn, scattered by spin on the device
    DevBuf<double> u_raw;
    DevBuf<int32_t> stream_bad;
    DevBuf<int8_t> strace, cfg, snap_g;
    // The buffers that live in the arena, with their element counts, in arena order: nlmc_create sizes the arena by this list and
    // carves it up by it.  +16 entries of padding behind the row arrays: fixed-width row windows are read unconditionally (never used
    // past the row end).
    template <typename F> void arena_buffers(F &&f)
    {
        const size_t N = (size_t)n, nz = (size_t)nnz + 16, R = (size_t)std::max(n_chains, 1), states = R * (size_t)n_pad;
        f(rowptr, N + 1); f(col, nz); f(val64, nz); f(edge32, nz); f(h64, N); f(hq, N);
        f(spins, states); f(best, states); f(flags, states);
        f(efix, R); f(emin, R); f(argmin, R); f(energy, R);
    }
    int strace_nrec = 0;          // recorded configurations per chain held in strace by the last sweep call (0: none)
    int strace_rows = 0;          // chains (rows) of that trace: the subset the call ran on
    // chain subsets (nlmc_pt_mark_slots / nlmc_select_chains): sweeps, hand-offs and backbone inference of a call act on
    // the local chains that currently sit on unmarked / marked temperature slots
    int subset = 0;               // NLMC_CHAINS_ALL / _UNMARKED / _MARKED
    int n_marked_local = 0;       // marked slots x local ladders (static: ladders are whole inside a context)
    bool sub_dirty = true;        // slots moved since the list was built
    DevBuf<uint8_t> slot_mark;    // [ladder_len]
    DevBuf<int32_t> sub_list_buf; // [n_chains]: unmarked chains ascending, then marked chains ascending
    int sub_count() const { return subset == 0 ? n_chains : subset == 1 ? n_chains - n_marked_local : n_marked_local; }
    const int32_t *sub_list() const { return subset == 0 ? nullptr : subset == 1 ? sub_list_buf.p : sub_list_buf.p + (n_chains - n_marked_local); }
    bool track_min = false;       // sweep calls keep running minimum + argmin state on the device (nlmc_track_minimum)
    int track_min_stride = 1;     // ... over the sweeps 0, stride, 2 stride, ... of a call (the reference's M[:, ::M_skip])
    // run-long best-state record (nlmc_best_begin): allocated at the first begin, kept until the context goes
    bool best_on = false;
    double best_target = 0.0;     // NaN: no first-passage stamp
    DevBuf<long long> rec_efix;   // [n_chains]
    DevBuf<int32_t> rec_stamp, rec_hit;
    DevBuf<int8_t> rec_state;     // [n_chains][n_pad]
    BestRec best_rec() const { return BestRec{rec_efix.p, rec_stamp.p, rec_hit.p, rec_state.p, best_target}; }
    // run-long per-round energy log (nlmc_elog_begin): rows of rounds [elog_round0, elog_round0 + elog_rounds), allocated at the first
    // begin, kept until the context goes (a later, larger window grows them)
    bool elog_on = false;
    uint32_t elog_round0 = 0;
    int elog_rounds = 0;          // rows of the window most recently begun (what nlmc_elog_read returns, also after nlmc_elog_end)
    DevBuf<double> elog_energy;   // [elog_rounds][n_chains]
    DevBuf<int32_t> elog_slot;
    // The open log as the observer of a launch whose first round is r0 and that runs k rounds: energy = nullptr when no log is open or
    // none of the launch's rounds lies inside the window (rounds outside it are not logged and are no error: pt_log.covers' rule,
    // per round).  In 64 bits, so that a window or a call at the top of the 32-bit round range does not wrap.
    ElogRec elog_rec(uint32_t r0, int k) const
    {
        ElogRec e{};
        const int64_t d = (int64_t)r0 - (int64_t)elog_round0;
        if (!elog_on || d >= (int64_t)elog_rounds || d + (int64_t)k <= 0) return e;
        e.energy = elog_energy.p; e.slot = elog_slot.p; e.row0 = (int)d; e.n_rows = elog_rounds; e.n_chains = n_chains;
        return e;
    }
    bool observed() const { return best_on || elog_on; }   // the observing instantiations of k_rounds_fused / k_rounds_lanes serve both
    DevBuf<int8_t> seed_snap;    // nlmc_backbone_seed: the configurations later backbone inferences are seeded with
    bool seed_snap_on = false;
    DevBuf<uint8_t> cmask;        // [n_chains][n_pad] backbone mask of the last inference per chain
    DevBuf<uint8_t> cmask_scratch; // chains too long for LDS: the two membership arrays of k_cluster_mask per problem
    DevBuf<int32_t> big_flag;     // ... "changed" words of the levelizer's relaxation passes
    DevBuf<long long> big_esum;   // ... energy deltas of the running sweep per block row
    // chain-per-lane sweeps (csrc/nlmc_lanes.h)
    int lane_mode = 0;            // nlmc_set_lane_sweeps: 0 off, 1 auto, 2 force
    int last_route = 0;           // nlmc_last_sweep_route: NLMC_ROUTE_* of the most recent sweep call
    int64_t stat_lane_orders = 0; // visiting orders the most recent sweep call built for the lane kernels
    DevBuf<uint16_t> lane_perm;   // [orders of a window][n]
    // NMC phase cycles inside a lane launch (csrc/nlmc_lane_nmc.h): orders of their own, so that a call on the second stream does not
    // wait for the lane sweeps of the main one; the per-phase minima of the last call that asked for them
    DevBuf<uint16_t> nmc_perm;    // [orders of a launch][n]
    DevBuf<long long> nmc_pmin;   // [rows][phases]
    DevBuf<int32_t> nmc_pargmin;
    // wave-per-chain sweeps (csrc/nlmc_waves.h)
    int wave_mode = 0;            // nlmc_set_wave_sweeps: 0 off, 1 auto, 2 force
    bool wave_rounds = false;     // nlmc_set_wave_rounds: nlmc_pt_rounds_deferred takes k_rounds_waves where the sweeps go to the wave kernels
    bool wave_long_rounds = false;   // nlmc_set_wave_long_rounds: nlmc_pt_rounds_deferred takes k_rounds_waves_long for chains of more than NLMC_WAVE_N spins on the wave route
    bool wave_long = false;       // nlmc_set_wave_long: the wave route takes chains of up to NLMC_WAVE_LONG_N spins (k_sweep_waves_long)
    DevBuf<int32_t> wave_J;       // [n][64 R] dense fixed-point matrix, built on the first wave call (k_wave_matrix): 256 KB at n = 256, 4 MB at n = 1024
    bool wave_J_built = false;
    DevBuf<int32_t> nmc_status;   // sticky: a backbone inference diverged at its first lambda
    DevBuf<double> nmc_thr;       // thresholds of the cluster growth
    std::vector<double> nmc_thr_host, tab_host, lbp_eps_host, lbp_lams_host;   // contents of the device copies (uploads skipped when unchanged)
    double lbp_tJ_beta = 0.0; bool lbp_tJ_valid = false;
    // schedule scratch (per call) and plan cache (persistent)
    struct Sched {            // one set of level-schedule buffers (per-call scratch, or the persistent plan)
        DevBuf<int2> order, head32;
        DevBuf<int32_t> lvl_off, nlev, hi_max, ellc64;
        DevBuf<EdgeQ> ell32;
        DevBuf<double> ellv64, headh64;
        DevBuf<uint32_t> bkey, bcur;      // chains too long for LDS (csrc/nlmc_big.h): the levelizer's keys / cursors
        DevBuf<int32_t> blvl;
        hipError_t reserve_big(size_t orders, size_t n, bool philox_keys)
        {
            hipError_t e;
            if ((e = order.reserve(orders * n)) != hipSuccess) return e;
            if ((e = lvl_off.reserve(orders * (n + 1))) != hipSuccess) return e;
            if ((e = nlev.reserve(orders)) != hipSuccess) return e;
            if ((e = hi_max.reserve(orders)) != hipSuccess) return e;
            if (philox_keys && (e = bkey.reserve(orders * n)) != hipSuccess) return e;
            if ((e = blvl.reserve(orders * n)) != hipSuccess) return e;
            return bcur.reserve(orders * (n + 2));
        }
        hipError_t reserve(size_t orders, size_t n, int mode /*0 none, 1 f32, 2 f64*/)
        {
            hipError_t e;
            if ((e = order.reserve(orders * n)) != hipSuccess) return e;
            if ((e = lvl_off.reserve(orders * (n + 1))) != hipSuccess) return e;
            if ((e = nlev.reserve(orders)) != hipSuccess) return e;
            if ((e = hi_max.reserve(orders)) != hipSuccess) return e;
            if (mode == 1) {
                if ((e = head32.reserve(orders * n)) != hipSuccess) return e;
                if ((e = ell32.reserve(orders * n * NLMC_ELL_W32)) != hipSuccess) return e;
            } else if (mode == 2) {
                if ((e = headh64.reserve(orders * n)) != hipSuccess) return e;
                if ((e = ellc64.reserve(orders * n * NLMC_ELL_W)) != hipSuccess) return e;
                if ((e = ellv64.reserve(orders * n * NLMC_ELL_W)) != hipSuccess) return e;
            }
            return hipSuccess;
        }
    };
    Sched scratch, plan;
    int n_cu = 0;                        // compute units of the device (asked once)
    bool big = false;                    // n > NLMC_LDS_N: every sweep runs the global-memory kernels of csrc/nlmc_big.h
    bool plan_big = false;               // the cached plan was built by k_levelize_big (its items are { k, row start })
    int plan_precision = 0;
    bool plan_valid = false;
    int plan_mode = 0;
    uint32_t plan_sweep0 = 0;
    int plan_count = 0;
    uint64_t plan_seed = 0;
    // fused-window plan (k_levelize_fused / k_sweep_fused)
    int max_deg = 0;
    int n_long = 0;                    // schedule positions a sweep takes beyond one per row in a fused plan: one for a row of more than
                                       // NLMC_FZ_W entries (a lane pair), three for one of more than 2 NLMC_FZ_W (a lane quad)
    int stat_fused_window = -1;          // >= 0: the most recent sweep call ran this fused window
    int stat_head_path = 0;              // NLMC_HEADS_*: where the most recent fused launch read its item heads (0: no such launch yet)
    // Two plan slots (nlmc_plan_slot): a replica-exchange round whose marked slots run NMC cycles sweeps its plain chains
    // on windows of one length and its NMC phases on windows of another (NPT/npt.py:577-580).
    struct FusedPlan {
        bool valid = false;
        uint32_t sweep0 = 0;
        int windows = 0, T = 0, workers = 13;
        uint64_t seed = 0;
        std::vector<int32_t> nlev_host, npos_host;
        int pstride = 0, gen0 = 0;
        int fmt = 0;                  // entry format of the plan (NLMC_FMT_*)
        bool has_val = false;         // the plan carries the fp64 value plane (entries in row order): the real-valued fp64 variant
        FusedLevelizeArgs built{};    // what the planner was launched with (read-back: nlmc_plan_get_items)
        DevBuf<int32_t> npos;
        DevBuf<int2> head;
        DevBuf<EdgeQ> ell;
        DevBuf<double> val;           // [windows][NLMC_FZ_VAL_WORDS * pstride] (has_val only)
        DevBuf<int32_t> loff, nlev, himax, send;
        bool has_hs = false;          // the plan carries the head stream (fused_plan_stream)
        DevBuf<int4> hs;              // [windows][fused_hs_window(workers)] head stream (fused_hs_index), has_hs only
        void release() { npos.release(); head.release(); ell.release(); val.release(); loff.release(); nlev.release(); himax.release(); send.release(); hs.release(); }
        struct Arrays { const int32_t *loff, *nlev, *himax, *send, *npos; const int2 *head; const EdgeQ *ell; const double *val; const int4 *hs; };
        Arrays at(int w) const        // the plan arrays at window w (val: nullptr without the value plane)
        {
            const size_t W = (size_t)w, PS = (size_t)pstride;
            return {loff.p + W * (NLMC_LCAP + 1), nlev.p + W, himax.p + W, send.p + W * T, npos.p + W, head.p + W * PS, ell.p + W * PS * NLMC_FZ_W,
                    has_val ? val.p + W * NLMC_FZ_VAL_WORDS * PS : nullptr, has_hs ? hs.p + W * fused_hs_window(workers) : nullptr};
        }
    };
    FusedPlan fz[2];
    int fz_slot = 0;                  // slot the planning entry points write to
    int stat_fused_slot = 0;
    DevBuf<uint16_t> fz_glv;          // planning scratch, shared by the slots (planning is stream-ordered)
    DevBuf<uint32_t> fz_perm;
    DevBuf<uint16_t> fz_adj;
    DevBuf<long long> fz_stats;
    bool fz_adj_ready = false;
    // PT
    int ladder_len = 0;
    bool pt_tab_valid = false;
    double pt_tab_temp_x = 1.0;
    std::vector<double> beta_list;
    DevBuf<double> pt_tab, pt_beta, pt_energies_all;
    DevBuf<int32_t> slot_of_chain, chain_of_slot, pt_pairs, pt_status, pt_plan_pairs, pt_plan_ok;
    // A window of consecutive swap rounds that has one row per round in device buffers: the planned pair selections (nlmc_pt_plan)
    // and the device-side swap log (nlmc_pt_log_begin; it has no seed).
    struct RoundWindow {
        bool on = false;
        uint32_t round0 = 0;
        int rounds = 0, npairs = 0;
        uint64_t seed = 0;
        // Rounds [r0, r0 + n) lie inside the window, with its pairs per round and seed.  In 64 bits: the single-round launchers used
        // to ask `round < round0 + (uint32_t)rounds`, which wraps; the two forms agree whenever round0 + rounds <= 2^32, which is
        // every window the library's callers make.
        bool covers(uint32_t r0, int n, int n_pairs, uint64_t sd = 0) const
        {
            return on && seed == sd && npairs == n_pairs && r0 >= round0 && (uint64_t)r0 + (uint64_t)n <= (uint64_t)round0 + (uint64_t)rounds;
        }
        size_t row(uint32_t r) const { return (size_t)(r - round0); }       // of a round covers() said yes to
    };
    RoundWindow pt_plan, pt_log;
    DevBuf<uint8_t> pt_acc, pt_log_acc;
    DevBuf<int32_t> pt_log_pairs;
    std::vector<uint8_t> stage_in, stage_out;      // padded host staging for row copies
    // ICM
    DevBuf<int32_t> icm_label, icm_info, icm_pairs;
    // loopy BP (edge graph built on first use)
    bool lbp_graph_ready = false;
    DevBuf<int32_t> lbp_src, lbp_rev, lbp_flag, lbp_out_i;
    DevBuf<unsigned int> lbp_bar;
    DevBuf<double> lbp_part;
    DevBuf<double> lbp_tJ, lbp_eps, lbp_ms, lbp_lams, lbp_w0, lbp_w1, lbp_hm, lbp_tot, lbp_mag, lbp_mag_all;
    // timing / stats
    std::vector<hipEvent_t> events;
    size_t ev_used = 0, ev_call_start = 0;
    std::vector<uint8_t> ev_kind;      // per event triple: 0 = {start, after levelize, after sweep}, 1 = {start, -, end} of a sweep
                                       // launch, 2 = {start, -, end} of a planning kernel (the middle event is not recorded)
    bool ev_accumulate = false;
    long long launches_total = 0;
    int launches_sweep = 0;
    int64_t stat_orders = 0, stat_levels = 0;
    bool stats_pending = false;
    const int32_t *stats_nlev_ptr = nullptr;
    int64_t stats_nlev_count = 0;

    // APT run cut into slot blocks over ranks (nlmc_apt_shard, csrc/nlmc_apt.h)
    int apt_R = 0, apt_world = 0, apt_rank = 0;      // global ladder length; 0: not sharded by slot
    int rng_stride = 0, rng_base = 0;                // random numbers keyed by (ladder, global slot): SweepArgs::rng_*
    int apt_systems = 1;                             // independent APT systems of n_ladders / apt_systems ladders each (nlmc_apt_systems)
    DevBuf<double> apt_beta;                         // [apt_R] the global ladder
    DevBuf<long long> apt_e_all;                     // [world][K][ladder_len]
    DevBuf<int8_t> apt_send, apt_recv;               // [2][K][n_pad]
    DevBuf<int32_t> apt_bd;                          // [2][K]
    DevBuf<double> rounds_ebuf;                      // nlmc_pt_rounds_deferred: [2][n_chains_global] published energies
    DevBuf<unsigned long long> rounds_rec;           // k_rounds_fused: [rounds of a launch][n_chains_global] energies by slot
    int rounds_route = 0;                            // nlmc_pt_rounds_route
    const void *rounds_res_kfun = nullptr;           // the last residency question (rounds_resident) and its answer
    size_t rounds_res_lds = 0;
    int rounds_res_nt = 0;
    bool rounds_res_yes = false;
    DevBuf<unsigned char> rounds_args;               // its argument structs (read through constant-memory pointers), 2 slots
    std::vector<unsigned char> rounds_args_host[2];  // ... as uploaded (pageable memory: staged by hipMemcpyAsync before it returns)
    int rounds_args_slot = 0;
    void *comm = nullptr;              // RCCL communicator of the sharded tempering (nlmc_comm_init): the per-round all-gather of
    int comm_world = 0, comm_rank = 0; // the energies is issued by the library on the kernels' own stream

    std::string err;
    CsrDev g{};
};

namespace {

int fail(nlmc_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

#define HIP_TRY(c, expr)                                                                                   \
    do {                                                                                                   \
        hipError_t e__ = (expr);                                                                           \
        if (e__ != hipSuccess)                                                                             \
            return fail((c), NLMC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));            \
    } while (0)

// [rows][n] host rows <-> [rows][n_pad] device rows.  Pitched 2-D copies from pageable memory are served row by row
// by the runtime (~80 us per row); one linear copy through a padded staging buffer costs one transfer.
int rows_to_device(nlmc_ctx *c, void *dst_dev, const void *src_host, int rows);
int rows_to_host_begin(nlmc_ctx *c, const void *src_dev, int rows);               // async copy into c->stage
void rows_to_host_finish(nlmc_ctx *c, void *dst_host, int rows);                  // after the stream was synchronised

hipEvent_t next_event(nlmc_ctx *c)
{
    if (c->ev_used == c->events.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        c->events.push_back(e);
    }
    return c->events[c->ev_used++];
}

// An event triple of kind `kind` (ev_kind) around work on one stream.  The launchers open one only while timings accumulate
// (nlmc_timing_reset); span_mid / span_end of a span that was never begun do nothing.  A span takes its three events even where the
// middle one is never recorded: triple_ms indexes by threes.
struct TimerSpan { hipEvent_t mid = nullptr, end = nullptr; hipStream_t st = nullptr; };

int span_begin(nlmc_ctx *c, TimerSpan &s, uint8_t kind, hipStream_t st)
{
    hipEvent_t e0 = next_event(c);
    s.mid = next_event(c); s.end = next_event(c); s.st = st;
    if (!e0 || !s.mid || !s.end) return fail(c, NLMC_ERR_HIP, "hipEventCreate failed");
    const size_t t = c->ev_used / 3 - 1;
    if (c->ev_kind.size() <= t) c->ev_kind.resize(t + 1, 0);
    c->ev_kind[t] = kind;
    HIP_TRY(c, hipEventRecord(e0, st));
    return NLMC_OK;
}

int span_mid(nlmc_ctx *c, const TimerSpan &s) { if (s.mid) HIP_TRY(c, hipEventRecord(s.mid, s.st)); return NLMC_OK; }
int span_end(nlmc_ctx *c, const TimerSpan &s) { if (s.end) HIP_TRY(c, hipEventRecord(s.end, s.st)); return NLMC_OK; }

// opens a sweep call for nlmc_last_timing: its events and launches count from here
void begin_sweep_call(nlmc_ctx *c)
{
    if (!c->ev_accumulate) c->ev_used = 0;
    c->ev_call_start = c->ev_used;
    c->launches_sweep = 0;
}

// k launches of the open sweep call are on their stream (a chunk of k rounds in one launch counts k); `timed`: inside a timer span
void count_launches(nlmc_ctx *c, int k, bool timed)
{
    c->launches_sweep += k;
    c->launches_total += k;
    if (timed) c->launches_timed += k;
}

// c->n_cu, asked of the device once
int cu_count(nlmc_ctx *c)
{
    if (c->n_cu == 0) HIP_TRY(c, hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, c->device));
    return NLMC_OK;
}

// elapsed (levelize, sweep) milliseconds of triple t
int triple_ms(nlmc_ctx *c, size_t t, float &lev, float &sw)
{
    const size_t i = 3 * t;
    const uint8_t kind = t < c->ev_kind.size() ? c->ev_kind[t] : 0;
    lev = sw = 0.f;
    HIP_TRY(c, hipEventSynchronize(c->events[i + 2]));
    if (kind == 0) {
        HIP_TRY(c, hipEventElapsedTime(&lev, c->events[i], c->events[i + 1]));
        HIP_TRY(c, hipEventElapsedTime(&sw, c->events[i + 1], c->events[i + 2]));
    } else if (kind == 1) {
        HIP_TRY(c, hipEventElapsedTime(&sw, c->events[i], c->events[i + 2]));
    } else {
        HIP_TRY(c, hipEventElapsedTime(&lev, c->events[i], c->events[i + 2]));
    }
    return NLMC_OK;
}

int sweep_block(const nlmc_ctx *c)
{
    const int v = c->knobs.sweep_nt;
    if (v >= 64 && v <= 1024 && v % 64 == 0) return v;
    int nt = ((c->n + 7) / 8 + 63) / 64 * 64;
    return std::min(1024, std::max(64, nt));
}

// fp64-field philox kernels: 8 waves at most (256 registers per lane; with 16 waves the 128-register cap spilled 13-27
// registers per lane to scratch inside the level loop); levels wider than the workgroup are split when the schedule is built
// (fixed-point kernel with self-couplings: 12 waves, 170 registers: at 16 waves it spilled 2)
int sweep_block_for(const nlmc_ctx *c, bool f64_philox, bool f32_diag = false)
{
    return std::min(f64_philox ? 512 : f32_diag ? 768 : 1024, sweep_block(c));
}

// beyond the default dynamic-LDS window a kernel has to opt in (once per kernel and size step)
constexpr size_t NLMC_LDS_BYTES_MAX = (size_t)158 * 1024;      // dynamic LDS a workgroup may ask for

static_assert(NLMC_WAVE_LONG_LDS_MAX == NLMC_LDS_BYTES_MAX, "csrc/nlmc_wave_shape.h keeps its own copy of the ceiling");
static_assert(NLMC_WAVE_LONG_MIN_N == NLMC_WAVE_N + 1 && NLMC_WAVE_LONG_MAX_N == NLMC_WAVE_LONG_N, "csrc/nlmc_wave_shape.h keeps its own copy of the chain lengths");
static_assert(NLMC_WAVE_LONG_N <= NLMC_LANE_N, "k_lane_orders builds the visiting orders of the wave kernels");
int ensure_lds(nlmc_ctx *c, const void *func, size_t bytes)
{
    if (bytes > NLMC_LDS_BYTES_MAX) return fail(c, NLMC_ERR_UNSUPPORTED, "instance too large for the LDS-resident kernels of this build");
    if (bytes <= (size_t)60 * 1024) return NLMC_OK;
    auto it = std::find_if(c->lds_granted.begin(), c->lds_granted.end(), [&](const auto &e) { return e.first == func; });
    if (it != c->lds_granted.end() && bytes <= it->second) return NLMC_OK;
    HIP_TRY(c, hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (it != c->lds_granted.end()) it->second = bytes;
    else c->lds_granted.emplace_back(func, bytes);
    return NLMC_OK;
}

// Pointer table of a kernel family: entry k is Entry<k>::get(), nullptr for a combination that is not instantiated.  Built once.
template <template <int> class Entry, size_t... K> const void *kernel_at(size_t k, std::index_sequence<K...>)
{
    static const void *const table[] = {Entry<(int)K>::get()...};
    return table[k];
}

int level_block(int n)
{
    int nt = ((n + 3) / 4 + 63) / 64 * 64;
    return std::min(1024, std::max(64, nt));
}

// (chains too long for LDS: read in place, csrc/nlmc_big.h)
void launch_energy(nlmc_ctx *c, unsigned count, hipStream_t st, const EnergyArgs &a)
{
    const dim3 nt(c->n >= 4096 ? 1024 : 256);          // (the partial sums are per thread: one width for both variants)
    if (c->big) hipLaunchKernelGGL(k_energy<true>, dim3(count), nt, 0, st, a);
    else hipLaunchKernelGGL(k_energy<false>, dim3(count), nt, (size_t)c->n_pad, st, a);
}

// energies of the context's own chains -> efix (+ optional double output on device)
int launch_energy_self(nlmc_ctx *c, double *dev_out)
{
    EnergyArgs a{};
    a.g = c->g;
    a.spins = c->spins.p;
    a.stride = c->n_pad;
    a.out = dev_out;
    a.efix = c->efix.p;
    a.escale = c->escale;
    if (c->n_chains > 0) launch_energy(c, (unsigned)c->n_chains, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return NLMC_OK;
}

int run_levelize(nlmc_ctx *c, int n_orders, const uint32_t *keys_in, int per_chain, int n_sweeps, uint32_t sweep0,
                 uint64_t seed, nlmc_ctx::Sched &sc, int ell_mode)
{
    if (n_orders <= 0) return NLMC_OK;
    if (ell_mode < 0) {            // spins in global memory (csrc/nlmc_big.h); sc was reserved with reserve_big
        BigLevelizeArgs b{};
        b.g = c->g;
        b.n_orders = n_orders;
        b.keys_in = keys_in;
        b.seed_lo = (uint32_t)seed; b.seed_hi = (uint32_t)(seed >> 32); b.sweep0 = sweep0;
        b.per_chain = per_chain; b.n_sweeps = n_sweeps; b.chain_base = c->chain_base;
        b.key = sc.bkey.p; b.lvl = sc.blvl.p; b.cur = sc.bcur.p;
        b.ord2 = sc.order.p; b.lvl_off = sc.lvl_off.p; b.nlev = sc.nlev.p; b.hi_max = sc.hi_max.p;
        HIP_TRY(c, c->big_flag.reserve(NLMC_BIG_PASSES));
        b.flag = c->big_flag.p;
        // grid.y carries the order: batches of at most 65535 orders
        const unsigned gx = (unsigned)((c->n + 255) / 256);
        for (int ob = 0; ob < n_orders; ob += 65535) {
            const int no = std::min(65535, n_orders - ob);
            BigLevelizeArgs q = b;
            const size_t n = (size_t)c->n;
            q.n_orders = no;
            if (q.keys_in) q.keys_in += (size_t)ob * n;
            q.key = b.key ? b.key + (size_t)ob * n : nullptr; q.lvl += (size_t)ob * n; q.cur += (size_t)ob * (n + 2);
            q.ord2 += (size_t)ob * n; q.lvl_off += (size_t)ob * (n + 1); q.nlev += ob; q.hi_max += ob;
            // (Philox keys of per-chain orders are numbered over the whole call: the batch's first order id)
            if (!q.keys_in && per_chain && n_orders > 65535) return fail(c, NLMC_ERR_UNSUPPORTED, "more than 65535 per-chain orders of a long chain in one window");
            if (!q.keys_in) q.sweep0 = sweep0 + (uint32_t)ob;
            hipLaunchKernelGGL(k_blv_init, dim3(gx, no), dim3(256), 0, c->cur, q);
            HIP_TRY(c, hipGetLastError());
            // passes until no spin waits for a neighbour's level any more (the depth of the schedule: ~20-40 for sparse graphs, n at worst)
            bool settled = false;
            for (long long done = 0; !settled && done <= (long long)c->n + NLMC_BIG_PASSES; done += NLMC_BIG_PASSES) {
                int32_t fl[NLMC_BIG_PASSES];
                HIP_TRY(c, hipMemsetAsync(q.flag, 0, sizeof(fl), c->cur));
                for (int p = 0; p < NLMC_BIG_PASSES; ++p) hipLaunchKernelGGL(k_blv_pass, dim3(gx, no), dim3(256), 0, c->cur, q, p);
                HIP_TRY(c, hipGetLastError());
                HIP_TRY(c, hipMemcpyAsync(fl, q.flag, sizeof(fl), hipMemcpyDeviceToHost, c->cur));
                HIP_TRY(c, hipStreamSynchronize(c->cur));
                for (int p = 0; p < NLMC_BIG_PASSES; ++p) settled = settled || fl[p] == 0;
            }
            // (the order is total: n passes always suffice; never walk on with unset levels)
            if (!settled) return fail(c, NLMC_ERR_STATE, "level schedule of a long chain did not settle");
            const unsigned gt = (unsigned)((c->n + NLMC_BIG_TILE - 1) / NLMC_BIG_TILE);
            hipLaunchKernelGGL(k_blv_hist, dim3(gt, no), dim3(256), 0, c->cur, q);
            hipLaunchKernelGGL(k_blv_scan, dim3(no), dim3(1024), 0, c->cur, q);
            hipLaunchKernelGGL(k_blv_place, dim3(gt, no), dim3(256), 0, c->cur, q);
            HIP_TRY(c, hipGetLastError());
        }
        return NLMC_OK;
    }
    LevelizeArgs a{};
    a.g = c->g;
    a.n_orders = n_orders;
    a.keys_in = keys_in;
    a.seed_lo = (uint32_t)seed;
    a.seed_hi = (uint32_t)(seed >> 32);
    a.sweep0 = sweep0;
    a.per_chain = per_chain;
    a.n_sweeps = n_sweeps;
    a.chain_base = c->chain_base;
    a.level_cap = sweep_block_for(c, ell_mode == 2, ell_mode == 1 && c->has_diag);
    a.ord2 = sc.order.p;
    a.lvl_off = sc.lvl_off.p;
    a.nlev = sc.nlev.p;
    a.hi_max = sc.hi_max.p;
    if (ell_mode == 1) { a.ell32 = sc.ell32.p; a.head32 = sc.head32.p; }
    if (ell_mode == 2) { a.ellc64 = sc.ellc64.p; a.ellv64 = sc.ellv64.p; a.headh64 = sc.headh64.p; a.pack16 = c->f64_pack16 ? 1 : 0; }
    const size_t lds_one = (size_t)(c->n + 2) * 4 + (((size_t)c->n * 2 + 3) / 4) * 4;
    const size_t lds_two = lds_one + (size_t)(c->n + 2) * 4;
    a.two_sided = lds_two + 16 <= (size_t)150 * 1024;
    const size_t lds = (a.two_sided ? lds_two : lds_one) + 16;
    { int rc = ensure_lds(c, reinterpret_cast<const void *>(k_levelize), lds); if (rc) return rc; }
    hipLaunchKernelGGL(k_levelize, dim3(n_orders), dim3(level_block(c->n)), lds, c->cur, a);
    HIP_TRY(c, hipGetLastError());
    return NLMC_OK;
}

// ---- fused-window path ------------------------------------------------------------------------------------
// worker waves of a sweep workgroup of nt threads; the others generate uniforms and warm the cache
// (NLMC_FUSED_WORKERS: tuning knob for the 16-wave case)
// threads of a fused sweep workgroup: at least 4 waves (3 workers + 1 helper) also for small instances
// (3 n / 16 threads: 6-14 % faster than the n / 8 of the sweep-by-sweep kernels between N = 2000 and N = 6000 -- more worker
// waves per level, fewer levels split at the workgroup's width; N = 10^3 is flat from 256 to 768 threads, N >= 5500 has 1024)
int fused_block(const nlmc_ctx *c)
{
    if (c->knobs.sweep_nt >= 0) return std::max(256, sweep_block(c));
    const int nt = ((3 * c->n + 15) / 16 + 63) / 64 * 64;
    return std::min(1024, std::max(256, nt));
}

int fused_workers(const nlmc_ctx *c, int nt)
{
    const int waves = nt / 64;
    if (waves < 16) return waves - 1;
    if (c->knobs.fused_workers) return c->knobs.fused_workers;
    return 15;      // (one wave left to pull the next window's schedule towards the chip: 16 workers measured 137 vs 124 us
                    // per launch when the plans of 256 windows lie cold in HBM)
}

// LDS of k_sweep_fused: spins (+16: scratch spin of the dummy items, zero bytes) | (address format) negated spins (+16) |
// flags (+16) | 3 threshold tables of n_pad words | (per-sweep outputs only) 3 snapshot slots of n_pad bytes | reduction
// scratch
struct FusedLds { int neg_off, flags_off, u_off, u_bytes, snap_off, red_off, kt_off; size_t total; };
FusedLds fused_lds(int n_pad, bool has_flags, bool with_out, bool with_neg, int kt_entries = 0)
{
    FusedLds L{};
    L.neg_off = with_neg ? n_pad + 16 : 0;
    L.flags_off = (n_pad + 16) * (with_neg ? 2 : 1);
    int cur = L.flags_off + (has_flags ? n_pad + 16 : 0);
    cur = (cur + 15) / 16 * 16;
    L.u_off = cur;
    L.u_bytes = n_pad * 4;               // threshold word of (slot, k) = slot * n_pad + k = its snapshot byte, too
    cur += 3 * L.u_bytes;
    L.snap_off = cur;
    if (with_out) cur += 3 * n_pad + 16;
    L.red_off = cur;
    L.kt_off = cur + 32;                 // fp64 mode: Khi | Klo, one 4-byte word each per value of the integer field
    L.total = (size_t)cur + 32 + (size_t)kt_entries * 8;
    return L;
}

// LDS of the sweep-by-sweep kernels: spins | flags | uniforms of one sweep (philox) | level offsets (philox) | reduction scratch
struct StepLds { int flags_off, u_off, u_bytes, loff_off, red_off; bool dbuf; size_t total; };
StepLds step_lds(const nlmc_ctx *c, bool stream_mode, bool f64)
{
    StepLds L{};
    L.flags_off = c->n_pad;
    int cur = c->n_pad * (c->has_flags ? 2 : 1);
    cur = (cur + 15) / 16 * 16;
    L.u_off = cur;
    L.u_bytes = stream_mode ? 0 : ((c->n + 3) / 4 * 4 * (f64 ? 8 : 4) + 15) / 16 * 16;
    // second copy of the per-sweep uniforms / level offsets when it fits: lets the idle waves prepare sweep t+1 while
    // wave 0 runs the narrow tail of sweep t
    L.dbuf = !stream_mode && (size_t)cur + 2 * (size_t)L.u_bytes + 2 * NLMC_LCAP * 4 + 32 <= (size_t)150 * 1024 && !c->knobs.no_dbuf;
    cur += L.u_bytes * (L.dbuf ? 2 : 1);
    L.loff_off = cur;
    cur += NLMC_LCAP * 4 * (L.dbuf ? 2 : 1);               // (stream mode: one copy, the level offsets of the running sweep)
    L.red_off = cur;
    L.total = (size_t)cur + 16;
    return L;
}

// the address format needs the negated copy of the spins next to everything else (flags counted in: they may be switched
// on after planning)
bool fused_addr_format(const nlmc_ctx *c)
{
    return c->sign8 && 2 * (c->n_pad + 16) <= 0xFFFF && fused_lds(c->n_pad, true, false, true).total <= (size_t)150 * 1024;
}

// Do the context's fused plans carry a head stream (FusedPlan::hs)?  Only where a launch can read it (head_stream below): an
// instance without a field term whose plans have the address or the compact format, NLMC_NO_HEAD_STREAM unset.  Every other
// context neither reserves the stream's memory nor has the planner write it.
bool fused_plan_stream(const nlmc_ctx *c)
{
    return c->no_field && !c->knobs.no_head_stream && (fused_addr_format(c) || c->compact16);
}

// schedule positions reserved per window: one per update, two or four for a row on a lane pair or quad (n_long more per sweep),
// plus the padding of every level to a chunk boundary
int fused_pstride(int n, int n_long, int T) { return (int)((((size_t)T * ((size_t)n + n_long) + 63) / 64 + NLMC_LCAP) * 64); }

// first wave that produces thresholds (NLMC_FUSED_GEN0: tuning knob): the trailing half of the workgroup -- the
// waves that rarely or never hold a chunk
int fused_gen0(const nlmc_ctx *c, int nt)
{
    const int waves = nt / 64, v = c->knobs.fused_gen0;
    if (v >= 0 && v < waves) return v;
    return waves / 2;
}

// Instances the fused kernels are built for: a sweep workgroup of at least 4 waves (3 workers + 1 helper), degree in 14 bits, three
// uniform tables next to the spins in LDS (flags counted in: they may be switched on later).
bool fused_supported(const nlmc_ctx *c, int T)
{
    if (c->knobs.no_fused || c->big) return false;
    if (c->n < 256 || c->n > NLMC_FZ_SPT * 1024 || c->max_deg > 0x3FFF || T < 3 || T > NLMC_FUSED_TMAX) return false;
    if ((size_t)T * ((size_t)c->n + c->n_long) > ((size_t)1 << 22)) return false;   // 32-bit buffer offsets of the packed planes
    if (c->n_pad + 16 > 0x3FFF) return false;                          // spin address in 14 bits of the item head
    const FusedLds L = fused_lds(c->n_pad, true, false, false);
    if (3 * L.u_bytes / 4 > 0xFFFF) return false;                      // threshold word index in 16 bits
    return L.total <= (size_t)150 * 1024;
}

// k_sweep_fused's arithmetic: fixed point ("f32"), fp64 with integer thresholds (F64), fp64 real-valued (F64 + R64)
enum { NOT_FUSED = -1, ARITH_F32 = 0, ARITH_F64 = 1, ARITH_R64 = 2 };
// the launchers on fused windows: run_sweeps, nlmc_pt_rounds_deferred, nlmc_pt_rounds_fused
enum class Via { sweeps, deferred, rounds };

// The one rule for whether a call runs on fused windows, and on which arithmetic: NOT_FUSED or ARITH_*.  `slot`: the plan slot whose
// windows of T sweeps cover the call (fused_plan_for), or -1 to ask whether such windows could carry the precision at all
// (nlmc_fused_modes).  `sweep_temps`, `flags`: the call has a temperature per sweep, phase flags in force (both together: sweep by
// sweep in the fp64 mode).
int fused_route(const nlmc_ctx *c, int precision, int order_mode, bool sweep_temps, bool flags, int slot, int T, Via via)
{
    if (order_mode != NLMC_ORDER_SHARED || !fused_supported(c, T)) return NOT_FUSED;
    if (precision == NLMC_F32) return ARITH_F32;
    if (c->knobs.no_fused64) return NOT_FUSED;
    // the fp64 mode.  A temperature per sweep (an anneal) with phase flags in force stays sweep by sweep; without flags the
    // integer-threshold variant takes it (fused_levels<.., SWT>), the real-valued one does not (below)
    if (sweep_temps && flags) return NOT_FUSED;
    if (c->f64_exact) {
        // exact dyadic couplings and fields (the field is an integer): a per-chain threshold table per value of the field in LDS beside
        // the rest; with phase flags a second one (scaled rows), counted at its worst (negated copy of the spins in), so that the
        // answer depends on n and xmax alone -- otherwise the call runs sweep by sweep
        if (c->xmax > 4095 || fused_lds(c->n_pad, false, false, fused_addr_format(c), 2 * c->xmax + 1).total > (size_t)156 * 1024)
            return NOT_FUSED;
        if (flags && fused_lds(c->n_pad, true, false, true, 2 * (2 * c->xmax + 1)).total > (size_t)156 * 1024) return NOT_FUSED;
        // a temperature per sweep: a ring of three tables, one per threshold slot, counted like the two above (no flags); and the
        // 2 xmax + 1 entries a sweep rebuilds stay below an eighth of its n updates (at most a handful per producing thread: the
        // workgroup has about 3 n / 32 of them).  Otherwise the call runs sweep by sweep.
        if (sweep_temps && (8 * (2 * c->xmax + 1) > c->n ||
                            fused_lds(c->n_pad, false, false, true, 3 * (2 * c->xmax + 1)).total > (size_t)156 * 1024))
            return NOT_FUSED;
        return ARITH_F64;
    }
    // real couplings or fields: opt-in (nlmc_set_fused_f64_real), plans with the fp64 value plane, no tables (the f32 mode's LDS),
    // on all three launchers.  One temperature per chain only: with a temperature per sweep the real-valued output variant
    // was measured at 0.69-0.74x of the sweep-by-sweep kernel (anneals of 10^3 sweeps, DESIGN.md section 2: measured and rejected)
    if (!c->f64_real || sweep_temps || (slot >= 0 && !c->fz[slot].has_val)) return NOT_FUSED;
    return ARITH_R64;
}

// k_sweep_fused<DIAG, FLAGS, OUT, FMT, F64, DEFER, R64> by {diag, flags, outs, fmt, arith, defer}: 90 kernels, the deferred swap
// (DEFER) without phase flags and per-sweep outputs
template <int K> struct FusedKernel {
    static constexpr bool diag = K & 1, flags = K >> 1 & 1, outs = K >> 2 & 1, defer = K / 72;
    static constexpr int fmt = K / 8 % 3, arith = K / 24 % 3;
    static const void *get()
    {
        if constexpr (defer && (flags || outs)) return nullptr;
        else return reinterpret_cast<const void *>(k_sweep_fused<diag, flags, outs, fmt, arith != ARITH_F32, defer, arith == ARITH_R64>);
    }
};
const void *fused_kernel(bool diag, bool flags, bool outs, int fmt, int arith, bool defer)
{
    static_assert(NLMC_FMT_WIDE == 0 && NLMC_FMT_COMPACT == 1 && NLMC_FMT_ADDR == 2, "key order");
    const size_t key = (((size_t)defer * 3 + arith) * 3 + fmt) * 8 + (outs ? 4 : 0) + (flags ? 2 : 0) + (diag ? 1 : 0);
    return kernel_at<FusedKernel>(key, std::make_index_sequence<144>{});
}

// k_rounds_fused<DIAG, FMT, F64, R64, BEST> by {diag, fmt, arith, best}: 36 kernels (best: an observer -- best-state record, energy log -- is open)
template <int K> struct RoundsKernel {
    static constexpr bool diag = K & 1, best = K / 18;
    static constexpr int fmt = K / 2 % 3, arith = K / 6 % 3;
    static const void *get()
    {
        return reinterpret_cast<const void *>(k_rounds_fused<diag, fmt, arith != ARITH_F32, arith == ARITH_R64, best>);
    }
};
const void *rounds_kernel(bool diag, int fmt, int arith, bool best)
{
    return kernel_at<RoundsKernel>((((size_t)best * 3 + arith) * 3 + fmt) * 2 + (diag ? 1 : 0), std::make_index_sequence<36>{});
}

// the sweep-by-sweep kernels: k_sweep_stream, or k_sweep_philox<float | double, DIAG, PK> by {diag, pk, f64} (PK, the packed 16-bit
// schedule window: fp64 only)
template <int K> struct PhiloxKernel {
    static constexpr bool diag = K & 1, pk = K >> 1 & 1, f64 = K >> 2 & 1;
    static const void *get()
    {
        if constexpr (pk && !f64) return nullptr;
        else return reinterpret_cast<const void *>(k_sweep_philox<std::conditional_t<f64, double, float>, diag, pk>);
    }
};
const void *sweep_kernel(bool stream_mode, bool f64, bool diag, bool pk)
{
    if (stream_mode) return reinterpret_cast<const void *>(k_sweep_stream);
    return kernel_at<PhiloxKernel>((f64 ? 4 : 0) + (pk ? 2 : 0) + (diag ? 1 : 0), std::make_index_sequence<8>{});
}

// The SweepArgs fields every sweep launch sets: graph, chains and state, temperatures (`tab` with strides tab_cs / tab_ss; use_slots:
// its rows by temperature slot), random numbers, energy bookkeeping, running minimum.  The launchers add their own.
SweepArgs sweep_args(const nlmc_ctx *c, uint32_t sweep0, int n_sweeps, uint64_t seed, const double *tab, int tab_cs, int tab_ss,
                     bool use_slots)
{
    SweepArgs a{};
    a.g = c->g; a.chain_base = c->chain_base; a.chain_list = c->sub_list(); a.spins = c->spins.p;
    a.flags = c->has_flags ? c->flags.p : nullptr; a.temp_x = c->temp_x;
    a.n_sweeps = n_sweeps; a.sweep0 = sweep0; a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    a.tab = tab; a.tab_cs = tab_cs; a.tab_ss = tab_ss; a.slot_of_chain = use_slots ? c->slot_of_chain.p : nullptr;
    a.efix = c->efix.p; a.escale = c->escale; a.eshift = c->escale - c->qs; a.qinv = std::ldexp(1.0f, -c->qs); a.qinv64 = std::ldexp(1.0, -c->qs);
    a.rng_stride = c->rng_stride; a.rng_base = c->rng_base; a.rng_ladder_len = std::max(1, c->ladder_len);
    a.min_stride = c->track_min ? c->track_min_stride : 1; a.argmin = c->argmin.p;
    return a;
}

// What the two launchers on fused windows (run_fused, rounds_in_launch) set alike: the plan's layout and wave roles, the LDS carve-up
// of the launch, the range of the integer field.
void fused_args(const nlmc_ctx *c, const nlmc_ctx::FusedPlan &P, const FusedLds &L, SweepArgs &a)
{
    a.fz_pstride = P.pstride; a.fz_fmt = P.fmt; a.fz_qmask = c->knobs.no_quads ? 0xC000 : 0x8000;
    a.f_workers = P.workers; a.f_gen0 = P.gen0; a.f_gen_prio = c->knobs.no_prio ? 0 : 1;
#ifdef NLMC_DEBUG_KNOBS
    a.dbg_flags = c->knobs.dbg_flags;
#endif
    a.lds_neg_off = L.neg_off; a.lds_flags_off = L.flags_off; a.lds_u_off = L.u_off; a.lds_u_stride = L.u_bytes; a.lds_red_off = L.red_off;
    a.lds_snap_off = L.snap_off; a.lds_kt_off = L.kt_off; a.f64_xmax = c->xmax; a.f64_tie_mask = c->knobs.tie_mask;
}

// Does a fused launch read its item heads from the plan's head stream (fused_levels<.., HS>)?  The plain integer-field loops of an
// instance without a field term: head.y, which the stream does not carry, is 0 in every item.  Any other launch loads head[].
// And not a plan in the wide entry format, whose kernels have no such loop (fused_window: registers).  The plan was built with the
// stream exactly where these conditions on the context hold (fused_plan_stream).
bool head_stream(const nlmc_ctx *c, const nlmc_ctx::FusedPlan &P, bool outs, int arith)
{
    return P.has_hs && c->no_field && !outs && arith != ARITH_R64 && P.fmt != NLMC_FMT_WIDE && !c->knobs.no_head_stream;
}

// NLMC_STAMPS builds: the per-wave cycle sums of a launch of `rows` workgroups go to c->dbg, cleared on the launch's stream
int stamps_arm([[maybe_unused]] nlmc_ctx *c, [[maybe_unused]] SweepArgs &a, [[maybe_unused]] int rows, [[maybe_unused]] hipStream_t st)
{
#ifdef NLMC_STAMPS
    HIP_TRY(c, c->dbg.reserve((size_t)rows * 16 * 8 + 96));
    HIP_TRY(c, hipMemsetAsync(c->dbg.p, 0, ((size_t)rows * 16 * 8 + 96) * sizeof(long long), st));
    a.dbg = c->dbg.p;
#endif
    return NLMC_OK;
}

struct SweepOut {
    int record_stride;
    int8_t *out_spins;
    double *out_energy;
    double *out_min_energy;
    int32_t *out_argmin;
    int8_t *out_argmin_state;
};

// What a sweep call is, built once per call (run_sweeps, nlmc_pt_rounds_deferred) and read by the route drivers: n_sweeps sweeps from
// sweep0 on, the temperatures (`tab` with strides tab_cs / tab_ss; use_slots: its rows by temperature slot), the caller's orders and
// uniforms (stream mode), and what the sweeps leave in the context's device buffers besides the state (run_sweeps derives these from
// the caller's SweepOut): the energy trace, the running minimum, its state, a configuration every `rec` sweeps (0: none).
struct SweepCall {
    bool stream_mode; int precision, order_mode, n_sweeps; uint32_t sweep0; uint64_t seed;
    const double *tab; int tab_cs, tab_ss; bool use_slots;
    const uint32_t *keys_dev; const double *ustream_dev;
    bool want_energy, want_min, want_state; int rec;
    // per-sweep outputs, or a temperature per sweep: the output variant of the fused kernels
    bool outs() const { return want_energy || want_min || rec != 0 || tab_ss != 0; }
    int per_chain() const { return (stream_mode || order_mode == NLMC_ORDER_PER_CHAIN) ? 1 : 0; }
};

// sweep_args of the window of w sweeps that starts `at` sweeps into the call
SweepArgs window_args(const nlmc_ctx *c, const SweepCall &s, int at, int w)
{
    return sweep_args(c, s.sweep0 + (uint32_t)at, w, s.seed, s.tab + (size_t)at * s.tab_ss, s.tab_cs, s.tab_ss, s.use_slots);
}

// The per-sweep output fields of a launch whose sweeps are [t0, t0 + a.n_sweeps) of the call's: rows of the traces, the running minimum
// and its state in the context's device buffers (sized by run_sweeps).  `outs` false (the plain fused variant): none of them, a trace
// of the launch's own sweeps.
void sweep_outputs(const nlmc_ctx *c, const SweepCall &s, bool outs, int t0, SweepArgs &a)
{
    a.trace_sweeps = outs ? s.n_sweeps : a.n_sweeps;
    a.t0 = t0;
    a.rec_stride = s.rec ? s.rec : 1;
    if (!outs) return;
    a.etrace = s.want_energy ? c->etrace.p : nullptr;
    a.strace = s.rec ? c->strace.p : nullptr;
    a.emin = s.want_min ? c->emin.p : nullptr;
    a.best = (s.want_min && s.want_state) ? c->best.p : nullptr;
}

// One fused window on arithmetic `arith` (fused_route): window w of plan `slot`, `at` sweeps into the call.  Where the call has
// per-sweep outputs (SweepCall::outs) the launch also produces them, as sweeps [at, at + T) of the call.  `defer` (nullable): the
// previous round's swap decided in this launch's prologue (plain chains, no outputs: checked by the caller).
int run_fused(nlmc_ctx *c, const SweepCall &s, int slot, int w, int at, int arith, const DeferSwap *defer = nullptr,
              double *sink_override = nullptr)
{
    const nlmc_ctx::FusedPlan &P = c->fz[slot];
    const int R = c->sub_count(), T = P.T;
    const bool real = arith == ARITH_R64, outs = s.outs();
    if (real && !P.has_val) return fail(c, NLMC_ERR_STATE, "run_fused: the plan has no fp64 value plane");
    // per-sweep outputs: three snapshot slots in LDS when they fit beside the threshold tables, in global memory otherwise
    // (phase flags: K0 and K1; a temperature per sweep: one table per threshold slot)
    const int kt = arith == ARITH_F64 ? (c->has_flags ? 2 : s.tab_ss != 0 ? 3 : 1) * (2 * c->xmax + 1) : 0;
    const bool snap_lds = outs && fused_lds(c->n_pad, c->has_flags, true, P.fmt == NLMC_FMT_ADDR, kt).total <= (size_t)150 * 1024;
    const FusedLds L = fused_lds(c->n_pad, c->has_flags, snap_lds, P.fmt == NLMC_FMT_ADDR, kt);
    if (outs && !snap_lds) HIP_TRY(c, c->snap_g.reserve((size_t)R * (3 * (size_t)c->n_pad + 16)));
    const void *kfun = fused_kernel(c->has_diag, c->has_flags, outs, P.fmt, arith, defer != nullptr);
    if (!kfun) return fail(c, NLMC_ERR_STATE, "run_fused: no kernel for this combination (deferred swap with phase flags / outputs)");
    { int rc = ensure_lds(c, kfun, L.total); if (rc) return rc; }
    // events around the launch (two stream commands) only while timings accumulate (nlmc_timing_reset): every launch or
    // every ev_every-th one.  An event record costs ~2.5 us of stream time: none on the plain product path.
    const bool timed = c->ev_accumulate && (c->ev_every <= 1 || c->launches_total % c->ev_every == 0);
    TimerSpan ts;
    if (timed) { int rc = span_begin(c, ts, 1, c->cur); if (rc) return rc; }
    SweepArgs a = window_args(c, s, at, T);
    fused_args(c, P, L, a);
    const nlmc_ctx::FusedPlan::Arrays A = P.at(w);
    a.lvl_off = A.loff; a.nlev = A.nlev; a.hi_max = A.himax; a.fsend = A.send;
    a.ell32 = A.ell; a.head32 = A.head;
    const bool stream = head_stream(c, P, outs, arith);
    a.hs = stream ? A.hs : nullptr;
    if (w + 1 < P.windows && P.nlev_host[(size_t)w + 1] > 0 && !c->knobs.no_warm) {
        a.warm_head = stream ? reinterpret_cast<const int2 *>(P.at(w + 1).hs) : P.at(w + 1).head;
        a.warm_ell = P.at(w + 1).ell;
        a.fz_npos_next = P.npos_host[(size_t)w + 1];
        a.fz_nl_next = P.nlev_host[(size_t)w + 1];
    }
    a.energy_sink = sink_override ? sink_override : c->energy_sink;
    if (defer) a.defer = *defer;
    sweep_outputs(c, s, outs, outs ? at : 0, a);
    a.snap_g = (outs && !snap_lds) ? c->snap_g.p : nullptr;
    a.fz_val = real ? A.val : nullptr;
    { int rc = stamps_arm(c, a, R, c->cur); if (rc) return rc; }
    void *kargs[] = {&a};
    HIP_TRY(c, hipLaunchKernel(kfun, dim3(R), dim3(fused_block(c)), kargs, L.total, c->cur));
    HIP_TRY(c, hipGetLastError());
    { int rc = span_end(c, ts); if (rc) return rc; }
    count_launches(c, 1, timed);
    c->stat_fused_window = w;
    c->stat_fused_slot = slot;
    c->stat_head_path = stream ? NLMC_HEADS_STREAM : NLMC_HEADS_LOADS;
    return NLMC_OK;
}

// device result buffers of a sweep call -> the caller's host arrays.  Rows of the recorded traces are dense in the launch's
// blocks; minima / argmin states live in per-chain rows and are gathered through the subset's chain list.
int read_sweep_outputs(nlmc_ctx *c, const SweepOut &o, int n_sweeps, int rec, int n_rec)
{
    const int R = c->sub_count(), RA = c->n_chains, n = c->n;
    bool need_sync = false;
    std::vector<long long> h_ll;
    if (o.out_energy) {
        h_ll.resize((size_t)R * n_sweeps);
        HIP_TRY(c, hipMemcpyAsync(h_ll.data(), c->etrace.p, sizeof(long long) * h_ll.size(), hipMemcpyDeviceToHost, c->cur));
        need_sync = true;
    }
    std::vector<long long> h_min;
    std::vector<int32_t> h_arg, h_list;
    const bool gather = c->subset != 0 && (o.out_min_energy || o.out_argmin || o.out_argmin_state);
    if (gather) {
        h_list.resize((size_t)R);
        HIP_TRY(c, hipMemcpyAsync(h_list.data(), c->sub_list(), sizeof(int32_t) * R, hipMemcpyDeviceToHost, c->cur));
    }
    if (o.out_min_energy) {
        h_min.resize((size_t)RA);
        HIP_TRY(c, hipMemcpyAsync(h_min.data(), c->emin.p, sizeof(long long) * RA, hipMemcpyDeviceToHost, c->cur));
        need_sync = true;
    }
    if (o.out_argmin) {
        h_arg.resize((size_t)RA);
        HIP_TRY(c, hipMemcpyAsync(h_arg.data(), c->argmin.p, sizeof(int32_t) * RA, hipMemcpyDeviceToHost, c->cur));
        need_sync = true;
    }
    if (o.out_argmin_state) {
        int rc = rows_to_host_begin(c, c->best.p, RA);
        if (rc) return rc;
        need_sync = true;
    }
    if (rec) {
        HIP_TRY(c, hipMemcpyAsync(o.out_spins, c->strace.p, (size_t)R * n_rec * n, hipMemcpyDeviceToHost, c->cur));
        need_sync = true;
    }
    if (need_sync) HIP_TRY(c, hipStreamSynchronize(c->cur));
    auto row = [&](int i) { return gather ? (int)h_list[(size_t)i] : i; };
    if (o.out_argmin_state)
        for (int i = 0; i < R; ++i)
            std::memcpy(o.out_argmin_state + (size_t)i * n, c->stage_out.data() + (size_t)row(i) * c->n_pad, (size_t)n);
    const double inv = std::ldexp(1.0, -c->escale);
    if (o.out_energy) for (size_t i = 0; i < h_ll.size(); ++i) o.out_energy[i] = (double)h_ll[i] * inv;
    if (o.out_min_energy) for (int i = 0; i < R; ++i) o.out_min_energy[i] = (double)h_min[(size_t)row(i)] * inv;
    if (o.out_argmin) for (int i = 0; i < R; ++i) o.out_argmin[i] = h_arg[(size_t)row(i)];
    return NLMC_OK;
}

// the ladder's temperature table (-2 log2(e) {beta, beta / temp_x} per slot), uploaded on `st` only when temp_x changed since the
// last upload (no host sync on the hot path)
int upload_ladder_tab(nlmc_ctx *c, hipStream_t st)
{
    if (c->pt_tab_valid && c->pt_tab_temp_x == c->temp_x) return NLMC_OK;
    std::vector<double> tab((size_t)c->ladder_len * 2);
    for (int r = 0; r < c->ladder_len; ++r) {
        tab[2 * r + 0] = -2.0 * LOG2E * c->beta_list[r];
        tab[2 * r + 1] = -2.0 * LOG2E * (c->beta_list[r] / c->temp_x);
    }
    HIP_TRY(c, hipMemcpyAsync(c->pt_tab.p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    c->pt_tab_valid = true;
    c->pt_tab_temp_x = c->temp_x;
    return NLMC_OK;
}

// chain list of the selected subset, rebuilt (one small launch) after anything that moved chains between slots
int ensure_subset(nlmc_ctx *c)
{
    if (c->subset == 0 || !c->sub_dirty) return NLMC_OK;
    hipLaunchKernelGGL(k_subset_build, dim3(1), dim3(1024), 0, c->stream, c->n_chains, c->chain_base, c->slot_of_chain.p, c->slot_mark.p,
                       c->n_chains - c->n_marked_local, c->sub_list_buf.p);
    HIP_TRY(c, hipGetLastError());
    c->sub_dirty = false;
    return NLMC_OK;
}

// the fused plan slot whose windows cover sweeps [sweep0, sweep0 + n_sweeps) exactly, or -1
int fused_plan_for(const nlmc_ctx *c, uint32_t sweep0, int n_sweeps, uint64_t seed)
{
    for (int k = 0; k < 2; ++k) {
        const nlmc_ctx::FusedPlan &P = c->fz[k];
        if (!P.valid || P.seed != seed || sweep0 < P.sweep0 || (sweep0 - P.sweep0) % (uint32_t)P.T != 0 || n_sweeps % P.T != 0 ||
            (uint64_t)(sweep0 - P.sweep0) + (uint64_t)n_sweeps > (uint64_t)P.T * (uint64_t)P.windows)
            continue;
        const int w0 = (int)((sweep0 - P.sweep0) / (uint32_t)P.T), nw = n_sweeps / P.T;
        bool all_ok = true;
        for (int w = w0; w < w0 + nw; ++w) all_ok = all_ok && P.nlev_host[(size_t)w] > 0;
        if (all_ok) return k;
    }
    return -1;
}

// Chains whose state does not fit in LDS next to what the mode keeps there run the kernels of csrc/nlmc_big.h.  The LDS need is
// taken at its worst (phase flags on, one copy of the uniforms), so that the answer does not change during a context's life: a
// cached plan is in the format of the levelizer that goes with the answer.
bool sweeps_big(const nlmc_ctx *c, bool stream_mode, bool f64)
{
    if (c->big) return true;
    const size_t n4 = ((size_t)c->n + 3) / 4 * 4, u_bytes = stream_mode ? 0 : n4 * (f64 ? 8 : 4);
    return 2 * (size_t)c->n_pad + 32 + u_bytes + (size_t)NLMC_LCAP * 4 + 32 > (size_t)158 * 1024;
}

// The kernels for chains too long for LDS (csrc/nlmc_big.h), by arithmetic: the whole window in one launch, or one level per launch
const void *big_kernel(bool per_level, bool stream_mode, bool f64)
{
    static const void *const table[2][3] = {
        {reinterpret_cast<const void *>(k_sweep_big<NLMC_BIG_STREAM>), reinterpret_cast<const void *>(k_sweep_big<NLMC_BIG_F64>), reinterpret_cast<const void *>(k_sweep_big<NLMC_BIG_F32>)},
        {reinterpret_cast<const void *>(k_big_level<NLMC_BIG_STREAM>), reinterpret_cast<const void *>(k_big_level<NLMC_BIG_F64>), reinterpret_cast<const void *>(k_big_level<NLMC_BIG_F32>)}};
    return table[per_level ? 1 : 0][stream_mode ? 0 : f64 ? 1 : 2];
}

// What the routes with schedule or order scratch (sweep by sweep, short chains) do first: the scratch is shared with whatever the main
// stream is sweeping, so a call on the second stream waits for it; and an order per chain has no rows for a chain subset.  (Not the
// fused route: its plans are read-only.)
int scratch_route_begin(nlmc_ctx *c, const SweepCall &s)
{
    if (c->cur != c->stream) HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (s.per_chain() && c->subset != 0) return fail(c, NLMC_ERR_UNSUPPORTED, "chain subsets run shared-order philox sweeps only");
    return NLMC_OK;
}

// The sweep-by-sweep half of run_sweeps: windows of sweeps -> levelize (or the cached plan) -> the sweep kernel, one launch per window
// (chains too long for LDS: per window or per level).  The outputs stay in the context's device buffers.
int run_sweeps_stepwise(nlmc_ctx *c, const SweepCall &s)
{
    const int R = c->sub_count(), n = c->n, n_sweeps = s.n_sweeps, per_chain = s.per_chain();
    { int rc = scratch_route_begin(c, s); if (rc) return rc; }
    // plan cache hit?
    const bool f64 = s.stream_mode || s.precision == NLMC_F64;
    const bool big = sweeps_big(c, s.stream_mode, f64);      // spins stay in global memory (csrc/nlmc_big.h)
    const int ell_mode = big ? -1 : s.stream_mode ? 0 : (f64 ? 2 : 1);
    const bool cached = !s.stream_mode && c->plan_valid && c->plan_mode == s.order_mode && c->plan_seed == s.seed && c->plan_big == big &&
                        c->plan_precision == s.precision && !per_chain && s.sweep0 >= c->plan_sweep0 &&
                        (uint64_t)s.sweep0 + (uint64_t)n_sweeps <= (uint64_t)c->plan_sweep0 + (uint64_t)c->plan_count;
    // window size: keep the schedule scratch under ~256 MiB
    const size_t per_sweep_orders = per_chain ? (size_t)R : 1;
    const size_t item_bytes = big ? 8 + 12 : ell_mode == 1 ? 8 + 8 + 8 * NLMC_ELL_W32 : (ell_mode == 2 ? 8 + 8 + 12 * NLMC_ELL_W : 8);
    const size_t bytes_per_sweep = per_sweep_orders * ((size_t)n * item_bytes + (size_t)(n + 1) * 4 + 4);
    int W = n_sweeps;
    if (!cached) {
        // stream mode indexes its uniforms/keys by (chain, sweep) over the WHOLE call -> single window there
        if (!s.stream_mode) W = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_sweeps, ((size_t)256 << 20) / bytes_per_sweep));
        const size_t orders = per_sweep_orders * (size_t)W;
        if (big) HIP_TRY(c, c->scratch.reserve_big(orders, (size_t)n, !s.stream_mode));
        else HIP_TRY(c, c->scratch.reserve(orders, (size_t)n, ell_mode));
    }

    const int nt = big ? 1024 : sweep_block_for(c, !s.stream_mode && f64, !s.stream_mode && !f64 && c->has_diag);
    const StepLds L = step_lds(c, s.stream_mode, f64);
    const void *kfun = sweep_kernel(s.stream_mode, f64, c->has_diag, f64 && c->f64_pack16);
    if (!big) { int rc = ensure_lds(c, kfun, L.total); if (rc) return rc; }
    // chains too long for LDS (csrc/nlmc_big.h): enough of them to fill the chip -> one workgroup per chain for the whole
    // window (its spins stay in that CU's L1 from level to level); few -> one launch per level over all chains, so that a
    // single chain of a million spins still uses every CU (NLMC_BIG_PER_LEVEL = 0 / 1: test knob)
    bool per_level = false;
    const void *kbig = nullptr;
    if (big) {
        { int rc = cu_count(c); if (rc) return rc; }
        per_level = (long long)R * 8 <= c->n_cu;
        if (c->knobs.big_per_level >= 0) per_level = c->knobs.big_per_level != 0;
        if (R > 65535) per_level = false;
        kbig = big_kernel(per_level, s.stream_mode, f64);
    }

    for (int t0 = 0; t0 < n_sweeps; t0 += W) {
        const int w = std::min(W, n_sweeps - t0);
        const nlmc_ctx::Sched &sc = cached ? c->plan : c->scratch;
        size_t o0 = 0;
        TimerSpan ts;
        if (c->ev_accumulate) { int rc = span_begin(c, ts, 0, c->cur); if (rc) return rc; }
        if (cached) {
            o0 = (size_t)(s.sweep0 - c->plan_sweep0) + t0;
        } else {
            const int n_orders = (int)per_sweep_orders * w;
            int rc = run_levelize(c, n_orders, s.keys_dev, per_chain, w, s.sweep0 + (uint32_t)t0, s.seed, c->scratch, ell_mode);
            if (rc) return rc;
            c->stats_nlev_ptr = c->scratch.nlev.p;
            c->stats_nlev_count = n_orders;
            c->stats_pending = true;
        }
        { int rc = span_mid(c, ts); if (rc) return rc; }

        SweepArgs a = window_args(c, s, t0, w);
        a.ord2 = sc.order.p + o0 * n;
        a.lvl_off = sc.lvl_off.p + o0 * (size_t)(n + 1);
        a.nlev = sc.nlev.p + o0;
        a.hi_max = sc.hi_max.p + o0;
        if (ell_mode == 1) { a.ell32 = sc.ell32.p + o0 * (size_t)n * NLMC_ELL_W32; a.head32 = sc.head32.p + o0 * n; }
        if (ell_mode == 2) {
            a.ellc64 = sc.ellc64.p + o0 * (size_t)n * NLMC_ELL_W;
            a.ellv64 = sc.ellv64.p + o0 * (size_t)n * NLMC_ELL_W;
            a.headh64 = sc.headh64.p + o0 * n;
        }
        a.per_chain = per_chain;
        a.ustream = s.ustream_dev;
        a.energy_sink = c->energy_sink;
        sweep_outputs(c, s, true, t0, a);
        { int rc = stamps_arm(c, a, R, c->cur); if (rc) return rc; }
        a.lds_u_stride = L.dbuf ? L.u_bytes : 0;
        a.lds_loff_stride = L.dbuf ? NLMC_LCAP * 4 : 0;
        a.lds_flags_off = L.flags_off; a.lds_u_off = L.u_off; a.lds_loff_off = L.loff_off; a.lds_red_off = L.red_off;
        void *kargs[] = {&a};
        if (big && !per_level) {
            HIP_TRY(c, hipLaunchKernel(kbig, dim3(R), dim3(1024), kargs, 0, c->cur));
        } else if (big) {
            // the numbers of levels come back first
            const size_t n_ord = per_sweep_orders * (size_t)w;
            std::vector<int32_t> nlev_h(n_ord);
            HIP_TRY(c, hipMemcpyAsync(nlev_h.data(), a.nlev, sizeof(int32_t) * n_ord, hipMemcpyDeviceToHost, c->cur));
            HIP_TRY(c, hipStreamSynchronize(c->cur));
            HIP_TRY(c, c->big_esum.reserve((size_t)R));
            HIP_TRY(c, hipMemsetAsync(c->big_esum.p, 0, sizeof(long long) * (size_t)R, c->cur));
            const bool per_sweep_out = a.etrace || a.emin || a.strace;
            const unsigned gx = (unsigned)std::max(1, std::min(256, (n / 16 + 255) / 256));
            for (int t = 0; t < w; ++t) {
                int nl = 0;
                if (per_chain) for (size_t q = 0; q < per_sweep_orders; ++q) nl = std::max(nl, nlev_h[q * (size_t)w + t]);
                else nl = nlev_h[(size_t)t];
                for (int l = 0; l < nl; ++l) {
                    void *largs[] = {&a, &t, &l, &c->big_esum.p};
                    HIP_TRY(c, hipLaunchKernel(kbig, dim3(gx, R), dim3(256), largs, 0, c->cur));
                }
                if (per_sweep_out || t == w - 1) hipLaunchKernelGGL(k_big_sweep_end, dim3(R), dim3(1024), 0, c->cur, a, t, c->big_esum.p);
                HIP_TRY(c, hipGetLastError());
            }
        } else {
            HIP_TRY(c, hipLaunchKernel(kfun, dim3(R), dim3(nt), kargs, L.total, c->cur));
        }
        HIP_TRY(c, hipGetLastError());
        { int rc = span_end(c, ts); if (rc) return rc; }
        count_launches(c, 1, c->ev_accumulate);
    }
    return NLMC_OK;
}

// Whether a philox call over R rows takes the chain-per-lane kernels (nlmc_set_lane_sweeps): forced, whenever the chain fits; auto,
// below the fused windows' floor from NLMC_LANE_AUTO_ROWS rows on (include/nlmc.h: where the route was measured ahead)
bool lanes_route(const nlmc_ctx *c, int R)
{
    if (c->knobs.force_big || c->n > NLMC_LANE_N) return false;
    if (c->lane_mode == 2) return true;
    return c->lane_mode == 1 && c->n < 256 && R >= NLMC_LANE_AUTO_ROWS;
}

// LDS of k_sweep_lanes: transposed spins | transposed flags | (where it fits) one sweep's random numbers, a word per (spin, lane)
struct LaneLds { int flags_off, u_off; bool tab; size_t total; };
LaneLds lane_lds(const nlmc_ctx *c)
{
    LaneLds L{};
    const size_t plane = (size_t)c->n_pad * NLMC_LANE_STRIDE;
    L.flags_off = (int)plane;
    const size_t state = plane * (c->has_flags ? 2 : 1), tab = (size_t)((c->n + 3) / 4 * 4) * 256;
    L.u_off = (int)state;
    // the table where four waves still share a compute unit (one per SIMD): 40 KB per wave
    L.tab = c->knobs.lane_rng != 0 && state + tab <= (size_t)40 * 1024;
    L.total = state + (L.tab ? tab : 0);
    return L;
}

const void *lanes_kernel(bool f64, bool per_chain)
{
    static const void *const table[2][2] = {
        {reinterpret_cast<const void *>(k_sweep_lanes<false, false>), reinterpret_cast<const void *>(k_sweep_lanes<false, true>)},
        {reinterpret_cast<const void *>(k_sweep_lanes<true, false>), reinterpret_cast<const void *>(k_sweep_lanes<true, true>)}};
    return table[f64 ? 1 : 0][per_chain ? 1 : 0];
}

const void *rounds_lanes_kernel(bool f64, bool observed)
{
    static const void *const table[2][2] = {
        {reinterpret_cast<const void *>(k_rounds_lanes<false, false>), reinterpret_cast<const void *>(k_rounds_lanes<false, true>)},
        {reinterpret_cast<const void *>(k_rounds_lanes<true, false>), reinterpret_cast<const void *>(k_rounds_lanes<true, true>)}};
    return table[f64 ? 1 : 0][observed ? 1 : 0];
}

const void *apt_lanes_kernel(bool f64, bool elog)
{
    static const void *const table[2][2] = {
        {reinterpret_cast<const void *>(k_apt_rounds_lanes<false, false>), reinterpret_cast<const void *>(k_apt_rounds_lanes<false, true>)},
        {reinterpret_cast<const void *>(k_apt_rounds_lanes<true, false>), reinterpret_cast<const void *>(k_apt_rounds_lanes<true, true>)}};
    return table[f64 ? 1 : 0][elog ? 1 : 0];
}

// k_lane_orders: the n_orders visiting orders of a lane launch into c->lane_perm (or `perm`), n_sweeps from sweep0 on (per_chain: for
// each chain).
int launch_lane_orders(nlmc_ctx *c, hipStream_t st, size_t n_orders, int n_sweeps, int per_chain, uint32_t sweep0, uint64_t seed,
                       uint16_t *perm = nullptr)
{
    LaneOrderArgs oa{};
    oa.n = c->n; oa.n_sweeps = n_sweeps; oa.per_chain = per_chain; oa.chain_base = c->chain_base;
    oa.seed_lo = (uint32_t)seed; oa.seed_hi = (uint32_t)(seed >> 32); oa.sweep0 = sweep0;
    oa.perm = perm ? perm : c->lane_perm.p;
    hipLaunchKernelGGL(k_lane_orders, dim3((unsigned)n_orders), dim3(256), 0, st, oa);
    HIP_TRY(c, hipGetLastError());
    c->stat_lane_orders += (int64_t)n_orders;
    return NLMC_OK;
}

// The SweepArgs fields every lane kernel reads besides those of sweep_args: `rows` chains, the orders launch_lane_orders wrote, the
// random-number table at LDS offset u_off where there is one.
void lane_fields(const nlmc_ctx *c, SweepArgs &a, int rows, bool tab, size_t u_off)
{
    a.energy_sink = c->energy_sink;
    a.lane_perm = c->lane_perm.p; a.lane_rows = rows; a.lane_diag = c->has_diag ? 1 : 0; a.lane_tab = tab ? 1 : 0;
    a.lds_u_off = (int)u_off;
}

// What a short-chain route supplies to run_sweeps_short: its kernel with dynamic LDS, grid and block (LDS limit raised, whatever the
// kernel reads once per context in place), and the SweepArgs fields of its own -- lanes: the flags plane and the random-number table
// (lane_lds); waves: the dense matrix.  The rest stay zero.
struct ShortRoute { const void *kfun; size_t lds; dim3 grid, block; int lds_flags_off; bool tab; size_t u_off; const int32_t *wave_J; };

// k_sweep_lanes: a chain per lane, 64 to a workgroup of one wave
int lanes_sweeps(nlmc_ctx *c, const SweepCall &s, ShortRoute &r)
{
    const LaneLds L = lane_lds(c);
    r.kfun = lanes_kernel(s.precision == NLMC_F64, s.per_chain() != 0);
    r.lds = L.total; r.grid = dim3((unsigned)((c->sub_count() + 63) / 64)); r.block = dim3(64);
    r.lds_flags_off = L.flags_off; r.tab = L.tab; r.u_off = (size_t)L.u_off;
    return ensure_lds(c, r.kfun, r.lds);
}

// Whether a philox call over R rows takes the wave-per-chain kernels (nlmc_set_wave_sweeps): fixed point only, chains of at most
// NLMC_WAVE_N spins (NLMC_WAVE_LONG_N under nlmc_set_wave_long); forced, every such call; auto, up to NLMC_WAVE_AUTO_MAX_ROWS rows
// (include/nlmc.h: where the route was measured ahead).  A call it does not take goes on to the lane rule and the rest: never an error.
bool waves_route(const nlmc_ctx *c, int R, int precision)
{
    if (c->wave_mode == 0 || precision != NLMC_F32 || c->knobs.force_big || c->n > (c->wave_long ? NLMC_WAVE_LONG_N : NLMC_WAVE_N)) return false;
    return c->wave_mode == 2 || (long long)R <= (long long)NLMC_WAVE_AUTO_MAX_ROWS;
}

// Row of a wave kernel table: R = 1, 2, 4, 8, 16 fields per lane (nlmc_wave_fields)
int wave_fields_row(int R) { return R == 1 ? 0 : R == 2 ? 1 : R == 4 ? 2 : R == 8 ? 3 : 4; }

// k_sweep_waves<R, jlds> for R <= 4, k_sweep_waves_long<R, ahead> beyond
const void *waves_kernel(int R, bool variant)
{
    static const void *const table[5][2] = {
        {reinterpret_cast<const void *>(k_sweep_waves<1, false>), reinterpret_cast<const void *>(k_sweep_waves<1, true>)},
        {reinterpret_cast<const void *>(k_sweep_waves<2, false>), reinterpret_cast<const void *>(k_sweep_waves<2, true>)},
        {reinterpret_cast<const void *>(k_sweep_waves<4, false>), reinterpret_cast<const void *>(k_sweep_waves<4, true>)},
        {reinterpret_cast<const void *>(k_sweep_waves_long<8, false>), reinterpret_cast<const void *>(k_sweep_waves_long<8, true>)},
        {reinterpret_cast<const void *>(k_sweep_waves_long<16, false>), reinterpret_cast<const void *>(k_sweep_waves_long<16, true>)}};
    return table[wave_fields_row(R)][variant ? 1 : 0];
}

// The dense matrix of the wave kernels, once per context (the couplings of a context never change).  Built on the stream of the
// first wave call and waited for, so that a later call on the other stream finds it complete.
int ensure_wave_matrix(nlmc_ctx *c, size_t stride)
{
    if (c->wave_J_built) return NLMC_OK;
    const size_t count = (size_t)c->n * stride;
    HIP_TRY(c, c->wave_J.reserve(count));
    HIP_TRY(c, hipMemsetAsync(c->wave_J.p, 0, count * sizeof(int32_t), c->cur));
    WaveMatrixArgs m{};
    m.n = c->n; m.stride = (int)stride; m.rowptr = c->g.rowptr; m.edge32 = c->g.edge32; m.Jd = c->wave_J.p;
    hipLaunchKernelGGL(k_wave_matrix, dim3((unsigned)c->n), dim3(64), 0, c->cur, m);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->cur));
    c->wave_J_built = true;
    return NLMC_OK;
}

// A chain per wave over the dense matrix, in the shape csrc/nlmc_wave_shape.h picks for the device: k_sweep_waves (nlmc_wave_shape), or
// k_sweep_waves_long for chains of more than NLMC_WAVE_N spins (nlmc_wave_long_shape)
int waves_sweeps(nlmc_ctx *c, const SweepCall &, ShortRoute &r)
{
    { int rc = cu_count(c); if (rc) return rc; }
    const bool longs = c->n > NLMC_WAVE_N;
    const NlmcWaveShape S = longs ? nlmc_wave_long_shape(c->n, c->n_pad, c->sub_count(), c->n_cu, c->knobs.wave_waves)
                                  : nlmc_wave_shape(c->n, c->n_pad, c->sub_count(), c->n_cu, c->knobs.wave_waves, c->knobs.wave_jlds ? 1 : 0);
    if (S.R == 0) return fail(c, NLMC_ERR_STATE, "waves_sweeps: the chain does not fit the wave kernels");
    r.kfun = waves_kernel(S.R, longs ? c->knobs.wave_long_ahead : S.jlds != 0);
    r.lds = S.lds; r.grid = dim3((unsigned)S.blocks); r.block = dim3((unsigned)(64 * S.W));
    { int rc = ensure_lds(c, r.kfun, r.lds); if (rc) return rc; }
    { int rc = ensure_wave_matrix(c, S.stride); if (rc) return rc; }
    r.wave_J = c->wave_J.p;
    return NLMC_OK;
}

// The short-chain half of run_sweeps (`route`: lanes_sweeps, waves_sweeps): windows of sweeps -> k_lane_orders (the "levelize" half of
// the timings) -> the route's kernel, one launch per window.  Windows are cut against the order scratch (NLMC_LANE_SCRATCH), as those
// of run_sweeps_stepwise against its bound.  The outputs stay in the context's buffers.
int run_sweeps_short(nlmc_ctx *c, const SweepCall &s, int (*route)(nlmc_ctx *, const SweepCall &, ShortRoute &))
{
    const int R = c->sub_count(), per_chain = s.per_chain();
    { int rc = scratch_route_begin(c, s); if (rc) return rc; }
    const size_t per_sweep_orders = per_chain ? (size_t)R : 1;
    const size_t bytes_per_sweep = per_sweep_orders * (size_t)c->n * sizeof(uint16_t);
    const int W = (int)std::max<size_t>(1, std::min<size_t>((size_t)s.n_sweeps, c->knobs.lane_scratch / bytes_per_sweep));
    if (per_sweep_orders * (size_t)W > (size_t)INT_MAX) return fail(c, NLMC_ERR_UNSUPPORTED, "too many per-chain orders in one window");
    HIP_TRY(c, c->lane_perm.reserve(per_sweep_orders * (size_t)W * (size_t)c->n));
    ShortRoute r{};
    { int rc = route(c, s, r); if (rc) return rc; }
    for (int t0 = 0; t0 < s.n_sweeps; t0 += W) {
        const int w = std::min(W, s.n_sweeps - t0);
        TimerSpan ts;
        if (c->ev_accumulate) { int rc = span_begin(c, ts, 0, c->cur); if (rc) return rc; }
        { int rc = launch_lane_orders(c, c->cur, per_sweep_orders * (size_t)w, w, per_chain, s.sweep0 + (uint32_t)t0, s.seed); if (rc) return rc; }
        { int rc = span_mid(c, ts); if (rc) return rc; }

        SweepArgs a = window_args(c, s, t0, w);
        lane_fields(c, a, R, r.tab, r.u_off);
        a.per_chain = per_chain;
        a.lds_flags_off = r.lds_flags_off;
        a.wave_J = r.wave_J;
        sweep_outputs(c, s, true, t0, a);
        void *kargs[] = {&a};
        HIP_TRY(c, hipLaunchKernel(r.kfun, r.grid, r.block, kargs, r.lds, c->cur));
        HIP_TRY(c, hipGetLastError());
        { int rc = span_end(c, ts); if (rc) return rc; }
        count_launches(c, 1, c->ev_accumulate);
    }
    return NLMC_OK;
}

// Shared driver: completes the call's descriptor (the output wishes, from `o` and nlmc_track_minimum), picks the route, runs its driver
// and reads the outputs back.
int run_sweeps(nlmc_ctx *c, SweepCall s, const SweepOut &o)
{
    const int R = c->sub_count(), n = c->n, n_sweeps = s.n_sweeps;
    begin_sweep_call(c);
    c->stat_orders = 0;
    c->stat_levels = 0;
    c->stats_pending = false;
    c->strace_nrec = 0;
    c->strace_rows = 0;
    c->stat_lane_orders = 0;
    if (R == 0 || n_sweeps == 0) return NLMC_OK;
    { int rc = ensure_subset(c); if (rc) return rc; }
    // running minimum + argmin state: asked for through host outputs, or kept on the device for the hand-off between NMC
    // phases (nlmc_track_minimum; NMC/nmc.py:394-395)
    s.want_energy = o.out_energy != nullptr;
    s.want_min = o.out_min_energy || o.out_argmin || o.out_argmin_state || c->track_min;
    s.want_state = o.out_argmin_state || c->track_min;
    c->stat_fused_window = -1;
    s.rec = o.out_spins ? std::max(1, o.record_stride) : 0;
    const int n_rec = s.rec ? (n_sweeps + s.rec - 1) / s.rec : 0;
    // Fused-window schedule: planned ahead (nlmc_plan_philox_fused), same results.  Calls without per-sweep outputs
    // and with one temperature per chain take the plain variant; calls WITH outputs (energy trace, running minimum /
    // argmin state, recorded configurations) or a temperature per sweep take the output variant (its three snapshot slots in
    // LDS or, for large n, in a global ring: run_fused); any whole number of planned windows per call either way.  Which calls
    // run there, and on which arithmetic: fused_route.
    const int fslot = fused_plan_for(c, s.sweep0, n_sweeps, s.seed);
    int arith = fslot < 0 ? NOT_FUSED : fused_route(c, s.precision, s.order_mode, s.tab_ss != 0, c->has_flags, fslot, c->fz[fslot].T, Via::sweeps);
    if (s.outs() && c->knobs.no_fused_out) arith = NOT_FUSED;
    const bool waves = !s.stream_mode && waves_route(c, R, s.precision);   // short chains, one per wave (csrc/nlmc_waves.h): asked first
    const bool lanes = !waves && !s.stream_mode && lanes_route(c, R);      // short chains, one per lane (csrc/nlmc_lanes.h): before the fused windows
    if (lanes || waves) arith = NOT_FUSED;
    c->last_route = waves ? NLMC_ROUTE_WAVES : lanes ? NLMC_ROUTE_LANES : arith != NOT_FUSED ? NLMC_ROUTE_FUSED : NLMC_ROUTE_STEPWISE;
    if (o.out_energy) HIP_TRY(c, c->etrace.reserve((size_t)R * n_sweeps));
    if (s.rec) HIP_TRY(c, c->strace.reserve((size_t)R * n_rec * n));
    c->strace_nrec = n_rec;
    c->strace_rows = s.rec ? R : 0;
    if (s.want_min) {
        hipLaunchKernelGGL(k_fill_min, dim3((R + 255) / 256), dim3(256), 0, c->cur, R, c->sub_list(), c->emin.p, c->argmin.p);
        HIP_TRY(c, hipGetLastError());
    }
    int rc = NLMC_OK;
    if (arith != NOT_FUSED) {
        const nlmc_ctx::FusedPlan &P = c->fz[fslot];
        const int w0 = (int)((s.sweep0 - P.sweep0) / (uint32_t)P.T), nw = n_sweeps / P.T;
        for (int j = 0; j < nw && !rc; ++j) rc = run_fused(c, s, fslot, w0 + j, j * P.T, arith);
    } else if (waves || lanes) {
        rc = run_sweeps_short(c, s, waves ? waves_sweeps : lanes_sweeps);
    } else {
        rc = run_sweeps_stepwise(c, s);
    }
    if (rc) return rc;
    return read_sweep_outputs(c, o, n_sweeps, s.rec, n_rec);
}

// ---- RCCL, bound at run time (dlopen): a process that never shards a ladder over GPUs needs no librccl -----------------
// The library the process already holds (PyTorch ships one under the same soname) is reused.
struct Rccl {
    typedef struct { char internal[128]; } UniqueId;                      // ncclUniqueId (NCCL_UNIQUE_ID_BYTES = 128)
    int (*GetUniqueId)(UniqueId *) = nullptr;
    int (*CommInitRank)(void **, int, UniqueId, int) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*CommGetAsyncError)(void *, int *) = nullptr;
    int (*CommAbort)(void *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool tried = false, ok = false;
    std::string why;
};
Rccl g_rccl;

bool rccl_load()
{
    Rccl &r = g_rccl;
    if (r.tried) return r.ok;
    r.tried = true;
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) { r.why = std::string("librccl.so.1 could not be loaded: ") + (dlerror() ? dlerror() : "?"); return false; }
    r.GetUniqueId = reinterpret_cast<int (*)(Rccl::UniqueId *)>(dlsym(h, "ncclGetUniqueId"));
    r.CommInitRank = reinterpret_cast<int (*)(void **, int, Rccl::UniqueId, int)>(dlsym(h, "ncclCommInitRank"));
    r.AllGather = reinterpret_cast<int (*)(const void *, void *, size_t, int, void *, hipStream_t)>(dlsym(h, "ncclAllGather"));
    r.CommDestroy = reinterpret_cast<int (*)(void *)>(dlsym(h, "ncclCommDestroy"));
    r.GetErrorString = reinterpret_cast<const char *(*)(int)>(dlsym(h, "ncclGetErrorString"));
    r.Send = reinterpret_cast<int (*)(const void *, size_t, int, int, void *, hipStream_t)>(dlsym(h, "ncclSend"));
    r.Recv = reinterpret_cast<int (*)(void *, size_t, int, int, void *, hipStream_t)>(dlsym(h, "ncclRecv"));
    r.GroupStart = reinterpret_cast<int (*)()>(dlsym(h, "ncclGroupStart"));
    r.GroupEnd = reinterpret_cast<int (*)()>(dlsym(h, "ncclGroupEnd"));
    r.CommGetAsyncError = reinterpret_cast<int (*)(void *, int *)>(dlsym(h, "ncclCommGetAsyncError"));
    r.CommAbort = reinterpret_cast<int (*)(void *)>(dlsym(h, "ncclCommAbort"));
    r.ok = r.GetUniqueId && r.CommInitRank && r.AllGather && r.CommDestroy && r.Send && r.Recv && r.GroupStart && r.GroupEnd &&
           r.CommGetAsyncError && r.CommAbort;
    if (!r.ok) r.why = "librccl.so.1 lacks one of ncclGetUniqueId / ncclCommInitRank / ncclAllGather / ncclSend / ncclRecv / ncclGroupStart / "
                       "ncclGroupEnd / ncclCommGetAsyncError / ncclCommAbort / ncclCommDestroy";
    return r.ok;
}

std::string rccl_err(int rc) { return g_rccl.GetErrorString ? std::string(g_rccl.GetErrorString(rc)) : ("ncclResult " + std::to_string(rc)); }

int rows_to_device(nlmc_ctx *c, void *dst_dev, const void *src_host, int rows)
{
    const size_t n = (size_t)c->n, np = (size_t)c->n_pad;
    const void *src = src_host;
    if (n != np) {
        c->stage_in.assign(np * rows, 0);
        for (int r = 0; r < rows; ++r) std::memcpy(c->stage_in.data() + r * np, (const uint8_t *)src_host + r * n, n);
        src = c->stage_in.data();
    }
    HIP_TRY(c, hipMemcpyAsync(dst_dev, src, np * rows, hipMemcpyHostToDevice, c->stream));
    if (n != np) HIP_TRY(c, hipStreamSynchronize(c->stream));      // the staging buffer is reused by the next call
    return NLMC_OK;
}

int rows_to_host_begin(nlmc_ctx *c, const void *src_dev, int rows)
{
    c->stage_out.resize((size_t)c->n_pad * rows);
    HIP_TRY(c, hipMemcpyAsync(c->stage_out.data(), src_dev, c->stage_out.size(), hipMemcpyDeviceToHost, c->cur));
    return NLMC_OK;
}

void rows_to_host_finish(nlmc_ctx *c, void *dst_host, int rows)
{
    const size_t n = (size_t)c->n, np = (size_t)c->n_pad;
    for (int r = 0; r < rows; ++r) std::memcpy((uint8_t *)dst_host + r * n, c->stage_out.data() + r * np, n);
}

// threads of a swap workgroup: one lane per selected pair when the selection is planned (the in-kernel selection is written for ONE wave)
int swap_block(bool planned, int n_pairs) { return std::max(64, planned ? std::min(256, (n_pairs + 63) / 64 * 64) : 64); }

// Where one swap round (k_pt_swap, k_apt_swap; `rows` ladders wide) writes its pairs and decisions and finds its planned selection: the
// round's rows of the device-side log (read back once: nlmc_pt_log_read) unless the caller wants them on the host now, of the plan
template <typename Args> void swap_window_rows(nlmc_ctx *c, Args &a, uint32_t round, uint64_t seed, int n_pairs, size_t rows, bool to_host)
{
    if (c->pt_log.covers(round, 1, n_pairs) && !to_host) {
        a.out_pairs = c->pt_log_pairs.p + c->pt_log.row(round) * rows * n_pairs * 2;
        a.out_acc = c->pt_log_acc.p + c->pt_log.row(round) * rows * n_pairs;
    }
    if (c->pt_plan.covers(round, 1, n_pairs, seed)) {
        a.plan_pairs = c->pt_plan_pairs.p + c->pt_plan.row(round) * rows * n_pairs * 2;
        a.plan_ok = c->pt_plan_ok.p + c->pt_plan.row(round) * rows;
    }
}

// The tail of a swap launch whose caller asked for the pairs or the decisions of its `rows` ladders: they come back with the status word,
// and a selection that ran out of pairs is reported (and the status cleared).
int swap_read_back(nlmc_ctx *c, int rows, int n_pairs, int32_t *out_pairs, uint8_t *out_accepted)
{
    if (!out_pairs && !out_accepted) return NLMC_OK;
    int32_t st = 0;
    if (out_pairs) HIP_TRY(c, hipMemcpyAsync(out_pairs, c->pt_pairs.p, sizeof(int32_t) * (size_t)rows * n_pairs * 2, hipMemcpyDeviceToHost, c->stream));
    if (out_accepted) HIP_TRY(c, hipMemcpyAsync(out_accepted, c->pt_acc.p, (size_t)rows * n_pairs, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&st, c->pt_status.p, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (st != 0) {
        HIP_TRY(c, hipMemsetAsync(c->pt_status.p, 0, sizeof(int32_t), c->stream));
        return fail(c, NLMC_ERR_ARG, "Cannot find non-overlapping pairs.");
    }
    return NLMC_OK;
}

}  // namespace

extern "C" {

static int ensure_adjacency(nlmc_ctx *c);
int nlmc_pt_check(nlmc_ctx *c);

int nlmc_abi_version(void) { return NLMC_ABI_VERSION; }

int nlmc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *nlmc_last_error(const nlmc_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int nlmc_create(nlmc_ctx **out, int device, void *hip_stream, int n, int64_t nnz, const int32_t *rowptr,
                const int32_t *colidx, const double *vals, const double *h, int n_chains, int chain_base,
                int n_chains_global)
{
    NlmcInstance I;     // every instance error comes before the device is asked for
    const int irc = nlmc_instance_prepare(I, out, n, nnz, rowptr, colidx, vals, h, n_chains, chain_base, n_chains_global, NLMC_FZ_W);
    if (out) *out = nullptr;
    if (irc != NLMC_OK) return fail(nullptr, irc, I.err);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, NLMC_ERR_HIP, "nlmc_create: no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(nullptr, NLMC_ERR_ARG, "nlmc_create: device index out of range");

    nlmc_ctx *c = new nlmc_ctx();
    auto bail = [&](int code) { g_create_error = c->err; nlmc_destroy(c); return code; };
#define CT(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { c->err = std::string(#expr) + ": " + hipGetErrorString(e__); return bail(NLMC_ERR_HIP); } } while (0)
    CT(hipSetDevice(device));
    c->device = device;
    c->stream = reinterpret_cast<hipStream_t>(hip_stream);
    c->cur = c->stream;
    c->n = n;
    c->knobs = read_knobs();
    c->big = n > NLMC_LDS_N || c->knobs.force_big;
    c->n_pad = (n + 15) / 16 * 16;
    c->nnz = nnz;
    c->n_chains = n_chains;
    c->chain_base = chain_base;
    c->n_chains_global = n_chains_global;
    c->has_diag = I.has_diag;
    c->has_zero_vals = I.has_zero_vals;
    c->max_deg = I.max_deg;
    c->n_long = I.n_gt1 + (c->knobs.no_quads ? 0 : 2 * I.n_gt2);
    c->qs = I.qs;
    c->escale = I.escale;
    c->xmax = I.xmax;
    c->compact16 = I.fits16 && !c->knobs.no_compact;
    c->f64_pack16 = I.fits16 && I.exact_q && n <= 65535 && !c->knobs.no_pack64;
    c->sign8 = c->compact16 && I.pm1 && nnz > 0 && !c->knobs.no_signfmt;
    c->f64_exact = I.exact_q && I.exact_h;
    c->no_field = I.no_field;

    size_t total = 256, off = 0;
    c->arena_buffers([&](auto &buf, size_t count) { total += buf.arena_bytes(count); });
    CT(c->arena.reserve(total));
    c->arena_buffers([&](auto &buf, size_t count) { buf.borrow(c->arena.p, off, count); });
    assert(off <= total);
    // everything zero (padding, states, flags, tracked energies), then the instance: stream-ordered, ONE wait (the host arrays
    // handed to the copies are the caller's and this function's own: both outlive the wait)
    CT(hipMemsetAsync(c->arena.p, 0, total, c->stream));
    CT(hipMemcpyAsync(c->rowptr.p, rowptr, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream));
    if (nnz > 0) {
        CT(hipMemcpyAsync(c->col.p, colidx, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, c->stream));
        CT(hipMemcpyAsync(c->val64.p, vals, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, c->stream));
        CT(hipMemcpyAsync(c->edge32.p, I.e32.data(), sizeof(EdgeQ) * (size_t)nnz, hipMemcpyHostToDevice, c->stream));
    }
    CT(hipMemcpyAsync(c->h64.p, h, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    CT(hipMemcpyAsync(c->hq.p, I.hq.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    CT(hipStreamSynchronize(c->stream));

    c->g.n = n; c->g.n_pad = c->n_pad;
    c->g.rowptr = c->rowptr.p; c->g.col = c->col.p; c->g.val64 = c->val64.p; c->g.edge32 = c->edge32.p;
    c->g.h64 = c->h64.p; c->g.hq = c->hq.p;

#undef CT
    *out = c;
    return NLMC_OK;
}

void nlmc_destroy(nlmc_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream); else (void)hipDeviceSynchronize();
#ifdef NLMC_STAMPS
    if (!c->knobs.stamp_file.empty()) {      // diagnostic build: dump the last launch's per-wave cycle sums
        if (c->dbg.p) {
            std::vector<long long> hbuf((size_t)c->n_chains * 16 * 8 + 96);
            if (hipMemcpy(hbuf.data(), c->dbg.p, hbuf.size() * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess) {
                if (FILE *f = fopen(c->knobs.stamp_file.c_str(), "wb")) { fwrite(hbuf.data(), sizeof(long long), hbuf.size(), f); fclose(f); }
            }
        }
    }
#endif
    if (c->comm && g_rccl.ok) (void)g_rccl.CommDestroy(c->comm);
    for (hipEvent_t e : c->events) (void)hipEventDestroy(e);
    if (c->aux) { (void)hipStreamSynchronize(c->aux); (void)hipStreamDestroy(c->aux); }
    if (c->owns_stream && c->stream) { (void)hipStreamDestroy(c->stream); c->stream = nullptr; }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    delete c;       // every buffer, then the arena, with the context's device current
}

int nlmc_set_spins(nlmc_ctx *c, const int8_t *spins)
{
    if (!c || !spins) return fail(c, NLMC_ERR_ARG, "nlmc_set_spins: NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->n_chains == 0) return NLMC_OK;
    int rc = rows_to_device(c, c->spins.p, spins, c->n_chains);
    if (rc) return rc;
    rc = launch_energy_self(c, nullptr);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NLMC_OK;
}

int nlmc_get_spins(nlmc_ctx *c, int8_t *spins)
{
    if (!c || !spins) return fail(c, NLMC_ERR_ARG, "nlmc_get_spins: NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->n_chains == 0) return NLMC_OK;
    int rc = rows_to_host_begin(c, c->spins.p, c->n_chains);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    rows_to_host_finish(c, spins, c->n_chains);
    return NLMC_OK;
}

int nlmc_set_flags(nlmc_ctx *c, const uint8_t *flags, double temp_x)
{
    if (!c) return NLMC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!flags) { c->has_flags = false; c->temp_x = 1.0; return NLMC_OK; }
    if (!(temp_x > 0.0) && !(temp_x < 0.0)) return fail(c, NLMC_ERR_ARG, "nlmc_set_flags: temp_x must be non-zero");
    for (size_t i = 0; i < (size_t)c->n_chains * c->n; ++i)
        if (flags[i] > 3) return fail(c, NLMC_ERR_ARG, "nlmc_set_flags: flag value out of range");
    if (c->n_chains > 0) {
        int rc = rows_to_device(c, c->flags.p, flags, c->n_chains);
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    c->has_flags = true;
    c->temp_x = temp_x;
    return NLMC_OK;
}

int nlmc_energy(nlmc_ctx *c, double *out)
{
    if (!c || !out) return fail(c, NLMC_ERR_ARG, "nlmc_energy: NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->n_chains == 0) return NLMC_OK;
    int rc = launch_energy_self(c, c->energy.p);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(out, c->energy.p, sizeof(double) * c->n_chains, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NLMC_OK;
}

int nlmc_energy_dev(nlmc_ctx *c, double *dev_out)
{
    if (!c || !dev_out) return fail(c, NLMC_ERR_ARG, "nlmc_energy_dev: NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->n_chains == 0) return NLMC_OK;
    hipLaunchKernelGGL(k_efix_to_double, dim3((c->n_chains + 255) / 256), dim3(256), 0, c->stream, c->efix.p, dev_out,
                       c->n_chains, c->escale);
    HIP_TRY(c, hipGetLastError());
    return NLMC_OK;
}

int nlmc_energy_tracked(nlmc_ctx *c, double *out)
{
    if (!c || !out) return fail(c, NLMC_ERR_ARG, "nlmc_energy_tracked: NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->n_chains == 0) return NLMC_OK;
    std::vector<long long> e((size_t)c->n_chains);
    HIP_TRY(c, hipMemcpyAsync(e.data(), c->efix.p, sizeof(long long) * e.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const double inv = std::ldexp(1.0, -c->escale);
    for (size_t i = 0; i < e.size(); ++i) out[i] = (double)e[i] * inv;
    return NLMC_OK;
}

int nlmc_set_energy_sink(nlmc_ctx *c, double *dev_out)
{
    if (!c) return NLMC_ERR_ARG;
    c->energy_sink = dev_out;
    return NLMC_OK;
}

int nlmc_energy_scale(const nlmc_ctx *c) { return c ? c->escale : 0; }

int nlmc_field_scale(const nlmc_ctx *c) { return c ? c->qs : 0; }

int nlmc_energy_of(nlmc_ctx *c, const int8_t *spins, int64_t count, double *out)
{
    if (!c || !spins || !out || count < 0) return fail(c, NLMC_ERR_ARG, "nlmc_energy_of: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t chunk = std::max<int64_t>(1, ((int64_t)64 << 20) / c->n);
    for (int64_t b = 0; b < count; b += chunk) {
        const int64_t m = std::min(chunk, count - b);
        HIP_TRY(c, c->cfg.reserve((size_t)m * c->n));
        HIP_TRY(c, c->etrace_d.reserve((size_t)m));
        HIP_TRY(c, hipMemcpyAsync(c->cfg.p, spins + b * c->n, (size_t)m * c->n, hipMemcpyHostToDevice, c->stream));
        EnergyArgs a{};
        a.g = c->g; a.spins = c->cfg.p; a.stride = c->n; a.out = c->etrace_d.p; a.efix = nullptr; a.escale = c->escale;
        launch_energy(c, (unsigned)m, c->stream, a);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(out + b, c->etrace_d.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return NLMC_OK;
}

int nlmc_energy_of_recorded(nlmc_ctx *c, int first, int count, double *out)
{
    if (!c || !out || first < 0 || count < 0) return fail(c, NLMC_ERR_ARG, "nlmc_energy_of_recorded: bad argument");
    if (first + count > c->strace_nrec)
        return fail(c, NLMC_ERR_STATE, "nlmc_energy_of_recorded: the last sweep call recorded fewer configurations per chain");
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t m = (int64_t)c->strace_rows * count;
    if (m == 0) return NLMC_OK;
    HIP_TRY(c, c->etrace_d.reserve((size_t)m));
    EnergyArgs a{};
    a.g = c->g; a.spins = c->strace.p + (size_t)first * c->n; a.stride = c->n; a.stride_outer = (int64_t)c->strace_nrec * c->n;
    a.inner = count; a.out = c->etrace_d.p; a.efix = nullptr; a.escale = c->escale;
    launch_energy(c, (unsigned)m, c->cur, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, c->etrace_d.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, c->cur));
    HIP_TRY(c, hipStreamSynchronize(c->cur));
    return NLMC_OK;
}

int nlmc_sweep_stream(nlmc_ctx *c, int n_sweeps, const int32_t *perm, const double *u, const double *beta,
                      int chain_stride, int sweep_stride, int record_stride, int8_t *out_spins, double *out_energy,
                      double *out_min_energy, int32_t *out_argmin, int8_t *out_argmin_state)
{
    if (!c) return NLMC_ERR_ARG;
    if (n_sweeps < 0 || !beta || (n_sweeps > 0 && c->n_chains > 0 && (!perm || !u)) || (out_spins && record_stride < 1))
        return fail(c, NLMC_ERR_ARG, "nlmc_sweep_stream: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const int R = c->n_chains, n = c->n;
    if (R == 0 || n_sweeps == 0) return NLMC_OK;
    const size_t tot = (size_t)R * n_sweeps;
    // beta table -> dense [R][n_sweeps]
    std::vector<double> tab(tot);
    for (int r = 0; r < R; ++r)
        for (int t = 0; t < n_sweeps; ++t) tab[(size_t)r * n_sweeps + t] = beta[(size_t)r * chain_stride + (size_t)t * sweep_stride];
    HIP_TRY(c, c->keys.reserve(tot * n));
    HIP_TRY(c, c->ustream.reserve(tot * n));
    HIP_TRY(c, c->perm_raw.reserve(tot * n));
    HIP_TRY(c, c->u_raw.reserve(tot * n));
    HIP_TRY(c, c->stream_bad.reserve(1));
    c->tab_host.clear();
    HIP_TRY(c, c->tab.reserve(tot));
    // the stream goes up as it was drawn and is scattered by spin on the device (rank[perm[i]] = i, u_spin[perm[i]] = u[i]; the
    // host loop + its staging vectors were 9 + 9 ms per 2000 sweeps at N = 2048), which also checks that every row IS a permutation
    HIP_TRY(c, hipMemsetAsync(c->stream_bad.p, 0, sizeof(int32_t), c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->perm_raw.p, perm, sizeof(int32_t) * tot * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->u_raw.p, u, sizeof(double) * tot * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->tab.p, tab.data(), sizeof(double) * tot, hipMemcpyHostToDevice, c->stream));
    if (c->big || (size_t)n * 4 > (size_t)150 * 1024) {       // (the seen-marks of k_stream_scatter live in LDS)
        HIP_TRY(c, hipMemsetAsync(c->keys.p, 0xFF, sizeof(uint32_t) * tot * n, c->stream));
        for (size_t ob = 0; ob < tot; ob += 65535) {
            const size_t no = std::min<size_t>(65535, tot - ob), sh = ob * (size_t)n;
            hipLaunchKernelGGL(k_stream_scatter_big, dim3((unsigned)((n + 255) / 256), (unsigned)no), dim3(256), 0, c->stream, n, c->perm_raw.p + sh,
                               c->u_raw.p + sh, c->keys.p + sh, c->ustream.p + sh, c->stream_bad.p);
        }
    } else {
        { int rc = ensure_lds(c, reinterpret_cast<const void *>(k_stream_scatter), (size_t)n * 4); if (rc) return rc; }
        hipLaunchKernelGGL(k_stream_scatter, dim3((unsigned)tot), dim3(256), (size_t)n * 4, c->stream, n, c->perm_raw.p, c->u_raw.p, c->keys.p,
                           c->ustream.p, c->stream_bad.p);
    }
    HIP_TRY(c, hipGetLastError());
    int32_t bad = 0;
    HIP_TRY(c, hipMemcpyAsync(&bad, c->stream_bad.p, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));          // (also: the caller's buffers and `tab` may go away)
    if (bad) return fail(c, NLMC_ERR_ARG, "nlmc_sweep_stream: perm is not a permutation");
    SweepOut o{record_stride, out_spins, out_energy, out_min_energy, out_argmin, out_argmin_state};
    SweepCall s{};
    s.stream_mode = true; s.precision = NLMC_F64; s.order_mode = NLMC_ORDER_PER_CHAIN; s.n_sweeps = n_sweeps;
    s.tab = c->tab.p; s.tab_cs = n_sweeps; s.tab_ss = 1; s.keys_dev = c->keys.p; s.ustream_dev = c->ustream.p;
    int rc = run_sweeps(c, s, o);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NLMC_OK;
}

int nlmc_sweep_philox(nlmc_ctx *c, int precision, int order_mode, int n_sweeps, uint32_t sweep0, uint64_t seed,
                      const double *beta, int chain_stride, int sweep_stride, int record_stride, int8_t *out_spins,
                      double *out_energy, double *out_min_energy, int32_t *out_argmin, int8_t *out_argmin_state)
{
    if (!c) return NLMC_ERR_ARG;
    if (n_sweeps < 0 || (precision != NLMC_F32 && precision != NLMC_F64) ||
        (order_mode != NLMC_ORDER_SHARED && order_mode != NLMC_ORDER_PER_CHAIN) || (out_spins && record_stride < 1))
        return fail(c, NLMC_ERR_ARG, "nlmc_sweep_philox: bad argument");
    if (!beta && c->ladder_len == 0) return fail(c, NLMC_ERR_STATE, "nlmc_sweep_philox: beta == NULL needs nlmc_pt_init first");
    HIP_TRY(c, hipSetDevice(c->device));
    const int R = c->sub_count();
    if (R == 0 || n_sweeps == 0) return NLMC_OK;
    if (beta && chain_stride && c->subset != 0)
        return fail(c, NLMC_ERR_UNSUPPORTED, "nlmc_sweep_philox: a per-chain beta table with a chain subset (use the ladder or one beta)");
    SweepCall s{};
    s.precision = precision; s.order_mode = order_mode; s.n_sweeps = n_sweeps; s.sweep0 = sweep0; s.seed = seed;
    if (beta) {
        const int rows = chain_stride ? R : 1, T = sweep_stride ? n_sweeps : 1;
        std::vector<double> tab((size_t)rows * T * 2);
        for (int r = 0; r < rows; ++r)
            for (int t = 0; t < T; ++t) {
                const double b = beta[(size_t)r * chain_stride + (size_t)t * sweep_stride];
                tab[((size_t)r * T + t) * 2 + 0] = -2.0 * LOG2E * b;
                tab[((size_t)r * T + t) * 2 + 1] = -2.0 * LOG2E * (b / c->temp_x);
            }
        if (tab != c->tab_host) {          // (the same table as last time -- every NMC phase of a run -- is not uploaded again)
            HIP_TRY(c, c->tab.reserve(tab.size()));
            HIP_TRY(c, hipStreamSynchronize(c->cur));         // launches still reading the previous table
            HIP_TRY(c, hipMemcpyAsync(c->tab.p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, c->cur));
            HIP_TRY(c, hipStreamSynchronize(c->cur));
            c->tab_host.swap(tab);
        }
        s.tab = c->tab.p; s.tab_cs = chain_stride ? T * 2 : 0; s.tab_ss = sweep_stride ? 2 : 0;
    } else {
        { int rc = upload_ladder_tab(c, c->cur); if (rc) return rc; }
        s.tab = c->pt_tab.p; s.tab_cs = 2; s.use_slots = true;
    }
    SweepOut o{record_stride, out_spins, out_energy, out_min_energy, out_argmin, out_argmin_state};
    return run_sweeps(c, s, o);
}

int nlmc_plan_philox(nlmc_ctx *c, int precision, int order_mode, uint32_t sweep0, int n_sweeps, uint64_t seed)
{
    if (!c) return NLMC_ERR_ARG;
    if (order_mode != NLMC_ORDER_SHARED) return fail(c, NLMC_ERR_UNSUPPORTED, "nlmc_plan_philox: only shared orders are cached");
    if (n_sweeps < 0 || (precision != NLMC_F32 && precision != NLMC_F64)) return fail(c, NLMC_ERR_ARG, "nlmc_plan_philox: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    c->plan_valid = false;
    if (n_sweeps == 0) return NLMC_OK;
    const bool big = sweeps_big(c, false, precision == NLMC_F64);
    const int ell_mode = big ? -1 : precision == NLMC_F64 ? 2 : 1;
    if (big) HIP_TRY(c, c->plan.reserve_big((size_t)n_sweeps, (size_t)c->n, true));
    else HIP_TRY(c, c->plan.reserve((size_t)n_sweeps, (size_t)c->n, ell_mode));
    TimerSpan ts;                                                // planning time -> levelize time of nlmc_timing_total
    if (c->ev_accumulate) { int rc = span_begin(c, ts, 2, c->stream); if (rc) return rc; }
    int rc = run_levelize(c, n_sweeps, nullptr, 0, n_sweeps, sweep0, seed, c->plan, ell_mode);
    if (rc) return rc;
    if ((rc = span_end(c, ts)) != NLMC_OK) return rc;
    c->plan_valid = true;
    c->plan_big = big;
    c->plan_mode = order_mode;
    c->plan_precision = precision;
    c->plan_sweep0 = sweep0;
    c->plan_count = n_sweeps;
    c->plan_seed = seed;
    return NLMC_OK;
}

static int reserve_fused_plan(nlmc_ctx *c, int n_windows, int T, bool with_val = false)
{
    nlmc_ctx::FusedPlan &P = c->fz[c->fz_slot];
    const size_t W = (size_t)n_windows, TN = (size_t)T * c->n, PS = (size_t)fused_pstride(c->n, c->n_long, T);
    if (with_val) HIP_TRY(c, P.val.reserve(W * PS * NLMC_FZ_VAL_WORDS));
    HIP_TRY(c, c->fz_glv.reserve(W * TN));
    HIP_TRY(c, c->fz_perm.reserve(W * PS));
    HIP_TRY(c, P.head.reserve(W * PS));
    if (fused_plan_stream(c)) HIP_TRY(c, P.hs.reserve(W * fused_hs_window(fused_workers(c, fused_block(c)))));
    HIP_TRY(c, P.ell.reserve(W * PS * NLMC_FZ_W));
    HIP_TRY(c, P.loff.reserve(W * (NLMC_LCAP + 1)));
    HIP_TRY(c, P.nlev.reserve(W));
    HIP_TRY(c, P.npos.reserve(W));
    HIP_TRY(c, P.himax.reserve(W));
    HIP_TRY(c, P.send.reserve(W * T));
    return NLMC_OK;
}

int nlmc_plan_reserve_fused(nlmc_ctx *c, int n_windows, int window)
{
    if (!c) return NLMC_ERR_ARG;
    if (n_windows < 0 || window < 1) return fail(c, NLMC_ERR_ARG, "nlmc_plan_reserve_fused: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    if (n_windows == 0 || !fused_supported(c, window)) return NLMC_OK;
    c->fz[c->fz_slot].valid = false;              // (growing a buffer drops its contents)
    return reserve_fused_plan(c, n_windows, window, c->f64_real && !c->f64_exact);
}

int nlmc_plan_philox_fused(nlmc_ctx *c, uint32_t sweep0, int n_windows, int window, uint64_t seed, int32_t *out_planned)
{
    if (!c) return NLMC_ERR_ARG;
    if (n_windows < 0 || window < 1) return fail(c, NLMC_ERR_ARG, "nlmc_plan_philox_fused: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    nlmc_ctx::FusedPlan &P = c->fz[c->fz_slot];
    P.valid = false;
    if (out_planned) *out_planned = 0;
    if (n_windows == 0 || !fused_supported(c, window)) return NLMC_OK;
    const int n = c->n, T = window;
    const size_t W = (size_t)n_windows;
    // the fp64 value plane only where the real-valued fp64 variant may run on the plan: other plans stay byte for byte as they were
    const bool with_val = c->f64_real && !c->f64_exact;
    P.pstride = fused_pstride(n, c->n_long, T);
    if (reserve_fused_plan(c, n_windows, T, with_val) != NLMC_OK) {
        // no room for this many windows: not an error -- nothing is planned, the caller's sweeps take the
        // sweep-by-sweep path (or it asks again for fewer windows); what was allocated for the attempt is given back
        (void)hipGetLastError();
        P.release(); c->fz_glv.release(); c->fz_perm.release();
        c->err.clear();
        return NLMC_OK;
    }
    { int rc = ensure_adjacency(c); if (rc) return rc; }
    FusedLevelizeArgs a{};
    a.g = c->g;
    a.T = T;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.sweep0 = sweep0;
    P.workers = fused_workers(c, fused_block(c));
    P.gen0 = fused_gen0(c, fused_block(c));
    a.level_cap = P.workers * 64;
    a.level_fill = c->knobs.no_level_fill ? 0 : 1;
    a.pstride = P.pstride;
    a.tab_words = c->n_pad;
    a.k_dummy = c->n_pad;
    a.fmt = fused_addr_format(c) ? NLMC_FMT_ADDR : c->compact16 ? NLMC_FMT_COMPACT : NLMC_FMT_WIDE;
    a.k_zero = c->n_pad + 8;
    a.neg_off = c->n_pad + 16;
    a.bank_aware = (with_val || c->knobs.no_bank_aware) ? 0 : 1;    // (the fp64 sum runs in row order)
    a.quads = c->knobs.no_quads ? 0 : 1;
    a.val = with_val ? P.val.p : nullptr;
    P.fmt = a.fmt;
    P.has_val = with_val;
    a.adj = reinterpret_cast<const uint4 *>(c->fz_adj.p); a.glv = c->fz_glv.p; a.perm = c->fz_perm.p; a.head = P.head.p; a.ell = P.ell.p;
    P.has_hs = fused_plan_stream(c);
    a.hs = P.has_hs ? P.hs.p : nullptr; a.loff = P.loff.p; a.nlev = P.nlev.p;
    a.hi_max = P.himax.p; a.send = P.send.p; a.npos = P.npos.p;
    P.built = a;
    const size_t n4 = ((size_t)n + 3) & ~(size_t)3;
    const size_t lds = (size_t)n * 8 + n4 * 2 + n4 + n4 * 2 + 2 * (size_t)(NLMC_LCAP + 2) * 4 + 16;
    { int rc = ensure_lds(c, reinterpret_cast<const void *>(k_levelize_fused), lds); if (rc) return rc; }
    const bool fz_diag = c->knobs.fz_stats;     // diagnostic: phase cycle counts of window 0 on stderr
    if (fz_diag) { HIP_TRY(c, c->fz_stats.reserve(W * 8)); a.stats = c->fz_stats.p; }
    // planning time counts as levelize time of the accumulating timer (nlmc_timing_total): an event triple whose
    // sweep part is empty
    TimerSpan ts;
    if (c->ev_accumulate) { int rc = span_begin(c, ts, 2, c->stream); if (rc) return rc; }
    hipLaunchKernelGGL(k_levelize_fused, dim3(n_windows), dim3(1024), lds, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    { int rc = span_end(c, ts); if (rc) return rc; }
    P.nlev_host.assign(W, 0);
    P.npos_host.assign(W, 0);
    HIP_TRY(c, hipMemcpyAsync(P.nlev_host.data(), P.nlev.p, sizeof(int32_t) * W, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(P.npos_host.data(), P.npos.p, sizeof(int32_t) * W, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (fz_diag) {
        long long st[8] = {0};
        HIP_TRY(c, hipMemcpy(st, c->fz_stats.p, sizeof(st), hipMemcpyDeviceToHost));
        fprintf(stderr, "k_levelize_fused window 0 (cycles): keys %lld, init %lld, passes %lld (%lld passes), place-1 %lld, place-2 %lld\n", st[0], st[1], st[2], st[3], st[4], st[5]);
    }
    int ok = 0;
    for (int32_t v : P.nlev_host) ok += v > 0;
    P.valid = true;
    P.sweep0 = sweep0; P.windows = n_windows; P.T = T; P.seed = seed;
    if (out_planned) *out_planned = ok;
    return NLMC_OK;
}

int nlmc_fused_modes(nlmc_ctx *c, int window)
{
    if (!c) return 0;
    auto can = [&](int precision) { return fused_route(c, precision, NLMC_ORDER_SHARED, false, false, -1, window, Via::sweeps) != NOT_FUSED; };
    return (can(NLMC_F32) ? 1 : 0) | (can(NLMC_F64) ? 2 : 0);
}

int nlmc_last_sweep_fused(const nlmc_ctx *c) { return c && c->stat_fused_window >= 0 ? 1 : 0; }

int nlmc_set_lane_sweeps(nlmc_ctx *c, int mode)
{
    if (!c) return NLMC_ERR_ARG;
    if (mode < 0 || mode > 2) return fail(c, NLMC_ERR_ARG, "nlmc_set_lane_sweeps: mode must be 0 (off), 1 (auto) or 2 (force)");
    c->lane_mode = mode;
    return NLMC_OK;
}

int nlmc_set_wave_sweeps(nlmc_ctx *c, int mode)
{
    if (!c) return NLMC_ERR_ARG;
    if (mode < 0 || mode > 2) return fail(c, NLMC_ERR_ARG, "nlmc_set_wave_sweeps: mode must be 0 (off), 1 (auto) or 2 (force)");
    c->wave_mode = mode;
    return NLMC_OK;
}

int nlmc_last_sweep_route(const nlmc_ctx *c) { return c ? c->last_route : NLMC_ROUTE_NONE; }

int nlmc_probe_level_round(nlmc_ctx *c, int waves, int conflict_free, int rounds, int n_workgroups, double *out_ns_per_round)
{
    if (!c || !out_ns_per_round || waves < 1 || waves > 16 || rounds < 1 || n_workgroups < 1)
        return fail(c, NLMC_ERR_ARG, "nlmc_probe_level_round: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const int lds_bytes = 2 * 16384;
    int *sink = nullptr;
    HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&sink), sizeof(int)));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = NLMC_OK;
    float ms = 0.f;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = fail(c, NLMC_ERR_HIP, "hipEventCreate failed");
    if (!rc) {
        hipLaunchKernelGGL(k_level_round_probe, dim3(n_workgroups), dim3(waves * 64), (size_t)lds_bytes, c->stream, std::min(rounds, 256), conflict_free, lds_bytes, sink);   // warm-up
        (void)hipEventRecord(e0, c->stream);
        hipLaunchKernelGGL(k_level_round_probe, dim3(n_workgroups), dim3(waves * 64), (size_t)lds_bytes, c->stream, rounds, conflict_free, lds_bytes, sink);
        (void)hipEventRecord(e1, c->stream);
        if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess || hipGetLastError() != hipSuccess)
            rc = fail(c, NLMC_ERR_HIP, "nlmc_probe_level_round: launch failed");
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(sink);
    if (!rc) *out_ns_per_round = (double)ms * 1e6 / rounds;
    return rc;
}

int nlmc_plan_get_levels(nlmc_ctx *c, int window, int32_t *out_level_chunk_offsets, int32_t capacity, int32_t *out_n_levels)
{
    if (!c || !out_level_chunk_offsets || !out_n_levels) return fail(c, NLMC_ERR_ARG, "nlmc_plan_get_levels: NULL argument");
    const nlmc_ctx::FusedPlan &P = c->fz[c->fz_slot];
    if (!P.valid || window < 0 || window >= P.windows) return fail(c, NLMC_ERR_STATE, "nlmc_plan_get_levels: no such planned window in the selected slot");
    const int nl = P.nlev_host[(size_t)window];
    *out_n_levels = nl;
    if (capacity < nl + 1) return fail(c, NLMC_ERR_ARG, "nlmc_plan_get_levels: capacity < levels + 1");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out_level_chunk_offsets, P.loff.p + (size_t)window * (NLMC_LCAP + 1), sizeof(int32_t) * (size_t)(nl + 1),
                              hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NLMC_OK;
}

int nlmc_plan_get_items(nlmc_ctx *c, int window, int64_t *out_info, int32_t *out_head, int32_t *out_ell, double *out_val,
                        int32_t *out_loff, int32_t *out_send, int64_t capacity)
{
    if (!c || !out_info) return fail(c, NLMC_ERR_ARG, "nlmc_plan_get_items: NULL argument");
    const nlmc_ctx::FusedPlan &P = c->fz[c->fz_slot];
    if (!P.valid || window < 0 || window >= P.windows) return fail(c, NLMC_ERR_STATE, "nlmc_plan_get_items: no such planned window in the selected slot");
    HIP_TRY(c, hipSetDevice(c->device));
    const FusedLevelizeArgs &b = P.built;
    const nlmc_ctx::FusedPlan::Arrays A = P.at(window);
    const int nl = P.nlev_host[(size_t)window], np = P.npos_host[(size_t)window];
    const int planes = P.fmt == NLMC_FMT_ADDR ? 1 : P.fmt == NLMC_FMT_COMPACT ? 2 : 4;
    int32_t himax = 0;
    HIP_TRY(c, hipMemcpyAsync(&himax, A.himax, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int64_t info[NLMC_PLAN_INFO_WORDS] = {P.fmt, P.pstride, P.T, (int64_t)P.sweep0, (int64_t)P.seed, P.workers, b.quads, b.bank_aware, c->n_pad,
                                                b.k_dummy, b.k_zero, b.neg_off, b.tab_words, nl, np, himax, P.has_val ? 1 : 0, b.level_fill, planes, P.has_hs ? 1 : 0};
    for (int i = 0; i < NLMC_PLAN_INFO_WORDS; ++i) out_info[i] = info[i];
    if (!out_head || nl == 0) return NLMC_OK;
    if (!out_ell || !out_loff || !out_send || (P.has_val && !out_val)) return fail(c, NLMC_ERR_ARG, "nlmc_plan_get_items: NULL array");
    if (capacity < np) return fail(c, NLMC_ERR_ARG, "nlmc_plan_get_items: capacity < positions of the window");
    const size_t PS = (size_t)P.pstride, NP = (size_t)np;
    HIP_TRY(c, hipMemcpyAsync(out_head, A.head, sizeof(int2) * NP, hipMemcpyDeviceToHost, c->stream));
    for (int q = 0; q < planes; ++q)       // plane q of the window: 16 bytes per position, pstride positions apart
        HIP_TRY(c, hipMemcpyAsync(out_ell + (size_t)q * NP * 4, reinterpret_cast<const int4 *>(A.ell) + (size_t)q * PS, sizeof(int4) * NP,
                                  hipMemcpyDeviceToHost, c->stream));
    if (P.has_val) {
        for (int q = 0; q < NLMC_FZ_W / 2; ++q)
            HIP_TRY(c, hipMemcpyAsync(out_val + (size_t)q * NP * 2, A.val + (size_t)q * PS * 2, sizeof(double) * 2 * NP, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(out_val + (size_t)NLMC_FZ_W * NP, A.val + (size_t)NLMC_FZ_W * PS, sizeof(double) * NP, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(out_loff, A.loff, sizeof(int32_t) * (size_t)(nl + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out_send, A.send, sizeof(int32_t) * (size_t)P.T, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NLMC_OK;
}

int nlmc_plan_get_head_stream(nlmc_ctx *c, int window, int32_t *out_hs, int64_t capacity)
{
    if (!c || !out_hs) return fail(c, NLMC_ERR_ARG, "nlmc_plan_get_head_stream: NULL argument");
    const nlmc_ctx::FusedPlan &P = c->fz[c->fz_slot];
    if (!P.valid || window < 0 || window >= P.windows) return fail(c, NLMC_ERR_STATE, "nlmc_plan_get_head_stream: no such planned window in the selected slot");
    if (!P.has_hs) return fail(c, NLMC_ERR_STATE, "nlmc_plan_get_head_stream: the plan has no head stream (a field term, 8-byte entries, or NLMC_NO_HEAD_STREAM)");
    const int nl = P.nlev_host[(size_t)window];
    const size_t count = fused_hs_index(nl + 3, P.workers, 0, 0);       // int4 elements of the quads of levels [0, nl)
    if (capacity < (int64_t)(count * 4)) return fail(c, NLMC_ERR_ARG, "nlmc_plan_get_head_stream: capacity < 4 * 64 * workers * ceil(nlev / 4)");
    if (count == 0) return NLMC_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out_hs, P.at(window).hs, sizeof(int4) * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NLMC_OK;
}

int nlmc_last_head_path(nlmc_ctx *c) { return c ? c->stat_head_path : 0; }

int nlmc_plan_get_order(nlmc_ctx *c, int order, int64_t *out_info, int32_t *out_order, int32_t *out_lvl_off, int64_t capacity)
{
    if (!c || !out_info) return fail(c, NLMC_ERR_ARG, "nlmc_plan_get_order: NULL argument");
    if (!c->plan_valid || order < 0 || order >= c->plan_count) return fail(c, NLMC_ERR_STATE, "nlmc_plan_get_order: no such planned order");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->n, o = (size_t)order;
    int32_t nl = 0, himax = 0;
    HIP_TRY(c, hipMemcpyAsync(&nl, c->plan.nlev.p + o, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&himax, c->plan.hi_max.p + o, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // (the cap run_levelize gave the planner: the sweep workgroup's width; the global-memory levelizer publishes whole levels)
    const int cap = c->plan_big ? 0 : sweep_block_for(c, c->plan_precision == NLMC_F64, c->plan_precision == NLMC_F32 && c->has_diag);
    const int64_t info[8] = {(int64_t)c->n, nl, himax, c->plan_big ? 1 : 0, cap, c->plan_count, (int64_t)c->plan_sweep0, 0};
    for (int i = 0; i < 8; ++i) out_info[i] = info[i];
    if (!out_order) return NLMC_OK;
    if (!out_lvl_off) return fail(c, NLMC_ERR_ARG, "nlmc_plan_get_order: NULL array");
    if (capacity < (int64_t)n || nl < 0 || (size_t)nl > n) return fail(c, NLMC_ERR_ARG, "nlmc_plan_get_order: capacity < spins");
    HIP_TRY(c, hipMemcpyAsync(out_order, c->plan.order.p + o * n, sizeof(int2) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out_lvl_off, c->plan.lvl_off.p + o * (n + 1), sizeof(int32_t) * (size_t)(nl + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NLMC_OK;
}

int nlmc_last_timing(nlmc_ctx *c, float *ms_levelize, float *ms_sweep, int32_t *launches_sweep)
{
    if (!c) return NLMC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    float lev = 0.f, sw = 0.f;
    for (size_t i = c->ev_call_start; i + 3 <= c->ev_used; i += 3) {
        float a = 0.f, b = 0.f;
        int rc = triple_ms(c, i / 3, a, b);
        if (rc) return rc;
        lev += a; sw += b;
    }
    if (ms_levelize) *ms_levelize = lev;
    if (ms_sweep) *ms_sweep = sw;
    if (launches_sweep) *launches_sweep = c->launches_sweep;
    return NLMC_OK;
}

int nlmc_timing_reset(nlmc_ctx *c, int enable)
{
    if (!c || enable < 0) return NLMC_ERR_ARG;
    c->ev_used = 0;
    c->ev_call_start = 0;
    c->launches_total = 0;
    c->launches_timed = 0;
    c->ev_accumulate = enable != 0;
    c->ev_every = enable > 1 ? enable : 1;
    return NLMC_OK;
}

int nlmc_timing_total(nlmc_ctx *c, double *ms_levelize, double *ms_sweep, int64_t *launches_sweep, int64_t *launches_timed)
{
    if (!c) return NLMC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    double lev = 0.0, sw = 0.0;
    for (size_t i = 0; i + 3 <= c->ev_used; i += 3) {
        float a = 0.f, b = 0.f;
        int rc = triple_ms(c, i / 3, a, b);
        if (rc) return rc;
        lev += a; sw += b;
    }
    if (ms_levelize) *ms_levelize = lev;
    if (ms_sweep) *ms_sweep = sw;
    if (launches_sweep) *launches_sweep = c->launches_total;
    if (launches_timed) *launches_timed = c->launches_timed;
    return NLMC_OK;
}

int nlmc_last_schedule_stats(nlmc_ctx *c, int64_t *n_orders, int64_t *n_levels)
{
    if (!c) return NLMC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((c->last_route == NLMC_ROUTE_LANES || c->last_route == NLMC_ROUTE_WAVES) && c->stat_fused_window < 0) {   // chain-per-lane / wave-per-chain sweeps: visiting orders, no levels
        if (n_orders) *n_orders = c->stat_lane_orders;
        if (n_levels) *n_levels = 0;
        return NLMC_OK;
    }
    if (c->stat_fused_window >= 0) {       // one merged level list for fz_T sweeps
        if (n_orders) *n_orders = c->fz[c->stat_fused_slot].T;
        if (n_levels) *n_levels = c->fz[c->stat_fused_slot].nlev_host[(size_t)c->stat_fused_window];
        return NLMC_OK;
    }
    const int32_t *p = c->stats_pending ? c->stats_nlev_ptr : (c->plan_valid ? c->plan.nlev.p : nullptr);
    const int64_t cnt = c->stats_pending ? c->stats_nlev_count : (c->plan_valid ? c->plan_count : 0);
    int64_t lv = 0;
    if (p && cnt > 0) {
        std::vector<int32_t> hnl((size_t)cnt);
        HIP_TRY(c, hipMemcpyAsync(hnl.data(), p, sizeof(int32_t) * (size_t)cnt, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (int32_t v : hnl) lv += v;
    }
    if (n_orders) *n_orders = cnt;
    if (n_levels) *n_levels = lv;
    return NLMC_OK;
}

// ---------------------------------------------------------------------------------------------------
// replica exchange
// ---------------------------------------------------------------------------------------------------
int nlmc_pt_init(nlmc_ctx *c, int ladder_len, const double *beta_list)
{
    if (!c || !beta_list || ladder_len < 1) return fail(c, NLMC_ERR_ARG, "nlmc_pt_init: bad argument");
    if (c->n_chains_global % ladder_len != 0) return fail(c, NLMC_ERR_ARG, "nlmc_pt_init: n_chains_global not a multiple of ladder_len");
    HIP_TRY(c, hipSetDevice(c->device));
    c->ladder_len = ladder_len;
    c->apt_systems = 1;
    c->subset = 0; c->n_marked_local = 0; c->sub_dirty = true;
    c->pt_tab_valid = false;
    c->pt_plan.on = false;
    c->beta_list.assign(beta_list, beta_list + ladder_len);
    const int G = c->n_chains_global;
    HIP_TRY(c, c->pt_tab.reserve((size_t)ladder_len * 2));
    HIP_TRY(c, c->pt_beta.reserve((size_t)ladder_len));
    HIP_TRY(c, c->slot_of_chain.reserve((size_t)G));
    HIP_TRY(c, c->chain_of_slot.reserve((size_t)G));
    HIP_TRY(c, c->pt_status.reserve(1));
    std::vector<int32_t> ident((size_t)G);
    for (int i = 0; i < G; ++i) ident[i] = i % ladder_len;
    // (stream-ordered: the context's stream may be a non-blocking one, which legacy NULL-stream copies are not ordered against)
    std::vector<int32_t> cos((size_t)G);
    for (int i = 0; i < G; ++i) cos[i] = i;     // chain_of_slot[ladder*L + slot] = global chain id
    HIP_TRY(c, hipMemcpyAsync(c->slot_of_chain.p, ident.data(), sizeof(int32_t) * G, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->chain_of_slot.p, cos.data(), sizeof(int32_t) * G, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->pt_beta.p, beta_list, sizeof(double) * ladder_len, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->pt_status.p, 0, sizeof(int32_t), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NLMC_OK;
}

int nlmc_pt_plan(nlmc_ctx *c, uint32_t round0, int n_rounds, uint64_t seed, int n_pairs)
{
    if (!c) return NLMC_ERR_ARG;
    if (c->ladder_len == 0) return fail(c, NLMC_ERR_STATE, "nlmc_pt_plan: call nlmc_pt_init first");
    // (a context cut by temperature slot plans the selections of the GLOBAL ladder of its K sub-replica ladders: every rank the same)
    const int nl = c->n_chains_global / c->ladder_len, L = c->apt_R > 0 ? c->apt_R : c->ladder_len;
    if (n_rounds < 0 || n_pairs < 0 || n_pairs > std::max(0, L - 1)) return fail(c, NLMC_ERR_ARG, "Cannot find non-overlapping pairs.");
    if (L > 4096) return fail(c, NLMC_ERR_UNSUPPORTED, "nlmc_pt_plan: ladder_len > 4096");
    HIP_TRY(c, hipSetDevice(c->device));
    c->pt_plan.on = false;
    if (n_rounds == 0 || n_pairs == 0) return NLMC_OK;
    HIP_TRY(c, c->pt_plan_pairs.reserve((size_t)n_rounds * nl * n_pairs * 2));
    HIP_TRY(c, c->pt_plan_ok.reserve((size_t)n_rounds * nl));
    PtSelectArgs a{};
    a.ladder_len = L; a.n_pairs = n_pairs; a.n_ladders = nl; a.round0 = round0;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    a.plan_pairs = c->pt_plan_pairs.p; a.plan_ok = c->pt_plan_ok.p;
    hipLaunchKernelGGL(k_pt_select, dim3(n_rounds * nl), dim3(64), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    // the selection depends on the RNG only: an exhausted greedy selection (NPT/npt.py:526 raises ValueError in that
    // round) is known now -- report it here instead of silently skipping that round's swaps later
    std::vector<int32_t> ok((size_t)n_rounds * nl);
    HIP_TRY(c, hipMemcpyAsync(ok.data(), c->pt_plan_ok.p, sizeof(int32_t) * ok.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int32_t v : ok)
        if (!v) return fail(c, NLMC_ERR_ARG, "Cannot find non-overlapping pairs.");
    c->pt_plan.on = true;
    c->pt_plan.round0 = round0; c->pt_plan.rounds = n_rounds; c->pt_plan.npairs = n_pairs; c->pt_plan.seed = seed;
    return NLMC_OK;
}

int nlmc_pt_get_slots(nlmc_ctx *c, int32_t *slot_of_chain)
{
    if (!c || !slot_of_chain) return fail(c, NLMC_ERR_ARG, "nlmc_pt_get_slots: NULL argument");
    if (c->ladder_len == 0) return fail(c, NLMC_ERR_STATE, "nlmc_pt_get_slots: call nlmc_pt_init first");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(slot_of_chain, c->slot_of_chain.p, sizeof(int32_t) * c->n_chains_global, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NLMC_OK;
}

int nlmc_pt_set_slots(nlmc_ctx *c, const int32_t *slot_of_chain)
{
    if (!c || !slot_of_chain) return fail(c, NLMC_ERR_ARG, "nlmc_pt_set_slots: NULL argument");
    if (c->ladder_len == 0) return fail(c, NLMC_ERR_STATE, "nlmc_pt_set_slots: call nlmc_pt_init first");
    HIP_TRY(c, hipSetDevice(c->device));
    const int G = c->n_chains_global, L = c->ladder_len;
    std::vector<int32_t> cos((size_t)G, -1);
    for (int i = 0; i < G; ++i) {
        const int s = slot_of_chain[i];
        if (s < 0 || s >= L || cos[(size_t)(i / L) * L + s] != -1) return fail(c, NLMC_ERR_ARG, "nlmc_pt_set_slots: not a permutation per ladder");
        cos[(size_t)(i / L) * L + s] = i;
    }
    c->sub_dirty = true;
    HIP_TRY(c, hipMemcpyAsync(c->slot_of_chain.p, slot_of_chain, sizeof(int32_t) * G, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->chain_of_slot.p, cos.data(), sizeof(int32_t) * G, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NLMC_OK;
}

int nlmc_pt_apply_swap(nlmc_ctx *c, int ladder, int slot_a, int slot_b)
{
    if (!c) return NLMC_ERR_ARG;
    if (c->ladder_len == 0) return fail(c, NLMC_ERR_STATE, "nlmc_pt_apply_swap: call nlmc_pt_init first");
    const int L = c->ladder_len;
    if (ladder < 0 || ladder >= c->n_chains_global / L || slot_a < 0 || slot_a >= L || slot_b < 0 || slot_b >= L || slot_a == slot_b)
        return fail(c, NLMC_ERR_ARG, "nlmc_pt_apply_swap: bad ladder/slot");
    HIP_TRY(c, hipSetDevice(c->device));
    c->sub_dirty = true;
    hipLaunchKernelGGL(k_pt_apply_swap, dim3(1), dim3(1), 0, c->stream, c->slot_of_chain.p, c->chain_of_slot.p, L, ladder, slot_a, slot_b);
    HIP_TRY(c, hipGetLastError());
    return NLMC_OK;
}

int nlmc_pt_swap_philox(nlmc_ctx *c, uint32_t round, uint64_t seed, int n_pairs, const double *energies_all_dev,
                        int32_t *out_pairs, uint8_t *out_accepted)
{
    if (!c) return NLMC_ERR_ARG;
    if (c->ladder_len == 0) return fail(c, NLMC_ERR_STATE, "nlmc_pt_swap_philox: call nlmc_pt_init first");
    const int L = c->ladder_len, G = c->n_chains_global, nl = G / L;
    if (n_pairs < 0 || n_pairs > std::max(0, L - 1)) return fail(c, NLMC_ERR_ARG, "Cannot find non-overlapping pairs.");
    // a context that owns whole ladders needs nobody else's energies: it decides its own ladders from its tracked energies
    // (same Philox keys -- round, GLOBAL ladder index, pair -- as the context that holds all chains)
    const bool whole_ladders = c->chain_base % L == 0 && c->n_chains % L == 0;
    if (!energies_all_dev && !whole_ladders)
        return fail(c, NLMC_ERR_ARG, "nlmc_pt_swap_philox: a context whose block cuts a ladder needs the all-gathered energies");
    if (L > 4096) return fail(c, NLMC_ERR_UNSUPPORTED, "nlmc_pt_swap_philox: ladder_len > 4096");
    if (c->apt_R > 0 && c->apt_world > 1) return fail(c, NLMC_ERR_STATE, "nlmc_pt_swap_philox: this context is one slot block of a cut ladder (nlmc_apt_shard): use nlmc_apt_swap_*");
    HIP_TRY(c, hipSetDevice(c->device));
    if (n_pairs == 0) return NLMC_OK;
    HIP_TRY(c, c->pt_pairs.reserve((size_t)nl * n_pairs * 2));
    HIP_TRY(c, c->pt_acc.reserve((size_t)nl * n_pairs));
    PtSwapArgs a{};
    a.ladder_len = L; a.n_pairs = n_pairs; a.round = round;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    a.beta = c->pt_beta.p;
    a.energies = energies_all_dev;
    a.efix = energies_all_dev ? nullptr : c->efix.p;
    a.escale = c->escale;
    a.slot_of_chain = c->slot_of_chain.p; a.chain_of_slot = c->chain_of_slot.p;
    a.out_pairs = c->pt_pairs.p; a.out_acc = c->pt_acc.p; a.status = c->pt_status.p;
    a.ladder0 = energies_all_dev ? 0 : c->chain_base / L;
    a.chain_base = c->chain_base;
    const int n_decide = energies_all_dev ? nl : c->n_chains / L;            // ladders this launch decides
    swap_window_rows(c, a, round, seed, n_pairs, (size_t)nl, out_pairs || out_accepted);
    c->sub_dirty = true;
    if ((out_pairs || out_accepted) && n_decide < nl) {          // rows of the ladders other contexts decide: "no pair"
        HIP_TRY(c, hipMemsetAsync(c->pt_pairs.p, 0xFF, sizeof(int32_t) * (size_t)nl * n_pairs * 2, c->stream));
        HIP_TRY(c, hipMemsetAsync(c->pt_acc.p, 0, (size_t)nl * n_pairs, c->stream));
    }
    hipLaunchKernelGGL(k_pt_swap, dim3(n_decide), dim3(swap_block(a.plan_pairs != nullptr, n_pairs)), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return swap_read_back(c, nl, n_pairs, out_pairs, out_accepted);
}

int nlmc_pt_swap_philox_host(nlmc_ctx *c, uint32_t round, uint64_t seed, int n_pairs, const double *energies_all_host,
                             int32_t *out_pairs, uint8_t *out_accepted)
{
    if (!c || !energies_all_host) return fail(c, NLMC_ERR_ARG, "nlmc_pt_swap_philox_host: NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->pt_energies_all.reserve((size_t)c->n_chains_global));
    HIP_TRY(c, hipMemcpyAsync(c->pt_energies_all.p, energies_all_host, sizeof(double) * (size_t)c->n_chains_global,
                              hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // the caller's buffer may go away after the call
    return nlmc_pt_swap_philox(c, round, seed, n_pairs, c->pt_energies_all.p, out_pairs, out_accepted);
}

// ---- replica-sharded ladders: the ONE collective of a round, issued by the library on the kernels' stream -----------------
int nlmc_comm_unique_id(uint8_t *out_id)
{
    if (!out_id) return fail(nullptr, NLMC_ERR_ARG, "nlmc_comm_unique_id: NULL argument");
    if (!rccl_load()) return fail(nullptr, NLMC_ERR_UNSUPPORTED, g_rccl.why);
    Rccl::UniqueId id;
    const int rc = g_rccl.GetUniqueId(&id);
    if (rc != 0) return fail(nullptr, NLMC_ERR_HIP, "ncclGetUniqueId: " + rccl_err(rc));
    std::memcpy(out_id, id.internal, sizeof(id.internal));
    return NLMC_OK;
}

int nlmc_comm_init(nlmc_ctx *c, const uint8_t *id, int world, int rank)
{
    if (!c || !id || world < 1 || rank < 0 || rank >= world) return fail(c, NLMC_ERR_ARG, "nlmc_comm_init: bad argument");
    const bool apt = c->apt_R > 0;         // cut by temperature slot (nlmc_apt_shard): a self-contained block of chains per rank
    if (apt ? (c->apt_world != world || c->apt_rank != rank)
            : (c->n_chains * world != c->n_chains_global || c->chain_base != rank * c->n_chains))
        return fail(c, NLMC_ERR_ARG, "nlmc_comm_init: the context must own block `rank` of `world` equal blocks of chains (or be shard `rank` of `world` of nlmc_apt_shard)");
    if (!rccl_load()) return fail(c, NLMC_ERR_UNSUPPORTED, g_rccl.why);
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->comm) { (void)g_rccl.CommDestroy(c->comm); c->comm = nullptr; }
    Rccl::UniqueId uid;
    std::memcpy(uid.internal, id, sizeof(uid.internal));
    const int rc = g_rccl.CommInitRank(&c->comm, world, uid, rank);
    if (rc != 0) { c->comm = nullptr; return fail(c, NLMC_ERR_HIP, "ncclCommInitRank: " + rccl_err(rc)); }
    c->comm_world = world; c->comm_rank = rank;
    if (apt) return NLMC_OK;               // (its gathered vector is apt_e_all, filled by k_apt_pack)
    HIP_TRY(c, c->pt_energies_all.reserve((size_t)c->n_chains_global));
    HIP_TRY(c, hipMemsetAsync(c->pt_energies_all.p, 0, sizeof(double) * (size_t)c->n_chains_global, c->stream));
    // the sweep kernels store their chains' tracked energies straight into this rank's block of the gathered vector
    c->energy_sink = c->pt_energies_all.p + c->chain_base;
    return NLMC_OK;
}

int nlmc_pt_swap_philox_collective(nlmc_ctx *c, uint32_t round, uint64_t seed, int n_pairs, int refresh_energies,
                                   int32_t *out_pairs, uint8_t *out_accepted)
{
    if (!c) return NLMC_ERR_ARG;
    if (!c->comm) return fail(c, NLMC_ERR_STATE, "nlmc_pt_swap_philox_collective: call nlmc_comm_init first");
    if (c->apt_R > 0) return fail(c, NLMC_ERR_STATE, "nlmc_pt_swap_philox_collective: this context is a slot block of nlmc_apt_shard: use nlmc_apt_swap_collective");
    HIP_TRY(c, hipSetDevice(c->device));
    double *block = c->pt_energies_all.p + c->chain_base;
    if (refresh_energies || c->energy_sink != block) {        // (no sweep since the last state change wrote the block)
        hipLaunchKernelGGL(k_efix_to_double, dim3((c->n_chains + 255) / 256), dim3(256), 0, c->stream, c->efix.p, block, c->n_chains, c->escale);
        HIP_TRY(c, hipGetLastError());
    }
    // in-place all-gather (send = this rank's block of the receive buffer), on the stream the sweep and swap kernels use:
    // stream order is the only synchronisation a round needs
    const int rc = g_rccl.AllGather(block, c->pt_energies_all.p, (size_t)c->n_chains, /*ncclDouble*/ 8, c->comm, c->stream);
    if (rc != 0) return fail(c, NLMC_ERR_HIP, "ncclAllGather: " + rccl_err(rc));
    return nlmc_pt_swap_philox(c, round, seed, n_pairs, c->pt_energies_all.p, out_pairs, out_accepted);
}

int nlmc_comm_probe(void)
{
    return rccl_load() ? NLMC_OK : fail(nullptr, NLMC_ERR_UNSUPPORTED, g_rccl.why);
}

// Asynchronous failures of the library-issued collectives: ncclCommGetAsyncError, and a BOUNDED wait for the stream the collectives
// were queued on (a lost rank leaves the others spinning inside a collective kernel for ever).  On either, the communicator is
// aborted (ncclCommAbort ends the kernels that wait for the lost peer) and the call fails; the context keeps no communicator.
int nlmc_comm_check(nlmc_ctx *c, int timeout_ms)
{
    if (!c) return NLMC_ERR_ARG;
    if (!c->comm) return NLMC_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    auto abort_comm = [&](const std::string &why) {
        (void)g_rccl.CommAbort(c->comm);
        c->comm = nullptr;
        return fail(c, NLMC_ERR_HIP, why + "; the RCCL communicator was aborted (ncclCommAbort)");
    };
    int async = 0;
    int rc = g_rccl.CommGetAsyncError(c->comm, &async);
    if (rc != 0) return abort_comm("ncclCommGetAsyncError: " + rccl_err(rc));
    if (async != 0) return abort_comm("RCCL asynchronous error: " + rccl_err(async));
    if (timeout_ms < 0) return NLMC_OK;                      // error flag only, no wait
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipStreamQuery(c->stream);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) return abort_comm(std::string("hipStreamQuery: ") + hipGetErrorString(q));
        rc = g_rccl.CommGetAsyncError(c->comm, &async);
        if (rc != 0 || async != 0) return abort_comm("RCCL asynchronous error: " + rccl_err(rc != 0 ? rc : async));
        if (std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() > timeout_ms)
            return abort_comm("the collectives queued on the context's stream did not finish within " + std::to_string(timeout_ms) + " ms (a rank lost?)");
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    return NLMC_OK;
}

// ---- APT run cut into temperature-slot blocks over ranks (csrc/nlmc_apt.h) ---------------------------------------------------
int nlmc_apt_shard(nlmc_ctx *c, int R_global, int world, int rank, const double *beta_global)
{
    if (!c || !beta_global) return fail(c, NLMC_ERR_ARG, "nlmc_apt_shard: NULL argument");
    if (c->ladder_len == 0) return fail(c, NLMC_ERR_STATE, "nlmc_apt_shard: call nlmc_pt_init with this rank's block of the ladder first");
    const int L = c->ladder_len;
    if (world < 1 || rank < 0 || rank >= world || R_global != world * L)
        return fail(c, NLMC_ERR_ARG, "nlmc_apt_shard: R_global must be world x the local ladder length");
    if (c->apt_systems > 1)
        return fail(c, NLMC_ERR_UNSUPPORTED, "nlmc_apt_shard: the context is divided into several systems (nlmc_apt_systems): slot-keyed random numbers know one");
    if (c->chain_base != 0 || c->n_chains != c->n_chains_global)
        return fail(c, NLMC_ERR_ARG, "nlmc_apt_shard: the context must be self-contained (K ladders of its own slots: chain_base 0, n_chains_global == n_chains)");
    for (int i = 0; i < L; ++i)
        if (beta_global[(size_t)rank * L + i] != c->beta_list[(size_t)i])
            return fail(c, NLMC_ERR_ARG, "nlmc_apt_shard: nlmc_pt_init was not given block `rank` of beta_global");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t K = (size_t)(c->n_chains / L);
    HIP_TRY(c, c->apt_beta.reserve((size_t)R_global));
    HIP_TRY(c, c->apt_e_all.reserve((size_t)world * K * L));
    HIP_TRY(c, c->apt_send.reserve(2 * K * (size_t)c->n_pad));
    HIP_TRY(c, c->apt_recv.reserve(2 * K * (size_t)c->n_pad));
    HIP_TRY(c, c->apt_bd.reserve(2 * K));
    HIP_TRY(c, hipMemcpyAsync(c->apt_beta.p, beta_global, sizeof(double) * (size_t)R_global, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->apt_e_all.p, 0, sizeof(long long) * (size_t)world * K * L, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->apt_recv.p, 0, 2 * K * (size_t)c->n_pad, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->apt_bd.p, 0, sizeof(int32_t) * 2 * K, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->apt_R = R_global; c->apt_world = world; c->apt_rank = rank;
    c->rng_stride = R_global; c->rng_base = rank * L;
    c->pt_plan.on = false;                           // (a selection planned over the local ladder is not this mode's)
    return NLMC_OK;
}

// A context of M K ladders as M independent APT systems: system s owns ladders s K .. s K + K - 1 and only its Houdayer pairing changes
// (nlmc_icm_round_ladders, nlmc_apt_rounds_lanes); everything else is keyed by global chain or ladder ids as before.
int nlmc_apt_systems(nlmc_ctx *c, int n_systems)
{
    if (!c) return NLMC_ERR_ARG;
    if (c->ladder_len == 0) return fail(c, NLMC_ERR_STATE, "nlmc_apt_systems: call nlmc_pt_init first");
    if (n_systems < 1 || (c->n_chains_global / c->ladder_len) % n_systems != 0)
        return fail(c, NLMC_ERR_ARG, "nlmc_apt_systems: n_systems must be at least 1 and divide the number of ladders");
    if (n_systems > 1 && c->rng_stride != 0)
        return fail(c, NLMC_ERR_UNSUPPORTED, "nlmc_apt_systems: random numbers keyed by temperature slot (nlmc_apt_shard) know one system");
    c->apt_systems = n_systems;
    return NLMC_OK;
}

static int apt_require(nlmc_ctx *c, const char *who)
{
    if (!c) return NLMC_ERR_ARG;
    if (c->apt_R == 0) return fail(c, NLMC_ERR_STATE, std::string(who) + ": call nlmc_apt_shard first");
    return NLMC_OK;
}

static int apt_launch_pack(nlmc_ctx *c)
{
    const int L = c->ladder_len, K = c->n_chains / L;
    AptPackArgs a{};
    a.L = L; a.K = K; a.n_pad = c->n_pad;
    a.chain_of_slot = c->chain_of_slot.p; a.efix = c->efix.p; a.spins = c->spins.p;
    a.e_block = c->apt_e_all.p + (size_t)c->apt_rank * K * L;
    a.send = c->apt_send.p;
    hipLaunchKernelGGL(k_apt_pack, dim3(2 * K + 1), dim3(256), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return NLMC_OK;
}

// decision of every selected pair + label exchanges inside the block + adoption of the accepted boundary pairs
static int apt_launch_swap(nlmc_ctx *c, uint32_t round, uint64_t seed, int n_pairs, int32_t *out_pairs, uint8_t *out_accepted)
{
    const int L = c->ladder_len, K = c->n_chains / L;
    HIP_TRY(c, c->pt_pairs.reserve((size_t)K * n_pairs * 2));
    HIP_TRY(c, c->pt_acc.reserve((size_t)K * n_pairs));
    AptSwapArgs a{};
    a.L = L; a.R = c->apt_R; a.K = K; a.n_pairs = n_pairs; a.world = c->apt_world; a.rank = c->apt_rank;
    a.round = round; a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    a.beta = c->apt_beta.p; a.e_all = c->apt_e_all.p; a.escale = c->escale;
    a.slot_of_chain = c->slot_of_chain.p; a.chain_of_slot = c->chain_of_slot.p;
    a.out_pairs = c->pt_pairs.p; a.out_acc = c->pt_acc.p; a.status = c->pt_status.p; a.bd = c->apt_bd.p;
    swap_window_rows(c, a, round, seed, n_pairs, (size_t)K, out_pairs || out_accepted);
    c->sub_dirty = true;
    hipLaunchKernelGGL(k_apt_swap, dim3(K), dim3(swap_block(a.plan_pairs != nullptr, n_pairs)), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    if (c->apt_world > 1) {
        AptAdoptArgs d{};
        d.L = L; d.K = K; d.n_pad = c->n_pad; d.world = c->apt_world; d.rank = c->apt_rank; d.escale = c->escale;
        d.bd = c->apt_bd.p; d.chain_of_slot = c->chain_of_slot.p; d.recv = c->apt_recv.p; d.e_all = c->apt_e_all.p;
        d.spins = c->spins.p; d.efix = c->efix.p; d.energy_sink = c->energy_sink;
        hipLaunchKernelGGL(k_apt_adopt, dim3(2 * K), dim3(256), 0, c->stream, d);
        HIP_TRY(c, hipGetLastError());
    }
    return swap_read_back(c, K, n_pairs, out_pairs, out_accepted);
}

static int apt_check_pairs(nlmc_ctx *c, int n_pairs)
{
    if (n_pairs < 0 || n_pairs > std::max(0, c->apt_R - 1)) return fail(c, NLMC_ERR_ARG, "Cannot find non-overlapping pairs.");
    if (c->apt_R > 4096) return fail(c, NLMC_ERR_UNSUPPORTED, "nlmc_apt_swap: ladder_len > 4096");
    return NLMC_OK;
}

int nlmc_apt_pack(nlmc_ctx *c, int64_t *out_slot_efix, int8_t *out_lo, int8_t *out_hi)
{
    { int rc = apt_require(c, "nlmc_apt_pack"); if (rc) return rc; }
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = apt_launch_pack(c); if (rc) return rc; }
    const int L = c->ladder_len, K = c->n_chains / L;
    if (out_slot_efix)
        HIP_TRY(c, hipMemcpyAsync(out_slot_efix, c->apt_e_all.p + (size_t)c->apt_rank * K * L, sizeof(long long) * (size_t)K * L, hipMemcpyDeviceToHost, c->stream));
    for (int side = 0; side < 2; ++side) {
        int8_t *dst = side ? out_hi : out_lo;
        if (!dst) continue;
        c->stage_out.resize((size_t)c->n_pad * K);
        HIP_TRY(c, hipMemcpyAsync(c->stage_out.data(), c->apt_send.p + (size_t)side * K * c->n_pad, c->stage_out.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        rows_to_host_finish(c, dst, K);
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NLMC_OK;
}

int nlmc_apt_swap_host(nlmc_ctx *c, uint32_t round, uint64_t seed, int n_pairs, const int64_t *efix_all, const int8_t *recv_lo,
                       const int8_t *recv_hi, int32_t *out_pairs, uint8_t *out_accepted)
{
    { int rc = apt_require(c, "nlmc_apt_swap_host"); if (rc) return rc; }
    { int rc = apt_check_pairs(c, n_pairs); if (rc) return rc; }
    if (!efix_all || (c->apt_rank > 0 && !recv_lo) || (c->apt_rank + 1 < c->apt_world && !recv_hi))
        return fail(c, NLMC_ERR_ARG, "nlmc_apt_swap_host: the gathered energies and the neighbours' boundary configurations are required");
    HIP_TRY(c, hipSetDevice(c->device));
    if (n_pairs == 0) return NLMC_OK;
    const int L = c->ladder_len, K = c->n_chains / L;
    HIP_TRY(c, hipMemcpyAsync(c->apt_e_all.p, efix_all, sizeof(long long) * (size_t)c->apt_world * K * L, hipMemcpyHostToDevice, c->stream));
    if (c->apt_rank > 0) { int rc = rows_to_device(c, c->apt_recv.p, recv_lo, K); if (rc) return rc; }
    if (c->apt_rank + 1 < c->apt_world) { int rc = rows_to_device(c, c->apt_recv.p + (size_t)K * c->n_pad, recv_hi, K); if (rc) return rc; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));          // the caller's buffers may go away after the call
    return apt_launch_swap(c, round, seed, n_pairs, out_pairs, out_accepted);
}

// Rehearsal of the neighbour exchange on ONE rank: the grouped ncclSend / ncclRecv pair of nlmc_apt_swap_collective with this rank
// as its own neighbour on both sides (a send to oneself inside a group is legal): what rank - 1 would receive from this rank's
// bottom-slot chains comes back as `from the upper neighbour`, and the other way round.
int nlmc_apt_selftest_exchange(nlmc_ctx *c, int8_t *out_recv_lo, int8_t *out_recv_hi)
{
    { int rc = apt_require(c, "nlmc_apt_selftest_exchange"); if (rc) return rc; }
    if (!c->comm) return fail(c, NLMC_ERR_STATE, "nlmc_apt_selftest_exchange: call nlmc_comm_init first");
    if (!out_recv_lo || !out_recv_hi) return fail(c, NLMC_ERR_ARG, "nlmc_apt_selftest_exchange: NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = apt_launch_pack(c); if (rc) return rc; }
    const int L = c->ladder_len, K = c->n_chains / L, me = c->comm_rank;
    const size_t rowbytes = (size_t)K * c->n_pad;
    int rc = g_rccl.GroupStart();
    if (rc == 0) rc = g_rccl.Send(c->apt_send.p, rowbytes, /*ncclInt8*/ 0, me, c->comm, c->stream);                 // my bottom-slot chains ...
    if (rc == 0) rc = g_rccl.Recv(c->apt_recv.p + rowbytes, rowbytes, 0, me, c->comm, c->stream);                   // ... arrive as the upper neighbour's
    if (rc == 0) rc = g_rccl.Send(c->apt_send.p + rowbytes, rowbytes, 0, me, c->comm, c->stream);                   // my top-slot chains ...
    if (rc == 0) rc = g_rccl.Recv(c->apt_recv.p, rowbytes, 0, me, c->comm, c->stream);                              // ... as the lower neighbour's
    const int rc2 = g_rccl.GroupEnd();
    if (rc != 0 || rc2 != 0) return fail(c, NLMC_ERR_HIP, "ncclSend / ncclRecv: " + rccl_err(rc != 0 ? rc : rc2));
    for (int side = 0; side < 2; ++side) {
        c->stage_out.resize(rowbytes);
        HIP_TRY(c, hipMemcpyAsync(c->stage_out.data(), c->apt_recv.p + (size_t)side * rowbytes, rowbytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        rows_to_host_finish(c, side ? out_recv_hi : out_recv_lo, K);
    }
    return nlmc_comm_check(c, 10000);
}

int nlmc_apt_swap_collective(nlmc_ctx *c, uint32_t round, uint64_t seed, int n_pairs, int32_t *out_pairs, uint8_t *out_accepted)
{
    { int rc = apt_require(c, "nlmc_apt_swap_collective"); if (rc) return rc; }
    { int rc = apt_check_pairs(c, n_pairs); if (rc) return rc; }
    if (c->apt_world > 1 && !c->comm) return fail(c, NLMC_ERR_STATE, "nlmc_apt_swap_collective: call nlmc_comm_init first");
    HIP_TRY(c, hipSetDevice(c->device));
    if (n_pairs == 0) return NLMC_OK;
    { int rc = apt_launch_pack(c); if (rc) return rc; }
    if (c->comm) {                          // (also with ONE rank: the in-place all-gather then rehearses the path on one GPU)
        const int L = c->ladder_len, K = c->n_chains / L, W = c->apt_world, me = c->apt_rank;
        const size_t blk = (size_t)K * L, rowbytes = (size_t)K * c->n_pad;
        // all on the stream the kernels run on: stream order is the only synchronisation.  The all-gather is in place (send = this
        // rank's block of the receive buffer); the two neighbour exchanges are one group (no deadlock whatever the order).
        int rc = g_rccl.AllGather(c->apt_e_all.p + (size_t)me * blk, c->apt_e_all.p, blk, /*ncclInt64*/ 4, c->comm, c->stream);
        if (rc != 0) return fail(c, NLMC_ERR_HIP, "ncclAllGather: " + rccl_err(rc));
        rc = g_rccl.GroupStart();
        if (rc == 0 && me > 0) rc = g_rccl.Send(c->apt_send.p, rowbytes, /*ncclInt8*/ 0, me - 1, c->comm, c->stream);
        if (rc == 0 && me > 0) rc = g_rccl.Recv(c->apt_recv.p, rowbytes, 0, me - 1, c->comm, c->stream);
        if (rc == 0 && me + 1 < W) rc = g_rccl.Send(c->apt_send.p + rowbytes, rowbytes, 0, me + 1, c->comm, c->stream);
        if (rc == 0 && me + 1 < W) rc = g_rccl.Recv(c->apt_recv.p + rowbytes, rowbytes, 0, me + 1, c->comm, c->stream);
        const int rc2 = g_rccl.GroupEnd();
        if (rc != 0 || rc2 != 0) return fail(c, NLMC_ERR_HIP, "ncclSend / ncclRecv: " + rccl_err(rc != 0 ? rc : rc2));
    }
    return apt_launch_swap(c, round, seed, n_pairs, out_pairs, out_accepted);
}

// One observation of every local chain for the open best-state record (k_best_update), on the context's stream.
static int launch_best_update(nlmc_ctx *c, uint32_t stamp)
{
    if (c->n_chains == 0) return NLMC_OK;
    BestArgs a{};
    a.b = c->best_rec(); a.efix = c->efix.p; a.spins = c->spins.p; a.n_pad = c->n_pad; a.escale = c->escale; a.stamp = (int32_t)stamp;
    hipLaunchKernelGGL(k_best_update, dim3((unsigned)c->n_chains), dim3(256), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return NLMC_OK;
}

// One observation of every local chain for the open energy log (k_elog_update), on the context's stream: the row of `round`, nothing
// when the round lies outside the window.
static int launch_elog_update(nlmc_ctx *c, uint32_t round)
{
    const ElogRec e = c->elog_rec(round, 1);
    if (!e.energy || c->n_chains == 0) return NLMC_OK;
    hipLaunchKernelGGL(k_elog_update, dim3((unsigned)((c->n_chains + 255) / 256)), dim3(256), 0, c->stream, e, c->efix.p, c->slot_of_chain.p,
                       c->chain_base, c->escale);
    HIP_TRY(c, hipGetLastError());
    return NLMC_OK;
}

// Why a context cannot run whole rounds by itself whatever the kernel, or nullptr: what nlmc_pt_rounds_fused, nlmc_pt_rounds_deferred
// and nlmc_pt_rounds_lanes refuse alike.  `strict` (deferred, lanes): a tracked minimum is refused too.
const char *rounds_context_refusal(const nlmc_ctx *c, bool strict)
{
    const int L = c->ladder_len;
    if (c->chain_base % L != 0 || c->n_chains % L != 0) return "the context's block cuts a ladder (the swap needs other contexts' energies)";
    if (c->comm || (c->apt_R > 0 && c->apt_world > 1)) return "the context takes part in a collective swap round";
    if (c->has_flags || c->subset != 0 || c->cur != c->stream || (strict && c->track_min))
        return strict ? "phase flags, a chain subset or a tracked minimum are in force" : "phase flags or a chain subset are in force";
    return nullptr;
}

// What every rounds entry point (`name`) checks first, in this order: the arguments, a ladder, anything to do.  NLMC_OK with go = false
// when there is nothing to do.
bool rounds_args_ok(int precision, int n_rounds, int T, int n_pairs)
{
    return n_rounds >= 0 && T >= 1 && (precision == NLMC_F32 || precision == NLMC_F64) && n_pairs >= 0;
}

int rounds_entry_check(nlmc_ctx *c, const std::string &name, int precision, int n_rounds, int T, int n_pairs, bool &go)
{
    go = false;
    if (!rounds_args_ok(precision, n_rounds, T, n_pairs)) return fail(c, NLMC_ERR_ARG, name + "bad argument");
    if (c->ladder_len == 0) return fail(c, NLMC_ERR_STATE, name + "call nlmc_pt_init first");
    go = n_rounds != 0 && c->n_chains != 0;
    return NLMC_OK;
}

// The same without a word, for nlmc_pt_rounds_deferred before it tries a short-chain route: the arguments are fine, there is a ladder
// and something to do, the pairs are in range and NLMC_NO_DEFERRED is unset.  (Where this says no the call goes on to rounds_check, which
// reports what is wrong.)
bool rounds_deferred_quiet_ok(const nlmc_ctx *c, int precision, int n_rounds, int T, int n_pairs)
{
    return rounds_args_ok(precision, n_rounds, T, n_pairs) && c->ladder_len > 0 && n_rounds != 0 && c->n_chains != 0 && n_pairs >= 1 &&
           n_pairs <= c->ladder_len - 1 && !c->knobs.no_deferred;
}

// The plan rows and the log rows (nullptr where `log` is false) of `round`, nl ladders wide: where a launch that starts at that round
// finds its planned selections and writes its pairs and decisions.  The windows cover the round (RoundWindow::covers).
struct RoundRows { const int32_t *plan_pairs; int32_t *log_pairs; uint8_t *log_acc; };
RoundRows round_rows(const nlmc_ctx *c, uint32_t round, size_t nl, int n_pairs, bool log)
{
    RoundRows r{};
    const size_t per_round = nl * (size_t)n_pairs;
    if (n_pairs > 0) r.plan_pairs = c->pt_plan_pairs.p + c->pt_plan.row(round) * per_round * 2;
    if (log) {
        r.log_pairs = c->pt_log_pairs.p + c->pt_log.row(round) * per_round * 2;
        r.log_acc = c->pt_log_acc.p + c->pt_log.row(round) * per_round;
    }
    return r;
}

// The checks nlmc_pt_rounds_fused (via rounds) and nlmc_pt_rounds_deferred (via deferred) share, in their order.  NLMC_OK with the
// plan slot and the arithmetic of the rounds in fslot / arith, fslot = -1 when there is nothing to do.
int rounds_check(nlmc_ctx *c, Via via, int precision, int n_rounds, int T, uint32_t sweep0, uint32_t round0, uint64_t seed, int n_pairs,
                 int &fslot, int &arith)
{
    const bool d = via == Via::deferred;
    const std::string name = d ? "nlmc_pt_rounds_deferred: " : "nlmc_pt_rounds_fused: ";
    fslot = -1;
    bool go = false;
    { int rc = rounds_entry_check(c, name, precision, n_rounds, T, n_pairs, go); if (rc || !go) return rc; }
    const int L = c->ladder_len;
    auto no = [&](const char *why) { return fail(c, NLMC_ERR_UNSUPPORTED, name + why); };
    if (d ? c->knobs.no_deferred : c->knobs.no_persistent) return no(d ? "switched off (NLMC_NO_DEFERRED)" : "switched off (NLMC_NO_PERSISTENT)");
    if (const char *why = rounds_context_refusal(c, d)) return no(why);
    if (d && n_pairs < 1) return no("no swap pairs");
    if (n_pairs > std::max(0, L - 1)) return fail(c, NLMC_ERR_ARG, "Cannot find non-overlapping pairs.");
    const int k = fused_plan_for(c, sweep0, n_rounds * T, seed);
    if (k < 0 || c->fz[k].T != T) return no("no fused-window plan of one window per round covers these sweeps");
    arith = fused_route(c, precision, NLMC_ORDER_SHARED, false, false, k, T, via);
    if (arith == NOT_FUSED) return no("the fp64 mode does not run on fused windows for this instance");
    if (n_pairs > 0 && !c->pt_plan.covers(round0, n_rounds, n_pairs, seed))
        return no("the pair selections of these rounds are not planned (nlmc_pt_plan)");
    fslot = k;
    return NLMC_OK;
}

// Can k_rounds_fused run this context's chains (all workgroups resident at once: they wait for each other)?  NLMC_OK with the answer
// in `yes`.  Asked of the runtime, which also refuses such a launch.
// The answer is kept per (kernel, block, LDS): the number of chains of a context does not change.
static int rounds_resident(nlmc_ctx *c, const void *kfun, int nt, size_t lds, bool &yes)
{
    if (c->rounds_res_kfun != kfun || c->rounds_res_nt != nt || c->rounds_res_lds != lds) {
        int per_cu = 0, n_cu = 0;
        HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfun, nt, lds));
        HIP_TRY(c, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device));
        c->rounds_res_kfun = kfun; c->rounds_res_nt = nt; c->rounds_res_lds = lds;
        c->rounds_res_yes = (long long)per_cu * n_cu >= c->n_chains;
    }
    yes = c->rounds_res_yes;
    return NLMC_OK;
}

// n_rounds rounds (T sweeps at the ladder temperatures + the swap round) in cooperative launches of k_rounds_fused, at most
// NLMC_ROUNDS_PER_LAUNCH rounds each (the rows of the record array).  The checks of rounds_check have passed.  `resident` = false
// (and nothing queued) when the device does not hold all the chains' workgroups at once.
static int rounds_in_launch(nlmc_ctx *c, int fslot, int arith, int n_rounds, int T, uint32_t sweep0, uint32_t round0, uint64_t seed, int n_pairs,
                            bool &resident)
{
    const int L = c->ladder_len;
    const nlmc_ctx::FusedPlan &P = c->fz[fslot];
    const bool real = arith == ARITH_R64;
    if (real && !P.has_val) return fail(c, NLMC_ERR_STATE, "k_rounds_fused: the plan has no fp64 value plane");
    const int kt = arith == ARITH_F64 ? 2 * c->xmax + 1 : 0;          // (the real-valued variant has no K tables: the f32 mode's LDS)
    const FusedLds Lds = fused_lds(c->n_pad, false, false, P.fmt == NLMC_FMT_ADDR, kt);
    const void *kfun = rounds_kernel(c->has_diag, P.fmt, arith, c->observed());
    if (!kfun) return fail(c, NLMC_ERR_STATE, "k_rounds_fused: no kernel for this arithmetic");
    { int rc = ensure_lds(c, kfun, Lds.total); if (rc) return rc; }
    const int nt = fused_block(c);
    { int rc = rounds_resident(c, kfun, nt, Lds.total, resident); if (rc || !resident) return rc; }
    const int nl = c->n_chains_global / L;
    const size_t G = (size_t)c->n_chains_global;
    HIP_TRY(c, c->rounds_rec.reserve((size_t)std::min(n_rounds, NLMC_ROUNDS_PER_LAUNCH) * G));
    { int rc = upload_ladder_tab(c, c->stream); if (rc) return rc; }
    const bool log = n_pairs > 0 && c->pt_log.covers(round0, n_rounds, n_pairs);
    // the two argument structs travel through device memory (k_rounds_fused reads them through laundered constant-memory pointers);
    // two device slots written in stream order, so that a launch still running never sees the next one's arguments.  The host
    // copies are pageable memory: hipMemcpyAsync has staged such a source when it returns, so a slot's host buffer may be filled
    // again by the chunk after next of the same call.
    const size_t a_bytes = (sizeof(SweepArgs) + 255) & ~(size_t)255, slot_bytes = a_bytes + ((sizeof(RoundsArgs) + 255) & ~(size_t)255);
    HIP_TRY(c, c->rounds_args.reserve(2 * slot_bytes));
    for (int at = 0; at < n_rounds; at += NLMC_ROUNDS_PER_LAUNCH) {
        const int k = std::min(NLMC_ROUNDS_PER_LAUNCH, n_rounds - at);
        const uint32_t s0 = sweep0 + (uint32_t)at * (uint32_t)T, r0 = round0 + (uint32_t)at;
        const int w0 = (int)((s0 - P.sweep0) / (uint32_t)T);
        // no record yet: all ones, a NaN that no energy equals (0.0 is a legal energy)
        HIP_TRY(c, hipMemsetAsync(c->rounds_rec.p, 0xFF, sizeof(unsigned long long) * (size_t)k * G, c->stream));
        SweepArgs a = sweep_args(c, s0, T, seed, c->pt_tab.p, 2, 0, true);
        fused_args(c, P, Lds, a);
        a.trace_sweeps = T; a.rec_stride = 1;
        { int rc = stamps_arm(c, a, c->n_chains, c->stream); if (rc) return rc; }
        RoundsArgs q{};
        q.n_rounds = k; q.n_windows_avail = c->knobs.no_warm ? k : P.windows - w0;
        const nlmc_ctx::FusedPlan::Arrays A = P.at(w0);
        q.loff = A.loff; q.nlev = A.nlev; q.himax = A.himax; q.send = A.send; q.npos = A.npos; q.head = A.head; q.ell = A.ell;
        q.val = real ? A.val : nullptr;
        q.hs = head_stream(c, P, false, arith) ? A.hs : nullptr;
        q.ladder_len = L; q.n_pairs = n_pairs; q.n_ladders = nl; q.round0 = r0;
        const RoundRows rows = round_rows(c, r0, (size_t)nl, n_pairs, log);
        q.plan_pairs = rows.plan_pairs; q.log_pairs = rows.log_pairs; q.log_acc = rows.log_acc;
        q.beta = c->pt_beta.p; q.slot_of_chain = c->slot_of_chain.p; q.chain_of_slot = c->chain_of_slot.p;
        q.rec = c->rounds_rec.p; q.status = c->pt_status.p;
        q.timeout_ticks = 100000000ll * 20;                   // 20 s of the 100 MHz wall clock
        if (c->best_on) q.best = c->best_rec();               // (the record lives in global memory: it carries over from launch to launch)
        q.elog = c->elog_rec(r0, k);                          // (the row of the launch's first round: round0 + at of the call)
        // events around the launch while timings accumulate: its time counts for its k rounds
        TimerSpan ts;
        if (c->ev_accumulate) { int rc = span_begin(c, ts, 1, c->stream); if (rc) return rc; }
        const int as = c->rounds_args_slot ^= 1;
        std::vector<unsigned char> &hb = c->rounds_args_host[as];
        hb.assign(slot_bytes, 0);
        std::memcpy(hb.data(), &a, sizeof(SweepArgs));
        std::memcpy(hb.data() + a_bytes, &q, sizeof(RoundsArgs));
        unsigned char *dargs = c->rounds_args.p + (size_t)as * slot_bytes;
        HIP_TRY(c, hipMemcpyAsync(dargs, hb.data(), slot_bytes, hipMemcpyHostToDevice, c->stream));
        const SweepArgs *ap_dev = reinterpret_cast<const SweepArgs *>(dargs);
        const RoundsArgs *qp_dev = reinterpret_cast<const RoundsArgs *>(dargs + a_bytes);
        void *kargs[] = {&ap_dev, &qp_dev};
        HIP_TRY(c, hipLaunchCooperativeKernel(kfun, dim3(c->n_chains), dim3(nt), kargs, (unsigned)Lds.total, c->stream));
        HIP_TRY(c, hipGetLastError());
        { int rc = span_end(c, ts); if (rc) return rc; }
        count_launches(c, k, c->ev_accumulate);
        c->stat_fused_window = w0 + k - 1;
    }
    c->stat_fused_slot = fslot;
    c->stat_head_path = head_stream(c, P, false, arith) ? NLMC_HEADS_STREAM : NLMC_HEADS_LOADS;
    c->sub_dirty = true;
    c->rounds_route = NLMC_ROUNDS_IN_LAUNCH;
    return NLMC_OK;
}

// ---- tempering rounds of short chains: a ladder per wave (k_rounds_lanes, csrc/nlmc_lane_rounds.h) ----------------------------------
// The routes that run whole rounds of short chains in one launch: k_rounds_lanes, k_rounds_waves, k_rounds_waves_long, k_apt_rounds_lanes.
enum class ShortRounds { lanes, waves, waves_long, apt_lanes };

// The reach of a route's kernels: the chain lengths they take, whether they have the fixed-point arithmetic only, and what a chain or
// a ladder beyond them is told (a ladder lives inside one wave, or inside one workgroup's swap wave).  Rows in the order of ShortRounds.
struct ShortReach { int n_min, n_max; bool f32_only; const char *why_n, *why_ladder; };
ShortReach short_reach(ShortRounds route)
{
    static const char *const lane_n = "the chain-per-lane kernels take chains of at most NLMC_LANE_N spins";
    static const char *const in_wave = "a ladder of more than 64 temperatures does not fit a wave";
    static const char *const in_swap_wave = "a ladder of more than 64 temperatures does not fit a workgroup's swap wave";
    static const ShortReach reach[] = {
        {0, NLMC_LANE_N, false, lane_n, in_wave},
        {0, NLMC_WAVE_N, true, "the wave-per-chain kernels take chains of at most NLMC_WAVE_N spins", in_swap_wave},
        {NLMC_WAVE_N + 1, NLMC_WAVE_LONG_N, true,
         "the long wave-per-chain kernels take chains of more than NLMC_WAVE_N and at most NLMC_WAVE_LONG_N spins", in_swap_wave},
        {0, NLMC_LANE_N, false, lane_n, in_wave}};
    return reach[(int)route];
}

// Why this context cannot run rounds [round0, round0 + n_rounds) on `route`, or nullptr: the checks of rounds_check that do not concern
// fused plans, the reach of the route's kernels (short_reach; waves_long: also one ladder's regions inside a workgroup's LDS).  The APT
// rounds have their Houdayer step: n_pairs = 0, a round without swaps, is taken.  Arguments are checked by the callers.
const char *short_rounds_refusal(const nlmc_ctx *c, ShortRounds route, int precision, int n_rounds, int T, uint32_t round0, uint64_t seed, int n_pairs)
{
    const ShortReach reach = short_reach(route);
    if (const char *why = rounds_context_refusal(c, true)) return why;
    if (n_pairs < 1 && route != ShortRounds::apt_lanes) return "no swap pairs";
    if (reach.f32_only && precision != NLMC_F32) return "the wave-per-chain kernels have the fixed-point arithmetic (NLMC_F32) only";
    if (c->knobs.force_big || c->n < reach.n_min || c->n > reach.n_max) return reach.why_n;
    if (c->ladder_len > 64) return reach.why_ladder;
    // (whether ONE ladder fits a workgroup depends neither on the device nor on the number of ladders)
    if (route == ShortRounds::waves_long && nlmc_wave_long_rounds_shape(c->n, c->n_pad, c->ladder_len, 1, 1, 0).R == 0)
        return "the ladders of a workgroup do not fit its LDS";
    if (n_pairs >= 1 && !c->pt_plan.covers(round0, n_rounds, n_pairs, seed)) return "the pair selections of these rounds are not planned (nlmc_pt_plan)";
    if ((size_t)T * (size_t)c->n * sizeof(uint16_t) > c->knobs.lane_scratch)
        return "the visiting orders of one round exceed the order scratch (NLMC_LANE_SCRATCH)";
    return nullptr;
}

// The LaneRoundsArgs of a launch of k rounds from round r0 on, nl ladders in the plan and log rows, the slot maps at LDS offset map_off.
// Observers: the open best-state record and the rows of the open energy log the launch falls on.
LaneRoundsArgs lane_rounds_args(const nlmc_ctx *c, int k, uint32_t r0, int n_pairs, size_t nl, bool log, size_t map_off)
{
    LaneRoundsArgs q{};
    q.n_rounds = k; q.ladder_len = c->ladder_len; q.n_pairs = n_pairs; q.n_ladders = (int)nl; q.round0 = r0;
    const RoundRows rows = round_rows(c, r0, nl, n_pairs, log);
    q.plan_pairs = rows.plan_pairs; q.log_pairs = rows.log_pairs; q.log_acc = rows.log_acc;
    q.beta = c->pt_beta.p; q.slot_of_chain = c->slot_of_chain.p; q.chain_of_slot = c->chain_of_slot.p;
    q.lds_map_off = (int)map_off;
    if (c->best_on) q.best = c->best_rec();
    q.elog = c->elog_rec(r0, k);
    return q;
}

// What every launch of a lane rounds driver passes first: the SweepArgs of T sweeps from s0 at the ladder temperatures (lane_fields over
// all chains; uniform tables in LDS at u_off where `tab`) and the LaneRoundsArgs of k rounds from r0 (lane_rounds_args).
struct LaneLaunchArgs { SweepArgs a; LaneRoundsArgs q; };
LaneLaunchArgs lane_launch_args(const nlmc_ctx *c, int T, uint64_t seed, uint32_t s0, int k, uint32_t r0, int n_pairs, size_t nl, bool log, bool tab,
                                size_t u_off, size_t map_off)
{
    LaneLaunchArgs x{sweep_args(c, s0, T, seed, c->pt_tab.p, 2, 0, true), lane_rounds_args(c, k, r0, n_pairs, nl, log, map_off)};
    lane_fields(c, x.a, c->n_chains, tab, u_off);
    return x;
}

// The launches of a lane rounds driver: n_rounds rounds in chunks of as many whole rounds as the order scratch holds visiting orders
// for.  Per chunk of k rounds from round r0 (sweep s0, `at` rounds into the call): k_lane_orders (the "levelize" half of the timings),
// then launch(at, k, s0, r0) puts the caller's kernel kfun (lds bytes of dynamic LDS) on the context's stream.  `route`: the
// NLMC_ROUTE_* nlmc_last_sweep_route reports after the call.
extern "C++" template <typename Launch>
int lane_rounds_chunks(nlmc_ctx *c, const void *kfun, size_t lds, int n_rounds, int T, uint32_t sweep0, uint32_t round0, uint64_t seed, int route,
                       Launch launch)
{
    const size_t bytes_per_round = (size_t)T * (size_t)c->n * sizeof(uint16_t);
    const int K = (int)std::max<size_t>(1, std::min<size_t>({(size_t)n_rounds, c->knobs.lane_scratch / bytes_per_round, (size_t)(INT_MAX / 2) / (size_t)T}));
    begin_sweep_call(c);
    c->stat_orders = 0; c->stat_levels = 0; c->stats_pending = false;
    c->stat_fused_window = -1;
    c->stat_lane_orders = 0;
    HIP_TRY(c, c->lane_perm.reserve((size_t)K * (size_t)T * (size_t)c->n));
    { int rc = upload_ladder_tab(c, c->stream); if (rc) return rc; }
    { int rc = ensure_lds(c, kfun, lds); if (rc) return rc; }
    for (int at = 0; at < n_rounds; at += K) {
        const int k = std::min(K, n_rounds - at);
        const uint32_t s0 = sweep0 + (uint32_t)at * (uint32_t)T, r0 = round0 + (uint32_t)at;
        TimerSpan ts;
        if (c->ev_accumulate) { int rc = span_begin(c, ts, 0, c->stream); if (rc) return rc; }
        { int rc = launch_lane_orders(c, c->stream, (size_t)k * T, k * T, 0, s0, seed); if (rc) return rc; }
        { int rc = span_mid(c, ts); if (rc) return rc; }
        { int rc = launch(at, k, s0, r0); if (rc) return rc; }
        HIP_TRY(c, hipGetLastError());
        { int rc = span_end(c, ts); if (rc) return rc; }
        count_launches(c, k, c->ev_accumulate);
    }
    c->sub_dirty = true;
    c->last_route = route;
    return NLMC_OK;
}

// n_rounds rounds in launches of k_rounds_lanes.  short_rounds_refusal said nullptr.
int rounds_lanes(nlmc_ctx *c, int precision, int n_rounds, int T, uint32_t sweep0, uint32_t round0, uint64_t seed, int n_pairs)
{
    const int L = c->ladder_len, P = 64 / L, ladders = c->n_chains / L;
    LaneLds Lds = lane_lds(c);
    const size_t map_off = (Lds.total + 15) & ~(size_t)15;              // lane_of_slot | slot_of_lane, 64 bytes each
    Lds.total = map_off + 128;
    const void *kfun = rounds_lanes_kernel(precision == NLMC_F64, c->observed());
    const bool log = c->pt_log.covers(round0, n_rounds, n_pairs);
    int rc = lane_rounds_chunks(c, kfun, Lds.total, n_rounds, T, sweep0, round0, seed, NLMC_ROUTE_LANES, [&](int, int k, uint32_t s0, uint32_t r0) -> int {
        LaneLaunchArgs x = lane_launch_args(c, T, seed, s0, k, r0, n_pairs, (size_t)(c->n_chains_global / L), log, Lds.tab, Lds.u_off, map_off);
        void *kargs[] = {&x.a, &x.q};
        HIP_TRY(c, hipLaunchKernel(kfun, dim3((unsigned)((ladders + P - 1) / P)), dim3(64), kargs, Lds.total, c->stream));
        return NLMC_OK;
    });
    if (rc) return rc;
    c->rounds_route = NLMC_ROUNDS_LANES;
    return NLMC_OK;
}

// ---- tempering rounds inside a wave launch: a ladder per workgroup (k_rounds_waves, csrc/nlmc_wave_rounds.h; k_rounds_waves_long for
// chains of more than NLMC_WAVE_N spins, csrc/nlmc_wave_long_rounds.h) ----------------------------------------------------------------
// k_rounds_waves<R, jlds, observed> for R <= 4; k_rounds_waves_long<R, observed> beyond, which never stages the matrix
const void *rounds_waves_kernel(int R, bool jlds, bool observed)
{
#define NLMC_RW(R_) {{reinterpret_cast<const void *>(k_rounds_waves<R_, false, false>), reinterpret_cast<const void *>(k_rounds_waves<R_, false, true>)}, \
                     {reinterpret_cast<const void *>(k_rounds_waves<R_, true, false>), reinterpret_cast<const void *>(k_rounds_waves<R_, true, true>)}}
#define NLMC_RWL(R_) {{reinterpret_cast<const void *>(k_rounds_waves_long<R_, false>), reinterpret_cast<const void *>(k_rounds_waves_long<R_, true>)}, \
                      {nullptr, nullptr}}
    static const void *const table[5][2][2] = {NLMC_RW(1), NLMC_RW(2), NLMC_RW(4), NLMC_RWL(8), NLMC_RWL(16)};
#undef NLMC_RW
#undef NLMC_RWL
    return table[wave_fields_row(R)][jlds ? 1 : 0][observed ? 1 : 0];
}

// n_rounds rounds in launches of k_rounds_waves (route waves) or k_rounds_waves_long (route waves_long).  short_rounds_refusal said nullptr.
int rounds_waves(nlmc_ctx *c, ShortRounds route, int n_rounds, int T, uint32_t sweep0, uint32_t round0, uint64_t seed, int n_pairs)
{
    const int L = c->ladder_len, ladders = c->n_chains / L;
    const bool longs = route == ShortRounds::waves_long;
    { int rc = cu_count(c); if (rc) return rc; }
    const NlmcWaveRoundsShape S =
        longs ? nlmc_wave_long_rounds_shape(c->n, c->n_pad, L, ladders, c->n_cu, c->knobs.wave_rounds_ladders)
              : nlmc_wave_rounds_shape(c->n, c->n_pad, L, ladders, c->n_cu, c->knobs.wave_rounds_ladders, c->knobs.wave_jlds ? 1 : 0);
    if (S.R == 0)
        return fail(c, NLMC_ERR_STATE, longs ? "rounds_waves_long: the chain or the ladder does not fit the wave kernels"
                                             : "rounds_waves: the chain or the ladder does not fit the wave kernels");
    const void *kfun = rounds_waves_kernel(S.R, S.jlds != 0, c->observed());
    { int rc = ensure_wave_matrix(c, S.stride); if (rc) return rc; }
    const bool log = c->pt_log.covers(round0, n_rounds, n_pairs);
    WaveRoundsArgs w{S.P, S.C};
    int rc = lane_rounds_chunks(c, kfun, S.lds, n_rounds, T, sweep0, round0, seed, NLMC_ROUTE_WAVES, [&](int, int k, uint32_t s0, uint32_t r0) -> int {
        LaneLaunchArgs x = lane_launch_args(c, T, seed, s0, k, r0, n_pairs, (size_t)(c->n_chains_global / L), log, false, 0, 0);
        x.a.wave_J = c->wave_J.p;
        void *kargs[] = {&x.a, &x.q, &w};
        HIP_TRY(c, hipLaunchKernel(kfun, dim3((unsigned)S.blocks), dim3((unsigned)(64 * S.W)), kargs, S.lds, c->stream));
        return NLMC_OK;
    });
    if (rc) return rc;
    c->rounds_route = longs ? NLMC_ROUNDS_WAVES_LONG : NLMC_ROUNDS_WAVES;
    return NLMC_OK;
}

// n_rounds rounds on `route` (lanes, waves or waves_long), for which short_rounds_refusal said nullptr.
int short_rounds(nlmc_ctx *c, ShortRounds route, int precision, int n_rounds, int T, uint32_t sweep0, uint32_t round0, uint64_t seed, int n_pairs)
{
    HIP_TRY(c, hipSetDevice(c->device));
    return route == ShortRounds::lanes ? rounds_lanes(c, precision, n_rounds, T, sweep0, round0, seed, n_pairs)
                                       : rounds_waves(c, route, n_rounds, T, sweep0, round0, seed, n_pairs);
}

// nlmc_pt_rounds_lanes / nlmc_pt_rounds_waves / nlmc_pt_rounds_waves_long (`fn`): n_rounds rounds in launches of the route's kernel, whatever the lane
// or wave mode is and whatever nlmc_pt_rounds_deferred would choose.
int short_rounds_by_name(nlmc_ctx *c, ShortRounds route, const char *fn, int precision, int n_rounds, int T, uint32_t sweep0, uint32_t round0,
                         uint64_t seed, int n_pairs)
{
    if (!c) return NLMC_ERR_ARG;
    const std::string name = std::string(fn) + ": ";
    bool go = false;
    { int rc = rounds_entry_check(c, name, precision, n_rounds, T, n_pairs, go); if (rc || !go) return rc; }
    if (n_pairs > std::max(0, c->ladder_len - 1)) return fail(c, NLMC_ERR_ARG, "Cannot find non-overlapping pairs.");
    if (const char *why = short_rounds_refusal(c, route, precision, n_rounds, T, round0, seed, n_pairs)) return fail(c, NLMC_ERR_UNSUPPORTED, name + why);
    return short_rounds(c, route, precision, n_rounds, T, sweep0, round0, seed, n_pairs);
}

int nlmc_pt_rounds_lanes(nlmc_ctx *c, int precision, int n_rounds, int sweeps_per_round, uint32_t sweep0, uint32_t round0, uint64_t seed,
                         int n_pairs)
{
    return short_rounds_by_name(c, ShortRounds::lanes, "nlmc_pt_rounds_lanes", precision, n_rounds, sweeps_per_round, sweep0, round0, seed, n_pairs);
}

int nlmc_pt_rounds_waves(nlmc_ctx *c, int precision, int n_rounds, int sweeps_per_round, uint32_t sweep0, uint32_t round0, uint64_t seed,
                         int n_pairs)
{
    return short_rounds_by_name(c, ShortRounds::waves, "nlmc_pt_rounds_waves", precision, n_rounds, sweeps_per_round, sweep0, round0, seed, n_pairs);
}

int nlmc_pt_rounds_waves_long(nlmc_ctx *c, int precision, int n_rounds, int sweeps_per_round, uint32_t sweep0, uint32_t round0, uint64_t seed,
                              int n_pairs)
{
    return short_rounds_by_name(c, ShortRounds::waves_long, "nlmc_pt_rounds_waves_long", precision, n_rounds, sweeps_per_round, sweep0, round0, seed,
                                n_pairs);
}

int nlmc_set_wave_long_rounds(nlmc_ctx *c, int on)
{
    if (!c) return NLMC_ERR_ARG;
    c->wave_long_rounds = on != 0;
    return NLMC_OK;
}

int nlmc_set_wave_rounds(nlmc_ctx *c, int on)
{
    if (!c) return NLMC_ERR_ARG;
    c->wave_rounds = on != 0;
    return NLMC_OK;
}

int nlmc_set_wave_long(nlmc_ctx *c, int on)
{
    if (!c) return NLMC_ERR_ARG;
    c->wave_long = on != 0;
    return NLMC_OK;
}

// Whether nlmc_pt_rounds_deferred takes k_rounds_lanes where the lane mode routes the context's sweeps to the lane kernels.  The rule
// (that of ROUNDS_REAL_IN_LAUNCH): only if its median time per run is not above that of lane sweeps round by round on the same build
// by more than the run-to-run spread at any shape of scripts/lane_rounds_throughput.py.  Measured (DESIGN.md section 6,
// profiles/lane_rounds_throughput.txt): below it at all 48 shapes, 1.02-1.08x at T = 1000 up to 4.7-6.4x at T = 1 on n = 10.
constexpr bool ROUNDS_LANES_IN_LAUNCH = true;
// (APT_LANES_IN_LAUNCH, the same rule for APT_ICM's rounds in k_apt_rounds_lanes, is a constant of engine.py: the class, not this
// library, chooses between nlmc_apt_rounds_lanes and a call per step.)

// n_rounds rounds in cooperative launches of k_rounds_fused, whatever nlmc_pt_rounds_deferred would choose.
int nlmc_pt_rounds_fused(nlmc_ctx *c, int precision, int n_rounds, int sweeps_per_round, uint32_t sweep0, uint32_t round0, uint64_t seed,
                         int n_pairs)
{
    if (!c) return NLMC_ERR_ARG;
    int fslot = -1, arith = NOT_FUSED;
    { int rc = rounds_check(c, Via::rounds, precision, n_rounds, sweeps_per_round, sweep0, round0, seed, n_pairs, fslot, arith); if (rc || fslot < 0) return rc; }
    HIP_TRY(c, hipSetDevice(c->device));
    bool resident = false;
    int rc = rounds_in_launch(c, fslot, arith, n_rounds, sweeps_per_round, sweep0, round0, seed, n_pairs, resident);
    if (rc == NLMC_OK && !resident)
        return fail(c, NLMC_ERR_UNSUPPORTED, "nlmc_pt_rounds_fused: more chains than workgroups the device holds at once");
    return rc;
}

// Whether nlmc_pt_rounds_deferred takes k_rounds_fused for real-valued fp64 instances too.  The rule: only when
// its median time per round is below the launch-per-round one by more than the run-to-run spread at both shapes of
// scripts/f64_real_throughput.py; not shown so far, so such calls keep a launch per round and nlmc_pt_rounds_fused reaches the kernel.
constexpr bool ROUNDS_REAL_IN_LAUNCH = false;

// n_rounds rounds as n_rounds sweep calls at the ladder temperatures and n_rounds swap calls, on whatever route the sweep calls take:
// what a caller that drives the rounds one by one queues.  An open best-state record and energy log observe every round between
// its sweeps and its swap, as they do on the other rounds routes.
int rounds_waves_call_by_call(nlmc_ctx *c, int precision, int n_rounds, int T, uint32_t sweep0, uint32_t round0, uint64_t seed, int n_pairs)
{
    for (int r = 0; r < n_rounds; ++r) {
        int rc = nlmc_sweep_philox(c, precision, NLMC_ORDER_SHARED, T, sweep0 + (uint32_t)r * (uint32_t)T, seed, nullptr, 0, 0, 0, nullptr, nullptr,
                                   nullptr, nullptr, nullptr);
        if (rc) return rc;
        if (c->best_on) { rc = launch_best_update(c, round0 + (uint32_t)r); if (rc) return rc; }
        if (c->elog_on) { rc = launch_elog_update(c, round0 + (uint32_t)r); if (rc) return rc; }
        rc = nlmc_pt_swap_philox(c, round0 + (uint32_t)r, seed, n_pairs, nullptr, nullptr, nullptr);
        if (rc) return rc;
    }
    c->rounds_route = NLMC_ROUNDS_LAUNCH_PER_ROUND;
    return NLMC_OK;
}

// n_rounds rounds of a context that owns whole ladders.  Where k_rounds_fused qualifies (nlmc_pt_rounds_fused's conditions, the
// residency of all workgroups among them; NLMC_NO_PERSISTENT switches it off) the rounds run inside its launches, every swap
// included.  Otherwise n_rounds sweep launches + ONE swap launch: launch i decides the swap of round i - 1 in its prologue
// (k_sweep_fused<.., DEFER>), the last round's swap is the ordinary k_pt_swap.
int nlmc_pt_rounds_deferred(nlmc_ctx *c, int precision, int n_rounds, int sweeps_per_round, uint32_t sweep0, uint32_t round0, uint64_t seed,
                            int n_pairs)
{
    if (!c) return NLMC_ERR_ARG;
    // a short-chain route the context's sweeps are on, before any fused plan is asked for: under nlmc_set_wave_rounds the rounds inside
    // k_rounds_waves where the sweeps go to the wave kernels, then the rounds inside k_rounds_lanes where they go to the lane kernels
    if (rounds_deferred_quiet_ok(c, precision, n_rounds, sweeps_per_round, n_pairs)) {
        auto takes = [&](ShortRounds route) { return !short_rounds_refusal(c, route, precision, n_rounds, sweeps_per_round, round0, seed, n_pairs); };
        if (c->wave_rounds && waves_route(c, c->n_chains, precision)) {
            // k_rounds_waves ends at NLMC_WAVE_N spins: longer chains on the wave route (nlmc_set_wave_long) run inside
            // k_rounds_waves_long under nlmc_set_wave_long_rounds where it takes them, and otherwise a sweep call and a swap call
            // per round, the sweeps in k_sweep_waves_long
            const bool longs = c->n > NLMC_WAVE_N;
            const ShortRounds route = longs ? ShortRounds::waves_long : ShortRounds::waves;
            if ((!longs || c->wave_long_rounds) && takes(route))
                return short_rounds(c, route, precision, n_rounds, sweeps_per_round, sweep0, round0, seed, n_pairs);
            if (longs && !rounds_context_refusal(c, true))
                return rounds_waves_call_by_call(c, precision, n_rounds, sweeps_per_round, sweep0, round0, seed, n_pairs);
        }
        if (ROUNDS_LANES_IN_LAUNCH && lanes_route(c, c->n_chains) && takes(ShortRounds::lanes))
            return short_rounds(c, ShortRounds::lanes, precision, n_rounds, sweeps_per_round, sweep0, round0, seed, n_pairs);
    }
    int fslot = -1, arith = NOT_FUSED;
    { int rc = rounds_check(c, Via::deferred, precision, n_rounds, sweeps_per_round, sweep0, round0, seed, n_pairs, fslot, arith); if (rc || fslot < 0) return rc; }
    HIP_TRY(c, hipSetDevice(c->device));
    const int L = c->ladder_len, T = sweeps_per_round;
    begin_sweep_call(c);
    if (!c->knobs.no_persistent && (arith != ARITH_R64 || ROUNDS_REAL_IN_LAUNCH)) {
        bool resident = false;
        int rc = rounds_in_launch(c, fslot, arith, n_rounds, T, sweep0, round0, seed, n_pairs, resident);
        if (rc || resident) return rc;
    }
    const nlmc_ctx::FusedPlan &P = c->fz[fslot];
    const int w0 = (int)((sweep0 - P.sweep0) / (uint32_t)T), nl = c->n_chains_global / L;
    const size_t G = (size_t)c->n_chains_global;
    HIP_TRY(c, c->rounds_ebuf.reserve(2 * G));
    { int rc = upload_ladder_tab(c, c->stream); if (rc) return rc; }
    const bool log = c->pt_log.covers(round0, n_rounds, n_pairs);
    // the rounds' sweeps as one call: the ladder's temperatures by slot, no per-sweep outputs
    SweepCall s{};
    s.precision = precision; s.order_mode = NLMC_ORDER_SHARED; s.n_sweeps = n_rounds * T; s.sweep0 = sweep0; s.seed = seed;
    s.tab = c->pt_tab.p; s.tab_cs = 2; s.use_slots = true;
    for (int r = 0; r < n_rounds; ++r) {
        DeferSwap d{};
        d.ladder_len = L; d.n_ladders = nl; d.beta = c->pt_beta.p;
        d.slot_of_chain = c->slot_of_chain.p; d.chain_of_slot = c->chain_of_slot.p;
        if (r > 0) {                          // the swap of round round0 + r - 1, on the energies the previous launch published
            const uint32_t rr = round0 + (uint32_t)(r - 1);
            d.n_pairs = n_pairs; d.round = rr;
            const RoundRows rows = round_rows(c, rr, (size_t)nl, n_pairs, log);
            d.plan_pairs = rows.plan_pairs; d.log_pairs = rows.log_pairs; d.log_acc = rows.log_acc;
            d.e_prev = c->rounds_ebuf.p + (size_t)((r - 1) & 1) * G;
        }
        // (this launch publishes its chains' final energies for the next one: rows of the local chains inside the global vector)
        double *sink = c->rounds_ebuf.p + (size_t)(r & 1) * G + c->chain_base;
        int rc = run_fused(c, s, fslot, w0 + r, r * T, arith, &d, sink);
        if (rc) return rc;
        // an open record observes the round here: a swap is a label exchange, so chain c's spins and tracked energy in the state
        // arrays after this launch are the state of round r, whatever the next launch's prologue decides about its slot
        if (c->best_on) { rc = launch_best_update(c, round0 + (uint32_t)r); if (rc) return rc; }
        // the energy log likewise: this launch's prologue has applied the swap of round r - 1 to the slot maps, so slot_of_chain is
        // the slot of round r, and the label exchange the next prologue decides leaves chain c's tracked energy where it is
        if (c->elog_on) { rc = launch_elog_update(c, round0 + (uint32_t)r); if (rc) return rc; }
    }
    c->sub_dirty = true;
    c->rounds_route = NLMC_ROUNDS_LAUNCH_PER_ROUND;
    // the last round's swap: the ordinary kernel on the tracked energies
    return nlmc_pt_swap_philox(c, round0 + (uint32_t)(n_rounds - 1), seed, n_pairs, nullptr, nullptr, nullptr);
}

int nlmc_pt_rounds_route(nlmc_ctx *c) { return c ? c->rounds_route : 0; }

int nlmc_pt_log_begin(nlmc_ctx *c, uint32_t round0, int n_rounds, int n_pairs)
{
    if (!c) return NLMC_ERR_ARG;
    if (c->ladder_len == 0) return fail(c, NLMC_ERR_STATE, "nlmc_pt_log_begin: call nlmc_pt_init first");
    if (n_rounds < 0 || n_pairs < 0) return fail(c, NLMC_ERR_ARG, "nlmc_pt_log_begin: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nl = (size_t)(c->n_chains_global / c->ladder_len), tot = (size_t)n_rounds * nl * (size_t)n_pairs;
    c->pt_log.on = false;
    if (tot == 0) return NLMC_OK;
    HIP_TRY(c, c->pt_log_pairs.reserve(tot * 2));
    HIP_TRY(c, c->pt_log_acc.reserve(tot));
    HIP_TRY(c, hipMemsetAsync(c->pt_log_pairs.p, 0xFF, sizeof(int32_t) * tot * 2, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->pt_log_acc.p, 0, tot, c->stream));
    c->pt_log.on = true;
    c->pt_log.round0 = round0; c->pt_log.rounds = n_rounds; c->pt_log.npairs = n_pairs;
    return NLMC_OK;
}

int nlmc_pt_log_read(nlmc_ctx *c, int32_t *out_pairs, uint8_t *out_accepted)
{
    if (!c || !out_pairs || !out_accepted) return fail(c, NLMC_ERR_ARG, "nlmc_pt_log_read: NULL argument");
    if (!c->pt_log.on) return fail(c, NLMC_ERR_STATE, "nlmc_pt_log_read: no log was begun");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nl = (size_t)(c->n_chains_global / c->ladder_len), tot = (size_t)c->pt_log.rounds * nl * (size_t)c->pt_log.npairs;
    HIP_TRY(c, hipMemcpyAsync(out_pairs, c->pt_log_pairs.p, sizeof(int32_t) * tot * 2, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out_accepted, c->pt_log_acc.p, tot, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return nlmc_pt_check(c);
}

int nlmc_pt_check(nlmc_ctx *c)
{
    if (!c) return NLMC_ERR_ARG;
    if (c->ladder_len == 0) return NLMC_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    int32_t st = 0;
    HIP_TRY(c, hipMemcpyAsync(&st, c->pt_status.p, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (st != 0) {
        HIP_TRY(c, hipMemsetAsync(c->pt_status.p, 0, sizeof(int32_t), c->stream));
        if (st == 3) return fail(c, NLMC_ERR_HIP, "k_rounds_fused: a chain waited for its swap partner's energy in vain (timed out); the chains' states are not valid");
        return fail(c, NLMC_ERR_ARG, "Cannot find non-overlapping pairs.");
    }
    return NLMC_OK;
}

// ---------------------------------------------------------------------------------------------------
// iso-cluster move
// ---------------------------------------------------------------------------------------------------
// 16-bit neighbour table shared by k_levelize_fused and k_icm_components (built once per context)
static int ensure_adjacency(nlmc_ctx *c)
{
    if (c->fz_adj_ready) return NLMC_OK;
    HIP_TRY(c, c->fz_adj.reserve((size_t)c->n * NLMC_FZ_ADJ));
    hipLaunchKernelGGL(k_fused_adjacency, dim3((c->n + 255) / 256), dim3(256), 0, c->stream, c->n, c->rowptr.p, c->col.p, c->fz_adj.p);
    HIP_TRY(c, hipGetLastError());
    c->fz_adj_ready = true;
    return NLMC_OK;
}

static int icm_launch_components(nlmc_ctx *c, const int32_t *pairs_dev, int n_pairs)
{
    HIP_TRY(c, c->icm_label.reserve((size_t)n_pairs * c->n));
    HIP_TRY(c, c->icm_info.reserve((size_t)n_pairs * 2));
    IcmArgs a{};
    a.g = c->g; a.spins = c->spins.p; a.pairs = pairs_dev; a.label = c->icm_label.p; a.info = c->icm_info.p;
    if (c->big) {                   // the forest lives in the labels themselves (csrc/nlmc_big.h)
        hipLaunchKernelGGL(k_icm_components_big, dim3(n_pairs), dim3(1024), 0, c->stream, a);
        HIP_TRY(c, hipGetLastError());
        return NLMC_OK;
    }
    if (!c->has_zero_vals && c->n <= 65535) {
        int rc = ensure_adjacency(c);
        if (rc) return rc;
        a.adj = reinterpret_cast<const uint4 *>(c->fz_adj.p);
    }
    const size_t lds = (size_t)c->n * 4 + (((size_t)c->n + 1) & ~(size_t)1) * 2 + 16;
    { int rc = ensure_lds(c, reinterpret_cast<const void *>(k_icm_components), lds); if (rc) return rc; }
    hipLaunchKernelGGL(k_icm_components, dim3(n_pairs), dim3(c->n >= 4096 ? 1024 : 256), lds, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return NLMC_OK;
}

// components + pick + move + incremental energies of a batch of pairs in one launch (k_icm_round)
static int icm_launch_round(nlmc_ctx *c, const int32_t *pairs_dev, int n_pairs, uint32_t round, uint64_t seed, int katz,
                            int pair_R = 0, int pair_K = 0)
{
    HIP_TRY(c, c->icm_info.reserve((size_t)n_pairs * 2));
    IcmRoundArgs a{};
    a.g = c->g; a.spins = c->spins.p; a.pairs = pairs_dev; a.info = c->icm_info.p;
    a.pair_R = pair_R; a.pair_K = pair_K; a.chain_of_slot = c->chain_of_slot.p;
    a.slot0 = c->rng_base; a.rng_stride = c->rng_stride; a.rng_base = c->rng_base;
    if (!c->has_zero_vals && c->n <= 65535) {
        int rc = ensure_adjacency(c);
        if (rc) return rc;
        a.adj = reinterpret_cast<const uint4 *>(c->fz_adj.p);
    }
    a.round = round; a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.katz = katz; a.chain_base = c->chain_base;
    a.efix = c->efix.p; a.energy_sink = c->energy_sink; a.eshift = c->escale - c->qs; a.escale = c->escale;
    // k_icm_round keeps labels, candidates and both states in LDS: 8 bytes a spin, which the workgroup's LDS holds up to n =
    // 20 220 only.  Chains from there to NLMC_LDS_N take the global-memory kernel (same pairing keys, same pick, same integers).
    size_t cur = (size_t)c->n * 4;
    a.lds_cand_off = (int)cur; cur += (((size_t)c->n + 7) & ~(size_t)7) * 2;
    cur = (cur + 15) & ~(size_t)15;
    a.lds_sa_off = (int)cur; cur += (size_t)c->n_pad;
    a.lds_sb_off = (int)cur; cur += (size_t)c->n_pad;
    const size_t lds = cur + 16;
    if (c->big || lds > NLMC_LDS_BYTES_MAX) {
        if (!pairs_dev && pair_K > 1024) return fail(c, NLMC_ERR_UNSUPPORTED, "icm: more sub-replicas than threads of a workgroup");
        HIP_TRY(c, c->icm_label.reserve((size_t)n_pairs * c->n));
        a.adj = nullptr;
        hipLaunchKernelGGL(k_icm_round_big, dim3(n_pairs), dim3(1024), 0, c->stream, a, c->icm_label.p);
        HIP_TRY(c, hipGetLastError());
        return NLMC_OK;
    }
    { int rc = ensure_lds(c, reinterpret_cast<const void *>(k_icm_round), lds); if (rc) return rc; }
    hipLaunchKernelGGL(k_icm_round, dim3(n_pairs), dim3(c->n >= 4096 ? 1024 : 256), lds, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return NLMC_OK;
}

static int icm_check_pair(nlmc_ctx *c, int a, int b)
{
    if (a < 0 || b < 0 || a >= c->n_chains || b >= c->n_chains || a == b) return fail(c, NLMC_ERR_ARG, "icm: bad chain pair");
    return NLMC_OK;
}

int nlmc_icm_components(nlmc_ctx *c, int chain_a, int chain_b, int32_t *out_n_components)
{
    if (!c || !out_n_components) return fail(c, NLMC_ERR_ARG, "nlmc_icm_components: NULL argument");
    int rc = icm_check_pair(c, chain_a, chain_b);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->icm_pairs.reserve(2));
    const int32_t pr[2] = {chain_a, chain_b};
    HIP_TRY(c, hipMemcpyAsync(c->icm_pairs.p, pr, sizeof(pr), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    rc = icm_launch_components(c, c->icm_pairs.p, 1);
    if (rc) return rc;
    int32_t info[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(info, c->icm_info.p, sizeof(info), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (info[0] < 0) return fail(c, NLMC_ERR_STATE, "icm: the component search did not converge");
    *out_n_components = info[0];
    return NLMC_OK;
}

int nlmc_icm_get_labels(nlmc_ctx *c, int32_t *out)
{
    if (!c || !out) return fail(c, NLMC_ERR_ARG, "nlmc_icm_get_labels: NULL argument");
    if (c->icm_label.cap < (size_t)c->n) return fail(c, NLMC_ERR_STATE, "nlmc_icm_get_labels: no component search has run yet");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out, c->icm_label.p, sizeof(int32_t) * (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < c->n; ++k) if (out[k] == INT_MAX) out[k] = -1;
    return NLMC_OK;
}

static int icm_apply(nlmc_ctx *c, int n_pairs, const int64_t *pick_dev_or_null, int64_t pick_host, uint32_t round,
                     uint64_t seed, int katz, int philox)
{
    IcmMoveArgs m{};
    m.g = c->g; m.spins = c->spins.p; m.pairs = c->icm_pairs.p; m.label = c->icm_label.p; m.info = c->icm_info.p;
    m.pick_host = pick_host; m.use_philox = philox; m.round = round;
    m.seed_lo = (uint32_t)seed; m.seed_hi = (uint32_t)(seed >> 32); m.katz = katz; m.chain_base = c->chain_base;
    (void)pick_dev_or_null;
    hipLaunchKernelGGL(k_icm_move, dim3(n_pairs), dim3(c->n >= 4096 ? 1024 : 256), 0, c->stream, m);
    HIP_TRY(c, hipGetLastError());
    return NLMC_OK;
}

int nlmc_icm_move(nlmc_ctx *c, int chain_a, int chain_b, int64_t pick_index, int katzgraber, int32_t *out_info)
{
    if (!c) return NLMC_ERR_ARG;
    int rc = icm_check_pair(c, chain_a, chain_b);
    if (rc) return rc;
    if (pick_index < 0) return fail(c, NLMC_ERR_ARG, "nlmc_icm_move: pick_index < 0");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->icm_pairs.reserve(2));
    const int32_t pr[2] = {chain_a, chain_b};
    HIP_TRY(c, hipMemcpyAsync(c->icm_pairs.p, pr, sizeof(pr), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    rc = icm_launch_components(c, c->icm_pairs.p, 1);
    if (rc) return rc;
    rc = icm_apply(c, 1, nullptr, pick_index, 0, 0, katzgraber, 0);
    if (rc) return rc;
    rc = launch_energy_self(c, nullptr);   // states changed non-incrementally: resync tracked energies
    if (rc) return rc;
    int32_t info[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(info, c->icm_info.p, sizeof(info), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (info[0] < 0) return fail(c, NLMC_ERR_STATE, "icm: the component search did not converge");
    if (out_info) { out_info[0] = info[0]; out_info[1] = info[1]; }
    return NLMC_OK;
}

int nlmc_icm_round_philox(nlmc_ctx *c, const int32_t *pairs, int n_pairs, uint32_t round, uint64_t seed, int katzgraber,
                          int32_t *out_info)
{
    if (!c || (n_pairs > 0 && !pairs) || n_pairs < 0) return fail(c, NLMC_ERR_ARG, "nlmc_icm_round_philox: bad argument");
    if (n_pairs == 0) return NLMC_OK;
    std::vector<uint8_t> used((size_t)c->n_chains, 0);
    for (int p = 0; p < n_pairs; ++p) {
        int rc = icm_check_pair(c, pairs[2 * p], pairs[2 * p + 1]);
        if (rc) return rc;
        if (used[pairs[2 * p]] || used[pairs[2 * p + 1]]) return fail(c, NLMC_ERR_ARG, "nlmc_icm_round_philox: a chain appears in two pairs");
        used[pairs[2 * p]] = used[pairs[2 * p + 1]] = 1;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->icm_pairs.reserve((size_t)n_pairs * 2));
    HIP_TRY(c, hipMemcpyAsync(c->icm_pairs.p, pairs, sizeof(int32_t) * 2 * n_pairs, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // the tracked energies must be the energies of the current states in the fixed-point model: true after sweeps and
    // moves of this kind; a caller that overwrote the states gets them re-synchronised by nlmc_set_spins / nlmc_energy
    int rc = icm_launch_round(c, c->icm_pairs.p, n_pairs, round, seed, katzgraber);
    if (rc) return rc;
    if (out_info) {
        HIP_TRY(c, hipMemcpyAsync(out_info, c->icm_info.p, sizeof(int32_t) * 2 * n_pairs, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (int p = 0; p < n_pairs; ++p)
            if (out_info[2 * p] < 0) return fail(c, NLMC_ERR_STATE, "icm: the component search did not converge");
    }
    return NLMC_OK;
}

int nlmc_icm_round_ladders(nlmc_ctx *c, uint32_t round, uint64_t seed, int katzgraber, int32_t *out_n_pairs,
                           int32_t *out_info)
{
    if (!c) return NLMC_ERR_ARG;
    if (c->ladder_len == 0) return fail(c, NLMC_ERR_STATE, "nlmc_icm_round_ladders: nlmc_pt_init first");
    if (c->chain_base != 0 || c->n_chains != c->n_chains_global)
        return fail(c, NLMC_ERR_UNSUPPORTED, "nlmc_icm_round_ladders: the sub-replicas of a temperature must live in one context");
    const int R = c->ladder_len, M = c->apt_systems, K = c->n_chains_global / R / M, n_pairs = M * R * (K / 2);   // K ladders a system
    if (out_n_pairs) *out_n_pairs = n_pairs;
    if (n_pairs == 0) return NLMC_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const int nt_round = c->n >= 4096 ? 1024 : 256;
    const bool pair_in_kernel = K <= nt_round;          // the pairing (a sort of K Philox keys per slot) is made by the move kernel itself
    if (!pair_in_kernel && c->rng_stride) return fail(c, NLMC_ERR_UNSUPPORTED, "nlmc_icm_round_ladders: more sub-replicas than threads with slot-keyed random numbers");
    if (!pair_in_kernel) {
        HIP_TRY(c, c->icm_pairs.reserve((size_t)n_pairs * 2));
        hipLaunchKernelGGL(k_icm_pair_ladders, dim3((M * R * K + 63) / 64), dim3(64), 0, c->stream, M, R, K, round, (uint32_t)seed,
                           (uint32_t)(seed >> 32), c->chain_of_slot.p, c->icm_pairs.p);
        HIP_TRY(c, hipGetLastError());
    }
    // one launch: components, pick, move, incremental fixed-point energies (k_icm_round; round 2's separate row walk of the
    // cluster ran one thread per cluster spin from a cold kernel: 41 us -- inside the components workgroup, with both
    // states in LDS, it is a few us)
    int rc = icm_launch_round(c, pair_in_kernel ? nullptr : c->icm_pairs.p, n_pairs, round, seed, katzgraber, R, K);
    if (rc) return rc;
    if (out_info) {
        HIP_TRY(c, hipMemcpyAsync(out_info, c->icm_info.p, sizeof(int32_t) * 2 * n_pairs, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (int p = 0; p < n_pairs; ++p)
            if (out_info[2 * p] < 0) return fail(c, NLMC_ERR_STATE, "icm: the component search did not converge");
    }
    return NLMC_OK;
}

// ---- APT rounds of short chains: one system per workgroup, a workgroup per system (k_apt_rounds_lanes, csrc/nlmc_lane_apt.h) --------
// LDS of k_apt_rounds_lanes for W waves: spins of every wave | slot maps | pair_col | energy deltas | labels, sharing their bytes with
// the waves' random-number tables where those fit too.  ok = false: the carve-up without the tables exceeds NLMC_APT_LANES_LDS.
constexpr size_t NLMC_APT_LANES_LDS = (size_t)150 * 1024;
struct AptLanesLds { size_t wave, map_off, pcol_off, de_off, u_off, tab_wave, total; int lab_stride; bool tab, ok; };
static AptLanesLds apt_lanes_lds(const nlmc_ctx *c, int K, int L, int W)
{
    AptLanesLds A{};
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    A.wave = (size_t)c->n_pad * NLMC_LANE_STRIDE;
    A.map_off = A.wave * (size_t)W;
    A.pcol_off = A.map_off + (size_t)W * 128;
    A.de_off = up16(A.pcol_off + (size_t)L * K * sizeof(uint16_t));
    A.u_off = up16(A.de_off + (size_t)W * 64 * sizeof(long long));
    A.lab_stride = (L * (K / 2) + 1) & ~1;
    const size_t labels = (size_t)c->n * (size_t)A.lab_stride * sizeof(uint16_t);
    A.tab_wave = (size_t)((c->n + 3) / 4 * 4) * 256;
    A.ok = A.u_off + labels <= NLMC_APT_LANES_LDS;
    A.tab = A.ok && c->knobs.lane_rng != 0 && A.u_off + A.tab_wave * (size_t)W <= NLMC_APT_LANES_LDS;
    A.total = A.u_off + std::max(labels, A.tab ? A.tab_wave * (size_t)W : (size_t)0);
    return A;
}

int nlmc_apt_rounds_lanes(nlmc_ctx *c, int precision, int n_rounds, int sweeps_per_round, uint32_t sweep0, uint32_t round0, uint64_t seed,
                          int n_pairs, int katzgraber, int32_t *out_info)
{
    if (!c) return NLMC_ERR_ARG;
    const std::string name = "nlmc_apt_rounds_lanes: ";
    const int T = sweeps_per_round;
    bool go = false;
    { int rc = rounds_entry_check(c, name, precision, n_rounds, T, n_pairs, go); if (rc || !go) return rc; }
    if (n_pairs > std::max(0, c->ladder_len - 1)) return fail(c, NLMC_ERR_ARG, "Cannot find non-overlapping pairs.");
    auto no = [&](const char *why) { return fail(c, NLMC_ERR_UNSUPPORTED, name + why); };
    if (c->best_on) return no("a best-state record is open: k_apt_rounds_lanes keeps none (run the round step by step with nlmc_best_update)");
    if (c->chain_base != 0 || c->n_chains != c->n_chains_global) return no("the sub-replicas of a temperature must live in one context");
    if (c->rng_stride != 0) return no("random numbers keyed by temperature slot (nlmc_apt_shard) keep the round-by-round route");
    if (const char *why = short_rounds_refusal(c, ShortRounds::apt_lanes, precision, n_rounds, T, round0, seed, n_pairs)) return no(why);
    // (M systems, nlmc_apt_systems: a workgroup each; K, W, NP and the LDS carve-up are those of ONE system)
    const int L = c->ladder_len, M = c->apt_systems, K = c->n_chains_global / L / M, P = 64 / L, W = (K + P - 1) / P, NP = L * (K / 2);
    if (W > 16) return no("the system needs more than 16 waves: it does not fit one workgroup");
    const AptLanesLds A = apt_lanes_lds(c, K, L, W);
    if (!A.ok) return no("the system's chains and labels exceed one workgroup's LDS (150 KB)");
    HIP_TRY(c, hipSetDevice(c->device));

    const bool want_info = out_info && NP > 0;
    if (want_info) HIP_TRY(c, c->icm_info.reserve((size_t)n_rounds * M * NP * 2));
    const bool elog = c->elog_rec(round0, n_rounds).energy != nullptr;          // (a launch none of whose rounds is logged stores nothing anyway)
    const void *kfun = apt_lanes_kernel(precision == NLMC_F64, elog);
    const bool log = n_pairs > 0 && c->pt_log.covers(round0, n_rounds, n_pairs);
    int rc = lane_rounds_chunks(c, kfun, A.total, n_rounds, T, sweep0, round0, seed, NLMC_ROUTE_LANES, [&](int at, int k, uint32_t s0, uint32_t r0) -> int {
        LaneLaunchArgs la = lane_launch_args(c, T, seed, s0, k, r0, n_pairs, (size_t)M * K, log, A.tab, A.u_off, A.map_off);   // (plan and log rows hold every ladder of the context)
        LaneAptArgs x{};
        x.n_sub = K; x.n_icm = NP; x.katz = katzgraber ? 1 : 0;
        x.info = want_info ? c->icm_info.p + (size_t)at * M * NP * 2 : nullptr;
        x.lds_wave_bytes = (int)A.wave; x.lds_tab_bytes = (int)A.tab_wave; x.lds_pcol_off = (int)A.pcol_off; x.lds_de_off = (int)A.de_off;
        x.lds_lab_off = (int)A.u_off; x.lab_stride = A.lab_stride;
        void *kargs[] = {&la.a, &la.q, &x};
        HIP_TRY(c, hipLaunchKernel(kfun, dim3((unsigned)M), dim3((unsigned)(64 * W)), kargs, A.total, c->stream));
        return NLMC_OK;
    });
    if (rc) return rc;
    c->rounds_route = NLMC_ROUNDS_APT_LANES;
    if (want_info) {
        const size_t cnt = (size_t)n_rounds * M * NP * 2;
        HIP_TRY(c, hipMemcpyAsync(out_info, c->icm_info.p, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (size_t p = 0; p < cnt; p += 2)
            if (out_info[p] < 0) return fail(c, NLMC_ERR_STATE, "icm: the component search did not converge");
    }
    return NLMC_OK;
}

// ---- NMC phase cycles in one launch: a chain per lane (k_nmc_phases_lanes, csrc/nlmc_lane_nmc.h), a chain per wave (k_nmc_phases_waves,
// csrc/nlmc_wave_nmc.h) and a chain of NLMC_WAVE_N < n <= NLMC_WAVE_LONG_N spins per wave (k_nmc_phases_waves_long, csrc/nlmc_wave_long_nmc.h)
enum class NmcRoute { lanes, waves, waves_long };

// The reach of a route's kernel: the test knob that switches it off (read at nlmc_create) and what it says, the chain lengths it takes,
// whether it has the fixed-point arithmetic only, and what a chain beyond it is told.  Rows in the order of NmcRoute.
struct NmcReach { bool Knobs::*off; const char *why_off; int n_min, n_max; bool f32_only; const char *why_n; };
static NmcReach nmc_reach(NmcRoute route)
{
    static const NmcReach reach[] = {
        {&Knobs::no_lane_nmc, "switched off (NLMC_NO_LANE_NMC)", 0, NLMC_LANE_N, false,
         "the chain-per-lane kernels take chains of at most NLMC_LANE_N spins, resident in LDS"},
        {&Knobs::no_wave_nmc, "switched off (NLMC_NO_WAVE_NMC)", 0, NLMC_WAVE_N, true,
         "the wave-per-chain phase kernel takes chains of at most NLMC_WAVE_N spins"},
        {&Knobs::no_wave_long_nmc, "switched off (NLMC_NO_WAVE_LONG_NMC)", NLMC_WAVE_N + 1, NLMC_WAVE_LONG_N, true,
         "the long wave-per-chain phase kernel takes chains of NLMC_WAVE_N + 1 to NLMC_WAVE_LONG_N spins"}};
    return reach[(int)route];
}

// LDS of k_nmc_phases_lanes: transposed spins | transposed backbone mask | (where it fits) a transposed best-state plane | (where it
// fits) one sweep's random numbers.  The table under lane_lds' rule -- four waves still share a compute unit, 40 KB per wave -- and the
// best-state plane where that still holds beside the rest; best_off = 0: the best state stays in global memory.
struct LaneNmcLds { size_t mask_off, best_off, u_off, total; bool tab, ok; };
static LaneNmcLds lane_nmc_lds(const nlmc_ctx *c)
{
    LaneNmcLds L{};
    const size_t plane = (size_t)c->n_pad * NLMC_LANE_STRIDE, tab = (size_t)((c->n + 3) / 4 * 4) * 256, share = (size_t)40 * 1024;
    size_t state = 2 * plane;
    L.mask_off = plane;
    L.ok = state <= NLMC_LDS_BYTES_MAX;
    L.tab = c->knobs.lane_rng != 0 && state + tab <= share;
    if (state + plane + (L.tab ? tab : 0) <= share) { L.best_off = state; state += plane; }
    L.u_off = state;
    L.total = state + (L.tab ? tab : 0);
    return L;
}

// Why this context cannot run NMC phases of S sweeps inside the kernel of `route`, or nullptr.  (The entry points have the shared visiting
// order only: a per-chain order cannot be asked for.)  They are reached by name: nlmc_set_lane_sweeps, nlmc_set_wave_sweeps and
// nlmc_set_wave_long are not looked at, and chains of more than NLMC_WAVE_N spins are refused by `waves` under nlmc_set_wave_long too.
// Arguments and call order are checked by the caller.
static const char *nmc_refusal(const nlmc_ctx *c, NmcRoute route, int S, int precision)
{
    const NmcReach reach = nmc_reach(route);
    if (c->knobs.*reach.off) return reach.why_off;
    if (c->knobs.force_big || c->big || c->n < reach.n_min || c->n > reach.n_max) return reach.why_n;
    if (reach.f32_only && precision != NLMC_F32) return "the wave-per-chain kernels keep exact fixed-point fields: f32 only";
    if (c->rng_stride != 0) return "random numbers keyed by temperature slot (nlmc_apt_shard) keep the phase-by-phase route";
    if ((size_t)S * (size_t)c->n * sizeof(uint16_t) > c->knobs.lane_scratch)
        return "the visiting orders of one phase exceed the order scratch (NLMC_LANE_SCRATCH)";
    if (route == NmcRoute::lanes && !lane_nmc_lds(c).ok) return "spins and backbone mask exceed one workgroup's LDS";
    if (route == NmcRoute::waves_long && nlmc_wave_long_nmc_shape(c->n, c->n_pad, 1, 1, 0).R == 0)
        return "the padded chain does not fit a row of the wave kernels' matrix";
    return nullptr;
}

// What a route supplies to nmc_phases_by_name: its kernel with dynamic LDS, grid and block (LDS limit raised, whatever the kernel reads once
// per context in place), the SweepArgs / NmcPhasesArgs fields of its own -- lanes: the LDS carve-up (lane_nmc_lds); waves: the dense
// matrix -- and the NLMC_ROUTE_* it reports.
struct NmcLaunch { const void *kfun; size_t lds; dim3 grid, block; bool tab; size_t u_off, mask_off, best_off; const int32_t *wave_J; int route; };

// k_nmc_phases_lanes: a chain per lane, 64 to a workgroup of one wave
static int lanes_nmc(nlmc_ctx *c, int precision, NmcLaunch &r)
{
    const LaneNmcLds L = lane_nmc_lds(c);
    r.kfun = precision == NLMC_F64 ? reinterpret_cast<const void *>(k_nmc_phases_lanes<true>) : reinterpret_cast<const void *>(k_nmc_phases_lanes<false>);
    r.lds = L.total; r.grid = dim3((unsigned)((c->sub_count() + 63) / 64)); r.block = dim3(64);
    r.tab = L.tab; r.u_off = L.u_off; r.mask_off = L.mask_off; r.best_off = L.best_off;
    r.route = NLMC_ROUTE_LANES;
    return ensure_lds(c, r.kfun, r.lds);
}

// k_nmc_phases_waves<R, jlds> for R <= 4: a chain per wave in k_sweep_waves' shape (nlmc_wave_shape); k_nmc_phases_waves_long<R, ahead>
// beyond (`longs`): k_sweep_waves_long's shape with the larger regions (nlmc_wave_long_nmc_shape), NLMC_WAVE_LONG_AHEAD picks as for the sweeps
static int waves_nmc(nlmc_ctx *c, bool longs, NmcLaunch &r)
{
#define NLMC_NW(K_, R_) {reinterpret_cast<const void *>(K_<R_, false>), reinterpret_cast<const void *>(K_<R_, true>)}
    static const void *const table[5][2] = {NLMC_NW(k_nmc_phases_waves, 1), NLMC_NW(k_nmc_phases_waves, 2), NLMC_NW(k_nmc_phases_waves, 4),
                                            NLMC_NW(k_nmc_phases_waves_long, 8), NLMC_NW(k_nmc_phases_waves_long, 16)};
#undef NLMC_NW
    { int rc = cu_count(c); if (rc) return rc; }
    const NlmcWaveShape S = longs ? nlmc_wave_long_nmc_shape(c->n, c->n_pad, c->sub_count(), c->n_cu, c->knobs.wave_waves)
                                  : nlmc_wave_shape(c->n, c->n_pad, c->sub_count(), c->n_cu, c->knobs.wave_waves, c->knobs.wave_jlds ? 1 : 0);
    if ((longs ? S.R != 8 && S.R != 16 : S.R == 0 || S.R > 4) || c->n_pad > 64 * S.R)
        return fail(c, NLMC_ERR_STATE, longs ? "waves_long_nmc: the chain does not fit the wave kernels" : "waves_nmc: the chain does not fit the wave kernels");
    r.kfun = table[wave_fields_row(S.R)][(longs ? c->knobs.wave_long_ahead : S.jlds) ? 1 : 0];
    r.lds = S.lds; r.grid = dim3((unsigned)S.blocks); r.block = dim3((unsigned)(64 * S.W));
    r.route = NLMC_ROUTE_WAVES;
    { int rc = ensure_lds(c, r.kfun, r.lds); if (rc) return rc; }
    { int rc = ensure_wave_matrix(c, S.stride); if (rc) return rc; }
    r.wave_J = c->wave_J.p;
    return NLMC_OK;
}

// nlmc_nmc_phases_lanes / nlmc_nmc_phases_waves / nlmc_nmc_phases_waves_long (`fn`), whatever the lane or wave mode is: the checks
// (nmc_refusal last), launches of as many whole phases as the order scratch holds visiting orders for (and the kernel arguments hold kinds
// for) -- k_lane_orders into nmc_perm, then the route's kernel -- and the optional read-backs.
static int nmc_phases_by_name(nlmc_ctx *c, NmcRoute route, const char *fn, int precision, const int32_t *kinds, int n_phases,
                              int sweeps_per_phase, uint32_t sweep0, uint64_t seed, double beta, double temp_x, int min_stride,
                              int64_t *out_phase_min, int32_t *out_phase_argmin, int8_t *out_last_best)
{
    if (!c) return NLMC_ERR_ARG;
    const std::string name = std::string(fn) + ": ";
    const int P = n_phases, S = sweeps_per_phase;
    if ((precision != NLMC_F32 && precision != NLMC_F64) || !kinds || P < 1 || S < 1 || min_stride < 1 || (long long)P * S > (long long)(INT_MAX / 2))
        return fail(c, NLMC_ERR_ARG, name + "bad argument");
    for (int p = 0; p < P; ++p)
        if (kinds[p] < NLMC_PHASE_ALL || kinds[p] > NLMC_PHASE_BACKBONE_FROZEN) return fail(c, NLMC_ERR_ARG, name + "bad phase");
    if (!(temp_x > 0.0) && !(temp_x < 0.0)) return fail(c, NLMC_ERR_ARG, name + "temp_x must be non-zero");
    if (!c->cmask.p) return fail(c, NLMC_ERR_STATE, name + "no backbone inference has run");
    if (c->track_min) return fail(c, NLMC_ERR_STATE, name + "a tracked minimum is open (nlmc_track_minimum): the call keeps its own");
    if (const char *why = nmc_refusal(c, route, S, precision)) return fail(c, NLMC_ERR_UNSUPPORTED, name + why);
    HIP_TRY(c, hipSetDevice(c->device));
    const int R = c->sub_count(), n = c->n;
    if (R == 0) return NLMC_OK;
    { int rc = ensure_subset(c); if (rc) return rc; }
    NmcLaunch r{};
    { int rc = route == NmcRoute::lanes ? lanes_nmc(c, precision, r) : waves_nmc(c, route == NmcRoute::waves_long, r); if (rc) return rc; }
    const size_t bytes_per_phase = (size_t)S * (size_t)n * sizeof(uint16_t);
    const int K = (int)std::max<size_t>(1, std::min<size_t>({(size_t)P, c->knobs.lane_scratch / bytes_per_phase, (size_t)NLMC_NMC_PHASES_LAUNCH}));
    begin_sweep_call(c);
    c->stat_orders = 0; c->stat_levels = 0; c->stats_pending = false;
    c->stat_fused_window = -1;
    c->stat_lane_orders = 0;
    c->strace_nrec = 0; c->strace_rows = 0;
    HIP_TRY(c, c->nmc_perm.reserve((size_t)K * (size_t)S * (size_t)n));
    const bool want_min = out_phase_min || out_phase_argmin;
    if (want_min) {
        HIP_TRY(c, c->nmc_pmin.reserve((size_t)R * P));
        HIP_TRY(c, c->nmc_pargmin.reserve((size_t)R * P));
    }
    for (int at = 0; at < P; at += K) {
        const int k = std::min(K, P - at);
        const uint32_t s0 = sweep0 + (uint32_t)at * (uint32_t)S;
        TimerSpan ts;
        if (c->ev_accumulate) { int rc = span_begin(c, ts, 0, c->cur); if (rc) return rc; }
        { int rc = launch_lane_orders(c, c->cur, (size_t)k * S, k * S, 0, s0, seed, c->nmc_perm.p); if (rc) return rc; }
        { int rc = span_mid(c, ts); if (rc) return rc; }
        SweepArgs a = sweep_args(c, s0, S, seed, nullptr, 0, 0, false);
        lane_fields(c, a, R, r.tab, r.u_off);
        a.flags = nullptr; a.lane_perm = c->nmc_perm.p; a.min_stride = min_stride;
        a.emin = c->emin.p; a.best = c->best.p;
        a.wave_J = r.wave_J;
        NmcPhasesArgs q{};
        q.n_phases = k; q.phase0 = at; q.phases_total = P;
        for (int p = 0; p < k; ++p) q.kinds[p >> 4] |= (uint32_t)kinds[at + p] << (2 * (p & 15));
        q.cb0 = -2.0 * LOG2E * beta; q.cb1 = -2.0 * LOG2E * (beta / temp_x);
        q.mask = c->cmask.p;
        q.phase_min = want_min ? c->nmc_pmin.p : nullptr; q.phase_argmin = want_min ? c->nmc_pargmin.p : nullptr;
        q.lds_mask_off = (int)r.mask_off; q.lds_best_off = (int)r.best_off;
        void *kargs[] = {&a, &q};
        HIP_TRY(c, hipLaunchKernel(r.kfun, r.grid, r.block, kargs, r.lds, c->cur));
        HIP_TRY(c, hipGetLastError());
        { int rc = span_end(c, ts); if (rc) return rc; }
        count_launches(c, k, c->ev_accumulate);
    }
    c->last_route = r.route;
    if (!want_min && !out_last_best) return NLMC_OK;

    // the optional read-backs: rows of the subset (the best states live in per-chain rows: gathered through the chain list)
    std::vector<int32_t> h_list;
    if (out_phase_min) HIP_TRY(c, hipMemcpyAsync(out_phase_min, c->nmc_pmin.p, sizeof(long long) * (size_t)R * P, hipMemcpyDeviceToHost, c->cur));
    if (out_phase_argmin) HIP_TRY(c, hipMemcpyAsync(out_phase_argmin, c->nmc_pargmin.p, sizeof(int32_t) * (size_t)R * P, hipMemcpyDeviceToHost, c->cur));
    if (out_last_best) {
        if (c->subset != 0) {
            h_list.resize((size_t)R);
            HIP_TRY(c, hipMemcpyAsync(h_list.data(), c->sub_list(), sizeof(int32_t) * (size_t)R, hipMemcpyDeviceToHost, c->cur));
        }
        int rc = rows_to_host_begin(c, c->best.p, c->n_chains);
        if (rc) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->cur));
    if (out_last_best)
        for (int i = 0; i < R; ++i)
            std::memcpy(out_last_best + (size_t)i * n, c->stage_out.data() + (size_t)(c->subset != 0 ? h_list[(size_t)i] : i) * c->n_pad, (size_t)n);
    return NLMC_OK;
}

int nlmc_nmc_phases_lanes(nlmc_ctx *c, int precision, const int32_t *kinds, int n_phases, int sweeps_per_phase, uint32_t sweep0, uint64_t seed,
                          double beta, double temp_x, int min_stride, int64_t *out_phase_min, int32_t *out_phase_argmin, int8_t *out_last_best)
{
    return nmc_phases_by_name(c, NmcRoute::lanes, "nlmc_nmc_phases_lanes", precision, kinds, n_phases, sweeps_per_phase, sweep0, seed, beta, temp_x,
                              min_stride, out_phase_min, out_phase_argmin, out_last_best);
}

int nlmc_nmc_phases_waves(nlmc_ctx *c, int precision, const int32_t *kinds, int n_phases, int sweeps_per_phase, uint32_t sweep0, uint64_t seed,
                          double beta, double temp_x, int min_stride, int64_t *out_phase_min, int32_t *out_phase_argmin, int8_t *out_last_best)
{
    return nmc_phases_by_name(c, NmcRoute::waves, "nlmc_nmc_phases_waves", precision, kinds, n_phases, sweeps_per_phase, sweep0, seed, beta, temp_x,
                              min_stride, out_phase_min, out_phase_argmin, out_last_best);
}

int nlmc_nmc_phases_waves_long(nlmc_ctx *c, int precision, const int32_t *kinds, int n_phases, int sweeps_per_phase, uint32_t sweep0, uint64_t seed,
                               double beta, double temp_x, int min_stride, int64_t *out_phase_min, int32_t *out_phase_argmin, int8_t *out_last_best)
{
    return nmc_phases_by_name(c, NmcRoute::waves_long, "nlmc_nmc_phases_waves_long", precision, kinds, n_phases, sweeps_per_phase, sweep0, seed, beta, temp_x,
                              min_stride, out_phase_min, out_phase_argmin, out_last_best);
}

// Why f32 phases of sweeps_per_phase sweeps would be refused on `route`, or nullptr
static const char *nmc_why_not(const nlmc_ctx *c, NmcRoute route, int sweeps_per_phase)
{
    return c ? nmc_refusal(c, route, std::max(1, sweeps_per_phase), NLMC_F32) : "no context";
}

const char *nlmc_nmc_phases_lanes_refusal(const nlmc_ctx *c, int sweeps_per_phase) { return nmc_why_not(c, NmcRoute::lanes, sweeps_per_phase); }
const char *nlmc_nmc_phases_waves_refusal(const nlmc_ctx *c, int sweeps_per_phase) { return nmc_why_not(c, NmcRoute::waves, sweeps_per_phase); }
const char *nlmc_nmc_phases_waves_long_refusal(const nlmc_ctx *c, int sweeps_per_phase) { return nmc_why_not(c, NmcRoute::waves_long, sweeps_per_phase); }

// ------------------------------------------------------------------------------------------------------
// convexified loopy belief propagation (backbone inference), batched over problems
// ------------------------------------------------------------------------------------------------------
// graph, buffers, constants of a batch of n_problems inferences; seeds (lbp_ms) are the caller's business
static int lbp_setup(nlmc_ctx *c, int n_problems, const double *epsilon, const double *lambdas, int n_lambdas, double beta,
                     bool want_all)
{
    if (c->nnz > (int64_t)INT_MAX / 2) return fail(c, NLMC_ERR_UNSUPPORTED, "nlmc_lbp_convexified: nnz too large");
    const int n = c->n, nnz = (int)c->nnz;
    const size_t P = (size_t)n_problems, E = (size_t)std::max(nnz, 1);
    if (!c->lbp_graph_ready) {
        HIP_TRY(c, c->lbp_src.reserve(E));
        HIP_TRY(c, c->lbp_rev.reserve(E));
        HIP_TRY(c, c->lbp_flag.reserve(1));
        HIP_TRY(c, hipMemsetAsync(c->lbp_flag.p, 0, sizeof(int32_t), c->cur));
        hipLaunchKernelGGL(k_lbp_src, dim3((n + 255) / 256), dim3(256), 0, c->cur, n, c->rowptr.p, c->lbp_src.p);
        HIP_TRY(c, hipGetLastError());
        if (nnz > 0) {
            hipLaunchKernelGGL(k_lbp_rev, dim3((nnz + 255) / 256), dim3(256), 0, c->cur, nnz, c->rowptr.p, c->col.p,
                               c->lbp_src.p, c->lbp_rev.p, c->lbp_flag.p);
            HIP_TRY(c, hipGetLastError());
        }
        int32_t flag = 0;
        HIP_TRY(c, hipMemcpyAsync(&flag, c->lbp_flag.p, sizeof(flag), hipMemcpyDeviceToHost, c->cur));
        HIP_TRY(c, hipStreamSynchronize(c->cur));
        if (flag) return fail(c, NLMC_ERR_ARG, "LBP needs a structurally symmetric J");
        c->lbp_graph_ready = true;
    }
    HIP_TRY(c, c->lbp_tJ.reserve(E));
    HIP_TRY(c, c->lbp_eps.reserve((size_t)n));
    HIP_TRY(c, c->lbp_ms.reserve(P * n));
    HIP_TRY(c, c->lbp_lams.reserve((size_t)n_lambdas));
    HIP_TRY(c, c->lbp_w0.reserve(P * E));
    HIP_TRY(c, c->lbp_w1.reserve(P * E));
    HIP_TRY(c, c->lbp_hm.reserve(P * E));
    HIP_TRY(c, c->lbp_tot.reserve(P * n));
    HIP_TRY(c, c->lbp_mag.reserve(P * n));
    HIP_TRY(c, c->lbp_out_i.reserve(P * (2 + (size_t)n_lambdas)));
    if (want_all) HIP_TRY(c, c->lbp_mag_all.reserve(P * (size_t)n_lambdas * n));
    // constants of the run: uploaded when they change only (a replica-exchange run infers backbones once per round with the
    // same epsilon, lambda list and beta: no host synchronisation on that path)
    const std::vector<double> eps_h(epsilon, epsilon + n), lam_h(lambdas, lambdas + n_lambdas);
    if (eps_h != c->lbp_eps_host || lam_h != c->lbp_lams_host) {
        HIP_TRY(c, hipStreamSynchronize(c->cur));
        HIP_TRY(c, hipMemcpyAsync(c->lbp_eps.p, eps_h.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->cur));
        HIP_TRY(c, hipMemcpyAsync(c->lbp_lams.p, lam_h.data(), sizeof(double) * n_lambdas, hipMemcpyHostToDevice, c->cur));
        HIP_TRY(c, hipStreamSynchronize(c->cur));
        c->lbp_eps_host = eps_h;
        c->lbp_lams_host = lam_h;
    }
    if (nnz > 0 && (!c->lbp_tJ_valid || c->lbp_tJ_beta != beta)) {
        hipLaunchKernelGGL(k_lbp_tanhJ, dim3((nnz + 255) / 256), dim3(256), 0, c->cur, nnz, c->val64.p, beta, c->lbp_tJ.p);
        HIP_TRY(c, hipGetLastError());
        c->lbp_tJ_valid = true;
        c->lbp_tJ_beta = beta;
    }
    return NLMC_OK;
}

// the batched lambda loop on the seeds in lbp_ms (stream-ordered, no synchronisation)
static int lbp_launch(nlmc_ctx *c, int n_problems, int n_lambdas, double beta, double tolerance, int max_iterations, double sat,
                      bool want_all, bool single_workgroup = false)
{
    const int n = c->n, nnz = (int)c->nnz;
    const size_t P = (size_t)n_problems;
    HIP_TRY(c, hipMemsetAsync(c->lbp_mag.p, 0, sizeof(double) * P * n, c->cur));
    HIP_TRY(c, hipMemsetAsync(c->lbp_out_i.p, 0, sizeof(int32_t) * P * (2 + (size_t)n_lambdas), c->cur));
    LbpArgs a{};
    a.n = n; a.nnz = nnz; a.n_lams = n_lambdas; a.max_iter = max_iterations;
    a.rowptr = c->rowptr.p; a.col = c->col.p; a.src = c->lbp_src.p; a.rev = c->lbp_rev.p;
    a.val = c->val64.p; a.tJ = c->lbp_tJ.p; a.h = c->h64.p; a.eps = c->lbp_eps.p; a.m_star = c->lbp_ms.p; a.lams = c->lbp_lams.p;
    a.beta = beta; a.inv_beta = 1.0 / beta; a.tol = tolerance; a.sat = sat; a.usat = std::atanh(sat) / beta;
    a.w0 = c->lbp_w0.p; a.w1 = c->lbp_w1.p; a.hm = c->lbp_hm.p; a.tot = c->lbp_tot.p; a.mag = c->lbp_mag.p;
    a.mag_all = want_all ? c->lbp_mag_all.p : nullptr;
    a.out_nlam = c->lbp_out_i.p; a.out_status = c->lbp_out_i.p + P; a.out_iters = c->lbp_out_i.p + 2 * P;
    // Workgroups per problem (a problem is bound by the fp64 VALU of the CUs it runs on): up to 8 when FEW problems
    // are in flight and each has work for them.  The group barrier costs two agent-scope fences per iteration, and L2
    // write-backs from many workgroups at once are expensive -- measured: 1 problem of 10^4 spins 23 -> 6.6 ms with 8
    // workgroups, 4 problems 23 -> 8.9 ms, but 64 problems 41 -> 67 ms with 4 each (and 8x slower at 10^3 spins): so
    // at most 32 workgroups take part in barriers, every launch stays resident (<= one workgroup per CU) in any case.
    int cus = 0;
    HIP_TRY(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    int group = 1;
    while (group < 8 && (long long)n_problems * group * 2 <= std::min(32, cus) && n / (group * 2) >= 1024) group *= 2;
    if (const int v = c->knobs.lbp_group; v >= 1 && v <= 8 && (long long)n_problems * v <= cus) group = v;
    if (single_workgroup) group = 1;
    a.group = group;
    a.poll_budget = c->knobs.lbp_poll_budget;      // (test knob: provoke the timeout path)
    HIP_TRY(c, c->lbp_bar.reserve(P));
    HIP_TRY(c, c->lbp_part.reserve(P * 2 * (size_t)group * 4));
    HIP_TRY(c, hipMemsetAsync(c->lbp_bar.p, 0, sizeof(unsigned int) * P, c->cur));
    a.bar = c->lbp_bar.p; a.part = c->lbp_part.p;
    // small instances: messages in LDS, a thread's edges in registers (k_lbp_lds; same bits): 8 waves x 12 edges per thread, two
    // messages in lock step (other shapes: see the kernel's header)
    if (group == 1 && n <= 2048 && nnz <= 6144 && !c->knobs.lbp_global) {
        const size_t lds_small = ((size_t)2 * (6144 + 1) + 2048 + 1 + 64) * sizeof(double);
        const void *kf = c->has_diag ? reinterpret_cast<const void *>(k_lbp_lds<512, 12, 4, true, 2>)
                                     : reinterpret_cast<const void *>(k_lbp_lds<512, 12, 4, false, 2>);
        { int rc = ensure_lds(c, kf, lds_small); if (rc) return rc; }
        void *kargs[] = {&a};
        HIP_TRY(c, hipLaunchKernel(kf, dim3(n_problems), dim3(512), kargs, lds_small, c->cur));
        return NLMC_OK;
    }
    hipLaunchKernelGGL(k_lbp, dim3(n_problems * group), dim3(NLMC_LBP_THREADS), 0, c->cur, a);
    HIP_TRY(c, hipGetLastError());
    return NLMC_OK;
}

int nlmc_lbp_convexified(nlmc_ctx *c, int n_problems, const double *m_star, const double *epsilon, const double *lambdas,
                         int n_lambdas, double beta, double tolerance, int max_iterations, double sat,
                         double *out_mag, double *out_mag_all, int32_t *out_n_lambdas, int32_t *out_iters,
                         int32_t *out_status)
{
    if (!c) return NLMC_ERR_ARG;
    if (n_problems < 1 || n_lambdas < 1 || !m_star || !epsilon || !lambdas || !out_mag || !out_n_lambdas || !out_iters ||
        !out_status || max_iterations < 0 || !(beta != 0.0))
        return fail(c, NLMC_ERR_ARG, "nlmc_lbp_convexified: bad sizes or NULL arrays");
    HIP_TRY(c, hipSetDevice(c->device));
    const int n = c->n;
    const size_t P = (size_t)n_problems;
    { int rc = lbp_setup(c, n_problems, epsilon, lambdas, n_lambdas, beta, out_mag_all != nullptr); if (rc) return rc; }
    HIP_TRY(c, hipMemcpyAsync(c->lbp_ms.p, m_star, sizeof(double) * P * n, hipMemcpyHostToDevice, c->cur));
    { int rc = lbp_launch(c, n_problems, n_lambdas, beta, tolerance, max_iterations, sat, out_mag_all != nullptr); if (rc) return rc; }
    std::vector<int32_t> oi(P * (2 + (size_t)n_lambdas));
    HIP_TRY(c, hipMemcpyAsync(oi.data(), c->lbp_out_i.p, sizeof(int32_t) * oi.size(), hipMemcpyDeviceToHost, c->cur));
    HIP_TRY(c, hipMemcpyAsync(out_mag, c->lbp_mag.p, sizeof(double) * P * n, hipMemcpyDeviceToHost, c->cur));
    if (out_mag_all)
        HIP_TRY(c, hipMemcpyAsync(out_mag_all, c->lbp_mag_all.p, sizeof(double) * P * (size_t)n_lambdas * n, hipMemcpyDeviceToHost, c->cur));
    HIP_TRY(c, hipStreamSynchronize(c->cur));
    bool lost = false;
    for (size_t q = 0; q < P; ++q) lost = lost || oi[P + q] == 2;
    if (lost) {
        // The workgroups that share a problem poll each other with a bounded budget; they only find each other when all of
        // them are resident, which another context on the same GPU can prevent.  Once more with ONE workgroup per
        // problem -- slower, no barrier between workgroups, same bits -- before giving up.
        HIP_TRY(c, hipMemcpyAsync(c->lbp_ms.p, m_star, sizeof(double) * P * n, hipMemcpyHostToDevice, c->cur));
        { int rc = lbp_launch(c, n_problems, n_lambdas, beta, tolerance, max_iterations, sat, out_mag_all != nullptr, true); if (rc) return rc; }
        HIP_TRY(c, hipMemcpyAsync(oi.data(), c->lbp_out_i.p, sizeof(int32_t) * oi.size(), hipMemcpyDeviceToHost, c->cur));
        HIP_TRY(c, hipMemcpyAsync(out_mag, c->lbp_mag.p, sizeof(double) * P * n, hipMemcpyDeviceToHost, c->cur));
        if (out_mag_all)
            HIP_TRY(c, hipMemcpyAsync(out_mag_all, c->lbp_mag_all.p, sizeof(double) * P * (size_t)n_lambdas * n, hipMemcpyDeviceToHost, c->cur));
        HIP_TRY(c, hipStreamSynchronize(c->cur));
    }
    for (size_t q = 0; q < P; ++q)
        if (oi[P + q] == 2) return fail(c, NLMC_ERR_HIP, "nlmc_lbp_convexified: the workgroups of a problem lost each other (group barrier timed out)");
    std::memcpy(out_n_lambdas, oi.data(), sizeof(int32_t) * P);
    std::memcpy(out_status, oi.data() + P, sizeof(int32_t) * P);
    std::memcpy(out_iters, oi.data() + 2 * P, sizeof(int32_t) * P * (size_t)n_lambdas);
    return NLMC_OK;
}

// ------------------------------------------------------------------------------------------------------
// replica-exchange rounds whose marked temperature slots run NMC cycles: chain subsets, device-side hand-offs
// ------------------------------------------------------------------------------------------------------
int nlmc_pt_mark_slots(nlmc_ctx *c, const uint8_t *marks)
{
    if (!c) return NLMC_ERR_ARG;
    if (c->ladder_len == 0) return fail(c, NLMC_ERR_STATE, "nlmc_pt_mark_slots: call nlmc_pt_init first");
    const int L = c->ladder_len;
    if (c->chain_base % L != 0 || c->n_chains % L != 0)
        return fail(c, NLMC_ERR_UNSUPPORTED, "nlmc_pt_mark_slots: every ladder must lie inside one context");
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<uint8_t> m((size_t)L, 0);
    int k = 0;
    if (marks) for (int r = 0; r < L; ++r) { m[(size_t)r] = marks[r] ? 1 : 0; k += m[(size_t)r]; }
    HIP_TRY(c, c->slot_mark.reserve((size_t)L));
    HIP_TRY(c, c->sub_list_buf.reserve((size_t)std::max(c->n_chains, 1)));
    HIP_TRY(c, c->cmask.reserve((size_t)std::max(c->n_chains, 1) * c->n_pad));
    HIP_TRY(c, c->nmc_status.reserve(1));
    HIP_TRY(c, hipMemcpyAsync(c->slot_mark.p, m.data(), (size_t)L, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->nmc_status.p, 0, sizeof(int32_t), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->cmask.p, 0, (size_t)std::max(c->n_chains, 1) * c->n_pad, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));          // (`m` goes away)
    c->n_marked_local = k * (c->n_chains / L);
    c->subset = 0;
    c->sub_dirty = true;
    return NLMC_OK;
}

int nlmc_select_chains(nlmc_ctx *c, int which)
{
    if (!c) return NLMC_ERR_ARG;
    if (which < NLMC_CHAINS_ALL || which > NLMC_CHAINS_MARKED) return fail(c, NLMC_ERR_ARG, "nlmc_select_chains: bad selector");
    if (which != NLMC_CHAINS_ALL && !c->slot_mark.p) return fail(c, NLMC_ERR_STATE, "nlmc_select_chains: call nlmc_pt_mark_slots first");
    HIP_TRY(c, hipSetDevice(c->device));
    // the subset-aware launches of the marked chains go to the second stream when overlap is on: forked from the main stream
    // where the first subset of a round is selected (after the chain lists are up to date, before any subset work is
    // queued), joined again where all chains are selected
    if (which != NLMC_CHAINS_ALL) {
        c->subset = which;
        if (c->cur == c->stream) { int rc = ensure_subset(c); if (rc) return rc; }
        if (c->overlap && !c->forked) {
            HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));
            c->forked = true;
        }
        if (c->overlap && which == NLMC_CHAINS_MARKED && c->cur == c->stream) {
            HIP_TRY(c, hipStreamWaitEvent(c->aux, c->ev_fork, 0));
            c->cur = c->aux;
        } else if (which == NLMC_CHAINS_UNMARKED && c->cur != c->stream) {
            return fail(c, NLMC_ERR_STATE, "nlmc_select_chains: select all chains between the marked and the unmarked subset of a round");
        }
        return NLMC_OK;
    }
    if (c->cur != c->stream) {
        HIP_TRY(c, hipEventRecord(c->ev_join, c->aux));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
        c->cur = c->stream;
    }
    c->forked = false;
    c->subset = which;
    return NLMC_OK;
}

int nlmc_own_stream(nlmc_ctx *c)
{
    if (!c) return NLMC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->owns_stream) return NLMC_OK;
    if (c->cur != c->stream) return fail(c, NLMC_ERR_STATE, "nlmc_own_stream: select all chains first");
    if (c->comm) return fail(c, NLMC_ERR_STATE, "nlmc_own_stream: call it before nlmc_comm_init");
    // whatever was queued on the stream given at creation is finished first: from here on the two streams are unrelated
    if (c->stream) HIP_TRY(c, hipStreamSynchronize(c->stream)); else HIP_TRY(c, hipDeviceSynchronize());
    hipStream_t s = nullptr;
    HIP_TRY(c, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    c->stream = s;
    c->cur = s;
    c->owns_stream = true;
    return NLMC_OK;
}

int nlmc_overlap_subsets(nlmc_ctx *c, int on)
{
    if (!c) return NLMC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->cur != c->stream) return fail(c, NLMC_ERR_STATE, "nlmc_overlap_subsets: select all chains first");
    if (on && !c->aux) {
        HIP_TRY(c, hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking));
        HIP_TRY(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        HIP_TRY(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    }
    c->overlap = on != 0;
    return NLMC_OK;
}

int nlmc_subset_count(const nlmc_ctx *c) { return c ? c->sub_count() : 0; }

int nlmc_get_subset(nlmc_ctx *c, int32_t *out_chains)
{
    if (!c || !out_chains) return fail(c, NLMC_ERR_ARG, "nlmc_get_subset: NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const int R = c->sub_count();
    if (c->subset == 0) { for (int i = 0; i < R; ++i) out_chains[i] = i; return NLMC_OK; }
    { int rc = ensure_subset(c); if (rc) return rc; }
    HIP_TRY(c, hipMemcpyAsync(out_chains, c->sub_list(), sizeof(int32_t) * (size_t)R, hipMemcpyDeviceToHost, c->cur));
    HIP_TRY(c, hipStreamSynchronize(c->cur));
    return NLMC_OK;
}

int nlmc_track_minimum(nlmc_ctx *c, int on)
{
    if (!c) return NLMC_ERR_ARG;
    c->track_min = on != 0;
    c->track_min_stride = on > 1 ? on : 1;
    return NLMC_OK;
}

// ---- run-long best-state record --------------------------------------------------------------------------------------------------
int nlmc_best_begin(nlmc_ctx *c, double target)
{
    if (!c) return NLMC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t R = (size_t)c->n_chains;
    HIP_TRY(c, c->rec_efix.reserve(R));
    HIP_TRY(c, c->rec_stamp.reserve(R));
    HIP_TRY(c, c->rec_hit.reserve(R));
    HIP_TRY(c, c->rec_state.reserve(R * (size_t)c->n_pad));
    c->best_target = target;
    if (R > 0) {
        hipLaunchKernelGGL(k_best_init, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, c->stream, c->best_rec(), (int)R);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemsetAsync(c->rec_state.p, 0, R * (size_t)c->n_pad, c->stream));
    }
    c->best_on = true;
    return NLMC_OK;
}

int nlmc_best_update(nlmc_ctx *c, uint32_t stamp)
{
    if (!c) return NLMC_ERR_ARG;
    if (!c->best_on) return fail(c, NLMC_ERR_STATE, "nlmc_best_update: no record is open (nlmc_best_begin)");
    if (stamp > (uint32_t)INT32_MAX) return fail(c, NLMC_ERR_ARG, "nlmc_best_update: the stamp does not fit 31 bits");
    if (c->subset != 0 || c->cur != c->stream)
        return fail(c, NLMC_ERR_UNSUPPORTED, "nlmc_best_update: a chain subset is selected (an observation takes every local chain: select all chains first)");
    HIP_TRY(c, hipSetDevice(c->device));
    return launch_best_update(c, stamp);
}

int nlmc_best_read(nlmc_ctx *c, double *out_energy, int32_t *out_stamp, int32_t *out_first_hit, int8_t *out_state)
{
    if (!c) return NLMC_ERR_ARG;
    if (!c->rec_efix.p) return fail(c, NLMC_ERR_STATE, "nlmc_best_read: no record was begun (nlmc_best_begin)");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t R = (size_t)c->n_chains;
    if (R == 0) return NLMC_OK;
    std::vector<long long> e(out_energy ? R : 0);
    if (out_energy) HIP_TRY(c, hipMemcpyAsync(e.data(), c->rec_efix.p, sizeof(long long) * R, hipMemcpyDeviceToHost, c->stream));
    if (out_stamp) HIP_TRY(c, hipMemcpyAsync(out_stamp, c->rec_stamp.p, sizeof(int32_t) * R, hipMemcpyDeviceToHost, c->stream));
    if (out_first_hit) HIP_TRY(c, hipMemcpyAsync(out_first_hit, c->rec_hit.p, sizeof(int32_t) * R, hipMemcpyDeviceToHost, c->stream));
    if (out_state) {
        c->stage_out.resize((size_t)c->n_pad * R);
        HIP_TRY(c, hipMemcpyAsync(c->stage_out.data(), c->rec_state.p, c->stage_out.size(), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (out_state) rows_to_host_finish(c, out_state, (int)R);
    if (out_energy) {
        const double inv = std::ldexp(1.0, -c->escale);         // nlmc_energy_tracked's conversion; a chain never observed reads +inf
        for (size_t i = 0; i < R; ++i) out_energy[i] = e[i] == LLONG_MAX ? HUGE_VAL : (double)e[i] * inv;
    }
    return NLMC_OK;
}

int nlmc_best_end(nlmc_ctx *c)
{
    if (!c) return NLMC_ERR_ARG;
    c->best_on = false;
    return NLMC_OK;
}

// ---- run-long per-round energy log -----------------------------------------------------------------------------------------------
int nlmc_elog_begin(nlmc_ctx *c, uint32_t round0, int n_rounds)
{
    if (!c) return NLMC_ERR_ARG;
    if (n_rounds < 0) return fail(c, NLMC_ERR_ARG, "nlmc_elog_begin: bad argument");
    if (c->ladder_len == 0) return fail(c, NLMC_ERR_STATE, "nlmc_elog_begin: call nlmc_pt_init first");
    if (c->comm || (c->apt_R > 0 && c->apt_world > 1) || c->chain_base % c->ladder_len != 0 || c->n_chains % c->ladder_len != 0)
        return fail(c, NLMC_ERR_UNSUPPORTED, "nlmc_elog_begin: the context has a communicator or holds a cut ladder (the log takes contexts of whole ladders)");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t tot = (size_t)n_rounds * (size_t)c->n_chains;
    c->elog_on = false;
    HIP_TRY(c, c->elog_energy.reserve(std::max<size_t>(tot, 1)));
    HIP_TRY(c, c->elog_slot.reserve(std::max<size_t>(tot, 1)));
    if (tot > 0) {                                  // all ones: a NaN and -1, a row no observation reached
        HIP_TRY(c, hipMemsetAsync(c->elog_energy.p, 0xFF, sizeof(double) * tot, c->stream));
        HIP_TRY(c, hipMemsetAsync(c->elog_slot.p, 0xFF, sizeof(int32_t) * tot, c->stream));
    }
    c->elog_round0 = round0; c->elog_rounds = n_rounds;
    c->elog_on = true;
    return NLMC_OK;
}

int nlmc_elog_update(nlmc_ctx *c, uint32_t round)
{
    if (!c) return NLMC_ERR_ARG;
    if (c->ladder_len == 0) return fail(c, NLMC_ERR_STATE, "nlmc_elog_update: call nlmc_pt_init first");
    if (!c->elog_on) return fail(c, NLMC_ERR_STATE, "nlmc_elog_update: no log is open (nlmc_elog_begin)");
    if (c->subset != 0 || c->cur != c->stream)
        return fail(c, NLMC_ERR_UNSUPPORTED, "nlmc_elog_update: a chain subset is selected (an observation takes every local chain: select all chains first)");
    HIP_TRY(c, hipSetDevice(c->device));
    return launch_elog_update(c, round);
}

int nlmc_elog_read(nlmc_ctx *c, double *out_energy, int32_t *out_slot)
{
    if (!c) return NLMC_ERR_ARG;
    if (!c->elog_energy.p) return fail(c, NLMC_ERR_STATE, "nlmc_elog_read: no log was begun (nlmc_elog_begin)");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t tot = (size_t)c->elog_rounds * (size_t)c->n_chains;
    if (tot == 0) return NLMC_OK;
    if (out_energy) HIP_TRY(c, hipMemcpyAsync(out_energy, c->elog_energy.p, sizeof(double) * tot, hipMemcpyDeviceToHost, c->stream));
    if (out_slot) HIP_TRY(c, hipMemcpyAsync(out_slot, c->elog_slot.p, sizeof(int32_t) * tot, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NLMC_OK;
}

int nlmc_elog_end(nlmc_ctx *c)
{
    if (!c) return NLMC_ERR_ARG;
    c->elog_on = false;
    return NLMC_OK;
}

int nlmc_backbone_seed(nlmc_ctx *c, int mode)
{
    if (!c) return NLMC_ERR_ARG;
    if (mode < 0 || mode > 1) return fail(c, NLMC_ERR_ARG, "nlmc_backbone_seed: mode must be 0 or 1");
    HIP_TRY(c, hipSetDevice(c->device));
    if (mode == 0) { c->seed_snap_on = false; return NLMC_OK; }
    const size_t bytes = (size_t)std::max(c->n_chains, 1) * c->n_pad;
    HIP_TRY(c, c->seed_snap.reserve(bytes));
    HIP_TRY(c, hipMemcpyAsync(c->seed_snap.p, c->spins.p, bytes, hipMemcpyDeviceToDevice, c->cur));
    c->seed_snap_on = true;
    return NLMC_OK;
}

int nlmc_adopt_best(nlmc_ctx *c)
{
    if (!c) return NLMC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const int R = c->sub_count();
    if (R == 0) return NLMC_OK;
    { int rc = ensure_subset(c); if (rc) return rc; }
    hipLaunchKernelGGL(k_adopt_best, dim3(R), dim3(256), 0, c->cur, c->n_pad, c->sub_list(), c->spins.p, c->best.p, c->efix.p, c->emin.p);
    HIP_TRY(c, hipGetLastError());
    return NLMC_OK;
}

int nlmc_backbone_clusters(nlmc_ctx *c, const double *epsilon, const double *lambdas, int n_lambdas, double beta, double tolerance,
                           int max_iterations, double sat, const double *thresholds, int n_thresholds)
{
    if (!c) return NLMC_ERR_ARG;
    if (!epsilon || !lambdas || n_lambdas < 1 || !thresholds || n_thresholds < 1 || max_iterations < 0 || !(beta != 0.0))
        return fail(c, NLMC_ERR_ARG, "nlmc_backbone_clusters: bad sizes or NULL arrays");
    HIP_TRY(c, hipSetDevice(c->device));
    const int P = c->sub_count();
    if (P == 0) return NLMC_OK;
    { int rc = ensure_subset(c); if (rc) return rc; }
    { int rc = lbp_setup(c, P, epsilon, lambdas, n_lambdas, beta, false); if (rc) return rc; }
    HIP_TRY(c, c->cmask.reserve((size_t)c->n_chains * c->n_pad));
    if (!c->nmc_status.p) {
        HIP_TRY(c, c->nmc_status.reserve(1));
        HIP_TRY(c, hipMemsetAsync(c->nmc_status.p, 0, sizeof(int32_t), c->cur));
    }
    const std::vector<double> thr(thresholds, thresholds + n_thresholds);
    if (thr != c->nmc_thr_host) {
        HIP_TRY(c, c->nmc_thr.reserve((size_t)n_thresholds));
        HIP_TRY(c, hipStreamSynchronize(c->cur));
        HIP_TRY(c, hipMemcpyAsync(c->nmc_thr.p, thr.data(), sizeof(double) * thr.size(), hipMemcpyHostToDevice, c->cur));
        HIP_TRY(c, hipStreamSynchronize(c->cur));
        c->nmc_thr_host = thr;
    }
    hipLaunchKernelGGL(k_lbp_seeds, dim3(P), dim3(256), 0, c->cur, c->n, c->n_pad, c->sub_list(), c->seed_snap_on ? c->seed_snap.p : c->spins.p, c->lbp_ms.p);
    HIP_TRY(c, hipGetLastError());
    { int rc = lbp_launch(c, P, n_lambdas, beta, tolerance, max_iterations, sat, false); if (rc) return rc; }
    if (c->big || (size_t)2 * c->n_pad > (size_t)60 * 1024) {
        HIP_TRY(c, c->cmask_scratch.reserve((size_t)P * 2 * c->n_pad));
        hipLaunchKernelGGL(k_cluster_mask<true>, dim3(P), dim3(1024), 0, c->cur, c->g, c->sub_list(), c->lbp_mag.p,
                           c->lbp_out_i.p + P, c->nmc_thr.p, n_thresholds, c->cmask.p, c->nmc_status.p, c->cmask_scratch.p);
    } else
        hipLaunchKernelGGL(k_cluster_mask<false>, dim3(P), dim3(256), (size_t)2 * c->n_pad, c->cur, c->g, c->sub_list(), c->lbp_mag.p,
                           c->lbp_out_i.p + P, c->nmc_thr.p, n_thresholds, c->cmask.p, c->nmc_status.p, (uint8_t *)nullptr);
    HIP_TRY(c, hipGetLastError());
    return NLMC_OK;
}

int nlmc_backbone_check(nlmc_ctx *c)
{
    if (!c) return NLMC_ERR_ARG;
    if (!c->nmc_status.p) return NLMC_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    int32_t st = 0;
    HIP_TRY(c, hipMemcpyAsync(&st, c->nmc_status.p, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (st != 0) {
        HIP_TRY(c, hipMemsetAsync(c->nmc_status.p, 0, sizeof(int32_t), c->stream));
        if (st & 2) return fail(c, NLMC_ERR_HIP, "nlmc_backbone_clusters: the workgroups of a problem lost each other (group barrier timed out)");
        return fail(c, NLMC_ERR_ARG, "LBP diverged at initial lambda, please try a larger lambda_start or increase max_iterations or beta");
    }
    return NLMC_OK;
}

int nlmc_get_cluster_mask(nlmc_ctx *c, uint8_t *out)
{
    if (!c || !out) return fail(c, NLMC_ERR_ARG, "nlmc_get_cluster_mask: NULL argument");
    if (!c->cmask.p) return fail(c, NLMC_ERR_STATE, "nlmc_get_cluster_mask: no backbone inference has run");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->n_chains == 0) return NLMC_OK;
    int rc = rows_to_host_begin(c, c->cmask.p, c->n_chains);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    rows_to_host_finish(c, out, c->n_chains);
    return NLMC_OK;
}

int nlmc_set_cluster_mask(nlmc_ctx *c, const uint8_t *mask)
{
    if (!c || !mask) return fail(c, NLMC_ERR_ARG, "nlmc_set_cluster_mask: NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->n_chains == 0) return NLMC_OK;
    HIP_TRY(c, c->cmask.reserve((size_t)c->n_chains * c->n_pad));
    for (size_t i = 0; i < (size_t)c->n_chains * c->n; ++i)
        if (mask[i] > 1) return fail(c, NLMC_ERR_ARG, "nlmc_set_cluster_mask: entries must be 0 or 1");
    int rc = rows_to_device(c, c->cmask.p, mask, c->n_chains);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NLMC_OK;
}

int nlmc_set_phase(nlmc_ctx *c, int kind, double temp_x)
{
    if (!c) return NLMC_ERR_ARG;
    if (kind < NLMC_PHASE_ALL || kind > NLMC_PHASE_BACKBONE_FROZEN) return fail(c, NLMC_ERR_ARG, "nlmc_set_phase: bad phase");
    HIP_TRY(c, hipSetDevice(c->device));
    if (kind == NLMC_PHASE_ALL) { c->has_flags = false; return NLMC_OK; }     // (temp_x stays: the uploaded temperature tables stay valid)
    if (!(temp_x > 0.0) && !(temp_x < 0.0)) return fail(c, NLMC_ERR_ARG, "nlmc_set_phase: temp_x must be non-zero");
    if (!c->cmask.p) return fail(c, NLMC_ERR_STATE, "nlmc_set_phase: no backbone inference has run");
    const int R = c->sub_count();
    if (R > 0) {
        { int rc = ensure_subset(c); if (rc) return rc; }
        hipLaunchKernelGGL(k_phase_flags, dim3(R), dim3(256), 0, c->cur, c->n_pad, c->sub_list(), c->cmask.p, kind, c->flags.p);
        HIP_TRY(c, hipGetLastError());
    }
    c->has_flags = true;
    c->temp_x = temp_x;
    return NLMC_OK;
}

int nlmc_set_fused_f64_real(nlmc_ctx *c, int on)
{
    if (!c) return NLMC_ERR_ARG;
    const bool v = on != 0;
    if (v != c->f64_real) {                 // plans are made for one setting (value plane, entry order): drop them
        c->f64_real = v;
        c->fz[0].valid = false;
        c->fz[1].valid = false;
    }
    return NLMC_OK;
}

int nlmc_plan_slot(nlmc_ctx *c, int slot)
{
    if (!c) return NLMC_ERR_ARG;
    if (slot < 0 || slot > 1) return fail(c, NLMC_ERR_ARG, "nlmc_plan_slot: slot must be 0 or 1");
    c->fz_slot = slot;
    return NLMC_OK;
}

int nlmc_find_clusters(int n, const int32_t *rowptr, const int32_t *colidx, const double *vals, const double *mag,
                       double threshold_initial, double threshold_cutoff, double threshold_step, int32_t *out_members,
                       int64_t members_capacity, int32_t *out_sizes, int32_t *out_n_clusters)
{
    if (n < 1 || !rowptr || !mag || !out_members || !out_sizes || !out_n_clusters || (rowptr[n] > 0 && (!colidx || !vals)))
        return fail(nullptr, NLMC_ERR_ARG, "nlmc_find_clusters: bad sizes or NULL arrays");
    if (!(threshold_step > 0.0)) return fail(nullptr, NLMC_ERR_ARG, "nlmc_find_clusters: threshold_step must be > 0");
    if (host_find_clusters(n, rowptr, colidx, vals, mag, threshold_initial, threshold_cutoff, threshold_step, out_members,
                           members_capacity, out_sizes, out_n_clusters) != 0)
        return fail(nullptr, NLMC_ERR_ARG, "nlmc_find_clusters: out_members too small");
    return NLMC_OK;
}

int nlmc_host_prefault(void *ptr, int64_t bytes, int n_threads)
{
    if (!ptr || bytes < 0) return fail(nullptr, NLMC_ERR_ARG, "nlmc_host_prefault: bad argument");
    if (n_threads <= 0) n_threads = (int)std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    const int64_t page = 4096, pages = (bytes + page - 1) / page;
    const int64_t nt = std::max<int64_t>(1, std::min<int64_t>(n_threads, pages / 256 + 1));
    auto part = [&](int64_t p0, int64_t p1) {
        volatile unsigned char *b = static_cast<volatile unsigned char *>(ptr);
        for (int64_t q = p0; q < p1; ++q) b[q * page] = 0;
    };
    if (nt == 1) { part(0, pages); return NLMC_OK; }
    std::vector<std::thread> th;
    for (int64_t i = 0; i < nt; ++i) th.emplace_back(part, pages * i / nt, pages * (i + 1) / nt);
    for (auto &t : th) t.join();
    return NLMC_OK;
}

int nlmc_trace_layout(const int8_t *src, int64_t n_blocks, int64_t n_sweeps, int64_t n, const int32_t *dst_block,
                      const int32_t *dst_col, int64_t n_dst_blocks, int64_t row_len, void *dst, int elem_bytes, int n_threads)
{
    if (n_blocks < 0 || n_sweeps < 0 || n < 1 || (n_blocks * n_sweeps > 0 && (!src || !dst)) || row_len < n_sweeps ||
        (!dst_block && n_dst_blocks < n_blocks))
        return fail(nullptr, NLMC_ERR_ARG, "nlmc_trace_layout: bad sizes or NULL arrays");
    if (elem_bytes != 1 && elem_bytes != 8) return fail(nullptr, NLMC_ERR_ARG, "nlmc_trace_layout: elem_bytes must be 1 or 8");
    if ((dst_block || dst_col) && n_sweeps > 0) {    // destinations: in range, whole column groups, distinct (threads write disjointly)
        const int64_t groups = row_len / n_sweeps;
        std::vector<uint8_t> seen((size_t)(n_dst_blocks * groups), 0);
        for (int64_t b = 0; b < n_blocks; ++b) {
            const int64_t r = dst_block ? dst_block[b] : b, c = dst_col ? dst_col[b] : 0;
            if (r < 0 || r >= n_dst_blocks || c < 0 || c % n_sweeps || c + n_sweeps > row_len || seen[r * groups + c / n_sweeps])
                return fail(nullptr, NLMC_ERR_ARG, "nlmc_trace_layout: destinations must be distinct (block, column group) pairs in range");
            seen[r * groups + c / n_sweeps] = 1;
        }
    }
    if (n_threads <= 0) n_threads = (int)std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    if (elem_bytes == 8) host_trace_layout<double>(src, n_blocks, n_sweeps, n, dst_block, dst_col, row_len, (double *)dst, n_threads);
    else host_trace_layout<int8_t>(src, n_blocks, n_sweeps, n, dst_block, dst_col, row_len, (int8_t *)dst, n_threads);
    return NLMC_OK;
}

}  // extern "C"
