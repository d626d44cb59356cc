// nlmc_lane_rounds.h -- tempering rounds of short chains in one launch: a ladder per wave (gfx950 / wave64).
//
// k_sweep_lanes (csrc/nlmc_lanes.h) gives a chain a lane.  A ladder of L <= 64 temperatures then fits inside one wave, and a swap round
// needs nothing from outside it: the partner's energy is another lane's register, the decision one Philox call.  k_rounds_lanes runs
// n_rounds rounds -- T sweeps at the ladder temperatures, then the swap round of k_pt_swap -- with the spins transposed in LDS for the
// whole launch.  No wave waits for another one: no barrier, no atomic, no poll, no cooperative launch, no residency condition.
//
//   launch : workgroup = one wave holding P = 64 / L whole ladders; lane l < P L of block b owns local chain b P L + l, so ladder
//            (l / L) of the wave is local ladder b P + l / L.  Lanes past the wave's last ladder are the tail lanes of k_sweep_lanes:
//            valid addresses, a zeroed LDS column, nothing written, no pair.
//   sweeps : the update of k_sweep_lanes<F64, shared order> operation for operation (no flags, no per-sweep outputs).
//   swaps  : the planned selection of the round; lane p of a ladder's lane group decides pair p from the two energies the wave
//            shuffles to it, with the key and arithmetic of k_pt_swap (pt_swap_decide).  Chains never move: two byte maps in LDS,
//            lane_of_slot[ladder in wave][slot] and slot_of_lane[lane], exchange entries, and a lane whose slot moved reloads its
//            inverse temperature (and its RNG key where that follows the slot).  One body, lane_swap_round, here and in
//            k_apt_rounds_lanes.
// Same bits as nlmc_sweep_philox(beta = NULL) + nlmc_pt_swap_philox round by round, on any route.
#pragma once
#include "nlmc_lanes.h"

struct LaneRoundsArgs {
    int n_rounds, ladder_len, n_pairs;
    int n_ladders;                   // of the GLOBAL chain set (rows of the plan and of the log)
    uint32_t round0;
    const int32_t *plan_pairs;       // [n_rounds][n_ladders][n_pairs][2] at round0
    const double *beta;              // [ladder_len]
    int32_t *slot_of_chain, *chain_of_slot;
    int32_t *log_pairs;              // the rows of the device-side swap log at round0, or nullptr
    uint8_t *log_acc;
    int lds_map_off;                 // LDS offset of the two 64-byte maps: lane_of_slot | slot_of_lane
    BestRec best;                    // k_rounds_lanes<.., BEST>: the open best-state record (nlmc_best_begin), efix = nullptr: none
    ElogRec elog;                    // k_rounds_lanes<.., BEST>, k_apt_rounds_lanes<.., ELOG>: the open energy log (nlmc_elog_begin), energy = nullptr: none
};

// The wave's chains come in: their nrow rows (consecutive, `rows` the first) read coalesced and written transposed to the wave's LDS
// region, the columns of the tail lanes zeroed (tail lanes walk the wave's first chain on a zeroed column and write nothing), and the
// two slot maps set up from the lane's slot.  The workgroup's LDS accesses of one wave execute in program order (lane_lds_fence).
__device__ __forceinline__ void lane_ladders_in(unsigned char *lds, const int8_t *rows, int n_pad, int nrow, int lane, bool live, int base,
                                                int slot, uint8_t *lane_of_slot, uint8_t *slot_of_lane)
{
    for (int r = 0; r < 64; ++r) {
        if (r < nrow) lane_column_in(lds, NLMC_LANE_STRIDE, r, rows + (size_t)r * n_pad, n_pad, lane);
        else for (int j = lane; j < n_pad; j += 64) lds[j * NLMC_LANE_STRIDE + r] = 0;
    }
    lane_of_slot[lane] = (uint8_t)lane;
    slot_of_lane[lane] = (uint8_t)slot;
    lane_lds_fence();
    if (live) lane_of_slot[base + slot] = (uint8_t)lane;                // (the slots of a ladder are a permutation: every entry below nrow)
    lane_lds_fence();
}

// THE swap round of k_pt_swap inside a wave, for round r of the launch: planned selection, one lane per pair (lane p of a ladder's lane
// group decides pair p), energies by shuffle, the key and arithmetic of pt_swap_decide.  g: the lane's global ladder, base: its first
// entry of lane_of_slot, E: the lane's tracked energy; p = lane - base and decides = live && p < n_pairs are the caller's, computed
// once per launch (inside this function they cost k_apt_rounds_lanes<f64> its register allocation: DESIGN.md section 6).  Chains never
// move: the two maps exchange entries.  Returns whether the lane's slot moved (slot is then the new one): the caller reloads what it
// keeps per slot.
__device__ __forceinline__ bool lane_swap_round(const LaneRoundsArgs &q, int r, int g, int base, int lane, int p, bool decides, long long E, double inv,
                                                uint32_t seed_lo, uint32_t seed_hi, uint8_t *lane_of_slot, uint8_t *slot_of_lane, int &slot)
{
    if (q.n_pairs <= 0) return false;
    const uint32_t round = q.round0 + (uint32_t)r;
    const size_t at = ((size_t)r * q.n_ladders + g) * q.n_pairs + (decides ? p : 0);
    const int i = decides ? q.plan_pairs[2 * at] : 0;
    const int la = decides ? (int)lane_of_slot[base + i] : lane, lb = decides ? (int)lane_of_slot[base + i + 1] : lane;
    const int elo = (int)(unsigned)(unsigned long long)E, ehi = (int)(unsigned)((unsigned long long)E >> 32);
    const unsigned alo = (unsigned)__shfl(elo, la, 64), ahi = (unsigned)__shfl(ehi, la, 64);
    const unsigned blo = (unsigned)__shfl(elo, lb, 64), bhi = (unsigned)__shfl(ehi, lb, 64);
    const double Ea = (double)(long long)(((unsigned long long)ahi << 32) | alo) * inv;
    const double Eb = (double)(long long)(((unsigned long long)bhi << 32) | blo) * inv;
    lane_lds_fence();
    if (decides) {
        const bool acc = pt_swap_decide(p, i, i, Ea, Eb, q.beta, round, g, seed_lo, seed_hi);
        if (acc) {                                   // selected pairs are disjoint: no two lanes touch one entry
            lane_of_slot[base + i] = (uint8_t)lb; lane_of_slot[base + i + 1] = (uint8_t)la;
            slot_of_lane[la] = (uint8_t)(i + 1); slot_of_lane[lb] = (uint8_t)i;
        }
        if (q.log_pairs) {
            q.log_pairs[2 * at] = i; q.log_pairs[2 * at + 1] = i + 1;
            q.log_acc[at] = acc ? 1 : 0;
        }
    }
    lane_lds_fence();
    const int ns = (int)slot_of_lane[lane];
    const bool moved = ns != slot;
    slot = ns;
    return moved;
}

// SweepArgs fields of this kernel: those of k_sweep_lanes' shared order without flags and outputs; n_sweeps = sweeps per round, sweep0 =
// the first sweep of the launch, lane_perm = the orders of all its n_rounds * n_sweeps sweeps, lane_rows = the context's chains,
// tab = the ladder's table (two entries per slot).
// BEST: an observer is open -- a best-state record, an energy log or both (the records' pointers say which).  Record: after a round's
// sweeps every live lane compares its own energy with its chain's record (three registers, read in the prologue and written back at
// the end of the launch); the columns of the lanes that improved go out one at a time, the whole wave writing one chain's row.  Log:
// at the same place every live lane stores its energy and slot to the round's row (chains of a wave are consecutive: the stores
// coalesce).  Tail lanes record nothing.  Without BEST the kernel is the one it was.
template <bool F64, bool BEST = false>
__global__ __launch_bounds__(64) void k_rounds_lanes(SweepArgs a, LaneRoundsArgs q)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    typedef std::conditional_t<F64, double, float> T;
    const int lane = threadIdx.x;
    constexpr int stride = NLMC_LANE_STRIDE;
    const int n = a.g.n, n_pad = a.g.n_pad;
    const int L = q.ladder_len, P = 64 / L;
    const int lad0 = (int)blockIdx.x * P;                               // first local ladder of this wave
    const int nlad = min(P, a.lane_rows / L - lad0);                    // its ladders (wave-uniform)
    const int row0 = lad0 * L, nrow = nlad * L;
    const bool live = lane < nrow;
    const int c = live ? row0 + lane : row0;                            // local chain (tail lanes: the wave's first, read only)
    const int lw = live ? lane / L : 0, base = lw * L;                  // ladder in the wave, its first entry of lane_of_slot
    const int g = a.chain_base / L + lad0 + lw;                         // global ladder: Philox key, rows of plan / log / chain_of_slot
    int8_t *s = reinterpret_cast<int8_t *>(lds_raw);
    uint32_t *rtab = a.lane_tab ? reinterpret_cast<uint32_t *>(lds_raw + a.lds_u_off) : nullptr;   // word (spin k, lane l) at k * 64 + l
    uint8_t *lane_of_slot = lds_raw + q.lds_map_off, *slot_of_lane = lane_of_slot + 64;

    const uint32_t gc_chain = (uint32_t)(a.chain_base + c);
    int slot = q.slot_of_chain[gc_chain];
    lane_ladders_in(lds_raw, a.spins + (size_t)row0 * n_pad, n_pad, nrow, lane, live, base, slot, lane_of_slot, slot_of_lane);

    const bool key_by_slot = a.rng_stride != 0;
    uint32_t gc = key_by_slot ? (uint32_t)((c / a.rng_ladder_len) * a.rng_stride + a.rng_base + slot) : gc_chain;
    T cb0 = scale_cb((T)a.tab[(size_t)slot * a.tab_cs], a.qinv);       // (the slot's second entry scales flagged spins: none here)
    const double esc = __longlong_as_double((long long)(1023 + a.escale) << 52);   // 2^escale
    const double inv = __longlong_as_double((long long)(1023 - a.escale) << 52);   // 2^-escale
    long long E = a.efix[c];
    const int p = lane - base;
    const bool decides = live && p < q.n_pairs;                        // lane p of a ladder's group decides pair p
    long long rec_e = 0x7FFFFFFFFFFFFFFFll;
    int32_t rec_stamp = -1, rec_hit = -1;
    const bool has_best = BEST && q.best.efix != nullptr;
    if (has_best && live) { rec_e = q.best.efix[c]; rec_stamp = q.best.stamp[c]; rec_hit = q.best.first_hit[c]; }

    for (int r = 0; r < q.n_rounds; ++r) {
        long long e_loc = 0;
        for (int t = 0; t < a.n_sweeps; ++t) {
            const uint32_t tt = a.sweep0 + (uint32_t)(r * a.n_sweeps + t);
            const uint16_t *pp = a.lane_perm + ((size_t)r * a.n_sweeps + t) * (size_t)n;
            // random numbers of the sweep (k_sweep_lanes): f32 the logistic thresholds, f64 the UNIFORM words
            if (rtab) {
                for (int b = 0; b < (n + 3) / 4; ++b) {
                    const u32x4 rr = philox4x32_10((uint32_t)b, tt, gc, NLMC_TAG_UNIFORM, a.seed_lo, a.seed_hi);
                    uint32_t *d = rtab + (size_t)(4 * b) * 64 + lane;
                    if (F64) { d[0] = rr.x; d[64] = rr.y; d[128] = rr.z; d[192] = rr.w; }
                    else {
                        d[0] = __float_as_uint(threshold_spec(rr.x)); d[64] = __float_as_uint(threshold_spec(rr.y));
                        d[128] = __float_as_uint(threshold_spec(rr.z)); d[192] = __float_as_uint(threshold_spec(rr.w));
                    }
                }
            }
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int kv = (i0 + lane < n) ? (int)pp[i0 + lane] : 0;   // 64 entries of the order in one load, handed out as scalars
                const int ni = min(64, n - i0);
                for (int ii = 0; ii < ni; ++ii) {
                    const int k = __builtin_amdgcn_readlane(kv, ii);
                    const int so = (int)s[k * stride + lane];
                    const int rs = lane_ro<true>(a.g.rowptr + k), re = lane_ro<true>(a.g.rowptr + k + 1);
                    const uint32_t hi = rtab ? rtab[(size_t)k * 64 + lane]
                                             : (F64 ? lane_word(philox4x32_10((uint32_t)(k >> 2), tt, gc, NLMC_TAG_UNIFORM, a.seed_lo, a.seed_hi), k)
                                                    : __float_as_uint(threshold_spec(lane_word(philox4x32_10((uint32_t)(k >> 2), tt, gc, NLMC_TAG_UNIFORM, a.seed_lo, a.seed_hi), k))));
                    int sn;
                    long long de;
                    if constexpr (F64) {
                        double xs, xd;                               // xd: the diagonal term, left out of the energy delta
                        if (a.lane_diag) lane_field<true, true>(a.g, s, lane, k, rs, re, xs, xd);
                        else lane_field<true, false>(a.g, s, lane, k, rs, re, xs, xd);
                        const double hk = lane_ro<true>(a.g.h64 + k);
                        const double x_true = (xs - xd) + hk, xf = xs + hk;
                        const uint32_t lo = lane_word(philox4x32_10((uint32_t)(k >> 2), tt, gc, NLMC_TAG_UNIFORM_LO, a.seed_lo, a.seed_hi), k);
                        const double z = cb0 * xf;
                        sn = accept_up(uniform53_spec(hi, lo), z) ? 1 : -1;
                        de = (sn != so) ? fixed_delta_slow(x_true, sn - so, esc) : 0ll;
                    } else {
                        int X = lane_ro<true>(a.g.hq + k), Xd;
                        if (a.lane_diag) lane_field<true, true>(a.g, s, lane, k, rs, re, X, Xd);
                        else lane_field<true, false>(a.g, s, lane, k, rs, re, X, Xd);
                        const float z = cb0 * (float)X;
                        sn = (z < __uint_as_float(hi)) ? 1 : -1;
                        de = (long long)(X - Xd) * (long long)((so - sn) * (1 << a.eshift));
                    }
                    e_loc += de;
                    s[k * stride + lane] = (int8_t)sn;
                }
            }
        }
        E += e_loc;

        if constexpr (BEST) {                               // one observation of every chain of the wave, before the swap round
            if (q.elog.energy && live) elog_store(q.elog, r, c, (double)E * inv, slot);
            const int32_t stamp = (int32_t)(q.round0 + (uint32_t)r);
            const bool imp = has_best && live && (double)E < (double)rec_e;   // strict: the first attainment is kept
            if (imp) { rec_e = E; rec_stamp = stamp; }
            if (has_best && live && rec_hit < 0 && (double)E * inv <= q.best.target) rec_hit = stamp;
            unsigned long long m = __ballot(imp);
            if (m) lane_lds_fence();
            while (m) {                                     // (only live lanes improve: rows below nrow)
                const int lr = __ffsll((long long)m) - 1;
                m &= m - 1;
                lane_column_out(lds_raw, stride, lr, q.best.state + (size_t)(row0 + lr) * n_pad, n_pad, lane);
            }
        }

        if (lane_swap_round(q, r, g, base, lane, p, decides, E, inv, a.seed_lo, a.seed_hi, lane_of_slot, slot_of_lane, slot)) {
            cb0 = scale_cb((T)a.tab[(size_t)slot * a.tab_cs], a.qinv);
            if (key_by_slot) gc = (uint32_t)((c / a.rng_ladder_len) * a.rng_stride + a.rng_base + slot);
        }
    }
    lane_lds_fence();
    for (int r = 0; r < nrow; ++r) lane_column_out(lds_raw, stride, r, a.spins + (size_t)(row0 + r) * n_pad, n_pad, lane);
    if (live) {
        a.efix[c] = E;
        if (a.energy_sink) a.energy_sink[c] = (double)E * inv;
        q.slot_of_chain[gc_chain] = slot;
        q.chain_of_slot[(size_t)g * L + slot] = (int)gc_chain;
        if (has_best) { q.best.efix[c] = rec_e; q.best.stamp[c] = rec_stamp; q.best.first_hit[c] = rec_hit; }
    }
}
