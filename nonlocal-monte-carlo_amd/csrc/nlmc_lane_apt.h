// nlmc_lane_apt.h -- APT rounds of short chains in one launch: one whole system in one workgroup (gfx950 / wave64).
//
// An APT system is K sub-replica ladders of L temperatures (chain j L + i belongs to ladder j).  k_rounds_lanes (nlmc_lane_rounds.h)
// keeps a ladder inside a wave; the Houdayer step pairs chains of DIFFERENT ladders on the same temperature slot, and after a few
// swaps any chain of one ladder can meet any chain of another.  So the K L chains share one workgroup's LDS: wave w holds ladders
// w P .. w P + P - 1 (P = 64 / L) in a region of its own, sweeps and swaps stay wave-private as in k_rounds_lanes, and the waves meet
// at a barrier only around the Houdayer step, where a LANE owns a pair (nlmc_lane_icm.h).  A round is what
// APT_ICM._run_device_resident does in one round:
//   sweeps   : the update of k_rounds_lanes<F64> operation for operation.
//   Houdayer : every chain ranks its ladder among the K keys philox(j', round, slot, ICM_PAIR) (k_icm_pair_ladders' rule) and writes
//              its column to pair_col[slot][rank]; barrier; thread p = r (K / 2) + i takes the columns ranked 2 i and 2 i + 1 of slot
//              r: components, pick, Katzgraber flip or exchange, the integer energy deltas of k_icm_round; barrier; every lane adds the
//              delta of its column to its tracked energy.  (The barrier "before" the step is the one after the pairing: the pairing
//              reads registers and writes a table nobody reads before it.)
//   swaps    : the swap round of k_rounds_lanes, unchanged.
// Same bits as nlmc_sweep_philox(beta = NULL) + nlmc_icm_round_ladders + nlmc_pt_swap_philox round by round, on any route.  No wave
// waits on memory written by another workgroup: no poll, no atomic, no cooperative launch, no fence but the barriers.
// Grid = M systems (nlmc_apt_systems), a workgroup each: workgroup b owns chains b K L .. and ladders b K .., reads and writes only their
// rows of every array, and ranks only its own K pairing keys.  Random numbers, plan and log rows stay keyed by the GLOBAL chain / ladder
// id, so workgroup 0 has the bits of a one-system launch.  No residency condition: M may exceed the number of compute units.
#pragma once
#include "nlmc_lane_rounds.h"
#include "nlmc_lane_icm.h"
#include "nlmc_pt_icm.h"

struct LaneAptArgs {
    int n_sub;                       // K, sub-replica ladders of the system
    int n_icm;                       // Houdayer pairs per round, L (K / 2): threads 0 .. n_icm - 1 own one each
    int katz;
    int32_t *info;                   // [n_rounds][gridDim.x][n_icm][2] {n_components, picked size} at the launch's first round, or nullptr
    int lds_wave_bytes;              // a wave's transposed spins: n_pad * 64
    int lds_tab_bytes;               // a wave's random-number table (SweepArgs::lds_u_off + wave * lds_tab_bytes)
    int lds_pcol_off;                // pair_col[slot][rank], 16-bit columns (wave * 64 + lane)
    int lds_de_off;                  // an 8-byte energy delta per column
    int lds_lab_off, lab_stride;     // label plane: (spin k, pair p) at k * lab_stride + p, 16 bits (may share the tables' bytes)
};

// SweepArgs / LaneRoundsArgs fields as in k_rounds_lanes; lds_map_off = the maps of wave 0 (128 bytes per wave).
// ELOG: an energy log is open (nlmc_elog_begin) -- behind the Houdayer step's energy deltas and before the swap round every live lane
// stores its energy and slot to the round's row (q.elog, rows of the context's chains).  Without ELOG the kernel is the one it was.
template <bool F64, bool ELOG = false>
__global__ __launch_bounds__(1024) void k_apt_rounds_lanes(SweepArgs a, LaneRoundsArgs q, LaneAptArgs x)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    typedef std::conditional_t<F64, double, float> T;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr int stride = NLMC_LANE_STRIDE;
    const int n = a.g.n, n_pad = a.g.n_pad;
    const int L = q.ladder_len, P = 64 / L, K = x.n_sub;
    const int lad0 = w * P;                                             // first ladder of this wave
    const int nlad = min(P, K - lad0);                                  // its ladders (wave-uniform, >= 1)
    const int row0 = lad0 * L, nrow = nlad * L;
    const bool live = lane < nrow;
    const int sys = blockIdx.x, g0 = sys * K;                           // this workgroup's system and its first ladder
    const size_t c0 = (size_t)g0 * L;                                   // its first chain: row of spins, efix, sink, slot_of_chain
    const int c = live ? row0 + lane : row0;                            // chain of the system (tail lanes: the wave's first, read only)
    const int lw = live ? lane / L : 0, base = lw * L;
    const int g = g0 + lad0 + lw;                                       // GLOBAL ladder: Philox key, rows of plan / log / chain_of_slot
    unsigned char *lds_w = lds_raw + (size_t)w * x.lds_wave_bytes;      // this wave's region
    int8_t *s = reinterpret_cast<int8_t *>(lds_w);
    uint32_t *rtab = a.lane_tab ? reinterpret_cast<uint32_t *>(lds_raw + a.lds_u_off + (size_t)w * x.lds_tab_bytes) : nullptr;
    uint8_t *lane_of_slot = lds_raw + q.lds_map_off + w * 128, *slot_of_lane = lane_of_slot + 64;
    uint16_t *pcol = reinterpret_cast<uint16_t *>(lds_raw + x.lds_pcol_off);
    long long *dEw = reinterpret_cast<long long *>(lds_raw + x.lds_de_off);
    uint16_t *lab = reinterpret_cast<uint16_t *>(lds_raw + x.lds_lab_off);

    // prologue: the rows of the wave's chains, read coalesced, written transposed
    for (int r = 0; r < 64; ++r) {
        if (r < nrow) lane_column_in(lds_w, stride, r, a.spins + (c0 + row0 + r) * n_pad, n_pad, lane);
        else for (int j = lane; j < n_pad; j += 64) lds_w[j * stride + r] = 0;
    }
    int slot = q.slot_of_chain[c0 + c];
    lane_of_slot[lane] = (uint8_t)lane;
    slot_of_lane[lane] = (uint8_t)slot;
    dEw[tid] = 0;
    lane_lds_fence();
    if (live) lane_of_slot[base + slot] = (uint8_t)lane;
    lane_lds_fence();

    const uint32_t gc = (uint32_t)(c0 + c);                             // (random numbers keyed by the global chain id)
    T cb0 = scale_cb((T)a.tab[(size_t)slot * a.tab_cs], a.qinv);
    const double esc = __longlong_as_double((long long)(1023 + a.escale) << 52);   // 2^escale
    const double inv = __longlong_as_double((long long)(1023 - a.escale) << 52);   // 2^-escale
    long long E = a.efix[c0 + c];
    const bool decides = live && (lane - base) < q.n_pairs;
    const int p = lane - base;

    for (int r = 0; r < q.n_rounds; ++r) {
        long long e_loc = 0;
        for (int t = 0; t < a.n_sweeps; ++t) {
            const uint32_t tt = a.sweep0 + (uint32_t)(r * a.n_sweeps + t);
            const uint16_t *pp = a.lane_perm + ((size_t)r * a.n_sweeps + t) * (size_t)n;
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
                const int kv = (i0 + lane < n) ? (int)pp[i0 + lane] : 0;
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
                        double xs, xd;
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
        const uint32_t round = q.round0 + (uint32_t)r;

        // the Houdayer step of nlmc_icm_round_ladders: the only place where waves read each other's columns
        if (x.n_icm > 0) {
            if (live) {
                const uint32_t kj = philox4x32_10((uint32_t)g, round, (uint32_t)slot, NLMC_TAG_ICM_PAIR, a.seed_lo, a.seed_hi).x;
                int rank = 0;                                 // position of this ladder in the shuffled order of its slot
                for (int j = g0; j < g0 + K; ++j) {
                    const uint32_t ki = philox4x32_10((uint32_t)j, round, (uint32_t)slot, NLMC_TAG_ICM_PAIR, a.seed_lo, a.seed_hi).x;
                    rank += (j != g) && ((ki < kj) || (ki == kj && j < g));
                }
                pcol[slot * K + rank] = (uint16_t)tid;        // (column id = wave * 64 + lane; ranks of a slot are a permutation)
            }
            __syncthreads();                                  // sweeps and pairing of every wave are done
            if (tid < x.n_icm) {                              // idle lanes skip the move; every thread reaches both barriers
                const int half = K / 2, rr = tid / half, i = tid - rr * half;
                const int ca = (int)pcol[rr * K + 2 * i], cb = (int)pcol[rr * K + 2 * i + 1];
                int8_t *sa = reinterpret_cast<int8_t *>(lds_raw) + (size_t)(ca >> 6) * x.lds_wave_bytes + (ca & 63);
                int8_t *sb = reinterpret_cast<int8_t *>(lds_raw) + (size_t)(cb >> 6) * x.lds_wave_bytes + (cb & 63);
                const int ls = x.lab_stride;
                uint16_t *lb = lab + tid;
                const LaneIcmGraph gg{n, a.g.rowptr, reinterpret_cast<const int32_t *>(a.g.edge32), a.g.val64};
                const LaneIcmPair pr{sa, sb, stride, lb, ls};
                const bool converged = nlmc_lane_icm_components(gg, pr);
                int ncomp = 0;
                for (int k = 0; k < n; ++k) ncomp += (int)lb[k * ls] == k;
                if (!converged) ncomp = -1;
                int root = -1, size = 0;
                if (ncomp > 0) {
                    // component number floor(u ncomp / 2^32) in ascending order of the roots, keyed by the two chain ids (k_icm_round)
                    const uint32_t ida = (uint32_t)c0 + (uint32_t)((ca >> 6) * P * L + (ca & 63)), idb = (uint32_t)c0 + (uint32_t)((cb >> 6) * P * L + (cb & 63));
                    const uint32_t u = philox4x32_10(ida, round, idb, NLMC_TAG_ICM, a.seed_lo, a.seed_hi).x;
                    const int pick = (int)(((unsigned long long)u * (unsigned long long)ncomp) >> 32);
                    int seen = 0;
                    for (int k = 0; k < n; ++k)
                        if ((int)lb[k * ls] == k) { if (seen == pick) root = k; ++seen; }
                    for (int k = 0; k < n; ++k) size += (int)lb[k * ls] == root;
                }
                const bool flip = ncomp > 0 && x.katz && size > n / 2;       // state a = -state a: the field term changes sign
                const bool exch = ncomp > 0 && !flip;                        // the component changes sides
                long long dEa = 0, dEb = 0;
                for (int k = 0; k < n; ++k) {
                    const int va = (int)sa[k * stride], vb = (int)sb[k * stride];
                    const long long hk = (long long)lane_ro<true>(a.g.hq + k);
                    if (flip) { dEa += 2ll * hk * (long long)va; sa[k * stride] = (int8_t)-va; }
                    const bool in = exch && (int)lb[k * ls] == root;
                    if (__ballot(in) == 0ull) continue;                      // wave-uniform: the row is walked where a lane needs it
                    const int rs = lane_ro<true>(a.g.rowptr + k), re = lane_ro<true>(a.g.rowptr + k + 1);
                    long long fa = hk, fb = hk;
                    for (int e = rs; e < re; ++e) {
                        const unsigned long long ew = lane_ro<true>(reinterpret_cast<const unsigned long long *>(a.g.edge32 + e));
                        const int j = (int)(uint32_t)ew, jq = (int)(uint32_t)(ew >> 32);
                        if (in && (int)lb[j * ls] != root) {                 // bonds inside the cluster (and the diagonal) keep their energy
                            fa += (long long)jq * (long long)sa[j * stride];
                            fb += (long long)jq * (long long)sb[j * stride];
                        }
                    }
                    if (in) {
                        dEa += 2ll * (long long)va * fa;
                        dEb += 2ll * (long long)vb * fb;
                        sa[k * stride] = (int8_t)vb;
                        sb[k * stride] = (int8_t)va;
                    }
                }
                dEw[ca] = dEa;
                dEw[cb] = dEb;
                if (x.info) {
                    int32_t *o = x.info + (((size_t)r * gridDim.x + sys) * x.n_icm + tid) * 2;
                    o[0] = ncomp; o[1] = size;
                }
            }
            __syncthreads();
            E += dEw[tid] * (1ll << a.eshift);
            dEw[tid] = 0;                                     // (written again only after the next round's first barrier)
        }

        if constexpr (ELOG) {
            if (live) elog_store(q.elog, r, (int)c0 + c, (double)E * inv, slot);
        }

        // the swap round of k_rounds_lanes: lane_swap_round (nlmc_lane_rounds.h) written out, as the prologue above is lane_ladders_in.
        // Calling the two here moves this kernel's register allocation and costs 1 .. 4 % a round.
        if (q.n_pairs > 0) {
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
                const bool acc = pt_swap_decide(p, i, i, Ea, Eb, q.beta, round, g, a.seed_lo, a.seed_hi);
                if (acc) {
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
            if (ns != slot) {
                slot = ns;
                cb0 = scale_cb((T)a.tab[(size_t)slot * a.tab_cs], a.qinv);
            }
        }
    }
    lane_lds_fence();
    for (int r = 0; r < nrow; ++r) lane_column_out(lds_w, stride, r, a.spins + (c0 + row0 + r) * n_pad, n_pad, lane);
    if (live) {
        a.efix[c0 + c] = E;
        if (a.energy_sink) a.energy_sink[c0 + c] = (double)E * inv;
        q.slot_of_chain[c0 + c] = slot;
        q.chain_of_slot[(size_t)g * L + slot] = (int32_t)(c0 + c);
    }
}
