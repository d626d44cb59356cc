// nlmc_lanes.h -- chain-per-lane sweeps for short chains (n <= NLMC_LANE_N), gfx950 / wave64.
//
// The LDS kernels (k_sweep_philox, k_sweep_fused) give a chain a workgroup and find their parallelism inside a sweep: spins of one
// level are updated together.  A complete graph has one spin per level, a chain of 40 spins then occupies a compute unit for 40
// barrier rounds with one lane at work.  Here a LANE owns a chain: the 64 chains of a wave walk the same sequential sweep in lock
// step, so a sweep is sequential by construction -- no level schedule, no barrier, no atomic, no wait.  The results are those of the
// spec (oracle.sweeps_philox: a pure function of seed, global chain id, sweep, spin) and therefore of the other kernels, bit for bit.
//
//   k_lane_orders : one workgroup per order.  perm[o][i] = spin visited i-th, by the key and tie rule of k_levelize.
//   k_sweep_lanes : workgroup = one wave, lane l of block b owns row 64 b + l of the call.  The spins (and phase flags) of the 64
//                   chains sit transposed in LDS, byte (spin j, lane l) at j * stride + l: in the shared order all lanes read the
//                   same spin, 64 consecutive bytes.  In the shared order the visited spin is wave-uniform, its CSR row is read
//                   through uniform addresses (scalar loads) and the row loop has a uniform trip count; in the per-chain order the
//                   row walk is a per-lane loop (the instance is a few KB and stays in cache).
#pragma once
#include "nlmc_kernels.h"
#include "nlmc_lane_order.h"
#include <type_traits>



#ifndef NLMC_LANE_STRIDE
#define NLMC_LANE_STRIDE 64       // LDS bytes between consecutive spins of the transposed state: a compile-time constant, so that a spin's
#endif                            // address is a shift (a padded stride, e.g. -DNLMC_LANE_STRIDE=68, makes the transposes conflict-free)

struct LaneOrderArgs {
    int n, n_sweeps, per_chain, chain_base;      // order id o = c * n_sweeps + t (group chain_base + c + 1), or o = t (group 0)
    uint32_t seed_lo, seed_hi, sweep0;
    uint16_t *perm;                              // [n_orders][n]
};

__global__ __launch_bounds__(256) void k_lane_orders(LaneOrderArgs a)
{
    __shared__ uint32_t key[NLMC_LANE_N];
    const int n = a.n, tid = threadIdx.x;
    const size_t o = blockIdx.x;
    const uint32_t t = a.sweep0 + (uint32_t)(a.per_chain ? (o % (size_t)a.n_sweeps) : o);
    const uint32_t grp = a.per_chain ? (uint32_t)(a.chain_base + (int)(o / (size_t)a.n_sweeps) + 1) : 0u;
    for (int k = tid; k < n; k += 256) key[k] = philox4x32_10((uint32_t)k, t, grp, NLMC_TAG_ORDER, a.seed_lo, a.seed_hi).x;
    __syncthreads();
    uint16_t *perm = a.perm + o * (size_t)n;
    for (int k = tid; k < n; k += 256) perm[nlmc_lane_rank(key, n, k)] = (uint16_t)k;     // ranks are a permutation: in range
}

// The workgroup is ONE wave: its LDS accesses execute in program order, so a lane may read what another lane wrote before it without
// a barrier.  The fence keeps the compiler from moving LDS accesses across the points where lanes read each other's columns.
__device__ __forceinline__ void lane_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Read-only data of the launch (CSR arrays, visiting orders) through the constant address space: where the address is wave-uniform
// (shared order: the visited spin and its row are) the load is a scalar load, which the compiler does not dare for a plain global
// pointer once the kernel has stored to global memory.  Nothing in the launch writes these arrays.
template <bool UNIFORM, typename U> __device__ __forceinline__ U lane_ro(const U *p)
{
    if constexpr (UNIFORM) return *(const U __attribute__((address_space(4))) *)(p);
    else return *p;
}

// word k & 3 of a Philox call
__device__ __forceinline__ uint32_t lane_word(const u32x4 &r, int k)
{
    const int q = k & 3;
    return q == 0 ? r.x : q == 1 ? r.y : q == 2 ? r.z : r.w;
}

// column `r` of a transposed LDS array (the n_pad bytes of one chain) <-> n_pad consecutive bytes in global memory, four at a time
// (n_pad is a multiple of 16 and the rows of the state arrays are 16-byte aligned)
__device__ __forceinline__ void lane_column_in(uint8_t *lds, int stride, int r, const void *src, int n_pad, int lane)
{
    const uint32_t *s4 = reinterpret_cast<const uint32_t *>(src);
    for (int j4 = lane; j4 < n_pad / 4; j4 += 64) {
        const uint32_t w = s4[j4];
#pragma unroll
        for (int q = 0; q < 4; ++q) lds[(4 * j4 + q) * stride + r] = (uint8_t)(w >> (8 * q));
    }
}
__device__ __forceinline__ void lane_column_out(const uint8_t *lds, int stride, int r, void *dst, int n_pad, int lane)
{
    uint32_t *d4 = reinterpret_cast<uint32_t *>(dst);
    for (int j4 = lane; j4 < n_pad / 4; j4 += 64) {
        uint32_t w = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) w |= (uint32_t)lds[(4 * j4 + q) * stride + r] << (8 * q);
        d4[j4] = w;
    }
}

// The field of spin k from its CSR row, for the lane's chain (column `lane` of the transposed spins).  UNI: the row is wave-uniform.
// DIAG: the instance has diagonal entries; their term is also summed on its own (it is left out of the energy delta).
// fp64 (update_spin<double>): entries in CSR order from 0, one fma each.
template <bool UNI, bool DIAG>
__device__ __forceinline__ void lane_field(const CsrDev &g, const int8_t *s, int lane, int k, int rs, int re, double &xs, double &xd)
{
    xs = 0.0; xd = 0.0;
#pragma unroll 4
    for (int e = rs; e < re; ++e) {
        const int j = lane_ro<UNI>(g.col + e);
        const double v = lane_ro<UNI>(g.val64 + e), sj = (double)s[j * NLMC_LANE_STRIDE + lane];
        xs = fma_rn(v, sj, xs);
        if (DIAG && j == k) xd = fma_rn(v, sj, xd);
    }
}
// fixed point (update_spin_q): an exact int32 whatever the order of the sum.  X starts at hq_k.
template <bool UNI, bool DIAG>
__device__ __forceinline__ void lane_field(const CsrDev &g, const int8_t *s, int lane, int k, int rs, int re, int &X, int &Xd)
{
    Xd = 0;
#pragma unroll 4
    for (int e = rs; e < re; ++e) {
        const unsigned long long w = lane_ro<UNI>(reinterpret_cast<const unsigned long long *>(g.edge32 + e));   // EdgeQ { col, q }
        const int j = (int)(uint32_t)w, q = (int)(uint32_t)(w >> 32);
        const int tm = __mul24(q, (int)s[j * NLMC_LANE_STRIDE + lane]);
        X += tm;
        if (DIAG && j == k) Xd += tm;
    }
}

// Random numbers of sweep tt of chain gc into the lane's column of the table, one Philox call per four spins: f32 the logistic
// thresholds, f64 the UNIFORM words (the 27 high bits of u; the UNIFORM_LO call is made at the update).  (The table has
// (n + 3) / 4 * 4 rows.)
template <bool F64>
__device__ __forceinline__ void lane_fill_rtab(uint32_t *rtab, int n, int lane, uint32_t tt, uint32_t gc, uint32_t seed_lo, uint32_t seed_hi)
{
    for (int b = 0; b < (n + 3) / 4; ++b) {
        const u32x4 r = philox4x32_10((uint32_t)b, tt, gc, NLMC_TAG_UNIFORM, seed_lo, seed_hi);
        uint32_t *d = rtab + (size_t)(4 * b) * 64 + lane;
        if (F64) { d[0] = r.x; d[64] = r.y; d[128] = r.z; d[192] = r.w; }
        else {
            d[0] = __float_as_uint(threshold_spec(r.x)); d[64] = __float_as_uint(threshold_spec(r.y));
            d[128] = __float_as_uint(threshold_spec(r.z)); d[192] = __float_as_uint(threshold_spec(r.w));
        }
    }
}

// The update of spin k of the lane's chain in sweep tt, as k_sweep_lanes writes it out (k_nmc_phases_lanes; k_sweep_lanes, k_rounds_lanes
// and k_apt_rounds_lanes keep their own text: sharing this body cost them speed): phase flag f (1: cb1, >= 2: the spin keeps
// its value and adds no energy), random numbers from the table where there is one (rtab), else a Philox call.  The energy delta goes to
// e_loc.  UNI: k is wave-uniform.
template <bool F64, bool UNI, typename T>
__device__ __forceinline__ void lane_update(const SweepArgs &a, int8_t *s, const uint32_t *rtab, int lane, int k, unsigned f, uint32_t tt,
                                            uint32_t gc, T cb0, T cb1, double esc, long long &e_loc)
{
    constexpr int stride = NLMC_LANE_STRIDE;
    const int so = (int)s[k * stride + lane];
    const int rs = lane_ro<UNI>(a.g.rowptr + k), re = lane_ro<UNI>(a.g.rowptr + k + 1);
    const uint32_t hi = rtab ? rtab[(size_t)k * 64 + lane]
                             : (F64 ? lane_word(philox4x32_10((uint32_t)(k >> 2), tt, gc, NLMC_TAG_UNIFORM, a.seed_lo, a.seed_hi), k)
                                    : __float_as_uint(threshold_spec(lane_word(philox4x32_10((uint32_t)(k >> 2), tt, gc, NLMC_TAG_UNIFORM, a.seed_lo, a.seed_hi), k))));
    int sn;
    long long de;
    if constexpr (F64) {
        double xs, xd;                               // xd: the diagonal term, left out of the energy delta
        if (a.lane_diag) lane_field<UNI, true>(a.g, s, lane, k, rs, re, xs, xd);
        else lane_field<UNI, false>(a.g, s, lane, k, rs, re, xs, xd);
        const double hk = lane_ro<UNI>(a.g.h64 + k);
        const double x_true = (xs - xd) + hk, xf = xs + hk;
        const uint32_t lo = lane_word(philox4x32_10((uint32_t)(k >> 2), tt, gc, NLMC_TAG_UNIFORM_LO, a.seed_lo, a.seed_hi), k);
        const double z = (f == 1u ? cb1 : cb0) * xf;
        sn = accept_up(uniform53_spec(hi, lo), z) ? 1 : -1;
        de = (sn != so) ? fixed_delta_slow(x_true, sn - so, esc) : 0ll;
    } else {
        int X = lane_ro<UNI>(a.g.hq + k), Xd;
        if (a.lane_diag) lane_field<UNI, true>(a.g, s, lane, k, rs, re, X, Xd);
        else lane_field<UNI, false>(a.g, s, lane, k, rs, re, X, Xd);
        const float z = (f == 1u ? cb1 : cb0) * (float)X;
        sn = (z < __uint_as_float(hi)) ? 1 : -1;
        de = (long long)(X - Xd) * (long long)((so - sn) * (1 << a.eshift));
    }
    if (f < 2u) {                                    // frozen spins keep their value
        e_loc += de;
        s[k * stride + lane] = (int8_t)sn;
    }
}

// F64: the fp64 mode (update_spin<double>), else the fixed-point "f32" mode (update_spin_q).  PER_CHAIN: every chain has its own
// visiting order.  Phase flags, diagonal entries, outputs, temperature source and chain subset are runtime branches, wave-uniform
// or plain per-lane predicates.  SweepArgs fields of this kernel: lane_perm, lane_rows, lane_tab, lane_diag; lds_flags_off,
// lds_u_off (the random-number table).
template <bool F64, bool PER_CHAIN>
__global__ __launch_bounds__(64) void k_sweep_lanes(SweepArgs a)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    typedef std::conditional_t<F64, double, float> T;
    const int lane = threadIdx.x;
    constexpr int stride = NLMC_LANE_STRIDE;
    constexpr bool UNI = !PER_CHAIN;                      // the visited spin is wave-uniform
    const int n = a.g.n, n_pad = a.g.n_pad;
    const int row0 = (int)blockIdx.x * 64;
    const int nrow = min(64, a.lane_rows - row0);          // rows of this wave (wave-uniform)
    const bool live = lane < nrow;
    // lanes past the last row walk the wave's first chain (valid addresses everywhere) on a zeroed LDS column and write nothing
    const int row = live ? row0 + lane : row0;
    const int c = a.chain_list ? a.chain_list[row] : row;
    int8_t *s = reinterpret_cast<int8_t *>(lds_raw);
    const uint8_t *fl = a.flags ? lds_raw + a.lds_flags_off : nullptr;
    uint32_t *rtab = a.lane_tab ? reinterpret_cast<uint32_t *>(lds_raw + a.lds_u_off) : nullptr;   // word (spin k, lane l) at k * 64 + l

    // prologue: the rows of the 64 chains, read coalesced, written transposed
    for (int r = 0; r < 64; ++r) {
        if (r < nrow) {
            const int cr = a.chain_list ? a.chain_list[row0 + r] : row0 + r;
            lane_column_in(lds_raw, stride, r, a.spins + (size_t)cr * n_pad, n_pad, lane);
            if (fl) lane_column_in(lds_raw + a.lds_flags_off, stride, r, a.flags + (size_t)cr * n_pad, n_pad, lane);
        } else {
            for (int j = lane; j < n_pad; j += 64) { lds_raw[j * stride + r] = 0; if (fl) lds_raw[a.lds_flags_off + j * stride + r] = 0; }
        }
    }
    lane_lds_fence();

    const uint32_t gc_chain = (uint32_t)(a.chain_base + c);
    const int trow = a.slot_of_chain ? a.slot_of_chain[gc_chain] : c;
    const uint32_t gc = (a.rng_stride && a.slot_of_chain) ? (uint32_t)((c / a.rng_ladder_len) * a.rng_stride + a.rng_base + trow) : gc_chain;
    const double esc = __longlong_as_double((long long)(1023 + a.escale) << 52);   // 2^escale
    long long E = a.efix[c], e_loc = 0;
    long long Emin = a.emin ? a.emin[c] : 0;
    int amin = a.emin ? a.argmin[c] : 0;
    const bool per_sweep = (a.etrace != nullptr) || (a.emin != nullptr);
    const int n_rec = a.strace ? (a.trace_sweeps + a.rec_stride - 1) / a.rec_stride : 0;

    for (int t = 0; t < a.n_sweeps; ++t) {
        const uint32_t tt = a.sweep0 + (uint32_t)t;
        const T cb0 = scale_cb((T)a.tab[(size_t)trow * a.tab_cs + (size_t)t * a.tab_ss], a.qinv);
        const T cb1 = scale_cb((T)a.tab[(size_t)trow * a.tab_cs + (size_t)t * a.tab_ss + 1], a.qinv);
        const uint16_t *pp = a.lane_perm + (PER_CHAIN ? ((size_t)row * a.n_sweeps + t) : (size_t)t) * (size_t)n;

        // random numbers of the sweep, one Philox call per four spins of the chain: f32 the logistic thresholds, f64 the UNIFORM words
        // (the 27 high bits of u; the UNIFORM_LO call is made at the update).  Without the table the call is made at every update.
        if (rtab) {
            for (int b = 0; b < (n + 3) / 4; ++b) {
                const u32x4 r = philox4x32_10((uint32_t)b, tt, gc, NLMC_TAG_UNIFORM, a.seed_lo, a.seed_hi);
                uint32_t *d = rtab + (size_t)(4 * b) * 64 + lane;              // (the table has (n + 3) / 4 * 4 rows)
                if (F64) { d[0] = r.x; d[64] = r.y; d[128] = r.z; d[192] = r.w; }
                else {
                    d[0] = __float_as_uint(threshold_spec(r.x)); d[64] = __float_as_uint(threshold_spec(r.y));
                    d[128] = __float_as_uint(threshold_spec(r.z)); d[192] = __float_as_uint(threshold_spec(r.w));
                }
            }
        }

        for (int i0 = 0; i0 < n; i0 += 64) {
            // shared order: 64 entries of the order in one coalesced load, handed out lane by lane as scalars
            int kv = 0;
            if (!PER_CHAIN) kv = (i0 + lane < n) ? (int)pp[i0 + lane] : 0;
            const int ni = min(64, n - i0);
            for (int ii = 0; ii < ni; ++ii) {
                const int k = PER_CHAIN ? (int)pp[i0 + ii] : __builtin_amdgcn_readlane(kv, ii);
                const unsigned f = fl ? (unsigned)fl[k * stride + lane] : 0u;
                const int so = (int)s[k * stride + lane];
                const int rs = lane_ro<UNI>(a.g.rowptr + k), re = lane_ro<UNI>(a.g.rowptr + k + 1);
                const uint32_t hi = rtab ? rtab[(size_t)k * 64 + lane]
                                         : (F64 ? lane_word(philox4x32_10((uint32_t)(k >> 2), tt, gc, NLMC_TAG_UNIFORM, a.seed_lo, a.seed_hi), k)
                                                : __float_as_uint(threshold_spec(lane_word(philox4x32_10((uint32_t)(k >> 2), tt, gc, NLMC_TAG_UNIFORM, a.seed_lo, a.seed_hi), k))));
                int sn;
                long long de;
                if constexpr (F64) {
                    double xs, xd;                               // xd: the diagonal term, left out of the energy delta
                    if (a.lane_diag) lane_field<UNI, true>(a.g, s, lane, k, rs, re, xs, xd);
                    else lane_field<UNI, false>(a.g, s, lane, k, rs, re, xs, xd);
                    const double hk = lane_ro<UNI>(a.g.h64 + k);
                    const double x_true = (xs - xd) + hk, xf = xs + hk;
                    const uint32_t lo = lane_word(philox4x32_10((uint32_t)(k >> 2), tt, gc, NLMC_TAG_UNIFORM_LO, a.seed_lo, a.seed_hi), k);
                    const double z = (f == 1u ? cb1 : cb0) * xf;
                    sn = accept_up(uniform53_spec(hi, lo), z) ? 1 : -1;
                    de = (sn != so) ? fixed_delta_slow(x_true, sn - so, esc) : 0ll;
                } else {
                    int X = lane_ro<UNI>(a.g.hq + k), Xd;
                    if (a.lane_diag) lane_field<UNI, true>(a.g, s, lane, k, rs, re, X, Xd);
                    else lane_field<UNI, false>(a.g, s, lane, k, rs, re, X, Xd);
                    const float z = (f == 1u ? cb1 : cb0) * (float)X;
                    sn = (z < __uint_as_float(hi)) ? 1 : -1;
                    de = (long long)(X - Xd) * (long long)((so - sn) * (1 << a.eshift));
                }
                if (f < 2u) {                                    // frozen spins keep their value
                    e_loc += de;
                    s[k * stride + lane] = (int8_t)sn;
                }
            }
        }

        // end of the sweep (sweep_epilogue): energy trace, running minimum + its state, recorded configurations
        const int tg = a.t0 + t;
        if (per_sweep) {
            E += e_loc;
            e_loc = 0;
            const bool better = a.emin && E < Emin && (tg % a.min_stride == 0);      // strict <: the first argmin
            if (better) { Emin = E; amin = tg; }
            if (a.etrace && live) a.etrace[(size_t)row * a.trace_sweeps + tg] = E;
            if (a.best) {
                lane_lds_fence();
                unsigned long long m = __ballot(better && live);
                while (m) {                                      // wave-uniform: 64 lanes write consecutive spins of one chain
                    const int r = __builtin_ctzll(m);
                    m &= m - 1;
                    const int cr = a.chain_list ? a.chain_list[row0 + r] : row0 + r;
                    lane_column_out(lds_raw, stride, r, a.best + (size_t)cr * n_pad, n_pad, lane);
                }
            }
        }
        if (a.strace && (tg % a.rec_stride == 0)) {
            lane_lds_fence();
            for (int r = 0; r < nrow; ++r) {
                int8_t *dst = a.strace + ((size_t)(row0 + r) * n_rec + (size_t)(tg / a.rec_stride)) * n;
                for (int j = lane; j < n; j += 64) dst[j] = s[j * stride + r];
            }
        }
    }
    if (!per_sweep) E += e_loc;

    lane_lds_fence();
    for (int r = 0; r < nrow; ++r) {
        const int cr = a.chain_list ? a.chain_list[row0 + r] : row0 + r;
        lane_column_out(lds_raw, stride, r, a.spins + (size_t)cr * n_pad, n_pad, lane);
    }
    if (live) {
        a.efix[c] = E;
        if (a.energy_sink) a.energy_sink[c] = (double)E * __longlong_as_double((long long)(1023 - a.escale) << 52);
        if (a.emin) { a.emin[c] = Emin; a.argmin[c] = amin; }
    }
}
