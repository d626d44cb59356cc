// nlmc_waves_long.h -- wave-per-chain sweeps with resident local fields for dense chains of NLMC_WAVE_N < n <= NLMC_WAVE_LONG_N spins,
// gfx950 / wave64.
//
// k_sweep_waves (csrc/nlmc_waves.h) ends at 256 spins: the decision for the visited spin k reads lane k & 63's register k >> 6
// through v_readlane and a select tree, which four registers a lane allow and sixteen do not.  Here lane l still owns the fields of
// the spins l, l + 64, .. in registers (R = 8 for n <= 512, 16 beyond), and every flip writes them through to a copy in LDS that the
// wave keeps to itself next to the spins, the phase flags and the sweep's thresholds (nlmc_wave_long_region).  An update is then four
// broadcast LDS reads in flight together and one compare, a flip R adds per lane on row k of the dense matrix plus the write-back.
// Fixed point ("f32") only: the int32 field is exact whatever the order of the sum.  From X on the operations are update_spin_q's,
// so the bits are the spec's.
//
// No workgroup barrier, no atomic, no level schedule.  A wave's LDS accesses execute in program order, so what a lane wrote is what
// any lane of the wave reads next; wave_long_fence keeps the compiler from moving LDS accesses across the points where lanes read
// each other's words (wavefront scope: an order for the compiler, no wait for the hardware).
//
// The registers are kept beside the LDS copy because a flip would otherwise read, add and write R words per lane where it now adds
// and writes them; the spins and flags live in LDS only (one lane writes a flipped spin).
//
// AHEAD: the row of the NEXT visited spin is requested before the current one is decided, as k_sweep_waves does (4 R 64 bytes per
// update and wave, whether the spin flips or not); otherwise the row is requested on a flip only.  NLMC_WAVE_LONG_AHEAD picks
// (DESIGN.md section 6 has the measurements).
#pragma once
#include "nlmc_waves.h"
#include "nlmc_wave_shape.h"

#ifndef NLMC_WAVE_LONG_AHEAD_DEFAULT
#define NLMC_WAVE_LONG_AHEAD_DEFAULT 0    // what NLMC_WAVE_LONG_AHEAD is when unset: the faster variant of the measurements
#endif

__device__ __forceinline__ void wave_long_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float wave_long_uniform(float x)
{
    return __int_as_float(__builtin_amdgcn_readfirstlane((int)__float_as_uint(x)));
}

// SweepArgs fields of this kernel: those of k_sweep_waves.  The matrix rows come from global memory (row stride 64 R ints, columns
// past n zero), so a lane's R columns are always inside the row.
template <int R, bool AHEAD>
__global__ __launch_bounds__(1024) void k_sweep_waves_long(SweepArgs a)
{
    static_assert(R == 8 || R == 16, "eight or sixteen registers");
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int JS = 64 * R;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), W = (int)(blockDim.x >> 6);
    const int n = a.g.n, n_pad = a.g.n_pad;
    const int32_t *Jg = a.wave_J;
    const int row = (int)blockIdx.x * W + wv;                      // wave-uniform
    if (row >= a.lane_rows) return;                                // (no barrier anywhere: a wave without a row just leaves)
    const int c = __builtin_amdgcn_readfirstlane(a.chain_list ? a.chain_list[row] : row);

    const NlmcWaveLongRegion G = nlmc_wave_long_region(n, n_pad);
    unsigned char *reg = lds_raw + (size_t)wv * (size_t)G.bytes;
    int32_t *Xl = reinterpret_cast<int32_t *>(reg);
    float *Wl = reinterpret_cast<float *>(reg + G.w_off);
    int8_t *sl = reinterpret_cast<int8_t *>(reg + G.s_off);
    int8_t *fl = reinterpret_cast<int8_t *>(reg + G.f_off);

    // spins and flags of the chain into LDS, four bytes at a time (n_pad is a multiple of 16, the state rows are 16-byte aligned);
    // the padding bytes travel with the spins and are never visited
    {
        const uint32_t *s4 = reinterpret_cast<const uint32_t *>(a.spins + (size_t)c * n_pad);
        const uint32_t *f4 = a.flags ? reinterpret_cast<const uint32_t *>(a.flags + (size_t)c * n_pad) : nullptr;
        for (int j4 = lane; j4 < n_pad / 4; j4 += 64) {
            reinterpret_cast<uint32_t *>(sl)[j4] = s4[j4];
            reinterpret_cast<uint32_t *>(fl)[j4] = f4 ? f4[j4] : 0u;
        }
    }
    wave_long_fence();

    int X[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = lane + 64 * r;
        X[r] = j < n ? a.g.hq[j] : 0;
    }
    auto load_row = [&](int (&d)[R], int k) {
#pragma unroll
        for (int r = 0; r < R; ++r) d[r] = Jg[(size_t)k * JS + lane + 64 * r];
    };
    // prologue: X_j = hq_j + sum_i Jd[i][j] s_i, row by row
#pragma unroll 2
    for (int i = 0; i < n; ++i) {
        const int si = (int)sl[i];
        int Jr[R];
        load_row(Jr, i);
#pragma unroll
        for (int q = 0; q < R; ++q) X[q] += Jr[q] * si;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) Xl[lane + 64 * r] = X[r];          // (the region has a word per lane and register)
    wave_long_fence();

    const uint32_t gc_chain = (uint32_t)(a.chain_base + c);
    const int trow = a.slot_of_chain ? a.slot_of_chain[gc_chain] : c;
    const uint32_t gc = (a.rng_stride && a.slot_of_chain) ? (uint32_t)((c / a.rng_ladder_len) * a.rng_stride + a.rng_base + trow) : gc_chain;
    long long E = uniform64(a.efix[c]), e_loc = 0;
    long long Emin = a.emin ? uniform64(a.emin[c]) : 0;
    int amin = a.emin ? __builtin_amdgcn_readfirstlane(a.argmin[c]) : 0;
    const bool per_sweep = (a.etrace != nullptr) || (a.emin != nullptr);
    const int n_rec = a.strace ? (a.trace_sweeps + a.rec_stride - 1) / a.rec_stride : 0;
    const int nblk = (n + 3) / 4;                                  // <= 256: lane l makes the Philox calls of blocks l, l + 64, ..

    for (int t = 0; t < a.n_sweeps; ++t) {
        const uint32_t tt = a.sweep0 + (uint32_t)t;
        // (wave-uniform, and made scalars here so that the conversion from double stays out of the update loop)
        const float cb0 = wave_long_uniform(scale_cb((float)a.tab[(size_t)trow * a.tab_cs + (size_t)t * a.tab_ss], a.qinv));
        const float cb1 = wave_long_uniform(scale_cb((float)a.tab[(size_t)trow * a.tab_cs + (size_t)t * a.tab_ss + 1], a.qinv));
        const uint16_t *pp = a.lane_perm + (a.per_chain ? ((size_t)row * a.n_sweeps + t) : (size_t)t) * (size_t)n;

        // the sweep's thresholds: those of spins 4 b .. 4 b + 3 from one call
        for (int b = lane; b < nblk; b += 64) {
            const u32x4 rr = philox4x32_10((uint32_t)b, tt, gc, NLMC_TAG_UNIFORM, a.seed_lo, a.seed_hi);
            float4 w4;
            w4.x = threshold_spec(rr.x); w4.y = threshold_spec(rr.y); w4.z = threshold_spec(rr.z); w4.w = threshold_spec(rr.w);
            reinterpret_cast<float4 *>(Wl)[b] = w4;
        }
        wave_long_fence();

        for (int i0 = 0; i0 < n; i0 += 64) {
            // 64 entries of the order in one coalesced load, handed out as scalars
            const int kv = (i0 + lane < n) ? (int)pp[i0 + lane] : 0;
            const int ni = min(64, n - i0);
            int Jc[R], Jkk = 0;
            if constexpr (AHEAD) {
                const int k0 = __builtin_amdgcn_readlane(kv, 0);
                load_row(Jc, k0);
                Jkk = Jg[(size_t)k0 * JS + k0];
            }
            for (int ii = 0; ii < ni; ++ii) {
                const int k = __builtin_amdgcn_readlane(kv, ii);
                int Jn[R], Jnn = 0;
                if constexpr (AHEAD) {                               // the next visited spin's row, in flight while k is decided
                    const int kn = __builtin_amdgcn_readlane(kv, min(ii + 1, ni - 1));
                    load_row(Jn, kn);
                    Jnn = Jg[(size_t)kn * JS + kn];
                }
                // four broadcast reads of the wave's own region in flight together, then scalars.  The decision is made for frozen
                // spins too and dropped: a branch on the flag first would put a second LDS round trip behind it.
                const int Xk = __builtin_amdgcn_readfirstlane(Xl[k]), so = __builtin_amdgcn_readfirstlane((int)sl[k]);
                const int fk = __builtin_amdgcn_readfirstlane((int)fl[k]);
                const float wk = wave_long_uniform(Wl[k]);
                const float z = (fk == 1 ? cb1 : cb0) * (float)Xk;
                const int sn = (z < wk) ? 1 : -1;
                if (fk < 2 && sn != so) {                            // frozen spins keep their value and add nothing
                    if constexpr (!AHEAD) {
                        load_row(Jc, k);
                        Jkk = Jg[(size_t)k * JS + k];
                    }
                    // the diagonal term stays out of the energy delta, not of the field
                    e_loc += (long long)(Xk - Jkk * so) * (long long)((so - sn) * (1 << a.eshift));
                    const int d = sn - so;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        X[r] += d * Jc[r];
                        Xl[lane + 64 * r] = X[r];
                    }
                    if (lane == 0) sl[k] = (int8_t)sn;
                    wave_long_fence();                               // the write-back stays ahead of the next update's reads
                }
                if constexpr (AHEAD) {
#pragma unroll
                    for (int r = 0; r < R; ++r) Jc[r] = Jn[r];
                    Jkk = Jnn;
                }
            }
        }

        // end of the sweep (sweep_epilogue): energy trace, running minimum + its state, recorded configurations.  The energy and the
        // minimum are wave-uniform: one lane stores them.
        const int tg = a.t0 + t;
        if (per_sweep) {
            E += e_loc;
            e_loc = 0;
            const bool better = a.emin && E < Emin && (tg % a.min_stride == 0);      // strict <: the first argmin
            if (better) { Emin = E; amin = tg; }
            if (a.etrace && lane == 0) a.etrace[(size_t)row * a.trace_sweeps + tg] = E;
            if (a.best && better) {
                uint32_t *b4 = reinterpret_cast<uint32_t *>(a.best + (size_t)c * n_pad);
                for (int j4 = lane; j4 < n_pad / 4; j4 += 64) b4[j4] = reinterpret_cast<const uint32_t *>(sl)[j4];
            }
        }
        if (a.strace && (tg % a.rec_stride == 0)) {
            int8_t *dst = a.strace + ((size_t)row * n_rec + (size_t)(tg / a.rec_stride)) * n;
#pragma unroll
            for (int r = 0; r < R; ++r) if (lane + 64 * r < n) dst[lane + 64 * r] = sl[lane + 64 * r];
        }
    }
    if (!per_sweep) E += e_loc;

    {
        uint32_t *s4 = reinterpret_cast<uint32_t *>(a.spins + (size_t)c * n_pad);
        for (int j4 = lane; j4 < n_pad / 4; j4 += 64) s4[j4] = reinterpret_cast<const uint32_t *>(sl)[j4];
    }
    if (lane == 0) {
        a.efix[c] = E;
        if (a.energy_sink) a.energy_sink[c] = (double)E * __longlong_as_double((long long)(1023 - a.escale) << 52);
        if (a.emin) { a.emin[c] = Emin; a.argmin[c] = amin; }
    }
}
