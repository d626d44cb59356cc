// nlmc_wave_long_nmc.h -- the NMC phase cycles of dense chains of NLMC_WAVE_N < n <= NLMC_WAVE_LONG_N spins in one wave launch: a chain
// per wave (gfx950 / wave64).
//
// k_nmc_phases_waves (csrc/nlmc_wave_nmc.h) runs the phases of a round's marked chains in one launch for chains of at most 256 spins;
// this is the same phase frame around the update of k_sweep_waves_long (csrc/nlmc_waves_long.h), whose phase loop pays, per phase,
// k_adopt_best, k_phase_flags, k_fill_min, k_lane_orders and a k_sweep_waves_long launch that rebuilds the resident fields from n rows
// of the dense matrix and writes the best state to global memory on every improving sweep.  The fixed-point field is an exact int32
// whatever the order of the sum, so the fields of the best state are kept in registers (Xb beside X: 2 R of the 128 a lane has) and
// the argmin hand-off between two phases is a register copy plus the write-back of the LDS copy.  The best state's spins and the
// backbone mask are two more byte planes of the wave's LDS region (nlmc_wave_long_nmc_region).
//
//   launch : k_sweep_waves_long's (nlmc_wave_long_nmc_shape): workgroup = W waves = W rows of the selected subset, R = 8 / 16 fields
//            per lane, matrix rows from global memory.  No workgroup barrier, no atomic; a wave without a row leaves at once.
//   phase  : adopt the previous phase's minimum (k_adopt_best: s <- s_best, X <- X_best, E <- Emin), reset the running minimum
//            (k_fill_min), write the flag plane from the mask plane (k_phase_flags' rule), S sweeps of k_sweep_waves_long's update in
//            the shared order, after every sweep its rule for the running minimum, with the state and its fields copied inside the
//            wave; then the phase's minimum and argmin go out.  No global write inside the phase loop but those two.
// Same bits as the call sequence on any route; the context's flags array is neither read nor written.
#pragma once
#include "nlmc_waves_long.h"
#include "nlmc_nmc_frame.h"

// SweepArgs fields of this kernel: those of k_nmc_phases_waves.
template <int R, bool AHEAD>
__global__ __launch_bounds__(1024) void k_nmc_phases_waves_long(SweepArgs a, NmcPhasesArgs q)
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

    const NlmcWaveLongNmcRegion G = nlmc_wave_long_nmc_region(n, n_pad);
    unsigned char *reg = lds_raw + (size_t)wv * (size_t)G.bytes;
    int32_t *Xl = reinterpret_cast<int32_t *>(reg);
    float *Wl = reinterpret_cast<float *>(reg + G.sweep.w_off);
    int8_t *sl = reinterpret_cast<int8_t *>(reg + G.sweep.s_off);
    int8_t *fl = reinterpret_cast<int8_t *>(reg + G.sweep.f_off);
    int8_t *bl = reinterpret_cast<int8_t *>(reg + G.b_off);
    const uint8_t *ml = reinterpret_cast<const uint8_t *>(reg + G.m_off);
    const int n4 = n_pad / 4;                                      // n_pad is a multiple of 16, the state rows are 16-byte aligned

    // spins and mask of the chain into LDS, four bytes at a time; a launch that continues a call starts from the best state the
    // launch before it left.  The padding bytes travel with the spins and are never visited.  The best plane starts as the spins:
    // sweep 0 of a phase always improves, so it is whole before a hand-off or the epilogue reads it either way.
    {
        const uint32_t *s4 = reinterpret_cast<const uint32_t *>(nmc_state_in(a, q) + (size_t)c * n_pad);
        const uint32_t *m4 = reinterpret_cast<const uint32_t *>(q.mask + (size_t)c * n_pad);
        for (int j4 = lane; j4 < n4; j4 += 64) {
            const uint32_t v = s4[j4];
            reinterpret_cast<uint32_t *>(sl)[j4] = v;
            reinterpret_cast<uint32_t *>(bl)[j4] = v;
            reinterpret_cast<uint32_t *>(reg + G.m_off)[j4] = m4[j4];
        }
    }
    wave_long_fence();

    int X[R], Xb[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = lane + 64 * r;
        X[r] = j < n ? a.g.hq[j] : 0;
    }
    auto load_row = [&](int (&d)[R], int k) {
#pragma unroll
        for (int r = 0; r < R; ++r) d[r] = Jg[(size_t)k * JS + lane + 64 * r];
    };
    // prologue: X_j = hq_j + sum_i Jd[i][j] s_i, row by row, once per launch
#pragma unroll 2
    for (int i = 0; i < n; ++i) {
        const int si = (int)sl[i];
        int Jr[R];
        load_row(Jr, i);
#pragma unroll
        for (int p = 0; p < R; ++p) X[p] += Jr[p] * si;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        Xl[lane + 64 * r] = X[r];                                  // (the region has a word per lane and register)
        Xb[r] = X[r];
    }
    wave_long_fence();

    const uint32_t gc = (uint32_t)(a.chain_base + c);
    const float cb0 = wave_long_uniform(scale_cb((float)q.cb0, a.qinv)), cb1 = wave_long_uniform(scale_cb((float)q.cb1, a.qinv));
    long long E = uniform64(nmc_energy_in(a, q, c));
    long long Emin = 0;
    int amin = 0;
    const int nblk = (n + 3) / 4;                                  // <= 256: lane l makes the Philox calls of blocks l, l + 64, ..

    for (int p = 0; p < q.n_phases; ++p) {
        const unsigned kind = nmc_phase_kind(q, p);
        if (p > 0) {                                               // k_adopt_best: spins <- best, fields <- its fields, tracked energy <- the minimum
#pragma unroll
            for (int r = 0; r < R; ++r) {
                X[r] = Xb[r];
                Xl[lane + 64 * r] = X[r];
            }
            for (int j4 = lane; j4 < n4; j4 += 64) reinterpret_cast<uint32_t *>(sl)[j4] = reinterpret_cast<const uint32_t *>(bl)[j4];
            E = Emin;
        }
        Emin = 0x7FFFFFFFFFFFFFFFll;                               // k_fill_min
        amin = 0;
        for (int j = lane; j < n_pad; j += 64) fl[j] = (int8_t)nmc_phase_flag(kind, ml[j]);
        wave_long_fence();

        for (int t = 0; t < a.n_sweeps; ++t) {
            const int idx = p * a.n_sweeps + t;
            const uint32_t tt = a.sweep0 + (uint32_t)idx;
            const uint16_t *pp = a.lane_perm + (size_t)idx * (size_t)n;
            long long e_loc = 0;

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
                    if constexpr (AHEAD) {                           // the next visited spin's row, in flight while k is decided
                        const int kn = __builtin_amdgcn_readlane(kv, min(ii + 1, ni - 1));
                        load_row(Jn, kn);
                        Jnn = Jg[(size_t)kn * JS + kn];
                    }
                    // four broadcast reads of the wave's own region in flight together, then scalars.  The decision is made for frozen
                    // spins too and dropped: a branch on the flag first would put a second LDS round trip behind it.  With the best
                    // state's fields live across the loop the scheduler otherwise issues the reads one by one through one register,
                    // each behind a wait (+34% a sweep at R = 16): the scheduling barrier keeps the four ahead of the first use.
                    const int xv = Xl[k], sv = (int)sl[k], fv = (int)fl[k];
                    const float wv = Wl[k];
                    __builtin_amdgcn_sched_barrier(0);
                    const int Xk = __builtin_amdgcn_readfirstlane(xv), so = __builtin_amdgcn_readfirstlane(sv);
                    const int fk = __builtin_amdgcn_readfirstlane(fv);
                    const float wk = wave_long_uniform(wv);
                    const float z = (fk == 1 ? cb1 : cb0) * (float)Xk;
                    const int sn = (z < wk) ? 1 : -1;
                    if (fk < 2 && sn != so) {                        // frozen spins keep their value and add nothing
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
                        wave_long_fence();                           // the write-back stays ahead of the next update's reads
                    }
                    if constexpr (AHEAD) {
#pragma unroll
                        for (int r = 0; r < R; ++r) Jc[r] = Jn[r];
                        Jkk = Jnn;
                    }
                }
            }

            // end of the sweep: k_sweep_waves_long's running minimum (t counts from 0 within the phase), its state and -- here -- its
            // fields, all inside the wave
            if (nmc_sweep_end(E, e_loc, Emin, amin, t, a.min_stride)) {              // wave-uniform
#pragma unroll
                for (int r = 0; r < R; ++r) Xb[r] = X[r];
                for (int j4 = lane; j4 < n4; j4 += 64) reinterpret_cast<uint32_t *>(bl)[j4] = reinterpret_cast<const uint32_t *>(sl)[j4];
                wave_long_fence();
            }
        }
        if (lane == 0) nmc_phase_out(q, row, p, Emin, amin);
    }

    // epilogue: the last phase's final state (no adoption), its best state, the tracked energy and the minimum
    {
        uint32_t *s4 = reinterpret_cast<uint32_t *>(a.spins + (size_t)c * n_pad);
        uint32_t *b4 = reinterpret_cast<uint32_t *>(a.best + (size_t)c * n_pad);
        for (int j4 = lane; j4 < n4; j4 += 64) {
            s4[j4] = reinterpret_cast<const uint32_t *>(sl)[j4];
            b4[j4] = reinterpret_cast<const uint32_t *>(bl)[j4];
        }
    }
    if (lane == 0) nmc_chain_out(a, c, E, Emin, amin);
}
