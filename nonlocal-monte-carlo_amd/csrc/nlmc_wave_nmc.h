// nlmc_wave_nmc.h -- the NMC phase cycles of short dense chains (n <= NLMC_WAVE_N) in one wave launch: a chain per wave (gfx950 / wave64).
//
// k_nmc_phases_lanes (csrc/nlmc_lane_nmc.h) runs the phases of a round's marked chains in one launch on the lane shape; this is the
// same call on k_sweep_waves' shape (csrc/nlmc_waves.h), whose phase loop pays, per phase, k_adopt_best, k_phase_flags, k_fill_min,
// k_lane_orders and a k_sweep_waves launch that stages the matrix and rebuilds the resident fields in its prologue.  In the fixed-point
// mode the field X_j = hq_j + sum_i Jq_ji s_i is an exact int32 whatever the order of the sum, so the fields of the best state can be
// kept beside its spins: the argmin hand-off between two phases is a register copy, with no LDS plane, no global round trip and no
// field rebuild.
//
//   launch : k_sweep_waves' (nlmc_wave_shape): workgroup = W waves = W rows of the selected subset, R = 1 / 2 / 4 fields per lane, the
//            matrix staged in LDS up to n = NLMC_WAVE_JLDS_N behind the kernel's only barrier, else rows from global memory with the
//            next visited row requested ahead.  Waves without a row leave behind the barrier.
//   phase  : adopt the previous phase's minimum (k_adopt_best: s <- s_best, X <- X_best, E <- Emin), reset the running minimum
//            (k_fill_min), S sweeps of k_sweep_waves' update in the shared order with the flag of an owned spin computed from its mask
//            byte (k_phase_flags' rule), after every sweep k_sweep_waves' rule for the running minimum, its state and -- here -- its
//            fields; then the phase's minimum and argmin go out.
// Same bits as the call sequence on any route; the context's flags array is neither read nor written.
#pragma once
#include "nlmc_waves.h"
#include "nlmc_nmc_frame.h"

// SweepArgs fields of this kernel: graph, chain_base, chain_list, spins, efix, energy_sink, the energy scales, seed, sweep0 = the
// first sweep of the launch, n_sweeps = sweeps per phase, min_stride, emin / argmin / best (the context's arrays), lane_perm = the
// orders of all n_phases * n_sweeps sweeps of the launch, lane_rows, wave_J.  Of csrc/nlmc_nmc_frame.h this kernel takes the arguments
// and the flag rule only: with the other helpers (nmc_sweep_end alone left out, too) its R = 2 and R = 4 code measured 1.0-1.7 % slower
// at 128 and 256 spins with every register figure unchanged, so the rest of the frame stays written out here and the kernel compiles
// to the instructions it had before the frame.
template <int R, bool JLDS>
__global__ __launch_bounds__(1024) void k_nmc_phases_waves(SweepArgs a, NmcPhasesArgs q)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int JS = 64 * R;                                     // row stride of the matrix in global memory
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), W = (int)(blockDim.x >> 6);
    const int n = a.g.n, n_pad = a.g.n_pad;
    const int32_t *Jg = a.wave_J;
    const int32_t *Jl = reinterpret_cast<const int32_t *>(lds_raw);
    if constexpr (JLDS) {
        int32_t *dst = reinterpret_cast<int32_t *>(lds_raw);
        for (int k = wv; k < n; k += W)
            for (int j = lane; j < n_pad; j += 64) dst[k * n_pad + j] = Jg[(size_t)k * JS + j];
        __syncthreads();                                           // the only barrier: waves without a row leave behind it
    }
    const int row = (int)blockIdx.x * W + wv;                      // wave-uniform
    if (row >= a.lane_rows) return;
    const int c = __builtin_amdgcn_readfirstlane(a.chain_list ? a.chain_list[row] : row);

    // lane l owns spins l + 64 r, their mask bytes and, twice, their fields: of the running state and of the phase's best state.  A
    // launch that continues a call starts from the best state the launch before it left.  Padding bytes and the columns of lanes past
    // n_pad: as in k_sweep_waves.
    int jj[R], s[R], X[R], f[R], mk[R], sb[R], Xb[R];
    bool own[R];
    const int8_t *src = (q.phase0 > 0 ? a.best : a.spins) + (size_t)c * n_pad;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = lane + 64 * r;
        own[r] = j < n_pad;
        jj[r] = JLDS ? min(j, n_pad - 1) : j;
        s[r] = own[r] ? (int)src[j] : 0;
        mk[r] = own[r] ? (int)q.mask[(size_t)c * n_pad + j] : 0;
        X[r] = j < n ? a.g.hq[j] : 0;
        f[r] = 0; sb[r] = 0; Xb[r] = 0;
    }
    auto load_row = [&](int (&d)[R], int k) {
#pragma unroll
        for (int r = 0; r < R; ++r) d[r] = JLDS ? Jl[k * n_pad + jj[r]] : Jg[(size_t)k * JS + jj[r]];
    };
    // prologue: X_j = hq_j + sum_i Jd[i][j] s_i, row by row
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int ni = min(64, n - 64 * r);
        for (int ii = 0; ii < ni; ++ii) {
            const int si = __builtin_amdgcn_readlane(s[r], ii);
            int Jr[R];
            load_row(Jr, 64 * r + ii);
#pragma unroll
            for (int p = 0; p < R; ++p) X[p] += Jr[p] * si;
        }
    }

    const uint32_t gc = (uint32_t)(a.chain_base + c);
    const float cb0 = scale_cb((float)q.cb0, a.qinv), cb1 = scale_cb((float)q.cb1, a.qinv);
    long long E = uniform64(q.phase0 > 0 ? a.emin[c] : a.efix[c]);
    long long Emin = 0;
    int amin = 0;
    const int nblk = (n + 3) / 4;                                  // <= 64: lane l makes the Philox call of block l

    for (int p = 0; p < q.n_phases; ++p) {
        const unsigned kind = (q.kinds[p >> 4] >> (2 * (p & 15))) & 3u;
        if (p > 0) {                                               // k_adopt_best: spins <- best, tracked energy <- the minimum
#pragma unroll
            for (int r = 0; r < R; ++r) { s[r] = sb[r]; X[r] = Xb[r]; }
            E = Emin;
        }
        Emin = 0x7FFFFFFFFFFFFFFFll;                               // k_fill_min
        amin = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) f[r] = (int)nmc_phase_flag(kind, (unsigned)mk[r]);

        for (int t = 0; t < a.n_sweeps; ++t) {
            const int idx = p * a.n_sweeps + t;
            const uint32_t tt = a.sweep0 + (uint32_t)idx;
            const uint16_t *pp = a.lane_perm + (size_t)idx * (size_t)n;
            long long e_loc = 0;

            // the thresholds of spins 4 l .. 4 l + 3 (one call per lane and sweep)
            int Wt[4] = {0, 0, 0, 0};
            if (lane < nblk) {
                const u32x4 rr = philox4x32_10((uint32_t)lane, tt, gc, NLMC_TAG_UNIFORM, a.seed_lo, a.seed_hi);
                Wt[0] = (int)__float_as_uint(threshold_spec(rr.x)); Wt[1] = (int)__float_as_uint(threshold_spec(rr.y));
                Wt[2] = (int)__float_as_uint(threshold_spec(rr.z)); Wt[3] = (int)__float_as_uint(threshold_spec(rr.w));
            }

            for (int i0 = 0; i0 < n; i0 += 64) {
                // 64 entries of the order in one coalesced load, handed out as scalars
                const int kv = (i0 + lane < n) ? (int)pp[i0 + lane] : 0;
                const int ni = min(64, n - i0);
                int Jc[R];
                load_row(Jc, __builtin_amdgcn_readlane(kv, 0));
                for (int ii = 0; ii < ni; ++ii) {
                    const int k = __builtin_amdgcn_readlane(kv, ii);
                    int Jn[R];                                       // the next visited spin's row, in flight while k is decided
                    load_row(Jn, __builtin_amdgcn_readlane(kv, min(ii + 1, ni - 1)));
                    const int kl = k & 63, kr = k >> 6;
                    const int fk = kind != NLMC_PHASE_ALL ? wave_get<R>(f, kl, kr) : 0;
                    if (fk < 2) {                                    // frozen spins keep their value and add nothing
                        const int Xk = wave_get<R>(X, kl, kr), so = wave_get<R>(s, kl, kr);
                        const float wk = __int_as_float(wave_get<4>(Wt, k >> 2, k & 3));
                        const float z = (fk == 1 ? cb1 : cb0) * (float)Xk;
                        const int sn = (z < wk) ? 1 : -1;
                        if (sn != so) {
                            const int Jkk = wave_get<R>(Jc, kl, kr); // the diagonal term stays out of the energy delta, not of the field
                            e_loc += (long long)(Xk - Jkk * so) * (long long)((so - sn) * (1 << a.eshift));
                            const int d = sn - so;
#pragma unroll
                            for (int r = 0; r < R; ++r) {
                                X[r] += d * Jc[r];
                                s[r] = (r == kr && lane == kl) ? sn : s[r];
                            }
                        }
                    }
#pragma unroll
                    for (int r = 0; r < R; ++r) Jc[r] = Jn[r];
                }
            }

            // end of the sweep: k_sweep_waves' running minimum (t counts from 0 within the phase), its state and its fields.  Sweep 0
            // of a phase always improves, so the best registers are whole before a hand-off reads them.
            E += e_loc;
            const bool better = E < Emin && (t % a.min_stride == 0);                 // strict <: the first argmin; wave-uniform
            if (better) {
                Emin = E; amin = t;
#pragma unroll
                for (int r = 0; r < R; ++r) { sb[r] = s[r]; Xb[r] = X[r]; }
            }
        }
        if (q.phase_min && lane == 0) {
            const size_t o = (size_t)row * q.phases_total + (size_t)(q.phase0 + p);
            q.phase_min[o] = Emin;
            q.phase_argmin[o] = amin;
        }
    }

    // epilogue: the last phase's final state (no adoption), its best state, the tracked energy and the minimum
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (own[r]) {
            a.spins[(size_t)c * n_pad + lane + 64 * r] = (int8_t)s[r];
            a.best[(size_t)c * n_pad + lane + 64 * r] = (int8_t)sb[r];
        }
    if (lane == 0) {
        a.efix[c] = E;
        if (a.energy_sink) a.energy_sink[c] = (double)E * __longlong_as_double((long long)(1023 - a.escale) << 52);
        a.emin[c] = Emin;
        a.argmin[c] = amin;
    }
}
