// nlmc_waves.h -- wave-per-chain sweeps with resident local fields for short chains (n <= NLMC_WAVE_N), gfx950 / wave64.
//
// The third shape next to "a chain per workgroup" (k_sweep_philox, k_sweep_fused) and "a chain per lane" (k_sweep_lanes): a WAVE owns
// a chain.  In the fixed-point ("f32") mode the local field X_j = hq_j + sum_i Jq_ji s_i is an exact int32 whatever the order of the
// sum, so it need not be recomputed at every update: lane l keeps the fields and the spins of the spins l, l + 64, .. in registers,
// and a flip of spin k corrects every field by one multiply-add on row k of a dense coupling matrix.  The decision for the visited
// spin is a v_readlane and one compare, wave-uniform: no level schedule, no barrier, no atomic, and the per-chain visiting order
// costs what the shared one costs.  From X on the operations are update_spin_q's, so the bits are the spec's.
//
//   k_wave_matrix : Jd[k][j] += Jq of every stored entry (k, j), on a zeroed buffer: dense int32, row stride 64 R, diagonal included.
//   k_sweep_waves : workgroup = W waves = W rows of the call.  JLDS: the workgroup stages the n rows of Jd into LDS once (row stride
//                   n_pad there) behind the kernel's only barrier; else a row comes from global memory, one coalesced load per owned
//                   field, and in both variants the row of the NEXT visited spin is requested before the current one is decided.
#pragma once
#include "nlmc_lanes.h"

struct WaveMatrixArgs {
    int n, stride;                // row stride of Jd in ints: 64 R
    const int32_t *rowptr;
    const EdgeQ *edge32;
    int32_t *Jd;                  // [n][stride], zeroed before the launch
};

// one workgroup per row; entries of one row with the same column add up, as they do in the CSR walk of the other kernels
__global__ __launch_bounds__(64) void k_wave_matrix(WaveMatrixArgs a)
{
    const int k = blockIdx.x;
    if (k >= a.n) return;
    const int rs = a.rowptr[k], re = a.rowptr[k + 1];
    for (int e = rs + (int)threadIdx.x; e < re; e += 64) {
        const EdgeQ q = a.edge32[e];
        if (q.col >= 0 && q.col < a.n) atomicAdd(a.Jd + (size_t)k * a.stride + q.col, q.q);
    }
}

// Register q (wave-uniform) of lane l (wave-uniform) of a per-lane array: one v_readlane per register, then a tree of scalar selects on
// the bits of q.  The candidates are named scalars on purpose: a select between two elements of a local array comes back from the
// optimiser as a load at a computed index, and the array as scratch memory.
template <int R> __device__ __forceinline__ int wave_get(const int (&v)[R], int l, int q)
{
    static_assert(R == 1 || R == 2 || R == 4, "one, two or four registers");
    const int t0 = __builtin_amdgcn_readlane(v[0], l);
    if constexpr (R == 1) return t0;
    else {
        const int t1 = __builtin_amdgcn_readlane(v[1], l);
        const int a = (q & 1) ? t1 : t0;
        if constexpr (R == 2) return a;
        else {
            const int t2 = __builtin_amdgcn_readlane(v[2], l), t3 = __builtin_amdgcn_readlane(v[3], l);
            const int b = (q & 1) ? t3 : t2;
            return (q & 2) ? b : a;
        }
    }
}

// R fields per lane (n <= 64 R).  SweepArgs fields of this kernel: lane_perm, lane_rows, per_chain (every row has its own orders),
// wave_J.  Phase flags, outputs, temperature source and chain subset are wave-uniform runtime branches.
template <int R, bool JLDS>
__global__ __launch_bounds__(1024) void k_sweep_waves(SweepArgs a)
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

    // lane l owns spins l + 64 r.  The padding bytes of a state row (j in [n, n_pad)) travel with the spins and are never visited;
    // the matrix columns of lanes past n_pad are read at a clamped, valid address and feed fields nobody reads.
    int jj[R], s[R], X[R], f[R];
    bool own[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = lane + 64 * r;
        own[r] = j < n_pad;
        jj[r] = JLDS ? min(j, n_pad - 1) : j;
        s[r] = own[r] ? (int)a.spins[(size_t)c * n_pad + j] : 0;
        f[r] = (a.flags && own[r]) ? (int)a.flags[(size_t)c * n_pad + j] : 0;
        X[r] = j < n ? a.g.hq[j] : 0;
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
            for (int q = 0; q < R; ++q) X[q] += Jr[q] * si;
        }
    }

    const uint32_t gc_chain = (uint32_t)(a.chain_base + c);
    const int trow = a.slot_of_chain ? a.slot_of_chain[gc_chain] : c;
    const uint32_t gc = (a.rng_stride && a.slot_of_chain) ? (uint32_t)((c / a.rng_ladder_len) * a.rng_stride + a.rng_base + trow) : gc_chain;
    long long E = uniform64(a.efix[c]), e_loc = 0;
    long long Emin = a.emin ? uniform64(a.emin[c]) : 0;
    int amin = a.emin ? __builtin_amdgcn_readfirstlane(a.argmin[c]) : 0;
    const bool per_sweep = (a.etrace != nullptr) || (a.emin != nullptr);
    const int n_rec = a.strace ? (a.trace_sweeps + a.rec_stride - 1) / a.rec_stride : 0;
    const int nblk = (n + 3) / 4;                                  // <= 64: lane l makes the Philox call of block l

    for (int t = 0; t < a.n_sweeps; ++t) {
        const uint32_t tt = a.sweep0 + (uint32_t)t;
        const float cb0 = scale_cb((float)a.tab[(size_t)trow * a.tab_cs + (size_t)t * a.tab_ss], a.qinv);
        const float cb1 = scale_cb((float)a.tab[(size_t)trow * a.tab_cs + (size_t)t * a.tab_ss + 1], a.qinv);
        const uint16_t *pp = a.lane_perm + (a.per_chain ? ((size_t)row * a.n_sweeps + t) : (size_t)t) * (size_t)n;

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
                int Jn[R];                                           // the next visited spin's row, in flight while k is decided
                load_row(Jn, __builtin_amdgcn_readlane(kv, min(ii + 1, ni - 1)));
                const int kl = k & 63, kr = k >> 6;
                const int fk = a.flags ? wave_get<R>(f, kl, kr) : 0;
                if (fk < 2) {                                        // frozen spins keep their value and add nothing
                    const int Xk = wave_get<R>(X, kl, kr), so = wave_get<R>(s, kl, kr);
                    const float wk = __int_as_float(wave_get<4>(Wt, k >> 2, k & 3));
                    const float z = (fk == 1 ? cb1 : cb0) * (float)Xk;
                    const int sn = (z < wk) ? 1 : -1;
                    if (sn != so) {
                        const int Jkk = wave_get<R>(Jc, kl, kr);     // the diagonal term stays out of the energy delta, not of the field
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
#pragma unroll
                for (int r = 0; r < R; ++r) if (own[r]) a.best[(size_t)c * n_pad + lane + 64 * r] = (int8_t)s[r];
            }
        }
        if (a.strace && (tg % a.rec_stride == 0)) {
            int8_t *dst = a.strace + ((size_t)row * n_rec + (size_t)(tg / a.rec_stride)) * n;
#pragma unroll
            for (int r = 0; r < R; ++r) if (lane + 64 * r < n) dst[lane + 64 * r] = (int8_t)s[r];
        }
    }
    if (!per_sweep) E += e_loc;

#pragma unroll
    for (int r = 0; r < R; ++r) if (own[r]) a.spins[(size_t)c * n_pad + lane + 64 * r] = (int8_t)s[r];
    if (lane == 0) {
        a.efix[c] = E;
        if (a.energy_sink) a.energy_sink[c] = (double)E * __longlong_as_double((long long)(1023 - a.escale) << 52);
        if (a.emin) { a.emin[c] = Emin; a.argmin[c] = amin; }
    }
}
