// nlmc_wave_rounds.h -- tempering rounds of short chains inside a wave launch: a ladder per workgroup (gfx950 / wave64).
//
// k_sweep_waves (csrc/nlmc_waves.h) gives a chain a wave and keeps its exact int32 local fields in registers.  k_rounds_waves runs
// n_rounds rounds -- T sweeps at the ladder temperatures, then the swap round of k_pt_swap -- in one launch, so that the field
// prologue, the staging of the matrix into LDS and the launches are paid once per chunk of rounds and not once per round.
//
//   launch : workgroup = W waves holding P whole ladders of L <= 64 temperatures, Q = P L <= 64 chains (csrc/nlmc_wave_shape.h:
//            nlmc_wave_rounds_shape).  Wave w owns the workgroup's chains w, w + W, .. below Q, at most C = ceil(Q / 16) of them.  The
//            last workgroup may hold fewer ladders: its waves past the last chain sweep nothing and meet every barrier.
//   sweeps : the update of k_sweep_waves' shared order without flags and per-sweep outputs, operation for operation.  A wave that owns
//            one chain keeps s, X, the energy, the slot, cb0 and the Philox key in registers for the whole launch; a wave that owns
//            several runs them in turn within a round and parks s (int8) and X (int32) in LDS between its turns.
//   swaps  : lane 0 of every wave leaves its chains' energies in an int64 array in LDS; behind a barrier lane t of wave 0 decides pair
//            t mod n_pairs of ladder t / n_pairs of the workgroup from the planned selection, with the key and arithmetic of k_pt_swap
//            (wave_swap_round) and the log entry of lane_swap_round.  Chains never move: two byte maps in LDS, chain_of_slot[ladder][slot]
//            and slot_of_chain[chain], exchange entries; behind a second barrier a wave whose chain's slot moved reloads its inverse
//            temperature (and its RNG key where that follows the slot).
//   frame  : the workgroup's geometry, the maps, the key rule, the observer, the swap round and the epilogue stores are those of
//            csrc/nlmc_wave_frame.h, shared with k_rounds_waves_long; the prologue and the sweeps are written out here (that header says why).
// Same bits as nlmc_sweep_philox(beta = NULL) + nlmc_pt_swap_philox round by round, on any route.
#pragma once
#include "nlmc_wave_frame.h"
#include "nlmc_waves.h"

// SweepArgs fields of this kernel: those of k_sweep_waves' shared order without flags and outputs; n_sweeps = sweeps per round, sweep0 =
// the first sweep of the launch, lane_perm = the orders of all its n_rounds * n_sweeps sweeps, lane_rows = the context's chains, tab =
// the ladder's table (two entries per slot), wave_J.  LaneRoundsArgs: as in k_rounds_lanes, without lds_map_off: the LDS carve-up is
// nlmc_wave_rounds_layout of (n, n_pad, P L, C, JLDS), the host's own.
// OBS: an observer is open -- a best-state record, an energy log or both (the records' pointers say which); one observation per chain
// and round, after the sweeps and before the swap.  The three words of a chain's record stay in global memory, read and written by
// lane 0 of the wave that owns the chain.  Without OBS the kernel carries none of this.
//
// BARRIERS.  Every wave of a workgroup executes every barrier of the kernel: one behind the staging, two per round.  There is no early
// return; no barrier stands inside a branch that depends on the wave or on a chain; the trip counts of the round loop (q.n_rounds) and
// of the turn loops (w.C) are launch constants.  Nothing polls, nothing is atomic, nothing waits on another workgroup.
template <int R, bool JLDS, bool OBS>
__global__ __launch_bounds__(1024) void k_rounds_waves(SweepArgs a, LaneRoundsArgs q, WaveRoundsArgs w)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int JS = 64 * R;                                     // row stride of the matrix in global memory
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), W = (int)(blockDim.x >> 6);
    const int n = a.g.n, n_pad = a.g.n_pad;
    const int L = q.ladder_len, T = a.n_sweeps;
    const WaveGroup G = wave_group(a, q, w.P);
    const int row0 = G.row0, nlive = G.nlive;
    const int32_t *Jg = a.wave_J;
    const int32_t *Jl = reinterpret_cast<const int32_t *>(lds_raw);
    const NlmcWaveRoundsLayout Y = nlmc_wave_rounds_layout(n, n_pad, w.P * L, w.C, JLDS);
    int32_t *Xp = reinterpret_cast<int32_t *>(lds_raw + Y.x_off);  // parked X | parked s (both only where C > 1) | energies | maps
    int8_t *sp = reinterpret_cast<int8_t *>(lds_raw + Y.s_off);
    long long *el = reinterpret_cast<long long *>(lds_raw + Y.e_off);
    uint8_t *cos_l = lds_raw + Y.map_off, *soc_l = cos_l + w.P * L;   // chain_of_slot[ladder in workgroup][slot], slot_of_chain[chain in workgroup]

    if constexpr (JLDS) {
        int32_t *dst = reinterpret_cast<int32_t *>(lds_raw);
        for (int k = wv; k < n; k += W)
            for (int j = lane; j < n_pad; j += 64) dst[k * n_pad + j] = Jg[(size_t)k * JS + j];
    }
    wave_maps_in(a, q, G, cos_l, soc_l);
    __syncthreads();

    // the chains this wave owns: wv, wv + W, .. below nlive (wave-uniform)
    const int nown = wv < nlive ? (nlive - 1 - wv) / W + 1 : 0;
    const bool multi = nown > 1;

    int jj[R], s[R], X[R];
    bool own[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = lane + 64 * r;
        own[r] = j < n_pad;
        jj[r] = JLDS ? min(j, n_pad - 1) : j;
        s[r] = 0; X[r] = 0;
    }
    auto load_row = [&](int (&d)[R], int k) {
#pragma unroll
        for (int r = 0; r < R; ++r) d[r] = JLDS ? Jl[k * n_pad + jj[r]] : Jg[(size_t)k * JS + jj[r]];
    };
    auto park = [&](int ch) {
#pragma unroll
        for (int r = 0; r < R; ++r) { Xp[(ch * R + r) * 64 + lane] = X[r]; sp[(ch * R + r) * 64 + lane] = (int8_t)s[r]; }
    };
    auto unpark = [&](int ch) {
#pragma unroll
        for (int r = 0; r < R; ++r) { X[r] = Xp[(ch * R + r) * 64 + lane]; s[r] = (int)sp[(ch * R + r) * 64 + lane]; }
    };

    // prologue, once per chain and launch: spins in, X_j = hq_j + sum_i Jd[i][j] s_i row by row, the energy to LDS
    for (int turn = 0; turn < w.C; ++turn) {
        const int ch = wv + turn * W;
        if (ch < nlive) {
            const int c = row0 + ch;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int j = lane + 64 * r;
                s[r] = own[r] ? (int)a.spins[(size_t)c * n_pad + j] : 0;
                X[r] = j < n ? a.g.hq[j] : 0;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int ni = min(64, n - 64 * r);
                for (int ii = 0; ii < ni; ++ii) {
                    const int si = __builtin_amdgcn_readlane(s[r], ii);
                    int Jr[R];
                    load_row(Jr, 64 * r + ii);
#pragma unroll
                    for (int u = 0; u < R; ++u) X[u] += Jr[u] * si;
                }
            }
            if (multi) park(ch);
            if (lane == 0) el[ch] = a.efix[c];
        }
    }

    // what a wave with one chain keeps for the whole launch (a wave with several reloads it at every turn)
    const int ch1 = min(wv, max(nlive - 1, 0));
    int slot = __builtin_amdgcn_readfirstlane((int)soc_l[ch1]);
    uint32_t gc = wave_key(a, row0 + ch1, slot);
    float cb0 = scale_cb((float)a.tab[(size_t)slot * a.tab_cs], a.qinv);
    long long E = nown ? uniform64(a.efix[row0 + ch1]) : 0;
    const double inv = __longlong_as_double((long long)(1023 - a.escale) << 52);   // 2^-escale
    const int nblk = (n + 3) / 4;                                  // <= 64: lane l makes the Philox call of block l
    const bool has_best = OBS && q.best.efix != nullptr;

    for (int r = 0; r < q.n_rounds; ++r) {
        for (int turn = 0; turn < w.C; ++turn) {
            const int ch = wv + turn * W;
            if (ch < nlive) {
                const int c = row0 + ch;
                if (multi) {
                    unpark(ch);
                    slot = __builtin_amdgcn_readfirstlane((int)soc_l[ch]);
                    gc = wave_key(a, c, slot);
                    cb0 = scale_cb((float)a.tab[(size_t)slot * a.tab_cs], a.qinv);
                    E = uniform64(el[ch]);
                }
                long long e_loc = 0;
                for (int t = 0; t < T; ++t) {
                    const uint32_t tt = a.sweep0 + (uint32_t)(r * T + t);
                    const uint16_t *pp = a.lane_perm + ((size_t)r * T + t) * (size_t)n;
                    // the thresholds of spins 4 l .. 4 l + 3 (one call per lane and sweep)
                    int Wt[4] = {0, 0, 0, 0};
                    if (lane < nblk) {
                        const u32x4 rr = philox4x32_10((uint32_t)lane, tt, gc, NLMC_TAG_UNIFORM, a.seed_lo, a.seed_hi);
                        Wt[0] = (int)__float_as_uint(threshold_spec(rr.x)); Wt[1] = (int)__float_as_uint(threshold_spec(rr.y));
                        Wt[2] = (int)__float_as_uint(threshold_spec(rr.z)); Wt[3] = (int)__float_as_uint(threshold_spec(rr.w));
                    }
                    for (int i0 = 0; i0 < n; i0 += 64) {
                        const int kv = (i0 + lane < n) ? (int)pp[i0 + lane] : 0;   // 64 entries of the order in one load, handed out as scalars
                        const int ni = min(64, n - i0);
                        int Jc[R];
                        load_row(Jc, __builtin_amdgcn_readlane(kv, 0));
                        for (int ii = 0; ii < ni; ++ii) {
                            const int k = __builtin_amdgcn_readlane(kv, ii);
                            int Jn[R];                                   // the next visited spin's row, in flight while k is decided
                            load_row(Jn, __builtin_amdgcn_readlane(kv, min(ii + 1, ni - 1)));
                            const int kl = k & 63, kr = k >> 6;
                            const int Xk = wave_get<R>(X, kl, kr), so = wave_get<R>(s, kl, kr);
                            const float wk = __int_as_float(wave_get<4>(Wt, k >> 2, k & 3));
                            const float z = cb0 * (float)Xk;
                            const int sn = (z < wk) ? 1 : -1;
                            if (sn != so) {
                                const int Jkk = wave_get<R>(Jc, kl, kr);     // the diagonal term stays out of the energy delta, not of the field
                                e_loc += (long long)(Xk - Jkk * so) * (long long)((so - sn) * (1 << a.eshift));
                                const int d = sn - so;
#pragma unroll
                                for (int u = 0; u < R; ++u) {
                                    X[u] += d * Jc[u];
                                    s[u] = (u == kr && lane == kl) ? sn : s[u];
                                }
                            }
#pragma unroll
                            for (int u = 0; u < R; ++u) Jc[u] = Jn[u];
                        }
                    }
                }
                E += e_loc;
                if (lane == 0) el[ch] = E;
                if (multi) park(ch);

                if constexpr (OBS) {                            // one observation of the chain, before the swap round; its state from registers
                    wave_observe(q, has_best, r, c, E, inv, slot, lane, [&]() __attribute__((always_inline)) {
#pragma unroll
                        for (int u = 0; u < R; ++u) if (own[u]) q.best.state[(size_t)c * n_pad + lane + 64 * u] = (int8_t)s[u];
                    });
                }
            }
        }
        __syncthreads();                                        // every chain's energy of this round is in LDS

        if (wv == 0) wave_swap_round(a, q, G, r, lane, inv, el, cos_l, soc_l);   // lane t of wave 0 decides pair t mod n_pairs of ladder t / n_pairs
        __syncthreads();                                        // the maps of the next round

        if (!multi) {
            const int ns = __builtin_amdgcn_readfirstlane((int)soc_l[ch1]);
            if (ns != slot) {
                slot = ns;
                cb0 = scale_cb((float)a.tab[(size_t)slot * a.tab_cs], a.qinv);
                gc = wave_key(a, row0 + ch1, slot);
            }
        }
    }

    // epilogue, once per chain and launch
    for (int turn = 0; turn < w.C; ++turn) {
        const int ch = wv + turn * W;
        if (ch < nlive) {
            const int c = row0 + ch;
            if (multi) unpark(ch);
#pragma unroll
            for (int r = 0; r < R; ++r) if (own[r]) a.spins[(size_t)c * n_pad + lane + 64 * r] = (int8_t)s[r];
            if (lane == 0) wave_chain_out(a, q, G, ch, inv, el, soc_l);
        }
    }
}
