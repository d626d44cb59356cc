// nlmc_wave_long_rounds.h -- tempering rounds of dense chains of NLMC_WAVE_N < n <= NLMC_WAVE_LONG_N spins inside a wave launch
// (gfx950 / wave64): the frame k_rounds_waves has too (csrc/nlmc_wave_frame.h, once for both) around the sweep body of
// k_sweep_waves_long (csrc/nlmc_waves_long.h), written out here as that header says why.
//
// A swap is a label exchange and the spins never move, so the local fields X_j = hq_j + sum_i Jd[i][j] s_i stay valid across rounds.
// k_rounds_waves_long builds them once per chain and launch -- n rows of 64 R ints from global memory, about what n / 2 flips cost --
// and keeps them in LDS for all n_rounds rounds, where a sweep call and a swap call per round build them again every round.
//
//   launch : workgroup = W <= 16 waves holding P whole ladders of L <= 64 temperatures, Q = P L chains (csrc/nlmc_wave_shape.h:
//            nlmc_wave_long_rounds_shape).  Wave w owns the workgroup's chains w, w + W, .. below Q, at most C = ceil(Q / 16) of them.
//            The last workgroup may hold fewer ladders: its waves past the last chain sweep nothing and meet every barrier.
//   LDS    : nlmc_wave_long_rounds_layout -- per chain the field copy X [64 R] int32 and the spins [n_pad] int8, per wave the sweep's
//            thresholds, per workgroup the energies [Q] int64 and the byte maps chain_of_slot[P][L], slot_of_chain[Q].  A chain's
//            region is touched by the wave that owns it and by no other.  The fields live there by write-through, so a wave that runs
//            several chains in turn parks nothing: at a turn it reloads its R field registers from the chain's region.
//   sweeps : the update of k_sweep_waves_long<R, false>, shared order, without flags and per-sweep outputs, operation for operation:
//            three broadcast LDS reads (no flag) and one compare; on a flip one matrix row from global memory, R adds with write-back, the spin
//            written by one lane, wave_long_fence.
//   swaps  : those of k_rounds_waves: lane 0 of every wave leaves its chains' energies in LDS; behind a barrier lane t of wave 0 decides
//            pair t mod n_pairs of ladder t / n_pairs from the planned selection (wave_swap_round) and exchanges map entries; behind a
//            second barrier every wave reads its chains' slots again at its next turn.
// Same bits as nlmc_sweep_philox(beta = NULL) + nlmc_pt_swap_philox round by round, on any route.  Fixed point ("f32") only.
#pragma once
#include "nlmc_wave_frame.h"
#include "nlmc_waves_long.h"

// SweepArgs fields of this kernel: those of k_sweep_waves_long's shared order without flags and outputs; n_sweeps = sweeps per round,
// sweep0 = the first sweep of the launch, lane_perm = the orders of all its n_rounds * n_sweeps sweeps, lane_rows = the context's chains,
// tab = the ladder's table (two entries per slot), wave_J (row stride 64 R ints, columns past n zero).  LaneRoundsArgs: as in
// k_rounds_waves (the layout function says where the maps are).
// OBS: an observer is open -- a best-state record, an energy log or both (the records' pointers say which); one observation per chain
// and round, after the sweeps and before the swap.  The three words of a chain's record stay in global memory, read and written by
// lane 0 of the wave that owns the chain; an improved chain's spins go out from its LDS region.
//
// BARRIERS.  Every wave of a workgroup executes every barrier of the kernel: one behind the prologue, two per round.  There is no early
// return; no barrier stands inside a branch that depends on the wave or on a chain; the trip counts of the round loop (q.n_rounds) and
// of the turn loops (w.C) are launch constants.  Nothing polls, nothing is atomic, nothing waits on another workgroup.
template <int R, bool OBS>
__global__ __launch_bounds__(1024) void k_rounds_waves_long(SweepArgs a, LaneRoundsArgs q, WaveRoundsArgs w)
{
    static_assert(R == 8 || R == 16, "eight or sixteen registers");
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int JS = 64 * R;                                     // row stride of the matrix in global memory
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), W = (int)(blockDim.x >> 6);
    const int n = a.g.n, n_pad = a.g.n_pad;
    const int L = q.ladder_len, T = a.n_sweeps;
    const WaveGroup Gr = wave_group(a, q, w.P);
    const int row0 = Gr.row0, nlive = Gr.nlive;
    const int32_t *Jg = a.wave_J;

    const NlmcWaveLongRoundsLayout G = nlmc_wave_long_rounds_layout(n, n_pad, w.P * L, W);
    float *Wl = reinterpret_cast<float *>(lds_raw + G.w_off + (size_t)wv * (size_t)G.w_bytes);   // the wave's thresholds
    long long *el = reinterpret_cast<long long *>(lds_raw + G.e_off);
    uint8_t *cos_l = lds_raw + G.map_off, *soc_l = cos_l + w.P * L;   // chain_of_slot[ladder in workgroup][slot], slot_of_chain[chain in workgroup]
    auto fields_of = [&](int ch) { return reinterpret_cast<int32_t *>(lds_raw + (size_t)ch * (size_t)G.chain_bytes); };
    auto spins_of = [&](int ch) { return reinterpret_cast<int8_t *>(lds_raw + (size_t)ch * (size_t)G.chain_bytes + G.s_off); };

    wave_maps_in(a, q, Gr, cos_l, soc_l);

    int X[R];
    auto load_row = [&](int (&d)[R], int k) {
#pragma unroll
        for (int r = 0; r < R; ++r) d[r] = Jg[(size_t)k * JS + lane + 64 * r];
    };

    // prologue, once per chain and launch: spins in four bytes at a time (n_pad is a multiple of 16, the state rows are 16-byte aligned;
    // the padding bytes travel with the spins and are never visited), X_j = hq_j + sum_i Jd[i][j] s_i row by row, the energy to LDS
    for (int turn = 0; turn < w.C; ++turn) {
        const int ch = wv + turn * W;
        if (ch < nlive) {
            const int c = row0 + ch;
            int32_t *Xl = fields_of(ch);
            int8_t *sl = spins_of(ch);
            const uint32_t *s4 = reinterpret_cast<const uint32_t *>(a.spins + (size_t)c * n_pad);
            for (int j4 = lane; j4 < n_pad / 4; j4 += 64) reinterpret_cast<uint32_t *>(sl)[j4] = s4[j4];
            wave_long_fence();
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int j = lane + 64 * r;
                X[r] = j < n ? a.g.hq[j] : 0;
            }
#pragma unroll 2
            for (int i = 0; i < n; ++i) {
                const int si = (int)sl[i];
                int Jr[R];
                load_row(Jr, i);
#pragma unroll
                for (int u = 0; u < R; ++u) X[u] += Jr[u] * si;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) Xl[lane + 64 * r] = X[r];  // (the region has a word per lane and register)
            if (lane == 0) el[ch] = a.efix[c];
        }
    }
    __syncthreads();                                               // the maps, every chain's fields and energy

    const double inv = __longlong_as_double((long long)(1023 - a.escale) << 52);   // 2^-escale
    const int nblk = (n + 3) / 4;                                  // <= 256: lane l makes the Philox calls of blocks l, l + 64, ..
    const bool has_best = OBS && q.best.efix != nullptr;

    for (int r = 0; r < q.n_rounds; ++r) {
        for (int turn = 0; turn < w.C; ++turn) {
            const int ch = wv + turn * W;
            if (ch < nlive) {
                const int c = row0 + ch;
                int32_t *Xl = fields_of(ch);
                int8_t *sl = spins_of(ch);
                // what the turn needs of the chain: its fields from its region, its slot from the map the last swap round left
#pragma unroll
                for (int u = 0; u < R; ++u) X[u] = Xl[lane + 64 * u];
                const int slot = __builtin_amdgcn_readfirstlane((int)soc_l[ch]);
                const uint32_t gc = wave_key(a, c, slot);
                const float cb0 = wave_long_uniform(scale_cb((float)a.tab[(size_t)slot * a.tab_cs], a.qinv));
                long long e_loc = 0;
                for (int t = 0; t < T; ++t) {
                    const uint32_t tt = a.sweep0 + (uint32_t)(r * T + t);
                    const uint16_t *pp = a.lane_perm + ((size_t)r * T + t) * (size_t)n;
                    // the sweep's thresholds: those of spins 4 b .. 4 b + 3 from one call
                    for (int b = lane; b < nblk; b += 64) {
                        const u32x4 rr = philox4x32_10((uint32_t)b, tt, gc, NLMC_TAG_UNIFORM, a.seed_lo, a.seed_hi);
                        float4 w4;
                        w4.x = threshold_spec(rr.x); w4.y = threshold_spec(rr.y); w4.z = threshold_spec(rr.z); w4.w = threshold_spec(rr.w);
                        reinterpret_cast<float4 *>(Wl)[b] = w4;
                    }
                    wave_long_fence();
                    for (int i0 = 0; i0 < n; i0 += 64) {
                        const int kv = (i0 + lane < n) ? (int)pp[i0 + lane] : 0;   // 64 entries of the order in one load, handed out as scalars
                        const int ni = min(64, n - i0);
                        for (int ii = 0; ii < ni; ++ii) {
                            const int k = __builtin_amdgcn_readlane(kv, ii);
                            // three broadcast reads of the chain's region and the wave's thresholds in flight together, then scalars
                            const int Xk = __builtin_amdgcn_readfirstlane(Xl[k]), so = __builtin_amdgcn_readfirstlane((int)sl[k]);
                            const float wk = wave_long_uniform(Wl[k]);
                            const float z = cb0 * (float)Xk;
                            const int sn = (z < wk) ? 1 : -1;
                            if (sn != so) {
                                int Jc[R];
                                load_row(Jc, k);
                                const int Jkk = Jg[(size_t)k * JS + k];
                                // the diagonal term stays out of the energy delta, not of the field
                                e_loc += (long long)(Xk - Jkk * so) * (long long)((so - sn) * (1 << a.eshift));
                                const int d = sn - so;
#pragma unroll
                                for (int u = 0; u < R; ++u) {
                                    X[u] += d * Jc[u];
                                    Xl[lane + 64 * u] = X[u];
                                }
                                if (lane == 0) sl[k] = (int8_t)sn;
                                wave_long_fence();                   // the write-back stays ahead of the next update's reads
                            }
                        }
                    }
                    wave_long_fence();                               // the next sweep's thresholds stay behind this sweep's reads
                }
                const long long E = uniform64(el[ch]) + e_loc;
                if (lane == 0) el[ch] = E;

                if constexpr (OBS) {                            // one observation of the chain, before the swap round; its state from its region
                    wave_observe(q, has_best, r, c, E, inv, slot, lane, [&]() __attribute__((always_inline)) {
                        uint32_t *b4 = reinterpret_cast<uint32_t *>(q.best.state + (size_t)c * n_pad);
                        for (int j4 = lane; j4 < n_pad / 4; j4 += 64) b4[j4] = reinterpret_cast<const uint32_t *>(sl)[j4];
                    });
                }
            }
        }
        __syncthreads();                                        // every chain's energy of this round is in LDS

        if (wv == 0) wave_swap_round(a, q, Gr, r, lane, inv, el, cos_l, soc_l);   // lane t of wave 0 decides pair t mod n_pairs of ladder t / n_pairs
        __syncthreads();                                        // the maps of the next round
    }

    // epilogue, once per chain and launch
    for (int turn = 0; turn < w.C; ++turn) {
        const int ch = wv + turn * W;
        if (ch < nlive) {
            const int c = row0 + ch;
            const int8_t *sl = spins_of(ch);
            uint32_t *s4 = reinterpret_cast<uint32_t *>(a.spins + (size_t)c * n_pad);
            for (int j4 = lane; j4 < n_pad / 4; j4 += 64) s4[j4] = reinterpret_cast<const uint32_t *>(sl)[j4];
            if (lane == 0) wave_chain_out(a, q, Gr, ch, inv, el, soc_l);
        }
    }
}
