// nlmc_lane_nmc.h -- the NMC phase cycles of short chains in one launch: a chain per lane (gfx950 / wave64).
//
// A round whose marked temperature slots run NMC cycles (NPT/npt.py:357-477) sweeps those chains in PHASES -- backbone spins hot and
// the rest frozen ("C"), backbone frozen ("NC"), all spins plain ("ALL") -- and every phase starts from the argmin-energy configuration
// of the one before.  Call by call that is, per phase, k_adopt_best, k_phase_flags, k_fill_min, k_lane_orders and k_sweep_lanes, each
// sweep launch transposing the chains into LDS and back for a handful of sweeps.  Nothing in it needs the host or another chain: the
// flags are a function of the backbone mask and the phase kind, the hand-off is per chain, the visiting orders are known in advance.
// k_nmc_phases_lanes runs all phases of a call with spins, mask and best state in LDS across the hand-offs.
//
//   launch : workgroup = one wave, lane l of block b owns row 64 b + l of the selected subset (chain_list), as in k_sweep_lanes; tail
//            lanes walk the wave's first chain on a zeroed column and write nothing.
//   LDS    : transposed spins | transposed backbone mask (from the context's mask array: there is no flags plane) | where it fits, a
//            transposed best-state plane (otherwise the context's best array in global memory, as k_sweep_lanes uses it) | where it
//            fits, one sweep's random numbers.
//   phase  : adopt the previous phase's minimum (k_adopt_best), reset the running minimum (k_fill_min), S sweeps of lane_update in the
//            shared order with the flag of a spin computed from its mask byte (k_phase_flags' rule), after every sweep
//            k_sweep_lanes' rule for the running minimum and its state; then the phase's minimum and argmin go out.
// Same bits as the call sequence on any route; the context's flags array is neither read nor written.
#pragma once
#include "nlmc_lanes.h"
#include "nlmc_nmc_frame.h"

static_assert(NLMC_LANE_STRIDE % 4 == 0, "the best-state plane is copied a word (four lanes of one spin) at a time");

// SweepArgs fields of this kernel: graph, chain_base, chain_list, spins, efix, energy_sink, the energy scales, seed, sweep0 = the
// first sweep of the launch, n_sweeps = sweeps per phase, min_stride, emin / argmin / best (the context's arrays), lane_perm = the
// orders of all n_phases * n_sweeps sweeps of the launch, lane_rows, lane_diag, lane_tab, lds_u_off.
template <bool F64>
__global__ __launch_bounds__(64) void k_nmc_phases_lanes(SweepArgs a, NmcPhasesArgs q)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    typedef std::conditional_t<F64, double, float> T;
    const int lane = threadIdx.x;
    constexpr int stride = NLMC_LANE_STRIDE;
    const int n = a.g.n, n_pad = a.g.n_pad;
    const int row0 = (int)blockIdx.x * 64;
    const int nrow = min(64, a.lane_rows - row0);          // rows of this wave (wave-uniform)
    const bool live = lane < nrow;
    const int row = live ? row0 + lane : row0;
    const int c = a.chain_list ? a.chain_list[row] : row;
    int8_t *s = reinterpret_cast<int8_t *>(lds_raw);
    const uint8_t *mk = lds_raw + q.lds_mask_off;
    unsigned char *bl = q.lds_best_off ? lds_raw + q.lds_best_off : nullptr;
    uint32_t *rtab = a.lane_tab ? reinterpret_cast<uint32_t *>(lds_raw + a.lds_u_off) : nullptr;   // word (spin k, lane l) at k * 64 + l
    const int8_t *state_in = nmc_state_in(a, q);

    // prologue: state and mask of the 64 chains, read coalesced, written transposed.  A launch that continues a call starts from the
    // best state the launch before it left.
    for (int r = 0; r < 64; ++r) {
        if (r < nrow) {
            const int cr = a.chain_list ? a.chain_list[row0 + r] : row0 + r;
            lane_column_in(lds_raw, stride, r, state_in + (size_t)cr * n_pad, n_pad, lane);
            lane_column_in(lds_raw + q.lds_mask_off, stride, r, q.mask + (size_t)cr * n_pad, n_pad, lane);
        } else {
            for (int j = lane; j < n_pad; j += 64) {
                lds_raw[j * stride + r] = 0; lds_raw[q.lds_mask_off + j * stride + r] = 0;
                if (bl) bl[j * stride + r] = 0;
            }
        }
    }
    lane_lds_fence();

    const uint32_t gc = (uint32_t)(a.chain_base + c);
    const double esc = __longlong_as_double((long long)(1023 + a.escale) << 52);   // 2^escale
    const T cb0 = scale_cb((T)q.cb0, a.qinv), cb1 = scale_cb((T)q.cb1, a.qinv);
    long long E = nmc_energy_in(a, q, c);
    long long Emin = 0;
    int amin = 0;
    // the lanes whose bytes a lane's word of a plane row holds (the best-state copy): lanes 4 (lane & 15) .. + 3
    const int wq = lane & 15;

    for (int p = 0; p < q.n_phases; ++p) {
        const unsigned kind = nmc_phase_kind(q, p);
        if (p > 0) {                                     // k_adopt_best: spins <- best, tracked energy <- the minimum
            if (bl) {
                const uint32_t *src = reinterpret_cast<const uint32_t *>(bl);
                uint32_t *dst = reinterpret_cast<uint32_t *>(lds_raw);
                for (int w = lane; w < n_pad * (stride / 4); w += 64) dst[w] = src[w];
            } else {
                __threadfence();                         // the rows other lanes of the wave stored
                for (int r = 0; r < nrow; ++r) {
                    const int cr = a.chain_list ? a.chain_list[row0 + r] : row0 + r;
                    lane_column_in(lds_raw, stride, r, a.best + (size_t)cr * n_pad, n_pad, lane);
                }
            }
            lane_lds_fence();
            E = Emin;
        }
        Emin = 0x7FFFFFFFFFFFFFFFll;                     // k_fill_min
        amin = 0;

        for (int t = 0; t < a.n_sweeps; ++t) {
            const int idx = p * a.n_sweeps + t;
            const uint32_t tt = a.sweep0 + (uint32_t)idx;
            const uint16_t *pp = a.lane_perm + (size_t)idx * (size_t)n;
            long long e_loc = 0;
            if (rtab) lane_fill_rtab<F64>(rtab, n, lane, tt, gc, a.seed_lo, a.seed_hi);

            for (int i0 = 0; i0 < n; i0 += 64) {
                const int kv = (i0 + lane < n) ? (int)pp[i0 + lane] : 0;    // 64 entries of the order in one load, handed out as scalars
                const int ni = min(64, n - i0);
                for (int ii = 0; ii < ni; ++ii) {
                    const int k = __builtin_amdgcn_readlane(kv, ii);
                    unsigned f = 0u;                     // (a plain phase does not read the mask plane)
                    if (kind != NLMC_PHASE_ALL) f = nmc_phase_flag(kind, mk[k * stride + lane]);
                    lane_update<F64, true>(a, s, rtab, lane, k, f, tt, gc, cb0, cb1, esc, e_loc);
                }
            }

            // end of the sweep: k_sweep_lanes' running minimum and its state (t counts from 0 within the phase)
            const bool better = nmc_sweep_end(E, e_loc, Emin, amin, t, a.min_stride);
            lane_lds_fence();
            unsigned long long m = __ballot(better && live);
            if (bl) {
                if (m) {                                 // every word takes the bytes of its improved lanes
                    const unsigned nib = (unsigned)(m >> (4 * wq)) & 15u;
                    const uint32_t sel = (nib & 1u ? 0xFFu : 0u) | (nib & 2u ? 0xFF00u : 0u) | (nib & 4u ? 0xFF0000u : 0u) | (nib & 8u ? 0xFF000000u : 0u);
                    for (int j = lane >> 4; j < n_pad; j += 4) {
                        const uint32_t sv = *reinterpret_cast<const uint32_t *>(lds_raw + j * stride + 4 * wq);
                        uint32_t *b = reinterpret_cast<uint32_t *>(bl + j * stride + 4 * wq);
                        *b = (sv & sel) | (*b & ~sel);
                    }
                    lane_lds_fence();
                }
            } else {
                while (m) {                              // wave-uniform: 64 lanes write consecutive spins of one chain
                    const int r = __builtin_ctzll(m);
                    m &= m - 1;
                    const int cr = a.chain_list ? a.chain_list[row0 + r] : row0 + r;
                    lane_column_out(lds_raw, stride, r, a.best + (size_t)cr * n_pad, n_pad, lane);
                }
            }
        }
        if (live) nmc_phase_out(q, row, p, Emin, amin);
    }

    // epilogue: the last phase's final state (no adoption), its best state, the tracked energy and the minimum
    lane_lds_fence();
    for (int r = 0; r < nrow; ++r) {
        const int cr = a.chain_list ? a.chain_list[row0 + r] : row0 + r;
        lane_column_out(lds_raw, stride, r, a.spins + (size_t)cr * n_pad, n_pad, lane);
        if (bl) lane_column_out(bl, stride, r, a.best + (size_t)cr * n_pad, n_pad, lane);
    }
    if (live) nmc_chain_out(a, c, E, Emin, amin);
}
