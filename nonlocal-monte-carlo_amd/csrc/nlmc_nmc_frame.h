// nlmc_nmc_frame.h -- the frame of an NMC phases kernel, once (gfx950 / wave64): what k_nmc_phases_lanes (csrc/nlmc_lane_nmc.h),
// k_nmc_phases_waves (csrc/nlmc_wave_nmc.h) and k_nmc_phases_waves_long (csrc/nlmc_wave_long_nmc.h) do around their sweeps -- the phase
// kinds and the flag rule, where a launch starts from, the running minimum at the end of a sweep, and the outputs of a phase and of a
// chain -- each a function below, all forced inline.  None contains a barrier, a fence or an early return: every __syncthreads(),
// wave_long_fence() and lane_lds_fence() stands in a kernel body, where it can be checked by reading one function.  SweepArgs travels by
// value: handed on by reference it cost k_nmc_phases_waves_long 8 to 26 vector registers and a wave per SIMD.
//
// Where the sharing stops ("Single sources, and where they stop"): the field prologues, the sweep from its threshold
// production through the update loop, and how the best state is copied stay written out in each kernel; k_nmc_phases_waves takes the
// argument struct and the flag rule only, its code measured slower with the rest.
#pragma once
#include "nlmc_kernels.h"

#define NLMC_NMC_PHASES_LAUNCH 128      // phases one launch takes: their kinds travel in the kernel arguments, two bits each

struct NmcPhasesArgs {
    int n_phases;                    // phases of this launch
    int phase0;                      // its first phase inside the call: column of the outputs; > 0: the launch starts from the
                                     // context's best state and minimum (what the launch before it left)
    int phases_total;                // phases of the call: row length of the outputs
    uint32_t kinds[NLMC_NMC_PHASES_LAUNCH / 16];   // NLMC_PHASE_* of phase p of the launch: bits 2 (p & 15) .. of word p >> 4
    double cb0, cb1;                 // -2 log2(e) {beta, beta / temp_x}
    const uint8_t *mask;             // [n_chains][n_pad] backbone masks
    long long *phase_min;            // [rows][phases_total] or nullptr
    int32_t *phase_argmin;           // [rows][phases_total] or nullptr
    int lds_mask_off;                // k_nmc_phases_lanes only, as the next
    int lds_best_off;                // 0: the best state lives in global memory (SweepArgs::best)
};

// NLMC_PHASE_* of phase p of the launch
__device__ __forceinline__ unsigned nmc_phase_kind(const NmcPhasesArgs &q, int p) { return (q.kinds[p >> 4] >> (2 * (p & 15))) & 3u; }

// The sweep flag of a spin with backbone mask byte m in a phase of `kind` (0 plain, 1 scaled by temp_x, 2 frozen): hot = backbone scaled,
// the rest frozen; frozen = backbone frozen; all = every spin plain.
__device__ __forceinline__ unsigned nmc_phase_flag(unsigned kind, unsigned m)
{
    return kind == NLMC_PHASE_ALL ? 0u : kind == NLMC_PHASE_BACKBONE_HOT ? (m ? 1u : 2u) : (m ? 2u : 0u);
}

// Where a launch starts from: one that continues a call (phase0 > 0) from the best state and the minimum the launch before it left
__device__ __forceinline__ const int8_t *nmc_state_in(const SweepArgs a, const NmcPhasesArgs &q) { return q.phase0 > 0 ? a.best : a.spins; }
__device__ __forceinline__ long long nmc_energy_in(const SweepArgs a, const NmcPhasesArgs &q, int c) { return q.phase0 > 0 ? a.emin[c] : a.efix[c]; }

// End of sweep t of a phase (t counts from 0 within the phase): the tracked energy and the running minimum, which looks at every
// min_stride-th sweep.  Strict <: the first argmin.  Returns whether the sweep improved: the caller copies the state.
__device__ __forceinline__ bool nmc_sweep_end(long long &E, long long e_loc, long long &Emin, int &amin, int t, int min_stride)
{
    E += e_loc;
    const bool better = E < Emin && (t % min_stride == 0);
    if (better) { Emin = E; amin = t; }
    return better;
}

// The minimum and argmin of phase p of the launch, row `row` of the subset (one lane per row calls it)
__device__ __forceinline__ void nmc_phase_out(const NmcPhasesArgs &q, int row, int p, long long Emin, int amin)
{
    if (q.phase_min) {
        const size_t o = (size_t)row * q.phases_total + (size_t)(q.phase0 + p);
        q.phase_min[o] = Emin;
        q.phase_argmin[o] = amin;
    }
}

// The tracked energy and the last phase's minimum of chain c (one lane per chain calls it)
__device__ __forceinline__ void nmc_chain_out(const SweepArgs a, int c, long long E, long long Emin, int amin)
{
    a.efix[c] = E;
    if (a.energy_sink) a.energy_sink[c] = (double)E * __longlong_as_double((long long)(1023 - a.escale) << 52);
    a.emin[c] = Emin;
    a.argmin[c] = amin;
}
