// nlmc_wave_frame.h -- the frame of a tempering-rounds kernel inside a wave launch, once (gfx950 / wave64): what k_rounds_waves
// (csrc/nlmc_wave_rounds.h) and k_rounds_waves_long (csrc/nlmc_wave_long_rounds.h) do around their sweeps:
// the workgroup's geometry, its slot maps, the Philox key rule, the observer, the swap round and the epilogue stores, each a function below,
// all forced inline, lambdas included.  None contains a barrier or returns early for a wave: the barriers stand in the kernel bodies,
// where their BARRIERS paragraphs can be checked by reading one function.
//
// Where the sharing stops: the sweeps.  The span from a sweep's threshold production through the update loop to the end of the sweep,
// and the field prologues, stay written out in each of the four wave kernels (k_sweep_waves, k_sweep_waves_long and the two here).  The
// lane kernels measured that limit ("Single sources, and where they stop"): sharing the frame was free or faster,
// sharing the sweep text was slower with every register figure unchanged.
#pragma once
#include "nlmc_lane_rounds.h"
#include "nlmc_wave_shape.h"

// Both kernels take their LDS carve-up from csrc/nlmc_wave_shape.h (nlmc_wave_rounds_layout, nlmc_wave_long_rounds_layout), as the host does.
struct WaveRoundsArgs {
    int P, C;                        // ladders per workgroup, chains a wave runs in turn at most (waves: blockDim.x / 64)
};

struct WaveGroup {
    int lad0, nlad, row0, nlive;     // first local ladder of this workgroup, its ladders (the last may hold fewer than P); first local chain, its chains
    int g0;                          // global ladder of its first: Philox key, rows of plan / log / chain_of_slot
};
__device__ __forceinline__ WaveGroup wave_group(const SweepArgs &a, const LaneRoundsArgs &q, int P)
{
    const int L = q.ladder_len;
    WaveGroup G;
    G.lad0 = (int)blockIdx.x * P; G.nlad = max(0, min(P, a.lane_rows / L - G.lad0));
    G.row0 = G.lad0 * L; G.nlive = G.nlad * L; G.g0 = a.chain_base / L + G.lad0;
    return G;
}

// cos_l: chain_of_slot[ladder in workgroup][slot], soc_l: slot_of_chain[chain in workgroup].  Thread t < nlive brings in chain t (the
// slots of a ladder are a permutation: every entry is written).  The caller's next barrier publishes the maps.
__device__ __forceinline__ void wave_maps_in(const SweepArgs &a, const LaneRoundsArgs &q, const WaveGroup &G, uint8_t *cos_l, uint8_t *soc_l)
{
    if ((int)threadIdx.x < G.nlive) {
        const int L = q.ladder_len, ch = (int)threadIdx.x, slot = q.slot_of_chain[a.chain_base + G.row0 + ch];
        soc_l[ch] = (uint8_t)slot;
        cos_l[ch / L * L + slot] = (uint8_t)ch;
    }
}

// The Philox key of local chain c at `slot`: the slot's where the random numbers follow the slot (rng_stride), else the chain's.
__device__ __forceinline__ uint32_t wave_key(const SweepArgs &a, int c, int slot)
{
    return a.rng_stride ? (uint32_t)((c / a.rng_ladder_len) * a.rng_stride + a.rng_base + slot) : (uint32_t)(a.chain_base + c);
}

// One observation of local chain c (energy E, at `slot`) in round r of the launch, before the swap round; the whole wave that owns the
// chain calls it.  The three words of the chain's record stay in global memory, read and written by lane 0.  state_out(): the wave
// stores the chain's spins to q.best.state, called where the energy improved on the record.
template <typename StateOut>
__device__ __forceinline__ void wave_observe(const LaneRoundsArgs &q, bool has_best, int r, int c, long long E, double inv, int slot, int lane,
                                             StateOut &&state_out)
{
    if (q.elog.energy && lane == 0) elog_store(q.elog, r, c, (double)E * inv, slot);
    if (has_best) {
        const int32_t stamp = (int32_t)(q.round0 + (uint32_t)r);
        long long rec_e = 0;
        int rec_hit = 0;
        if (lane == 0) { rec_e = q.best.efix[c]; rec_hit = q.best.first_hit[c]; }
        rec_e = uniform64(rec_e);
        rec_hit = __builtin_amdgcn_readfirstlane(rec_hit);
        const bool imp = (double)E < (double)rec_e;          // strict: the first attainment is kept
        if (lane == 0) {
            if (imp) { q.best.efix[c] = E; q.best.stamp[c] = stamp; }
            if (rec_hit < 0 && (double)E * inv <= q.best.target) q.best.first_hit[c] = stamp;
        }
        if (imp) state_out();
    }
}

// The swap round of round r, called by ONE wave of the workgroup between the round's two barriers: lane t decides pair t mod n_pairs of
// ladder t / n_pairs from the planned selection, with the key and arithmetic of k_pt_swap and the log entry of
// lane_swap_round; lanes past the last pair do nothing.  el: the chains' energies of this round.  Chains never move: the maps exchange
// entries (selected pairs are disjoint: no two lanes touch one map entry).
__device__ __forceinline__ void wave_swap_round(const SweepArgs &a, const LaneRoundsArgs &q, const WaveGroup &G, int r, int lane, double inv,
                                                const long long *el, uint8_t *cos_l, uint8_t *soc_l)
{
    if (lane < G.nlad * q.n_pairs) {
        const int lw = lane / q.n_pairs, p = lane - lw * q.n_pairs, g = G.g0 + lw, base = lw * q.ladder_len;
        const uint32_t round = q.round0 + (uint32_t)r;
        const size_t at = ((size_t)r * q.n_ladders + g) * q.n_pairs + p;
        const int i = q.plan_pairs[2 * at];
        const int ca = (int)cos_l[base + i], cb = (int)cos_l[base + i + 1];
        const double Ea = (double)el[ca] * inv, Eb = (double)el[cb] * inv;
        const bool acc = pt_swap_decide(p, i, i, Ea, Eb, q.beta, round, g, a.seed_lo, a.seed_hi);
        if (acc) {
            cos_l[base + i] = (uint8_t)cb; cos_l[base + i + 1] = (uint8_t)ca;
            soc_l[ca] = (uint8_t)(i + 1); soc_l[cb] = (uint8_t)i;
        }
        if (q.log_pairs) {
            q.log_pairs[2 * at] = i; q.log_pairs[2 * at + 1] = i + 1;
            q.log_acc[at] = acc ? 1 : 0;
        }
    }
}

// What ONE lane stores of the workgroup's chain ch at the end of the launch: the energy (efix, energy_sink) and both global maps.
__device__ __forceinline__ void wave_chain_out(const SweepArgs &a, const LaneRoundsArgs &q, const WaveGroup &G, int ch, double inv, const long long *el,
                                               const uint8_t *soc_l)
{
    const int L = q.ladder_len, c = G.row0 + ch;
    const long long Ef = el[ch];
    const int slot = (int)soc_l[ch];
    a.efix[c] = Ef;
    if (a.energy_sink) a.energy_sink[c] = (double)Ef * inv;
    q.slot_of_chain[a.chain_base + c] = slot;
    q.chain_of_slot[(size_t)(G.g0 + ch / L) * L + slot] = a.chain_base + c;
}
