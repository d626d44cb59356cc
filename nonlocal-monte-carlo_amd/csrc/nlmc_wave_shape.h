// nlmc_wave_shape.h -- host-side launch shapes of the wave-per-chain sweeps (csrc/nlmc_waves.h, csrc/nlmc_waves_long.h) and of the
// tempering rounds inside a wave launch (csrc/nlmc_wave_rounds.h), pure functions with no HIP in them (checked on the host under the
// sanitizers: scripts/wave_shape_check.cpp, scripts/wave_long_shape_check.cpp, scripts/wave_rounds_shape_check.cpp,
// scripts/wave_long_rounds_shape_check.cpp, scripts/wave_long_nmc_shape_check.cpp).  No result depends on W or P.
// Each rule stands once (nlmc_wave_fields, nlmc_wave_rows, nlmc_wave_ladders, NLMC_WAVE_LONG_LDS_MAX); the shape functions put them together,
// the long ones then lower W or P to what the LDS holds.  The LDS carve-ups are host/device functions the kernels call too.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NLMC_WS_HD __host__ __device__
#else
#define NLMC_WS_HD
#endif

#define NLMC_WAVE_JLDS_N 192                            // longest chain whose matrix the workgroup stages in LDS: n n_pad 4 <= 144 KB
#define NLMC_WAVE_LONG_MIN_N 257                        // NLMC_WAVE_N + 1: shorter chains have k_sweep_waves, longer ones k_sweep_waves_long
#define NLMC_WAVE_LONG_MAX_N 1024                       // NLMC_WAVE_LONG_N of include/nlmc.h
#define NLMC_WAVE_LONG_LDS_MAX ((size_t)158 * 1024)     // dynamic LDS a workgroup of ANY wave kernel may ask for (NLMC_LDS_BYTES_MAX of csrc/nlmc.hip; the long kernels named it)

// Fields per lane of a chain of n spins, 64 R >= n: 1, 2, 4 (k_sweep_waves, k_rounds_waves), 8, 16 (the long kernels); 0: the chain does
// not fit.  The long half stands apart for the layout functions of the long kernels, which run on the device where n is known to be
// long: through it they compile to one compare, as before they called anything.
NLMC_WS_HD static inline int nlmc_wave_long_fields(int n) { return n <= 512 ? 8 : 16; }
NLMC_WS_HD static inline int nlmc_wave_fields(int n)
{
    return n < 1 || n > NLMC_WAVE_LONG_MAX_N ? 0 : n <= 64 ? 1 : n <= 128 ? 2 : n < NLMC_WAVE_LONG_MIN_N ? 4 : nlmc_wave_long_fields(n);
}

// Rows (= waves) per workgroup of a sweep launch.  rows >= 1.  n_cu: compute units of the device.  knob_waves: NLMC_WAVE_WAVES (0: unset).
// Enough workgroups to cover the compute units first, then up to 16 waves per workgroup.
static inline int nlmc_wave_rows(int rows, int n_cu, int knob_waves)
{
    const int cu = n_cu > 0 ? n_cu : 1;
    long long w = knob_waves > 0 ? knob_waves : ((long long)rows + cu - 1) / cu;
    if (w < 1) w = 1;
    if (w > 16) w = 16;
    return (int)w;
}

// Ladders per workgroup of a rounds launch and the turns that follow.  ladders >= 1 of 1 <= L <= 64 temperatures each.  knob_ladders:
// NLMC_WAVE_ROUNDS_LADDERS (0: by the rule).  p_max: a further ceiling on P (0: none; what the LDS of the long chains holds).  The rule:
// enough workgroups to cover the compute units first, then as many ladders as fit 16 waves (a chain per wave); a ladder of more than
// 16 temperatures has the workgroup to itself and its waves run chains in turn.
struct NlmcWaveLadders {
    int P;            // whole ladders per workgroup: Q = P L <= 64 chains
    int C;            // chains a wave runs in turn at most: ceil(Q / 16), 1 .. 4
    int W;            // waves per workgroup: ceil(Q / C) <= 16; wave w owns the workgroup's chains w, w + W, .. below Q
    int blocks;       // workgroups: ceil(ladders / P)
};
static inline NlmcWaveLadders nlmc_wave_ladders(int L, int ladders, int n_cu, int knob_ladders, int p_max)
{
    const int cu = n_cu > 0 ? n_cu : 1;
    long long p = knob_ladders > 0 ? knob_ladders : ((long long)ladders + cu - 1) / cu;
    const long long cap = knob_ladders > 0 ? 64 / L : (16 / L > 1 ? 16 / L : 1);
    if (p > cap) p = cap;
    if (p > ladders) p = ladders;
    if (p_max > 0 && p > p_max) p = p_max;
    if (p < 1) p = 1;
    const int Q = (int)p * L, C = (Q + 15) / 16;
    const NlmcWaveLadders g = {(int)p, C, (Q + C - 1) / C, (int)((ladders + p - 1) / p)};
    return g;
}

// ---- sweeps, a wave per chain (csrc/nlmc_waves.h: k_sweep_waves, n <= 256; csrc/nlmc_waves_long.h: k_sweep_waves_long, 256 < n <= 1024) ----
// The LDS region a wave of k_sweep_waves_long keeps to itself, each part 16-byte aligned: X [64 R] int32 (a word per lane and register:
// the write-back of a flip needs no bounds) | thresholds [4 ceil(n / 4)] float | spins [n_pad] int8 | phase flags [n_pad] int8.  The
// kernel and the shape function both take the layout from here.
struct NlmcWaveLongRegion { int w_off, s_off, f_off, bytes; };
NLMC_WS_HD static inline NlmcWaveLongRegion nlmc_wave_long_region(int n, int n_pad)
{
    NlmcWaveLongRegion g;
    g.w_off = 256 * nlmc_wave_long_fields(n);
    g.s_off = g.w_off + 16 * ((n + 3) / 4);
    g.f_off = g.s_off + ((n_pad + 15) & ~15);
    g.bytes = g.f_off + ((n_pad + 15) & ~15);
    return g;
}

// One shape for both sweep kernels (k_sweep_waves stages the matrix and keeps no regions, k_sweep_waves_long the reverse): one host driver.
struct NlmcWaveShape {
    int R;            // fields per lane (nlmc_wave_fields); 0: the chain does not fit
    int W;            // waves (= rows of the call) per workgroup, 1 .. 16, of the long chains as many as the LDS holds regions at most
    int blocks;       // workgroups: ceil(rows / W)
    int jlds;         // the matrix is staged in LDS (never of the long chains)
    size_t region;    // LDS of one wave in bytes (nlmc_wave_long_region; 0 of the short chains)
    size_t lds;       // dynamic LDS of the launch in bytes: the staged matrix, or W regions
    size_t stride;    // row stride of the matrix in global memory, in ints: 64 R
};

// n <= 256.  allow_lds: NLMC_WAVE_JLDS is not 0.
static inline NlmcWaveShape nlmc_wave_shape(int n, int n_pad, int rows, int n_cu, int knob_waves, int allow_lds)
{
    NlmcWaveShape s = {0, 1, 0, 0, 0, 0, 0};
    if (n < 1 || n >= NLMC_WAVE_LONG_MIN_N || n_pad < n || rows < 1) return s;
    s.R = nlmc_wave_fields(n);
    s.stride = (size_t)64 * (size_t)s.R;
    s.W = nlmc_wave_rows(rows, n_cu, knob_waves);
    s.blocks = (int)(((long long)rows + s.W - 1) / s.W);
    s.jlds = allow_lds && n <= NLMC_WAVE_JLDS_N;
    s.lds = s.jlds ? (size_t)n * (size_t)n_pad * sizeof(int) : 0;
    return s;
}

// 256 < n <= 1024: as many waves as have their regions in a workgroup's LDS.
static inline NlmcWaveShape nlmc_wave_long_shape(int n, int n_pad, int rows, int n_cu, int knob_waves)
{
    NlmcWaveShape s = {0, 1, 0, 0, 0, 0, 0};
    if (n < NLMC_WAVE_LONG_MIN_N || n > NLMC_WAVE_LONG_MAX_N || n_pad < n || rows < 1) return s;
    const int R = nlmc_wave_fields(n);
    if (n_pad > 64 * R) return s;                       // the padded state row must fit a matrix row
    s.R = R;
    s.stride = (size_t)64 * (size_t)R;
    s.region = (size_t)nlmc_wave_long_region(n, n_pad).bytes;
    const int fit = (int)(NLMC_WAVE_LONG_LDS_MAX / s.region);                        // >= 15: a region is at most 10 KB
    s.W = nlmc_wave_rows(rows, n_cu, knob_waves);
    if (s.W > fit) s.W = fit;
    s.blocks = (int)(((long long)rows + s.W - 1) / s.W);
    s.lds = (size_t)s.W * s.region;
    return s;
}

// ---- NMC phase cycles of the long chains in one wave launch (csrc/nlmc_wave_long_nmc.h: k_nmc_phases_waves_long) ----
// The LDS region a wave of k_nmc_phases_waves_long keeps to itself: nlmc_wave_long_region's parts (at offset 0, so the update is
// k_sweep_waves_long's) | best spins [n_pad] int8 | backbone mask [n_pad] int8, each part 16-byte aligned.  The best state's fields
// live in registers.  The kernel and the shape function both take the layout from here.
struct NlmcWaveLongNmcRegion { NlmcWaveLongRegion sweep; int b_off, m_off, bytes; };
NLMC_WS_HD static inline NlmcWaveLongNmcRegion nlmc_wave_long_nmc_region(int n, int n_pad)
{
    NlmcWaveLongNmcRegion g;
    g.sweep = nlmc_wave_long_region(n, n_pad);
    g.b_off = g.sweep.bytes;
    g.m_off = g.b_off + ((n_pad + 15) & ~15);
    g.bytes = g.m_off + ((n_pad + 15) & ~15);
    return g;
}

// 256 < n <= 1024: nlmc_wave_long_shape's rule, with W lowered to what the LDS holds of the larger regions (13 at 1024 spins).  R = 0
// where the chain does not fit.  No result depends on W.
static inline NlmcWaveShape nlmc_wave_long_nmc_shape(int n, int n_pad, int rows, int n_cu, int knob_waves)
{
    NlmcWaveShape s = nlmc_wave_long_shape(n, n_pad, rows, n_cu, knob_waves);
    if (s.R == 0) return s;
    s.region = (size_t)nlmc_wave_long_nmc_region(n, n_pad).bytes;
    const int fit = (int)(NLMC_WAVE_LONG_LDS_MAX / s.region);                        // >= 13: a region is at most 12 KB
    s.W = nlmc_wave_rows(rows, n_cu, knob_waves);
    if (s.W > fit) s.W = fit;
    s.blocks = (int)(((long long)rows + s.W - 1) / s.W);
    s.lds = (size_t)s.W * s.region;
    return s;
}

// ---- tempering rounds inside a wave launch (csrc/nlmc_wave_rounds.h: k_rounds_waves, k_rounds_waves_long): a workgroup holds P whole ladders
// The LDS of a workgroup of k_rounds_waves, Q chains of which a wave runs at most C in turn, each part 16-byte aligned: matrix
// [n][n_pad] int32 (jlds) | parked X [Q][R][64] int32 (C > 1) | parked s [Q][R][64] int8 (C > 1) | energies [Q] int64 | maps
// chain_of_slot [P][L] + slot_of_chain [Q] bytes.  The kernel and the shape function both take the layout from here.
struct NlmcWaveRoundsLayout { size_t x_off, s_off, e_off, map_off, total; };
NLMC_WS_HD static inline NlmcWaveRoundsLayout nlmc_wave_rounds_layout(int n, int n_pad, int Q, int C, int jlds)
{
    const size_t a16 = 15, stride = (size_t)64 * (size_t)nlmc_wave_fields(n);
    const size_t park_x = C > 1 ? (size_t)Q * stride * sizeof(int) : 0, park_s = C > 1 ? (size_t)Q * stride : 0;
    NlmcWaveRoundsLayout g;
    g.x_off = jlds ? ((size_t)n * (size_t)n_pad * sizeof(int) + a16) & ~a16 : 0;
    g.s_off = g.x_off + ((park_x + a16) & ~a16);
    g.e_off = g.s_off + ((park_s + a16) & ~a16);
    g.map_off = g.e_off + (((size_t)Q * 8 + a16) & ~a16);
    g.total = g.map_off + (((size_t)2 * Q + a16) & ~a16);
    return g;
}

// The LDS of a workgroup of k_rounds_waves_long, Q chains on W waves, each part 16-byte aligned: Q chain regions of chain_bytes each --
// X [64 R] int32 (a word per lane and register, as in nlmc_wave_long_region) | spins [n_pad] int8 at s_off -- | W threshold regions of
// w_bytes each, [4 ceil(n / 4)] float, one per wave | energies [Q] int64 | maps chain_of_slot [P][L] + slot_of_chain [Q] bytes.  No
// phase-flag plane: these are plain chains.  The kernel and the shape function both take the layout from here.
struct NlmcWaveLongRoundsLayout { int s_off, chain_bytes, w_bytes, w_off, e_off, map_off, total; };
NLMC_WS_HD static inline NlmcWaveLongRoundsLayout nlmc_wave_long_rounds_layout(int n, int n_pad, int Q, int W)
{
    NlmcWaveLongRoundsLayout g;
    g.s_off = 256 * nlmc_wave_long_fields(n);
    g.chain_bytes = g.s_off + ((n_pad + 15) & ~15);
    g.w_bytes = 16 * ((n + 3) / 4);
    g.w_off = Q * g.chain_bytes;
    g.e_off = g.w_off + W * g.w_bytes;
    g.map_off = g.e_off + ((8 * Q + 15) & ~15);
    g.total = g.map_off + ((2 * Q + 15) & ~15);
    return g;
}

// One shape for both rounds kernels: they differ in jlds alone, which the long chains never have, so one host driver launches either.
struct NlmcWaveRoundsShape {
    int R;            // fields per lane (nlmc_wave_fields); 0: the chain, the ladder or (long chains) one ladder's regions do not fit
    int P, C, W, blocks;   // nlmc_wave_ladders
    int jlds;         // the matrix is staged in LDS (never of the long chains)
    size_t lds;       // dynamic LDS of the launch in bytes (nlmc_wave_rounds_layout or nlmc_wave_long_rounds_layout of Q = P L)
    size_t stride;    // row stride of the matrix in global memory, in ints: 64 R
};

// n <= 256.  ladders >= 1 of L temperatures each.  knob_ladders: NLMC_WAVE_ROUNDS_LADDERS (0: by the rule of nlmc_wave_ladders).  The
// matrix is staged where allow_lds says so and it fits next to the rest.  No result depends on P or W.
static inline NlmcWaveRoundsShape nlmc_wave_rounds_shape(int n, int n_pad, int L, int ladders, int n_cu, int knob_ladders, int allow_lds)
{
    NlmcWaveRoundsShape s = {0, 1, 1, 1, 0, 0, 0, 0};
    if (n < 1 || n >= NLMC_WAVE_LONG_MIN_N || n_pad < n || n_pad > 256 || L < 1 || L > 64 || ladders < 1) return s;
    const NlmcWaveLadders g = nlmc_wave_ladders(L, ladders, n_cu, knob_ladders, 0);
    s.R = nlmc_wave_fields(n);
    s.P = g.P; s.C = g.C; s.W = g.W; s.blocks = g.blocks;
    s.stride = (size_t)64 * (size_t)s.R;
    s.jlds = allow_lds && n <= NLMC_WAVE_JLDS_N && nlmc_wave_rounds_layout(n, n_pad, s.P * L, s.C, 1).total <= NLMC_WAVE_LONG_LDS_MAX;
    s.lds = nlmc_wave_rounds_layout(n, n_pad, s.P * L, s.C, s.jlds).total;
    return s;
}

// 256 < n <= 1024.  nlmc_wave_rounds_shape's rule, and on top of it P is lowered until the workgroup's regions fit its LDS.  R = 0
// where one ladder alone does not.  No result depends on P or W.
static inline NlmcWaveRoundsShape nlmc_wave_long_rounds_shape(int n, int n_pad, int L, int ladders, int n_cu, int knob_ladders)
{
    NlmcWaveRoundsShape s = {0, 1, 1, 1, 0, 0, 0, 0};
    if (n < NLMC_WAVE_LONG_MIN_N || n > NLMC_WAVE_LONG_MAX_N || n_pad < n || L < 1 || L > 64 || ladders < 1) return s;
    const int R = nlmc_wave_fields(n);
    if (n_pad > 64 * R) return s;                       // the padded state row must fit a matrix row
    for (int p_max = 0;;) {
        const NlmcWaveLadders g = nlmc_wave_ladders(L, ladders, n_cu, knob_ladders, p_max);
        const size_t total = (size_t)nlmc_wave_long_rounds_layout(n, n_pad, g.P * L, g.W).total;
        if (total <= NLMC_WAVE_LONG_LDS_MAX) {
            s.R = R; s.P = g.P; s.C = g.C; s.W = g.W; s.blocks = g.blocks;
            s.lds = total;
            s.stride = (size_t)64 * (size_t)R;
            return s;
        }
        if (g.P == 1) return s;                         // one ladder alone does not fit
        p_max = g.P - 1;
    }
}
