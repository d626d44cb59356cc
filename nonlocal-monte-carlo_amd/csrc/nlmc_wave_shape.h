// nlmc_wave_shape.h -- host-side launch shapes of the wave-per-chain sweeps (csrc/nlmc_waves.h, csrc/nlmc_waves_long.h) and of the
// tempering rounds inside a wave launch (csrc/nlmc_wave_rounds.h, csrc/nlmc_wave_long_rounds.h), pure functions with no HIP in them
// (checked on the host under the sanitizers: scripts/wave_shape_check.cpp, scripts/wave_long_shape_check.cpp,
// scripts/wave_rounds_shape_check.cpp, scripts/wave_long_rounds_shape_check.cpp).  No result depends on W or P.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NLMC_WS_HD __host__ __device__
#else
#define NLMC_WS_HD
#endif

#define NLMC_WAVE_JLDS_N 192      // longest chain whose matrix the workgroup stages in LDS: n n_pad 4 <= 144 KB

struct NlmcWaveShape {
    int R;            // fields per lane: 1, 2 or 4 (n <= 64 R); 0: the chain does not fit
    int W;            // waves (= rows of the call) per workgroup, 1 .. 16
    int blocks;       // workgroups: ceil(rows / W)
    int jlds;         // the matrix is staged in LDS
    size_t lds;       // dynamic LDS of the launch in bytes
    size_t stride;    // row stride of the matrix in global memory, in ints: 64 R
};

// rows >= 1.  n_cu: compute units of the device.  knob_waves: NLMC_WAVE_WAVES (0: unset).  allow_lds: NLMC_WAVE_JLDS is not 0.
// Enough workgroups to cover the compute units first, then up to 16 waves per workgroup.
static inline NlmcWaveShape nlmc_wave_shape(int n, int n_pad, int rows, int n_cu, int knob_waves, int allow_lds)
{
    NlmcWaveShape s = {0, 1, 0, 0, 0, 0};
    if (n < 1 || n > 256 || n_pad < n || rows < 1) return s;
    s.R = n <= 64 ? 1 : n <= 128 ? 2 : 4;
    s.stride = (size_t)64 * (size_t)s.R;
    long long w = knob_waves > 0 ? knob_waves : ((long long)rows + (n_cu > 0 ? n_cu : 1) - 1) / (n_cu > 0 ? n_cu : 1);
    if (w < 1) w = 1;
    if (w > 16) w = 16;
    s.W = (int)w;
    s.blocks = (int)(((long long)rows + s.W - 1) / s.W);
    s.jlds = allow_lds && n <= NLMC_WAVE_JLDS_N;
    s.lds = s.jlds ? (size_t)n * (size_t)n_pad * sizeof(int) : 0;
    return s;
}

// ---- long chains, a wave per chain (csrc/nlmc_waves_long.h: k_sweep_waves_long), 256 < n <= 1024 ------------------------------------------
#define NLMC_WAVE_LONG_MIN_N 257                        // NLMC_WAVE_N + 1: shorter chains have k_sweep_waves
#define NLMC_WAVE_LONG_MAX_N 1024                       // NLMC_WAVE_LONG_N of include/nlmc.h
#define NLMC_WAVE_LONG_LDS_MAX ((size_t)158 * 1024)     // dynamic LDS a workgroup may ask for (NLMC_LDS_BYTES_MAX of csrc/nlmc.hip)

// The LDS region a wave keeps to itself, each part 16-byte aligned: X [64 R] int32 (a word per lane and register: the write-back of a
// flip needs no bounds) | thresholds [4 ceil(n / 4)] float | spins [n_pad] int8 | phase flags [n_pad] int8.  The kernel and the shape
// function both take the layout from here.
struct NlmcWaveLongRegion { int w_off, s_off, f_off, bytes; };
NLMC_WS_HD static inline NlmcWaveLongRegion nlmc_wave_long_region(int n, int n_pad)
{
    NlmcWaveLongRegion g;
    g.w_off = 256 * (n <= 512 ? 8 : 16);
    g.s_off = g.w_off + 16 * ((n + 3) / 4);
    g.f_off = g.s_off + ((n_pad + 15) & ~15);
    g.bytes = g.f_off + ((n_pad + 15) & ~15);
    return g;
}

struct NlmcWaveLongShape {
    int R;            // fields per lane: 8 (n <= 512) or 16; 0: the chain does not fit
    int W;            // waves (= rows of the call) per workgroup, 1 .. 16, as many as the LDS holds regions at most
    int blocks;       // workgroups: ceil(rows / W)
    size_t region;    // LDS of one wave in bytes (nlmc_wave_long_region)
    size_t lds;       // dynamic LDS of the launch in bytes: W regions
    size_t stride;    // row stride of the matrix in global memory, in ints: 64 R
};

// rows >= 1.  n_cu: compute units of the device.  knob_waves: NLMC_WAVE_WAVES (0: unset).  Enough workgroups to cover the compute
// units first, then up to 16 waves per workgroup, or as many as have their regions in a workgroup's LDS.
static inline NlmcWaveLongShape nlmc_wave_long_shape(int n, int n_pad, int rows, int n_cu, int knob_waves)
{
    NlmcWaveLongShape s = {0, 1, 0, 0, 0, 0};
    if (n < NLMC_WAVE_LONG_MIN_N || n > NLMC_WAVE_LONG_MAX_N || n_pad < n || rows < 1) return s;
    const int R = n <= 512 ? 8 : 16;
    if (n_pad > 64 * R) return s;                       // the padded state row must fit a matrix row
    s.R = R;
    s.stride = (size_t)64 * (size_t)R;
    s.region = (size_t)nlmc_wave_long_region(n, n_pad).bytes;
    long long w = knob_waves > 0 ? knob_waves : ((long long)rows + (n_cu > 0 ? n_cu : 1) - 1) / (n_cu > 0 ? n_cu : 1);
    const long long fit = (long long)(NLMC_WAVE_LONG_LDS_MAX / s.region);      // >= 15: a region is at most 10 KB
    if (w > fit) w = fit;
    if (w < 1) w = 1;
    if (w > 16) w = 16;
    s.W = (int)w;
    s.blocks = (int)(((long long)rows + s.W - 1) / s.W);
    s.lds = (size_t)s.W * s.region;
    return s;
}

// ---- tempering rounds inside a wave launch (csrc/nlmc_wave_rounds.h: k_rounds_waves): a workgroup holds P whole ladders ----------------
#define NLMC_WAVE_ROUNDS_LDS_MAX ((size_t)158 * 1024)   // dynamic LDS a workgroup may ask for (NLMC_LDS_BYTES_MAX of csrc/nlmc.hip)

struct NlmcWaveRoundsShape {
    int R;            // fields per lane: 1, 2 or 4; 0: the chain or the ladder does not fit
    int P;            // whole ladders per workgroup: Q = P L <= 64 chains
    int C;            // chains a wave runs in turn at most: ceil(Q / 16), 1 .. 4
    int W;            // waves per workgroup: ceil(Q / C) <= 16; wave w owns the workgroup's chains w, w + W, .. below Q
    int blocks;       // workgroups: ceil(ladders / P)
    int jlds;         // the matrix is staged in LDS
    size_t stride;    // row stride of the matrix in global memory, in ints: 64 R
    // LDS regions, each 16-byte aligned: matrix [n][n_pad] int32 (jlds) | parked X [Q][R][64] int32 (C > 1) | parked s [Q][R][64]
    // int8 (C > 1) | energies [Q] int64 | maps chain_of_slot [P][L] + slot_of_chain [Q] bytes
    size_t x_off, s_off, e_off, map_off, lds;
};

// ladders >= 1 of L temperatures each.  knob_ladders: NLMC_WAVE_ROUNDS_LADDERS (0: by the rule).  The rule: enough workgroups to cover
// the compute units first, then as many ladders as fit 16 waves (a chain per wave); a ladder of more than 16 temperatures has the
// workgroup to itself and its waves run chains in turn.  No result depends on P or W.
static inline NlmcWaveRoundsShape nlmc_wave_rounds_shape(int n, int n_pad, int L, int ladders, int n_cu, int knob_ladders, int allow_lds)
{
    NlmcWaveRoundsShape s = {0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0};
    if (n < 1 || n > 256 || n_pad < n || n_pad > 256 || L < 1 || L > 64 || ladders < 1) return s;
    s.R = n <= 64 ? 1 : n <= 128 ? 2 : 4;
    s.stride = (size_t)64 * (size_t)s.R;
    const int cu = n_cu > 0 ? n_cu : 1;
    long long p = knob_ladders > 0 ? knob_ladders : ((long long)ladders + cu - 1) / cu;
    const long long cap = knob_ladders > 0 ? 64 / L : (16 / L > 1 ? 16 / L : 1);
    if (p > cap) p = cap;
    if (p > ladders) p = ladders;
    if (p < 1) p = 1;
    s.P = (int)p;
    const int Q = s.P * L;
    s.C = (Q + 15) / 16;
    s.W = (Q + s.C - 1) / s.C;
    s.blocks = (ladders + s.P - 1) / s.P;
    const size_t a16 = 15;
    const size_t park_x = s.C > 1 ? (size_t)Q * s.stride * sizeof(int) : 0, park_s = s.C > 1 ? (size_t)Q * s.stride : 0;
    const size_t rest = ((park_x + a16) & ~a16) + ((park_s + a16) & ~a16) + (((size_t)Q * 8 + a16) & ~a16) + (((size_t)2 * Q + a16) & ~a16);
    const size_t mat = ((size_t)n * (size_t)n_pad * sizeof(int) + a16) & ~a16;
    s.jlds = allow_lds && n <= NLMC_WAVE_JLDS_N && mat + rest <= NLMC_WAVE_ROUNDS_LDS_MAX;
    s.x_off = s.jlds ? mat : 0;
    s.s_off = s.x_off + ((park_x + a16) & ~a16);
    s.e_off = s.s_off + ((park_s + a16) & ~a16);
    s.map_off = s.e_off + (((size_t)Q * 8 + a16) & ~a16);
    s.lds = s.map_off + (((size_t)2 * Q + a16) & ~a16);
    return s;
}

// ---- tempering rounds of long chains inside a wave launch (csrc/nlmc_wave_long_rounds.h: k_rounds_waves_long), 256 < n <= 1024 ----------
// The LDS of a workgroup of Q chains on W waves, each part 16-byte aligned: Q chain regions of chain_bytes each -- X [64 R] int32 (a
// word per lane and register, as in nlmc_wave_long_region) | spins [n_pad] int8 at s_off -- | W threshold regions of w_bytes each,
// [4 ceil(n / 4)] float, one per wave | energies [Q] int64 | maps chain_of_slot [P][L] + slot_of_chain [Q] bytes.  No phase-flag
// plane: these are plain chains.  The kernel and the shape function both take the layout from here.
struct NlmcWaveLongRoundsLayout { int s_off, chain_bytes, w_bytes, w_off, e_off, map_off, total; };
NLMC_WS_HD static inline NlmcWaveLongRoundsLayout nlmc_wave_long_rounds_layout(int n, int n_pad, int Q, int W)
{
    NlmcWaveLongRoundsLayout g;
    g.s_off = 256 * (n <= 512 ? 8 : 16);
    g.chain_bytes = g.s_off + ((n_pad + 15) & ~15);
    g.w_bytes = 16 * ((n + 3) / 4);
    g.w_off = Q * g.chain_bytes;
    g.e_off = g.w_off + W * g.w_bytes;
    g.map_off = g.e_off + ((8 * Q + 15) & ~15);
    g.total = g.map_off + ((2 * Q + 15) & ~15);
    return g;
}

struct NlmcWaveLongRoundsShape {
    int R;            // fields per lane: 8 (n <= 512) or 16; 0: the chain, the ladder or one ladder's regions do not fit
    int P;            // whole ladders per workgroup: Q = P L <= 64 chains
    int C;            // chains a wave runs in turn at most: ceil(Q / 16), 1 .. 4
    int W;            // waves per workgroup: ceil(Q / C) <= 16; wave w owns the workgroup's chains w, w + W, .. below Q
    int blocks;       // workgroups: ceil(ladders / P)
    size_t lds;       // dynamic LDS of the launch in bytes (nlmc_wave_long_rounds_layout of Q, W)
    size_t stride;    // row stride of the matrix in global memory, in ints: 64 R
};

// ladders >= 1 of L temperatures each.  knob_ladders: NLMC_WAVE_ROUNDS_LADDERS (0: by the rule).  The rule of nlmc_wave_rounds_shape --
// enough workgroups to cover the compute units first, then as many ladders as fit 16 waves (a chain per wave); a ladder of more than
// 16 temperatures has the workgroup to itself and its waves run chains in turn -- and on top of it P is lowered until the workgroup's
// regions fit its LDS.  R = 0 where one ladder alone does not.  No result depends on P or W.
static inline NlmcWaveLongRoundsShape nlmc_wave_long_rounds_shape(int n, int n_pad, int L, int ladders, int n_cu, int knob_ladders)
{
    NlmcWaveLongRoundsShape s = {0, 1, 1, 1, 0, 0, 0};
    if (n < NLMC_WAVE_LONG_MIN_N || n > NLMC_WAVE_LONG_MAX_N || n_pad < n || L < 1 || L > 64 || ladders < 1) return s;
    const int R = n <= 512 ? 8 : 16;
    if (n_pad > 64 * R) return s;                       // the padded state row must fit a matrix row
    const int cu = n_cu > 0 ? n_cu : 1;
    long long p = knob_ladders > 0 ? knob_ladders : ((long long)ladders + cu - 1) / cu;
    const long long cap = knob_ladders > 0 ? 64 / L : (16 / L > 1 ? 16 / L : 1);
    if (p > cap) p = cap;
    if (p > ladders) p = ladders;
    if (p < 1) p = 1;
    for (;; --p) {
        const int Q = (int)p * L, C = (Q + 15) / 16, W = (Q + C - 1) / C;
        const NlmcWaveLongRoundsLayout g = nlmc_wave_long_rounds_layout(n, n_pad, Q, W);
        if ((size_t)g.total <= NLMC_WAVE_LONG_LDS_MAX) {
            s.R = R; s.P = (int)p; s.C = C; s.W = W;
            s.blocks = (ladders + s.P - 1) / s.P;
            s.lds = (size_t)g.total;
            s.stride = (size_t)64 * (size_t)R;
            return s;
        }
        if (p == 1) return s;                           // one ladder alone does not fit
    }
}
