// nlmc_wave_shape.h -- host-side launch shapes of the wave-per-chain sweeps (csrc/nlmc_waves.h) and of the tempering rounds inside a wave
// launch (csrc/nlmc_wave_rounds.h), pure functions with no HIP in them (checked on the host under the sanitizers:
// scripts/wave_shape_check.cpp, scripts/wave_rounds_shape_check.cpp).  No result depends on W or P.
#pragma once
#include <stddef.h>

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
