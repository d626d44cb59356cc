// nlmc_wave_shape.h -- host-side launch shape of the wave-per-chain sweeps (csrc/nlmc_waves.h), a pure function with no HIP in it
// (checked on the host under the sanitizers: scripts/wave_shape_check.cpp).  No result depends on W.
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
