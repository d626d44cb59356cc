// Host check of the launch shape of the NMC phase cycles of long chains in one wave launch (csrc/nlmc_wave_shape.h:
// nlmc_wave_long_nmc_shape, nlmc_wave_long_nmc_region) over every chain length 257 .. 1024 with the padded length the library uses
// (n rounded up to 16) and every row count 1 .. 5000, for several compute-unit counts and knob values: eight or sixteen fields per
// lane hold the chain, the parts of a wave's LDS region are 16-byte aligned, do not overlap and hold what the kernel puts there, the
// sweep parts are those of nlmc_wave_long_region, W regions stay within the dynamic LDS a workgroup may ask for, a workgroup has
// 1 .. 16 waves, and the workgroups cover the rows.  Build and run under the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/wave_long_nmc_shape_check.cpp -o wave_long_nmc_shape_check
//   ./wave_long_nmc_shape_check
#include "../nonlocal-monte-carlo_amd/csrc/nlmc_wave_shape.h"

#include <climits>
#include <cstdio>
#include <initializer_list>

static const size_t LDS_MAX = (size_t)158 * 1024;

static int check(int n, int n_pad, int rows, int n_cu, int knob)
{
    const NlmcWaveShape s = nlmc_wave_long_nmc_shape(n, n_pad, rows, n_cu, knob);
    const int R = n <= 512 ? 8 : 16;
    if (n <= 256 || n > 1024 || n_pad < n || n_pad > 64 * R) return s.R == 0 ? 0 : 1;
    int bad = 0;
    bad += s.R != R || n > 64 * s.R || n_pad > 64 * s.R;                                           // the padded row fits a matrix row
    bad += s.stride != (size_t)64 * (size_t)s.R;
    const NlmcWaveLongNmcRegion g = nlmc_wave_long_nmc_region(n, n_pad);
    const NlmcWaveLongRegion w = nlmc_wave_long_region(n, n_pad);
    // the sweep's parts as k_sweep_waves_long has them: X [64 R] words | thresholds | spins | flags, then best spins | mask
    bad += g.sweep.w_off != w.w_off || g.sweep.s_off != w.s_off || g.sweep.f_off != w.f_off || g.sweep.bytes != w.bytes;
    bad += w.w_off != 256 * s.R || w.w_off < 4 * n_pad || w.s_off < w.w_off + 16 * ((n + 3) / 4) || w.f_off < w.s_off + n_pad;
    bad += g.b_off < w.f_off + n_pad || g.m_off < g.b_off + n_pad || g.bytes < g.m_off + n_pad;    // non-overlap, in this order
    bad += (w.w_off | w.s_off | w.f_off | g.b_off | g.m_off | g.bytes) & 15;                       // float4 stores, word copies; regions follow each other
    bad += g.bytes > 12 * 1024 + 96;                                                               // about twelve bytes a spin
    bad += s.region != (size_t)g.bytes || s.lds != (size_t)s.W * s.region || s.lds > LDS_MAX;
    bad += s.W < 1 || s.W > 16;
    const int fit = (int)(LDS_MAX / s.region) < 16 ? (int)(LDS_MAX / s.region) : 16;               // the knob holds up to what fits
    bad += knob >= 1 && s.W != (knob < fit ? knob : fit);
    bad += (long long)s.blocks * s.W < rows || (long long)(s.blocks - 1) * s.W >= rows;           // cover, no empty workgroup
    if (knob <= 0 && n_cu > 0) {                                                                  // the compute units first, then what fits
        bad += s.W > 1 && (long long)(s.W - 1) * n_cu >= rows;
        bad += s.W < fit && (long long)s.W * n_cu < rows;
    }
    // the rule is nlmc_wave_long_shape's but for W: nothing else moved
    const NlmcWaveShape l = nlmc_wave_long_shape(n, n_pad, rows, n_cu, knob);
    bad += l.R != s.R || l.stride != s.stride || l.jlds != s.jlds || s.W > l.W;
    if (bad) std::printf("n = %d, n_pad = %d, rows = %d, n_cu = %d, knob = %d: R = %d, W = %d, blocks = %d, region = %zu, lds = %zu\n", n, n_pad, rows,
                         n_cu, knob, s.R, s.W, s.blocks, s.region, s.lds);
    return bad ? 1 : 0;
}

int main()
{
    long long bad = 0, cases = 0;
    for (int n = 257; n <= 1024; ++n) {
        const int p16 = (n + 15) / 16 * 16;
        for (int rows = 1; rows <= 5000; ++rows)
            for (int n_cu : {1, 256})
                for (int knob : {0, 4, 16}) { bad += check(n, p16, rows, n_cu, knob); ++cases; }
    }
    // the edges: lengths around the range, padded lengths the library does not use, huge row counts, more knobs
    const int rows_list[] = {1, 16, 17, 4097, 1 << 20, INT_MAX - 1, INT_MAX};
    for (int n = 250; n <= 1030; ++n) {
        const int p16 = (n + 15) / 16 * 16;
        for (int n_pad : {n - 1, n, p16, p16 + 16, 512, 1024, 1040})
            for (int rows : rows_list)
                for (int n_cu : {0, 1, 64, 304})
                    for (int knob : {0, 1, 13, 15, 99}) { bad += check(n, n_pad, rows, n_cu, knob); ++cases; }
    }
    // arguments the host never passes are refused, not computed with
    for (int rows : {0, -1}) { bad += nlmc_wave_long_nmc_shape(300, 304, rows, 256, 0).R != 0; ++cases; }
    bad += nlmc_wave_long_nmc_shape(256, 256, 1, 256, 0).R != 0; ++cases;
    bad += nlmc_wave_long_nmc_shape(1025, 1040, 1, 256, 0).R != 0; ++cases;
    bad += nlmc_wave_long_nmc_shape(300, 288, 1, 256, 0).R != 0; ++cases;
    // the figures the documents quote: thirteen waves at 1024 spins, sixteen up to 512
    bad += nlmc_wave_long_nmc_shape(1024, 1024, 4096, 256, 0).W != 13; ++cases;
    bad += nlmc_wave_long_nmc_shape(512, 512, 4096, 256, 0).W != 16; ++cases;
    std::printf("%lld cases, %lld wrong\n", cases, bad);
    return bad ? 1 : 0;
}
