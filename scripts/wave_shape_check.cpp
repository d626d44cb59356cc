// Host check of the launch shape of the wave-per-chain sweeps (csrc/nlmc_wave_shape.h: nlmc_wave_shape) over every chain length
// 1 .. 257, row counts from 1 to 2^31 - 1, compute-unit counts and both knobs: the registers hold the chain, the workgroups cover
// the rows exactly, a workgroup has 1 .. 16 waves, the staged matrix fits the dynamic LDS a workgroup may ask for, and nothing
// overflows on the way.  Build and run under the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/wave_shape_check.cpp -o wave_shape_check
//   ./wave_shape_check
#include "../nonlocal-monte-carlo_amd/csrc/nlmc_wave_shape.h"

#include <climits>
#include <cstdio>
#include <initializer_list>

static int check(int n, int rows, int n_cu, int knob, int allow_lds)
{
    const int n_pad = (n + 15) / 16 * 16;
    const NlmcWaveShape s = nlmc_wave_shape(n, n_pad, rows, n_cu, knob, allow_lds);
    if (n > 256) return s.R == 0 ? 0 : 1;
    int bad = 0;
    bad += !(s.R == 1 || s.R == 2 || s.R == 4) || n > 64 * s.R || (s.R > 1 && n <= 32 * s.R);      // the smallest R that holds the chain
    bad += n_pad > 64 * s.R;                                                                      // the padded row fits a matrix row
    bad += s.stride != (size_t)64 * (size_t)s.R;
    bad += s.W < 1 || s.W > 16 || (knob >= 1 && knob <= 16 && s.W != knob);
    bad += (long long)s.blocks * s.W < rows || (long long)(s.blocks - 1) * s.W >= rows;           // exact cover, no empty workgroup
    if (knob <= 0 && n_cu > 0) {                                                                  // the compute units first, then up to 16 waves
        bad += s.W > 1 && (long long)(s.W - 1) * n_cu >= rows;
        bad += s.W < 16 && (long long)s.W * n_cu < rows;
    }
    bad += s.jlds != (allow_lds && n <= NLMC_WAVE_JLDS_N ? 1 : 0);
    bad += s.lds != (s.jlds ? (size_t)n * (size_t)n_pad * 4 : 0) || s.lds > (size_t)158 * 1024;
    if (bad) std::printf("n = %d, rows = %d, n_cu = %d, knob = %d, lds = %d: R = %d, W = %d, blocks = %d, jlds = %d, lds = %zu\n", n, rows, n_cu, knob,
                         allow_lds, s.R, s.W, s.blocks, s.jlds, s.lds);
    return bad ? 1 : 0;
}

int main()
{
    int bad = 0, cases = 0;
    const int rows_list[] = {1, 2, 15, 16, 17, 255, 256, 257, 1024, 4095, 4096, 4097, 16384, 1 << 20, INT_MAX - 1, INT_MAX};
    for (int n = 1; n <= 257; ++n)
        for (int rows : rows_list)
            for (int n_cu : {0, 1, 64, 256, 304})
                for (int knob : {0, 1, 4, 16, 99})
                    for (int allow : {0, 1}) { bad += check(n, rows, n_cu, knob, allow); ++cases; }
    // arguments the host never passes are refused, not computed with
    for (int rows : {0, -1}) { bad += nlmc_wave_shape(40, 48, rows, 256, 0, 1).R != 0; ++cases; }
    bad += nlmc_wave_shape(0, 0, 1, 256, 0, 1).R != 0; ++cases;
    bad += nlmc_wave_shape(40, 32, 1, 256, 0, 1).R != 0; ++cases;
    std::printf("%d cases, %d wrong\n", cases, bad);
    return bad ? 1 : 0;
}
