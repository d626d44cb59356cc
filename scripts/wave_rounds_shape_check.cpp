// Host check of the launch shape of the tempering rounds inside a wave launch (csrc/nlmc_wave_shape.h: nlmc_wave_rounds_shape, nlmc_wave_rounds_layout) over
// every chain length 1 .. 257, ladder length 1 .. 65 and ladder counts 1 .. 40, with and without NLMC_WAVE_ROUNDS_LADDERS, with the
// staging allowed and not: every chain of a workgroup is owned by exactly one wave, a workgroup holds at most 64 chains on at most 16
// waves, the LDS regions are 16-byte aligned, do not overlap and lie inside the total, the total fits the dynamic LDS a workgroup may
// ask for, and the workgroups cover the ladders.  Build and run under the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/wave_rounds_shape_check.cpp -o wave_rounds_shape_check
//   ./wave_rounds_shape_check
#include "../nonlocal-monte-carlo_amd/csrc/nlmc_wave_shape.h"

#include <cstdio>
#include <initializer_list>
#include <vector>

static int check(int n, int L, int ladders, int n_cu, int knob, int allow_lds)
{
    const int n_pad = (n + 15) / 16 * 16;
    const NlmcWaveRoundsShape s = nlmc_wave_rounds_shape(n, n_pad, L, ladders, n_cu, knob, allow_lds);
    if (n > 256 || L > 64) return s.R == 0 ? 0 : 1;
    int bad = 0;
    bad += !(s.R == 1 || s.R == 2 || s.R == 4) || n > 64 * s.R || (s.R > 1 && n <= 32 * s.R) || n_pad > 64 * s.R;
    bad += s.stride != (size_t)64 * (size_t)s.R;
    const int Q = s.P * L;
    bad += s.P < 1 || Q > 64 || s.W < 1 || s.W > 16 || s.C < 1 || s.C > 4 || s.C != (Q + 15) / 16;
    bad += (long long)s.blocks * s.P < ladders || (long long)(s.blocks - 1) * s.P >= ladders;       // the ladders are covered, no empty workgroup
    if (knob > 0) bad += s.P != (knob < 64 / L ? (knob < ladders ? knob : ladders) : (64 / L < ladders ? 64 / L : ladders));
    else {
        bad += L > 16 && s.P != 1;
        bad += L <= 16 && s.P * L > 16;                                                              // a chain per wave by the rule
        if (n_cu > 0) bad += s.P > 1 && (long long)(s.P - 1) * n_cu >= ladders;                      // the compute units first
    }
    // wave w owns chains w, w + W, .. below Q, at most C of them: every chain exactly once
    std::vector<int> owner(Q, 0);
    for (int w = 0; w < s.W; ++w)
        for (int t = 0; t < s.C; ++t)
            if (w + t * s.W < Q) owner[w + t * s.W]++;
    for (int c = 0; c < Q; ++c) bad += owner[c] != 1;
    // regions: matrix | parked X | parked s | energies | maps
    const size_t mat = s.jlds ? (size_t)n * n_pad * 4 : 0, px = s.C > 1 ? (size_t)Q * s.stride * 4 : 0, ps = s.C > 1 ? (size_t)Q * s.stride : 0;
    const NlmcWaveRoundsLayout g = nlmc_wave_rounds_layout(n, n_pad, Q, s.C, s.jlds);
    bad += s.lds != g.total;
    const size_t off[5] = {0, g.x_off, g.s_off, g.e_off, g.map_off}, len[5] = {mat, px, ps, (size_t)Q * 8, (size_t)2 * Q};
    for (int i = 0; i < 5; ++i) {
        bad += off[i] % 16 != 0 || off[i] + len[i] > s.lds;
        if (i + 1 < 5) bad += off[i] + len[i] > off[i + 1];
    }
    bad += s.lds > NLMC_WAVE_LONG_LDS_MAX;
    const size_t rest = s.lds - g.x_off;
    const size_t mat16 = ((size_t)n * n_pad * 4 + 15) & ~(size_t)15;
    bad += s.jlds != ((allow_lds && n <= NLMC_WAVE_JLDS_N && mat16 + rest <= NLMC_WAVE_LONG_LDS_MAX) ? 1 : 0);
    if (bad) std::printf("n = %d, L = %d, ladders = %d, n_cu = %d, knob = %d, lds = %d: R = %d, P = %d, C = %d, W = %d, blocks = %d, jlds = %d, total = %zu\n",
                         n, L, ladders, n_cu, knob, allow_lds, s.R, s.P, s.C, s.W, s.blocks, s.jlds, s.lds);
    return bad ? 1 : 0;
}

int main()
{
    int bad = 0, cases = 0;
    for (int n = 1; n <= 257; ++n)
        for (int L = 1; L <= 65; ++L)
            for (int ladders = 1; ladders <= 40; ++ladders)
                for (int knob : {0, 1, 3, 8, 99})
                    for (int allow : {0, 1}) { bad += check(n, L, ladders, knob == 0 && ladders % 2 ? 4 : 256, knob, allow); ++cases; }
    // the case the ceiling decides: a 64-rung ladder with parked state next to a 144 KB matrix falls back to global rows
    bad += nlmc_wave_rounds_shape(192, 192, 64, 1, 256, 0, 1).jlds != 0; ++cases;
    bad += nlmc_wave_rounds_shape(192, 192, 16, 1, 256, 0, 1).jlds != 1; ++cases;
    // arguments the host never passes are refused, not computed with
    for (int ladders : {0, -1}) { bad += nlmc_wave_rounds_shape(40, 48, 5, ladders, 256, 0, 1).R != 0; ++cases; }
    bad += nlmc_wave_rounds_shape(0, 0, 5, 1, 256, 0, 1).R != 0; ++cases;
    bad += nlmc_wave_rounds_shape(40, 32, 5, 1, 256, 0, 1).R != 0; ++cases;
    bad += nlmc_wave_rounds_shape(40, 48, 0, 1, 256, 0, 1).R != 0; ++cases;
    std::printf("%d cases, %d wrong\n", cases, bad);
    return bad ? 1 : 0;
}
