// Host check of the launch shape of the tempering rounds of long chains inside a wave launch (csrc/nlmc_wave_shape.h:
// nlmc_wave_long_rounds_shape, nlmc_wave_long_rounds_layout) over every chain length 250 .. 1030, ladder length 1 .. 65 and ladder
// counts 1 .. 40, with and without NLMC_WAVE_ROUNDS_LADDERS: every chain of a workgroup is owned by exactly one wave, a workgroup
// holds at most 64 chains on at most 16 waves, the LDS regions (a chain's fields and spins, a wave's thresholds, the energies, the
// maps) are 16-byte aligned, do not overlap and lie inside the total, the total fits the dynamic LDS a workgroup may ask for, P is
// the rule's unless the LDS lowered it (and then P + 1 does not fit), a shape is refused exactly where one ladder alone does not fit,
// and the workgroups cover the ladders.  Build and run under the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/wave_long_rounds_shape_check.cpp -o wave_long_rounds_shape_check
//   ./wave_long_rounds_shape_check
#include "../nonlocal-monte-carlo_amd/csrc/nlmc_wave_shape.h"

#include <algorithm>
#include <cstdio>
#include <initializer_list>
#include <utility>
#include <vector>

// the LDS of P ladders of L, from the layout function
static size_t total_of(int n, int n_pad, int L, int P)
{
    const int Q = P * L, C = (Q + 15) / 16, W = (Q + C - 1) / C;
    return (size_t)nlmc_wave_long_rounds_layout(n, n_pad, Q, W).total;
}

static int check(int n, int L, int ladders, int n_cu, int knob)
{
    const int n_pad = (n + 15) / 16 * 16;
    const NlmcWaveRoundsShape s = nlmc_wave_long_rounds_shape(n, n_pad, L, ladders, n_cu, knob);
    if (n < 257 || n > 1024 || L > 64) return s.R == 0 ? 0 : 1;
    const int R = n <= 512 ? 8 : 16;
    if (n_pad > 64 * R) return s.R == 0 ? 0 : 1;                       // (never with n_pad = n rounded up to 16; kept for the rule)
    // the rule of nlmc_wave_rounds_shape before the LDS has its say
    long long want = knob > 0 ? knob : ((long long)ladders + n_cu - 1) / n_cu;
    const long long cap = knob > 0 ? 64 / L : std::max(16 / L, 1);
    want = std::max(1ll, std::min({want, cap, (long long)ladders}));
    if (total_of(n, n_pad, L, 1) > NLMC_WAVE_LONG_LDS_MAX) return s.R == 0 ? 0 : 1;   // one ladder alone does not fit: refused
    int bad = 0;
    bad += s.R != R || s.stride != (size_t)64 * (size_t)R;
    const int Q = s.P * L;
    bad += s.P < 1 || s.P > want || Q > 64 || s.W < 1 || s.W > 16 || s.C < 1 || s.C > 4 || s.C != (Q + 15) / 16 || s.W != (Q + s.C - 1) / s.C;
    bad += (long long)s.blocks * s.P < ladders || (long long)(s.blocks - 1) * s.P >= ladders;       // the ladders are covered, no empty workgroup
    bad += s.P < want && total_of(n, n_pad, L, s.P + 1) <= NLMC_WAVE_LONG_LDS_MAX;                   // lowered by the LDS and by nothing else
    if (knob == 0) bad += (L > 16 && s.P != 1) || (L <= 16 && s.P * L > 16);                         // a chain per wave by the rule
    // wave w owns chains w, w + W, .. below Q, at most C of them: every chain exactly once
    std::vector<int> owner(Q, 0);
    for (int w = 0; w < s.W; ++w)
        for (int t = 0; t < s.C; ++t)
            if (w + t * s.W < Q) owner[w + t * s.W]++;
    for (int c = 0; c < Q; ++c) bad += owner[c] != 1;
    // regions: per chain X | spins, per wave thresholds, energies, maps -- sorted by offset they must not overlap
    const NlmcWaveLongRoundsLayout g = nlmc_wave_long_rounds_layout(n, n_pad, Q, s.W);
    std::vector<std::pair<size_t, size_t>> reg;                        // (offset, length)
    for (int c = 0; c < Q; ++c) {
        reg.push_back({(size_t)c * g.chain_bytes, (size_t)256 * R});
        reg.push_back({(size_t)c * g.chain_bytes + g.s_off, (size_t)n_pad});
    }
    for (int w = 0; w < s.W; ++w) reg.push_back({(size_t)g.w_off + (size_t)w * g.w_bytes, (size_t)16 * ((n + 3) / 4)});
    reg.push_back({(size_t)g.e_off, (size_t)Q * 8});
    reg.push_back({(size_t)g.map_off, (size_t)2 * Q});
    std::sort(reg.begin(), reg.end());
    for (size_t i = 0; i < reg.size(); ++i) {
        bad += reg[i].first % 16 != 0 || reg[i].first + reg[i].second > (size_t)g.total;
        if (i + 1 < reg.size()) bad += reg[i].first + reg[i].second > reg[i + 1].first;
    }
    bad += s.lds != (size_t)g.total || s.lds > NLMC_WAVE_LONG_LDS_MAX;
    if (bad) std::printf("n = %d, L = %d, ladders = %d, n_cu = %d, knob = %d: R = %d, P = %d, C = %d, W = %d, blocks = %d, total = %zu\n",
                         n, L, ladders, n_cu, knob, s.R, s.P, s.C, s.W, s.blocks, s.lds);
    return bad ? 1 : 0;
}

int main()
{
    int bad = 0, cases = 0;
    for (int n = 250; n <= 1030; ++n)
        for (int L = 1; L <= 65; ++L)
            for (int ladders = 1; ladders <= 40; ++ladders)
                for (int knob : {0, 1, 3, 8, 99}) { bad += check(n, L, ladders, knob == 0 && ladders % 2 ? 4 : 256, knob); ++cases; }
    // the two fixed cases: sixteen chains of 1024 spins, a chain per wave, fit one workgroup; sixty-four do not (256 KB of fields)
    {
        const NlmcWaveRoundsShape s = nlmc_wave_long_rounds_shape(1024, 1024, 16, 1, 256, 0);
        bad += !(s.R == 16 && s.P == 1 && s.C == 1 && s.W == 16 && s.blocks == 1 && s.lds <= NLMC_WAVE_LONG_LDS_MAX); ++cases;
        bad += nlmc_wave_long_rounds_shape(1024, 1024, 64, 1, 256, 0).R != 0; ++cases;
        bad += nlmc_wave_long_rounds_shape(1024, 1024, 64, 7, 256, 3).R != 0; ++cases;
    }
    // arguments the host never passes are refused, not computed with
    for (int ladders : {0, -1}) { bad += nlmc_wave_long_rounds_shape(300, 304, 5, ladders, 256, 0).R != 0; ++cases; }
    bad += nlmc_wave_long_rounds_shape(300, 288, 5, 1, 256, 0).R != 0; ++cases;
    bad += nlmc_wave_long_rounds_shape(300, 304, 0, 1, 256, 0).R != 0; ++cases;
    bad += nlmc_wave_long_rounds_shape(512, 528, 5, 1, 256, 0).R != 0; ++cases;      // a padded row past 64 R
    std::printf("%d cases, %d wrong\n", cases, bad);
    return bad ? 1 : 0;
}
