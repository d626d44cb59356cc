// Host check of the visiting-order rule of the chain-per-lane sweeps (csrc/nlmc_lane_order.h: nlmc_lane_rank) against
// std::stable_sort on (key, index), for n in {1, 2, 5, 64, 1024} with duplicate keys included.  Build and run under the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/lane_order_check.cpp -o lane_order_check
//   ./lane_order_check
#include "../nonlocal-monte-carlo_amd/csrc/nlmc_lane_order.h"

#include <algorithm>
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>

static int check(int n, uint32_t key_range, uint32_t seed)
{
    std::mt19937 gen(seed);
    std::vector<uint32_t> key((size_t)n);
    for (auto &k : key) k = key_range ? (uint32_t)(gen() % key_range) : (uint32_t)gen();
    std::vector<int> ref((size_t)n);
    std::iota(ref.begin(), ref.end(), 0);
    std::stable_sort(ref.begin(), ref.end(), [&](int a, int b) { return key[(size_t)a] < key[(size_t)b]; });   // ties keep index order
    std::vector<int> perm((size_t)n, -1);
    for (int k = 0; k < n; ++k) {
        const int r = nlmc_lane_rank(key.data(), n, k);
        if (r < 0 || r >= n || perm[(size_t)r] != -1) { std::printf("n = %d: rank %d of spin %d out of range or taken\n", n, r, k); return 1; }
        perm[(size_t)r] = k;
    }
    for (int i = 0; i < n; ++i)
        if (perm[(size_t)i] != ref[(size_t)i]) { std::printf("n = %d, range %u: position %d holds %d, expected %d\n", n, key_range, i, perm[(size_t)i], ref[(size_t)i]); return 1; }
    return 0;
}

int main()
{
    int bad = 0, cases = 0;
    for (int n : {1, 2, 5, 64, 1024})
        for (uint32_t range : {0u, 1u, 2u, 7u, 300u})          // 0: full 32-bit keys; small ranges: many duplicates (1: all keys equal)
            for (uint32_t seed = 1; seed <= 3; ++seed) { bad += check(n, range, seed * 7919u + (uint32_t)n); ++cases; }
    std::printf("%d cases, %d wrong\n", cases, bad);
    return bad ? 1 : 0;
}
