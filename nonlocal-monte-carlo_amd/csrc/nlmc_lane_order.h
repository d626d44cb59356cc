// nlmc_lane_order.h -- the visiting-order rule of the chain-per-lane sweeps (csrc/nlmc_lanes.h) as plain C++: no HIP type, so
// that a host program can check it (scripts/lane_order_check.cpp does, against std::stable_sort, under the sanitizers).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NLMC_HD __host__ __device__
#else
#define NLMC_HD
#endif

// spin j comes before spin k: smaller key first, equal keys by index (the rule of `precedes`, csrc/nlmc_kernels.h)
NLMC_HD inline bool nlmc_lane_precedes(uint32_t kj, int j, uint32_t kk, int k) { return kj < kk || (kj == kk && j < k); }

// position of spin k in the visiting order of the keys key[0 .. n): the number of spins that come before it.  The order is total,
// so the ranks of the n spins are a permutation of 0 .. n - 1.  O(n) per spin: enough at n <= NLMC_LANE_N.
NLMC_HD inline int nlmc_lane_rank(const uint32_t *key, int n, int k)
{
    const uint32_t kk = key[k];
    int r = 0;
    for (int j = 0; j < n; ++j) r += nlmc_lane_precedes(key[j], j, kk, k) ? 1 : 0;
    return r;
}
