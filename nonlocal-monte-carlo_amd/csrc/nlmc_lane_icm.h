// nlmc_lane_icm.h -- connected components of the disagreement graph of a pair of chains as lane code (gfx950 / wave64), plain C++: no
// HIP type, so that a host program can check it (scripts/lane_icm_check.cpp does, against a BFS, under the sanitizers).
//
// k_icm_round (csrc/nlmc_pt_icm.h) spends a workgroup and a union-find with compare-and-swap on one pair.  Here a LANE owns a pair:
// the two configurations are columns of the transposed byte planes of the lane kernels (csrc/nlmc_lanes.h), the labels a plane of
// their own, 16 bits per (spin, pair).  The 64 pairs of a wave walk the same rows in lock step: the visited spin is wave-uniform, its
// CSR row is read through uniform addresses (scalar loads), and an entry costs every lane one LDS read.  No atomic, no barrier.
//
//   candidate : spin k with s_a[k] * s_b[k] == -1; every other spin holds NLMC_ICM_AGREE
//   start     : a candidate holds its own index
//   one pass  : spins 0 .. n-1, then n-1 .. 0, in place: a candidate takes the minimum of its label and the labels of the candidates
//               among its neighbours (NLMC_ICM_AGREE is the largest 16-bit value: the minimum leaves it out by itself)
//   repeat    : while any pair of the wave changed a label (a pair that is done keeps walking and changes nothing)
//   end       : every candidate holds the smallest member of its component -- the root k_icm_round ends with, and the order
//               find_disagreement_clusters lists the clusters in
// Edges are k_icm_round's: stored off-diagonal entries whose coupling is non-zero in either representation; J is symmetric (the
// sweeps read the same rows), so the labels of the two ends of an edge meet whichever row is walked.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NLMC_ICM_HD __host__ __device__
#else
#define NLMC_ICM_HD
#endif

#if defined(__HIP_DEVICE_COMPILE__)
// read-only data of the launch through the constant address space: a uniform address gives a scalar load (lane_ro<true>, nlmc_lanes.h)
#define NLMC_ICM_RO(T, p) (*(const T __attribute__((address_space(4))) *)(p))
// true where any lane of the wave says so: the loops below stay wave-uniform
#define NLMC_ICM_ANY(x) (__ballot(x) != 0ull)
#else
#define NLMC_ICM_RO(T, p) (*(p))
#define NLMC_ICM_ANY(x) (x)
#endif

#define NLMC_ICM_AGREE 0xFFFFu

// The graph as the kernels hold it (CsrDev, csrc/nlmc_kernels.h): edge32[e] = { col, q } as two int32.
struct LaneIcmGraph {
    int n;
    const int32_t *rowptr;
    const int32_t *edge32;   // [nnz][2]
    const double *val64;     // [nnz]
};

// The pair of one lane: spin k of configuration a at sa[k * sstride], of b at sb[k * sstride]; its label at lab[k * lstride].
struct LaneIcmPair {
    int8_t *sa, *sb;
    int sstride;
    uint16_t *lab;
    int lstride;
};

NLMC_ICM_HD inline void nlmc_lane_icm_start(const LaneIcmGraph &g, const LaneIcmPair &p)
{
    for (int k = 0; k < g.n; ++k) {
        const bool d = (int)p.sa[k * p.sstride] * (int)p.sb[k * p.sstride] == -1;
        p.lab[k * p.lstride] = (uint16_t)(d ? (unsigned)k : NLMC_ICM_AGREE);
    }
}

// spin k takes the minimum over its row; true when its label changed
NLMC_ICM_HD inline bool nlmc_lane_icm_visit(const LaneIcmGraph &g, const LaneIcmPair &p, int k)
{
    const unsigned own = p.lab[k * p.lstride];
    unsigned m = own;
    const int rs = NLMC_ICM_RO(int32_t, g.rowptr + k), re = NLMC_ICM_RO(int32_t, g.rowptr + k + 1);
    for (int e = rs; e < re; ++e) {
        const int j = NLMC_ICM_RO(int32_t, g.edge32 + 2 * e), q = NLMC_ICM_RO(int32_t, g.edge32 + 2 * e + 1);
        if (q == 0 && NLMC_ICM_RO(double, g.val64 + e) == 0.0) continue;       // a stored zero is no edge (wave-uniform)
        const unsigned lj = p.lab[j * p.lstride];                             // (j == k, the diagonal: its own label)
        m = lj < m ? lj : m;
    }
    const bool ch = own != NLMC_ICM_AGREE && m != own;
    if (ch) p.lab[k * p.lstride] = (uint16_t)m;
    return ch;
}

// one pass, down and up; true when a label of this pair changed
NLMC_ICM_HD inline bool nlmc_lane_icm_pass(const LaneIcmGraph &g, const LaneIcmPair &p)
{
    bool ch = false;
    for (int k = 0; k < g.n; ++k) ch |= nlmc_lane_icm_visit(g, p, k);
    for (int k = g.n - 1; k >= 0; --k) ch |= nlmc_lane_icm_visit(g, p, k);
    return ch;
}

// Labels of the pair's disagreement components.  Pass i carries a component's smallest index at least i edges further, a component
// has at most n - 1 edges on a shortest path, and one more pass sees that nothing changes: n passes are enough for any graph.
// false: the n-th pass still changed a label of this pair (cannot happen; the caller reports it as k_icm_round's n_components = -1).
NLMC_ICM_HD inline bool nlmc_lane_icm_components(const LaneIcmGraph &g, const LaneIcmPair &p)
{
    nlmc_lane_icm_start(g, p);
    bool mine = false;
    for (int pass = 0; pass < g.n; ++pass) {
        mine = nlmc_lane_icm_pass(g, p);
        if (!NLMC_ICM_ANY(mine)) return true;
    }
    return !mine;
}
