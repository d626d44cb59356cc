// Host check of the lane code for the components of a pair's disagreement graph (csrc/nlmc_lane_icm.h) against a BFS, 64 pairs in
// lock step as a wave walks them: n in {1, 2, 5, 64, 300}; the empty graph, the complete graph, a path numbered by a random
// permutation (several passes), a random degree-3 graph, a graph with stored zero couplings and a diagonal; pairs that agree
// everywhere, disagree everywhere, and at random.  Build and run under the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/lane_icm_check.cpp -o lane_icm_check
//   ./lane_icm_check
#include "../nonlocal-monte-carlo_amd/csrc/nlmc_lane_icm.h"

#include <algorithm>
#include <cstdio>
#include <numeric>
#include <queue>
#include <random>
#include <set>
#include <utility>
#include <vector>

namespace {

constexpr int LANES = 64;

struct Graph {
    int n = 0;
    std::vector<int32_t> rowptr, edge32;
    std::vector<double> val64;
};

// entries (k, j, q, v) given once per unordered pair are stored in both rows; (k, k, ..) is a diagonal entry
struct Entry { int k, j, q; double v; };

Graph build(int n, const std::vector<Entry> &es)
{
    std::vector<std::vector<Entry>> rows((size_t)n);
    for (const Entry &e : es) {
        rows[(size_t)e.k].push_back(e);
        if (e.j != e.k) rows[(size_t)e.j].push_back({e.j, e.k, e.q, e.v});
    }
    Graph g;
    g.n = n;
    g.rowptr.push_back(0);
    for (auto &r : rows) {
        std::sort(r.begin(), r.end(), [](const Entry &a, const Entry &b) { return a.j < b.j; });
        for (const Entry &e : r) { g.edge32.push_back(e.j); g.edge32.push_back(e.q); g.val64.push_back(e.v); }
        g.rowptr.push_back((int32_t)g.val64.size());
    }
    return g;
}

enum Kind { EMPTY, COMPLETE, PATH, DEG3, ZEROS };
const char *const kind_name[] = {"empty", "complete", "permuted path", "degree 3", "stored zeros + diagonal"};

Graph make(Kind kind, int n, std::mt19937 &gen)
{
    std::vector<Entry> es;
    std::set<std::pair<int, int>> seen;
    auto add = [&](int a, int b, int q, double v) {
        if (a == b || !seen.insert({std::min(a, b), std::max(a, b)}).second) return;
        es.push_back({a, b, q, v});
    };
    if (kind == COMPLETE)
        for (int a = 0; a < n; ++a) for (int b = a + 1; b < n; ++b) add(a, b, (a + b) % 2 ? 3 : -3, 0.75);
    if (kind == PATH) {
        std::vector<int> perm((size_t)n);
        std::iota(perm.begin(), perm.end(), 0);
        std::shuffle(perm.begin(), perm.end(), gen);
        for (int i = 0; i + 1 < n; ++i) add(perm[(size_t)i], perm[(size_t)i + 1], 1, 1.0);
    }
    if (kind == DEG3 || kind == ZEROS)
        for (int a = 0; a < n; ++a) for (int t = 0; t < 2; ++t) add(a, (int)(gen() % (unsigned)n), -2, -0.5);
    if (kind == ZEROS) {
        // a third of the entries stored with both representations zero (no edge), a third zero in one of them only (an edge)
        for (size_t i = 0; i < es.size(); ++i) {
            if (i % 3 == 0) { es[i].q = 0; es[i].v = 0.0; }
            else if (i % 3 == 1) { if (i % 2) es[i].q = 0; else es[i].v = 0.0; }
        }
        for (int a = 0; a < n; a += 2) es.push_back({a, a, 5, 1.25});
    }
    return build(n, es);
}

// smallest member of the component of every candidate (NLMC_ICM_AGREE elsewhere), by BFS from the spins in ascending order
std::vector<uint16_t> reference(const Graph &g, const std::vector<int8_t> &a, const std::vector<int8_t> &b)
{
    const int n = g.n;
    std::vector<uint16_t> lab((size_t)n, (uint16_t)NLMC_ICM_AGREE);
    std::vector<char> cand((size_t)n), done((size_t)n, 0);
    for (int k = 0; k < n; ++k) cand[(size_t)k] = a[(size_t)k] * b[(size_t)k] == -1;
    for (int r = 0; r < n; ++r) {
        if (!cand[(size_t)r] || done[(size_t)r]) continue;
        std::queue<int> q;
        q.push(r);
        done[(size_t)r] = 1;
        while (!q.empty()) {
            const int k = q.front();
            q.pop();
            lab[(size_t)k] = (uint16_t)r;
            for (int e = g.rowptr[(size_t)k]; e < g.rowptr[(size_t)k + 1]; ++e) {
                const int j = g.edge32[2 * (size_t)e];
                if (g.edge32[2 * (size_t)e + 1] == 0 && g.val64[(size_t)e] == 0.0) continue;
                if (j == k || !cand[(size_t)j] || done[(size_t)j]) continue;
                done[(size_t)j] = 1;
                q.push(j);
            }
        }
    }
    return lab;
}

int check(Kind kind, int n, uint32_t seed, int &max_passes)
{
    std::mt19937 gen(seed);
    const Graph G = make(kind, n, gen);
    const LaneIcmGraph g{n, G.rowptr.data(), G.edge32.data(), G.val64.data()};
    // the two configurations of lane l: columns l and 64 + l of one transposed plane; lane 0 agrees everywhere, lane 1 disagrees
    // everywhere, the others disagree on a random share of the spins
    std::vector<int8_t> s((size_t)n * 2 * LANES);
    for (int l = 0; l < LANES; ++l) {
        const unsigned share = l == 0 ? 0u : l == 1 ? 100u : 5u + (unsigned)(gen() % 91u);
        for (int k = 0; k < n; ++k) {
            const int8_t va = (gen() & 1u) ? 1 : -1;
            const bool dis = (gen() % 100u) < share;
            s[(size_t)k * 2 * LANES + (size_t)l] = va;
            s[(size_t)k * 2 * LANES + LANES + (size_t)l] = dis ? (int8_t)-va : va;
        }
    }
    std::vector<uint16_t> lab((size_t)n * LANES, 0), solo((size_t)n * LANES, 0);
    auto pair_of = [&](std::vector<uint16_t> &plane, int l) {
        return LaneIcmPair{s.data() + l, s.data() + LANES + l, 2 * LANES, plane.data() + l, LANES};
    };
    // lock step: every lane walks every pass until no lane changed a label; a lane that is done changes nothing afterwards
    for (int l = 0; l < LANES; ++l) nlmc_lane_icm_start(g, pair_of(lab, l));
    std::vector<char> done((size_t)LANES, 0);
    int passes = 0;
    for (;;) {
        if (passes == n) { std::printf("%s, n = %d: still changing in pass %d\n", kind_name[kind], n, passes); return 1; }
        bool any = false;
        for (int l = 0; l < LANES; ++l) {
            const bool ch = nlmc_lane_icm_pass(g, pair_of(lab, l));
            if (ch && done[(size_t)l]) { std::printf("%s, n = %d: lane %d changed a label after a pass without change\n", kind_name[kind], n, l); return 1; }
            if (!ch) done[(size_t)l] = 1;
            any |= ch;
        }
        ++passes;
        if (!any) break;
    }
    max_passes = std::max(max_passes, passes);
    for (int l = 0; l < LANES; ++l) {
        if (!nlmc_lane_icm_components(g, pair_of(solo, l))) { std::printf("%s, n = %d: lane %d did not converge\n", kind_name[kind], n, l); return 1; }
        std::vector<int8_t> a((size_t)n), b((size_t)n);
        for (int k = 0; k < n; ++k) { a[(size_t)k] = s[(size_t)k * 2 * LANES + (size_t)l]; b[(size_t)k] = s[(size_t)k * 2 * LANES + LANES + (size_t)l]; }
        const std::vector<uint16_t> ref = reference(G, a, b);
        for (int k = 0; k < n; ++k) {
            const uint16_t got = lab[(size_t)k * LANES + (size_t)l], one = solo[(size_t)k * LANES + (size_t)l];
            if (got != ref[(size_t)k] || one != ref[(size_t)k]) {
                std::printf("%s, n = %d, lane %d, spin %d: label %u (alone %u), expected %u\n", kind_name[kind], n, l, k, (unsigned)got,
                            (unsigned)one, (unsigned)ref[(size_t)k]);
                return 1;
            }
        }
    }
    return 0;
}

}  // namespace

int main()
{
    int bad = 0, cases = 0, max_passes = 0;
    for (int n : {1, 2, 5, 64, 300})
        for (Kind kind : {EMPTY, COMPLETE, PATH, DEG3, ZEROS})
            for (uint32_t seed = 1; seed <= 3; ++seed) { bad += check(kind, n, seed * 7919u + (uint32_t)n, max_passes); ++cases; }
    std::printf("%d cases of 64 pairs, %d wrong, at most %d passes\n", cases, bad, max_passes);
    return bad ? 1 : 0;
}
