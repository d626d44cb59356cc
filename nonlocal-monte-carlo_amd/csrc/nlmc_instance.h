// nlmc_instance.h -- what nlmc_create derives from the caller's instance before it asks for a device: the argument and CSR checks,
// the row facts, the fixed-point scales, the quantised couplings and the format facts.  Plain C++: no HIP type, so that a host
// program can check it (scripts/instance_prep_check.cpp does, under the sanitizers; tests/test_instance_prep_cpu.py runs it).
#pragma once
#include "../../include/nlmc.h"

#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <vector>

// 8-byte packed CSR entry of the "f32" throughput path (one dwordx2 load): column and the coupling in 24-bit fixed
// point, q = rint(J 2^qs).  The field of a spin is then an exact int32, independent of summation order.
struct EdgeQ { int32_t col; int32_t q; };

struct NlmcInstance {
    const char *err = "";              // the text of a refusal (nlmc_last_error(NULL) after a failed nlmc_create)
    bool has_diag = false;             // a stored diagonal entry is not 0
    bool has_zero_vals = false;        // a stored entry is 0.0
    int max_deg = 0;
    int n_gt1 = 0, n_gt2 = 0;          // rows longer than one / two row windows (fz_w entries) of a fused plan
    int qs = 0, escale = 0;            // field scale (Jq = rint(J 2^qs)) and energy scale
    bool fits16 = false;               // n <= 65535 and every Jq fits 16 bits (compact schedule entries: col << 16 | (Jq & 0xFFFF))
    bool pm1 = false;                  // every Jq is +-1 (sign format: col | (Jq < 0) << 15)
    bool exact_q = false;              // every J is Jq 2^-qs exactly (packed fp64 schedule window)
    bool exact_h = false;              // every h is hq 2^-qs exactly
    bool no_field = false;             // every hq is 0: no item of a fused plan carries a field (the head stream's condition)
    int xmax = 0;                      // max over rows of sum |Jq| + |hq|: the range of the integer field
    std::vector<EdgeQ> e32;            // [max(nnz, 1)] (column, Jq) in CSR order: what nlmc_create uploads
    std::vector<int32_t> hq;           // [n]
};

// NLMC_OK, or the code of the refusal with its text in I.err; nothing of I is valid then.  `out` is only compared with NULL.
inline int nlmc_instance_prepare(NlmcInstance &I, const void *out, int n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                                 const double *vals, const double *h, int n_chains, int chain_base, int n_chains_global, int fz_w)
{
    auto refuse = [&](int code, const char *msg) { I.err = msg; return code; };
    if (!out) return refuse(NLMC_ERR_ARG, "nlmc_create: out is NULL");
    if (n < 1 || nnz < 0 || !rowptr || (nnz > 0 && (!colidx || !vals)) || !h || n_chains < 0 || chain_base < 0 ||
        n_chains_global < chain_base + n_chains)
        return refuse(NLMC_ERR_ARG, "nlmc_create: bad sizes or NULL arrays");
    if (n > NLMC_MAX_N) return refuse(NLMC_ERR_UNSUPPORTED, "nlmc_create: n exceeds NLMC_MAX_N");
    if (rowptr[0] != 0 || rowptr[n] != nnz) return refuse(NLMC_ERR_ARG, "nlmc_create: rowptr[0] != 0 or rowptr[n] != nnz");
    for (int k = 0; k < n; ++k) {
        // the row's end is bounded by nnz before any of its entries is read (rowptr = {0, 5, 2} with nnz = 2 passes the check above)
        if (rowptr[k + 1] < rowptr[k] || rowptr[k + 1] > nnz) return refuse(NLMC_ERR_ARG, "nlmc_create: rowptr not monotone");
        I.max_deg = std::max(I.max_deg, (int)(rowptr[k + 1] - rowptr[k]));
        I.n_gt1 += (rowptr[k + 1] - rowptr[k]) > fz_w;
        I.n_gt2 += (rowptr[k + 1] - rowptr[k]) > 2 * fz_w;
        for (int e = rowptr[k]; e < rowptr[k + 1]; ++e) {
            if (colidx[e] < 0 || colidx[e] >= n) return refuse(NLMC_ERR_ARG, "nlmc_create: column index out of range");
            if (colidx[e] == k && vals[e] != 0.0) I.has_diag = true;
            if (vals[e] == 0.0) I.has_zero_vals = true;
        }
    }

    // fixed-point scales.  Energies: integers in units of 2^-escale, |E| <= sum|J|/2 + sum|h|.  Couplings of the "f32"
    // throughput path: Jq = rint(J 2^qs), hq = rint(h 2^qs) with qs the largest exponent such that every |Jq| fits a
    // signed 24-bit multiplier and every row sum  sum|Jq| + |hq|  fits int32 (the field is then an exact int32);
    // qs <= escale <= qs + 29, so that an energy delta is the field times +-2^(escale - qs + 1) in one 32 x 32 -> 64
    // bit multiply-add.  (Restated in oracle/nlo.c: nlo_field_scale.)
    double bound = 0.0, maxabs = 0.0, maxh = 0.0;
    for (int64_t e = 0; e < nnz; ++e) { bound += std::fabs(vals[e]) * 0.5; maxabs = std::max(maxabs, std::fabs(vals[e])); }
    for (int k = 0; k < n; ++k) { bound += std::fabs(h[k]); maxh = std::max(maxh, std::fabs(h[k])); }
    int ex = 0;
    std::frexp(std::max(bound, 1.0), &ex);       // bound < 2^ex
    const int escale0 = std::max(0, std::min(52, 60 - ex));
    int qs = 0;
    auto rq = [](double v, int q) { return (int64_t)std::llrint(std::ldexp(v, q)); };
    const double ref = maxabs > 0.0 ? maxabs : maxh;
    if (ref > 0.0) {
        int exr = 0;
        std::frexp(ref, &exr);
        qs = std::min(23 - exr, escale0);
        for (;;) {
            bool ok = true;
            for (int k = 0; k < n && ok; ++k) {
                int64_t row = std::llabs(rq(h[k], qs));
                for (int e = rowptr[k]; e < rowptr[k + 1]; ++e) {
                    const int64_t q = std::llabs(rq(vals[e], qs));
                    if (q > 8388607) ok = false;
                    row += q;
                }
                if (row > 2147483647LL) ok = false;
            }
            if (ok) break;
            --qs;
        }
        // canonical form: drop the power of two common to every Jq and hq (+-J instances: Jq = +-1).  Where every value is an exact
        // multiple of 2^-qs (so that a smaller scale just shifts the integers) the common power is found in ONE pass -- the loop
        // below, one pass per bit, was 22 passes over the couplings for a +-J instance: most of the 6 ms of nlmc_create at N = 10^4.
        {
            bool exact = true, any = false;
            int min_tz = 63;
            auto scan = [&](double v) {
                const int64_t q = rq(v, qs);
                if (std::ldexp((double)q, -qs) != v) exact = false;
                if (q) { any = true; min_tz = std::min(min_tz, __builtin_ctzll((unsigned long long)(q < 0 ? -q : q))); }
            };
            for (int64_t e = 0; e < nnz && exact; ++e) scan(vals[e]);
            for (int k = 0; k < n && exact; ++k) scan(h[k]);
            if (exact && any && min_tz > 0) qs -= min_tz;        // (the loop below then stops at its first pass: some integer is odd)
        }
        for (;;) {
            bool even = true, any = false;
            for (int64_t e = 0; e < nnz && even; ++e) { const int64_t q = rq(vals[e], qs); if (q & 1) even = false; if (q) any = true; }
            for (int k = 0; k < n && even; ++k) { const int64_t q = rq(h[k], qs); if (q & 1) even = false; if (q) any = true; }
            if (!even || !any) break;
            --qs;
        }
    }
    I.qs = qs;
    I.escale = std::min(escale0, qs + 29);

    I.e32.resize((size_t)std::max<int64_t>(nnz, 1));
    I.hq.resize((size_t)n);
    std::vector<EdgeQ> &e32 = I.e32;
    bool fits16 = n <= 65535, pm1 = true, exact_q = true;
    for (int64_t e = 0; e < nnz; ++e) {
        e32[e].col = colidx[e]; e32[e].q = (int32_t)rq(vals[e], qs);
        if (e32[e].q > 32767 || e32[e].q < -32768) fits16 = false;
        if (std::ldexp((double)e32[e].q, -qs) != vals[e]) exact_q = false;
        if (e32[e].q != 1 && e32[e].q != -1) pm1 = false;
    }
    I.fits16 = fits16; I.pm1 = pm1; I.exact_q = exact_q;
    I.exact_h = true;
    I.no_field = true;
    for (int k = 0; k < n; ++k) {
        I.hq[k] = (int32_t)rq(h[k], qs);
        if (I.hq[k] != 0) I.no_field = false;
        if (std::ldexp((double)I.hq[k], -qs) != h[k]) I.exact_h = false;
        int64_t row = std::llabs((int64_t)I.hq[k]);
        for (int e = rowptr[k]; e < rowptr[k + 1]; ++e) row += std::llabs((int64_t)e32[e].q);
        I.xmax = (int)std::min<int64_t>(std::max<int64_t>(I.xmax, row), INT_MAX);
    }
    return NLMC_OK;
}
