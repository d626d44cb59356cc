// Host run of the instance preparation of nlmc_create (csrc/nlmc_instance.h: nlmc_instance_prepare) on one instance read from a
// binary file; prints the return code, the error text and, on success, every fact the function returns (Jq and hq included).
// tests/test_instance_prep_cpu.py builds it plainly (-O1 -g), writes the files and compares the output with exact references;
// NLMC_KEEP_INSTANCE_INPUTS=dir makes that test keep its files, for a run of the same inputs under the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/instance_prep_check.cpp -o instance_prep_check
//   for f in dir/*.bin; do ./instance_prep_check $f > /dev/null || echo "FAILED $f"; done
//
// File: 10 int64 { null_mask, n, nnz, n_chains, chain_base, n_chains_global, len_rowptr, len_colidx, len_vals, len_h }, then
// rowptr and colidx (int32), vals and h (double) with those lengths.  null_mask: bit 0 out, 1 rowptr, 2 colidx, 3 vals, 4 h are
// handed over as NULL.  The arrays are heap blocks of exactly their stated lengths, whatever n and nnz say, so that a read past an
// array is a read past a heap block.
#include "../nonlocal-monte-carlo_amd/csrc/nlmc_instance.h"

#include <cinttypes>
#include <cstdio>
#include <memory>

template <typename T> static std::unique_ptr<T[]> read_array(FILE *f, int64_t len)
{
    std::unique_ptr<T[]> a(new T[(size_t)len]);
    if (len && fread(a.get(), sizeof(T), (size_t)len, f) != (size_t)len) { std::fprintf(stderr, "short file\n"); std::exit(2); }
    return a;
}

int main(int argc, char **argv)
{
    FILE *f = argc == 2 ? std::fopen(argv[1], "rb") : nullptr;
    if (!f) { std::fprintf(stderr, "usage: instance_prep_check FILE\n"); return 2; }
    int64_t hd[10];
    if (fread(hd, sizeof(int64_t), 10, f) != 10 || hd[6] < 0 || hd[7] < 0 || hd[8] < 0 || hd[9] < 0) { std::fprintf(stderr, "bad header\n"); return 2; }
    const auto rowptr = read_array<int32_t>(f, hd[6]);
    const auto colidx = read_array<int32_t>(f, hd[7]);
    const auto vals = read_array<double>(f, hd[8]);
    const auto h = read_array<double>(f, hd[9]);
    std::fclose(f);
    const int64_t mask = hd[0], nnz = hd[2];
    int out = 0;
    NlmcInstance I;
    const int rc = nlmc_instance_prepare(I, mask & 1 ? nullptr : &out, (int)hd[1], nnz, mask & 2 ? nullptr : rowptr.get(),
                                         mask & 4 ? nullptr : colidx.get(), mask & 8 ? nullptr : vals.get(), mask & 16 ? nullptr : h.get(),
                                         (int)hd[3], (int)hd[4], (int)hd[5], 8 /* NLMC_FZ_W */);
    std::printf("rc %d\nerr %s\n", rc, I.err);
    if (rc != NLMC_OK) return 0;
    std::printf("has_diag %d\nhas_zero_vals %d\nmax_deg %d\nn_gt1 %d\nn_gt2 %d\nqs %d\nescale %d\n", I.has_diag, I.has_zero_vals, I.max_deg,
                I.n_gt1, I.n_gt2, I.qs, I.escale);
    std::printf("fits16 %d\npm1 %d\nexact_q %d\nexact_h %d\nxmax %d\n", I.fits16, I.pm1, I.exact_q, I.exact_h, I.xmax);
    std::printf("col");
    for (int64_t e = 0; e < nnz; ++e) std::printf(" %" PRId32, I.e32[(size_t)e].col);
    std::printf("\nJq");
    for (int64_t e = 0; e < nnz; ++e) std::printf(" %" PRId32, I.e32[(size_t)e].q);
    std::printf("\nhq");
    for (int32_t q : I.hq) std::printf(" %" PRId32, q);
    std::printf("\n");
    return 0;
}
