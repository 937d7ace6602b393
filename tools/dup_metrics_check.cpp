// dup_metrics_check.cpp — host/dup_metrics.cpp on its own: the groups table, rule 14 and the metrics text, as a program to build with
// -fsanitize=address,undefined and run on the CPU (tests/test_dup_metrics_host.py does, and compares what it prints):
//   g++ -std=c++17 -fsanitize=address,undefined -Iinclude -Ibwa-mem-scale_amd/host bwa-mem-scale_amd/host/dup_metrics.cpp tools/dup_metrics_check.cpp
// Input: header text on stdin.  Output: "groups <rc>", then "<n_rg> <n_lib>" and a line per library; "size n c -> v" for every pair
// of arguments; the metrics text of rows made from the library ordinals (row k: pairs 1000 (k + 1), duplicates 100 (k + 1), ...),
// asked for once with no room (its size) and once into a buffer of exactly that size.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "bwams.h"
#include "dup_groups.h"

int main(int argc, char **argv) {
    std::string text;
    char buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, stdin)) > 0;) text.append(buf, k);
    bwams_dup_groups_t *g = nullptr;
    const int rc = bwams_dup_groups_create(text.data(), (int64_t)text.size(), &g);
    printf("groups %d\n", rc);
    for (int i = 1; i + 1 < argc; i += 2) {
        const long long n = atoll(argv[i]), c = atoll(argv[i + 1]);
        printf("size %lld %lld -> %lld\n", n, c, (long long)bwams_dup_library_size(n, c));
    }
    if (rc) return g ? 1 : 0;                                   // a refusal leaves no table
    int64_t n_rg = 0, n_lib = 0;
    if (bwams_dup_groups_info(g, &n_rg, &n_lib)) return 1;
    printf("%lld %lld\n", (long long)n_rg, (long long)n_lib);
    for (int64_t k = 0; k < n_lib; ++k) printf("%s\n", bwams_dup_groups_library(g, k));
    if (bwams_dup_groups_library(g, n_lib) || bwams_dup_groups_library(g, -1)) return 1;
    std::vector<bwams_dup_lib_stats_t> rows((size_t)n_lib);
    for (int64_t k = 0; k < n_lib; ++k) {
        bwams_dup_lib_stats_t &r = rows[(size_t)k];
        r = bwams_dup_lib_stats_t{};
        if (k % 2 == 0) {                                       // odd libraries stay empty: no row
            r.unpaired_examined = 7 + k; r.pairs_examined = 1000 * (k + 1); r.secondary_or_supplementary = 3; r.unmapped = 11;
            r.unpaired_duplicates = 2; r.pair_duplicates = 100 * (k + 1); r.pair_optical_duplicates = k;
        }
        bwams::dup_lib_finish(&r);
    }
    int64_t need = 0, got = 0;
    if (bwams_dup_metrics_text(g, rows.data(), n_lib, "check", nullptr, 0, &need) != BWAMS_ERR_CAPACITY) return 1;
    if (bwams_dup_metrics_text(g, rows.data(), n_lib + 1, "check", nullptr, 0, &need) != BWAMS_ERR_ARG) return 1;
    std::vector<char> out((size_t)need);
    if (bwams_dup_metrics_text(g, rows.data(), n_lib, "check", out.data(), need - 1, &got) != BWAMS_ERR_CAPACITY || got != need) return 1;
    if (bwams_dup_metrics_text(g, rows.data(), n_lib, "check", out.data(), need, &got) || got != need) return 1;
    fwrite(out.data(), 1, (size_t)got, stdout);
    bwams_dup_groups_destroy(g);
    bwams_dup_groups_destroy(nullptr);
    return 0;
}
