// pileup_text_check.cpp — host/pileup_text.cpp on its own: the text of the pileup rules (include/bwams.h, rule 9), as a program to
// build with -fsanitize=address,undefined and run on the CPU (tests/test_pileup_text_host.py does, and compares what it prints):
//   g++ -std=c++17 -fsanitize=address,undefined -Iinclude -Ibwa-mem-scale_amd/host bwa-mem-scale_amd/host/pileup_text.cpp tools/pileup_text_check.cpp
// Input: none.  Output: for the example of rule 9, for two sites of tests/test_pileup.py's hand-built case and for no site at all, a
// line "== <case>" and the text.
#include <cstdio>
#include <string>
#include <vector>

#include "pileup_host.h"

namespace {

struct Case {
    const char *tag;
    std::string names;                               // NUL after each
    int32_t n_ref;
    std::vector<bwams_pileup_region_t> regions;
    std::vector<bwams_pileup_site_t> sites;
};

int run(const Case &c) {
    std::string out;
    if (bwams::pileup_text_format(c.names.data(), c.n_ref, c.regions.data(), (int32_t)c.regions.size(), c.sites.data(),
                                  (int64_t)c.sites.size(), &out)) return 1;
    printf("== %s\n", c.tag);
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}

}  // namespace

int main() {
    const std::vector<Case> cases = {
        {"example", std::string("c1\0", 3), 1, {{0, 0, 8}},
         {{0, 2, 2, 1u << 3, 5, {0, 0, 3, 1, 0, 0, 0, 1, 0, 0, 0, 0}}, {0, 4, 0, 1u << 4, 7, {4, 0, 0, 0, 1, 0, 0, 0, 0, 2, 0, 0}},
          {0, 5, 1, 1u << 5, 7, {0, 6, 0, 0, 0, 1, 0, 0, 0, 0, 2, 0}}}},
        {"hand", std::string("c0\0c1\0", 6), 2, {{0, 2, 12}, {0, 12, 16}, {1, 1, 2}},
         {{0, 5, 1, 1u << 0, 4, {1, 2, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0}}, {0, 6, 2, 7u << 3, 3, {0, 0, 1, 1, 0, 0, 0, 0, 0, 1, 1, 0}},
          {2, 1, 1, 0x2Cu, 3, {0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 1, 0}}}},
        {"none", std::string(), 0, {}, {}},
    };
    for (const Case &c : cases)
        if (run(c)) return 1;
    std::string out;
    const bwams_pileup_region_t region{0, 0, 8};
    bwams_pileup_site_t outside{};
    outside.region = 1;                              // a site of a region the list does not have
    return bwams::pileup_text_format("c1", 1, &region, 1, &outside, 1, &out) == BWAMS_ERR_ARG ? 0 : 1;
}
