// pileup_vcf_check.cpp — host/pileup_vcf.cpp on its own: the VCF text of the pileup's calls (include/bwams.h, rule 13), as a program
// to build with -fsanitize=address,undefined and run on the CPU (tests/test_pileup_vcf_host.py does, and compares what it prints):
//   g++ -std=c++17 -fsanitize=address,undefined -Iinclude -Ibwa-mem-scale_amd/host bwa-mem-scale_amd/host/pileup_vcf.cpp tools/pileup_vcf_check.cpp
// Input: none.  Output: for the example of rule 13, for the calls of tests/test_pileup_calls.py's hand-built case and for no call and
// no reference at all, a line "== <case>" and the text.
#include <cstdio>
#include <string>
#include <vector>

#include "pileup_host.h"

namespace {

struct Case {
    const char *tag;
    std::string names;                               // NUL after each
    std::vector<int32_t> l_ref;
    std::vector<bwams_pileup_region_t> regions;
    const char *sample;
    std::vector<bwams_pileup_call_t> calls;
};

int run(const Case &c) {
    std::string out;
    if (bwams::pileup_vcf_format(c.names.data(), c.l_ref.data(), (int32_t)c.l_ref.size(), c.regions.data(), (int32_t)c.regions.size(),
                                 c.sample, c.calls.data(), (int64_t)c.calls.size(), &out)) return 1;
    printf("== %s\n", c.tag);
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}

}  // namespace

int main() {
    const std::vector<Case> cases = {
        {"example", std::string("c1\0", 3), {8}, {{0, 0, 8}}, "s1",
         {{0, 2, 2, 2, 3, 54, 54, 5, {0, 0, 3, 2}, {159, 159, 159, 64, 64, 54, 95, 95, 0, 89}}}},
        {"hand", std::string("h\0", 2), {12}, {{0, 0, 12}}, "smp",
         {{0, 0, 3, 0, 1, 64, 0, 3, {1, 1, 1, 0}, {29, 0, 29, 0, 0, 29, 32, 32, 32, 64}},
          {0, 1, 3, 0, 1, 191, 86, 6, {3, 3, 0, 0}, {86, 0, 86, 95, 95, 191, 95, 95, 191, 191}},
          {0, 2, 0, 2, 2, 87, 12, 4, {0, 0, 4, 0}, {87, 87, 87, 12, 12, 0, 87, 87, 12, 87}},
          {0, 9, 3, 1, 1, 60, 6, 2, {0, 2, 0, 0}, {60, 6, 0, 60, 6, 60, 60, 6, 60, 60}},
          {0, 10, 0, 1, 1, 60, 6, 2, {0, 2, 0, 0}, {60, 6, 0, 60, 6, 60, 60, 6, 60, 60}}}},
        // two references and a region that does not begin at 0; the reference allele above, between and below the two others; the
        // largest values of every field
        {"orders", std::string("chrA\0b\0", 7), {2147483647, 0}, {{0, 5, 9}, {0, 2147483000, 2147483647}}, "a sample",
         {{0, 6, 1, 0, 1, 0, 0, 1, {1, 1, 0, 0}, {1, 0, 2, 3, 4, 5, 6, 7, 8, 9}},
          {1, 2147483646, 1, 0, 3, 2147483647, 99, 4294967295u, {4294967295u, 7, 8, 4294967294u},
           {10, 11, 2147483647, 13, 14, 15, 0, 17, 18, 19}},
          {1, 2147483646, 3, 0, 2, 5, 6, 7, {1, 2, 3, 4}, {10, 11, 12, 13, 14, 15, 16, 17, 18, 19}},
          {1, 2147483646, 0, 2, 3, 5, 6, 7, {1, 2, 3, 4}, {10, 11, 12, 13, 14, 15, 16, 17, 18, 19}}}},
        {"none", std::string(), {}, {}, "", {}},
    };
    for (const Case &c : cases)
        if (run(c)) return 1;
    std::string out;
    const bwams_pileup_region_t region{0, 0, 8};
    const int32_t l_ref = 8;
    bwams_pileup_call_t bad[4] = {{1, 0, 0, 0, 1, 0, 0, 0, {0, 0, 0, 0}, {0}},     // a region the list does not have
                                  {0, 0, 4, 0, 1, 0, 0, 0, {0, 0, 0, 0}, {0}},     // a reference base that is no base
                                  {0, 0, 0, 2, 1, 0, 0, 0, {0, 0, 0, 0}, {0}},     // alleles out of order
                                  {0, 0, 2, 2, 2, 0, 0, 0, {0, 0, 0, 0}, {0}}};    // the reference genotype is no call
    for (const bwams_pileup_call_t &b : bad)
        if (bwams::pileup_vcf_format("c1", &l_ref, 1, &region, 1, "s", &b, 1, &out) != BWAMS_ERR_ARG) return 1;
    return 0;
}
