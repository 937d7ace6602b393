// pileup_indel_vcf_check.cpp — host/pileup_indel_vcf.cpp and host/pileup_vcf.cpp on their own: the VCF text of the pileup's indel
// calls and its merge with the SNV rows (include/bwams.h, rule 17), as a program to build with -fsanitize=address,undefined and run on
// the CPU (tests/test_pileup_indel_vcf_host.py does, and compares what it prints):
//   g++ -std=c++17 -fsanitize=address,undefined -Iinclude -Ibwa-mem-scale_amd/host bwa-mem-scale_amd/host/pileup_vcf.cpp \
//       bwa-mem-scale_amd/host/pileup_indel_vcf.cpp tools/pileup_indel_vcf_check.cpp
// Input: none.  Output: for each case a line "== <case>" and the text.
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
    std::vector<bwams_pileup_call_t> snvs;
    std::vector<bwams_pileup_indel_t> indels;
};

int run(const Case &c) {
    std::string out;
    if (bwams::pileup_indel_vcf_format(c.names.data(), c.l_ref.data(), (int32_t)c.l_ref.size(), c.regions.data(), (int32_t)c.regions.size(),
                                       c.sample, c.snvs.data(), (int64_t)c.snvs.size(), c.indels.data(), (int64_t)c.indels.size(), &out)) return 1;
    printf("== %s\n", c.tag);
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}

bwams_pileup_indel_t indel(int32_t region, int32_t pos, int32_t ref, int32_t type, int32_t len, uint64_t seq, int32_t gt, int32_t qual, int32_t gq,
                           uint32_t depth, uint32_t n_ref, uint32_t n_alt, uint32_t n_other, int32_t pl0, int32_t pl1, int32_t pl2) {
    bwams_pileup_indel_t x{};
    x.region = region; x.pos = pos; x.ref = ref; x.type = type; x.len = len; x.seq = seq; x.gt = gt; x.qual = qual; x.gq = gq;
    x.depth = depth; x.n_ref = n_ref; x.n_alt = n_alt; x.n_other = n_other;
    x.pl[0] = pl0; x.pl[1] = pl1; x.pl[2] = pl2;
    return x;
}

}  // namespace

int main() {
    const bwams_pileup_call_t ex_snv = {0, 2, 2, 2, 3, 54, 54, 5, {0, 0, 3, 2}, {159, 159, 159, 64, 64, 54, 95, 95, 0, 89}};
    const bwams_pileup_indel_t ex_del = indel(0, 3, 3, 0, 1, 0, 1, 74, 74, 5, 3, 2, 0, 74, 0, 119);       // del_ref[0] = 0: A
    const bwams_pileup_indel_t ex_ins = indel(0, 5, 1, 1, 2, 15, 1, 68, 68, 7, 5, 2, 0, 68, 0, 203);
    // the extremes: 32 inserted bases, all T and ACGT eight times; 32 deleted bases with N among them; the largest value of every field;
    // an SNV and two indels at one position, an SNV behind them, an indel in a later region before an SNV of it
    bwams_pileup_indel_t del32 = indel(1, 2147483646, 0, 0, 32, 0, 2, 2147483647, 99, 4294967295u, 4294967295u, 4294967294u, 7, 2147483647, 12, 0);
    for (int j = 0; j < 32; ++j) del32.del_ref[j] = (uint8_t)(j % 5);
    const std::vector<Case> cases = {
        {"example", std::string("c1\0", 3), {8}, {{0, 0, 8}}, "s1", {}, {ex_del, ex_ins}},
        {"all", std::string("c1\0", 3), {8}, {{0, 0, 8}}, "s1", {ex_snv}, {ex_del, ex_ins}},
        {"extremes", std::string("chrA\0b\0", 7), {2147483647, 0}, {{0, 5, 9}, {0, 2147483000, 2147483647}}, "a sample",
         {{0, 6, 1, 0, 1, 0, 0, 1, {1, 1, 0, 0}, {1, 0, 2, 3, 4, 5, 6, 7, 8, 9}},
          {0, 7, 1, 0, 1, 0, 0, 1, {1, 1, 0, 0}, {1, 0, 2, 3, 4, 5, 6, 7, 8, 9}},
          {1, 2147483646, 3, 0, 2, 5, 6, 7, {1, 2, 3, 4}, {10, 11, 12, 13, 14, 15, 16, 17, 18, 19}}},
         {indel(0, 6, 2, 1, 32, ~0ULL, 2, 0, 0, 1, 0, 1, 0, 0, 0, 0), indel(0, 6, 3, 1, 32, 0xE4E4E4E4E4E4E4E4ULL, 1, 21, 3, 9, 4, 3, 2, 21, 0, 3),
          indel(1, 2147483000, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1), del32}},
        {"none", std::string(), {}, {}, "", {}, {}},
    };
    for (const Case &c : cases)
        if (run(c)) return 1;
    std::string out;
    const bwams_pileup_region_t region{0, 0, 8};
    const int32_t l_ref = 8;
    bwams_pileup_indel_t bad[6] = {indel(1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0),      // a region the list does not have
                                   indel(0, 0, 4, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0),      // a reference base that is no base
                                   indel(0, 0, 0, 2, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0),      // OTHER is no allele
                                   indel(0, 0, 0, 1, 33, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0),     // longer than a sequence word
                                   indel(0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),      // the reference genotype is no call
                                   indel(0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0)};     // a deleted code above 4
    bad[5].del_ref[0] = 5;
    for (const bwams_pileup_indel_t &b : bad)
        if (bwams::pileup_indel_vcf_format("c1", &l_ref, 1, &region, 1, "s", nullptr, 0, &b, 1, &out) != BWAMS_ERR_ARG) return 1;
    return 0;
}
