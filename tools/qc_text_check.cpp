// qc_text_check.cpp — host/qc_text.cpp on its own: the texts of the QC rules (include/bwams.h, rule 7), as a program to build with
// -fsanitize=address,undefined and run on the CPU (tests/test_qc_text_host.py does, and compares what it prints):
//   g++ -std=c++17 -fsanitize=address,undefined -Iinclude -Ibwa-mem-scale_amd/host bwa-mem-scale_amd/host/qc_text.cpp tools/qc_text_check.cpp
// Input: none.  Output: for the counters of the header's example and for a handle nothing was added to, a line "== <case> <text>"
// and the text.
#include <cstdio>
#include <string>
#include <vector>

#include "qc_host.h"

namespace {

struct Counters {
    bwams_qc_opt_t opt;
    bwams_qc_summary_t sum{};
    std::vector<int64_t> rl, qual, base, mapq, isize, indel;
    explicit Counters(bwams_qc_opt_t o)
        : opt(o), rl(2 * (size_t)(o.max_cycle + 1)), qual(2 * (size_t)o.max_cycle * 64), base(2 * (size_t)o.max_cycle * 5), mapq(256),
          isize(3 * (size_t)(o.max_isize + 1)), indel(2 * 65) {}
    bwams::QcTables tables() const {
        return bwams::QcTables{opt, sum, {rl.data(), qual.data(), base.data(), mapq.data(), isize.data(), indel.data()}};
    }
};

int run(const char *tag, const Counters &c) {
    static const char *const kText[2] = {"flagstat", "stats"};
    for (int32_t what = 0; what < 2; ++what) {
        std::string out;
        if (bwams::qc_text_format(c.tables(), what, &out)) return 1;
        printf("== %s %s\n", tag, kText[what]);
        fwrite(out.data(), 1, out.size(), stdout);
    }
    return 0;
}

}  // namespace

int main() {
    Counters hand(bwams_qc_opt_t{0x900, 64, 100, 0});
    const int64_t flags[2][16] = {{9, 8, 0, 1, 0, 0, 8, 7, 8, 5, 3, 2, 6, 1, 2, 1}, {1, 1, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0}};
    const int64_t scalars[11] = {9, 27, 8, 23, 1, 2, 1, 632, 24, 0, 1};
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 16; ++k) hand.sum.flags[c][k] = flags[c][k];
    for (int k = 0; k < 11; ++k) hand.sum.scalars[k] = scalars[k];
    const int rl[][3] = {{0, 2, 3}, {0, 3, 1}, {0, 4, 2}, {1, 2, 1}, {1, 3, 1}, {1, 5, 1}};                  // class, length, count
    for (auto &e : rl) hand.rl[(size_t)(e[0] * 65 + e[1])] = e[2];
    const int qual[][4] = {{0, 0, 2, 1}, {0, 0, 30, 3}, {0, 0, 63, 1}, {0, 1, 30, 5}, {0, 2, 20, 1}, {0, 2, 30, 1}, {0, 3, 10, 1}, {0, 3, 30, 1},
                           {1, 0, 10, 2}, {1, 0, 30, 1}, {1, 1, 10, 1}, {1, 1, 20, 1}, {1, 1, 30, 1}, {1, 2, 10, 1}, {1, 2, 30, 1}, {1, 3, 40, 1},
                           {1, 4, 40, 1}};                                                                   // class, cycle, bin, count
    for (auto &e : qual) hand.qual[(size_t)((e[0] * 64 + e[1]) * 64 + e[2])] = e[3];
    const int base[][7] = {{0, 0, 3, 0, 2, 0, 1}, {0, 1, 2, 1, 2, 1, 0}, {0, 2, 0, 1, 2, 0, 0}, {0, 3, 0, 0, 1, 1, 0}, {1, 0, 0, 0, 1, 2, 0},
                           {1, 1, 1, 0, 1, 1, 0}, {1, 2, 0, 1, 0, 1, 0}, {1, 3, 0, 0, 1, 0, 0}, {1, 4, 0, 0, 0, 1, 0}};   // class, cycle, A C G T N
    for (auto &e : base)
        for (int k = 0; k < 5; ++k) hand.base[(size_t)((e[0] * 64 + e[1]) * 5 + k)] = e[2 + k];
    hand.mapq[0] = hand.mapq[4] = hand.mapq[9] = hand.mapq[30] = 1;
    hand.mapq[60] = 4;
    hand.isize[100] = hand.isize[101 + 42] = hand.isize[2 * 101 + 22] = 1;
    hand.indel[1] = 1;
    if (run("hand", hand)) return 1;
    if (run("empty", Counters(bwams_qc_opt_t{0x900, 512, 8000, 0}))) return 1;
    Counters big(bwams_qc_opt_t{0x900, 64, 1 << 20, 0});                 // n * S2 past 64 bits: 2^40 pairs at 2^20 - 1 and at 1
    big.isize[(1 << 20) - 1] = big.isize[(size_t)(1 << 20) + 1 + 1] = (int64_t)1 << 40;
    if (run("big", big)) return 1;
    std::string out;
    return bwams::qc_text_format(hand.tables(), 2, &out) == BWAMS_ERR_ARG ? 0 : 1;
}
