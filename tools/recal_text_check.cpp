// recal_text_check.cpp — host/recal_text.cpp on its own: the text of the recalibration tables (include/bwams.h, rule 10), as a program
// to build with -fsanitize=address,undefined and run on the CPU (tests/test_recal_text_host.py does, and compares what it prints):
//   g++ -std=c++17 -fsanitize=address,undefined -Iinclude -Ibwa-mem-scale_amd/host bwa-mem-scale_amd/host/recal_text.cpp tools/recal_text_check.cpp
// Input: none.  Output: for the tables of the header's example, for a handle nothing was added to, and for a handle without read
// groups whose cells sit at the ends of every table, a line "== <case>" and the text.
#include <cstdio>
#include <string>
#include <vector>

#include "recal_host.h"

namespace {

struct Tables {
    int32_t max_cycle;
    std::vector<std::string> ids;
    std::vector<int64_t> rg, qual, cycle, context;
    Tables(int32_t mc, std::vector<std::string> names)
        : max_cycle(mc), ids(std::move(names)), rg(2 * (ids.size() + 1)), qual(rg.size() * 94), cycle(qual.size() * (size_t)(2 * mc + 1)),
          context(qual.size() * 16) {}
    size_t cols() const { return (size_t)(2 * max_cycle + 1); }
    void add(size_t g, size_t q, int cyc, int ctx, int64_t obs, int64_t err) {        // one cell of each table (ctx < 0: none)
        const int64_t v[2] = {obs, err};
        for (size_t e = 0; e < 2; ++e) {
            rg[2 * g + e] += v[e];
            qual[2 * (g * 94 + q) + e] += v[e];
            cycle[2 * ((g * 94 + q) * cols() + (size_t)(cyc + max_cycle)) + e] += v[e];
            if (ctx >= 0) context[2 * ((g * 94 + q) * 16 + (size_t)ctx) + e] += v[e];
        }
    }
    void print(const char *tag) const {
        const bwams::RecalTables t{max_cycle, ids, {rg.data(), qual.data(), cycle.data(), context.data()}};
        std::string out;
        bwams::recal_text_format(t, &out);
        printf("== %s\n", tag);
        fwrite(out.data(), 1, out.size(), stdout);
    }
};

}  // namespace

int main() {
    Tables hand(10, {"a"});                                              // the header's example, base by base
    const int ctx1[8] = {-1, 1, 6, 11, 12, 1, 6, 11}, ctx2[8] = {-1, 1, 6, 11, 12, 0, 2, 11};      // machine order: ACGTACGT, ACGTAAGT
    for (int m = 0; m < 8; ++m) {
        hand.add(0, 30, m + 1, ctx1[m], 1, 0);
        hand.add(0, 30, m + 1, ctx2[m], 1, m == 5 ? 1 : 0);
    }
    hand.print("hand");
    Tables(500, {"a", "b"}).print("empty");
    Tables edges(3, {});                                                 // no read groups: the one row prints as `*`
    edges.add(0, 0, -3, 0, 5, 0);
    edges.add(0, 93, 3, 15, (int64_t)1 << 40, (int64_t)1 << 39);
    edges.add(0, 93, -1, -1, 1, 1);
    edges.print("edges");
    Tables two(2, {"left", "r\xC3\xA9" "2"});                            // the last named row and the row behind it
    two.add(1, 6, 1, 9, 3, 2);
    two.add(2, 7, 2, -1, 1, 0);
    two.print("two");
    return 0;
}
