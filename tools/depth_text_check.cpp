// depth_text_check.cpp — host/depth_text.cpp on its own: the three texts of the depth rules (include/bwams.h, rule 11), as a program to
// build with -fsanitize=address,undefined and run on the CPU (tests/test_depth_text_host.py does, and compares what it prints):
//   g++ -std=c++17 -fsanitize=address,undefined -Iinclude -Ibwa-mem-scale_amd/host bwa-mem-scale_amd/host/depth_text.cpp tools/depth_text_check.cpp
// Input: none.  Output: for the example of rule 11 (c1: depths 2 2 2 2 2 0 0 0 0 1, c2: length 0), for tests/test_depth.py's
// hand-built case and for a handle of no reference, a line "== <case> <what>" and the text.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "depth_host.h"

namespace {

struct Case {
    const char *tag;
    std::string names;                               // NUL after each
    std::vector<std::vector<int32_t>> depth;         // per reference
    int32_t n_bins, w;
};

int run(const Case &c) {
    const int32_t n_ref = (int32_t)c.depth.size();
    std::vector<bwams_depth_ref_t> rows((size_t)n_ref);
    std::vector<int64_t> hist((size_t)(n_ref + 1) * (size_t)c.n_bins, 0), sums;
    for (int32_t r = 0; r < n_ref; ++r) {
        const std::vector<int32_t> &d = c.depth[(size_t)r];
        bwams_depth_ref_t &x = rows[(size_t)r];
        x = bwams_depth_ref_t{(int64_t)d.size(), 0, 0, 0};
        for (size_t i = 0; i < d.size(); ++i) {
            x.bases += d[i];
            x.min = i ? std::min(x.min, d[i]) : d[i];
            x.max = i ? std::max(x.max, d[i]) : d[i];
            const int32_t bin = std::min(d[i], c.n_bins - 1);
            ++hist[(size_t)bin];
            ++hist[(size_t)(r + 1) * (size_t)c.n_bins + (size_t)bin];
            if (i % (size_t)c.w == 0) sums.push_back(0);
            sums.back() += d[i];
        }
    }
    bwams::DepthTextIn in;
    in.names = c.names.data(); in.n_ref = n_ref; in.rows = rows.data(); in.hist = hist.data(); in.n_bins = c.n_bins;
    in.sums = sums.data(); in.w = c.w;
    static const char *what[] = {"summary", "dist", "windows"};
    for (int32_t k = 0; k < 3; ++k) {
        std::string out;
        if (bwams::depth_text_format(k, in, &out)) return 1;
        printf("== %s %s\n", c.tag, what[k]);
        fwrite(out.data(), 1, out.size(), stdout);
    }
    std::string out;
    return bwams::depth_text_format(3, in, &out) == BWAMS_ERR_ARG ? 0 : 1;
}

}  // namespace

int main() {
    const std::vector<Case> cases = {
        {"example", std::string("c1\0c2\0", 6), {{2, 2, 2, 2, 2, 0, 0, 0, 0, 1}, {}}, 1024, 4},
        {"hand", std::string("c0\0c1\0c2\0c3\0", 12),
         {{1, 1, 2, 2, 3, 2, 3, 1, 0, 1, 2, 2, 0, 0, 0, 2, 2, 1, 1, 1}, {1}, {}, {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}}, 3, 8},
        {"none", std::string(), {}, 2, 1},
    };
    for (const Case &c : cases)
        if (run(c)) return 1;
    return 0;
}
