// bai_plan_check.cpp — host/bam_query.cpp on its own: the BAI parser and the planner of a region query (include/bwams.h, "BAM file by
// region", rules 2 and 3), as a program to build with -fsanitize=address,undefined and run on the CPU (tests/test_bam_query_plan.py
// does, and compares what it prints with bwams/bai.py's plan):
//   g++ -std=c++17 -fsanitize=address,undefined -Iinclude -Ibwa-mem-scale_amd/host bwa-mem-scale_amd/host/bam_query.cpp tools/bai_plan_check.cpp
// Input: the path of a BAI and the path of a text file with a region "ref beg end" per line.  Output: a line "beg end" (virtual
// offsets, decimal) per interval of the plan.  Exit status 1 with the reason on stderr when the index or a region is refused.
// With "--truncations" in place of the regions: the index is parsed again cut off at every length below its own, each time from an
// allocation of exactly that length, and every length at which the parser did not return an error is printed (none is expected).
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bam_query.h"

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: bai_plan_check <file.bai> <regions.txt>\n");
        return 2;
    }
    std::vector<uint8_t> raw;
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) { fprintf(stderr, "%s: cannot be opened\n", argv[1]); return 2; }
    uint8_t buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, fp)) > 0;) raw.insert(raw.end(), buf, buf + k);
    fclose(fp);
    if (!strcmp(argv[2], "--truncations")) {
        for (size_t len = 0; len < raw.size(); ++len) {
            std::unique_ptr<uint8_t[]> cut(new uint8_t[len]);          // a read past `len` is a read past the allocation
            if (len) memcpy(cut.get(), raw.data(), len);
            bwams::Bai index;
            std::string err;
            if (bwams::bai_parse(cut.get(), (int64_t)len, &index, &err) == 0) printf("%zu\n", len);
        }
        return 0;
    }
    std::unique_ptr<uint8_t[]> exact(new uint8_t[raw.size()]);
    if (!raw.empty()) memcpy(exact.get(), raw.data(), raw.size());
    std::vector<bwams_pileup_region_t> regions;
    fp = fopen(argv[2], "r");
    if (!fp) { fprintf(stderr, "%s: cannot be opened\n", argv[2]); return 2; }
    bwams_pileup_region_t g;
    while (fscanf(fp, "%d %d %d", &g.ref, &g.beg, &g.end) == 3) regions.push_back(g);
    fclose(fp);
    bwams::Bai index;
    std::string err;
    if (bwams::bai_parse(exact.get(), (int64_t)raw.size(), &index, &err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return 1;
    }
    std::vector<bwams_pileup_region_t> merged;
    if (bwams::regions_merge(regions.data(), (int32_t)regions.size(), (int32_t)index.refs.size(), &merged, &err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return 1;
    }
    std::vector<uint64_t> beg, end;
    bwams::bai_plan(index, merged, &beg, &end);
    for (size_t k = 0; k < beg.size(); ++k) printf("%llu %llu\n", (unsigned long long)beg[k], (unsigned long long)end[k]);
    return 0;
}
