// bam_header_merge_check.cpp — host/bam_merge_header.cpp on its own: the header merge of bwams_bam_file_open_merge (include/bwams.h,
// rules M2 and M3), as a program to build with -fsanitize=address,undefined and run on the CPU (tests/test_bam_merge.py does, and
// compares what it writes with bwams/merge.py's merge_header):
//   g++ -std=c++17 -fsanitize=address,undefined -Iinclude -Ibwa-mem-scale_amd/host bwa-mem-scale_amd/host/bam_merge_header.cpp tools/bam_header_merge_check.cpp
// usage: bam_header_merge_check <out> <block 0> <block 1> ...    the merged block goes to <out>, "pg_dropped N" to stdout
//        bam_header_merge_check --truncations <block 0> ...      every block in turn is cut off at every length below its own, each
//                                                                time from an allocation of exactly that length, and "file length"
//                                                                is printed wherever the merge did not return an error (none is expected)
// Exit status 1 with "rc: reason" on stderr when the merge is refused.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bam_query.h"

static bool slurp(const char *path, std::vector<uint8_t> *out) {
    FILE *fp = fopen(path, "rb");
    if (!fp) { fprintf(stderr, "%s: cannot be opened\n", path); return false; }
    uint8_t buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, fp)) > 0;) out->insert(out->end(), buf, buf + k);
    fclose(fp);
    return true;
}

int main(int argc, char **argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: bam_header_merge_check <out> | --truncations  <block> ...\n");
        return 2;
    }
    const int n = argc - 2;
    std::vector<std::unique_ptr<uint8_t[]>> exact((size_t)n);          // a read past a block is a read past its allocation
    std::vector<const void *> blocks((size_t)n);
    std::vector<int64_t> sizes((size_t)n);
    for (int k = 0; k < n; ++k) {
        std::vector<uint8_t> raw;
        if (!slurp(argv[2 + k], &raw)) return 2;
        exact[(size_t)k].reset(new uint8_t[raw.size()]);
        if (!raw.empty()) memcpy(exact[(size_t)k].get(), raw.data(), raw.size());
        blocks[(size_t)k] = exact[(size_t)k].get();
        sizes[(size_t)k] = (int64_t)raw.size();
    }
    std::string out, err;
    int32_t dropped = 0;
    if (!strcmp(argv[1], "--truncations")) {
        for (int k = 0; k < n; ++k) {
            const void *whole = blocks[(size_t)k];
            const int64_t size = sizes[(size_t)k];
            for (int64_t len = 0; len < size; ++len) {
                std::unique_ptr<uint8_t[]> cut(new uint8_t[(size_t)len]);
                if (len) memcpy(cut.get(), whole, (size_t)len);
                blocks[(size_t)k] = cut.get();
                sizes[(size_t)k] = len;
                if (bwams::bam_header_merge(blocks.data(), sizes.data(), n, &out, &dropped, &err) == 0) printf("%d %lld\n", k, (long long)len);
            }
            blocks[(size_t)k] = whole;
            sizes[(size_t)k] = size;
        }
        return 0;
    }
    if (int rc = bwams::bam_header_merge(blocks.data(), sizes.data(), n, &out, &dropped, &err)) {
        fprintf(stderr, "%d: %s\n", rc, err.c_str());
        return 1;
    }
    FILE *fp = fopen(argv[1], "wb");
    if (!fp || fwrite(out.data(), 1, out.size(), fp) != out.size()) { fprintf(stderr, "%s: cannot be written\n", argv[1]); return 2; }
    fclose(fp);
    printf("pg_dropped %d\n", dropped);
    return 0;
}
