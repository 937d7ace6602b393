// recal_text.cpp — the text of the recalibration tables (include/bwams.h, rule 10): a tab-separated row per cell with observations.
// Plain C++ with no HIP header: it also builds alone, with tools/recal_text_check.cpp, under the host sanitizers.  bwams/recal.py
// restates it byte for byte.
#include <cstdarg>
#include <cstdio>

#include "recal_host.h"

namespace bwams {
namespace {

void put(std::string *out, const char *fmt, ...) {
    char buf[96];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    out->append(buf);
}

}  // namespace

void recal_text_format(const RecalTables &t, std::string *out) {
    out->clear();
    const int64_t rows = (int64_t)t.ids.size() + 1, cols = 2 * (int64_t)t.max_cycle + 1;
    auto id = [&](int64_t g) { return g + 1 < rows ? t.ids[(size_t)g].c_str() : "*"; };
    const int64_t *rg = t.table[BWAMS_RECAL_TABLE_RG], *qual = t.table[BWAMS_RECAL_TABLE_QUAL];
    const int64_t *cycle = t.table[BWAMS_RECAL_TABLE_CYCLE], *context = t.table[BWAMS_RECAL_TABLE_CONTEXT];
    for (int64_t g = 0; g < rows; ++g)
        if (rg[2 * g] > 0) {
            out->append("RG\t").append(id(g));
            put(out, "\t%lld\t%lld\n", (long long)rg[2 * g], (long long)rg[2 * g + 1]);
        }
    for (int64_t g = 0; g < rows; ++g)
        for (int64_t q = 0; q < 94; ++q) {
            const int64_t *c = qual + 2 * (g * 94 + q);
            if (c[0] <= 0) continue;
            out->append("QUAL\t").append(id(g));
            put(out, "\t%lld\t%lld\t%lld\n", (long long)q, (long long)c[0], (long long)c[1]);
        }
    for (int64_t g = 0; g < rows; ++g)
        for (int64_t q = 0; q < 94; ++q)
            for (int64_t k = 0; k < cols; ++k) {
                const int64_t *c = cycle + 2 * ((g * 94 + q) * cols + k);
                if (c[0] <= 0) continue;
                out->append("CYCLE\t").append(id(g));
                put(out, "\t%lld\t%lld\t%lld\t%lld\n", (long long)q, (long long)(k - t.max_cycle), (long long)c[0], (long long)c[1]);
            }
    for (int64_t g = 0; g < rows; ++g)
        for (int64_t q = 0; q < 94; ++q)
            for (int64_t k = 0; k < 16; ++k) {
                const int64_t *c = context + 2 * ((g * 94 + q) * 16 + k);
                if (c[0] <= 0) continue;
                out->append("CONTEXT\t").append(id(g));
                put(out, "\t%lld\t%c%c\t%lld\t%lld\n", (long long)q, "ACGT"[k >> 2], "ACGT"[k & 3], (long long)c[0], (long long)c[1]);
            }
}

}  // namespace bwams
