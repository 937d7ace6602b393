// qc_text.cpp — the texts of the QC rules (include/bwams.h, rule 7): the flagstat lines and the tagged sections of the stats text.
// Plain C++ with no HIP header: it also builds alone, with tools/qc_text_check.cpp, under the host sanitizers.  bwams/qc.py restates
// it byte for byte.
#include <cmath>
#include <cstdarg>
#include <cstdio>

#include "qc_host.h"

namespace bwams {
namespace {

void put(std::string *out, const char *fmt, ...) {
    char buf[128];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    out->append(buf);
}

void percent(std::string *out, int64_t a, int64_t b) {
    if (b) put(out, "%.2f%%", 100.0 * (double)a / (double)b);
    else out->append("N/A");
}

void flagstat(const QcTables &t, std::string *out) {
    static const char *const kLabel[16] = {"in total (QC-passed reads + QC-failed reads)", "primary", "secondary", "supplementary",
                                           "duplicates", "primary duplicates", "mapped", "primary mapped", "paired in sequencing", "read1",
                                           "read2", "properly paired", "with itself and mate mapped", "singletons",
                                           "with mate mapped to a different chr", "with mate mapped to a different chr (mapQ>=5)"};
    static const int kOver[16] = {-1, -1, -1, -1, -1, -1, 0, 1, -1, -1, -1, 8, -1, 8, -1, -1};     // the denominator's counter
    for (int k = 0; k < 16; ++k) {
        put(out, "%lld + %lld %s", (long long)t.sum.flags[0][k], (long long)t.sum.flags[1][k], kLabel[k]);
        if (kOver[k] >= 0) {
            out->append(" (");
            percent(out, t.sum.flags[0][k], t.sum.flags[0][kOver[k]]);
            out->append(" : ");
            percent(out, t.sum.flags[1][k], t.sum.flags[1][kOver[k]]);
            out->push_back(')');
        }
        out->push_back('\n');
    }
}

bool any(const int64_t *v, int64_t n) {
    for (int64_t k = 0; k < n; ++k)
        if (v[k]) return true;
    return false;
}

void stats(const QcTables &t, std::string *out) {
    static const char *const kScalar[11] = {"reads", "bases", "mapped", "bases_mapped", "clipped", "nm_sum", "nm_missing", "qual_sum",
                                            "qual_bases", "bases_over", "no_qual"};
    const int64_t *s = t.sum.scalars;
    const int64_t mc = t.opt.max_cycle, mi = t.opt.max_isize;
    for (int k = 0; k < 11; ++k) put(out, "SN\t%s\t%lld\n", kScalar[k], (long long)s[k]);
    if (s[BWAMS_QC_BASES_MAPPED]) put(out, "SN\terror_rate\t%.6e\n", (double)s[BWAMS_QC_NM_SUM] / (double)s[BWAMS_QC_BASES_MAPPED]);
    else out->append("SN\terror_rate\t0\n");
    if (s[BWAMS_QC_QUAL_BASES]) put(out, "SN\taverage_quality\t%.1f\n", (double)s[BWAMS_QC_QUAL_SUM] / (double)s[BWAMS_QC_QUAL_BASES]);
    else out->append("SN\taverage_quality\t0\n");
    const int64_t *is = t.table[BWAMS_QC_TABLE_ISIZE];
    auto pairs_at = [&](int64_t x) { return is[x] + is[mi + 1 + x] + is[2 * (mi + 1) + x]; };
    unsigned __int128 n = 0, s1 = 0, s2 = 0;                             // the bins below max_isize
    for (int64_t x = 0; x < mi; ++x) {
        const unsigned __int128 c = (unsigned __int128)pairs_at(x);
        n += c; s1 += c * (unsigned __int128)x; s2 += c * (unsigned __int128)x * (unsigned __int128)x;
    }
    put(out, "SN\tinsert_size_n\t%lld\n", (long long)n);
    if (n) {
        int64_t median = 0;
        unsigned __int128 cum = 0;
        for (int64_t x = 0; x < mi; ++x) {
            cum += (unsigned __int128)pairs_at(x);
            if (cum >= (n + 1) / 2) { median = x; break; }
        }
        put(out, "SN\tinsert_size_mean\t%.1f\n", (double)s1 / (double)n);
        put(out, "SN\tinsert_size_sd\t%.1f\n", std::sqrt((double)(n * s2 - s1 * s1)) / (double)n);
        put(out, "SN\tinsert_size_median\t%lld\n", (long long)median);
    } else {
        out->append("SN\tinsert_size_mean\t0\nSN\tinsert_size_sd\t0\nSN\tinsert_size_median\t0\n");
    }
    const int64_t *rl = t.table[BWAMS_QC_TABLE_RL];
    for (int64_t x = 0; x <= mc; ++x)
        if (rl[x] || rl[mc + 1 + x]) put(out, "RL\t%lld\t%lld\t%lld\n", (long long)x, (long long)rl[x], (long long)rl[mc + 1 + x]);
    const int64_t *qual = t.table[BWAMS_QC_TABLE_QUAL];
    for (int c = 0; c < 2; ++c) {
        const int64_t *q = qual + c * mc * 64;
        int64_t last = mc;
        while (last > 0 && !any(q + (last - 1) * 64, 64)) --last;
        for (int64_t cyc = 0; cyc < last; ++cyc) {
            put(out, "%s\t%lld", c ? "LFQ" : "FFQ", (long long)cyc + 1);
            for (int k = 0; k < 64; ++k) put(out, "\t%lld", (long long)q[cyc * 64 + k]);
            out->push_back('\n');
        }
    }
    const int64_t *base = t.table[BWAMS_QC_TABLE_BASE];
    int64_t last = mc;
    while (last > 0 && !any(base + (last - 1) * 5, 5) && !any(base + (mc + last - 1) * 5, 5)) --last;
    for (int64_t cyc = 0; cyc < last; ++cyc) {
        put(out, "GCC\t%lld", (long long)cyc + 1);
        for (int c = 0; c < 2; ++c)
            for (int k = 0; k < 5; ++k) put(out, "\t%lld", (long long)base[(c * mc + cyc) * 5 + k]);
        out->push_back('\n');
    }
    const int64_t *mapq = t.table[BWAMS_QC_TABLE_MAPQ];
    for (int x = 0; x < 256; ++x)
        if (mapq[x]) put(out, "MAPQ\t%d\t%lld\n", x, (long long)mapq[x]);
    for (int64_t x = 0; x <= mi; ++x)
        if (pairs_at(x)) put(out, "IS\t%lld\t%lld\t%lld\t%lld\n", (long long)x, (long long)is[x], (long long)is[mi + 1 + x], (long long)is[2 * (mi + 1) + x]);
    const int64_t *id = t.table[BWAMS_QC_TABLE_INDEL];
    for (int x = 0; x < 65; ++x)
        if (id[x] || id[65 + x]) put(out, "ID\t%d\t%lld\t%lld\n", x, (long long)id[x], (long long)id[65 + x]);
}

}  // namespace

int qc_text_format(const QcTables &t, int32_t what, std::string *out) {
    out->clear();
    if (what == BWAMS_QC_TEXT_FLAGSTAT) flagstat(t, out);
    else if (what == BWAMS_QC_TEXT_STATS) stats(t, out);
    else return BWAMS_ERR_ARG;
    return BWAMS_OK;
}

}  // namespace bwams
