// dup_metrics.cpp — the host side of duplicate marking's rules 9 and 13-15 (include/bwams.h above bwams_bam_templates): the groups
// table of a SAM header's @RG lines (bwams_dup_groups_*), Picard's estimateLibrarySize (bwams_dup_library_size) and the
// DuplicationMetrics text (bwams_dup_metrics_text).  Picard's histogram section (the return-on-investment table under the metrics) is
// not written.  Plain C++ with no HIP and no other file of the library behind it, so that it also builds alone, under a sanitizer.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>

#include "bwams.h"
#include "dup_groups.h"

namespace bwams {

int64_t dup_library_size(int64_t n_, int64_t c_) {
    if (n_ <= 0 || n_ - c_ <= 0 || c_ <= 0) return -1;      // c <= 0 (every pair a duplicate of nothing kept) cannot occur with n > 0
    const double n = (double)n_, c = (double)c_;
    auto f = [&](double x) { return c / x - 1.0 + std::exp(-n / x); };
    double m = 1.0, M = 100.0;
    while (f(M * c) > 0) M *= 10.0;
    for (int i = 0; i < 40; ++i) {
        const double r = (m + M) / 2.0, u = f(r * c);
        if (u == 0) break;
        if (u > 0) m = r;
        else M = r;
    }
    return (int64_t)(c * (m + M) / 2.0);
}

void dup_lib_finish(bwams_dup_lib_stats_t *r) {
    const int64_t den = r->unpaired_examined + 2 * r->pairs_examined;
    r->percent_duplication = den ? (double)(r->unpaired_duplicates + 2 * r->pair_duplicates) / (double)den : 0.0;
    r->estimated_library_size = dup_library_size(r->pairs_examined - r->pair_optical_duplicates, r->pairs_examined - r->pair_duplicates);
}

}  // namespace bwams

namespace {

const char kUnknown[] = "Unknown Library";
const char kColumns[] = "LIBRARY\tUNPAIRED_READS_EXAMINED\tREAD_PAIRS_EXAMINED\tSECONDARY_OR_SUPPLEMENTARY_RDS\tUNMAPPED_READS\t"
                        "UNPAIRED_READ_DUPLICATES\tREAD_PAIR_DUPLICATES\tREAD_PAIR_OPTICAL_DUPLICATES\tPERCENT_DUPLICATION\t"
                        "ESTIMATED_LIBRARY_SIZE\n";

// the value of `tag` (two letters) among the tab-separated fields of line[0, n) behind its first one: false when absent
bool field(const char *line, size_t n, const char *tag, std::string *out) {
    size_t at = 0;
    while (at < n) {
        size_t e = at;
        while (e < n && line[e] != '\t') ++e;
        if (at > 0 && e - at >= 3 && line[at] == tag[0] && line[at + 1] == tag[1] && line[at + 2] == ':') {
            out->assign(line + at + 3, e - at - 3);
            return true;
        }
        at = e + 1;
    }
    return false;
}

}  // namespace

extern "C" {

int bwams_dup_groups_create(const char *header_text, int64_t n_text, bwams_dup_groups_t **out) {
    if (!out || n_text < 0 || (n_text && !header_text)) return BWAMS_ERR_ARG;
    *out = nullptr;
    bwams_dup_groups *g = new (std::nothrow) bwams_dup_groups();
    if (!g) return BWAMS_ERR_NOMEM;
    try {
        std::vector<std::string> lb;                          // each read group's LB, empty for none
        std::vector<char> has_lb;
        for (size_t at = 0, n = (size_t)n_text; at < n;) {
            size_t e = at;
            while (e < n && header_text[e] != '\n') ++e;
            size_t len = e - at;
            if (len && header_text[at + len - 1] == '\r') --len;
            const char *line = header_text + at;
            at = e + 1;
            if (len < 3 || memcmp(line, "@RG", 3) != 0 || (len > 3 && line[3] != '\t')) continue;
            std::string id, l;
            if (!field(line, len, "ID", &id)) { delete g; return BWAMS_ERR_ARG; }
            for (const std::string &x : g->ids)
                if (x == id) { delete g; return BWAMS_ERR_ARG; }
            g->ids.push_back(id);
            has_lb.push_back(field(line, len, "LB", &l));
            lb.push_back(l);
        }
        for (size_t k = 0; k < lb.size(); ++k) {
            if (!has_lb[k]) continue;
            size_t j = 0;
            while (j < g->libs.size() && g->libs[j] != lb[k]) ++j;
            if (j == g->libs.size()) g->libs.push_back(lb[k]);
        }
        const int32_t unknown = (int32_t)g->libs.size();
        for (size_t k = 0; k < lb.size(); ++k) {
            int32_t j = unknown;
            if (has_lb[k])
                for (j = 0; g->libs[(size_t)j] != lb[k]; ++j) {}
            g->rg_lib.push_back(j);
        }
        g->libs.push_back(kUnknown);
    } catch (...) {
        delete g;
        return BWAMS_ERR_NOMEM;
    }
    *out = g;
    return BWAMS_OK;
}

int bwams_dup_groups_info(const bwams_dup_groups_t *g, int64_t *n_rg, int64_t *n_lib) {
    if (!g) return BWAMS_ERR_ARG;
    if (n_rg) *n_rg = (int64_t)g->ids.size();
    if (n_lib) *n_lib = (int64_t)g->libs.size();
    return BWAMS_OK;
}

const char *bwams_dup_groups_library(const bwams_dup_groups_t *g, int64_t lib) {
    if (!g) return lib == 0 ? kUnknown : nullptr;
    return lib >= 0 && lib < (int64_t)g->libs.size() ? g->libs[(size_t)lib].c_str() : nullptr;
}

const char *bwams_dup_groups_rg_id(const bwams_dup_groups_t *g, int64_t rg) {
    return g && rg >= 0 && rg < (int64_t)g->ids.size() ? g->ids[(size_t)rg].c_str() : nullptr;
}

void bwams_dup_groups_destroy(bwams_dup_groups_t *g) { delete g; }

int64_t bwams_dup_library_size(int64_t n, int64_t c) { return bwams::dup_library_size(n, c); }

int bwams_dup_metrics_text(const bwams_dup_groups_t *g, const bwams_dup_lib_stats_t *lib_stats, int64_t n_lib, const char *comment,
                           char *out, int64_t cap, int64_t *n_out) {
    if (n_lib < 0 || (n_lib && !lib_stats) || cap < 0 || (cap && !out) || n_lib != (g ? (int64_t)g->libs.size() : 1)) return BWAMS_ERR_ARG;
    try {
        std::string s = "## htsjdk.samtools.metrics.StringHeader\n# ";
        s += comment ? comment : "";
        s += "\n## METRICS CLASS\tpicard.sam.DuplicationMetrics\n";
        s += kColumns;
        for (int64_t k = 0; k < n_lib; ++k) {
            const bwams_dup_lib_stats_t &r = lib_stats[k];
            if (r.unpaired_examined <= 0 && r.pairs_examined <= 0 && r.secondary_or_supplementary <= 0 && r.unmapped <= 0 &&
                r.unpaired_duplicates <= 0 && r.pair_duplicates <= 0 && r.pair_optical_duplicates <= 0)
                continue;
            char row[256];
            snprintf(row, sizeof row, "\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%.6f\t", (long long)r.unpaired_examined,
                     (long long)r.pairs_examined, (long long)r.secondary_or_supplementary, (long long)r.unmapped,
                     (long long)r.unpaired_duplicates, (long long)r.pair_duplicates, (long long)r.pair_optical_duplicates,
                     r.percent_duplication);
            s += bwams_dup_groups_library(g, k);
            s += row;
            if (r.estimated_library_size >= 0) s += std::to_string((long long)r.estimated_library_size);
            s += "\n";
        }
        s += "\n";
        if (n_out) *n_out = (int64_t)s.size();
        if ((int64_t)s.size() > cap) return BWAMS_ERR_CAPACITY;
        memcpy(out, s.data(), s.size());
    } catch (...) {
        return BWAMS_ERR_NOMEM;
    }
    return BWAMS_OK;
}

}  // extern "C"
