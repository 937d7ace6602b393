// depth_text.cpp — the three texts of the depth rules (include/bwams.h, rule 11) from the small results of the queries: the summary
// table, the distribution and the windows BED.  Plain C++ with no HIP header: it also builds alone, with tools/depth_text_check.cpp,
// under the host sanitizers.  bwams/depth.py restates it byte for byte.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "depth_host.h"

namespace bwams {
namespace {

void put(std::string *out, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void put(std::string *out, const char *fmt, ...) {
    char buf[128];
    va_list ap;
    va_start(ap, fmt);
    const int k = vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (k > 0) out->append(buf, (size_t)std::min<int>(k, (int)sizeof buf - 1));
}

void summary_row(std::string *out, const char *name, int64_t length, int64_t bases, int32_t mn, int32_t mx) {
    out->append(name);
    put(out, "\t%lld\t%lld\t%.2f\t%d\t%d\n", (long long)length, (long long)bases, length ? (double)bases / (double)length : 0.0, mn, mx);
}

// rows from the largest occupied bin down to 0: the fraction of the positions at or above each depth
void dist_block(std::string *out, const char *name, const int64_t *hist, int32_t n_bins) {
    int64_t total = 0;
    int32_t top = -1;
    for (int32_t v = 0; v < n_bins; ++v) {
        total += hist[v];
        if (hist[v]) top = v;
    }
    int64_t above = 0;
    for (int32_t v = top; v >= 0; --v) {
        above += hist[v];
        out->append(name);
        put(out, "\t%d\t%.4f\n", v, (double)above / (double)total);
    }
}

}  // namespace

int depth_text_format(int32_t what, const DepthTextIn &in, std::string *out) {
    out->clear();
    std::vector<const char *> name((size_t)in.n_ref);
    const char *p = in.names;
    for (int32_t r = 0; r < in.n_ref; ++r) { name[(size_t)r] = p; p += strlen(p) + 1; }
    if (what == BWAMS_DEPTH_TEXT_SUMMARY) {
        out->append("chrom\tlength\tbases\tmean\tmin\tmax\n");
        int64_t length = 0, bases = 0;
        int32_t mn = 0, mx = 0;
        bool any = false;
        for (int32_t r = 0; r < in.n_ref; ++r) {
            const bwams_depth_ref_t &x = in.rows[r];
            summary_row(out, name[(size_t)r], x.length, x.bases, x.min, x.max);
            length += x.length; bases += x.bases;
            if (x.length > 0) {
                mn = any ? std::min(mn, x.min) : x.min;
                mx = any ? std::max(mx, x.max) : x.max;
                any = true;
            }
        }
        summary_row(out, "total", length, bases, mn, mx);
        return BWAMS_OK;
    }
    if (what == BWAMS_DEPTH_TEXT_DIST) {
        dist_block(out, "total", in.hist, in.n_bins);
        for (int32_t r = 0; r < in.n_ref; ++r) dist_block(out, name[(size_t)r], in.hist + (int64_t)(r + 1) * in.n_bins, in.n_bins);
        return BWAMS_OK;
    }
    if (what == BWAMS_DEPTH_TEXT_WINDOWS) {
        int64_t k = 0;
        for (int32_t r = 0; r < in.n_ref; ++r)
            for (int64_t beg = 0; beg < in.rows[r].length; beg += in.w, ++k) {
                const int64_t end = std::min<int64_t>(beg + in.w, in.rows[r].length);
                out->append(name[(size_t)r]);
                put(out, "\t%lld\t%lld\t%.2f\n", (long long)beg, (long long)end, (double)in.sums[k] / (double)(end - beg));
            }
        return BWAMS_OK;
    }
    return BWAMS_ERR_ARG;
}

}  // namespace bwams
