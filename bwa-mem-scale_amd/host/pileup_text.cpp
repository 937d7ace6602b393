// pileup_text.cpp — the text of the pileup rules (include/bwams.h, rule 9): a header line and a row per candidate site.  Plain C++ with
// no HIP header: it also builds alone, with tools/pileup_text_check.cpp, under the host sanitizers.  bwams/pileup.py restates it byte
// for byte.
#include <cstdio>
#include <cstring>

#include "pileup_host.h"

namespace bwams {

int pileup_text_format(const char *names, int32_t n_ref, const bwams_pileup_region_t *regions, int32_t n_regions,
                       const bwams_pileup_site_t *sites, int64_t n_sites, std::string *out) {
    static const char *kAllele[6] = {"A", "C", "G", "T", "DEL", "INS"};
    out->assign("chrom\tpos\tref\tdepth\tA+\tC+\tG+\tT+\tA-\tC-\tG-\tT-\tN\tDEL\tINS\talt\n");
    std::vector<const char *> name((size_t)n_ref);
    const char *p = names;
    for (int32_t r = 0; r < n_ref; ++r) { name[(size_t)r] = p; p += strlen(p) + 1; }
    char buf[32];
    for (int64_t k = 0; k < n_sites; ++k) {
        const bwams_pileup_site_t &s = sites[k];
        if (s.region < 0 || s.region >= n_regions || regions[s.region].ref < 0 || regions[s.region].ref >= n_ref || s.ref < 0 || s.ref > 4)
            return BWAMS_ERR_ARG;
        out->append(name[(size_t)regions[s.region].ref]);
        snprintf(buf, sizeof buf, "\t%lld\t%c\t%u", (long long)s.pos + 1, "ACGTN"[s.ref], s.depth);
        out->append(buf);
        for (int ch = 0; ch < BWAMS_PILEUP_CHANNELS - 1; ++ch) {
            snprintf(buf, sizeof buf, "\t%u", s.c[ch]);
            out->append(buf);
        }
        out->push_back('\t');
        bool first = true;
        for (int a = 0; a < 6; ++a)
            if (s.kinds >> a & 1) {
                if (!first) out->push_back(',');
                out->append(kAllele[a]);
                first = false;
            }
        out->push_back('\n');
    }
    return BWAMS_OK;
}

}  // namespace bwams
