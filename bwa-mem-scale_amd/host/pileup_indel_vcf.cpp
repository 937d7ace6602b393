// pileup_indel_vcf.cpp — the VCF text of the pileup's indel calls (include/bwams.h, rule 17): the header with its INDEL line, a row per
// indel call, and the merge with the SNV rows of host/pileup_vcf.cpp by position.  Plain C++ with no HIP header: it also builds alone,
// with tools/pileup_indel_vcf_check.cpp, under the host sanitizers.  bwams/pileup.py restates it byte for byte.
#include <cstdio>

#include "pileup_host.h"

namespace bwams {

int pileup_indel_vcf_row(const std::vector<const char *> &name, const bwams_pileup_region_t *regions, int32_t n_regions,
                         const bwams_pileup_indel_t &c, std::string *out) {
    const int32_t n_ref = (int32_t)name.size();
    if (c.region < 0 || c.region >= n_regions || regions[c.region].ref < 0 || regions[c.region].ref >= n_ref || c.ref < 0 || c.ref > 3 ||
        (c.type != BWAMS_PILEUP_EV_DEL && c.type != BWAMS_PILEUP_EV_INS) || c.len < 0 || c.len > BWAMS_PILEUP_INDEL_MAX || c.gt < 1 || c.gt > 2)
        return BWAMS_ERR_ARG;
    if (c.type == BWAMS_PILEUP_EV_DEL)
        for (int j = 0; j < c.len; ++j)
            if (c.del_ref[j] > 4) return BWAMS_ERR_ARG;
    char buf[160];                                                       // the longest piece: seven numbers of at most 11 characters and 40 of text
    out->append(name[(size_t)regions[c.region].ref]);
    snprintf(buf, sizeof buf, "\t%lld\t.\t%c", (long long)c.pos + 1, "ACGT"[c.ref]);
    out->append(buf);
    if (c.type == BWAMS_PILEUP_EV_DEL)                                   // REF: the anchor and the deleted letters; ALT: the anchor
        for (int j = 0; j < c.len; ++j) out->push_back("ACGTN"[c.del_ref[j]]);
    out->push_back('\t');
    out->push_back("ACGT"[c.ref]);
    if (c.type == BWAMS_PILEUP_EV_INS)                                   // REF: the anchor; ALT: the anchor and the inserted letters
        for (int j = 0; j < c.len; ++j) out->push_back("ACGT"[c.seq >> (2 * j) & 3]);
    snprintf(buf, sizeof buf, "\t%d\t.\tDP=%u;INDEL\tGT:AD:DP:GQ:PL\t%s:%u,%u:%u:%d:", c.qual, c.depth, c.gt == 1 ? "0/1" : "1/1", c.n_ref, c.n_alt,
             c.depth, c.gq);
    out->append(buf);
    snprintf(buf, sizeof buf, "%d,%d,%d\n", c.pl[0], c.pl[1], c.pl[2]);
    out->append(buf);
    return BWAMS_OK;
}

int pileup_indel_vcf_format(const char *names, const int32_t *l_ref, int32_t n_ref, const bwams_pileup_region_t *regions, int32_t n_regions,
                            const char *sample, const bwams_pileup_call_t *snvs, int64_t n_snvs, const bwams_pileup_indel_t *indels,
                            int64_t n_indels, std::string *out) {
    std::vector<const char *> name;
    pileup_vcf_header(names, l_ref, n_ref, sample, true, &name, out);
    int64_t i = 0, j = 0;
    while (i < n_snvs || j < n_indels) {                                 // both lists ascend by (region, pos): the SNV first where they meet
        const bool snv = j >= n_indels || (i < n_snvs && (snvs[i].region < indels[j].region ||
                                                           (snvs[i].region == indels[j].region && snvs[i].pos <= indels[j].pos)));
        if (int rc = snv ? pileup_vcf_row(name, regions, n_regions, snvs[i++], out) : pileup_indel_vcf_row(name, regions, n_regions, indels[j++], out))
            return rc;
    }
    return BWAMS_OK;
}

}  // namespace bwams
