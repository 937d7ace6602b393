// pileup_vcf.cpp — the VCF text of the pileup's SNV calls (include/bwams.h, rule 13 and the paragraph on bwams_pileup_vcf): the header
// lines and a row per call.  Plain C++ with no HIP header: it also builds alone, with tools/pileup_vcf_check.cpp, under the host
// sanitizers.  bwams/pileup.py restates it byte for byte.
#include <cstdio>
#include <cstring>

#include "pileup_host.h"

namespace bwams {

void pileup_vcf_header(const char *names, const int32_t *l_ref, int32_t n_ref, const char *sample, bool indel, std::vector<const char *> *names_out,
                       std::string *out) {
    std::vector<const char *> &name = *names_out;
    name.resize((size_t)n_ref);
    const char *p = names;
    for (int32_t r = 0; r < n_ref; ++r) { name[(size_t)r] = p; p += strlen(p) + 1; }
    char buf[48];
    out->assign("##fileformat=VCFv4.2\n##source=bwams\n");
    for (int32_t r = 0; r < n_ref; ++r) {
        out->append("##contig=<ID=").append(name[(size_t)r]);
        snprintf(buf, sizeof buf, ",length=%d>\n", l_ref[r]);
        out->append(buf);
    }
    out->append("##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Bases counted\">\n");
    if (indel) out->append("##INFO=<ID=INDEL,Number=0,Type=Flag,Description=\"An insertion or deletion, as the CIGARs give it\">\n");
    out->append("##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
                "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Bases counted per allele\">\n"
                "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Bases counted\">\n"
                "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality\">\n"
                "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Genotype costs in phred, the least at 0\">\n"
                "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t");
    out->append(sample).push_back('\n');
}

int pileup_vcf_row(const std::vector<const char *> &name, const bwams_pileup_region_t *regions, int32_t n_regions, const bwams_pileup_call_t &c,
                   std::string *out) {
    const int32_t n_ref = (int32_t)name.size();
    char buf[48];
    if (c.region < 0 || c.region >= n_regions || regions[c.region].ref < 0 || regions[c.region].ref >= n_ref || c.ref < 0 || c.ref > 3 ||
        c.a1 < 0 || c.a1 > c.a2 || c.a2 > 3 || (c.a1 == c.ref && c.a2 == c.ref))
        return BWAMS_ERR_ARG;
    int allele[3] = {c.ref, 0, 0}, n_alleles = 1;                    // REF, then the genotype's other alleles in base order
    if (c.a1 != c.ref) allele[n_alleles++] = c.a1;
    if (c.a2 != c.ref && c.a2 != c.a1) allele[n_alleles++] = c.a2;
    int gt[2] = {0, 0};                                              // the indices of a1 and a2 among the alleles
    for (int i = 0; i < n_alleles; ++i) {
        if (allele[i] == c.a1) gt[0] = i;
        if (allele[i] == c.a2) gt[1] = i;
    }
    if (gt[0] > gt[1]) { const int t = gt[0]; gt[0] = gt[1]; gt[1] = t; }
    out->append(name[(size_t)regions[c.region].ref]);
    snprintf(buf, sizeof buf, "\t%lld\t.\t%c\t", (long long)c.pos + 1, "ACGT"[c.ref]);
    out->append(buf);
    for (int i = 1; i < n_alleles; ++i) {
        if (i > 1) out->push_back(',');
        out->push_back("ACGT"[allele[i]]);
    }
    snprintf(buf, sizeof buf, "\t%d\t.\tDP=%u\tGT:AD:DP:GQ:PL\t%d/%d:", c.qual, c.depth, gt[0], gt[1]);
    out->append(buf);
    for (int i = 0; i < n_alleles; ++i) {
        snprintf(buf, sizeof buf, i ? ",%u" : "%u", c.n[allele[i]]);
        out->append(buf);
    }
    snprintf(buf, sizeof buf, ":%u:%d:", c.depth, c.gq);
    out->append(buf);
    for (int j = 0; j < n_alleles; ++j)                              // VCF's genotype order over the alleles' indices
        for (int i = 0; i <= j; ++i) {
            const int lo = allele[i] < allele[j] ? allele[i] : allele[j], hi = allele[i] < allele[j] ? allele[j] : allele[i];
            snprintf(buf, sizeof buf, i || j ? ",%d" : "%d", c.pl[hi * (hi + 1) / 2 + lo]);
            out->append(buf);
        }
    out->push_back('\n');
    return BWAMS_OK;
}

int pileup_vcf_format(const char *names, const int32_t *l_ref, int32_t n_ref, const bwams_pileup_region_t *regions, int32_t n_regions,
                      const char *sample, const bwams_pileup_call_t *calls, int64_t n_calls, std::string *out) {
    std::vector<const char *> name;
    pileup_vcf_header(names, l_ref, n_ref, sample, false, &name, out);
    for (int64_t k = 0; k < n_calls; ++k)
        if (int rc = pileup_vcf_row(name, regions, n_regions, calls[k], out)) return rc;
    return BWAMS_OK;
}

}  // namespace bwams
