// pileup_host.h — what the pileup handle (csrc/api_pileup.hip) shares with plain host code: the text of rule 9 (host/pileup_text.cpp,
// which also builds alone: tools/pileup_text_check.cpp), the VCF text of rule 13's calls (host/pileup_vcf.cpp, which builds alone too:
// tools/pileup_vcf_check.cpp) and what the sorted BAM writer asks of a handle.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "bwams.h"

namespace bwams {

// Rule 9's text of n_sites sites.  names: the references' NUL-terminated names back to back (n_ref of them); regions: the handle's list.
int pileup_text_format(const char *names, int32_t n_ref, const bwams_pileup_region_t *regions, int32_t n_regions,
                       const bwams_pileup_site_t *sites, int64_t n_sites, std::string *out);    // BWAMS_OK, or BWAMS_ERR_ARG for a site outside the lists

// The VCF text of n_calls calls: the header lines, then a row per call.  names as above, l_ref: the references' lengths (the contig
// lines); sample: the name of the one sample column.
int pileup_vcf_format(const char *names, const int32_t *l_ref, int32_t n_ref, const bwams_pileup_region_t *regions, int32_t n_regions,
                      const char *sample, const bwams_pileup_call_t *calls, int64_t n_calls, std::string *out);    // BWAMS_OK, or BWAMS_ERR_ARG for a call outside the lists or with alleles that are not 0 <= a1 <= a2 <= 3

// The parts of that text, for host/pileup_indel_vcf.cpp: the header lines (indel: with the INDEL line behind DP; *name: the n_ref names,
// for the rows) and the row of one SNV call.
void pileup_vcf_header(const char *names, const int32_t *l_ref, int32_t n_ref, const char *sample, bool indel, std::vector<const char *> *name,
                       std::string *out);
int pileup_vcf_row(const std::vector<const char *> &name, const bwams_pileup_region_t *regions, int32_t n_regions, const bwams_pileup_call_t &c,
                   std::string *out);

// Rule 17's text: the header with the INDEL line, then the rows of the n_snvs SNV calls (none for bwams_pileup_indel_vcf) and the
// n_indels indel calls merged by (region, pos), the SNV first at one position.
int pileup_indel_vcf_row(const std::vector<const char *> &name, const bwams_pileup_region_t *regions, int32_t n_regions,
                         const bwams_pileup_indel_t &c, std::string *out);    // BWAMS_ERR_ARG for a call outside the lists, of no type 0 or 1, len above 32, gt not 1 or 2 or a del_ref above 4
int pileup_indel_vcf_format(const char *names, const int32_t *l_ref, int32_t n_ref, const bwams_pileup_region_t *regions, int32_t n_regions,
                            const char *sample, const bwams_pileup_call_t *snvs, int64_t n_snvs, const bwams_pileup_indel_t *indels,
                            int64_t n_indels, std::string *out);

int pileup_device(const bwams_pileup *p);
const std::vector<int32_t> &pileup_l_ref(const bwams_pileup *p);

}  // namespace bwams
