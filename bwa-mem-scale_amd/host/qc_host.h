// qc_host.h — what the QC handle (csrc/api_qc.hip) shares with plain host code: the texts of rule 7 (host/qc_text.cpp, which also
// builds alone: tools/qc_text_check.cpp) and what the sorted BAM writer asks of a handle.
#pragma once

#include <cstdint>
#include <string>

#include "bwams.h"

namespace bwams {

// The handle's counters on the host: the summary and rule 4's six tables, each in its flat shape, indexed by BWAMS_QC_TABLE_*.
struct QcTables {
    bwams_qc_opt_t opt;
    bwams_qc_summary_t sum;
    const int64_t *table[6];
};

// Rule 7's text `what` of the counters in t.  BWAMS_OK, or BWAMS_ERR_ARG for a `what` there is none of.
int qc_text_format(const QcTables &t, int32_t what, std::string *out);

int qc_device(const bwams_qc *q);

}  // namespace bwams
