// recal_host.h — what the recalibration handle (csrc/api_recal.hip) shares with plain host code: the text of rule 10
// (host/recal_text.cpp, which also builds alone: tools/recal_text_check.cpp) and what the sorted BAM writer asks of a handle.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "bwams.h"

namespace bwams {

// The handle's tables on the host, each in its flat shape of rule 6 (int64 pairs), indexed by BWAMS_RECAL_TABLE_*; ids: the n_rg read
// groups' IDs by ordinal (the row behind them prints as `*`).
struct RecalTables {
    int32_t max_cycle;
    std::vector<std::string> ids;
    const int64_t *table[4];
};

// Rule 10's text of the tables in t.
void recal_text_format(const RecalTables &t, std::string *out);

int recal_device(const bwams_recal *r);
const std::vector<int32_t> &recal_l_ref(const bwams_recal *r);

}  // namespace bwams
