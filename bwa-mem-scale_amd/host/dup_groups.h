// dup_groups.h — the groups table of duplicate marking (rule 9 of include/bwams.h) as the library's own code sees it, and the
// host arithmetic of rules 13-14.  dup_metrics.cpp implements them; api_bam.hip and bam_sort.cpp read the table.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "bwams_types.h"

struct bwams_dup_groups {
    std::vector<std::string> ids;          // read groups' IDs, by ordinal
    std::vector<int32_t> rg_lib;           // each read group's library ordinal (the last library, "Unknown Library", without LB)
    std::vector<std::string> libs;         // libraries' names, by ordinal; the last is "Unknown Library"
};

namespace bwams {
int64_t dup_library_size(int64_t n, int64_t c);        // rule 14: -1 for none
void dup_lib_finish(bwams_dup_lib_stats_t *row);       // percent_duplication and estimated_library_size from the row's counts
}
