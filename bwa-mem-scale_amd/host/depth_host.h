// depth_host.h — what the depth handle (csrc/api_depth.hip) shares with plain host code: the text of rule 11 (host/depth_text.cpp,
// which also builds alone: tools/depth_text_check.cpp) and what the sorted BAM writer asks of a handle.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "bwams.h"

namespace bwams {

// The small results bwams_depth_text prints.  names: n_ref NUL-terminated names back to back.  rows: n_ref.  hist: (n_ref + 1) rows
// of n_bins, the first for all references (BWAMS_DEPTH_TEXT_DIST).  sums: rule 9's windows of w bases (BWAMS_DEPTH_TEXT_WINDOWS).
struct DepthTextIn {
    const char *names = nullptr;
    int32_t n_ref = 0;
    const bwams_depth_ref_t *rows = nullptr;
    const int64_t *hist = nullptr;
    int32_t n_bins = 0;
    const int64_t *sums = nullptr;
    int32_t w = 0;
};
int depth_text_format(int32_t what, const DepthTextIn &in, std::string *out);    // BWAMS_OK, or BWAMS_ERR_ARG for an unknown `what`

void set_last_error(const std::string &s);                                       // csrc/api.hip: bwams_last_error's text
int depth_device(const bwams_depth *d);
const std::vector<int32_t> &depth_l_ref(const bwams_depth *d);

}  // namespace bwams
