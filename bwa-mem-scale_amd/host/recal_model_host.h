// recal_model_host.h — the quality model of base recalibration (include/bwams.h, "Applying base recalibration") as plain host code:
// host/recal_model.cpp makes it from the four count tables in integer arithmetic; csrc/api_recal_apply.hip wraps it into the C-ABI
// and puts it on a device.  It also builds alone (tools/recal_model_check.cpp).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "bwams.h"

struct bwams_recal_model {
    int32_t n_rg = 0, max_cycle = 0;
    bwams_recal_model_opt_t opt{};
    std::vector<int16_t> rg;                 // [n_rg + 1][3]: Qrep, QG, G
    std::vector<int16_t> b;                  // [n_rg + 1][94]
    std::vector<int16_t> dc;                 // [n_rg + 1][94][2 max_cycle + 1]
    std::vector<int16_t> dx;                 // [n_rg + 1][94][16]
    const std::vector<int16_t> &table(int32_t what) const { return what == 0 ? rg : what == 1 ? b : what == 2 ? dc : dx; }
};

namespace bwams {

constexpr int kModelQuals = 94, kModelContexts = 16, kModelMaxQ = 60;
extern const uint64_t kRecalS[kModelMaxQ + 1];       // S[k], k = 1..60; [0] is not used
extern const uint64_t kRecalP[kModelQuals];          // P[q], q = 0..93

// the number of k in 1..cap with num * S[k] <= den << 16
int recal_phred(unsigned __int128 num, unsigned __int128 den, int cap);
// the quality of a cell of n observations and e errors after m pseudo-observations at the prior quality qp
int recal_post(uint64_t n, uint64_t e, int qp, uint64_t m, int cap);

// The model of the four tables (int64 pairs, as bwams_recal_table lays them out) into *out: BWAMS_OK, or BWAMS_ERR_ARG /
// BWAMS_ERR_UNSUPPORTED with the reason in *err and *out untouched.
int recal_model_make(const int64_t *rg, const int64_t *qual, const int64_t *cycle, const int64_t *context, int32_t n_rg, int32_t max_cycle,
                     const bwams_recal_model_opt_t *opt, bwams_recal_model *out, std::string *err);

}  // namespace bwams
