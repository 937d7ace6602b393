// recal_model.cpp — the quality model of base recalibration (include/bwams.h, "Applying base recalibration"): read group, then
// reported quality, then cycle and context deltas, every cell shrunk towards its parent by prior_obs pseudo-observations.  Integer
// arithmetic throughout: a quality is a count of comparisons of products below 2^128 against the two constant tables below, so no
// floating point and no libm call stands between the count tables and the model.  bwams/recal_apply.py restates it.
#include "recal_model_host.h"

namespace bwams {

// S[k]: the largest s with s^20 <= 2^320 * 10^(2k - 1), that is floor(2^16 * 10^((2k - 1) / 20)): the ratio, scaled by 2^16, at which
// a quality rounds from k - 1 up to k.
const uint64_t kRecalS[kModelMaxQ + 1] = {
    0ULL,
    73532ULL, 92572ULL, 116541ULL, 146716ULL, 184705ULL, 232530ULL,
    292738ULL, 368536ULL, 463959ULL, 584090ULL, 735326ULL, 925720ULL,
    1165413ULL, 1467168ULL, 1847055ULL, 2325305ULL, 2927385ULL, 3685360ULL,
    4639593ULL, 5840902ULL, 7353260ULL, 9257206ULL, 11654131ULL, 14671682ULL,
    18470554ULL, 23253050ULL, 29273855ULL, 36853601ULL, 46395934ULL, 58409021ULL,
    73532601ULL, 92572060ULL, 116541319ULL, 146716828ULL, 184705543ULL, 232530502ULL,
    292738558ULL, 368536010ULL, 463959349ULL, 584090214ULL, 735326014ULL, 925720605ULL,
    1165413194ULL, 1467168285ULL, 1847055437ULL, 2325305027ULL, 2927385589ULL, 3685360108ULL,
    4639593492ULL, 5840902148ULL, 7353260142ULL, 9257206052ULL, 11654131941ULL, 14671682853ULL,
    18470554378ULL, 23253050276ULL, 29273855895ULL, 36853601087ULL, 46395934925ULL, 58409021481ULL,
};

// P[q]: the largest p with p^10 * 10^q <= 2^400, that is floor(2^40 * 10^(-q / 10)): the error rate of quality q, scaled by 2^40.
const uint64_t kRecalP[kModelQuals] = {
    1099511627776ULL, 873373130350ULL, 693744936886ULL, 551061191066ULL, 437723463124ULL, 347696105761ULL,
    276184833909ULL, 219381411577ULL, 174260849389ULL, 138420312877ULL, 109951162777ULL, 87337313035ULL,
    69374493688ULL, 55106119106ULL, 43772346312ULL, 34769610576ULL, 27618483390ULL, 21938141157ULL,
    17426084938ULL, 13842031287ULL, 10995116277ULL, 8733731303ULL, 6937449368ULL, 5510611910ULL,
    4377234631ULL, 3476961057ULL, 2761848339ULL, 2193814115ULL, 1742608493ULL, 1384203128ULL,
    1099511627ULL, 873373130ULL, 693744936ULL, 551061191ULL, 437723463ULL, 347696105ULL,
    276184833ULL, 219381411ULL, 174260849ULL, 138420312ULL, 109951162ULL, 87337313ULL,
    69374493ULL, 55106119ULL, 43772346ULL, 34769610ULL, 27618483ULL, 21938141ULL,
    17426084ULL, 13842031ULL, 10995116ULL, 8733731ULL, 6937449ULL, 5510611ULL,
    4377234ULL, 3476961ULL, 2761848ULL, 2193814ULL, 1742608ULL, 1384203ULL,
    1099511ULL, 873373ULL, 693744ULL, 551061ULL, 437723ULL, 347696ULL,
    276184ULL, 219381ULL, 174260ULL, 138420ULL, 109951ULL, 87337ULL,
    69374ULL, 55106ULL, 43772ULL, 34769ULL, 27618ULL, 21938ULL,
    17426ULL, 13842ULL, 10995ULL, 8733ULL, 6937ULL, 5510ULL,
    4377ULL, 3476ULL, 2761ULL, 2193ULL, 1742ULL, 1384ULL,
    1099ULL, 873ULL, 693ULL, 551ULL,
};

// num < 2^88 and S[k] < 2^36, den << 16 < 2^98: every product stays below 2^128.  S grows with k, so the count ends at the first miss.
int recal_phred(unsigned __int128 num, unsigned __int128 den, int cap) {
    int k = 0;
    while (k < cap && num * kRecalS[k + 1] <= den << 16) ++k;
    return k;
}

int recal_post(uint64_t n, uint64_t e, int qp, uint64_t m, int cap) {
    return recal_phred(((unsigned __int128)e << 40) + (unsigned __int128)m * kRecalP[qp], (unsigned __int128)(n + m) << 40, cap);
}

namespace {

constexpr int64_t kMaxCount = (int64_t)1 << 40;

// the first cell of n cells (int64 pairs) that the model does not take, or -1
int64_t first_bad_cell(const int64_t *t, int64_t n) {
    for (int64_t k = 0; k < n; ++k) {
        const int64_t obs = t[2 * k], err = t[2 * k + 1];
        if (obs < 0 || err < 0 || err > obs || obs >= kMaxCount) return k;
    }
    return -1;
}

}  // namespace

int recal_model_make(const int64_t *rg, const int64_t *qual, const int64_t *cycle, const int64_t *context, int32_t n_rg, int32_t max_cycle,
                     const bwams_recal_model_opt_t *opt, bwams_recal_model *out, std::string *err) {
    const bwams_recal_model_opt_t o = opt ? *opt : bwams_recal_model_opt_t{0, 6, 60, 1024, 0};
    if (!rg || !qual || !cycle || !context || !out || n_rg < 0 || n_rg > (1 << 24) || max_cycle < 1 || max_cycle > (1 << 20)) {
        *err = "the four tables, 0 <= n_rg <= 2^24 and 1 <= max_cycle <= 2^20 are required";
        return BWAMS_ERR_ARG;
    }
    if (o.exclude > 0xFFFFu || o.preserve_below < 0 || o.preserve_below > 93 || o.max_q < 1 || o.max_q > kModelMaxQ || o.prior_obs < 1 ||
        o.prior_obs > (1 << 20) || o.reserved != 0) {
        *err = "exclude within 16 bits, preserve_below in [0, 93], max_q in [1, 60], prior_obs in [1, 2^20] and reserved == 0 are required";
        return BWAMS_ERR_ARG;
    }
    const int64_t rows = (int64_t)n_rg + 1, cols = 2 * (int64_t)max_cycle + 1;
    const int64_t cells[4] = {rows, rows * kModelQuals, rows * kModelQuals * cols, rows * kModelQuals * kModelContexts};
    const int64_t *tables[4] = {rg, qual, cycle, context};
    static const char *const names[4] = {"RG", "QUAL", "CYCLE", "CONTEXT"};
    for (int t = 0; t < 4; ++t) {
        const int64_t bad = first_bad_cell(tables[t], cells[t]);
        if (bad >= 0) {
            *err = std::string("cell ") + std::to_string(bad) + " of table " + names[t] +
                   " is negative, has more errors than observations, or holds 2^40 or more";
            return BWAMS_ERR_UNSUPPORTED;
        }
    }
    bwams_recal_model m;
    m.n_rg = n_rg;
    m.max_cycle = max_cycle;
    m.opt = o;
    m.rg.assign((size_t)rows * 3, 0);
    m.b.assign((size_t)cells[1], 0);
    m.dc.assign((size_t)cells[2], 0);
    m.dx.assign((size_t)cells[3], 0);
    const uint64_t prior = (uint64_t)o.prior_obs;
    const int cap = o.max_q;
    for (int64_t g = 0; g < rows; ++g) {
        int16_t *r = m.rg.data() + 3 * g;
        const uint64_t n_g = (uint64_t)rg[2 * g], e_g = (uint64_t)rg[2 * g + 1];
        if (n_g > 0) {
            unsigned __int128 e_rep = 0;                                 // the errors the reported qualities promise, scaled by 2^40
            for (int q = 0; q < kModelQuals; ++q) e_rep += (unsigned __int128)(uint64_t)qual[2 * (g * kModelQuals + q)] * kRecalP[q];
            const int q_rep = recal_phred(e_rep, (unsigned __int128)n_g << 40, cap);
            const int q_g = recal_post(n_g, e_g, q_rep, prior, cap);
            r[0] = (int16_t)q_rep; r[1] = (int16_t)q_g; r[2] = (int16_t)(q_g - q_rep);
        } else {
            r[0] = r[1] = -1; r[2] = 0;
        }
        for (int q = 0; q < kModelQuals; ++q) {
            const int64_t row = g * kModelQuals + q;
            const int qp = q + r[2] < 0 ? 0 : q + r[2] > 93 ? 93 : q + r[2];
            const uint64_t n_q = (uint64_t)qual[2 * row], e_q = (uint64_t)qual[2 * row + 1];
            const int b = n_q > 0 ? recal_post(n_q, e_q, qp, prior, cap) : qp;
            m.b[(size_t)row] = (int16_t)b;
            for (int64_t c = 0; c < cols; ++c) {
                const int64_t at = row * cols + c;
                if (cycle[2 * at] > 0) m.dc[(size_t)at] = (int16_t)(recal_post((uint64_t)cycle[2 * at], (uint64_t)cycle[2 * at + 1], b, prior, cap) - b);
            }
            for (int64_t x = 0; x < kModelContexts; ++x) {
                const int64_t at = row * kModelContexts + x;
                if (context[2 * at] > 0)
                    m.dx[(size_t)at] = (int16_t)(recal_post((uint64_t)context[2 * at], (uint64_t)context[2 * at + 1], b, prior, cap) - b);
            }
        }
    }
    *out = std::move(m);
    return BWAMS_OK;
}

}  // namespace bwams
