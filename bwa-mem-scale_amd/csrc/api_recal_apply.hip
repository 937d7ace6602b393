// api_recal_apply.hip — C-ABI entry points of the quality model and its application (include/bwams.h, "Applying base
// recalibration"): the model over host/recal_model.cpp, and the apply handle that holds the model and a groups table on a device
// and rewrites the QUAL bytes of host records or of a batch's records, over recal_apply.hip.
// No CPU fallback: every apply runs HIP kernels or returns an error.
#include <algorithm>
#include <cstring>
#include <memory>

#include "rec_consumer.h"
#include "../host/dup_groups.h"
#include "../host/recal_model_host.h"

using namespace bwams;

struct bwams_recal_apply : RecConsumer {
    int32_t n_rg = 0;
    RecalModelDev M{};
    MdGroupsDev G{};
    DevBuf<uint8_t> b;                               // the model (RecalModelDev)
    DevBuf<int8_t> dc, dx;
    DevBuf<unsigned long long> call;                 // [0] rule B's first bad record, [1] the records of a piece that rule A took
    DevBuf<uint8_t> g_ids;                           // the groups table on the device
    DevBuf<int64_t> g_off;
    DevBuf<int32_t> g_ord, g_lib;
    DevBuf<uint32_t> keys;                           // the keys of a piece
    int64_t model_bytes = 0;
    int64_t last[2] = {0, 0};                        // of the last apply: records given, records rewritten
    float ms_check = 0, ms_apply = 0;                // ... and its device time
    uint32_t n_keys() const { return 2u * (uint32_t)(n_rg + 1); }
};

namespace {

constexpr int64_t kPiece = 1 << 24;                  // records keyed at a time: 4 bytes of scratch per record

// rule B over the records: BWAMS_OK, or the refusal
int apply_check(bwams_recal_apply *a, const DevRecords &R, const char *who) {
    hipStream_t st = a->stream;
    a->ms_check = 0;
    if (R.n_rec <= 0) return BWAMS_OK;
    unsigned long long h = 0;
    if (int rc = consumer_check(a, a->call.p, 1, &h, &a->ms_check, [&] {
            launch_recal_apply_check(R.bam, R.off, R.n_rec, a->M, a->G.walk, a->call.p, a->cu_count, st);
        })) return rc;
    if (h != ~0ULL) {                                                    // by kRecalBad*: rule B has neither of the first two
        static const char *const why[5] = {"", "", " ends inside its SEQ or QUAL (bounds)", " is longer than the model's max_cycle (cycle)",
                                           " has aux fields that do not chain to its end (aux)"};
        return consumer_refuse_packed(who, h, why);
    }
    return BWAMS_OK;
}

// rule C over records that apply_check let through (these, or a copy of them in another order)
int apply_rewrite(bwams_recal_apply *a, const DevRecords &R, int64_t *n_rewritten) {
    hipStream_t st = a->stream;
    const uint32_t n_keys = a->n_keys();
    const int64_t n_rec = R.n_rec;
    int64_t rewritten = 0;
    a->ms_apply = 0;
    if (n_rec > 0) BWAMS_HIP(a->keys.ensure_n((size_t)std::min(kPiece, n_rec)));
    for (int64_t r0 = 0; r0 < n_rec; r0 += kPiece) {
        const int64_t n = std::min(kPiece, n_rec - r0);
        unsigned long long *n_taken = a->call.p + 1, h = 0;
        if (int rc = consumer_piece(a, n_taken, 1, &h, &a->ms_apply, [&] {
                launch_recal_apply_records(R.bam, R.off + r0, n, a->M, a->G, n_keys, a->keys.p, n_taken, a->cu_count, st);
                launch_recal_apply(R.bam, R.off + r0, n, a->M, a->keys.p, n_keys, a->cu_count, st);
                return BWAMS_OK;
            })) return rc;
        rewritten += (int64_t)h;
    }
    a->last[0] = n_rec; a->last[1] = rewritten;
    if (n_rewritten) *n_rewritten = rewritten;
    return BWAMS_OK;
}

// a device copy of n values of the model as bytes
template <class T> int model_upload(DevBuf<T> &dst, const std::vector<int16_t> &src, hipStream_t st) {
    std::vector<T> bytes(src.begin(), src.end());
    BWAMS_HIP(dst.alloc(std::max<size_t>(bytes.size(), 1)));
    BWAMS_HIP(hipMemcpyAsync(dst.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipStreamSynchronize(st));                                 // the host vector ends here
    return BWAMS_OK;
}

}  // namespace

extern "C" {

int bwams_recal_model_create(const int64_t *rg, const int64_t *qual, const int64_t *cycle, const int64_t *context, int32_t n_rg,
                             int32_t max_cycle, const bwams_recal_model_opt_t *opt, bwams_recal_model_t **out) {
    if (!out) {
        set_last_error("bwams_recal_model_create: out is required");
        return BWAMS_ERR_ARG;
    }
    *out = nullptr;
    std::unique_ptr<bwams_recal_model> m(new bwams_recal_model());
    std::string err;
    if (int rc = recal_model_make(rg, qual, cycle, context, n_rg, max_cycle, opt, m.get(), &err)) {
        set_last_error("bwams_recal_model_create: " + err);
        return rc;
    }
    *out = m.release();
    return BWAMS_OK;
}

int bwams_recal_model_from(bwams_recal_t *r, const bwams_recal_model_opt_t *opt, bwams_recal_model_t **out) {
    int64_t n[4] = {0, 0, 0, 0};
    if (!r || !out) {
        set_last_error("bwams_recal_model_from: a recalibration handle and out are required");
        return BWAMS_ERR_ARG;
    }
    *out = nullptr;
    std::vector<int64_t> t[4];
    for (int32_t k = 0; k < 4; ++k) {
        if (int rc = bwams_recal_table(r, k, nullptr, 0, &n[k])) return rc;
        t[k].resize((size_t)n[k]);
        if (int rc = bwams_recal_table(r, k, t[k].data(), n[k], nullptr)) return rc;
    }
    const int64_t rows = n[0] / 2, cols = n[2] / (n[1] ? n[1] : 1);      // [rows][2], [rows][94][2], [rows][94][cols][2]
    return bwams_recal_model_create(t[0].data(), t[1].data(), t[2].data(), t[3].data(), (int32_t)(rows - 1), (int32_t)((cols - 1) / 2), opt,
                                    out);
}

int bwams_recal_model_table(const bwams_recal_model_t *m, int32_t what, int16_t *out, int64_t cap, int64_t *n) {
    if (!m || cap < 0 || what < 0 || what > 3) {
        set_last_error("bwams_recal_model_table: a model, a table of BWAMS_RECAL_TABLE_* and cap >= 0 are required");
        return BWAMS_ERR_ARG;
    }
    const std::vector<int16_t> &t = m->table(what);
    if (n) *n = (int64_t)t.size();
    if (!out) return BWAMS_OK;
    if (cap < (int64_t)t.size()) {
        set_last_error("bwams_recal_model_table: " + std::to_string(t.size()) + " values do not fit a capacity of " + std::to_string(cap));
        return BWAMS_ERR_CAPACITY;
    }
    memcpy(out, t.data(), t.size() * sizeof(int16_t));
    return BWAMS_OK;
}

int bwams_recal_model_constants(int64_t *S, int64_t *P) {
    if (!S || !P) return BWAMS_ERR_ARG;
    for (int k = 1; k <= kModelMaxQ; ++k) S[k - 1] = (int64_t)kRecalS[k];
    for (int q = 0; q < kModelQuals; ++q) P[q] = (int64_t)kRecalP[q];
    return BWAMS_OK;
}

int bwams_recal_model_destroy(bwams_recal_model_t *m) {
    delete m;
    return BWAMS_OK;
}

int bwams_recal_apply_open(int device, const bwams_recal_model_t *m, const bwams_dup_groups_t *groups, bwams_recal_apply_t **out) {
    if (!out || !m) {
        set_last_error("bwams_recal_apply_open: a model and out are required");
        return BWAMS_ERR_ARG;
    }
    *out = nullptr;
    if ((groups ? (int64_t)groups->ids.size() : 0) != m->n_rg) {
        set_last_error("bwams_recal_apply_open: the model has " + std::to_string(m->n_rg) + " read groups, the groups table " +
                       (groups ? std::to_string(groups->ids.size()) : std::string("is missing")));
        return BWAMS_ERR_ARG;
    }
    std::unique_ptr<bwams_recal_apply> a(new bwams_recal_apply());
    if (int rc = a->open(device)) return rc;
    a->n_rg = m->n_rg;
    hipStream_t st = a->stream;
    BWAMS_HIP(a->call.alloc(2 * 8));
    if (int rc = model_upload(a->b, m->b, st)) return rc;
    if (int rc = model_upload(a->dc, m->dc, st)) return rc;
    if (int rc = model_upload(a->dx, m->dx, st)) return rc;
    a->model_bytes = (int64_t)(m->b.size() + m->dc.size() + m->dx.size());
    a->M = RecalModelDev{a->b.p, a->dc.p, a->dx.p, m->n_rg, m->max_cycle, m->opt.preserve_below, m->opt.max_q, m->opt.exclude};
    if (int rc = groups_upload(a->g_ids, a->g_off, a->g_ord, a->g_lib, groups, &a->G, st)) return rc;
    BWAMS_HIP(hipStreamSynchronize(st));
    *out = a.release();
    return BWAMS_OK;
}

int bwams_recal_apply_close(bwams_recal_apply_t *a) {
    delete a;
    return BWAMS_OK;
}

int bwams_recal_apply_records(bwams_recal_apply_t *a, void *bam, int64_t n_bytes, int64_t *n_rewritten) {
    DevRecords R;
    if (int rc = consumer_records(a, bam, n_bytes, "bwams_recal_apply_records", &R)) return rc;
    if (int rc = apply_check(a, R, "bwams_recal_apply_records")) return rc;
    if (int rc = apply_rewrite(a, R, n_rewritten)) return rc;
    if (n_bytes) BWAMS_HIP(hipMemcpyAsync(bam, R.bam, (size_t)n_bytes, hipMemcpyDeviceToHost, a->stream));
    BWAMS_HIP(hipStreamSynchronize(a->stream));
    return BWAMS_OK;
}

int bwams_recal_apply_file(bwams_recal_apply_t *a, bwams_bam_file_t *f, int64_t *n_rewritten) {
    DevRecords R;
    if (int rc = consumer_file(a, f, "bwams_recal_apply_file", &R)) return rc;
    if (int rc = apply_check(a, R, "bwams_recal_apply_file")) return rc;
    return apply_rewrite(a, R, n_rewritten);
}

int bwams_recal_apply_batch(bwams_recal_apply_t *a, bwams_batch_t *b, int64_t *n_rewritten) {
    DevRecords R;
    StageState *s = nullptr;
    if (int rc = consumer_batch(a, b, "bwams_recal_apply_batch", &R, nullptr, &s)) return rc;
    if (int rc = apply_check(a, R, "bwams_recal_apply_batch")) return rc;
    int64_t n = 0;
    float ms = 0;
    outdated(b, Product::templates);                         // the templates' scores are sums of the old qualities
    if (has(b, Product::sorted)) {                           // the sorted copy holds the same records: the check above covers it
        if (int rc = apply_rewrite(a, DevRecords{s->bs.out.p, s->bs.off.p, s->bs.nrec}, &n)) return rc;
        ms = a->ms_apply;
    }
    if (int rc = apply_rewrite(a, R, &n)) return rc;
    a->ms_apply += ms;
    if (n_rewritten) *n_rewritten = n;
    return BWAMS_OK;
}

int bwams_recal_apply_info(const bwams_recal_apply_t *a, bwams_recal_apply_info_t *info) {
    if (!a || !info) return BWAMS_ERR_ARG;
    *info = bwams_recal_apply_info_t{a->last[0], a->last[1], a->model_bytes, a->ms_check, a->ms_apply};
    return BWAMS_OK;
}

}  // extern "C"
