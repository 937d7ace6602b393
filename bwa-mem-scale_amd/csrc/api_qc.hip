// api_qc.hip — C-ABI entry points of the alignment QC (include/bwams.h, "Alignment QC"): the handle, the adds from a batch and from
// host records, and the queries, over qc.hip; the texts over host/qc_text.cpp.
// No CPU fallback: every entry point runs HIP kernels or returns an error.
#include <algorithm>
#include <cstring>
#include <memory>

#include "rec_consumer.h"
#include "../host/qc_host.h"

using namespace bwams;

struct bwams_qc : RecConsumer {
    bwams_qc_opt_t opt{};
    QcLayout lay{};
    DevBuf<unsigned long long> counters;             // lay.words() of them (rule 6)
    DevBuf<unsigned long long> call;                 // [0] rule 1's first bad record, then kQcCallWords words of a piece
    DevBuf<uint32_t> lists;                          // the filtered-in records of a piece, a list per class
    int64_t last[3] = {0, 0, 0};                     // of the last add: records given, records counted, bases past max_cycle
    float ms_check = 0, ms_add = 0;                  // ... and its device time
};

namespace bwams {
int qc_device(const bwams_qc *q) { return q->device; }
}  // namespace bwams

namespace {

constexpr int64_t kPiece = 1 << 24;                  // records listed at a time: 8 bytes of scratch per record

// check first, then add (rule 1)
int qc_add(bwams_qc *q, const DevRecords &R, int64_t *n_counted, const char *who) {
    const int64_t n_rec = R.n_rec;
    if (n_rec > 0x7FFFFFFFLL) {
        set_last_error(std::string(who) + ": more than 2^31 - 1 records in one call");
        return BWAMS_ERR_UNSUPPORTED;
    }
    hipStream_t st = q->stream;
    int64_t counted = 0, over = 0;
    q->ms_check = q->ms_add = 0;
    if (n_rec > 0) {
        unsigned long long h[kQcCallWords];
        if (int rc = consumer_check(q, q->call.p, 1, h, &q->ms_check,
                                    [&] { launch_qc_check(R.bam, R.off, n_rec, q->opt.exclude, q->call.p, q->cu_count, st); })) return rc;
        if (h[0] != ~0ULL) {
            static const char *const why[4] = {" has a negative l_seq or a CIGAR that ends behind the record (bounds)",
                                               " has a CIGAR op code above 8 (op)", " ends inside its SEQ or QUAL (bounds)",
                                               " has an aux area that cannot be walked (aux)"};
            return consumer_refuse_packed(who, h[0], why);
        }
        BWAMS_HIP(q->lists.ensure_n((size_t)(2 * std::min(kPiece, n_rec))));     // before the first counter moves
        const int lanes = knobs().qc_lanes != 0;
        for (int64_t r0 = 0; r0 < n_rec; r0 += kPiece) {
            const int64_t n = std::min(kPiece, n_rec - r0);
            unsigned long long *call = q->call.p + 1;
            if (int rc = consumer_piece(q, call, kQcCallWords, h, &q->ms_add, [&] {
                    launch_qc_records(R.bam, R.off + r0, n, q->lay, q->counters.p, q->lists.p, call, q->cu_count, st);
                    launch_qc_cycles(R.bam, R.off + r0, n, q->lay, q->counters.p, q->lists.p, call, lanes, q->cu_count, st);
                    return BWAMS_OK;
                })) return rc;
            counted += (int64_t)h[kQcCallCounted];
            over += (int64_t)h[kQcCallOver];
        }
    }
    q->last[0] = n_rec; q->last[1] = counted; q->last[2] = over;
    if (n_counted) *n_counted = counted;
    return BWAMS_OK;
}

// the whole counter block on the host
int qc_fetch(bwams_qc *q, std::vector<int64_t> *host) {
    host->resize((size_t)q->lay.words());
    BWAMS_HIP(hipSetDevice(q->device));
    BWAMS_HIP(hipMemcpyAsync(host->data(), q->counters.p, host->size() * 8, hipMemcpyDeviceToHost, q->stream));
    BWAMS_HIP(hipStreamSynchronize(q->stream));
    return BWAMS_OK;
}

// where table `what` starts in the block, and its number of values
bool qc_table_at(const QcLayout &L, int32_t what, int64_t *at, int64_t *n) {
    const int64_t start[7] = {L.rl(), L.qual(), L.base(), L.mapq(), L.isize(), L.indel(), L.words()};
    if (what < 0 || what > 5) return false;
    *at = start[what];
    *n = start[what + 1] - start[what];
    return true;
}

}  // namespace

extern "C" {

int bwams_qc_open(int device, const bwams_qc_opt_t *opt, bwams_qc_t **out) {
    if (!out || (opt && (opt->exclude > 0xFFFFu || opt->reserved != 0 || opt->max_cycle < 64 || opt->max_cycle > 4096 || opt->max_cycle % 64 ||
                         opt->max_isize < 1 || opt->max_isize > (1 << 20)))) {
        set_last_error("bwams_qc_open: exclude within 16 bits, max_cycle a multiple of 64 in [64, 4096], max_isize in [1, 2^20] and "
                       "reserved == 0 are required");
        return BWAMS_ERR_ARG;
    }
    *out = nullptr;
    std::unique_ptr<bwams_qc> q(new bwams_qc());
    if (int rc = q->open(device)) return rc;
    q->opt = opt ? *opt : bwams_qc_opt_t{0x900, 512, 8000, 0};
    q->lay = QcLayout{q->opt.max_cycle, q->opt.max_isize, q->opt.exclude};
    BWAMS_HIP(q->counters.alloc((size_t)q->lay.words() * 8));
    BWAMS_HIP(q->call.alloc((1 + kQcCallWords) * 8));
    BWAMS_HIP(hipMemsetAsync(q->counters.p, 0, (size_t)q->lay.words() * 8, q->stream));
    BWAMS_HIP(hipStreamSynchronize(q->stream));
    *out = q.release();
    return BWAMS_OK;
}

int bwams_qc_close(bwams_qc_t *q) {
    delete q;
    return BWAMS_OK;
}

int bwams_qc_reset(bwams_qc_t *q) {
    if (!q) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(q->device));
    BWAMS_HIP(hipMemsetAsync(q->counters.p, 0, (size_t)q->lay.words() * 8, q->stream));
    BWAMS_HIP(hipStreamSynchronize(q->stream));
    std::fill(q->last, q->last + 3, 0);
    return BWAMS_OK;
}

int bwams_qc_add_batch(bwams_qc_t *q, bwams_batch_t *b, int64_t *n_counted) {
    DevRecords R;
    if (int rc = consumer_batch(q, b, "bwams_qc_add_batch", &R)) return rc;
    return qc_add(q, R, n_counted, "bwams_qc_add_batch");
}

int bwams_qc_add_records(bwams_qc_t *q, const void *bam, int64_t n_bytes, int64_t *n_counted) {
    DevRecords R;
    if (int rc = consumer_records(q, bam, n_bytes, "bwams_qc_add_records", &R)) return rc;
    return qc_add(q, R, n_counted, "bwams_qc_add_records");
}

int bwams_qc_add_file(bwams_qc_t *q, bwams_bam_file_t *f, int64_t *n_counted) {
    DevRecords R;
    if (int rc = consumer_file(q, f, "bwams_qc_add_file", &R)) return rc;
    return qc_add(q, R, n_counted, "bwams_qc_add_file");
}

int bwams_qc_summary(bwams_qc_t *q, bwams_qc_summary_t *out) {
    if (!q || !out) return BWAMS_ERR_ARG;
    static_assert(sizeof(bwams_qc_summary_t) == 48 * 8, "the summary is the head of the counter block");
    BWAMS_HIP(hipSetDevice(q->device));
    BWAMS_HIP(hipMemcpyAsync(out, q->counters.p, sizeof *out, hipMemcpyDeviceToHost, q->stream));
    BWAMS_HIP(hipStreamSynchronize(q->stream));
    return BWAMS_OK;
}

int bwams_qc_table(bwams_qc_t *q, int32_t what, int64_t *out, int64_t cap, int64_t *n) {
    int64_t at = 0, len = 0;
    if (!q || cap < 0 || !qc_table_at(q->lay, what, &at, &len)) {
        set_last_error("bwams_qc_table: a handle, a table of BWAMS_QC_TABLE_* and cap >= 0 are required");
        return BWAMS_ERR_ARG;
    }
    if (n) *n = len;
    if (!out) return BWAMS_OK;
    if (cap < len) {
        set_last_error("bwams_qc_table: " + std::to_string(len) + " values do not fit a capacity of " + std::to_string(cap));
        return BWAMS_ERR_CAPACITY;
    }
    BWAMS_HIP(hipSetDevice(q->device));
    BWAMS_HIP(hipMemcpyAsync(out, q->counters.p + at, (size_t)len * 8, hipMemcpyDeviceToHost, q->stream));
    BWAMS_HIP(hipStreamSynchronize(q->stream));
    return BWAMS_OK;
}

int bwams_qc_text(bwams_qc_t *q, int32_t what, char *out, int64_t cap, int64_t *n) {
    if (!q || (what != BWAMS_QC_TEXT_FLAGSTAT && what != BWAMS_QC_TEXT_STATS)) {
        set_last_error("bwams_qc_text: a handle and a text of BWAMS_QC_TEXT_* are required");
        return BWAMS_ERR_ARG;
    }
    std::vector<int64_t> host;
    if (int rc = qc_fetch(q, &host)) return rc;
    QcTables t;
    t.opt = q->opt;
    memcpy(&t.sum, host.data(), sizeof t.sum);
    for (int32_t k = 0; k < 6; ++k) {
        int64_t at = 0, len = 0;
        qc_table_at(q->lay, k, &at, &len);
        t.table[k] = host.data() + at;
    }
    std::string text;
    if (int rc = qc_text_format(t, what, &text)) return rc;
    if (n) *n = (int64_t)text.size();
    if (!out || cap < (int64_t)text.size()) {
        set_last_error("bwams_qc_text: the text needs " + std::to_string(text.size()) + " bytes");
        return BWAMS_ERR_CAPACITY;
    }
    memcpy(out, text.data(), text.size());
    return BWAMS_OK;
}

int bwams_qc_info(const bwams_qc_t *q, bwams_qc_info_t *info) {
    if (!q || !info) return BWAMS_ERR_ARG;
    *info = bwams_qc_info_t{kQcIsizeLds, kQcSlice, q->last[0], q->last[1], q->last[2], q->ms_check, q->ms_add};
    return BWAMS_OK;
}

}  // extern "C"
