// api_bam_file.hip — C-ABI entry points of a BAM file read back by region (include/bwams.h, "BAM file by region"): the handle, the
// query, the pieces and their fetch, over host/bam_query.h (header, index, plan, the file's members) and bam_query.hip (the records
// of a piece found, selected and copied on the device); bwams_bai_plan, the plan alone.  The consumers reach the current piece
// through consumer_file (rec_consumer.h).  No CPU fallback: the records are found and selected by HIP kernels or the call fails.
#include <memory>

#include "rec_consumer.h"
#include "../host/bam_query.h"

using namespace bwams;

struct bwams_bam_file {
    int device = 0, cu_count = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {};
    BamFileHost host;
    BamQueryScratch *scratch = nullptr;
    DevBuf<uint8_t> buf[2];                          // a piece: the carried bytes, then the inflated members; the next carry goes to the other
    int cur = 0;
    int64_t carry = 0;
    DevBuf<bwams_pileup_region_t> regions;           // rule 2's merged regions
    int32_t n_regions = 0;
    DevBuf<uint8_t> recs;                            // the current piece: the kept records back to back, 16 bytes of slack,
    DevBuf<int64_t> roff;                            // their offsets (n_rec + 1)
    DevBuf<bwams_bam_coord_t> coords;                // and coords
    int64_t n_rec = 0, n_bytes = 0;
    enum State { kNoQuery, kQueried, kPiece, kLast, kConsumed } state = kNoQuery;
    bwams_bam_file_info_t info{};
    ~bwams_bam_file() {
        (void)hipSetDevice(device);
        bam_query_scratch_free(scratch);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
    bool has_piece() const { return state == kPiece || state == kLast; }
};

namespace {

// bwams_inflater_run decodes a member with one wave, so a call takes a member's latency (some 30 ms) whatever it holds: the fewer
// and larger the pieces, the better
constexpr int64_t kDefaultPiece = (int64_t)128 << 20;

const char *no_piece_text(const bwams_bam_file *f) {
    return f->state == bwams_bam_file::kNoQuery   ? "call bwams_bam_file_query first"
           : f->state == bwams_bam_file::kQueried ? "call bwams_bam_file_next first: the query has no current piece yet"
                                                  : "the query's last piece was consumed (bwams_bam_file_query starts another)";
}

int fail(const char *who, int rc, const std::string &why) {
    set_last_error(std::string(who) + ": " + why);
    return rc;
}

}  // namespace

namespace bwams {
int bam_file_piece(bwams_bam_file *f, const char *who, int *device, hipStream_t *stream, DevRecords *out) {
    if (!f->has_piece()) return consumer_refusal(who, no_piece_text(f));
    *device = f->device;
    *stream = f->stream;
    *out = DevRecords{f->recs.p, f->roff.p, f->n_rec};
    return BWAMS_OK;
}
}  // namespace bwams

extern "C" {

int bwams_bam_file_open(const char *path, const char *bai_path, int device, int64_t piece_bytes, bwams_bam_file_t **out) {
    const char *who = "bwams_bam_file_open";
    if (!path || !out || piece_bytes < 0 || (piece_bytes && piece_bytes < 65536) || piece_bytes > ((int64_t)1 << 31))
        return fail(who, BWAMS_ERR_ARG, "a path, out and piece_bytes of 0 or in [65536, 2^31] are required");
    *out = nullptr;
    if (int rc = check_device(device)) return rc;
    BWAMS_HIP(hipSetDevice(device));
    std::unique_ptr<bwams_bam_file> f(new bwams_bam_file());
    f->device = device;
    BWAMS_HIP(hipDeviceGetAttribute(&f->cu_count, hipDeviceAttributeMultiprocessorCount, device));
    BWAMS_HIP(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
    for (hipEvent_t &e : f->ev) BWAMS_HIP(hipEventCreate(&e));
    f->scratch = bam_query_scratch_new();
    std::string err;
    if (int rc = f->host.open(path, bai_path, device, piece_bytes ? piece_bytes : kDefaultPiece, &err)) return fail(who, rc, err);
    // a piece: up to piece_bytes carried (a record larger than that is refused) and piece_bytes inflated, and the gather's slack
    for (DevBuf<uint8_t> &b : f->buf) BWAMS_HIP(b.alloc((size_t)f->host.piece_bytes * 2 + 64));
    *out = f.release();
    return BWAMS_OK;
}

int bwams_bam_file_close(bwams_bam_file_t *f) {
    delete f;
    return BWAMS_OK;
}

int bwams_bam_file_header(const bwams_bam_file_t *f, const char **text, int64_t *n_text, int32_t *n_ref) {
    if (!f) return BWAMS_ERR_ARG;
    if (text) *text = f->host.hdr.text.data();
    if (n_text) *n_text = (int64_t)f->host.hdr.text.size();
    if (n_ref) *n_ref = f->host.hdr.n_ref;
    return BWAMS_OK;
}

int bwams_bam_file_header_block(const bwams_bam_file_t *f, const void **block, int64_t *n) {
    if (!f || !block || !n) return BWAMS_ERR_ARG;
    *block = f->host.header_block.data();
    *n = (int64_t)f->host.header_block.size();
    return BWAMS_OK;
}

int bwams_bam_file_refs(const bwams_bam_file_t *f, int32_t *l_ref, int32_t cap) {
    if (!f || cap < 0 || (cap && !l_ref)) return BWAMS_ERR_ARG;
    if (cap < f->host.hdr.n_ref)
        return fail("bwams_bam_file_refs", BWAMS_ERR_CAPACITY, std::to_string(f->host.hdr.n_ref) + " references do not fit a capacity of " + std::to_string(cap));
    std::copy(f->host.hdr.l_ref.begin(), f->host.hdr.l_ref.end(), l_ref);
    return BWAMS_OK;
}

int bwams_bam_file_query(bwams_bam_file_t *f, const bwams_pileup_region_t *regions, int32_t n_regions) {
    const char *who = "bwams_bam_file_query";
    if (!f) return fail(who, BWAMS_ERR_ARG, "a handle is required");
    std::vector<bwams_pileup_region_t> merged;
    std::string err;
    if (int rc = f->host.query(regions, n_regions, &merged, &err)) return fail(who, rc, err);      // a refused query leaves the last one's state
    BWAMS_HIP(hipSetDevice(f->device));
    f->n_regions = (int32_t)merged.size();
    if (f->n_regions) {
        BWAMS_HIP(hipStreamSynchronize(f->stream));
        BWAMS_HIP(f->regions.ensure_n(merged.size()));
        BWAMS_HIP(hipMemcpyAsync(f->regions.p, merged.data(), merged.size() * sizeof(bwams_pileup_region_t), hipMemcpyHostToDevice, f->stream));
        BWAMS_HIP(hipStreamSynchronize(f->stream));
    }
    f->carry = 0;
    f->n_rec = f->n_bytes = 0;
    f->info = bwams_bam_file_info_t{};
    f->info.intervals = (int64_t)f->host.iv_beg.size();
    f->state = bwams_bam_file::kQueried;
    return BWAMS_OK;
}

int bwams_bam_file_next(bwams_bam_file_t *f, int64_t *n_records, int64_t *n_bytes, int32_t *done) {
    const char *who = "bwams_bam_file_next";
    if (!f) return fail(who, BWAMS_ERR_ARG, "a handle is required");
    if (f->state == bwams_bam_file::kNoQuery) return fail(who, BWAMS_ERR_ARG, no_piece_text(f));
    if (f->state == bwams_bam_file::kLast || f->state == bwams_bam_file::kConsumed) {
        f->state = bwams_bam_file::kConsumed;
        return fail(who, BWAMS_ERR_ARG, no_piece_text(f));
    }
    BWAMS_HIP(hipSetDevice(f->device));
    hipStream_t st = f->stream;
    BWAMS_HIP(hipStreamSynchronize(st));                     // a consumer may still read the piece that this one replaces
    auto broken = [&](int rc, const std::string &why) {      // nothing more comes of this query
        f->state = bwams_bam_file::kConsumed;
        return fail(who, rc, why);
    };
    f->n_rec = f->n_bytes = 0;
    BamQueryResult R{};
    bool last = true;
    if (f->host.exhausted()) {                               // a plan without intervals: one empty piece
        if (int rc = bam_query_piece(f->scratch, f->buf[f->cur].p, 0, 0, 0, nullptr, 0, f->recs, f->roff, f->coords, f->ev, f->cu_count, st, &R))
            return rc;
        f->info.pieces += 1;
    } else {
        BamPiece P;
        std::string err;
        uint8_t *d = f->buf[f->cur].p;
        if (int rc = f->host.next_piece(d + f->carry, &P, &err)) return broken(rc, err);
        const int64_t n = f->carry + P.n_out;
        const int64_t start = P.first ? P.start : 0, stop = P.stop >= 0 ? f->carry + P.stop : n;
        const std::string where = f->host.path + ": piece at file offset " + std::to_string(P.file_off) + ": ";
        if (start > stop) return broken(BWAMS_ERR_IO, where + "the chunk starts behind its end");
        if (int rc = bam_query_piece(f->scratch, d, n, start, stop, f->regions.p, f->n_regions, f->recs, f->roff, f->coords, f->ev, f->cu_count,
                                     st, &R)) {
            f->state = bwams_bam_file::kConsumed;
            return rc;
        }
        const int64_t ordinal = f->info.records_seen + R.n_rec;
        if (R.bad_rec >= 0)
            return broken(BWAMS_ERR_IO, where + "record " + std::to_string(f->info.records_seen + R.bad_rec) + " at byte " +
                                            std::to_string(R.bad_rec_at - f->carry) + " of its inflated bytes: refID < -1 or POS outside [-1, 2^31 - 2]");
        if (R.bad || (R.cut && P.last))
            return broken(BWAMS_ERR_IO, where + "record " + std::to_string(ordinal) + " at byte " + std::to_string(R.at - f->carry) +
                                            " of its inflated bytes is " + (R.bad ? "not a well-formed BAM record (block_size, l_read_name, l_seq, the name's NUL)"
                                                                                  : "cut off by the end of its chunk"));
        const int64_t carry = R.cut ? n - R.at : 0;
        if (carry > f->host.piece_bytes || (R.cut && R.cut_size > f->host.piece_bytes))         // rule 5: as soon as its size is seen
            return broken(BWAMS_ERR_CAPACITY, where + "record " + std::to_string(ordinal) + " of " + std::to_string(R.cut_size) +
                                                  " bytes does not fit piece_bytes " + std::to_string(f->host.piece_bytes));
        if (carry) BWAMS_HIP(hipMemcpyAsync(f->buf[f->cur ^ 1].p, d + R.at, (size_t)carry, hipMemcpyDeviceToDevice, st));
        BWAMS_HIP(hipStreamSynchronize(st));
        f->cur ^= 1;
        f->carry = carry;
        last = f->host.exhausted();
        f->info.members += P.members; f->info.compressed_bytes += P.n_in; f->info.inflated_bytes += P.n_out;
        f->info.candidates += R.n_cand; f->info.records_seen += R.n_rec; f->info.records_kept += R.n_kept;
        f->info.pieces += 1; f->info.carried += carry;
        f->info.ms_read += P.ms_read; f->info.ms_inflate += P.ms_inflate;
        f->info.ms_discover += R.ms_discover; f->info.ms_select += R.ms_select; f->info.ms_gather += R.ms_gather;
    }
    f->n_rec = R.n_kept;
    f->n_bytes = R.kept_bytes;
    f->state = last ? bwams_bam_file::kLast : bwams_bam_file::kPiece;
    if (n_records) *n_records = f->n_rec;
    if (n_bytes) *n_bytes = f->n_bytes;
    if (done) *done = last ? 1 : 0;
    return BWAMS_OK;
}

int bwams_bam_file_fetch(bwams_bam_file_t *f, void *bam, int64_t cap, bwams_bam_coord_t *coords) {
    const char *who = "bwams_bam_file_fetch";
    if (!f) return fail(who, BWAMS_ERR_ARG, "a handle is required");
    if (!f->has_piece()) return fail(who, BWAMS_ERR_ARG, no_piece_text(f));
    if (cap < f->n_bytes || (f->n_bytes && !bam))
        return fail(who, BWAMS_ERR_CAPACITY, std::to_string(f->n_bytes) + " bytes of records do not fit a capacity of " + std::to_string(cap));
    BWAMS_HIP(hipSetDevice(f->device));
    if (f->n_bytes) BWAMS_HIP(hipMemcpyAsync(bam, f->recs.p, (size_t)f->n_bytes, hipMemcpyDeviceToHost, f->stream));
    if (coords && f->n_rec) BWAMS_HIP(hipMemcpyAsync(coords, f->coords.p, (size_t)f->n_rec * sizeof(bwams_bam_coord_t), hipMemcpyDeviceToHost, f->stream));
    BWAMS_HIP(hipStreamSynchronize(f->stream));
    return BWAMS_OK;
}

int bwams_bam_file_info(const bwams_bam_file_t *f, bwams_bam_file_info_t *info) {
    if (!f || !info) return BWAMS_ERR_ARG;
    *info = f->info;
    return BWAMS_OK;
}

int bwams_bai_plan(const void *bai, int64_t n_bai, const bwams_pileup_region_t *regions, int32_t n_regions, uint64_t *chunk_beg,
                   uint64_t *chunk_end, int64_t cap, int64_t *n_chunks) {
    const char *who = "bwams_bai_plan";
    Bai index;
    std::string err;
    if (int rc = bai_parse(bai, n_bai, &index, &err)) return fail(who, rc, err);
    std::vector<bwams_pileup_region_t> merged;
    if (int rc = regions_merge(regions, n_regions, (int32_t)std::min<size_t>(index.refs.size(), 0x7FFFFFFF), &merged, &err)) return fail(who, rc, err);
    std::vector<uint64_t> b, e;
    bai_plan(index, merged, &b, &e);
    if (n_chunks) *n_chunks = (int64_t)b.size();
    if (cap < (int64_t)b.size() || (!b.empty() && (!chunk_beg || !chunk_end)))
        return fail(who, BWAMS_ERR_CAPACITY, std::to_string(b.size()) + " intervals do not fit a capacity of " + std::to_string(cap));
    std::copy(b.begin(), b.end(), chunk_beg);
    std::copy(e.begin(), e.end(), chunk_end);
    return BWAMS_OK;
}

}  // extern "C"
