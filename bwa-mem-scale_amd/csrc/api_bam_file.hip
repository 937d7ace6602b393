// api_bam_file.hip — C-ABI entry points of a BAM file read back by region (include/bwams.h, "BAM file by region"): the handle, the
// query, the pieces and their fetch, over host/bam_query.h (header, index, plan, the file's members) and bam_query.hip (the records
// of a piece found, selected and copied on the device); bwams_bai_plan, the plan alone.  The consumers reach the current piece
// through consumer_file (rec_consumer.h).  No CPU fallback: the records are found and selected by HIP kernels or the call fails.
// A handle of bwams_bam_file_open_merge is the same struct with a merge part: it owns a plain handle per file and its pieces are
// rounds of bam_merge.hip's kernels over the children's current pieces (rules M1 to M9); bwams_bam_header_merge, the header alone.
#include <chrono>
#include <cstring>
#include <memory>
#include <thread>

#include "rec_consumer.h"
#include "../host/bam_query.h"

using namespace bwams;

struct bwams_bam_file;

// The merge part of a handle that bwams_bam_file_open_merge made (rules M1 to M9): the children it owns, a cursor per child into the
// child's current piece, and what a round's kernels need.  The merged piece itself goes to the handle's own recs / roff / coords.
struct BamMerge {
    std::vector<bwams_bam_file *> kids;
    std::vector<std::string> names;                  // "file k (path): "
    int64_t child_bytes = 0;
    std::vector<int64_t> cur, seen;                  // of child j: its window starts at record cur[j] of its piece; records of the pieces before
    std::vector<int32_t> parity;
    HostBuf<BmChild> h_kids;
    HostBuf<BmPlan> h_plan;
    DevBuf<BmChild> d_kids;
    DevBuf<BmPlan> d_plan;
    DevBuf<uint64_t> last_key;                       // two words per child (bm_check_kernel)
    DevBuf<const uint8_t *> src;                     // of each record of the piece
    DevBuf<int64_t> size;
    DevBuf<> tmp;                                    // the scan's
    hipEvent_t ev[7] = {};                           // check, frontier | rank, scan, gather: the host reads the plan in between
    bwams_bam_merge_info_t info{};
    ~BamMerge();
};

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
    std::unique_ptr<BamMerge> merge;                 // null: a plain handle
    ~bwams_bam_file() {
        merge.reset();                               // the children first: each makes its own device current
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

// ---- several files merged (rules M1 to M9) ----

constexpr int kRefillThreads = 16;       // children advanced at a time

// the text a child's call left, without the entry point's name in front of it
std::string child_text(const char *entry) {
    std::string t = bwams_last_error();
    const std::string head = std::string(entry) + ": ";
    return t.compare(0, head.size(), head) == 0 ? t.substr(head.size()) : t;
}

// a HIP call's result as a return code, with the call's name and HIP's text as the last error (what BWAMS_HIP does, without its return)
int hip_rc(hipError_t e, const char *what) {
    if (e == hipSuccess) return BWAMS_OK;
    set_last_error(std::string(what) + " -> " + hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? BWAMS_ERR_NOMEM : BWAMS_ERR_DEVICE;
}

bool kid_open(const bwams_bam_file *k) { return k->state == bwams_bam_file::kQueried || k->state == bwams_bam_file::kPiece; }
int64_t kid_window(const BamMerge *m, size_t j) { return m->kids[j]->has_piece() ? m->kids[j]->n_rec - m->cur[j] : 0; }

int merge_query(bwams_bam_file *f, const bwams_pileup_region_t *regions, int32_t n_regions) {
    const char *who = "bwams_bam_file_query";
    BamMerge *m = f->merge.get();
    if (n_regions > 0)
        for (size_t k = 0; k < m->kids.size(); ++k)
            if (!m->kids[k]->host.has_index) return fail(who, BWAMS_ERR_ARG, m->names[k] + "a query with regions needs an index, and this file has none");
    // Child 0 checks the regions for all (M2: one reference list), so a refusal by it leaves the last query's state as the plain
    // handle's does.  From the first child that took the query on, the last query is gone: whatever fails then leaves no query.
    auto no_query = [&](int rc) {
        f->n_rec = f->n_bytes = 0;
        f->state = bwams_bam_file::kNoQuery;
        return rc;
    };
    for (size_t k = 0; k < m->kids.size(); ++k)
        if (int rc = bwams_bam_file_query(m->kids[k], regions, n_regions)) {
            fail(who, rc, m->names[k] + child_text(who));
            return k ? no_query(rc) : rc;
        }
    if (int rc = hip_rc(hipSetDevice(f->device), "hipSetDevice")) return no_query(rc);
    if (int rc = hip_rc(hipStreamSynchronize(f->stream), "hipStreamSynchronize")) return no_query(rc);
    if (int rc = hip_rc(hipMemsetAsync(m->last_key.p, 0, m->last_key.cap, f->stream), "hipMemsetAsync")) return no_query(rc);
    if (int rc = hip_rc(hipStreamSynchronize(f->stream), "hipStreamSynchronize")) return no_query(rc);
    std::fill(m->cur.begin(), m->cur.end(), 0);
    std::fill(m->seen.begin(), m->seen.end(), 0);
    std::fill(m->parity.begin(), m->parity.end(), 0);
    const bwams_bam_merge_info_t was = m->info;
    m->info = bwams_bam_merge_info_t{};
    m->info.n_files = was.n_files; m->info.child_bytes = was.child_bytes; m->info.pg_dropped = was.pg_dropped;
    f->n_rec = f->n_bytes = 0;
    f->state = bwams_bam_file::kQueried;
    return BWAMS_OK;
}

// Rule M7's advance: every open child whose window is empty gets its next piece, again while pieces come back empty.  A thread per
// child, kRefillThreads at a time; each child has its own stream, inflater and scratch, and what a child returns depends on that
// child alone, so the threads decide nothing (rule M8).  refilled[j]: child j has a new piece.
int merge_refill(bwams_bam_file *f, std::vector<char> *refilled, std::string *why) {
    BamMerge *m = f->merge.get();
    const size_t K = m->kids.size();
    std::vector<size_t> need;
    for (size_t j = 0; j < K; ++j)
        if (kid_open(m->kids[j]) && kid_window(m, j) == 0) need.push_back(j);
    if (need.empty()) return BWAMS_OK;
    std::vector<int> rc(K, BWAMS_OK);
    std::vector<int64_t> calls(K, 0);
    std::vector<std::string> text(K);
    auto advance = [&](size_t j) {
        bwams_bam_file *k = m->kids[j];
        do {
            if (k->has_piece()) m->seen[j] += k->n_rec;
            rc[j] = bwams_bam_file_next(k, nullptr, nullptr, nullptr);
            if (rc[j]) { text[j] = child_text("bwams_bam_file_next"); return; }
            calls[j] += 1;
        } while (k->n_rec == 0 && kid_open(k));
        m->cur[j] = 0;
    };
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t at = 0; at < need.size(); at += kRefillThreads) {
        const size_t end = std::min(need.size(), at + (size_t)kRefillThreads);
        if (end - at == 1) { advance(need[at]); continue; }
        std::vector<std::thread> pool;
        for (size_t i = at; i < end; ++i) pool.emplace_back(advance, need[i]);
        for (std::thread &t : pool) t.join();
    }
    m->info.ms_refill += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (size_t j : need) {
        m->info.refills += calls[j];
        (*refilled)[j] = 1;
    }
    for (size_t j : need)
        if (rc[j]) { *why = m->names[j] + text[j]; return rc[j]; }
    return BWAMS_OK;
}

// One round (rule M7): the next piece of the merged stream into f->recs / roff / coords.  *last: it is the query's last.
int merge_round(bwams_bam_file *f, const char *who, bool *last) {
    BamMerge *m = f->merge.get();
    const size_t K = m->kids.size();
    hipStream_t st = f->stream;
    auto broken = [&](int rc, const std::string &why) {
        f->state = bwams_bam_file::kConsumed;
        return why.empty() ? rc : fail(who, rc, why);
    };
    std::vector<char> refilled(K, 0);
    std::string why;
    if (int rc = merge_refill(f, &refilled, &why)) return broken(rc, why);
    auto failed = [&](int rc) { f->state = bwams_bam_file::kConsumed; return rc; };      // the text is set already
#define BM_HIP(call) do { if (int rc_ = hip_rc(call, #call)) return failed(rc_); } while (0)
    BM_HIP(hipSetDevice(f->device));                         // a child's call on this thread may have left another device current
    bool any_open = false;
    int64_t max_new = 0, room = 0;
    for (size_t j = 0; j < K; ++j) {
        bwams_bam_file *k = m->kids[j];
        const bool fresh_piece = refilled[j] && k->n_rec > 0;
        if (fresh_piece) m->parity[j] ^= 1;
        BmChild &c = m->h_kids.p[j];
        c = BmChild{k->coords.p, k->recs.p, k->roff.p, m->cur[j], k->has_piece() ? k->n_rec : 0, m->seen[j], kid_open(k) ? 1 : 0,
                    fresh_piece ? 1 : 0, m->parity[j], 0};
        any_open |= kid_open(k);
        if (fresh_piece) max_new = std::max(max_new, k->n_rec);
        if (k->has_piece()) room += k->n_bytes;
    }
    BM_HIP(hipMemcpyAsync(m->d_kids.p, m->h_kids.p, K * sizeof(BmChild), hipMemcpyHostToDevice, st));
    BM_HIP(hipMemsetAsync(m->d_plan.p, 0xFF, sizeof(BmPlan), st));
    BM_HIP(hipEventRecord(m->ev[0], st));
    launch_bm_check(m->d_kids.p, (int)K, max_new, m->last_key.p, m->d_plan.p, f->cu_count, st);
    BM_HIP(hipEventRecord(m->ev[1], st));
    launch_bm_frontier(m->d_kids.p, (int)K, m->d_plan.p, st);
    BM_HIP(hipEventRecord(m->ev[2], st));
    BM_HIP(hipMemcpyAsync(m->h_plan.p, m->d_plan.p, sizeof(BmPlan), hipMemcpyDeviceToHost, st));
    BM_HIP(hipStreamSynchronize(st));
    BM_HIP(hipGetLastError());
    const BmPlan &P = *m->h_plan.p;
    for (size_t j = 0; j < K; ++j)
        if (P.bad[j] != ~0ULL)                               // rule M5
            return broken(BWAMS_ERR_IO, m->names[j] + "record " + std::to_string(P.bad[j]) + ": key below its predecessor's");
    const int64_t total = P.total;
    if (total < 0 || total >= ((int64_t)1 << 32)) return broken(BWAMS_ERR_UNSUPPORTED, "a merged piece of 2^32 records or more");
    const size_t n1 = (size_t)total + 1;
    if (int rc = fresh(m->src, n1, who, "a merged piece's source addresses")) return failed(rc);
    if (int rc = fresh(m->size, n1, who, "a merged piece's record sizes")) return failed(rc);
    if (int rc = fresh(f->roff, n1, who, "a merged piece's offsets")) return failed(rc);
    if (int rc = fresh(f->coords, n1, who, "a merged piece's coords")) return failed(rc);
    if (int rc = fresh(f->recs, (size_t)room + 16, who, "a merged piece's records")) return failed(rc);
    int64_t n_bytes = 0;
    if (total > 0) {
        BM_HIP(hipEventRecord(m->ev[3], st));                // behind the plan's round trip and the allocations: the rank alone
        launch_bm_rank(m->d_kids.p, (int)K, m->d_plan.p, total, m->src.p, m->size.p, f->coords.p, st);
        BM_HIP(hipEventRecord(m->ev[4], st));
        if (int rc = with_tmp(m->tmp, st, "bwams_bam_file_next: exclusive_scan", [&](void *tmp, size_t &tb) {
                return bm_scan(tmp, tb, m->size.p, f->roff.p, (int64_t)n1, st);
            })) return failed(rc);
        BM_HIP(hipEventRecord(m->ev[5], st));
        launch_bm_gather(m->src.p, f->roff.p, total, f->recs.p, f->cu_count, st);
        BM_HIP(hipEventRecord(m->ev[6], st));
        BM_HIP(hipMemcpyAsync(&n_bytes, f->roff.p + total, 8, hipMemcpyDeviceToHost, st));
    } else {
        BM_HIP(hipMemsetAsync(f->roff.p, 0, 8, st));
    }
    BM_HIP(hipStreamSynchronize(st));
    BM_HIP(hipGetLastError());
#undef BM_HIP
    if (n_bytes < 0 || n_bytes > room) return broken(BWAMS_ERR_DEVICE, "a merged piece's size does not add up to its children's");
    float t = 0;
    bwams_bam_merge_info_t &I = m->info;
    if (hipEventElapsedTime(&t, m->ev[0], m->ev[1]) == hipSuccess) I.ms_check += t;
    if (hipEventElapsedTime(&t, m->ev[1], m->ev[2]) == hipSuccess) I.ms_frontier += t;
    if (total > 0) {
        if (hipEventElapsedTime(&t, m->ev[3], m->ev[4]) == hipSuccess) I.ms_rank += t;
        if (hipEventElapsedTime(&t, m->ev[4], m->ev[5]) == hipSuccess) I.ms_scan += t;
        if (hipEventElapsedTime(&t, m->ev[5], m->ev[6]) == hipSuccess) I.ms_gather += t;
    }
    for (size_t j = 0; j < K; ++j) {
        m->cur[j] += P.count[j];
        I.max_window_left = std::max(I.max_window_left, kid_window(m, j));
    }
    I.rounds += 1; I.records += total; I.bytes += n_bytes;
    I.max_piece_records = std::max(I.max_piece_records, total);
    I.max_piece_bytes = std::max(I.max_piece_bytes, n_bytes);
    f->n_rec = total;
    f->n_bytes = n_bytes;
    *last = !any_open;
    return BWAMS_OK;
}

}  // namespace

BamMerge::~BamMerge() {
    for (bwams_bam_file *k : kids) delete k;
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
}

namespace {

void sum_info(const BamMerge *m, bwams_bam_file_info_t *out) {
    *out = bwams_bam_file_info_t{};
    for (const bwams_bam_file *k : m->kids) {
        const bwams_bam_file_info_t &i = k->info;
        out->intervals += i.intervals; out->members += i.members; out->compressed_bytes += i.compressed_bytes;
        out->inflated_bytes += i.inflated_bytes; out->candidates += i.candidates; out->records_seen += i.records_seen;
        out->records_kept += i.records_kept; out->pieces += i.pieces; out->carried += i.carried;
        out->ms_read += i.ms_read; out->ms_inflate += i.ms_inflate; out->ms_discover += i.ms_discover;
        out->ms_select += i.ms_select; out->ms_gather += i.ms_gather;
    }
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

int bwams_bam_file_open_merge(const char *const *paths, const char *const *bai_paths, int32_t n_files, int device, int64_t piece_bytes,
                              const bwams_bam_merge_opt_t *opt, bwams_bam_file_t **out) {
    const char *who = "bwams_bam_file_open_merge";
    if (!paths || !out || n_files < 1 || n_files > kBmMaxFiles || piece_bytes < 0)
        return fail(who, BWAMS_ERR_ARG, "paths, out, n_files in [1, 64] and piece_bytes of 0 or more are required");
    *out = nullptr;
    for (int32_t k = 0; k < n_files; ++k)
        if (!paths[k]) return fail(who, BWAMS_ERR_ARG, "file " + std::to_string(k) + " has no path");
    if (opt && (opt->reserved != 0 || opt->child_bytes < 0)) return fail(who, BWAMS_ERR_ARG, "opt->reserved must be 0 and opt->child_bytes 0 or more");
    const int64_t child_bytes = opt && opt->child_bytes ? opt->child_bytes : ((piece_bytes ? piece_bytes : kDefaultPiece) / n_files) & ~(int64_t)0xFFFF;
    if (child_bytes < 65536)
        return fail(who, BWAMS_ERR_ARG, "a child piece of " + std::to_string(child_bytes) + " bytes is below 65536: " + std::to_string(n_files) +
                                            " files need piece_bytes of at least " + std::to_string((int64_t)65536 * n_files));
    if (int rc = check_device(device)) return rc;
    BWAMS_HIP(hipSetDevice(device));
    std::unique_ptr<bwams_bam_file> f(new bwams_bam_file());
    f->device = device;
    BWAMS_HIP(hipDeviceGetAttribute(&f->cu_count, hipDeviceAttributeMultiprocessorCount, device));
    BWAMS_HIP(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
    for (hipEvent_t &e : f->ev) BWAMS_HIP(hipEventCreate(&e));
    f->merge.reset(new BamMerge());
    BamMerge *m = f->merge.get();
    for (hipEvent_t &e : m->ev) BWAMS_HIP(hipEventCreate(&e));
    m->child_bytes = child_bytes;
    for (int32_t k = 0; k < n_files; ++k) {
        const std::string name = "file " + std::to_string(k) + " (" + paths[k] + "): ";
        bwams_bam_file_t *kid = nullptr;
        if (int rc = bwams_bam_file_open(paths[k], bai_paths ? bai_paths[k] : nullptr, device, child_bytes, &kid))
            return fail(who, rc, name + child_text("bwams_bam_file_open"));
        m->kids.push_back(kid);
        m->names.push_back(name);
    }
    std::vector<const void *> blocks;
    std::vector<int64_t> sizes;
    for (const bwams_bam_file *k : m->kids) {
        blocks.push_back(k->host.header_block.data());
        sizes.push_back((int64_t)k->host.header_block.size());
    }
    std::string block, err;
    if (int rc = bam_header_merge(blocks.data(), sizes.data(), n_files, &block, &m->info.pg_dropped, &err)) return fail(who, rc, err);
    int32_t l_text = 0;
    memcpy(&l_text, block.data() + 4, 4);
    f->host.path = "the merge of " + std::to_string(n_files) + " files";
    f->host.header_block.assign(block.begin(), block.end());
    f->host.hdr.text.assign(block, 8, (size_t)l_text);
    f->host.hdr.n_ref = m->kids[0]->host.hdr.n_ref;
    f->host.hdr.l_ref = m->kids[0]->host.hdr.l_ref;
    m->info.n_files = n_files;
    m->info.child_bytes = child_bytes;
    m->cur.assign((size_t)n_files, 0); m->seen.assign((size_t)n_files, 0); m->parity.assign((size_t)n_files, 0);
    BWAMS_HIP(hipSetDevice(device));
    BWAMS_HIP(m->h_kids.alloc(kBmMaxFiles * sizeof(BmChild))); BWAMS_HIP(m->h_plan.alloc(sizeof(BmPlan)));
    BWAMS_HIP(m->d_kids.alloc(kBmMaxFiles * sizeof(BmChild))); BWAMS_HIP(m->d_plan.alloc(sizeof(BmPlan)));
    BWAMS_HIP(m->last_key.alloc(2 * kBmMaxFiles * sizeof(uint64_t)));
    BWAMS_HIP(f->roff.ensure_n(1)); BWAMS_HIP(f->recs.ensure_n(16));
    *out = f.release();
    return BWAMS_OK;
}

int bwams_bam_merge_info(const bwams_bam_file_t *f, bwams_bam_merge_info_t *info) {
    if (!f || !info) return BWAMS_ERR_ARG;
    if (!f->merge) return fail("bwams_bam_merge_info", BWAMS_ERR_ARG, "the handle is a plain one: bwams_bam_file_open_merge makes a merged one");
    *info = f->merge->info;
    return BWAMS_OK;
}

int bwams_bam_header_merge(const void *const *blocks, const int64_t *n_block, int32_t n_files, void *out, int64_t cap, int64_t *n_out,
                           int32_t *pg_dropped) {
    const char *who = "bwams_bam_header_merge";
    std::string block, err;
    if (int rc = bam_header_merge(blocks, n_block, n_files, &block, pg_dropped, &err)) return fail(who, rc, err);
    if (n_out) *n_out = (int64_t)block.size();
    if (cap < (int64_t)block.size() || !out)
        return fail(who, BWAMS_ERR_CAPACITY, std::to_string(block.size()) + " bytes of header do not fit a capacity of " + std::to_string(cap));
    memcpy(out, block.data(), block.size());
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
    if (f->merge) return merge_query(f, regions, n_regions);
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
    if (f->merge) {                                          // a round over the children's windows (rule M7)
        bool last = false;
        if (int rc = merge_round(f, who, &last)) return rc;
        f->state = last ? bwams_bam_file::kLast : bwams_bam_file::kPiece;
        if (n_records) *n_records = f->n_rec;
        if (n_bytes) *n_bytes = f->n_bytes;
        if (done) *done = last ? 1 : 0;
        return BWAMS_OK;
    }
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
    if (f->merge) sum_info(f->merge.get(), info);
    else *info = f->info;
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
