// api_dup_join.hip — C-ABI entry points of duplicate marking over records that are not query-grouped (include/bwams.h, "Duplicate
// marking, templates joined by name"): the handle, pass 1's adds from host records and from a BAM file's pieces, the finish (join,
// md_decide, counts), the fetch, and pass 2's applies, over dup_join.hip and markdup.hip; bwams_dupjoin_key, rule J1 on the host.
// No CPU fallback: every entry point but _key runs HIP kernels or returns an error.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>

#include "rec_consumer.h"
#include "markdup_dev.h"
#include "../host/dup_groups.h"

using namespace bwams;

struct bwams_dupjoin : RecConsumer {
    bool has_groups = false;
    bwams_dup_groups groups;                         // a copy: the caller's table may go
    DevBuf<uint8_t> g_ids;
    DevBuf<int64_t> g_off;
    DevBuf<int32_t> g_ord, g_lib;
    MdGroupsDev G{};
    int64_t d = 0, max_set = 0;                      // rule 12's options
    enum State { kEmpty, kAdding, kFinished, kRefused } state = kEmpty;
    DjEntries E;                                     // pass 1: an entry per record, freed at the end of _finish
    int64_t cap = 0, n_rec = 0;                      // entries there is room for, entries held
    struct Add { int64_t base, n; unsigned long long sum, wsum; };
    std::vector<Add> adds;                           // J8: what each add left
    size_t applied = 0;                              // applies done
    DjScratch S;
    DjJoined J;
    MdDecide decide;
    DevBuf<uint8_t> dup, optical;
    DevBuf<unsigned long long> call, lib_counts;
    bwams_dup_stats_t stats{};
    std::vector<bwams_dup_lib_stats_t> rows;
    float ms_add = 0, ms_sort = 0, ms_ends = 0, ms_decide = 0, ms_apply = 0;
};

namespace {

int refuse_state(const char *who, const bwams_dupjoin *j, bool want_finished) {
    const char *why = j->state == bwams_dupjoin::kRefused ? "bwams_dupjoin_finish refused the records: only bwams_dupjoin_reset and _close remain"
                      : want_finished                     ? "call bwams_dupjoin_finish first"
                                                          : "the handle is finished: bwams_dupjoin_reset starts another round";
    return consumer_refusal(who, why);
}

// room for n entries, what is held kept; grown by half at least
template <class T> int grow_keep(DevBuf<T> &b, int64_t have, int64_t n, hipStream_t st) {
    DevBuf<T> nb;
    const hipError_t e = nb.alloc((size_t)n * sizeof(T));
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        set_last_error("bwams_dupjoin_add: " + std::to_string((size_t)n * sizeof(T)) + " bytes of device memory for " + std::to_string(n) +
                       " entries could not be had");
        return BWAMS_ERR_NOMEM;
    }
    BWAMS_HIP(e);
    if (have) BWAMS_HIP(hipMemcpyAsync(nb.p, b.p, (size_t)have * sizeof(T), hipMemcpyDeviceToDevice, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    b = std::move(nb);
    return BWAMS_OK;
}

int reserve(bwams_dupjoin *j, int64_t n) {
    if (n <= j->cap) return BWAMS_OK;
    const int64_t to = std::max(n, j->cap + j->cap / 2 + 4096);
    hipStream_t st = j->stream;
    if (int rc = grow_keep(j->E.k0, j->n_rec, to, st)) return rc;
    if (int rc = grow_keep(j->E.k1, j->n_rec, to, st)) return rc;
    if (int rc = grow_keep(j->E.len, j->n_rec, to, st)) return rc;
    if (int rc = grow_keep(j->E.rec, j->n_rec, to, st)) return rc;
    if (int rc = grow_keep(j->E.loc, j->n_rec, to, st)) return rc;
    j->cap = to;
    return BWAMS_OK;
}

void drop_entries(bwams_dupjoin *j) {
    j->E.k0.release(); j->E.k1.release(); j->E.len.release(); j->E.rec.release(); j->E.loc.release();
    j->S.release();
    j->cap = 0;
}

int dj_add(bwams_dupjoin *j, const DevRecords &R, int64_t *n_added, const char *who) {
    if (j->n_rec + R.n_rec > 0xFFFFFFFFLL) {
        set_last_error(std::string(who) + ": more than 2^32 - 1 records");
        return BWAMS_ERR_UNSUPPORTED;
    }
    if (int rc = reserve(j, j->n_rec + R.n_rec)) return rc;
    unsigned long long h[3] = {0, 0, ~0ULL};
    if (R.n_rec > 0) {
        hipStream_t st = j->stream;
        float t = 0;
        BWAMS_HIP(hipMemcpyAsync(j->call.p, h, 24, hipMemcpyHostToDevice, st));
        BWAMS_HIP(hipEventRecord(j->ev[0], st));
        launch_dj_entries(R.bam, R.off, R.n_rec, j->n_rec, j->G, j->E, j->call.p, j->cu_count, st);
        BWAMS_HIP(hipEventRecord(j->ev[1], st));
        BWAMS_HIP(hipMemcpyAsync(h, j->call.p, 24, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipStreamSynchronize(st));
        BWAMS_HIP(hipGetLastError());
        BWAMS_HIP(hipEventElapsedTime(&t, j->ev[0], j->ev[1]));
        j->ms_add += t;
        if (h[2] != ~0ULL) {                                 // J4: the add never happened; its entries lie behind n_rec
            set_last_error(std::string(who) + ": record " + std::to_string(h[2]) + ": " + md_reason_text(4));
            return BWAMS_ERR_UNSUPPORTED;
        }
    }
    j->adds.push_back({j->n_rec, R.n_rec, h[0], h[1]});
    j->n_rec += R.n_rec;
    j->state = bwams_dupjoin::kAdding;
    if (n_added) *n_added = R.n_rec;
    return BWAMS_OK;
}

// J8's check, then the marks; R's records are those of the next add to be applied
int dj_apply(bwams_dupjoin *j, const DevRecords &R, int64_t *n_marked, const char *who) {
    if (j->applied >= j->adds.size())
        return consumer_refusal(who, "every one of the " + std::to_string(j->adds.size()) + " adds has been applied");
    const bwams_dupjoin::Add &a = j->adds[j->applied];
    if (R.n_rec != a.n)
        return consumer_refusal(who, "apply " + std::to_string(j->applied) + " was given " + std::to_string(R.n_rec) + " records, add " +
                                         std::to_string(j->applied) + " " + std::to_string(a.n));
    unsigned long long h[3] = {0, 0, 0};
    if (R.n_rec > 0) {
        hipStream_t st = j->stream;
        float t = 0;
        BWAMS_HIP(hipMemsetAsync(j->call.p, 0, 24, st));
        BWAMS_HIP(hipEventRecord(j->ev[0], st));
        launch_dj_key_sum(R.bam, R.off, R.n_rec, j->call.p, j->cu_count, st);
        BWAMS_HIP(hipMemcpyAsync(h, j->call.p, 16, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipStreamSynchronize(st));
        BWAMS_HIP(hipGetLastError());
        if (h[0] != a.sum || h[1] != a.wsum)
            return consumer_refusal(who, "apply " + std::to_string(j->applied) + ": the records' names are not those of add " +
                                             std::to_string(j->applied) + " or not in its order (the sums of their keys differ)");
        launch_md_apply(R.bam, R.off, nullptr, j->J.rec_tmpl.p + a.base, j->dup.p, R.n_rec, j->call.p + 2, j->cu_count, st);
        BWAMS_HIP(hipEventRecord(j->ev[1], st));
        BWAMS_HIP(hipMemcpyAsync(h, j->call.p, 24, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipStreamSynchronize(st));
        BWAMS_HIP(hipGetLastError());
        BWAMS_HIP(hipEventElapsedTime(&t, j->ev[0], j->ev[1]));
        j->ms_apply += t;
    }
    j->applied += 1;
    if (n_marked) *n_marked = (int64_t)h[2];
    return BWAMS_OK;
}

}  // namespace

extern "C" {

int bwams_dupjoin_open(int device, const bwams_dup_groups_t *groups, const bwams_dup_opt_t *opt, bwams_dupjoin_t **out) {
    int64_t d = 0, max_set = 0;
    if (!out || !dup_opt_values(opt, &d, &max_set)) {
        set_last_error("bwams_dupjoin_open: out, optical_distance >= 0 and max_optical_set >= 0 are required");
        return BWAMS_ERR_ARG;
    }
    *out = nullptr;
    std::unique_ptr<bwams_dupjoin> j(new bwams_dupjoin());
    if (int rc = j->open(device)) return rc;
    j->d = d;
    j->max_set = max_set;
    if (groups) { j->groups = *groups; j->has_groups = true; }
    if (int rc = groups_upload(j->g_ids, j->g_off, j->g_ord, j->g_lib, groups ? &j->groups : nullptr, &j->G, j->stream)) return rc;
    BWAMS_HIP(j->call.alloc(32));
    BWAMS_HIP(j->lib_counts.alloc((size_t)j->G.n_lib * 7 * 8));
    *out = j.release();
    return BWAMS_OK;
}

int bwams_dupjoin_close(bwams_dupjoin_t *j) {
    delete j;
    return BWAMS_OK;
}

int bwams_dupjoin_reset(bwams_dupjoin_t *j) {
    if (!j) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(j->device));
    BWAMS_HIP(hipStreamSynchronize(j->stream));
    drop_entries(j);
    j->n_rec = 0;
    j->adds.clear();
    j->applied = 0;
    j->J.n_t = j->J.n_e = 0;
    j->stats = bwams_dup_stats_t{};
    j->rows.clear();
    j->ms_add = j->ms_sort = j->ms_ends = j->ms_decide = j->ms_apply = 0;
    j->state = bwams_dupjoin::kEmpty;
    return BWAMS_OK;
}

int bwams_dupjoin_add_records(bwams_dupjoin_t *j, const void *bam, int64_t n_bytes, int64_t *n_added) {
    const char *who = "bwams_dupjoin_add_records";
    if (j && j->state >= bwams_dupjoin::kFinished) return refuse_state(who, j, false);
    DevRecords R;
    if (int rc = consumer_records(j, bam, n_bytes, who, &R)) return rc;
    return dj_add(j, R, n_added, who);
}

int bwams_dupjoin_add_file(bwams_dupjoin_t *j, bwams_bam_file_t *f, int64_t *n_added) {
    const char *who = "bwams_dupjoin_add_file";
    if (j && j->state >= bwams_dupjoin::kFinished) return refuse_state(who, j, false);
    DevRecords R;
    if (int rc = consumer_file(j, f, who, &R)) return rc;
    return dj_add(j, R, n_added, who);
}

int bwams_dupjoin_finish(bwams_dupjoin_t *j, bwams_dup_stats_t *st_out, bwams_dup_lib_stats_t *lib_stats, int64_t cap_lib) {
    const char *who = "bwams_dupjoin_finish";
    if (!j) return consumer_refusal(who, "a handle is required");
    if (j->state >= bwams_dupjoin::kFinished) return refuse_state(who, j, false);
    const int64_t n_lib = j->G.n_lib;
    if (lib_stats && cap_lib < n_lib) {
        set_last_error(std::string(who) + ": " + std::to_string(n_lib) + " libraries do not fit a capacity of " + std::to_string(cap_lib));
        return BWAMS_ERR_CAPACITY;
    }
    BWAMS_HIP(hipSetDevice(j->device));
    hipStream_t q = j->stream;
    float ms[2] = {0, 0};
    if (int rc = dj_join(j->E, j->n_rec, j->S, j->J, who, ms, j->cu_count, q)) {
        if (rc == BWAMS_ERR_UNSUPPORTED) {                   // rules 2-3: nothing of this round is of use
            drop_entries(j);
            j->state = bwams_dupjoin::kRefused;
        }
        return rc;
    }
    j->ms_sort = ms[0];
    j->ms_ends = ms[1];
    const int64_t n_t = j->J.n_t, n_e = j->J.n_e;
    const auto t0 = std::chrono::steady_clock::now();
    BWAMS_HIP(j->dup.ensure_n((size_t)std::max<int64_t>(n_t, 1)));
    MdDecideMore more{n_e ? j->J.locs.p : nullptr, (int32_t)n_lib, j->d, j->max_set, nullptr, j->lib_counts.p};
    if (more.loc && j->d > 0) {
        BWAMS_HIP(j->optical.ensure_n((size_t)std::max<int64_t>(n_t, 1)));
        BWAMS_HIP(hipMemsetAsync(j->optical.p, 0, (size_t)n_t, q));
        more.optical = j->optical.p;
    }
    BWAMS_HIP(hipMemsetAsync(j->lib_counts.p, 0, (size_t)n_lib * 7 * 8, q));
    BWAMS_HIP(hipMemsetAsync(j->call.p, 0, 16, q));
    int64_t cnt[3] = {0, 0, 0};
    if (int rc = md_decide(j->decide, j->J.ends.p, n_e, n_t, j->dup.p, cnt, j->cu_count, q, &more)) return rc;
    launch_dj_counts(j->E.rec.p, j->J.rec_tmpl.p, j->J.tloc.p, j->dup.p, j->n_rec, (int)n_lib, j->lib_counts.p, j->call.p, j->cu_count, q);
    std::vector<unsigned long long> c((size_t)n_lib * 7);
    unsigned long long marked = 0;
    BWAMS_HIP(hipMemcpyAsync(c.data(), j->lib_counts.p, c.size() * 8, hipMemcpyDeviceToHost, q));
    BWAMS_HIP(hipMemcpyAsync(&marked, j->call.p, 8, hipMemcpyDeviceToHost, q));
    BWAMS_HIP(hipStreamSynchronize(q));
    BWAMS_HIP(hipGetLastError());
    j->ms_decide = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    j->rows.resize((size_t)n_lib);
    lib_rows(j->rows.data(), n_lib, c.data());
    dup_stats(&j->stats, n_t, n_e, cnt, j->ms_decide);
    j->stats.records_marked = (int64_t)marked;
    drop_entries(j);                                         // rec_tmpl, dup and optical stay
    j->decide = MdDecide();
    j->applied = 0;
    j->state = bwams_dupjoin::kFinished;
    if (st_out) *st_out = j->stats;
    if (lib_stats) std::copy(j->rows.begin(), j->rows.end(), lib_stats);
    return BWAMS_OK;
}

int bwams_dupjoin_fetch(bwams_dupjoin_t *j, bwams_dup_end_t *ends, bwams_dup_loc_t *loc, int64_t cap_ends, uint32_t *rec_tmpl,
                        int64_t cap_rec, uint8_t *dup, uint8_t *optical, int64_t cap_tmpl) {
    const char *who = "bwams_dupjoin_fetch";
    if (!j) return consumer_refusal(who, "a handle is required");
    if (j->state != bwams_dupjoin::kFinished) return refuse_state(who, j, true);
    const int64_t n_t = j->J.n_t, n_e = j->J.n_e, n = j->n_rec;
    if (((ends || loc) && cap_ends < n_e) || (rec_tmpl && cap_rec < n) || ((dup || optical) && cap_tmpl < n_t)) {
        set_last_error(std::string(who) + ": " + std::to_string(n_e) + " ends, " + std::to_string(n) + " records and " + std::to_string(n_t) +
                       " templates do not fit the capacities " + std::to_string(cap_ends) + ", " + std::to_string(cap_rec) + " and " +
                       std::to_string(cap_tmpl));
        return BWAMS_ERR_CAPACITY;
    }
    BWAMS_HIP(hipSetDevice(j->device));
    hipStream_t q = j->stream;
    if (ends && n_e) BWAMS_HIP(hipMemcpyAsync(ends, j->J.ends.p, (size_t)n_e * sizeof(bwams_dup_end_t), hipMemcpyDeviceToHost, q));
    if (loc && n_e) BWAMS_HIP(hipMemcpyAsync(loc, j->J.locs.p, (size_t)n_e * sizeof(bwams_dup_loc_t), hipMemcpyDeviceToHost, q));
    if (rec_tmpl && n) BWAMS_HIP(hipMemcpyAsync(rec_tmpl, j->J.rec_tmpl.p, (size_t)n * 4, hipMemcpyDeviceToHost, q));
    if (dup && n_t) BWAMS_HIP(hipMemcpyAsync(dup, j->dup.p, (size_t)n_t, hipMemcpyDeviceToHost, q));
    if (optical && n_t) {
        if (j->d > 0 && n_e) BWAMS_HIP(hipMemcpyAsync(optical, j->optical.p, (size_t)n_t, hipMemcpyDeviceToHost, q));
        else memset(optical, 0, (size_t)n_t);
    }
    BWAMS_HIP(hipStreamSynchronize(q));
    return BWAMS_OK;
}

int bwams_dupjoin_apply_records(bwams_dupjoin_t *j, void *bam, int64_t n_bytes, int64_t *n_marked) {
    const char *who = "bwams_dupjoin_apply_records";
    if (j && j->state != bwams_dupjoin::kFinished) return refuse_state(who, j, true);
    DevRecords R;
    if (int rc = consumer_records(j, bam, n_bytes, who, &R)) return rc;
    if (int rc = dj_apply(j, R, n_marked, who)) return rc;
    if (n_bytes) BWAMS_HIP(hipMemcpyAsync(bam, R.bam, (size_t)n_bytes, hipMemcpyDeviceToHost, j->stream));
    BWAMS_HIP(hipStreamSynchronize(j->stream));
    return BWAMS_OK;
}

int bwams_dupjoin_apply_file(bwams_dupjoin_t *j, bwams_bam_file_t *f, int64_t *n_marked) {
    const char *who = "bwams_dupjoin_apply_file";
    if (j && j->state != bwams_dupjoin::kFinished) return refuse_state(who, j, true);
    DevRecords R;
    if (int rc = consumer_file(j, f, who, &R)) return rc;
    return dj_apply(j, R, n_marked, who);
}

int bwams_dupjoin_info(const bwams_dupjoin_t *j, bwams_dupjoin_info_t *info) {
    if (!j || !info) return BWAMS_ERR_ARG;
    memset(info, 0, sizeof *info);
    info->records = j->n_rec;
    info->templates = j->J.n_t;
    info->ends = j->J.n_e;
    info->adds = (int64_t)j->adds.size();
    info->applied = (int64_t)j->applied;
    info->entry_bytes = kDjEntryBytes;
    info->hbm_bytes = (int64_t)(j->E.k0.cap + j->E.k1.cap + j->E.len.cap + j->E.rec.cap + j->E.loc.cap + j->J.rec_tmpl.cap + j->J.ends.cap +
                                j->J.locs.cap + j->J.tloc.cap + j->dup.cap + j->optical.cap + j->recs.cap + j->roff.cap);
    info->state = (int32_t)j->state;
    info->ms_add = j->ms_add; info->ms_sort = j->ms_sort; info->ms_ends = j->ms_ends; info->ms_decide = j->ms_decide;
    info->ms_apply = j->ms_apply;
    return BWAMS_OK;
}

int bwams_dupjoin_key(const void *name, int32_t n, uint64_t key[2]) {
    if (n < 0 || n > 254 || (n && !name) || !key) {
        set_last_error("bwams_dupjoin_key: a name of 0 to 254 bytes and key are required");
        return BWAMS_ERR_ARG;
    }
    name_key(static_cast<const uint8_t *>(name), (uint32_t)n, &key[0], &key[1]);
    return BWAMS_OK;
}

}  // extern "C"
