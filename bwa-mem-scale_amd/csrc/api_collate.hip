// api_collate.hip — C-ABI entry points of the collate handle (include/bwams.h, "Collating a coordinate-sorted BAM by read name"): the
// handle with its pool of waiting records, the add from host records and from a BAM file's piece (entry, sort, match and placement,
// the refusals, then the copies), the finish, the output and its fetch, over collate.hip.  An add decides everything before it
// copies or frees anything, so a refusal at any point leaves the handle as it was.
// No CPU fallback: every entry point runs HIP kernels or returns an error.
#include <algorithm>
#include <cstring>
#include <memory>

#include "rec_consumer.h"

using namespace bwams;

namespace {
constexpr int64_t kSlack = 16;                               // behind every buffer the copies read (rec_gather.h)
constexpr int64_t kMinBlock = 1 << 16;
constexpr int kEvents = 9;
}  // namespace

struct bwams_collate : RecConsumer {
    int64_t cap_bytes = 0;                                   // C8's cap, 0: none
    uint64_t mask = ~0ULL;
    enum State { kEmpty, kAdding, kFinished } state = kEmpty;
    CoEntries E, F;                                          // the waiting entries, in ordinal order; the next add's
    int64_t e_cap = 0, n_pend = 0;
    struct Block {
        DevBuf<uint8_t> buf;                                 // kSlack bytes more than it may hold
        int64_t used = 0;
        int64_t room() const { return (int64_t)buf.cap - kSlack - used; }
    };
    std::vector<Block> pool;                                 // a block is never moved; records go behind the last one's `used`
    int64_t live = 0, dead = 0;                              // bytes of the pool's records that wait, and that do not any more
    // an add's scratch, kept between adds
    DevBuf<uint8_t> cls, fate;
    DevBuf<uint64_t> nkey, skey;
    DevBuf<uint32_t> paired, place, idx, sidx, partner;
    DevBuf<CoPlace> w_in, w_at, p_in, p_at, s_in, s_at;
    DevBuf<uint8_t> tmp;
    DevBuf<unsigned long long> call;
    // the output of the last add or finish
    DevBuf<uint8_t> pairs, singles;
    DevBuf<int64_t> pair_off, single_off;
    int64_t pairs_bytes = 0, n_pairs = 0, singles_bytes = 0, n_singles = 0;
    bwams_collate_info_t I{};
    hipEvent_t t[kEvents] = {};
    ~bwams_collate() {
        (void)hipSetDevice(device);
        for (hipEvent_t e : t)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

// room for n elements, the first `have` kept
template <class T> int grow_keep(DevBuf<T> &b, int64_t have, int64_t n, const char *who, hipStream_t st) {
    DevBuf<T> nb;
    const hipError_t e = nb.alloc((size_t)n * sizeof(T));
    if (e == hipErrorOutOfMemory) return no_memory(who, (size_t)n * sizeof(T), "the waiting records' entries");
    BWAMS_HIP(e);
    if (have) BWAMS_HIP(hipMemcpyAsync(nb.p, b.p, (size_t)have * sizeof(T), hipMemcpyDeviceToDevice, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    b = std::move(nb);
    return BWAMS_OK;
}

int reserve_entries(bwams_collate *c, int64_t n, const char *who) {
    if (n <= c->e_cap) return BWAMS_OK;
    const int64_t to = std::max(n, c->e_cap + c->e_cap / 2 + 4096);
    hipStream_t st = c->stream;
    if (int rc = grow_keep(c->E.key, c->n_pend, to, who, st)) return rc;
    if (int rc = grow_keep(c->E.ptr, c->n_pend, to, who, st)) return rc;
    if (int rc = grow_keep(c->E.ord, c->n_pend, to, who, st)) return rc;
    if (int rc = grow_keep(c->E.size, c->n_pend, to, who, st)) return rc;
    if (int rc = grow_keep(c->E.seg, c->n_pend, to, who, st)) return rc;
    c->e_cap = to;
    return BWAMS_OK;
}

int fresh_entries(CoEntries &F, int64_t n, const char *who) {
    const char *what = "the waiting records' entries";
    if (int rc = fresh(F.key, (size_t)n, who, what)) return rc;
    if (int rc = fresh(F.ptr, (size_t)n, who, what)) return rc;
    if (int rc = fresh(F.ord, (size_t)n, who, what)) return rc;
    if (int rc = fresh(F.size, (size_t)n, who, what)) return rc;
    return fresh(F.seg, (size_t)n, who, what);
}

CoEntryArrays arrays(const CoEntries &E) { return CoEntryArrays{E.key.p, E.ptr.p, E.ord.p, E.size.p, E.seg.p}; }

int64_t entries_cap(const CoEntries &E) {
    return (int64_t)std::min({E.key.cap / 8, E.ptr.cap / 8, E.ord.cap / 8, E.size.cap / 4, E.seg.cap});
}

const char *const kReasons[2] = {"FLAG 0x1 with both or neither of 0x40 and 0x80",
                                 "a second record of its segment while its name waits for the mate"};

int refuse_finished(const char *who) {
    return consumer_refusal(who, "the handle is finished: bwams_collate_reset starts another round");
}

void set_output(bwams_collate *c, int64_t pb, int64_t np, int64_t sb, int64_t ns) {
    c->pairs_bytes = pb; c->n_pairs = np; c->singles_bytes = sb; c->n_singles = ns;
}

int co_add(bwams_collate *c, const DevRecords &R, int64_t *n_added, const char *who) {
    const int64_t n = R.n_rec, n_pend = c->n_pend, base = c->I.records;
    hipStream_t st = c->stream;
    if (n == 0) {                                            // an add all the same: its output is empty
        set_output(c, 0, 0, 0, 0);
        c->I.adds += 1;
        c->state = bwams_collate::kAdding;
        if (n_added) *n_added = 0;
        return BWAMS_OK;
    }
    // the records' classes and keys, and how many are paired
    const char *scratch = "an add's scratch";
    if (int rc = fresh(c->cls, (size_t)n, who, scratch)) return rc;
    if (int rc = fresh(c->nkey, (size_t)n, who, scratch)) return rc;
    if (int rc = fresh(c->paired, (size_t)n + 1, who, scratch)) return rc;
    if (int rc = fresh(c->place, (size_t)n + 1, who, scratch)) return rc;
    if (int rc = fresh(c->s_in, (size_t)n + 1, who, scratch)) return rc;
    if (int rc = fresh(c->s_at, (size_t)n + 1, who, scratch)) return rc;
    size_t tb = 0;
    if (int rc = co_scan_u32(nullptr, tb, c->paired.p, c->place.p, n + 1, st)) return rc;
    if (int rc = fresh(c->tmp, tb, who, scratch)) return rc;
    unsigned long long h[kCoCallWords] = {};
    h[kCoCallBad] = ~0ULL;
    BWAMS_HIP(hipMemcpyAsync(c->call.p, h, sizeof h, hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipEventRecord(c->t[0], st));
    launch_co_entry(R.bam, R.off, n, base, c->mask, c->cls.p, c->nkey.p, c->paired.p, c->call.p, c->cu_count, st);
    if (int rc = co_scan_u32(c->tmp.p, tb, c->paired.p, c->place.p, n + 1, st)) return rc;
    BWAMS_HIP(hipEventRecord(c->t[1], st));
    uint32_t m32 = 0;
    BWAMS_HIP(hipMemcpyAsync(&m32, c->place.p + n, 4, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    const int64_t m = m32, N = n_pend + m;
    if (N > 0xFFFFFFFFLL) {
        set_last_error(std::string(who) + ": more than 2^32 - 1 records would wait or be joined in one add");
        return BWAMS_ERR_UNSUPPORTED;
    }
    // the entries behind the waiting ones, the sort, the walk, the placement
    if (int rc = reserve_entries(c, N, who)) return rc;
    if (int rc = fresh(c->skey, (size_t)N, who, scratch)) return rc;
    if (int rc = fresh(c->idx, (size_t)N, who, scratch)) return rc;
    if (int rc = fresh(c->sidx, (size_t)N, who, scratch)) return rc;
    if (int rc = fresh(c->fate, (size_t)N, who, scratch)) return rc;
    if (int rc = fresh(c->partner, (size_t)N, who, scratch)) return rc;
    if (int rc = fresh(c->w_in, (size_t)N + 1, who, scratch)) return rc;
    if (int rc = fresh(c->w_at, (size_t)N + 1, who, scratch)) return rc;
    if (int rc = fresh(c->p_in, (size_t)m + 1, who, scratch)) return rc;
    if (int rc = fresh(c->p_at, (size_t)m + 1, who, scratch)) return rc;
    size_t need = 0;
    if (N > 0) {
        if (int rc = co_sort(nullptr, tb, c->E.key.p, c->skey.p, c->idx.p, c->sidx.p, N, st)) return rc;
        need = std::max(need, tb);
    }
    if (int rc = co_scan_place(nullptr, tb, c->w_in.p, c->w_at.p, std::max(N, n) + 1, st)) return rc;
    need = std::max(need, tb);
    if (int rc = fresh(c->tmp, need, who, scratch)) return rc;
    const CoEntryArrays E = arrays(c->E);
    BWAMS_HIP(hipEventRecord(c->t[2], st));
    launch_co_append(R.bam, R.off, n, base, c->cls.p, c->nkey.p, c->place.p, n_pend, E, c->idx.p, N, c->cu_count, st);
    BWAMS_HIP(hipEventRecord(c->t[3], st));
    if (N > 0) {
        tb = need;
        if (int rc = co_sort(c->tmp.p, tb, c->E.key.p, c->skey.p, c->idx.p, c->sidx.p, N, st)) return rc;
    }
    BWAMS_HIP(hipEventRecord(c->t[4], st));
    if (N > 0) {
        BWAMS_HIP(hipMemsetAsync(c->fate.p, 0, (size_t)N, st));
        launch_co_match(c->skey.p, c->sidx.p, N, n_pend, E, c->fate.p, c->partner.p, c->call.p, c->cu_count, st);
    }
    BWAMS_HIP(hipEventRecord(c->t[5], st));
    launch_co_place(c->fate.p, c->partner.p, c->E.size.p, N, n_pend, c->cls.p, R.off, n, c->w_in.p, c->p_in.p, c->s_in.p, c->cu_count, st);
    tb = need;
    if (int rc = co_scan_place(c->tmp.p, tb, c->w_in.p, c->w_at.p, N + 1, st)) return rc;
    tb = need;
    if (int rc = co_scan_place(c->tmp.p, tb, c->p_in.p, c->p_at.p, m + 1, st)) return rc;
    tb = need;
    if (int rc = co_scan_place(c->tmp.p, tb, c->s_in.p, c->s_at.p, n + 1, st)) return rc;
    launch_co_totals(c->w_at.p, c->p_at.p, c->s_at.p, N, n_pend, n, c->call.p, st);
    BWAMS_HIP(hipEventRecord(c->t[6], st));
    BWAMS_HIP(hipMemcpyAsync(h, c->call.p, sizeof h, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    if (h[kCoCallBad] != ~0ULL) {                            // C6: nothing was copied, nothing is to be undone
        set_last_error(std::string(who) + ": record " + std::to_string(h[kCoCallBad] >> 3) + ": " + kReasons[h[kCoCallBad] & 1]);
        return BWAMS_ERR_UNSUPPORTED;
    }
    const int64_t wait_bytes = (int64_t)h[kCoCallWaitBytes], wait_n = (int64_t)h[kCoCallWaitN], old_bytes = (int64_t)h[kCoCallOldBytes];
    const int64_t pair_bytes = (int64_t)h[kCoCallPairBytes], np = (int64_t)h[kCoCallPairN];
    const int64_t single_bytes = (int64_t)h[kCoCallSingleBytes], ns = (int64_t)h[kCoCallSingleN];
    const int64_t died = (int64_t)h[kCoCallDied], new_bytes = wait_bytes - old_bytes;
    if (old_bytes != c->live - died) {
        set_last_error(std::string(who) + ": the pool's bytes do not add up (internal error)");
        return BWAMS_ERR_DEVICE;
    }
    // C8: the cap, whether to compact, and every allocation, before anything is written
    if (c->cap_bytes > 0 && wait_bytes > c->cap_bytes) {
        set_last_error(std::string(who) + ": " + std::to_string(wait_bytes) + " bytes of records would wait for their mates, pool_bytes is " +
                       std::to_string(c->cap_bytes));
        return BWAMS_ERR_NOMEM;
    }
    int64_t used = 0, capacity = 0;
    for (const bwams_collate::Block &b : c->pool) { used += b.used; capacity += (int64_t)b.buf.cap - kSlack; }
    const int64_t dead = c->dead + died;
    const bool compact = dead > old_bytes || (c->cap_bytes > 0 && used + new_bytes > c->cap_bytes);
    const int64_t into = compact ? wait_bytes : new_bytes;   // bytes that go behind a block's tail
    const bool new_block = into > 0 && (compact || c->pool.empty() || c->pool.back().room() < into);
    bwams_collate::Block nb;
    if (new_block) {
        int64_t want = std::max({into, capacity, kMinBlock});
        if (c->cap_bytes > 0) want = std::max(into, std::min(want, c->cap_bytes - (compact ? 0 : used)));
        const hipError_t e = nb.buf.alloc((size_t)(want + kSlack));
        if (e == hipErrorOutOfMemory) return no_memory(who, (size_t)(want + kSlack), "the pool of waiting records");
        BWAMS_HIP(e);
    }
    if (int rc = fresh_entries(c->F, wait_n, who)) return rc;
    Staged<uint8_t> o_pairs{&c->pairs, {}}, o_singles{&c->singles, {}};
    Staged<int64_t> o_poff{&c->pair_off, {}}, o_soff{&c->single_off, {}};
    if (int rc = o_pairs.stage((size_t)(pair_bytes + kSlack), who, "the pairs")) return rc;
    if (int rc = o_poff.stage((size_t)(2 * np + 1), who, "the pairs' offsets")) return rc;
    if (int rc = o_singles.stage((size_t)(single_bytes + kSlack), who, "the singles")) return rc;
    if (int rc = o_soff.stage((size_t)(ns + 1), who, "the singles' offsets")) return rc;
    // the copies; from here on the add happens
    o_pairs.commit(); o_poff.commit(); o_singles.commit(); o_soff.commit();
    uint8_t *dst = new_block ? nb.buf.p : into > 0 ? c->pool.back().buf.p + c->pool.back().used : nullptr;
    BWAMS_HIP(hipEventRecord(c->t[7], st));
    if (np > 0) launch_co_pairs(E, c->fate.p, c->partner.p, c->p_at.p, n_pend, m, c->pairs.p, c->pair_off.p, c->cu_count, st);
    if (ns > 0) launch_co_singles(R.bam, R.off, c->cls.p, c->s_at.p, n, c->singles.p, c->single_off.p, c->cu_count, st);
    if (wait_n > 0)
        launch_co_pool(E, c->fate.p, c->w_at.p, compact ? 0 : n_pend, N, dst, compact ? 0 : old_bytes, arrays(c->F), nullptr, c->cu_count, st);
    BWAMS_HIP(hipEventRecord(c->t[8], st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    if (compact) {
        c->pool.clear();
        c->I.compactions += 1;
        c->I.bytes_compacted += old_bytes;
        c->dead = 0;
    } else {
        c->dead = dead;
    }
    if (new_block) c->pool.push_back(std::move(nb));
    if (into > 0) c->pool.back().used += into;
    c->live = wait_bytes;
    std::swap(c->E, c->F);
    c->e_cap = entries_cap(c->E);
    c->n_pend = wait_n;
    set_output(c, pair_bytes, np, single_bytes, ns);
    float ms[5] = {0, 0, 0, 0, 0}, x = 0;
    BWAMS_HIP(hipEventElapsedTime(&ms[0], c->t[0], c->t[1]));
    BWAMS_HIP(hipEventElapsedTime(&x, c->t[2], c->t[3]));
    BWAMS_HIP(hipEventElapsedTime(&ms[1], c->t[3], c->t[4]));
    BWAMS_HIP(hipEventElapsedTime(&ms[2], c->t[4], c->t[5]));
    BWAMS_HIP(hipEventElapsedTime(&ms[3], c->t[5], c->t[6]));
    BWAMS_HIP(hipEventElapsedTime(&ms[4], c->t[7], c->t[8]));
    c->I.ms_entry += ms[0] + x; c->I.ms_group += ms[1]; c->I.ms_match += ms[2]; c->I.ms_place += ms[3]; c->I.ms_copy += ms[4];
    c->I.records += n;
    c->I.skipped += n - m - ns;
    c->I.pairs += np;
    c->I.singles += ns;
    c->I.bytes_pooled += new_bytes;
    c->I.max_run = std::max(c->I.max_run, (int64_t)h[kCoCallMaxRun]);
    c->I.adds += 1;
    c->state = bwams_collate::kAdding;
    if (n_added) *n_added = n;
    return BWAMS_OK;
}

}  // namespace

extern "C" {

int bwams_collate_open(int device, const bwams_collate_opt_t *opt, bwams_collate_t **out) {
    if (!out || (opt && (opt->pool_bytes < 0 || opt->reserved[0] || opt->reserved[1]))) {
        set_last_error("bwams_collate_open: out, pool_bytes >= 0 and reserved words of 0 are required");
        return BWAMS_ERR_ARG;
    }
    *out = nullptr;
    std::unique_ptr<bwams_collate> c(new bwams_collate());
    if (int rc = c->open(device)) return rc;
    for (hipEvent_t &e : c->t) BWAMS_HIP(hipEventCreate(&e));
    if (opt) { c->cap_bytes = opt->pool_bytes; c->mask = opt->key_mask; }
    BWAMS_HIP(c->call.alloc(kCoCallWords * 8));
    *out = c.release();
    return BWAMS_OK;
}

int bwams_collate_close(bwams_collate_t *c) {
    delete c;
    return BWAMS_OK;
}

int bwams_collate_reset(bwams_collate_t *c) {
    if (!c) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(c->device));
    BWAMS_HIP(hipStreamSynchronize(c->stream));
    c->pool.clear();
    c->n_pend = c->live = c->dead = 0;
    set_output(c, 0, 0, 0, 0);
    c->I = bwams_collate_info_t{};
    c->state = bwams_collate::kEmpty;
    return BWAMS_OK;
}

int bwams_collate_add_records(bwams_collate_t *c, const void *bam, int64_t n_bytes, int64_t *n_added) {
    const char *who = "bwams_collate_add_records";
    if (c && c->state == bwams_collate::kFinished) return refuse_finished(who);
    DevRecords R;
    if (int rc = consumer_records(c, bam, n_bytes, who, &R)) return rc;
    return co_add(c, R, n_added, who);
}

int bwams_collate_add_file(bwams_collate_t *c, bwams_bam_file_t *f, int64_t *n_added) {
    const char *who = "bwams_collate_add_file";
    if (c && c->state == bwams_collate::kFinished) return refuse_finished(who);
    DevRecords R;
    if (int rc = consumer_file(c, f, who, &R)) return rc;
    return co_add(c, R, n_added, who);
}

int bwams_collate_finish(bwams_collate_t *c, int64_t *n_orphans) {
    const char *who = "bwams_collate_finish";
    if (!c) return consumer_refusal(who, "a handle is required");
    if (c->state == bwams_collate::kFinished) return refuse_finished(who);
    BWAMS_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int64_t N = c->n_pend;
    if (N > 0) {                                             // C5: every waiting record, in entry order, as the singles
        const char *scratch = "the finish's scratch";
        if (int rc = fresh(c->fate, (size_t)N, who, scratch)) return rc;
        if (int rc = fresh(c->partner, (size_t)N, who, scratch)) return rc;
        if (int rc = fresh(c->w_in, (size_t)N + 1, who, scratch)) return rc;
        if (int rc = fresh(c->w_at, (size_t)N + 1, who, scratch)) return rc;
        if (int rc = fresh(c->p_in, 1, who, scratch)) return rc;
        if (int rc = fresh(c->s_in, 1, who, scratch)) return rc;
        size_t tb = 0;
        if (int rc = co_scan_place(nullptr, tb, c->w_in.p, c->w_at.p, N + 1, st)) return rc;
        if (int rc = fresh(c->tmp, tb, who, scratch)) return rc;
        Staged<uint8_t> o_singles{&c->singles, {}};
        Staged<int64_t> o_soff{&c->single_off, {}};
        if (int rc = o_singles.stage((size_t)(c->live + kSlack), who, "the orphans")) return rc;
        if (int rc = o_soff.stage((size_t)(N + 1), who, "the orphans' offsets")) return rc;
        o_singles.commit(); o_soff.commit();
        BWAMS_HIP(hipMemsetAsync(c->fate.p, 0, (size_t)N, st));
        launch_co_place(c->fate.p, c->partner.p, c->E.size.p, N, N, nullptr, nullptr, 0, c->w_in.p, c->p_in.p, c->s_in.p, c->cu_count, st);
        if (int rc = co_scan_place(c->tmp.p, tb, c->w_in.p, c->w_at.p, N + 1, st)) return rc;
        launch_co_pool(arrays(c->E), c->fate.p, c->w_at.p, 0, N, c->singles.p, 0, CoEntryArrays{}, c->single_off.p, c->cu_count, st);
        BWAMS_HIP(hipStreamSynchronize(st));
        BWAMS_HIP(hipGetLastError());
    }
    set_output(c, 0, 0, c->live, N);
    c->pool.clear();
    c->I.orphans += N;
    c->n_pend = c->live = c->dead = 0;
    c->state = bwams_collate::kFinished;
    if (n_orphans) *n_orphans = N;
    return BWAMS_OK;
}

int bwams_collate_out(const bwams_collate_t *c, bwams_collate_out_t *out) {
    if (!c || !out) return consumer_refusal("bwams_collate_out", "a handle and out are required");
    out->pairs = c->n_pairs ? c->pairs.p : nullptr;
    out->pairs_bytes = c->pairs_bytes;
    out->n_pairs = c->n_pairs;
    out->singles = c->n_singles ? c->singles.p : nullptr;
    out->singles_bytes = c->singles_bytes;
    out->n_singles = c->n_singles;
    return BWAMS_OK;
}

int bwams_collate_fetch(bwams_collate_t *c, void *pairs, int64_t cap_pairs, int64_t *pair_off, void *singles, int64_t cap_singles,
                        int64_t *single_off) {
    const char *who = "bwams_collate_fetch";
    if (!c) return consumer_refusal(who, "a handle is required");
    if ((pairs && cap_pairs < c->pairs_bytes) || (singles && cap_singles < c->singles_bytes)) {
        set_last_error(std::string(who) + ": " + std::to_string(c->pairs_bytes) + " bytes of pairs and " + std::to_string(c->singles_bytes) +
                       " of singles do not fit the capacities " + std::to_string(cap_pairs) + " and " + std::to_string(cap_singles));
        return BWAMS_ERR_CAPACITY;
    }
    BWAMS_HIP(hipSetDevice(c->device));
    hipStream_t q = c->stream;
    if (pairs && c->pairs_bytes) BWAMS_HIP(hipMemcpyAsync(pairs, c->pairs.p, (size_t)c->pairs_bytes, hipMemcpyDeviceToHost, q));
    if (singles && c->singles_bytes) BWAMS_HIP(hipMemcpyAsync(singles, c->singles.p, (size_t)c->singles_bytes, hipMemcpyDeviceToHost, q));
    if (pair_off) {
        if (c->n_pairs) BWAMS_HIP(hipMemcpyAsync(pair_off, c->pair_off.p, (size_t)(2 * c->n_pairs + 1) * 8, hipMemcpyDeviceToHost, q));
        else pair_off[0] = 0;
    }
    if (single_off) {
        if (c->n_singles) BWAMS_HIP(hipMemcpyAsync(single_off, c->single_off.p, (size_t)(c->n_singles + 1) * 8, hipMemcpyDeviceToHost, q));
        else single_off[0] = 0;
    }
    BWAMS_HIP(hipStreamSynchronize(q));
    return BWAMS_OK;
}

int bwams_collate_info(const bwams_collate_t *c, bwams_collate_info_t *info) {
    if (!c || !info) return BWAMS_ERR_ARG;
    *info = c->I;
    info->pending = c->n_pend;
    info->pending_bytes = c->live;
    info->pool_capacity = 0;
    for (const bwams_collate::Block &b : c->pool) info->pool_capacity += (int64_t)b.buf.cap - kSlack;
    info->state = (int32_t)c->state;
    return BWAMS_OK;
}

}  // extern "C"
