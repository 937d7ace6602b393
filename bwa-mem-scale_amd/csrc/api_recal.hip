// api_recal.hip — C-ABI entry points of the base recalibration tables (include/bwams.h, "Base recalibration tables"): the handle over
// the reference lengths and a groups table, the reference and the known sites of its per-position store, the adds from a batch and
// from host records, and the queries, over recal.hip; the text over host/recal_text.cpp.
// No CPU fallback: every entry point runs HIP kernels or returns an error.
#include <algorithm>
#include <cstring>
#include <memory>

#include <rocprim/rocprim.hpp>

#include "rec_consumer.h"
#include "../host/dup_groups.h"
#include "../host/recal_host.h"

using namespace bwams;

namespace {
constexpr int kCallWords = 8;                        // a piece's words of bwams_recal::call behind the first (kRecalCall*)
}

struct bwams_recal : RecConsumer {
    bwams_recal_opt_t opt{};
    std::vector<int32_t> l_ref;
    std::vector<int64_t> ref_word;                   // n_ref + 1: reference r's first word of the store; the last is the number of words
    std::vector<std::string> ids;                    // the read groups' IDs by ordinal (rule 10)
    RecalLayout lay{};
    MdGroupsDev G{};
    DevBuf<uint32_t> store;                          // rule 1: eight positions a word
    DevBuf<int64_t> d_ref_word;
    DevBuf<int32_t> d_l_ref;
    DevBuf<unsigned long long> tables;               // lay.words() of them (rule 6)
    DevBuf<unsigned long long> call;                 // [0] rule 5's first bad record, then kCallWords words of a piece
    DevBuf<uint8_t> g_ids;                           // the groups table on the device
    DevBuf<int64_t> g_off;
    DevBuf<int32_t> g_ord, g_lib;
    DevBuf<uint32_t> keys, keys2, vals, vals2, key_first;        // the (key, record) entries of a piece, twice for the sort
    DevBuf<int64_t> item_first;
    DevBuf<> tmp;                                    // rocPRIM temporary storage
    DevBuf<uint8_t> codes;                           // bwams_recal_set_ref: the uploaded codes
    DevBuf<bwams_recal_site_t> sites;                // bwams_recal_add_known: the uploaded intervals
    DevBuf<int64_t> hole_off;                        // bwams_recal_set_ref_index: the index's .amb holes
    DevBuf<int32_t> hole_len;
    int64_t n_added = 0;                             // records given so far (rule 8)
    int64_t last[3] = {0, 0, 0};                     // of the last add: records given, records counted, bases observed
    int last_lds = 1;                                // ... the path it took
    float ms_check = 0, ms_add = 0;                  // ... and its device time
    int32_t n_ref() const { return (int32_t)l_ref.size(); }
    int64_t n_words() const { return ref_word.back(); }
    uint32_t n_keys() const { return 2u * (uint32_t)(lay.n_rg + 1); }
    RecalStore dev_store() const { return RecalStore{store.p, d_ref_word.p, d_l_ref.p}; }
    RecalFilter filter() const { return RecalFilter{opt.exclude, opt.min_mapq, opt.min_baseq, opt.max_cycle, n_ref()}; }
};

namespace bwams {
int recal_device(const bwams_recal *r) { return r->device; }
const std::vector<int32_t> &recal_l_ref(const bwams_recal *r) { return r->l_ref; }
}  // namespace bwams

namespace {

constexpr int64_t kPiece = 1 << 24;                  // records keyed and sorted at a time: 16 bytes of scratch per record

// check first, then add (rule 5)
int recal_add(bwams_recal *r, const DevRecords &R, int64_t *n_counted, const char *who) {
    const int64_t n_rec = R.n_rec;
    if (r->n_added + n_rec > 0x7FFFFFFFLL) {
        set_last_error(std::string(who) + ": more than 2^31 - 1 records added in total");
        return BWAMS_ERR_UNSUPPORTED;
    }
    hipStream_t st = r->stream;
    int64_t counted = 0, bases = 0;
    r->ms_check = r->ms_add = 0;
    const int lds = knobs().recal_lds != 0;
    if (n_rec > 0) {
        const RecalFilter f = r->filter();
        const RecalStore S = r->dev_store();
        const uint32_t n_keys = r->n_keys();
        unsigned long long h[kCallWords];
        if (int rc = consumer_check(r, r->call.p, 1, h, &r->ms_check,
                                    [&] { launch_recal_check(R.bam, R.off, n_rec, f, r->G.walk, r->call.p, r->cu_count, st); })) return rc;
        if (h[0] != ~0ULL) {
            static const char *const why[5] = {" has a CIGAR op code above 8 (op)", " has a CIGAR whose query length is not l_seq (length)",
                                               " ends inside its SEQ or QUAL (bounds)", " is longer than max_cycle (cycle)",
                                               " has aux fields that do not chain to its end (aux)"};
            return consumer_refuse_packed(who, h[0], why);
        }
        unsigned bits = 1;
        while ((1ULL << bits) <= n_keys) ++bits;                         // the keys are 0 .. n_keys
        const int64_t n_max = std::min(kPiece, n_rec);                   // every buffer for the largest piece before the first counter
        BWAMS_HIP(r->keys.ensure_n((size_t)n_max));                      // moves: an allocation that fails adds nothing
        BWAMS_HIP(r->vals.ensure_n((size_t)n_max));
        if (lds) {
            BWAMS_HIP(r->keys2.ensure_n((size_t)n_max)); BWAMS_HIP(r->vals2.ensure_n((size_t)n_max));
            size_t tb = 0;                                               // the sort's temporary storage too
            BWAMS_HIP(rocprim::radix_sort_pairs(nullptr, tb, r->keys.p, r->keys2.p, r->vals.p, r->vals2.p, (size_t)n_max, 0u, bits, st));
            if (tb > r->tmp.cap || !r->tmp.p) BWAMS_HIP(r->tmp.alloc(std::max<size_t>(tb, 256)));
        }
        for (int64_t r0 = 0; r0 < n_rec; r0 += kPiece) {
            const int64_t n = std::min(kPiece, n_rec - r0);
            unsigned long long *call = r->call.p + 1;
            if (int rc = consumer_piece(r, call, kCallWords, h, &r->ms_add, [&]() -> int {
                    launch_recal_records(R.bam, R.off + r0, n, f, r->G, n_keys, r->keys.p, r->vals.p, call, r->cu_count, st);
                    if (lds) {
                        if (int rc = with_tmp(r->tmp, st, (std::string(who) + ": radix_sort_pairs").c_str(), [&](void *tmp, size_t &tb) {
                                return rocprim::radix_sort_pairs(tmp, tb, r->keys.p, r->keys2.p, r->vals.p, r->vals2.p, (size_t)n, 0u, bits, st);
                            })) return rc;
                        launch_recal_items(r->keys2.p, n, n_keys, call + kRecalCallMaxLen, r->key_first.p, r->item_first.p,
                                           call + kRecalCallItems, st);
                        launch_recal_bases(R.bam, R.off + r0, n, f, S, r->lay, r->vals2.p, n_keys, r->key_first.p, r->item_first.p,
                                           call + kRecalCallItems, r->tables.p, call, r->cu_count, st);
                    } else {
                        launch_recal_plain(R.bam, R.off + r0, n, f, S, r->lay, r->keys.p, n_keys, r->tables.p, call, r->cu_count, st);
                    }
                    return BWAMS_OK;
                })) return rc;
            counted += (int64_t)h[kRecalCallCounted];
            bases += (int64_t)h[kRecalCallBases];
        }
    }
    r->n_added += n_rec;
    r->last[0] = n_rec; r->last[1] = counted; r->last[2] = bases;
    r->last_lds = lds;
    if (n_counted) *n_counted = counted;
    return BWAMS_OK;
}

// where table `what` starts in the block, and its number of values
bool recal_table_at(const RecalLayout &L, int32_t what, int64_t *at, int64_t *n) {
    const int64_t start[5] = {L.rg(), L.qual(), L.cycle(), L.context(), L.words()};
    if (what < 0 || what > 3) return false;
    *at = start[what];
    *n = start[what + 1] - start[what];
    return true;
}

}  // namespace

extern "C" {

int bwams_recal_open(int device, const int32_t *l_ref, int32_t n_ref, const bwams_dup_groups_t *groups, const bwams_recal_opt_t *opt,
                     bwams_recal_t **out) {
    if (!out || n_ref < 0 || (n_ref && !l_ref) ||
        (opt && (opt->exclude > 0xFFFFu || opt->reserved != 0 || opt->min_baseq < 0 || opt->min_baseq > 93 || opt->max_cycle < 1))) {
        set_last_error("bwams_recal_open: n_ref >= 0 lengths, exclude within 16 bits, min_baseq in [0, 93], max_cycle >= 1 and "
                       "reserved == 0 are required");
        return BWAMS_ERR_ARG;
    }
    *out = nullptr;
    for (int32_t k = 0; k < n_ref; ++k)
        if (l_ref[k] < 0) {
            set_last_error("bwams_recal_open: reference " + std::to_string(k) + " has a negative length");
            return BWAMS_ERR_ARG;
        }
    if (groups && groups->ids.size() > (size_t)(1 << 24)) {
        set_last_error("bwams_recal_open: more than 2^24 read groups");
        return BWAMS_ERR_UNSUPPORTED;
    }
    std::unique_ptr<bwams_recal> r(new bwams_recal());
    if (int rc = r->open(device)) return rc;
    r->opt = opt ? *opt : bwams_recal_opt_t{0x704, 1, 6, 500, 0};
    r->l_ref.assign(l_ref, l_ref + n_ref);
    r->ref_word.assign((size_t)n_ref + 1, 0);
    for (int32_t k = 0; k < n_ref; ++k) r->ref_word[(size_t)k + 1] = r->ref_word[(size_t)k] + ((int64_t)l_ref[k] + 7) / 8;
    if (groups) r->ids = groups->ids;
    r->lay = RecalLayout{(int32_t)r->ids.size(), r->opt.max_cycle};
    hipStream_t st = r->stream;
    const size_t words = (size_t)std::max<int64_t>(r->n_words(), 1), n_keys = r->n_keys();
    BWAMS_HIP(r->store.alloc(words * 4));                                // rule 1: BWAMS_ERR_NOMEM when they do not fit
    BWAMS_HIP(r->tables.alloc((size_t)r->lay.words() * 8));
    BWAMS_HIP(r->call.alloc((1 + kCallWords) * 8));
    BWAMS_HIP(r->d_ref_word.alloc(((size_t)n_ref + 1) * 8)); BWAMS_HIP(r->d_l_ref.alloc(std::max<size_t>((size_t)n_ref, 1) * 4));
    BWAMS_HIP(r->key_first.alloc((n_keys + 1) * 4)); BWAMS_HIP(r->item_first.alloc((n_keys + 1) * 8));
    BWAMS_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(r->store.p), 0x44444444, words, st));       // rule 2: every code 4
    BWAMS_HIP(hipMemsetAsync(r->tables.p, 0, (size_t)r->lay.words() * 8, st));
    BWAMS_HIP(hipMemcpyAsync(r->d_ref_word.p, r->ref_word.data(), ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, st));
    if (n_ref) BWAMS_HIP(hipMemcpyAsync(r->d_l_ref.p, r->l_ref.data(), (size_t)n_ref * 4, hipMemcpyHostToDevice, st));
    if (int rc = groups_upload(r->g_ids, r->g_off, r->g_ord, r->g_lib, groups, &r->G, st)) return rc;
    BWAMS_HIP(hipStreamSynchronize(st));
    *out = r.release();
    return BWAMS_OK;
}

int bwams_recal_close(bwams_recal_t *r) {
    delete r;
    return BWAMS_OK;
}

int bwams_recal_reset(bwams_recal_t *r) {
    if (!r) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(r->device));
    BWAMS_HIP(hipMemsetAsync(r->tables.p, 0, (size_t)r->lay.words() * 8, r->stream));
    BWAMS_HIP(hipStreamSynchronize(r->stream));
    r->n_added = 0;
    std::fill(r->last, r->last + 3, 0);
    return BWAMS_OK;
}

int bwams_recal_add_batch(bwams_recal_t *r, bwams_batch_t *b, int64_t *n_counted) {
    DevRecords R;
    if (int rc = consumer_batch(r, b, "bwams_recal_add_batch", &R)) return rc;
    return recal_add(r, R, n_counted, "bwams_recal_add_batch");
}

int bwams_recal_add_records(bwams_recal_t *r, const void *bam, int64_t n_bytes, int64_t *n_counted) {
    DevRecords R;
    if (int rc = consumer_records(r, bam, n_bytes, "bwams_recal_add_records", &R)) return rc;
    return recal_add(r, R, n_counted, "bwams_recal_add_records");
}

int bwams_recal_add_file(bwams_recal_t *r, bwams_bam_file_t *f, int64_t *n_counted) {
    DevRecords R;
    if (int rc = consumer_file(r, f, "bwams_recal_add_file", &R)) return rc;
    return recal_add(r, R, n_counted, "bwams_recal_add_file");
}

int bwams_recal_set_ref(bwams_recal_t *r, int32_t ref, const uint8_t *codes) {
    if (!r || ref < 0 || ref >= r->n_ref() || (!codes && r->l_ref[(size_t)ref] > 0)) {
        set_last_error("bwams_recal_set_ref: a handle, a reference in [0, n_ref) and its codes are required");
        return BWAMS_ERR_ARG;
    }
    const int32_t n = r->l_ref[(size_t)ref];
    for (int32_t k = 0; k < n; ++k)
        if (codes[k] > 4) {
            set_last_error("bwams_recal_set_ref: code " + std::to_string(k) + " is above 4");
            return BWAMS_ERR_ARG;
        }
    if (n == 0) return BWAMS_OK;
    BWAMS_HIP(hipSetDevice(r->device));
    hipStream_t st = r->stream;
    BWAMS_HIP(r->codes.ensure_n((size_t)n));
    BWAMS_HIP(hipMemcpyAsync(r->codes.p, codes, (size_t)n, hipMemcpyHostToDevice, st));
    launch_recal_set_ref(r->store.p, r->ref_word[(size_t)ref], r->codes.p, n, r->cu_count, st);
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    return BWAMS_OK;
}

int bwams_recal_set_ref_index(bwams_recal_t *r, const bwams_index_t *ix) {
    if (!r || !ix || ix->device != r->device || !ix->fmi.ref || !ix->d_contigs.p || ix->n_seqs != r->n_ref()) {
        set_last_error("bwams_recal_set_ref_index: an index on the handle's device with its .0123 and the handle's n_ref contigs is required");
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(r->device));
    std::vector<bwams_contig_t> c((size_t)ix->n_seqs);
    if (!c.empty()) BWAMS_HIP(hipMemcpy(c.data(), ix->d_contigs.p, c.size() * sizeof(bwams_contig_t), hipMemcpyDeviceToHost));
    const int64_t l_pac = (ix->fmi.ref_seq_len - 1) / 2;                 // the forward strand of .0123, as bwams_index_set_contigs has it
    for (size_t k = 0; k < c.size(); ++k)
        if (c[k].len != r->l_ref[k] || c[k].offset < 0 || c[k].offset + c[k].len > l_pac) {
            set_last_error("bwams_recal_set_ref_index: contig " + std::to_string(k) + " has not the handle's length, or lies outside the index");
            return BWAMS_ERR_ARG;
        }
    hipStream_t st = r->stream;
    const BnsMeta *m = ix->bns;
    const size_t n_holes = m ? m->hole_off.size() : 0;
    if (n_holes) {                                                       // in the handle: nothing queued outlives its buffer
        BWAMS_HIP(r->hole_off.ensure_n(n_holes)); BWAMS_HIP(r->hole_len.ensure_n(n_holes));
        BWAMS_HIP(hipMemcpyAsync(r->hole_off.p, m->hole_off.data(), n_holes * 8, hipMemcpyHostToDevice, st));
        BWAMS_HIP(hipMemcpyAsync(r->hole_len.p, m->hole_len.data(), n_holes * 4, hipMemcpyHostToDevice, st));
    }
    launch_recal_ref_index(r->store.p, r->d_ref_word.p, r->n_ref(), r->n_words(), ix->fmi.ref, ix->d_contigs.as<const bwams_contig_t>(),
                           r->hole_off.p, r->hole_len.p, (int32_t)n_holes, r->cu_count, st);
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    return BWAMS_OK;
}

int bwams_recal_add_known(bwams_recal_t *r, const bwams_recal_site_t *sites, int64_t n) {
    if (!r || n < 0 || (n && !sites)) {
        set_last_error("bwams_recal_add_known: a handle and n >= 0 intervals are required");
        return BWAMS_ERR_ARG;
    }
    for (int64_t k = 0; k < n; ++k) {                                    // rule 3: all of them before any flag is set
        const bwams_recal_site_t &s = sites[k];
        if (s.ref < 0 || s.ref >= r->n_ref() || s.beg < 0 || s.beg >= s.end || s.end > r->l_ref[(size_t)s.ref]) {
            set_last_error("bwams_recal_add_known: interval " + std::to_string(k) + " is not 0 <= beg < end <= l_ref[ref]");
            return BWAMS_ERR_ARG;
        }
    }
    if (n == 0) return BWAMS_OK;
    BWAMS_HIP(hipSetDevice(r->device));
    hipStream_t st = r->stream;
    BWAMS_HIP(r->sites.ensure_n((size_t)n));
    BWAMS_HIP(hipMemcpyAsync(r->sites.p, sites, (size_t)n * sizeof(bwams_recal_site_t), hipMemcpyHostToDevice, st));
    launch_recal_known(r->store.p, r->d_ref_word.p, r->sites.p, n, r->cu_count, st);
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    return BWAMS_OK;
}

int bwams_recal_table(bwams_recal_t *r, int32_t what, int64_t *out, int64_t cap, int64_t *n) {
    int64_t at = 0, len = 0;
    if (!r || cap < 0 || !recal_table_at(r->lay, what, &at, &len)) {
        set_last_error("bwams_recal_table: a handle, a table of BWAMS_RECAL_TABLE_* and cap >= 0 are required");
        return BWAMS_ERR_ARG;
    }
    if (n) *n = len;
    if (!out) return BWAMS_OK;
    if (cap < len) {
        set_last_error("bwams_recal_table: " + std::to_string(len) + " values do not fit a capacity of " + std::to_string(cap));
        return BWAMS_ERR_CAPACITY;
    }
    BWAMS_HIP(hipSetDevice(r->device));
    BWAMS_HIP(hipMemcpyAsync(out, r->tables.p + at, (size_t)len * 8, hipMemcpyDeviceToHost, r->stream));
    BWAMS_HIP(hipStreamSynchronize(r->stream));
    return BWAMS_OK;
}

int bwams_recal_text(bwams_recal_t *r, const bwams_dup_groups_t *names, char *out, int64_t cap, int64_t *n) {
    if (!r || (names ? names->ids.size() : 0) != r->ids.size()) {
        set_last_error("bwams_recal_text: a handle and a groups table with the handle's number of read groups are required");
        return BWAMS_ERR_ARG;
    }
    std::vector<int64_t> host((size_t)r->lay.words());
    BWAMS_HIP(hipSetDevice(r->device));
    BWAMS_HIP(hipMemcpyAsync(host.data(), r->tables.p, host.size() * 8, hipMemcpyDeviceToHost, r->stream));
    BWAMS_HIP(hipStreamSynchronize(r->stream));
    RecalTables t;
    t.max_cycle = r->opt.max_cycle;
    if (names) t.ids = names->ids;
    for (int32_t k = 0; k < 4; ++k) {
        int64_t at = 0, len = 0;
        recal_table_at(r->lay, k, &at, &len);
        t.table[k] = host.data() + at;
    }
    std::string text;
    recal_text_format(t, &text);
    if (n) *n = (int64_t)text.size();
    if (!out || cap < (int64_t)text.size()) {
        set_last_error("bwams_recal_text: the text needs " + std::to_string(text.size()) + " bytes");
        return BWAMS_ERR_CAPACITY;
    }
    memcpy(out, text.data(), text.size());
    return BWAMS_OK;
}

int bwams_recal_info(const bwams_recal_t *r, bwams_recal_info_t *info) {
    if (!r || !info) return BWAMS_ERR_ARG;
    *info = bwams_recal_info_t{r->last_lds, kRecalSlice, r->last[0], r->last[1], r->last[2], r->n_words() * 4, r->ms_check, r->ms_add};
    return BWAMS_OK;
}

}  // extern "C"
