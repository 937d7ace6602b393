// api_pileup.hip — C-ABI entry points of the pileup (include/bwams.h, "Pileup"): the handle over a list of regions, the adds from a
// batch and from host records, the reference bases, the quality plane, the indel store, and the queries, over pileup.hip and
// pileup_indel.hip; the texts over host/pileup_text.cpp, host/pileup_vcf.cpp and host/pileup_indel_vcf.cpp.
// No CPU fallback: every entry point runs HIP kernels or returns an error.
#include <algorithm>
#include <cstring>
#include <memory>

#include <rocprim/rocprim.hpp>

#include "rec_consumer.h"
#include "../host/pileup_host.h"

using namespace bwams;

struct bwams_pileup : RecConsumer {
    bwams_pileup_opt_t opt{};
    std::vector<int32_t> l_ref;
    std::vector<bwams_pileup_region_t> regions;
    std::vector<int64_t> reg_off;                    // n_regions + 1: region k's first slot; the last is the number of slots
    DevBuf<uint32_t> counts;                         // kPileupChannels per slot
    DevBuf<uint32_t> sums;                           // rule 11's plane, kPileupChannels per slot; none before bwams_pileup_set_quality
    bwams_pileup_gl_opt_t gl{};
    bool clean = true;                               // no add since the open or the last _reset: the counters are zero
    DevBuf<uint8_t> ref;                             // rule 7: a code per slot
    DevBuf<int32_t> d_beg, d_end, d_ref_first, d_reg_ref;
    DevBuf<int64_t> d_off;
    DevBuf<> tmp;                                    // rocPRIM temporary storage
    DevBuf<unsigned long long> flag;                 // [0..2] rule 3's first bad records, [3..5] the route counters of a piece
    DevBuf<uint32_t> keys, keys2, vals, vals2, heads, n_heads;       // the (tile, record) entries of a piece, twice for the sort
    DevBuf<uint8_t> route;
    DevBuf<int64_t> sel, sel_cnt;                    // the queries' device results, kept between calls
    DevBuf<bwams_pileup_site_t> d_sites;
    DevBuf<bwams_pileup_call_t> d_calls;
    DevBuf<int64_t> hole_off;                        // bwams_pileup_set_ref_index: the index's .amb holes
    DevBuf<int32_t> hole_len;
    int64_t n_added = 0;                             // records given so far (rule 6)
    int64_t last[3] = {0, 0, 0};                     // of the last add: records counted, tile entries, records routed direct
    float ms_check = 0, ms_add = 0;                  // ... and its device time
    // The indel store (rules 14 to 17); none before bwams_pileup_set_indels.
    bool indels = false;
    bwams_pileup_indel_opt_t io{};
    DevBuf<uint32_t> diff;                           // rule 15 as a difference array: four per entry, n_slots + 1 entries
    DevBuf<PileupSpan> span;                         // its inclusive scan, made by the first query after an add
    DevBuf<PileupEvKey> ev_keys, ev_sorted, grp_keys;        // the events as appended; sorted; one key per group
    DevBuf<uint32_t> ev_qe, ev_qe_sorted;
    DevBuf<PileupEvSums> grp_sums;
    DevBuf<unsigned long long> ev_n;                 // [0] the events held, as the event pass counts on; [1] the count pass of an add
    DevBuf<bwams_pileup_indel_allele_t> d_alleles;
    DevBuf<bwams_pileup_indel_t> d_icalls;
    int64_t n_events = 0, ev_cap = 0, n_appended = 0, n_groups = 0;
    bool span_valid = false, groups_valid = false;   // span and the groups answer for everything added: an add or a _reset clears both
    float ms_indel = 0;                              // the indel kernels of the last add
    // Rule 18; off before bwams_pileup_set_indel_leftalign.
    bool leftalign = false;
    std::vector<uint8_t> ref_set;                    // per region: a _set_ref* has given its bases
    DevBuf<uint32_t> ev_run;                         // transient, per event of an add: the slots below its anchor that the run ending there spans
    bool ref_complete() const { return std::find(ref_set.begin(), ref_set.end(), 0) == ref_set.end(); }
    PileupIndelStore store(unsigned long long *n) const { return PileupIndelStore{diff.p, ev_keys.p, ev_qe.p, n, ev_cap, io.indel_q, io.max_len}; }
    size_t diff_bytes() const { return ((size_t)n_slots() + 1) * 16; }
    int32_t n_ref() const { return (int32_t)l_ref.size(); }
    int32_t n_regions() const { return (int32_t)regions.size(); }
    int64_t n_slots() const { return reg_off.back(); }
    PileupRegions dev_regions() const { return PileupRegions{d_beg.p, d_end.p, d_ref_first.p, d_off.p}; }
    PileupQuality quality() const { return PileupQuality{sums.p, gl.no_qual_q}; }
    size_t plane_bytes() const { return (size_t)std::max<int64_t>(n_slots(), 1) * kPileupChannels * 4; }
};

namespace bwams {
int pileup_device(const bwams_pileup *p) { return p->device; }
const std::vector<int32_t> &pileup_l_ref(const bwams_pileup *p) { return p->l_ref; }
}  // namespace bwams

namespace {

constexpr int64_t kPiece = 1 << 24;                  // records routed and sorted at a time: 32 bytes of scratch per record

template <class Test> struct SlotCount {             // 1 at a slot the test selects
    Test f;
    __host__ __device__ int64_t operator()(int64_t s) const { return f(s) ? 1 : 0; }
};

// launch() on the handle's stream between its two events, waited for; the device time is added to *ms
template <class Launch> int timed(bwams_pileup *p, float *ms, Launch &&launch) {
    hipStream_t st = p->stream;
    float t = 0;
    BWAMS_HIP(hipEventRecord(p->ev[0], st));
    launch();
    BWAMS_HIP(hipEventRecord(p->ev[1], st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    BWAMS_HIP(hipEventElapsedTime(&t, p->ev[0], p->ev[1]));
    *ms += t;
    return BWAMS_OK;
}

// Rule 14's count pass: the events the records would append, and an event buffer that holds them beside the ones it has.  Nothing of
// the handle has moved when this fails.
int indel_reserve(bwams_pileup *p, const DevRecords &recs, const PileupFilter &f, int64_t *n_new) {
    hipStream_t st = p->stream;
    unsigned long long count = 0;
    BWAMS_HIP(hipMemsetAsync(p->ev_n.p + 1, 0, 8, st));
    if (int rc = timed(p, &p->ms_indel, [&] {
            launch_pileup_indel_events(recs.bam, recs.off, recs.n_rec, f, p->dev_regions(), p->store(p->ev_n.p + 1), 0, p->cu_count, st);
        })) return rc;
    BWAMS_HIP(hipMemcpyAsync(&count, p->ev_n.p + 1, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    const int64_t need = p->n_events + (int64_t)count;
    if (need > p->ev_cap) {                                              // grow by half, keeping the events held
        const int64_t cap = std::max<int64_t>(need + need / 2, 256);
        DevBuf<PileupEvKey> keys;
        DevBuf<uint32_t> qe;
        BWAMS_HIP(keys.alloc((size_t)cap * sizeof(PileupEvKey))); BWAMS_HIP(qe.alloc((size_t)cap * 4));
        if (p->n_events) {
            BWAMS_HIP(hipMemcpyAsync(keys.p, p->ev_keys.p, (size_t)p->n_events * sizeof(PileupEvKey), hipMemcpyDeviceToDevice, st));
            BWAMS_HIP(hipMemcpyAsync(qe.p, p->ev_qe.p, (size_t)p->n_events * 4, hipMemcpyDeviceToDevice, st));
            BWAMS_HIP(hipStreamSynchronize(st));
        }
        p->ev_keys = std::move(keys);
        p->ev_qe = std::move(qe);
        p->ev_cap = cap;
    }
    if (p->leftalign) BWAMS_HIP(p->ev_run.ensure_n((size_t)(p->ev_cap - p->n_events)));       // a word for every event the buffer has room for
    *n_new = (int64_t)count;
    return BWAMS_OK;
}

// check first, then add (rule 3)
int pileup_add(bwams_pileup *p, const DevRecords &recs, int64_t *n_counted, const char *who) {
    const uint8_t *dev_bam = recs.bam;
    const int64_t *dev_off = recs.off;
    const int64_t n_rec = recs.n_rec;
    if (p->n_added + n_rec > 0x7FFFFFFFLL) {
        set_last_error(std::string(who) + ": more than 2^31 - 1 records added in total");
        return BWAMS_ERR_UNSUPPORTED;
    }
    if (p->leftalign && !p->ref_complete()) {                            // rule 18 shifts against the bases in place
        set_last_error(std::string(who) + ": a left-aligning handle needs every region's reference bases (bwams_pileup_set_ref*) before the records");
        return BWAMS_ERR_ARG;
    }
    hipStream_t st = p->stream;
    int64_t sum[3] = {0, 0, 0};
    p->ms_check = p->ms_add = 0;
    if (n_rec > 0) {
        const PileupFilter f{p->opt.exclude, p->opt.min_mapq, p->n_ref()};
        unsigned long long h[3] = {0, 0, 0};
        if (int rc = consumer_check(p, p->flag.p, 3, h, &p->ms_check,
                                    [&] { launch_pileup_check(dev_bam, dev_off, n_rec, f, p->flag.p, p->cu_count, st); })) return rc;
        const int first = (int)(std::min_element(h, h + 3) - h);         // the first bad record; a record is in one list only
        if (h[first] != ~0ULL) {
            static const char *const why[3] = {" has a CIGAR op code above 8", " has a CIGAR whose query length is not l_seq",
                                               " ends inside its SEQ or QUAL"};
            set_last_error(std::string(who) + ": record " + std::to_string(h[first]) + why[first]);
            return BWAMS_ERR_ARG;
        }
        int64_t n_events_new = 0;
        p->ms_indel = 0;
        p->n_appended = 0;
        if (p->indels)
            if (int rc = indel_reserve(p, recs, f, &n_events_new)) return rc;
        const int64_t n_tiles = (p->n_slots() + kPileupTile - 1) / kPileupTile;
        const int tiled = knobs().pileup_tiled != 0 && n_tiles > 0;
        unsigned bits = 1;
        while ((1LL << bits) <= n_tiles) ++bits;                         // the keys are 0 .. n_tiles
        const PileupRegions R = p->dev_regions();
        const PileupQuality Q = p->quality();
        const int64_t n_max = std::min(kPiece, n_rec);                   // every buffer for the largest piece before the first counter
        BWAMS_HIP(p->route.ensure_n((size_t)n_max));                     // moves: an allocation that fails adds nothing
        if (tiled) {
            BWAMS_HIP(p->keys.ensure_n((size_t)(2 * n_max))); BWAMS_HIP(p->keys2.ensure_n((size_t)(2 * n_max)));
            BWAMS_HIP(p->vals.ensure_n((size_t)(2 * n_max))); BWAMS_HIP(p->vals2.ensure_n((size_t)(2 * n_max)));
            BWAMS_HIP(p->heads.ensure_n((size_t)std::min(2 * n_max, n_tiles)));
            size_t tb = 0;                                               // the sort's temporary storage too
            BWAMS_HIP(rocprim::radix_sort_pairs(nullptr, tb, p->keys.p, p->keys2.p, p->vals.p, p->vals2.p, (size_t)(2 * n_max), 0u, bits, st));
            if (tb > p->tmp.cap || !p->tmp.p) BWAMS_HIP(p->tmp.alloc(std::max<size_t>(tb, 256)));
        }
        p->clean = false;
        for (int64_t r0 = 0; r0 < n_rec; r0 += kPiece) {
            const int64_t n = std::min(kPiece, n_rec - r0), n_ent = 2 * n;
            if (tiled) BWAMS_HIP(hipMemsetAsync(p->n_heads.p, 0, 4, st));
            if (int rc = consumer_piece(p, p->flag.p + 3, 3, h, &p->ms_add, [&]() -> int {
                    launch_pileup_route(dev_bam, dev_off + r0, n, f, R, (uint32_t)n_tiles, tiled, p->keys.p, p->vals.p, p->route.p,
                                        p->flag.p + 3, p->cu_count, st);
                    if (tiled) {
                        if (int rc = with_tmp(p->tmp, st, (std::string(who) + ": radix_sort_pairs").c_str(), [&](void *tmp, size_t &tb) {
                                return rocprim::radix_sort_pairs(tmp, tb, p->keys.p, p->keys2.p, p->vals.p, p->vals2.p, (size_t)n_ent, 0u, bits, st);
                            })) return rc;
                        if (launch_pileup_tiles(dev_bam, dev_off + r0, R, p->opt.min_baseq, p->keys2.p, p->vals2.p, n_ent, (uint32_t)n_tiles,
                                                p->heads.p, p->n_heads.p, p->n_slots(), p->counts.p, Q, p->cu_count, st)) {
                            set_last_error(std::string(who) + ": the device refused the LDS of the quality tile");
                            return BWAMS_ERR_DEVICE;
                        }
                    }
                    launch_pileup_direct(dev_bam, dev_off + r0, n, R, p->opt.min_baseq, p->route.p, p->counts.p, Q, p->cu_count, st);
                    return BWAMS_OK;
                })) return rc;
            for (int k = 0; k < 3; ++k) sum[k] += (int64_t)h[k];
        }
        if (p->indels) {                                                 // the events and the span runs of every record of the call
            p->span_valid = p->groups_valid = false;
            if (int rc = timed(p, &p->ms_indel, [&] {
                    if (!p->leftalign) {
                        launch_pileup_indel_events(dev_bam, dev_off, n_rec, f, R, p->store(p->ev_n.p), 1, p->cu_count, st);
                        return;
                    }
                    launch_pileup_indel_events_run(dev_bam, dev_off, n_rec, f, R, p->store(p->ev_n.p), p->ev_run.p, p->n_events, p->cu_count, st);
                    launch_pileup_indel_align(R, p->n_regions(), p->ref.p, p->ev_keys.p + p->n_events, p->ev_qe.p + p->n_events, p->ev_run.p,
                                              n_events_new, p->diff.p, p->cu_count, st);      // rule 18 over the events just appended
                })) return rc;
            p->n_events += n_events_new;
            p->n_appended = n_events_new;
        }
    }
    p->n_added += n_rec;
    std::copy(sum, sum + 3, p->last);
    if (n_counted) *n_counted = sum[0];
    return BWAMS_OK;
}

int thresholds(const bwams_pileup *p, int32_t min_alt, int32_t min_permille, const char *who, PileupSiteTest *t) {
    if (min_alt < 0) min_alt = p->opt.min_alt;
    if (min_permille < 0) min_permille = p->opt.min_permille;
    if (min_alt < 1 || min_permille > 1000) {
        set_last_error(std::string(who) + ": min_alt >= 1 and min_permille <= 1000 are required (negative: the handle's)");
        return BWAMS_ERR_ARG;
    }
    *t = PileupSiteTest{p->counts.p, p->ref.p, (uint32_t)min_alt, (uint32_t)min_permille};
    return BWAMS_OK;
}

int call_thresholds(const bwams_pileup *p, int32_t min_qual, int32_t min_depth, const char *who, PileupCallTest *t) {
    if (!p->sums.p) {
        set_last_error(std::string(who) + ": the handle has no quality plane (bwams_pileup_set_quality)");
        return BWAMS_ERR_ARG;
    }
    if (min_qual < 0) min_qual = p->gl.min_qual;
    if (min_depth < 0) min_depth = p->gl.min_depth;
    if (min_depth < 1) {
        set_last_error(std::string(who) + ": min_depth >= 1 is required (negative: the handle's)");
        return BWAMS_ERR_ARG;
    }
    *t = PileupCallTest{p->counts.p, p->sums.p, p->ref.p, min_qual, min_depth};
    return BWAMS_OK;
}

// What an indel query reads, brought up to date with the adds (cached until the next add or _reset): rule 15's sums, the inclusive scan
// of the difference array; with `groups`, rule 16's groups too: the events sorted by (slot, type, len, seq) and each run of one key
// reduced to its n, Q, HOM and HET.  BWAMS_ERR_ARG on a handle without the store; the handle's device is current afterwards.
int indel_prepare(bwams_pileup *p, const char *who, bool groups) {
    if (!p->indels) {
        set_last_error(std::string(who) + ": the handle has no indel store (bwams_pileup_set_indels)");
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(p->device));
    hipStream_t st = p->stream;
    if (!p->span_valid && p->n_slots() > 0) {
        if (int rc = with_tmp(p->tmp, st, (std::string(who) + ": inclusive_scan").c_str(), [&](void *tmp, size_t &tb) {
                return rocprim::inclusive_scan(tmp, tb, p->diff.as<const PileupSpan>(), p->span.p, (size_t)p->n_slots(), rocprim::plus<PileupSpan>(), st);
            })) return rc;
        BWAMS_HIP(hipStreamSynchronize(st));
    }
    p->span_valid = true;
    if (!groups || p->groups_valid) return BWAMS_OK;
    const size_t n = (size_t)p->n_events;
    int64_t n_groups = 0;
    if (n > 0) {
        BWAMS_HIP(p->ev_sorted.ensure_n(n)); BWAMS_HIP(p->ev_qe_sorted.ensure_n(n));
        BWAMS_HIP(p->grp_keys.ensure_n(n)); BWAMS_HIP(p->grp_sums.ensure_n(n)); BWAMS_HIP(p->sel_cnt.ensure_n(8));
        if (int rc = with_tmp(p->tmp, st, (std::string(who) + ": merge_sort").c_str(), [&](void *tmp, size_t &tb) {
                return rocprim::merge_sort(tmp, tb, p->ev_keys.p, p->ev_sorted.p, p->ev_qe.p, p->ev_qe_sorted.p, n, PileupEvLess(), st);
            })) return rc;
        auto shares = rocprim::make_transform_iterator(p->ev_qe_sorted.p, PileupEvSumsOf());
        if (int rc = with_tmp(p->tmp, st, (std::string(who) + ": reduce_by_key").c_str(), [&](void *tmp, size_t &tb) {
                return rocprim::reduce_by_key(tmp, tb, p->ev_sorted.p, shares, n, p->grp_keys.p, p->grp_sums.p, p->sel_cnt.p,
                                              rocprim::plus<PileupEvSums>(), PileupEvEqual(), st);
            })) return rc;
        BWAMS_HIP(hipMemcpyAsync(&n_groups, p->sel_cnt.p, 8, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipStreamSynchronize(st));
    }
    p->n_groups = n_groups;
    p->groups_valid = true;
    return BWAMS_OK;
}

int indel_thresholds(bwams_pileup *p, int32_t min_qual, int32_t min_depth, const char *who, PileupIndelTest *t) {
    if (int rc = indel_prepare(p, who, true)) return rc;
    if (min_qual < 0) min_qual = p->io.min_qual;
    if (min_depth < 0) min_depth = p->io.min_depth;
    if (min_depth < 1) {
        set_last_error(std::string(who) + ": min_depth >= 1 is required (negative: the handle's)");
        return BWAMS_ERR_ARG;
    }
    *t = PileupIndelTest{p->grp_keys.p, p->grp_sums.p, p->n_groups, p->span.p, p->ref.p, min_qual, min_depth};
    return BWAMS_OK;
}

// a text into out[0, cap): *n the bytes written, or needed with BWAMS_ERR_CAPACITY
int text_out(const char *who, const std::string &text, char *out, int64_t cap, int64_t *n) {
    if (n) *n = (int64_t)text.size();
    if (!out || cap < (int64_t)text.size()) {
        set_last_error(std::string(who) + ": the text needs " + std::to_string(text.size()) + " bytes");
        return BWAMS_ERR_CAPACITY;
    }
    memcpy(out, text.data(), text.size());
    return BWAMS_OK;
}

void launch_records(const PileupSiteTest &test, bwams_pileup *p, int64_t n, bwams_pileup_site_t *out) {
    launch_pileup_sites(test, p->dev_regions(), p->n_regions(), p->sel.p, n, out, p->cu_count, p->stream);
}
void launch_records(const PileupCallTest &test, bwams_pileup *p, int64_t n, bwams_pileup_call_t *out) {
    launch_pileup_calls(test, p->dev_regions(), p->n_regions(), p->sel.p, n, out, p->cu_count, p->stream);
}

void launch_records(const PileupIndelTest &test, bwams_pileup *p, int64_t n, bwams_pileup_indel_t *out) {
    launch_pileup_indel_calls(test, p->dev_regions(), p->n_regions(), p->sel.p, n, out, p->cu_count, p->stream);
}

// rules 8, 13 and 16: the slots that `test` selects, counted and selected in slot order, and their records (sites or calls; d_out: the
// handle's device buffer for them) into host memory
// n_slots: the items `test` is asked about, 0 .. n_slots - 1 (the handle's slots, or rule 16's groups)
template <class Test, class Rec>
int pileup_select(bwams_pileup *p, const Test &test, DevBuf<Rec> &d_out, const char *who, const char *what, bool count_only, int64_t cap,
                  Rec *sites, std::vector<Rec> *own, int64_t *n_out, int64_t n_slots) {
    hipStream_t st = p->stream;
    int64_t n_sites = 0;
    rocprim::counting_iterator<int64_t> slot(0);
    BWAMS_HIP(p->sel_cnt.ensure_n(8));
    if (n_slots > 0) {
        auto ones = rocprim::make_transform_iterator(slot, SlotCount<Test>{test});
        if (int rc = with_tmp(p->tmp, st, (std::string(who) + ": reduce").c_str(), [&](void *tmp, size_t &tb) {
                return rocprim::reduce(tmp, tb, ones, p->sel_cnt.p, (int64_t)0, (size_t)n_slots, rocprim::plus<int64_t>(), st);
            })) return rc;
        BWAMS_HIP(hipMemcpyAsync(&n_sites, p->sel_cnt.p, 8, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipStreamSynchronize(st));
    }
    *n_out = n_sites;
    if (count_only || n_sites == 0) return BWAMS_OK;
    if (!own && cap < n_sites) {
        set_last_error(std::string(who) + ": " + std::to_string(n_sites) + " " + what + " do not fit a capacity of " + std::to_string(cap));
        return BWAMS_ERR_CAPACITY;
    }
    BWAMS_HIP(p->sel.ensure_n((size_t)n_sites)); BWAMS_HIP(d_out.ensure_n((size_t)n_sites));
    if (int rc = with_tmp(p->tmp, st, (std::string(who) + ": select").c_str(), [&](void *tmp, size_t &tb) {
            return rocprim::select(tmp, tb, slot, p->sel.p, p->sel_cnt.p, (size_t)n_slots, test, st);
        })) return rc;
    launch_records(test, p, n_sites, d_out.p);
    if (own) { own->resize((size_t)n_sites); sites = own->data(); }
    BWAMS_HIP(hipMemcpyAsync(sites, d_out.p, (size_t)n_sites * sizeof(Rec), hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    return BWAMS_OK;
}

}  // namespace

extern "C" {

int bwams_pileup_open(int device, const int32_t *l_ref, int32_t n_ref, const bwams_pileup_region_t *regions, int32_t n_regions,
                      const bwams_pileup_opt_t *opt, bwams_pileup_t **out) {
    if (!out || n_ref < 0 || (n_ref && !l_ref) || n_regions < 0 || (n_regions && !regions) ||
        (opt && (opt->exclude > 0xFFFFu || opt->reserved != 0 || opt->min_baseq < 0 || opt->min_baseq > 255 || opt->min_alt < 1 ||
                 opt->min_permille < 0 || opt->min_permille > 1000))) {
        set_last_error("bwams_pileup_open: n_ref >= 0 lengths, n_regions >= 0 regions, exclude within 16 bits, min_baseq in [0, 255], "
                       "min_alt >= 1, min_permille in [0, 1000] and reserved == 0 are required");
        return BWAMS_ERR_ARG;
    }
    *out = nullptr;
    for (int32_t r = 0; r < n_ref; ++r)
        if (l_ref[r] < 0) {
            set_last_error("bwams_pileup_open: reference " + std::to_string(r) + " has a negative length");
            return BWAMS_ERR_ARG;
        }
    for (int32_t k = 0; k < n_regions; ++k) {                            // rule 1
        const bwams_pileup_region_t &g = regions[k];
        const bool inside = g.ref >= 0 && g.ref < n_ref && g.beg >= 0 && g.beg < g.end && g.end <= l_ref[g.ref];
        const bool ordered = k == 0 || regions[k - 1].ref < g.ref || (regions[k - 1].ref == g.ref && regions[k - 1].end <= g.beg);
        if (!inside || !ordered) {
            set_last_error("bwams_pileup_open: region " + std::to_string(k) +
                           (inside ? " overlaps the one before it or is not in (ref, beg) order" : " is not 0 <= beg < end <= l_ref[ref]"));
            return BWAMS_ERR_ARG;
        }
    }
    std::unique_ptr<bwams_pileup> p(new bwams_pileup());
    if (int rc = p->open(device)) return rc;
    p->opt = opt ? *opt : bwams_pileup_opt_t{0x704, 0, 13, 2, 200, 0};
    p->l_ref.assign(l_ref, l_ref + n_ref);
    if (n_regions) p->regions.assign(regions, regions + n_regions);
    else
        for (int32_t r = 0; r < n_ref; ++r)
            if (l_ref[r] > 0) p->regions.push_back(bwams_pileup_region_t{r, 0, l_ref[r]});
    const size_t n_reg = p->regions.size();
    p->ref_set.assign(n_reg, 0);
    std::vector<int32_t> beg(n_reg), end(n_reg), reg_ref(n_reg), ref_first((size_t)n_ref + 1, 0);
    p->reg_off.assign(n_reg + 1, 0);
    for (size_t k = 0; k < n_reg; ++k) {
        const bwams_pileup_region_t &g = p->regions[k];
        beg[k] = g.beg; end[k] = g.end; reg_ref[k] = g.ref;
        p->reg_off[k + 1] = p->reg_off[k] + (g.end - g.beg);
        ++ref_first[(size_t)g.ref + 1];
    }
    for (int32_t r = 0; r < n_ref; ++r) ref_first[(size_t)r + 1] += ref_first[(size_t)r];
    hipStream_t st = p->stream;
    const size_t slots = (size_t)std::max<int64_t>(p->n_slots(), 1);
    BWAMS_HIP(p->counts.alloc(slots * kPileupChannels * 4));            // rule 1: BWAMS_ERR_NOMEM when they do not fit
    BWAMS_HIP(p->ref.alloc(slots));
    BWAMS_HIP(p->d_beg.alloc(std::max<size_t>(n_reg, 1) * 4)); BWAMS_HIP(p->d_end.alloc(std::max<size_t>(n_reg, 1) * 4));
    BWAMS_HIP(p->d_reg_ref.alloc(std::max<size_t>(n_reg, 1) * 4)); BWAMS_HIP(p->d_off.alloc((n_reg + 1) * 8));
    BWAMS_HIP(p->d_ref_first.alloc(((size_t)n_ref + 1) * 4));
    BWAMS_HIP(p->flag.alloc(6 * 8)); BWAMS_HIP(p->n_heads.alloc(4));
    BWAMS_HIP(hipMemsetAsync(p->counts.p, 0, slots * kPileupChannels * 4, st));
    BWAMS_HIP(hipMemsetAsync(p->ref.p, 4, slots, st));
    if (n_reg) {
        BWAMS_HIP(hipMemcpyAsync(p->d_beg.p, beg.data(), n_reg * 4, hipMemcpyHostToDevice, st));
        BWAMS_HIP(hipMemcpyAsync(p->d_end.p, end.data(), n_reg * 4, hipMemcpyHostToDevice, st));
        BWAMS_HIP(hipMemcpyAsync(p->d_reg_ref.p, reg_ref.data(), n_reg * 4, hipMemcpyHostToDevice, st));
    }
    BWAMS_HIP(hipMemcpyAsync(p->d_off.p, p->reg_off.data(), (n_reg + 1) * 8, hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipMemcpyAsync(p->d_ref_first.p, ref_first.data(), ((size_t)n_ref + 1) * 4, hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipStreamSynchronize(st));                                 // the host vectors above end here
    *out = p.release();
    return BWAMS_OK;
}

int bwams_pileup_close(bwams_pileup_t *p) {
    delete p;
    return BWAMS_OK;
}

int bwams_pileup_reset(bwams_pileup_t *p) {
    if (!p) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(p->device));
    BWAMS_HIP(hipMemsetAsync(p->counts.p, 0, p->plane_bytes(), p->stream));
    if (p->sums.p) BWAMS_HIP(hipMemsetAsync(p->sums.p, 0, p->plane_bytes(), p->stream));
    if (p->indels) {
        BWAMS_HIP(hipMemsetAsync(p->diff.p, 0, p->diff_bytes(), p->stream));
        BWAMS_HIP(hipMemsetAsync(p->ev_n.p, 0, 16, p->stream));
        p->n_events = p->n_appended = p->n_groups = 0;
        p->span_valid = p->groups_valid = false;
    }
    BWAMS_HIP(hipStreamSynchronize(p->stream));
    p->clean = true;
    p->n_added = 0;
    std::fill(p->last, p->last + 3, 0);
    return BWAMS_OK;
}

int bwams_pileup_add_batch(bwams_pileup_t *p, bwams_batch_t *b, int64_t *n_counted) {
    DevRecords recs;
    if (int rc = consumer_batch(p, b, "bwams_pileup_add_batch", &recs)) return rc;
    return pileup_add(p, recs, n_counted, "bwams_pileup_add_batch");
}

int bwams_pileup_add_records(bwams_pileup_t *p, const void *bam, int64_t n_bytes, int64_t *n_counted) {
    DevRecords recs;
    if (int rc = consumer_records(p, bam, n_bytes, "bwams_pileup_add_records", &recs)) return rc;
    return pileup_add(p, recs, n_counted, "bwams_pileup_add_records");
}

int bwams_pileup_add_file(bwams_pileup_t *p, bwams_bam_file_t *f, int64_t *n_counted) {
    DevRecords recs;
    if (int rc = consumer_file(p, f, "bwams_pileup_add_file", &recs)) return rc;
    return pileup_add(p, recs, n_counted, "bwams_pileup_add_file");
}

int bwams_pileup_set_ref(bwams_pileup_t *p, int32_t region, const uint8_t *codes) {
    if (!p || region < 0 || region >= p->n_regions() || !codes) {
        set_last_error("bwams_pileup_set_ref: a handle, a region in [0, n_regions) and its codes are required");
        return BWAMS_ERR_ARG;
    }
    const int64_t n = p->reg_off[(size_t)region + 1] - p->reg_off[(size_t)region];
    for (int64_t k = 0; k < n; ++k)
        if (codes[k] > 4) {
            set_last_error("bwams_pileup_set_ref: code " + std::to_string(k) + " is above 4");
            return BWAMS_ERR_ARG;
        }
    if (p->leftalign && !p->clean) {                                     // rule 18: the events held were shifted against the bases in place
        set_last_error("bwams_pileup_set_ref: a left-aligning handle takes its reference before the first add, or directly after bwams_pileup_reset");
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(p->device));
    BWAMS_HIP(hipMemcpyAsync(p->ref.p + p->reg_off[(size_t)region], codes, (size_t)n, hipMemcpyHostToDevice, p->stream));
    BWAMS_HIP(hipStreamSynchronize(p->stream));
    p->ref_set[(size_t)region] = 1;
    return BWAMS_OK;
}

int bwams_pileup_set_ref_index(bwams_pileup_t *p, const bwams_index_t *ix) {
    if (!p || !ix || ix->device != p->device || !ix->fmi.ref || !ix->d_contigs.p || ix->n_seqs != p->n_ref()) {
        set_last_error("bwams_pileup_set_ref_index: an index on the handle's device with its .0123 and the handle's n_ref contigs is required");
        return BWAMS_ERR_ARG;
    }
    if (p->leftalign && !p->clean) {
        set_last_error("bwams_pileup_set_ref_index: a left-aligning handle takes its reference before the first add, or directly after bwams_pileup_reset");
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(p->device));
    std::vector<bwams_contig_t> c((size_t)ix->n_seqs);
    if (!c.empty()) BWAMS_HIP(hipMemcpy(c.data(), ix->d_contigs.p, c.size() * sizeof(bwams_contig_t), hipMemcpyDeviceToHost));
    const int64_t l_pac = (ix->fmi.ref_seq_len - 1) / 2;                 // the forward strand of .0123, as bwams_index_set_contigs has it
    for (size_t r = 0; r < c.size(); ++r)
        if (c[r].len != p->l_ref[r] || c[r].offset < 0 || c[r].offset + c[r].len > l_pac) {
            set_last_error("bwams_pileup_set_ref_index: contig " + std::to_string(r) + " has not the handle's length, or lies outside the index");
            return BWAMS_ERR_ARG;
        }
    hipStream_t st = p->stream;
    const BnsMeta *m = ix->bns;
    const size_t n_holes = m ? m->hole_off.size() : 0;
    if (n_holes) {                                                       // in the handle: nothing queued outlives its buffer
        BWAMS_HIP(p->hole_off.ensure_n(n_holes)); BWAMS_HIP(p->hole_len.ensure_n(n_holes));
        BWAMS_HIP(hipMemcpyAsync(p->hole_off.p, m->hole_off.data(), n_holes * 8, hipMemcpyHostToDevice, st));
        BWAMS_HIP(hipMemcpyAsync(p->hole_len.p, m->hole_len.data(), n_holes * 4, hipMemcpyHostToDevice, st));
    }
    launch_pileup_ref(p->dev_regions(), p->n_regions(), p->d_reg_ref.p, p->n_slots(), ix->fmi.ref, ix->d_contigs.as<const bwams_contig_t>(),
                      p->hole_off.p, p->hole_len.p, (int32_t)n_holes, p->ref.p, p->cu_count, st);
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    std::fill(p->ref_set.begin(), p->ref_set.end(), 1);
    return BWAMS_OK;
}

int bwams_pileup_fetch(bwams_pileup_t *p, int32_t region, int32_t beg, int32_t end, uint32_t *counts) {
    if (!p || region < 0 || region >= p->n_regions() || beg < p->regions[(size_t)region].beg || end < beg ||
        end > p->regions[(size_t)region].end || (end > beg && !counts)) {
        set_last_error("bwams_pileup_fetch: a region in [0, n_regions) and region.beg <= beg <= end <= region.end are required");
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(p->device));
    if (end > beg) {
        const int64_t first = p->reg_off[(size_t)region] + (beg - p->regions[(size_t)region].beg);
        BWAMS_HIP(hipMemcpyAsync(counts, p->counts.p + first * kPileupChannels, (size_t)(end - beg) * kPileupChannels * 4,
                                 hipMemcpyDeviceToHost, p->stream));
        BWAMS_HIP(hipStreamSynchronize(p->stream));
    }
    return BWAMS_OK;
}

int bwams_pileup_set_quality(bwams_pileup_t *p, const bwams_pileup_gl_opt_t *opt) {
    const bwams_pileup_gl_opt_t o = opt ? *opt : bwams_pileup_gl_opt_t{20, 1, 30, 0};
    if (!p || o.min_qual < 0 || o.min_depth < 1 || o.no_qual_q < 0 || o.no_qual_q > 93 || o.reserved != 0) {
        set_last_error("bwams_pileup_set_quality: a handle, min_qual >= 0, min_depth >= 1, no_qual_q in [0, 93] and reserved == 0 are required");
        return BWAMS_ERR_ARG;
    }
    if (!p->clean) {
        set_last_error("bwams_pileup_set_quality: the counters are not zero: before the first add, or directly after bwams_pileup_reset");
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(p->device));
    if (!p->sums.p) BWAMS_HIP(p->sums.alloc(p->plane_bytes()));         // BWAMS_ERR_NOMEM when the plane does not fit, as rule 1's counters
    BWAMS_HIP(hipMemsetAsync(p->sums.p, 0, p->plane_bytes(), p->stream));
    BWAMS_HIP(hipStreamSynchronize(p->stream));
    p->gl = o;
    return BWAMS_OK;
}

int bwams_pileup_fetch_quality(bwams_pileup_t *p, int32_t region, int32_t beg, int32_t end, uint32_t *sums) {
    if (!p || !p->sums.p || region < 0 || region >= p->n_regions() || beg < p->regions[(size_t)region].beg || end < beg ||
        end > p->regions[(size_t)region].end || (end > beg && !sums)) {
        set_last_error("bwams_pileup_fetch_quality: a handle with a quality plane, a region in [0, n_regions) and region.beg <= beg <= end <= "
                       "region.end are required");
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(p->device));
    if (end > beg) {
        const int64_t first = p->reg_off[(size_t)region] + (beg - p->regions[(size_t)region].beg);
        BWAMS_HIP(hipMemcpyAsync(sums, p->sums.p + first * kPileupChannels, (size_t)(end - beg) * kPileupChannels * 4, hipMemcpyDeviceToHost,
                                 p->stream));
        BWAMS_HIP(hipStreamSynchronize(p->stream));
    }
    return BWAMS_OK;
}

int bwams_pileup_calls(bwams_pileup_t *p, int32_t min_qual, int32_t min_depth, bwams_pileup_call_t *calls, int64_t cap, int64_t *n) {
    if (!p || cap < 0) return BWAMS_ERR_ARG;
    PileupCallTest test;
    if (int rc = call_thresholds(p, min_qual, min_depth, "bwams_pileup_calls", &test)) return rc;
    BWAMS_HIP(hipSetDevice(p->device));
    int64_t n_calls = 0;
    const int rc = pileup_select<PileupCallTest, bwams_pileup_call_t>(p, test, p->d_calls, "bwams_pileup_calls", "calls", !calls, cap, calls, nullptr, &n_calls, p->n_slots());
    if (n) *n = n_calls;
    return rc;
}

int bwams_pileup_vcf(bwams_pileup_t *p, const char *names, const char *sample, int32_t min_qual, int32_t min_depth, char *out, int64_t cap,
                     int64_t *n) {
    if (!p || (!names && p->n_ref()) || !sample) {
        set_last_error("bwams_pileup_vcf: a handle, the references' names and a sample name are required");
        return BWAMS_ERR_ARG;
    }
    PileupCallTest test;
    if (int rc = call_thresholds(p, min_qual, min_depth, "bwams_pileup_vcf", &test)) return rc;
    BWAMS_HIP(hipSetDevice(p->device));
    std::vector<bwams_pileup_call_t> calls;
    int64_t n_calls = 0;
    if (int rc = pileup_select<PileupCallTest, bwams_pileup_call_t>(p, test, p->d_calls, "bwams_pileup_vcf", "calls", false, 0, nullptr, &calls, &n_calls, p->n_slots()))
        return rc;
    std::string text;
    if (int rc = pileup_vcf_format(names, p->l_ref.data(), p->n_ref(), p->regions.data(), p->n_regions(), sample, calls.data(), n_calls, &text))
        return rc;
    if (n) *n = (int64_t)text.size();
    if (!out || cap < (int64_t)text.size()) {
        set_last_error("bwams_pileup_vcf: the text needs " + std::to_string(text.size()) + " bytes");
        return BWAMS_ERR_CAPACITY;
    }
    memcpy(out, text.data(), text.size());
    return BWAMS_OK;
}

int bwams_pileup_sites(bwams_pileup_t *p, int32_t min_alt, int32_t min_permille, bwams_pileup_site_t *sites, int64_t cap, int64_t *n) {
    if (!p || cap < 0) return BWAMS_ERR_ARG;
    PileupSiteTest test;
    if (int rc = thresholds(p, min_alt, min_permille, "bwams_pileup_sites", &test)) return rc;
    BWAMS_HIP(hipSetDevice(p->device));
    int64_t n_sites = 0;
    const int rc = pileup_select<PileupSiteTest, bwams_pileup_site_t>(p, test, p->d_sites, "bwams_pileup_sites", "sites", !sites, cap, sites, nullptr, &n_sites, p->n_slots());
    if (n) *n = n_sites;
    return rc;
}

int bwams_pileup_text(bwams_pileup_t *p, const char *names, int32_t min_alt, int32_t min_permille, char *out, int64_t cap, int64_t *n) {
    if (!p || (!names && p->n_ref())) {
        set_last_error("bwams_pileup_text: a handle and the references' names are required");
        return BWAMS_ERR_ARG;
    }
    PileupSiteTest test;
    if (int rc = thresholds(p, min_alt, min_permille, "bwams_pileup_text", &test)) return rc;
    BWAMS_HIP(hipSetDevice(p->device));
    std::vector<bwams_pileup_site_t> sites;
    int64_t n_sites = 0;
    if (int rc = pileup_select<PileupSiteTest, bwams_pileup_site_t>(p, test, p->d_sites, "bwams_pileup_text", "sites", false, 0, nullptr, &sites, &n_sites, p->n_slots()))
        return rc;
    std::string text;
    if (int rc = pileup_text_format(names, p->n_ref(), p->regions.data(), p->n_regions(), sites.data(), n_sites, &text)) return rc;
    if (n) *n = (int64_t)text.size();
    if (!out || cap < (int64_t)text.size()) {
        set_last_error("bwams_pileup_text: the text needs " + std::to_string(text.size()) + " bytes");
        return BWAMS_ERR_CAPACITY;
    }
    memcpy(out, text.data(), text.size());
    return BWAMS_OK;
}

int bwams_pileup_set_indels(bwams_pileup_t *p, const bwams_pileup_indel_opt_t *opt) {
    const bwams_pileup_indel_opt_t o = opt ? *opt : bwams_pileup_indel_opt_t{20, 1, 40, BWAMS_PILEUP_INDEL_MAX, 0};
    if (!p || o.min_qual < 0 || o.min_depth < 1 || o.indel_q < 0 || o.indel_q > 93 || o.max_len < 1 || o.max_len > BWAMS_PILEUP_INDEL_MAX ||
        o.reserved != 0) {
        set_last_error("bwams_pileup_set_indels: a handle, min_qual >= 0, min_depth >= 1, indel_q in [0, 93], max_len in [1, 32] and reserved == 0 "
                       "are required");
        return BWAMS_ERR_ARG;
    }
    if (!p->clean) {
        set_last_error("bwams_pileup_set_indels: the counters are not zero: before the first add, or directly after bwams_pileup_reset");
        return BWAMS_ERR_ARG;
    }
    if (p->n_slots() >= (1LL << 32)) {
        set_last_error("bwams_pileup_set_indels: an event's key holds a slot below 2^32; the handle has " + std::to_string(p->n_slots()));
        return BWAMS_ERR_UNSUPPORTED;
    }
    BWAMS_HIP(hipSetDevice(p->device));
    if (!p->diff.p) BWAMS_HIP(p->diff.alloc(p->diff_bytes()));           // BWAMS_ERR_NOMEM when the span sums do not fit
    if (!p->span.p) BWAMS_HIP(p->span.alloc((size_t)std::max<int64_t>(p->n_slots(), 1) * sizeof(PileupSpan)));
    if (!p->ev_n.p) BWAMS_HIP(p->ev_n.alloc(16));
    BWAMS_HIP(hipMemsetAsync(p->diff.p, 0, p->diff_bytes(), p->stream));
    BWAMS_HIP(hipMemsetAsync(p->ev_n.p, 0, 16, p->stream));
    BWAMS_HIP(hipStreamSynchronize(p->stream));
    p->n_events = p->n_appended = p->n_groups = 0;
    p->span_valid = p->groups_valid = false;
    p->io = o;
    p->indels = true;
    p->leftalign = false;                                                // the call replaces the store's options
    return BWAMS_OK;
}

int bwams_pileup_set_indel_leftalign(bwams_pileup_t *p, int32_t on) {
    if (!p || !p->indels || (on != 0 && on != 1)) {
        set_last_error("bwams_pileup_set_indel_leftalign: a handle with an indel store (bwams_pileup_set_indels) and on in {0, 1} are required");
        return BWAMS_ERR_ARG;
    }
    if (!p->clean) {
        set_last_error("bwams_pileup_set_indel_leftalign: the counters are not zero: before the first add, or directly after bwams_pileup_reset");
        return BWAMS_ERR_ARG;
    }
    p->leftalign = on != 0;
    return BWAMS_OK;
}

int bwams_pileup_fetch_span(bwams_pileup_t *p, int32_t region, int32_t beg, int32_t end, uint32_t *sums) {
    if (!p || !p->indels || region < 0 || region >= p->n_regions() || beg < p->regions[(size_t)region].beg || end < beg ||
        end > p->regions[(size_t)region].end || (end > beg && !sums)) {
        set_last_error("bwams_pileup_fetch_span: a handle with an indel store, a region in [0, n_regions) and region.beg <= beg <= end <= "
                       "region.end are required");
        return BWAMS_ERR_ARG;
    }
    if (int rc = indel_prepare(p, "bwams_pileup_fetch_span", false)) return rc;
    if (end > beg) {
        const int64_t first = p->reg_off[(size_t)region] + (beg - p->regions[(size_t)region].beg);
        BWAMS_HIP(hipMemcpyAsync(sums, p->span.p + first, (size_t)(end - beg) * sizeof(PileupSpan), hipMemcpyDeviceToHost, p->stream));
        BWAMS_HIP(hipStreamSynchronize(p->stream));
    }
    return BWAMS_OK;
}

int bwams_pileup_indel_alleles(bwams_pileup_t *p, bwams_pileup_indel_allele_t *alleles, int64_t cap, int64_t *n) {
    if (!p || cap < 0) return BWAMS_ERR_ARG;
    if (int rc = indel_prepare(p, "bwams_pileup_indel_alleles", true)) return rc;
    if (n) *n = p->n_groups;
    if (!alleles || p->n_groups == 0) return BWAMS_OK;
    if (cap < p->n_groups) {
        set_last_error("bwams_pileup_indel_alleles: " + std::to_string(p->n_groups) + " alleles do not fit a capacity of " + std::to_string(cap));
        return BWAMS_ERR_CAPACITY;
    }
    BWAMS_HIP(p->d_alleles.ensure_n((size_t)p->n_groups));
    launch_pileup_indel_alleles(p->grp_keys.p, p->grp_sums.p, p->n_groups, p->dev_regions(), p->n_regions(), p->d_alleles.p, p->cu_count, p->stream);
    BWAMS_HIP(hipMemcpyAsync(alleles, p->d_alleles.p, (size_t)p->n_groups * sizeof(bwams_pileup_indel_allele_t), hipMemcpyDeviceToHost, p->stream));
    BWAMS_HIP(hipStreamSynchronize(p->stream));
    BWAMS_HIP(hipGetLastError());
    return BWAMS_OK;
}

int bwams_pileup_indel_calls(bwams_pileup_t *p, int32_t min_qual, int32_t min_depth, bwams_pileup_indel_t *calls, int64_t cap, int64_t *n) {
    if (!p || cap < 0) return BWAMS_ERR_ARG;
    PileupIndelTest test;
    if (int rc = indel_thresholds(p, min_qual, min_depth, "bwams_pileup_indel_calls", &test)) return rc;
    int64_t n_calls = 0;
    const int rc = pileup_select<PileupIndelTest, bwams_pileup_indel_t>(p, test, p->d_icalls, "bwams_pileup_indel_calls", "indel calls", !calls, cap,
                                                                        calls, nullptr, &n_calls, p->n_groups);
    if (n) *n = n_calls;
    return rc;
}

int bwams_pileup_indel_vcf(bwams_pileup_t *p, const char *names, const char *sample, int32_t min_qual, int32_t min_depth, char *out, int64_t cap,
                           int64_t *n) {
    if (!p || (!names && p->n_ref()) || !sample) {
        set_last_error("bwams_pileup_indel_vcf: a handle, the references' names and a sample name are required");
        return BWAMS_ERR_ARG;
    }
    PileupIndelTest test;
    if (int rc = indel_thresholds(p, min_qual, min_depth, "bwams_pileup_indel_vcf", &test)) return rc;
    std::vector<bwams_pileup_indel_t> indels;
    int64_t n_indels = 0;
    if (int rc = pileup_select<PileupIndelTest, bwams_pileup_indel_t>(p, test, p->d_icalls, "bwams_pileup_indel_vcf", "indel calls", false, 0, nullptr,
                                                                      &indels, &n_indels, p->n_groups)) return rc;
    std::string text;
    if (int rc = pileup_indel_vcf_format(names, p->l_ref.data(), p->n_ref(), p->regions.data(), p->n_regions(), sample, nullptr, 0, indels.data(),
                                         n_indels, &text)) return rc;
    return text_out("bwams_pileup_indel_vcf", text, out, cap, n);
}

int bwams_pileup_vcf_all(bwams_pileup_t *p, const char *names, const char *sample, int32_t min_qual, int32_t min_depth, int32_t indel_min_qual,
                         int32_t indel_min_depth, char *out, int64_t cap, int64_t *n) {
    if (!p || (!names && p->n_ref()) || !sample) {
        set_last_error("bwams_pileup_vcf_all: a handle, the references' names and a sample name are required");
        return BWAMS_ERR_ARG;
    }
    PileupCallTest snv_test;
    PileupIndelTest test;
    if (int rc = call_thresholds(p, min_qual, min_depth, "bwams_pileup_vcf_all", &snv_test)) return rc;
    if (int rc = indel_thresholds(p, indel_min_qual, indel_min_depth, "bwams_pileup_vcf_all", &test)) return rc;
    std::vector<bwams_pileup_call_t> snvs;
    std::vector<bwams_pileup_indel_t> indels;
    int64_t n_snvs = 0, n_indels = 0;
    if (int rc = pileup_select<PileupCallTest, bwams_pileup_call_t>(p, snv_test, p->d_calls, "bwams_pileup_vcf_all", "calls", false, 0, nullptr, &snvs,
                                                                    &n_snvs, p->n_slots())) return rc;
    if (int rc = pileup_select<PileupIndelTest, bwams_pileup_indel_t>(p, test, p->d_icalls, "bwams_pileup_vcf_all", "indel calls", false, 0, nullptr,
                                                                      &indels, &n_indels, p->n_groups)) return rc;
    std::string text;
    if (int rc = pileup_indel_vcf_format(names, p->l_ref.data(), p->n_ref(), p->regions.data(), p->n_regions(), sample, snvs.data(), n_snvs,
                                         indels.data(), n_indels, &text)) return rc;
    return text_out("bwams_pileup_vcf_all", text, out, cap, n);
}

int bwams_pileup_indel_info(const bwams_pileup_t *p, bwams_pileup_indel_info_t *info) {
    if (!p || !info) return BWAMS_ERR_ARG;
    if (!p->indels) {
        set_last_error("bwams_pileup_indel_info: the handle has no indel store (bwams_pileup_set_indels)");
        return BWAMS_ERR_ARG;
    }
    *info = bwams_pileup_indel_info_t{p->n_events, p->ev_cap, p->n_appended, p->ms_indel, 0};
    return BWAMS_OK;
}

int bwams_pileup_info(const bwams_pileup_t *p, bwams_pileup_info_t *info) {
    if (!p || !info) return BWAMS_ERR_ARG;
    *info = bwams_pileup_info_t{kPileupTile, p->n_regions(), p->n_slots(), p->last[0], p->last[1], p->last[2], p->ms_check, p->ms_add};
    return BWAMS_OK;
}

}  // extern "C"
