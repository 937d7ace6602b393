// api_bam.hip — C-ABI entry points of the BAM side (include/bwams.h): bwams_bam_run, _fetch, _fetch_bgzf and _upload, the
// coordinate sort (bwams_bam_sort, _sorted_fetch) and duplicate marking (bwams_bam_templates / _templates2, _templates_fetch / _fetch_loc,
// _lib_record_counts, _markdup / _markdup2, bwams_dup_decide / _decide2), over bam.hip, bam_sort.hip and markdup.hip.  No CPU fallback: every entry point runs HIP kernels or returns an error.
#include <algorithm>
#include <chrono>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "stage_state.h"
#include "../host/dup_groups.h"

using namespace bwams;

namespace bwams {
int bam_record_offsets(const char *who, const void *bam, int64_t n_bytes, std::vector<int64_t> *offsets, int32_t *max_rid) {
    const uint8_t *p = static_cast<const uint8_t *>(bam);
    auto i32 = [&](int64_t at) { int32_t v; memcpy(&v, p + at, 4); return v; };
    std::vector<int64_t> &off = *offsets;
    off.assign(1, 0);
    *max_rid = -1;
    auto rec = [&]() { return std::string(who) + ": record " + std::to_string(off.size() - 1); };       // built on an error only
    for (int64_t at = 0; at < n_bytes;) {                   // the block_size chain, and what the kernels read inside it
        if (n_bytes - at < 4) { set_last_error(rec() + " is cut off"); return BWAMS_ERR_ARG; }
        const int64_t bs = (uint32_t)i32(at);
        if (bs < 32 || bs > n_bytes - at - 4) {
            set_last_error(rec() + ": block_size " + std::to_string(bs) + (bs < 32 ? " < 32" : " runs past n_bytes"));
            return BWAMS_ERR_ARG;
        }
        const int32_t rid = i32(at + 4), pos = i32(at + 8);
        const int64_t l_name = p[at + 12], n_cig = (int64_t)p[at + 16] | (int64_t)p[at + 17] << 8;
        if (rid < -1 || pos < -1 || pos > 0x7FFFFFFE || 32 + l_name + 4 * n_cig > bs) {
            set_last_error(rec() + ": refID < -1, POS outside [-1, 2^31 - 2], or its name and CIGAR run past block_size");
            return BWAMS_ERR_ARG;
        }
        *max_rid = std::max(*max_rid, rid);
        at += 4 + bs;
        off.push_back(at);
    }
    return BWAMS_OK;
}
// The groups table as the device reads it (MdGroupsDev): IDs sorted by bytes, uploaded into the caller's buffers (g null: no table).
int groups_upload(DevBuf<uint8_t> &g_ids, DevBuf<int64_t> &g_off, DevBuf<int32_t> &g_ord, DevBuf<int32_t> &g_lib,
                  const bwams_dup_groups_t *g, MdGroupsDev *G, hipStream_t st) {
    memset(G, 0, sizeof *G);
    G->n_lib = 1;
    if (!g) return BWAMS_OK;
    const size_t n = g->ids.size();
    std::vector<int32_t> ord(n);
    for (size_t k = 0; k < n; ++k) ord[k] = (int32_t)k;
    std::sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return g->ids[(size_t)a] < g->ids[(size_t)b]; });   // by unsigned bytes
    std::vector<int64_t> off(n + 1, 0);
    std::string ids;
    for (size_t k = 0; k < n; ++k) { ids += g->ids[(size_t)ord[k]]; off[k + 1] = (int64_t)ids.size(); }
    BWAMS_HIP(g_ids.ensure_n(ids.size() + 1)); BWAMS_HIP(g_off.ensure_n(n + 1));
    BWAMS_HIP(g_ord.ensure_n(n + 1)); BWAMS_HIP(g_lib.ensure_n(n + 1));
    if (!ids.empty()) BWAMS_HIP(hipMemcpyAsync(g_ids.p, ids.data(), ids.size(), hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipMemcpyAsync(g_off.p, off.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    if (n) {
        BWAMS_HIP(hipMemcpyAsync(g_ord.p, ord.data(), n * 4, hipMemcpyHostToDevice, st));
        BWAMS_HIP(hipMemcpyAsync(g_lib.p, g->rg_lib.data(), n * 4, hipMemcpyHostToDevice, st));
    }
    BWAMS_HIP(hipStreamSynchronize(st));                       // the host vectors above end here
    G->ids = g_ids.p; G->id_off = g_off.p; G->id_ord = g_ord.p; G->rg_lib = g_lib.p;
    G->n_rg = (int32_t)n; G->n_lib = (int32_t)g->libs.size(); G->walk = 1;
    return BWAMS_OK;
}
// the decision's counts (md_decide: pairs, pair duplicates, fragment duplicates) as the caller's statistics
void dup_stats(bwams_dup_stats_t *st, int64_t n_t, int64_t n_e, const int64_t cnt[3], float ms) {
    memset(st, 0, sizeof *st);
    st->templates = n_t;
    st->pairs_examined = cnt[0];
    st->unpaired_examined = n_e - cnt[0];
    st->pair_duplicates = cnt[1];
    st->unpaired_duplicates = cnt[2];
    st->ms_decide = ms;
}

// rule 13's rows from the device's counts (md_decide's and md_lib_recs': 7 words per library), rule 14 and the percentage added
void lib_rows(bwams_dup_lib_stats_t *rows, int64_t n_lib, const unsigned long long *c) {
    for (int64_t k = 0; k < n_lib; ++k, c += 7) {
        bwams_dup_lib_stats_t &r = rows[k];
        memset(&r, 0, sizeof r);
        r.unpaired_examined = (int64_t)c[0]; r.pairs_examined = (int64_t)c[1]; r.unpaired_duplicates = (int64_t)c[2];
        r.pair_duplicates = (int64_t)c[3]; r.pair_optical_duplicates = (int64_t)c[4]; r.secondary_or_supplementary = (int64_t)c[5];
        r.unmapped = (int64_t)c[6];
        dup_lib_finish(&r);
    }
}

// opt as md_decide takes it: d (0: off) and the largest group examined; false for a negative value
bool dup_opt_values(const bwams_dup_opt_t *opt, int64_t *d, int64_t *max_set) {
    *d = opt ? opt->optical_distance : 0;
    *max_set = opt && opt->max_optical_set ? opt->max_optical_set : 300000;
    return *d >= 0 && *max_set > 0;
}
}  // namespace bwams

extern "C" {
/* ------------------------------------------------------------ BAM records (bam.hip) ---- */

int bwams_bam_run(bwams_batch_t *b, int64_t *bam_bytes, int64_t *n_records) {
    if (!has(b, Product::sam)) {
        set_last_error("bwams_bam_run: run bwams_sam_run first");
        return BWAMS_ERR_ARG;
    }
    bwams_index *ix = b->idx;
    if (!ix->d_ctg_sorted.p || (int64_t)ix->h_ctg_names.size() != ix->n_seqs) {
        set_last_error("bwams_bam_run: the index has no sequence names (bwams_index_set_contig_names)");
        return BWAMS_ERR_ARG;
    }
    if (ix->ctg_dup) {
        set_last_error("bwams_bam_run: two of the index's sequences have the same name; BAM cannot tell them apart");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    BWAMS_HIP(hipSetDevice(ix->device));
    hipStream_t st = b->stream;
    outdated(b, Product::bam);
    s->bm.nref = (uint32_t)ix->n_seqs;
    const int64_t nseq = s->sm.merged_n >= 0 ? s->sm.merged_n : s->ch.nseq;
    DevBuf<int64_t> ends;
    int64_t n_rec = 0;
    int rc = line_ends(s->sm.out.p, s->sm.bytes, st, &ends, &n_rec);
    if (rc) return rc;
    BWAMS_HIP(s->bm.size.ensure_n((size_t)(n_rec + 1))); BWAMS_HIP(s->bm.roff.ensure_n((size_t)(n_rec + 1)));
    BWAMS_HIP(s->bm.off.ensure_n((size_t)(nseq + 1))); BWAMS_HIP(s->bm.bad.ensure_n(8));
    if (n_rec == 0) {                                         // no text (a chunk of no reads): no records
        BWAMS_HIP(hipMemsetAsync(s->bm.off.p, 0, (size_t)(nseq + 1) * 8, st));
        BWAMS_HIP(hipStreamSynchronize(st));
        s->bm.bytes = 0; s->bm.nrec = 0; s->bm.nseq = nseq;
        if (bam_bytes) *bam_bytes = 0;
        if (n_records) *n_records = 0;
        produced(b, Product::bam);
        return BWAMS_OK;
    }
    BamArgs A;
    memset(&A, 0, sizeof A);
    A.text = s->sm.out.p; A.line_end = ends.p; A.read_off = s->sm.off.p; A.n_rec = n_rec; A.nseq = nseq;
    A.ctg_names = ix->d_ctg_names.as<const char>(); A.ctg_off = ix->d_ctg_off.as<const int32_t>();
    A.ctg_sorted = ix->d_ctg_sorted.as<const int32_t>(); A.n_ctg = ix->n_seqs; A.size = s->bm.size.p; A.rec_off = s->bm.roff.p; A.bad = s->bm.bad.p;
    BWAMS_HIP(hipMemsetAsync(s->bm.bad.p, 0xFF, 8, st));
    BWAMS_HIP(hipMemsetAsync(A.size + n_rec, 0, 8, st));
    launch_bam_count(A, b->cu_count, st);
    if ((rc = scan_rows(b, A.size, s->bm.roff.p, 1, n_rec + 1))) return rc;
    int64_t total = 0;
    unsigned long long bad = 0;
    BWAMS_HIP(hipMemcpyAsync(&total, s->bm.roff.p + n_rec, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipMemcpyAsync(&bad, s->bm.bad.p, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    if (bad != ~0ULL) {
        static const char *why[] = {"", "a line that is not a SAM record BAM can hold", "a read name longer than 254 bytes",
                                    "an optional field that is not TG:T:value of type A, i, f, Z or H (a copied FASTQ comment?)",
                                    "an integer field outside int32 / uint32", "more than 65535 CIGAR operations", "SEQ and QUAL of different lengths"};
        const unsigned r = (unsigned)(bad & 0xFF);
        set_last_error("bwams_bam_run: read " + std::to_string(bad >> 8) + ": " + (r < 7 ? why[r] : "?"));
        return BWAMS_ERR_UNSUPPORTED;
    }
    BWAMS_HIP(s->bm.out.ensure_n((size_t)total + 16));
    A.out = s->bm.out.p;
    launch_bam_write(A, s->bm.off.p, b->cu_count, st);
    BWAMS_HIP(hipGetLastError());
    BWAMS_HIP(hipStreamSynchronize(st));
    s->bm.bytes = total; s->bm.nrec = n_rec; s->bm.nseq = nseq;
    if (bam_bytes) *bam_bytes = total;
    if (n_records) *n_records = n_rec;
    produced(b, Product::bam);
    return BWAMS_OK;
}

int bwams_bam_fetch(bwams_batch_t *b, void *bam, int64_t cap, int64_t *read_off) {
    if (!has(b, Product::bam)) {
        set_last_error("bwams_bam_fetch: run bwams_bam_run first");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    if (bam && s->bm.bytes > cap) return BWAMS_ERR_CAPACITY;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    if (bam && s->bm.bytes) BWAMS_HIP(hipMemcpyAsync(bam, s->bm.out.p, (size_t)s->bm.bytes, hipMemcpyDeviceToHost, st));
    if (read_off) BWAMS_HIP(hipMemcpyAsync(read_off, s->bm.off.p, (size_t)(s->bm.nseq + 1) * 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    return BWAMS_OK;
}

int bwams_bam_fetch_bgzf(bwams_batch_t *b, bwams_deflater_t *d, void *out, int64_t cap, int32_t flags, int64_t *n_out) {
    if (!d || !has(b, Product::bam)) {
        set_last_error("bwams_bam_fetch_bgzf: run bwams_bam_run first");
        return BWAMS_ERR_ARG;
    }
    if (deflater_device(d) != b->idx->device) {
        set_last_error("bwams_bam_fetch_bgzf: the deflater is on device " + std::to_string(deflater_device(d)) + ", the batch on device " +
                       std::to_string(b->idx->device));
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    return deflater_run_after(d, b->stream, s->bm.out.p, s->bm.bytes, 1, out, cap, 0, flags, n_out, nullptr);
}

/* ------------------------------------------------------------ BAM coordinate sort (bam_sort.hip) ---- */

int bwams_bam_upload(bwams_batch_t *b, const void *bam, int64_t n_bytes, int64_t *n_records) {
    if (!b || n_bytes < 0 || (n_bytes && !bam)) {
        set_last_error("bwams_bam_upload: a batch and host records are required");
        return BWAMS_ERR_ARG;
    }
    std::vector<int64_t> off;
    int32_t max_rid = -1;
    if (int rc = bam_record_offsets("bwams_bam_upload", bam, n_bytes, &off, &max_rid)) return rc;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    StageState *s;
    int rc = get_state(b, &s);
    if (rc) return rc;
    hipStream_t st = b->stream;
    const int64_t n_rec = (int64_t)off.size() - 1;
    outdated(b, Product::bam);
    BWAMS_HIP(hipStreamSynchronize(st));                     // the buffers below may still be read by queued work
    BWAMS_HIP(s->bm.out.ensure_n((size_t)n_bytes + 16)); BWAMS_HIP(s->bm.roff.ensure_n((size_t)(n_rec + 1)));
    BWAMS_HIP(s->bm.off.ensure_n((size_t)(n_rec + 1)));
    if (n_bytes) BWAMS_HIP(hipMemcpyAsync(s->bm.out.p, bam, (size_t)n_bytes, hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipMemcpyAsync(s->bm.roff.p, off.data(), (size_t)(n_rec + 1) * 8, hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipMemcpyAsync(s->bm.off.p, off.data(), (size_t)(n_rec + 1) * 8, hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    s->bm.bytes = n_bytes; s->bm.nrec = n_rec; s->bm.nseq = n_rec; s->bm.nref = (uint32_t)(max_rid + 1);
    if (n_records) *n_records = n_rec;
    produced(b, Product::bam);
    return BWAMS_OK;
}

int bwams_bam_sort(bwams_batch_t *b, int64_t *n_records) {
    if (!has(b, Product::bam)) {
        set_last_error("bwams_bam_sort: run bwams_bam_run or bwams_bam_upload first");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    if (has(b, Product::sorted)) {
        if (n_records) *n_records = s->bs.nrec;
        return BWAMS_OK;
    }
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    const int64_t n = s->bm.nrec;
    if (n > 0xFFFFFFFFLL) {
        set_last_error("bwams_bam_sort: more than 2^32 records");
        return BWAMS_ERR_UNSUPPORTED;
    }
    BWAMS_HIP(s->bs.out.ensure_n((size_t)s->bm.bytes + 16)); BWAMS_HIP(s->bs.coord.ensure_n((size_t)(n + 1)));
    BWAMS_HIP(s->bs.coord0.ensure_n((size_t)(n + 1))); BWAMS_HIP(s->bs.keys.ensure_n((size_t)(n + 1)));
    BWAMS_HIP(s->bs.keys2.ensure_n((size_t)(n + 1))); BWAMS_HIP(s->bs.idx.ensure_n((size_t)(n + 1))); BWAMS_HIP(s->bs.idx2.ensure_n((size_t)(n + 1)));
    BWAMS_HIP(s->bs.size.ensure_n((size_t)(n + 1))); BWAMS_HIP(s->bs.off.ensure_n((size_t)(n + 1)));
    if (n > 0) {
        const uint8_t *src = s->bm.out.p;
        const int64_t *roff = s->bm.roff.p;
        launch_bam_sort_keys(src, roff, n, s->bm.nref, s->bs.coord0.p, s->bs.keys.p, s->bs.idx.p, b->cu_count, st);
        const unsigned bits = (unsigned)bam_sort_bits(s->bm.nref);
        if (int rc = with_tmp(b, "bwams_bam_sort: radix_sort_pairs", [&](void *tmp, size_t &tb) {
                return rocprim::radix_sort_pairs(tmp, tb, s->bs.keys.p, s->bs.keys2.p, s->bs.idx.p, s->bs.idx2.p, (size_t)n, 0u, bits, st);
            })) return rc;
        const uint32_t *idx = s->bs.idx2.p;
        BWAMS_HIP(hipMemsetAsync(s->bs.size.p + n, 0, 8, st));
        launch_bam_sort_permute(s->bs.coord0.p, idx, n, s->bs.coord.p, s->bs.size.p, b->cu_count, st);
        if (int rc = scan_rows(b, s->bs.size.p, s->bs.off.p, 1, n + 1)) return rc;
        launch_bam_sort_gather(src, roff, idx, s->bs.off.p, n, s->bs.out.p, b->cu_count, st);
        BWAMS_HIP(hipGetLastError());
    }
    BWAMS_HIP(hipStreamSynchronize(st));
    s->bs.bytes = s->bm.bytes; s->bs.nrec = n;
    if (n_records) *n_records = n;
    produced(b, Product::sorted);
    return BWAMS_OK;
}

int bwams_bam_sorted_fetch(bwams_batch_t *b, void *bam, int64_t cap, bwams_bam_coord_t *coords) {
    if (!has(b, Product::bam, Product::sorted)) {
        set_last_error("bwams_bam_sorted_fetch: run bwams_bam_sort first");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    if (bam && s->bs.bytes > cap) return BWAMS_ERR_CAPACITY;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    if (bam && s->bs.bytes) BWAMS_HIP(hipMemcpyAsync(bam, s->bs.out.p, (size_t)s->bs.bytes, hipMemcpyDeviceToHost, st));
    if (coords && s->bs.nrec)
        BWAMS_HIP(hipMemcpyAsync(coords, s->bs.coord.p, (size_t)s->bs.nrec * sizeof(bwams_bam_coord_t), hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    return BWAMS_OK;
}

/* ------------------------------------------------------------ duplicate marking (markdup.hip) ---- */

int bwams_bam_templates(bwams_batch_t *b, int64_t *n_templates, int64_t *n_ends) {
    if (!has(b, Product::bam)) {
        set_last_error("bwams_bam_templates: run bwams_bam_run or bwams_bam_upload first");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    if (!has(b, Product::templates)) {                       // (and so no template_locs either: they go when the templates go)
        if (s->bm.nrec > 0xFFFFFFFFLL) {
            set_last_error("bwams_bam_templates: more than 2^32 - 1 records");
            return BWAMS_ERR_UNSUPPORTED;
        }
        BWAMS_HIP(hipSetDevice(b->idx->device));
        BWAMS_HIP(hipStreamSynchronize(b->stream));          // the buffers below may still be read by queued work
        if (int rc = md_templates(s->md.t, s->bm.out.p, s->bm.roff.p, s->bm.nrec, b->cu_count, b->stream)) return rc;
        produced(b, Product::templates);
    }
    if (n_templates) *n_templates = s->md.t.n_t;
    if (n_ends) *n_ends = s->md.t.n_e;
    return BWAMS_OK;
}

int bwams_bam_templates_fetch(bwams_batch_t *b, bwams_dup_end_t *ends, int64_t cap, uint32_t *rec_tmpl, int32_t sorted) {
    if (!has(b, Product::bam, Product::templates) || (sorted && !has(b, Product::sorted))) {
        set_last_error("bwams_bam_templates_fetch: run bwams_bam_templates (and bwams_bam_sort for sorted = 1) on the current records first");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    if (ends && s->md.t.n_e > cap) return BWAMS_ERR_CAPACITY;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    const int64_t n = s->bm.nrec;
    if (ends && s->md.t.n_e)
        BWAMS_HIP(hipMemcpyAsync(ends, s->md.t.ends.p, (size_t)s->md.t.n_e * sizeof(bwams_dup_end_t), hipMemcpyDeviceToHost, st));
    if (rec_tmpl && n) {
        const uint32_t *src = s->md.t.rtmpl.as<const uint32_t>();
        if (sorted) {
            BWAMS_HIP(s->md.sorted.ensure_n((size_t)n));
            launch_md_gather32(src, s->bs.idx2.p, n, s->md.sorted.p, b->cu_count, st);
            src = s->md.sorted.p;
        }
        BWAMS_HIP(hipMemcpyAsync(rec_tmpl, src, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    }
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    return BWAMS_OK;
}

static int decide_host(int device, const bwams_dup_end_t *ends, const bwams_dup_loc_t *loc, int64_t n_ends, int64_t n_templates,
                       int64_t n_lib, const bwams_dup_opt_t *opt, uint8_t *dup, uint8_t *optical, bwams_dup_lib_stats_t *lib_stats,
                       int64_t cnt[3]) {
    int64_t d = 0, max_set = 0;
    if (n_ends < 0 || n_templates < 0 || (n_ends && !ends) || (n_templates && !dup)) {
        set_last_error("bwams_dup_decide: host ends and a dup array of n_templates bytes are required");
        return BWAMS_ERR_ARG;
    }
    if (n_lib < 1 || n_lib > 0x7FFFFFFF || !dup_opt_values(opt, &d, &max_set)) {
        set_last_error("bwams_dup_decide: n_lib >= 1, optical_distance >= 0 and max_optical_set >= 0 are required");
        return BWAMS_ERR_ARG;
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
        set_last_error("bwams_dup_decide: no device " + std::to_string(device));
        return BWAMS_ERR_DEVICE;
    }
    BWAMS_HIP(hipSetDevice(device));
    int cus = 0;
    BWAMS_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    hipStream_t q = nullptr;
    BWAMS_HIP(hipStreamCreateWithFlags(&q, hipStreamNonBlocking));
    struct StreamGuard { hipStream_t q; ~StreamGuard() { (void)hipStreamDestroy(q); } } guard{q};
    MdDecide w;
    DevBuf<bwams_dup_end_t> d_ends;
    DevBuf<bwams_dup_loc_t> d_loc;
    DevBuf<uint8_t> d_dup, d_opt;
    DevBuf<unsigned long long> d_cnt;
    BWAMS_HIP(d_ends.alloc((size_t)std::max<int64_t>(n_ends, 1) * sizeof(bwams_dup_end_t)));
    BWAMS_HIP(d_dup.alloc((size_t)std::max<int64_t>(n_templates, 1)));
    if (n_ends) BWAMS_HIP(hipMemcpyAsync(d_ends.p, ends, (size_t)n_ends * sizeof(bwams_dup_end_t), hipMemcpyHostToDevice, q));
    MdDecideMore more{nullptr, (int32_t)n_lib, d, max_set, nullptr, nullptr};
    const bool any_more = loc || lib_stats;
    if (loc && n_ends) {
        BWAMS_HIP(d_loc.alloc((size_t)n_ends * sizeof(bwams_dup_loc_t)));
        BWAMS_HIP(hipMemcpyAsync(d_loc.p, loc, (size_t)n_ends * sizeof(bwams_dup_loc_t), hipMemcpyHostToDevice, q));
        more.loc = d_loc.p;
        if (d > 0 && n_templates) {
            BWAMS_HIP(d_opt.alloc((size_t)n_templates));
            BWAMS_HIP(hipMemsetAsync(d_opt.p, 0, (size_t)n_templates, q));
            more.optical = d_opt.p;
        }
    }
    if (lib_stats) {
        BWAMS_HIP(d_cnt.alloc((size_t)n_lib * 7 * 8));
        BWAMS_HIP(hipMemsetAsync(d_cnt.p, 0, (size_t)n_lib * 7 * 8, q));
        more.lib_counts = d_cnt.p;
    }
    if (int rc = md_decide(w, d_ends.p, n_ends, n_templates, d_dup.p, cnt, cus, q, any_more ? &more : nullptr)) {
        (void)hipStreamSynchronize(q);
        return rc;
    }
    if (n_templates) BWAMS_HIP(hipMemcpyAsync(dup, d_dup.p, (size_t)n_templates, hipMemcpyDeviceToHost, q));
    if (optical && n_templates) {
        if (more.optical) BWAMS_HIP(hipMemcpyAsync(optical, d_opt.p, (size_t)n_templates, hipMemcpyDeviceToHost, q));
        else memset(optical, 0, (size_t)n_templates);
    }
    std::vector<unsigned long long> c;
    if (lib_stats) {
        c.resize((size_t)n_lib * 7);
        BWAMS_HIP(hipMemcpyAsync(c.data(), d_cnt.p, c.size() * 8, hipMemcpyDeviceToHost, q));
    }
    BWAMS_HIP(hipStreamSynchronize(q));
    if (lib_stats) lib_rows(lib_stats, n_lib, c.data());
    return BWAMS_OK;
}

int bwams_dup_decide(int device, const bwams_dup_end_t *ends, int64_t n_ends, int64_t n_templates, uint8_t *dup, bwams_dup_stats_t *st) {
    const auto t0 = std::chrono::steady_clock::now();
    int64_t cnt[3] = {0, 0, 0};
    if (int rc = decide_host(device, ends, nullptr, n_ends, n_templates, 1, nullptr, dup, nullptr, nullptr, cnt)) return rc;
    if (st) dup_stats(st, n_templates, n_ends, cnt, std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return BWAMS_OK;
}

int bwams_dup_decide2(int device, const bwams_dup_end_t *ends, const bwams_dup_loc_t *loc, int64_t n_ends, int64_t n_templates,
                      int64_t n_lib, const bwams_dup_opt_t *opt, uint8_t *dup, uint8_t *optical, bwams_dup_lib_stats_t *lib_stats) {
    int64_t cnt[3] = {0, 0, 0};
    return decide_host(device, ends, loc, n_ends, n_templates, n_lib, opt, dup, optical, lib_stats, cnt);
}

// the groups table as md_loc_kernel reads it: IDs sorted by bytes, uploaded into the stage's buffers (null: no table)
static int groups_upload(StageState *s, const bwams_dup_groups_t *g, MdGroupsDev *G, hipStream_t st) {
    return bwams::groups_upload(s->md.g_ids, s->md.g_off, s->md.g_ord, s->md.g_lib, g, G, st);
}

int bwams_bam_templates2(bwams_batch_t *b, const bwams_dup_groups_t *groups, int64_t *n_templates, int64_t *n_ends) {
    if (int rc = bwams_bam_templates(b, n_templates, n_ends)) return rc;
    StageState *s = b->stages;
    outdated(b, Product::template_locs);
    BWAMS_HIP(hipSetDevice(b->idx->device));
    MdGroupsDev G;
    if (int rc = groups_upload(s, groups, &G, b->stream)) return rc;
    if (int rc = md_locs(s->md.t, s->bm.out.p, s->bm.roff.p, s->bm.nrec, G, b->cu_count, b->stream)) return rc;
    s->md.n_lib = G.n_lib;
    produced(b, Product::template_locs);
    return BWAMS_OK;
}

int bwams_bam_templates_fetch_loc(bwams_batch_t *b, bwams_dup_loc_t *loc, int64_t cap) {
    if (!has(b, Product::bam, Product::templates, Product::template_locs)) {
        set_last_error("bwams_bam_templates_fetch_loc: run bwams_bam_templates2 on the current records first");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    if (loc && s->md.t.n_e > cap) return BWAMS_ERR_CAPACITY;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    if (loc && s->md.t.n_e)
        BWAMS_HIP(hipMemcpyAsync(loc, s->md.t.locs.p, (size_t)s->md.t.n_e * sizeof(bwams_dup_loc_t), hipMemcpyDeviceToHost, b->stream));
    BWAMS_HIP(hipStreamSynchronize(b->stream));
    return BWAMS_OK;
}

int bwams_bam_lib_record_counts(bwams_batch_t *b, int64_t *secondary_or_supplementary, int64_t *unmapped, int64_t cap_lib) {
    if (!has(b, Product::bam, Product::templates)) {
        set_last_error("bwams_bam_lib_record_counts: run bwams_bam_templates or _templates2 on the current records first");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    const bool locs = has(b, Product::template_locs);
    const int64_t n_lib = locs ? s->md.n_lib : 1;
    if (cap_lib < n_lib) return BWAMS_ERR_CAPACITY;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t q = b->stream;
    BWAMS_HIP(s->md.lib_counts.ensure_n((size_t)n_lib * 7));
    BWAMS_HIP(hipMemsetAsync(s->md.lib_counts.p, 0, (size_t)n_lib * 7 * 8, q));
    launch_md_lib_recs(s->md.t, s->bm.nrec, locs && s->md.t.n_t ? s->md.t.tloc.as<const bwams_dup_loc_t>() : nullptr,
                       (int)n_lib, s->md.lib_counts.p, b->cu_count, q);
    std::vector<unsigned long long> c((size_t)n_lib * 7);
    BWAMS_HIP(hipMemcpyAsync(c.data(), s->md.lib_counts.p, c.size() * 8, hipMemcpyDeviceToHost, q));
    BWAMS_HIP(hipStreamSynchronize(q));
    BWAMS_HIP(hipGetLastError());
    for (int64_t k = 0; k < n_lib; ++k) {
        if (secondary_or_supplementary) secondary_or_supplementary[k] = (int64_t)c[(size_t)k * 7 + 5];
        if (unmapped) unmapped[k] = (int64_t)c[(size_t)k * 7 + 6];
    }
    return BWAMS_OK;
}

int bwams_bam_markdup2(bwams_batch_t *b, const bwams_dup_groups_t *groups, const bwams_dup_opt_t *opt, bwams_dup_stats_t *st,
                       bwams_dup_lib_stats_t *lib_stats, int64_t cap_lib) {
    int64_t n_t = 0, n_e = 0, d = 0, max_set = 0;
    if (!dup_opt_values(opt, &d, &max_set)) {
        set_last_error("bwams_bam_markdup2: optical_distance >= 0 and max_optical_set >= 0 are required");
        return BWAMS_ERR_ARG;
    }
    const int64_t n_lib = groups ? (int64_t)groups->libs.size() : 1;
    if (lib_stats && cap_lib < n_lib) return BWAMS_ERR_CAPACITY;
    const bool locs = groups || d > 0;                       // without either: one library, no location, and bwams_bam_markdup's kernels
    if (int rc = locs ? bwams_bam_templates2(b, groups, &n_t, &n_e) : bwams_bam_templates(b, &n_t, &n_e)) return rc;
    StageState *s = b->stages;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t q = b->stream;
    const auto t0 = std::chrono::steady_clock::now();
    BWAMS_HIP(s->md.dup.ensure_n((size_t)std::max<int64_t>(n_t, 1))); BWAMS_HIP(s->md.cnt.ensure_n(2));
    MdDecideMore more{locs && n_e ? s->md.t.locs.as<const bwams_dup_loc_t>() : nullptr, (int32_t)n_lib, d, max_set, nullptr, nullptr};
    if (more.loc && d > 0) {
        BWAMS_HIP(s->md.optical.ensure_n((size_t)std::max<int64_t>(n_t, 1)));
        BWAMS_HIP(hipMemsetAsync(s->md.optical.p, 0, (size_t)n_t, q));
        more.optical = s->md.optical.p;
    }
    if (lib_stats) {
        BWAMS_HIP(s->md.lib_counts.ensure_n((size_t)n_lib * 7));
        BWAMS_HIP(hipMemsetAsync(s->md.lib_counts.p, 0, (size_t)n_lib * 7 * 8, q));
        more.lib_counts = s->md.lib_counts.p;
    }
    int64_t cnt[3] = {0, 0, 0};
    if (int rc = md_decide(s->md.decide, s->md.t.ends.as<const bwams_dup_end_t>(), n_e, n_t, s->md.dup.p, cnt, b->cu_count, q,
                           more.loc || lib_stats ? &more : nullptr))
        return rc;
    const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    unsigned long long *marked = s->md.cnt.p;
    BWAMS_HIP(hipMemsetAsync(marked, 0, 16, q));
    const int64_t n = s->bm.nrec;
    const uint32_t *rt = s->md.t.rtmpl.as<const uint32_t>();
    const uint8_t *dup = s->md.dup.p;
    launch_md_apply(s->bm.out.p, s->bm.roff.p, nullptr, rt, dup, n, marked, b->cu_count, q);
    if (has(b, Product::sorted))                             // the sorted copy: record i is the unsorted record bs.idx2[i]
        launch_md_apply(s->bs.out.p, s->bs.off.p, s->bs.idx2.p, rt, dup, n, marked + 1, b->cu_count, q);
    std::vector<unsigned long long> c;
    if (lib_stats) {
        launch_md_lib_recs(s->md.t, n, locs && n_t ? s->md.t.tloc.as<const bwams_dup_loc_t>() : nullptr, (int)n_lib, more.lib_counts,
                           b->cu_count, q);
        c.resize((size_t)n_lib * 7);
        BWAMS_HIP(hipMemcpyAsync(c.data(), more.lib_counts, c.size() * 8, hipMemcpyDeviceToHost, q));
    }
    unsigned long long h[2] = {0, 0};
    BWAMS_HIP(hipMemcpyAsync(h, marked, 16, hipMemcpyDeviceToHost, q));
    BWAMS_HIP(hipStreamSynchronize(q));
    BWAMS_HIP(hipGetLastError());
    if (lib_stats) lib_rows(lib_stats, n_lib, c.data());
    if (st) {
        dup_stats(st, n_t, n_e, cnt, ms);
        st->records_marked = (int64_t)h[0];
    }
    return BWAMS_OK;
}

int bwams_bam_markdup(bwams_batch_t *b, bwams_dup_stats_t *st) { return bwams_bam_markdup2(b, nullptr, nullptr, st, nullptr, 0); }
}  // extern "C"
