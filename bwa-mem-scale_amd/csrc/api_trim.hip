// api_trim.hip — read trimming and FASTQ text of a decoded chunk through the public C-ABI (include/bwams.h): bwams_trim_opt_default,
// bwams_fastq_trim, bwams_fastq_text and bwams_fastq_text_fetch.  The kernels are trim.hip's.
#include <cstring>
#include <memory>
#include <rocprim/rocprim.hpp>

#include "common.h"

using namespace bwams;

namespace {

int refuse(const char *field, const char *why) {
    set_last_error(std::string("bwams_fastq_trim: ") + field + ": " + why);
    return BWAMS_ERR_ARG;
}

// T9 over the options; the adapters' bit planes on the way
int check_options(const bwams_trim_opt_t &o, TrimParams *P) {
    struct { const char *name; int32_t v, min, max; } f[] = {
        {"trim_front", o.trim_front, 0, INT32_MAX}, {"trim_tail", o.trim_tail, 0, INT32_MAX}, {"cut_window", o.cut_window, 1, 64},
        {"cut_quality", o.cut_quality, 0, INT32_MAX}, {"overlap_min", o.overlap_min, 1, INT32_MAX},
        {"overlap_max_diff", o.overlap_max_diff, 0, INT32_MAX}, {"overlap_diff_pct", o.overlap_diff_pct, 0, INT32_MAX},
        {"adapter_min_match", o.adapter_min_match, 1, INT32_MAX}, {"adapter_mismatch_per", o.adapter_mismatch_per, 1, INT32_MAX},
        {"max_len", o.max_len, 0, INT32_MAX}, {"min_len", o.min_len, 1, INT32_MAX}, {"n_limit", o.n_limit, 0, INT32_MAX},
        {"qual_floor", o.qual_floor, 0, INT32_MAX}, {"low_qual_pct", o.low_qual_pct, 0, INT32_MAX},
    };
    for (const auto &x : f)
        if (x.v < x.min || x.v > x.max) return refuse(x.name, "outside its range");
    *P = TrimParams{o.trim_front, o.trim_tail, o.cut_front, o.cut_tail, o.cut_window, o.cut_quality, o.overlap, o.overlap_min,
                    o.overlap_max_diff, o.overlap_diff_pct, o.adapter_min_match, o.adapter_mismatch_per, o.max_len, o.min_len, o.n_limit,
                    o.qual_floor, o.low_qual_pct, 0, 0, {0, 0}, {{0, 0}, {0, 0}}, {{0, 0}, {0, 0}}};
    const char *ad[2] = {o.adapter1, o.adapter2};
    const char *names[2] = {"adapter1", "adapter2"};
    for (int w = 0; w < 2; ++w) {
        const void *nul = memchr(ad[w], 0, 129);
        if (!nul) return refuse(names[w], "no NUL within its 129 bytes");
        const int m = (int)((const char *)nul - ad[w]);
        for (int k = 0; k < m; ++k) {
            const char *at = strchr("ACGT", ad[w][k]);
            if (!at) return refuse(names[w], "a letter other than A, C, G, T");
            const unsigned long long code = (unsigned long long)(at - "ACGT");
            P->a_lo[w][k >> 6] |= (code & 1) << (k & 63);
            P->a_hi[w][k >> 6] |= (code >> 1) << (k & 63);
        }
        P->a_len[w] = m;
    }
    return BWAMS_OK;
}

// T8: every number from the report and the input lengths
void fill_stats(const std::vector<bwams_trim_read_t> &rep, const bwams_fastq *in, int paired, bwams_trim_stats_t *s) {
    memset(s, 0, sizeof *s);
    s->reads_in = in->n_reads; s->bases_in = in->n_bases;
    for (size_t i = 0; i < rep.size(); ++i) {
        const bwams_trim_read_t &r = rep[i];
        if (r.reason == BWAMS_TRIM_KEPT) { ++s->reads_out; s->bases_out += r.len; }
        else ++s->dropped[r.reason - 1];
        for (int k = 0; k < BWAMS_TRIM_N_STEPS; ++k)
            if (r.removed[k] > 0) { ++s->step_reads[k]; s->step_bases[k] += r.removed[k]; }
        if (paired && !(i & 1)) {
            if (r.insert > 0) ++s->pairs_insert;
            if (r.steps & BWAMS_TRIM_STEP_SKIPPED) ++s->pairs_skipped;
        }
    }
}

// the three offset arrays of f in device memory, back to back: name_off, comment_off, cum (n + 1 entries each)
int upload_offsets(const bwams_fastq *f, DevBuf<int64_t> *d, hipStream_t st) {
    const size_t n1 = (size_t)f->n_reads + 1;
    BWAMS_HIP(d->alloc(3 * n1 * 8));
    BWAMS_HIP(hipMemcpyAsync(d->p, f->name_off.data(), n1 * 8, hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipMemcpyAsync(d->p + n1, f->comment_off.data(), n1 * 8, hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipMemcpyAsync(d->p + 2 * n1, f->cum.data(), n1 * 8, hipMemcpyHostToDevice, st));
    return BWAMS_OK;
}

TrimArrays arrays_of(bwams_fastq *f, const int64_t *d_offs) {
    const int64_t n1 = f->n_reads + 1;
    return TrimArrays{f->d_enc.p, f->has_qual ? f->d_qual.p : nullptr, f->d_names.p, f->d_comments.p, d_offs ? d_offs + 2 * n1 : nullptr, d_offs,
                      d_offs ? d_offs + n1 : nullptr};
}

struct Events {                       // destroyed on every way out
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

}  // namespace

extern "C" {

int bwams_trim_opt_default(bwams_trim_opt_t *o) {
    if (!o) return BWAMS_ERR_ARG;
    memset(o, 0, sizeof *o);
    o->cut_tail = 1; o->cut_window = 4; o->cut_quality = 20;
    o->overlap = 1; o->overlap_min = 30; o->overlap_max_diff = 5; o->overlap_diff_pct = 20;
    o->adapter_min_match = 4; o->adapter_mismatch_per = 8;
    o->min_len = 15; o->n_limit = 5; o->qual_floor = 15; o->low_qual_pct = 40;
    return BWAMS_OK;
}

int bwams_fastq_trim(bwams_fastq_t *in, const bwams_trim_opt_t *opt, int32_t paired, bwams_fastq_t **out, bwams_trim_read_t *report,
                     bwams_trim_stats_t *stats) {
    if (out) *out = nullptr;
    if (!in || !opt || !out) {
        set_last_error("bwams_fastq_trim: a chunk, options and a place for the new chunk are required");
        return BWAMS_ERR_ARG;
    }
    TrimParams P;
    if (int rc = check_options(*opt, &P)) return rc;
    if (paired && (in->n_reads & 1)) return refuse("paired", "a paired-end chunk holds an even number of reads (ends interleaved)");
    P.paired = paired ? 1 : 0;
    P.has_qual = in->has_qual ? 1 : 0;
    const int64_t n = in->n_reads, n1 = n + 1;
    BWAMS_HIP(hipSetDevice(in->device));
    hipStream_t st = nullptr;
    Events evs;
    for (hipEvent_t &x : evs.e) BWAMS_HIP(hipEventCreate(&x));
    std::unique_ptr<bwams_fastq> g(new bwams_fastq());
    g->device = in->device; g->has_qual = in->has_qual;
    DevBuf<int64_t> d_in_off, wide, offs;
    DevBuf<bwams_trim_read_t> d_rep;
    DevBuf<> scan_tmp;
    if (int rc = upload_offsets(in, &d_in_off, st)) return rc;
    BWAMS_HIP(d_rep.alloc((size_t)n1 * sizeof(bwams_trim_read_t)));
    BWAMS_HIP(wide.alloc((size_t)n1 * 3 * 8));
    BWAMS_HIP(offs.alloc((size_t)n1 * 3 * 8));
    const TrimArrays A = arrays_of(in, d_in_off.p);
    BWAMS_HIP(hipEventRecord(evs.e[0], st));
    // (1) T1 to T7, a wave per read or pair; (2) what every read brings, and where it goes
    launch_trim_reads(in->d_enc.p, in->d_qual.p, A.cum, n, P, d_rep.p, st);
    launch_trim_widths(d_rep.p, A.name_off, A.comment_off, n, wide.p, st);
    size_t tb = 0;
    BWAMS_HIP(rocprim::exclusive_scan(nullptr, tb, wide.p, offs.p, (int64_t)0, (size_t)n1, rocprim::plus<int64_t>(), st));
    BWAMS_HIP(scan_tmp.alloc(tb + 16));
    for (int row = 0; row < 3; ++row)
        BWAMS_HIP(rocprim::exclusive_scan(scan_tmp.p, tb, wide.p + row * n1, offs.p + row * n1, (int64_t)0, (size_t)n1, rocprim::plus<int64_t>(), st));
    BWAMS_HIP(hipEventRecord(evs.e[1], st));
    // the one report that comes back: the new chunk's host offset arrays and the stats are filled from it
    std::vector<bwams_trim_read_t> rep((size_t)n);
    if (n) BWAMS_HIP(hipMemcpyAsync(rep.data(), d_rep.p, (size_t)n * sizeof(bwams_trim_read_t), hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    g->cum.reserve((size_t)n1); g->name_off.reserve((size_t)n1); g->comment_off.reserve((size_t)n1);
    g->cum.assign(1, 0); g->name_off.assign(1, 0); g->comment_off.assign(1, 0);
    for (int64_t i = 0; i < n; ++i) {
        if (rep[(size_t)i].reason != BWAMS_TRIM_KEPT) continue;
        g->cum.push_back(g->cum.back() + rep[(size_t)i].len);
        g->name_off.push_back(g->name_off.back() + (in->name_off[(size_t)i + 1] - in->name_off[(size_t)i]));
        g->comment_off.push_back(g->comment_off.back() + (in->comment_off[(size_t)i + 1] - in->comment_off[(size_t)i]));
    }
    g->n_reads = (int64_t)g->cum.size() - 1;
    g->n_bases = g->cum.back(); g->name_bytes = g->name_off.back(); g->comment_bytes = g->comment_off.back();
    // (3) one gather into the new chunk
    BWAMS_HIP(g->d_enc.alloc((size_t)g->n_bases + 64));
    BWAMS_HIP(g->d_qual.alloc((size_t)g->n_bases + 64));
    BWAMS_HIP(g->d_names.alloc((size_t)g->name_bytes + 64));
    BWAMS_HIP(g->d_comments.alloc((size_t)g->comment_bytes + 64));
    BWAMS_HIP(hipEventRecord(evs.e[2], st));
    launch_trim_gather(d_rep.p, n, A, offs.p, arrays_of(g.get(), nullptr), st);
    BWAMS_HIP(hipEventRecord(evs.e[3], st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    float ms_plan = 0, ms_gather = 0;                      // the device's time: not the report's way to the host between the two
    (void)hipEventElapsedTime(&ms_plan, evs.e[0], evs.e[1]);
    (void)hipEventElapsedTime(&ms_gather, evs.e[2], evs.e[3]);
    g->ms = ms_plan + ms_gather;
    if (report && n) memcpy(report, rep.data(), (size_t)n * sizeof(bwams_trim_read_t));
    if (stats) fill_stats(rep, in, P.paired, stats);
    *out = g.release();
    return BWAMS_OK;
}

int bwams_fastq_text(bwams_fastq_t *f, int32_t with_comment, const char **d_text, int64_t *n_bytes) {
    if (!f) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(f->device));
    hipStream_t st = nullptr;
    const int64_t n = f->n_reads, n1 = n + 1;
    f->text_bytes = -1;
    DevBuf<int64_t> d_off, wide, off;
    DevBuf<> scan_tmp;
    if (int rc = upload_offsets(f, &d_off, st)) return rc;
    BWAMS_HIP(wide.alloc((size_t)n1 * 8));
    BWAMS_HIP(off.alloc((size_t)n1 * 8));
    const TrimArrays A = arrays_of(f, d_off.p);
    launch_fastq_text_widths(A, n, with_comment ? 1 : 0, wide.p, st);
    size_t tb = 0;
    BWAMS_HIP(rocprim::exclusive_scan(nullptr, tb, wide.p, off.p, (int64_t)0, (size_t)n1, rocprim::plus<int64_t>(), st));
    BWAMS_HIP(scan_tmp.alloc(tb + 16));
    BWAMS_HIP(rocprim::exclusive_scan(scan_tmp.p, tb, wide.p, off.p, (int64_t)0, (size_t)n1, rocprim::plus<int64_t>(), st));
    int64_t total = 0;                                     // the scan's last entry (the width behind the last read is 0): the text's size
    BWAMS_HIP(hipMemcpyAsync(&total, off.p + n, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(f->d_text.alloc((size_t)total + 64));
    launch_fastq_text_emit(A, n, with_comment ? 1 : 0, off.p, f->d_text.p, st);
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    f->text_bytes = total;
    if (d_text) *d_text = f->d_text.p;
    if (n_bytes) *n_bytes = total;
    return BWAMS_OK;
}

int bwams_fastq_text_fetch(bwams_fastq_t *f, char *out, int64_t cap) {
    if (!f || f->text_bytes < 0 || (!out && f->text_bytes)) {
        set_last_error("bwams_fastq_text_fetch: a chunk with a text (bwams_fastq_text) and a buffer are required");
        return BWAMS_ERR_ARG;
    }
    if (cap < f->text_bytes) {
        set_last_error("bwams_fastq_text_fetch: the text holds " + std::to_string(f->text_bytes) + " bytes");
        return BWAMS_ERR_CAPACITY;
    }
    BWAMS_HIP(hipSetDevice(f->device));
    if (f->text_bytes) BWAMS_HIP(hipMemcpy(out, f->d_text.p, (size_t)f->text_bytes, hipMemcpyDeviceToHost));
    return BWAMS_OK;
}

}  // extern "C"
