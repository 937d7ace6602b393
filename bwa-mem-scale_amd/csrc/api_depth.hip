// api_depth.hip — C-ABI entry points of the depth of coverage (include/bwams.h, "Depth of coverage"): the handle, the adds from a
// batch and from host records, the scan that finishes it, and the queries, over depth.hip; the text over host/depth_text.cpp.
// No CPU fallback: every entry point runs HIP kernels or returns an error.
#include <algorithm>
#include <climits>
#include <cstring>
#include <memory>

#include <rocprim/rocprim.hpp>

#include "rec_consumer.h"
#include "../host/depth_host.h"

using namespace bwams;

struct bwams_depth : RecConsumer {
    bwams_depth_opt_t opt{};
    std::vector<int32_t> l_ref;
    std::vector<int64_t> slot_off;                   // n_ref + 1: reference r's first slot; the last is the number of slots
    DevBuf<int32_t> slots;                           // differences until finished, depths after
    DevBuf<int64_t> d_slot_off;
    DevBuf<> tmp;                                    // rocPRIM temporary storage
    DevBuf<unsigned long long> flag;                 // [0] first record with a bad op code, [1] records counted
    DevBuf<unsigned long long> hist;                 // the queries' device results, kept between calls
    DevBuf<int64_t> run_cnt;
    DevBuf<int32_t> run_start, run_depth;
    int64_t n_added = 0;                             // records given so far (rule 5)
    bool finished = false, have_rows = false;
    std::vector<bwams_depth_ref_t> rows;             // rule 7, computed at the first query that needs it
    int32_t n_ref() const { return (int32_t)l_ref.size(); }
    int64_t n_slots() const { return slot_off.back(); }
    const char *finished_text() const { return finished ? "the handle is finished (bwams_depth_reset starts it again)" : nullptr; }
};

namespace bwams {
int depth_device(const bwams_depth *d) { return d->device; }
const std::vector<int32_t> &depth_l_ref(const bwams_depth *d) { return d->l_ref; }
}  // namespace bwams

namespace {

struct IsRunStart {                                  // rule 10: position pos of [beg, end) starts a run
    const int32_t *p;                                // the reference's first slot
    int32_t beg;
    __host__ __device__ bool operator()(int32_t pos) const { return pos == beg || p[pos] != p[pos - 1]; }
};
struct RunStartCount {
    IsRunStart f;
    __host__ __device__ int64_t operator()(int32_t pos) const { return f(pos) ? 1 : 0; }
};

int query_ready(const bwams_depth *d, const char *who) {
    if (!d || !d->finished) {
        set_last_error(std::string(who) + ": a handle after bwams_depth_finish is required");
        return BWAMS_ERR_ARG;
    }
    return BWAMS_OK;
}

// check first, then add (rule 3)
int depth_add(bwams_depth *d, const DevRecords &R, int64_t *n_counted, const char *who) {
    const int64_t n_rec = R.n_rec;
    if (d->n_added + n_rec > 0x7FFFFFFFLL) {
        set_last_error(std::string(who) + ": more than 2^31 - 1 records added in total");
        return BWAMS_ERR_UNSUPPORTED;
    }
    hipStream_t st = d->stream;
    unsigned long long h[2] = {~0ULL, 0};
    if (n_rec > 0) {
        float ms = 0;                                                    // the check's time: nothing asks for it
        BWAMS_HIP(hipMemsetAsync(d->flag.p + 1, 0, 8, st));
        if (int rc = consumer_check(d, d->flag.p, 1, h, &ms, [&] { launch_depth_check(R.bam, R.off, n_rec, d->flag.p, d->cu_count, st); }))
            return rc;
        if (h[0] != ~0ULL) {
            set_last_error(std::string(who) + ": record " + std::to_string(h[0]) + " has a CIGAR op code above 8");
            return BWAMS_ERR_ARG;
        }
        launch_depth_add(R.bam, R.off, n_rec, d->opt, d->n_ref(), d->d_slot_off.p, d->slots.p, d->flag.p + 1, knobs().depth_combine,
                         d->cu_count, st);
        BWAMS_HIP(hipMemcpyAsync(h + 1, d->flag.p + 1, 8, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipStreamSynchronize(st));
        BWAMS_HIP(hipGetLastError());
    }
    d->n_added += n_rec;
    if (n_counted) *n_counted = (int64_t)h[1];
    return BWAMS_OK;
}

int depth_rows(bwams_depth *d) {                     // rule 7, once
    if (d->have_rows) return BWAMS_OK;
    const int32_t n_ref = d->n_ref();
    d->rows.assign((size_t)n_ref, bwams_depth_ref_t{});
    if (n_ref > 0) {
        hipStream_t st = d->stream;
        DevBuf<unsigned long long> sum;
        DevBuf<int32_t> mn, mx;
        BWAMS_HIP(sum.ensure_n((size_t)n_ref)); BWAMS_HIP(mn.ensure_n((size_t)n_ref)); BWAMS_HIP(mx.ensure_n((size_t)n_ref));
        BWAMS_HIP(hipMemsetAsync(sum.p, 0, (size_t)n_ref * 8, st));
        BWAMS_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(mn.p), INT_MAX, (size_t)n_ref, st));
        BWAMS_HIP(hipMemsetAsync(mx.p, 0, (size_t)n_ref * 4, st));
        launch_depth_summary(d->slots.p, d->d_slot_off.p, n_ref, d->n_slots(), sum.p, mn.p, mx.p, d->cu_count, st);
        std::vector<unsigned long long> h_sum((size_t)n_ref);
        std::vector<int32_t> h_mn((size_t)n_ref), h_mx((size_t)n_ref);
        BWAMS_HIP(hipMemcpyAsync(h_sum.data(), sum.p, (size_t)n_ref * 8, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipMemcpyAsync(h_mn.data(), mn.p, (size_t)n_ref * 4, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipMemcpyAsync(h_mx.data(), mx.p, (size_t)n_ref * 4, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipStreamSynchronize(st));
        BWAMS_HIP(hipGetLastError());
        for (int32_t r = 0; r < n_ref; ++r) {
            bwams_depth_ref_t &x = d->rows[(size_t)r];
            x.length = d->l_ref[(size_t)r];
            x.bases = (int64_t)h_sum[(size_t)r];
            x.min = x.length ? h_mn[(size_t)r] : 0;
            x.max = x.length ? h_mx[(size_t)r] : 0;
        }
    }
    d->have_rows = true;
    return BWAMS_OK;
}

int64_t window_offsets(const bwams_depth *d, int32_t w, std::vector<int64_t> *off) {      // rule 9: reference r's first window
    off->assign(d->l_ref.size() + 1, 0);
    for (size_t r = 0; r < d->l_ref.size(); ++r) (*off)[r + 1] = (*off)[r] + ((int64_t)d->l_ref[r] + w - 1) / w;
    return off->back();
}

}  // namespace

extern "C" {

int bwams_depth_open(int device, const int32_t *l_ref, int32_t n_ref, const bwams_depth_opt_t *opt, bwams_depth_t **out) {
    if (!out || n_ref < 0 || (n_ref && !l_ref) || (opt && (opt->exclude > 0xFFFFu || opt->reserved != 0))) {
        set_last_error("bwams_depth_open: n_ref >= 0 lengths, exclude within 16 bits and reserved == 0 are required");
        return BWAMS_ERR_ARG;
    }
    *out = nullptr;
    for (int32_t r = 0; r < n_ref; ++r)
        if (l_ref[r] < 0) {
            set_last_error("bwams_depth_open: reference " + std::to_string(r) + " has a negative length");
            return BWAMS_ERR_ARG;
        }
    std::unique_ptr<bwams_depth> d(new bwams_depth());
    if (int rc = d->open(device)) return rc;
    d->opt = opt ? *opt : bwams_depth_opt_t{0x704, 0, 0, 0};
    d->l_ref.assign(l_ref, l_ref + n_ref);
    d->slot_off.assign((size_t)n_ref + 1, 0);
    for (int32_t r = 0; r < n_ref; ++r) d->slot_off[(size_t)r + 1] = d->slot_off[(size_t)r] + l_ref[r] + 1;
    BWAMS_HIP(d->slots.alloc((size_t)std::max<int64_t>(d->n_slots(), 1) * 4));
    BWAMS_HIP(d->d_slot_off.alloc(((size_t)n_ref + 1) * 8));
    BWAMS_HIP(d->flag.alloc(16));
    BWAMS_HIP(hipMemsetAsync(d->slots.p, 0, (size_t)std::max<int64_t>(d->n_slots(), 1) * 4, d->stream));
    BWAMS_HIP(hipMemcpyAsync(d->d_slot_off.p, d->slot_off.data(), ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, d->stream));
    BWAMS_HIP(hipStreamSynchronize(d->stream));
    *out = d.release();
    return BWAMS_OK;
}

int bwams_depth_close(bwams_depth_t *d) {
    delete d;
    return BWAMS_OK;
}

int bwams_depth_reset(bwams_depth_t *d) {
    if (!d) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(d->device));
    BWAMS_HIP(hipMemsetAsync(d->slots.p, 0, (size_t)std::max<int64_t>(d->n_slots(), 1) * 4, d->stream));
    BWAMS_HIP(hipStreamSynchronize(d->stream));
    d->n_added = 0;
    d->finished = d->have_rows = false;
    return BWAMS_OK;
}

int bwams_depth_add_batch(bwams_depth_t *d, bwams_batch_t *b, int64_t *n_counted) {
    DevRecords R;
    if (int rc = consumer_batch(d, b, "bwams_depth_add_batch", &R, d ? d->finished_text() : nullptr)) return rc;
    return depth_add(d, R, n_counted, "bwams_depth_add_batch");
}

int bwams_depth_add_records(bwams_depth_t *d, const void *bam, int64_t n_bytes, int64_t *n_counted) {
    DevRecords R;
    if (int rc = consumer_records(d, bam, n_bytes, "bwams_depth_add_records", &R, d ? d->finished_text() : nullptr)) return rc;
    return depth_add(d, R, n_counted, "bwams_depth_add_records");
}

int bwams_depth_add_file(bwams_depth_t *d, bwams_bam_file_t *f, int64_t *n_counted) {
    DevRecords R;
    if (int rc = consumer_file(d, f, "bwams_depth_add_file", &R, d ? d->finished_text() : nullptr)) return rc;
    return depth_add(d, R, n_counted, "bwams_depth_add_file");
}

int bwams_depth_finish(bwams_depth_t *d) {
    if (!d) return BWAMS_ERR_ARG;
    if (d->finished) return BWAMS_OK;
    BWAMS_HIP(hipSetDevice(d->device));
    if (d->n_slots() > 0)
        if (int rc = with_tmp(d->tmp, d->stream, "bwams_depth_finish: inclusive_scan", [&](void *tmp, size_t &tb) {
                return rocprim::inclusive_scan(tmp, tb, d->slots.p, d->slots.p, (size_t)d->n_slots(), rocprim::plus<int32_t>(), d->stream);
            })) return rc;
    BWAMS_HIP(hipStreamSynchronize(d->stream));
    d->finished = true;
    return BWAMS_OK;
}

int bwams_depth_summary(bwams_depth_t *d, bwams_depth_ref_t *rows, int64_t cap) {
    if (int rc = query_ready(d, "bwams_depth_summary")) return rc;
    if (cap < d->n_ref() || (d->n_ref() && !rows)) return BWAMS_ERR_CAPACITY;
    BWAMS_HIP(hipSetDevice(d->device));
    if (int rc = depth_rows(d)) return rc;
    std::copy(d->rows.begin(), d->rows.end(), rows);
    return BWAMS_OK;
}

int bwams_depth_hist(bwams_depth_t *d, int32_t ref, int64_t *hist, int32_t n_bins) {
    if (int rc = query_ready(d, "bwams_depth_hist")) return rc;
    if (ref < -1 || ref >= d->n_ref() || !hist || n_bins < 2 || n_bins > (1 << 20)) {
        set_last_error("bwams_depth_hist: ref in [-1, n_ref) and 2 <= n_bins <= 2^20 are required");
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(d->device));
    hipStream_t st = d->stream;
    DevBuf<unsigned long long> &h = d->hist;
    BWAMS_HIP(h.ensure_n((size_t)n_bins));
    BWAMS_HIP(hipMemsetAsync(h.p, 0, (size_t)n_bins * 8, st));
    // all references: every slot, then the n_ref slots at l_ref[r], which hold 0 after the scan, taken out of bin 0
    const int64_t lo = ref < 0 ? 0 : d->slot_off[(size_t)ref], hi = ref < 0 ? d->n_slots() : lo + d->l_ref[(size_t)ref];
    launch_depth_hist(d->slots.p, lo, hi, n_bins, h.p, d->cu_count, st);
    BWAMS_HIP(hipMemcpyAsync(hist, h.p, (size_t)n_bins * 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    if (ref < 0) hist[0] -= d->n_ref();
    return BWAMS_OK;
}

int bwams_depth_windows(bwams_depth_t *d, int32_t w, int64_t *sums, int64_t cap, int64_t *n) {
    if (int rc = query_ready(d, "bwams_depth_windows")) return rc;
    if (w < 1) {
        set_last_error("bwams_depth_windows: w >= 1 is required");
        return BWAMS_ERR_ARG;
    }
    std::vector<int64_t> off;
    const int64_t n_win = window_offsets(d, w, &off);
    if (n) *n = n_win;
    if (!sums) return BWAMS_OK;
    if (cap < n_win) return BWAMS_ERR_CAPACITY;
    if (n_win == 0) return BWAMS_OK;
    BWAMS_HIP(hipSetDevice(d->device));
    hipStream_t st = d->stream;
    DevBuf<unsigned long long> s;
    DevBuf<int64_t> d_off;
    BWAMS_HIP(s.ensure_n((size_t)n_win)); BWAMS_HIP(d_off.ensure_n(off.size()));
    BWAMS_HIP(hipMemsetAsync(s.p, 0, (size_t)n_win * 8, st));
    BWAMS_HIP(hipMemcpyAsync(d_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, st));
    launch_depth_windows(d->slots.p, d->d_slot_off.p, d->n_ref(), d->n_slots(), d_off.p, w, s.p, d->cu_count, st);
    BWAMS_HIP(hipMemcpyAsync(sums, s.p, (size_t)n_win * 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    return BWAMS_OK;
}

int bwams_depth_runs(bwams_depth_t *d, int32_t ref, int32_t beg, int32_t end, int32_t *start, int32_t *depth, int64_t cap, int64_t *n) {
    if (int rc = query_ready(d, "bwams_depth_runs")) return rc;
    if (ref < 0 || ref >= d->n_ref() || beg < 0 || end < beg || end > d->l_ref[(size_t)ref] || (!start) != (!depth)) {
        set_last_error("bwams_depth_runs: ref in [0, n_ref), 0 <= beg <= end <= l_ref[ref], and start and depth both or neither are required");
        return BWAMS_ERR_ARG;
    }
    const int64_t len = (int64_t)end - beg;
    int64_t n_runs = 0;
    BWAMS_HIP(hipSetDevice(d->device));
    hipStream_t st = d->stream;
    const int64_t base = d->slot_off[(size_t)ref];
    const IsRunStart pred{d->slots.p + base, beg};
    rocprim::counting_iterator<int32_t> pos(beg);
    DevBuf<int64_t> &cnt = d->run_cnt;
    BWAMS_HIP(cnt.ensure_n(8));
    if (len > 0) {
        auto ones = rocprim::make_transform_iterator(pos, RunStartCount{pred});
        if (int rc = with_tmp(d->tmp, st, "bwams_depth_runs: reduce", [&](void *tmp, size_t &tb) {
                return rocprim::reduce(tmp, tb, ones, cnt.p, (int64_t)0, (size_t)len, rocprim::plus<int64_t>(), st);
            })) return rc;
        BWAMS_HIP(hipMemcpyAsync(&n_runs, cnt.p, 8, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipStreamSynchronize(st));
    }
    if (n) *n = n_runs;
    if (!start) return BWAMS_OK;
    if (cap < n_runs) return BWAMS_ERR_CAPACITY;
    if (n_runs == 0) return BWAMS_OK;
    DevBuf<int32_t> &d_start = d->run_start, &d_depth = d->run_depth;
    BWAMS_HIP(d_start.ensure_n((size_t)n_runs)); BWAMS_HIP(d_depth.ensure_n((size_t)n_runs));
    if (int rc = with_tmp(d->tmp, st, "bwams_depth_runs: select", [&](void *tmp, size_t &tb) {
            return rocprim::select(tmp, tb, pos, d_start.p, cnt.p, (size_t)len, pred, st);
        })) return rc;
    launch_depth_gather(d->slots.p, base, d_start.p, n_runs, d_depth.p, d->cu_count, st);
    BWAMS_HIP(hipMemcpyAsync(start, d_start.p, (size_t)n_runs * 4, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipMemcpyAsync(depth, d_depth.p, (size_t)n_runs * 4, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    return BWAMS_OK;
}

int bwams_depth_fetch(bwams_depth_t *d, int32_t ref, int32_t beg, int32_t end, int32_t *depth) {
    if (int rc = query_ready(d, "bwams_depth_fetch")) return rc;
    if (ref < 0 || ref >= d->n_ref() || beg < 0 || end < beg || end > d->l_ref[(size_t)ref] || (end > beg && !depth)) {
        set_last_error("bwams_depth_fetch: ref in [0, n_ref) and 0 <= beg <= end <= l_ref[ref] are required");
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(d->device));
    if (end > beg) {
        BWAMS_HIP(hipMemcpyAsync(depth, d->slots.p + d->slot_off[(size_t)ref] + beg, (size_t)(end - beg) * 4, hipMemcpyDeviceToHost, d->stream));
        BWAMS_HIP(hipStreamSynchronize(d->stream));
    }
    return BWAMS_OK;
}

int bwams_depth_text(bwams_depth_t *d, const char *names, int32_t what, int32_t arg, char *out, int64_t cap, int64_t *n) {
    if (int rc = query_ready(d, "bwams_depth_text")) return rc;
    if (!names && d->n_ref()) {
        set_last_error("bwams_depth_text: the references' names are required");
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(d->device));
    if (int rc = depth_rows(d)) return rc;
    DepthTextIn in;
    in.names = names; in.n_ref = d->n_ref(); in.rows = d->rows.data();
    std::vector<int64_t> v;
    if (what == BWAMS_DEPTH_TEXT_DIST) {
        in.n_bins = arg ? arg : 1024;
        if (in.n_bins < 2 || in.n_bins > (1 << 20)) { set_last_error("bwams_depth_text: 2 <= n_bins <= 2^20 is required"); return BWAMS_ERR_ARG; }
        v.assign(((size_t)in.n_ref + 1) * (size_t)in.n_bins, 0);
        for (int32_t r = -1; r < in.n_ref; ++r)
            if (int rc = bwams_depth_hist(d, r, v.data() + (size_t)(r + 1) * (size_t)in.n_bins, in.n_bins)) return rc;
        in.hist = v.data();
    } else if (what == BWAMS_DEPTH_TEXT_WINDOWS) {
        in.w = arg;
        int64_t n_win = 0;
        if (int rc = bwams_depth_windows(d, arg, nullptr, 0, &n_win)) return rc;
        v.assign((size_t)std::max<int64_t>(n_win, 1), 0);
        if (int rc = bwams_depth_windows(d, arg, v.data(), n_win, nullptr)) return rc;
        in.sums = v.data();
    } else if (what != BWAMS_DEPTH_TEXT_SUMMARY) {
        set_last_error("bwams_depth_text: what is BWAMS_DEPTH_TEXT_SUMMARY, _DIST or _WINDOWS");
        return BWAMS_ERR_ARG;
    }
    std::string text;
    if (int rc = depth_text_format(what, in, &text)) return rc;
    if (n) *n = (int64_t)text.size();
    if (!out || cap < (int64_t)text.size()) return BWAMS_ERR_CAPACITY;
    memcpy(out, text.data(), text.size());
    return BWAMS_OK;
}

}  // extern "C"
