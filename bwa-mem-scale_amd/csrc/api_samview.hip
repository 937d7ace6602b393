// api_samview.hip — C-ABI entry points of the view handle (include/bwams.h, "Viewing BAM records as SAM text"): the handle with the
// reference names on the device, the add from host records, from a batch and from a BAM file's piece (the counting pass and its scan,
// the refusal, every allocation, then the writing pass), the output, its fetch and its fetch through the deflater, over samview.hip;
// and bwams_fmt_float, fmt_g.h on the host.  An add decides everything before it writes, so a refusal leaves the handle as it was.
// No CPU fallback: every entry point but bwams_fmt_float runs HIP kernels or returns an error.
#include <cstring>
#include <memory>

#include "rec_consumer.h"
#include "fmt_g.h"

using namespace bwams;

struct bwams_samview : RecConsumer {
    bwams_samview_opt_t opt{};
    int32_t n_ref = 0;
    DevBuf<uint8_t> names;                                   // the reference names back to back, and where each starts
    DevBuf<int64_t> name_off;
    // an add's scratch, kept between adds
    DevBuf<CoPlace> size, at;
    DevBuf<uint8_t> tmp;
    DevBuf<unsigned long long> call;
    // the output of the last add
    DevBuf<uint8_t> text;
    DevBuf<int64_t> line_off;
    int64_t n_bytes = 0, n_lines = 0, n_records = 0;
    bwams_samview_info_t I{};
    hipEvent_t t[4] = {};
    ~bwams_samview() {
        (void)hipSetDevice(device);
        for (hipEvent_t e : t)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

constexpr int64_t kSlack = 16;                               // behind the text: the deflater and later readers may read whole words

const char *const kReasons[5] = {": refID or next refID outside [-1, n_ref)",
                                 ": l_read_name is 0, the name does not end in NUL, or it holds a NUL",
                                 ": a CIGAR op code above 8",
                                 ": l_seq < 0, or the name, CIGAR, SEQ and QUAL pass the record's end",
                                 ": the aux fields do not chain to the record's end"};

int sv_add(bwams_samview *v, const DevRecords &R, int64_t *n_lines, const char *who) {
    const int64_t n = R.n_rec;
    hipStream_t st = v->stream;
    const char *scratch = "an add's scratch";
    if (int rc = fresh(v->size, (size_t)n + 1, who, scratch)) return rc;
    if (int rc = fresh(v->at, (size_t)n + 1, who, scratch)) return rc;
    size_t tb = 0;
    if (int rc = co_scan_place(nullptr, tb, v->size.p, v->at.p, n + 1, st)) return rc;
    if (int rc = fresh(v->tmp, tb, who, scratch)) return rc;
    SvArgs A{};
    A.bam = R.bam; A.rec_off = R.off; A.n_rec = n;
    A.names = v->names.p; A.name_off = v->name_off.p; A.n_ref = v->n_ref;
    A.require = v->opt.flag_require; A.exclude = v->opt.flag_exclude;
    A.min_mapq = v->opt.min_mapq > 0 ? (uint32_t)v->opt.min_mapq : 0u;
    A.size = v->size.p; A.at = v->at.p; A.bad = v->call.p;
    // the counting pass: sizes, the refusal, the places
    BWAMS_HIP(hipMemsetAsync(v->call.p, 0xFF, 8, st));
    BWAMS_HIP(hipEventRecord(v->t[0], st));
    launch_samview_count(A, v->cu_count, st);
    if (int rc = co_scan_place(v->tmp.p, tb, v->size.p, v->at.p, n + 1, st)) return rc;
    BWAMS_HIP(hipEventRecord(v->t[1], st));
    unsigned long long bad = 0;
    CoPlace total{0, 0};
    BWAMS_HIP(hipMemcpyAsync(&bad, v->call.p, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipMemcpyAsync(&total, v->at.p + n, sizeof total, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    if (bad != ~0ULL) {                                      // V6: nothing was written
        (void)consumer_refuse_packed(who, bad, kReasons);
        return BWAMS_ERR_UNSUPPORTED;
    }
    // every allocation, then the writing pass; from the commit on the add happens
    Staged<uint8_t> o_text{&v->text, {}};
    Staged<int64_t> o_off{&v->line_off, {}};
    if (int rc = o_text.stage((size_t)(total.bytes + kSlack), who, "the text")) return rc;
    if (int rc = o_off.stage((size_t)(total.n + 1), who, "the lines' offsets")) return rc;
    o_text.commit(); o_off.commit();
    A.text = v->text.p; A.line_off = v->line_off.p;
    BWAMS_HIP(hipEventRecord(v->t[2], st));
    launch_samview_write(A, v->cu_count, st);
    BWAMS_HIP(hipEventRecord(v->t[3], st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    float ms_count = 0, ms_write = 0;
    BWAMS_HIP(hipEventElapsedTime(&ms_count, v->t[0], v->t[1]));
    BWAMS_HIP(hipEventElapsedTime(&ms_write, v->t[2], v->t[3]));
    v->n_bytes = total.bytes; v->n_lines = total.n; v->n_records = n;
    v->I.records += n; v->I.lines += total.n; v->I.filtered += n - total.n; v->I.bytes += total.bytes; v->I.adds += 1;
    v->I.ms_count += ms_count; v->I.ms_write += ms_write;
    if (n_lines) *n_lines = total.n;
    return BWAMS_OK;
}

// The reference names of a BAM header block, back to back without their NULs, and their n_ref + 1 offsets; false when the block is
// cut off, has the wrong magic or a negative count.
bool header_names(const uint8_t *h, int64_t n, std::string *names, std::vector<int64_t> *off) {
    auto i32 = [&](int64_t at) { int32_t x; memcpy(&x, h + at, 4); return x; };
    if (n < 12 || memcmp(h, "BAM\1", 4) != 0) return false;
    const int64_t l_text = i32(4);
    if (l_text < 0 || l_text > n - 12) return false;
    int64_t at = 8 + l_text;
    const int64_t n_ref = i32(at);
    at += 4;
    if (n_ref < 0) return false;
    off->assign(1, 0);
    for (int64_t r = 0; r < n_ref; ++r) {
        if (n - at < 4) return false;
        const int64_t l_name = i32(at);
        if (l_name < 1 || l_name > n - at - 8 || h[at + 4 + l_name - 1] != 0) return false;
        names->append(reinterpret_cast<const char *>(h + at + 4), (size_t)l_name - 1);
        off->push_back((int64_t)names->size());
        at += 8 + l_name;
    }
    return true;
}

}  // namespace

extern "C" {

int bwams_samview_open(int device, const void *bam_header, int64_t n_header, const bwams_samview_opt_t *opt, bwams_samview_t **out) {
    const char *who = "bwams_samview_open";
    if (!out || !bam_header || n_header < 0 || (opt && opt->reserved))
        return consumer_refusal(who, "out, a BAM header block and a reserved word of 0 are required");
    *out = nullptr;
    std::string names;
    std::vector<int64_t> off;
    if (!header_names(static_cast<const uint8_t *>(bam_header), n_header, &names, &off))
        return consumer_refusal(who, "the BAM header block is cut off or does not start with the magic");
    if (off.size() - 1 > 0x7FFFFFFFu) return consumer_refusal(who, "more than 2^31 - 1 references");
    std::unique_ptr<bwams_samview> v(new bwams_samview());
    if (int rc = v->open(device)) return rc;
    for (hipEvent_t &e : v->t) BWAMS_HIP(hipEventCreate(&e));
    if (opt) v->opt = *opt;
    v->n_ref = (int32_t)(off.size() - 1);
    BWAMS_HIP(v->names.alloc(names.size() + kSlack));
    BWAMS_HIP(v->name_off.alloc(off.size() * 8));
    BWAMS_HIP(v->call.alloc(8));
    BWAMS_HIP(v->line_off.alloc(8));                         // V1: empty before any add
    if (!names.empty()) BWAMS_HIP(hipMemcpy(v->names.p, names.data(), names.size(), hipMemcpyHostToDevice));
    BWAMS_HIP(hipMemcpy(v->name_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice));
    BWAMS_HIP(hipMemset(v->line_off.p, 0, 8));
    BWAMS_HIP(hipDeviceSynchronize());
    *out = v.release();
    return BWAMS_OK;
}

int bwams_samview_close(bwams_samview_t *v) {
    delete v;
    return BWAMS_OK;
}

int bwams_samview_add_records(bwams_samview_t *v, const void *bam, int64_t n_bytes, int64_t *n_lines) {
    const char *who = "bwams_samview_add_records";
    DevRecords R;
    if (int rc = consumer_records(v, bam, n_bytes, who, &R)) return rc;
    return sv_add(v, R, n_lines, who);
}

int bwams_samview_add_batch(bwams_samview_t *v, bwams_batch_t *b, int64_t *n_lines) {
    const char *who = "bwams_samview_add_batch";
    DevRecords R;
    if (int rc = consumer_batch(v, b, who, &R)) return rc;
    return sv_add(v, R, n_lines, who);
}

int bwams_samview_add_file(bwams_samview_t *v, bwams_bam_file_t *f, int64_t *n_lines) {
    const char *who = "bwams_samview_add_file";
    DevRecords R;
    if (int rc = consumer_file(v, f, who, &R)) return rc;
    return sv_add(v, R, n_lines, who);
}

int bwams_samview_out(const bwams_samview_t *v, bwams_samview_out_t *out) {
    if (!v || !out) return consumer_refusal("bwams_samview_out", "a handle and out are required");
    out->text = v->n_bytes ? reinterpret_cast<const char *>(v->text.p) : nullptr;
    out->n_bytes = v->n_bytes;
    out->line_off = v->line_off.p;
    out->n_lines = v->n_lines;
    out->n_records = v->n_records;
    return BWAMS_OK;
}

int bwams_samview_fetch(bwams_samview_t *v, char *text, int64_t cap, int64_t *line_off) {
    const char *who = "bwams_samview_fetch";
    if (!v) return consumer_refusal(who, "a handle is required");
    if (text && cap < v->n_bytes) {
        set_last_error(std::string(who) + ": " + std::to_string(v->n_bytes) + " bytes of text do not fit the capacity " + std::to_string(cap));
        return BWAMS_ERR_CAPACITY;
    }
    BWAMS_HIP(hipSetDevice(v->device));
    hipStream_t q = v->stream;
    if (text && v->n_bytes) BWAMS_HIP(hipMemcpyAsync(text, v->text.p, (size_t)v->n_bytes, hipMemcpyDeviceToHost, q));
    if (line_off) BWAMS_HIP(hipMemcpyAsync(line_off, v->line_off.p, (size_t)(v->n_lines + 1) * 8, hipMemcpyDeviceToHost, q));
    BWAMS_HIP(hipStreamSynchronize(q));
    return BWAMS_OK;
}

int bwams_samview_fetch_bgzf(bwams_samview_t *v, bwams_deflater_t *d, void *out, int64_t cap, int32_t flags, int64_t *n_out) {
    const char *who = "bwams_samview_fetch_bgzf";
    if (!v || !d) return consumer_refusal(who, "a handle and a deflater are required");
    if (deflater_device(d) != v->device)
        return consumer_refusal(who, "the deflater is on device " + std::to_string(deflater_device(d)) + ", the handle on device " +
                                         std::to_string(v->device));
    return deflater_run_after(d, v->stream, v->text.p, v->n_bytes, 1, out, cap, 0, flags, n_out, nullptr);
}

int bwams_samview_info(const bwams_samview_t *v, bwams_samview_info_t *info) {
    if (!v || !info) return BWAMS_ERR_ARG;
    *info = v->I;
    return BWAMS_OK;
}

int bwams_fmt_float(float x, char out[16], int32_t *n) {
    if (!out || !n) return BWAMS_ERR_ARG;
    uint32_t bits;
    memcpy(&bits, &x, 4);
    const Text16 t = fmt_g(bits);
    for (int k = 0; k < t.n; ++k) out[k] = (char)t.at(k);
    out[t.n] = 0;
    *n = t.n;
    return BWAMS_OK;
}

}  // extern "C"
