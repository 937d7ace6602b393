// rec_consumer.h — what the handles that read BAM records on the device share (depth, pileup, QC, recalibration and its apply, duplicate marking joined by name, collating by name; host
// only, for their api_*.hip): the base of the handle structs, the three ways to the records of an add (a batch's, in HBM; host
// records, uploaded into the handle; the current piece of a BAM file read by region) with their refusals, and the timed sequences around a check kernel and around a piece's kernels.
// A base struct and free functions: each *_add stays in its own file as check, size buffers, loop over pieces.
#pragma once
#include "stage_state.h"

namespace bwams {

// The head of every such handle.  Its destructor runs after the derived struct's buffers are freed; hipFree asks for no current device.
struct RecConsumer {
    int device = 0, cu_count = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};           // around a check kernel, around a piece's kernels
    DevBuf<uint8_t> recs;                            // consumer_records: the uploaded records and their offsets
    DevBuf<int64_t> roff;
    int open(int dev) {                              // the ordinal checked and made current, then what the fields above need of it
        if (int rc = check_device(dev)) return rc;
        BWAMS_HIP(hipSetDevice(dev));
        device = dev;
        BWAMS_HIP(hipDeviceGetAttribute(&cu_count, hipDeviceAttributeMultiprocessorCount, dev));
        BWAMS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        for (hipEvent_t &e : ev) BWAMS_HIP(hipEventCreate(&e));
        return BWAMS_OK;
    }
    RecConsumer() = default;
    RecConsumer(const RecConsumer &) = delete;
    RecConsumer &operator=(const RecConsumer &) = delete;
    ~RecConsumer() {
        (void)hipSetDevice(device);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// The records of one add, on the device: n_rec of them at bam + off[r].  Not const: the apply rewrites their QUAL where they lie.
struct DevRecords {
    uint8_t *bam = nullptr;
    const int64_t *off = nullptr;
    int64_t n_rec = 0;
};

inline int consumer_refusal(const char *who, const std::string &what) {
    set_last_error(std::string(who) + ": " + what);
    return BWAMS_ERR_ARG;
}

// The current BAM records of batch b for handle c (null: refused as a missing batch is), with c's device current and what b has queued
// done, since queued work may still write them.  refuse: a text that refuses the call once the arguments are known to be there and
// before anything else is looked at (null: none).  *state: the batch's stages.
inline int consumer_batch(const RecConsumer *c, bwams_batch *b, const char *who, DevRecords *out, const char *refuse = nullptr,
                          StageState **state = nullptr) {
    if (!c || !has(b, Product::bam)) return consumer_refusal(who, "run bwams_bam_run or bwams_bam_upload first");
    if (refuse) return consumer_refusal(who, refuse);
    if (b->idx->device != c->device)
        return consumer_refusal(who, "the handle is on device " + std::to_string(c->device) + ", the batch on device " +
                                         std::to_string(b->idx->device));
    BWAMS_HIP(hipSetDevice(c->device));
    BWAMS_HIP(hipStreamSynchronize(b->stream));
    StageState *s = b->stages;
    *out = DevRecords{s->bm.out.p, s->bm.roff.p, s->bm.nrec};
    if (state) *state = s;
    return BWAMS_OK;
}

// Host records bam[0, n_bytes) for handle c: their chain checked as bwams_bam_upload checks it, then uploaded into c->recs (with the
// 16 bytes of slack behind them that a batch's record buffers have, api_bam.hip: the kernels read both alike) and their offsets into
// c->roff.  refuse: as above.
inline int consumer_records(RecConsumer *c, const void *bam, int64_t n_bytes, const char *who, DevRecords *out, const char *refuse = nullptr) {
    if (!c || n_bytes < 0 || (n_bytes && !bam)) return consumer_refusal(who, "a handle and host records are required");
    if (refuse) return consumer_refusal(who, refuse);
    std::vector<int64_t> off;
    int32_t max_rid = -1;
    if (int rc = bam_record_offsets(who, bam, n_bytes, &off, &max_rid)) return rc;
    const int64_t n_rec = (int64_t)off.size() - 1;
    BWAMS_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    BWAMS_HIP(c->recs.ensure_n((size_t)n_bytes + 16)); BWAMS_HIP(c->roff.ensure_n((size_t)n_rec + 1));
    if (n_bytes) BWAMS_HIP(hipMemcpyAsync(c->recs.p, bam, (size_t)n_bytes, hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipMemcpyAsync(c->roff.p, off.data(), (size_t)(n_rec + 1) * 8, hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipStreamSynchronize(st));                     // the host vector above ends here
    *out = DevRecords{c->recs.p, c->roff.p, n_rec};
    return BWAMS_OK;
}

// api_bam_file.hip: the current piece of f (refused with `who` and a text when it has none), the device and the stream of f
int bam_file_piece(bwams_bam_file *f, const char *who, int *device, hipStream_t *stream, DevRecords *out);

// The current piece of BAM file f for handle c (bwams_bam_file_next made it), with c's device current and what f has queued done.  The
// records lie in f and stay until its next bwams_bam_file_next or _query.  refuse: as above.
inline int consumer_file(const RecConsumer *c, bwams_bam_file *f, const char *who, DevRecords *out, const char *refuse = nullptr) {
    if (!c || !f) return consumer_refusal(who, "a handle and a BAM file are required");
    if (refuse) return consumer_refusal(who, refuse);
    int device = 0;
    hipStream_t stream = nullptr;
    if (int rc = bam_file_piece(f, who, &device, &stream, out)) return rc;
    if (device != c->device)
        return consumer_refusal(who, "the handle is on device " + std::to_string(c->device) + ", the file on device " + std::to_string(device));
    BWAMS_HIP(hipSetDevice(c->device));
    BWAMS_HIP(hipStreamSynchronize(stream));
    return BWAMS_OK;
}

// A check kernel, timed: the `words` first-bad words at dev are set to ~0, launch() queues the kernel on c->stream, the words come
// back in h and the kernel's time in *ms.  What the words say is the caller's.
template <class Launch> int consumer_check(RecConsumer *c, unsigned long long *dev, int words, unsigned long long *h, float *ms, Launch &&launch) {
    hipStream_t st = c->stream;
    BWAMS_HIP(hipMemsetAsync(dev, 0xFF, (size_t)words * 8, st));
    BWAMS_HIP(hipEventRecord(c->ev[0], st));
    launch();
    BWAMS_HIP(hipEventRecord(c->ev[1], st));
    BWAMS_HIP(hipMemcpyAsync(h, dev, (size_t)words * 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    BWAMS_HIP(hipEventElapsedTime(ms, c->ev[0], c->ev[1]));
    return BWAMS_OK;
}

// The refusal a packed first-bad word (record << 3 | reason) stands for; why[reason] is the text behind the record's number.
inline int consumer_refuse_packed(const char *who, unsigned long long word, const char *const *why) {
    return consumer_refusal(who, "record " + std::to_string(word >> 3) + why[word & 7]);
}

// One piece of an add, timed: the `words` call words at dev are zeroed, launch() queues the piece's kernels on c->stream and returns
// BWAMS_OK or what failed, the words come back in h and the kernels' time is added to *ms.
template <class Launch> int consumer_piece(RecConsumer *c, unsigned long long *dev, int words, unsigned long long *h, float *ms, Launch &&launch) {
    hipStream_t st = c->stream;
    float t = 0;
    BWAMS_HIP(hipMemsetAsync(dev, 0, (size_t)words * 8, st));
    BWAMS_HIP(hipEventRecord(c->ev[0], st));
    if (int rc = launch()) return rc;
    BWAMS_HIP(hipEventRecord(c->ev[1], st));
    BWAMS_HIP(hipMemcpyAsync(h, dev, (size_t)words * 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    BWAMS_HIP(hipEventElapsedTime(&t, c->ev[0], c->ev[1]));
    *ms += t;
    return BWAMS_OK;
}

// Device memory for a handle's buffers: a failed allocation is BWAMS_ERR_NOMEM with the size asked for, and leaves what was there.
inline int no_memory(const char *who, size_t bytes, const char *what) {
    (void)hipGetLastError();
    set_last_error(std::string(who) + ": " + std::to_string(bytes) + " bytes of device memory for " + what + " could not be had");
    return BWAMS_ERR_NOMEM;
}

// room for n elements; what b held is not kept, and b is left as it was when the memory cannot be had
template <class T> int fresh(DevBuf<T> &b, size_t n, const char *who, const char *what) {
    const size_t bytes = n * sizeof(T);
    if (bytes <= b.cap) return BWAMS_OK;
    DevBuf<T> nb;
    const hipError_t e = nb.alloc(bytes + bytes / 8 + 4096);
    if (e == hipErrorOutOfMemory) return no_memory(who, bytes, what);
    BWAMS_HIP(e);
    b = std::move(nb);
    return BWAMS_OK;
}

// An output buffer that is too small gets a replacement in `next`; nothing of the handle changes before commit.
template <class T> struct Staged {
    DevBuf<T> *cur;
    DevBuf<T> next;
    int stage(size_t n, const char *who, const char *what) {
        const size_t bytes = n * sizeof(T);
        if (bytes <= cur->cap) return BWAMS_OK;
        const hipError_t e = next.alloc(bytes + bytes / 8 + 4096);
        if (e == hipErrorOutOfMemory) return no_memory(who, bytes, what);
        BWAMS_HIP(e);
        return BWAMS_OK;
    }
    T *p() const { return next.p ? next.p : cur->p; }
    void commit() { if (next.p) *cur = std::move(next); }
};

}  // namespace bwams
