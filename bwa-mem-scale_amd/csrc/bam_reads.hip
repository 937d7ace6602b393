// bam_reads.hip — BAM as read input: a buffer of BAM alignment records becomes the decoded chunk (bwams_fastq_t) that FASTQ text
// becomes in fastq.hip.  The reference reads FASTQ / FASTA only; the behaviour reproduced is `samtools fastq` (htslib's bam2fq) in
// front of `bwa mem`, with the rules written out in include/bwams.h above bwams_bam_reads_decode and restated in bwams/bam_reads.py.
//
// Record discovery: bam_discover.h (candidate filter, successors, binary lifting), shared with the region reader of bam_query.hip;
// here the chain runs from byte 0 and must end at the end of the buffer.  Its scratch is about 0.75 byte per input byte for a million
// 150-base reads.
// Behind it: br_measure_kernel, a lane per record (its offset by lifting; FLAG, lengths, the aux walk, rules 4 and 6), four exclusive
// scans, br_compact_kernel (the offsets of the kept reads), br_emit_kernel, 16 lanes per record: the packed SEQ in 4-byte loads, a
// nibble to its code by shifts of a constant, qualities, names and comments lane by lane.
// All kernels stream: the filter reads the input once (HBM bound), the emit reads ~0.8 and writes ~1.1 of it; the lifting's
// `levels` dependent 4-byte gathers per record are latency bound and small beside them.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "bam_discover.h"

namespace bwams {
namespace {

constexpr int kMaxTags = 32;

struct Tags {                                 // the listed tags, by value in the kernel arguments
    int32_t n;
    uint8_t t[2 * kMaxTags];
};

struct BrRec {                                // a record as the emit kernel reads it
    int64_t name_at, seq_at, end;             // end: one past the record
    int32_t l_name, l_seq;
    uint32_t flag;                            // FLAG | kept << 16
    int32_t pad_;
};

// ---- aux fields ----
// the field at p in [p, end): the position behind it; -1: it runs past the record, -2: a type SAMv1 does not know.  *val / *type
// receive where its value starts and its type
__device__ int64_t aux_next(const uint8_t *__restrict__ d, int64_t p, int64_t end, int64_t *val, int *type) {
    if (p + 3 > end) return -1;
    const int ty = d[p + 2];
    int64_t v = p + 3, e;
    *type = ty; *val = v;
    switch (ty) {
    case 'A': case 'c': case 'C': e = v + 1; break;
    case 's': case 'S': e = v + 2; break;
    case 'i': case 'I': case 'f': e = v + 4; break;
    case 'Z': case 'H':
        for (e = v; e < end && d[e]; ++e) {}
        if (e >= end) return -1;                                 // no NUL inside the record
        ++e;
        break;
    case 'B': {
        if (v + 5 > end) return -1;
        const int sub = d[v];
        const int64_t cnt = ld_u32(d + v + 1);
        const int sz = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
        if (!sz) return -2;
        e = v + 5 + cnt * sz;
        break;
    }
    default: return -2;
    }
    return e <= end ? e : -1;
}
// the record's first field with tag (t0, t1) in [a, end) (already validated): its value position and type, or -1
__device__ int64_t aux_find(const uint8_t *__restrict__ d, int64_t a, int64_t end, uint8_t t0, uint8_t t1, int *type) {
    while (a < end) {
        int64_t val;
        int ty;
        const int64_t nx = aux_next(d, a, end, &val, &ty);
        if (nx < 0) return -1;
        if (d[a] == t0 && d[a + 1] == t1) { *type = ty; return val; }
        a = nx;
    }
    return -1;
}
__device__ __forceinline__ int64_t aux_int(const uint8_t *__restrict__ d, int64_t v, int ty) {
    switch (ty) {
    case 'c': return (int8_t)d[v];
    case 'C': return d[v];
    case 's': return (int16_t)ld_u16(d + v);
    case 'S': return ld_u16(d + v);
    case 'i': return (int32_t)ld_u32(d + v);
    default:  return ld_u32(d + v);
    }
}
__device__ __forceinline__ int dec_len(int64_t x) {
    int l = x < 0 ? 1 : 0;
    unsigned long long u = x < 0 ? (unsigned long long)(-x) : (unsigned long long)x;
    do { ++l; u /= 10; } while (u);
    return l;
}
// bytes of "TG:T:value" for the field whose value starts at v
__device__ int aux_text_len(const uint8_t *__restrict__ d, int64_t v, int ty) {
    if (ty == 'A') return 6;
    if (ty == 'Z' || ty == 'H') { int l = 0; while (d[v + l]) ++l; return 5 + l; }
    return 5 + dec_len(aux_int(d, v, ty));
}
__device__ void aux_text_write(const uint8_t *__restrict__ d, int64_t v, int ty, uint8_t t0, uint8_t t1, char *__restrict__ out) {
    out[0] = (char)t0; out[1] = (char)t1; out[2] = ':'; out[4] = ':';
    if (ty == 'A') { out[3] = 'A'; out[5] = (char)d[v]; return; }
    if (ty == 'Z' || ty == 'H') {
        out[3] = (char)ty;
        for (int l = 0; d[v + l]; ++l) out[5 + l] = (char)d[v + l];
        return;
    }
    out[3] = 'i';
    const int64_t x = aux_int(d, v, ty);
    int l = dec_len(x);
    unsigned long long u = x < 0 ? (unsigned long long)(-x) : (unsigned long long)x;
    if (x < 0) out[5] = '-';
    do { out[5 + --l] = (char)('0' + u % 10); u /= 10; } while (u);
}

// what br_measure_kernel reports: err = min over records of (ordinal << 8 | reason); first_q / first_n = the first kept record with /
// without qualities (~0: none)
struct BrFlags {
    unsigned long long err, first_q, first_n;
};
enum { kErrLseq0 = 1, kErrMixed = 2, kErrAuxType = 3, kErrAuxBad = 4 };

// a lane per record: its offset by lifting, then FLAG, the lengths, rules 4 and 6.  wide: 4 rows of n_rec + 1 (name, comment, bases, kept)
__global__ __launch_bounds__(256) void br_measure_kernel(const uint8_t *__restrict__ d, const uint32_t *__restrict__ up, int levels, uint32_t n_cand,
                                                         const int64_t *__restrict__ cand_off, int64_t n_rec, Tags tags, BrRec *__restrict__ rec,
                                                         int64_t *__restrict__ wide, BrFlags *__restrict__ fl) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rec) return;
    const int64_t n1 = n_rec + 1;
    if (r == n_rec) { wide[r] = wide[n1 + r] = wide[2 * n1 + r] = wide[3 * n1 + r] = 0; return; }
    const int64_t q = cand_off[br_lift(up, levels, n_cand, 0, r)];
    const uint8_t *p = d + q;
    const uint32_t block_size = bam_block_size(p), l_name = bam_l_name(p), n_cig = bam_n_cig(p), flag = bam_flag(p);
    const int32_t l_seq = bam_l_seq(p);
    const bool kept = !(flag & 0x900);
    BrRec R;
    R.name_at = q + kBamName; R.seq_at = q + bam_seq_at(l_name, n_cig); R.end = q + 4 + (int64_t)block_size;
    R.l_name = (int32_t)l_name - 1; R.l_seq = l_seq; R.flag = flag | (kept ? 1u << 16 : 0u); R.pad_ = 0;
    int l_comment = 0;
    if (kept) {
        unsigned long long err = 0;
        const int64_t qual_at = q + bam_qual_at(l_name, n_cig, l_seq), aux_at = q + bam_aux_at(l_name, n_cig, l_seq);
        if (l_seq == 0) err = kErrLseq0;
        else {
            // the first kept record of either kind: the minimum settles with the first blocks, so look before the atomic (a stale
            // value only costs an atomic; a million of them on one address cost 10 ms)
            unsigned long long *first = d[qual_at] == 0xFF ? &fl->first_n : &fl->first_q;
            if ((unsigned long long)r < __atomic_load_n(first, __ATOMIC_RELAXED)) atomicMin(first, (unsigned long long)r);
            if (tags.n) {
                for (int64_t a = aux_at; a < R.end && !err;) {          // every field inside the record, of a known type
                    int64_t val;
                    int ty;
                    const int64_t nx = aux_next(d, a, R.end, &val, &ty);
                    if (nx < 0) { err = kErrAuxBad; break; }
                    if (ty == 'f' || ty == 'B') {                          // refused when it is a listed tag's first field
                        for (int t = 0; t < tags.n; ++t)
                            if (d[a] == tags.t[2 * t] && d[a + 1] == tags.t[2 * t + 1]) {
                                int ty1;
                                if (aux_find(d, aux_at, a, tags.t[2 * t], tags.t[2 * t + 1], &ty1) < 0) err = kErrAuxType;     // no earlier field of this tag
                                break;
                            }
                    }
                    a = nx;
                }
                if (!err)
                    for (int t = 0; t < tags.n; ++t) {
                        int ty;
                        const int64_t v = aux_find(d, aux_at, R.end, tags.t[2 * t], tags.t[2 * t + 1], &ty);
                        if (v >= 0) l_comment += aux_text_len(d, v, ty) + (l_comment ? 1 : 0);
                    }
            }
        }
        if (err) atomicMin(&fl->err, (unsigned long long)r << 8 | err);
    }
    rec[r] = R;
    wide[r] = kept ? R.l_name : 0;
    wide[n1 + r] = l_comment;
    wide[2 * n1 + r] = kept ? l_seq : 0;
    wide[3 * n1 + r] = kept ? 1 : 0;
}

// the offsets of the kept reads: comp = 3 rows of n_rec + 1 (name, comment, bases), entry k of a row = the kept read k's offset
__global__ __launch_bounds__(256) void br_compact_kernel(const int64_t *__restrict__ wide, const int64_t *__restrict__ offs, int64_t n_rec,
                                                         int64_t *__restrict__ comp) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rec) return;
    const int64_t n1 = n_rec + 1;
    if (r < n_rec && !wide[3 * n1 + r]) return;
    const int64_t k = offs[3 * n1 + r];
    for (int row = 0; row < 3; ++row) comp[row * n1 + k] = offs[row * n1 + r];
}

// a nibble's base code (1, 2, 4, 8 -> 0 .. 3, anything else 4): digit c of a constant
__device__ __forceinline__ uint32_t nib_code(uint32_t c) { return (uint32_t)(0x4444444344424104ull >> (4 * c)) & 15; }

// kGroup lanes per record
__global__ __launch_bounds__(256) void br_emit_kernel(const uint8_t *__restrict__ d, int64_t n, const BrRec *__restrict__ rec, int64_t n_rec,
                                                      const int64_t *__restrict__ offs, Tags tags, int has_qual, char *__restrict__ names,
                                                      char *__restrict__ comments, uint8_t *__restrict__ enc, char *__restrict__ qual) {
    const int lane = threadIdx.x & (kGroup - 1);
    const int64_t n1 = n_rec + 1;
    const int64_t group = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup, n_groups = ((int64_t)gridDim.x * blockDim.x) / kGroup;
    for (int64_t r = group; r < n_rec; r += n_groups) {
        const BrRec R = rec[r];
        if (!(R.flag >> 16)) continue;
        const bool rev = R.flag & 0x10;
        const int64_t no = offs[r], co = offs[n1 + r], so = offs[2 * n1 + r];
        const int l = R.l_seq;
        for (int i = lane; i < R.l_name; i += kGroup) names[no + i] = (char)d[R.name_at + i];
        // bases: 4 packed bytes = 8 bases per lane and step
        for (int s = lane * 8; s < l; s += kGroup * 8) {
            const uint32_t w = ld_wide(d, R.seq_at + (s >> 1), n);
            for (int k = 0; k < 8 && s + k < l; ++k) {
                uint32_t c = nib_code((w >> (8 * (k >> 1) + ((k & 1) ? 0 : 4))) & 15);
                if (rev && c < 4) c = 3 - c;
                enc[so + (rev ? l - 1 - (s + k) : s + k)] = (uint8_t)c;
            }
        }
        if (has_qual) {
            const int64_t qual_at = R.seq_at + ((int64_t)l + 1) / 2;
            for (int i = lane; i < l; i += kGroup) qual[so + i] = (char)(d[qual_at + (rev ? l - 1 - i : i)] + 33);
        }
        // comment: lanes take the listed tags, a prefix sum over the group places each field
        if (tags.n) {
            const int64_t aux_at = R.seq_at + ((int64_t)l + 1) / 2 + l;
            int before = 0;                                                   // bytes of the fields of the rounds before
            for (int t0 = 0; t0 < tags.n; t0 += kGroup) {
                const int t = t0 + lane;
                int ty = 0, len = 0;
                int64_t v = -1;
                if (t < tags.n) {
                    v = aux_find(d, aux_at, R.end, tags.t[2 * t], tags.t[2 * t + 1], &ty);
                    if (v >= 0) len = aux_text_len(d, v, ty) + 1;             // with the tab in front of it
                }
                int incl = len;
                for (int o = 1; o < kGroup; o <<= 1) {
                    const int x = __shfl_up(incl, o, kGroup);
                    if (lane >= o) incl += x;
                }
                const int excl = before + incl - len;
                if (v >= 0) {
                    char *out = comments + co + excl - 1;                     // the first field has no tab
                    if (excl) out[0] = '\t';
                    aux_text_write(d, v, ty, tags.t[2 * t], tags.t[2 * t + 1], out + 1);
                }
                before += __shfl(incl, kGroup - 1, kGroup);
            }
        }
    }
}

}  // namespace
}  // namespace bwams

using namespace bwams;

extern "C" {

int bwams_bam_reads_decode(int device, const void *bam, int64_t n_bytes, const char *tags, bwams_fastq_t **out, int64_t *n_reads,
                           int64_t *n_bases, int64_t *n_records) {
    if (!bam || n_bytes < 0 || !out) return BWAMS_ERR_ARG;
    *out = nullptr;
    Tags tg;
    memset(&tg, 0, sizeof tg);
    if (tags) {
        const size_t lt = strlen(tags);
        if ((lt & 1) || lt > 2 * kMaxTags) {
            set_last_error("bwams_bam_reads_decode: tags must be two-letter tags back to back, at most 32 of them");
            return BWAMS_ERR_ARG;
        }
        tg.n = (int32_t)(lt / 2);
        memcpy(tg.t, tags, lt);
    }
    if (n_bytes >= ((int64_t)1 << 36)) {
        set_last_error("bwams_bam_reads_decode: a buffer of 2^36 bytes or more (cut the records into chunks)");
        return BWAMS_ERR_UNSUPPORTED;
    }
    BWAMS_HIP(hipSetDevice(device));
    hipStream_t st = nullptr;
    std::unique_ptr<bwams_fastq> f(new bwams_fastq());
    f->device = device;
    auto finish = [&](int64_t n_rec) {
        if (n_reads) *n_reads = f->n_reads;
        if (n_bases) *n_bases = f->n_bases;
        if (n_records) *n_records = n_rec;
        f->n_records = n_rec;
        *out = f.release();
        return BWAMS_OK;
    };
    auto empty = [&](int64_t n_rec) -> int {          // rule 7: the handle of a text without records
        f->cum.assign(1, 0); f->name_off.assign(1, 0); f->comment_off.assign(1, 0);
        BWAMS_HIP(f->d_enc.alloc(64)); BWAMS_HIP(f->d_qual.alloc(64)); BWAMS_HIP(f->d_names.alloc(64)); BWAMS_HIP(f->d_comments.alloc(64));
        return finish(n_rec);
    };
    if (n_bytes == 0) return empty(0);
    struct Events {
        hipEvent_t a = nullptr, b = nullptr, c = nullptr;
        ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); if (c) (void)hipEventDestroy(c); }
    } evs;
    BWAMS_HIP(hipEventCreate(&evs.a)); BWAMS_HIP(hipEventCreate(&evs.b)); BWAMS_HIP(hipEventCreate(&evs.c));
    // the records may already be in this GPU's memory; the kernels want them 16-byte aligned
    hipPointerAttribute_t attr;
    const bool on_dev = hipPointerGetAttributes(&attr, bam) == hipSuccess && attr.type == hipMemoryTypeDevice;
    (void)hipGetLastError();
    DevBuf<uint8_t> own;
    BrDiscover disc;
    DevBuf<int64_t> wide, offs, comp;
    DevBuf<BrRec> recs;
    DevBuf<BrFlags> flags;
    const uint8_t *d = static_cast<const uint8_t *>(bam);
    if (!on_dev || (reinterpret_cast<uintptr_t>(bam) & 15)) {
        BWAMS_HIP(own.alloc((size_t)n_bytes + 16));
        BWAMS_HIP(hipMemcpy(own.p, bam, (size_t)n_bytes, on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        d = own.p;
    }
    BWAMS_HIP(hipEventRecord(evs.a, st));
    auto bad_record = [&](int64_t ordinal, int64_t at) {
        set_last_error("bwams_bam_reads_decode: record " + std::to_string(ordinal) + " at byte " + std::to_string(at) +
                       " is not a well-formed BAM record inside the buffer (block_size, l_read_name, l_seq, the name's NUL), or the "
                       "records do not end at n_bytes");
        return BWAMS_ERR_ARG;
    };
    // the records: the chain from byte 0 must end at n_bytes
    BrEnd ch;
    if (int rc = disc.run(d, n_bytes, 0, n_bytes, st, &ch)) return rc;
    BWAMS_HIP(hipEventRecord(evs.b, st));
    if (ch.how != kBrStopped) return bad_record(ch.n_rec, ch.at);
    const int64_t n_rec = ch.n_rec, n1 = n_rec + 1;
    const uint32_t n_cand = disc.n_cand;
    const int levels = disc.levels;
    DevBuf<uint32_t> &up = disc.up;
    DevBuf<int64_t> &cand_off = disc.cand_off;
    DevBuf<> &scan_tmp = disc.scan_tmp;
    f->n_cand = n_cand;
    // measure, scans, the kept reads' offsets
    BWAMS_HIP(recs.alloc((size_t)n1 * sizeof(BrRec)));
    BWAMS_HIP(wide.alloc((size_t)n1 * 4 * 8));
    BWAMS_HIP(offs.alloc((size_t)n1 * 4 * 8));
    BWAMS_HIP(comp.alloc((size_t)n1 * 3 * 8));
    BWAMS_HIP(flags.alloc(sizeof(BrFlags)));
    BWAMS_HIP(hipMemsetAsync(flags.p, 0xFF, sizeof(BrFlags), st));
    br_measure_kernel<<<(unsigned)((n1 + 255) / 256), 256, 0, st>>>(d, up.p, levels, n_cand, cand_off.p, n_rec, tg, recs.p, wide.p, flags.p);
    {
        size_t tb = 0;                                // the four rows are scans of one size
        BWAMS_HIP(rocprim::exclusive_scan(nullptr, tb, wide.p, offs.p, (int64_t)0, (size_t)n1, rocprim::plus<int64_t>(), st));
        BWAMS_HIP(scan_tmp.ensure(tb + 16));
        for (int row = 0; row < 4; ++row)
            BWAMS_HIP(rocprim::exclusive_scan(scan_tmp.p, tb, wide.p + row * n1, offs.p + row * n1, (int64_t)0, (size_t)n1, rocprim::plus<int64_t>(), st));
    }
    br_compact_kernel<<<(unsigned)((n1 + 255) / 256), 256, 0, st>>>(wide.p, offs.p, n_rec, comp.p);
    BrFlags h_fl;
    int64_t tot[4] = {0, 0, 0, 0};
    BWAMS_HIP(hipMemcpyAsync(&h_fl, flags.p, sizeof h_fl, hipMemcpyDeviceToHost, st));
    for (int row = 0; row < 4; ++row) BWAMS_HIP(hipMemcpyAsync(&tot[row], offs.p + row * n1 + n_rec, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    // rules 4 and 6: the earliest record decides; within one record l_seq 0, then mixed qualities, then the aux fields
    unsigned long long err = h_fl.err;
    if (h_fl.first_q != ~0ull && h_fl.first_n != ~0ull) {
        const unsigned long long mixed = std::max(h_fl.first_q, h_fl.first_n) << 8 | kErrMixed;
        if (mixed < err) err = mixed;
    }
    if (err != ~0ull) {
        const int64_t ordinal = (int64_t)(err >> 8);
        int64_t at = 0;
        BrRec R;
        BWAMS_HIP(hipMemcpy(&R, recs.p + ordinal, sizeof R, hipMemcpyDeviceToHost));
        at = R.name_at - 36;
        const std::string where = "bwams_bam_reads_decode: record " + std::to_string(ordinal) + " at byte " + std::to_string(at) + ": ";
        switch (err & 0xFF) {
        case kErrLseq0: set_last_error(where + "a read without bases (l_seq 0)"); return BWAMS_ERR_UNSUPPORTED;
        case kErrMixed:
            set_last_error(where + (h_fl.first_q < h_fl.first_n ? "no qualities, while record " + std::to_string(h_fl.first_q) + " has them"
                                                                : "qualities, while record " + std::to_string(h_fl.first_n) + " has none"));
            return BWAMS_ERR_UNSUPPORTED;
        case kErrAuxType: set_last_error(where + "a listed tag of type f or B"); return BWAMS_ERR_UNSUPPORTED;
        default: set_last_error(where + "an aux field of unknown type, or one that runs past its record"); return BWAMS_ERR_ARG;
        }
    }
    const int64_t n_kept = tot[3];
    if (n_kept == 0) return empty(n_rec);
    const size_t k1 = (size_t)n_kept + 1;
    f->name_off.resize(k1); f->comment_off.resize(k1); f->cum.resize(k1);
    BWAMS_HIP(hipMemcpyAsync(f->name_off.data(), comp.p, k1 * 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipMemcpyAsync(f->comment_off.data(), comp.p + n1, k1 * 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipMemcpyAsync(f->cum.data(), comp.p + 2 * n1, k1 * 8, hipMemcpyDeviceToHost, st));
    f->has_qual = h_fl.first_q != ~0ull;
    f->n_reads = n_kept; f->name_bytes = tot[0]; f->comment_bytes = tot[1]; f->n_bases = tot[2];
    BWAMS_HIP(f->d_enc.alloc((size_t)f->n_bases + 64));
    BWAMS_HIP(f->d_qual.alloc((size_t)f->n_bases + 64));
    BWAMS_HIP(f->d_names.alloc((size_t)f->name_bytes + 64));
    BWAMS_HIP(f->d_comments.alloc((size_t)f->comment_bytes + 64));
    {
        int64_t blocks = (n_rec + 256 / kGroup - 1) / (256 / kGroup);
        if (blocks > 256 * 256) blocks = 256 * 256;
        br_emit_kernel<<<(unsigned)blocks, 256, 0, st>>>(d, n_bytes, recs.p, n_rec, offs.p, tg, f->has_qual ? 1 : 0, f->d_names.p,
                                                         f->d_comments.p, f->d_enc.p, f->d_qual.p);
    }
    BWAMS_HIP(hipEventRecord(evs.c, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    float ms_emit = 0;
    (void)hipEventElapsedTime(&f->ms_discover, evs.a, evs.b);
    (void)hipEventElapsedTime(&ms_emit, evs.b, evs.c);
    f->ms = f->ms_discover + ms_emit;
    return finish(n_rec);
}

int bwams_bam_reads_info(const bwams_fastq_t *f, float *ms_discover, float *ms_emit, int64_t *n_candidates, int64_t *n_records) {
    if (!f) return BWAMS_ERR_ARG;
    if (ms_discover) *ms_discover = f->ms_discover;
    if (ms_emit) *ms_emit = f->ms - f->ms_discover;
    if (n_candidates) *n_candidates = f->n_cand;
    if (n_records) *n_records = f->n_records;
    return BWAMS_OK;
}

}  // extern "C"
