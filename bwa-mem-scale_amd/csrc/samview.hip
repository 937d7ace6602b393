// samview.hip — BAM alignment records printed as SAM lines on the device (bwams_samview_t; rules V1-V8 in include/bwams.h above
// bwams_samview_open, restated in bwams/samview.py).  bam.hip turned round, and of its shape:
//   samview_count_kernel  every record's line length, or nothing when rule V2 filters it, as (bytes, lines) for the scan; rule V6's
//                         check of every record, filtered ones too, with atomicMin of ordinal << 3 | reason into the first-bad word;
//   rocprim::exclusive_scan (collate.hip's co_scan_place) over the n + 1 pairs: each line's offset and ordinal, and the totals;
//   samview_write_kernel  the same walk again, storing.  Nothing is carried between the passes except the sizes.
// Sixteen lanes own a record.  The short fields (FLAG, POS, MAPQ, PNEXT, TLEN, an integer or float aux value with its tag) are
// formatted by all sixteen lanes alike into a Text16 (fmt_g.h: sixteen bytes in two registers) and lane k stores byte k: one
// store instruction a text.  The long fields — name, reference names, SEQ, QUAL, Z and H values, most of a 150-base read's line —
// are striped across the group: up to three bytes to the next four-byte boundary of the output, then a 32-bit store a lane a step
// (64 bytes a group a step), then up to three bytes.  CIGAR operations and the elements of a B array are short items of varying
// width: sixteen of them a step, a lane formats one, their offsets come from a prefix sum over the group's widths (four
// shuffles), each lane stores its own item.  The digit count of an integer comes from dec_digits_u32 in both passes; the writing
// pass formats with put_u32, which loops over that same count.
// No LDS, no scratch (nothing indexes an array with a variable), no floating point: "%g" is fmt_g's integer arithmetic.  Every read
// of a record is bounded by the record's end, every store by the size the counting pass found over the same walk.
#include "common.h"
#include "aux_rg.h"
#include "fmt_g.h"

namespace bwams {
namespace {

__device__ __forceinline__ int group_lane() { return (int)(threadIdx.x & (kGroup - 1)); }
__device__ __forceinline__ unsigned group_bits(bool hit) { return (unsigned)(__ballot(hit) >> (threadIdx.x & 48)) & 0xFFFFu; }

// the sum of v over the lanes of the group up to and including this one
__device__ __forceinline__ int group_scan(int v) {
    const int g = group_lane();
#pragma unroll
    for (int d = 1; d < kGroup; d <<= 1) {
        const int t = __shfl_up(v, d, kGroup);
        if (g >= d) v += t;
    }
    return v;
}

__device__ __forceinline__ void min_if_less(unsigned long long *word, unsigned long long v) {
    if (v < *reinterpret_cast<volatile unsigned long long *>(word)) atomicMin(word, v);
}

__device__ __forceinline__ uint32_t nt16_char(uint32_t code) {        // "=ACMGRSVTWYHKDBN"
    const uint64_t w = code < 8 ? 0x565352474D43413DULL : 0x4E42444B48595754ULL;   // "=ACMGRSV", "TWYHKDBN"
    return (uint32_t)(w >> (8 * (code & 7))) & 255u;
}
__device__ __forceinline__ uint32_t cigar_char(uint32_t code) {       // "MIDNSHP=X", code <= 8
    return code == 8 ? (uint32_t)'X' : (uint32_t)(0x3D5048534E44494DULL >> (8 * code)) & 255u;
}

// A short text in the making.  The counting pass only adds up the bytes.
template <bool EMIT> struct Txt {
    Text16 t;
    __device__ __forceinline__ void ch(uint32_t c) { if (EMIT) t.put(c); else ++t.n; }
    __device__ __forceinline__ void u32(uint32_t v) { if (EMIT) put_u32(t, v); else t.n += dec_digits_u32(v); }
    __device__ __forceinline__ void i64(int64_t v) { if (EMIT) put_i64(t, v); else t.n += dec_digits_i64(v); }
};

// The line of one record: counted always, stored (EMIT) from p + n on.
template <bool EMIT> struct Out {
    uint8_t *p;
    int64_t n;
    __device__ __forceinline__ void ch(uint32_t c) {                   // lane 0 stores
        if (EMIT && group_lane() == 0) p[n] = (uint8_t)c;
        ++n;
    }
    __device__ __forceinline__ void text(const Txt<EMIT> &x) {         // lane k stores byte k
        if (EMIT && group_lane() < x.t.n) p[n + group_lane()] = (uint8_t)x.t.at(group_lane());
        n += x.t.n;
    }
    // lane by lane, each its own text at n + at: the items of a group step
    __device__ __forceinline__ void item(const Text16 &t, int at, bool have) {
        if (EMIT && have)
            for (int k = 0; k < t.n; ++k) p[n + at + k] = (uint8_t)t.at(k);
    }
    // len bytes, byte k being gen(k), striped over the group
    template <class Gen> __device__ __forceinline__ void bytes(int64_t len, Gen gen) {
        if (EMIT) {
            uint8_t *d = p + n;
            const int g = group_lane();
            int64_t head = (int64_t)((4 - (reinterpret_cast<uintptr_t>(d) & 3)) & 3);
            if (head > len) head = len;
            if (g < head) d[g] = (uint8_t)gen((int64_t)g);
            const int64_t words = (len - head) >> 2;
            for (int64_t w = g; w < words; w += kGroup) {
                const int64_t k = head + 4 * w;
                *reinterpret_cast<uint32_t *>(d + k) = gen(k) | gen(k + 1) << 8 | gen(k + 2) << 16 | gen(k + 3) << 24;
            }
            const int64_t k = head + 4 * words + g;
            if (k < len) d[k] = (uint8_t)gen(k);
        }
        n += len;
    }
};

// RNAME / RNEXT: the reference's name
template <bool EMIT> __device__ __forceinline__ void ref_name(const SvArgs &A, int32_t rid, Out<EMIT> &o) {
    const int64_t a = A.name_off[rid];
    const uint8_t *s = A.names + a;
    o.bytes(A.name_off[rid + 1] - a, [&](int64_t k) { return (uint32_t)s[k]; });
}

// the value of aux type ty (A c C s S i I f) at v behind what x holds
template <bool EMIT> __device__ __forceinline__ void aux_value(Txt<EMIT> &x, uint32_t ty, const uint8_t *v) {
    if (ty == 'A') x.ch(v[0]);
    else if (ty == 'c') x.i64((int8_t)v[0]);
    else if (ty == 'C') x.u32(v[0]);
    else if (ty == 's') x.i64((int16_t)ld_u16(v));
    else if (ty == 'S') x.u32(ld_u16(v));
    else if (ty == 'i') x.i64((int32_t)ld_u32(v));
    else if (ty == 'I') x.u32(ld_u32(v));
    else {                                                              // f: both passes format it
        const Text16 f = fmt_g(ld_u32(v));
        if (EMIT)
            for (int k = 0; k < f.n; ++k) x.t.put(f.at(k));
        else x.t.n += f.n;
    }
}

enum SvReason : unsigned { kSvRef = 1, kSvName = 2, kSvOp = 3, kSvBounds = 4, kSvAux = 5 };

// One line from the record at p (span bytes to the next record).  Returns 0 and the line's bytes in o.n, or rule V6's reason: the
// first that holds in the order 1, 4, 2, 3, 5 (what 4 refuses cannot be read for 2, 3 and 5).  The writing pass runs only over
// records the counting pass passed, and skips the checks that read nothing it needs.
template <bool EMIT> __device__ unsigned sv_record(const SvArgs &A, const uint8_t *p, int64_t span, Out<EMIT> &o) {
    const int g = group_lane();
    int64_t n = (int64_t)bam_block_size(p) + 4;                         // the record's end
    if (n > span) n = span;
    const int32_t rid = bam_ref_id(p), nrid = bam_next_ref_id(p);
    if (rid < -1 || rid >= A.n_ref || nrid < -1 || nrid >= A.n_ref) return kSvRef;
    const uint32_t l_name = bam_l_name(p), n_cig = bam_n_cig(p);
    const int64_t l_seq = bam_l_seq(p);
    if (l_seq < 0) return kSvBounds;
    const int64_t aux0 = bam_aux_at(l_name, n_cig, l_seq);
    if (aux0 > n) return kSvBounds;
    if (l_name == 0) return kSvName;
    const uint8_t *name = p + kBamName;
    if (!EMIT) {                                                        // the NUL at the end and nowhere else
        bool bad = false;
        for (uint32_t k = g; k < l_name; k += kGroup) bad |= (name[k] == 0) != (k == l_name - 1);
        if (group_bits(bad)) return kSvName;
    }
    // QNAME FLAG RNAME POS MAPQ
    o.bytes((int64_t)l_name - 1, [&](int64_t k) { return (uint32_t)name[k]; });
    {
        Txt<EMIT> x;
        x.ch('\t'); x.u32(bam_flag(p)); x.ch('\t');
        if (rid < 0) x.ch('*');
        o.text(x);
    }
    if (rid >= 0) ref_name(A, rid, o);
    {
        Txt<EMIT> x;
        x.ch('\t'); x.u32((uint32_t)(bam_pos(p) + 1)); x.ch('\t'); x.u32(bam_mapq(p)); x.ch('\t');
        o.text(x);
    }
    if (n_cig == 0) o.ch('*');
    // CIGAR: sixteen operations a step
    const uint8_t *cig = p + bam_cigar_at(l_name);
    bool bad_op = false;
    for (uint32_t base = 0; base < n_cig; base += kGroup) {
        const uint32_t k = base + g;
        const bool have = k < n_cig;
        const uint32_t op = have ? ld_u32(cig + 4 * (int64_t)k) : 0u, code = op & 15u;
        bad_op |= code > 8;
        const int w = have ? dec_digits_u32(op >> 4) + 1 : 0;
        const int incl = group_scan(w);
        if (EMIT) {
            Text16 t;
            put_u32(t, op >> 4);
            t.put(cigar_char(code));
            o.item(t, incl - w, have);
        }
        o.n += __shfl(incl, kGroup - 1, kGroup);
    }
    if (!EMIT && group_bits(bad_op)) return kSvOp;
    // RNEXT PNEXT TLEN
    {
        Txt<EMIT> x;
        x.ch('\t');
        if (nrid < 0) x.ch('*');
        else if (nrid == rid) x.ch('=');
        o.text(x);
    }
    if (nrid >= 0 && nrid != rid) ref_name(A, nrid, o);
    {
        Txt<EMIT> x;
        x.ch('\t'); x.u32((uint32_t)(bam_next_pos(p) + 1)); x.ch('\t');
        o.text(x);
    }
    {
        Txt<EMIT> x;
        x.i64(bam_tlen(p)); x.ch('\t');
        if (l_seq == 0) { x.ch('*'); x.ch('\t'); x.ch('*'); }
        o.text(x);
    }
    // SEQ QUAL
    if (l_seq > 0) {
        const uint8_t *seq = p + bam_seq_at(l_name, n_cig), *qual = seq + (l_seq + 1) / 2;
        o.bytes(l_seq, [&](int64_t k) { return nt16_char((uint32_t)(seq[k >> 1] >> ((k & 1) ? 0 : 4)) & 15u); });
        o.ch('\t');
        if (qual[0] == 0xFF) o.ch('*');
        else o.bytes(l_seq, [&](int64_t k) { return (uint32_t)(uint8_t)(qual[k] + 33); });
    }
    // the aux fields, by aux_first_rg's walk
    int64_t a = aux0;
    while (a < n) {
        if (a + 3 > n) return kSvAux;
        const uint32_t c0 = p[a], c1 = p[a + 1], ty = p[a + 2];
        a += 3;
        Txt<EMIT> x;
        x.ch('\t'); x.ch(c0); x.ch(c1); x.ch(':');
        if (ty == 'Z' || ty == 'H') {
            int64_t e = a;
            for (;;) {                                                  // the NUL, sixteen bytes a step
                const int64_t q = e + g;
                const unsigned bits = group_bits(q >= n || p[q] == 0);
                if (bits) { e += __builtin_ctz(bits); break; }
                e += kGroup;
            }
            if (e >= n) return kSvAux;
            x.ch(ty); x.ch(':');
            o.text(x);
            const uint8_t *v = p + a;
            o.bytes(e - a, [&](int64_t k) { return (uint32_t)v[k]; });
            a = e + 1;
        } else if (ty == 'B') {
            if (a + 5 > n) return kSvAux;
            const uint32_t sub = p[a];
            const int sz = aux_size(sub);
            if (!sz || sub == 'A') return kSvAux;
            const int64_t cnt = ld_u32(p + a + 1), end = a + 5 + (int64_t)sz * cnt;
            if (end > n) return kSvAux;
            x.ch('B'); x.ch(':'); x.ch(sub);
            o.text(x);
            const uint8_t *v = p + a + 5;
            for (int64_t base = 0; base < cnt; base += kGroup) {        // sixteen elements a step
                const int64_t k = base + g;
                const bool have = k < cnt;
                Txt<EMIT> el;
                if (have) { el.ch(','); aux_value(el, sub, v + (int64_t)sz * k); }
                const int w = el.t.n, incl = group_scan(w);
                o.item(el.t, incl - w, have);
                o.n += __shfl(incl, kGroup - 1, kGroup);
            }
            a = end;
        } else {
            const int sz = aux_size(ty);
            if (!sz || a + sz > n) return kSvAux;
            x.ch((ty == 'A' || ty == 'f') ? ty : (uint32_t)'i'); x.ch(':');
            o.text(x);
            Txt<EMIT> val;
            aux_value(val, ty, p + a);
            o.text(val);
            a += sz;
        }
    }
    o.ch('\n');
    return 0;
}

__global__ void __launch_bounds__(256) samview_count_kernel(SvArgs A) {
    const int64_t n_groups = (int64_t)gridDim.x * (blockDim.x / kGroup);
    for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup; r <= A.n_rec; r += n_groups) {
        if (r == A.n_rec) {                                             // the scan's last slot: its totals
            if (group_lane() == 0) A.size[r] = CoPlace{0, 0};
            continue;
        }
        const uint8_t *p = A.bam + A.rec_off[r];
        Out<false> o{nullptr, 0};
        const unsigned why = sv_record<false>(A, p, A.rec_off[r + 1] - A.rec_off[r], o);
        const uint32_t flag = bam_flag(p);
        const bool keep = (flag & A.require) == A.require && (flag & A.exclude) == 0 && bam_mapq(p) >= A.min_mapq;
        if (group_lane() == 0) {
            A.size[r] = (why || !keep) ? CoPlace{0, 0} : CoPlace{o.n, 1};
            if (why) min_if_less(A.bad, (unsigned long long)r << 3 | (why - 1));
        }
    }
}

__global__ void __launch_bounds__(256) samview_write_kernel(SvArgs A) {
    const int64_t n_groups = (int64_t)gridDim.x * (blockDim.x / kGroup);
    for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup; r <= A.n_rec; r += n_groups) {
        const CoPlace at = A.at[r];
        if (r == A.n_rec) {                                             // the end of the last line
            if (group_lane() == 0) A.line_off[at.n] = at.bytes;
            continue;
        }
        if (A.size[r].n == 0) continue;
        if (group_lane() == 0) A.line_off[at.n] = at.bytes;
        Out<true> o{A.text, at.bytes};
        (void)sv_record<true>(A, A.bam + A.rec_off[r], A.rec_off[r + 1] - A.rec_off[r], o);
    }
}

}  // namespace

void launch_samview_count(const SvArgs &A, int cu_count, hipStream_t st) {
    samview_count_kernel<<<grid_of(A.n_rec + 1, 256 / kGroup, cu_count), 256, 0, st>>>(A);
}

void launch_samview_write(const SvArgs &A, int cu_count, hipStream_t st) {
    samview_write_kernel<<<grid_of(A.n_rec + 1, 256 / kGroup, cu_count), 256, 0, st>>>(A);
}

}  // namespace bwams
