// bam.hip — a batch's SAM text re-encoded as BAM alignment records (SAMv1 §4.2) on the device.
//
// The input is the text every SAM producer leaves in HBM (sam_text.hip's single-end, paired-end and EMF branches, and the smart
// merge), so one encoder covers them all.  The rules are htslib's sam_parse1 + bam_write1 (restated for the tests in
// bwams/bam.py): little-endian fixed fields, 0-based positions, bin = reg2bin(pos, bam_endpos), CIGAR as len << 4 | op, SEQ as
// 4-bit codes high nibble first, QUAL - 33 (0xFF when '*'), aux fields in text order with the smallest integer type.
//
// Mapping.  Like sam_text.hip: a counting pass (bam_count_kernel: every record's size, and its refusal), an exclusive scan, a
// writing pass (bam_write_kernel) over the same parse; nothing is kept between the passes.  Sixteen lanes own a record (a line):
// the separators are found sixteen bytes a step (one coalesced load across the group and a ballot), the small fields are parsed by
// all sixteen lanes alike (same loads, same values; lane 0 stores them), and the long fields — the name, SEQ, QUAL and Z values,
// most of the output — are stored by the sixteen lanes together, a byte each per step.
#include <algorithm>
#include <cstring>
#include "common.h"
#include "bam_rec.h"

namespace bwams {
namespace {

enum BamRefusal : unsigned { kBadLine = 1, kLongName = 2, kBadAux = 3, kBadInt = 4, kManyOps = 5, kSeqQual = 6 };

__device__ __forceinline__ int group_lane() { return (int)(threadIdx.x & (kGroup - 1)); }

// first q in [p, end] with t[q] == '\t', or end (the line's '\n')
__device__ int64_t next_sep(const char *t, int64_t p, int64_t end) {
    const int g = group_lane();
    for (;;) {
        const int64_t q = p + g;
        const bool hit = q >= end || t[q] == '\t';
        const unsigned bits = (unsigned)(__ballot(hit) >> (threadIdx.x & 48)) & 0xFFFFu;
        if (bits) return p + __builtin_ctz(bits);
        p += kGroup;
    }
}

// [+-]?[0-9]{1,18}
__device__ bool parse_int(const char *t, int64_t a, int64_t b, int64_t *v) {
    bool neg = false;
    if (a < b && (t[a] == '-' || t[a] == '+')) neg = t[a++] == '-';
    if (a >= b || b - a > 18) return false;
    int64_t x = 0;
    for (int64_t i = a; i < b; ++i) {
        const char c = t[i];
        if (c < '0' || c > '9') return false;
        x = x * 10 + (c - '0');
    }
    *v = neg ? -x : x;
    return true;
}

// [+-]?(digits[.digits] | .digits), at most 15 digits: (float)strtod, exactly (the mantissa and 10^k are exact doubles, so the one
// division rounds as strtod does)
__device__ bool parse_float(const char *t, int64_t a, int64_t b, float *v) {
    bool neg = false, dot = false;
    if (a < b && (t[a] == '-' || t[a] == '+')) neg = t[a++] == '-';
    int nd = 0, k = 0;
    int64_t m = 0;
    for (int64_t i = a; i < b; ++i) {
        const char c = t[i];
        if (c == '.' && !dot) { dot = true; continue; }
        if (c < '0' || c > '9') return false;
        m = m * 10 + (c - '0');
        ++nd;
        k += dot;
    }
    if (nd == 0 || nd > 15) return false;
    double d = 1.0;
    for (int i = 0; i < k; ++i) d *= 10.0;
    const double x = (double)m / d;
    *v = (float)(neg ? -x : x);
    return true;
}

__device__ __forceinline__ uint8_t nt16(char c) {      // "=ACMGRSVTWYHKDBN", anything else 15
    switch (c) {
    case '=': return 0; case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5;
    case 'S': return 6; case 'V': return 7; case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11;
    case 'K': return 12; case 'D': return 13; case 'B': return 14; default: return 15;
    }
}

__device__ __forceinline__ int cigar_op(char c) {
    switch (c) {
    case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4; case 'H': return 5;
    case 'P': return 6; case '=': return 7; case 'X': return 8; default: return -1;
    }
}

// the output of one record: counted always, stored (EMIT) within [n, lim) only
template <bool EMIT> struct Out {
    uint8_t *p;
    int64_t n, lim;
    __device__ __forceinline__ void b(uint32_t v) {            // lane 0 stores
        if (EMIT && group_lane() == 0 && n < lim) p[n] = (uint8_t)v;
        ++n;
    }
    __device__ __forceinline__ void u16(uint32_t v) { b(v); b(v >> 8); }
    __device__ __forceinline__ void u32(uint32_t v) { b(v); b(v >> 8); b(v >> 16); b(v >> 24); }
    __device__ __forceinline__ void copy(const char *s, int64_t len, int sub) {   // the group stores s[k] - sub, a byte a lane a step
        if (EMIT)
            for (int64_t k = group_lane(); k < len; k += kGroup)
                if (n + k < lim) p[n + k] = (uint8_t)(s[k] - sub);
        n += len;
    }
    __device__ __forceinline__ void fill(uint8_t v, int64_t len) {
        if (EMIT)
            for (int64_t k = group_lane(); k < len; k += kGroup)
                if (n + k < lim) p[n + k] = v;
        n += len;
    }
    __device__ __forceinline__ void seq(const char *s, int64_t l) {           // two bases a byte, high nibble first
        const int64_t nb = (l + 1) >> 1;
        if (EMIT)
            for (int64_t k = group_lane(); k < nb; k += kGroup)
                if (n + k < lim) p[n + k] = (uint8_t)(nt16(s[2 * k]) << 4 | (2 * k + 1 < l ? nt16(s[2 * k + 1]) : 0));
        n += nb;
    }
};

// RNAME -> refID: binary search over the names' sorted permutation (bam_names_index); -2 = unknown
__device__ int ref_id(const BamArgs &A, const char *t, int64_t a, int64_t b) {
    if (b - a == 1 && t[a] == '*') return -1;
    int lo = 0, hi = A.n_ctg;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int id = A.ctg_sorted[mid];
        const char *s = A.ctg_names + A.ctg_off[id];
        int c = 0;
        int64_t i = 0;
        for (; a + i < b; ++i) {
            const unsigned char x = (unsigned char)t[a + i], y = (unsigned char)s[i];
            if (x != y) { c = x < y ? -1 : 1; break; }
        }
        if (a + i == b) c = s[i] ? -1 : 0;
        if (c == 0) return id;
        if (c < 0) hi = mid;
        else lo = mid + 1;
    }
    return -2;
}

// reg2bin (SAMv1 §5.3) of [beg, end)
__device__ __forceinline__ int reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// One record from the line [s, end) ('\n' at end).  Returns 0 and the record's bytes in o.n (block_size + 4), or a BamRefusal.
template <bool EMIT> __device__ unsigned bam_record(const BamArgs &A, int64_t s, int64_t end, Out<EMIT> &o) {
    const char *t = A.text;
    int64_t f[12];                        // field k is [f[k], sep[k])
    int64_t sep[11];
    int64_t p = s;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
        f[k] = p;
        sep[k] = next_sep(t, p, end);
        if (sep[k] == end && k < 10) return kBadLine;
        p = sep[k] + 1;
    }
    f[11] = p;                            // the aux fields, up to end
    int64_t flag, pos, mapq, pnext, tlen;
    if (!parse_int(t, f[1], sep[1], &flag) || flag < 0 || flag > 0xFFFF || !parse_int(t, f[3], sep[3], &pos) || pos < 0 ||
        pos > 0x7FFFFFFFLL || !parse_int(t, f[4], sep[4], &mapq) || mapq < 0 || mapq > 255 || !parse_int(t, f[7], sep[7], &pnext) ||
        pnext < 0 || pnext > 0x7FFFFFFFLL || !parse_int(t, f[8], sep[8], &tlen) || tlen < INT32_MIN || tlen > INT32_MAX)
        return kBadLine;
    const int64_t l_name = sep[0] - f[0];
    if (l_name < 1) return kBadLine;
    if (l_name > 254) return kLongName;
    const int rid = ref_id(A, t, f[2], sep[2]);
    int nrid = (sep[6] - f[6] == 1 && t[f[6]] == '=') ? rid : ref_id(A, t, f[6], sep[6]);
    if (rid == -2 || nrid == -2) return kBadLine;
    // CIGAR: ops and reference length
    int64_t n_cig = 0, rlen = 0;
    const bool no_cig = sep[5] - f[5] == 1 && t[f[5]] == '*';
    if (!no_cig) {
        int64_t len = 0;
        bool digits = false;
        for (int64_t i = f[5]; i < sep[5]; ++i) {
            const char c = t[i];
            if (c >= '0' && c <= '9') {
                len = len * 10 + (c - '0');
                if (len >= (1 << 28)) return kBadLine;
                digits = true;
                continue;
            }
            const int op = cigar_op(c);
            if (op < 0 || !digits) return kBadLine;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += len;
            ++n_cig;
            len = 0;
            digits = false;
        }
        if (digits || n_cig == 0) return kBadLine;
        if (n_cig > 0xFFFF) return kManyOps;
    }
    const bool no_seq = sep[9] - f[9] == 1 && t[f[9]] == '*', no_qual = sep[10] - f[10] == 1 && t[f[10]] == '*';
    const int64_t l_seq = no_seq ? 0 : sep[9] - f[9];
    if (!no_qual && sep[10] - f[10] != l_seq) return kSeqQual;
    const int64_t pos0 = pos - 1;
    const int64_t endpos = ((flag & 4) || n_cig == 0 || rlen == 0) ? pos0 + 1 : pos0 + rlen;
    const int64_t start = o.n;
    o.u32(0);                             // block_size, stored at the end
    o.u32((uint32_t)rid);
    o.u32((uint32_t)pos0);
    o.b((uint32_t)(l_name + 1));
    o.b((uint32_t)mapq);
    o.u16((uint32_t)reg2bin(pos0, endpos));
    o.u16((uint32_t)n_cig);
    o.u16((uint32_t)flag);
    o.u32((uint32_t)l_seq);
    o.u32((uint32_t)nrid);
    o.u32((uint32_t)(pnext - 1));
    o.u32((uint32_t)(int32_t)tlen);
    o.copy(t + f[0], l_name, 0);
    o.b(0);
    if (!no_cig) {
        int64_t len = 0;
        for (int64_t i = f[5]; i < sep[5]; ++i) {
            const char c = t[i];
            if (c >= '0' && c <= '9') { len = len * 10 + (c - '0'); continue; }
            o.u32((uint32_t)(len << 4 | cigar_op(c)));
            len = 0;
        }
    }
    o.seq(t + f[9], l_seq);
    if (no_qual) o.fill(0xFF, l_seq);
    else o.copy(t + f[10], l_seq, 33);
    // aux fields: TG:T:value
    for (p = f[11]; sep[10] < end;) {                   // a tab after QUAL starts a field (an empty one is refused)
        const int64_t e = next_sep(t, p, end);
        if (e - p < 5 || t[p + 2] != ':' || t[p + 4] != ':') return kBadAux;
        const char ty = t[p + 3];
        const int64_t v = p + 5;
        o.b((uint8_t)t[p]);
        o.b((uint8_t)t[p + 1]);
        if (ty == 'A') {
            if (e - v != 1) return kBadAux;
            o.b('A');
            o.b((uint8_t)t[v]);
        } else if (ty == 'i') {
            int64_t x;
            if (!parse_int(t, v, e, &x)) return kBadAux;
            if (x < INT32_MIN || x > 0xFFFFFFFFLL) return kBadInt;
            if (x < 0) {
                if (x >= -128) { o.b('c'); o.b((uint32_t)x); }
                else if (x >= -32768) { o.b('s'); o.u16((uint32_t)x); }
                else { o.b('i'); o.u32((uint32_t)x); }
            } else if (x <= 255) { o.b('C'); o.b((uint32_t)x); }
            else if (x <= 65535) { o.b('S'); o.u16((uint32_t)x); }
            else { o.b('I'); o.u32((uint32_t)x); }
        } else if (ty == 'f') {
            float x;
            if (!parse_float(t, v, e, &x)) return kBadAux;
            o.b('f');
            o.u32(__float_as_uint(x));
        } else if (ty == 'Z' || ty == 'H') {
            o.b((uint8_t)ty);
            o.copy(t + v, e - v, 0);
            o.b(0);
        } else {
            return kBadAux;                       // B arrays and unknown types
        }
        if (e == end) break;
        p = e + 1;
    }
    const int64_t bs = o.n - start - 4;
    if (EMIT && group_lane() == 0 && start + 3 < o.lim) {
        o.p[start] = (uint8_t)bs; o.p[start + 1] = (uint8_t)(bs >> 8); o.p[start + 2] = (uint8_t)(bs >> 16); o.p[start + 3] = (uint8_t)(bs >> 24);
    }
    return 0;
}

__device__ __forceinline__ int64_t line_start(const BamArgs &A, int64_t r) { return r == 0 ? 0 : A.line_end[r - 1] + 1; }

// sizes (block_size + 4) of every record; a refusal sets bad[0] = min(read << 8 | reason)
__global__ void __launch_bounds__(256) bam_count_kernel(BamArgs A) {
    const int64_t n_groups = (int64_t)gridDim.x * (blockDim.x / kGroup);
    for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup; r < A.n_rec; r += n_groups) {
        const int64_t s = line_start(A, r);
        Out<false> o{nullptr, 0, 0};
        const unsigned why = bam_record<false>(A, s, A.line_end[r], o);
        if (group_lane() == 0) {
            A.size[r] = why ? 0 : o.n;
            if (why) {
                int64_t lo = 0, hi = A.nseq;              // the read whose text holds the line: last i with read_off[i] <= s
                while (lo < hi) {
                    const int64_t mid = (lo + hi + 1) >> 1;
                    if (A.read_off[mid] <= s) lo = mid;
                    else hi = mid - 1;
                }
                atomicMin(A.bad, (unsigned long long)lo << 8 | why);
            }
        }
    }
}

__global__ void __launch_bounds__(256) bam_write_kernel(BamArgs A) {
    const int64_t n_groups = (int64_t)gridDim.x * (blockDim.x / kGroup);
    for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup; r < A.n_rec; r += n_groups) {
        Out<true> o{A.out, A.rec_off[r], A.rec_off[r + 1]};
        (void)bam_record<true>(A, line_start(A, r), A.line_end[r], o);
    }
}

// a read's records start at the record of its first line: bam_off[i] = rec_off[#line ends before read_off[i]]
__global__ void __launch_bounds__(256) bam_read_off_kernel(BamArgs A, int64_t *bam_off) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= A.nseq; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t at = A.read_off[i];
        int64_t lo = 0, hi = A.n_rec;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (A.line_end[mid] < at) lo = mid + 1;
            else hi = mid;
        }
        bam_off[i] = A.rec_off[lo];
    }
}

}  // namespace

void launch_bam_count(const BamArgs &A, int cu_count, hipStream_t st) {
    if (A.n_rec > 0) bam_count_kernel<<<grid_of(A.n_rec, 256 / kGroup, cu_count), 256, 0, st>>>(A);
}

void launch_bam_write(const BamArgs &A, int64_t *bam_off, int cu_count, hipStream_t st) {
    if (A.n_rec > 0) bam_write_kernel<<<grid_of(A.n_rec, 256 / kGroup, cu_count), 256, 0, st>>>(A);
    bam_read_off_kernel<<<grid_of(A.nseq + 1, 256, cu_count), 256, 0, st>>>(A, bam_off);
}

// The eager RNAME lookup of bwams_index_set_contig_names: the host copy of the names, their sorted permutation on the device, and
// whether two names are equal (the BAM entry points refuse such an index: a name would not say which refID it is).
int bam_names_index(bwams_index *ix, const char *names, const int32_t *name_off, int32_t n) {
    std::vector<int32_t> perm((size_t)n);
    for (int32_t i = 0; i < n; ++i) perm[(size_t)i] = i;
    std::sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) { return strcmp(names + name_off[a], names + name_off[b]) < 0; });
    bool dup = false;
    for (int32_t i = 1; i < n; ++i) dup |= strcmp(names + name_off[perm[(size_t)i - 1]], names + name_off[perm[(size_t)i]]) == 0;
    ix->d_ctg_sorted.release();
    ix->h_ctg_names.clear();
    BWAMS_HIP(ix->d_ctg_sorted.alloc((size_t)n * 4));
    BWAMS_HIP(hipMemcpy(ix->d_ctg_sorted.p, perm.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    for (int32_t i = 0; i < n; ++i) ix->h_ctg_names.emplace_back(names + name_off[i]);
    ix->ctg_dup = dup;
    return BWAMS_OK;
}

}  // namespace bwams

using namespace bwams;

namespace {

// the index's sequences as the header needs them: names (host copy), lengths and is_alt (from the device table)
int header_seqs(const bwams_index_t *idx, const char *who, std::vector<bwams_contig_t> *c) {
    if (!idx || !idx->d_contigs.p || (int64_t)idx->h_ctg_names.size() != idx->n_seqs) {
        set_last_error(std::string(who) + ": the index has no sequence names (bwams_index_set_contig_names)");
        return BWAMS_ERR_ARG;
    }
    c->resize((size_t)idx->n_seqs);
    BWAMS_HIP(hipSetDevice(idx->device));
    BWAMS_HIP(hipMemcpy(c->data(), idx->d_contigs.p, c->size() * sizeof(bwams_contig_t), hipMemcpyDeviceToHost));
    return BWAMS_OK;
}

int put_out(const std::string &s, void *out, int64_t cap, int64_t *n_out) {
    if (n_out) *n_out = (int64_t)s.size();
    if ((int64_t)s.size() > cap || (!out && !s.empty())) return BWAMS_ERR_CAPACITY;
    if (!s.empty()) memcpy(out, s.data(), s.size());
    return BWAMS_OK;
}

}  // namespace

extern "C" {

int bwams_sam_header(const bwams_index_t *idx, const char *hdr_line, const char *pg_line, char *out, int64_t cap, int64_t *n_out) {
    if (!n_out || cap < 0) return BWAMS_ERR_ARG;
    std::vector<bwams_contig_t> c;
    if (int rc = header_seqs(idx, "bwams_sam_header", &c)) return rc;
    int n_sq = 0;                                             // @SQ lines the -H text carries already
    if (hdr_line)
        for (const char *p = hdr_line; (p = strstr(p, "@SQ\t")) != nullptr; p += 4)
            if (p == hdr_line || p[-1] == '\n') ++n_sq;
    std::string s;
    if (n_sq == 0)
        for (size_t i = 0; i < c.size(); ++i) {
            char buf[500];                                    // the line is cut at 498 bytes, as bwa_print_sam_hdr's buffer cuts it
            snprintf(buf, 499, "@SQ\tSN:%s\tLN:%d", idx->h_ctg_names[i].c_str(), c[i].len);
            s += buf;
            s += c[i].is_alt ? "\tAH:*\n" : "\n";
        }
    if (hdr_line) { s += hdr_line; s += '\n'; }
    if (pg_line) s += pg_line;
    return put_out(s, out, cap, n_out);
}

int bwams_bam_header(const bwams_index_t *idx, const char *text, int64_t n_text, void *out, int64_t cap, int64_t *n_out) {
    if (!n_out || cap < 0 || n_text < 0 || (n_text && !text) || n_text > 0x7FFFFFFFLL) return BWAMS_ERR_ARG;
    std::vector<bwams_contig_t> c;
    if (int rc = header_seqs(idx, "bwams_bam_header", &c)) return rc;
    std::string s("BAM\1", 4);
    auto u32 = [&](uint32_t v) { for (int k = 0; k < 4; ++k) s.push_back((char)(v >> (8 * k))); };
    u32((uint32_t)n_text);
    s.append(text ? text : "", (size_t)n_text);
    u32((uint32_t)c.size());
    for (size_t i = 0; i < c.size(); ++i) {
        const std::string &nm = idx->h_ctg_names[i];
        u32((uint32_t)nm.size() + 1);
        s.append(nm);
        s.push_back('\0');
        u32((uint32_t)c[i].len);
    }
    return put_out(s, out, cap, n_out);
}

}  // extern "C"
