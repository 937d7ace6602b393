// fasta_ref.hip — a reference FASTA becomes an index on the device.
//
// Replaces bns_fasta2bntseq (reference src/bntseq.cpp:269-372, for_only = 1) as bwa_idx_build_mem2 calls it
// (src/bwtindex.cpp:377-394) ahead of FMI_search::build_index: kseq_read's FASTA grammar (src/kseq.h:358-400, OPT_RW), the
// base codes of nst_nt4_table with every code >= 4 replaced by lrand48() & 3 after srand48(11), the holes of add1 (a run of one
// ambiguous byte value inside one contig), the 2-bit .pac (_set_pac: first base in the high bits), and bns_dump's .ann / .amb.
// bns_restore (src/bntseq.cpp:114-246) is here too, as bwams_index_load_bns.
//
// Mapping.  HBM streaming over bytes, lane per 16 bytes, no MFMA:
//   (1) line ends: fastq.hip's index (line_ends); (2) a lane per line: header / sequence / empty, the CR rule, the bytes it adds;
//   (3) exclusive scan of those into each line's base position (a header line's position is its contig's offset);
//   (4) lane per 16 text bytes: the kept bytes into a raw array of l_pac bytes (one binary search per lane, then a cursor);
//   (5) lane per 16 bases: ambiguous bases, hole starts, hole ends (previous / next raw byte and the contig starts); three scans;
//   (6) lane per 16 bases: codes (an ambiguous base of global rank r takes lrand48 draw r + 1: the state at the lane's first rank
//       by jump-ahead over a 48-entry table of 2^i-step affine maps, then one step per base), 4 .pac bytes, the hole records.
// Header lines are few: their bytes go to the host, where names and comments are cut as kseq cuts them.  The codes stay in HBM
// and go to fmi_build_device; the text and every temporary are freed before it starts.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "common.h"

namespace bwams {
int fmi_build_device(bwams_index *ix, const uint8_t *d_fw, int64_t l_pac, int keep_ref, int64_t chunk_rows, int verbose,
                     bwams_build_stats_t *bs);                   // fmi_build.hip

namespace {

constexpr uint64_t kLcgA = 0x5DEECE66DULL, kLcgC = 0xB, kLcgMask = (1ULL << 48) - 1;
constexpr uint32_t kSeed = 11;                                   // bns->seed (src/bntseq.cpp:284)

// x -> a x + c (mod 2^48) for 2^i steps of glibc's lrand48 generator
struct LcgJump {
    uint64_t a[48], c[48];
};

LcgJump make_jump() {
    LcgJump j;
    uint64_t a = kLcgA, c = kLcgC;
    for (int i = 0; i < 48; ++i) {
        j.a[i] = a; j.c[i] = c;
        c = (a * c + c) & kLcgMask;                              // the map composed with itself
        a = (a * a) & kLcgMask;
    }
    return j;
}

__constant__ unsigned char kNt4Ref[256] = {      // nst_nt4_table (src/bntseq.cpp:64-81)
    4,4,4,4,4,4,4,4,4,4,4,4,4,4,4,4, 4,4,4,4,4,4,4,4,4,4,4,4,4,4,4,4, 4,4,4,4,4,4,4,4,4,4,4,4,4,5,4,4, 4,4,4,4,4,4,4,4,4,4,4,4,4,4,4,4,
    4,0,4,1,4,4,4,2,4,4,4,4,4,4,4,4, 4,4,4,4,3,4,4,4,4,4,4,4,4,4,4,4, 4,0,4,1,4,4,4,2,4,4,4,4,4,4,4,4, 4,4,4,4,3,4,4,4,4,4,4,4,4,4,4,4,
    4,4,4,4,4,4,4,4,4,4,4,4,4,4,4,4, 4,4,4,4,4,4,4,4,4,4,4,4,4,4,4,4, 4,4,4,4,4,4,4,4,4,4,4,4,4,4,4,4, 4,4,4,4,4,4,4,4,4,4,4,4,4,4,4,4,
    4,4,4,4,4,4,4,4,4,4,4,4,4,4,4,4, 4,4,4,4,4,4,4,4,4,4,4,4,4,4,4,4, 4,4,4,4,4,4,4,4,4,4,4,4,4,4,4,4, 4,4,4,4,4,4,4,4,4,4,4,4,4,4,4,4};

enum : uint8_t { kEmpty = 0, kHeader = 1, kSeq = 2 };

// 16 bytes from p[0, min(16, n)): one 16-byte load when the piece is whole and aligned, bytes otherwise
__device__ __forceinline__ void load16(const uint8_t *__restrict__ p, int64_t n, uint8_t v[16]) {
    if (n >= 16 && ((uintptr_t)p & 15) == 0) {
        const uint4 w = *reinterpret_cast<const uint4 *>(p);
        memcpy(v, &w, 16);
    } else {
        for (int j = 0; j < 16; ++j) v[j] = j < n ? p[j] : 0;
    }
}

// first index i in a[0, n) with a[i] >= x
__device__ __forceinline__ int64_t lower_bound64(const int64_t *__restrict__ a, int64_t n, int64_t x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// position of the first '>' or '@' (kseq_read skips every byte before it, even in mid-line)
__global__ __launch_bounds__(256) void fa_first_kernel(const uint8_t *__restrict__ text, int64_t n, unsigned long long *first) {
    const int64_t n16 = (n + 15) / 16;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n16; k += (int64_t)gridDim.x * blockDim.x) {
        uint8_t v[16];
        load16(text + k * 16, n - k * 16, v);
        for (int j = 0; j < 16 && k * 16 + j < n; ++j)
            if (v[j] == '>' || v[j] == '@') { atomicMin(first, (unsigned long long)(k * 16 + j)); break; }
    }
}

// a lane per line [b, e): its kind and the bytes it adds to its record's sequence.  Line 0 is the first header.  A sequence line
// adds its bytes (ks_getuntil_line2 appends them) less one trailing '\r' when the record's accumulated string is then longer than one
// byte; a lone "\r" is that record's first byte only when no non-empty sequence line came before it in the record, and a lone "\r"
// ending the text without '\n' is always kept (the append returns at EOF before its CR test).  '+' at a line start = FASTQ.
__global__ __launch_bounds__(256) void fa_line_kernel(const uint8_t *__restrict__ text, int64_t n, const int64_t *__restrict__ ends,
                                                      int64_t n_nl, int64_t n_lines, int64_t *__restrict__ contrib,
                                                      uint8_t *__restrict__ kind, unsigned long long *bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_lines) return;
    const int64_t b = i ? ends[i - 1] + 1 : 0, e = i < n_nl ? ends[i] : n;
    const int64_t k = e - b;
    uint8_t kd = kEmpty;
    int64_t add = 0;
    if (i == 0) kd = kHeader;
    else if (k > 0) {
        const uint8_t c0 = text[b];
        if (c0 == '>' || c0 == '@') kd = kHeader;
        else if (c0 == '+') atomicOr(bad, 1ULL);
        else {
            kd = kSeq;
            add = k;
            if (text[e - 1] == '\r') {
                if (k >= 2) --add;
                else if (i < n_nl) {                         // a lone "\r": dropped when the record already holds a base
                    int64_t j = i - 1;
                    while (j > 0 && ends[j] == (j ? ends[j - 1] + 1 : 0)) --j;   // skip the empty lines before it
                    const int64_t bj = j ? ends[j - 1] + 1 : 0;
                    const bool after_header = j == 0 || text[bj] == '>' || text[bj] == '@';
                    if (!after_header) add = 0;
                }
            }
        }
    }
    kind[i] = kd;
    contrib[i] = add;
}

// a lane per 16 text bytes: the bytes each sequence line keeps, at their base positions
__global__ __launch_bounds__(256) void fa_raw_kernel(const uint8_t *__restrict__ text, int64_t n, const int64_t *__restrict__ ends,
                                                     int64_t n_nl, const int64_t *__restrict__ contrib, const int64_t *__restrict__ off,
                                                     uint8_t *__restrict__ raw) {
    const int64_t c = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (c >= n) return;
    uint8_t v[16];
    load16(text + c, n - c, v);
    int64_t L = lower_bound64(ends, n_nl, c);             // the line holding byte c
    int64_t b = L ? ends[L - 1] + 1 : 0, e = L < n_nl ? ends[L] : n;
    int64_t keep = contrib[L], at = off[L];
    for (int j = 0; j < 16; ++j) {
        const int64_t p = c + j;
        if (p >= n) break;
        while (p > e) {
            ++L;
            b = e + 1;
            e = L < n_nl ? ends[L] : n;
            keep = contrib[L]; at = off[L];
        }
        if (p < e && p - b < keep) raw[at + (p - b)] = v[j];
    }
}

// monotone cursor over the sorted contig offsets: is q the first base of some contig?
struct CtgCursor {
    const int64_t *off;
    int64_t n, i, nb;
    __device__ void init(const int64_t *o, int64_t n_, int64_t from) {
        off = o; n = n_;
        i = lower_bound64(o, n_, from);
        nb = i < n ? o[i] : INT64_MAX;
    }
    __device__ bool starts_at(int64_t q) {
        while (nb < q) { ++i; nb = i < n ? off[i] : INT64_MAX; }
        return nb == q;
    }
};

// the base at p: ambiguous; begins a hole (add1: the byte differs from the previous raw byte of its contig); ends one
__device__ __forceinline__ void base_flags(const uint8_t *__restrict__ raw, int64_t l_pac, int64_t p, uint8_t x, CtgCursor &cc,
                                           bool &amb, bool &hs, bool &he) {
    amb = kNt4Ref[x] >= 4;
    hs = he = false;
    if (!amb) return;
    hs = p == 0 || cc.starts_at(p) || raw[p - 1] != x;
    he = p + 1 == l_pac || cc.starts_at(p + 1) || raw[p + 1] != x;
}

// a lane per 16 bases: ambiguous bases | hole starts << 8 | hole ends << 16
__global__ __launch_bounds__(256) void fa_count_kernel(const uint8_t *__restrict__ raw, int64_t l_pac, const int64_t *__restrict__ ctg_off,
                                                       int64_t n_seqs, uint32_t *__restrict__ cnt) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, c = k * 16;
    if (c >= l_pac) return;
    uint8_t v[16];
    load16(raw + c, l_pac - c, v);
    CtgCursor cc;
    cc.init(ctg_off, n_seqs, c);
    uint32_t na = 0, ns = 0, ne = 0;
    for (int j = 0; j < 16 && c + j < l_pac; ++j) {
        bool a, s, e;
        base_flags(raw, l_pac, c + j, v[j], cc, a, s, e);
        na += a; ns += s; ne += e;
    }
    cnt[k] = na | ns << 8 | ne << 16;
}

struct CountField {
    int shift;
    __host__ __device__ uint64_t operator()(const uint32_t &x) const { return (x >> shift) & 0xff; }
};

// a lane per 16 bases: codes (lrand48 draws by global rank), 4 .pac bytes, the hole records
__global__ __launch_bounds__(256) void fa_emit_kernel(const uint8_t *__restrict__ raw, int64_t l_pac, const int64_t *__restrict__ ctg_off,
                                                      int64_t n_seqs, const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ r_amb,
                                                      const uint64_t *__restrict__ r_hs, const uint64_t *__restrict__ r_he, LcgJump jmp,
                                                      uint8_t *__restrict__ fw, uint8_t *__restrict__ pac, int64_t *__restrict__ hole_b,
                                                      int64_t *__restrict__ hole_e, uint8_t *__restrict__ hole_amb) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, c = k * 16;
    if (c >= l_pac) return;
    uint8_t v[16];
    load16(raw + c, l_pac - c, v);
    uint64_t x = ((uint64_t)kSeed << 16) | 0x330E;            // srand48(11)
    if (cnt[k] & 0xff) {                                         // jump to the state after r_amb[k] draws
        const uint64_t r = r_amb[k];
        for (int i = 0; i < 48; ++i)
            if ((r >> i) & 1) x = (jmp.a[i] * x + jmp.c[i]) & kLcgMask;
    }
    CtgCursor cc;
    cc.init(ctg_off, n_seqs, c);
    uint64_t hs = r_hs[k], he = r_he[k];
    uint8_t code[16];
    for (int j = 0; j < 16; ++j) {
        const int64_t p = c + j;
        if (p >= l_pac) { code[j] = 0; continue; }
        bool a, s, e;
        base_flags(raw, l_pac, p, v[j], cc, a, s, e);
        uint8_t cd = kNt4Ref[v[j]];
        if (a) {
            x = (kLcgA * x + kLcgC) & kLcgMask;
            cd = (uint8_t)((x >> 17) & 3);                       // lrand48() & 3
        }
        if (s) { hole_b[hs] = p; hole_amb[hs] = v[j]; ++hs; }
        if (e) { hole_e[he] = p + 1; ++he; }
        code[j] = cd;
    }
    uint4 w;
    memcpy(&w, code, 16);
    *reinterpret_cast<uint4 *>(fw + c) = w;                      // fw has 16 bytes of slack
    uint32_t pk = 0;
    for (int q = 0; q < 4; ++q)
        pk |= (uint32_t)(code[4 * q] << 6 | code[4 * q + 1] << 4 | code[4 * q + 2] << 2 | code[4 * q + 3]) << (8 * q);
    *reinterpret_cast<uint32_t *>(pac + k * 4) = pk;
}

template <class In, class Out> hipError_t exscan(In in, Out out, size_t n, hipStream_t st) {
    using T = typename std::iterator_traits<Out>::value_type;
    size_t tb = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, tb, in, out, (T)0, n, rocprim::plus<T>(), st);
    DevBuf<> tmp;
    if (e == hipSuccess) e = tmp.alloc(tb + 16);
    if (e == hipSuccess) e = rocprim::exclusive_scan(tmp.p, tb, in, out, (T)0, n, rocprim::plus<T>(), st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
}

struct HeaderPos { int64_t b, e, off; };

__global__ void fa_header_kernel(const int64_t *__restrict__ hdr, int64_t n_seqs, const int64_t *__restrict__ ends, int64_t n_nl, int64_t n,
                                 const int64_t *__restrict__ off, HeaderPos *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_seqs) return;
    const int64_t L = hdr[i];
    out[i].b = L ? ends[L - 1] + 1 : 0;
    out[i].e = L < n_nl ? ends[L] : n;
    out[i].off = off[L];
}

struct IsHeader {
    const uint8_t *kind;
    __device__ bool operator()(const int64_t &i) const { return kind[i] == kHeader; }
};

inline bool c_isspace(unsigned char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

// kseq_read on one header line (without its '\n'; hdr[0] is the '>' or '@'): name up to the first isspace(), then — unless that
// byte ended the line — the rest of the line is the comment, less a trailing '\r' when longer than one byte (ks_getuntil_line)
void cut_header(const char *h, int64_t len, std::string *name, std::string *comment) {
    int64_t p = 1;
    while (p < len && !c_isspace((unsigned char)h[p])) ++p;
    name->assign(h + 1, (size_t)(p - 1));
    comment->clear();
    if (p < len) {                                     // the delimiter was a space / tab / CR: the comment follows it
        comment->assign(h + p + 1, (size_t)(len - p - 1));
        if (comment->size() > 1 && comment->back() == '\r') comment->pop_back();
    }
}

// text already in HBM -> codes in HBM (into *fw, l_pac + 16 bytes) and the bns in *m (its .pac in HBM)
int fasta_pack(const uint8_t *d_text, int64_t n_bytes, hipStream_t st, BnsMeta *m, DevBuf<uint8_t> *fw, int64_t *n_ambig) {
    if (n_bytes <= 0) {
        set_last_error("bwams_index_from_fasta: empty text");
        return BWAMS_ERR_ARG;
    }
    // the device temporaries of the pack, freed when it returns (the line tables once the bytes are placed)
    DevBuf<unsigned long long> flag;
    DevBuf<int64_t> ends, contrib, offs, hdrs, cnt, ctg, hole_b, hole_e;
    DevBuf<uint8_t> kind, raw, hole_amb;
    DevBuf<HeaderPos> hps;
    DevBuf<char> hdr_bytes;
    DevBuf<uint32_t> cnt16;
    DevBuf<uint64_t> ra, rs, re;
    BWAMS_HIP(flag.alloc(64));
    unsigned long long *d_flag = flag.p;
    // where the first record begins
    uint8_t b0 = 0;
    BWAMS_HIP(hipMemcpy(&b0, d_text, 1, hipMemcpyDeviceToHost));
    int64_t p0 = 0;
    if (b0 != '>' && b0 != '@') {
        const unsigned long long none = ~0ULL;
        BWAMS_HIP(hipMemcpyAsync(d_flag, &none, 8, hipMemcpyHostToDevice, st));
        fa_first_kernel<<<2048, 256, 0, st>>>(d_text, n_bytes, d_flag);
        BWAMS_HIP(hipGetLastError());
        unsigned long long f = 0;
        BWAMS_HIP(hipMemcpyAsync(&f, d_flag, 8, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipStreamSynchronize(st));
        if (f == none) {
            set_last_error("bwams_index_from_fasta: no '>' header in the text");
            return BWAMS_ERR_ARG;
        }
        p0 = (int64_t)f;
    }
    const uint8_t *t = d_text + p0;
    const int64_t n = n_bytes - p0;
    // (1) lines
    int64_t n_nl = 0;
    {
        int rc = line_ends(reinterpret_cast<const char *>(t), n, st, &ends, &n_nl);
        if (rc) return rc;
    }
    const int64_t *d_ends = ends.p;
    uint8_t last = 0;
    BWAMS_HIP(hipMemcpy(&last, t + n - 1, 1, hipMemcpyDeviceToHost));
    const int64_t n_lines = n_nl + (last != '\n' ? 1 : 0);
    // (2) kinds and contributions, (3) base positions
    BWAMS_HIP(contrib.alloc((size_t)(n_lines + 1) * 8));
    BWAMS_HIP(offs.alloc((size_t)(n_lines + 1) * 8));
    BWAMS_HIP(kind.alloc((size_t)n_lines + 16));
    int64_t *d_contrib = contrib.p, *d_off = offs.p;
    uint8_t *d_kind = kind.p;
    BWAMS_HIP(hipMemsetAsync(d_flag, 0, 8, st));
    fa_line_kernel<<<(unsigned)((n_lines + 255) / 256), 256, 0, st>>>(t, n, d_ends, n_nl, n_lines, d_contrib, d_kind, d_flag);
    BWAMS_HIP(hipGetLastError());
    BWAMS_HIP(hipMemsetAsync(d_contrib + n_lines, 0, 8, st));
    BWAMS_HIP(exscan(d_contrib, d_off, (size_t)n_lines + 1, st));
    unsigned long long bad = 0;
    int64_t l_pac = 0;
    BWAMS_HIP(hipMemcpy(&bad, d_flag, 8, hipMemcpyDeviceToHost));
    BWAMS_HIP(hipMemcpy(&l_pac, d_off + n_lines, 8, hipMemcpyDeviceToHost));
    if (bad) {
        set_last_error("bwams_index_from_fasta: a line starts with '+' (FASTQ text is not a reference)");
        return BWAMS_ERR_UNSUPPORTED;
    }
    // headers: positions on the device, bytes to the host
    int64_t n_seqs = 0;
    BWAMS_HIP(cnt.alloc(64));
    BWAMS_HIP(hdrs.alloc((size_t)n_lines * 8 + 16));
    int64_t *d_hdr = hdrs.p, *d_cnt = cnt.p;
    {
        rocprim::counting_iterator<int64_t> it(0);
        IsHeader pred{d_kind};
        size_t tb = 0;
        BWAMS_HIP(rocprim::select(nullptr, tb, it, d_hdr, d_cnt, (size_t)n_lines, pred, st));
        DevBuf<> tmp;
        BWAMS_HIP(tmp.alloc(tb + 16));
        BWAMS_HIP(rocprim::select(tmp.p, tb, it, d_hdr, d_cnt, (size_t)n_lines, pred, st));
        BWAMS_HIP(hipMemcpyAsync(&n_seqs, d_cnt, 8, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipStreamSynchronize(st));
    }
    if (n_seqs > 0x7fffffffLL) {
        set_last_error("bwams_index_from_fasta: more than 2^31 - 1 sequences");
        return BWAMS_ERR_UNSUPPORTED;
    }
    std::vector<HeaderPos> hp((size_t)n_seqs);
    {
        BWAMS_HIP(hps.alloc((size_t)n_seqs * sizeof(HeaderPos)));
        HeaderPos *d_hp = hps.p;
        fa_header_kernel<<<(unsigned)((n_seqs + 255) / 256), 256, 0, st>>>(d_hdr, n_seqs, d_ends, n_nl, n, d_off, d_hp);
        BWAMS_HIP(hipGetLastError());
        BWAMS_HIP(hipMemcpyAsync(hp.data(), d_hp, (size_t)n_seqs * sizeof(HeaderPos), hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipStreamSynchronize(st));
    }
    // a '>' that is the text's last byte starts no record (ks_getuntil_space returns -1 at EOF when it read nothing)
    if (n_seqs && hp.back().b + 1 == n && hp.back().e == n) { hp.pop_back(); --n_seqs; }
    std::vector<char> hbytes;
    std::vector<int64_t> hoff((size_t)n_seqs + 1, 0);
    {
        for (int64_t i = 0; i < n_seqs; ++i) hoff[(size_t)i + 1] = hoff[(size_t)i] + (hp[(size_t)i].e - hp[(size_t)i].b);
        BWAMS_HIP(hdr_bytes.alloc((size_t)hoff[(size_t)n_seqs] + 16));
        char *d_hb = hdr_bytes.p;
        std::vector<SegMove> mv;
        mv.reserve((size_t)n_seqs);
        for (int64_t i = 0; i < n_seqs; ++i)
            mv.push_back({reinterpret_cast<const char *>(t) + hp[(size_t)i].b, d_hb + hoff[(size_t)i], hp[(size_t)i].e - hp[(size_t)i].b});
        int rc = segment_copy(mv, st);
        if (rc) return rc;
        hbytes.resize((size_t)hoff[(size_t)n_seqs] + 1);
        BWAMS_HIP(hipMemcpyAsync(hbytes.data(), d_hb, (size_t)hoff[(size_t)n_seqs], hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipStreamSynchronize(st));
    }
    m->l_pac = l_pac;
    m->names.resize((size_t)n_seqs);
    m->comments.resize((size_t)n_seqs);
    m->ctg_off.resize((size_t)n_seqs);
    m->ctg_len.resize((size_t)n_seqs);
    m->ctg_ambs.assign((size_t)n_seqs, 0);
    for (int64_t i = 0; i < n_seqs; ++i) {
        cut_header(hbytes.data() + hoff[(size_t)i], hoff[(size_t)i + 1] - hoff[(size_t)i], &m->names[(size_t)i], &m->comments[(size_t)i]);
        const int64_t o = hp[(size_t)i].off, next = i + 1 < n_seqs ? hp[(size_t)i + 1].off : l_pac;
        if (next - o > 0x7fffffffLL) {
            set_last_error("bwams_index_from_fasta: sequence '" + m->names[(size_t)i] + "' is longer than 2^31 - 1 bases");
            return BWAMS_ERR_UNSUPPORTED;
        }
        m->ctg_off[(size_t)i] = o;
        m->ctg_len[(size_t)i] = (int32_t)(next - o);
    }
    if (l_pac <= 0) {
        set_last_error("bwams_index_from_fasta: the text holds no bases");
        return BWAMS_ERR_ARG;
    }
    // (4) the kept bytes, at their base positions
    BWAMS_HIP(raw.alloc((size_t)l_pac + 16));
    const uint8_t *d_raw = raw.p;
    {
        const int64_t lanes = (n + 15) / 16;
        fa_raw_kernel<<<(unsigned)((lanes + 255) / 256), 256, 0, st>>>(t, n, d_ends, n_nl, d_contrib, d_off, raw.p);
        BWAMS_HIP(hipGetLastError());
        BWAMS_HIP(hipStreamSynchronize(st));
    }
    ends.release(); contrib.release(); offs.release(); kind.release(); hdrs.release();
    // (5) ambiguous bases and holes per 16 bases, three scans
    BWAMS_HIP(ctg.alloc((size_t)n_seqs * 8 + 8));
    const int64_t *d_ctg = ctg.p;
    BWAMS_HIP(hipMemcpy(ctg.p, m->ctg_off.data(), (size_t)n_seqs * 8, hipMemcpyHostToDevice));
    const int64_t n16 = (l_pac + 15) / 16;
    const unsigned grid = (unsigned)((n16 + 255) / 256);
    BWAMS_HIP(cnt16.alloc((size_t)(n16 + 1) * 4));
    BWAMS_HIP(ra.alloc((size_t)(n16 + 1) * 8));
    BWAMS_HIP(rs.alloc((size_t)(n16 + 1) * 8));
    BWAMS_HIP(re.alloc((size_t)(n16 + 1) * 8));
    uint32_t *d_cnt16 = cnt16.p;
    uint64_t *d_ra = ra.p, *d_rs = rs.p, *d_re = re.p;
    fa_count_kernel<<<grid, 256, 0, st>>>(d_raw, l_pac, d_ctg, n_seqs, d_cnt16);
    BWAMS_HIP(hipGetLastError());
    BWAMS_HIP(hipMemsetAsync(d_cnt16 + n16, 0, 4, st));
    BWAMS_HIP(exscan(rocprim::make_transform_iterator(d_cnt16, CountField{0}), d_ra, (size_t)n16 + 1, st));
    BWAMS_HIP(exscan(rocprim::make_transform_iterator(d_cnt16, CountField{8}), d_rs, (size_t)n16 + 1, st));
    BWAMS_HIP(exscan(rocprim::make_transform_iterator(d_cnt16, CountField{16}), d_re, (size_t)n16 + 1, st));
    uint64_t tot[3] = {0, 0, 0};
    BWAMS_HIP(hipMemcpy(&tot[0], d_ra + n16, 8, hipMemcpyDeviceToHost));
    BWAMS_HIP(hipMemcpy(&tot[1], d_rs + n16, 8, hipMemcpyDeviceToHost));
    BWAMS_HIP(hipMemcpy(&tot[2], d_re + n16, 8, hipMemcpyDeviceToHost));
    if (tot[1] != tot[2] || tot[1] > 0x7fffffffULL) {
        set_last_error(tot[1] != tot[2] ? "bwams_index_from_fasta: internal error, hole starts and ends differ"
                                        : "bwams_index_from_fasta: more than 2^31 - 1 holes");
        return tot[1] != tot[2] ? BWAMS_ERR_DEVICE : BWAMS_ERR_UNSUPPORTED;
    }
    const int64_t n_holes = (int64_t)tot[1];
    // (6) codes, .pac, holes
    BWAMS_HIP(fw->alloc((size_t)n16 * 16 + 16));
    BWAMS_HIP(m->d_pac.alloc((size_t)n16 * 4 + 16));
    BWAMS_HIP(hole_b.alloc((size_t)n_holes * 8 + 8));
    BWAMS_HIP(hole_e.alloc((size_t)n_holes * 8 + 8));
    BWAMS_HIP(hole_amb.alloc((size_t)n_holes + 16));
    int64_t *d_hb = hole_b.p, *d_he = hole_e.p;
    uint8_t *d_hamb = hole_amb.p;
    fa_emit_kernel<<<grid, 256, 0, st>>>(d_raw, l_pac, d_ctg, n_seqs, d_cnt16, d_ra, d_rs, d_re, make_jump(), fw->p, m->d_pac.as<uint8_t>(), d_hb,
                                         d_he, d_hamb);
    BWAMS_HIP(hipGetLastError());
    std::vector<int64_t> hb((size_t)n_holes), he((size_t)n_holes);
    m->hole_amb.resize((size_t)n_holes);
    if (n_holes) {
        BWAMS_HIP(hipMemcpyAsync(hb.data(), d_hb, (size_t)n_holes * 8, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipMemcpyAsync(he.data(), d_he, (size_t)n_holes * 8, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipMemcpyAsync(m->hole_amb.data(), d_hamb, (size_t)n_holes, hipMemcpyDeviceToHost, st));
    }
    BWAMS_HIP(hipStreamSynchronize(st));
    m->hole_off = hb;
    m->hole_len.resize((size_t)n_holes);
    for (int64_t i = 0; i < n_holes; ++i) m->hole_len[(size_t)i] = (int32_t)(he[(size_t)i] - hb[(size_t)i]);
    for (int64_t i = 0; i < n_seqs; ++i) {               // n_ambs: the holes inside each contig
        const int64_t o = m->ctg_off[(size_t)i];
        m->ctg_ambs[(size_t)i] = (int32_t)(std::lower_bound(hb.begin(), hb.end(), o + m->ctg_len[(size_t)i]) -
                                           std::lower_bound(hb.begin(), hb.end(), o));
    }
    *n_ambig = (int64_t)tot[0];
    return BWAMS_OK;
}

// the handle carries its sequences as bwams_index_set_contigs / _names / _annos leave them (annotations as bns_restore reads
// them back: "(null)" = none)
int attach_contigs(bwams_index *ix, const std::vector<int64_t> &off, const std::vector<int32_t> &len, const std::vector<int32_t> &alt,
                   const std::vector<std::string> &names, const std::vector<std::string> &annos) {
    const size_t n = off.size();
    std::vector<bwams_contig_t> c(n);
    for (size_t i = 0; i < n; ++i) { c[i].offset = off[i]; c[i].len = len[i]; c[i].is_alt = alt.empty() ? 0 : alt[i]; }
    BWAMS_HIP(hipSetDevice(ix->device));
    BWAMS_HIP(ix->d_contigs.alloc(n * sizeof(bwams_contig_t)));
    BWAMS_HIP(hipMemcpy(ix->d_contigs.p, c.data(), n * sizeof(bwams_contig_t), hipMemcpyHostToDevice));
    ix->n_seqs = (int32_t)n;
    auto blob = [&](const std::vector<std::string> &s, std::string *b, std::vector<int32_t> *o) {
        o->assign(n + 1, 0);
        for (size_t i = 0; i < n; ++i) { (*o)[i] = (int32_t)b->size(); b->append(s[i]); b->push_back('\0'); }
        (*o)[n] = (int32_t)b->size();
    };
    std::string nb, ab;
    std::vector<int32_t> no, ao;
    blob(names, &nb, &no);
    blob(annos, &ab, &ao);
    int rc = bwams_index_set_contig_names(ix, nb.data(), no.data());
    if (!rc) rc = bwams_index_set_contig_annos(ix, ab.data(), ao.data());
    return rc;
}

}  // namespace

// bns_dump's .ann and .amb, and the .pac of bns_fasta2bntseq (always l_pac/4 + 2 bytes, the last one l_pac % 4)
int bns_save(bwams_index *ix, const char *prefix) {
    const BnsMeta &m = *ix->bns;
    BWAMS_HIP(hipSetDevice(ix->device));
    std::string path = std::string(prefix) + ".ann";
    FILE *f = fopen(path.c_str(), "w");
    int rc = f ? BWAMS_OK : BWAMS_ERR_IO;
    if (f) {
        if (fprintf(f, "%lld %d %u\n", (long long)m.l_pac, (int)m.names.size(), kSeed) < 0) rc = BWAMS_ERR_IO;
        for (size_t i = 0; i < m.names.size() && !rc; ++i) {
            const char *anno = m.comments[i].empty() ? "(null)" : m.comments[i].c_str();   // add1's anno
            if (fprintf(f, "%d %s", 0, m.names[i].c_str()) < 0 ||
                (anno[0] ? fprintf(f, " %s\n", anno) : fprintf(f, "\n")) < 0 ||
                fprintf(f, "%lld %d %d\n", (long long)m.ctg_off[i], m.ctg_len[i], m.ctg_ambs[i]) < 0)
                rc = BWAMS_ERR_IO;
        }
        if (fclose(f) != 0) rc = BWAMS_ERR_IO;
    }
    if (!rc) {
        path = std::string(prefix) + ".amb";
        f = fopen(path.c_str(), "w");
        rc = f ? BWAMS_OK : BWAMS_ERR_IO;
        if (f) {
            if (fprintf(f, "%lld %d %u\n", (long long)m.l_pac, (int)m.names.size(), (unsigned)m.hole_off.size()) < 0) rc = BWAMS_ERR_IO;
            for (size_t i = 0; i < m.hole_off.size() && !rc; ++i)
                if (fprintf(f, "%lld %d %c\n", (long long)m.hole_off[i], m.hole_len[i], m.hole_amb[i]) < 0) rc = BWAMS_ERR_IO;
            if (fclose(f) != 0) rc = BWAMS_ERR_IO;
        }
    }
    if (!rc) {
        path = std::string(prefix) + ".pac";
        f = fopen(path.c_str(), "wb");
        rc = f ? BWAMS_OK : BWAMS_ERR_IO;
        if (f) {
            const size_t body = (size_t)(m.l_pac >> 2) + ((m.l_pac & 3) ? 1 : 0);
            const size_t kSlab = (size_t)64 << 20;
            std::vector<uint8_t> slab(std::min(kSlab, body) + 2);
            for (size_t o = 0; o < body && !rc; o += kSlab) {
                const size_t k = std::min(kSlab, body - o);
                if (hipMemcpy(slab.data(), m.d_pac.as<const uint8_t>() + o, k, hipMemcpyDeviceToHost) != hipSuccess) rc = BWAMS_ERR_DEVICE;
                else if (fwrite(slab.data(), 1, k, f) != k) rc = BWAMS_ERR_IO;
            }
            uint8_t tail[2] = {0, (uint8_t)(m.l_pac % 4)};
            if (!rc && fwrite(m.l_pac % 4 == 0 ? tail : tail + 1, 1, m.l_pac % 4 == 0 ? 2 : 1, f) != (m.l_pac % 4 == 0 ? 2u : 1u))
                rc = BWAMS_ERR_IO;
            if (fclose(f) != 0 && !rc) rc = BWAMS_ERR_IO;
        }
    }
    if (rc == BWAMS_ERR_IO) set_last_error("write failed: " + path);
    if (rc == BWAMS_ERR_DEVICE) set_last_error("bwams_index_save: reading the .pac back from HBM failed");
    return rc;
}

}  // namespace bwams

using namespace bwams;

static int from_fasta(int device, const char *text, int64_t n_bytes, int text_on_device, int keep_ref, int64_t chunk_rows,
                      float ms_host_read, bwams_fasta_stats_t *stats, bwams_index_t **out) {
    if (!text || !out || n_bytes <= 0) {
        set_last_error("bwams_index_from_fasta: null or empty text");
        return BWAMS_ERR_ARG;
    }
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
        (void)hipGetLastError();
        set_last_error("no usable HIP device");
        return BWAMS_ERR_DEVICE;
    }
    BWAMS_HIP(hipSetDevice(device));
    bwams_fasta_stats_t S;
    memset(&S, 0, sizeof S);
    S.ms_host_read = ms_host_read;
    hipStream_t st = nullptr;
    struct Events {
        hipEvent_t e[4] = {};
        ~Events() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    for (auto &x : ev.e) BWAMS_HIP(hipEventCreate(&x));
    DevBuf<uint8_t> own;
    BWAMS_HIP(hipEventRecord(ev.e[0], st));
    const uint8_t *d_text = reinterpret_cast<const uint8_t *>(text);
    if (!text_on_device) {
        BWAMS_HIP(own.alloc((size_t)n_bytes + 16));
        BWAMS_HIP(hipMemcpy(own.p, text, (size_t)n_bytes, hipMemcpyHostToDevice));
        d_text = own.p;
    }
    BWAMS_HIP(hipEventRecord(ev.e[1], st));
    std::unique_ptr<BnsMeta> m(new BnsMeta());
    DevBuf<uint8_t> fw;
    int64_t n_ambig = 0;
    int rc = fasta_pack(d_text, n_bytes, st, m.get(), &fw, &n_ambig);
    own.release();                                                 // the text goes before suffix sorting starts
    if (rc) return rc;
    BWAMS_HIP(hipEventRecord(ev.e[2], st));
    bwams_index *ix = new bwams_index();
    ix->device = device;
    rc = fmi_build_device(ix, fw.p, m->l_pac, keep_ref, chunk_rows, knobs().verbose != 0, &S.build);
    fw.release();
    if (rc) { bwams_index_close(ix); return rc; }
    BWAMS_HIP(hipEventRecord(ev.e[3], st));
    BWAMS_HIP(hipEventSynchronize(ev.e[3]));
    std::vector<std::string> annos(m->comments.size());
    for (size_t i = 0; i < annos.size(); ++i) annos[i] = m->comments[i] == "(null)" ? std::string() : m->comments[i];
    ix->bns = m.release();
    rc = attach_contigs(ix, ix->bns->ctg_off, ix->bns->ctg_len, {}, ix->bns->names, annos);
    if (rc) { bwams_index_close(ix); return rc; }
    if (stats) {
        S.l_pac = ix->bns->l_pac;
        S.n_seqs = (int32_t)ix->bns->names.size();
        S.n_holes = (int32_t)ix->bns->hole_off.size();
        S.n_ambig_bases = n_ambig;
        BWAMS_HIP(hipEventElapsedTime(&S.ms_upload, ev.e[0], ev.e[1]));
        BWAMS_HIP(hipEventElapsedTime(&S.ms_device_pack, ev.e[1], ev.e[2]));
        BWAMS_HIP(hipEventElapsedTime(&S.ms_fm_build, ev.e[2], ev.e[3]));
        *stats = S;
    }
    *out = ix;
    return BWAMS_OK;
}

extern "C" {

int bwams_index_from_fasta(int device, const char *text, int64_t n_bytes, int text_on_device, int keep_ref, int64_t chunk_rows,
                           bwams_fasta_stats_t *stats, bwams_index_t **out) {
    return from_fasta(device, text, n_bytes, text_on_device, keep_ref, chunk_rows, 0.f, stats, out);
}

int bwams_index_from_fasta_file(const char *path, int device, int keep_ref, int64_t chunk_rows, bwams_fasta_stats_t *stats,
                                bwams_index_t **out) {
    if (!path || !out) return BWAMS_ERR_ARG;
    *out = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    struct stat sb;
    if (stat(path, &sb) != 0) {
        set_last_error(std::string("cannot open ") + path);
        return BWAMS_ERR_IO;
    }
    gzFile fp = gzopen(path, "rb");
    if (!fp) {
        set_last_error(std::string("cannot open ") + path);
        return BWAMS_ERR_IO;
    }
    gzbuffer(fp, 1 << 20);
    // page-locked, grown by doubling (a gzip file's inflated size is not known up front)
    size_t cap = std::max<size_t>((size_t)sb.st_size + 16, (size_t)1 << 20), have = 0;
    HostBuf<char> buf;
    if (buf.alloc(cap) != hipSuccess) {
        gzclose(fp);
        set_last_error("bwams_index_from_fasta_file: page-locked allocation failed");
        return BWAMS_ERR_NOMEM;
    }
    int rc = BWAMS_OK;
    for (;;) {
        if (have == cap) {
            HostBuf<char> nb;
            if (nb.alloc(cap * 2) != hipSuccess) { rc = BWAMS_ERR_NOMEM; break; }
            memcpy(nb.p, buf.p, have);
            buf = std::move(nb);
            cap *= 2;
        }
        const unsigned want = (unsigned)std::min<size_t>(cap - have, (size_t)1 << 30);
        const int got = gzread(fp, buf.p + have, want);
        if (got < 0) {
            int e_ = 0;
            set_last_error(std::string(path) + ": " + gzerror(fp, &e_));
            rc = BWAMS_ERR_IO;
            break;
        }
        if (got == 0) break;
        have += (size_t)got;
    }
    gzclose(fp);
    if (!rc && have == 0) {
        set_last_error(std::string(path) + ": empty");
        rc = BWAMS_ERR_ARG;
    }
    const float ms_read = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (!rc) rc = from_fasta(device, buf.p, (int64_t)have, 0, keep_ref, chunk_rows, ms_read, stats, out);
    return rc;
}

// bns_restore (src/bntseq.cpp:114-246) onto a handle: .ann, the .amb header checked against it, .alt when present
int bwams_index_load_bns(bwams_index_t *ix, const char *prefix) {
    if (!ix || !prefix) return BWAMS_ERR_ARG;
    const int64_t l_pac_ix = (ix->fmi.ref_seq_len - 1) / 2;
    std::string path = std::string(prefix) + ".ann";
    FILE *fp = fopen(path.c_str(), "r");
    if (!fp) {
        set_last_error("cannot open " + path);
        return BWAMS_ERR_IO;
    }
    long long xx = 0;
    int n_seqs = 0;
    unsigned seed = 0;
    auto bad = [&](const std::string &why) {
        if (fp) fclose(fp);
        fp = nullptr;
        set_last_error(path + ": " + why);
        return BWAMS_ERR_IO;
    };
    if (fscanf(fp, "%lld%d%u", &xx, &n_seqs, &seed) != 3 || n_seqs <= 0) return bad("parse error in the header");
    const int64_t l_pac = xx;
    std::vector<int64_t> off((size_t)n_seqs);
    std::vector<int32_t> len((size_t)n_seqs), alt((size_t)n_seqs, 0);
    std::vector<std::string> names((size_t)n_seqs), annos((size_t)n_seqs);
    static thread_local char str[8193];
    for (int i = 0; i < n_seqs; ++i) {
        unsigned gi = 0;
        if (fscanf(fp, "%u%8192s", &gi, str) != 2) return bad("parse error in sequence " + std::to_string(i));
        names[(size_t)i] = str;
        char *q = str;
        int c = 0;
        while (q - str < (long)sizeof(str) - 1 && (c = fgetc(fp)) != '\n' && c != EOF) *q++ = (char)c;
        while (c != '\n' && c != EOF) c = fgetc(fp);
        if (c == EOF) return bad("unexpected end of file");
        *q = 0;
        annos[(size_t)i] = (q - str > 1 && strcmp(str, " (null)") != 0) ? std::string(str + 1) : std::string();
        int n_ambs = 0;
        if (fscanf(fp, "%lld%d%d", &xx, &len[(size_t)i], &n_ambs) != 3) return bad("parse error in sequence " + std::to_string(i));
        off[(size_t)i] = xx;
    }
    fclose(fp);
    fp = nullptr;
    path = std::string(prefix) + ".amb";
    fp = fopen(path.c_str(), "r");
    if (!fp) {
        set_last_error("cannot open " + path);
        return BWAMS_ERR_IO;
    }
    int amb_seqs = 0, n_holes = 0;
    if (fscanf(fp, "%lld%d%d", &xx, &amb_seqs, &n_holes) != 3) return bad("parse error in the header");
    fclose(fp);
    fp = nullptr;
    if (xx != l_pac || amb_seqs != n_seqs) {
        set_last_error(std::string(prefix) + ": inconsistent .ann and .amb files");
        return BWAMS_ERR_IO;
    }
    if (l_pac != l_pac_ix) {
        set_last_error(std::string(prefix) + ".ann: l_pac " + std::to_string(l_pac) + " is not the index's " + std::to_string(l_pac_ix));
        return BWAMS_ERR_ARG;
    }
    int64_t at = 0;
    for (int i = 0; i < n_seqs; ++i) {
        if (off[(size_t)i] != at || len[(size_t)i] < 0) {
            set_last_error(std::string(prefix) + ".ann: sequences do not tile [0, l_pac) in order");
            return BWAMS_ERR_IO;
        }
        at += len[(size_t)i];
    }
    if (at != l_pac) {
        set_last_error(std::string(prefix) + ".ann: sequence lengths do not add up to l_pac");
        return BWAMS_ERR_IO;
    }
    // .alt: the first column of every line not starting with '@' names an ALT contig (src/bntseq.cpp:215-244)
    path = std::string(prefix) + ".alt";
    if ((fp = fopen(path.c_str(), "r")) != nullptr) {
        std::unordered_map<std::string, int> h;
        for (int i = 0; i < n_seqs; ++i) h[names[(size_t)i]] = i;            // kh_put + kh_val: the last of equal names
        std::string s;
        int c;
        while ((c = fgetc(fp)) != EOF) {
            if (c == '\t' || c == '\n' || c == '\r') {
                if (s.empty() || s[0] != '@') {
                    auto k = h.find(s);
                    if (k != h.end()) alt[(size_t)k->second] = 1;
                }
                while (c != '\n' && c != EOF) c = fgetc(fp);
                s.clear();
            } else {
                if (s.size() >= 1022) {
                    fclose(fp);
                    set_last_error(path + ": sequence name longer than 1023 characters");
                    return BWAMS_ERR_IO;
                }
                s.push_back((char)c);
            }
        }
        fclose(fp);
    }
    return attach_contigs(ix, off, len, alt, names, annos);
}

}  // extern "C"
