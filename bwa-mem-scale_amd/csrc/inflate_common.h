// inflate_common.h — what the two DEFLATE decoders share: inflate.hip (BGZF, a wave per member) and gunzip.hip (plain gzip, a wave per
// piece).  The statuses and their texts, RFC 1951's length / distance tables, a canonical Huffman code in LDS (build, decode), and the
// wave-uniform bit reader over an LDS window of the compressed bytes.  The LDS layout is the including file's: a struct L with
//   uint8_t in[kInWin]; uint16_t off[16], next[16];
// and whatever tables its Code objects point into.  The reader's byte positions are int (a BGZF member) or int64_t (a whole stream).
#pragma once

#include <string>

#include "common.h"

namespace {

constexpr int kInWin = 4096;             // LDS window over the compressed bytes
constexpr int kLRoot = 10, kDRoot = 8;   // first-level table bits: literal/length, distance

enum Status : int32_t {
    ST_OK = 0, ST_BTYPE, ST_STORED_LEN, ST_COUNTS, ST_CODE_LENS, ST_REPEAT, ST_NO_EOB, ST_OVERSUB, ST_INCOMPLETE, ST_BAD_LITLEN,
    ST_BAD_DIST, ST_FAR, ST_OVERFLOW, ST_OVERRUN, ST_TRAILING, ST_ISIZE, ST_CRC,
    ST_GZ_METHOD, ST_GZ_FLAGS, ST_END,     // gunzip.hip: a gzip header inside the stream; ST_END: bytes behind a member that are no header
};

inline const char *status_text(int s) {
    switch (s) {
        case ST_BTYPE: return "invalid block type";
        case ST_STORED_LEN: return "stored block LEN is not ~NLEN";
        case ST_COUNTS: return "too many length or distance symbols";
        case ST_CODE_LENS: return "invalid code lengths code";
        case ST_REPEAT: return "invalid bit length repeat";
        case ST_NO_EOB: return "missing end-of-block code";
        case ST_OVERSUB: return "over-subscribed Huffman code";
        case ST_INCOMPLETE: return "incomplete Huffman code";
        case ST_BAD_LITLEN: return "invalid literal/length code";
        case ST_BAD_DIST: return "invalid distance code";
        case ST_FAR: return "distance too far back";
        case ST_OVERFLOW: return "more output than ISIZE";
        case ST_OVERRUN: return "DEFLATE data runs past the member";
        case ST_TRAILING: return "bytes between the end of the DEFLATE data and the trailer";
        case ST_ISIZE: return "ISIZE does not match the inflated size";
        case ST_CRC: return "CRC32 mismatch";
        case ST_GZ_METHOD: return "gzip header: unknown compression method";
        case ST_GZ_FLAGS: return "gzip header: reserved flag bits set";
        case ST_END: return "end of the gzip members";
    }
    return "unknown status";
}

__constant__ uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131,
                                      163, 195, 227, 258};
__constant__ uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537,
                                       2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// A canonical Huffman code in LDS: cnt[len], the symbols sorted by (length, value), the first-level table (entry = symbol | len << 9;
// len 0: the code is longer than the table's bits, or no code has that prefix).
struct Code {
    uint16_t *tab, *cnt, *sym;
    int root;
};

// The bit reader: wave-uniform.  ip: next byte of the data to enter bb; [base, base + kInWin) is in the LDS window.
template <class I> struct BitsT {
    uint64_t bb;
    int bc;
    I ip, base;
};

template <class L, class I>
__device__ __forceinline__ void window_load(L &s, const uint8_t *__restrict__ in, I in_len, I base, int lane) {
    __syncthreads();
    for (int j = lane; j < kInWin; j += 64) s.in[j] = base + j < in_len ? in[base + j] : 0;
    __syncthreads();
}

// at least 57 bits in bb (bytes at and past in_len read as 0)
template <class L, class I>
__device__ __forceinline__ void refill(BitsT<I> &b, L &s, const uint8_t *__restrict__ in, I in_len, int lane) {
    while (b.bc <= 56) {
        if (b.ip - b.base >= kInWin) {
            b.base = b.ip;
            window_load(s, in, in_len, b.base, lane);
        }
        b.bb |= (uint64_t)s.in[b.ip - b.base] << b.bc;
        b.bc += 8;
        ++b.ip;
    }
}

template <class I> __device__ __forceinline__ uint32_t take(BitsT<I> &b, int n) {
    const uint32_t v = (uint32_t)(b.bb & ((1ull << n) - 1));
    b.bb >>= n;
    b.bc -= n;
    return v;
}

// one symbol (needs 15 bits in bb); -1: no code of this code has that bit string
template <class I> __device__ __forceinline__ int decode(BitsT<I> &b, const Code &c) {
    const uint32_t e = c.tab[b.bb & ((1u << c.root) - 1)];
    if (e >> 9) {
        take(b, (int)(e >> 9));
        return (int)(e & 511);
    }
    uint64_t bits = b.bb;                             // canonical walk, one bit at a time (codes longer than the table's bits)
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {
        code |= (int)(bits & 1);
        bits >>= 1;
        const int count = c.cnt[len];
        if (code - count < first) {
            take(b, len);
            return c.sym[index + (code - first)];
        }
        index += count;
        first = (first + count) << 1;
        code <<= 1;
    }
    return -1;
}

// the code of lens[0, n) into c; `cl`: the code lengths code (an incomplete code is refused even with one code of length 1)
template <class L> __device__ int build(L &s, const uint8_t *lens, int n, const Code &c, bool cl, int lane) {
    __syncthreads();
    for (int i = lane; i < (1 << c.root); i += 64) c.tab[i] = 0;
    int k = 0;
    if (lane < 16)
        for (int i = 0; i < n; ++i) k += lens[i] == lane;
    if (lane < 16) c.cnt[lane] = (uint16_t)(lane ? k : 0);
    __syncthreads();
    int left = 1, max = 0, code = 0, off = 0;
    for (int len = 1; len <= 15; ++len) {
        const int m = c.cnt[len];
        left = (left << 1) - m;
        if (left < 0) return ST_OVERSUB;
        if (m) max = len;
        code = (code + (len > 1 ? c.cnt[len - 1] : 0)) << 1;
        if (lane == len) { s.off[len] = (uint16_t)off; s.next[len] = (uint16_t)code; }
        off += m;
    }
    if (max == 0) return ST_OK;                       // no symbols at all (zlib accepts it; any decode then fails)
    if (left > 0 && (cl || max != 1)) return ST_INCOMPLETE;
    __syncthreads();
    if (lane >= 1 && lane < 16) {                     // lane = length: its symbols in value order
        int at = s.off[lane];
        for (int i = 0; i < n; ++i)
            if (lens[i] == lane) c.sym[at++] = (uint16_t)i;
    }
    __syncthreads();
    for (int i = lane; i < off; i += 64) {            // every code that fits the table: all its entries
        int len = 1;
        while (len < 15 && i >= s.off[len] + c.cnt[len]) ++len;
        if (len > c.root) continue;
        const uint32_t cd = s.next[len] + (uint32_t)(i - s.off[len]);
        const uint32_t rev = __builtin_bitreverse32(cd) >> (32 - len);
        const uint16_t e = (uint16_t)(c.sym[i] | len << 9);
        for (uint32_t j = rev; j < (1u << c.root); j += 1u << len) c.tab[j] = e;
    }
    __syncthreads();
    return ST_OK;
}

inline int device_ok(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) {
        (void)hipGetLastError();
        bwams::set_last_error("no usable HIP device");
        return BWAMS_ERR_DEVICE;
    }
    hipDeviceProp_t p;
    BWAMS_HIP(hipGetDeviceProperties(&p, device));
    if (std::string(p.gcnArchName).rfind("gfx950", 0) != 0) {
        bwams::set_last_error(std::string("device is ") + p.gcnArchName + ", this library is built for gfx950 only");
        return BWAMS_ERR_DEVICE;
    }
    return BWAMS_OK;
}

}  // namespace
