// bam_discover.h — record discovery in a buffer of BAM alignment records, shared by bam_reads.hip (a whole buffer, from byte 0 to its
// end) and bam_query.hip (a piece of a file: from an offset, up to an offset, and the last record possibly cut off by the end of the
// buffer).  Where record k + 1 starts follows from record k's block_size, so the records are a linked list through the bytes.  Every
// position is parsed as if a record began there and the real records are the chain of successors from the start, found by binary
// lifting over the few positions that can be a record at all:
//   (1) br_filter_kernel: a lane per byte offset, the bytes staged through LDS in 16-byte loads, tests that a well-formed record
//       starts there (sizes consistent, the name's NUL in place, the end inside the buffer).  The wave's ballot is one word of a
//       bitmap; its population count goes into a second array whose exclusive scan gives, for any offset q, "index of the candidate
//       at q" in O(1).
//   (2) br_succ_kernel: a lane per bitmap word lists its candidates' offsets and their successors — the candidate index at
//       q + 4 + block_size, END when that is n_bytes, BAD when nothing well formed starts there.
//   (3) br_double_kernel, ceil(log2(candidates)) + 1 levels; br_count_kernel (one lane) descends them from the candidate at `start`
//       while the next record begins below `stop`: the number of records, where the chain ended and how (BrEnd).
// Quality and aux bytes do give false candidates (a Z value may hold a whole record); the chain never visits them.
// Scratch: 1/8 byte (bitmap) + 1/16 byte (ranks) per input byte, 8 + 4 * levels bytes per candidate.
// Every read of the buffer is bounded by n: the bytes are a file's, or a caller's.
#pragma once
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "bam_rec.h"
#include "common.h"

namespace bwams {
namespace {

constexpr int kTile = 4096;                   // bytes per block of br_filter_kernel: 64 bitmap words
constexpr int kHalo = 48;                     // a record's fixed part (36 bytes) behind the tile's last offset, in 16-byte pieces

// the aligned word w of the buffer (d is 16-byte aligned): one load when it lies inside [0, n), its bytes inside otherwise
__device__ __forceinline__ uint32_t ld_word(const uint8_t *__restrict__ d, int64_t w, int64_t n) {
    const int64_t p = w * 4;
    if (p + 4 <= n) return *reinterpret_cast<const uint32_t *>(d + p);
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k)
        if (p + k < n) v |= (uint32_t)d[p + k] << (8 * k);
    return v;
}
// the four bytes at p (any alignment), bytes outside [0, n) as zeros
__device__ __forceinline__ uint32_t ld_wide(const uint8_t *__restrict__ d, int64_t p, int64_t n) {
    const int64_t w = p >> 2;
    const int sh = (int)(p & 3) * 8;
    const uint32_t lo = ld_word(d, w, n);
    if (!sh) return lo;
    return lo >> sh | ld_word(d, w + 1, n) << (32 - sh);
}

// a record's fields at offset q, everything but where it ends and the name's NUL
__device__ __forceinline__ bool fields_ok(uint32_t block_size, uint32_t l_name, uint32_t n_cig, int32_t l_seq) {
    if (block_size < 32 || l_name < 1 || l_seq < 0) return false;
    const int64_t need = bam_aux_at(l_name, n_cig, l_seq) - 4;
    return need <= (int64_t)block_size;
}
// the same with the end inside the buffer
__device__ __forceinline__ bool fixed_ok(int64_t q, int64_t n, uint32_t block_size, uint32_t l_name, uint32_t n_cig, int32_t l_seq) {
    return fields_ok(block_size, l_name, n_cig, l_seq) && q + 4 + (int64_t)block_size <= n;
}

// (1) a lane per offset.  Block b takes offsets [b * kTile, (b + 1) * kTile); bm: one bit per offset, cnt[w] = popcount(bm[w]).
__global__ __launch_bounds__(256) void br_filter_kernel(const uint8_t *__restrict__ d, int64_t n, unsigned long long *__restrict__ bm,
                                                        uint32_t *__restrict__ cnt) {
    __shared__ uint32_t lds[(kTile + kHalo) / 4 + 1];
    const int64_t t0 = (int64_t)blockIdx.x * kTile;
    for (int piece = threadIdx.x; piece < (kTile + kHalo) / 16; piece += 256) {
        const int64_t p = t0 + (int64_t)piece * 16;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (p + 16 <= n) v = *reinterpret_cast<const uint4 *>(d + p);
        else if (p < n) { v.x = ld_word(d, p >> 2, n); v.y = ld_word(d, (p >> 2) + 1, n); v.z = ld_word(d, (p >> 2) + 2, n); v.w = ld_word(d, (p >> 2) + 3, n); }
        lds[piece * 4] = v.x; lds[piece * 4 + 1] = v.y; lds[piece * 4 + 2] = v.z; lds[piece * 4 + 3] = v.w;
    }
    if (threadIdx.x == 0) lds[(kTile + kHalo) / 4] = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = 0; k < kTile / 256; ++k) {
        const int t = k * 256 + threadIdx.x;                     // consecutive lanes, consecutive offsets: four lanes share a word
        const int64_t q = t0 + t;
        const int sh = (t & 3) * 8, w = t >> 2;
        auto u32_at = [&](int word) -> uint32_t {
            const uint32_t lo = lds[word], hi = lds[word + 1];
            return sh ? (lo >> sh | hi << (32 - sh)) : lo;
        };
        bool ok = false;
        if (q + kBamName <= n) {
            const uint32_t block_size = u32_at(w);
            if (block_size >= 32 && q + 4 + (int64_t)block_size <= n) {
                const uint32_t l_name = u32_at(w + 3) & 0xFF, n_cig = u32_at(w + 4) & 0xFFFF;
                const int32_t l_seq = (int32_t)u32_at(w + 5);
                ok = fixed_ok(q, n, block_size, l_name, n_cig, l_seq) && d[q + kBamName - 1 + l_name] == 0;     // the name's last byte: inside the record
            }
        }
        const unsigned long long m = __ballot(ok);
        if (lane == 0) {
            const int64_t word = (t0 >> 6) + k * 4 + wave;
            bm[word] = m;
            cnt[word] = (uint32_t)__popcll(m);
        }
    }
}

// (2) a lane per bitmap word: offsets and successors of its candidates.  END = n_cand, BAD = n_cand + 1 (both map to themselves).
__global__ __launch_bounds__(256) void br_succ_kernel(const uint8_t *__restrict__ d, int64_t n, const unsigned long long *__restrict__ bm,
                                                      const uint32_t *__restrict__ rank, int64_t n_words, uint32_t n_cand,
                                                      int64_t *__restrict__ cand_off, uint32_t *__restrict__ up0) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w == 0) { up0[n_cand] = n_cand; up0[n_cand + 1] = n_cand + 1; }
    if (w >= n_words) return;
    unsigned long long bits = bm[w];
    uint32_t idx = rank[w];
    while (bits) {
        const int b = __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        const int64_t q = w * 64 + b;
        const int64_t q2 = q + 4 + (int64_t)bam_block_size(d + q);           // <= n: the filter saw to it
        uint32_t nx = n_cand + 1;
        if (q2 == n) nx = n_cand;
        else {
            const unsigned long long m = bm[q2 >> 6];
            const int s = (int)(q2 & 63);
            if ((m >> s) & 1) nx = rank[q2 >> 6] + (uint32_t)__popcll(m & ((1ull << s) - 1));
        }
        cand_off[idx] = q;
        up0[idx] = nx;
        ++idx;
    }
}

// (3) up[k + 1] = up[k] o up[k]
__global__ __launch_bounds__(256) void br_double_kernel(const uint32_t *__restrict__ a, uint32_t *__restrict__ b, int64_t n) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) b[j] = a[a[j]];
}

// How a chain ended, and what br_count_kernel reports of it.
enum : int64_t {
    kBrStopped = 0,                           // the next record would begin at `stop` or behind it, or the last one ends the buffer
    kBrCut = 1,                               // the bytes at `at` may begin a record that the end of the buffer cuts off
    kBrBad = 2                                // no well-formed record starts at `at`
};
struct BrEnd {
    int64_t n_rec, how, at;                   // at: behind the chain's last record (the start when there is none)
    int64_t cut_size;                         // kBrCut: block_size + 4 of the cut-off record when its first four bytes are there, else 0
    int64_t first;                            // the candidate index of the chain's first record
};

// what is at q < n when no candidate is: a record the buffer's end cuts off, or nothing well formed
__device__ __forceinline__ int64_t br_probe(const uint8_t *__restrict__ d, int64_t q, int64_t n, int64_t *cut_size) {
    *cut_size = 0;
    if (q + 4 > n) return kBrCut;
    const uint32_t block_size = ld_wide(d, q, n);
    *cut_size = 4 + (int64_t)block_size;
    if (block_size < 32) return kBrBad;
    if (q + kBamName > n) return kBrCut;
    const uint32_t l_name = d[q + 12], n_cig = ld_u16(d + q + 16);
    const int32_t l_seq = (int32_t)ld_u32(d + q + 20);
    if (!fields_ok(block_size, l_name, n_cig, l_seq)) return kBrBad;
    const int64_t nul = q + kBamName - 1 + l_name;
    if (nul < n && d[nul] != 0) return kBrBad;
    return q + 4 + (int64_t)block_size > n ? kBrCut : kBrBad;
}

// one lane: the chain from the record at `start` (0 <= start <= stop <= n) over the records that begin below `stop`
__global__ void br_count_kernel(const uint8_t *__restrict__ d, int64_t n, const unsigned long long *__restrict__ bm,
                                const uint32_t *__restrict__ rank, const uint32_t *__restrict__ up, int levels, uint32_t n_cand,
                                const int64_t *__restrict__ cand_off, int64_t start, int64_t stop, BrEnd *__restrict__ out) {
    BrEnd e{0, kBrStopped, start, 0, 0};
    if (start < stop) {
        const unsigned long long m = bm[start >> 6];
        const int s = (int)(start & 63);
        if (!((m >> s) & 1)) e.how = br_probe(d, start, n, &e.cut_size);
        else {
            const int64_t stride = (int64_t)n_cand + 2;
            uint32_t cur = rank[start >> 6] + (uint32_t)__popcll(m & ((1ull << s) - 1));
            e.first = cur;
            int64_t cnt = 0;
            for (int k = levels - 1; k >= 0; --k) {
                const uint32_t nx = up[(int64_t)k * stride + cur];
                if (nx < n_cand && cand_off[nx] < stop) { cur = nx; cnt += (int64_t)1 << k; }
            }
            e.n_rec = cnt + 1;
            e.at = cand_off[cur] + 4 + (int64_t)bam_block_size(d + cand_off[cur]);
            if (e.at < stop && up[cur] == n_cand + 1) e.how = br_probe(d, e.at, n, &e.cut_size);
        }
    }
    *out = e;
}

// The scratch of a discovery and its run: filter, ranks, successors, lifting and count over d[0, n) (16-byte aligned, device), all on
// st, which is drained twice (the candidates' number sizes the lifting; the count comes back in *end).  ms: a device event pair
// around it all, or null.
struct BrDiscover {
    DevBuf<unsigned long long> bm;
    DevBuf<uint32_t> rank, up;
    DevBuf<int64_t> cand_off;
    DevBuf<BrEnd> res;
    DevBuf<> scan_tmp;
    uint32_t n_cand = 0;
    int levels = 1;
    int run(const uint8_t *d, int64_t n, int64_t start, int64_t stop, hipStream_t st, BrEnd *end) {
        const int64_t n_tiles = (n + kTile - 1) / kTile, n_words = n_tiles * (kTile / 64);
        BWAMS_HIP(bm.ensure_n((size_t)n_words));
        BWAMS_HIP(rank.ensure_n((size_t)n_words + 1));
        BWAMS_HIP(res.ensure_n(1));
        br_filter_kernel<<<(unsigned)n_tiles, 256, 0, st>>>(d, n, bm.p, rank.p);
        BWAMS_HIP(hipMemsetAsync(rank.p + n_words, 0, 4, st));
        if (int rc = with_tmp(scan_tmp, st, "record discovery: exclusive_scan", [&](void *tmp, size_t &tb) {
                return rocprim::exclusive_scan(tmp, tb, rank.p, rank.p, 0u, (size_t)(n_words + 1), rocprim::plus<uint32_t>(), st);
            })) return rc;
        BWAMS_HIP(hipMemcpyAsync(&n_cand, rank.p + n_words, 4, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipStreamSynchronize(st));
        levels = 1;
        while (((int64_t)1 << (levels - 1)) < (int64_t)n_cand) ++levels;
        const int64_t stride = (int64_t)n_cand + 2;
        BWAMS_HIP(cand_off.ensure_n((size_t)n_cand + 1));
        BWAMS_HIP(up.ensure_n((size_t)levels * (size_t)stride));
        br_succ_kernel<<<(unsigned)((n_words + 255) / 256), 256, 0, st>>>(d, n, bm.p, rank.p, n_words, n_cand, cand_off.p, up.p);
        for (int k = 1; k < levels; ++k)
            br_double_kernel<<<(unsigned)((stride + 255) / 256), 256, 0, st>>>(up.p + (int64_t)(k - 1) * stride, up.p + (int64_t)k * stride, stride);
        br_count_kernel<<<1, 1, 0, st>>>(d, n, bm.p, rank.p, up.p, levels, n_cand, cand_off.p, start, stop, res.p);
        BWAMS_HIP(hipMemcpyAsync(end, res.p, sizeof(BrEnd), hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipStreamSynchronize(st));
        BWAMS_HIP(hipGetLastError());
        return BWAMS_OK;
    }
};

// the candidate index of record r of a chain that starts at candidate `first`
__device__ __forceinline__ uint32_t br_lift(const uint32_t *__restrict__ up, int levels, uint32_t n_cand, uint32_t first, int64_t r) {
    const int64_t stride = (int64_t)n_cand + 2;
    uint32_t cur = first;
    for (int k = 0; k < levels; ++k)
        if ((r >> k) & 1) cur = up[(int64_t)k * stride + cur];
    return cur;
}

}  // namespace
}  // namespace bwams
