// deflate.hip — text in HBM compressed into BGZF members on the device: RFC 1951 DEFLATE, one 256-lane workgroup per member.
//
// The output side's counterpart of inflate.hip.  The text is cut every 65280 bytes from its byte 0 (bgzip's and htslib's cut); each
// piece becomes one standalone gzip member with bgzip's header (the 'BC' subfield carries BSIZE), one DEFLATE block and the CRC32 /
// ISIZE trailer.  Members depend on their own bytes only, so the output does not depend on how the text is split into launches.
//
// deflate_kernel, one workgroup per member (a grid-stride loop over the launch's members; the workspace is per workgroup):
//   * the member's bytes are loaded into LDS (as words, 8 zero bytes behind them) and its CRC32 is taken (crc32.h);
//   * match candidates: prev[i] = the last position before i whose 3 bytes hash alike (12-bit hash).  Positions go 256 at a time;
//     a lane finds its predecessor inside the group by scanning the group's hashes back, otherwise in a head table in LDS that the last
//     position of each hash in the group then updates (no atomics: which lane is last follows from the predecessors);
//   * match[i]: the longest match among up to kChain links of that chain inside the 32 KiB window, lengths 3-258 (the nearest wins a
//     tie), compared 4 bytes at a time in LDS;
//   * the greedy parse (a match of length >= 3 is taken, else a literal) in 256 segments of 255 bytes: each lane walks its segment from
//     where the previous lane's walk left it, and the walks repeat until no start moves (usually 2-3 rounds: walks resynchronise);
//   * symbol histograms (LDS atomics: counts, their order is immaterial), then codes built by one lane: a two-queue Huffman tree over
//     the symbols sorted by (count, value), its depths limited to 15 (7 for the code lengths code) by JPEG's Annex K.3 rebalancing,
//     lengths given in that order.  A code with fewer than two symbols gets symbols 0 and 1, as zlib does;
//   * the block type is the one with the fewest exact bits (stored, then fixed, then dynamic on a tie).  Each lane sums its segment's
//     bits, a scan gives it its bit offset, and its symbols are ORed into the member's 64 KiB staging slot (zeroed first).  ORs
//     commute, so the bytes do not depend on the order of the atomics;
// deflate_scan then gives each member its output offset (an exclusive scan of the sizes), and deflate_copy moves the members from
// their slots to the contiguous output.  LDS 79 088 B: two members per CU.
#include <algorithm>
#include <cstring>
#include <string>

#include "common.h"
#include "crc32.h"

using namespace bwams;

namespace {

constexpr int kBlock = 65280;            // input bytes per member: bgzip's cut
constexpr int kSlot = 65536;             // a member's staging slot: BSIZE + 1 <= 65536
constexpr int kNT = 256;                 // lanes per member
constexpr int kSeg = (kBlock + kNT - 1) / kNT;   // parse segment of a lane: 255 bytes
constexpr int kHashBits = 12;
constexpr int kChain = 12;               // chain links tried per position
constexpr int kWindow = 32768, kMaxMatch = 258;
constexpr uint16_t kNone = 0xFFFF;
constexpr int kHdr = 18, kTrl = 8;       // bgzip's header, CRC32 + ISIZE
constexpr int kEofLen = 28;
const uint8_t kEofMember[kEofLen] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0,
                                     0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

__constant__ uint8_t kLenExtraD[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint8_t kDistExtraD[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t kClOrderD[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct Huff {                            // scratch of a code build (aliases the hash head table)
    uint32_t sw[288];                    // symbol weights
    uint32_t wt[2 * 288];                // tree node weights (leaves first, sorted), then depths
    uint16_t parent[2 * 288];
    uint16_t order[288];                 // used symbols by (count, value)
    uint16_t bl[32];                     // codes per length
    uint32_t next[16];                   // next canonical code per length
};

struct Lds {
    uint32_t in[kBlock / 4 + 2];         // the member's bytes, zero behind them
    union {
        uint32_t crc_tab[256];
        uint16_t head[1 << kHashBits];
        Huff h;
    } u;
    uint32_t part[kNT];                  // CRC slices / the group's hashes / per-lane bit counts
    uint32_t lfreq[288], dfreq[32], cfreq[20];
    uint16_t lcode[288], dcode[32], ccode[20];   // codes, bit-reversed (sent LSB first)
    uint8_t llen[288], dlen[32], clen[20];
    uint8_t rle_sym[320], rle_ext[320];  // the code lengths, run-length coded (16/17/18 carry their extra bits)
    uint8_t notlast[kNT];
    int32_t seg[kNT];                    // where each lane's parse starts
    int32_t n_rle, hlit, hdist, hclen, btype, hdr_bits, body_bytes;
};

__device__ __forceinline__ uint32_t byte_at(const Lds &s, int p) { return (s.in[p >> 2] >> ((p & 3) * 8)) & 255u; }

__device__ __forceinline__ uint32_t load4(const Lds &s, int p) {
    const uint64_t w = (uint64_t)s.in[(p >> 2) + 1] << 32 | s.in[p >> 2];
    return (uint32_t)(w >> ((p & 3) * 8));
}

__device__ __forceinline__ uint32_t hash3(const Lds &s, int p) {
    return ((load4(s, p) & 0xFFFFFFu) * 2654435761u) >> (32 - kHashBits);
}

// common prefix of the bytes at a < b, at most `max`
__device__ __forceinline__ int match_len(const Lds &s, int a, int b, int max) {
    int l = 0;
    while (l < max) {
        const uint32_t x = load4(s, a + l) ^ load4(s, b + l);
        if (x) return min(l + (__builtin_ctz(x) >> 3), max);
        l += 4;
    }
    return max;
}

// length 3..258 -> symbol - 257, extra bits, their value
__device__ __forceinline__ void len_code(int len, int &code, int &nx, int &x) {
    if (len == 258) { code = 28; nx = 0; x = 0; return; }
    const int l = len - 3;
    if (l < 8) { code = l; nx = 0; x = 0; return; }
    nx = 29 - __clz(l);                          // floor(log2 l) - 2
    code = 4 * (nx + 1) + ((l >> nx) & 3);
    x = l & ((1 << nx) - 1);
}

// distance 1..32768 -> symbol, extra bits, their value
__device__ __forceinline__ void dist_code(int dist, int &code, int &nx, int &x) {
    const int d = dist - 1;
    if (d < 4) { code = d; nx = 0; x = 0; return; }
    nx = 30 - __clz(d);                          // floor(log2 d) - 1
    code = 2 * (nx + 1) + ((d >> nx) & 1);
    x = d & ((1 << nx) - 1);
}

__device__ __forceinline__ int step_at(const uint32_t *match, int p) {
    const int l = (int)(match[p] >> 16);
    return l ? l : 1;
}

// v (n <= 48 bits) ORed into the slot at bit `pos`
__device__ __forceinline__ void put_bits(uint32_t *o, uint32_t pos, uint64_t v, int n) {
    if (n == 0) return;
    const uint32_t w = pos >> 5, sh = pos & 31;
    v &= (n == 64 ? ~0ull : (1ull << n) - 1);
    const uint64_t lo = v << sh;
    const uint32_t hi = sh ? (uint32_t)(v >> (64 - sh)) : 0u;
    if ((uint32_t)lo && w < kSlot / 4) atomicOr(o + w, (uint32_t)lo);
    if ((uint32_t)(lo >> 32) && w + 1 < kSlot / 4) atomicOr(o + w + 1, (uint32_t)(lo >> 32));
    if (hi && w + 2 < kSlot / 4) atomicOr(o + w + 2, hi);
}

__device__ __forceinline__ uint32_t bitrev(uint32_t c, int len) { return __builtin_bitreverse32(c) >> (32 - len); }

// Code lengths (<= limit) of freq[0, nsym) into len[], canonical bit-reversed codes into code[].  Every lane calls it.
__device__ void build_code(Lds &s, const uint32_t *freq, int nsym, int limit, uint8_t *len, uint16_t *code, int lane) {
    Huff &h = s.u.h;
    __syncthreads();
    for (int i = lane; i < nsym; i += kNT) {        // rank of each used symbol by (count, value); at least two symbols
        const uint32_t f = freq[i];
        len[i] = 0;
        h.sw[i] = f;
    }
    __syncthreads();
    if (lane == 0) {
        int used = 0;
        for (int i = 0; i < nsym; ++i) used += h.sw[i] != 0;
        for (int i = 0; i < 2 && used < 2; ++i)
            if (!h.sw[i]) { h.sw[i] = 1; ++used; }
    }
    __syncthreads();
    for (int i = lane; i < nsym; i += kNT) {
        const uint32_t f = h.sw[i];
        if (!f) continue;
        int r = 0;
        for (int j = 0; j < nsym; ++j) {
            const uint32_t g = h.sw[j];
            r += g && (g < f || (g == f && j < i));
        }
        h.order[r] = (uint16_t)i;
    }
    __syncthreads();
    if (lane == 0) {
        int m = 0;
        for (int i = 0; i < nsym; ++i) m += h.sw[i] != 0;
        // the tree's nodes: leaves 0..m-1 (sorted), internal nodes m..2m-2 in the order they are made (two queues; a leaf wins a tie)
        for (int x = 0; x < m; ++x) h.wt[x] = h.sw[h.order[x]];
        int i = 0, j = m;
        for (int k = m; k < 2 * m - 1; ++k) {
            const int a = (i < m && (j >= k || h.wt[i] <= h.wt[j])) ? i++ : j++;
            const int b = (i < m && (j >= k || h.wt[i] <= h.wt[j])) ? i++ : j++;
            h.wt[k] = h.wt[a] + h.wt[b];
            h.parent[a] = h.parent[b] = (uint16_t)k;
        }
        h.wt[2 * m - 2] = 0;                          // depths, from the root down
        for (int k = 2 * m - 3; k >= 0; --k) h.wt[k] = h.wt[h.parent[k]] + 1;
        for (int l = 0; l < 32; ++l) h.bl[l] = 0;
        int maxd = 0;
        for (int x = 0; x < m; ++x) {
            const int d = min((int)h.wt[x], 31);
            ++h.bl[d];
            maxd = max(maxd, d);
        }
        for (int l = maxd; l > limit; --l)            // JPEG Annex K.3: lift pairs of the deepest leaves
            while (h.bl[l] > 0) {
                int q = l - 2;
                while (q > 1 && h.bl[q] == 0) --q;
                h.bl[l] -= 2;
                h.bl[l - 1] += 1;
                h.bl[q + 1] += 2;
                h.bl[q] -= 1;
            }
        int x = 0;                                    // the rarest symbols get the longest codes
        for (int l = min(maxd, limit); l >= 1; --l)
            for (int c = 0; c < h.bl[l]; ++c) len[h.order[x++]] = (uint8_t)l;
        uint32_t c = 0;                               // canonical codes in symbol order
        for (int l = 1; l <= 15; ++l) {
            c = (c + (l > 1 ? h.bl[l - 1] : 0)) << 1;
            h.next[l] = c;
        }
        for (int k = 0; k < nsym; ++k)
            if (len[k]) code[k] = (uint16_t)bitrev(h.next[len[k]]++, len[k]);
            else code[k] = 0;
    }
    __syncthreads();
}

__device__ void deflate_member(Lds &s, const uint8_t *__restrict__ src, int n, uint16_t *__restrict__ prev, uint32_t *__restrict__ match,
                               uint32_t *__restrict__ o, int32_t *__restrict__ size_out, int lane) {
    // the bytes into LDS, zero behind them
    const int nw = (n + 3) >> 2;
    __syncthreads();
    if (((uintptr_t)src & 3) == 0) {
        const uint32_t *s32 = reinterpret_cast<const uint32_t *>(src);
        for (int w = lane; w < kBlock / 4 + 2; w += kNT) {
            uint32_t v = 0;
            if (4 * w + 4 <= n) v = s32[w];
            else for (int b = 0; b < 4 && 4 * w + b < n; ++b) v |= (uint32_t)src[4 * w + b] << (8 * b);
            s.in[w] = v;
        }
    } else {
        for (int w = lane; w < kBlock / 4 + 2; w += kNT) {
            uint32_t v = 0;
            for (int b = 0; b < 4 && 4 * w + b < n; ++b) v |= (uint32_t)src[4 * w + b] << (8 * b);
            s.in[w] = v;
        }
    }
    crc32_table<kNT>(s.u.crc_tab, lane);
    for (int i = lane; i < 288; i += kNT) s.lfreq[i] = 0;
    if (lane < 32) s.dfreq[lane] = 0;
    __syncthreads();
    const uint32_t crc = crc32_lds<kNT>(reinterpret_cast<const uint8_t *>(s.in), n, s.u.crc_tab, s.part, lane);
    __syncthreads();

    // hash chains
    const int npos = n - 2;                             // positions with 3 bytes
    for (int i = lane; i < (1 << kHashBits); i += kNT) s.u.head[i] = kNone;
    for (int base = 0; base < npos; base += kNT) {
        const int i = base + lane;
        const bool valid = i < npos;
        const uint32_t hv = valid ? hash3(s, i) : 0x10000u + (uint32_t)lane;
        s.part[lane] = hv;
        s.notlast[lane] = 0;
        __syncthreads();
        int jin = -1;
        if (valid) {
            for (int j = lane - 1; j >= 0; --j)
                if (s.part[j] == hv) { jin = j; break; }
            prev[i] = jin >= 0 ? (uint16_t)(base + jin) : s.u.head[hv];
            if (jin >= 0) s.notlast[jin] = 1;
        }
        __syncthreads();
        if (valid && !s.notlast[lane]) s.u.head[hv] = (uint16_t)i;
    }
    __syncthreads();

    // the longest match at every position
    for (int i = lane; i < n; i += kNT) {
        int best = 0, bd = 0;
        if (i < npos) {
            const int maxl = min(kMaxMatch, n - i);
            int p = prev[i];
            for (int k = 0; k < kChain && p != kNone && i - p <= kWindow; ++k) {
                const int l = match_len(s, p, i, maxl);
                if (l > best) { best = l; bd = i - p; if (l == maxl) break; }
                p = prev[p];
            }
        }
        match[i] = best >= 3 ? (uint32_t)best << 16 | (uint32_t)(bd - 1) : 0u;
    }

    // the greedy parse: segment walks until every start is where the walk in front of it ends
    const int seg_end = min((lane + 1) * kSeg, n);
    s.seg[lane] = min(lane * kSeg, n);
    for (;;) {
        __syncthreads();
        int p = s.seg[lane];
        while (p < seg_end) p += step_at(match, p);
        __syncthreads();
        bool moved = false;                            // p >= seg_end: where the next lane's walk starts
        if (lane + 1 < kNT && s.seg[lane + 1] != p) {
            s.seg[lane + 1] = p;
            moved = true;
        }
        if (!__syncthreads_or(moved)) break;
    }
    const int start = s.seg[lane];

    // histograms
    for (int p = start; p < seg_end;) {
        const uint32_t mv = match[p];
        if (mv >> 16) {
            int c, nx, x;
            len_code((int)(mv >> 16), c, nx, x);
            atomicAdd(&s.lfreq[257 + c], 1u);
            dist_code((int)(mv & 0xFFFF) + 1, c, nx, x);
            atomicAdd(&s.dfreq[c], 1u);
            p += (int)(mv >> 16);
        } else {
            atomicAdd(&s.lfreq[byte_at(s, p)], 1u);
            ++p;
        }
    }
    if (lane == 0) s.lfreq[256] = 1;                   // end of block

    // codes: literal/length, distance, then the code lengths code over their run-length coding
    build_code(s, s.lfreq, 286, 15, s.llen, s.lcode, lane);
    build_code(s, s.dfreq, 30, 15, s.dlen, s.dcode, lane);
    if (lane == 0) {
        int hlit = 286, hdist = 30;
        while (hlit > 257 && !s.llen[hlit - 1]) --hlit;
        while (hdist > 1 && !s.dlen[hdist - 1]) --hdist;
        for (int k = 0; k < 20; ++k) s.cfreq[k] = 0;
        // zlib's scan_tree over the lengths of both codes as one sequence (runs may cross from one code into the other)
        const int total = hlit + hdist;
        auto lens = [&](int k) { return k < hlit ? (int)s.llen[k] : (int)s.dlen[k - hlit]; };
        int nr = 0, prevlen = -1, count = 0, nextlen = lens(0);
        int max_count = nextlen ? 7 : 138, min_count = nextlen ? 4 : 3;
        auto emit = [&](int sym, int ext) { s.rle_sym[nr] = (uint8_t)sym; s.rle_ext[nr] = (uint8_t)ext; ++nr; ++s.cfreq[sym]; };
        for (int k = 0; k < total; ++k) {
            const int cur = nextlen;
            nextlen = k + 1 < total ? lens(k + 1) : -1;
            if (++count < max_count && cur == nextlen) continue;
            if (count < min_count) {
                for (int r = 0; r < count; ++r) emit(cur, 0);
            } else if (cur != 0) {
                if (cur != prevlen) { emit(cur, 0); --count; }
                if (count >= 3) emit(16, count - 3);
                else for (int r = 0; r < count; ++r) emit(cur, 0);
            } else if (count <= 10) {
                emit(17, count - 3);
            } else {
                emit(18, count - 11);
            }
            count = 0;
            prevlen = cur;
            if (nextlen == 0) { max_count = 138; min_count = 3; }
            else if (cur == nextlen) { max_count = 6; min_count = 3; }
            else { max_count = 7; min_count = 4; }
        }
        s.n_rle = nr;
        s.hlit = hlit;
        s.hdist = hdist;
    }
    build_code(s, s.cfreq, 19, 7, s.clen, s.ccode, lane);
    if (lane == 0) {
        int hclen = 19;
        while (hclen > 4 && !s.clen[kClOrderD[hclen - 1]]) --hclen;
        s.hclen = hclen;
        uint64_t dyn = 3 + 14 + 3 * (uint64_t)hclen, fix = 3;
        for (int k = 0; k < s.n_rle; ++k) {
            const int sym = s.rle_sym[k];
            dyn += s.clen[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
        }
        const uint64_t dyn_hdr = dyn;
        for (int k = 0; k < 286; ++k) {
            const uint64_t f = s.lfreq[k];
            if (!f) continue;
            const int ex = k > 256 ? kLenExtraD[k - 257] : 0;
            dyn += f * (s.llen[k] + ex);
            fix += f * ((k < 144 ? 8 : k < 256 ? 9 : k < 280 ? 7 : 8) + ex);
        }
        for (int k = 0; k < 30; ++k) {
            const uint64_t f = s.dfreq[k];
            dyn += f * (s.dlen[k] + kDistExtraD[k]);
            fix += f * (5 + kDistExtraD[k]);
        }
        const int64_t stored_b = (int64_t)n + 5, fix_b = (int64_t)((fix + 7) / 8), dyn_b = (int64_t)((dyn + 7) / 8);
        int bt = 0;
        int64_t best = stored_b;
        if (fix_b < best) { bt = 1; best = fix_b; }
        if (dyn_b < best) { bt = 2; best = dyn_b; }
        s.btype = bt;
        s.body_bytes = (int32_t)best;
        s.hdr_bits = bt == 2 ? (int32_t)dyn_hdr : 3;
    }
    __syncthreads();
    const int bt = s.btype, body = s.body_bytes, total = kHdr + body + kTrl;
    if (bt == 1) {                                       // the fixed codes
        for (int k = lane; k < 288; k += kNT) {
            const int l = k < 144 ? 8 : k < 256 ? 9 : k < 280 ? 7 : 8;
            const uint32_t c = k < 144 ? 0x30 + k : k < 256 ? 0x190 + (k - 144) : k < 280 ? (k - 256) : 0xC0 + (k - 280);
            s.llen[k] = (uint8_t)l;
            s.lcode[k] = (uint16_t)bitrev(c, l);
        }
        if (lane < 30) { s.dlen[lane] = 5; s.dcode[lane] = (uint16_t)bitrev((uint32_t)lane, 5); }
    }
    for (int w = lane; w < (total + 3) / 4; w += kNT) o[w] = 0;
    __syncthreads();

    const uint32_t b0 = 8 * kHdr;
    if (bt == 0) {                                       // one stored block
        if (lane == 0) {
            put_bits(o, b0, 1, 3);
            put_bits(o, b0 + 8, (uint32_t)n | (uint32_t)(~n & 0xFFFF) << 16, 32);
        }
        for (int w = lane; w < nw; w += kNT) put_bits(o, b0 + 40 + 32 * w, s.in[w], 32);
    } else {
        if (lane == 0) {
            put_bits(o, b0, 1 | bt << 1, 3);
            if (bt == 2) {
                uint32_t p = b0 + 3;
                put_bits(o, p, (uint32_t)(s.hlit - 257) | (uint32_t)(s.hdist - 1) << 5 | (uint32_t)(s.hclen - 4) << 10, 14);
                p += 14;
                for (int k = 0; k < s.hclen; ++k, p += 3) put_bits(o, p, s.clen[kClOrderD[k]], 3);
                for (int k = 0; k < s.n_rle; ++k) {
                    const int sym = s.rle_sym[k];
                    put_bits(o, p, s.ccode[sym], s.clen[sym]);
                    p += s.clen[sym];
                    const int nx = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
                    put_bits(o, p, s.rle_ext[k], nx);
                    p += nx;
                }
            }
        }
        // bits of the lane's symbols, their offsets, then the symbols
        uint32_t bits = 0;
        for (int p = start; p < seg_end;) {
            const uint32_t mv = match[p];
            if (mv >> 16) {
                int c, nx, x, dc, dnx, dx;
                len_code((int)(mv >> 16), c, nx, x);
                dist_code((int)(mv & 0xFFFF) + 1, dc, dnx, dx);
                bits += s.llen[257 + c] + nx + s.dlen[dc] + dnx;
                p += (int)(mv >> 16);
            } else {
                bits += s.llen[byte_at(s, p)];
                ++p;
            }
        }
        s.part[lane] = bits;
        __syncthreads();
        if (lane == 0) {
            uint32_t acc = 0;
            for (int t = 0; t < kNT; ++t) { const uint32_t v = s.part[t]; s.part[t] = acc; acc += v; }
            put_bits(o, b0 + s.hdr_bits + acc, s.lcode[256], s.llen[256]);
        }
        __syncthreads();
        uint32_t q = b0 + s.hdr_bits + s.part[lane];
        for (int p = start; p < seg_end;) {
            const uint32_t mv = match[p];
            if (mv >> 16) {
                int c, nx, x, dc, dnx, dx;
                len_code((int)(mv >> 16), c, nx, x);
                dist_code((int)(mv & 0xFFFF) + 1, dc, dnx, dx);
                uint64_t v = s.lcode[257 + c];
                int nb = s.llen[257 + c];
                v |= (uint64_t)x << nb; nb += nx;
                v |= (uint64_t)s.dcode[dc] << nb; nb += s.dlen[dc];
                v |= (uint64_t)dx << nb; nb += dnx;
                put_bits(o, q, v, nb);
                q += nb;
                p += (int)(mv >> 16);
            } else {
                const uint32_t c = byte_at(s, p);
                put_bits(o, q, s.lcode[c], s.llen[c]);
                q += s.llen[c];
                ++p;
            }
        }
    }
    if (lane == 0) {                                     // bgzip's header, the trailer, the size
        const uint32_t bsize = (uint32_t)(total - 1);
        put_bits(o, 0, 0x04088b1fu, 32);                 // ID1 ID2 CM FLG(FEXTRA)
        put_bits(o, 64, 0x0006ff00u, 32);                // XFL OS(255) XLEN = 6
        put_bits(o, 96, 0x00024342u, 32);                // 'B' 'C' SLEN = 2
        put_bits(o, 128, bsize, 16);
        put_bits(o, 8u * (kHdr + body), crc, 32);
        put_bits(o, 8u * (kHdr + body) + 32, (uint32_t)n, 32);
        *size_out = total;
    }
}

__global__ __launch_bounds__(kNT, 2) void deflate_kernel(const uint8_t *__restrict__ in, int64_t n, int n_members,
                                                         uint16_t *__restrict__ prev_ws, uint32_t *__restrict__ match_ws,
                                                         uint32_t *__restrict__ slots, int32_t *__restrict__ sizes) {
    __shared__ Lds s;
    const int lane = (int)threadIdx.x;
    uint16_t *prev = prev_ws + (size_t)blockIdx.x * kBlock;
    uint32_t *match = match_ws + (size_t)blockIdx.x * kBlock;
    for (int k = (int)blockIdx.x; k < n_members; k += (int)gridDim.x) {
        const int64_t a = (int64_t)k * kBlock;
        const int len = (int)min((int64_t)kBlock, n - a);
        deflate_member(s, in + a, len, prev, match, slots + (size_t)k * (kSlot / 4), sizes + k, lane);
    }
}

// off[k] = sum of sizes[0, k), off[n_members] = the total; one workgroup
__global__ __launch_bounds__(kNT) void deflate_scan(const int32_t *__restrict__ sizes, int n_members, int64_t *__restrict__ off) {
    __shared__ int64_t part[kNT];
    const int lane = (int)threadIdx.x;
    const int per = (n_members + kNT - 1) / kNT, a = min(lane * per, n_members), e = min(a + per, n_members);
    int64_t t = 0;
    for (int k = a; k < e; ++k) t += sizes[k];
    part[lane] = t;
    __syncthreads();
    if (lane == 0) {
        int64_t acc = 0;
        for (int i = 0; i < kNT; ++i) { const int64_t v = part[i]; part[i] = acc; acc += v; }
        off[n_members] = acc;
    }
    __syncthreads();
    int64_t acc = part[lane];
    for (int k = a; k < e; ++k) { off[k] = acc; acc += sizes[k]; }
}

// member k from its slot to out + off[k]: bytes up to a 4-byte boundary of the destination, then dwords, then the tail
__global__ __launch_bounds__(kNT) void deflate_copy(const uint32_t *__restrict__ slots, const int32_t *__restrict__ sizes,
                                                    const int64_t *__restrict__ off, uint8_t *__restrict__ out) {
    const int k = (int)blockIdx.x, lane = (int)threadIdx.x;
    const uint32_t *src = slots + (size_t)k * (kSlot / 4);
    const uint8_t *sb = reinterpret_cast<const uint8_t *>(src);
    uint8_t *o = out + off[k];
    const int n = sizes[k];
    const int head = min((int)((4 - ((uintptr_t)o & 3)) & 3), n);
    if (lane < head) o[lane] = sb[lane];
    const int nw = (n - head) >> 2, sh = head * 8;
    uint32_t *ow = reinterpret_cast<uint32_t *>(o + head);
    for (int w = lane; w < nw; w += kNT) {
        ow[w] = sh ? (src[w] >> sh) | (src[w + 1] << (32 - sh)) : src[w];   // head < 4: byte head + 4w lies in word w
    }
    const int t = head + 4 * nw;
    if (t + lane < n) o[t + lane] = sb[t + lane];
}

int device_check(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) {
        (void)hipGetLastError();
        set_last_error("no usable HIP device");
        return BWAMS_ERR_DEVICE;
    }
    hipDeviceProp_t p;
    BWAMS_HIP(hipGetDeviceProperties(&p, device));
    if (std::string(p.gcnArchName).rfind("gfx950", 0) != 0) {
        set_last_error(std::string("device is ") + p.gcnArchName + ", this library is built for gfx950 only");
        return BWAMS_ERR_DEVICE;
    }
    return BWAMS_OK;
}

}  // namespace

struct bwams_deflater {
    int device = 0;
    int64_t max_in = 0, per_launch = 0;               // members one launch takes
    int grid = 0;                                     // workgroups (workspace slots)
    hipStream_t st = nullptr;
    hipEvent_t ev[4] = {}, after = nullptr;
    bwams::DevBuf<uint8_t> d_in, d_out;               // host input / host output staging
    bwams::DevBuf<uint16_t> d_prev;
    bwams::DevBuf<uint32_t> d_match, d_slots;
    bwams::DevBuf<int32_t> d_size;
    bwams::DevBuf<int64_t> d_off;
    bwams::HostBuf<int64_t> h_total;                  // page-locked
};

namespace bwams {

int deflater_device(const bwams_deflater *d) { return d->device; }

// bwams_deflater_run with its work ordered behind the work queued on `after` so far (nullptr: no wait)
int deflater_run_after(bwams_deflater *d, hipStream_t after, const void *in, int64_t n_bytes, int in_on_device, void *out, int64_t out_cap,
                       int out_on_device, int32_t flags, int64_t *n_out, bwams_deflate_stats_t *stats) {
    if (!d || n_bytes < 0 || (!in && n_bytes) || out_cap < 0 || !out || (flags & ~BWAMS_DEFLATE_EOF)) {
        set_last_error("bwams_deflater_run: invalid argument");
        return BWAMS_ERR_ARG;
    }
    if (n_out) *n_out = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    const int64_t need = bwams_deflate_bound(n_bytes);
    if (out_cap < need) {
        set_last_error("bwams_deflater_run: out_cap " + std::to_string(out_cap) + " is below bwams_deflate_bound(" + std::to_string(n_bytes) +
                       ") = " + std::to_string(need));
        if (n_out) *n_out = need;
        return BWAMS_ERR_CAPACITY;
    }
    BWAMS_HIP(hipSetDevice(d->device));
    if (after) {
        BWAMS_HIP(hipEventRecord(d->after, after));
        BWAMS_HIP(hipStreamWaitEvent(d->st, d->after, 0));
    }
    const int64_t step = d->per_launch * kBlock;
    int64_t pos = 0, members = 0;
    float ms[3] = {0, 0, 0};
    for (int64_t a = 0; a < n_bytes; a += step) {
        const int64_t len = std::min(step, n_bytes - a);
        const int nm = (int)((len + kBlock - 1) / kBlock);
        const uint8_t *src = static_cast<const uint8_t *>(in) + a;
        BWAMS_HIP(hipEventRecord(d->ev[0], d->st));
        if (!in_on_device) {
            BWAMS_HIP(hipMemcpyAsync(d->d_in.p, src, (size_t)len, hipMemcpyHostToDevice, d->st));
            src = d->d_in.p;
        }
        BWAMS_HIP(hipEventRecord(d->ev[1], d->st));
        hipLaunchKernelGGL(deflate_kernel, dim3((unsigned)std::min(nm, d->grid)), dim3(kNT), 0, d->st, src, len, nm, d->d_prev.p, d->d_match.p,
                           d->d_slots.p, d->d_size.p);
        BWAMS_HIP(hipGetLastError());
        hipLaunchKernelGGL(deflate_scan, dim3(1), dim3(kNT), 0, d->st, d->d_size.p, nm, d->d_off.p);
        BWAMS_HIP(hipGetLastError());
        uint8_t *dst = out_on_device ? static_cast<uint8_t *>(out) + pos : d->d_out.p;
        hipLaunchKernelGGL(deflate_copy, dim3((unsigned)nm), dim3(kNT), 0, d->st, d->d_slots.p, d->d_size.p, d->d_off.p, dst);
        BWAMS_HIP(hipGetLastError());
        BWAMS_HIP(hipEventRecord(d->ev[2], d->st));
        BWAMS_HIP(hipMemcpyAsync(d->h_total.p, d->d_off.p + nm, sizeof(int64_t), hipMemcpyDeviceToHost, d->st));
        BWAMS_HIP(hipStreamSynchronize(d->st));
        const int64_t got = *d->h_total.p;
        if (!out_on_device) BWAMS_HIP(hipMemcpyAsync(static_cast<uint8_t *>(out) + pos, d->d_out.p, (size_t)got, hipMemcpyDeviceToHost, d->st));
        BWAMS_HIP(hipEventRecord(d->ev[3], d->st));
        BWAMS_HIP(hipEventSynchronize(d->ev[3]));
        float t;
        BWAMS_HIP(hipEventElapsedTime(&t, d->ev[0], d->ev[1])); ms[0] += t;
        BWAMS_HIP(hipEventElapsedTime(&t, d->ev[1], d->ev[2])); ms[1] += t;
        BWAMS_HIP(hipEventElapsedTime(&t, d->ev[2], d->ev[3])); ms[2] += t;
        pos += got;
        members += nm;
    }
    if (flags & BWAMS_DEFLATE_EOF) {
        if (out_on_device) {
            BWAMS_HIP(hipMemcpyAsync(static_cast<uint8_t *>(out) + pos, kEofMember, kEofLen, hipMemcpyHostToDevice, d->st));
            BWAMS_HIP(hipStreamSynchronize(d->st));
        } else {
            memcpy(static_cast<uint8_t *>(out) + pos, kEofMember, kEofLen);
        }
        pos += kEofLen;
    }
    if (stats) {
        stats->members = members;
        stats->in_bytes = n_bytes;
        stats->out_bytes = pos;
        stats->ms_upload = ms[0];
        stats->ms_kernel = ms[1];
        stats->ms_download = ms[2];
    }
    if (n_out) *n_out = pos;
    return BWAMS_OK;
}

}  // namespace bwams

extern "C" {

int64_t bwams_deflate_bound(int64_t n_bytes) {
    if (n_bytes < 0) return 0;
    return n_bytes + 31 * ((n_bytes + kBlock - 1) / kBlock) + kEofLen;
}

int bwams_deflater_destroy(bwams_deflater_t *d) {
    if (!d) return BWAMS_OK;
    (void)hipSetDevice(d->device);
    if (d->st) (void)hipStreamSynchronize(d->st);
    for (auto e : d->ev) if (e) (void)hipEventDestroy(e);
    if (d->after) (void)hipEventDestroy(d->after);
    if (d->st) (void)hipStreamDestroy(d->st);
    delete d;
    return BWAMS_OK;
}

int bwams_deflater_create(int device, int64_t max_in_bytes, bwams_deflater_t **out) {
    if (!out) return BWAMS_ERR_ARG;
    *out = nullptr;
    if (max_in_bytes < kBlock || max_in_bytes > ((int64_t)1 << 40)) {
        set_last_error("bwams_deflater_create: max_in_bytes must be at least 65280 (one BGZF member's input)");
        return BWAMS_ERR_ARG;
    }
    if (int rc = device_check(device)) return rc;
    BWAMS_HIP(hipSetDevice(device));
    int cus = 0;
    BWAMS_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    auto *d = new bwams_deflater();
    d->device = device;
    d->max_in = max_in_bytes;
    d->per_launch = max_in_bytes / kBlock;
    d->grid = (int)std::min<int64_t>(d->per_launch, 2 * (int64_t)std::max(cus, 1));   // two members per CU
    const int64_t step = d->per_launch * kBlock;
    auto fail = [&](hipError_t e) {
        set_last_error(std::string("bwams_deflater_create: ") + hipGetErrorString(e));
        bwams_deflater_destroy(d);
        return e == hipErrorOutOfMemory ? BWAMS_ERR_NOMEM : BWAMS_ERR_DEVICE;
    };
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&d->st, hipStreamNonBlocking)) != hipSuccess) return fail(e);
    for (auto &x : d->ev)
        if ((e = hipEventCreate(&x)) != hipSuccess) return fail(e);
    if ((e = hipEventCreateWithFlags(&d->after, hipEventDisableTiming)) != hipSuccess) return fail(e);
    if ((e = d->d_in.alloc((size_t)step)) != hipSuccess) return fail(e);
    if ((e = d->d_out.alloc((size_t)(step + 31 * d->per_launch))) != hipSuccess) return fail(e);
    if ((e = d->d_prev.alloc(sizeof(uint16_t) * kBlock * (size_t)d->grid)) != hipSuccess) return fail(e);
    if ((e = d->d_match.alloc(sizeof(uint32_t) * kBlock * (size_t)d->grid)) != hipSuccess) return fail(e);
    if ((e = d->d_slots.alloc((size_t)kSlot * (size_t)d->per_launch)) != hipSuccess) return fail(e);
    if ((e = d->d_size.alloc(sizeof(int32_t) * (size_t)d->per_launch)) != hipSuccess) return fail(e);
    if ((e = d->d_off.alloc(sizeof(int64_t) * (size_t)(d->per_launch + 1))) != hipSuccess) return fail(e);
    if ((e = d->h_total.alloc(sizeof(int64_t))) != hipSuccess) return fail(e);
    *out = d;
    return BWAMS_OK;
}

int bwams_deflater_run(bwams_deflater_t *d, const void *in, int64_t n_bytes, int in_on_device, void *out, int64_t out_cap, int out_on_device,
                       int32_t flags, int64_t *n_out, bwams_deflate_stats_t *stats) {
    return deflater_run_after(d, nullptr, in, n_bytes, in_on_device, out, out_cap, out_on_device, flags, n_out, stats);
}

}  // extern "C"
