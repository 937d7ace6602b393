// gunzip.hip — plain gzip input inflated on the device: one DEFLATE stream decoded in parallel pieces, their windows resolved after.
//
// Replaces the gzread() behind kseq for a .gz file that is not BGZF: one stream (or a few members) with no table of member sizes.  The
// scheme is the two-stage one of pugz / rapidgzip.  The compressed bytes of a call are cut into pieces of piece_bytes; then
//   gz_find_kernel    a lane per bit offset of a piece: the first offset at which a non-final dynamic block header parses under the
//                     decoder's own rules (the 17 header bits and the Kraft sum of the code lengths code on every lane, the code
//                     lengths themselves for the few survivors).  A candidate is a hint, never trusted;
//   gz_count_kernel   a wave per piece decodes from its start (piece 0: the known position; later ones: their candidate) to the first
//                     block boundary at or behind the next piece's candidate, without output: the boundary reached, the bytes produced
//                     up to it, how far back behind its own start it referred, the gzip members that ended inside it;
//   (host)            the chain check: piece p + 1 stands when p ended exactly on its candidate; by induction from piece 0 a piece that
//                     stands is decoded as a sequential decoder would decode it.  A piece that does not stand is dropped and its
//                     predecessor counted again up to the next candidate.  An exclusive scan of the counts places every piece;
//   gz_decode_kernel  a wave per standing piece decodes again, now to 16-bit symbols: a byte, or 0x8000 | k = byte k of the 32 KiB in
//                     front of the piece's start.  The last 32768 symbols live in an LDS ring (back-references copy symbols, markers
//                     included); every symbol also goes to HBM at the piece's offset;
//   gz_window_kernel  one workgroup walks the pieces in order: the window behind piece p is the last 32768 symbols of (the window in
//                     front of p, p's output) with the markers looked up in the window in front of p.  The only sequential step;
//   gz_resolve_kernel every output byte in parallel: a symbol is itself or its window's byte; a tile's bytes are written in dwords and
//                     their CRC32 computed; the host joins the tiles' CRCs per member by x^(8n) mod P and compares with the trailers.
// No kernel reads outside [gz, gz + n_bytes) (bytes past the end read as 0 and count as an overrun) or writes outside its piece's
// ranges (the count pass writes its records only), and every decoder ends, since a symbol consumes at least one bit: damaged or
// speculative input gives a status, never a fault.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "crc32.h"
#include "inflate_common.h"

using namespace bwams;

namespace {

constexpr int kWin = 32768;              // DEFLATE's window
constexpr int kTile = 32768;             // output bytes per workgroup of the resolve pass
constexpr int kMemberMin = 18;           // two member ends are at least this many bytes apart (a header, an empty block, a trailer)
constexpr int64_t kNoTarget = INT64_MAX;
using Bits64 = BitsT<int64_t>;           // byte positions inside the call's input

enum Phase : int32_t { PH_DEFLATE = 0, PH_TRAILER, PH_HEADER, PH_DONE };   // what the stream's next bytes are

struct PieceIn {                         // one piece as a decoder sees it
    int64_t start_bit, target_bit;       // from here to the first boundary at or behind target_bit
    int64_t sym_off, count;              // decode pass: where its symbols go and how many
    int32_t phase, mem_slot;             // the phase at start_bit; count pass: its first slot of the member list
};
struct PieceRec {                        // what the count pass found
    int64_t end_bit, end_out, err_bit;   // the last boundary completed, the bytes produced up to it, where a status arose
    int32_t end_phase, status, reach, n_members;   // reach: the furthest back behind its own start, before any member boundary
};
struct MemberEnd {
    int64_t out_pos, trailer_byte;       // the piece's bytes in front of this member's end; where its trailer is
    uint32_t crc, isize;
};
struct Tile {
    int64_t off;                         // in the call's output (and in the symbols)
    int32_t n, win;                      // bytes; the window in front of its piece
};

struct LdsCount {
    uint8_t in[kInWin];
    uint16_t ltab[1 << kLRoot], dtab[1 << kDRoot];
    uint16_t lsym[288], dsym[32], lcnt[16], dcnt[16], off[16], next[16];
    uint8_t lens[320];
};
struct LdsDecode : LdsCount {
    uint16_t ring[kWin];
};

__device__ __forceinline__ int64_t bitpos(const Bits64 &b) { return b.ip * 8 - b.bc; }
__device__ __forceinline__ void seek(Bits64 &b, int64_t byte) { b.bb = 0; b.bc = 0; b.ip = byte; }

struct Out {                             // a decoder's output side
    int64_t pos, hist;                   // symbols so far; where the current member began (once `crossed`)
    int32_t reach, crossed;
    uint16_t *sym;                       // decode pass: the piece's symbols in HBM,
    int64_t count;                       //   and how many of them are its own
};

// One DEFLATE block behind its 3 header bits (`type`): the rules of inflate_member (inflate.hip), output as symbols or none.
template <bool EMIT, class L>
__device__ int block(L &s, const uint8_t *__restrict__ gz, int64_t n_bytes, Bits64 &b, int type, Out &o, int lane) {
    const int64_t n_bits = n_bytes * 8;
    const Code lc{s.ltab, s.lcnt, s.lsym, kLRoot}, dc{s.dtab, s.dcnt, s.dsym, kDRoot}, cc{s.ltab, s.lcnt, s.lsym, 7};
    if (type == 0) {                                  // stored
        take(b, b.bc & 7);
        const uint32_t len = take(b, 16), nlen = take(b, 16);
        if (bitpos(b) > n_bits) return ST_OVERRUN;
        if (len != (~nlen & 0xffffu)) return ST_STORED_LEN;
        const int64_t p = b.ip - b.bc / 8;            // the byte behind NLEN
        if (p + (int64_t)len > n_bytes) return ST_OVERRUN;
        if constexpr (EMIT) {
            __syncthreads();
            for (int i = lane; i < (int)len; i += 64) {
                const uint16_t v = gz[p + i];
                static_cast<LdsDecode &>(s).ring[(o.pos + i) & (kWin - 1)] = v;
                if (o.pos + i < o.count) o.sym[o.pos + i] = v;
            }
        }
        o.pos += len;
        seek(b, p + len);
        return ST_OK;
    }
    if (type == 3) return ST_BTYPE;
    int rc;
    if (type == 1) {                                  // fixed codes
        __syncthreads();
        for (int i = lane; i < 320; i += 64) s.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
        if ((rc = build(s, s.lens, 288, lc, false, lane))) return rc;
        if ((rc = build(s, s.lens + 288, 32, dc, false, lane))) return rc;
    } else {                                          // dynamic codes
        const int nlen = (int)take(b, 5) + 257, ndist = (int)take(b, 5) + 1, ncode = (int)take(b, 4) + 4;
        if (nlen > 286 || ndist > 30) return ST_COUNTS;
        refill(b, s, gz, n_bytes, lane);
        __syncthreads();
        if (lane < 19) s.lens[lane] = 0;
        __syncthreads();
        for (int i = 0; i < ncode; ++i) {
            const uint8_t v = (uint8_t)take(b, 3);
            if (lane == 0) s.lens[kClOrder[i]] = v;
        }
        if (build(s, s.lens, 19, cc, true, lane)) return ST_CODE_LENS;
        int n = 0, prev = 0;
        while (n < nlen + ndist) {
            if (b.bc < 32) refill(b, s, gz, n_bytes, lane);
            if (bitpos(b) > n_bits) return ST_OVERRUN;
            const int sym = decode(b, cc);
            if (sym < 0) return ST_CODE_LENS;
            if (sym < 16) {
                if (lane == 0) s.lens[n] = (uint8_t)sym;
                prev = sym;
                ++n;
                continue;
            }
            int v, rep;
            if (sym == 16) {
                if (n == 0) return ST_REPEAT;
                v = prev; rep = 3 + (int)take(b, 2);
            } else if (sym == 17) {
                v = 0; rep = 3 + (int)take(b, 3);
            } else {
                v = 0; rep = 11 + (int)take(b, 7);
            }
            if (n + rep > nlen + ndist) return ST_REPEAT;
            for (int i = lane; i < rep; i += 64) s.lens[n + i] = (uint8_t)v;
            prev = v;
            n += rep;
        }
        __syncthreads();
        if (s.lens[256] == 0) return ST_NO_EOB;
        if ((rc = build(s, s.lens, nlen, lc, false, lane))) return rc;
        if ((rc = build(s, s.lens + nlen, ndist, dc, false, lane))) return rc;
    }
    for (;;) {                                        // the block's symbols
        if (b.bc < 48) refill(b, s, gz, n_bytes, lane);
        if (bitpos(b) > n_bits) return ST_OVERRUN;
        int sym = decode(b, lc);
        if (sym < 0) return ST_BAD_LITLEN;
        if (sym < 256) {
            if constexpr (EMIT) {
                if (lane == 0) {
                    static_cast<LdsDecode &>(s).ring[o.pos & (kWin - 1)] = (uint16_t)sym;
                    if (o.pos < o.count) o.sym[o.pos] = (uint16_t)sym;
                }
            }
            ++o.pos;
            continue;
        }
        if (sym == 256) return ST_OK;
        sym -= 257;
        if (sym >= 29) return ST_BAD_LITLEN;
        const int len = kLenBase[sym] + (int)take(b, kLenExtra[sym]);
        const int dsym = decode(b, dc);
        if (dsym < 0 || dsym >= 30) return ST_BAD_DIST;
        const int dist = kDistBase[dsym] + (int)take(b, kDistExtra[dsym]);
        const int64_t have = o.pos - o.hist;          // bytes of this member the piece itself produced
        if (dist > have) {
            if (o.crossed) return ST_FAR;             // behind a member boundary the history is known to be empty
            o.reach = max(o.reach, (int32_t)(dist - have));
        }
        if constexpr (EMIT) {
            uint16_t *ring = static_cast<LdsDecode &>(s).ring;
            __syncthreads();                          // the literals and matches before this one are in LDS
            const int64_t from = o.pos - dist;        // below 0: the ring still holds the markers of the window in front of the piece
            for (int i = lane; i < len; i += 64) {
                const uint16_t v = ring[(from + (dist >= len ? i : i % dist)) & (kWin - 1)];
                ring[(o.pos + i) & (kWin - 1)] = v;
                if (o.pos + i < o.count) o.sym[o.pos + i] = v;
            }
        }
        o.pos += len;
    }
}

// A gzip member header at the (byte-aligned) reader: ID1 ID2 CM FLG MTIME XFL OS, then FEXTRA, FNAME, FCOMMENT and FHCRC skipped.
// *gzip = 0: the two bytes there are no gzip magic (nothing is consumed).
template <class L> __device__ int gz_header(L &s, const uint8_t *__restrict__ gz, int64_t n_bytes, Bits64 &b, int lane, int *gzip) {
    const int64_t n_bits = n_bytes * 8;
    refill(b, s, gz, n_bytes, lane);
    const int64_t left = n_bytes - (bitpos(b) >> 3);
    *gzip = 1;
    if (left < 2) return ST_OVERRUN;
    if ((b.bb & 0xffff) != 0x8b1f) { *gzip = 0; return ST_OK; }
    if (left < 4) return ST_OVERRUN;
    take(b, 16);
    const int cm = (int)take(b, 8), flg = (int)take(b, 8);
    if (cm != 8) return ST_GZ_METHOD;
    if (flg & 0xe0) return ST_GZ_FLAGS;
    refill(b, s, gz, n_bytes, lane);
    take(b, 32); take(b, 16);                         // MTIME, XFL, OS
    if (flg & 4) {                                    // FEXTRA
        refill(b, s, gz, n_bytes, lane);
        const int64_t xlen = take(b, 16);
        seek(b, (bitpos(b) >> 3) + xlen);
    }
    for (int f = 8; f <= 16; f <<= 1)                 // FNAME, FCOMMENT: zero-terminated
        if (flg & f) {
            uint32_t c;
            do {
                refill(b, s, gz, n_bytes, lane);
                if (bitpos(b) >= n_bits) return ST_OVERRUN;
                c = take(b, 8);
            } while (c);
        }
    if (flg & 2) {                                    // FHCRC
        refill(b, s, gz, n_bytes, lane);
        take(b, 16);
    }
    return bitpos(b) > n_bits ? ST_OVERRUN : ST_OK;
}

// The decoder of both passes: from pi.start_bit in pi.phase to the first boundary at or behind pi.target_bit, or to where a status
// stops it.  A boundary: the end of a block, of a trailer, of a header.  r holds the last boundary completed.
template <bool EMIT, class L>
__device__ void walk(L &s, const uint8_t *__restrict__ gz, int64_t n_bytes, const PieceIn &pi, MemberEnd *__restrict__ mem,
                     int64_t mem_cap, uint16_t *__restrict__ sym, int lane, PieceRec &r) {
    const int64_t n_bits = n_bytes * 8;
    Bits64 b{0, 0, pi.start_bit >> 3, pi.start_bit >> 3};
    window_load(s, gz, n_bytes, b.base, lane);
    refill(b, s, gz, n_bytes, lane);
    take(b, (int)(pi.start_bit & 7));
    Out o{0, 0, 0, 0, sym, pi.count};
    int phase = pi.phase, st = ST_OK, n_mem = 0;
    r = PieceRec{pi.start_bit, 0, pi.start_bit, phase, ST_OK, 0, 0};
    for (;;) {
        if (phase == PH_DEFLATE) {
            refill(b, s, gz, n_bytes, lane);
            if (bitpos(b) > n_bits) { st = ST_OVERRUN; break; }
            const int last = (int)take(b, 1), type = (int)take(b, 2);
            if ((st = block<EMIT>(s, gz, n_bytes, b, type, o, lane))) break;
            if (last) {
                take(b, b.bc & 7);
                phase = PH_TRAILER;
            }
        } else if (phase == PH_TRAILER) {
            const int64_t at = bitpos(b) >> 3;
            refill(b, s, gz, n_bytes, lane);
            const uint32_t crc = take(b, 32);
            refill(b, s, gz, n_bytes, lane);
            const uint32_t isize = take(b, 32);
            if (bitpos(b) > n_bits) { st = ST_OVERRUN; break; }
            if (!EMIT && lane == 0 && n_mem < mem_cap) mem[n_mem] = MemberEnd{o.pos, at, crc, isize};
            ++n_mem;
            o.hist = o.pos;
            o.crossed = 1;
            phase = PH_HEADER;
        } else {                                      // PH_HEADER
            int gzip;
            if ((st = gz_header(s, gz, n_bytes, b, lane, &gzip))) break;
            if (!gzip) {                              // what follows is not gzip: ignored, as gzread ignores it
                r.end_phase = PH_DONE;
                st = ST_END;
                break;
            }
            phase = PH_DEFLATE;
        }
        const int64_t bp = bitpos(b);
        if (bp > n_bits) { st = ST_OVERRUN; break; }
        r.end_bit = bp; r.end_out = o.pos; r.end_phase = phase; r.n_members = n_mem; r.reach = o.reach;
        if (bp >= pi.target_bit) break;
    }
    r.err_bit = min(bitpos(b), n_bits);
    // a status met within reach of the input's end may come from the zeros read behind it: the input ran out
    if (st != ST_OK && st != ST_END && bitpos(b) + 64 > n_bits) st = ST_OVERRUN;
    r.status = st;
}

__global__ __launch_bounds__(64) void gz_count_kernel(const uint8_t *__restrict__ gz, int64_t n_bytes, const PieceIn *__restrict__ pin,
                                                      const int32_t *__restrict__ todo, PieceRec *__restrict__ rec,
                                                      MemberEnd *__restrict__ mem, int64_t mem_cap) {
    __shared__ LdsCount s;
    const int lane = (int)threadIdx.x, p = todo[blockIdx.x];
    const PieceIn pi = pin[p];
    PieceRec r;
    walk<false>(s, gz, n_bytes, pi, mem + pi.mem_slot, mem_cap - pi.mem_slot, nullptr, lane, r);
    if (lane == 0) rec[p] = r;
}

__global__ __launch_bounds__(64) void gz_decode_kernel(const uint8_t *__restrict__ gz, int64_t n_bytes, const PieceIn *__restrict__ pin,
                                                       uint16_t *__restrict__ sym) {
    __shared__ LdsDecode s;
    const int lane = (int)threadIdx.x;
    const PieceIn pi = pin[blockIdx.x];
    for (int k = lane; k < kWin; k += 64) s.ring[k] = (uint16_t)(0x8000 | k);     // position k - 32768: byte k of the window in front
    PieceRec r;
    walk<true>(s, gz, n_bytes, pi, nullptr, 0, sym + pi.sym_off, lane, r);
}

// ---------------------------------------------------------------------------------------------------------------- candidates
__device__ __forceinline__ uint64_t peek_bits(const uint8_t *__restrict__ gz, int64_t n_bytes, int64_t bit, int n_load) {
    uint64_t v = 0;                                   // n_load bytes from the byte of `bit`, shifted down to it
    const int64_t at = bit >> 3;
    for (int i = 0; i < n_load; ++i) v |= (uint64_t)(at + i < n_bytes ? gz[at + i] : 0) << (8 * i);
    return v >> (bit & 7);
}

// Does a non-final dynamic block header parse at `bit`?  The rules are those of block(): the counts, a complete code lengths code,
// the repeat codes, an end-of-block code, neither an over-subscribed nor an incomplete literal/length or distance code.
__device__ bool candidate(const uint8_t *__restrict__ gz, int64_t n_bytes, int64_t bit) {
    const uint32_t h = (uint32_t)peek_bits(gz, n_bytes, bit, 3);
    if ((h & 7) != 4) return false;                   // BFINAL = 0, BTYPE = 2
    const int nlen = (int)(h >> 3 & 31) + 257, ndist = (int)(h >> 8 & 31) + 1, ncode = (int)(h >> 13 & 15) + 4;
    if (nlen > 286 || ndist > 30) return false;
    const uint64_t cl = peek_bits(gz, n_bytes, bit + 17, 8);
    int kraft = 0;
    for (int i = 0; i < ncode; ++i) {
        const int v = (int)(cl >> (3 * i) & 7);
        if (v) kraft += 128 >> v;
    }
    if (kraft != 128) return false;                   // one offset in some 2000 gets this far: the rest runs on few lanes
    uint8_t cnt[8] = {}, len19[19] = {};
    for (int i = 0; i < ncode; ++i) {
        const int v = (int)(cl >> (3 * i) & 7);
        len19[kClOrder[i]] = (uint8_t)v;
        ++cnt[v];
    }
    uint8_t sym[19];                                  // the code lengths code, canonical: symbols by (length, value)
    int ns = 0;
    for (int l = 1; l <= 7; ++l)
        for (int i = 0; i < 19; ++i)
            if (len19[i] == l) sym[ns++] = (uint8_t)i;
    const int64_t n_bits = n_bytes * 8, pos0 = bit + 17 + 3 * ncode;
    uint64_t bb = 0;                                  // the lane's own bit buffer: four bytes per refill, their loads independent
    int bc = 0;
    int64_t at = pos0 >> 3;
    auto fill = [&]() {
        while (bc <= 32) {
            uint32_t v = 0;
            for (int i = 0; i < 4; ++i) v |= (uint32_t)(at + i < n_bytes ? gz[at + i] : 0) << (8 * i);
            bb |= (uint64_t)v << bc;
            bc += 32;
            at += 4;
        }
    };
    fill();
    bb >>= pos0 & 7;
    bc -= (int)(pos0 & 7);
    uint16_t lcnt[16] = {}, dcnt[16] = {};
    int n = 0, prev = 0, eob = 0;
    const int total = nlen + ndist;
    while (n < total) {
        fill();
        if (at * 8 - bc > n_bits) return false;
        uint32_t bits = (uint32_t)bb;                 // a code of at most 7 bits, then at most 7 extra bits
        int code = 0, first = 0, index = 0, s = -1, l;
        for (l = 1; l <= 7; ++l) {
            code |= (int)(bits & 1);
            bits >>= 1;
            const int c = cnt[l];
            if (code - c < first) { s = sym[index + (code - first)]; break; }
            index += c;
            first = (first + c) << 1;
            code <<= 1;
        }
        if (s < 0) return false;
        int v = s, rep = 1, used = l;
        if (s == 16) {
            if (n == 0) return false;
            v = prev; rep = 3 + (int)(bits & 3); used += 2;
        } else if (s == 17) {
            v = 0; rep = 3 + (int)(bits & 7); used += 3;
        } else if (s == 18) {
            v = 0; rep = 11 + (int)(bits & 127); used += 7;
        }
        bb >>= used;
        bc -= used;
        if (n + rep > total) return false;
        for (int i = 0; i < rep; ++i, ++n) {
            if (n < nlen) ++lcnt[v]; else ++dcnt[v];
            if (n == 256) eob = v;
        }
        prev = v;
    }
    const int64_t pos = at * 8 - bc;
    if (pos > n_bits || eob == 0) return false;
    for (int k = 0; k < 2; ++k) {
        const uint16_t *c = k ? dcnt : lcnt;
        int left = 1, mx = 0;
        for (int l = 1; l <= 15; ++l) {
            left = (left << 1) - c[l];
            if (left < 0) return false;
            if (c[l]) mx = l;
        }
        if (mx && left > 0 && mx != 1) return false;
    }
    return true;
}

// cand[k], k >= 1: the first bit offset of piece k at which a block header parses, or -1
__global__ __launch_bounds__(256) void gz_find_kernel(const uint8_t *__restrict__ gz, int64_t n_bytes, int64_t piece_bits,
                                                      int64_t *__restrict__ cand) {
    __shared__ unsigned long long found;
    const int k = (int)blockIdx.x + 1;
    const int64_t a = k * piece_bits, e = min(a + piece_bits, n_bytes * 8);
    if (threadIdx.x == 0) found = ~0ull;
    __syncthreads();
    for (int64_t base = a; base < e; base += 256) {
        const int64_t bit = base + threadIdx.x;
        if (bit < e && candidate(gz, n_bytes, bit)) atomicMin(&found, (unsigned long long)bit);
        __syncthreads();
        const bool done = found != ~0ull;
        __syncthreads();
        if (done) break;
    }
    if (threadIdx.x == 0) cand[k] = found == ~0ull ? -1 : (int64_t)found;
}

// -------------------------------------------------------------------------------------------------------- windows and bytes
// win[p + 1] from win[p] and piece p's symbols, p = 0 .. m - 1 in order; off[p]: where piece p's symbols start (off[m]: their end)
__global__ __launch_bounds__(1024) void gz_window_kernel(const uint16_t *__restrict__ sym, const int64_t *__restrict__ off, int m,
                                                         uint8_t *__restrict__ win) {
    __shared__ uint8_t w[2][kWin];
    const int tid = (int)threadIdx.x;
    for (int k = tid; k < kWin; k += 1024) w[0][k] = win[k];
    __syncthreads();
    for (int p = 0; p < m; ++p) {
        const uint8_t *cur = w[p & 1];
        uint8_t *nxt = w[(p + 1) & 1];
        const int64_t o = off[p], n = off[p + 1] - o;
        uint32_t *dst = reinterpret_cast<uint32_t *>(win + (int64_t)(p + 1) * kWin);
        for (int q = tid; q < kWin / 4; q += 1024) {
            uint32_t word = 0;
            for (int i = 0; i < 4; ++i) {
                const int64_t j = n + 4 * q + i;      // in (window, output): the last 32768 of them
                uint32_t v;
                if (j < kWin) {
                    v = cur[j];
                } else {
                    const uint16_t y = sym[o + j - kWin];
                    v = y & 0x8000 ? cur[y & (kWin - 1)] : (y & 255);
                }
                nxt[4 * q + i] = (uint8_t)v;
                word |= v << (8 * i);
            }
            dst[q] = word;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void gz_resolve_kernel(const uint16_t *__restrict__ sym, const Tile *__restrict__ tiles,
                                                         const uint8_t *__restrict__ win, uint8_t *__restrict__ out,
                                                         uint32_t *__restrict__ crc) {
    __shared__ uint8_t buf[kTile];
    __shared__ uint32_t tab[256], part[256];
    const int tid = (int)threadIdx.x;
    const Tile t = tiles[blockIdx.x];
    const uint8_t *w = win + (int64_t)t.win * kWin;
    crc32_table<256>(tab, tid);
    for (int i = tid; i < t.n; i += 256) {
        const uint16_t y = sym[t.off + i];
        buf[i] = y & 0x8000 ? w[y & (kWin - 1)] : (uint8_t)y;
    }
    __syncthreads();
    const uint32_t c = crc32_lds<256>(buf, t.n, tab, part, tid);
    if (tid == 0) crc[blockIdx.x] = c;
    uint8_t *o = out + t.off;                          // bytes up to a 4-byte boundary, then dwords, then the tail
    const int head = min((int)((4 - ((uintptr_t)o & 3)) & 3), t.n);
    if (tid < head) o[tid] = buf[tid];
    const int nw = (t.n - head) >> 2;
    uint32_t *ow = reinterpret_cast<uint32_t *>(o + head);
    for (int q = tid; q < nw; q += 256) {
        const int at = head + 4 * q;
        ow[q] = (uint32_t)buf[at] | (uint32_t)buf[at + 1] << 8 | (uint32_t)buf[at + 2] << 16 | (uint32_t)buf[at + 3] << 24;
    }
    const int tail = head + 4 * nw;
    if (tail + tid < t.n) o[tail + tid] = buf[tail + tid];
}

// the host's copy of crc32.h's field arithmetic: joining the tiles' CRCs
uint32_t h_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
uint32_t h_x8n(uint32_t n) {
    uint32_t sq = 0x40000000u, r = 0x80000000u;
    for (int i = 0; i < 3; ++i) sq = h_mul(sq, sq);
    for (; n; n >>= 1) {
        if (n & 1) r = h_mul(r, sq);
        sq = h_mul(sq, sq);
    }
    return r;
}

}  // namespace

struct bwams_gunzip {
    int device = 0;
    int64_t max_in = 0, max_out = 0, piece = 0, max_pieces = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev[8] = {};
    DevBuf<uint8_t> d_in, d_out, d_win;               // d_win: window p in front of the call's p-th piece; window 0 is the handle's
    DevBuf<uint16_t> d_sym;
    DevBuf<int64_t> d_cand, d_off;
    DevBuf<PieceIn> d_pin;
    DevBuf<PieceRec> d_rec;
    DevBuf<MemberEnd> d_mem;
    DevBuf<int32_t> d_todo;
    DevBuf<Tile> d_tile;
    DevBuf<uint32_t> d_crc;
    HostBuf<int64_t> h_cand;
    HostBuf<PieceIn> h_pin;
    HostBuf<PieceRec> h_rec;
    HostBuf<int32_t> h_todo;
    // where in the stream the handle is
    int32_t phase = PH_HEADER, bit = 0;               // bit: 0-7 of the first unconsumed byte (PH_DEFLATE)
    uint32_t crc = 0;                                 // the current member's CRC32 and length so far
    int64_t len = 0;
    int64_t members_done = 0, bytes_done = 0;         // over every call
};

extern "C" {

int bwams_gunzip_destroy(bwams_gunzip_t *g) {
    if (!g) return BWAMS_OK;
    (void)hipSetDevice(g->device);
    if (g->st) (void)hipStreamSynchronize(g->st);
    for (auto e : g->ev) if (e) (void)hipEventDestroy(e);
    if (g->st) (void)hipStreamDestroy(g->st);
    delete g;
    return BWAMS_OK;
}

int bwams_gunzip_create(int device, int64_t max_in_bytes, int64_t max_out_bytes, int32_t piece_bytes, bwams_gunzip_t **out) {
    if (!out) return BWAMS_ERR_ARG;
    *out = nullptr;
    if (piece_bytes == 0) piece_bytes = 256 << 10;
    if (piece_bytes < 4096 || max_in_bytes < piece_bytes || max_out_bytes < 65536 || max_in_bytes > ((int64_t)1 << 36) ||
        max_out_bytes > ((int64_t)1 << 36)) {
        set_last_error("bwams_gunzip_create: piece_bytes must be at least 4096 (0: 256 KiB), max_in_bytes at least one piece, "
                       "max_out_bytes at least 65536");
        return BWAMS_ERR_ARG;
    }
    if (int rc = device_ok(device)) return rc;
    BWAMS_HIP(hipSetDevice(device));
    auto *g = new bwams_gunzip();
    g->device = device;
    g->max_in = max_in_bytes;
    g->max_out = max_out_bytes;
    g->piece = piece_bytes;
    g->max_pieces = (max_in_bytes + piece_bytes - 1) / piece_bytes;
    auto fail = [&](hipError_t e) {
        set_last_error(std::string("bwams_gunzip_create: ") + hipGetErrorString(e));
        bwams_gunzip_destroy(g);
        return e == hipErrorOutOfMemory ? BWAMS_ERR_NOMEM : BWAMS_ERR_DEVICE;
    };
    const size_t np = (size_t)g->max_pieces;
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking)) != hipSuccess) return fail(e);
    for (auto &x : g->ev)
        if ((e = hipEventCreate(&x)) != hipSuccess) return fail(e);
    if ((e = g->d_in.alloc((size_t)max_in_bytes)) != hipSuccess) return fail(e);
    if ((e = g->d_out.alloc((size_t)max_out_bytes)) != hipSuccess) return fail(e);
    if ((e = g->d_sym.alloc(sizeof(uint16_t) * (size_t)max_out_bytes)) != hipSuccess) return fail(e);
    if ((e = g->d_win.alloc((np + 1) * kWin)) != hipSuccess) return fail(e);
    if ((e = g->d_cand.alloc(sizeof(int64_t) * np)) != hipSuccess) return fail(e);
    if ((e = g->d_off.alloc(sizeof(int64_t) * (np + 1))) != hipSuccess) return fail(e);
    if ((e = g->d_pin.alloc(sizeof(PieceIn) * np)) != hipSuccess) return fail(e);
    if ((e = g->d_rec.alloc(sizeof(PieceRec) * np)) != hipSuccess) return fail(e);
    if ((e = g->d_todo.alloc(sizeof(int32_t) * np)) != hipSuccess) return fail(e);
    if ((e = g->d_mem.alloc(sizeof(MemberEnd) * (size_t)(max_in_bytes / kMemberMin + 2))) != hipSuccess) return fail(e);
    if ((e = g->h_cand.alloc(sizeof(int64_t) * np)) != hipSuccess) return fail(e);
    if ((e = g->h_pin.alloc(sizeof(PieceIn) * np)) != hipSuccess) return fail(e);
    if ((e = g->h_rec.alloc(sizeof(PieceRec) * np)) != hipSuccess) return fail(e);
    if ((e = g->h_todo.alloc(sizeof(int32_t) * np)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(g->d_win.p, 0, kWin, g->st)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(g->st)) != hipSuccess) return fail(e);
    *out = g;
    return BWAMS_OK;
}

int bwams_gunzip_run(bwams_gunzip_t *g, const uint8_t *gz, int64_t n_bytes, int32_t last, void *out, int64_t out_cap, int out_on_device,
                     int64_t *n_consumed, int64_t *n_out, bwams_gunzip_stats_t *stats) {
    if (!g || (!gz && n_bytes) || n_bytes < 0 || out_cap < 0 || (!out && out_cap)) return BWAMS_ERR_ARG;
    if (n_consumed) *n_consumed = 0;
    if (n_out) *n_out = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    BWAMS_HIP(hipSetDevice(g->device));
    auto where = [&](int64_t member, int64_t byte) {
        return "gzip member " + std::to_string(member) + " at byte " + std::to_string(g->bytes_done + byte) + ": ";
    };
    if (g->phase == PH_DONE) {                        // behind the members: ignored, as gzread ignores it
        g->bytes_done += n_bytes;
        if (n_consumed) *n_consumed = n_bytes;
        if (stats) stats->trailing_bytes = stats->in_bytes = n_bytes;
        return BWAMS_OK;
    }
    int64_t n = n_bytes;
    if (n > g->max_in) { n = g->max_in; last = 0; }
    if (g->phase == PH_HEADER && g->members_done == 0) {          // the first bytes of the file
        static const uint8_t magic[2] = {31, 139};
        for (int i = 0; i < 2; ++i)
            if ((i < n && gz[i] != magic[i]) || (i >= n && last)) {
                set_last_error("bwams_gunzip_run: not gzip (the file does not start with a gzip member header)");
                return BWAMS_ERR_UNSUPPORTED;
            }
    }
    if (n == 0) {
        if (!last || g->phase == PH_HEADER) return BWAMS_OK;
        set_last_error(where(g->members_done, 0) + "the stream ends inside a member");
        return BWAMS_ERR_IO;
    }
    const int64_t piece_bits = g->piece * 8, mem_cap = g->max_in / kMemberMin + 2;
    const int np = (int)((n + g->piece - 1) / g->piece);
    const int64_t out_lim = std::min(out_cap, g->max_out);        // the symbols of a call are staged in max_out_bytes entries
    // ---- upload, candidates
    BWAMS_HIP(hipEventRecord(g->ev[0], g->st));
    BWAMS_HIP(hipMemcpyAsync(g->d_in.p, gz, (size_t)n, hipMemcpyHostToDevice, g->st));
    BWAMS_HIP(hipEventRecord(g->ev[1], g->st));
    if (np > 1) {
        hipLaunchKernelGGL(gz_find_kernel, dim3((unsigned)(np - 1)), dim3(256), 0, g->st, g->d_in.p, n, piece_bits, g->d_cand.p);
        BWAMS_HIP(hipGetLastError());
        BWAMS_HIP(hipMemcpyAsync(g->h_cand.p, g->d_cand.p, sizeof(int64_t) * (size_t)np, hipMemcpyDeviceToHost, g->st));
    }
    BWAMS_HIP(hipEventRecord(g->ev[2], g->st));
    BWAMS_HIP(hipStreamSynchronize(g->st));
    // ---- count, chain check
    std::vector<int> live{0};
    for (int k = 1; k < np; ++k)
        if (g->h_cand.p[k] >= 0) live.push_back(k);
    std::vector<char> need((size_t)np, 1);
    PieceIn *pin = g->h_pin.p;
    const PieceRec *rec = g->h_rec.p;
    for (int k : live) {
        pin[k] = PieceIn{k ? g->h_cand.p[k] : (int64_t)g->bit, kNoTarget, 0, 0, k ? PH_DEFLATE : g->phase, 0};
        pin[k].mem_slot = (int32_t)((pin[k].start_bit >> 3) / kMemberMin);
    }
    int64_t dropped = 0, recounts = 0;
    bool settled = false;
    for (;;) {
        int nt = 0;
        for (size_t i = 0; i < live.size(); ++i) {
            const int k = live[i];
            if (!need[(size_t)k]) continue;
            pin[k].target_bit = i + 1 < live.size() ? pin[live[i + 1]].start_bit : kNoTarget;
            g->h_todo.p[nt++] = k;
            need[(size_t)k] = 0;
        }
        BWAMS_HIP(hipMemcpyAsync(g->d_pin.p, pin, sizeof(PieceIn) * (size_t)np, hipMemcpyHostToDevice, g->st));
        BWAMS_HIP(hipMemcpyAsync(g->d_todo.p, g->h_todo.p, sizeof(int32_t) * (size_t)nt, hipMemcpyHostToDevice, g->st));
        hipLaunchKernelGGL(gz_count_kernel, dim3((unsigned)nt), dim3(64), 0, g->st, g->d_in.p, n, g->d_pin.p, g->d_todo.p, g->d_rec.p,
                           g->d_mem.p, mem_cap);
        BWAMS_HIP(hipGetLastError());
        BWAMS_HIP(hipMemcpyAsync(g->h_rec.p, g->d_rec.p, sizeof(PieceRec) * (size_t)np, hipMemcpyDeviceToHost, g->st));
        BWAMS_HIP(hipStreamSynchronize(g->st));
        bool again = false;
        for (size_t i = 0; i + 1 < live.size();) {
            const PieceRec &r = rec[live[i]];
            const int64_t next = pin[live[i + 1]].start_bit;
            if (r.end_phase == PH_DEFLATE && r.end_bit == next) { ++i; continue; }      // piece i + 1 stands
            if (r.status != ST_OK) {                  // the stream stops in piece i (damage, or the members' end): nothing stands behind it
                dropped += (int64_t)(live.size() - (i + 1));
                live.resize(i + 1);
                break;
            }
            size_t j = i + 1;                         // i ran to a boundary behind the candidate: no boundary lies in between
            while (j < live.size() && (pin[live[j]].start_bit < r.end_bit ||
                                       (pin[live[j]].start_bit == r.end_bit && r.end_phase != PH_DEFLATE)))
                ++j;
            dropped += (int64_t)(j - (i + 1));
            live.erase(live.begin() + (std::ptrdiff_t)(i + 1), live.begin() + (std::ptrdiff_t)j);
            if (i + 1 < live.size() && pin[live[i + 1]].start_bit == r.end_bit) continue;
            need[(size_t)live[i]] = 1;                // again, up to the next candidate
            again = true;
            break;
        }
        if (!again) {
            // a dropped piece ran beside the others and may have written into their slots of the member list: once the chain
            // holds, the standing pieces are counted once more on their own
            if (dropped == 0 || settled) break;
            settled = true;
            for (int k : live) need[(size_t)k] = 1;
        }
        ++recounts;
    }
    BWAMS_HIP(hipEventRecord(g->ev[3], g->st));
    // ---- the prefix of the chain this call consumes
    int m = 0;
    int64_t o = 0, mlen = g->len;                     // mlen: the bytes the current member holds in front of the piece
    bool cap_stop = false;
    std::vector<std::vector<MemberEnd>> mem;
    for (size_t i = 0; i < live.size(); ++i) {
        const int k = live[i];
        const PieceRec &r = rec[k];
        if (r.end_bit == pin[k].start_bit && r.end_phase == pin[k].phase) break;       // no boundary reached
        if (o + r.end_out > out_lim) { cap_stop = true; break; }
        if ((r.end_out > 0 || r.n_members > 0) && r.reach > mlen) {
            set_last_error(where(g->members_done, pin[k].start_bit >> 3) + status_text(ST_FAR));
            return BWAMS_ERR_IO;
        }
        mem.emplace_back((size_t)r.n_members);
        if (pin[k].mem_slot + (int64_t)r.n_members > mem_cap) {
            set_last_error("bwams_gunzip_run: more member ends than the member list holds");
            return BWAMS_ERR_IO;
        }
        if (r.n_members) {
            BWAMS_HIP(hipMemcpyAsync(mem.back().data(), g->d_mem.p + pin[k].mem_slot, sizeof(MemberEnd) * (size_t)r.n_members,
                                     hipMemcpyDeviceToHost, g->st));
            BWAMS_HIP(hipStreamSynchronize(g->st));
            mlen = r.end_out - mem.back().back().out_pos;
        } else {
            mlen += r.end_out;
        }
        o += r.end_out;
        ++m;
    }
    const PieceRec &tail = rec[live[(size_t)std::min<size_t>((size_t)m, live.size() - 1)]];   // the piece the call stops in or in front of
    if (!cap_stop && tail.status != ST_OK && tail.status != ST_OVERRUN && tail.status != ST_END) {
        set_last_error(where(g->members_done, tail.err_bit >> 3) + status_text(tail.status));
        return BWAMS_ERR_IO;
    }
    if (m == 0) {
        if (cap_stop) {
            set_last_error("bwams_gunzip_run: the first piece's output (" + std::to_string(rec[0].end_out) + " bytes) does not fit out_cap " +
                           std::to_string(out_cap) + " / max_out_bytes " + std::to_string(g->max_out));
            return BWAMS_ERR_CAPACITY;
        }
        if (last) {
            set_last_error(where(g->members_done, n) + "the stream ends inside a member");
            return BWAMS_ERR_IO;
        }
        if (n == g->max_in) {
            set_last_error("bwams_gunzip_run: no block boundary lies inside max_in_bytes " + std::to_string(g->max_in));
            return BWAMS_ERR_CAPACITY;
        }
        return BWAMS_OK;                              // give more bytes
    }
    const PieceRec &end = rec[live[(size_t)m - 1]];
    int64_t consumed = end.end_bit >> 3, trailing = 0;
    int32_t end_phase = end.end_phase;
    if (end_phase == PH_DONE) {
        trailing = n - consumed;
        consumed = n;
    } else if (last && !cap_stop) {                   // no bytes follow: the stream must end between members
        if (end_phase == PH_HEADER && n - consumed < 2) {
            trailing = n - consumed;                  // (a lone byte: no header)
            consumed = n;
            end_phase = PH_DONE;
        } else if ((size_t)m < live.size() || end.status != ST_OK) {
            set_last_error(where(g->members_done, n) + "the stream ends inside a member");
            return BWAMS_ERR_IO;
        }
    }
    // ---- decode to symbols, windows, bytes
    uint8_t *d_out = out_on_device ? static_cast<uint8_t *>(out) : g->d_out.p;
    std::vector<PieceIn> dec;
    std::vector<int64_t> off((size_t)m + 1, 0);
    std::vector<Tile> tiles;
    struct Ev { int32_t tile; MemberEnd me; };        // in stream order: a tile of bytes (tile >= 0), or a member's end
    std::vector<Ev> evs;
    for (int i = 0; i < m; ++i) {
        const int k = live[(size_t)i];
        const PieceRec &r = rec[k];
        off[(size_t)i + 1] = off[(size_t)i] + r.end_out;
        if (r.end_out > 0) dec.push_back(PieceIn{pin[k].start_bit, r.end_bit, off[(size_t)i], r.end_out, pin[k].phase, 0});
        int64_t a = 0;
        auto cut = [&](int64_t b) {
            for (; a < b; a += kTile) {
                tiles.push_back(Tile{off[(size_t)i] + a, (int32_t)std::min<int64_t>(kTile, b - a), i});
                evs.push_back(Ev{(int32_t)tiles.size() - 1, {}});
            }
            a = b;
        };
        for (const MemberEnd &me : mem[(size_t)i]) {
            cut(me.out_pos);
            evs.push_back(Ev{-1, me});
        }
        cut(r.end_out);
    }
    std::vector<uint32_t> crcs(tiles.size());
    if (!dec.empty()) {
        BWAMS_HIP(hipMemcpyAsync(g->d_pin.p, dec.data(), sizeof(PieceIn) * dec.size(), hipMemcpyHostToDevice, g->st));
        hipLaunchKernelGGL(gz_decode_kernel, dim3((unsigned)dec.size()), dim3(64), 0, g->st, g->d_in.p, n, g->d_pin.p, g->d_sym.p);
        BWAMS_HIP(hipGetLastError());
    }
    BWAMS_HIP(hipEventRecord(g->ev[4], g->st));
    BWAMS_HIP(hipMemcpyAsync(g->d_off.p, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice, g->st));
    hipLaunchKernelGGL(gz_window_kernel, dim3(1), dim3(1024), 0, g->st, g->d_sym.p, g->d_off.p, m, g->d_win.p);
    BWAMS_HIP(hipGetLastError());
    BWAMS_HIP(hipEventRecord(g->ev[5], g->st));
    if (!tiles.empty()) {
        if (g->d_tile.ensure_n(tiles.size()) != hipSuccess || g->d_crc.ensure_n(tiles.size()) != hipSuccess) {
            set_last_error("bwams_gunzip_run: out of device memory for the tile list");
            return BWAMS_ERR_NOMEM;
        }
        BWAMS_HIP(hipMemcpyAsync(g->d_tile.p, tiles.data(), sizeof(Tile) * tiles.size(), hipMemcpyHostToDevice, g->st));
        hipLaunchKernelGGL(gz_resolve_kernel, dim3((unsigned)tiles.size()), dim3(256), 0, g->st, g->d_sym.p, g->d_tile.p, g->d_win.p, d_out,
                           g->d_crc.p);
        BWAMS_HIP(hipGetLastError());
        BWAMS_HIP(hipMemcpyAsync(crcs.data(), g->d_crc.p, sizeof(uint32_t) * tiles.size(), hipMemcpyDeviceToHost, g->st));
    }
    BWAMS_HIP(hipEventRecord(g->ev[6], g->st));
    BWAMS_HIP(hipStreamSynchronize(g->st));
    // ---- every member that ended: CRC32 and ISIZE
    uint32_t crc = g->crc;
    int64_t len = g->len, members = 0;
    const uint32_t x_tile = h_x8n(kTile);
    for (const Ev &e : evs) {
        if (e.tile >= 0) {
            const int32_t tn = tiles[(size_t)e.tile].n;
            crc = h_mul(tn == kTile ? x_tile : h_x8n((uint32_t)tn), crc) ^ crcs[(size_t)e.tile];
            len += tn;
            continue;
        }
        const int st = crc != e.me.crc ? ST_CRC : (uint32_t)len != e.me.isize ? ST_ISIZE : ST_OK;
        if (st) {
            set_last_error(where(g->members_done + members, e.me.trailer_byte) + status_text(st));
            return BWAMS_ERR_IO;
        }
        crc = 0;
        len = 0;
        ++members;
    }
    if (!out_on_device && o) BWAMS_HIP(hipMemcpyAsync(out, g->d_out.p, (size_t)o, hipMemcpyDeviceToHost, g->st));
    BWAMS_HIP(hipMemcpyAsync(g->d_win.p, g->d_win.p + (int64_t)m * kWin, kWin, hipMemcpyDeviceToDevice, g->st));   // the next call's window
    BWAMS_HIP(hipEventRecord(g->ev[7], g->st));
    BWAMS_HIP(hipEventSynchronize(g->ev[7]));
    if (stats) {
        stats->members = members;
        stats->pieces = m;
        stats->pieces_dropped = dropped;
        stats->recounts = recounts;
        stats->in_bytes = consumed;
        stats->out_bytes = o;
        stats->trailing_bytes = trailing;
        BWAMS_HIP(hipEventElapsedTime(&stats->ms_upload, g->ev[0], g->ev[1]));
        BWAMS_HIP(hipEventElapsedTime(&stats->ms_find, g->ev[1], g->ev[2]));
        BWAMS_HIP(hipEventElapsedTime(&stats->ms_count, g->ev[2], g->ev[3]));
        BWAMS_HIP(hipEventElapsedTime(&stats->ms_decode, g->ev[3], g->ev[4]));
        BWAMS_HIP(hipEventElapsedTime(&stats->ms_window, g->ev[4], g->ev[5]));
        BWAMS_HIP(hipEventElapsedTime(&stats->ms_resolve, g->ev[5], g->ev[6]));
        BWAMS_HIP(hipEventElapsedTime(&stats->ms_download, g->ev[6], g->ev[7]));
    }
    g->phase = end_phase;
    g->bit = end_phase == PH_DEFLATE ? (int32_t)(end.end_bit & 7) : 0;
    g->crc = crc;
    g->len = len;
    g->members_done += members;
    g->bytes_done += consumed;
    if (n_consumed) *n_consumed = consumed;
    if (n_out) *n_out = o;
    return BWAMS_OK;
}

}  // extern "C"
