// pileup.hip — per-base allele counts, candidate sites, quality sums and SNV calls (the rules are in include/bwams.h above
// bwams_pileup_open).
//
// Layout: a slot per region position, the regions' slots back to back in region order (reg_off[k] is region k's first slot); a slot is
// kPileupChannels uint32 counters (48 bytes), so slot s lives at counts + 12 * s.  ref_first[r] is the first region of reference r
// (n_ref + 1 entries), so a record looks only at its own reference's regions.
//   pileup_check_kernel   lane per record: rule 3.  The smallest index of a record with an op code above 8, of one that passes rule 2's
//                         filter with a CIGAR query length that is not l_seq, and of one whose SEQ or QUAL ends behind the record.
//   pileup_route_kernel   lane per record: rule 2's filter, then the slots the record can reach, from its reference span
//                         [POS, POS + reference length) (and POS - 1, the anchor of an insertion behind reference ops of length 0).
//                         A record whose slots lie in one or two tiles of kPileupTile positions gets a (tile, record) entry per tile
//                         at 2r and 2r + 1 (unused entries carry the key n_tiles and sort to the end); one that touches more tiles,
//                         or every record under BWAMS_PILEUP_TILED=0, is routed to the direct kernel.  No atomics but the three
//                         route counters, added once per wave.
//   pileup_heads_kernel   after the entries are sorted by tile (rocprim::radix_sort_pairs over the bits n_tiles needs): the index of
//                         the first entry of every occupied tile, appended to a list.
//   pileup_tile_kernel    a workgroup per occupied tile: the tile's 12 channels x kPileupTile counters are zeroed in LDS (48 KB, so three
//                         fit a CU's 160 KB; two are resident, being 16 waves each at 8 waves a SIMD), its waves take the tile's records in turn, the lanes of a wave the
//                         record's query bases in rounds of 64 and then its CIGAR ops in rounds of 64 (walk_record), adding with LDS
//                         atomics; positions of the record in another tile are left to that tile's workgroup.  The LDS array is
//                         channel-major, so the lanes of a round, which hold neighbouring positions, hit neighbouring banks.  At the
//                         end a thread per position adds the position's 12 counters to HBM with three 16-byte loads and stores when
//                         one of them is not zero: a tile has one owner per launch, so no global atomic is issued.
//   pileup_direct_kernel  a wave per record routed direct: the same walk with one global atomic per counted base.
//   pileup_tile_quality_kernel, pileup_direct_quality_kernel
//                         the same two for a handle with a quality plane (rules 10 and 11): a second plane of 12 uint32 per slot,
//                         Q[A..T] HOM[A..T] HET[A..T], and a counted base adds four values, its count and the three sums of its
//                         effective quality.  The tile holds both planes, 96 KB of dynamic LDS, so one workgroup is resident on a
//                         CU; the flush writes the second plane as it writes the first.  The count-only kernels are instantiated
//                         from the same walk with sinks that ignore the quality, and compile to what they were without it.
//   pileup_call_kernel    rule 13: PileupCallTest (common.h) gives the genotype costs of a slot from the two planes in 64-bit
//                         integers; api_pileup.hip counts and selects the calls with it as it does the sites, and this kernel
//                         fills the call records of the selected slots.
//   pileup_site_*         rule 8's predicate over the slots (SiteTest, given to rocprim::reduce and rocprim::select by
//                         api_pileup.hip) and the gather that fills the site records of the selected slots.
//   The indel store of rules 14 to 17 is pileup_indel.hip; pileup_dev.h holds what the two files share.
//   pileup_ref_kernel     rule 7: a lane per slot copies the forward strand's .0123 code at contig offset + position; a position in one
//                         of the .amb holes reads 4 (ref_code_at, ref_gather.h).
#include <algorithm>
#include "common.h"
#include "bam_rec.h"
#include "pileup_dev.h"
#include "ref_gather.h"
#include "wave_ops.h"

namespace bwams {
namespace {

__global__ void __launch_bounds__(256) pileup_check_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, PileupFilter f,
                                                           unsigned long long *bad) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t *p = bam + rec_off[r];
        const uint32_t n_cig = bam_n_cig(p);
        const uint8_t *c = p + bam_cigar_at(bam_l_name(p));
        bool any = false;
        int64_t qlen = 0;
        for (uint32_t k = 0; k < n_cig; ++k) {
            const uint32_t op = ld_u32(c + 4 * k), o = op & 15;
            any |= o > 8;
            if (op_takes_query(o)) qlen += op >> 4;
        }
        if (any) { atomicMin(bad, (unsigned long long)r); continue; }
        if (!record_counts(p, f)) continue;
        const int64_t l_seq = bam_l_seq(p);
        if (qlen != l_seq) atomicMin(bad + 1, (unsigned long long)r);
        else if (bam_aux_at(bam_l_name(p), n_cig, l_seq) > bam_end(p)) atomicMin(bad + 2, (unsigned long long)r);
    }
}

// A region held in registers: the usual record lies in one region, and its lanes then ask memory nothing to place a base.
struct RegionCursor {
    int32_t ri, beg, end;                  // region ri is [beg, end) ...
    int64_t off;                           // ... from slot off
};
__device__ __forceinline__ RegionCursor cursor_at(const PileupRegions &R, int32_t ri, int32_t r_end) {
    RegionCursor c{ri, 0, 0, 0};
    if (ri < r_end) { c.beg = R.beg[ri]; c.end = R.end[ri]; c.off = R.off[ri]; }
    return c;
}

// The slot of position x of the reference whose regions are [c.ri, r_end), or -1; the cursor only moves forward, so a caller asks for
// positions in ascending order.
__device__ __forceinline__ int64_t slot_at(const PileupRegions &R, RegionCursor &c, int32_t r_end, int64_t x) {
    while (c.ri < r_end && (int64_t)c.end <= x) c = cursor_at(R, c.ri + 1, r_end);
    if (c.ri < r_end && (int64_t)c.beg <= x) return c.off + (x - c.beg);
    return -1;
}

// What a wave needs of one record that passed rule 2's filter and rule 3's check.
struct RecView {
    const uint8_t *cig, *seq, *qual;
    uint32_t n_cig;
    int32_t l_seq, r_end;
    RegionCursor first;                    // the regions [first.ri, r_end) of its reference end above POS - 1
    int64_t pos;
    int strand;                            // 0, or 4 for FLAG 0x10
    int mapq;                              // rule 10; only a quality sink reads it
    bool has_qual;
};

__device__ __forceinline__ RecView view_of(const uint8_t *p, const PileupRegions &R) {
    RecView v;
    const uint32_t l_name = bam_l_name(p);
    v.n_cig = bam_n_cig(p);
    v.l_seq = bam_l_seq(p);
    v.cig = p + bam_cigar_at(l_name);
    v.seq = p + bam_seq_at(l_name, v.n_cig);
    v.qual = p + bam_qual_at(l_name, v.n_cig, v.l_seq);
    v.pos = bam_pos(p);
    v.strand = (bam_flag(p) & 0x10) ? 4 : 0;
    v.mapq = bam_mapq(p);
    v.has_qual = v.qual[0] != 0xFF;
    const int32_t rid = bam_ref_id(p);
    v.r_end = R.ref_first[rid + 1];
    v.first = cursor_at(R, first_region_ending_above(R, R.ref_first[rid], v.r_end, v.pos - 1), v.r_end);
    return v;
}

// inclusive prefix sum over the 64 lanes
__device__ __forceinline__ int64_t wave_scan(int64_t v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t u = __shfl_up((long long)v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// One round of the lane-per-op walk: lane's op k0 + lane (code 15 beyond the CIGAR), the reference position x of its start from a wave
// prefix sum over the ops before it, and whether a reference op precedes it; the carries go on to the next round.
struct OpRound {
    uint32_t o;
    int64_t len, x;
    bool seen;
};
__device__ __forceinline__ OpRound op_round(const RecView &v, uint32_t k0, int lane, int64_t &x_carry, bool &seen_carry) {
    OpRound r{15, 0, 0, false};
    const uint32_t kk = k0 + lane;
    if (kk < v.n_cig) {
        const uint32_t w = ld_u32(v.cig + 4 * kk);
        r.o = w & 15;
        r.len = w >> 4;
    }
    const bool tr = op_takes_ref(r.o);
    const int64_t incl = wave_scan(tr ? r.len : 0, lane);
    r.x = x_carry + incl - (tr ? r.len : 0);
    const uint64_t refs = __ballot(tr);
    r.seen = seen_carry || (refs & ((1ULL << lane) - 1)) != 0;
    x_carry += shfl64(incl, 63);
    seen_carry |= refs != 0;
    return r;
}

// Rule 4 for one record by one wave: sink.add(slot, channel, qe) for everything the record counts; qe is rule 10's effective quality of
// a base in one of the eight base channels, worked out only for a sink with kQuality (0 otherwise).  First the query bases, a lane per
// base in rounds of 64: a lane keeps the op that holds its base and the query and reference offsets of that op's start, and moves
// them forward from round to round (its bases ascend).  Then the CIGAR ops, a lane per op in rounds of 64 (op_round): an I is counted
// by its lane; when the record has a D, a second pass over the ops counts the positions of each D by the whole wave.
template <class Sink> __device__ __forceinline__ void walk_record(const PileupRegions &R, const RecView &v, int min_baseq, int lane, Sink &sink) {
    uint32_t k = 0, op = v.n_cig ? ld_u32(v.cig) : 0;
    int64_t q0 = 0, x0 = v.pos;
    RegionCursor c = v.first;
    for (int64_t q = lane; q < v.l_seq; q += 64) {
        const uint32_t qual = v.qual[q], two = v.seq[q >> 1];            // both loads leave before anything branches on either
        while (k < v.n_cig) {
            const uint32_t o = op & 15;
            const int64_t len = op >> 4;
            const bool tq = op_takes_query(o);
            if (tq && q < q0 + len) break;
            if (tq) q0 += len;
            if (op_takes_ref(o)) x0 += len;
            if (++k < v.n_cig) op = ld_u32(v.cig + 4 * k);
        }
        if (k >= v.n_cig) break;                                         // not reached: rule 3 made the query length l_seq
        if (!op_is_match(op & 15)) continue;
        if (v.has_qual && (int)qual < min_baseq) continue;
        const int64_t s = slot_at(R, c, v.r_end, x0 + (q - q0));
        if (s < 0) continue;
        const uint32_t code = (two >> ((q & 1) ? 0 : 4)) & 15;
        const int base = code == 1 ? 0 : code == 2 ? 1 : code == 4 ? 2 : code == 8 ? 3 : -1;
        int qe = 0;
        if constexpr (Sink::kQuality)
            qe = std::min(std::max(std::min(v.has_qual ? (int)qual : sink.no_qual_q, v.mapq), kPileupGlMinQ), kPileupGlMaxQ);
        sink.add(s, base < 0 ? kPileupN : base + v.strand, qe);
    }
    int64_t x_carry = v.pos;
    bool seen_carry = false, any_del = false;
    c = v.first;
    for (uint32_t k0 = 0; k0 < v.n_cig; k0 += 64) {                      // the I ops, each by its lane
        const OpRound r = op_round(v, k0, lane, x_carry, seen_carry);
        if (r.o == 1 && r.seen) {
            const int64_t s = slot_at(R, c, v.r_end, r.x - 1);
            if (s >= 0) sink.add(s, kPileupIns, 0);
        }
        any_del |= __ballot(r.o == 2) != 0;
    }
    if (!any_del) return;
    // The D ops in a pass of their own (few records have one, and its registers stay out of the passes above): a D at a time, its
    // region positions spread over the lanes, so a long deletion costs the wave len / 64 steps and not one lane len.
    x_carry = v.pos;
    seen_carry = false;
    int32_t d_ri = v.first.ri;                                           // wave-uniform: a record's deletions ascend
    for (uint32_t k0 = 0; k0 < v.n_cig; k0 += 64) {
        const OpRound r = op_round(v, k0, lane, x_carry, seen_carry);
        for (uint64_t dels = __ballot(r.o == 2); dels; dels &= dels - 1) {
            const int src = __ffsll((unsigned long long)dels) - 1;
            const int64_t dx = shfl64(r.x, src), d_end = dx + shfl64(r.len, src);
            while (d_ri < v.r_end && (int64_t)R.end[d_ri] <= dx) ++d_ri;
            for (int32_t rj = d_ri; rj < v.r_end && (int64_t)R.beg[rj] < d_end; ++rj) {
                const int64_t lo = std::max<int64_t>(dx, R.beg[rj]), hi = std::min<int64_t>(d_end, R.end[rj]);
                for (int64_t y = lo + lane; y < hi; y += 64) sink.add(R.off[rj] + (y - R.beg[rj]), kPileupDel, 0);
            }
        }
    }
}

// The slots [*lo, *hi] a record can reach; false when there is none.  Its positions are [POS, POS + reference length), and POS - 1
// when an I stands behind reference ops that are all of length 0 (rule 4 counts it at the position before).
__device__ __forceinline__ bool reach_of(const uint8_t *p, const PileupRegions &R, int64_t *lo, int64_t *hi) {
    const int32_t rid = bam_ref_id(p);
    const uint32_t n_cig = bam_n_cig(p);
    const uint8_t *c = p + bam_cigar_at(bam_l_name(p));
    int64_t rlen = 0;
    bool seen = false, before = false;
    for (uint32_t k = 0; k < n_cig; ++k) {
        const uint32_t op = ld_u32(c + 4 * k), o = op & 15;
        before |= o == 1 && seen && rlen == 0;
        if (op_takes_ref(o)) { rlen += op >> 4; seen = true; }
    }
    const int64_t a = (int64_t)bam_pos(p) - (before ? 1 : 0);
    const int64_t b = (int64_t)bam_pos(p) + rlen - 1;                                      // the last position
    if (b < a) return false;
    const int32_t first = R.ref_first[rid], last = R.ref_first[rid + 1];
    const int32_t r_lo = first_region_ending_above(R, first, last, a);                     // holds a or lies behind it
    int32_t r_hi = first_region_ending_above(R, first, last, b);                           // holds b or lies behind it ...
    if (r_hi == last || (int64_t)R.beg[r_hi] > b) --r_hi;                                  // ... the last that begins at or before b
    if (r_lo == last || r_hi < r_lo) return false;
    *lo = R.off[r_lo] + (std::max<int64_t>(a, R.beg[r_lo]) - R.beg[r_lo]);
    *hi = R.off[r_hi] + (std::min<int64_t>(b, (int64_t)R.end[r_hi] - 1) - R.beg[r_hi]);
    return *hi >= *lo;
}

__global__ void __launch_bounds__(256) pileup_route_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, PileupFilter f,
                                                           PileupRegions R, uint32_t n_tiles, int tiled, uint32_t *keys, uint32_t *vals,
                                                           uint8_t *route, unsigned long long *counts) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t rounded = (n_rec + 63) & ~(int64_t)63;                 // whole waves enter every round: the ballots need them
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rounded; r += stride) {
        bool counted = false;
        int n_ent = 0;
        uint32_t k0 = n_tiles, k1 = n_tiles;
        uint8_t way = kPileupSkip;
        if (r < n_rec) {
            const uint8_t *p = bam + rec_off[r];
            counted = record_counts(p, f);
            int64_t lo = 0, hi = 0;
            if (counted && reach_of(p, R, &lo, &hi)) {
                const int64_t t0 = lo / kPileupTile, t1 = hi / kPileupTile;
                if (!tiled || t1 - t0 > 1) {
                    way = kPileupDirect;
                } else {
                    way = kPileupTiled;
                    k0 = (uint32_t)t0;
                    n_ent = 1;
                    if (t1 != t0) { k1 = (uint32_t)t1; n_ent = 2; }
                }
            }
            route[r] = way;
            if (tiled) {
                keys[2 * r] = k0; keys[2 * r + 1] = k1;
                vals[2 * r] = (uint32_t)r; vals[2 * r + 1] = (uint32_t)r;
            }
        }
        const uint64_t m_counted = __ballot(counted), m_direct = __ballot(way == kPileupDirect);
        const int64_t ents = wave_sum(n_ent);
        if (lane == 0) {
            if (m_counted) atomicAdd(counts, (unsigned long long)__popcll((unsigned long long)m_counted));
            if (ents) atomicAdd(counts + 1, (unsigned long long)ents);
            if (m_direct) atomicAdd(counts + 2, (unsigned long long)__popcll((unsigned long long)m_direct));
        }
    }
}

__global__ void __launch_bounds__(256) pileup_heads_kernel(const uint32_t *keys, int64_t n, uint32_t n_tiles, uint32_t *heads,
                                                           uint32_t *n_heads) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t key = keys[i];
        if (key < n_tiles && (i == 0 || keys[i - 1] != key)) heads[atomicAdd(n_heads, 1u)] = (uint32_t)i;
    }
}

constexpr int kTileThreads = 1024;                                      // 16 waves a tile; two tiles a CU while the kernel stays at or under 64 VGPRs (make resource-usage)

struct TileSink {                                                        // the workgroup's tile in LDS, channel-major
    static constexpr bool kQuality = false;
    uint32_t *lds;
    int64_t first;                                                       // the tile's first slot
    __device__ __forceinline__ void add(int64_t slot, int channel, int) {
        const uint64_t at = (uint64_t)(slot - first);
        if (at < (uint64_t)kPileupTile) atomicAdd(lds + channel * kPileupTile + (int)at, 1u);
    }
};

struct DirectSink {
    static constexpr bool kQuality = false;
    uint32_t *counts;
    __device__ __forceinline__ void add(int64_t slot, int channel, int) { atomicAdd(counts + slot * kPileupChannels + channel, 1u); }
};

// The quality-on sinks (rule 11): a counted base adds four values, its count and Q, HOM and HET of its base, both strands together.
struct TileQualitySink {                                                 // both planes of the tile in LDS: the counters' 12 channels, then the sums' 12
    static constexpr bool kQuality = true;
    uint32_t *lds;
    int64_t first;
    int no_qual_q;
    __device__ __forceinline__ void add(int64_t slot, int channel, int qe) {
        const uint64_t at = (uint64_t)(slot - first);
        if (at >= (uint64_t)kPileupTile) return;
        atomicAdd(lds + channel * kPileupTile + (int)at, 1u);
        if (channel >= 8) return;
        uint32_t *q = lds + (kPileupChannels + (channel & 3)) * kPileupTile + (int)at;
        atomicAdd(q + BWAMS_PILEUP_Q * kPileupTile, (uint32_t)qe);
        atomicAdd(q + BWAMS_PILEUP_HOM * kPileupTile, pileup_gl_hom(qe));
        atomicAdd(q + BWAMS_PILEUP_HET * kPileupTile, pileup_gl_het(qe));
    }
};

struct DirectQualitySink {
    static constexpr bool kQuality = true;
    uint32_t *counts, *sums;
    int no_qual_q;
    __device__ __forceinline__ void add(int64_t slot, int channel, int qe) {
        atomicAdd(counts + slot * kPileupChannels + channel, 1u);
        if (channel >= 8) return;
        uint32_t *q = sums + slot * kPileupChannels + (channel & 3);
        atomicAdd(q + BWAMS_PILEUP_Q, (uint32_t)qe);
        atomicAdd(q + BWAMS_PILEUP_HOM, pileup_gl_hom(qe));
        atomicAdd(q + BWAMS_PILEUP_HET, pileup_gl_het(qe));
    }
};

// the slot's 12 values of one plane of the tile (lds: the plane's first channel) added to HBM at g, when one of them is not zero
__device__ __forceinline__ void flush_slot(const uint32_t *lds, int i, uint32_t *g_slot) {
    uint32_t c[kPileupChannels];
    uint32_t any = 0;
    for (int ch = 0; ch < kPileupChannels; ++ch) { c[ch] = lds[ch * kPileupTile + i]; any |= c[ch]; }
    if (!any) return;
    uint4 *g = reinterpret_cast<uint4 *>(g_slot);
    for (int j = 0; j < kPileupChannels / 4; ++j) {
        uint4 x = g[j];
        x.x += c[4 * j]; x.y += c[4 * j + 1]; x.z += c[4 * j + 2]; x.w += c[4 * j + 3];
        g[j] = x;
    }
}

// A workgroup's tile: the planes of the sink (one, or the counters and the sums) zeroed in LDS, the tile's records walked, the planes
// added to HBM.  sums: the quality plane in HBM, read only by a sink with kQuality.
template <class Sink> __device__ __forceinline__ void tile_body(uint32_t *lds, Sink &sink, const uint8_t *bam, const int64_t *rec_off,
                                                                const PileupRegions &R, int min_baseq, const uint32_t *keys,
                                                                const uint32_t *vals, int64_t n_ent, int64_t head, uint32_t tile,
                                                                int64_t n_slots, uint32_t *counts, uint32_t *sums) {
    constexpr int kWords = (Sink::kQuality ? 2 : 1) * kPileupChannels * kPileupTile;
    for (int i = threadIdx.x; i < kWords; i += blockDim.x) lds[i] = 0;
    __syncthreads();
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), n_waves = (int)(blockDim.x >> 6);
    for (int64_t e = head + wave; e < n_ent && keys[e] == tile; e += n_waves) {
        const RecView v = view_of(bam + rec_off[vals[e]], R);
        walk_record(R, v, min_baseq, lane, sink);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kPileupTile; i += blockDim.x) {
        const int64_t slot = sink.first + i;
        if (slot >= n_slots) break;
        flush_slot(lds, i, counts + slot * kPileupChannels);
        if constexpr (Sink::kQuality) flush_slot(lds + kPileupChannels * kPileupTile, i, sums + slot * kPileupChannels);
    }
}

__global__ void __launch_bounds__(kTileThreads) pileup_tile_kernel(const uint8_t *bam, const int64_t *rec_off, PileupRegions R, int min_baseq,
                                                          const uint32_t *keys, const uint32_t *vals, int64_t n_ent, const uint32_t *heads,
                                                          const uint32_t *n_heads, int64_t n_slots, uint32_t *counts) {
    __shared__ uint32_t lds[kPileupChannels * kPileupTile];
    if (blockIdx.x >= *n_heads) return;
    const int64_t head = heads[blockIdx.x];
    const uint32_t tile = keys[head];
    TileSink sink{lds, (int64_t)tile * kPileupTile};
    tile_body(lds, sink, bam, rec_off, R, min_baseq, keys, vals, n_ent, head, tile, n_slots, counts, nullptr);
}

// The tile with both planes: 2 x 12 channels x kPileupTile x 4 bytes = 96 KB, above the 64 KB a kernel may declare, so the LDS is
// dynamic and the launch raises the kernel's maximum; one workgroup fits a CU.
constexpr int kTileQualityLds = 2 * kPileupChannels * kPileupTile * 4;
__global__ void __launch_bounds__(kTileThreads) pileup_tile_quality_kernel(const uint8_t *bam, const int64_t *rec_off, PileupRegions R,
                                                                  int min_baseq, const uint32_t *keys, const uint32_t *vals, int64_t n_ent,
                                                                  const uint32_t *heads, const uint32_t *n_heads, int64_t n_slots,
                                                                  uint32_t *counts, PileupQuality quality) {
    extern __shared__ __align__(16) uint32_t lds_both[];
    if (blockIdx.x >= *n_heads) return;
    const int64_t head = heads[blockIdx.x];
    const uint32_t tile = keys[head];
    TileQualitySink sink{lds_both, (int64_t)tile * kPileupTile, quality.no_qual_q};
    tile_body(lds_both, sink, bam, rec_off, R, min_baseq, keys, vals, n_ent, head, tile, n_slots, counts, quality.sums);
}

__global__ void __launch_bounds__(256) pileup_direct_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, PileupRegions R,
                                                            int min_baseq, const uint8_t *route, uint32_t *counts) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    DirectSink sink{counts};
    for (int64_t r = wave; r < n_rec; r += n_waves) {
        if (route[r] != kPileupDirect) continue;
        const RecView v = view_of(bam + rec_off[r], R);
        walk_record(R, v, min_baseq, lane, sink);
    }
}

__global__ void __launch_bounds__(256) pileup_direct_quality_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, PileupRegions R,
                                                                    int min_baseq, const uint8_t *route, uint32_t *counts,
                                                                    PileupQuality quality) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    DirectQualitySink sink{counts, quality.sums, quality.no_qual_q};
    for (int64_t r = wave; r < n_rec; r += n_waves) {
        if (route[r] != kPileupDirect) continue;
        const RecView v = view_of(bam + rec_off[r], R);
        walk_record(R, v, min_baseq, lane, sink);
    }
}

__global__ void __launch_bounds__(256) pileup_call_kernel(PileupCallTest test, PileupRegions R, int32_t n_regions, const int64_t *slots,
                                                          int64_t n, bwams_pileup_call_t *out) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = slots[k];
        bwams_pileup_call_t x;
        test.genotype(s, &x);
        x.region = region_of_slot(R, n_regions, s);
        x.pos = (int32_t)(R.beg[x.region] + (s - R.off[x.region]));
        out[k] = x;
    }
}

__global__ void __launch_bounds__(256) pileup_site_kernel(PileupSiteTest test, PileupRegions R, int32_t n_regions, const int64_t *slots,
                                                          int64_t n, bwams_pileup_site_t *out) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = slots[k];
        const int32_t lo = region_of_slot(R, n_regions, s);
        bwams_pileup_site_t x;
        x.region = lo;
        x.pos = (int32_t)(R.beg[lo] + (s - R.off[lo]));
        x.ref = test.ref[s];
        x.kinds = test.kinds(s, &x.depth);
        for (int ch = 0; ch < kPileupChannels; ++ch) x.c[ch] = test.counts[s * kPileupChannels + ch];
        out[k] = x;
    }
}

__global__ void __launch_bounds__(256) pileup_ref_kernel(PileupRegions R, int32_t n_regions, const int32_t *reg_ref, int64_t n_slots,
                                                         const uint8_t *ref0123, const bwams_contig_t *contigs, const int64_t *hole_off,
                                                         const int32_t *hole_len, int32_t n_holes, uint8_t *out) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n_slots; s += (int64_t)gridDim.x * blockDim.x) {
        const int32_t lo = region_of_slot(R, n_regions, s);
        out[s] = ref_code_at(ref0123, contigs[reg_ref[lo]].offset + R.beg[lo] + (s - R.off[lo]), hole_off, hole_len, n_holes);
    }
}

}  // namespace

void launch_pileup_check(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const PileupFilter &f, unsigned long long *bad,
                         int cu_count, hipStream_t st) {
    if (n_rec > 0) pileup_check_kernel<<<grid_of(n_rec, 256, cu_count), 256, 0, st>>>(bam, rec_off, n_rec, f, bad);
}

void launch_pileup_route(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const PileupFilter &f, const PileupRegions &R,
                         uint32_t n_tiles, int tiled, uint32_t *keys, uint32_t *vals, uint8_t *route, unsigned long long *counts,
                         int cu_count, hipStream_t st) {
    if (n_rec > 0)
        pileup_route_kernel<<<grid_of(n_rec, 256, cu_count), 256, 0, st>>>(bam, rec_off, n_rec, f, R, n_tiles, tiled, keys, vals, route, counts);
}

int launch_pileup_tiles(const uint8_t *bam, const int64_t *rec_off, const PileupRegions &R, int min_baseq, const uint32_t *keys,
                        const uint32_t *vals, int64_t n_ent, uint32_t n_tiles, uint32_t *heads, uint32_t *n_heads, int64_t n_slots,
                        uint32_t *counts, const PileupQuality &quality, int cu_count, hipStream_t st) {
    if (n_ent <= 0) return 0;
    // the opt-in for more than 64 KB of dynamic LDS belongs to the current device: set per launch, and checked, before anything is queued
    if (quality.sums && hipFuncSetAttribute(reinterpret_cast<const void *>(pileup_tile_quality_kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, kTileQualityLds) != hipSuccess) return -1;
    pileup_heads_kernel<<<grid_of(n_ent, 256, cu_count), 256, 0, st>>>(keys, n_ent, n_tiles, heads, n_heads);
    const unsigned grid = (unsigned)std::min<int64_t>(n_ent, n_tiles);   // no more tiles can be occupied; the blocks beyond *n_heads leave at once
    if (quality.sums)
        pileup_tile_quality_kernel<<<grid, kTileThreads, kTileQualityLds, st>>>(bam, rec_off, R, min_baseq, keys, vals, n_ent, heads, n_heads,
                                                                               n_slots, counts, quality);
    else
        pileup_tile_kernel<<<grid, kTileThreads, 0, st>>>(bam, rec_off, R, min_baseq, keys, vals, n_ent, heads, n_heads, n_slots, counts);
    return 0;
}

void launch_pileup_direct(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const PileupRegions &R, int min_baseq,
                          const uint8_t *route, uint32_t *counts, const PileupQuality &quality, int cu_count, hipStream_t st) {
    if (n_rec <= 0) return;
    if (quality.sums)
        pileup_direct_quality_kernel<<<grid_of(n_rec, 4, cu_count), 256, 0, st>>>(bam, rec_off, n_rec, R, min_baseq, route, counts, quality);
    else
        pileup_direct_kernel<<<grid_of(n_rec, 4, cu_count), 256, 0, st>>>(bam, rec_off, n_rec, R, min_baseq, route, counts);
}

void launch_pileup_calls(const PileupCallTest &test, const PileupRegions &R, int32_t n_regions, const int64_t *slots, int64_t n,
                         bwams_pileup_call_t *out, int cu_count, hipStream_t st) {
    if (n > 0) pileup_call_kernel<<<grid_of(n, 256, cu_count), 256, 0, st>>>(test, R, n_regions, slots, n, out);
}

void launch_pileup_sites(const PileupSiteTest &test, const PileupRegions &R, int32_t n_regions, const int64_t *slots, int64_t n,
                         bwams_pileup_site_t *out, int cu_count, hipStream_t st) {
    if (n > 0) pileup_site_kernel<<<grid_of(n, 256, cu_count), 256, 0, st>>>(test, R, n_regions, slots, n, out);
}

void launch_pileup_ref(const PileupRegions &R, int32_t n_regions, const int32_t *reg_ref, int64_t n_slots, const uint8_t *ref0123,
                       const bwams_contig_t *contigs, const int64_t *hole_off, const int32_t *hole_len, int32_t n_holes, uint8_t *out,
                       int cu_count, hipStream_t st) {
    if (n_slots > 0)
        pileup_ref_kernel<<<grid_of(n_slots, 256, cu_count), 256, 0, st>>>(R, n_regions, reg_ref, n_slots, ref0123, contigs, hole_off, hole_len,
                                                                          n_holes, out);
}

}  // namespace bwams
