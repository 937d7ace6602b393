// pileup_indel.hip — the indel store of a pileup handle: events, span sums, allele and call records (rules 14 to 17 in include/bwams.h
// above bwams_pileup_open).  It runs beside pileup.hip's route, tile and direct kernels and touches none of their counters.
//   pileup_indel_kernel<false>  the count pass, a lane per record that rule 2 counts: the lane walks the record's CIGAR OPS (not its
//                         bases, so a record costs its n_cigar_op whatever its length, and any number of ops) and counts the I and D ops
//                         that give an event inside a region slot.  One atomic per wave adds the wave's sum to the call's count; the host
//                         sizes the event buffer from it before any counter of the call moves.
//   pileup_indel_kernel<true>   the event pass: the same walk twice.  The first gives the lane's count; a wave prefix sum and ONE atomic
//                         per wave reserve the wave's place in the buffer; the second writes each event's 16-byte key (k0 = slot << 8 |
//                         type << 6 | len, seq) and its qe.  The second walk also closes every maximal run of M/=/X ops and adds rule
//                         15's four values to the difference array at the run's first spanned slot of a region and subtracts them one
//                         past its last: eight global atomics per run and region.  The subtraction may land on the next region's first
//                         slot or on entry n_slots; both are what a difference array wants.
//   pileup_indel_run_kernel     the event pass of a left-aligning handle (rule 18): the same, and per event one transient word, how far
//                         below the anchor the run of match ops that ends there spans (0 behind any other op).
//   pileup_indel_align_kernel   rule 18 over the events an add appended: the shift against the handle's reference bases, the key rewritten
//                         in place, and eight atomics that take the record's span back between the new anchor and the old one.  The
//                         two kernels above are not touched by it: a handle without the option launches exactly what it launched.
//   pileup_indel_allele_kernel  a lane per group of the sorted, reduced events: the allele record.
//   pileup_indel_call_kernel    a lane per selected first group of a slot: PileupIndelTest (common.h) picks ALT and works rule 16 out in
//                         64-bit integers; the kernel adds region, pos and, for a deletion, the reference codes behind the anchor.
// api_pileup.hip sorts the events with rocprim::merge_sort, reduces them with rocprim::reduce_by_key, scans the difference array with
// rocprim::inclusive_scan and selects the calls with rocprim::reduce and rocprim::select, as it selects the sites and the SNV calls.
#include <algorithm>
#include "common.h"
#include "bam_rec.h"
#include "pileup_dev.h"
#include "wave_ops.h"

namespace bwams {
namespace {

// rule 15 for one run of match ops over positions [a, b): slot s is spanned when s and s + 1 are both in the run
__device__ __forceinline__ void span_run(const PileupRegions &R, int32_t r_first, int32_t r_end, int64_t a, int64_t b, const uint32_t (&v)[4],
                                         uint32_t *diff) {
    const int64_t last = b - 1;                                          // the spanned positions are [a, last)
    if (last <= a) return;
    for (int32_t ri = first_region_ending_above(R, r_first, r_end, a); ri < r_end && (int64_t)R.beg[ri] < last; ++ri) {
        const int64_t beg = R.beg[ri], lo = std::max<int64_t>(a, beg), hi = std::min<int64_t>(last, R.end[ri]);
        if (lo >= hi) continue;
        uint32_t *d0 = diff + 4 * (R.off[ri] + (lo - beg)), *d1 = diff + 4 * (R.off[ri] + (hi - beg));     // hi - beg <= the region's length: entry n_slots at most
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            atomicAdd(d0 + j, v[j]);
            atomicAdd(d1 + j, 0u - v[j]);
        }
    }
}

// One record by one lane.  kWrite == false: the number of its events (rule 14) whose anchor has a slot.  kWrite == true: the same,
// and the events written to S.keys / S.qe from index `at` on, and rule 15's runs added to S.diff.
// kRun (the event pass of a left-aligning handle): run[at + i - first] too, the number of slots below event i's anchor that the run of
// match ops ending at the anchor spans, 0 when the op before the event's is no match op: what rule 18 may clip.
template <bool kWrite, bool kRun = false>
__device__ __forceinline__ int walk_ops(const uint8_t *p, const PileupRegions &R, const PileupIndelStore &S, int64_t at, uint32_t *run = nullptr,
                                        int64_t first = 0) {
    const uint32_t l_name = bam_l_name(p), n_cig = bam_n_cig(p);
    const uint8_t *cig = p + bam_cigar_at(l_name), *seq = p + bam_seq_at(l_name, n_cig);
    const int32_t rid = bam_ref_id(p), r_first = R.ref_first[rid], r_end = R.ref_first[rid + 1];
    const int qe = std::min(std::max(std::min((int)bam_mapq(p), S.indel_q), kPileupGlMinQ), kPileupGlMaxQ);
    const uint32_t v[4] = {1u, (uint32_t)qe, pileup_gl_hom(qe), pileup_gl_het(qe)};
    int64_t x = bam_pos(p), q = 0, run_a = 0;
    bool seen = false, in_run = false;
    int n_ev = 0;
    for (uint32_t k = 0; k < n_cig; ++k) {
        const uint32_t w = ld_u32(cig + 4 * k), o = w & 15;
        const int64_t len = w >> 4;
        if ((o == 1 || o == 2) && seen) {
            const int64_t a = x - 1;                                     // the anchor
            const int32_t ri = first_region_ending_above(R, r_first, r_end, a);
            if (ri < r_end && (int64_t)R.beg[ri] <= a) {
                if constexpr (kWrite) {
                    uint64_t type = o == 1 ? BWAMS_PILEUP_EV_INS : BWAMS_PILEUP_EV_DEL, bits = 0;
                    if (len > S.max_len) type = BWAMS_PILEUP_EV_OTHER;
                    else if (o == 2) { if (x + len - 1 >= (int64_t)R.end[ri]) type = BWAMS_PILEUP_EV_OTHER; }
                    else
                        for (int64_t j = 0; j < len; ++j) {
                            const int base = base_of_code(seq_code(seq, (int32_t)(q + j)));
                            if (base < 0) { type = BWAMS_PILEUP_EV_OTHER; break; }
                            bits |= (uint64_t)base << (2 * j);
                        }
                    const bool other = type == BWAMS_PILEUP_EV_OTHER;
                    const uint64_t slot = (uint64_t)(R.off[ri] + (a - R.beg[ri]));
                    if (at + n_ev < S.cap) {                             // the count pass sized the buffer: never false
                        S.keys[at + n_ev] = PileupEvKey{slot << 8 | type << 6 | (other ? 0 : (uint64_t)len), other ? 0 : bits};
                        S.qe[at + n_ev] = (uint32_t)qe;
                        if constexpr (kRun)                              // run holds S.cap - first words, and the add's events begin at first
                            if (at + n_ev >= first) run[at + n_ev - first] = in_run ? (uint32_t)std::min<int64_t>(std::max<int64_t>(a - run_a, 0), 0x7FFFFFFF) : 0u;
                    }
                }
                ++n_ev;
            }
        }
        if constexpr (kWrite) {
            if (op_is_match(o)) {
                if (!in_run) { in_run = true; run_a = x; }
            } else if (in_run) {
                in_run = false;
                span_run(R, r_first, r_end, run_a, x, v, S.diff);
            }
        }
        if (op_takes_ref(o)) { x += len; seen = true; }
        if (op_takes_query(o)) q += len;
    }
    if constexpr (kWrite)
        if (in_run) span_run(R, r_first, r_end, run_a, x, v, S.diff);
    return n_ev;
}

template <bool kEmit>
__global__ void __launch_bounds__(256) pileup_indel_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, PileupFilter f,
                                                           PileupRegions R, PileupIndelStore S) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t rounded = (n_rec + 63) & ~(int64_t)63;                 // whole waves enter every round: the shuffles need them
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rounded; r += stride) {
        const uint8_t *p = r < n_rec ? bam + rec_off[r] : nullptr;
        const bool counted = p && record_counts(p, f);
        const int n_ev = counted ? walk_ops<false>(p, R, S, 0) : 0;
        int64_t incl = n_ev;                                             // inclusive prefix sum over the wave
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t u = shfl64(incl, lane >= d ? lane - d : lane);
            if (lane >= d) incl += u;
        }
        const int64_t total = shfl64(incl, 63);
        int64_t base = 0;
        if (lane == 0 && total) base = (int64_t)atomicAdd(S.n_events, (unsigned long long)total);       // one atomic per wave
        if constexpr (kEmit) {
            base = shfl64(base, 0);
            if (counted) walk_ops<true>(p, R, S, base + incl - n_ev);
        }
    }
}

// The event pass of a left-aligning handle: pileup_indel_kernel<true> with run[] for the align kernel.  It is a kernel of its own and
// not a third instantiation through a shared body, because routing the two kernels above through one moved their registers, and a
// handle without the option must run the code it ran.
__global__ void __launch_bounds__(256) pileup_indel_run_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, PileupFilter f,
                                                               PileupRegions R, PileupIndelStore S, uint32_t *run, int64_t first) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t rounded = (n_rec + 63) & ~(int64_t)63;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rounded; r += stride) {
        const uint8_t *p = r < n_rec ? bam + rec_off[r] : nullptr;
        const bool counted = p && record_counts(p, f);
        const int n_ev = counted ? walk_ops<false>(p, R, S, 0) : 0;
        int64_t incl = n_ev;
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t u = shfl64(incl, lane >= d ? lane - d : lane);
            if (lane >= d) incl += u;
        }
        const int64_t total = shfl64(incl, 63);
        int64_t base = 0;
        if (lane == 0 && total) base = (int64_t)atomicAdd(S.n_events, (unsigned long long)total);
        base = shfl64(base, 0);
        if (counted) walk_ops<true, true>(p, R, S, base + incl - n_ev, run, first);
    }
}

// Rule 18's test j of an event of length L at slot s: X[s - j] == X[s + L - j], neither of them an N.  Inside a region the slots are the
// positions.  The caller keeps j below the anchor's distance from its region's first slot, so s - j lies above that slot; s + L - j is
// at most s + L, which rule 14 kept inside the region for a deletion, and at most s for an insertion's j >= L.
__device__ __forceinline__ bool shift_holds(const uint8_t *ref, int64_t s, int L, bool ins, uint64_t seq, int64_t j) {
    const uint32_t c = ref[s - j];
    const uint32_t d = ins && j < L ? (uint32_t)(seq >> (2 * (L - 1 - (int)j))) & 3u : (uint32_t)ref[s + L - j];
    return c < 4 && c == d;
}

constexpr int kAlignHead = 8;                        // the tests a lane makes alone before the wave takes its event over

// Rule 18 over the n events an add appended (keys, qe and run begin at the add's first event), a lane per event.  The tests of rule
// 18 are independent, so the shift is the index of the first that fails.  A lane makes the first kAlignHead itself: most events do not
// move, and the rest mostly by a few bases.  An event still open after that is finished by the whole wave, 64 tests a step over
// consecutive reference bytes, one ballot and its first set bit.  A moved event gets its new slot, an insertion its sequence rotated
// by the shift modulo its length (X has period L over the shifted stretch), and the run of match ops that ended at the old anchor
// loses its span over the slots the event crossed: four values taken from the difference array where the lost stretch begins and
// given back at the old anchor.
__global__ void __launch_bounds__(256) pileup_indel_align_kernel(PileupRegions R, int32_t n_regions, const uint8_t *ref, PileupEvKey *keys,
                                                                 const uint32_t *qe, const uint32_t *run, int64_t n, uint32_t *diff) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t rounded = (n + 63) & ~(int64_t)63;                     // whole waves enter every round: the ballots need them
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rounded; i += stride) {
        const PileupEvKey key = i < n ? keys[i] : PileupEvKey{(uint64_t)BWAMS_PILEUP_EV_OTHER << 6, 0};
        const int L = key.len();
        const bool ins = key.type() == BWAMS_PILEUP_EV_INS;
        const int64_t s = key.slot();
        bool open = key.type() != BWAMS_PILEUP_EV_OTHER && L > 0;
        const int64_t room = open ? s - R.off[region_of_slot(R, n_regions, s)] : 0;      // the shift never leaves the anchor's region
        int64_t k = 0;
        for (int j = 0; j < kAlignHead && open; ++j) {
            if (j < room && shift_holds(ref, s, L, ins, key.seq, j)) ++k;
            else open = false;
        }
        for (unsigned long long pend = __ballot(open); pend; pend &= pend - 1) {
            const int src = __ffsll((long long)pend) - 1;
            const int64_t s_w = shfl64(s, src), room_w = shfl64(room, src);
            const uint64_t seq_w = (uint64_t)shfl64((int64_t)key.seq, src);
            const int L_w = __shfl(L, src);
            const bool ins_w = __shfl((int)ins, src) != 0;
            int64_t k_w = kAlignHead;
            for (;;) {                                                   // ends at room_w at the latest
                const int64_t j = k_w + lane;
                const unsigned long long fails = __ballot(!(j < room_w && shift_holds(ref, s_w, L_w, ins_w, seq_w, j)));
                if (fails) { k_w += __ffsll((long long)fails) - 1; break; }
                k_w += 64;
            }
            if (lane == src) k = k_w;
        }
        if (k > 0) {
            uint64_t seq = key.seq;
            const int r = ins ? (int)((uint32_t)k % (uint32_t)L) : 0;    // a slot, and so a shift, is below 2^32
            if (r) {                                                     // 2 r and 2 (L - r) lie in [2, 62], also for L = 32
                const uint64_t mask = L == 32 ? ~0ULL : (1ULL << (2 * L)) - 1;
                seq = (seq << (2 * r) | seq >> (2 * (L - r))) & mask;
            }
            keys[i] = PileupEvKey{(uint64_t)(s - k) << 8 | (key.k0 & 0xFF), seq};
            const int64_t gone = std::min<int64_t>(k, run[i]);
            if (gone > 0) {
                const int q = (int)qe[i];
                const uint32_t v[4] = {1u, (uint32_t)q, pileup_gl_hom(q), pileup_gl_het(q)};
                uint32_t *d0 = diff + 4 * (s - gone), *d1 = diff + 4 * s;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    atomicAdd(d0 + c, 0u - v[c]);
                    atomicAdd(d1 + c, v[c]);
                }
            }
        }
    }
}

__global__ void __launch_bounds__(256) pileup_indel_allele_kernel(const PileupEvKey *keys, const PileupEvSums *sums, int64_t n_groups,
                                                                  PileupRegions R, int32_t n_regions, bwams_pileup_indel_allele_t *out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_groups; i += (int64_t)gridDim.x * blockDim.x) {
        const PileupEvKey k = keys[i];
        const PileupEvSums s = sums[i];
        const int32_t ri = region_of_slot(R, n_regions, k.slot());
        out[i] = bwams_pileup_indel_allele_t{ri, (int32_t)(R.beg[ri] + (k.slot() - R.off[ri])), k.type(), k.len(), k.seq, s.n, s.q, s.hom, s.het};
    }
}

__global__ void __launch_bounds__(256) pileup_indel_call_kernel(PileupIndelTest test, PileupRegions R, int32_t n_regions, const int64_t *groups,
                                                                int64_t n, bwams_pileup_indel_t *out) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = groups[k], s = test.keys[i].slot();
        bwams_pileup_indel_t x;
        uint64_t depth;
        test.genotype(i, &x, &depth);
        x.region = region_of_slot(R, n_regions, s);
        x.pos = (int32_t)(R.beg[x.region] + (s - R.off[x.region]));
        // del_ref: the codes behind the anchor, which rule 14 keeps inside the anchor's region; eight words, no array indexed by a variable
        const int n_del = x.type == BWAMS_PILEUP_EV_DEL ? x.len : 0;
        uint32_t *d = reinterpret_cast<uint32_t *>(out[k].del_ref);
        out[k] = x;                                                      // but del_ref, which the words below fill
#pragma unroll
        for (int w = 0; w < BWAMS_PILEUP_INDEL_MAX / 4; ++w) {
            uint32_t word = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * w + b < n_del) word |= (uint32_t)test.ref[s + 1 + 4 * w + b] << (8 * b);
            d[w] = word;
        }
    }
}

}  // namespace

void launch_pileup_indel_events(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const PileupFilter &f, const PileupRegions &R,
                                const PileupIndelStore &S, int emit, int cu_count, hipStream_t st) {
    if (n_rec <= 0) return;
    if (emit) pileup_indel_kernel<true><<<grid_of(n_rec, 256, cu_count), 256, 0, st>>>(bam, rec_off, n_rec, f, R, S);
    else pileup_indel_kernel<false><<<grid_of(n_rec, 256, cu_count), 256, 0, st>>>(bam, rec_off, n_rec, f, R, S);
}

void launch_pileup_indel_events_run(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const PileupFilter &f, const PileupRegions &R,
                                    const PileupIndelStore &S, uint32_t *run, int64_t first, int cu_count, hipStream_t st) {
    if (n_rec > 0) pileup_indel_run_kernel<<<grid_of(n_rec, 256, cu_count), 256, 0, st>>>(bam, rec_off, n_rec, f, R, S, run, first);
}

void launch_pileup_indel_align(const PileupRegions &R, int32_t n_regions, const uint8_t *ref, PileupEvKey *keys, const uint32_t *qe,
                               const uint32_t *run, int64_t n, uint32_t *diff, int cu_count, hipStream_t st) {
    if (n > 0) pileup_indel_align_kernel<<<grid_of(n, 256, cu_count), 256, 0, st>>>(R, n_regions, ref, keys, qe, run, n, diff);
}

void launch_pileup_indel_alleles(const PileupEvKey *keys, const PileupEvSums *sums, int64_t n_groups, const PileupRegions &R, int32_t n_regions,
                                 bwams_pileup_indel_allele_t *out, int cu_count, hipStream_t st) {
    if (n_groups > 0) pileup_indel_allele_kernel<<<grid_of(n_groups, 256, cu_count), 256, 0, st>>>(keys, sums, n_groups, R, n_regions, out);
}

void launch_pileup_indel_calls(const PileupIndelTest &test, const PileupRegions &R, int32_t n_regions, const int64_t *groups, int64_t n,
                               bwams_pileup_indel_t *out, int cu_count, hipStream_t st) {
    if (n > 0) pileup_indel_call_kernel<<<grid_of(n, 256, cu_count), 256, 0, st>>>(test, R, n_regions, groups, n, out);
}

}  // namespace bwams
