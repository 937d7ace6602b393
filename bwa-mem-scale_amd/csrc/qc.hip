// qc.hip — alignment QC: flag counts, insert sizes and per-cycle tables (the rules are in include/bwams.h above bwams_qc_open).
//
// Layout: every counter is a 64-bit word of one block in HBM (QcLayout, common.h): flags[2][16], scalars[16], then the tables RL,
// QUAL, BASE, MAPQ, ISIZE, INDEL in the shapes of rule 4.
//   qc_check_kernel    lane per record: rule 1.  *bad = min(*bad, record << 3 | reason): the smallest bad index with the first reason
//                      of that record (CIGAR bounds, op, SEQ / QUAL bounds, aux).
//   qc_record_kernel   lane per record: the head, the CIGAR and the aux walk for NM.  The flag counters come from ballots (lane k of a
//                      wave keeps counter k in a register while the wave strides over the records); they, MAPQ, INDEL, RL and the ISIZE
//                      bins below kQcIsizeLds are counted in LDS and the non-zero bins added to HBM once per workgroup; the ISIZE bins
//                      from kQcIsizeLds on go by global atomics.  The scalars stay in registers, are reduced over the wave and added once
//                      per wave.  The indices of the filtered-in records with l_seq > 0 go to one list per class (a ballot and one
//                      atomic per wave and class reserve the places; order is free, the counts commute), with the largest l_seq per
//                      class, which bounds the cycle blocks the next kernel visits.
//   qc_cycle_kernel    tables b and c without an atomic per base.  A workgroup is one wave and owns one item at a time: (class, block of 64
//                      cycles, slice of kQcSlice records of the class's list); lane l owns cycle c0 + l.  The wave takes 64 records a round:
//                      lane j reads record j's head (where SEQ starts, l_seq, the strand, whether it has qualities), then the records go one
//                      after another, their values broadcast by v_readlane: every lane reads the one QUAL byte and the one SEQ nibble of its
//                      cycle (mirrored and complemented under 0x10); the bytes are neighbours, so the wave's read is one segment; four
//                      records' loads leave before the first is counted, with no branch around them (a lane past a record's end reads the
//                      record's last cycle and drops it).  A lane's 64 quality bins are its own LDS row (64 x 64 x 4 B = 16 KB a wave, row
//                      stride 65 words so that equal qualities fall into different banks), updated with plain read-modify-write: no other
//                      lane touches it.  The five base counts and the quality sum are registers.  After the slice the lane adds its non-zero
//                      bins to HBM.  16.25 KB a workgroup: nine one-wave workgroups share a CU's 160 KB; a workgroup of more waves would hold
//                      no more of them (three of three waves under the 64 KB static limit), and one wave needs no barrier.
//   qc_plain_kernel    BWAMS_QC_LANES=0: a wave per listed record, a lane per base in rounds of 64, one global atomic per base and
//                      one per quality.  The A/B baseline (tools/qc_rate.py) and the cross-check of every GPU test.
#include <algorithm>
#include "common.h"
#include "bam_rec.h"
#include "aux_rg.h"
#include "wave_ops.h"

namespace bwams {
namespace {

// Rule 1's walk over the aux area a[0, n) and rule 5's NM (-1: no such field); false when the area cannot be walked.
__device__ __forceinline__ bool aux_walk(const uint8_t *a, int64_t n, int64_t *nm_out) {
    int64_t at = 0, nm = -1;
    while (at < n) {
        if (at + 3 > n) return false;
        const uint32_t t0 = a[at], t1 = a[at + 1], t = a[at + 2];
        at += 3;
        int64_t size = aux_size(t);
        if (size == 0) {
            if (t == 'Z' || t == 'H') {
                int64_t e = at;
                while (e < n && a[e] != 0) ++e;
                if (e >= n) return false;
                size = e + 1 - at;
            } else if (t == 'B') {
                if (at + 5 > n) return false;
                const uint32_t sub = a[at];
                const int w = sub == 'A' ? 0 : aux_size(sub);
                if (w == 0) return false;
                size = 5 + (int64_t)w * ld_u32(a + at + 1);
            } else {
                return false;
            }
        }
        if (at + size > n) return false;
        if (nm < 0 && t0 == 'N' && t1 == 'M' && t != 'A' && t != 'f' && t != 'Z' && t != 'H' && t != 'B') {
            int64_t v;
            if (t == 'c') v = (int8_t)a[at];
            else if (t == 'C') v = a[at];
            else if (t == 's') v = (int16_t)ld_u16(a + at);
            else if (t == 'S') v = ld_u16(a + at);
            else if (t == 'i') v = (int32_t)ld_u32(a + at);
            else v = ld_u32(a + at);
            if (v >= 0) nm = v;
        }
        at += size;
    }
    *nm_out = nm;
    return true;
}

__global__ void __launch_bounds__(256) qc_check_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, uint32_t exclude,
                                                       unsigned long long *bad) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t *p = bam + rec_off[r];
        const int64_t end = bam_end(p), l_seq = bam_l_seq(p);
        const uint32_t n_cig = bam_n_cig(p), l_name = bam_l_name(p);
        int why = -1;
        if (l_seq < 0 || bam_seq_at(l_name, n_cig) > end) {
            why = kQcBadBounds;
        } else {
            const uint8_t *c = p + bam_cigar_at(l_name);
            bool any = false;
            for (uint32_t k = 0; k < n_cig; ++k) any |= (c[4 * k] & 15) > 8;
            const uint32_t flag = bam_flag(p);
            const int64_t aux_at = bam_aux_at(l_name, n_cig, l_seq);
            int64_t nm;
            if (any) why = kQcBadOp;
            else if (flag & exclude) why = -1;
            else if (aux_at > end) why = kQcBadSeq;
            else if (!(flag & 0x4) && !aux_walk(p + aux_at, end - aux_at, &nm)) why = kQcBadAux;
        }
        if (why >= 0) atomicMin(bad, (unsigned long long)r << 3 | (unsigned)why);
    }
}

// the record kernel's LDS, in 32-bit words: flags[2][16], MAPQ[256], INDEL[2][65], ISIZE[3][kQcIsizeLds], RL[2][max_cycle + 1]
constexpr int kLdsFlags = 0, kLdsMapq = 32, kLdsIndel = kLdsMapq + 256, kLdsIsize = kLdsIndel + 130, kLdsRl = kLdsIsize + 3 * kQcIsizeLds;

__device__ __forceinline__ void flush_bins(const uint32_t *lds, int n, unsigned long long *out) {
    for (int i = threadIdx.x; i < n; i += blockDim.x)
        if (lds[i]) atomicAdd(out + i, (unsigned long long)lds[i]);
}

__global__ void __launch_bounds__(256) qc_record_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, QcLayout L,
                                                        unsigned long long *cnt, uint32_t *lists, unsigned long long *call) {
    extern __shared__ uint32_t lds[];
    const int rl_n = L.max_cycle + 1, n_lds = kLdsRl + 2 * rl_n;
    for (int i = threadIdx.x; i < n_lds; i += blockDim.x) lds[i] = 0;
    __syncthreads();
    const int lane = (int)(threadIdx.x & 63);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t rounded = (n_rec + 63) & ~(int64_t)63;                 // whole waves enter every round: the ballots need them
    uint32_t my_flag = 0;                                                // lane k < 32: flag counter k & 15 of class k >> 4
    int64_t reads = 0, bases = 0, mapped_n = 0, bases_mapped = 0, clipped = 0, nm_sum = 0, nm_missing = 0, over = 0, no_qual = 0;
    int32_t max_len0 = 0, max_len1 = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rounded; r += stride) {
        uint32_t bits = 0;                                               // rule 2's sixteen predicates of this record
        int qc_class = 0, list = -1;                                     // list: the class whose list takes the record
        if (r < n_rec) {
            const uint8_t *p = bam + rec_off[r];
            const uint32_t flag = bam_flag(p), mapq = bam_mapq(p), n_cig = bam_n_cig(p), l_name = bam_l_name(p);
            const int32_t rid = bam_ref_id(p), nrid = bam_next_ref_id(p), l_seq = bam_l_seq(p);
            const bool primary = !(flag & 0x900), mapped = !(flag & 0x4), dup = (flag & 0x400) != 0;
            const bool pp = primary && (flag & 0x1), both = pp && !(flag & 0xC), far = both && nrid != rid;
            qc_class = (flag & 0x200) ? 1 : 0;
            bits = 1u | (uint32_t)primary << 1 | (uint32_t)((flag & 0x100) != 0) << 2 | (uint32_t)((flag & 0x900) == 0x800) << 3 |
                   (uint32_t)dup << 4 | (uint32_t)(primary && dup) << 5 | (uint32_t)mapped << 6 | (uint32_t)(primary && mapped) << 7 |
                   (uint32_t)pp << 8 | (uint32_t)(pp && (flag & 0x40)) << 9 | (uint32_t)(pp && (flag & 0x80)) << 10 |
                   (uint32_t)(pp && (flag & 0x2) && mapped) << 11 | (uint32_t)both << 12 | (uint32_t)(pp && (flag & 0x8) && mapped) << 13 |
                   (uint32_t)far << 14 | (uint32_t)(far && mapq >= 5) << 15;
            if (!(flag & L.exclude)) {                                   // rule 3
                const int c = (flag & 0x80) ? 1 : 0;
                ++reads;
                bases += l_seq;
                const int32_t shown = min(l_seq, L.max_cycle);
                over += l_seq - shown;
                atomicAdd(lds + kLdsRl + c * rl_n + shown, 1u);
                if (l_seq > 0) {
                    list = c;
                    if (c) max_len1 = max(max_len1, l_seq);
                    else max_len0 = max(max_len0, l_seq);
                    if (p[bam_qual_at(l_name, n_cig, l_seq)] == 0xFF) ++no_qual;
                }
                if (mapped) {
                    ++mapped_n;
                    atomicAdd(lds + kLdsMapq + mapq, 1u);
                    const uint8_t *cig = p + bam_cigar_at(l_name);
                    for (uint32_t k = 0; k < n_cig; ++k) {
                        const uint32_t op = ld_u32(cig + 4 * k), o = op & 15, len = op >> 4;
                        if (o == 0 || o == 1 || o == 7 || o == 8) bases_mapped += len;
                        if (o == 4) clipped += len;
                        if ((o == 1 || o == 2) && len >= 1) atomicAdd(lds + kLdsIndel + (o - 1) * 65 + (int)min(len, 64u), 1u);
                    }
                    const int64_t aux_at = bam_aux_at(l_name, n_cig, l_seq);
                    int64_t nm = -1;
                    aux_walk(p + aux_at, bam_end(p) - aux_at, &nm);                              // rule 1 walked it already
                    if (nm < 0) ++nm_missing;
                    else nm_sum += nm;
                }
                const int32_t tlen = bam_tlen(p);
                if ((flag & 0x1) && !(flag & 0xC) && rid == nrid && rid >= 0 && tlen > 0) {      // rule 4e
                    const bool rev = (flag & 0x10) != 0;
                    const int row = rev == ((flag & 0x20) != 0) ? 2 : (bam_pos(p) <= bam_next_pos(p)) ? (int)rev : 1 - (int)rev;
                    const int32_t bin = min(tlen, L.max_isize);
                    if (bin < kQcIsizeLds) atomicAdd(lds + kLdsIsize + row * kQcIsizeLds + bin, 1u);
                    else atomicAdd(cnt + L.isize() + (int64_t)row * (L.max_isize + 1) + bin, 1ULL);
                }
            }
        }
        for (int k = 0; k < 32; ++k) {                                   // rule 2: a ballot per counter and class
            const uint64_t m = __ballot((bits >> (k & 15) & 1) && qc_class == (k >> 4));
            if (lane == k) my_flag += (uint32_t)__popcll((unsigned long long)m);
        }
        for (int c = 0; c < 2; ++c) {                                    // the lists: places reserved once per wave and class
            const uint64_t m = __ballot(list == c);
            if (!m) continue;
            unsigned long long at = 0;
            if (lane == 0) at = atomicAdd(call + kQcCallList + c, (unsigned long long)__popcll((unsigned long long)m));
            at = (unsigned long long)readlane64((int64_t)at, 0);
            if (list == c) lists[(int64_t)c * n_rec + (int64_t)at + __popcll((unsigned long long)(m & ((1ULL << lane) - 1)))] = (uint32_t)r;
        }
    }
    if (lane < 32 && my_flag) atomicAdd(lds + kLdsFlags + lane, my_flag);
    const int64_t s_reads = wave_sum(reads), s_bases = wave_sum(bases), s_mapped = wave_sum(mapped_n), s_bm = wave_sum(bases_mapped),
                  s_clip = wave_sum(clipped), s_nm = wave_sum(nm_sum), s_miss = wave_sum(nm_missing), s_over = wave_sum(over),
                  s_noq = wave_sum(no_qual);
    const int32_t m0 = wave_max(max_len0), m1 = wave_max(max_len1);
    if (lane == 0 && s_reads) {
        unsigned long long *s = cnt + L.scalars();
        atomicAdd(s + BWAMS_QC_READS, (unsigned long long)s_reads);
        if (s_bases) atomicAdd(s + BWAMS_QC_BASES, (unsigned long long)s_bases);
        if (s_mapped) atomicAdd(s + BWAMS_QC_MAPPED, (unsigned long long)s_mapped);
        if (s_bm) atomicAdd(s + BWAMS_QC_BASES_MAPPED, (unsigned long long)s_bm);
        if (s_clip) atomicAdd(s + BWAMS_QC_CLIPPED, (unsigned long long)s_clip);
        if (s_nm) atomicAdd(s + BWAMS_QC_NM_SUM, (unsigned long long)s_nm);
        if (s_miss) atomicAdd(s + BWAMS_QC_NM_MISSING, (unsigned long long)s_miss);
        if (s_over) { atomicAdd(s + BWAMS_QC_BASES_OVER, (unsigned long long)s_over); atomicAdd(call + kQcCallOver, (unsigned long long)s_over); }
        if (s_noq) atomicAdd(s + BWAMS_QC_NO_QUAL, (unsigned long long)s_noq);
        atomicAdd(call + kQcCallCounted, (unsigned long long)s_reads);
        if (m0) atomicMax(call + kQcCallMaxLen, (unsigned long long)m0);
        if (m1) atomicMax(call + kQcCallMaxLen + 1, (unsigned long long)m1);
    }
    __syncthreads();
    flush_bins(lds + kLdsFlags, 32, cnt + L.flags());
    flush_bins(lds + kLdsMapq, 256, cnt + L.mapq());
    flush_bins(lds + kLdsIndel, 130, cnt + L.indel());
    for (int row = 0; row < 3; ++row)
        flush_bins(lds + kLdsIsize + row * kQcIsizeLds, min(kQcIsizeLds, L.max_isize + 1), cnt + L.isize() + (int64_t)row * (L.max_isize + 1));
    flush_bins(lds + kLdsRl, 2 * rl_n, cnt + L.rl());
}

// A, C, G, T, N (0..4) of a 4-bit SEQ code, complemented for a reverse record
__device__ __forceinline__ int base_of(uint32_t code, bool rev) {
    const int b = code == 1 ? 0 : code == 2 ? 1 : code == 4 ? 2 : code == 8 ? 3 : 4;
    return rev && b < 4 ? 3 - b : b;
}

constexpr int kRowStride = 65;                                           // words between two lanes' rows
constexpr int kUnroll = 4;                                               // records whose bytes a wave of the cycle kernel has in flight

__global__ void __launch_bounds__(64) qc_cycle_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, QcLayout L,
                                                      unsigned long long *cnt, const uint32_t *lists, const unsigned long long *call) {
    __shared__ uint32_t rows[64 * kRowStride];
    const int lane = (int)threadIdx.x;
    uint32_t *row = rows + lane * kRowStride;
    // the items: class c has blocks[c] cycle blocks x slices[c] slices, class 0's items first
    int64_t len[2], slices[2], blocks[2];
    for (int c = 0; c < 2; ++c) {
        len[c] = (int64_t)call[kQcCallList + c];
        slices[c] = (len[c] + kQcSlice - 1) / kQcSlice;
        blocks[c] = (std::min<int64_t>((int64_t)call[kQcCallMaxLen + c], L.max_cycle) + 63) / 64;
    }
    const int64_t items0 = blocks[0] * slices[0], items = items0 + blocks[1] * slices[1];
    unsigned long long q_sum = 0, q_bases = 0;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int c = item < items0 ? 0 : 1;
        const int64_t it = c ? item - items0 : item;
        const int32_t cycle = (int32_t)(it % blocks[c]) * 64 + lane;     // neighbouring workgroups share a slice's records in cache
        const int64_t first = (it / blocks[c]) * kQcSlice, last = std::min<int64_t>(first + kQcSlice, len[c]);
        const uint32_t *list = lists + (int64_t)c * n_rec;
        for (int k = 0; k < 64; ++k) row[k] = 0;
        uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0, b4 = 0, sum = 0, n_q = 0;
        for (int64_t j0 = first; j0 < last; j0 += 64) {
            const int n = (int)std::min<int64_t>(64, last - j0);
            int64_t my_seq = 0;                                          // lane j: record j0 + j, where its SEQ starts ...
            int32_t my_len = 0, my_bits = 0;                             // ... its l_seq; bit 0: 0x10, bit 1: it has qualities
            if (lane < n) {
                const int64_t off = rec_off[list[j0 + lane]];
                const uint8_t *p = bam + off;
                my_len = bam_l_seq(p);
                my_seq = off + bam_seq_at(bam_l_name(p), bam_n_cig(p));
                my_bits = ((bam_flag(p) & 0x10) ? 1 : 0) | (bam[my_seq + (my_len + 1) / 2] != 0xFF ? 2 : 0);
            }
            for (int j = 0; j < n; j += kUnroll) {                       // the loads of kUnroll records leave before the first count
                uint32_t two[kUnroll], q[kUnroll];
                int state[kUnroll];                                      // -1: the record has no such cycle; else bit 0: 0x10, bit 1: low nibble, bit 2: qualities
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    // No branch around the loads, or each would be waited for where its branch ends: a lane past the record's end
                    // reads the bytes of the record's last cycle (every listed record has l_seq > 0), a slot past the round's end
                    // the round's last record again; state says what counts.
                    const int ju = min(j + u, n - 1);
                    const int32_t l_seq = __builtin_amdgcn_readlane(my_len, ju), rbits = __builtin_amdgcn_readlane(my_bits, ju);
                    const uint8_t *seq = bam + readlane64(my_seq, ju);
                    const int32_t at = min(cycle, l_seq - 1), i = (rbits & 1) ? l_seq - 1 - at : at;
                    two[u] = seq[i >> 1];
                    q[u] = seq[(l_seq + 1) / 2 + i];
                    state[u] = (j + u < n && cycle < l_seq) ? (rbits & 1) | (i & 1) << 1 | (rbits & 2) << 1 : -1;
                }
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    if (state[u] < 0) continue;
                    if (state[u] & 4) {
                        row[min(q[u], 63u)] += 1;
                        sum += q[u];
                        ++n_q;
                    }
                    const int b = base_of((two[u] >> ((state[u] & 2) ? 0 : 4)) & 15, state[u] & 1);
                    b0 += b == 0; b1 += b == 1; b2 += b == 2; b3 += b == 3; b4 += b == 4;
                }
            }
        }
        unsigned long long *qual = cnt + L.qual() + ((int64_t)c * L.max_cycle + cycle) * 64;
        for (int k = 0; k < 64; ++k)
            if (row[k]) atomicAdd(qual + k, (unsigned long long)row[k]);
        unsigned long long *base = cnt + L.base() + ((int64_t)c * L.max_cycle + cycle) * 5;
        if (b0) atomicAdd(base, (unsigned long long)b0);
        if (b1) atomicAdd(base + 1, (unsigned long long)b1);
        if (b2) atomicAdd(base + 2, (unsigned long long)b2);
        if (b3) atomicAdd(base + 3, (unsigned long long)b3);
        if (b4) atomicAdd(base + 4, (unsigned long long)b4);
        q_sum += sum;                                                    // at most kQcSlice x 255 an item
        q_bases += n_q;
    }
    const int64_t s = wave_sum((int64_t)q_sum), nb = wave_sum((int64_t)q_bases);
    if (lane == 0 && nb) {
        atomicAdd(cnt + L.scalars() + BWAMS_QC_QUAL_BASES, (unsigned long long)nb);
        if (s) atomicAdd(cnt + L.scalars() + BWAMS_QC_QUAL_SUM, (unsigned long long)s);
    }
}

__global__ void __launch_bounds__(256) qc_plain_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, QcLayout L,
                                                       unsigned long long *cnt, const uint32_t *lists, const unsigned long long *call) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t len0 = (int64_t)call[kQcCallList], total = len0 + (int64_t)call[kQcCallList + 1];
    int64_t q_sum = 0, q_bases = 0;
    for (int64_t e = wave; e < total; e += n_waves) {
        const int c = e < len0 ? 0 : 1;
        const uint8_t *p = bam + rec_off[lists[(int64_t)c * n_rec + (c ? e - len0 : e)]];
        const int32_t l_seq = bam_l_seq(p);
        const uint8_t *seq = p + bam_seq_at(bam_l_name(p), bam_n_cig(p)), *qual = seq + (l_seq + 1) / 2;
        const bool rev = (bam_flag(p) & 0x10) != 0, has_qual = qual[0] != 0xFF;
        for (int32_t cycle = lane; cycle < min(l_seq, L.max_cycle); cycle += 64) {
            const int32_t i = rev ? l_seq - 1 - cycle : cycle;
            const int64_t at = (int64_t)c * L.max_cycle + cycle;
            atomicAdd(cnt + L.base() + at * 5 + base_of((seq[i >> 1] >> ((i & 1) ? 0 : 4)) & 15, rev), 1ULL);
            if (has_qual) {
                const uint32_t q = qual[i];
                atomicAdd(cnt + L.qual() + at * 64 + min(q, 63u), 1ULL);
                q_sum += q;
                ++q_bases;
            }
        }
    }
    const int64_t s = wave_sum(q_sum), nb = wave_sum(q_bases);
    if (lane == 0 && nb) {
        atomicAdd(cnt + L.scalars() + BWAMS_QC_QUAL_BASES, (unsigned long long)nb);
        if (s) atomicAdd(cnt + L.scalars() + BWAMS_QC_QUAL_SUM, (unsigned long long)s);
    }
}

}  // namespace

void launch_qc_check(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, uint32_t exclude, unsigned long long *bad, int cu_count,
                     hipStream_t st) {
    if (n_rec > 0) qc_check_kernel<<<grid_of(n_rec, 256, cu_count, 16), 256, 0, st>>>(bam, rec_off, n_rec, exclude, bad);
}

void launch_qc_records(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const QcLayout &L, unsigned long long *counters,
                       uint32_t *lists, unsigned long long *call, int cu_count, hipStream_t st) {
    const size_t lds = (size_t)(kLdsRl + 2 * (L.max_cycle + 1)) * 4;     // 13.6 KB + at most 32 KB
    if (n_rec > 0) qc_record_kernel<<<grid_of(n_rec, 256, cu_count, 8), 256, lds, st>>>(bam, rec_off, n_rec, L, counters, lists, call);
}

void launch_qc_cycles(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const QcLayout &L, unsigned long long *counters,
                      const uint32_t *lists, const unsigned long long *call, int lanes, int cu_count, hipStream_t st) {
    if (n_rec <= 0) return;
    if (lanes) {                                                         // no more items than this exist; the workgroups beyond leave at once
        const int64_t most = (int64_t)(L.max_cycle / 64) * ((n_rec + kQcSlice - 1) / kQcSlice + 1);
        qc_cycle_kernel<<<grid_of(most, 1, cu_count, 36), 64, 0, st>>>(bam, rec_off, n_rec, L, counters, lists, call);
    } else {
        qc_plain_kernel<<<grid_of(n_rec, 4, cu_count, 16), 256, 0, st>>>(bam, rec_off, n_rec, L, counters, lists, call);
    }
}

}  // namespace bwams
