// markdup.hip — duplicate marking of BAM records in HBM (bwams_bam_templates, bwams_dup_decide, bwams_bam_markdup).
//
// The rules are Picard MarkDuplicates' for query-grouped input, written out in include/bwams.h above bwams_bam_templates and
// restated in bwams/markdup.py.  Templates and their ends, over n_rec records at bam + rec_off[r] (the buffer holds 16 bytes of slack
// past its last record, as bwams_bam_run / _upload allocate it):
//   md_head_kernel   lane per record: head[r] = 1 where its name differs from the previous record's (rule 1);
//   rocprim::inclusive_scan of head: tid[r], the template's ordinal + 1;
//   md_rec_kernel    sixteen lanes per record: rtmpl[r] = tid[r] - 1, tstart[template] at a head; for a mapped primary the unclipped
//                    5' coordinate (rule 3: lane 0 walks the leading clips, lane 1 the trailing ones, every lane sums a share of the
//                    reference length) and the score (rule 4: QUAL read as aligned dwords, bytes >= 15 summed, capped per lane and
//                    after a cross-lane reduction), into a 16-byte MdRec;
//   md_tmpl_kernel   lane per template: walks its MdRecs in order, applies rule 2 and 3's refusals (the first fault ends the walk;
//                    atomicMin of record << 2 | reason over all templates gives the first record concerned) and builds its end (rule 5);
//   rocprim::select  of the templates that have an end: the ends, in template order.
// The decision (rule 6) over n_e ends of templates [0, n_t):
//   md_check_kernel  lane per end: the ends' bounds (a tmpl outside [0, n_t) would be a store out of bounds), the largest refID, the pairs;
//   md_pair_keys / md_frag_keys  the sort keys of the pairs (one slot per end) and of the fragments (two slots per end: a pair's two
//                    ends as paired fragments).  A position key is ref << 33 | (pos + 2^31) << 1 | strand; slots that hold nothing take
//                    ref = the largest refID + 1, so they group apart and are skipped;
//   stable rocPRIM radix sorts, least significant key first, over the bits the values need: pairs by (32767 - score) << tb | tmpl,
//                    then key 2, then key 1; fragments by (unpaired << 15 | 32767 - score) << tb | tmpl, then the key.  In each group
//                    of equal keys the first slot is then the one kept (for fragments: a paired fragment whenever the group holds one);
//   md_mark_pairs / md_mark_frags  lane per sorted slot: a pair slot that is not its group's first, an unpaired fragment slot that is
//                    not its group's first, writes dup[tmpl] = 1 (each template has one end, so no slot races another's byte).
// md_apply_kernel: lane per record, sets or clears 0x400 in FLAG's high byte (byte 19 of the record) from dup[rtmpl[r]].
// Every kernel is memory-bound; none uses LDS or scratch.
#include <algorithm>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include "common.h"

namespace bwams {
namespace {

constexpr int kGroup = 16;
constexpr int kQualMin = 15, kScoreCap = 16383;
constexpr int32_t kMaxRef = 1 << 30;                  // refIDs of the decision: [0, 2^30), so that ref << 33 and one more fit 64 bits

__device__ __forceinline__ uint32_t ld_u32(const uint8_t *p) {          // little-endian, any alignment
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

__device__ __forceinline__ uint32_t qual_sum4(uint32_t w, uint32_t keep) {   // the bytes of w >= 15 that `keep` (bit per byte) selects
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t q = (w >> (8 * k)) & 0xFF;
        s += ((keep >> k) & 1) && q >= (uint32_t)kQualMin ? q : 0;
    }
    return s;
}

__global__ void __launch_bounds__(256) md_head_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, uint32_t *head) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (int64_t)gridDim.x * blockDim.x) {
        uint32_t h = 1;
        if (r > 0) {
            const uint8_t *p = bam + rec_off[r - 1], *q = bam + rec_off[r];
            const uint32_t l = p[12];
            if (l == q[12]) {
                uint32_t k = 0;
                while (k < l && p[36 + k] == q[36 + k]) ++k;
                h = k < l;
            }
        }
        head[r] = h;
    }
}

__global__ void __launch_bounds__(256) md_rec_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const uint32_t *head,
                                                     const uint32_t *tid, uint32_t *rtmpl, uint32_t *tstart, MdRec *rec) {
    const int g = (int)(threadIdx.x & (kGroup - 1));
    const int64_t n_groups = (int64_t)gridDim.x * (blockDim.x / kGroup);
    // every lane of a group runs the same number of iterations (r depends on the group only), so the shuffles below see all 16
    for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup; r < n_rec; r += n_groups) {
        const uint8_t *p = bam + rec_off[r];
        const int32_t rid = (int32_t)ld_u32(p + 4), pos = (int32_t)ld_u32(p + 8);
        const uint32_t l_name = p[12];
        const uint32_t n_cig = (uint32_t)p[16] | (uint32_t)p[17] << 8;
        const uint32_t flag = (uint32_t)p[18] | (uint32_t)p[19] << 8;
        const int64_t l_seq = (int32_t)ld_u32(p + 20);
        const bool want = !(flag & 0x904);                     // a mapped primary: its coordinate and score
        int64_t rlen = 0, clip = 0;
        uint32_t score = 0;
        if (want) {
            const uint8_t *c = p + 36 + l_name;
            for (uint32_t k = g; k < n_cig; k += kGroup) {
                const uint32_t op = ld_u32(c + 4 * k), o = op & 15;
                if (o == 0 || o == 2 || o == 3 || o == 7 || o == 8) rlen += op >> 4;
            }
            if (g == 0 && !(flag & 16)) {                    // forward: the S and H lengths before the first other op
                for (uint32_t k = 0; k < n_cig; ++k) {
                    const uint32_t op = ld_u32(c + 4 * k), o = op & 15;
                    if (o != 4 && o != 5) break;
                    clip += op >> 4;
                }
            }
            if (g == 1 && (flag & 16)) {                     // reverse: the S and H lengths after the last other op
                for (uint32_t k = n_cig; k-- > 0;) {
                    const uint32_t op = ld_u32(c + 4 * k), o = op & 15;
                    if (o != 4 && o != 5) break;
                    clip += op >> 4;
                }
            }
            const uint8_t *qs = c + 4 * (int64_t)n_cig + (l_seq + 1) / 2;
            const int64_t n_q = std::min<int64_t>(l_seq, (p + 4 + ld_u32(p)) - qs);     // never past the record's block_size
            if (n_q > 0 && qs[0] != 0xFF) {                   // QUAL present: aligned dwords over [qs, qs + n_q)
                const uintptr_t a0 = reinterpret_cast<uintptr_t>(qs) & ~(uintptr_t)3;
                const uintptr_t e = reinterpret_cast<uintptr_t>(qs) + (uintptr_t)n_q;
                const int64_t n_dw = (int64_t)((e - a0 + 3) >> 2);
                const uint32_t *w = reinterpret_cast<const uint32_t *>(a0);
                for (int64_t k = g; k < n_dw; k += kGroup) {
                    const uintptr_t at = a0 + 4 * (uintptr_t)k;
                    uint32_t keep = 0xF;
                    if (at < reinterpret_cast<uintptr_t>(qs)) keep &= 0xFu << (reinterpret_cast<uintptr_t>(qs) - at);
                    if (at + 4 > e) keep &= 0xFu >> (at + 4 - e);
                    score = min(score + qual_sum4(w[k], keep), (uint32_t)kScoreCap);
                }
            }
        }
#pragma unroll
        for (int m = kGroup / 2; m > 0; m >>= 1) {
            rlen += __shfl_xor(rlen, m, kGroup);
            clip += __shfl_xor(clip, m, kGroup);
            score += __shfl_xor(score, m, kGroup);
        }
        if (g == 0) {
            const uint32_t t = tid[r] - 1;
            rtmpl[r] = t;
            if (head[r]) tstart[t] = (uint32_t)r;
            MdRec m;
            m.c = !want ? 0 : (flag & 16) ? (int64_t)pos + (rlen ? rlen : 1) - 1 + clip : (int64_t)pos - clip;
            m.rid = rid;
            m.flag = (uint16_t)flag;
            m.score = (uint16_t)min(score, (uint32_t)kScoreCap);
            rec[r] = m;
        }
    }
}

// reasons of a refusal, in the low two bits of record << 2 | reason
enum { kTwoPrimaries = 0, kSegmentBits = 1, kMixed = 2, kCoordinate = 3 };

__global__ void __launch_bounds__(256) md_tmpl_kernel(const MdRec *rec, const uint32_t *tstart, int64_t n_t, int64_t n_rec,
                                                      bwams_dup_end_t *tend, uint8_t *has, unsigned long long *bad) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_t; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r0 = tstart[t], r1 = t + 1 < n_t ? (int64_t)tstart[t + 1] : n_rec;
        int64_t only = -1, first = -1, last = -1;            // the primary of each segment
        int paired = -1;
        unsigned long long fault = ~0ULL;
        for (int64_t r = r0; r < r1 && fault == ~0ULL; ++r) {
            const uint32_t f = rec[r].flag;
            if (f & 0x900) continue;
            const int p = f & 1;
            if (paired < 0) paired = p;
            int64_t &seg = !p ? only : (f & 0x40) ? first : last;
            if (p != paired) fault = (unsigned long long)r << 2 | kMixed;
            else if (p && ((f >> 6) & 1) == ((f >> 7) & 1)) fault = (unsigned long long)r << 2 | kSegmentBits;
            else if (seg >= 0) fault = (unsigned long long)r << 2 | kTwoPrimaries;
            else if (!(f & 4) && (rec[r].rid < 0 || rec[r].c < -(1LL << 31) || rec[r].c >= (1LL << 31)))
                fault = (unsigned long long)r << 2 | kCoordinate;
            else seg = r;
        }
        uint8_t h = 0;
        bwams_dup_end_t e;
        e.tmpl = t; e.ref2 = -1; e.pos2 = 0;
        const bool m_only = only >= 0 && !(rec[only].flag & 4), m_first = first >= 0 && !(rec[first].flag & 4);
        const bool m_last = last >= 0 && !(rec[last].flag & 4);
        if (fault != ~0ULL) {
            atomicMin(bad, fault);
        } else if (m_first && m_last) {                      // a pair: end 1 the smaller (refID, coordinate), on a tie the earlier record
            const int64_t a = min(first, last), b = max(first, last);
            const MdRec A = rec[a], B = rec[b];
            const bool swap = B.rid < A.rid || (B.rid == A.rid && B.c < A.c);
            const MdRec E1 = swap ? B : A, E2 = swap ? A : B;
            e.ref1 = E1.rid; e.pos1 = (int32_t)E1.c; e.ref2 = E2.rid; e.pos2 = (int32_t)E2.c;
            e.score = (int32_t)E1.score + (int32_t)E2.score;
            e.strands = (int32_t)((E1.flag >> 4) & 1) | (int32_t)((E2.flag >> 4) & 1) << 1;
            h = 1;
        } else if ((int)m_only + (int)m_first + (int)m_last == 1) {
            const MdRec E1 = rec[m_only ? only : m_first ? first : last];
            e.ref1 = E1.rid; e.pos1 = (int32_t)E1.c;
            e.score = E1.score;
            e.strands = (int32_t)((E1.flag >> 4) & 1);
            h = 1;
        }
        if (!h) { e.ref1 = -1; e.pos1 = 0; e.score = 0; e.strands = 0; }
        tend[t] = e;
        has[t] = h;
    }
}

// info[0]: the first bad end (atomicMin); info[1]: the largest refID + 1 (atomicMax); info[2]: the pairs
__global__ void __launch_bounds__(256) md_check_kernel(const bwams_dup_end_t *ends, int64_t n_e, int64_t n_t, unsigned long long *info) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_e; i += (int64_t)gridDim.x * blockDim.x) {
        const bwams_dup_end_t e = ends[i];
        if (e.tmpl < 0 || e.tmpl >= n_t || e.ref1 < 0 || e.ref1 >= kMaxRef || e.ref2 < -1 || e.ref2 >= kMaxRef || e.score < 0 ||
            e.score > 32767 || e.strands < 0 || e.strands > 3 || (e.ref2 < 0 && (e.strands & 2)))
            atomicMin(info, (unsigned long long)i);
        atomicMax(info + 1, (unsigned long long)(uint32_t)max(e.ref1, e.ref2) + 1);
        if (e.ref2 >= 0) atomicAdd(info + 2, 1ULL);
    }
}

__device__ __forceinline__ uint64_t pos_key(int32_t ref, int32_t pos, int strand) {
    return (uint64_t)(uint32_t)ref << 33 | (uint64_t)((uint32_t)pos ^ 0x80000000u) << 1 | (uint64_t)strand;
}

__device__ __forceinline__ uint64_t rank_of(const bwams_dup_end_t &e, int tb) {      // (32767 - score) << tb | tmpl
    return (uint64_t)(32767 - e.score) << tb | (uint64_t)e.tmpl;
}

__global__ void __launch_bounds__(256) md_pair_keys_kernel(const bwams_dup_end_t *ends, int64_t n_e, int32_t none_ref, int tb,
                                                           uint64_t *k1, uint64_t *k2, uint64_t *v, uint32_t *idx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_e; i += (int64_t)gridDim.x * blockDim.x) {
        const bwams_dup_end_t e = ends[i];
        const bool pair = e.ref2 >= 0;
        k1[i] = pair ? pos_key(e.ref1, e.pos1, e.strands & 1) : pos_key(none_ref, 0, 0);
        k2[i] = pair ? pos_key(e.ref2, e.pos2, (e.strands >> 1) & 1) : 0;
        v[i] = rank_of(e, tb);
        idx[i] = (uint32_t)i;
    }
}

__global__ void __launch_bounds__(256) md_frag_keys_kernel(const bwams_dup_end_t *ends, int64_t n_e, int32_t none_ref, int tb,
                                                           uint64_t *k, uint64_t *w, uint32_t *idx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_e; i += (int64_t)gridDim.x * blockDim.x) {
        const bwams_dup_end_t e = ends[i];
        const bool pair = e.ref2 >= 0;
        const uint64_t rank = (uint64_t)(pair ? 0 : 1) << (15 + tb) | rank_of(e, tb);
        k[2 * i] = pos_key(e.ref1, e.pos1, e.strands & 1);
        k[2 * i + 1] = pair ? pos_key(e.ref2, e.pos2, (e.strands >> 1) & 1) : pos_key(none_ref, 0, 0);
        w[2 * i] = w[2 * i + 1] = rank;
        idx[2 * i] = (uint32_t)(2 * i);
        idx[2 * i + 1] = (uint32_t)(2 * i + 1);
    }
}

__global__ void __launch_bounds__(256) md_gather64_kernel(const uint64_t *src, const uint32_t *idx, int64_t n, uint64_t *dst) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[idx[i]];
}

__global__ void __launch_bounds__(256) md_gather32_kernel(const uint32_t *src, const uint32_t *idx, int64_t n, uint32_t *dst) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[idx[i]];
}

// pairs, sorted: ks = key 1 in sorted order, k2 = key 2 by end, idx = end of each slot
__global__ void __launch_bounds__(256) md_mark_pairs_kernel(const uint64_t *ks, const uint64_t *k2, const uint32_t *idx, int64_t n,
                                                            uint64_t none_key, const bwams_dup_end_t *ends, uint8_t *dup,
                                                            unsigned long long *n_dup) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t e = idx[i];
        if (i > 0 && ks[i] != none_key && ks[i] == ks[i - 1] && k2[e] == k2[idx[i - 1]]) {
            dup[ends[e].tmpl] = 1;
            atomicAdd(n_dup, 1ULL);
        }
    }
}

// fragment slots, sorted: ks = key in sorted order, idx = slot (end * 2 + which end)
__global__ void __launch_bounds__(256) md_mark_frags_kernel(const uint64_t *ks, const uint32_t *idx, int64_t n, uint64_t none_key,
                                                            const bwams_dup_end_t *ends, uint8_t *dup, unsigned long long *n_dup) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const bwams_dup_end_t &e = ends[idx[i] >> 1];
        if (i > 0 && ks[i] != none_key && e.ref2 < 0 && ks[i] == ks[i - 1]) {
            dup[e.tmpl] = 1;
            atomicAdd(n_dup, 1ULL);
        }
    }
}

__global__ void __launch_bounds__(256) md_apply_kernel(uint8_t *bam, const int64_t *rec_off, const uint32_t *perm, const uint32_t *rtmpl,
                                                       const uint8_t *dup, int64_t n_rec, unsigned long long *n_marked) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rec; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t r = perm ? perm[i] : (uint32_t)i;
        const bool d = dup[rtmpl[r]] != 0;
        uint8_t *f = bam + rec_off[i] + 19;                  // FLAG's high byte: 0x400 is its bit 2
        *f = (uint8_t)((*f & ~4u) | (d ? 4u : 0u));
        if (d) atomicAdd(n_marked, 1ULL);
    }
}

unsigned grid_of(int64_t items, int64_t per_block, int cu_count) {
    int64_t g = (items + per_block - 1) / per_block;
    const int64_t cap = (int64_t)cu_count * 16;
    return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

int bit_width(uint64_t x) {
    int w = 0;
    while (w < 64 && (x >> w) != 0) ++w;
    return w;
}

const char *kReason[4] = {"two primaries of one segment", "a paired primary with neither or both of 0x40 / 0x80",
                          "paired and unpaired primaries mixed", "a mapped primary's unclipped 5' coordinate outside [-2^31, 2^31) or its refID -1"};

}  // namespace

int md_templates(MdTemplates &m, const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, int cu_count, hipStream_t st) {
    m.n_t = m.n_e = 0;
    if (n_rec == 0) return BWAMS_OK;
    const size_t n = (size_t)n_rec;
    BWAMS_HIP(m.head.ensure(n * 4)); BWAMS_HIP(m.tid.ensure(n * 4)); BWAMS_HIP(m.rtmpl.ensure(n * 4));
    BWAMS_HIP(m.tstart.ensure(n * 4)); BWAMS_HIP(m.rec.ensure(n * sizeof(MdRec)));
    BWAMS_HIP(m.info.ensure(16));
    md_head_kernel<<<grid_of(n_rec, 256, cu_count), 256, 0, st>>>(bam, rec_off, n_rec, m.head.as<uint32_t>());
    size_t tb = 0;
    BWAMS_HIP(rocprim::inclusive_scan(nullptr, tb, m.head.as<const uint32_t>(), m.tid.as<uint32_t>(), n, rocprim::plus<uint32_t>(), st));
    BWAMS_HIP(m.tmp.ensure(tb));
    BWAMS_HIP(rocprim::inclusive_scan(m.tmp.p, tb, m.head.as<const uint32_t>(), m.tid.as<uint32_t>(), n, rocprim::plus<uint32_t>(), st));
    md_rec_kernel<<<grid_of(n_rec, 256 / kGroup, cu_count), 256, 0, st>>>(bam, rec_off, n_rec, m.head.as<const uint32_t>(),
                                                                          m.tid.as<const uint32_t>(), m.rtmpl.as<uint32_t>(),
                                                                          m.tstart.as<uint32_t>(), m.rec.as<MdRec>());
    uint32_t n_t = 0;
    BWAMS_HIP(hipMemcpyAsync(&n_t, m.tid.as<uint32_t>() + n_rec - 1, 4, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    BWAMS_HIP(m.tend.ensure((size_t)n_t * sizeof(bwams_dup_end_t))); BWAMS_HIP(m.ends.ensure((size_t)n_t * sizeof(bwams_dup_end_t)));
    BWAMS_HIP(m.has.ensure((size_t)n_t));
    const unsigned long long init[2] = {~0ULL, 0};
    BWAMS_HIP(hipMemcpyAsync(m.info.p, init, 16, hipMemcpyHostToDevice, st));
    md_tmpl_kernel<<<grid_of(n_t, 256, cu_count), 256, 0, st>>>(m.rec.as<const MdRec>(), m.tstart.as<const uint32_t>(), n_t, n_rec,
                                                                m.tend.as<bwams_dup_end_t>(), m.has.as<uint8_t>(),
                                                                m.info.as<unsigned long long>());
    tb = 0;
    BWAMS_HIP(rocprim::select(nullptr, tb, m.tend.as<const bwams_dup_end_t>(), m.has.as<const uint8_t>(), m.ends.as<bwams_dup_end_t>(),
                              m.info.as<unsigned long long>() + 1, (size_t)n_t, st));
    BWAMS_HIP(m.tmp.ensure(tb));
    BWAMS_HIP(rocprim::select(m.tmp.p, tb, m.tend.as<const bwams_dup_end_t>(), m.has.as<const uint8_t>(), m.ends.as<bwams_dup_end_t>(),
                              m.info.as<unsigned long long>() + 1, (size_t)n_t, st));
    unsigned long long info[2];
    BWAMS_HIP(hipMemcpyAsync(info, m.info.p, 16, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    if (info[0] != ~0ULL) {
        set_last_error("bwams_bam_templates: record " + std::to_string(info[0] >> 2) + ": " + kReason[info[0] & 3]);
        return BWAMS_ERR_UNSUPPORTED;
    }
    m.n_t = n_t;
    m.n_e = (int64_t)info[1];
    return BWAMS_OK;
}

int md_decide(MdDecide &w, const bwams_dup_end_t *ends, int64_t n_e, int64_t n_t, uint8_t *dup, int64_t counts[3], int cu_count,
              hipStream_t st) {
    counts[0] = counts[1] = counts[2] = 0;                   // pairs, pair duplicates, fragment duplicates
    if (n_t > 0) BWAMS_HIP(hipMemsetAsync(dup, 0, (size_t)n_t, st));
    if (n_e == 0) return BWAMS_OK;
    if (n_e > 0x7FFFFFFFLL || n_t >= (1LL << 47)) {
        set_last_error("bwams_dup_decide: more than 2^31 - 1 ends or 2^47 templates");
        return BWAMS_ERR_UNSUPPORTED;
    }
    const size_t n2 = 2 * (size_t)n_e;
    BWAMS_HIP(w.info.ensure(32));
    const unsigned long long init[4] = {~0ULL, 0, 0, 0};
    BWAMS_HIP(hipMemcpyAsync(w.info.p, init, 32, hipMemcpyHostToDevice, st));
    unsigned long long *info = w.info.as<unsigned long long>();
    md_check_kernel<<<grid_of(n_e, 256, cu_count), 256, 0, st>>>(ends, n_e, n_t, info);
    unsigned long long h[3];
    BWAMS_HIP(hipMemcpyAsync(h, info, 24, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    if (h[0] != ~0ULL) {
        set_last_error("bwams_dup_decide: end " + std::to_string(h[0]) + ": tmpl outside [0, n_templates), a refID outside [0, 2^30) "
                       "(ref2: -1 too), score outside [0, 32767] or strands outside [0, 3] (bit 1 without end 2)");
        return BWAMS_ERR_ARG;
    }
    const int32_t none_ref = (int32_t)h[1];                  // the largest refID + 1: slots that hold nothing
    const uint64_t none_key = (uint64_t)(uint32_t)none_ref << 33 | (uint64_t)0x80000000u << 1;
    const unsigned kb = (unsigned)(33 + bit_width((uint64_t)none_ref)), tb = (unsigned)std::max(1, bit_width((uint64_t)n_t));
    counts[0] = (int64_t)h[2];
    BWAMS_HIP(hipMemsetAsync(info + 2, 0, 16, st));           // the duplicates' counters of the two mark kernels
    BWAMS_HIP(w.k1.ensure(n2 * 8)); BWAMS_HIP(w.k2.ensure(n2 * 8)); BWAMS_HIP(w.ka.ensure(n2 * 8)); BWAMS_HIP(w.kb.ensure(n2 * 8));
    BWAMS_HIP(w.i1.ensure(n2 * 4)); BWAMS_HIP(w.i2.ensure(n2 * 4));
    uint64_t *k1 = w.k1.as<uint64_t>(), *k2 = w.k2.as<uint64_t>(), *ka = w.ka.as<uint64_t>(), *kbuf = w.kb.as<uint64_t>();
    uint32_t *i1 = w.i1.as<uint32_t>(), *i2 = w.i2.as<uint32_t>();
    size_t need = 0;
    const std::pair<size_t, unsigned> sorts[4] = {{(size_t)n_e, 15 + tb}, {(size_t)n_e, kb}, {n2, 16 + tb}, {n2, kb}};
    for (const auto &q : sorts) {
        size_t t = 0;
        BWAMS_HIP(rocprim::radix_sort_pairs(nullptr, t, ka, kbuf, i1, i2, q.first, 0u, q.second, st));
        need = std::max(need, t);
    }
    BWAMS_HIP(w.tmp.ensure(need));
    auto sort = [&](uint64_t *kin, uint32_t *vin, uint32_t *vout, size_t n, unsigned bits) {
        size_t t = need;
        return rocprim::radix_sort_pairs(w.tmp.p, t, kin, kbuf, vin, vout, n, 0u, bits, st);
    };
    const unsigned g1 = grid_of(n_e, 256, cu_count), g2 = grid_of((int64_t)n2, 256, cu_count);
    // pairs: by rank, then key 2, then key 1
    md_pair_keys_kernel<<<g1, 256, 0, st>>>(ends, n_e, none_ref, (int)tb, k1, k2, ka, i1);
    BWAMS_HIP(sort(ka, i1, i2, (size_t)n_e, 15 + tb));
    md_gather64_kernel<<<g1, 256, 0, st>>>(k2, i2, n_e, ka);
    BWAMS_HIP(sort(ka, i2, i1, (size_t)n_e, kb));
    md_gather64_kernel<<<g1, 256, 0, st>>>(k1, i1, n_e, ka);
    BWAMS_HIP(sort(ka, i1, i2, (size_t)n_e, kb));
    md_mark_pairs_kernel<<<g1, 256, 0, st>>>(kbuf, k2, i2, n_e, none_key, ends, dup, info + 2);
    // fragments: by (unpaired, rank), then the key
    md_frag_keys_kernel<<<g1, 256, 0, st>>>(ends, n_e, none_ref, (int)tb, k1, ka, i1);
    BWAMS_HIP(sort(ka, i1, i2, n2, 16 + tb));
    md_gather64_kernel<<<g2, 256, 0, st>>>(k1, i2, (int64_t)n2, ka);
    BWAMS_HIP(sort(ka, i2, i1, n2, kb));
    md_mark_frags_kernel<<<g2, 256, 0, st>>>(kbuf, i1, (int64_t)n2, none_key, ends, dup, info + 3);
    BWAMS_HIP(hipMemcpyAsync(h, info + 2, 16, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    counts[1] = (int64_t)h[0];
    counts[2] = (int64_t)h[1];
    return BWAMS_OK;
}

void launch_md_apply(uint8_t *bam, const int64_t *rec_off, const uint32_t *perm, const uint32_t *rtmpl, const uint8_t *dup, int64_t n_rec,
                     unsigned long long *n_marked, int cu_count, hipStream_t st) {
    if (n_rec > 0) md_apply_kernel<<<grid_of(n_rec, 256, cu_count), 256, 0, st>>>(bam, rec_off, perm, rtmpl, dup, n_rec, n_marked);
}

void launch_md_gather32(const uint32_t *src, const uint32_t *idx, int64_t n, uint32_t *dst, int cu_count, hipStream_t st) {
    if (n > 0) md_gather32_kernel<<<grid_of(n, 256, cu_count), 256, 0, st>>>(src, idx, n, dst);
}

}  // namespace bwams
