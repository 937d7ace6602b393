// ksw_global2_wave.h — one row of ksw_global2 (ksw.cpp:588-637) with the whole wavefront on it: 64 columns per step.
//
// Within a row E and the diagonal term come from the row above, and F — max over the columns to the left of (M - gap open)
// minus the extensions in between — is a prefix maximum (ksw_global2 feeds F from M only, never from H: ksw.cpp:607-623), so
// the cells of a row are independent but for that scan and the scores are the serial loop's, cell for cell.  The callers
// (dedup.hip: score only; reg2aln.hip: with the direction bytes of the traceback) keep what differs between them: where the
// row's target base comes from, the first row, the row loop and its barrier.
#pragma once
#include "common.h"
#include "wave_ops.h"

namespace bwams {

constexpr int kMinusInf = -0x40000000;           // MINUS_INF of ksw.cpp
constexpr int kScanMasked = -2000000000;         // what a lane outside the row puts into the prefix maximum: below every f a row can hold

// the row of the scoring matrix as five bytes of one scalar: a lane's score is a shift and a sign extension
__device__ __forceinline__ uint64_t ksw_mat_row(const int8_t *mrow) {
    return (uint64_t)(uint8_t)mrow[0] | (uint64_t)(uint8_t)mrow[1] << 8 | (uint64_t)(uint8_t)mrow[2] << 16 |
           (uint64_t)(uint8_t)mrow[3] << 24 | (uint64_t)(uint8_t)mrow[4] << 32;
}

// Row i of band w: the columns [beg, end) of eh (LDS; (h, e) of the row above in, of this row out, eh[end] included) against
// the query bytes q (LDS).  All 64 lanes call this with wave-uniform i, w, qlen, mpk = ksw_mat_row of the row's target base
// and the gap-open sums oe_del = o_del + e_del, oe_ins = o_ins + e_ins, which the caller forms once, before its row loop; the caller puts a barrier between two rows.  TRACE: column j's direction byte goes to zi[j - beg].
// Branch-free but for the stores; lanes behind the row's end read its last column and are masked out of the scan.  Cross-lane
// moves are DPP (the neighbour) and v_readlane (lane 63, the row's last column): no LDS permutes.
template <bool TRACE>
__device__ __forceinline__ void ksw_global2_row_wave(const bwams_mem_opt_t &o, int oe_del, int oe_ins, uint64_t mpk, int i, int w,
                                                     int qlen, int2 *eh, const uint8_t *q, int lane, uint8_t *zi) {
    const int beg = i > w ? i - w : 0;
    const int end = i + w + 1 < qlen ? i + w + 1 : qlen;
    const int h1_first = beg == 0 ? -(o.o_del + o.e_del * (i + 1)) : kMinusInf;
    int f_carry = kMinusInf, h_carry = h1_first, h_end = h1_first;
    for (int c0 = beg; c0 < end; c0 += 64) {
        const int j = c0 + lane;
        const bool act = j < end;
        const int jj = act ? j : end - 1;
        const int2 p = eh[jj];
        int qb = q[jj];
        qb = qb > 4 ? 4 : qb;
        const int m = p.x + (int)(int8_t)(uint8_t)(mpk >> (qb << 3));
        int e = p.y;
        const int t_ins = m - oe_ins;
        const int g = act ? t_ins + j * o.e_ins : kScanMasked;
        const int P = scan_max(g);
        const int Pex = lane_shr1(P, kScanMasked);     // lane 0: nothing to its left in this chunk
        const int fc = f_carry - lane * o.e_ins;       // what the gap open before this chunk has become
        const int fp = Pex - (j - 1) * o.e_ins;
        const int f = fc > fp ? fc : fp;
        uint32_t d = m >= e ? 0u : 1u;
        int h = m >= e ? m : e;
        d = h >= f ? d : 2u;
        h = h >= f ? h : f;
        const int t = m - oe_del;
        e -= o.e_del;
        d |= e > t ? 1u << 2 : 0u;
        e = e > t ? e : t;
        const int fn = f - o.e_ins;
        d |= fn > t_ins ? 2u << 4 : 0u;
        const int hl = lane_shr1(h, h_carry);          // lane 0 takes the previous chunk's last h
        if (act) {
            eh[j] = make_int2(hl, e);
            if constexpr (TRACE) zi[j - beg] = (uint8_t)d;
        }
        const int fnext = fn > t_ins ? fn : t_ins;
        f_carry = __builtin_amdgcn_readlane(fnext, 63);
        h_carry = __builtin_amdgcn_readlane(h, 63);
        const int last = end - 1 - c0;                 // the row's last column, if it lies in this chunk
        if (last < 64) h_end = __builtin_amdgcn_readlane(h, last);
    }
    if (lane == 0) eh[end] = make_int2(h_end, kMinusInf);
}

}  // namespace bwams
