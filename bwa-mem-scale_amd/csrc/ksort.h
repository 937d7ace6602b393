// ksort.h — the reference's ksort.h introsort (ks_introsort: median-of-3 quicksort, 16-element cut-off, combsort fallback,
// final insertion sort; src/ksort.h there), operation by operation, over any record type T with a comparator LT: the sort
// is unstable, so only the same sequence of comparisons and swaps leaves tied records in the reference's order.  Every
// device sort is an instantiation of this file: the region sorts (region_sort.h, 24-byte SortRec) and the chain filter's
// (chain_dev.h, uint2 {weight, id}).  Each form exists twice: sequential (one lane, HBM pointers) and whole-wavefront (LDS).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bwams {
namespace {

// ---- sequential ------------------------------------------------------------------------------------------------------
template <class T, class LT> __device__ __forceinline__ void ks_insertsort(T *a, int s, int t, LT lt) {
    for (int i = s + 1; i < t; ++i)
        for (int j = i; j > s && lt(a[j], a[j - 1]); --j) { const T x = a[j]; a[j] = a[j - 1]; a[j - 1] = x; }
}
template <class T, class LT> __device__ __forceinline__ void ks_combsort(T *a, int n, LT lt) {
    const double shrink = 1.2473309501039786540366528676643;
    bool do_swap;
    unsigned long long gap = (unsigned long long)n;
    do {
        if (gap > 2) {
            gap = (unsigned long long)((double)gap / shrink);
            if (gap == 9 || gap == 10) gap = 11;
        }
        do_swap = false;
        for (long long i = 0; i < (long long)n - (long long)gap; ++i) {
            const long long j = i + (long long)gap;
            if (lt(a[j], a[i])) { const T x = a[i]; a[i] = a[j]; a[j] = x; do_swap = true; }
        }
    } while (do_swap || gap > 2);
    if (gap != 1) ks_insertsort(a, 0, n, lt);
}
// depth0 > 0 replaces the 2 ceil(log2 n) depth budget (tests reach the comb-sort fallback on any input with it)
// STK: entries of the explicit stack.  Only a part of more than 16 elements is ever pushed, so a caller that knows n <= 17 passes 1
// and keeps the three arrays (480 B per lane) out of scratch memory.
template <int STK = 40, class T, class LT> __device__ __forceinline__ void ks_introsort(T *a, int n, LT lt, int depth0 = 0) {
    if (n < 1) return;
    if (n == 2) { if (lt(a[1], a[0])) { const T x = a[0]; a[0] = a[1]; a[1] = x; } return; }
    int d;
    for (d = 2; (1ul << d) < (unsigned long)n; ++d);
    int stk_l[STK], stk_r[STK], stk_d[STK], top = 0;
    int s = 0, t = n - 1;
    d <<= 1;
    if (depth0 > 0) d = depth0;
    for (;;) {
        if (s < t) {
            if (--d == 0) { ks_combsort(a + s, t - s + 1, lt); t = s; continue; }
            int i = s, j = t, k = i + ((j - i) >> 1) + 1;
            if (lt(a[k], a[i])) { if (lt(a[k], a[j])) k = j; }
            else k = lt(a[j], a[i]) ? i : j;
            const T rp = a[k];
            if (k != t) { a[k] = a[t]; a[t] = rp; }
            for (;;) {
                do ++i; while (lt(a[i], rp));
                do --j; while (i <= j && lt(rp, a[j]));
                if (j <= i) break;
                const T x = a[i]; a[i] = a[j]; a[j] = x;
            }
            { const T x = a[i]; a[i] = a[t]; a[t] = x; }
            if (i - s > t - i) {
                if (i - s > 16) { stk_l[top] = s; stk_r[top] = i - 1; stk_d[top] = d; ++top; }
                s = t - i > 16 ? i + 1 : t;
            } else {
                if (t - i > 16) { stk_l[top] = i + 1; stk_r[top] = t; stk_d[top] = d; ++top; }
                t = i - s > 16 ? i - 1 : s;
            }
        } else {
            if (top == 0) { ks_insertsort(a, 0, n, lt); return; }
            --top; s = stk_l[top]; t = stk_r[top]; d = stk_d[top];
        }
    }
}

// ---- whole wavefront (all 64 lanes call these; a and the scratch in LDS) ---------------------------------------------
// The stable sort of a[0 .. n): every lane counts, from uniform LDS reads, the records that sort before its own (equal ones
// by position), writes its record to that place in tmp (n records) and the wave copies tmp back.  An insertion sort over
// the whole array is a stable sort, and a stable sort's result is unique: this is what ks_introsort and ks_combsort end with.
template <class T, class LT> __device__ __forceinline__ void wave_ks_stable_rank(T *a, int n, T *tmp, int lane, LT lt) {
    for (int x0 = 0; x0 < n; x0 += 64) {
        const int x = x0 + lane;
        if (x < n) {
            const T v = a[x];
            int pos = 0;
            for (int y = 0; y < n; ++y) {
                const T w = a[y];
                pos += (lt(w, v) || (!lt(v, w) && y < x)) ? 1 : 0;
            }
            tmp[pos] = v;
        }
    }
    __syncthreads();
    for (int x = lane; x < n; x += 64) a[x] = tmp[x];
    __syncthreads();
}
// wave_ks_introsort's default closing sort; scratch holds n records
struct KsRankClose {
    template <class T, class LT> __device__ __forceinline__ void operator()(T *a, int n, void *scratch, int lane, LT lt) const {
        wave_ks_stable_rank(a, n, reinterpret_cast<T *>(scratch), lane, lt);
    }
};

// ks_combsort operation by operation with the whole wavefront (tmp = n records of LDS scratch).  A pass with gap g compares
// (i, i + g) for i = 0 .. n - g - 1 in order; position i + g may have been written by the comparison at i - g, never by any
// other, so the pass is g independent chains (the residue classes of i mod g), each walked in order by one lane: the same
// compare-and-swap sequence per chain, hence the same array after the pass.  Gaps shrink to 2 (two lanes), where the loop
// repeats until a pass swaps nothing; ks_combsort then finishes with its insertion sort — a stable sort of what the passes
// left, i.e. the rank sort above.  This is introsort's depth-limit fallback in every wave form: no lane sorts alone on LDS
// while 63 wait at a barrier (the configuration that once hung, profiles/r01_notes.md 20).
template <class T, class LT> __device__ void wave_ks_combsort(T *a, int n, T *tmp, int lane, LT lt) {
    const double shrink = 1.2473309501039786540366528676643;
    unsigned long long gap = (unsigned long long)n;
    bool do_swap;
    do {
        if (gap > 2) {
            gap = (unsigned long long)((double)gap / shrink);
            if (gap == 9 || gap == 10) gap = 11;
        }
        const int g = (int)gap;
        bool sw = false;
        for (int r = lane; r < g; r += 64)
            for (int i = r; i + g < n; i += g)
                if (lt(a[i + g], a[i])) { const T x = a[i]; a[i] = a[i + g]; a[i + g] = x; sw = true; }
        __syncthreads();
        do_swap = __ballot(sw) != 0;
    } while (do_swap || gap > 2);
    if (gap != 1) wave_ks_stable_rank(a, n, tmp, lane, lt);
}

// ks_introsort operation by operation, but with the whole wavefront on every step.  The Hoare partition of a range [s, t]
// around the pivot rp (moved to a[t]) is determined by two lists: the "up stoppers" (x in s+1..t, ascending, with
// !lt(a[x], rp)) and the "down stoppers" (x in t-1..s+1, descending, with !lt(rp, a[x])); the scalar loop swaps the k-th up
// stopper with the k-th down stopper while the former lies below the latter (positions already swapped are never scanned
// again), m swaps in all, and the pivot lands on min(up[m], down[m-1]).  The lists are built with ballots, the swaps are
// independent.  The control flow between partitions (median of three, explicit stack, depth budget) is ksort's own.
// close(a, n, scratch, lane, lt) is the closing insertion sort over the whole array, i.e. THE stable sort of what the
// partitions left (not a local clean-up: ksort's median of three never examines a[s], so the element may lie far from its
// place and a windowed pass would be wrong).  The default is the rank sort; a caller with a faster stable sort passes its own.
// Scratch (LDS): the stopper lists are 2 n uint16_t at its start — hence n <= 65535 — and are dead whenever anything else
// uses it: the comb-sort fallback of the depth limit (wave_ks_combsort) writes at most n records from its start, and so
// does the default close.  stk = 120 ints of LDS that neither touches while the partitions run (it may lie in scratch
// behind n records).  depth0: see ks_introsort.
template <class T, class LT, class Close = KsRankClose>
__device__ void wave_ks_introsort(T *a, int n, void *scratch, int *stk, int lane, LT lt, Close close = Close(), int depth0 = 0) {
    if (n < 2) return;
    if (n == 2) {
        if (lane == 0 && lt(a[1], a[0])) { const T x = a[0]; a[0] = a[1]; a[1] = x; }
        __syncthreads();
        return;
    }
    uint16_t *ls = reinterpret_cast<uint16_t *>(scratch), *rs = ls + n;
    int d;
    for (d = 2; (1ul << d) < (unsigned long)n; ++d);
    int top = 0, s = 0, t = n - 1;
    d <<= 1;
    if (depth0 > 0) d = depth0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (;;) {
        if (s < t) {
            if (--d == 0) {
                __syncthreads();
                wave_ks_combsort(a + s, t - s + 1, reinterpret_cast<T *>(scratch), lane, lt);
                t = s;
                continue;
            }
            int i = s, j = t, k = i + ((j - i) >> 1) + 1;
            {
                const T ak = a[k], ai = a[i], aj = a[j];
                if (lt(ak, ai)) { if (lt(ak, aj)) k = j; }
                else k = lt(aj, ai) ? i : j;
            }
            const T rp = a[k];
            __syncthreads();
            if (lane == 0 && k != t) { a[k] = a[t]; a[t] = rp; }
            __syncthreads();
            int NL = 0, NR = 0;
            for (int x0 = s + 1; x0 <= t; x0 += 64) {
                const int x = x0 + lane;
                const bool f = x <= t && !lt(a[x], rp);
                const unsigned long long m = __ballot(f);
                if (f) ls[NL + __popcll(m & below)] = (uint16_t)x;
                NL += __popcll(m);
            }
            for (int x0 = t - 1; x0 >= s + 1; x0 -= 64) {
                const int x = x0 - lane;
                const bool f = x >= s + 1 && !lt(rp, a[x]);
                const unsigned long long m = __ballot(f);
                if (f) rs[NR + __popcll(m & below)] = (uint16_t)x;
                NR += __popcll(m);
            }
            __syncthreads();
            const int np = NL < NR ? NL : NR;
            int m_sw = 0;
            for (int k0 = 0; k0 < np; k0 += 64) {
                const int kk = k0 + lane;
                m_sw += __popcll(__ballot(kk < np && ls[kk] < rs[kk]));
            }
            for (int k0 = 0; k0 < m_sw; k0 += 64) {
                const int kk = k0 + lane;
                if (kk < m_sw) { const int p = ls[kk], q = rs[kk]; const T x = a[p]; a[p] = a[q]; a[q] = x; }
            }
            int i_f = ls[m_sw];                      // up[m] exists: t itself is an up stopper
            if (m_sw >= 1 && (int)rs[m_sw - 1] < i_f) i_f = rs[m_sw - 1];
            __syncthreads();
            if (lane == 0) { const T x = a[i_f]; a[i_f] = a[t]; a[t] = x; }
            __syncthreads();
            i = i_f;
            if (i - s > t - i) {
                if (i - s > 16) { stk[3 * top] = s; stk[3 * top + 1] = i - 1; stk[3 * top + 2] = d; ++top; }
                s = t - i > 16 ? i + 1 : t;
            } else {
                if (t - i > 16) { stk[3 * top] = i + 1; stk[3 * top + 1] = t; stk[3 * top + 2] = d; ++top; }
                t = i - s > 16 ? i - 1 : s;
            }
            __syncthreads();                         // the stack entries were written by every lane (same values)
        } else {
            if (top == 0) break;
            --top; s = stk[3 * top]; t = stk[3 * top + 1]; d = stk[3 * top + 2];
        }
    }
    __syncthreads();
    close(a, n, scratch, lane, lt);                  // the stopper lists and the stack are dead by now
}

// ---- sorting networks over LDS, for keys of which no two are equal (or whose ties are detected afterwards) -----------
// The bitonic sorter over P = 2^p slots: for every stage (k, j) the wave calls cx(i, l, up) once for each comparator
// (i, l = i | j), up = the pair is to end ascending, with a barrier after the stage.  cx does the compare-exchange, in
// whatever layout the keys have.
template <class CX> __device__ __forceinline__ void wave_bitonic_net(int P, int lane, CX cx) {
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (P >> 1); t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));          // j is a power of two
                cx(i, i | j, (i & k) == 0);
            }
            __syncthreads();
        }
}

// A rank sort into tmp: every lane counts the records that sort before its own (O(n^2 / 64) LDS reads, no dependent chain),
// which is the unique sorted order — and hence ksort.h's — whenever no two records compare equal.  Returns whether two do
// (then tmp is not to be used: the caller runs the operation-exact sort on the untouched a).  a and tmp hold n records.
template <class T, class LT> __device__ __forceinline__ bool wave_rank_pass(const T *a, T *tmp, int n, int lane, LT lt) {
    bool tie = false;
    for (int ib = 0; ib < n; ib += 64) {
        const int i = ib + lane;
        int eq = 0;
        if (i < n) {
            const T x = a[i];
            int rank = 0;
            for (int j = 0; j < n; ++j) {
                const T y = a[j];
                const bool l = lt(y, x);
                rank += l ? 1 : 0;
                eq += (!l && !lt(x, y)) ? 1 : 0;
            }
            tmp[rank] = x;                                   // collisions only with equal records (then tmp is not used)
        }
        tie = tie || (__ballot(eq > 1) != 0);
    }
    return tie;
}
// The same contract for more than a few dozen records: the bitonic network over the next power of two P >= n (tmp holds P
// records; the pads — pad.make(), recognised by pad.is(x) — sort behind everything).  n log^2 n / 128 compare-exchanges per
// lane instead of n^2 / 64 comparisons: a read in a satellite array reaches de-duplication with 500 .. 2000 regions, and two
// rank sorts of those were a millisecond of a wavefront that has a CU to itself.
template <class T, class LT, class PAD> __device__ __forceinline__ bool wave_bitonic_pass(const T *a, T *tmp, int n, int P, int lane, LT lt, PAD pad) {
    for (int i = lane; i < P; i += 64) tmp[i] = i < n ? a[i] : pad.make();
    __syncthreads();
    wave_bitonic_net(P, lane, [&](int i, int l, bool up) {
        const T A = tmp[i], B = tmp[l];
        const bool b_lt_a = !pad.is(B) && (pad.is(A) || lt(B, A));
        if (b_lt_a == up) { tmp[i] = B; tmp[l] = A; }
    });
    bool tie = false;
    for (int ib = 1; ib < n; ib += 64) {
        const int i = ib + lane;
        tie = tie || (__ballot(i < n && !lt(tmp[i - 1], tmp[i])) != 0);
    }
    return tie;
}

}  // namespace
}  // namespace bwams
