// region_sort.h — the region sorts: ksort.h's introsort (csrc/ksort.h, the algorithm) over 24-byte sort records with the
// orders of mem_sort_dedup_patch (bwamem.cpp:176-180), mem_mark_primary_se, mem_pair and the ERT walk.
// Used by dedup.hip, pair.hip and ert_chain.hip.
#pragma once
#include "ksort.h"

namespace bwams {
namespace {

struct SortRec { int64_t k; int32_t s, q, idx; int32_t pad_; };      // ars2: k = re; ars: k = rb, s = score, q = qb

struct LtEnd   { __device__ __forceinline__ bool operator()(const SortRec &a, const SortRec &b) const { return a.k < b.k; } };
struct LtScore { __device__ __forceinline__ bool operator()(const SortRec &a, const SortRec &b) const {
    return a.s > b.s || (a.s == b.s && (a.k < b.k || (a.k == b.k && a.q < b.q))); } };

// mem_mark_primary_se's two orders (alnreg_hlt / alnreg_hlt2, bwamem.cpp:182-186): k = hash (unsigned), s = score, q = is_alt
struct LtHash  { __device__ __forceinline__ bool operator()(const SortRec &a, const SortRec &b) const {
    return a.s > b.s || (a.s == b.s && (a.q < b.q || (a.q == b.q && (uint64_t)a.k < (uint64_t)b.k))); } };
struct LtHash2 { __device__ __forceinline__ bool operator()(const SortRec &a, const SortRec &b) const {
    return a.q < b.q || (a.q == b.q && (a.s > b.s || (a.s == b.s && (uint64_t)a.k < (uint64_t)b.k))); } };
// pair64_lt (utils.cpp:45) with x = k and y = (s, q), both halves non-negative
struct LtXY    { __device__ __forceinline__ bool operator()(const SortRec &a, const SortRec &b) const {
    return a.k < b.k || (a.k == b.k && (a.s < b.s || (a.s == b.s && a.q < b.q))); } };

// smem_lt_2 (bwamem.cpp:73): MEMs of the ERT walk by (start, end); k = start, s = end
struct LtStartEnd { __device__ __forceinline__ bool operator()(const SortRec &a, const SortRec &b) const {
    return a.k == b.k ? a.s < b.s : a.k < b.k; } };

struct SortRecPad {                                                   // what fills a sorting network up to a power of two
    __device__ __forceinline__ SortRec make() const { SortRec x; x.k = 0; x.s = 0; x.q = 0; x.idx = 0; x.pad_ = 1; return x; }
    __device__ __forceinline__ bool is(const SortRec &x) const { return x.pad_ != 0; }
};

// The sorts are called through this non-inlined wrapper: the pointer stays generic (LDS or HBM, flat accesses).
// Instantiated directly on a __shared__ array the inlined introsort spun forever on gfx950 (ROCm 7.2) for a
// six-record input that the same code sorts correctly through a generic pointer; see profiles/r01_notes.md.
__device__ __noinline__ void sort_records(SortRec *a, int n, int by_score, int depth0 = 0) {
    switch (by_score) {
    case 0: ks_introsort(a, n, LtEnd(), depth0); break;
    case 1: ks_introsort(a, n, LtScore(), depth0); break;
    case 2: ks_introsort(a, n, LtHash()); break;
    case 3: ks_introsort(a, n, LtHash2()); break;
    case 4: ks_introsort(a, n, LtXY()); break;
    default: ks_introsort(a, n, LtStartEnd()); break;
    }
}

// The same sorts for a one-wavefront block with the records in LDS: a rank sort or, beyond 96 records, the bitonic network,
// which give the unique sorted order — and hence ksort.h's — whenever no two records compare equal; if some do, the wave
// runs the operation-exact introsort (wave_ks_introsort) on the untouched input instead.  All 64 lanes call this; a and tmp
// hold n records each.  (Round 1 sent lane 0 alone into the sequential introsort here while 63 lanes waited at the barrier:
// the configuration in which an inlined LDS instantiation once hung, profiles/r01_notes.md 20.  No lane-0-only sort call
// on LDS is left in the wave tiers: the depth-limit fallback is wave_ks_combsort.)
// force_exact: take the operation-exact path even when no two keys are equal (tests); depth0: see ks_introsort
// cap: records tmp holds (a power of two at or above n lets the bitonic pass run)
__device__ __forceinline__ void wave_sort_records(SortRec *a, SortRec *tmp, int n, int by_score, int lane, bool force_exact = false, int depth0 = 0,
                                                  int cap = 0) {
    __shared__ int l_sort_stk[120];
    if (n < 2) return;
    bool tie = true;
    int P = 128;
    while (P < n) P <<= 1;
    if (!force_exact) {
        if (n > 96 && P <= cap) tie = by_score ? wave_bitonic_pass(a, tmp, n, P, lane, LtScore(), SortRecPad()) : wave_bitonic_pass(a, tmp, n, P, lane, LtEnd(), SortRecPad());
        else tie = by_score ? wave_rank_pass(a, tmp, n, lane, LtScore()) : wave_rank_pass(a, tmp, n, lane, LtEnd());
    }
    __syncthreads();
    if (!tie) {
        for (int i = lane; i < n; i += 64) a[i] = tmp[i];
        __syncthreads();
    } else if (by_score) {
        wave_ks_introsort(a, n, tmp, l_sort_stk, lane, LtScore(), KsRankClose(), depth0);
    } else {
        wave_ks_introsort(a, n, tmp, l_sort_stk, lane, LtEnd(), KsRankClose(), depth0);
    }
}

}  // namespace
}  // namespace bwams
