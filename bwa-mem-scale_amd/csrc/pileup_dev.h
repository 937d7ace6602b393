// pileup_dev.h — the device helpers that pileup.hip and pileup_indel.hip share: rule 2's filter and the two searches over the regions.
#pragma once
#include "common.h"
#include "bam_rec.h"

namespace bwams {

// rule 2, for a record at p
__device__ __forceinline__ bool record_counts(const uint8_t *p, const PileupFilter &f) {
    const int32_t rid = bam_ref_id(p);
    return !(bam_flag(p) & f.exclude) && (int32_t)bam_mapq(p) >= f.min_mapq && rid >= 0 && rid < f.n_ref && bam_n_cig(p) > 0 &&
           bam_l_seq(p) > 0;
}

// the first region of [lo, hi) whose end is above x (hi when there is none)
__device__ __forceinline__ int32_t first_region_ending_above(const PileupRegions &R, int32_t lo, int32_t hi, int64_t x) {
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if ((int64_t)R.end[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the region of slot s: the last whose first slot is at or before s
__device__ __forceinline__ int32_t region_of_slot(const PileupRegions &R, int32_t n_regions, int64_t s) {
    int32_t lo = 0, hi = n_regions - 1;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (R.off[mid] <= s) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

}  // namespace bwams
