// ref_gather.h — one reference code from an opened index (pileup rule 7, recalibration rule 2): the forward strand's .0123 byte at
// `at` (contig offset + position), 4 where `at` lies in one of the .amb holes (hole_off ascending) or the byte is above 3.
// pileup.hip's pileup_ref_kernel and recal.hip's recal_ref_index_kernel share it.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace bwams {

__device__ __forceinline__ uint8_t ref_code_at(const uint8_t *ref0123, int64_t at, const int64_t *hole_off, const int32_t *hole_len,
                                               int32_t n_holes) {
    int32_t a = 0, b = n_holes;                                          // the holes that begin at or before `at`: [0, a)
    while (a < b) {
        const int32_t mid = a + (b - a) / 2;
        if (hole_off[mid] <= at) a = mid + 1;
        else b = mid;
    }
    const bool hole = a > 0 && at < hole_off[a - 1] + hole_len[a - 1];
    const uint8_t code = ref0123[at];
    return hole || code > 3 ? 4 : code;
}

}  // namespace bwams
