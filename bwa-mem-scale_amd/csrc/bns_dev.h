// bns_dev.h — bntseq_t as the kernels see it, and the coordinate helpers every stage shares.
#pragma once
#include "common.h"

namespace bwams {

struct DevBns {
    const bwams_contig_t *contigs;
    int32_t n_seqs;
    int64_t l_pac;
};

// bns_pos2rid (bntseq.cpp:397-413): the sequence that holds forward-strand position pos_f, -1 beyond the forward strand
__device__ __forceinline__ int pos2rid(const DevBns &b, int64_t pos_f) {
    if (pos_f >= b.l_pac) return -1;
    int left = 0, mid = 0, right = b.n_seqs;
    while (left < right) {
        mid = (left + right) >> 1;
        if (pos_f >= b.contigs[mid].offset) {
            if (mid == b.n_seqs - 1) break;
            if (pos_f < b.contigs[mid + 1].offset) break;
            left = mid + 1;
        } else right = mid;
    }
    return mid;
}
// bns_depos without the strand: a position on either strand as a forward-strand position
__device__ __forceinline__ int64_t depos(const DevBns &b, int64_t pos) {
    return pos >= b.l_pac ? (b.l_pac << 1) - 1 - pos : pos;
}
// mem_infer_dir (bwamem_pair.cpp:57-65)
__device__ __forceinline__ int infer_dir(int64_t l_pac, int64_t b1, int64_t b2, int64_t *dist) {
    const int r1 = (b1 >= l_pac), r2 = (b2 >= l_pac);
    const int64_t p2 = r1 == r2 ? b2 : (l_pac << 1) - 1 - b2;
    *dist = p2 > b1 ? p2 - b1 : b1 - p2;
    return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}

}  // namespace bwams
