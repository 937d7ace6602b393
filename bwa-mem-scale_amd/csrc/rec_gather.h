// rec_gather.h — the byte-exact copy of one BAM record by the kGroup lanes that share it, one definition for the kernels that move
// whole records (bam_sort.hip's gather, collate.hip's copies): the head bytes up to the next 16-byte boundary of the destination and
// the tail bytes one a lane; the body as aligned 16-byte stores, each built from aligned dword loads of the source shifted into
// place (v_alignbyte), since records are not 4-byte aligned in general.  Every byte is read once and written once.
// Only dst[0, n) is written, so the head and tail bytes, which share a dword with the neighbouring records, never race.  The aligned
// loads reach up to 16 bytes past src + n: the source buffer holds that much slack behind its last record.
#pragma once
#include <algorithm>
#include "bam_rec.h"

namespace bwams {

// g: the lane's place in its group; every lane of the group calls
__device__ __forceinline__ void copy_record(const uint8_t *src, uint8_t *dst, int64_t n, int g) {
    const int64_t head = std::min<int64_t>((16 - (int64_t)(reinterpret_cast<uintptr_t>(dst) & 15)) & 15, n);
    const int64_t body = (n - head) & ~(int64_t)15;
    const int64_t tail = n - head - body;
    if (g < head) dst[g] = src[g];
    if (g < tail) dst[head + body + g] = src[head + body + g];
    const uint8_t *s0 = src + head;                          // source of the body's first byte
    const unsigned a = (unsigned)(reinterpret_cast<uintptr_t>(s0) & 3);
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(s0 - a);
    uint4 *dw = reinterpret_cast<uint4 *>(dst + head);
    for (int64_t k = g; k < body / 16; k += kGroup) {
        const uint32_t *q = sw + 4 * k;
        uint4 v;
        if (a == 0) {
            v.x = q[0]; v.y = q[1]; v.z = q[2]; v.w = q[3];
        } else {
            const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = q[4];
            v.x = __builtin_amdgcn_alignbyte(w1, w0, a);
            v.y = __builtin_amdgcn_alignbyte(w2, w1, a);
            v.z = __builtin_amdgcn_alignbyte(w3, w2, a);
            v.w = __builtin_amdgcn_alignbyte(w4, w3, a);
        }
        dw[k] = v;
    }
}

}  // namespace bwams
