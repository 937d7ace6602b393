// bam_rec.h — one BAM alignment record as the kernels read it: p points at its block_size, every field is little-endian
// and no field is aligned (SAM specification, section 4.2).
#pragma once
#include "common.h"

namespace bwams {

constexpr int kGroup = 16;                    // lanes that share a record in the kernels that copy or sum over its bytes

__device__ __forceinline__ uint32_t ld_u16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
__device__ __forceinline__ uint32_t ld_u32(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// the fixed fields
__device__ __forceinline__ uint32_t bam_block_size(const uint8_t *p) { return ld_u32(p); }       // the record without these four bytes
__device__ __forceinline__ int32_t bam_ref_id(const uint8_t *p) { return (int32_t)ld_u32(p + 4); }
__device__ __forceinline__ int32_t bam_pos(const uint8_t *p) { return (int32_t)ld_u32(p + 8); }
__device__ __forceinline__ uint32_t bam_l_name(const uint8_t *p) { return p[12]; }               // with the NUL
__device__ __forceinline__ uint32_t bam_mapq(const uint8_t *p) { return p[13]; }
__device__ __forceinline__ uint32_t bam_n_cig(const uint8_t *p) { return ld_u16(p + 16); }
__device__ __forceinline__ uint32_t bam_flag(const uint8_t *p) { return ld_u16(p + 18); }
__device__ __forceinline__ int32_t bam_l_seq(const uint8_t *p) { return (int32_t)ld_u32(p + 20); }
__device__ __forceinline__ int32_t bam_next_ref_id(const uint8_t *p) { return (int32_t)ld_u32(p + 24); }
__device__ __forceinline__ int32_t bam_next_pos(const uint8_t *p) { return (int32_t)ld_u32(p + 28); }
__device__ __forceinline__ int32_t bam_tlen(const uint8_t *p) { return (int32_t)ld_u32(p + 32); }
__device__ __forceinline__ int64_t bam_end(const uint8_t *p) { return 4 + (int64_t)bam_block_size(p); }   // the record's end, as an offset from p
// where the variable-length fields start, as offsets from p
constexpr int kBamName = 36;
__device__ __forceinline__ int64_t bam_cigar_at(uint32_t l_name) { return kBamName + (int64_t)l_name; }
__device__ __forceinline__ int64_t bam_seq_at(uint32_t l_name, uint32_t n_cig) { return bam_cigar_at(l_name) + 4 * (int64_t)n_cig; }
__device__ __forceinline__ int64_t bam_qual_at(uint32_t l_name, uint32_t n_cig, int64_t l_seq) { return bam_seq_at(l_name, n_cig) + (l_seq + 1) / 2; }
__device__ __forceinline__ int64_t bam_aux_at(uint32_t l_name, uint32_t n_cig, int64_t l_seq) { return bam_qual_at(l_name, n_cig, l_seq) + l_seq; }

// QUAL is there: its first byte is not 0xFF (l_seq > 0)
__device__ __forceinline__ bool bam_has_qual(const uint8_t *p, uint32_t l_name, uint32_t n_cig, int64_t l_seq) {
    return p[bam_qual_at(l_name, n_cig, l_seq)] != 0xFF;
}

// SEQ: the 4-bit code of base i; A C G T (codes 1 2 4 8) as 0..3, -1 for any other code
__device__ __forceinline__ uint32_t seq_code(const uint8_t *seq, int32_t i) { return (seq[i >> 1] >> ((i & 1) ? 0 : 4)) & 15; }
__device__ __forceinline__ int base_of_code(uint32_t code) { return code == 1 ? 0 : code == 2 ? 1 : code == 4 ? 2 : code == 8 ? 3 : -1; }

// CIGAR op codes: the ones that take reference positions (M D N = X), query bases (M I S = X), both as a match or mismatch (M = X)
__device__ __forceinline__ bool op_takes_ref(uint32_t o) { return o == 0 || o == 2 || o == 3 || o == 7 || o == 8; }
__device__ __forceinline__ bool op_takes_query(uint32_t o) { return o == 0 || o == 1 || o == 4 || o == 7 || o == 8; }
__device__ __forceinline__ bool op_is_match(uint32_t o) { return o == 0 || o == 7 || o == 8; }

// reference bases the CIGAR operations first, first + stride, ... of c[0, n_cig) cover
__device__ __forceinline__ int64_t cigar_ref_len(const uint8_t *c, uint32_t n_cig, uint32_t first, uint32_t stride) {
    int64_t rlen = 0;
    for (uint32_t k = first; k < n_cig; k += stride) {
        const uint32_t op = ld_u32(c + 4 * k), o = op & 15;
        if (op_takes_ref(o)) rlen += op >> 4;
    }
    return rlen;
}


// a record's place in coordinate order and the end reg2bin takes (bwams_bam_coord_t, include/bwams_types.h)
__device__ __forceinline__ bwams_bam_coord_t bam_coord(const uint8_t *p) {
    const int32_t rid = bam_ref_id(p), pos = bam_pos(p);
    const uint32_t n_cig = bam_n_cig(p), flag = bam_flag(p);
    const int64_t rlen = cigar_ref_len(p + bam_cigar_at(bam_l_name(p)), n_cig, 0, 1);
    const int64_t end = ((flag & 4) || n_cig == 0 || rlen == 0) ? (int64_t)pos + 1 : (int64_t)pos + rlen;
    bwams_bam_coord_t cd;
    cd.key = (uint64_t)(uint32_t)rid << 32 | (uint64_t)(uint32_t)(pos + 1) << 1 | ((flag >> 4) & 1);
    cd.end = (int32_t)end;
    cd.size = (int32_t)(bam_block_size(p) + 4);
    return cd;
}

}  // namespace bwams
