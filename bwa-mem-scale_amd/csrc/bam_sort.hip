// bam_sort.hip — a batch's BAM records in coordinate order, sorted where they lie (bwams_bam_sort).
//
// The order is bwams_bam_coord_t's key (include/bwams_types.h): refID (-1 last), POS, the reverse-strand bit; ties keep their input
// order.  Three launches and a rocPRIM sort, all memory-bound:
//   bam_sort_key_kernel     lane per record: reads refID, POS, FLAG and the CIGAR at rec_off[r], writes the published coord (key,
//                           end, size) and the DEVICE key, in which refID -1 is n_ref, so that the radix sort runs over
//                           32 + bit_width(n_ref) bits instead of 64 (the published key keeps 0xFFFFFFFF);
//   rocprim::radix_sort_pairs (device key, record index): stable, as the order needs;
//   bam_sort_permute_kernel lane per sorted slot: the coord of its record, and its size for the exclusive scan (scan_rows);
//   bam_sort_gather_kernel  sixteen lanes per record copy it from rec_off[idx[i]] to new_off[i] (rec_gather.h's copy_record: aligned
//                           16-byte stores built from aligned dword loads).  Every byte is read once and written once.
// A record's bytes are only written inside its own range, so the head and tail bytes, which share a dword with the next record,
// never race.  The source buffer holds 16 bytes of slack past its last record (bwams_bam_run / _upload allocate it), so the
// aligned loads that reach past a record's end stay in bounds.
#include <algorithm>
#include <cstring>
#include "common.h"
#include "bam_rec.h"
#include "rec_gather.h"

namespace bwams {
namespace {

__global__ void __launch_bounds__(256) bam_sort_key_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, uint32_t n_ref,
                                                           bwams_bam_coord_t *coord, uint64_t *dkey, uint32_t *idx) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t *p = bam + rec_off[r];
        const bwams_bam_coord_t cd = bam_coord(p);
        const int32_t rid = (int32_t)(cd.key >> 32);
        const uint64_t low = cd.key & 0xFFFFFFFFu;
        coord[r] = cd;
        dkey[r] = (uint64_t)(rid < 0 ? n_ref : (uint32_t)rid) << 32 | low;
        idx[r] = (uint32_t)r;
    }
}

__global__ void __launch_bounds__(256) bam_sort_permute_kernel(const bwams_bam_coord_t *coord, const uint32_t *idx, int64_t n_rec,
                                                               bwams_bam_coord_t *coord_out, int64_t *size) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rec; i += (int64_t)gridDim.x * blockDim.x) {
        const bwams_bam_coord_t cd = coord[idx[i]];
        coord_out[i] = cd;
        size[i] = cd.size;
    }
}

__global__ void __launch_bounds__(256) bam_sort_gather_kernel(const uint8_t *src, const int64_t *rec_off, const uint32_t *idx,
                                                              const int64_t *new_off, int64_t n_rec, uint8_t *dst) {
    const int g = (int)(threadIdx.x & (kGroup - 1));
    const int64_t n_groups = (int64_t)gridDim.x * (blockDim.x / kGroup);
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup; i < n_rec; i += n_groups) {
        const int64_t s = rec_off[idx[i]], d = new_off[i], n = new_off[i + 1] - d;
        copy_record(src + s, dst + d, n, g);
    }
}

}  // namespace

int bam_sort_bits(uint32_t n_ref) {                          // bits of the device key: POS + 1 and the strand, then refID in [0, n_ref]
    int w = 0;
    while (w < 32 && (n_ref >> w) != 0) ++w;
    return 32 + w;
}

void launch_bam_sort_keys(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, uint32_t n_ref, bwams_bam_coord_t *coord,
                          uint64_t *dkey, uint32_t *idx, int cu_count, hipStream_t st) {
    if (n_rec > 0) bam_sort_key_kernel<<<grid_of(n_rec, 256, cu_count), 256, 0, st>>>(bam, rec_off, n_rec, n_ref, coord, dkey, idx);
}

void launch_bam_sort_permute(const bwams_bam_coord_t *coord, const uint32_t *idx, int64_t n_rec, bwams_bam_coord_t *coord_out,
                             int64_t *size, int cu_count, hipStream_t st) {
    if (n_rec > 0) bam_sort_permute_kernel<<<grid_of(n_rec, 256, cu_count), 256, 0, st>>>(coord, idx, n_rec, coord_out, size);
}

void launch_bam_sort_gather(const uint8_t *src, const int64_t *rec_off, const uint32_t *idx, const int64_t *new_off, int64_t n_rec,
                            uint8_t *dst, int cu_count, hipStream_t st) {
    if (n_rec > 0)
        bam_sort_gather_kernel<<<grid_of(n_rec, 256 / kGroup, cu_count), 256, 0, st>>>(src, rec_off, idx, new_off, n_rec, dst);
}

}  // namespace bwams
