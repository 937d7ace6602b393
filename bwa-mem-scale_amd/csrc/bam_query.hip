// bam_query.hip — the device side of a BAM file read back by region (include/bwams.h, "BAM file by region"): the records of one piece
// found, tested against the regions and copied back to back.
//   discovery   bam_discover.h, the chain from the piece's start offset over the records that begin below its stop offset; a record
//               that the end of the buffer cuts off is where the carry begins, not an error (the caller decides).
//   bq_select_kernel   a lane per record: its offset by lifting, rule 1 against the merged regions (disjoint and sorted, so their ends
//               ascend within a reference: a binary search for the first region that ends behind POS, staged in LDS when they fit),
//               the keep flag, the size, the coord (bam_coord, the sorter's) and the check of refID and POS that bwams_bam_upload makes.
//   two exclusive scans (kept bytes, kept records), bq_compact_kernel (the kept records' ordinals, offsets and coords), and the
//               sorter's gather (launch_bam_sort_gather: sixteen lanes per record, source and destination of any mutual alignment).
// The select reads 36 bytes and the CIGAR of every record, the gather reads and writes every kept byte once; the filter of the
// discovery reads the piece once.  All reads of the piece lie inside records the filter found whole inside [0, n).
#include <algorithm>

#include "bam_discover.h"

namespace bwams {
namespace {

constexpr int kSelRegionsLds = 1024;          // regions staged in LDS: 12 KB

// rule 1 over regions sorted by (ref, beg) and disjoint within a reference
__device__ __forceinline__ bool overlaps(const bwams_pileup_region_t *__restrict__ g, int32_t n, int32_t rid, int32_t pos, int32_t end) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {                         // the first region that ends behind POS
        const int32_t mid = (lo + hi) >> 1;
        const bwams_pileup_region_t x = g[mid];
        if (x.ref < rid || (x.ref == rid && x.end <= pos)) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && g[lo].ref == rid && g[lo].beg < end;
}

// wide: 2 rows of n_rec + 1 (kept bytes, kept records)
__global__ __launch_bounds__(256) void bq_select_kernel(const uint8_t *__restrict__ d, const uint32_t *__restrict__ up, int levels, uint32_t n_cand,
                                                        const int64_t *__restrict__ cand_off, uint32_t first, int64_t n_rec,
                                                        const bwams_pileup_region_t *__restrict__ regions, int32_t n_regions,
                                                        int64_t *__restrict__ src_off, bwams_bam_coord_t *__restrict__ coord,
                                                        int64_t *__restrict__ wide, unsigned long long *__restrict__ bad) {
    __shared__ bwams_pileup_region_t lds[kSelRegionsLds];
    const bool staged = n_regions <= kSelRegionsLds;
    if (staged) {
        for (int k = threadIdx.x; k < n_regions; k += blockDim.x) lds[k] = regions[k];
        __syncthreads();
    }
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rec) return;
    const int64_t n1 = n_rec + 1;
    if (r == n_rec) { wide[r] = wide[n1 + r] = 0; return; }
    const int64_t q = cand_off[br_lift(up, levels, n_cand, first, r)];
    const uint8_t *p = d + q;
    const bwams_bam_coord_t cd = bam_coord(p);
    const int32_t rid = bam_ref_id(p), pos = bam_pos(p);
    if (rid < -1 || pos < -1 || pos > 0x7FFFFFFE) atomicMin(bad, (unsigned long long)r);
    const bool keep = n_regions == 0 || overlaps(staged ? lds : regions, n_regions, rid, pos, cd.end);
    src_off[r] = q;
    coord[r] = cd;
    wide[r] = keep ? cd.size : 0;
    wide[n1 + r] = keep ? 1 : 0;
}

// offs: the scans of wide.  Kept record r is number k = offs[n1 + r]: idx[k] = r, roff[k] = offs[r], coords[k] its coord.
__global__ __launch_bounds__(256) void bq_compact_kernel(const int64_t *__restrict__ wide, const int64_t *__restrict__ offs, int64_t n_rec,
                                                         const bwams_bam_coord_t *__restrict__ coord, uint32_t *__restrict__ idx,
                                                         int64_t *__restrict__ roff, bwams_bam_coord_t *__restrict__ coords) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rec) return;
    const int64_t n1 = n_rec + 1;
    const int64_t k = offs[n1 + r];
    if (r == n_rec) { roff[k] = offs[r]; return; }
    if (!wide[n1 + r]) return;
    idx[k] = (uint32_t)r;
    roff[k] = offs[r];
    coords[k] = coord[r];
}

}  // namespace

struct BamQueryScratch {
    BrDiscover disc;
    DevBuf<int64_t> src_off, wide, offs;
    DevBuf<bwams_bam_coord_t> coord;
    DevBuf<uint32_t> idx;
    DevBuf<unsigned long long> bad;
};

BamQueryScratch *bam_query_scratch_new() { return new BamQueryScratch(); }
void bam_query_scratch_free(BamQueryScratch *s) { delete s; }

int bam_query_piece(BamQueryScratch *s, const uint8_t *d, int64_t n, int64_t start, int64_t stop, const bwams_pileup_region_t *regions,
                    int32_t n_regions, DevBuf<uint8_t> &recs, DevBuf<int64_t> &roff, DevBuf<bwams_bam_coord_t> &coords, hipEvent_t ev[4],
                    int cu_count, hipStream_t st, BamQueryResult *out) {
    *out = BamQueryResult{};
    out->at = start;
    out->bad_rec = -1;
    BWAMS_HIP(roff.ensure_n(1));
    BWAMS_HIP(recs.ensure_n(16));
    if (n <= 0 || start >= stop) {                           // a piece without a record
        BWAMS_HIP(hipMemsetAsync(roff.p, 0, 8, st));
        BWAMS_HIP(hipStreamSynchronize(st));
        return BWAMS_OK;
    }
    BWAMS_HIP(hipEventRecord(ev[0], st));
    BrEnd ch;
    if (int rc = s->disc.run(d, n, start, stop, st, &ch)) return rc;
    BWAMS_HIP(hipEventRecord(ev[1], st));
    out->n_rec = ch.n_rec; out->at = ch.at; out->n_cand = s->disc.n_cand;
    out->cut = ch.how == kBrCut; out->bad = ch.how == kBrBad; out->cut_size = ch.cut_size;
    const int64_t n_rec = ch.n_rec, n1 = n_rec + 1;
    if (n_rec >= ((int64_t)1 << 32)) {
        set_last_error("a piece of 2^32 records or more");
        return BWAMS_ERR_UNSUPPORTED;
    }
    BWAMS_HIP(s->src_off.ensure_n((size_t)n1)); BWAMS_HIP(s->coord.ensure_n((size_t)n1)); BWAMS_HIP(s->idx.ensure_n((size_t)n1));
    BWAMS_HIP(s->wide.ensure_n((size_t)n1 * 2)); BWAMS_HIP(s->offs.ensure_n((size_t)n1 * 2)); BWAMS_HIP(s->bad.ensure_n(1));
    BWAMS_HIP(roff.ensure_n((size_t)n1)); BWAMS_HIP(coords.ensure_n((size_t)n1));
    BWAMS_HIP(hipMemsetAsync(s->bad.p, 0xFF, 8, st));
    const unsigned blocks = (unsigned)((n1 + 255) / 256);
    bq_select_kernel<<<blocks, 256, 0, st>>>(d, s->disc.up.p, s->disc.levels, s->disc.n_cand, s->disc.cand_off.p, (uint32_t)ch.first, n_rec,
                                             regions, n_regions, s->src_off.p, s->coord.p, s->wide.p, s->bad.p);
    for (int row = 0; row < 2; ++row)
        if (int rc = with_tmp(s->disc.scan_tmp, st, "record selection: exclusive_scan", [&](void *tmp, size_t &tb) {
                return rocprim::exclusive_scan(tmp, tb, s->wide.p + row * n1, s->offs.p + row * n1, (int64_t)0, (size_t)n1, rocprim::plus<int64_t>(), st);
            })) return rc;
    int64_t tot[2] = {0, 0};
    unsigned long long h_bad = ~0ULL;
    for (int row = 0; row < 2; ++row) BWAMS_HIP(hipMemcpyAsync(&tot[row], s->offs.p + row * n1 + n_rec, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipMemcpyAsync(&h_bad, s->bad.p, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipEventRecord(ev[2], st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    if (h_bad != ~0ULL) {
        out->bad_rec = (int64_t)h_bad;
        BWAMS_HIP(hipMemcpy(&out->bad_rec_at, s->src_off.p + h_bad, 8, hipMemcpyDeviceToHost));
        return BWAMS_OK;
    }
    out->kept_bytes = tot[0]; out->n_kept = tot[1];
    BWAMS_HIP(recs.ensure_n((size_t)tot[0] + 16));
    bq_compact_kernel<<<blocks, 256, 0, st>>>(s->wide.p, s->offs.p, n_rec, s->coord.p, s->idx.p, roff.p, coords.p);
    if (tot[1] > 0) launch_bam_sort_gather(d, s->src_off.p, s->idx.p, roff.p, tot[1], recs.p, cu_count, st);
    BWAMS_HIP(hipEventRecord(ev[3], st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    (void)hipEventElapsedTime(&out->ms_discover, ev[0], ev[1]);
    (void)hipEventElapsedTime(&out->ms_select, ev[1], ev[2]);
    (void)hipEventElapsedTime(&out->ms_gather, ev[2], ev[3]);
    return BWAMS_OK;
}

}  // namespace bwams
