// bam_merge.hip — the device side of coordinate-sorted BAM files merged as one record stream (include/bwams.h, above
// bwams_bam_file_open_merge, rules M4 to M8): the kernels of one round over the children's windows, which are read where the children's
// handles left them (their recs / roff / coords); nothing of a window is copied before the gather.
//   bm_check_kernel     a lane per record of a child's new piece: its key against its predecessor's (record 0 against the child's last
//                       key of the piece before, kept in a device word), the first bad ordinal by atomicMin (rule M5).
//   bm_frontier_kernel  one wave, a lane per child: the last key of each open child's window, their minimum F and the lowest child i*
//                       that has it (shuffles and a ballot), each lane's emit count by a binary search of its own window (lower
//                       bound of F, upper bound for children up to i*), a wave prefix sum for the bases (rule M7).
//   bm_rank_kernel      a lane per emitted record: its place in the piece is its rank in its own child plus, over the other
//                       children, the emitted records that go in front of it (key <= its own for lower children, key < its own for
//                       higher ones): K - 1 binary searches over keys in HBM / L2, the child descriptors in LDS.  It writes the
//                       record's source address, size and coord at its place (rule M4).
//   one exclusive scan of the sizes (rocPRIM) gives the offsets, and
//   bm_gather_kernel    kGroup lanes per record, copy_record (rec_gather.h) from the K source buffers into the piece.
// Every index a kernel stores through is a rank below the round's total, which the frontier kernel computed from the same counts.
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "common.h"
#include "rec_gather.h"
#include "wave_ops.h"

namespace bwams {
namespace {

__device__ __forceinline__ uint64_t key_at(const bwams_bam_coord_t *c, int64_t r) { return c[r].key; }

// records of c[lo, hi) with key < x (upper = false) or key <= x (upper = true), c sorted by key
__device__ __forceinline__ int64_t bound(const bwams_bam_coord_t *__restrict__ c, int64_t lo, int64_t hi, uint64_t x, bool upper) {
    const int64_t first = lo;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const uint64_t k = key_at(c, mid);
        if (k < x || (upper && k == x)) lo = mid + 1;
        else hi = mid;
    }
    return lo - first;
}

__global__ __launch_bounds__(256) void bm_check_kernel(const BmChild *__restrict__ kids, uint64_t *__restrict__ last_key, BmPlan *__restrict__ plan) {
    const int j = blockIdx.y;
    const BmChild c = kids[j];
    if (!c.refilled) return;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < c.n; r += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = key_at(c.coords, r);
        const uint64_t prev = r ? key_at(c.coords, r - 1) : last_key[2 * j + (c.parity ^ 1)];
        if (key < prev) atomicMin(&plan->bad[j], (unsigned long long)(c.seen + r));
        if (r == c.n - 1) last_key[2 * j + c.parity] = key;        // the other word: lane 0 of this launch reads the old one
    }
}

__global__ __launch_bounds__(64) void bm_frontier_kernel(const BmChild *__restrict__ kids, int n_kids, BmPlan *__restrict__ plan) {
    const int j = threadIdx.x;
    BmChild c{};
    if (j < n_kids) c = kids[j];
    const int64_t w = c.n - c.cur;
    const bool open = c.open && w > 0;
    const uint64_t L = open ? key_at(c.coords, c.n - 1) : ~0ULL;
    uint64_t F = L;
    for (int d = 32; d; d >>= 1) {
        const uint64_t o = (uint64_t)shfl64((int64_t)F, j ^ d);
        F = o < F ? o : F;
    }
    const unsigned long long is_open = __ballot(open);
    const unsigned long long at_f = __ballot(open && L == F);
    const int i_star = at_f ? __ffsll(at_f) - 1 : -1;
    int64_t count = w;                                         // no open child: every window whole
    if (is_open) count = w > 0 ? bound(c.coords, c.cur, c.n, F, j <= i_star) : 0;
    int64_t incl = count;
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t x = shfl64(incl, j >= d ? j - d : j);
        if (j >= d) incl += x;
    }
    plan->count[j] = count;
    plan->base[j] = incl - count;
    if (j == 63) {
        plan->total = incl;
        plan->frontier = F;
        plan->i_star = i_star;
        plan->any_open = is_open ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void bm_rank_kernel(const BmChild *__restrict__ kids, int n_kids, const BmPlan *__restrict__ plan,
                                                      const uint8_t **__restrict__ src, int64_t *__restrict__ size,
                                                      bwams_bam_coord_t *__restrict__ coords) {
    __shared__ const bwams_bam_coord_t *s_coords[kBmMaxFiles];      // of each child's first emitted record
    __shared__ const int64_t *s_roff[kBmMaxFiles];
    __shared__ const uint8_t *s_recs[kBmMaxFiles];
    __shared__ int64_t s_count[kBmMaxFiles], s_base[kBmMaxFiles];
    if (threadIdx.x < kBmMaxFiles) {
        const int j = threadIdx.x;
        const bool in = j < n_kids;
        s_coords[j] = in ? kids[j].coords + kids[j].cur : nullptr;
        s_roff[j] = in ? kids[j].roff + kids[j].cur : nullptr;
        s_recs[j] = in ? kids[j].recs : nullptr;
        s_count[j] = in ? plan->count[j] : 0;
        s_base[j] = in ? plan->base[j] : 0;
    }
    __syncthreads();
    const int64_t total = plan->total;
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g > total) return;
    if (g == total) { size[g] = 0; return; }
    int lo = 0, hi = n_kids;                                   // the last child whose base is at most g: the one that emits record g
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_base[mid] <= g) lo = mid + 1;
        else hi = mid;
    }
    const int j = lo - 1;
    const int64_t i = g - s_base[j];
    const bwams_bam_coord_t cd = s_coords[j][i];
    int64_t place = i;
    for (int o = 0; o < n_kids; ++o)
        if (o != j && s_count[o] > 0) place += bound(s_coords[o], 0, s_count[o], cd.key, o < j);
    src[place] = s_recs[j] + s_roff[j][i];
    size[place] = cd.size;
    coords[place] = cd;
}

__global__ __launch_bounds__(256) void bm_gather_kernel(const uint8_t *const *__restrict__ src, const int64_t *__restrict__ roff, int64_t n,
                                                        uint8_t *__restrict__ dst) {
    const int g = (int)(threadIdx.x & (kGroup - 1));
    const int64_t n_groups = (int64_t)gridDim.x * (blockDim.x / kGroup);
    for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup; r < n; r += n_groups) {
        const int64_t at = roff[r];
        copy_record(src[r], dst + at, roff[r + 1] - at, g);
    }
}

}  // namespace

void launch_bm_check(const BmChild *kids, int n_kids, int64_t max_n, uint64_t *last_key, BmPlan *plan, int cu_count, hipStream_t st) {
    if (max_n > 0) bm_check_kernel<<<dim3(grid_of(max_n, 256, cu_count), (unsigned)n_kids), 256, 0, st>>>(kids, last_key, plan);
}

void launch_bm_frontier(const BmChild *kids, int n_kids, BmPlan *plan, hipStream_t st) {
    bm_frontier_kernel<<<1, 64, 0, st>>>(kids, n_kids, plan);
}

void launch_bm_rank(const BmChild *kids, int n_kids, const BmPlan *plan, int64_t total, const uint8_t **src, int64_t *size,
                    bwams_bam_coord_t *coords, hipStream_t st) {
    bm_rank_kernel<<<(unsigned)((total + 1 + 255) / 256), 256, 0, st>>>(kids, n_kids, plan, src, size, coords);
}

hipError_t bm_scan(void *tmp, size_t &tmp_bytes, const int64_t *size, int64_t *roff, int64_t n1, hipStream_t st) {
    return rocprim::exclusive_scan(tmp, tmp_bytes, size, roff, (int64_t)0, (size_t)n1, rocprim::plus<int64_t>(), st);
}

void launch_bm_gather(const uint8_t *const *src, const int64_t *roff, int64_t n, uint8_t *dst, int cu_count, hipStream_t st) {
    if (n > 0) bm_gather_kernel<<<grid_of(n, 256 / kGroup, cu_count), 256, 0, st>>>(src, roff, n, dst);
}

}  // namespace bwams
