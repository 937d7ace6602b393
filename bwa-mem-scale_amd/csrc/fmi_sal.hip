// fmi_sal.hip — suffix-array lookup of SMEM occurrences for gfx950.
//
// Reference semantics: get_sa_entries_prefetch + call_one_step
// (/root/reference/src/FMI_search.cpp:2261-2379, :2206-2259) as driven by
// mem_chain_seeds (/root/reference/src/bwamem.cpp:861-873): SMEM i contributes
// the BWT rows k, k+step, ... (step = s/max_occ when s > max_occ, at most max_occ
// rows); each row is walked with LF-mapping until a multiple of 8, where the
// sampled SA (int8 high byte + uint32 low word) is read and the walk length added.
// A walk that meets the sentinel row yields 0 (reference quirk, :2234-2237).
//
// Mapping: every lookup is an independent chain of at most 7 dependent block
// reads, so one LANE per lookup; the owning SMEM is found by binary search in the
// prefix offsets, which stay L2-resident.
//
// SA[row] depends on the index alone: with the index's dense table (one entry per
// S-th row holding what the walk from that row produces, fmi_kernels.h) a lookup
// walks only to the next multiple of S and reads the rest; both counters stay what
// the reference walks.
#include "fmi_kernels.h"

namespace bwams {
namespace {

__device__ __forceinline__ uint64_t mk64(uint32_t lo, uint32_t hi) {
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

// S = 0: no table, every row walks to a sample of the index; S = 1, 2, 4: the dense table of that stride
template <int S>
__global__ __launch_bounds__(256) void sa_lookup_kernel(DevFmi f, const bwams_smem_t *__restrict__ sm,
                                                        int64_t n_smem, const int64_t *__restrict__ sa_off,
                                                        int64_t *__restrict__ coord, int64_t coord_cap,
                                                        int max_occ, DevCounters *ctr, const uint64_t *__restrict__ dense) {
    const int64_t total = sa_off[n_smem] < coord_cap ? sa_off[n_smem] : coord_cap;
    unsigned long long lf = 0;
    // The owner of position g is the last SMEM whose first position is <= g: a binary search over 9 M offsets, i.e. 23
    // DEPENDENT loads per lookup, more than the LF walk behind it.  A wave takes a contiguous range of positions instead:
    // one search for its first position, and from there the owners only move forward — 64 consecutive positions belong
    // to at most 64 consecutive SMEMs (every SMEM has at least one), whose offsets are one coalesced load into LDS and a
    // six-step search there.
    __shared__ int64_t win_s[4][65];
    int64_t *const win = win_s[threadIdx.x >> 6];
    const int lane = (int)(threadIdx.x & 63);
    const int64_t n_waves = (int64_t)gridDim.x * 4, wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t per = ((total + n_waves - 1) / n_waves + 63) & ~(int64_t)63;
    const int64_t start = wave * per, end = start + per < total ? start + per : total;
    int64_t lo0 = 0;
    if (start < end) {
        int64_t a = 0, b = n_smem;
        while (b - a > 1) {
            const int64_t mid = (a + b) >> 1;
            if (sa_off[mid] <= start) a = mid; else b = mid;
        }
        lo0 = a;
    }
    for (int64_t g0 = start; g0 < end; g0 += 64) {
        const int64_t g = g0 + lane;
        {
            const int64_t c = lo0 + 1 + lane;
            win[lane] = c <= n_smem ? sa_off[c] : INT64_MAX;
            if (lane == 0) win[64] = INT64_MAX;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        int t = 0;                                            // first candidate whose offset is beyond g
        for (int stp = 32; stp > 0; stp >>= 1)
            if (win[t + stp - 1] <= g) t += stp;
        if (t == 63 && win[63] <= g) t = 64;
        int64_t lo = lo0 + t;
        if (t == 64 && g < end) {                             // not within 64 SMEMs (never, while every SMEM has a position): search
            int64_t a = lo, b = n_smem;
            while (b - a > 1) {
                const int64_t mid = (a + b) >> 1;
                if (sa_off[mid] <= g) a = mid; else b = mid;
            }
            lo = a;
        }
        {   // the next trip starts from the owner of this trip's last position
            const int last = (int)((end - g0 < 64 ? end - g0 : 64) - 1);
            const uint32_t l_lo = (uint32_t)lo, l_hi = (uint32_t)((uint64_t)lo >> 32);
            lo0 = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)l_hi, last) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)l_lo, last));
        }
        __builtin_amdgcn_wave_barrier();
        if (g >= end) continue;
        const int64_t k = sm[lo].k, s = sm[lo].s;
        const int64_t step = s > (int64_t)max_occ ? s / max_occ : 1;
        int64_t sp = k + (g - sa_off[lo]) * step;
        int64_t val;
        if constexpr (S == 0) {
            const SaWalk w = sa_walk<8>(f, sp);
            val = w.sentinel ? 0 : sa_sample(f, w.sp) + (int64_t)w.steps;
            lf += w.steps;
        } else {
            // at most S - 1 steps of its own, then the entry of the row reached: what the reference's walk from there produces
            const SaWalk w = sa_walk<S>(f, sp);
            uint64_t e = kSaDenseSentinel;
            if (!w.sentinel) {
                e = dense[S == 1 ? w.sp : S == 2 ? w.sp >> 1 : w.sp >> 2];
                lf += e >> (kSaDenseCoordBits + 1);
            }
            val = (e & kSaDenseSentinel) ? 0 : (int64_t)(e & (kSaDenseSentinel - 1)) + (int64_t)w.steps;
            lf += w.steps;
        }
        coord[g] = val;
    }
    for (int o = 32; o > 0; o >>= 1)
        lf += mk64(__shfl_down((uint32_t)lf, o), __shfl_down((uint32_t)(lf >> 32), o));
    if ((threadIdx.x & 63) == 0 && lf) atomicAdd(&ctr->n_lf_steps, lf);
    if (blockIdx.x == 0 && threadIdx.x == 0) ctr->n_sa_lookups = (unsigned long long)sa_off[n_smem];
}

// One lane per entry: the present walk from row i * stride, packed
__global__ __launch_bounds__(256) void sa_dense_build_kernel(DevFmi f, int stride, int64_t n, uint64_t *__restrict__ table,
                                                             unsigned long long *bad) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const SaWalk w = sa_walk<8>(f, i * stride);
        if (w.steps >> kSaDenseStepBits) *bad = 1;
        const uint64_t c = w.sentinel ? kSaDenseSentinel : (uint64_t)(sa_sample(f, w.sp) + (int64_t)w.steps);
        if (!w.sentinel && (c >> kSaDenseCoordBits)) *bad = 1;
        table[i] = c | ((uint64_t)w.steps << (kSaDenseCoordBits + 1));
    }
}

}  // namespace

void launch_sa_lookup(const DevFmi &f, const bwams_smem_t *sorted, int64_t n_smem, const int64_t *sa_off,
                      int64_t *coord, int64_t coord_cap, int max_occ, DevCounters *ctr, int cu_count,
                      hipStream_t st, const uint64_t *dense, int stride) {
    if (n_smem <= 0) return;
    const unsigned grid = (unsigned)cu_count * 8;
    if (!dense) sa_lookup_kernel<0><<<grid, 256, 0, st>>>(f, sorted, n_smem, sa_off, coord, coord_cap, max_occ, ctr, nullptr);
    else if (stride == 1) sa_lookup_kernel<1><<<grid, 256, 0, st>>>(f, sorted, n_smem, sa_off, coord, coord_cap, max_occ, ctr, dense);
    else if (stride == 2) sa_lookup_kernel<2><<<grid, 256, 0, st>>>(f, sorted, n_smem, sa_off, coord, coord_cap, max_occ, ctr, dense);
    else sa_lookup_kernel<4><<<grid, 256, 0, st>>>(f, sorted, n_smem, sa_off, coord, coord_cap, max_occ, ctr, dense);
}

void launch_sa_dense_build(const DevFmi &f, int stride, int64_t n, uint64_t *table, unsigned long long *bad, int cu_count, hipStream_t st) {
    if (n <= 0) return;
    sa_dense_build_kernel<<<grid_of(n, 256, cu_count, 32), 256, 0, st>>>(f, stride, n, table, bad);
}

}  // namespace bwams
