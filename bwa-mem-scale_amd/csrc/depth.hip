// depth.hip — per-base depth of coverage (the rules are in include/bwams.h above bwams_depth_open).
//
// Layout: one int32 array of slots, l_ref[r] + 1 per reference, back to back; slot_off[r] is reference r's first slot
// (slot_off[n_ref] = all of them).  While records are added the array holds differences: a covered stretch [a, b) of reference r
// adds +1 at slot_off[r] + a and -1 at slot_off[r] + min(b, l_ref[r]), so the slot at l_ref[r] takes the -1 of whatever reaches the
// end, every reference's slots sum to zero, and ONE unsegmented inclusive scan of the whole array (bwams_depth_finish) turns it
// into depths without a carry crossing a reference boundary.  After the scan the slot at l_ref[r] holds 0; it is no position and
// stays out of every query.
//   depth_check_kernel   lane per record: walks the CIGAR of every record and keeps the smallest index of one with an op code above 8.
//   depth_add_kernel     lane per record: rule 2's filter, then the CIGAR walk; ops that are adjacent on the reference (M = X, and D
//                        when deletions count; I S H P between them do not part them) merge into one stretch, so the usual read
//                        issues one pair of atomics.  The wave emits stretches in rounds: every lane walks to its next stretch,
//                        then lanes that hold the SAME slot as their left neighbour are folded into it (compare with lane - 1, a
//                        ballot of the run heads, the head adds the run's length), because sorted input and amplicon pileups put
//                        most of a wave on one address and same-address atomics serialise in L2.
//   depth_seg_kernel     summary (sum, min, max per reference) and windows (sum per window): a wave takes 2048 consecutive slots in
//                        32 groups of 64; the slots' references come from a binary search in slot_off done once per wave when the
//                        whole piece lies in one reference, per lane otherwise.  A group whose positions share a key (reference, or
//                        window) is reduced across the wave and accumulated in registers until the key changes: one set of atomics
//                        per key per wave; a group of mixed keys (tiny references, windows shorter than 64) adds lane by lane.
//   depth_hist_kernel    depths below kDepthHistLds are counted in LDS and the non-zero bins flushed once per workgroup; the last bin
//                        (everything at or above n_bins - 1) is counted in registers and added once per wave; the rest by global atomics.
//   depth_gather_kernel  runs: depth[k] = slots[start[k]] (the starts come from rocprim::select over the positions whose depth differs
//                        from their left neighbour's).
// All of them are bound by HBM: every slot is read once.
#include <algorithm>
#include <climits>
#include "common.h"
#include "bam_rec.h"
#include "wave_ops.h"

namespace bwams {
namespace {

__global__ void __launch_bounds__(256) depth_check_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec,
                                                          unsigned long long *bad) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t *p = bam + rec_off[r];
        const uint32_t n_cig = bam_n_cig(p);
        const uint8_t *c = p + bam_cigar_at(bam_l_name(p));
        bool any = false;
        for (uint32_t k = 0; k < n_cig; ++k) any |= (c[4 * k] & 15) > 8;
        if (any) atomicMin(bad, (unsigned long long)r);
    }
}

// the slot of lane - 1, or -1 for lane 0
__device__ __forceinline__ int64_t left_neighbour(int64_t v, int lane) {
    const int64_t u = __shfl_up((long long)v, 1, 64);
    return lane == 0 ? -1 : u;
}

// adds `sign` at slot `key` for every lane with key >= 0; lanes that hold their left neighbour's key are folded into it
__device__ __forceinline__ void emit(int32_t *slots, int64_t key, int sign, int lane, bool combine) {
    if (!combine) {
        if (key >= 0) atomicAdd(slots + key, sign);
        return;
    }
    const int64_t prev = left_neighbour(key, lane);
    const bool head = lane == 0 || prev != key;
    const uint64_t heads = __ballot(head);
    const uint64_t above = lane == 63 ? 0 : heads >> (lane + 1);
    const int len = above ? __ffsll((unsigned long long)above) : 64 - lane;
    if (head && key >= 0) atomicAdd(slots + key, sign * len);
}

struct DepthFilter {
    uint32_t exclude;
    int32_t min_mapq, count_deletions, n_ref;
};

__global__ void __launch_bounds__(256) depth_add_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, DepthFilter f,
                                                        const int64_t *slot_off, int32_t *slots, unsigned long long *n_counted,
                                                        int combine) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t rounded = (n_rec + 63) & ~(int64_t)63;                 // whole waves enter every round: the ballots need them
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rounded; r += stride) {
        const uint8_t *c = nullptr;
        uint32_t n_cig = 0, k = 0;
        int64_t x = 0, base = 0, len_ref = 0;
        if (r < n_rec) {
            const uint8_t *p = bam + rec_off[r];
            const int32_t rid = bam_ref_id(p);
            const uint32_t mapq = bam_mapq(p), nc = bam_n_cig(p), flag = bam_flag(p);
            if (!(flag & f.exclude) && (int32_t)mapq >= f.min_mapq && rid >= 0 && rid < f.n_ref && nc > 0) {
                n_cig = nc;
                c = p + bam_cigar_at(bam_l_name(p));
                x = bam_pos(p);
                base = slot_off[rid];
                len_ref = slot_off[rid + 1] - base - 1;
            }
        }
        const uint64_t counted = __ballot(n_cig > 0);
        if (lane == 0 && counted) atomicAdd(n_counted, (unsigned long long)__popcll((unsigned long long)counted));
        for (;;) {                                                       // a round: every lane's next stretch, then the two adds
            int64_t a = -1, b = -1;
            bool open = false;
            int64_t beg = 0;
            while (k < n_cig) {
                const uint32_t op = ld_u32(c + 4 * k);
                const uint32_t o = op & 15;
                const int64_t len = op >> 4;
                const bool covers = o == 0 || o == 7 || o == 8 || (o == 2 && f.count_deletions);     // spelled out: op_is_match here costs 45 instructions
                if (covers) {
                    if (!open) { open = true; beg = x; }
                    x += len;
                } else if (o == 2 || o == 3) {
                    const int64_t end = x;
                    x += len;
                    if (open) {
                        open = false;
                        const int64_t lo = std::max<int64_t>(beg, 0), hi = std::min(end, len_ref);
                        if (lo < hi) { a = base + lo; b = base + hi; ++k; break; }
                    }
                }
                ++k;
            }
            if (a < 0 && open) {                                         // the stretch that the CIGAR's end closes
                const int64_t lo = std::max<int64_t>(beg, 0), hi = std::min(x, len_ref);
                if (lo < hi) { a = base + lo; b = base + hi; }
            }
            if (!__any(a >= 0)) break;
            emit(slots, a, 1, lane, combine != 0);
            emit(slots, b, -1, lane, combine != 0);
        }
    }
}

// the reference of slot s among [lo, hi]: the last r with slot_off[r] <= s
__device__ __forceinline__ int32_t ref_of(const int64_t *slot_off, int64_t s, int32_t lo, int32_t hi) {
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (slot_off[mid] <= s) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

constexpr int kSegGroups = 32;                                           // groups of 64 slots per wave

struct SegOut {
    unsigned long long *sum;                                             // per key
    int32_t *mn, *mx;                                                    // summary only
};

template <bool kWindows> __device__ __forceinline__ void seg_flush(const SegOut &o, int64_t key, int64_t sum, int32_t mn, int32_t mx) {
    if (key < 0) return;
    atomicAdd(o.sum + key, (unsigned long long)sum);
    if (!kWindows) { atomicMin(o.mn + key, mn); atomicMax(o.mx + key, mx); }
}

// kWindows: key = win_off[r] + pos / w; else key = r
template <bool kWindows>
__global__ void __launch_bounds__(256) depth_seg_kernel(const int32_t *slots, const int64_t *slot_off, int32_t n_ref, int64_t n_slots,
                                                        const int64_t *win_off, int32_t w, SegOut out) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    constexpr int64_t kPiece = 64 * kSegGroups;
    for (int64_t first = wave * kPiece; first < n_slots; first += n_waves * kPiece) {
        const int64_t last = std::min(first + kPiece, n_slots) - 1;
        const int32_t r_lo = ref_of(slot_off, first, 0, n_ref - 1), r_hi = ref_of(slot_off, last, r_lo, n_ref - 1);
        int64_t acc_key = -1, acc_sum = 0;                               // wave-uniform: the key being accumulated
        int32_t acc_mn = INT_MAX, acc_mx = 0;
        for (int j = 0; j < kSegGroups; ++j) {
            const int64_t s = first + (int64_t)j * 64 + lane;
            if (first + (int64_t)j * 64 > last) break;
            bool is_pos = false;
            int64_t key = -1;
            int32_t v = 0;
            if (s <= last) {
                const int32_t r = r_lo == r_hi ? r_lo : ref_of(slot_off, s, r_lo, r_hi);
                const int64_t pos = s - slot_off[r];
                is_pos = pos < slot_off[r + 1] - slot_off[r] - 1;
                if (is_pos) {
                    v = slots[s];
                    key = kWindows ? win_off[r] + (int64_t)((uint32_t)pos / (uint32_t)w) : (int64_t)r;
                }
            }
            const uint64_t have = __ballot(is_pos);
            if (!have) continue;
            const int64_t k0 = __shfl((long long)key, __ffsll((unsigned long long)have) - 1, 64);
            if (__ballot(is_pos && key != k0) == 0) {                    // one key: reduce, keep in registers
                const int64_t sum = wave_sum(is_pos ? (int64_t)v : 0);
                const int32_t mn = kWindows ? 0 : wave_min(is_pos ? v : INT_MAX), mx = kWindows ? 0 : wave_max(is_pos ? v : 0);
                if (k0 != acc_key) {
                    if (lane == 0) seg_flush<kWindows>(out, acc_key, acc_sum, acc_mn, acc_mx);
                    acc_key = k0; acc_sum = 0; acc_mn = INT_MAX; acc_mx = 0;
                }
                acc_sum += sum; acc_mn = min(acc_mn, mn); acc_mx = max(acc_mx, mx);
            } else if (is_pos) {
                seg_flush<kWindows>(out, key, v, v, v);
            }
        }
        if (lane == 0) seg_flush<kWindows>(out, acc_key, acc_sum, acc_mn, acc_mx);
    }
}

__global__ void __launch_bounds__(256) depth_hist_kernel(const int32_t *slots, int64_t lo, int64_t hi, int32_t n_bins,
                                                         unsigned long long *hist) {
    __shared__ uint32_t bins[kDepthHistLds];
    for (int k = threadIdx.x; k < kDepthHistLds; k += blockDim.x) bins[k] = 0;
    __syncthreads();
    const int32_t top = n_bins - 1, lds_top = min(top, kDepthHistLds);
    unsigned long long n_top = 0;
    // a workgroup's share stays below 2^32 slots: the LDS counters cannot wrap
    for (int64_t s = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < hi; s += (int64_t)gridDim.x * blockDim.x) {
        const int32_t v = slots[s];
        if (v >= top) ++n_top;
        else if ((uint32_t)v < (uint32_t)lds_top) atomicAdd(&bins[v], 1u);
        else if (v >= 0) atomicAdd(hist + v, 1ULL);
    }
    n_top = (unsigned long long)wave_sum((int64_t)n_top);
    if ((threadIdx.x & 63) == 0 && n_top) atomicAdd(hist + top, n_top);
    __syncthreads();
    for (int k = threadIdx.x; k < lds_top; k += blockDim.x)
        if (bins[k]) atomicAdd(hist + k, (unsigned long long)bins[k]);
}

__global__ void __launch_bounds__(256) depth_gather_kernel(const int32_t *slots, int64_t base, const int32_t *start, int64_t n,
                                                           int32_t *depth) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
        depth[k] = slots[base + start[k]];
}

}  // namespace

void launch_depth_check(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, unsigned long long *bad, int cu_count, hipStream_t st) {
    if (n_rec > 0) depth_check_kernel<<<grid_of(n_rec, 256, cu_count), 256, 0, st>>>(bam, rec_off, n_rec, bad);
}

void launch_depth_add(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const bwams_depth_opt_t &opt, int32_t n_ref,
                      const int64_t *slot_off, int32_t *slots, unsigned long long *n_counted, int combine, int cu_count, hipStream_t st) {
    const DepthFilter f{opt.exclude, opt.min_mapq, opt.count_deletions, n_ref};
    if (n_rec > 0 && n_ref > 0)
        depth_add_kernel<<<grid_of(n_rec, 256, cu_count), 256, 0, st>>>(bam, rec_off, n_rec, f, slot_off, slots, n_counted, combine);
}

void launch_depth_summary(const int32_t *slots, const int64_t *slot_off, int32_t n_ref, int64_t n_slots, unsigned long long *sum,
                          int32_t *mn, int32_t *mx, int cu_count, hipStream_t st) {
    if (n_ref > 0)
        depth_seg_kernel<false><<<grid_of(n_slots, 4 * 64 * kSegGroups, cu_count), 256, 0, st>>>(slots, slot_off, n_ref, n_slots, nullptr, 1,
                                                                                                 SegOut{sum, mn, mx});
}

void launch_depth_windows(const int32_t *slots, const int64_t *slot_off, int32_t n_ref, int64_t n_slots, const int64_t *win_off, int32_t w,
                          unsigned long long *sums, int cu_count, hipStream_t st) {
    if (n_ref > 0)
        depth_seg_kernel<true><<<grid_of(n_slots, 4 * 64 * kSegGroups, cu_count), 256, 0, st>>>(slots, slot_off, n_ref, n_slots, win_off, w,
                                                                                                SegOut{sums, nullptr, nullptr});
}

void launch_depth_hist(const int32_t *slots, int64_t lo, int64_t hi, int32_t n_bins, unsigned long long *hist, int cu_count, hipStream_t st) {
    if (hi > lo) depth_hist_kernel<<<grid_of(hi - lo, 256 * 64, cu_count), 256, 0, st>>>(slots, lo, hi, n_bins, hist);
}

void launch_depth_gather(const int32_t *slots, int64_t base, const int32_t *start, int64_t n, int32_t *depth, int cu_count, hipStream_t st) {
    if (n > 0) depth_gather_kernel<<<grid_of(n, 256, cu_count), 256, 0, st>>>(slots, base, start, n, depth);
}

}  // namespace bwams
