// collate.hip — a coordinate-sorted BAM collated by read name, piece by piece (bwams_collate_t; rules C1-C8 in include/bwams.h above
// bwams_collate_open, restated in bwams/collate.py).  Between adds only the records that still wait for their mate are kept: their
// bytes in the pool and an entry each (CoEntries, 29 bytes), in ordinal order.  Per added piece of n records, m of them paired:
//   co_entry_kernel    lane per record: C1's and C2's class from FLAG, J1's k0 of the name ANDed with key_mask; atomicMin of
//                      ordinal << 3 | reason into the first-bad word, only when a look says it can win;
//   rocprim::exclusive_scan of the paired flags: each paired record's place among the new entries, and m;
//   co_append_kernel   lane per record: the paired records' entries behind the n_pend pending ones, pointing into the piece;
//   rocprim::radix_sort_pairs (masked k0, entry index) over the N = n_pend + m entries, stable.  The entries lie in ordinal order
//                      (pending ones first), so every run of equal keys comes out in ordinal order.  The sort is over pending and
//                      new entries together: its cost grows with the pool (profiles/collate.md);
//   co_match_kernel    lane per sorted slot, the lane of a run's first slot walks the run with C3's state machine: for each entry the
//                      earlier entries of the run that still wait are compared with it byte by byte (length first), so a run that
//                      holds several names (C7) costs the square of its length and never a wrong pair.  It writes each entry's
//                      fate (waits / paired, with its partner) and the run's first fault into the same first-bad word.  Nothing has
//                      been copied yet: a refused add leaves nothing to undo;
//   co_place_kernel    lane per entry and per record: what each contributes to the three outputs, as (bytes, count);
//   rocprim::exclusive_scan three times: pairs by completing record, singles in piece order, waiting records in entry order;
//   co_totals_kernel   one lane: the scans' totals beside the call words, for one copy to the host;
//   co_pairs_kernel, co_singles_kernel, co_pool_kernel
//                      sixteen lanes a record (rec_gather.h's copy_record): the pairs (first, then last) from the piece and the
//                      pool, the singles from the piece, the records that now wait behind the pool's tail — or, when the pool is
//                      compacted, every waiting record into a fresh block — with the surviving entries written into the next
//                      entry arrays.  co_pool_kernel with every entry waiting is also _finish's copy of the orphans.
// Every kernel is memory-bound; none uses LDS, scratch or floating point.  Every index a kernel stores through comes from the
// scans, the sort's permutation or the slot itself; the names only decide which entries pair.
#include <algorithm>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include "common.h"
#include "markdup_dev.h"
#include "rec_gather.h"

namespace bwams {
namespace {

enum : uint8_t { kCoSkip = 0, kCoSingle = 1, kCoFirst = 2, kCoLast = 3, kCoBadBits = 4 };
enum : uint8_t { kCoWaits = 0, kCoPaired = 1 };

__device__ __forceinline__ void min_if_less(unsigned long long *word, unsigned long long v) {
    if (v < *reinterpret_cast<volatile unsigned long long *>(word)) atomicMin(word, v);
}

__global__ void __launch_bounds__(256) co_entry_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n, int64_t base, uint64_t mask,
                                                       uint8_t *cls, uint64_t *nkey, uint32_t *paired, unsigned long long *call) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n; r += (int64_t)gridDim.x * blockDim.x) {
        if (r == n) { paired[r] = 0; continue; }             // the scan's last slot: its total
        const uint8_t *p = bam + rec_off[r];
        const uint32_t f = bam_flag(p);
        uint8_t c;
        if (f & 0x900) c = kCoSkip;
        else if (!(f & 1)) c = kCoSingle;
        else if ((f & 0xC0) == 0x40) c = kCoFirst;
        else if ((f & 0xC0) == 0x80) c = kCoLast;
        else c = kCoBadBits;
        if (c == kCoBadBits) min_if_less(call + kCoCallBad, (unsigned long long)(base + r) << 3 | kCoReasonBits);
        const bool pr = c == kCoFirst || c == kCoLast;
        if (pr) {
            const uint32_t l_name = bam_l_name(p);
            uint64_t a, b;
            name_key(p + kBamName, l_name ? l_name - 1 : 0, &a, &b);
            nkey[r] = a & mask;
        }
        cls[r] = c;
        paired[r] = pr;
    }
}

__global__ void __launch_bounds__(256) co_append_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n, int64_t base,
                                                        const uint8_t *cls, const uint64_t *nkey, const uint32_t *place, int64_t n_pend,
                                                        CoEntryArrays E) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t c = cls[r];
        if (c != kCoFirst && c != kCoLast) continue;
        const int64_t e = n_pend + place[r];
        E.key[e] = nkey[r];
        E.ptr[e] = bam + rec_off[r];
        E.ord[e] = base + r;
        E.size[e] = (int32_t)(rec_off[r + 1] - rec_off[r]);
        E.seg[e] = c;
    }
}

__global__ void __launch_bounds__(256) co_iota_kernel(uint32_t *idx, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) idx[i] = (uint32_t)i;
}

// the names of the records at a and b, without their NULs: equal in length and byte for byte
__device__ __forceinline__ bool same_name(const uint8_t *a, const uint8_t *b) {
    const uint32_t la = bam_l_name(a), lb = bam_l_name(b);
    const uint32_t na = la ? la - 1 : 0, nb = lb ? lb - 1 : 0;
    if (na != nb) return false;
    for (uint32_t k = 0; k < na; ++k)
        if (a[kBamName + k] != b[kBamName + k]) return false;
    return true;
}

__global__ void __launch_bounds__(256) co_match_kernel(const uint64_t *skey, const uint32_t *sidx, int64_t N, int64_t n_pend, CoEntryArrays E,
                                                       uint8_t *fate, uint32_t *partner, unsigned long long *call) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = skey[i];
        if (i > 0 && skey[i - 1] == key) continue;           // not a run's first slot
        unsigned long long died = 0;
        int64_t t = i;
        for (; t < N && skey[t] == key; ++t) {
            const uint32_t e = sidx[t];
            const uint8_t *p = E.ptr[e];
            int64_t j = t - 1;
            uint32_t w = 0;
            for (; j >= i; --j) {                            // at most one entry of a name waits
                w = sidx[j];
                if (fate[w] == kCoWaits && same_name(E.ptr[w], p)) break;
            }
            if (j < i) { fate[e] = kCoWaits; continue; }
            if (E.seg[w] == E.seg[e]) {                      // C3: the run's first fault; what lies behind it is never used
                min_if_less(call + kCoCallBad, (unsigned long long)E.ord[e] << 3 | kCoReasonSegment);
                ++t;
                break;
            }
            fate[w] = kCoPaired; partner[w] = e;
            fate[e] = kCoPaired; partner[e] = w;
            if ((int64_t)w < n_pend) died += (unsigned long long)E.size[w];
        }
        if (died) atomicAdd(call + kCoCallDied, died);
        const unsigned long long len = (unsigned long long)(t - i);
        if (len > *reinterpret_cast<volatile unsigned long long *>(call + kCoCallMaxRun)) atomicMax(call + kCoCallMaxRun, len);
    }
}

// An entry e that is paired completes its pair when its partner lies in front of it: entries are in ordinal order.
__global__ void __launch_bounds__(256) co_place_kernel(const uint8_t *fate, const uint32_t *partner, const int32_t *size, int64_t N,
                                                       int64_t n_pend, const uint8_t *cls, const int64_t *rec_off, int64_t n, CoPlace *waits,
                                                       CoPlace *pairs, CoPlace *singles) {
    const int64_t top = std::max(N, n);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= top; i += (int64_t)gridDim.x * blockDim.x) {
        if (i <= N) {
            const bool w = i < N && fate[i] == kCoWaits;
            waits[i] = CoPlace{w ? (int64_t)size[i] : 0, w ? 1 : 0};
            if (i >= n_pend) {
                const bool done = i < N && fate[i] == kCoPaired && partner[i] < (uint32_t)i;
                pairs[i - n_pend] = CoPlace{done ? (int64_t)size[i] + size[partner[i]] : 0, done ? 1 : 0};
            }
        }
        if (i <= n) {
            const bool s = i < n && cls[i] == kCoSingle;
            singles[i] = CoPlace{s ? rec_off[i + 1] - rec_off[i] : 0, s ? 1 : 0};
        }
    }
}

__global__ void co_totals_kernel(const CoPlace *waits, const CoPlace *pairs, const CoPlace *singles, int64_t N, int64_t n_pend, int64_t n,
                                 unsigned long long *call) {
    if (threadIdx.x || blockIdx.x) return;
    const CoPlace all = waits[N], old = waits[n_pend], pr = pairs[N - n_pend], sg = singles[n];
    call[kCoCallWaitBytes] = (unsigned long long)all.bytes; call[kCoCallWaitN] = (unsigned long long)all.n;
    call[kCoCallOldBytes] = (unsigned long long)old.bytes;  call[kCoCallOldN] = (unsigned long long)old.n;
    call[kCoCallPairBytes] = (unsigned long long)pr.bytes;  call[kCoCallPairN] = (unsigned long long)pr.n;
    call[kCoCallSingleBytes] = (unsigned long long)sg.bytes; call[kCoCallSingleN] = (unsigned long long)sg.n;
}

__global__ void __launch_bounds__(256) co_pairs_kernel(CoEntryArrays E, const uint8_t *fate, const uint32_t *partner, const CoPlace *at,
                                                       int64_t n_pend, int64_t m, uint8_t *dst, int64_t *pair_off) {
    const int g = (int)(threadIdx.x & (kGroup - 1));
    const int64_t n_groups = (int64_t)gridDim.x * (blockDim.x / kGroup);
    for (int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup; j <= m; j += n_groups) {
        const CoPlace to = at[j];
        if (j == m) {                                        // the end of the last pair
            if (g == 0) pair_off[2 * to.n] = to.bytes;
            continue;
        }
        const int64_t e = n_pend + j;
        if (fate[e] != kCoPaired || partner[e] >= (uint32_t)e) continue;
        const int64_t w = partner[e];
        const int64_t first = E.seg[e] == kCoFirst ? e : w, last = first == e ? w : e;
        const int64_t n1 = E.size[first], n2 = E.size[last];
        copy_record(E.ptr[first], dst + to.bytes, n1, g);
        copy_record(E.ptr[last], dst + to.bytes + n1, n2, g);
        if (g == 0) { pair_off[2 * to.n] = to.bytes; pair_off[2 * to.n + 1] = to.bytes + n1; }
    }
}

__global__ void __launch_bounds__(256) co_singles_kernel(const uint8_t *bam, const int64_t *rec_off, const uint8_t *cls, const CoPlace *at,
                                                         int64_t n, uint8_t *dst, int64_t *single_off) {
    const int g = (int)(threadIdx.x & (kGroup - 1));
    const int64_t n_groups = (int64_t)gridDim.x * (blockDim.x / kGroup);
    for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup; r <= n; r += n_groups) {
        const CoPlace to = at[r];
        if (r == n) {
            if (g == 0) single_off[to.n] = to.bytes;
            continue;
        }
        if (cls[r] != kCoSingle) continue;
        copy_record(bam + rec_off[r], dst + to.bytes, rec_off[r + 1] - rec_off[r], g);
        if (g == 0) single_off[to.n] = to.bytes;
    }
}

// The waiting entries of E[0, N) into F in their order.  Those from entry `from` on are copied to dst + (their place - sub) and
// point there; the ones in front stay where they lie.  rec_at (or null): each copied record's offset, and the end behind the last.
__global__ void __launch_bounds__(256) co_pool_kernel(CoEntryArrays E, const uint8_t *fate, const CoPlace *at, int64_t from, int64_t N,
                                                      uint8_t *dst, int64_t sub, CoEntryArrays F, int64_t *rec_at) {
    const int g = (int)(threadIdx.x & (kGroup - 1));
    const int64_t n_groups = (int64_t)gridDim.x * (blockDim.x / kGroup);
    for (int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup; e <= N; e += n_groups) {
        const CoPlace to = at[e];
        if (e == N) {
            if (g == 0 && rec_at) rec_at[to.n] = to.bytes - sub;
            continue;
        }
        if (fate[e] != kCoWaits) continue;
        const uint8_t *p = E.ptr[e];
        const int64_t n = E.size[e];
        if (e >= from) {
            copy_record(p, dst + (to.bytes - sub), n, g);
            p = dst + (to.bytes - sub);
            if (g == 0 && rec_at) rec_at[to.n] = to.bytes - sub;
        }
        if (g == 0 && F.key) {
            F.key[to.n] = E.key[e]; F.ptr[to.n] = p; F.ord[to.n] = E.ord[e]; F.size[to.n] = (int32_t)n; F.seg[to.n] = E.seg[e];
        }
    }
}

struct CoPlus {
    __host__ __device__ CoPlace operator()(const CoPlace &a, const CoPlace &b) const { return CoPlace{a.bytes + b.bytes, a.n + b.n}; }
};

}  // namespace

void launch_co_entry(const uint8_t *bam, const int64_t *rec_off, int64_t n, int64_t base, uint64_t mask, uint8_t *cls, uint64_t *nkey,
                     uint32_t *paired, unsigned long long *call, int cu_count, hipStream_t st) {
    co_entry_kernel<<<grid_of(n + 1, 256, cu_count), 256, 0, st>>>(bam, rec_off, n, base, mask, cls, nkey, paired, call);
}

int co_scan_u32(void *tmp, size_t &tmp_bytes, const uint32_t *in, uint32_t *out, int64_t n, hipStream_t st) {
    BWAMS_HIP(rocprim::exclusive_scan(tmp, tmp_bytes, in, out, 0u, (size_t)n, rocprim::plus<uint32_t>(), st));
    return BWAMS_OK;
}

int co_scan_place(void *tmp, size_t &tmp_bytes, const CoPlace *in, CoPlace *out, int64_t n, hipStream_t st) {
    BWAMS_HIP(rocprim::exclusive_scan(tmp, tmp_bytes, in, out, CoPlace{0, 0}, (size_t)n, CoPlus(), st));
    return BWAMS_OK;
}

int co_sort(void *tmp, size_t &tmp_bytes, const uint64_t *key, uint64_t *skey, const uint32_t *idx, uint32_t *sidx, int64_t N, hipStream_t st) {
    BWAMS_HIP(rocprim::radix_sort_pairs(tmp, tmp_bytes, key, skey, idx, sidx, (size_t)N, 0u, 64u, st));
    return BWAMS_OK;
}

void launch_co_append(const uint8_t *bam, const int64_t *rec_off, int64_t n, int64_t base, const uint8_t *cls, const uint64_t *nkey,
                      const uint32_t *place, int64_t n_pend, const CoEntryArrays &E, uint32_t *idx, int64_t N, int cu_count, hipStream_t st) {
    if (n > 0) co_append_kernel<<<grid_of(n, 256, cu_count), 256, 0, st>>>(bam, rec_off, n, base, cls, nkey, place, n_pend, E);
    if (N > 0) co_iota_kernel<<<grid_of(N, 256, cu_count), 256, 0, st>>>(idx, N);
}

void launch_co_match(const uint64_t *skey, const uint32_t *sidx, int64_t N, int64_t n_pend, const CoEntryArrays &E, uint8_t *fate,
                     uint32_t *partner, unsigned long long *call, int cu_count, hipStream_t st) {
    if (N > 0) co_match_kernel<<<grid_of(N, 256, cu_count), 256, 0, st>>>(skey, sidx, N, n_pend, E, fate, partner, call);
}

void launch_co_place(const uint8_t *fate, const uint32_t *partner, const int32_t *size, int64_t N, int64_t n_pend, const uint8_t *cls,
                     const int64_t *rec_off, int64_t n, CoPlace *waits, CoPlace *pairs, CoPlace *singles, int cu_count, hipStream_t st) {
    co_place_kernel<<<grid_of(std::max(N, n) + 1, 256, cu_count), 256, 0, st>>>(fate, partner, size, N, n_pend, cls, rec_off, n, waits, pairs,
                                                                               singles);
}

void launch_co_totals(const CoPlace *waits, const CoPlace *pairs, const CoPlace *singles, int64_t N, int64_t n_pend, int64_t n,
                      unsigned long long *call, hipStream_t st) {
    co_totals_kernel<<<1, 64, 0, st>>>(waits, pairs, singles, N, n_pend, n, call);
}

void launch_co_pairs(const CoEntryArrays &E, const uint8_t *fate, const uint32_t *partner, const CoPlace *at, int64_t n_pend, int64_t m,
                     uint8_t *dst, int64_t *pair_off, int cu_count, hipStream_t st) {
    co_pairs_kernel<<<grid_of(m + 1, 256 / kGroup, cu_count), 256, 0, st>>>(E, fate, partner, at, n_pend, m, dst, pair_off);
}

void launch_co_singles(const uint8_t *bam, const int64_t *rec_off, const uint8_t *cls, const CoPlace *at, int64_t n, uint8_t *dst,
                       int64_t *single_off, int cu_count, hipStream_t st) {
    co_singles_kernel<<<grid_of(n + 1, 256 / kGroup, cu_count), 256, 0, st>>>(bam, rec_off, cls, at, n, dst, single_off);
}

void launch_co_pool(const CoEntryArrays &E, const uint8_t *fate, const CoPlace *at, int64_t from, int64_t N, uint8_t *dst, int64_t sub,
                    const CoEntryArrays &F, int64_t *rec_at, int cu_count, hipStream_t st) {
    co_pool_kernel<<<grid_of(N + 1, 256 / kGroup, cu_count), 256, 0, st>>>(E, fate, at, from, N, dst, sub, F, rec_at);
}

}  // namespace bwams
