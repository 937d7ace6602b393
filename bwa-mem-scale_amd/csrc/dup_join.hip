// dup_join.hip — duplicate marking's templates joined by read name, for records that are not query-grouped (bwams_dupjoin_t; rules
// J1-J9 in include/bwams.h above bwams_dupjoin_open, restated in bwams/markdup.py).  Everything behind the ends is markdup.hip's
// md_decide, unchanged; what both files need of a record is markdup_dev.h's.
// Per added piece, entries appended at the records' ordinals (DjEntries, 57 bytes per record):
//   dj_key_kernel    lane per record: J1's key of the name, L, and rules 9-10 of the record itself (with a table its aux fields are
//                    walked: atomicMin of the first ordinal that does not chain); a wave sums its k0, plain and weighted by
//                    2 * (place in the piece) + 1, and adds each sum once (J8);
//   dj_rec_kernel    sixteen lanes per record: the MdRec (md_rec_of).
// At finish, over all n entries:
//   three stable rocPRIM radix sorts of (key, entry index), least significant first: L (8 bits), k1, k0.  Entries lie in ordinal
//                    order, so every group of equal (L, k0, k1) comes out in ordinal order;
//   dj_head_kernel   lane per sorted slot: head[i] = 1 where (L, k0, k1) differs from slot i - 1's, and first[ordinal] = head[i]: the
//                    group's first slot holds its first record;
//   rocprim::inclusive_scan of first: a first record's template ordinal + 1 (J2: rank by first record, no sort of the groups);
//   dj_start_kernel  lane per sorted slot: tstart[template] = i at a head;
//   dj_tmpl_kernel   lane per template: walks its slots to the next head (MdWalk: rules 2-3 and 5 in ordinal order, atomicMin of
//                    ordinal << 2 | reason), scatters rec_tmpl[ordinal], picks the loc of its first primary or first record (J4);
//                    a lane's walk is as long as its group, which one name repeated through a file makes the whole file;
//   rocprim::select  twice: the ends, and their locs.
//   dj_counts_kernel lane per entry, behind md_decide: rule 13's record-level counts (LibCounter) and the records to be marked.
// dj_key_sum_kernel: J8's check before an apply, lane per record.  Every kernel is memory-bound; none uses scratch; only
// dj_counts_kernel uses LDS (1792 B).  Every index a kernel stores through is one it computed itself from the slot or the scan:
// two names with one key make one template, which can only change what is decided.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include "common.h"
#include "markdup_dev.h"

namespace bwams {
namespace {

// every lane of the block arrives; the wave's sum is added once
__device__ __forceinline__ void wave_add(unsigned long long *dst, unsigned long long v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

__global__ void __launch_bounds__(256) dj_key_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n, int64_t base, MdGroupsDev G,
                                                     uint64_t *k0, uint64_t *k1, uint8_t *len, bwams_dup_loc_t *loc,
                                                     unsigned long long *call) {
    unsigned long long sum = 0, wsum = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t *p = bam + rec_off[r];
        const uint32_t l_name = bam_l_name(p), L = l_name ? l_name - 1 : 0;
        uint64_t a, b;
        name_key(p + kBamName, L, &a, &b);
        bool ok;
        const bwams_dup_loc_t at = md_loc_of(p, G, &ok);
        if (!ok) atomicMin(call + 2, (unsigned long long)(base + r));
        k0[base + r] = a;
        k1[base + r] = b;
        len[base + r] = (uint8_t)L;
        loc[base + r] = at;
        sum += a;
        wsum += (2 * (unsigned long long)r + 1) * a;
    }
    wave_add(call, sum);
    wave_add(call + 1, wsum);
}

__global__ void __launch_bounds__(256) dj_rec_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n, int64_t base, MdRec *rec) {
    const int g = (int)(threadIdx.x & (kGroup - 1));
    const int64_t n_groups = (int64_t)gridDim.x * (blockDim.x / kGroup);
    // every lane of a group runs the same number of iterations (r depends on the group only), so md_rec_of's shuffles see all 16
    for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup; r < n; r += n_groups) {
        const MdRec m = md_rec_of(bam + rec_off[r], g);
        if (g == 0) rec[base + r] = m;
    }
}

__global__ void __launch_bounds__(256) dj_key_sum_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n, unsigned long long *out) {
    unsigned long long sum = 0, wsum = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t *p = bam + rec_off[r];
        const uint32_t l_name = bam_l_name(p);
        uint64_t a, b;
        name_key(p + kBamName, l_name ? l_name - 1 : 0, &a, &b);
        sum += a;
        wsum += (2 * (unsigned long long)r + 1) * a;
    }
    wave_add(out, sum);
    wave_add(out + 1, wsum);
}

__global__ void __launch_bounds__(256) dj_iota_kernel(uint32_t *idx, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) idx[i] = (uint32_t)i;
}

// k0s: k0 in sorted order; idx: the entry (= ordinal) of each slot
__global__ void __launch_bounds__(256) dj_head_kernel(const uint64_t *k0s, const uint64_t *k1, const uint8_t *len, const uint32_t *idx,
                                                      int64_t n, uint8_t *head, uint32_t *first) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t r = idx[i];
        bool h = true;
        if (i > 0) {
            const uint32_t q = idx[i - 1];
            h = k0s[i] != k0s[i - 1] || k1[r] != k1[q] || len[r] != len[q];
        }
        head[i] = h;
        first[r] = h;
    }
}

__global__ void __launch_bounds__(256) dj_start_kernel(const uint8_t *head, const uint32_t *idx, const uint32_t *tid, int64_t n,
                                                       uint32_t *tstart) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (head[i]) tstart[tid[idx[i]] - 1] = (uint32_t)i;
}

__global__ void __launch_bounds__(256) dj_tmpl_kernel(const MdRec *rec, const bwams_dup_loc_t *loc, const uint32_t *idx, const uint8_t *head,
                                                      const uint32_t *tstart, int64_t n_t, int64_t n, bwams_dup_end_t *tend, uint8_t *has,
                                                      bwams_dup_loc_t *tloc, uint32_t *rec_tmpl, unsigned long long *bad) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_t; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = tstart[t];
        MdWalk w;
        int64_t named = -1;                                  // J4: the first primary in add order
        for (int64_t i = s; i < n && (i == s || !head[i]); ++i) {
            const uint32_t r = idx[i];
            const MdRec m = rec[r];
            rec_tmpl[r] = (uint32_t)t;
            if (named < 0 && !(m.flag & 0x900)) named = r;
            w.step(r, m);
        }
        if (w.fault != ~0ULL) atomicMin(bad, w.fault);
        bwams_dup_end_t e;
        has[t] = w.end(rec, t, &e) ? 1 : 0;
        tend[t] = e;
        tloc[t] = loc[named >= 0 ? named : (int64_t)idx[s]];
    }
}

__global__ void __launch_bounds__(256) dj_counts_kernel(const MdRec *rec, const uint32_t *rec_tmpl, const bwams_dup_loc_t *tloc,
                                                        const uint8_t *dup, int64_t n, int n_lib, unsigned long long *counts,
                                                        unsigned long long *n_marked) {
    __shared__ unsigned int sh[kLdsLibs * kLibCounts];
    LibCounter c;
    c.init(sh, n_lib, counts);
    unsigned long long marked = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t f = rec[r].flag, t = rec_tmpl[r];
        marked += dup[t] != 0;
        if ((f & 4) || (f & 0x900)) c.add(tloc[t].lib, (f & 4) ? kUnmapped : kSecSup);
    }
    c.flush(n_lib);
    wave_add(n_marked, marked);
}

float ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

void launch_dj_entries(const uint8_t *bam, const int64_t *rec_off, int64_t n, int64_t base, const MdGroupsDev &G, DjEntries &E,
                       unsigned long long *call, int cu_count, hipStream_t st) {
    if (n <= 0) return;
    dj_key_kernel<<<grid_of(n, 256, cu_count), 256, 0, st>>>(bam, rec_off, n, base, G, E.k0.p, E.k1.p, E.len.p, E.loc.p, call);
    dj_rec_kernel<<<grid_of(n, 256 / kGroup, cu_count), 256, 0, st>>>(bam, rec_off, n, base, E.rec.p);
}

void launch_dj_key_sum(const uint8_t *bam, const int64_t *rec_off, int64_t n, unsigned long long *sum, int cu_count, hipStream_t st) {
    if (n > 0) dj_key_sum_kernel<<<grid_of(n, 256, cu_count), 256, 0, st>>>(bam, rec_off, n, sum);
}

void launch_dj_counts(const MdRec *rec, const uint32_t *rec_tmpl, const bwams_dup_loc_t *tloc, const uint8_t *dup, int64_t n, int n_lib,
                      unsigned long long *counts, unsigned long long *n_marked, int cu_count, hipStream_t st) {
    if (n > 0) dj_counts_kernel<<<grid_of(n, 256, cu_count), 256, 0, st>>>(rec, rec_tmpl, tloc, dup, n, n_lib, counts, n_marked);
}

int dj_join(const DjEntries &E, int64_t n_rec, DjScratch &S, DjJoined &J, const char *who, float ms[2], int cu_count, hipStream_t st) {
    J.n_t = J.n_e = 0;
    ms[0] = ms[1] = 0;
    if (n_rec == 0) return BWAMS_OK;
    const size_t n = (size_t)n_rec;
    const auto t0 = std::chrono::steady_clock::now();
    BWAMS_HIP(S.ka.ensure_n(n)); BWAMS_HIP(S.kb.ensure_n(n)); BWAMS_HIP(S.i1.ensure_n(n)); BWAMS_HIP(S.i2.ensure_n(n));
    BWAMS_HIP(S.first.ensure_n(n)); BWAMS_HIP(S.tid.ensure_n(n)); BWAMS_HIP(S.head.ensure_n(n)); BWAMS_HIP(S.info.ensure_n(2));
    BWAMS_HIP(J.rec_tmpl.ensure_n(n));
    uint64_t *ka = S.ka.p, *kb = S.kb.p;
    uint32_t *i1 = S.i1.p, *i2 = S.i2.p;
    uint8_t *len_out = S.kb.as<uint8_t>();                   // the sorted L of the first pass: nobody reads it
    size_t need = 0, tb = 0;
    BWAMS_HIP(rocprim::radix_sort_pairs(nullptr, tb, E.len.p, len_out, i1, i2, n, 0u, 8u, st));
    need = std::max(need, tb);
    BWAMS_HIP(rocprim::radix_sort_pairs(nullptr, tb, ka, kb, i1, i2, n, 0u, 64u, st));
    need = std::max(need, tb);
    BWAMS_HIP(rocprim::inclusive_scan(nullptr, tb, S.first.p, S.tid.p, n, rocprim::plus<uint32_t>(), st));
    need = std::max(need, tb);
    BWAMS_HIP(S.tmp.ensure(need));
    const unsigned g = grid_of(n_rec, 256, cu_count);
    dj_iota_kernel<<<g, 256, 0, st>>>(i1, n_rec);
    tb = need;
    BWAMS_HIP(rocprim::radix_sort_pairs(S.tmp.p, tb, E.len.p, len_out, i1, i2, n, 0u, 8u, st));
    launch_md_gather64(E.k1.p, i2, n_rec, ka, cu_count, st);
    tb = need;
    BWAMS_HIP(rocprim::radix_sort_pairs(S.tmp.p, tb, ka, kb, i2, i1, n, 0u, 64u, st));
    launch_md_gather64(E.k0.p, i1, n_rec, ka, cu_count, st);
    tb = need;
    BWAMS_HIP(rocprim::radix_sort_pairs(S.tmp.p, tb, ka, kb, i1, i2, n, 0u, 64u, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    ms[0] = ms_since(t0);
    const auto t1 = std::chrono::steady_clock::now();
    const uint32_t *idx = i2;                                // kb: k0 sorted; idx: each slot's entry
    dj_head_kernel<<<g, 256, 0, st>>>(kb, E.k1.p, E.len.p, idx, n_rec, S.head.p, S.first.p);
    tb = need;
    BWAMS_HIP(rocprim::inclusive_scan(S.tmp.p, tb, S.first.p, S.tid.p, n, rocprim::plus<uint32_t>(), st));
    uint32_t n_t = 0;
    BWAMS_HIP(hipMemcpyAsync(&n_t, S.tid.p + n_rec - 1, 4, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    const size_t nt = (size_t)n_t;
    BWAMS_HIP(S.tstart.ensure_n(nt)); BWAMS_HIP(S.tend.ensure_n(nt)); BWAMS_HIP(S.has.ensure_n(nt));
    BWAMS_HIP(J.tloc.ensure_n(nt)); BWAMS_HIP(J.ends.ensure_n(nt)); BWAMS_HIP(J.locs.ensure_n(nt));
    tb = 0;
    BWAMS_HIP(rocprim::select(nullptr, tb, J.tloc.p, S.has.p, J.locs.p, S.info.p + 1, nt, st));
    size_t tb2 = 0;
    BWAMS_HIP(rocprim::select(nullptr, tb2, S.tend.p, S.has.p, J.ends.p, S.info.p + 1, nt, st));
    BWAMS_HIP(S.tmp.ensure(std::max(tb, tb2)));
    const unsigned long long init[2] = {~0ULL, 0};
    BWAMS_HIP(hipMemcpyAsync(S.info.p, init, 16, hipMemcpyHostToDevice, st));
    dj_start_kernel<<<g, 256, 0, st>>>(S.head.p, idx, S.tid.p, n_rec, S.tstart.p);
    dj_tmpl_kernel<<<grid_of(n_t, 256, cu_count), 256, 0, st>>>(E.rec.p, E.loc.p, idx, S.head.p, S.tstart.p, n_t, n_rec, S.tend.p, S.has.p,
                                                               J.tloc.p, J.rec_tmpl.p, S.info.p);
    BWAMS_HIP(rocprim::select(S.tmp.p, tb, J.tloc.p, S.has.p, J.locs.p, S.info.p + 1, nt, st));
    BWAMS_HIP(rocprim::select(S.tmp.p, tb2, S.tend.p, S.has.p, J.ends.p, S.info.p + 1, nt, st));
    unsigned long long info[2];
    BWAMS_HIP(hipMemcpyAsync(info, S.info.p, 16, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    ms[1] = ms_since(t1);
    if (info[0] != ~0ULL) {
        set_last_error(std::string(who) + ": record " + std::to_string(info[0] >> 2) + ": " + md_reason_text((int)(info[0] & 3)));
        return BWAMS_ERR_UNSUPPORTED;
    }
    J.n_t = n_t;
    J.n_e = (int64_t)info[1];
    return BWAMS_OK;
}

}  // namespace bwams
