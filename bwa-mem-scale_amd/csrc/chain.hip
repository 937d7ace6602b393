// chain.hip — seed chaining and chain filtering on the device.
//
// Replaces, for a whole chunk of reads, the reference's
//   mem_chain_seeds   /root/reference/src/bwamem.cpp:789-959  (+ test_and_merge :379-421)
//   mem_chain_flt     bwamem.cpp:528-646  (+ mem_chain_weight :451-470)
// consuming the SMEMs and SA coordinates that the seeding stage left in HBM.  mem_flt_chained_seeds
// (bwamem.cpp:491-526) acts only on reads of ~1100 bases and more: this stage flags such reads, the
// re-scoring itself is seed_sw.hip.
//
// The work is sequential per read (each seed is tested against the chain found by an ordered
// lookup; then the read's chains are sorted and filtered pairwise) and reads are independent.
//   chain_lane_kernel   (chain_lane.hip) one lane per read with few seeds: chaining, chain weights, the sort
//                       and the filter, on the chip while the read's tree is one leaf; else chain_read<false>.
//   chain_wave_kernel   one wave per read with many seeds, heaviest reads first: the same code run
//                       in lockstep by 64 lanes (uniform loads = one request; lane 0 stores), the
//                       chain records and an ordered array of chain positions in LDS; a read in
//                       which a chain position repeats goes to chain_redo_kernel (B-tree, HBM).
//   chain_heavy_kernel  one wave per read with many chains: the sort runs on the whole wave over an
//                       LDS copy, the quadratic pairwise filter runs 64 candidates at a time.
// All state lives in HBM scratch indexed by the read's slice of the SA-coordinate array: a seed
// IS an SA hit, so every per-seed array shares the index space of sa_coord, and a chain is named
// by its first seed.  The latency of dependent loads is what a lane pays for, so the hot records
// are laid out to be fetched whole: a B-tree node carries its keys' positions (160 B, ten 16-byte
// loads in flight at once, searched in registers), and a chain record carries everything
// test_and_merge and mem_chain_weight read (64 B; the weight is maintained incrementally).
//
// Two generic pieces decide tie cases and are therefore kept behaviour-identical to klib:
//   * the ordered map is a B-tree of order t = 5 (what kb_init(chn, 512 + 8) gives for the
//     48-byte mem_chain_t, kbtree.h:64) with kbtree.h's search, split and insert rules, so that
//     equal positions resolve to the same chain and the in-order traversal is the same; while
//     all positions of a read are distinct the tree's shape cannot matter, and the wave tiers
//     use a plain sorted array until one repeats;
//   * chains are sorted by weight with ksort.h's introsort (median-of-3, 16-element cut-off,
//     final insertion sort, comb-sort depth fallback), which is not stable.
//
// Where the stage's code lives.  It is built as three code objects (chain_wave.h, at launch_chain_t, says what one cost):
//   chain_dev.h      records, size classes, the B-tree, the filter, chain_seeds_batch and chain_read: what all three compile
//   chain_wave.h     chain_wave_kernel, chain_redo_kernel, heavy_read, chain_heavy_kernel, the launch plan and launch_chain_t
//                    over it: what this file compiles for COUNT = false and chain_count.hip for COUNT = true
//   chain.hip        this file: the slice, count and emit kernels, the sort's test hook, the host helpers and launch_chain
//   chain_count.hip  launch_chain_counting = launch_chain_t<true>
//   chain_lane.hip   chain_lane_kernel over chain_dev.h, and launch_chain_lane
#include "chain_wave.h"

namespace bwams {
namespace {

// ---- the chaining kernel: one lane per read --------------------------------------------------
// lane per read: the read's slice of the sorted SMEM array and its seed count (the sort key that
// groups reads of similar cost into the same wave)
// a read's slice of the (rid, m, n)-sorted SMEM array from the array itself: lane per SMEM, a boundary where the read id changes (reads
// without SMEMs keep the zeroed [0, 0)).  A lane per read bisected the array twice: 46 dependent loads per read, 0.76 ms per million.
__global__ void chain_slice_kernel(ChainArgs A) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n_smem) return;
    const int64_t r = (int64_t)A.smem[i].rid;
    if (i == 0 || (int64_t)A.smem[i - 1].rid != r) A.slice[2 * r] = i;
    if (i + 1 == A.n_smem || (int64_t)A.smem[i + 1].rid != r) A.slice[2 * r + 1] = i + 1;
}
__global__ void chain_count_kernel(ChainArgs A, uint32_t *keys, uint32_t *vals) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = r < A.nseq;
    int64_t cnt = 0;
    if (live) {
        const int64_t beg = A.slice[2 * r], end = A.slice[2 * r + 1];
        cnt = beg < end ? A.sa_off[end] - A.sa_off[beg] : 0;
        keys[r] = (uint32_t)(cnt < 0xffffffffll ? cnt : 0xffffffffll);
        vals[r] = (uint32_t)r;
    }
    // class boundaries in the descending order: [0, c[0]) > L, [c[0], c[1]) > L1, [c[1], c[2]) > M, [c[2], c[3]) > M1,
    // [c[3], c[4]) > S, [c[4], c[5]) > lane tier; [0, c[6]) beyond XL, [c[6], c[0]) XL; [c[0], c[7]) class L, [c[7], c[1]) class L2;
    // [c[1], c[8]) class L1, [c[8], c[2]) class M2; [0, c[9]) beyond XL2 (HBM), [c[9], c[6]) XL2.  One atomic per wave and class.
    const int thr[10] = {kClassL, kClassL1, kClassM, kClassM1, kClassS, kLaneSeeds, kClassXL, kClassL2, kClassM2, kClassXL2};
    if (!__ballot(live && cnt > kLaneSeeds)) return;
#pragma unroll
    for (int c = 0; c < 10; ++c) {
        const unsigned long long m = __ballot(live && cnt > thr[c]);
        if (m && (threadIdx.x & 63) == 0) atomicAdd(&A.ctr->chain_class[c], (unsigned long long)__popcll(m));
    }
}

// flat chain and seed records.  Sixteen lanes per read, a lane per kept chain (sixteen chains a trip): the chains' seed offsets are a
// prefix sum of their seed counts inside the group, and every lane walks its own chain's seed list — a lane per read took the chains
// one after the other, three dependent loads each before the first seed (1.8 ms per million reads; 4.4 on the grch38_like genome)
__global__ __launch_bounds__(256) void chain_emit_kernel(ChainArgs A, const int64_t *__restrict__ chain_off, const int64_t *__restrict__ seed_off,
                                                         bwams_chain_t *chains, bwams_chain_seed_t *seeds) {
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int sub = threadIdx.x & 15;
    const bool live = r < A.nseq;                  // (whole 16-lane groups: the shuffles below stay inside a group)
    const int nk = live ? A.n_kept[r] : 0;
    if (nk == 0) return;
    const int64_t base = A.read_base[r];
    const uint2 *fl = A.flt + base;
    const int32_t *first = A.f_first + base;
    const int32_t *s_next = A.s_next + base;
    const int2 *s_ql = A.s_ql + base;
    const int64_t *pos = A.sa_coord + base;
    const ChainRec *crec = reinterpret_cast<const ChainRec *>(A.crec) + base;
    int64_t so0 = seed_off[r];
    const int64_t co = chain_off[r];
    const float frac = A.frac_rep[r];
    for (int j0 = 0; j0 < nk; j0 += 16) {
        const int j = j0 + sub;
        const bool has = j < nk;
        uint2 f = make_uint2(0u, 0u);
        ChainRec ch;
        ch.n = 0; ch.first_idx = -1; ch.rid = 0;
        if (has) { f = fl[j]; ch = crec[f.y]; }
        const int n = has ? ch.n : 0;
        int incl = n;                             // inclusive prefix of the seed counts over the group's sixteen lanes
        for (int d = 1; d < 16; d <<= 1) {
            const int o = __shfl_up(incl, d, 16);
            if (sub >= d) incl += o;
        }
        const int total = __shfl(incl, 15, 16);
        if (has) {
            int64_t so = so0 + (incl - n);
            bwams_chain_t c;
            c.seqid = (int32_t)r; c.cseed = 0;
            c.n = n;
            int m = 1;
            while (m < n) m <<= 1;               // SEEDS_PER_CHAIN = 1, doubled on demand (bwamem.cpp:398-412)
            c.m = m;
            c.first = first[j];
            c.rid = ch.rid;
            c.w_kept_alt = f.x;
            c.frac_rep = frac;
            c.pos = pos[ch.first_idx];
            c.seed_off = so;
            chains[co + j] = c;
            for (int32_t g = ch.first_idx; g >= 0; g = s_next[g]) {
                bwams_chain_seed_t sd;
                sd.rbeg = pos[g];
                sd.qbeg = s_ql[g].x; sd.len = s_ql[g].y; sd.score = sd.len;
                sd.done = 0; sd.pad0_[0] = sd.pad0_[1] = sd.pad0_[2] = 0;
                sd.aln = 0; sd.pad1_ = 0;
                seeds[so++] = sd;
            }
        }
        so0 += total;
    }
}

// test hook (bwams_debug_sort, which = 2): one wavefront sorts n {weight, index} pairs as the chain filter does, with LDS
// laid out like heavy_read's.  mode 0, 1: wave_flt_sort; 2: the sequential form by lane 0 on a copy in GLOBAL memory; 3 / 4:
// modes 1 / 2 with a depth budget of 2, so that the comb-sort fallback sorts nearly everything
constexpr int kFltTestN = 1024;
__global__ __launch_bounds__(64) void flt_sort_test_kernel(const uint2 *__restrict__ in, int n, int mode, int32_t *__restrict__ order,
                                                           uint2 *__restrict__ scratch) {
    __shared__ uint2 l_a[kFltTestN];
    __shared__ uint4 l_scr[kFltTestN];
    const int lane = threadIdx.x;
    if (mode == 2 || mode == 4) {
        for (int i = lane; i < n; i += 64) scratch[i] = in[i];
        __syncthreads();
        if (lane == 0) ks_introsort(scratch, n, FltLt(), mode == 4 ? 2 : 0);
        __syncthreads();
        for (int i = lane; i < n; i += 64) order[i] = (int32_t)scratch[i].y;
        return;
    }
    for (int i = lane; i < n; i += 64) l_a[i] = in[i];
    __syncthreads();
    wave_flt_sort(l_a, n, l_scr, lane, mode == 3 ? 2 : 0);
    for (int i = lane; i < n; i += 64) order[i] = (int32_t)l_a[i].y;
}

}  // namespace

size_t chain_node_bytes(int64_t n_sa, int64_t nseq) { return (size_t)((n_sa >> 1) + 2 * nseq + 4) * sizeof(Node); }
size_t chain_rec_bytes(int64_t n_sa) { return (size_t)(n_sa > 0 ? n_sa : 1) * sizeof(ChainRec); }

void launch_chain_count(const ChainArgs &A, uint32_t *keys, uint32_t *vals, hipStream_t st) {
    if (A.nseq <= 0) return;
    (void)hipMemsetAsync(A.slice, 0, (size_t)A.nseq * 16, st);
    if (A.n_smem > 0) chain_slice_kernel<<<(unsigned)((A.n_smem + 255) / 256), 256, 0, st>>>(A);
    chain_count_kernel<<<(unsigned)((A.nseq + 255) / 256), 256, 0, st>>>(A, keys, vals);
}

int launch_chain(const ChainArgs &A, const uint32_t *n_seeds, int cu_count, hipStream_t st, hipStream_t *aux,
                 hipEvent_t fork, hipEvent_t *join, bool count) {
    return count ? launch_chain_counting(A, n_seeds, cu_count, st, aux, fork, join) : launch_chain_t<false>(A, n_seeds, cu_count, st, aux, fork, join);
}
void launch_chain_emit(const ChainArgs &A, const int64_t *chain_off, const int64_t *seed_off, bwams_chain_t *chains,
                       bwams_chain_seed_t *seeds, hipStream_t st) {
    if (A.nseq <= 0) return;
    chain_emit_kernel<<<(unsigned)((A.nseq * 16 + 255) / 256), 256, 0, st>>>(A, chain_off, seed_off, chains, seeds);
}

int launch_flt_sort_test(const int64_t *w, int n, int mode, int32_t *order) {
    if (n < 0 || n > kFltTestN) return -1;
    std::vector<uint2> h((size_t)n + 1);
    for (int i = 0; i < n; ++i) h[i] = make_uint2((unsigned)w[i], (unsigned)i);
    DevBuf<uint2> d_in, d_scr;
    DevBuf<int32_t> d_ord;
    if (d_in.alloc(8 * (size_t)(n + 1)) != hipSuccess || d_scr.alloc(8 * (size_t)(n + 1)) != hipSuccess || d_ord.alloc(4 * (size_t)(n + 1)) != hipSuccess ||
        hipMemcpy(d_in.p, h.data(), 8 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) return -1;
    flt_sort_test_kernel<<<1, 64>>>(d_in.p, n, mode, d_ord.p, d_scr.p);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(order, d_ord.p, 4 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return 0;
}

}  // namespace bwams
