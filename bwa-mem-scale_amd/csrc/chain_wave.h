// chain_wave.h — the wave tiers of the chaining stage (chain.hip has the stage's overview): chain_wave_kernel and chain_redo_kernel
// over chain_dev.h's chain_read, heavy_read and chain_heavy_kernel for the reads with many chains, the launch plan, and
// launch_chain_t, which launches it.  Two code objects compile this header, each for one value of COUNT: chain.hip (false) and
// chain_count.hip (true); launch_chain_t says why they are two.  Reads with few seeds, one lane per read, are chain_lane.hip's.
#pragma once
#include "chain_dev.h"

namespace bwams {
namespace {

// reads with many seeds: one wave (= one block) per read, B-tree and chain records in LDS.  The reads
// order[lo .. hi) (sorted by descending seed count, so a size class is a range) are handed out by ticket.
// K = 0: no LDS (reads too large for a CU's LDS): state in HBM scratch.
template <bool COUNT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) void chain_wave_kernel(ChainArgs A, const unsigned long long *lo_p, const unsigned long long *hi_p,
                                                        unsigned long long *ticket, int K) {
    extern __shared__ __align__(16) unsigned char l_mem[];
    const int lane = threadIdx.x;
    const int64_t lo = lo_p ? (int64_t)*lo_p : 0, hi = (int64_t)*hi_p;
    ChainRec *l_crec = reinterpret_cast<ChainRec *>(l_mem);
    Node *l_nodes = reinterpret_cast<Node *>(l_mem + (size_t)(K > 0 ? K : 0) * sizeof(ChainRec));
    for (;;) {
        const unsigned long long t = wave_ticket(ticket, 1ull);
        if (lo + (int64_t)t >= hi) break;
        const int64_t r = (int64_t)A.order[lo + (int64_t)t];
#ifdef BWAMS_CHAINDBG
        const unsigned long long tk0 = wall_clock64();
#endif
        if (K < 0) {                 // class XL: ordered array of -K chains in LDS, chain records in HBM
            if (!chain_read<true, 1, true, COUNT>(A, r, lane, 64, reinterpret_cast<Node *>(l_mem), 0, nullptr, -K) && lane == 0)
                A.redo[atomicAdd(&A.ctr->chain_redo, 1ull)] = (int32_t)r;
        } else if (K) {
            if (!chain_read<true, 1, false, COUNT>(A, r, lane, 64, l_nodes, 0, l_crec, K) && lane == 0)
                A.redo[atomicAdd(&A.ctr->chain_redo, 1ull)] = (int32_t)r;
        } else chain_read<false, 0, false, COUNT>(A, r, lane, 64, nullptr, 0, nullptr, 0);
        __syncthreads();
#ifdef BWAMS_CHAINDBG
        if (lane == 0) {
            const int c = K < 0 ? 0 : K == kClassL ? 1 : K == kClassL2 ? 2 : K == kClassL1 ? 3 : K == kClassM2 ? 4 : K == kClassM ? 5 : K == kClassM1 ? 6 : 7;
            const unsigned long long dt = wall_clock64() - tk0;
            atomicAdd(&A.ctr->dbg[32 + 3 * c], 1ull); atomicAdd(&A.ctr->dbg[33 + 3 * c], dt); atomicMax(&A.ctr->dbg[34 + 3 * c], dt);
        }
#endif
    }
}

// reads whose chain positions repeat: again, with the B-tree (state in HBM scratch, wave per read)
template <bool COUNT>
__global__ __launch_bounds__(64) void chain_redo_kernel(ChainArgs A) {
    const int lane = threadIdx.x;
    const int64_t n = (int64_t)A.ctr->chain_redo;
    for (;;) {
        const int64_t t = (int64_t)wave_ticket(&A.ctr->chain_redo_ticket, 1ull);
        if (t >= n) break;
        chain_read<false, 0, false, COUNT>(A, A.redo[t], lane, 64, nullptr, 0, nullptr, 0);
    }
}

// ---- reads with many chains: one wave per read ---------------------------------------------------
// Size classes (chains per read): each class is its own launch with the LDS its largest read needs — 41 B per chain —
// so that the many reads with a few dozen chains run 12 waves to a CU instead of sharing the footprint of the rare read
// with thousands (reads in repeat families reach max_occ hits per SMEM: on a GRCh38-size index a read can carry > 2000
// chains, and the quadratic filter of such a read on one lane through HBM took 40 ms).  Every launch walks the whole
// list of many-chain reads with its own ticket counter and skips the other classes' reads.
constexpr int kHeavyCap[6] = {64, 128, 256, 512, 960, 3840};         // 2.7 / 5 / 10.5 / 21 / 39 / 157 KB of LDS
__host__ __device__ constexpr size_t heavy_lds_bytes(int cap) { return (size_t)cap * 41 + 64; }
static_assert(heavy_lds_bytes(kHeavyCap[5]) <= 160 * 1024, "the largest class must fit one CU's LDS");
static_assert(160 * 1024 / 41 <= 65535, "wave_ks_introsort's stopper lists are uint16_t: no LDS class may hold more chains");

// one read's sort, pairwise filter and totals by a whole wavefront.  lds: heavy_lds_bytes(cap) bytes, n_chn <= cap; fl[0 .. n_chn) in HBM
// holds the {weight, chain id} pairs in B-tree order.  All 64 lanes call this.
__device__ void heavy_read(const ChainArgs &A, int64_t r, int64_t base, int n_chn, unsigned char *lds, int cap, int lane) {
    uint4 *l_rec = reinterpret_cast<uint4 *>(lds);                       // by sorted position: {beg, end, w | alt, first}
    uint4 *l_sel = l_rec + cap;                // the kept ("selected") chains, in selection order: {beg, end, w | alt, position}
    uint2 *l_fl = reinterpret_cast<uint2 *>(l_sel + cap);
    uint8_t *l_kept = reinterpret_cast<uint8_t *>(l_fl + cap);
    const int L = (int)(A.cum[r + 1] - A.cum[r]);
    uint2 *fl = A.flt + base;
    const ChainRec *crec = reinterpret_cast<const ChainRec *>(A.crec) + base;
    const unsigned long long t_0 = __builtin_amdgcn_s_memtime();
    if (lane == 0) {
        const int bk = n_chn <= 32 ? 0 : n_chn <= 64 ? 1 : n_chn <= 128 ? 2 : n_chn <= 256 ? 3 : n_chn <= 512 ? 4 : n_chn <= 960 ? 5 : 6;
        atomicAdd(&A.ctr->dbg[bk], 1ull);
    }
    {
        __syncthreads();
        for (int i = lane; i < n_chn; i += 64) l_fl[i] = fl[i];
        __syncthreads();
        // ksort's introsort, operation for operation, by the whole wave; l_sel (16 B per chain, cap >= 64) is free until the
        // filter: it lends the sort its scratch, laid out as wave_flt_sort states
        wave_flt_sort(l_fl, n_chn, l_sel, lane);
        const unsigned long long t_1 = __builtin_amdgcn_s_memtime();
        for (int i = lane; i < n_chn; i += 64) {
            const uint2 f = l_fl[i];
            l_rec[i] = make_rec(A, crec[f.y], f.x);
            l_kept[i] = 0;
        }
        __syncthreads();
        // pairwise filter (mem_chain_flt, bwamem.cpp:575-617).  The sequential loop takes chain i through the chains selected so far,
        // in selection order, up to the first one that drops it; every selected chain it meets on the way with a large overlap
        // records i as its first shadowed chain if it has none yet.  Here SIXTY-FOUR candidates go through the selection at once, a
        // lane each: first through the chains selected before the batch (one broadcast LDS read per selected chain for all 64
        // lanes), then through the batch's own survivors in order (candidate l' is selected iff it is still alive when every
        // earlier candidate has been resolved; its record reaches the later lanes through v_readlane).  `first` is the SMALLEST
        // candidate that meets the chain: ds_min on the 0xffffffff-initialised field, issued by the lowest such lane — no round trip.
        // One candidate at a time against 64 selected chains per trip cost ~1800 cycles of latency per chain, whatever the selection's size.
        int n_sel = 1;
        if (lane == 0) { const uint4 r0 = l_rec[0]; l_sel[0] = make_uint4(r0.x, r0.y, r0.z, 0u); l_kept[0] = 3; }
        __syncthreads();
        const float mask_level = A.opt.mask_level, drop_ratio = A.opt.drop_ratio;
        const int max_gap = A.opt.max_chain_gap, min_dw = A.opt.min_seed_len << 1;
        for (int ib = 1; ib < n_chn; ib += 64) {
            const int i = ib + lane;
            const bool valid = i < n_chn;
            const uint4 ri = valid ? l_rec[i] : make_uint4(0, 0, 0, 0);
            const int bi = (int)ri.x, ei = (int)ri.y, wi = (int)(ri.z & 0x7fffffffu), li = ei - bi;
            const bool alt_i = (ri.z >> 31) != 0;
            const float fwi = (float)wi;
            bool alive = valid, large = false;
            const int n_sel0 = n_sel;
            for (int k0 = 0; k0 < n_sel0; k0 += 4) {
                uint4 rj[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) rj[u] = l_sel[k0 + u < n_sel0 ? k0 + u : n_sel0 - 1];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (k0 + u >= n_sel0) break;
                    const int bj = (int)rj[u].x, ej = (int)rj[u].y;
                    const int b_max = bj > bi ? bj : bi, e_min = ej < ei ? ej : ei;
                    const bool alt_j = (rj[u].z >> 31) != 0;
                    const int lj = ej - bj, min_l = li < lj ? li : lj;
                    const bool lg = alive && e_min > b_max && (!alt_j || alt_i) && (float)(e_min - b_max) >= (float)min_l * mask_level && min_l < max_gap;
                    const unsigned long long m_lg = __ballot(lg);
                    if (m_lg) {
                        if (lane == __builtin_ctzll(m_lg)) atomicMin(&l_rec[rj[u].w].w, (uint32_t)i);
                        if (lg) {
                            large = true;
                            const int wj = (int)(rj[u].z & 0x7fffffffu);
                            if (fwi < (float)wj * drop_ratio && wj - wi >= min_dw) alive = false;
                        }
                    }
                }
                if (!__ballot(alive)) break;
            }
            // the batch's own survivors, in order
            unsigned long long todo = __ballot(alive);
            while (todo) {
                const int lp = __builtin_ctzll(todo);                                    // alive, and every earlier candidate resolved: selected
                const int bj = __builtin_amdgcn_readlane(bi, lp), ej = __builtin_amdgcn_readlane(ei, lp);
                const uint32_t zj = (uint32_t)__builtin_amdgcn_readlane((int)ri.z, lp);
                if (lane == lp) { l_sel[n_sel] = make_uint4(ri.x, ri.y, ri.z, (uint32_t)i); l_kept[i] = large ? 2 : 3; }
                ++n_sel;
                const int b_max = bj > bi ? bj : bi, e_min = ej < ei ? ej : ei;
                const bool alt_j = (zj >> 31) != 0;
                const int lj = ej - bj, min_l = li < lj ? li : lj;
                const bool lg = alive && lane > lp && e_min > b_max && (!alt_j || alt_i) && (float)(e_min - b_max) >= (float)min_l * mask_level && min_l < max_gap;
                const unsigned long long m_lg = __ballot(lg);
                if (m_lg) {
                    if (lane == __builtin_ctzll(m_lg)) l_rec[ib + lp].w = (uint32_t)i;     // just selected: nobody has met it before
                    if (lg) {
                        large = true;
                        const int wj = (int)(zj & 0x7fffffffu);
                        if (fwi < (float)wj * drop_ratio && wj - wi >= min_dw) alive = false;
                    }
                }
                todo = __ballot(alive) & ~((2ull << lp) - 1ull);
            }
            __syncthreads();
        }
        for (int k = lane; k < n_sel; k += 64) {
            const int f = (int)l_rec[l_sel[k].w].w;
            if (f >= 0) l_kept[f] = 1;
        }
        __syncthreads();
        if (lane == 0) {
            const unsigned long long t_2 = __builtin_amdgcn_s_memtime();
            atomicAdd(&A.ctr->dbg[8], t_1 - t_0);
            atomicAdd(&A.ctr->dbg[9], t_2 - t_1);
            atomicMax(&A.ctr->dbg[12], t_1 - t_0);
            atomicMax(&A.ctr->dbg[13], t_2 - t_1);
            atomicMax(&A.ctr->dbg[14], (unsigned long long)n_chn);
            atomicMax(&A.ctr->dbg[15], (unsigned long long)n_sel);
            atomicAdd(&A.ctr->dbg[10], (unsigned long long)n_sel);
            atomicAdd(&A.ctr->dbg[11], (unsigned long long)n_chn);
        }
        // max_chain_extend (bwamem.cpp:618-625) can only bite when it is smaller than the chain count
        if (A.opt.max_chain_extend <= n_chn) {
            if (lane == 0) {
                int i, k;
                for (i = k = 0; i < n_chn; ++i) {
                    if (l_kept[i] == 0 || l_kept[i] == 3) continue;
                    if (++k >= A.opt.max_chain_extend) break;
                }
                for (; i < n_chn; ++i)
                    if (l_kept[i] < 3) l_kept[i] = 0;
            }
            __syncthreads();
        }
        // compaction of the kept chains and the read's totals, 64 chains at a time
        int32_t *first = A.f_first + base;
        int n_out = 0, n_seeds = 0;
        for (int ib = 0; ib < n_chn; ib += 64) {
            const int i = ib + lane;
            const int kp = i < n_chn ? (int)l_kept[i] : 0;
            const unsigned long long m = __ballot(kp != 0);
            if (kp) {
                const int o = n_out + __popcll(m & ((1ull << lane) - 1ull));
                const uint2 f = l_fl[i];
                const uint4 rc4 = l_rec[i];
                fl[o] = make_uint2(f.x | ((unsigned)kp << 29) | (rc4.z & 0x80000000u), f.y);
                first[o] = (int32_t)rc4.w;
                n_seeds += crec[f.y].n;
            }
            n_out += __popcll(m);
        }
        for (int d = 32; d >= 1; d >>= 1) n_seeds += __shfl_xor(n_seeds, d);
        if (lane == 0) {
            A.n_kept[r] = n_out;
            A.n_kept_seeds[r] = n_seeds;
            if (n_out) {
                const double min_l = A.opt.min_chain_weight ? (double)(1.1f * (float)A.opt.min_chain_weight) : (double)5.5f * log((double)L);
                if (!(min_l > (double)(0.05f * (float)L))) atomicAdd(&A.ctr->chain_longread, 1ull);
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void chain_heavy_kernel(ChainArgs A, const unsigned long long *n_heavy_p, int cap_lo, int cap,
                                                         unsigned long long *ticket) {
    extern __shared__ __align__(16) unsigned char l_heavy[];
    const int kLdsChains = cap;
    const int lane = threadIdx.x;
    const int64_t n_heavy = (int64_t)*n_heavy_p;
    for (;;) {
        const int64_t hi = (int64_t)wave_ticket(ticket, 1ull);
        if (hi >= n_heavy) break;
        const int64_t r = A.heavy[hi];
        const int64_t base = A.read_base[r];
        const int n_chn = A.n_chn[r];
        if (n_chn <= cap_lo || (n_chn > cap && cap != kHeavyCap[5])) continue;          // another class's read
        const int L = (int)(A.cum[r + 1] - A.cum[r]);
        uint2 *fl = A.flt + base;
        uint4 *rec = A.f_rec + base;
        int32_t *kept = A.f_kept + base;
        const ChainRec *crec = reinterpret_cast<const ChainRec *>(A.crec) + base;
        if (n_chn > kLdsChains) {              // beyond the LDS budget: the sequential form, on lane 0
            const unsigned long long t_0 = __builtin_amdgcn_s_memtime();
            if (lane == 0) {
                atomicAdd(&A.ctr->dbg[18], 1ull);            // a slot of its own: dbg[6] is heavy_read's bin for more than 960 chains
                ks_introsort(fl, n_chn, FltLt());
                for (int i = 0; i < n_chn; ++i) { rec[i] = make_rec(A, crec[fl[i].y], fl[i].x); kept[i] = 0; }
                filter_seq(A.opt, n_chn, rec, kept, A.f_sel + base);
                finish_read(A, r, base, n_chn, L);
                atomicAdd(&A.ctr->dbg[7], __builtin_amdgcn_s_memtime() - t_0);
            }
            continue;
        }
        heavy_read(A, r, base, n_chn, l_heavy, cap, lane);
    }
}

// The launch plan.  The classes are independent of each other: they run concurrently on LANES, streams forked from the batch's
// stream and joined back into it (one event out, one event per auxiliary lane back), and the filter of the many-chain reads follows
// in a second fork-join round on the same lanes.  A lane is a total order and a hardware queue completes its launches in order, so
// the plan says itself which launch waits for which; nothing is left to the streams that happen to share a queue
// (profiles/chain_plan.md has the traces and the plans that lost).  A row: lane, position in the lane, what to launch, grid blocks
// per CU.  Every class hands its reads out by ticket: the grid decides which block chains a read, not what a read produces.
//
// What the plan rests on:
//   * A class's grid is what its LDS admits per CU, so any of L2, L1, M2, M and the lane tier alone fills every CU's LDS, and S at
//     twelve per CU takes every wave slot (amdgpu_waves_per_eu(3, 3): twelve chaining waves a CU).  Classes XL2, XL and L want 156,
//     49 and 102 KB on ONE CU for each of their few reads, which last milliseconds; behind a class that has filled the CUs their
//     blocks wait until it drains (L 10.2 ms instead of 3.1 with S starting beside it; 8.4 with L2 at the fork; XL2 once 42 ms on
//     the grch38_like genome).  So every lane BEGINS with one of them, or with the HBM tier, whose blocks find no read and leave
//     within 60 us: by then the blocks of XL2, XL and L are placed.  Their blocks without a read leave at once.
//   * There are three such beginnings, hence three lanes.  A fourth lane, begun by L2, measured slower (17.9 against 16.3 ms).
//   * Behind the beginnings the LDS is the currency: the lanes are balanced by duration, longest first, and the lane tier, which
//     runs best with the chip to itself, comes last on the lane of S, the class that leaves the most LDS free.
//   * S at ten blocks per CU instead of twelve leaves two wave slots a CU to the classes beside it (16.5 -> 16.2 ms).
enum : int8_t { kRunXL2, kRunHbm, kRunXL, kRunL, kRunL2, kRunL1, kRunM2, kRunM, kRunM1, kRunS, kRunLaneTier };
struct PlanRow { int8_t lane, pos, run, per_cu; };
// Lane 0 is the batch's stream, which does not wait for the fork event; lanes 1 and 2 are aux[0] and aux[2].  (A process has
// four hardware queues and the runtime puts a new stream on the least used one; the null stream and the seeding's side stream hold
// one each, and aux[0] and aux[1] come to share the fourth — kernel trace.  Two lanes on one queue are one lane.)
constexpr int kLanes = 3;
constexpr int kLaneAux[kLanes] = {-1, 0, 2};
constexpr PlanRow kWavePlan[11] = {
    {0, 0, kRunXL2, 1}, {0, 1, kRunXL, 1},  {0, 2, kRunL1, 3}, {0, 3, kRunM, 5},
    {1, 0, kRunL, 1},   {1, 1, kRunM1, 8},  {1, 2, kRunL2, 2}, {1, 3, kRunM2, 4},
    {2, 0, kRunHbm, 8}, {2, 1, kRunS, 10},  {2, 2, kRunLaneTier, 0}};
// The filter of the many-chain reads; `run` is the class (kHeavyCap's index).  The class of the longest reads (a whole CU's LDS per
// read, a few dozen reads per million) is first on the batch's stream for the reason XL2 is: behind the other classes its blocks
// found no CU with 157 KB free until those drained (16.8 ms for 26 reads of ~4 ms).  A wave of this kernel runs on LDS latency,
// so what a class's footprint leaves of a CU's occupancy is its speed: five classes below it, the large ones first on their lanes.
constexpr PlanRow kHeavyPlan[6] = {{0, 0, 5, 1}, {0, 1, 1, 16}, {1, 0, 4, 4}, {1, 1, 2, 12}, {2, 0, 0, 24}, {2, 1, 3, 7}};
// a wave class: its reads are order[chain_class[lo] .. chain_class[hi]) (lo < 0: from 0), its ticket, chain_wave_kernel's K
struct WaveClass { int8_t lo, hi, ticket; int K; };
constexpr WaveClass kWaveClass[10] = {{9, 6, 9, -kClassXL2}, {-1, 9, 0, 0},       {6, 0, 6, -kClassXL}, {0, 7, 1, kClassL},  {7, 1, 7, kClassL2},
                                      {1, 8, 2, kClassL1},   {8, 2, 8, kClassM2}, {2, 3, 3, kClassM},   {3, 4, 4, kClassM1}, {4, 5, 5, kClassS}};
constexpr size_t wave_class_lds(int K) { return K < 0 ? lds_bytes_xl(-K) : K > 0 ? lds_bytes(K) : 0; }
template <int N> constexpr bool plan_ok(const PlanRow (&p)[N]) {   // rows lane by lane, positions counted from 0, every launch once
    unsigned seen = 0;
    for (int i = 0; i < N; ++i) {
        const bool first = i == 0 || p[i - 1].lane != p[i].lane;
        if (p[i].lane < 0 || p[i].lane >= kLanes || (i && p[i].lane < p[i - 1].lane)) return false;
        if (p[i].pos != (first ? 0 : p[i - 1].pos + 1)) return false;
        if (p[i].run < 0 || p[i].run >= N || (seen >> p[i].run & 1)) return false;
        seen |= 1u << p[i].run;
    }
    return true;
}
static_assert(plan_ok(kWavePlan) && plan_ok(kHeavyPlan), "a plan lists every launch once, lane by lane");
static_assert(kWavePlan[0].run == kRunXL2 && kHeavyPlan[0].run == 5, "the whole-CU classes go first on the batch's stream");

static int lanes_fork(hipStream_t st, hipStream_t *aux, hipEvent_t fork) {
    if (hipEventRecord(fork, st) != hipSuccess) return -1;
    for (int l = 1; l < kLanes; ++l)
        if (hipStreamWaitEvent(aux[kLaneAux[l]], fork, 0) != hipSuccess) return -1;
    return 0;
}
static int lanes_join(hipStream_t st, hipStream_t *aux, hipEvent_t *join) {
    for (int l = 1; l < kLanes; ++l) {
        if (hipEventRecord(join[l - 1], aux[kLaneAux[l]]) != hipSuccess) return -1;
        if (hipStreamWaitEvent(st, join[l - 1], 0) != hipSuccess) return -1;
    }
    return 0;
}

// COUNT: the instances that count into ctr->dbg (bwams_debug_chain_counts); a production launch runs the ones without any counting code.
// Each translation unit that includes this header instantiates ONE of the two: chain.hip COUNT = false (launch_chain), chain_count.hip
// COUNT = true (launch_chain_counting).  With both in ONE code object the compiler allocated the registers of chain_wave_kernel<false>
// and of the out-of-line heavy_read differently, and the chain stage measured 0.2 ms per million reads slower than before the counting
// instances existed; alone, chain.hip's kernels are instruction for instruction what they were then (the lane tier's
// chain_read<false> beside them cost registers the same way, hence chain_lane.hip).  chain_heavy_kernel has nothing conditional to
// count: the counting launch runs chain_count.hip's own copy.
template <bool COUNT>
static int launch_chain_t(const ChainArgs &A, const uint32_t *n_seeds, int cu_count, hipStream_t st, hipStream_t *aux,
                          hipEvent_t fork, hipEvent_t *join) {
    if (A.nseq <= 0) return 0;
    unsigned long long *cls = A.ctr->chain_class, *tk = A.ctr->chain_ticket;
    // the opt-in for more than 64 KB of dynamic LDS belongs to the CURRENT device: set per launch (a batch on a second GPU of the
    // process needs it too), and checked
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(chain_wave_kernel<COUNT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds_bytes_xl(kClassXL2)) != hipSuccess) return -1;
    if (lanes_fork(st, aux, fork)) return -1;
    for (const PlanRow &p : kWavePlan) {
        const hipStream_t q = p.lane ? aux[kLaneAux[p.lane]] : st;
        if (p.run == kRunLaneTier) {
            launch_chain_lane(A, q, COUNT);
            continue;
        }
        const WaveClass &c = kWaveClass[p.run];
        chain_wave_kernel<COUNT><<<(unsigned)(cu_count * p.per_cu), 64, wave_class_lds(c.K), q>>>(A, c.lo < 0 ? nullptr : cls + c.lo, cls + c.hi, tk + c.ticket, c.K);
    }
    if (lanes_join(st, aux, join)) return -1;
    chain_redo_kernel<COUNT><<<(unsigned)(cu_count * 2), 64, 0, st>>>(A);
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(chain_heavy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)heavy_lds_bytes(kHeavyCap[5])) != hipSuccess) return -1;
    if (lanes_fork(st, aux, fork)) return -1;
    for (const PlanRow &p : kHeavyPlan)
        chain_heavy_kernel<<<(unsigned)(cu_count * p.per_cu), 64, heavy_lds_bytes(kHeavyCap[p.run]), p.lane ? aux[kLaneAux[p.lane]] : st>>>(
            A, &A.ctr->n_heavy, p.run ? kHeavyCap[p.run - 1] : 0, kHeavyCap[p.run], A.ctr->heavy_tickets + p.run);
    return lanes_join(st, aux, join);
}

}  // namespace
}  // namespace bwams
