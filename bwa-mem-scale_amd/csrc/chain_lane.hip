// chain_lane.hip — the lane tier of the chaining stage: one lane per read of at most kLaneSeeds seeds.
//
// chain_dev.h's chain_read<false> keeps a read's whole working state in the read's HBM scratch, a line per lane and access: every
// lookup loads the root node again, every test_and_merge loads and stores a chain record, the sort and the filter walk small
// arrays element by element.  A read of the lane tier has at most 32 seeds and nearly always a handful of chains, and while the
// kbtree is ONE node — its root, a leaf of at most KB_MAXK = 9 keys — the same decisions can be taken with
//   * the leaf in registers (NodeR and node_search / sel_key / sel_pos, chain_dev.h's),
//   * the chain records, the filter's {weight, id} pairs, its records and its kept / selected marks in LDS, a row per lane,
// and every array the later kernels read (chain records, seed links, kept pairs, first shadowed chains, the per-read totals)
// written once.  A read that needs a tenth chain gives up: its lane chains it again from its first seed with chain_read<false>,
// unchanged, which rewrites everything the attempt had written (the attempt's decisions up to that seed are the ones the B-tree
// takes too, so the rewritten seed links are a superset with the same values).
// The reads come in the stage's descending seed-count order (A.order behind the wave tiers' range), so that a wavefront holds
// reads of nearly the same length.
// This file compiles chain_dev.h alone, for chain_read<false> and its helpers: the lane tier is a code object of its own
// (chain_wave.h, at launch_chain_t, says what a second set of kernels beside the wave tiers' cost), as chain_count.hip is for the
// counting instances.
#include "chain_dev.h"

namespace bwams {
namespace {

// A wavefront's on-chip state, a row per lane.  Rows of 9 records: 108, 36, 18 and 9 dwords, so that the lanes' accesses to
// the same element spread over the banks.  45 KB: three wavefronts to a CU.
struct LeafLds {
    ChainRec crec[64][KB_MAXK];          // by chain id
    uint4 rec[64][KB_MAXK];              // by sorted position, as filter_seq wants them
    uint2 fl[64][KB_MAXK];               // {weight, chain id}: leaf order, then sorted
    int32_t kept[64][KB_MAXK], sel[64][KB_MAXK];
};
static_assert(sizeof(LeafLds) <= 48 * 1024, "three wavefronts of the lane tier per CU");

// One read on one lane while its kbtree is a single leaf.  Returns false when the read needs a tenth chain.
// Every pointer into `S` is derived here from the __shared__ object and every helper is inlined, so that the accesses stay ds_*
// instructions (chain_dev.h, at chain_read, says what a flat access costs).
template <bool COUNT>
__device__ __forceinline__ bool chain_read_leaf(const ChainArgs &A, int64_t r, LeafLds &S, int lane) {
    A.n_kept[r] = 0;
    A.n_kept_seeds[r] = 0;
    A.read_base[r] = 0;
    A.n_chn[r] = 0;
    const bwams_smem_t *sm = A.smem;
    const int64_t beg = A.slice[2 * r], end = A.slice[2 * r + 1];
    const int L = (int)(A.cum[r + 1] - A.cum[r]);
    if (beg == end || L < A.opt.min_seed_len) return true;

    int b = 0, e = 0, l_rep = 0;                 // frac_rep, as chain_read
    for (int64_t i = beg; i < end; ++i) {
        const int sb = (int)sm[i].m, se = (int)sm[i].n + 1;
        if (sm[i].s <= (int64_t)A.opt.max_occ) continue;
        if (sb > e) { l_rep += e - b; b = sb; e = se; }
        else e = e > se ? e : se;
    }
    l_rep += e - b;
    A.frac_rep[r] = (float)l_rep / (float)L;

    const int64_t base = A.sa_off[beg];
    const int32_t cnt = (int32_t)(A.sa_off[end] - base);
    A.read_base[r] = base;
    if (cnt == 0) return true;
    const int64_t *pos = A.sa_coord + base;
    int32_t *s_next = A.s_next + base;
    int2 *s_ql = A.s_ql + base;
    ChainRec *crec = S.crec[lane];
    NodeR x;                                     // the root leaf
    x.n = 0; x.internal = 0;
#pragma unroll
    for (int t = 0; t < KB_MAXK; ++t) { x.pos[t] = 0; x.key[t] = 0; }
    RidCache rc;
    rc.lo = 0; rc.hi = -1; rc.rid = 0;
    const int64_t l_pac = A.bns.l_pac;

    for (int64_t i = beg; i < end; ++i) {
        const int qbeg = (int)sm[i].m, slen = (int)sm[i].n + 1 - (int)sm[i].m;
        const int32_t g0 = (int32_t)(A.sa_off[i] - base), g1 = (int32_t)(A.sa_off[i + 1] - base);
        for (int32_t g = g0; g < g1; ++g) {
            const int64_t rbeg = pos[g];
            const int rid = intv2rid(A.bns, rbeg, rbeg + slen, rc);
            if (rid < 0) continue;
            bool to_add = true, eq;
            const int at = node_search(x, rbeg, eq);         // kb_intervalp's slot in the leaf, and where kbt_put inserts behind
            if (at >= 0) {                                   // test_and_merge with the chain found
                const int32_t lower = sel_key(x, at);
                const int64_t fr = sel_pos(x, at);
                ChainRec ch = crec[lower];
                const int64_t lr = ch.last_rbeg;
                const int64_t qend = ch.last_qbeg + ch.last_len, rend = lr + ch.last_len;
                if (rid != ch.rid) to_add = true;
                else if (qbeg >= ch.first_qbeg && qbeg + slen <= qend && rbeg >= fr && rbeg + slen <= rend) to_add = false;   // contained
                else if ((lr < l_pac || fr < l_pac) && rbeg >= l_pac) to_add = true;
                else {
                    const int64_t dx = qbeg - ch.last_qbeg, dy = rbeg - lr;
                    if (dy >= 0 && dx - dy <= A.opt.w && dy - dx <= A.opt.w && dx - ch.last_len < A.opt.max_chain_gap &&
                        dy - ch.last_len < A.opt.max_chain_gap) {
                        s_ql[g] = make_int2(qbeg, slen);
                        s_next[g] = -1;
                        s_next[ch.last_idx] = g;
                        if (qbeg >= ch.endq) ch.wq += slen; else if (qbeg + slen > ch.endq) ch.wq += qbeg + slen - ch.endq;
                        ch.endq = (uint16_t)((int)ch.endq > qbeg + slen ? (int)ch.endq : qbeg + slen);
                        if (rbeg >= ch.endr) ch.wr += slen; else if (rbeg + slen > ch.endr) ch.wr += (int)(rbeg + slen - ch.endr);
                        ch.endr = ch.endr > rbeg + slen ? ch.endr : rbeg + slen;
                        ch.last_rbeg = rbeg; ch.last_qbeg = (uint16_t)qbeg; ch.last_len = (uint16_t)slen; ch.last_idx = g; ch.n += 1;
                        crec[lower] = ch;
                        to_add = false;
                    }
                }
            }
            if (to_add) {
                if (x.n == KB_MAXK) return false;            // kbt_put would split the root
                s_ql[g] = make_int2(qbeg, slen);
                s_next[g] = -1;
                ChainRec ch;
                ch.last_rbeg = rbeg; ch.endr = rbeg + slen;
                ch.first_qbeg = (uint16_t)qbeg; ch.last_qbeg = (uint16_t)qbeg; ch.last_len = (uint16_t)slen; ch.endq = (uint16_t)(qbeg + slen);
                ch.rid = rid; ch.n = 1; ch.first_idx = g; ch.last_idx = g; ch.wq = slen; ch.wr = slen;
                const int32_t cid = x.n;                     // chains are numbered in creation order
                crec[cid] = ch;
                // kbt_put's insertion into a leaf that is not full: behind slot `at`
#pragma unroll
                for (int t = KB_MAXK - 1; t >= 1; --t)
                    if (t > at + 1 && t <= x.n) { x.key[t] = x.key[t - 1]; x.pos[t] = x.pos[t - 1]; }
#pragma unroll
                for (int t = 0; t < KB_MAXK; ++t)
                    if (t == at + 1) { x.key[t] = cid; x.pos[t] = rbeg; }
                x.n += 1;
            }
        }
    }
    const int n_keys = x.n;
    if (n_keys == 0) return true;

    // the leaf IS the traversal: weights and the weight floor in its order
    uint2 *fl = S.fl[lane];
    int n_chn = 0;
#pragma unroll
    for (int t = 0; t < KB_MAXK; ++t) {
        if (t < n_keys) {
            const int32_t id = x.key[t];
            const int wq = crec[id].wq, wr = crec[id].wr;
            int w = wr < wq ? wr : wq;
            w = w < (1 << 30) ? w : (1 << 30) - 1;
            if (t == 0) fl[0] = make_uint2((unsigned)w, (unsigned)id);       // a_[0] stays in place when everything is dropped
            if (w >= A.opt.min_chain_weight) { fl[n_chn] = make_uint2((unsigned)w, (unsigned)id); ++n_chn; }
        }
    }
    if (n_chn == 0) n_chn = 1;                   // the reference keeps a_[0] in that case (bwamem.cpp:549-572)
    A.n_chn[r] = n_chn;                          // at most KB_MAXK <= kLightChains: sorted and filtered here
    if constexpr (COUNT) atomicAdd(&A.ctr->dbg[17], 1ull);
    ChainRec *crec_g = reinterpret_cast<ChainRec *>(A.crec) + base;
    for (int k = 0; k < n_keys; ++k) crec_g[k] = crec[k];

    ks_introsort<1>(fl, n_chn, FltLt());         // (n_chn <= 9: the partition never pushes)
    uint4 *rec = S.rec[lane];
    int32_t *kept = S.kept[lane];
    for (int i = 0; i < n_chn; ++i) {
        rec[i] = make_rec(A, crec[fl[i].y], fl[i].x);
        kept[i] = 0;
    }
    [[clang::always_inline]] filter_seq(A.opt, n_chn, rec, kept, S.sel[lane]);

    // finish_read over the on-chip copies: max_chain_extend, compaction, per-read totals (bwamem.cpp:618-640)
    int i, k;
    for (i = k = 0; i < n_chn; ++i) {
        if (kept[i] == 0 || kept[i] == 3) continue;
        if (++k >= A.opt.max_chain_extend) break;
    }
    for (; i < n_chn; ++i)
        if (kept[i] < 3) kept[i] = 0;
    uint2 *fl_g = A.flt + base;
    int32_t *first_g = A.f_first + base;
    int n_seeds = 0;
    for (i = k = 0; i < n_chn; ++i) {
        if (kept[i] == 0) continue;
        const uint2 f = fl[i];
        const uint4 rc4 = rec[i];
        fl_g[k] = make_uint2(f.x | ((unsigned)kept[i] << 29) | (rc4.z & 0x80000000u), f.y);
        first_g[k] = (int32_t)rc4.w;
        n_seeds += crec[f.y].n;
        ++k;
    }
    A.n_kept[r] = k;
    A.n_kept_seeds[r] = n_seeds;
    if (k) {                                     // mem_flt_chained_seeds re-scores seeds only for long reads (min_l <= 0.05 * l_query)
        const double min_l = A.opt.min_chain_weight ? (double)(1.1f * (float)A.opt.min_chain_weight) : (double)5.5f * log((double)L);
        if (!(min_l > (double)(0.05f * (float)L))) atomicAdd(&A.ctr->chain_longread, 1ull);
    }
    return true;
}

// A.order is the stage's descending seed-count order and ctr->chain_class[5] the number of reads beyond kLaneSeeds (chain_count_kernel):
// the lane tier's reads are the rest of the order, the reads without a seed at its end (they get their zeroed outputs here too).
// The host does not know the range's start without a read-back, so the grid covers every read and the blocks behind the range
// leave at once.
template <bool COUNT>
__global__ __launch_bounds__(64) void chain_lane_kernel(ChainArgs A) {
    __shared__ LeafLds S;
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)A.ctr->chain_class[5] + (int64_t)blockIdx.x * 64 + lane;
    if (t >= A.nseq) return;
    const int64_t r = (int64_t)A.order[t];
    const bool done = chain_read_leaf<COUNT>(A, r, S, lane);
    const unsigned long long gave_up = __ballot(!done);
    if (!gave_up) return;
    if (lane == __builtin_ctzll(gave_up)) atomicAdd(&A.ctr->chain_lane_giveup, (unsigned long long)__popcll(gave_up));
    if (!done) chain_read<false, 0, false, COUNT>(A, r, 0, 1, nullptr, 0, nullptr, 0);
}

}  // namespace

void launch_chain_lane(const ChainArgs &A, hipStream_t st, bool count) {
    if (A.nseq <= 0) return;
    const unsigned grid = (unsigned)((A.nseq + 63) / 64);
    if (count) chain_lane_kernel<true><<<grid, 64, 0, st>>>(A);
    else chain_lane_kernel<false><<<grid, 64, 0, st>>>(A);
}

}  // namespace bwams
