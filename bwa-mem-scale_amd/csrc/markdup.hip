// markdup.hip — duplicate marking of BAM records in HBM (bwams_bam_templates, bwams_dup_decide, bwams_bam_markdup).
//
// The rules are Picard MarkDuplicates' for query-grouped input, written out in include/bwams.h above bwams_bam_templates and
// restated in bwams/markdup.py.  Templates and their ends, over n_rec records at bam + rec_off[r] (the buffer holds 16 bytes of slack
// past its last record, as bwams_bam_run / _upload allocate it):
//   md_head_kernel   lane per record: head[r] = 1 where its name differs from the previous record's (rule 1);
//   rocprim::inclusive_scan of head: tid[r], the template's ordinal + 1;
//   md_rec_kernel    sixteen lanes per record: rtmpl[r] = tid[r] - 1, tstart[template] at a head; for a mapped primary the unclipped
//                    5' coordinate (rule 3: lane 0 walks the leading clips, lane 1 the trailing ones, every lane sums a share of the
//                    reference length) and the score (rule 4: QUAL read as aligned dwords, bytes >= 15 summed, capped per lane and
//                    after a cross-lane reduction), into a 16-byte MdRec;
//   md_tmpl_kernel   lane per template: walks its MdRecs in order, applies rule 2 and 3's refusals (the first fault ends the walk;
//                    atomicMin of record << 2 | reason over all templates gives the first record concerned) and builds its end (rule 5);
//   rocprim::select  of the templates that have an end: the ends, in template order.
// The decision (rule 6) over n_e ends of templates [0, n_t):
//   md_check_kernel  lane per end: the ends' bounds (a tmpl outside [0, n_t) would be a store out of bounds), the largest refID, the pairs;
//   md_pair_keys / md_frag_keys  the sort keys of the pairs (one slot per end) and of the fragments (two slots per end: a pair's two
//                    ends as paired fragments).  A position key is ref << 33 | (pos + 2^31) << 1 | strand; slots that hold nothing take
//                    ref = the largest refID + 1, so they group apart and are skipped;
//   stable rocPRIM radix sorts, least significant key first, over the bits the values need: pairs by (32767 - score) << tb | tmpl,
//                    then key 2, then key 1; fragments by (unpaired << 15 | 32767 - score) << tb | tmpl, then the key.  In each group
//                    of equal keys the first slot is then the one kept (for fragments: a paired fragment whenever the group holds one);
//   md_mark_pairs / md_mark_frags  lane per sorted slot: a pair slot that is not its group's first, an unpaired fragment slot that is
//                    not its group's first, writes dup[tmpl] = 1 (each template has one end, so no slot races another's byte).
// md_apply_kernel: lane per record, sets or clears 0x400 in FLAG's high byte (byte 19 of the record) from dup[rtmpl[r]].
// Rules 9-13 (bwams_bam_templates2, bwams_dup_decide2, bwams_bam_markdup2); none of this is launched by the calls of rules 1-8:
//   md_loc_kernel    lane per template, a pass of its own behind md_tmpl_kernel (md_rec_kernel's sixteen lanes and 45 VGPRs stay as
//                    they are): the record rule 9 names; with a table its aux fields walked by type to block_size (atomicMin of the
//                    first record that does not chain), the RG:Z value looked up by binary search in the table's IDs sorted by
//                    bytes; the name's colons counted and its three fields parsed (rule 10); one bwams_dup_loc_t per template, and
//                    rocprim::select with the ends' flags gives one per end;
//   md_check_loc / md_lib_ends_fold  the ends' libraries checked; with n_lib > 1 a copy of the ends whose refIDs are
//                    library * (largest refID + 1) + refID, so that the position keys above carry the library as their most
//                    significant part (rule 11) and the sorts and mark kernels run unchanged (the product must stay below 2^31);
//   optical clustering (rule 12), after md_mark_pairs while the pairs' slots lie sorted, a group's slots adjacent, its kept pair first:
//     md_opt_head / scan / md_opt_start   each slot's group and each group's first slot, so its size;
//     md_opt_keys      the slots of groups of 2..max_set members that have a location are keyed by (tile, x) and by (group, read
//                      group); two stable 64-bit radix sorts order them by (group, read group, tile, x), the others behind them;
//     md_opt_pts / md_opt_link   lane per sorted point: forward while the (group, read group) and tile are its own and x' - x <= d,
//                      joining the points also within d in y by union-find (find without compression, hook the larger root under
//                      the smaller with atomicMin).  A tree's root is its smallest slot whatever the schedule, in a group the
//                      best-ranked member, so the kept pair when the cluster holds it.  The scan is quadratic for many points at one
//                      x of one tile: Picard's own worst case, which max_set bounds;
//     md_opt_root / md_opt_mark  every slot's root; a cluster without the kept pair collects its smallest template ordinal
//                      (atomicMin); every member but the representative writes optical[tmpl] = 1;
//   md_lib_ends / md_lib_recs  rule 13's counts per library, lane per end and lane per record: a workgroup counts in 64 x 7 LDS words
//                    (1792 B) when n_lib <= 64 and adds what is not zero to global memory at its end; global atomics otherwise.
// Every kernel is memory-bound; none uses scratch, and only the two md_lib kernels use LDS.
#include <algorithm>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include "common.h"
#include "markdup_dev.h"

namespace bwams {
namespace {

constexpr int32_t kMaxRef = 1 << 30;                  // refIDs of the decision: [0, 2^30), so that ref << 33 and one more fit 64 bits

__global__ void __launch_bounds__(256) md_head_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, uint32_t *head) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (int64_t)gridDim.x * blockDim.x) {
        uint32_t h = 1;
        if (r > 0) {
            const uint8_t *p = bam + rec_off[r - 1], *q = bam + rec_off[r];
            const uint32_t l = bam_l_name(p);
            if (l == bam_l_name(q)) {
                uint32_t k = 0;
                while (k < l && p[kBamName + k] == q[kBamName + k]) ++k;
                h = k < l;
            }
        }
        head[r] = h;
    }
}

__global__ void __launch_bounds__(256) md_rec_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const uint32_t *head,
                                                     const uint32_t *tid, uint32_t *rtmpl, uint32_t *tstart, MdRec *rec) {
    const int g = (int)(threadIdx.x & (kGroup - 1));
    const int64_t n_groups = (int64_t)gridDim.x * (blockDim.x / kGroup);
    // every lane of a group runs the same number of iterations (r depends on the group only), so the shuffles below see all 16
    for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup; r < n_rec; r += n_groups) {
        const MdRec m = md_rec_of(bam + rec_off[r], g);      // rules 3-4 (markdup_dev.h)
        if (g == 0) {
            const uint32_t t = tid[r] - 1;
            rtmpl[r] = t;
            if (head[r]) tstart[t] = (uint32_t)r;
            rec[r] = m;
        }
    }
}

__global__ void __launch_bounds__(256) md_tmpl_kernel(const MdRec *rec, const uint32_t *tstart, int64_t n_t, int64_t n_rec,
                                                      bwams_dup_end_t *tend, uint8_t *has, unsigned long long *bad) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_t; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r0 = tstart[t], r1 = t + 1 < n_t ? (int64_t)tstart[t + 1] : n_rec;
        MdWalk w;                                            // rules 2-3 and 5 (markdup_dev.h)
        for (int64_t r = r0; r < r1 && w.fault == ~0ULL; ++r) w.step(r, rec[r]);
        if (w.fault != ~0ULL) atomicMin(bad, w.fault);
        bwams_dup_end_t e;
        const uint8_t h = w.end(rec, t, &e) ? 1 : 0;
        tend[t] = e;
        has[t] = h;
    }
}

// info[0]: the first bad end (atomicMin); info[1]: the largest refID + 1 (atomicMax); info[2]: the pairs
__global__ void __launch_bounds__(256) md_check_kernel(const bwams_dup_end_t *ends, int64_t n_e, int64_t n_t, unsigned long long *info) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_e; i += (int64_t)gridDim.x * blockDim.x) {
        const bwams_dup_end_t e = ends[i];
        if (e.tmpl < 0 || e.tmpl >= n_t || e.ref1 < 0 || e.ref1 >= kMaxRef || e.ref2 < -1 || e.ref2 >= kMaxRef || e.score < 0 ||
            e.score > 32767 || e.strands < 0 || e.strands > 3 || (e.ref2 < 0 && (e.strands & 2)))
            atomicMin(info, (unsigned long long)i);
        atomicMax(info + 1, (unsigned long long)(uint32_t)max(e.ref1, e.ref2) + 1);
        if (e.ref2 >= 0) atomicAdd(info + 2, 1ULL);
    }
}

__device__ __forceinline__ uint64_t pos_key(int32_t ref, int32_t pos, int strand) {
    return (uint64_t)(uint32_t)ref << 33 | (uint64_t)((uint32_t)pos ^ 0x80000000u) << 1 | (uint64_t)strand;
}

__device__ __forceinline__ uint64_t rank_of(const bwams_dup_end_t &e, int tb) {      // (32767 - score) << tb | tmpl
    return (uint64_t)(32767 - e.score) << tb | (uint64_t)e.tmpl;
}

__global__ void __launch_bounds__(256) md_pair_keys_kernel(const bwams_dup_end_t *ends, int64_t n_e, int32_t none_ref, int tb,
                                                           uint64_t *k1, uint64_t *k2, uint64_t *v, uint32_t *idx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_e; i += (int64_t)gridDim.x * blockDim.x) {
        const bwams_dup_end_t e = ends[i];
        const bool pair = e.ref2 >= 0;
        k1[i] = pair ? pos_key(e.ref1, e.pos1, e.strands & 1) : pos_key(none_ref, 0, 0);
        k2[i] = pair ? pos_key(e.ref2, e.pos2, (e.strands >> 1) & 1) : 0;
        v[i] = rank_of(e, tb);
        idx[i] = (uint32_t)i;
    }
}

__global__ void __launch_bounds__(256) md_frag_keys_kernel(const bwams_dup_end_t *ends, int64_t n_e, int32_t none_ref, int tb,
                                                           uint64_t *k, uint64_t *w, uint32_t *idx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_e; i += (int64_t)gridDim.x * blockDim.x) {
        const bwams_dup_end_t e = ends[i];
        const bool pair = e.ref2 >= 0;
        const uint64_t rank = (uint64_t)(pair ? 0 : 1) << (15 + tb) | rank_of(e, tb);
        k[2 * i] = pos_key(e.ref1, e.pos1, e.strands & 1);
        k[2 * i + 1] = pair ? pos_key(e.ref2, e.pos2, (e.strands >> 1) & 1) : pos_key(none_ref, 0, 0);
        w[2 * i] = w[2 * i + 1] = rank;
        idx[2 * i] = (uint32_t)(2 * i);
        idx[2 * i + 1] = (uint32_t)(2 * i + 1);
    }
}

__global__ void __launch_bounds__(256) md_gather64_kernel(const uint64_t *src, const uint32_t *idx, int64_t n, uint64_t *dst) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[idx[i]];
}

__global__ void __launch_bounds__(256) md_gather32_kernel(const uint32_t *src, const uint32_t *idx, int64_t n, uint32_t *dst) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[idx[i]];
}

// pairs, sorted: ks = key 1 in sorted order, k2 = key 2 by end, idx = end of each slot
__global__ void __launch_bounds__(256) md_mark_pairs_kernel(const uint64_t *ks, const uint64_t *k2, const uint32_t *idx, int64_t n,
                                                            uint64_t none_key, const bwams_dup_end_t *ends, uint8_t *dup,
                                                            unsigned long long *n_dup) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t e = idx[i];
        if (i > 0 && ks[i] != none_key && ks[i] == ks[i - 1] && k2[e] == k2[idx[i - 1]]) {
            dup[ends[e].tmpl] = 1;
            atomicAdd(n_dup, 1ULL);
        }
    }
}

// fragment slots, sorted: ks = key in sorted order, idx = slot (end * 2 + which end)
__global__ void __launch_bounds__(256) md_mark_frags_kernel(const uint64_t *ks, const uint32_t *idx, int64_t n, uint64_t none_key,
                                                            const bwams_dup_end_t *ends, uint8_t *dup, unsigned long long *n_dup) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const bwams_dup_end_t &e = ends[idx[i] >> 1];
        if (i > 0 && ks[i] != none_key && e.ref2 < 0 && ks[i] == ks[i - 1]) {
            dup[e.tmpl] = 1;
            atomicAdd(n_dup, 1ULL);
        }
    }
}

__global__ void __launch_bounds__(256) md_apply_kernel(uint8_t *bam, const int64_t *rec_off, const uint32_t *perm, const uint32_t *rtmpl,
                                                       const uint8_t *dup, int64_t n_rec, unsigned long long *n_marked) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rec; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t r = perm ? perm[i] : (uint32_t)i;
        const bool d = dup[rtmpl[r]] != 0;
        uint8_t *f = bam + rec_off[i] + 19;                  // FLAG's high byte: 0x400 is its bit 2
        *f = (uint8_t)((*f & ~4u) | (d ? 4u : 0u));
        if (d) atomicAdd(n_marked, 1ULL);
    }
}

// ---- rules 9-10: a template's read group, library and location, lane per template ----

__global__ void __launch_bounds__(256) md_loc_kernel(const uint8_t *bam, const int64_t *rec_off, const MdRec *rec, const uint32_t *tstart,
                                                     int64_t n_t, int64_t n_rec, MdGroupsDev G, bwams_dup_loc_t *tloc,
                                                     unsigned long long *bad) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_t; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r0 = tstart[t], r1 = t + 1 < n_t ? (int64_t)tstart[t + 1] : n_rec;
        int64_t r = r0;
        while (r < r1 && (rec[r].flag & 0x900)) ++r;         // the first primary, else the first record
        if (r == r1) r = r0;
        bool ok;
        const bwams_dup_loc_t L = md_loc_of(bam + rec_off[r], G, &ok);     // rules 9-10 (markdup_dev.h)
        if (!ok) atomicMin(bad, (unsigned long long)r);
        tloc[t] = L;
    }
}

// ---- rule 13: counts per library, through markdup_dev.h's LibCounter ----

// lane per end: its template's kind and what the decision made of it, to the end's library (loc null: library 0)
__global__ void __launch_bounds__(256) md_lib_ends_kernel(const bwams_dup_end_t *ends, const bwams_dup_loc_t *loc, int64_t n_e,
                                                          const uint8_t *dup, const uint8_t *optical, int n_lib,
                                                          unsigned long long *counts) {
    __shared__ unsigned int sh[kLdsLibs * kLibCounts];
    LibCounter c;
    c.init(sh, n_lib, counts);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_e; i += (int64_t)gridDim.x * blockDim.x) {
        const bwams_dup_end_t e = ends[i];
        const int lib = loc ? loc[i].lib : 0;
        const bool pair = e.ref2 >= 0;
        c.add(lib, pair ? kPairEx : kUnpEx);
        if (dup[e.tmpl]) c.add(lib, pair ? kPairDup : kUnpDup);
        if (optical && optical[e.tmpl]) c.add(lib, kOptical);
    }
    c.flush(n_lib);
}

// lane per record: secondary or supplementary and mapped, or unmapped, to its template's library (tloc null: library 0)
__global__ void __launch_bounds__(256) md_lib_recs_kernel(const MdRec *rec, const uint32_t *rtmpl, const bwams_dup_loc_t *tloc, int64_t n_rec,
                                                          int n_lib, unsigned long long *counts) {
    __shared__ unsigned int sh[kLdsLibs * kLibCounts];
    LibCounter c;
    c.init(sh, n_lib, counts);
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t f = rec[r].flag;
        if (!(f & 4) && !(f & 0x900)) continue;
        c.add(tloc ? tloc[rtmpl[r]].lib : 0, (f & 4) ? kUnmapped : kSecSup);
    }
    c.flush(n_lib);
}

// ---- the ends' libraries checked, and folded into the refIDs of the keys (rule 11) ----

// info[0]: the first end whose loc is out of range (atomicMin)
__global__ void __launch_bounds__(256) md_check_loc_kernel(const bwams_dup_loc_t *loc, int64_t n_e, int n_lib, unsigned long long *info) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_e; i += (int64_t)gridDim.x * blockDim.x) {
        const bwams_dup_loc_t L = loc[i];
        if (L.lib < 0 || L.lib >= n_lib || (L.has != 0 && L.has != 1)) atomicMin(info, (unsigned long long)i);
    }
}

// ends2[i] = ends[i] with refID + lib * stride for each refID: equal places in two libraries become different places
__global__ void __launch_bounds__(256) md_lib_ends_fold_kernel(const bwams_dup_end_t *ends, const bwams_dup_loc_t *loc, int64_t n_e,
                                                               int32_t stride, bwams_dup_end_t *ends2) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_e; i += (int64_t)gridDim.x * blockDim.x) {
        bwams_dup_end_t e = ends[i];
        const int32_t add = loc[i].lib * stride;
        e.ref1 += add;
        if (e.ref2 >= 0) e.ref2 += add;
        ends2[i] = e;
    }
}

// ---- rule 12: optical duplicates, over the pairs' slots as the pair sort left them (a group's slots adjacent, the kept pair first) ----

// head[i] = 1 where slot i opens a group (a slot that holds no pair is a group of its own)
__global__ void __launch_bounds__(256) md_opt_head_kernel(const uint64_t *ks, const uint64_t *k2, const uint32_t *idx, int64_t n,
                                                          uint64_t none_key, uint32_t *head) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        head[i] = !(i > 0 && ks[i] != none_key && ks[i] == ks[i - 1] && k2[idx[i]] == k2[idx[i - 1]]);
}

__global__ void __launch_bounds__(256) md_opt_start_kernel(const uint32_t *head, const uint32_t *gid, int64_t n, uint32_t *gstart) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (head[i]) gstart[gid[i] - 1] = (uint32_t)i;
}

// per slot: the two sort keys of the eligible slots, (tile, x) and (group, read group); others take ~0 as the second and sort last.
// Every slot starts as a cluster of its own.
__global__ void __launch_bounds__(256) md_opt_keys_kernel(const bwams_dup_end_t *ends, const bwams_dup_loc_t *loc, const uint32_t *idx,
                                                          const uint32_t *gid, const uint32_t *gstart, int64_t n, int64_t max_set,
                                                          uint64_t *key_a, uint64_t *key_b, uint32_t *slot, uint32_t *parent) {
    const int64_t n_g = gid[n - 1];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t e = idx[i];
        const bwams_dup_loc_t L = loc[e];
        const int64_t g = (int64_t)gid[i] - 1;
        const int64_t size = (g + 1 < n_g ? (int64_t)gstart[g + 1] : n) - (int64_t)gstart[g];
        const bool el = L.has == 1 && ends[e].ref2 >= 0 && size >= 2 && size <= max_set;
        key_a[i] = (uint64_t)((uint32_t)L.tile ^ 0x80000000u) << 32 | (uint64_t)((uint32_t)L.x ^ 0x80000000u);
        key_b[i] = el ? (uint64_t)g << 32 | (uint64_t)(uint32_t)(L.rg + 1) : ~0ULL;
        slot[i] = (uint32_t)i;
        parent[i] = (uint32_t)i;
    }
}

struct OptPt { int32_t tile, x, y; uint32_t slot; };

__global__ void __launch_bounds__(256) md_opt_pts_kernel(const bwams_dup_loc_t *loc, const uint32_t *idx, const uint32_t *slot, int64_t n,
                                                         OptPt *pts) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const bwams_dup_loc_t L = loc[idx[slot[j]]];
        pts[j] = OptPt{L.tile, L.x, L.y, slot[j]};
    }
}

__device__ __forceinline__ uint32_t opt_find(const uint32_t *parent, uint32_t x) {
    for (uint32_t p = parent[x]; p != x; p = parent[x]) x = p;
    return x;
}

// parent[] only ever decreases and parent[x] <= x, so every tree's root is its smallest slot: in a group, the best-ranked member
__device__ __forceinline__ void opt_union(uint32_t *parent, uint32_t a, uint32_t b) {
    volatile uint32_t *vp = parent;
    for (;;) {
        while (vp[a] != a) a = vp[a];
        while (vp[b] != b) b = vp[b];
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

// lane per sorted point: forward over the points of its (group, read group) and tile while x' - x <= d; joins those close in y too
__global__ void __launch_bounds__(256) md_opt_link_kernel(const uint64_t *kb, const OptPt *pts, int64_t n, int64_t d, uint32_t *parent) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = kb[j];
        if (key == ~0ULL) continue;
        const OptPt a = pts[j];
        for (int64_t k = j + 1; k < n && kb[k] == key; ++k) {
            const OptPt b = pts[k];
            if (b.tile != a.tile || (int64_t)b.x - (int64_t)a.x > d) break;
            const int64_t dy = (int64_t)b.y - (int64_t)a.y;
            if (dy <= d && -dy <= d) opt_union(parent, a.slot, b.slot);
        }
    }
}

// lane per slot: root[i]; a cluster whose root is not its group's kept pair collects its smallest template ordinal
__global__ void __launch_bounds__(256) md_opt_root_kernel(const bwams_dup_end_t *ends, const uint32_t *idx, const uint32_t *head,
                                                          const uint32_t *parent, int64_t n, uint32_t *root, unsigned long long *min_t) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t r = opt_find(parent, (uint32_t)i);
        root[i] = r;
        if (!head[r]) atomicMin(min_t + r, (unsigned long long)ends[idx[i]].tmpl);
    }
}

__global__ void __launch_bounds__(256) md_opt_mark_kernel(const bwams_dup_end_t *ends, const uint32_t *idx, const uint32_t *head,
                                                          const uint32_t *root, const unsigned long long *min_t, int64_t n,
                                                          uint8_t *optical) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t r = root[i];
        const int64_t t = ends[idx[i]].tmpl;
        if (head[r] ? r != (uint32_t)i : (unsigned long long)t != min_t[r]) optical[t] = 1;
    }
}

int bit_width(uint64_t x) {
    int w = 0;
    while (w < 64 && (x >> w) != 0) ++w;
    return w;
}

const char *kReason[4] = {"two primaries of one segment", "a paired primary with neither or both of 0x40 / 0x80",
                          "paired and unpaired primaries mixed", "a mapped primary's unclipped 5' coordinate outside [-2^31, 2^31) or its refID -1"};
const char *kReasonAux = "aux fields do not chain to the record's end";

}  // namespace

const char *md_reason_text(int reason) { return reason >= 0 && reason < 4 ? kReason[reason] : kReasonAux; }

int md_templates(MdTemplates &m, const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, int cu_count, hipStream_t st) {
    m.n_t = m.n_e = 0;
    if (n_rec == 0) return BWAMS_OK;
    const size_t n = (size_t)n_rec;
    BWAMS_HIP(m.head.ensure(n * 4)); BWAMS_HIP(m.tid.ensure(n * 4)); BWAMS_HIP(m.rtmpl.ensure(n * 4));
    BWAMS_HIP(m.tstart.ensure(n * 4)); BWAMS_HIP(m.rec.ensure(n * sizeof(MdRec)));
    BWAMS_HIP(m.info.ensure(16));
    md_head_kernel<<<grid_of(n_rec, 256, cu_count), 256, 0, st>>>(bam, rec_off, n_rec, m.head.as<uint32_t>());
    size_t tb = 0;
    BWAMS_HIP(rocprim::inclusive_scan(nullptr, tb, m.head.as<const uint32_t>(), m.tid.as<uint32_t>(), n, rocprim::plus<uint32_t>(), st));
    BWAMS_HIP(m.tmp.ensure(tb));
    BWAMS_HIP(rocprim::inclusive_scan(m.tmp.p, tb, m.head.as<const uint32_t>(), m.tid.as<uint32_t>(), n, rocprim::plus<uint32_t>(), st));
    md_rec_kernel<<<grid_of(n_rec, 256 / kGroup, cu_count), 256, 0, st>>>(bam, rec_off, n_rec, m.head.as<const uint32_t>(),
                                                                          m.tid.as<const uint32_t>(), m.rtmpl.as<uint32_t>(),
                                                                          m.tstart.as<uint32_t>(), m.rec.as<MdRec>());
    uint32_t n_t = 0;
    BWAMS_HIP(hipMemcpyAsync(&n_t, m.tid.as<uint32_t>() + n_rec - 1, 4, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    BWAMS_HIP(m.tend.ensure((size_t)n_t * sizeof(bwams_dup_end_t))); BWAMS_HIP(m.ends.ensure((size_t)n_t * sizeof(bwams_dup_end_t)));
    BWAMS_HIP(m.has.ensure((size_t)n_t));
    const unsigned long long init[2] = {~0ULL, 0};
    BWAMS_HIP(hipMemcpyAsync(m.info.p, init, 16, hipMemcpyHostToDevice, st));
    md_tmpl_kernel<<<grid_of(n_t, 256, cu_count), 256, 0, st>>>(m.rec.as<const MdRec>(), m.tstart.as<const uint32_t>(), n_t, n_rec,
                                                                m.tend.as<bwams_dup_end_t>(), m.has.as<uint8_t>(),
                                                                m.info.as<unsigned long long>());
    tb = 0;
    BWAMS_HIP(rocprim::select(nullptr, tb, m.tend.as<const bwams_dup_end_t>(), m.has.as<const uint8_t>(), m.ends.as<bwams_dup_end_t>(),
                              m.info.as<unsigned long long>() + 1, (size_t)n_t, st));
    BWAMS_HIP(m.tmp.ensure(tb));
    BWAMS_HIP(rocprim::select(m.tmp.p, tb, m.tend.as<const bwams_dup_end_t>(), m.has.as<const uint8_t>(), m.ends.as<bwams_dup_end_t>(),
                              m.info.as<unsigned long long>() + 1, (size_t)n_t, st));
    unsigned long long info[2];
    BWAMS_HIP(hipMemcpyAsync(info, m.info.p, 16, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    if (info[0] != ~0ULL) {
        set_last_error("bwams_bam_templates: record " + std::to_string(info[0] >> 2) + ": " + kReason[info[0] & 3]);
        return BWAMS_ERR_UNSUPPORTED;
    }
    m.n_t = n_t;
    m.n_e = (int64_t)info[1];
    return BWAMS_OK;
}

// rules 9-10 over the templates md_templates left in m: m.tloc per template, m.locs per end (parallel to m.ends)
int md_locs(MdTemplates &m, const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const MdGroupsDev &G, int cu_count, hipStream_t st) {
    if (m.n_t == 0) return BWAMS_OK;
    const size_t n_t = (size_t)m.n_t;
    BWAMS_HIP(m.tloc.ensure(n_t * sizeof(bwams_dup_loc_t))); BWAMS_HIP(m.locs.ensure(n_t * sizeof(bwams_dup_loc_t)));
    BWAMS_HIP(m.info.ensure(16));
    const unsigned long long init[2] = {~0ULL, 0};
    BWAMS_HIP(hipMemcpyAsync(m.info.p, init, 16, hipMemcpyHostToDevice, st));
    md_loc_kernel<<<grid_of(m.n_t, 256, cu_count), 256, 0, st>>>(bam, rec_off, m.rec.as<const MdRec>(), m.tstart.as<const uint32_t>(), m.n_t,
                                                                 n_rec, G, m.tloc.as<bwams_dup_loc_t>(), m.info.as<unsigned long long>());
    size_t tb = 0;
    BWAMS_HIP(rocprim::select(nullptr, tb, m.tloc.as<const bwams_dup_loc_t>(), m.has.as<const uint8_t>(), m.locs.as<bwams_dup_loc_t>(),
                              m.info.as<unsigned long long>() + 1, n_t, st));
    BWAMS_HIP(m.tmp.ensure(tb));
    BWAMS_HIP(rocprim::select(m.tmp.p, tb, m.tloc.as<const bwams_dup_loc_t>(), m.has.as<const uint8_t>(), m.locs.as<bwams_dup_loc_t>(),
                              m.info.as<unsigned long long>() + 1, n_t, st));
    unsigned long long bad = 0;
    BWAMS_HIP(hipMemcpyAsync(&bad, m.info.p, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    if (bad != ~0ULL) {
        set_last_error("bwams_bam_templates: record " + std::to_string(bad) + ": " + kReasonAux);
        return BWAMS_ERR_UNSUPPORTED;
    }
    return BWAMS_OK;
}

// rule 13's two record-level counts of the templates in m, added to counts[lib * 7 + 5 .. 6] (device); tloc null: library 0
void launch_md_lib_recs(const MdTemplates &m, int64_t n_rec, const bwams_dup_loc_t *tloc, int n_lib, unsigned long long *counts,
                        int cu_count, hipStream_t st) {
    if (n_rec > 0)
        md_lib_recs_kernel<<<grid_of(n_rec, 256, cu_count), 256, 0, st>>>(m.rec.as<const MdRec>(), m.rtmpl.as<const uint32_t>(), tloc, n_rec,
                                                                          n_lib, counts);
}

int md_decide(MdDecide &w, const bwams_dup_end_t *ends, int64_t n_e, int64_t n_t, uint8_t *dup, int64_t counts[3], int cu_count,
              hipStream_t st, const MdDecideMore *x) {
    counts[0] = counts[1] = counts[2] = 0;                   // pairs, pair duplicates, fragment duplicates
    if (n_t > 0) BWAMS_HIP(hipMemsetAsync(dup, 0, (size_t)n_t, st));
    if (n_e == 0) return BWAMS_OK;
    if (n_e > 0x7FFFFFFFLL || n_t >= (1LL << 47)) {
        set_last_error("bwams_dup_decide: more than 2^31 - 1 ends or 2^47 templates");
        return BWAMS_ERR_UNSUPPORTED;
    }
    const size_t n2 = 2 * (size_t)n_e;
    BWAMS_HIP(w.info.ensure(32));
    const unsigned long long init[4] = {~0ULL, 0, 0, ~0ULL};
    BWAMS_HIP(hipMemcpyAsync(w.info.p, init, 32, hipMemcpyHostToDevice, st));
    unsigned long long *info = w.info.as<unsigned long long>();
    const bwams_dup_loc_t *loc = x ? x->loc : nullptr;
    md_check_kernel<<<grid_of(n_e, 256, cu_count), 256, 0, st>>>(ends, n_e, n_t, info);
    if (loc) md_check_loc_kernel<<<grid_of(n_e, 256, cu_count), 256, 0, st>>>(loc, n_e, x->n_lib, info + 3);
    unsigned long long h[4];
    BWAMS_HIP(hipMemcpyAsync(h, info, 32, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    if (h[0] != ~0ULL) {
        set_last_error("bwams_dup_decide: end " + std::to_string(h[0]) + ": tmpl outside [0, n_templates), a refID outside [0, 2^30) "
                       "(ref2: -1 too), score outside [0, 32767] or strands outside [0, 3] (bit 1 without end 2)");
        return BWAMS_ERR_ARG;
    }
    if (h[3] != ~0ULL) {
        set_last_error("bwams_dup_decide: end " + std::to_string(h[3]) + ": loc.lib outside [0, n_lib) or loc.has outside {0, 1}");
        return BWAMS_ERR_ARG;
    }
    const bwams_dup_end_t *ends0 = ends;                     // as given: ends may become their folded copy
    int32_t none_ref = (int32_t)h[1];                        // the largest refID + 1: slots that hold nothing
    if (loc && x->n_lib > 1) {                               // rule 11: library l's refIDs become l * stride + refID
        const int32_t stride = none_ref;
        if ((int64_t)x->n_lib * stride >= (1LL << 31)) {
            set_last_error("bwams_dup_decide: n_lib * (the largest refID + 1) must stay below 2^31");
            return BWAMS_ERR_UNSUPPORTED;
        }
        BWAMS_HIP(w.e2.ensure((size_t)n_e * sizeof(bwams_dup_end_t)));
        md_lib_ends_fold_kernel<<<grid_of(n_e, 256, cu_count), 256, 0, st>>>(ends, loc, n_e, stride, w.e2.as<bwams_dup_end_t>());
        ends = w.e2.as<const bwams_dup_end_t>();
        none_ref = x->n_lib * stride;
    }
    const bool optical = loc && x->d > 0 && x->optical && h[2] > 0;
    const uint64_t none_key = (uint64_t)(uint32_t)none_ref << 33 | (uint64_t)0x80000000u << 1;
    const unsigned kb = (unsigned)(33 + bit_width((uint64_t)none_ref)), tb = (unsigned)std::max(1, bit_width((uint64_t)n_t));
    counts[0] = (int64_t)h[2];
    BWAMS_HIP(hipMemsetAsync(info + 2, 0, 16, st));           // the duplicates' counters of the two mark kernels
    BWAMS_HIP(w.k1.ensure(n2 * 8)); BWAMS_HIP(w.k2.ensure(n2 * 8)); BWAMS_HIP(w.ka.ensure(n2 * 8)); BWAMS_HIP(w.kb.ensure(n2 * 8));
    BWAMS_HIP(w.i1.ensure(n2 * 4)); BWAMS_HIP(w.i2.ensure(n2 * 4));
    uint64_t *k1 = w.k1.as<uint64_t>(), *k2 = w.k2.as<uint64_t>(), *ka = w.ka.as<uint64_t>(), *kbuf = w.kb.as<uint64_t>();
    uint32_t *i1 = w.i1.as<uint32_t>(), *i2 = w.i2.as<uint32_t>();
    size_t need = 0;
    const std::pair<size_t, unsigned> sorts[4] = {{(size_t)n_e, 15 + tb}, {(size_t)n_e, kb}, {n2, 16 + tb}, {n2, kb}};
    for (const auto &q : sorts) {
        size_t t = 0;
        BWAMS_HIP(rocprim::radix_sort_pairs(nullptr, t, ka, kbuf, i1, i2, q.first, 0u, q.second, st));
        need = std::max(need, t);
    }
    if (optical) {
        size_t t = 0;
        BWAMS_HIP(rocprim::radix_sort_pairs(nullptr, t, ka, kbuf, i1, i2, (size_t)n_e, 0u, 64u, st));
        need = std::max(need, t);
        t = 0;
        BWAMS_HIP(rocprim::inclusive_scan(nullptr, t, i1, i2, (size_t)n_e, rocprim::plus<uint32_t>(), st));
        need = std::max(need, t);
        BWAMS_HIP(w.opt.ensure(5 * (size_t)n_e * 4));
    }
    BWAMS_HIP(w.tmp.ensure(need));
    auto sort = [&](uint64_t *kin, uint32_t *vin, uint32_t *vout, size_t n, unsigned bits) {
        size_t t = need;
        return rocprim::radix_sort_pairs(w.tmp.p, t, kin, kbuf, vin, vout, n, 0u, bits, st);
    };
    const unsigned g1 = grid_of(n_e, 256, cu_count), g2 = grid_of((int64_t)n2, 256, cu_count);
    // pairs: by rank, then key 2, then key 1
    md_pair_keys_kernel<<<g1, 256, 0, st>>>(ends, n_e, none_ref, (int)tb, k1, k2, ka, i1);
    BWAMS_HIP(sort(ka, i1, i2, (size_t)n_e, 15 + tb));
    md_gather64_kernel<<<g1, 256, 0, st>>>(k2, i2, n_e, ka);
    BWAMS_HIP(sort(ka, i2, i1, (size_t)n_e, kb));
    md_gather64_kernel<<<g1, 256, 0, st>>>(k1, i1, n_e, ka);
    BWAMS_HIP(sort(ka, i1, i2, (size_t)n_e, kb));
    md_mark_pairs_kernel<<<g1, 256, 0, st>>>(kbuf, k2, i2, n_e, none_key, ends, dup, info + 2);
    if (optical) {                                           // rule 12, while kbuf / i2 hold the pairs' sorted key 1 and each slot's end
        uint32_t *head = w.opt.as<uint32_t>(), *gid = head + n_e, *gstart = gid + n_e, *parent = gstart + n_e, *v2 = parent + n_e;
        uint64_t *key_b = k1;                                // k1's first half; its second: every cluster's smallest template ordinal
        unsigned long long *min_t = reinterpret_cast<unsigned long long *>(k1 + n_e);
        OptPt *pts = reinterpret_cast<OptPt *>(k2);          // 16 bytes per end, as k2 has
        md_opt_head_kernel<<<g1, 256, 0, st>>>(kbuf, k2, i2, n_e, none_key, head);
        size_t t = need;
        BWAMS_HIP(rocprim::inclusive_scan(w.tmp.p, t, head, gid, (size_t)n_e, rocprim::plus<uint32_t>(), st));
        md_opt_start_kernel<<<g1, 256, 0, st>>>(head, gid, n_e, gstart);
        md_opt_keys_kernel<<<g1, 256, 0, st>>>(ends, loc, i2, gid, gstart, n_e, x->max_set, ka, key_b, i1, parent);
        BWAMS_HIP(sort(ka, i1, v2, (size_t)n_e, 64));
        md_gather64_kernel<<<g1, 256, 0, st>>>(key_b, v2, n_e, ka);
        BWAMS_HIP(sort(ka, v2, i1, (size_t)n_e, 64));
        md_opt_pts_kernel<<<g1, 256, 0, st>>>(loc, i2, i1, n_e, pts);
        md_opt_link_kernel<<<g1, 256, 0, st>>>(kbuf, pts, n_e, x->d, parent);
        BWAMS_HIP(hipMemsetAsync(min_t, 0xFF, (size_t)n_e * 8, st));
        uint32_t *root = gid;                                // the group ordinals are done with
        md_opt_root_kernel<<<g1, 256, 0, st>>>(ends, i2, head, parent, n_e, root, min_t);
        md_opt_mark_kernel<<<g1, 256, 0, st>>>(ends, i2, head, root, min_t, n_e, x->optical);
    }
    // fragments: by (unpaired, rank), then the key
    md_frag_keys_kernel<<<g1, 256, 0, st>>>(ends, n_e, none_ref, (int)tb, k1, ka, i1);
    BWAMS_HIP(sort(ka, i1, i2, n2, 16 + tb));
    md_gather64_kernel<<<g2, 256, 0, st>>>(k1, i2, (int64_t)n2, ka);
    BWAMS_HIP(sort(ka, i2, i1, n2, kb));
    md_mark_frags_kernel<<<g2, 256, 0, st>>>(kbuf, i1, (int64_t)n2, none_key, ends, dup, info + 3);
    if (x && x->lib_counts)
        md_lib_ends_kernel<<<g1, 256, 0, st>>>(ends0, loc, n_e, dup, x->optical, x->n_lib, x->lib_counts);
    BWAMS_HIP(hipMemcpyAsync(h, info + 2, 16, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    counts[1] = (int64_t)h[0];
    counts[2] = (int64_t)h[1];
    return BWAMS_OK;
}

void launch_md_apply(uint8_t *bam, const int64_t *rec_off, const uint32_t *perm, const uint32_t *rtmpl, const uint8_t *dup, int64_t n_rec,
                     unsigned long long *n_marked, int cu_count, hipStream_t st) {
    if (n_rec > 0) md_apply_kernel<<<grid_of(n_rec, 256, cu_count), 256, 0, st>>>(bam, rec_off, perm, rtmpl, dup, n_rec, n_marked);
}

void launch_md_gather64(const uint64_t *src, const uint32_t *idx, int64_t n, uint64_t *dst, int cu_count, hipStream_t st) {
    if (n > 0) md_gather64_kernel<<<grid_of(n, 256, cu_count), 256, 0, st>>>(src, idx, n, dst);
}

void launch_md_gather32(const uint32_t *src, const uint32_t *idx, int64_t n, uint32_t *dst, int cu_count, hipStream_t st) {
    if (n > 0) md_gather32_kernel<<<grid_of(n, 256, cu_count), 256, 0, st>>>(src, idx, n, dst);
}

}  // namespace bwams
