// recal.hip — base recalibration tables: observations and mismatches per read group, reported quality, machine cycle and dinucleotide
// context (the rules are in include/bwams.h above bwams_recal_open).
//
// The store and the tables are laid out as common.h says (RecalStore, RecalLayout).  An add:
//   recal_check_kernel    lane per record: rule 5.  *bad = min(*bad, record << 3 | reason).
//   recal_record_kernel   lane per record: rule 4's filter and rule 6's read group (aux_rg.h); key = 2 * group + (cycles negative), or
//                         n_keys for a record that does not count.  The records counted and the largest l_seq are reduced over the wave
//                         and added once per wave.
//   rocprim::radix_sort_pairs of (key, record) over the bits n_keys needs: a key's records lie together.
//   recal_items_kernel    one workgroup: key_first[k], the first sorted entry of key k (a binary search per key), and the item table: a
//                         key with n records has ceil(n / kRecalSlice) slices x B blocks of 64 cycles, B from the largest l_seq.
//   recal_base_kernel     the default path; no global atomic per base.  A workgroup of eight waves owns one item at a time: (key, block b
//                         of 64 cycles, slice of the key's records).  Its waves take the slice's records in turn; lane l of a wave holds
//                         cycle 64 b + 1 + l of the record, that is SEQ index i = cycle - 1, or l_seq - cycle under 0x10: the lanes of a
//                         record's round hold neighbouring bases and, within an M op, neighbouring nibbles of the store.  A lane finds the
//                         CIGAR op that holds its base from the record's start (recal_base), loads the store's word at the reference
//                         position, and counts in LDS: CYCLE as [94 qualities][64 lanes] 32-bit cells, observations in the low and
//                         errors in the high half (a record adds at most 1 to a cell, so kRecalSlice < 65536 keeps both halves exact):
//                         one ds_add per base, and cell (q, l) is bank l whatever q, so the lanes of a wave never meet in a bank;
//                         CONTEXT as [94][16] 64-bit cells (observations low, errors high): one ds_add_u64 per base.  36 KB a
//                         workgroup: four of them, 32 waves, share a CU.  At the item's end the non-zero cells go to HBM with 64-bit
//                         atomics; QUAL is folded there from the CYCLE cells (a wave sums a quality's 64 cells) and RG from QUAL.
//   recal_plain_kernel    BWAMS_RECAL_LDS=0: a wave per counted record, a lane per base in rounds of 64, one global atomic per update
//                         (up to eight a base).  The A/B baseline (tools/recal_rate.py) and the cross-check of every GPU test.
// The store's writers: recal_set_ref_kernel (host codes of one reference, a lane per word, the flags kept), recal_ref_index_kernel (the
// gather from an index, a lane per word, ref_gather.h) and recal_known_kernel (a lane per interval, atomicOr per word it touches:
// intervals overlap freely).
#include <algorithm>
#include "common.h"
#include "bam_rec.h"
#include "aux_rg.h"
#include "ref_gather.h"
#include "wave_ops.h"

namespace bwams {
namespace {

// rule 4 without its last test (the first QUAL byte), for a record at p
__device__ __forceinline__ bool head_counts(const uint8_t *p, const RecalFilter &f) {
    const int32_t rid = bam_ref_id(p);
    return !(bam_flag(p) & f.exclude) && (int32_t)bam_mapq(p) >= f.min_mapq && rid >= 0 && rid < f.n_ref && bam_n_cig(p) > 0 &&
           bam_l_seq(p) > 0;
}

__global__ void __launch_bounds__(256) recal_check_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, RecalFilter f,
                                                          int walk_aux, unsigned long long *bad) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t *p = bam + rec_off[r];
        const uint32_t n_cig = bam_n_cig(p), l_name = bam_l_name(p);
        const uint8_t *c = p + bam_cigar_at(l_name);
        bool any = false;
        int64_t qlen = 0;
        for (uint32_t k = 0; k < n_cig; ++k) {
            const uint32_t op = ld_u32(c + 4 * k), o = op & 15;
            any |= o > 8;
            if (op_takes_query(o)) qlen += op >> 4;
        }
        int why = -1;
        if (any) {
            why = kRecalBadOp;
        } else if (head_counts(p, f)) {
            const int64_t l_seq = bam_l_seq(p);
            bool found;
            int64_t v0, v1;
            if (bam_aux_at(l_name, n_cig, l_seq) > bam_end(p)) why = kRecalBadBounds;
            else if (!bam_has_qual(p, l_name, n_cig, l_seq)) why = -1;                         // rule 4 skips it
            else if (qlen != l_seq) why = kRecalBadLength;
            else if (l_seq > f.max_cycle) why = kRecalBadCycle;
            else if (walk_aux && !aux_first_rg(p, &found, &v0, &v1)) why = kRecalBadAux;
        }
        if (why >= 0) atomicMin(bad, (unsigned long long)r << 3 | (unsigned)why);
    }
}

__global__ void __launch_bounds__(256) recal_record_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, RecalFilter f,
                                                           MdGroupsDev G, uint32_t n_keys, uint32_t *keys, uint32_t *vals,
                                                           unsigned long long *call) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t rounded = (n_rec + 63) & ~(int64_t)63;                 // whole waves enter every round: the reductions need them
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rounded; r += stride) {
        bool counted = false;
        int32_t len = 0;
        if (r < n_rec) {
            const uint8_t *p = bam + rec_off[r];
            const int32_t l_seq = bam_l_seq(p);
            counted = head_counts(p, f) && bam_has_qual(p, bam_l_name(p), bam_n_cig(p), l_seq);
            uint32_t key = n_keys;
            if (counted) {
                key = rg_key(p, G);                                      // rule 6; rule 5 walked the aux fields already
                len = l_seq;
            }
            keys[r] = key;
            vals[r] = (uint32_t)r;
        }
        const uint64_t m = __ballot(counted);
        const int32_t mx = wave_max(len);
        if (lane == 0 && m) {
            atomicAdd(call + kRecalCallCounted, (unsigned long long)__popcll((unsigned long long)m));
            atomicMax(call + kRecalCallMaxLen, (unsigned long long)mx);
        }
    }
}

constexpr int kItemThreads = 256;

__global__ void __launch_bounds__(kItemThreads) recal_items_kernel(const uint32_t *keys, int64_t n_rec, uint32_t n_keys,
                                                                   const unsigned long long *call_max_len, uint32_t *key_first,
                                                                   int64_t *item_first, unsigned long long *n_items) {
    for (uint32_t k = threadIdx.x; k <= n_keys; k += blockDim.x) {       // the first entry whose key is at least k
        int64_t lo = 0, hi = n_rec;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (keys[mid] < k) lo = mid + 1;
            else hi = mid;
        }
        key_first[k] = (uint32_t)lo;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t blocks = ((int64_t)*call_max_len + 63) / 64;
        int64_t at = 0;
        for (uint32_t k = 0; k < n_keys; ++k) {
            item_first[k] = at;
            at += blocks * (((int64_t)key_first[k + 1] - key_first[k] + kRecalSlice - 1) / kRecalSlice);
        }
        item_first[n_keys] = at;
        *n_items = (unsigned long long)at;
    }
}

// What the lanes need of one counted record.
struct RecalRec {
    const uint8_t *cig, *seq, *qual;
    uint32_t n_cig;
    int32_t l_seq, l_ref;
    int64_t pos, nib0;                     // POS; the store's nibble of the reference's position 0
    bool rev;
};

__device__ __forceinline__ RecalRec rec_of(const uint8_t *p, const RecalStore &S) {
    RecalRec v;
    const uint32_t l_name = bam_l_name(p);
    const int32_t rid = bam_ref_id(p);
    v.n_cig = bam_n_cig(p);
    v.l_seq = bam_l_seq(p);
    v.cig = p + bam_cigar_at(l_name);
    v.seq = p + bam_seq_at(l_name, v.n_cig);
    v.qual = p + bam_qual_at(l_name, v.n_cig, v.l_seq);
    v.pos = bam_pos(p);
    v.rev = (bam_flag(p) & 0x10) != 0;
    v.l_ref = S.l_ref[rid];
    v.nib0 = S.ref_word[rid] * 8;
    return v;
}

// Rules 6 and 7 for SEQ index i of record v: false when the base is no observation; else its quality *q, its context *ctx (-1: none)
// and whether it is an error.  The lane walks the CIGAR from its start to the op that holds i.
__device__ __forceinline__ bool recal_base(const RecalStore &S, const RecalRec &v, int32_t i, int min_baseq, int *q, int *ctx, bool *err) {
    const uint32_t qual = v.qual[i], code = seq_code(v.seq, i);          // both loads leave before anything branches on either
    const int32_t j = v.rev ? i + 1 : i - 1;                             // the neighbour in sequencing order
    const uint32_t ncode = j >= 0 && j < v.l_seq ? seq_code(v.seq, j) : 0;
    int64_t q0 = 0, x0 = v.pos;
    uint32_t k = 0, o = 15;
    for (; k < v.n_cig; ++k) {
        const uint32_t op = ld_u32(v.cig + 4 * k);
        const int64_t len = op >> 4;
        o = op & 15;
        const bool tq = op_takes_query(o);
        if (tq && i < q0 + len) break;
        if (tq) q0 += len;
        if (op_takes_ref(o)) x0 += len;
    }
    if (k >= v.n_cig || !op_is_match(o)) return false;                   // the first: not reached, rule 5 made the query length l_seq
    const int b = base_of_code(code);
    if (b < 0 || (int)qual < min_baseq) return false;
    const int64_t x = x0 + (i - q0);
    if (x < 0 || x >= v.l_ref) return false;
    const int64_t nib = v.nib0 + x;
    const uint32_t s = (S.words[nib >> 3] >> (4 * (uint32_t)(nib & 7))) & 15;
    if (s >= 4) return false;                                            // N (4), or any code with the known flag (8 and up)
    *q = (int)min(qual, (uint32_t)(kRecalQuals - 1));
    *err = (int)s != b;
    const int nb = base_of_code(ncode);
    *ctx = nb < 0 ? -1 : recal_context(nb, b, v.rev);
    return true;
}

constexpr int kBaseThreads = 512;                                       // eight waves share a workgroup's tables: 32 waves a CU

__global__ void __launch_bounds__(kBaseThreads) recal_base_kernel(const uint8_t *bam, const int64_t *rec_off, RecalFilter f, RecalStore S,
                                                                  RecalLayout L, const uint32_t *vals, uint32_t n_keys,
                                                                  const uint32_t *key_first, const int64_t *item_first,
                                                                  const unsigned long long *n_items_p, unsigned long long *T,
                                                                  unsigned long long *call) {
    __shared__ uint32_t cyc[kRecalQuals * 64];
    __shared__ unsigned long long ctxt[kRecalQuals * kRecalContexts];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), n_waves = (int)(blockDim.x >> 6);
    const int64_t n_items = (int64_t)*n_items_p;
    const int64_t blocks = ((int64_t)call[kRecalCallMaxLen] + 63) / 64;
    for (int k = threadIdx.x; k < kRecalQuals * 64; k += blockDim.x) cyc[k] = 0;
    for (int k = threadIdx.x; k < kRecalQuals * kRecalContexts; k += blockDim.x) ctxt[k] = 0;
    __syncthreads();
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        uint32_t lo = 0, hi = n_keys;                                    // the last key whose first item is at or before `item` and that has items
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (item_first[mid] <= item) lo = mid;
            else hi = mid;
        }
        const uint32_t key = lo;
        const int64_t local = item - item_first[key];
        const int32_t block = (int32_t)(local % blocks);                 // neighbouring workgroups share a slice's records in cache
        const int64_t first = (int64_t)key_first[key] + (local / blocks) * kRecalSlice;
        const int64_t last = std::min<int64_t>(first + kRecalSlice, key_first[key + 1]);
        const int32_t cycle = 64 * block + 1 + lane;
        int64_t off = first + wave < last ? rec_off[vals[first + wave]] : 0;
        for (int64_t j = first + wave; j < last; j += n_waves) {
            const RecalRec v = rec_of(bam + off, S);
            if (j + n_waves < last) off = rec_off[vals[j + n_waves]];    // the next record's place: two loads that do not wait in its chain
            if (cycle > v.l_seq) continue;
            int q, ctx;
            bool err;
            if (!recal_base(S, v, v.rev ? v.l_seq - cycle : cycle - 1, f.min_baseq, &q, &ctx, &err)) continue;
            atomicAdd(cyc + q * 64 + lane, 1u | (uint32_t)err << 16);
            if (ctx >= 0) atomicAdd(ctxt + q * kRecalContexts + ctx, 1ULL | (unsigned long long)err << 32);
        }
        __syncthreads();
        const int64_t g = key >> 1;
        const int64_t col = ((key & 1) ? -(int64_t)cycle : (int64_t)cycle) + L.max_cycle;
        unsigned long long rg_sum = 0;
        for (int q = wave; q < kRecalQuals; q += n_waves) {
            const uint32_t v = cyc[q * 64 + lane];
            cyc[q * 64 + lane] = 0;
            const unsigned long long obs = v & 0xFFFFu, err = v >> 16;
            if (obs) {                                                   // a lane with a count has cycle <= l_seq <= max_cycle
                unsigned long long *cell = T + L.cycle() + 2 * ((g * kRecalQuals + q) * L.cols() + col);
                atomicAdd(cell, obs);
                if (err) atomicAdd(cell + 1, err);
            }
            const unsigned long long s = (unsigned long long)wave_sum((int64_t)(obs | err << 32));
            if (lane == 0 && s) {
                unsigned long long *cell = T + L.qual() + 2 * (g * kRecalQuals + q);
                atomicAdd(cell, s & 0xFFFFFFFFu);
                if (s >> 32) atomicAdd(cell + 1, s >> 32);
                rg_sum += s;                                             // at most 94 x 64 x kRecalSlice: no carry into the high half
            }
        }
        if (lane == 0 && rg_sum) {
            atomicAdd(T + L.rg() + 2 * g, rg_sum & 0xFFFFFFFFu);
            if (rg_sum >> 32) atomicAdd(T + L.rg() + 2 * g + 1, rg_sum >> 32);
            atomicAdd(call + kRecalCallBases, rg_sum & 0xFFFFFFFFu);
        }
        for (int k = threadIdx.x; k < kRecalQuals * kRecalContexts; k += blockDim.x) {
            const unsigned long long v = ctxt[k];
            if (!v) continue;
            ctxt[k] = 0;
            unsigned long long *cell = T + L.context() + 2 * (g * kRecalQuals * kRecalContexts + k);
            atomicAdd(cell, v & 0xFFFFFFFFu);
            if (v >> 32) atomicAdd(cell + 1, v >> 32);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) recal_plain_kernel(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, RecalFilter f,
                                                          RecalStore S, RecalLayout L, const uint32_t *keys, uint32_t n_keys,
                                                          unsigned long long *T, unsigned long long *call) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    int64_t n_bases = 0;
    for (int64_t r = wave; r < n_rec; r += n_waves) {
        const uint32_t key = keys[r];
        if (key >= n_keys) continue;
        const RecalRec v = rec_of(bam + rec_off[r], S);
        const int64_t g = key >> 1;
        for (int32_t i = lane; i < v.l_seq; i += 64) {
            int q, ctx;
            bool err;
            if (!recal_base(S, v, i, f.min_baseq, &q, &ctx, &err)) continue;
            const int64_t c = v.rev ? v.l_seq - i : i + 1;
            const int64_t col = ((key & 1) ? -c : c) + L.max_cycle;
            unsigned long long *cell[4] = {T + L.rg() + 2 * g, T + L.qual() + 2 * (g * kRecalQuals + q),
                                           T + L.cycle() + 2 * ((g * kRecalQuals + q) * L.cols() + col),
                                           ctx < 0 ? nullptr : T + L.context() + 2 * ((g * kRecalQuals + q) * kRecalContexts + ctx)};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (!cell[t]) continue;
                atomicAdd(cell[t], 1ULL);
                if (err) atomicAdd(cell[t] + 1, 1ULL);
            }
            ++n_bases;
        }
    }
    const int64_t s = wave_sum(n_bases);
    if (lane == 0 && s) atomicAdd(call + kRecalCallBases, (unsigned long long)s);
}

// nibble k of the word that holds positions [8 w, 8 w + 8) of a reference of length l_ref: code(pos), 4 past the reference's end
template <class Code> __device__ __forceinline__ uint32_t word_of_codes(int64_t w, int32_t l_ref, Code code) {
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int64_t pos = 8 * w + k;
        out |= (uint32_t)(pos < l_ref ? code(pos) : 4) << (4 * k);
    }
    return out;
}

__global__ void __launch_bounds__(256) recal_set_ref_kernel(uint32_t *words, int64_t first_word, const uint8_t *codes, int32_t l_ref) {
    const int64_t n = ((int64_t)l_ref + 7) / 8;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n; w += (int64_t)gridDim.x * blockDim.x)
        words[first_word + w] = (words[first_word + w] & 0x88888888u) | word_of_codes(w, l_ref, [&](int64_t pos) { return codes[pos]; });
}

__global__ void __launch_bounds__(256) recal_ref_index_kernel(uint32_t *words, const int64_t *ref_word, int32_t n_ref, int64_t n_words,
                                                              const uint8_t *ref0123, const bwams_contig_t *contigs,
                                                              const int64_t *hole_off, const int32_t *hole_len, int32_t n_holes) {
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (int64_t)gridDim.x * blockDim.x) {
        int32_t lo = 0, hi = n_ref - 1;                                  // the last reference whose first word is at or before w
        while (lo < hi) {
            const int32_t mid = lo + (hi - lo + 1) / 2;
            if (ref_word[mid] <= w) lo = mid;
            else hi = mid - 1;
        }
        const int64_t off = contigs[lo].offset;
        words[w] = (words[w] & 0x88888888u) | word_of_codes(w - ref_word[lo], (int32_t)contigs[lo].len, [&](int64_t pos) {
                       return ref_code_at(ref0123, off + pos, hole_off, hole_len, n_holes);
                   });
    }
}

__global__ void __launch_bounds__(256) recal_known_kernel(uint32_t *words, const int64_t *ref_word, const bwams_recal_site_t *sites,
                                                          int64_t n) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const bwams_recal_site_t s = sites[k];
        const int64_t a = ref_word[s.ref] * 8 + s.beg, b = ref_word[s.ref] * 8 + s.end;          // nibbles [a, b), a < b
        for (int64_t w = a >> 3; w <= (b - 1) >> 3; ++w) {
            const int lo = (int)std::max<int64_t>(a - 8 * w, 0), hi = (int)std::min<int64_t>(b - 8 * w, 8);      // nibbles [lo, hi) of word w
            const uint32_t upto_hi = hi == 8 ? 0x88888888u : 0x88888888u & ((1u << (4 * hi)) - 1);
            atomicOr(words + w, upto_hi & ~((1u << (4 * lo)) - 1));
        }
    }
}

}  // namespace

void launch_recal_check(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const RecalFilter &f, int walk_aux, unsigned long long *bad,
                        int cu_count, hipStream_t st) {
    if (n_rec > 0) recal_check_kernel<<<grid_of(n_rec, 256, cu_count, 16), 256, 0, st>>>(bam, rec_off, n_rec, f, walk_aux, bad);
}

void launch_recal_records(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const RecalFilter &f, const MdGroupsDev &G,
                          uint32_t n_keys, uint32_t *keys, uint32_t *vals, unsigned long long *call, int cu_count, hipStream_t st) {
    if (n_rec > 0) recal_record_kernel<<<grid_of(n_rec, 256, cu_count, 16), 256, 0, st>>>(bam, rec_off, n_rec, f, G, n_keys, keys, vals, call);
}

void launch_recal_items(const uint32_t *keys, int64_t n_rec, uint32_t n_keys, const unsigned long long *call_max_len, uint32_t *key_first,
                        int64_t *item_first, unsigned long long *n_items, hipStream_t st) {
    if (n_rec > 0) recal_items_kernel<<<1, kItemThreads, 0, st>>>(keys, n_rec, n_keys, call_max_len, key_first, item_first, n_items);
}

void launch_recal_bases(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const RecalFilter &f, const RecalStore &S,
                        const RecalLayout &L, const uint32_t *vals, uint32_t n_keys, const uint32_t *key_first, const int64_t *item_first,
                        const unsigned long long *n_items, unsigned long long *tables, unsigned long long *call, int cu_count, hipStream_t st) {
    if (n_rec <= 0) return;                                              // no more items than this exist; the workgroups beyond leave at once
    const int64_t most = ((int64_t)f.max_cycle + 63) / 64 * ((n_rec + kRecalSlice - 1) / kRecalSlice + n_keys);
    recal_base_kernel<<<grid_of(most, 1, cu_count, 16), kBaseThreads, 0, st>>>(bam, rec_off, f, S, L, vals, n_keys, key_first, item_first,
                                                                              n_items, tables, call);
}

void launch_recal_plain(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const RecalFilter &f, const RecalStore &S,
                        const RecalLayout &L, const uint32_t *keys, uint32_t n_keys, unsigned long long *tables, unsigned long long *call,
                        int cu_count, hipStream_t st) {
    if (n_rec > 0) recal_plain_kernel<<<grid_of(n_rec, 4, cu_count, 16), 256, 0, st>>>(bam, rec_off, n_rec, f, S, L, keys, n_keys, tables, call);
}

void launch_recal_set_ref(uint32_t *words, int64_t first_word, const uint8_t *codes, int32_t l_ref, int cu_count, hipStream_t st) {
    if (l_ref > 0) recal_set_ref_kernel<<<grid_of(((int64_t)l_ref + 7) / 8, 256, cu_count, 16), 256, 0, st>>>(words, first_word, codes, l_ref);
}

void launch_recal_ref_index(uint32_t *words, const int64_t *ref_word, int32_t n_ref, int64_t n_words, const uint8_t *ref0123,
                            const bwams_contig_t *contigs, const int64_t *hole_off, const int32_t *hole_len, int32_t n_holes, int cu_count,
                            hipStream_t st) {
    if (n_words > 0 && n_ref > 0)
        recal_ref_index_kernel<<<grid_of(n_words, 256, cu_count, 16), 256, 0, st>>>(words, ref_word, n_ref, n_words, ref0123, contigs,
                                                                                   hole_off, hole_len, n_holes);
}

void launch_recal_known(uint32_t *words, const int64_t *ref_word, const bwams_recal_site_t *sites, int64_t n, int cu_count, hipStream_t st) {
    if (n > 0) recal_known_kernel<<<grid_of(n, 256, cu_count, 16), 256, 0, st>>>(words, ref_word, sites, n);
}

}  // namespace bwams
