// markdup_dev.h — what the duplicate-marking kernels of markdup.hip (templates of adjacent records) and dup_join.hip (templates
// joined by name) share on the device, one definition each: a record's unclipped 5' coordinate and score (rules 3-4), the walk over a
// template's records with its refusals and its end (rules 2 and 5), a record's read group, library and location (rules 9-10), and
// the per-library counter of rule 13.  The rules are in include/bwams.h above bwams_bam_templates.
#pragma once
#include "bam_rec.h"
#include "aux_rg.h"

namespace bwams {

constexpr int kMdQualMin = 15, kMdScoreCap = 16383;

__device__ __forceinline__ uint32_t qual_sum4(uint32_t w, uint32_t keep) {   // the bytes of w >= 15 that `keep` (bit per byte) selects
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t q = (w >> (8 * k)) & 0xFF;
        s += ((keep >> k) & 1) && q >= (uint32_t)kMdQualMin ? q : 0;
    }
    return s;
}

// The MdRec of the record at p, by the kGroup lanes that share it (g: the lane's place in its group; every lane of the group calls,
// and every lane returns the whole value).  For a mapped primary the unclipped 5' coordinate (rule 3: lane 0 walks the leading clips,
// lane 1 the trailing ones, every lane sums a share of the reference length) and the score (rule 4: QUAL read as aligned dwords,
// bytes >= 15 summed, capped per lane and after the cross-lane reduction); 0 and 0 for any other record.
__device__ __forceinline__ MdRec md_rec_of(const uint8_t *p, int g) {
    const int32_t rid = bam_ref_id(p), pos = bam_pos(p);
    const uint32_t l_name = bam_l_name(p), n_cig = bam_n_cig(p), flag = bam_flag(p);
    const int64_t l_seq = bam_l_seq(p);
    const bool want = !(flag & 0x904);                     // a mapped primary: its coordinate and score
    int64_t rlen = 0, clip = 0;
    uint32_t score = 0;
    if (want) {
        const uint8_t *c = p + bam_cigar_at(l_name);
        rlen = cigar_ref_len(c, n_cig, g, kGroup);
        if (g == 0 && !(flag & 16)) {                    // forward: the S and H lengths before the first other op
            for (uint32_t k = 0; k < n_cig; ++k) {
                const uint32_t op = ld_u32(c + 4 * k), o = op & 15;
                if (o != 4 && o != 5) break;
                clip += op >> 4;
            }
        }
        if (g == 1 && (flag & 16)) {                     // reverse: the S and H lengths after the last other op
            for (uint32_t k = n_cig; k-- > 0;) {
                const uint32_t op = ld_u32(c + 4 * k), o = op & 15;
                if (o != 4 && o != 5) break;
                clip += op >> 4;
            }
        }
        const uint8_t *qs = p + bam_qual_at(l_name, n_cig, l_seq);
        const int64_t n_q = min(l_seq, (int64_t)((p + 4 + bam_block_size(p)) - qs));     // never past the record's block_size
        if (n_q > 0 && qs[0] != 0xFF) {                   // QUAL present: aligned dwords over [qs, qs + n_q)
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(qs) & ~(uintptr_t)3;
            const uintptr_t e = reinterpret_cast<uintptr_t>(qs) + (uintptr_t)n_q;
            const int64_t n_dw = (int64_t)((e - a0 + 3) >> 2);
            const uint32_t *w = reinterpret_cast<const uint32_t *>(a0);
            for (int64_t k = g; k < n_dw; k += kGroup) {
                const uintptr_t at = a0 + 4 * (uintptr_t)k;
                uint32_t keep = 0xF;
                if (at < reinterpret_cast<uintptr_t>(qs)) keep &= 0xFu << (reinterpret_cast<uintptr_t>(qs) - at);
                if (at + 4 > e) keep &= 0xFu >> (at + 4 - e);
                score = min(score + qual_sum4(w[k], keep), (uint32_t)kMdScoreCap);
            }
        }
    }
#pragma unroll
    for (int m = kGroup / 2; m > 0; m >>= 1) {
        rlen += __shfl_xor(rlen, m, kGroup);
        clip += __shfl_xor(clip, m, kGroup);
        score += __shfl_xor(score, m, kGroup);
    }
    MdRec m;
    m.c = !want ? 0 : (flag & 16) ? (int64_t)pos + (rlen ? rlen : 1) - 1 + clip : (int64_t)pos - clip;
    m.rid = rid;
    m.flag = (uint16_t)flag;
    m.score = (uint16_t)min(score, (uint32_t)kMdScoreCap);
    return m;
}

// reasons of a refusal, in the low two bits of record << 2 | reason
enum { kMdTwoPrimaries = 0, kMdSegmentBits = 1, kMdMixed = 2, kMdCoordinate = 3 };

// The walk over one template's records (rules 2-3 and 5).  step() takes them in walk order, r being the record's index into the
// MdRec array, which is also what a fault names and what "the earlier record" compares; the first fault ends the walk (later steps do
// nothing).  end() gives the template's end and whether it has one.
struct MdWalk {
    int64_t only = -1, first = -1, last = -1;            // the primary of each segment
    int paired = -1;
    unsigned long long fault = ~0ULL;
    __device__ __forceinline__ void step(int64_t r, const MdRec &m) {
        const uint32_t f = m.flag;
        if (fault != ~0ULL || (f & 0x900)) return;
        const int p = f & 1;
        if (paired < 0) paired = p;
        int64_t &seg = !p ? only : (f & 0x40) ? first : last;
        if (p != paired) fault = (unsigned long long)r << 2 | kMdMixed;
        else if (p && ((f >> 6) & 1) == ((f >> 7) & 1)) fault = (unsigned long long)r << 2 | kMdSegmentBits;
        else if (seg >= 0) fault = (unsigned long long)r << 2 | kMdTwoPrimaries;
        else if (!(f & 4) && (m.rid < 0 || m.c < -(1LL << 31) || m.c >= (1LL << 31)))
            fault = (unsigned long long)r << 2 | kMdCoordinate;
        else seg = r;
    }
    // the end of template t (rule 5), rec being the array step()'s r indexes; false: no end (a fault, or no mapped primary that counts)
    __device__ __forceinline__ bool end(const MdRec *rec, int64_t t, bwams_dup_end_t *out) const {
        bool h = false;
        bwams_dup_end_t e;
        e.tmpl = t; e.ref2 = -1; e.pos2 = 0;
        const bool m_only = only >= 0 && !(rec[only].flag & 4), m_first = first >= 0 && !(rec[first].flag & 4);
        const bool m_last = last >= 0 && !(rec[last].flag & 4);
        if (fault != ~0ULL) {
        } else if (m_first && m_last) {                      // a pair: end 1 the smaller (refID, coordinate), on a tie the earlier record
            const int64_t a = min(first, last), b = max(first, last);
            const MdRec A = rec[a], B = rec[b];
            const bool swap = B.rid < A.rid || (B.rid == A.rid && B.c < A.c);
            const MdRec E1 = swap ? B : A, E2 = swap ? A : B;
            e.ref1 = E1.rid; e.pos1 = (int32_t)E1.c; e.ref2 = E2.rid; e.pos2 = (int32_t)E2.c;
            e.score = (int32_t)E1.score + (int32_t)E2.score;
            e.strands = (int32_t)((E1.flag >> 4) & 1) | (int32_t)((E2.flag >> 4) & 1) << 1;
            h = true;
        } else if ((int)m_only + (int)m_first + (int)m_last == 1) {
            const MdRec E1 = rec[m_only ? only : m_first ? first : last];
            e.ref1 = E1.rid; e.pos1 = (int32_t)E1.c;
            e.score = E1.score;
            e.strands = (int32_t)((E1.flag >> 4) & 1);
            h = true;
        }
        if (!h) { e.ref1 = -1; e.pos1 = 0; e.score = 0; e.strands = 0; }
        *out = e;
        return h;
    }
};

// one field of a read name from s[at, n): an optional '-', then digits up to the first other byte; *ok cleared outside int32
__device__ __forceinline__ int32_t name_value(const uint8_t *s, uint32_t at, uint32_t n, bool *ok) {
    const bool neg = at < n && s[at] == '-';
    if (neg) ++at;
    int64_t v = 0;
    for (; at < n && s[at] >= '0' && s[at] <= '9'; ++at) v = min(v * 10 + (s[at] - '0'), (int64_t)1 << 40);
    if (neg) v = -v;
    if (v < -(1LL << 31) || v >= (1LL << 31)) *ok = false;
    return (int32_t)v;
}

// Rules 9-10 of the record at p: with a table its aux fields walked by type to block_size (*aux_ok false when they do not chain;
// true without a table, when nothing is walked), the RG:Z value looked up among the table's IDs; the name's colons counted and its
// three fields parsed.
__device__ __forceinline__ bwams_dup_loc_t md_loc_of(const uint8_t *p, const MdGroupsDev &G, bool *aux_ok) {
    const uint32_t l_name = bam_l_name(p);
    bwams_dup_loc_t L;
    L.rg = -1; L.lib = G.n_lib - 1; L.tile = L.x = L.y = 0; L.has = 0;
    *aux_ok = true;
    if (G.walk) {                                         // rule 9: the aux fields by their types, to the record's end (aux_rg.h)
        bool found = false;
        int64_t v0 = 0, v1 = 0;                           // RG's value: p[v0, v1)
        const bool ok = aux_first_rg(p, &found, &v0, &v1);
        *aux_ok = ok;
        if (ok && found) {                                // the ID among the table's, sorted by bytes
            const int32_t rg = groups_find(G, p + v0, v1 - v0);
            if (rg >= 0) { L.rg = rg; L.lib = G.rg_lib[rg]; }
        }
    }
    const uint8_t *s = p + kBamName;                            // rule 10: the name without its NUL
    const uint32_t n = l_name ? l_name - 1 : 0;
    uint32_t colons = 0;
    for (uint32_t k = 0; k < n; ++k) colons += s[k] == ':';
    const int first = colons == 4 ? 2 : (colons == 6 || colons == 7) ? 4 : -1;
    if (first >= 0) {
        uint32_t at = 0;
        for (int f = 0; f < first; ++at) f += s[at] == ':';
        bool ok = true;
        int32_t v[3];
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            v[f] = name_value(s, at, n, &ok);
            while (at < n && s[at] != ':') ++at;
            ++at;
        }
        if (ok) { L.tile = v[0]; L.x = v[1]; L.y = v[2]; L.has = 1; }
    }
    return L;
}

// ---- rule J1: a read name's key (bwams_dupjoin_key on the host, dup_join.hip's kernels on the device) ----

constexpr uint64_t kDjSeed0 = 0x9e3779b97f4a7c15ULL, kDjSeed1 = 0xc2b2ae3d27d4eb4fULL;

__host__ __device__ __forceinline__ uint64_t fmix64(uint64_t h) {           // MurmurHash3's finalizer
    h ^= h >> 33; h *= 0xff51afd7ed558ccdULL; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ULL; h ^= h >> 33;
    return h;
}

// (k0, k1) of the name s[0, L): its bytes as little-endian 64-bit words, zero-padded, each folded in by one fmix64 step per seed
__host__ __device__ __forceinline__ void name_key(const uint8_t *s, uint32_t L, uint64_t *k0, uint64_t *k1) {
    uint64_t a = kDjSeed0 ^ (uint64_t)L, b = kDjSeed1 ^ (uint64_t)L;
    const uint32_t n_w = L > 8 ? (L + 7) / 8 : 1;
    for (uint32_t i = 0; i < n_w; ++i) {
        uint64_t w = 0;
        for (uint32_t k = 0; k < 8 && 8 * i + k < L; ++k) w |= (uint64_t)s[8 * i + k] << (8 * k);
        a = fmix64(a ^ w);
        b = fmix64(b ^ w);
    }
    *k0 = a;
    *k1 = b;
}

// ---- rule 13: counts per library.  counts[lib * kLibCounts + which]; a workgroup counts in LDS when the libraries fit ----

constexpr int kLibCounts = 7, kLdsLibs = 64;
enum { kUnpEx = 0, kPairEx = 1, kUnpDup = 2, kPairDup = 3, kOptical = 4, kSecSup = 5, kUnmapped = 6 };

struct LibCounter {
    unsigned int *lds;                                        // kLdsLibs * kLibCounts words, or null: straight to global memory
    unsigned long long *out;
    __device__ void init(unsigned int *sh, int n_lib, unsigned long long *counts) {
        lds = n_lib <= kLdsLibs ? sh : nullptr;
        out = counts;
        if (lds) {
            for (int k = threadIdx.x; k < n_lib * kLibCounts; k += blockDim.x) lds[k] = 0;
            __syncthreads();
        }
    }
    __device__ void add(int lib, int which) {
        if (lds) atomicAdd(lds + lib * kLibCounts + which, 1u);
        else atomicAdd(out + (int64_t)lib * kLibCounts + which, 1ULL);
    }
    __device__ void flush(int n_lib) {
        if (!lds) return;
        __syncthreads();
        for (int k = threadIdx.x; k < n_lib * kLibCounts; k += blockDim.x)
            if (lds[k]) atomicAdd(out + k, (unsigned long long)lds[k]);
    }
};

}  // namespace bwams
