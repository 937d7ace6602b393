// aux_rg.h — a record's read group on the device (markdup rule 9, recalibration rule 6): the walk over the aux fields by their types to
// the record's first RG:Z value, and that value's ordinal in the groups table (MdGroupsDev, common.h).  markdup.hip's md_loc_kernel
// and recal.hip share them; recal.hip and recal_apply.hip share the key made of it; qc.hip shares aux_size.
#pragma once
#include "bam_rec.h"

namespace bwams {

// bytes of one value of aux type t (A c C s S i I f), 0 for any other
__device__ __forceinline__ int aux_size(uint32_t t) {
    return (t == 'A' || t == 'c' || t == 'C') ? 1 : (t == 's' || t == 'S') ? 2 : (t == 'i' || t == 'I' || t == 'f') ? 4 : 0;
}

// The aux fields of the record at p by their types, to the record's end: false when they do not chain to it (a type that is none of
// A c C s S i I f Z H B, a B subtype that is none of c C s S i I f, a field past the end, a Z or H without its NUL).  *found: the
// record has an RG:Z field, the first one's value being p[*v0, *v1).
__device__ __forceinline__ bool aux_first_rg(const uint8_t *p, bool *found, int64_t *v0, int64_t *v1) {
    const int64_t n = (int64_t)bam_block_size(p) + 4;                   // the record with its block_size
    const int64_t l_seq = bam_l_seq(p);
    int64_t a = bam_aux_at(bam_l_name(p), bam_n_cig(p), l_seq);
    bool ok = l_seq >= 0 && a <= n;
    *found = false;
    *v0 = *v1 = 0;
    while (ok && a < n) {
        if (a + 3 > n) { ok = false; break; }
        const uint32_t c0 = p[a], c1 = p[a + 1], ty = p[a + 2];
        a += 3;
        if (ty == 'Z' || ty == 'H') {
            const int64_t s = a;
            while (a < n && p[a] != 0) ++a;
            if (a >= n) { ok = false; break; }
            if (ty == 'Z' && c0 == 'R' && c1 == 'G' && !*found) { *found = true; *v0 = s; *v1 = a; }
            ++a;
        } else if (ty == 'B') {
            if (a + 5 > n) { ok = false; break; }
            const int sz = aux_size(p[a]);
            if (!sz || p[a] == 'A') { ok = false; break; }
            a += 5 + (int64_t)sz * (int64_t)ld_u32(p + a + 1);
        } else {
            const int sz = aux_size(ty);
            if (!sz) { ok = false; break; }
            a += sz;
        }
        if (a > n) ok = false;
    }
    return ok;
}

// the ordinal of the read group whose ID is v[0, lv) in the table (its IDs sorted by bytes), or -1
__device__ __forceinline__ int32_t groups_find(const MdGroupsDev &G, const uint8_t *v, int64_t lv) {
    int lo = 0, hi = G.n_rg;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const uint8_t *id = G.ids + G.id_off[mid];
        const int64_t ln = G.id_off[mid + 1] - G.id_off[mid];
        int64_t k = 0;
        while (k < ln && k < lv && id[k] == v[k]) ++k;
        const int cmp = k < ln && k < lv ? (id[k] < v[k] ? -1 : 1) : ln < lv ? -1 : ln > lv ? 1 : 0;
        if (cmp == 0) return G.id_ord[mid];
        if (cmp < 0) lo = mid + 1;
        else hi = mid;
    }
    return -1;
}

// The key that recalibration counts and rewrites the record at p under (rule 6): 2 * its read group's ordinal, the group after the
// table's last when it has no RG:Z or one the table does not hold, + 1 for the second read of a pair (its cycles are negative).  The
// aux fields were walked once already, by the check kernel.
__device__ __forceinline__ uint32_t rg_key(const uint8_t *p, const MdGroupsDev &G) {
    int32_t g = G.n_rg;
    if (G.walk) {
        bool found;
        int64_t v0, v1;
        if (aux_first_rg(p, &found, &v0, &v1) && found) {
            const int32_t rg = groups_find(G, p + v0, v1 - v0);
            if (rg >= 0) g = rg;
        }
    }
    return 2u * (uint32_t)g + ((bam_flag(p) & 0x81) == 0x81 ? 1u : 0u);
}

}  // namespace bwams
