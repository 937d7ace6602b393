// crc32.h — gzip's CRC-32 (reflected polynomial 0xEDB88320) of bytes in LDS, computed by a whole workgroup: a lane per 1/NT of the
// bytes with a byte table in LDS, the lanes' remainders joined by x^(8n) mod P.  Shared by inflate.hip (checks a member's output) and
// deflate.hip (writes a member's trailer); gunzip.hip computes one per tile of output and joins them on the host.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr uint32_t kPoly = 0xEDB88320u;  // CRC-32 (reflected)

// tab[256]: the byte table, filled by the NT lanes of the workgroup (the caller syncs before it is read)
template <int NT> __device__ __forceinline__ void crc32_table(uint32_t *tab, int lane) {
    for (int i = lane; i < 256; i += NT) {
        uint32_t c = (uint32_t)i;
        for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ kPoly : c >> 1;
        tab[i] = c;
    }
}

__device__ __forceinline__ uint32_t gf2_mul(uint32_t a, uint32_t b) {     // a * b mod P (reflected: bit 31 is x^0)
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ kPoly : b >> 1;
    }
    return p;
}

__device__ uint32_t x8n(uint32_t n) {                // x^(8n) mod P
    uint32_t sq = 0x40000000u, r = 0x80000000u;      // x^1, x^0
    for (int i = 0; i < 3; ++i) sq = gf2_mul(sq, sq);  // x^8
    for (; n; n >>= 1) {
        if (n & 1) r = gf2_mul(r, sq);
        sq = gf2_mul(sq, sq);
    }
    return r;
}

// CRC-32 of buf[0, n), the same value in every lane.  buf and tab must be complete in LDS (the caller syncs); part: NT words of LDS.
// Every lane of the workgroup calls it (it contains a barrier).
template <int NT> __device__ __forceinline__ uint32_t crc32_lds(const uint8_t *buf, int n, const uint32_t *tab, uint32_t *part, int lane) {
    const int L = (n + NT - 1) / NT, a = min(lane * L, n), e = min(a + L, n);
    uint32_t c = 0;                                // the raw remainder of the lane's slice (register starting at 0)
    for (int i = a; i < e; ++i) c = tab[(c ^ buf[i]) & 255] ^ (c >> 8);
    part[lane] = c;
    __syncthreads();
    const uint32_t xl = x8n((uint32_t)L);
    uint32_t acc = 0xFFFFFFFFu;                    // register after slice k = (register before) * x^(8 len_k) + slice k's remainder
    for (int k = 0; k < NT; ++k) {
        const int ka = min(k * L, n), ke = min(ka + L, n);
        if (ke == ka) break;
        acc = gf2_mul(ke - ka == L ? xl : x8n((uint32_t)(ke - ka)), acc) ^ part[k];
    }
    return ~acc;
}

}  // namespace
