// fmt_g.h — short decimal texts built in registers, for the host and the device alike: a float as C's "%g" prints it widened to
// double (rule V5 in include/bwams.h above bwams_samview_open), and the integers of a SAM line.  samview.hip's two passes and
// bwams_fmt_float call the same functions, so the float's text is testable without a GPU.  A text of at most 16 bytes is two 64-bit
// words (Text16): nothing here indexes an array with a variable, so nothing goes to scratch on the device.
//
// fmt_g in integer arithmetic only.  A finite float is M * 2^E with M < 2^24 and E in [-149, 104], an exact rational, and "%g"
// wants its first six significant decimal digits rounded half-even on that exact value:
//   E >= 0       the value is an integer below 2^128: its four 32-bit limbs are short-divided by 10^9 five times; the top two
//                non-zero nine-digit pieces hold the leading digits, anything below them is the sticky bit.  Every division
//                here is by a constant, which the compilers turn into a multiplication: none goes through a reciprocal;
//   E < 0, >= 1  the integer part is M >> -E (at most eight digits), the fraction's digits come from multiplying its numerator, below
//                2^23, by ten;
//   below 1      M is shifted to put the binary point at bit 156 of five limbs; each multiplication by ten leaves the next digit in
//                the top four bits.  Zeros are skipped, six digits are taken, what remains is compared with one half.
// Then the digits are laid out as "%g" does: scientific form when the decimal exponent is below -4 or at least 6, trailing zeros
// of the fraction and a bare point removed, at least two exponent digits.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace bwams {

struct Text16 {                          // n bytes, byte k in bits [8k, 8k + 8) of lo (k < 8) or hi
    uint64_t lo = 0, hi = 0;
    int n = 0;
    __host__ __device__ inline void put(uint32_t c) {
        if (n < 8) lo |= (uint64_t)(c & 255u) << (8 * n);
        else hi |= (uint64_t)(c & 255u) << (8 * (n - 8));
        ++n;
    }
    __host__ __device__ inline void set(int k, uint32_t c) {   // byte k, which nothing has written yet
        if (k < 8) lo |= (uint64_t)(c & 255u) << (8 * k);
        else hi |= (uint64_t)(c & 255u) << (8 * (k - 8));
    }
    __host__ __device__ inline uint32_t at(int k) const { return (uint32_t)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 255u); }
};

// decimal digits of v: 1 for 0
__host__ __device__ inline int dec_digits_u32(uint32_t v) {
    return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 : v < 10000000u ? 7
         : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}
// bytes of v in decimal with its sign; |v| < 2^32
__host__ __device__ inline int dec_digits_i64(int64_t v) { return v < 0 ? 1 + dec_digits_u32((uint32_t)(-v)) : dec_digits_u32((uint32_t)v); }

__host__ __device__ inline uint32_t pow10_u32(int k) {   // k in [0, 9]
    return k == 0 ? 1u : k == 1 ? 10u : k == 2 ? 100u : k == 3 ? 1000u : k == 4 ? 10000u : k == 5 ? 100000u : k == 6 ? 1000000u
         : k == 7 ? 10000000u : k == 8 ? 100000000u : 1000000000u;
}

// v in decimal behind what t holds: as many bytes as dec_digits_u32 says, the last digit first (every division is by the constant 10)
__host__ __device__ inline void put_u32(Text16 &t, uint32_t v) {
    const int n = dec_digits_u32(v);
    for (int k = n - 1; k >= 0; --k) {
        const uint32_t q = v / 10u;
        t.set(t.n + k, '0' + (v - q * 10u));
        v = q;
    }
    t.n += n;
}
__host__ __device__ inline void put_i64(Text16 &t, int64_t v) {       // |v| < 2^32
    if (v < 0) { t.put('-'); put_u32(t, (uint32_t)(-v)); }
    else put_u32(t, (uint32_t)v);
}

// the float with these bits as "%g" prints (double)x: at most 13 bytes
__host__ __device__ inline Text16 fmt_g(uint32_t bits) {
    Text16 t;
    const uint32_t e = (bits >> 23) & 255u, m = bits & 0x7FFFFFu;
    if (bits >> 31) t.put('-');
    if (e == 255u) {
        if (m) { t.put('n'); t.put('a'); t.put('n'); }
        else { t.put('i'); t.put('n'); t.put('f'); }
        return t;
    }
    if (e == 0 && m == 0) { t.put('0'); return t; }
    const uint32_t M = e ? (m | 0x800000u) : m;
    const int E = (int)(e ? e : 1u) - 150;
    uint32_t q = 0;                      // the six digits, 100000 .. 999999 (before the carry of rounding up)
    int X = 0;                           // the decimal exponent of the first of them
    bool up = false;
    if (E >= 0) {
        uint32_t a[4];                   // M << E, limb 0 lowest: E <= 104
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int lo = 32 * i - E;   // a[i] = bits [lo, lo + 32) of M
            a[i] = (lo >= 24 || lo <= -32) ? 0u : lo >= 0 ? M >> lo : M << -lo;
        }
        uint32_t c[5];                   // nine decimal digits each, c[0] lowest
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            uint64_t r = 0;
#pragma unroll
            for (int i = 3; i >= 0; --i) {
                const uint64_t x = r << 32 | a[i];
                a[i] = (uint32_t)(x / 1000000000u);
                r = x % 1000000000u;
            }
            c[j] = (uint32_t)r;
        }
        uint32_t hi = 0, lo = 0;
        int k = -1, below = 0;
        bool sticky = false;
#pragma unroll
        for (int j = 4; j >= 0; --j) {
            if (k < 0) { if (c[j]) { k = j; hi = c[j]; } }
            else if (below == 0) { lo = c[j]; below = 1; }
            else sticky |= c[j] != 0;
        }
        const uint64_t V = k > 0 ? (uint64_t)hi * 1000000000u + lo : hi;                      // the leading digits, nv of them
        const int nv = dec_digits_u32(hi) + (k > 0 ? 9 : 0);
        X = nv - 1 + (k > 0 ? 9 * (k - 1) : 0);
        if (nv > 6) {
            uint64_t W = V;
            uint32_t top = 0;                                // the last digit taken off, and whether anything below it was not 0
            for (int i = 0; i < nv - 6; ++i) {
                const uint64_t w = W / 10u;
                sticky |= top != 0;
                top = (uint32_t)(W - w * 10u);
                W = w;
            }
            q = (uint32_t)W;
            up = top > 5u || (top == 5u && (sticky || (q & 1u)));
        } else {
            q = (uint32_t)V * pow10_u32(6 - nv);
        }
    } else if (-E < 24 && (M >> -E) != 0) {
        const int s = -E;
        const uint32_t I = M >> s, mask = (1u << s) - 1u;
        uint32_t F = M & mask;
        const int ni = dec_digits_u32(I);
        X = ni - 1;
        if (ni > 6) {
            bool sticky = F != 0;
            uint32_t top = 0;
            q = I;
            for (int i = 0; i < ni - 6; ++i) {
                const uint32_t w = q / 10u;
                sticky |= top != 0;
                top = q - w * 10u;
                q = w;
            }
            up = top > 5u || (top == 5u && (sticky || (q & 1u)));
        } else {
            q = I;
            for (int i = 0; i < 6 - ni; ++i) {
                F *= 10u;
                q = q * 10u + (F >> s);
                F &= mask;
            }
            const uint32_t half = 1u << (s - 1);
            up = F > half || (F == half && (q & 1u));
        }
    } else {
        const int sh = 156 + E;          // M * 2^E < 1 with the binary point at bit 156: sh in [7, 132]
        uint32_t a[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int lo = 32 * i - sh;
            a[i] = (lo >= 24 || lo <= -32) ? 0u : lo >= 0 ? M >> lo : M << -lo;
        }
        int got = 0;
        while (got < 6) {
            uint64_t carry = 0;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const uint64_t x = (uint64_t)a[i] * 10u + carry;
                a[i] = (uint32_t)x;
                carry = x >> 32;
            }
            const uint32_t d = a[4] >> 28;
            a[4] &= 0x0FFFFFFFu;
            if (got == 0) {
                --X;
                if (d) { q = d; got = 1; }
            } else {
                q = q * 10u + d;
                ++got;
            }
        }
        const bool rest = (a[0] | a[1] | a[2] | a[3]) != 0;
        up = a[4] > 0x08000000u || (a[4] == 0x08000000u && (rest || (q & 1u)));
    }
    if (up && ++q == 1000000u) { q = 100000u; ++X; }
    const uint32_t d0 = q / 100000u, d1 = q / 10000u % 10u, d2 = q / 1000u % 10u, d3 = q / 100u % 10u, d4 = q / 10u % 10u, d5 = q % 10u;
    const int nsig = d5 ? 6 : d4 ? 5 : d3 ? 4 : d2 ? 3 : d1 ? 2 : 1;   // without the trailing zeros
    auto digit = [&](int i) -> uint32_t { return i == 0 ? d0 : i == 1 ? d1 : i == 2 ? d2 : i == 3 ? d3 : i == 4 ? d4 : d5; };
    if (X < -4 || X >= 6) {
        t.put('0' + d0);
        if (nsig > 1) {
            t.put('.');
            for (int i = 1; i < nsig; ++i) t.put('0' + digit(i));
        }
        t.put('e');
        t.put(X < 0 ? '-' : '+');
        const uint32_t ax = (uint32_t)(X < 0 ? -X : X);       // at most 45
        t.put('0' + ax / 10u);
        t.put('0' + ax % 10u);
    } else if (X >= 0) {
        for (int i = 0; i <= X; ++i) t.put('0' + digit(i));
        if (nsig > X + 1) {
            t.put('.');
            for (int i = X + 1; i < nsig; ++i) t.put('0' + digit(i));
        }
    } else {
        t.put('0');
        t.put('.');
        for (int i = -1; i > X; --i) t.put('0');
        for (int i = 0; i < nsig; ++i) t.put('0' + digit(i));
    }
    return t;
}

}  // namespace bwams
