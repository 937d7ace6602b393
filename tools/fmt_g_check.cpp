// fmt_g_check.cpp — csrc/fmt_g.h against the C library, on the host: every float of the named list (ties, edges, special values),
// every exponent byte with a few mantissas, and N seeded random bit patterns are formatted by fmt_g and by snprintf("%g") of the
// value widened to double, and compared byte for byte; the integers' texts against "%u" / "%lld".
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/fmt_g_check.cpp -o fmt_g_check && ./fmt_g_check [N]
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../bwa-mem-scale_amd/csrc/fmt_g.h"

static std::string text(const bwams::Text16 &t) {
    std::string s;
    for (int k = 0; k < t.n; ++k) s.push_back((char)t.at(k));
    return s;
}

static long long bad = 0, done = 0;

static void check(uint32_t bits) {
    float x;
    memcpy(&x, &bits, 4);
    char want[64];
    snprintf(want, sizeof want, "%g", (double)x);
    const bwams::Text16 t = bwams::fmt_g(bits);
    const std::string got = text(t);
    ++done;
    if (t.n > 13 || got != want) {
        if (bad++ < 20) fprintf(stderr, "bits %08x: fmt_g \"%s\", %%g \"%s\"\n", bits, got.c_str(), want);
    }
}

static void check_f(float x) {
    uint32_t b;
    memcpy(&b, &x, 4);
    check(b);
    check(b ^ 0x80000000u);
}

int main(int argc, char **argv) {
    const long long n = argc > 1 ? atoll(argv[1]) : 4000000;
    const float named[] = {1234565.f, 1234575.f, 9999995.f, 999999.5f, 99999.95f, 100000.f, 999999.f, 1e6f, 0.0001f,
                           nextafterf(0.0001f, 0.f), 1e-5f, FLT_MIN, FLT_MAX, 0.f, 1.f, 0.5f, 0.1f, 123456.f, 1234567.f, 16777216.f,
                           16777215.f, 8388608.5f, 2.5f, 3.5f, 1e10f, 1e-10f, 1e38f, 1e-38f, 1e-45f, 65504.f, 0.3f, 100.25f};
    for (float x : named) check_f(x);
    check(1u); check(0x80000001u);                                   // the smallest subnormal
    check(0x7F800000u); check(0xFF800000u); check(0x7FC00000u); check(0xFFC00000u); check(0x7F800001u);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (uint32_t e = 0; e < 256; ++e)
        for (int k = 0; k < 68; ++k) {
            const uint32_t m = k == 0 ? 0u : k == 1 ? 1u : k == 2 ? 0x400000u : k == 3 ? 0x7FFFFFu : (uint32_t)next() & 0x7FFFFFu;
            check(e << 23 | m);
            check(0x80000000u | e << 23 | m);
        }
    for (long long i = 0; i < n; ++i) check((uint32_t)next());
    for (long long i = 0; i < 200000; ++i) {                         // the integers
        const uint32_t v = i < 64 ? (uint32_t)(i < 32 ? (1ull << i) - 1 : 1ull << (i - 32)) : (uint32_t)next() >> (next() & 31);
        char want[32];
        bwams::Text16 t;
        bwams::put_u32(t, v);
        snprintf(want, sizeof want, "%u", v);
        ++done;
        if (text(t) != want || t.n != bwams::dec_digits_u32(v)) { if (bad++ < 20) fprintf(stderr, "u32 %u: \"%s\"\n", v, text(t).c_str()); }
        const int64_t w = (next() & 1) ? -(int64_t)v : (int64_t)v;
        bwams::Text16 u;
        bwams::put_i64(u, w);
        snprintf(want, sizeof want, "%lld", (long long)w);
        ++done;
        if (text(u) != want || u.n != bwams::dec_digits_i64(w)) { if (bad++ < 20) fprintf(stderr, "i64 %lld: \"%s\"\n", (long long)w, text(u).c_str()); }
    }
    printf("fmt_g_check: %lld texts compared, %lld differ\n", done, bad);
    return bad ? 1 : 0;
}
