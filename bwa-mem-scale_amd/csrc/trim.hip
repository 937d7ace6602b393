// trim.hip — read trimming in front of the mapper (rules T1 to T9 above bwams_fastq_trim in include/bwams.h; bwams/trim.py restates
// them) and a decoded chunk as FASTQ text.  One wave per read, or per pair: every step's state (the kept interval, the bases each step
// took) is wave-uniform, the lanes share out positions (T2, T4, T6) or candidate insert lengths (T3).
#include "common.h"
#include "wave_ops.h"

namespace bwams {
namespace {

constexpr int kWords = BWAMS_TRIM_OVERLAP_MAX_LEN / 64;       // words of one bit plane of an end in T3

// one end of a unit: [s, e) of its n0 input bases is what the steps so far have left
struct End {
    const uint8_t *c;
    const char *q;
    int n0, s, e, insert;
    int rem[BWAMS_TRIM_N_STEPS];
    bool skipped;
    __device__ __forceinline__ int n() const { return e - s; }
};

template <int STEP> __device__ __forceinline__ void end_cut(End &E, int s, int e) {
    E.rem[STEP] += (E.e - E.s) - (e - s);
    E.s = s; E.e = e;
}

__device__ __forceinline__ int first_lane(unsigned long long m) { return __ffsll(m) - 1; }

// T2, one direction.  q'[i] = q[i] (rev = false) or q[n - 1 - i] over the n > 0 current bases at q: the smallest s in [0, n - w] whose
// window sum reaches w * Q, moved on past the bases below Q; -1 when no window does.  Lane l of chunk c holds the exclusive prefix sum
// E[64 c + l]; the sum of the window that starts there is E[64 c + l + w] - E[64 c + l], w <= 64, so the far end is in this chunk's
// or the next chunk's registers.  The prefix is carried from chunk to chunk.
__device__ int first_window(const char *__restrict__ q, int n, int w0, int Q, bool rev, int lane) {
    const int w = min(w0, n), last = n - w;
    const int64_t need = (int64_t)w * Q;
    auto qat = [&](int i) -> int {
        if (i >= n) return 0;
        const int v = (int)(uint8_t)q[rev ? n - 1 - i : i] - 33;
        return v < 0 ? 0 : v;
    };
    int carry = 0;
    int v = qat(lane);
    int inc = scan_add(v);
    int e_cur = carry + inc - v;
    carry += __builtin_amdgcn_readlane(inc, 63);
    for (int c0 = 0; c0 <= last; c0 += 64) {
        v = c0 + 64 < n ? qat(c0 + 64 + lane) : 0;
        inc = scan_add(v);
        const int e_next = carry + inc - v;
        carry += __builtin_amdgcn_readlane(inc, 63);
        const int src = lane + w;
        const int a = __shfl(e_cur, src & 63), b = __shfl(e_next, src & 63);
        const int far = src < 64 ? a : b;
        const unsigned long long hit = __ballot(c0 + lane <= last && (int64_t)(far - e_cur) >= need);
        if (hit) {
            const int s = c0 + first_lane(hit);
            // a passing window holds a base of at least Q within its w <= 64 positions
            const unsigned long long good = __ballot(s + lane < n && qat(s + lane) >= Q);
            return s + first_lane(good);
        }
        e_cur = e_next;
    }
    return -1;
}

__device__ void before_overlap(End &E, const TrimParams &P, int lane) {      // T1, T2
    const int n = E.n();
    const int s = min(n, P.trim_front);
    end_cut<BWAMS_TRIM_STEP_FIXED>(E, s, max(s, n - P.trim_tail));
    if (!P.has_qual) return;
    if (P.cut_front && E.n() > 0) {
        const int k = first_window(E.q + E.s, E.n(), P.cut_window, P.cut_quality, false, lane);
        if (k >= 0) end_cut<BWAMS_TRIM_STEP_CUT_FRONT>(E, E.s + k, E.e);
        else end_cut<BWAMS_TRIM_STEP_CUT_FRONT>(E, E.s, E.s);
    }
    if (P.cut_tail && E.n() > 0) {
        const int k = first_window(E.q + E.s, E.n(), P.cut_window, P.cut_quality, true, lane);
        if (k >= 0) end_cut<BWAMS_TRIM_STEP_CUT_TAIL>(E, E.s, E.e - k);
        else end_cut<BWAMS_TRIM_STEP_CUT_TAIL>(E, E.s, E.s);
    }
}

// T3.  Both ends as three bit planes (low bit, high bit, N) of 64 positions a word in the wave's LDS: pl[0..2] = end 1, pl[3..5] =
// the reverse complement of end 2; positions past an end are zero in every plane of the words in use.  A lane owns one candidate I,
// a round tests 64 of them from the largest down, so the first round with a hit ends the pair and its lowest passing lane holds the
// largest I.
__device__ int find_insert(unsigned long long (*pl)[kWords], const uint8_t *__restrict__ c1, int n1, const uint8_t *__restrict__ c2, int n2,
                           const TrimParams &P, int lane) {
    const int i_max = n1 + n2 - P.overlap_min, i_min = P.overlap_min;
    if (i_max < i_min) return 0;
    const int nw = (max(n1, n2) + 63) >> 6;               // words in use: those behind them are neither written nor read
    unsigned long long mine[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < nw; ++k) {
        const int i = 64 * k + lane;
        const int a = i < n1 ? c1[i] : 0, r = i < n2 ? c2[n2 - 1 - i] : 4;
        const int b = r > 3 ? 0 : 3 - r;
        const unsigned long long w[6] = {__ballot(a & 1), __ballot(a & 2), __ballot(a > 3),
                                         __ballot(b & 1), __ballot(b & 2), __ballot(i < n2 && r > 3)};
        if (lane == k)
            for (int j = 0; j < 6; ++j) mine[j] = w[j];
    }
    __builtin_amdgcn_wave_barrier();                       // the lanes of the unit before have read their planes
    if (lane < nw)
        for (int j = 0; j < 6; ++j) pl[j][lane] = mine[j];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    auto word = [&](int j, int wi) -> unsigned long long { return (unsigned)wi < (unsigned)nw ? pl[j][wi] : 0ull; };
    for (int i0 = i_max; i0 >= i_min; i0 -= 64) {
        const int I = i0 - lane;
        bool ok = false;
        const int lo = max(0, I - n2), hi = min(n1, I), ov = hi - lo;
        if (I >= i_min && ov >= P.overlap_min) {
            const int off = n2 - I, k_lo = lo >> 6, k_hi = (hi - 1) >> 6;
            int d = 0;
            for (int k = k_lo; k <= k_hi && d <= P.overlap_max_diff; ++k) {
                unsigned long long mask = ~0ull;
                if (k == k_lo) mask &= ~0ull << (lo & 63);
                if (k == k_hi) mask &= ~0ull >> (63 - ((hi - 1) & 63));
                const int t = 64 * k + off, wi = t >> 6, sh = t & 63;      // b's bits [t, t + 64): a funnel shift of two words
                unsigned long long bw[3];
                for (int j = 0; j < 3; ++j) {
                    bw[j] = word(3 + j, wi) >> sh;
                    if (sh) bw[j] |= word(3 + j, wi + 1) << (64 - sh);
                }
                const unsigned long long x = ((pl[0][k] ^ bw[0]) | (pl[1][k] ^ bw[1]) | pl[2][k] | bw[2]) & mask;
                d += __popcll(x);
            }
            ok = d <= P.overlap_max_diff && 100 * (int64_t)d <= (int64_t)P.overlap_diff_pct * ov;
        }
        const unsigned long long hit = __ballot(ok);
        if (hit) return i0 - first_lane(hit);
    }
    return 0;
}

// T4.  The adapter's planes are wave-uniform words; the read's planes come 64 positions at a time from one ballot each, three words
// (192 positions) held at once: lane l of a round owns p = p0 + l and reads its up to 128 positions as a funnel shift by l.
__device__ int find_adapter(const uint8_t *__restrict__ c, int n, const unsigned long long *a_lo, const unsigned long long *a_hi, int m,
                            const TrimParams &P, int lane) {
    const int last = n - P.adapter_min_match;
    if (m == 0 || last < 0) return -1;
    unsigned long long lo[3], hi[3], nn[3];
    auto load = [&](int p0, int j) {
        const int i = p0 + lane;
        const int v = (p0 < n && i < n) ? c[i] : 0;
        lo[j] = __ballot(v & 1); hi[j] = __ballot(v & 2); nn[j] = __ballot(v > 3);
    };
    load(0, 0); load(64, 1); load(128, 2);
    auto funnel = [&](unsigned long long x, unsigned long long y) { return lane ? (x >> lane) | (y << (64 - lane)) : x; };
    for (int p0 = 0; p0 <= last; p0 += 64) {
        const int p = p0 + lane, cmp = min(n - p, m);
        const unsigned long long x0 = (funnel(lo[0], lo[1]) ^ a_lo[0]) | (funnel(hi[0], hi[1]) ^ a_hi[0]) | funnel(nn[0], nn[1]);
        const unsigned long long x1 = (funnel(lo[1], lo[2]) ^ a_lo[1]) | (funnel(hi[1], hi[2]) ^ a_hi[1]) | funnel(nn[1], nn[2]);
        const unsigned long long m0 = cmp >= 64 ? ~0ull : cmp > 0 ? (1ull << cmp) - 1 : 0ull;
        const unsigned long long m1 = cmp >= 128 ? ~0ull : cmp > 64 ? (1ull << (cmp - 64)) - 1 : 0ull;
        const int d = __popcll(x0 & m0) + __popcll(x1 & m1);
        const unsigned long long hit = __ballot(p <= last && (int64_t)d * P.adapter_mismatch_per <= cmp);
        if (hit) return p0 + first_lane(hit);
        lo[0] = lo[1]; hi[0] = hi[1]; nn[0] = nn[1];
        lo[1] = lo[2]; hi[1] = hi[2]; nn[1] = nn[2];
        if (p0 + 192 < n) load(p0 + 192, 2);
        else lo[2] = hi[2] = nn[2] = 0;
    }
    return -1;
}

__device__ void after_overlap(End &E, int which, const TrimParams &P, int lane) {      // T4, T5
    if (!E.insert) {
        const int p = find_adapter(E.c + E.s, E.n(), P.a_lo[which], P.a_hi[which], P.a_len[which], P, lane);
        if (p >= 0) end_cut<BWAMS_TRIM_STEP_ADAPTER>(E, E.s, E.s + p);
    }
    if (P.max_len > 0 && E.n() > P.max_len) end_cut<BWAMS_TRIM_STEP_MAX_LEN>(E, E.s, E.s + P.max_len);
}

__device__ int end_reason(const End &E, const TrimParams &P, int lane) {               // T6
    const int n = E.n();
    if (n < P.min_len) return BWAMS_TRIM_LEN;
    int n_n = 0, n_low = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool in = i < n;
        n_n += __popcll(__ballot(in && E.c[E.s + i] > 3));
        if (P.has_qual) {
            int v = in ? (int)(uint8_t)E.q[E.s + i] - 33 : 0;
            if (v < 0) v = 0;
            n_low += __popcll(__ballot(in && v < P.qual_floor));
        }
    }
    if (n_n > P.n_limit) return BWAMS_TRIM_N;
    if (P.has_qual && 100 * (int64_t)n_low > (int64_t)P.low_qual_pct * n) return BWAMS_TRIM_QUAL;
    return BWAMS_TRIM_KEPT;
}

__device__ void end_open(End &E, const uint8_t *enc, const char *qual, const int64_t *cum, int64_t r) {
    const int64_t base = cum[r];
    E.c = enc + base; E.q = qual + base;
    E.n0 = (int)(cum[r + 1] - base);
    E.s = 0; E.e = E.n0; E.insert = 0; E.skipped = false;
    for (int k = 0; k < BWAMS_TRIM_N_STEPS; ++k) E.rem[k] = 0;
}

__device__ void end_report(const End &E, int reason, bwams_trim_read_t *out) {
    bwams_trim_read_t R;
    R.start = E.s; R.len = E.n(); R.insert = E.insert;
    R.reason = (uint8_t)reason; R.pad_[0] = R.pad_[1] = 0;
    int steps = E.skipped ? BWAMS_TRIM_STEP_SKIPPED : 0;
    for (int k = 0; k < BWAMS_TRIM_N_STEPS; ++k) {
        R.removed[k] = E.rem[k];
        if (E.rem[k] > 0) steps |= 1 << k;
    }
    R.steps = (uint8_t)steps;
    *out = R;
}

// a wave per unit (a read, or the two ends of a pair): T1 to T7
__global__ __launch_bounds__(256) void trim_reads_kernel(const uint8_t *__restrict__ enc, const char *__restrict__ qual,
                                                         const int64_t *__restrict__ cum, int64_t n_units, const TrimParams P,
                                                         bwams_trim_read_t *__restrict__ report) {
    __shared__ unsigned long long planes[4][6][kWords];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t wave = (int64_t)blockIdx.x * 4 + wv, n_waves = (int64_t)gridDim.x * 4;
    for (int64_t u = wave; u < n_units; u += n_waves) {
        if (!P.paired) {
            End A;
            end_open(A, enc, qual, cum, u);
            before_overlap(A, P, lane);
            after_overlap(A, 0, P, lane);
            const int ra = end_reason(A, P, lane);
            if (lane == 0) end_report(A, ra, report + u);
            continue;
        }
        End A, B;
        end_open(A, enc, qual, cum, 2 * u);
        end_open(B, enc, qual, cum, 2 * u + 1);
        before_overlap(A, P, lane);
        before_overlap(B, P, lane);
        if (P.overlap) {
            if (A.n() > BWAMS_TRIM_OVERLAP_MAX_LEN || B.n() > BWAMS_TRIM_OVERLAP_MAX_LEN) A.skipped = B.skipped = true;
            else {
                const int I = find_insert(planes[wv], A.c + A.s, A.n(), B.c + B.s, B.n(), P, lane);
                if (I) {
                    A.insert = B.insert = I;
                    end_cut<BWAMS_TRIM_STEP_OVERLAP>(A, A.s, A.s + min(A.n(), I));
                    end_cut<BWAMS_TRIM_STEP_OVERLAP>(B, B.s, B.s + min(B.n(), I));
                }
            }
        }
        after_overlap(A, 0, P, lane);
        after_overlap(B, 1, P, lane);
        int ra = end_reason(A, P, lane), rb = end_reason(B, P, lane);
        if (ra || rb) {
            if (!ra) ra = BWAMS_TRIM_MATE;
            if (!rb) rb = BWAMS_TRIM_MATE;
        }
        if (lane == 0) {
            end_report(A, ra, report + 2 * u);
            end_report(B, rb, report + 2 * u + 1);
        }
    }
}

// what read i brings to the new chunk: name bytes, comment bytes, bases (0 for a dropped read and for the entry behind the last read)
__global__ __launch_bounds__(256) void trim_widths_kernel(const bwams_trim_read_t *__restrict__ report, const int64_t *__restrict__ name_off,
                                                          const int64_t *__restrict__ comment_off, int64_t n, int64_t *__restrict__ wide) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, n1 = n + 1;
    if (i >= n1) return;
    const bool kept = i < n && report[i].reason == BWAMS_TRIM_KEPT;
    wide[i] = kept ? name_off[i + 1] - name_off[i] : 0;
    wide[n1 + i] = kept ? comment_off[i + 1] - comment_off[i] : 0;
    wide[2 * n1 + i] = kept ? report[i].len : 0;
}

__device__ __forceinline__ void wave_copy(char *__restrict__ dst, const char *__restrict__ src, int64_t len, int lane) {
    for (int64_t i = lane; i < len; i += 64) dst[i] = src[i];
}

// a wave per read of the input: a kept read's name, comment, and the kept interval of its bases and qualities, to their new places
__global__ __launch_bounds__(256) void trim_gather_kernel(const bwams_trim_read_t *__restrict__ report, int64_t n, TrimArrays in,
                                                          const int64_t *__restrict__ offs, TrimArrays out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6, n1 = n + 1;
    for (int64_t r = wave; r < n; r += n_waves) {
        const bwams_trim_read_t R = report[r];
        if (R.reason != BWAMS_TRIM_KEPT) continue;
        wave_copy(out.names + offs[r], in.names + in.name_off[r], in.name_off[r + 1] - in.name_off[r], lane);
        wave_copy(out.comments + offs[n1 + r], in.comments + in.comment_off[r], in.comment_off[r + 1] - in.comment_off[r], lane);
        const int64_t from = in.cum[r] + R.start, to = offs[2 * n1 + r];
        wave_copy((char *)out.enc + to, (const char *)in.enc + from, R.len, lane);
        if (in.qual) wave_copy(out.qual + to, in.qual + from, R.len, lane);
    }
}

// ---- a decoded chunk as FASTQ text ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fastq_text_widths_kernel(TrimArrays in, int64_t n, int with_comment, int64_t *__restrict__ wide) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    int64_t w = 0;
    if (i < n) {
        const int64_t nl = in.name_off[i + 1] - in.name_off[i], cl = with_comment ? in.comment_off[i + 1] - in.comment_off[i] : 0;
        const int64_t l = in.cum[i + 1] - in.cum[i];
        w = 1 + nl + (cl ? 1 + cl : 0) + 1 + l + 1 + (in.qual ? 2 + l + 1 : 0);
    }
    wide[i] = w;
}

__global__ __launch_bounds__(256) void fastq_text_emit_kernel(TrimArrays in, int64_t n, int with_comment, const int64_t *__restrict__ off,
                                                              char *__restrict__ text) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave; r < n; r += n_waves) {
        const int64_t nl = in.name_off[r + 1] - in.name_off[r], cl = with_comment ? in.comment_off[r + 1] - in.comment_off[r] : 0;
        const int64_t l = in.cum[r + 1] - in.cum[r];
        char *o = text + off[r];
        if (lane == 0) o[0] = in.qual ? '@' : '>';
        ++o;
        wave_copy(o, in.names + in.name_off[r], nl, lane);
        o += nl;
        if (cl) {
            if (lane == 0) o[0] = ' ';
            wave_copy(o + 1, in.comments + in.comment_off[r], cl, lane);
            o += 1 + cl;
        }
        if (lane == 0) { o[0] = '\n'; o[1 + l] = '\n'; }
        ++o;
        const uint8_t *c = in.enc + in.cum[r];
        for (int64_t i = lane; i < l; i += 64) o[i] = "ACGTN"[c[i] > 4 ? 4 : c[i]];
        o += l + 1;
        if (in.qual) {
            if (lane == 0) { o[0] = '+'; o[1] = '\n'; o[2 + l] = '\n'; }
            wave_copy(o + 2, in.qual + in.cum[r], l, lane);
        }
    }
}

unsigned wave_grid(int64_t n_waves_wanted) {               // blocks of four waves, at most 16384 of them (the kernels stride)
    int64_t blocks = (n_waves_wanted + 3) / 4;
    if (blocks > 256 * 64) blocks = 256 * 64;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

}  // namespace

void launch_trim_reads(const uint8_t *enc, const char *qual, const int64_t *cum, int64_t n_reads, const TrimParams &P, bwams_trim_read_t *report,
                       hipStream_t st) {
    const int64_t n_units = P.paired ? n_reads / 2 : n_reads;
    if (n_units == 0) return;
    trim_reads_kernel<<<wave_grid(n_units), 256, 0, st>>>(enc, qual, cum, n_units, P, report);
}

void launch_trim_widths(const bwams_trim_read_t *report, const int64_t *name_off, const int64_t *comment_off, int64_t n, int64_t *wide,
                        hipStream_t st) {
    trim_widths_kernel<<<(unsigned)((n + 1 + 255) / 256), 256, 0, st>>>(report, name_off, comment_off, n, wide);
}

void launch_trim_gather(const bwams_trim_read_t *report, int64_t n, const TrimArrays &in, const int64_t *offs, const TrimArrays &out,
                        hipStream_t st) {
    if (n == 0) return;
    trim_gather_kernel<<<wave_grid(n), 256, 0, st>>>(report, n, in, offs, out);
}

void launch_fastq_text_widths(const TrimArrays &in, int64_t n, int with_comment, int64_t *wide, hipStream_t st) {
    fastq_text_widths_kernel<<<(unsigned)((n + 1 + 255) / 256), 256, 0, st>>>(in, n, with_comment, wide);
}

void launch_fastq_text_emit(const TrimArrays &in, int64_t n, int with_comment, const int64_t *off, char *text, hipStream_t st) {
    if (n == 0) return;
    fastq_text_emit_kernel<<<wave_grid(n), 256, 0, st>>>(in, n, with_comment, off, text);
}

}  // namespace bwams
