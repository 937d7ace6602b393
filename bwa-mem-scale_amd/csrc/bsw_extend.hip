// bsw_extend.hip — banded Smith-Waterman seed extension for gfx950 (MI355X).
//
// Reference semantics: BandedPairWiseSW::scalarBandedSWA
// (/root/reference/src/bandedSWA.cpp:116-237), i.e. ksw_extend2: affine-gap
// extension from (0,0) with initial score h0, a band that is clipped to |i-j| <= w
// and shrinks to the non-zero part of the previous row, z-drop exit, and the six
// outputs score / qle / tle / gtle / gscore / max_off.
//
// Mapping (DESIGN.md §"BSW kernel"): one extension task per WAVEFRONT, one query
// column per lane (column j belongs to lane j & 63, chunk j >> 6), rows walked in
// order.  A row is fully parallel across its columns because in this recurrence
// the horizontal gap F is opened from M (the diagonal move), never from H:
//     F(i,j+1) = max(F(i,j) - e_ins, max(M(i,j) - o_ins - e_ins, 0))
// so F is a max-plus prefix scan of values known from the previous row, done with
// wavefront shuffles; E and M are column-local.  The row-wise band bookkeeping of
// the scalar code (row maximum and its last column, first/last non-zero column,
// z-drop) becomes wave reductions and ballots, and every decision is taken on
// complete rows exactly as the scalar loop does — an anti-diagonal sweep cannot do
// that, because the band of row i depends on all of row i-1.  Arithmetic is int32
// (scores are < 2^15 for the reference's int16 class; no saturation is relied on).
#include "common.h"
#include "wave_ops.h"

namespace bwams {

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kTaskChunk = 8;      // tasks a wave reserves per atomic (one word serves ~90 M tickets/s)
constexpr size_t kBswLdsMax = 160 * 1024;      // LDS of one CU: the most a block of bsw_kernel may take

// LDS of one wave of bsw_kernel: the (h, e) row of qmax + 1 columns, then the query, 16-byte aligned
__host__ __device__ __forceinline__ size_t bsw_row_bytes(int qmax) {
    return (((size_t)(qmax + 1) * 8 + (size_t)qmax + 64 + 15) / 16) * 16;
}

// not wave_ops.h's scan_max: with the DPP form bsw_kernel's register counts change (90 -> 78 VGPRs, 85 -> 75 SGPRs), a rescheduling of its own
__device__ __forceinline__ int wave_incl_prefix_max(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o);
        if (lane >= o) v = max(v, t);
    }
    return v;
}

__global__ __launch_bounds__(kWavesPerBlock * 64) void bsw_kernel(
    bwams_seqpair_t *__restrict__ pairs, int64_t n, const uint8_t *__restrict__ ref,
    const uint8_t *__restrict__ qer, int w0, SwParams prm, int qmax, int qlo, DevCounters *ctr, unsigned long long *head,
    const int32_t *__restrict__ list, const unsigned long long *n_list, const int64_t *__restrict__ src, int dir) {
    extern __shared__ __align__(16) unsigned char lds[];
    n = (int64_t)*n_list;                              // this kernel walks the list of tasks left to the one-task-per-wave kernels
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t per_wave = bsw_row_bytes(qmax);
    int2 *eh = reinterpret_cast<int2 *>(lds + wave * per_wave);
    uint8_t *qs = reinterpret_cast<uint8_t *>(eh + (qmax + 1));

    const int o_del = prm.o_del, e_del = prm.e_del, o_ins = prm.o_ins, e_ins = prm.e_ins;
    const int oe_del = o_del + e_del, oe_ins = o_ins + e_ins;
    unsigned long long cells = 0;

    int64_t pid = 0, pid_end = 0;          // this wave's reserved task range
    while (true) {
        if (pid >= pid_end) {
            pid = (int64_t)wave_ticket(head, (unsigned long long)kTaskChunk);   // out of line: see wave_ops.h
            pid_end = pid + kTaskChunk < n ? pid + kTaskChunk : n;
            if (pid >= n) break;
        }
        const int64_t cur = list[pid++];

        const bwams_seqpair_t sp = pairs[cur];
        const int qlen = sp.len2, tlen = sp.len1, h0 = sp.h0;
        if (qlen <= qlo) continue;                        // handled by a register-resident variant
        // src != nullptr: in place — the task's sequences start at src[2 id] (query) / src[2 id + 1] (target) and run in direction dir
        const uint8_t *tq = qer + (src ? src[2 * (int64_t)sp.id] : (int64_t)sp.idq);
        const uint8_t *tr = ref + (src ? src[2 * (int64_t)sp.id + 1] : (int64_t)sp.idr);

        // row -1 of the DP and the query, each column on its owner lane
        for (int j = lane; j <= qlen; j += 64) {
            int h = h0;
            if (j >= 1) {
                h = h0 - oe_ins - (j - 1) * e_ins;
                h = h > 0 ? h : 0;
            }
            eh[j] = make_int2(h, 0);
            if (j < qlen) qs[j] = tq[j * dir];
        }

        // clamp the band to the longest gap the score can pay for (bandedSWA.cpp:147-156)
        int w = w0;
        {
            int max_ins = (int)((double)(qlen * prm.max_sc + prm.end_bonus - o_ins) / e_ins + 1.);
            max_ins = max_ins > 1 ? max_ins : 1;
            w = w < max_ins ? w : max_ins;
            int max_del = (int)((double)(qlen * prm.max_sc + prm.end_bonus - o_del) / e_del + 1.);
            max_del = max_del > 1 ? max_del : 1;
            w = w < max_del ? w : max_del;
        }

        int mx = h0, max_i = -1, max_j = -1, max_ie = -1, gscore = -1, max_off = 0;
        int beg = 0, end = qlen;

        int tb_next = tlen > 0 ? tr[0] : 4;
        for (int i = 0; i < tlen; ++i) {
            const int tb = tb_next;
            if (i + 1 < tlen) tb_next = tr[(i + 1) * dir];           // overlap the next row's load with this row
            if (beg < i - w) beg = i - w;
            if (end > i + w + 1) end = i + w + 1;
            if (end > qlen) end = qlen;
            int h1 = 0;
            if (beg == 0) {
                h1 = h0 - (o_del + e_del * (i + 1));
                if (h1 < 0) h1 = 0;
            }
            const int sc0 = prm.mat[tb * 5 + 0], sc1 = prm.mat[tb * 5 + 1], sc2 = prm.mat[tb * 5 + 2],
                      sc3 = prm.mat[tb * 5 + 3], sc4 = prm.mat[tb * 5 + 4];

            int m = 0, mj = -1;
            int first_nz = 1 << 30, last_nz = -1;
            int f_carry = 0, hl_carry = h1, h_last = h1;
            if (beg < end) {
                cells += (unsigned long long)(end - beg);
                const int c_lo = beg >> 6, c_hi = (end - 1) >> 6;
                for (int c = c_lo; c <= c_hi; ++c) {
                    const int jb = c << 6;
                    const int j = jb + lane;
                    const bool act = j >= beg && j < end;
                    const int c0 = jb > beg ? jb : beg;          // column the carries refer to
                    int2 cell = make_int2(0, 0);
                    int qj = 4;
                    if (act) {
                        cell = eh[j];
                        qj = qs[j];
                    }
                    const int S = qj == 0 ? sc0 : qj == 1 ? sc1 : qj == 2 ? sc2 : qj == 3 ? sc3 : sc4;
                    const int M = (act && cell.x) ? cell.x + S : 0;
                    const int e = cell.y;
                    int tj = M - oe_ins;
                    tj = tj > 0 ? tj : 0;
                    const int g = act ? tj + j * e_ins : NEG;
                    const int P = wave_incl_prefix_max(g, lane);
                    int Pex = __shfl_up(P, 1);
                    if (lane == 0) Pex = NEG;
                    int F = f_carry - (j - c0) * e_ins;
                    const int F2 = Pex - (j - 1) * e_ins;
                    F = F > F2 ? F : F2;
                    int h = M > e ? M : e;
                    h = h > F ? h : F;
                    int e2 = M - oe_del;
                    e2 = e2 > 0 ? e2 : 0;
                    const int e1 = e - e_del;
                    e2 = e2 > e1 ? e2 : e1;
                    int hl = __shfl_up(h, 1);
                    if (lane == 0 || j == beg) hl = hl_carry;
                    if (act) eh[j] = make_int2(hl, e2);

                    // row maximum and the last column that attains it
                    const int hm = act ? h : -1;
                    const int cm = wave_max(hm);
                    if (cm >= m) {
                        const unsigned long long eq = __ballot(act && h == cm);
                        m = cm;
                        mj = jb + 63 - __clzll((long long)eq);
                    }
                    // first / last column whose stored (h, e) is non-zero
                    const unsigned long long nz = __ballot(act && (hl != 0 || e2 != 0));
                    if (nz) {
                        const int lo = jb + __ffsll((long long)nz) - 1;
                        const int hi = jb + 63 - __clzll((long long)nz);
                        first_nz = first_nz < lo ? first_nz : lo;
                        last_nz = hi;
                    }
                    // carries into the next chunk / the row's last H
                    int fn = F - e_ins;
                    fn = fn > tj ? fn : tj;
                    const int last_lane = (end - 1 < jb + 63 ? end - 1 : jb + 63) - jb;
                    f_carry = __shfl(fn, 63);
                    hl_carry = __shfl(h, 63);
                    h_last = __shfl(h, last_lane);
                }
            }
            const int j_exit = beg < end ? end : beg;
            const int h1f = beg < end ? h_last : h1;
            if ((end & 63) == lane) eh[end] = make_int2(h1f, 0);
            if (j_exit == qlen) {
                max_ie = gscore > h1f ? max_ie : i;
                gscore = gscore > h1f ? gscore : h1f;
            }
            if (m == 0) break;
            if (m > mx) {
                mx = m; max_i = i; max_j = mj;
                int d = mj - i;
                d = d < 0 ? -d : d;
                max_off = max_off > d ? max_off : d;
            } else if (prm.zdrop > 0) {
                if (i - max_i > mj - max_j) {
                    if (mx - m - ((i - max_i) - (mj - max_j)) * e_del > prm.zdrop) break;
                } else {
                    if (mx - m - ((mj - max_j) - (i - max_i)) * e_ins > prm.zdrop) break;
                }
            }
            // next row's band: skip leading zeros, cut trailing zeros (bandedSWA.cpp:217-221)
            const int nbeg = first_nz < end ? first_nz : end;
            int jj;
            if (h1f != 0) jj = end;
            else if (last_nz >= nbeg) jj = last_nz;
            else jj = nbeg - 1;
            beg = nbeg;
            end = jj + 2 < qlen ? jj + 2 : qlen;
        }

        if (lane == 0) {
            bwams_seqpair_t *o = &pairs[cur];
            o->score = mx;
            o->qle = max_j + 1;
            o->tle = max_i + 1;
            o->gtle = max_ie + 1;
            o->gscore = gscore;
            o->max_off = max_off;
        }
    }
    if (lane == 0 && cells) atomicAdd(&ctr->bsw_cells, cells);
}

// ---- eight tasks per wavefront -------------------------------------------------------------
// bsw_kernel above spends one wavefront on one task, with the row's band bookkeeping (beg, end, row maximum and its
// column, z-drop, ...) in scalar registers: measured, a row of <= 128 cells cost ~110 vector but ~250 scalar
// instructions, and the one scalar unit of a CU serves four SIMDs (profiles/r01_notes.md 26-28) — the scalar pipe,
// not the vector one, bounded the one-task-per-wave kernels.  In bsw_qwin_kernel a task owns kBswLpt = 8 lanes (half a
// DPP row), so
//   * eight tasks share a wavefront and every cross-lane step stays inside a DPP row (quad_perm scans + one ds_swizzle for
//     the max-plus prefix of F, row_shr for the H shift, quad_perm / row_half_mirror butterflies for the four per-row
//     reductions);
//   * the bookkeeping lives in vector registers, replicated over the task's lanes: no scalar work per row at all;
//   * a task slot that finishes takes the next task from the wave's reservation while the others carry on.
// Tasks are binned by query length first (bsw_classify_kernel) — the class fixes the LDS per task — one launch per
// class, concurrently.  Results are bit-identical to scalarBandedSWA: the recurrences and every per-row decision are
// those of bsw_kernel above.  Measured on the bench workload (5.9 M tasks, 13.4 G cells per step): one task per wave
// 89 ms; 16 lanes x all columns in registers 83; 16 x 3-column window 80; 8 x 4 66; 8 x 3 71; 8 x 6 72; 4 x 8 73 (LDS
// and registers cost occupancy); one task per LANE with its row in LDS 170 (the row caps a CU at four waves).
constexpr int kQuadCpl[5] = {2, 4, 6, 9, 12};                 // a class holds queries of <= 16 * kQuadCpl - 1 bases (16 * kQuadCpl columns of LDS)
constexpr int kBswLpt = 8, kBswWin = 4;                       // lanes per task, window columns per lane (bsw_qwin_kernel)
constexpr int kNumBswClass = 6;                              // five quad classes + the rest (one task per wave, LDS)
constexpr int kQuadChunk = 16;                               // tasks a wave reserves per atomic

__host__ __device__ __forceinline__ int bsw_class_of(int qlen, int h0, int max_sc) {
    // a column's row state is one LDS word (H and E in 14 bits each, the query base on top): needs scores < 2^14
    const long long top = (long long)h0 + (long long)qlen * max_sc;       // no score of the task can exceed it
    if (qlen > 16 * kQuadCpl[4] - 1 || top >= (1 << 14) || h0 < 0) return 5;
    return qlen <= 16 * kQuadCpl[0] - 1 ? 0 : qlen <= 16 * kQuadCpl[1] - 1 ? 1 : qlen <= 16 * kQuadCpl[2] - 1 ? 2
           : qlen <= 16 * kQuadCpl[3] - 1 ? 3 : 4;
}

// list[c * n + k] = k-th task of class c (any order: results go back by task index).  Appends are aggregated per block of
// 1024 tasks: waves count into LDS, one global atomic per class and block (one per class and WAVE was 270 k atomics on six
// addresses per launch: 1.9 ms of a kernel that reads 160 MB).
__global__ __launch_bounds__(1024) void bsw_classify_kernel(const bwams_seqpair_t *__restrict__ pairs, int64_t n, int max_sc, int32_t *__restrict__ list,
                                                            unsigned long long *cnt) {
    __shared__ unsigned int l_cnt[kNumBswClass];
    __shared__ unsigned long long l_base[kNumBswClass];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < kNumBswClass) l_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int cls = t < n ? bsw_class_of(pairs[t].len2, pairs[t].h0, max_sc) : -1;
    unsigned int my_off = 0;                       // offset of this lane's task inside the block's share of its class
#pragma unroll
    for (int c = 0; c < kNumBswClass; ++c) {
        const unsigned long long m = __ballot(cls == c);
        if (m) {
            const int leader = __ffsll((long long)m) - 1;
            unsigned int wbase = 0;
            if (lane == leader) wbase = atomicAdd(&l_cnt[c], (unsigned int)__popcll(m));
            wbase = (unsigned int)__shfl((int)wbase, leader);
            if (cls == c) my_off = wbase + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
        }
    }
    __syncthreads();
    if (threadIdx.x < kNumBswClass && l_cnt[threadIdx.x]) l_base[threadIdx.x] = atomicAdd(&cnt[threadIdx.x], (unsigned long long)l_cnt[threadIdx.x]);
    __syncthreads();
    if (cls >= 0) list[(int64_t)cls * n + (int64_t)l_base[cls] + my_off] = (int32_t)t;
}

// row-local (16-lane) DPP helpers.  A VALU write followed by a DPP read of the same register needs two wait states.
__device__ __forceinline__ int row_scan_max(int v) {            // inclusive prefix max over the lanes of a DPP row
    asm("s_nop 4\n\t"
        "v_max_i32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_i32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_i32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_i32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf"
        : "+v"(v));
    return v;
}
__device__ __forceinline__ int row_all_max(int v) {             // maximum over the 16 lanes of a DPP row, in every lane
    asm("s_nop 4\n\t"
        "v_max_i32_dpp %0, %0, %0 row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_i32_dpp %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_i32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_i32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf"
        : "+v"(v));
    return v;
}
__device__ __forceinline__ int row_shr1(int v, int fill) { return dppi<0x111, 0xF, 0xF>(fill, v); }   // lane g gets lane g - 1's v; lane 0 the fill

// ---- row state in LDS, a register window that follows the band ----------------------------------------------------
// A kernel whose cost follows the query length computes mostly dead columns: the band of a typical extension is
// narrow: ~23 live columns per row on the bench workload, because it shrinks to the non-zero span of the previous row.
// Here the row state eh[] of a task lives in LDS (one word per column: H | E << 14 | the query base << 28), and each row loads just the
// live columns [beg, end) into a window of kWin columns per lane (LPT * kWin per task: 32 as launched), computes them (F as a prefix
// maximum: a lane's own columns sequentially, then four DPP steps over the lanes), and stores them back; a band wider than the window takes further passes with the prefix maximum and
// the last H carried over.  Columns outside the band keep their stale values in LDS, as scalarBandedSWA's eh[] does.
// cross-lane steps over a task's LPT lanes (16 = one DPP row, 8 = half a row)
template <int LPT> __device__ __forceinline__ int grp_scan_max(int v, int g);
template <> __device__ __forceinline__ __attribute__((unused)) int grp_scan_max<16>(int v, int) { return row_scan_max(v); }
template <> __device__ __forceinline__ __attribute__((unused)) int grp_scan_max<8>(int v, int g) {
    // inclusive scan inside each quad (two quad_perm steps), then lanes 4..7 take the first quad's total (lane 3 of the
    // half row, fetched with ds_swizzle: source = (lane & 0b11000) | 0b00011)
    asm("s_nop 4\n\t"
        "v_max_i32_dpp %0, %0, %0 quad_perm:[0,0,1,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_i32_dpp %0, %0, %0 quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf"
        : "+v"(v));
    const int t = __builtin_amdgcn_ds_swizzle(v, 0x78);
    return (g & 4) ? (v > t ? v : t) : v;
}
template <int LPT> __device__ __forceinline__ int grp_all_max(int v);
template <> __device__ __forceinline__ __attribute__((unused)) int grp_all_max<16>(int v) { return row_all_max(v); }
template <> __device__ __forceinline__ __attribute__((unused)) int grp_all_max<8>(int v) {
    asm("s_nop 4\n\t"
        "v_max_i32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_i32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_i32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf"
        : "+v"(v));
    return v;
}
// lane g of the group gets lane g - 1's v, lane 0 the fill
template <int LPT> __device__ __forceinline__ int grp_shr1(int v, int fill, int g) {
    const int t = row_shr1(v, fill);
    return (LPT < 16 && g == 0) ? fill : t;
}


// __any() goes through a 0 / 1 VGPR and a compare; the ballot itself is a scalar AND with exec
__device__ __forceinline__ bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }

template <int LPT, int kWin>
__global__ __launch_bounds__(kWavesPerBlock * 64) void bsw_qwin_kernel(
    bwams_seqpair_t *__restrict__ pairs, const int32_t *__restrict__ list, const unsigned long long *n_list_p,
    const uint8_t *__restrict__ ref, const uint8_t *__restrict__ qer, int w0, SwParams prm, DevCounters *ctr, unsigned long long *head,
    int cols, const int64_t *__restrict__ src, int dir) {
    extern __shared__ uint32_t qwin_lds[];                         // [wave][task slot][cols]: H (14 bits) | E << 14 | query base << 28
    constexpr int TPW = 64 / LPT;                                  // tasks per wavefront
    const int lane = threadIdx.x & 63, g = lane & (LPT - 1), q = lane / LPT;
    uint32_t *const row_eh = qwin_lds + (size_t)(((threadIdx.x >> 6) * TPW + q) * cols);
    const int o_del = prm.o_del, e_del = prm.e_del, o_ins = prm.o_ins, e_ins = prm.e_ins;
    const int oe_del = o_del + e_del, oe_ins = o_ins + e_ins;
    // score rows of the matrix, one per target base: {four scores packed to bytes, the score against N}; a lane picks its task's row
    // with one LDS read per DP row instead of a chain of selects
    __shared__ uint2 pk_tab[5];
    if (threadIdx.x < 5) {
        const int t = threadIdx.x;
        pk_tab[t] = make_uint2(((uint32_t)(uint8_t)prm.mat[t * 5 + 0]) | ((uint32_t)(uint8_t)prm.mat[t * 5 + 1] << 8) |
                               ((uint32_t)(uint8_t)prm.mat[t * 5 + 2] << 16) | ((uint32_t)(uint8_t)prm.mat[t * 5 + 3] << 24),
                               (uint32_t)(int)prm.mat[t * 5 + 4]);
    }
    __syncthreads();
    const int64_t n_list = (int64_t)*n_list_p;
    const unsigned long long kLeaders = LPT == 16 ? 0x0001000100010001ull : 0x0101010101010101ull;   // lane 0 of every task slot
    int64_t pid = 0, pid_end = 0;
    bool exhausted = false;
    bool alive = false;
    int cur = 0, qlen = 0, tlen = 0, h0 = 0, w = 0, i = 0, beg = 0, end = 0;
    int mx = 0, max_i = -1, max_j = -1, max_ie = -1, gscore = -1, max_off = 0, tb_next = 4;
    const uint8_t *tr = ref;
    unsigned long long cells = 0;

    for (;;) {
        const unsigned long long need_m = __ballot(!alive);
        if (need_m) {
            if (pid >= pid_end && !exhausted) {
                pid = (int64_t)wave_ticket(head, (unsigned long long)kQuadChunk);
                pid_end = pid + kQuadChunk < n_list ? pid + kQuadChunk : n_list;
                if (pid >= n_list) { exhausted = true; pid_end = pid; }
            }
            const int avail = (int)(pid_end - pid);
            const int nq = __popcll(need_m & kLeaders);
            const int rank = __popcll(need_m & kLeaders & ((1ull << (q * LPT)) - 1ull));
            if (!alive && rank < avail) {
                cur = list[pid + rank];
                const bwams_seqpair_t sp = pairs[cur];
                qlen = sp.len2; tlen = sp.len1; h0 = sp.h0;
                const uint8_t *tq = qer + (src ? src[2 * (int64_t)sp.id] : (int64_t)sp.idq);
                tr = ref + (src ? src[2 * (int64_t)sp.id + 1] : (int64_t)sp.idr);
                for (int c = g; c <= qlen; c += LPT) {            // row -1 of the DP and the query, LPT columns at a time
                    int h = h0;
                    if (c >= 1) { h = h0 - oe_ins - (c - 1) * e_ins; h = h > 0 ? h : 0; }
                    uint32_t qb = c < qlen ? (uint32_t)tq[c * dir] : 4u;
                    qb = qb > 4u ? 4u : qb;
                    row_eh[c] = (uint32_t)h | (qb << 28);
                }
                w = w0;
                {
                    int max_ins = (int)((double)(qlen * prm.max_sc + prm.end_bonus - o_ins) / e_ins + 1.);
                    max_ins = max_ins > 1 ? max_ins : 1;
                    w = w < max_ins ? w : max_ins;
                    int max_del = (int)((double)(qlen * prm.max_sc + prm.end_bonus - o_del) / e_del + 1.);
                    max_del = max_del > 1 ? max_del : 1;
                    w = w < max_del ? w : max_del;
                }
                mx = h0; max_i = -1; max_j = -1; max_ie = -1; gscore = -1; max_off = 0;
                beg = 0; end = qlen; i = 0;
                alive = tlen > 0;
                if (!alive && g == 0) {
                    bwams_seqpair_t *o = &pairs[cur];
                    o->score = mx; o->qle = 0; o->tle = 0; o->gtle = 0; o->gscore = -1; o->max_off = 0;
                }
                tb_next = alive ? (int)tr[0] : 4;
            }
            pid += nq < avail ? nq : avail;
            if (exhausted && !wave_any(alive)) break;
        }

        // ---- one row of every live task
        int tb = tb_next;
        tb = tb > 4 ? 4 : tb;
        if (alive && i + 1 < tlen) tb_next = tr[(i + 1) * dir];
        const uint2 pp = pk_tab[tb];
        const int pkt = (int)pp.x, pnt = (int)pp.y;
        if (beg < i - w) beg = i - w;
        if (end > i + w + 1) end = i + w + 1;
        if (end > qlen) end = qlen;
        int h1 = 0;
        if (beg == 0) {
            h1 = h0 - (o_del + e_del * (i + 1));
            h1 = h1 < 0 ? 0 : h1;
        }
        const bool row = alive && beg < end;
        int key = -1, first_nz = 1 << 20, last_nz = -1, hlast = -1;
        int c_max = NEG, c_h = h1;                                  // carried into a further pass: prefix maximum, last H
        for (int base = beg; wave_any(row && base < end); base += LPT * kWin) {
            const bool in = row && base < end;
            const int jb = base + g * kWin;
            int Mv[kWin], Pl[kWin], Ev[kWin];
            uint32_t Qb[kWin];
            int run = NEG;
#pragma unroll
            for (int c = 0; c < kWin; ++c) {
                const int j = jb + c;
                const bool act = in && j < end;
                uint32_t wd = 0u;
                if (act) wd = row_eh[j];
                const int hd = (int)(wd & 0x3fffu), e = (int)((wd >> 14) & 0x3fffu);
                const uint32_t qb = wd >> 28;
                // byte qb of {pnt : pkt} (v_perm_b32: selector 0-3 = bytes of pkt, 4 = the low byte of pnt), sign-extended
                const int S = __builtin_amdgcn_sbfe((int)__builtin_amdgcn_perm((uint32_t)pnt, (uint32_t)pkt, qb), 0u, 8u);
                const int M = hd ? hd + S : 0;                      // a column outside [beg, end) read wd = 0: M = 0 there
                int tj = M - oe_ins;
                tj = tj > 0 ? tj : 0;
                // columns >= end lie to the right of every live one and nothing of theirs is stored or carried (a further pass
                // exists only when all of this pass's columns are live): their term may enter the running maximum
                const int x = tj + j * e_ins;
                run = run > x ? run : x;
                Mv[c] = M; Pl[c] = run; Ev[c] = e; Qb[c] = wd;
            }
            const int scan = grp_scan_max<LPT>(run, g);
            int Lex = grp_shr1<LPT>(scan, NEG, g);
            Lex = Lex > c_max ? Lex : c_max;
            int Hh[kWin], E2[kWin];
#pragma unroll
            for (int c = 0; c < kWin; ++c) {
                const int j = jb + c;
                int Pex = c ? Pl[c - 1] : NEG;
                Pex = Pex > Lex ? Pex : Lex;
                int F = Pex - (j - 1) * e_ins;
                F = F > 0 ? F : 0;
                const int e = Ev[c];
                int h = Mv[c] > e ? Mv[c] : e;
                h = h > F ? h : F;
                int e2 = Mv[c] - oe_del;
                e2 = e2 > 0 ? e2 : 0;
                const int e1 = e - e_del;
                e2 = e2 > e1 ? e2 : e1;
                Hh[c] = h; E2[c] = e2;
            }
            const int h_in = grp_shr1<LPT>(Hh[kWin - 1], c_h, g);
#pragma unroll
            for (int c = 0; c < kWin; ++c) {
                const int j = jb + c;
                const bool act = in && j < end;
                // column beg is lane 0's first column of the first pass, where h_in = c_h = h1 already: no select for it
                const int hl = c ? Hh[c - 1] : h_in;
                if (act) {
                    const uint32_t he = (uint32_t)hl | ((uint32_t)E2[c] << 14);
                    row_eh[j] = (he & 0x0fffffffu) | (Qb[c] & ~0x0fffffffu);      // v_bfi_b32: the query base stays where it is
                    const int k = (Hh[c] << 8) | j;
                    key = key > k ? key : k;
                    if (hl != 0 || E2[c] != 0) { first_nz = first_nz < j ? first_nz : j; last_nz = j; }
                }
            }
            {                                                       // H of column end - 1, once per pass
                const int cl = end - 1 - jb;
                if (in && cl >= 0 && cl < kWin) {
                    int hv = Hh[0];
#pragma unroll
                    for (int c = 1; c < kWin; ++c) hv = cl == c ? Hh[c] : hv;
                    hlast = hv;
                }
            }
            if (wave_any(row && base + LPT * kWin < end)) {            // a further pass: carry the prefix maximum and the last column's H
                const int pm = grp_all_max<LPT>(scan);
                c_max = c_max > pm ? c_max : pm;
                c_h = grp_all_max<LPT>(g == LPT - 1 ? Hh[kWin - 1] : -1);
            }
        }
        key = grp_all_max<LPT>(key);
        first_nz = -grp_all_max<LPT>(-first_nz);
        last_nz = grp_all_max<LPT>(last_nz);
        hlast = grp_all_max<LPT>(hlast);
        const int m = row ? key >> 8 : 0, mj = row ? key & 0xff : -1;
        const int h1f = row ? hlast : h1;
        if (alive) {
            if (g == 0) {                                           // eh[end] = {h1f, 0}
                row_eh[end] = (uint32_t)h1f | (row_eh[end] & 0xf0000000u);
            }
            if (row) cells += (unsigned long long)(g == 0 ? end - beg : 0);
            const int j_exit = row ? end : beg;
            if (j_exit == qlen) {
                max_ie = gscore > h1f ? max_ie : i;
                gscore = gscore > h1f ? gscore : h1f;
            }
            bool fin = m == 0;
            if (!fin) {
                if (m > mx) {
                    mx = m; max_i = i; max_j = mj;
                    int d = mj - i;
                    d = d < 0 ? -d : d;
                    max_off = max_off > d ? max_off : d;
                } else if (prm.zdrop > 0) {
                    if (i - max_i > mj - max_j) fin = mx - m - ((i - max_i) - (mj - max_j)) * e_del > prm.zdrop;
                    else fin = mx - m - ((mj - max_j) - (i - max_i)) * e_ins > prm.zdrop;
                }
            }
            if (!fin) {
                const int nbeg = first_nz < end ? first_nz : end;
                int jj;
                if (h1f != 0) jj = end;
                else if (last_nz >= nbeg) jj = last_nz;
                else jj = nbeg - 1;
                beg = nbeg;
                end = jj + 2 < qlen ? jj + 2 : qlen;
                ++i;
                fin = i >= tlen;
            }
            if (fin) {
                if (g == 0) {
                    bwams_seqpair_t *o = &pairs[cur];
                    o->score = mx; o->qle = max_j + 1; o->tle = max_i + 1; o->gtle = max_ie + 1; o->gscore = gscore; o->max_off = max_off;
                }
                alive = false;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) cells += ((unsigned long long)__shfl_down((unsigned)(cells >> 32), o) << 32) | (unsigned)__shfl_down((unsigned)cells, o);
    if (lane == 0 && cells) atomicAdd(&ctr->bsw_cells, cells);
}


// ---- sixteen tasks per wavefront, packed 16-bit columns ---------------------------------------------------------------
// bsw_qwin_kernel spends ≈ 290 vector instructions on a row of eight tasks: 177 in the four-columns-per-lane pass, 114 in the
// row's bookkeeping, all of it 32-bit — although every score of these classes is below 2^14 and the packed 16-bit forms
// (v_pk_add / sub / max / min / mul_lo) issue at the same rate (tools/ubench_valu.hip).  Here a task owns FOUR lanes (one quad:
// every cross-lane step is a quad_perm DPP) and a lane owns EIGHT columns as four packed registers, so a wavefront carries sixteen
// tasks: the bookkeeping is shared by twice as many tasks and the pass handles two columns per instruction, with the register
// footprint of the 8 x 4 form (the 32-bit 4 x 8 form had lost to it on occupancy, note 32).
//   * Row state in LDS per task: three arrays of column PAIRS — H (H(i, j-1) as scalarBandedSWA's eh[].h), E, and the v_perm
//     selector that picks the two columns' scores out of the target base's score row — read and written 16 bytes per lane.
//   * The window of a pass starts at a multiple of 8 columns, so a lane's eight columns are one aligned 16-byte access; the
//     columns of the window outside [beg, end) are masked (their state reads as zero and is written back unchanged).
//   * F is the same max-plus prefix scan: inside the lane over its eight columns (packed, the carry broadcast with v_perm),
//     over the four lanes with two quad_perm steps.
//   * The row maximum and the last column attaining it travel as one 32-bit key (H << 8 | j) per column through v_max3.
// Recurrences and per-row decisions are those of bsw_qwin_kernel; results are bit-identical to scalarBandedSWA.
// Eligible: scores below 2^14 (the class condition), every score against N equal to -1 (the selector's 0xff bytes), gap
// extension costs small enough for j * e_ins to stay inside 16 bits.  Other scoring schemes keep the 32-bit kernel.
namespace pk {
__device__ __forceinline__ uint32_t add(uint32_t a, uint32_t b) { uint32_t d; asm("v_pk_add_u16 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ uint32_t sub(uint32_t a, uint32_t b) { uint32_t d; asm("v_pk_sub_i16 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ uint32_t max(uint32_t a, uint32_t b) { uint32_t d; asm("v_pk_max_i16 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ uint32_t max0(uint32_t a) { uint32_t d; asm("v_pk_max_i16 %0, %1, 0" : "=v"(d) : "v"(a)); return d; }
__device__ __forceinline__ uint32_t mul(uint32_t a, uint32_t b) { uint32_t d; asm("v_pk_mul_lo_u16 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ uint32_t mad(uint32_t a, uint32_t b, uint32_t c) { uint32_t d; asm("v_pk_mad_u16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c)); return d; }
// The second operand WAVE-UNIFORM, read from a scalar register (a packed instruction takes one): a constant of the launch then costs
// no vector register and no copy into one.  Only for values that are uniform by construction (kernel arguments and what is made of them)
__device__ __forceinline__ uint32_t adds(uint32_t a, uint32_t s) { uint32_t d; asm("v_pk_add_u16 %0, %1, %2" : "=v"(d) : "v"(a), "s"(s)); return d; }
__device__ __forceinline__ uint32_t subs(uint32_t a, uint32_t s) { uint32_t d; asm("v_pk_sub_i16 %0, %1, %2" : "=v"(d) : "v"(a), "s"(s)); return d; }
// small constants in both halves: the inline constant's low half taken for both (op_sel_hi)
__device__ __forceinline__ uint32_t add2(uint32_t a) { uint32_t d; asm("v_pk_add_u16 %0, %1, 2 op_sel_hi:[1,0]" : "=v"(d) : "v"(a)); return d; }
__device__ __forceinline__ uint32_t min1(uint32_t a) { uint32_t d; asm("v_pk_min_u16 %0, %1, 1 op_sel_hi:[1,0]" : "=v"(d) : "v"(a)); return d; }
__device__ __forceinline__ uint32_t hi2(uint32_t a) { return __builtin_amdgcn_perm(a, a, 0x03020302u); }      // the high half in both halves
__device__ __forceinline__ uint32_t lo2(uint32_t a) { return __builtin_amdgcn_perm(a, a, 0x01000100u); }      // the low half in both halves
// (a & mask) | (b & ~mask) as the one instruction it is (written in C it compiles to three or four)
__device__ __forceinline__ uint32_t bfi(uint32_t mask, uint32_t a, uint32_t b) { uint32_t d; asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(d) : "v"(mask), "v"(a), "v"(b)); return d; }
// quad_perm moves: every source lane exists, so bound_ctrl changes no value, and with it the move folds into the instruction that uses it
template <int CTRL> __device__ __forceinline__ int qdpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
__device__ __forceinline__ int quad_all_max(int v) {
    int t = qdpp<0xB1>(v);                       // quad_perm [1,0,3,2]
    v = v > t ? v : t;
    t = qdpp<0x4E>(v);                           // quad_perm [2,3,0,1]
    return v > t ? v : t;
}
}  // namespace pk

constexpr int kPkNeg = -16384;
#ifndef BWAMS_PK_WAVES
#define BWAMS_PK_WAVES 2
#endif
#ifndef BWAMS_BSW_EARLY_FORM
#define BWAMS_BSW_EARLY_FORM 1
#endif
constexpr int kPkEarlyForm = BWAMS_BSW_EARLY_FORM;   // how often the early exit is tested: 1 after every row, 2 after every fourth (the A-B of profiles/bsw_early_exit.md)
constexpr int kPkWaves = BWAMS_PK_WAVES;      // wavefronts per workgroup: LDS is handed out per workgroup, small ones pack a CU better

__host__ __device__ __forceinline__ bool bsw_pk_eligible(const SwParams &prm) {
    for (int i = 0; i < 5; ++i)
        if (prm.mat[i * 5 + 4] != -1 || prm.mat[4 * 5 + i] != -1) return false;
    return prm.e_ins >= 0 && prm.e_ins <= 64 && prm.e_del >= 0 && prm.e_del <= 64 && prm.o_ins >= 0 && prm.o_ins + prm.e_ins < 8000 &&
           prm.o_del >= 0 && prm.o_del + prm.e_del < 8000;
}

// EARLY: the early exit ("BSW kernel: the early exit").  After a completed row nothing a later row computes can exceed
//     P = max over the stored columns of  H(i, j) + a (qlen - 1 - j)  and  E(i + 1, j) + a (qlen - 1 - j)  (non-zero cells only)
//         and h1 + a qlen for the first-column value h1 of a row that starts at column 0
// (a = max_sc: only a diagonal step gains, at most a, and uses up a column; a zero cell is no source; the band clip and the trim only
// take cells away).  When P <= max and P < gscore the six outputs are final and the task ends there, exactly as a row maximum of 0
// ends it.  H(i, j) is what the row stores as column j + 1's diagonal source, so H and E of a column share one remainder and the
// potentials come from the pass's packed Hn and E2 registers.  The rule needs every stored cell to the right of the row's band to
// be zero: zr is a column beyond which that holds (stale cells lie there only from row -1 or where the w clip cut the band), set
// to the trim's last non-zero column after every row whose end reaches it.  It starts at qlen, not at row -1's last positive column:
// the rule cannot fire before gscore is set, which takes a row with end == qlen >= either, and from that row on the two agree.
// 0: none of it (the instance is the kernel without the rule); 1: tested after every row; 2: after the rows with (i & 3) == 3.
template <int EARLY>
__global__ __launch_bounds__(kPkWaves * 64) __attribute__((amdgpu_waves_per_eu(4, 4))) void bsw_pk_kernel(      // four waves per SIMD: 128 VGPRs
    bwams_seqpair_t *__restrict__ pairs, const int32_t *__restrict__ list, const unsigned long long *n_list_p,
    const uint8_t *__restrict__ ref, const uint8_t *__restrict__ qer, int w0, SwParams prm, DevCounters *ctr, unsigned long long *head,
    int cols, const int64_t *__restrict__ src, int dir) {
    // 16 words of score rows, then [wave][task slot][H pairs | E pairs | selector bytes]: 4 + 4 + 2 bytes per pair.  Everything is carved out
    // of the dynamic region: a static __shared__ array in front of it would shift its base off 16 bytes (16-byte DS accesses
    // off their alignment are replayed at 64 cycles each)
    extern __shared__ __align__(16) uint32_t pk_lds[];
    constexpr int LPT = 4, TPW = 16;
    const int lane = threadIdx.x & 63, g = lane & (LPT - 1), q = lane / LPT;
    const int P = cols >> 1;
    // per task 10 P + 24 bytes (P = cols / 2 pairs, a multiple of 4): H and E each P + 2 words, the selector bytes P / 2 + 1 words, and one
    // word to keep the next task 8-byte aligned.  The two spare words let a lane whose eight columns begin at cols - 4 read and write
    // back (masked) past the last pair without touching a neighbour
    uint32_t *const t_hp = pk_lds + 16 + (size_t)((threadIdx.x >> 6) * TPW + q) * (size_t)((5 * P) / 2 + 6);
    uint32_t *const t_ep = t_hp + P + 2;
    uint16_t *const t_sel = reinterpret_cast<uint16_t *>(t_ep + P + 2);   // per pair the selectors' low bytes {2 qb0, 2 qb1} (0x0d for N)
    uint16_t *const t_hp16 = reinterpret_cast<uint16_t *>(t_hp), *const t_ep16 = reinterpret_cast<uint16_t *>(t_ep);
    const int o_del = prm.o_del, e_del = prm.e_del, o_ins = prm.o_ins, e_ins = prm.e_ins;
    const int oe_del = o_del + e_del, oe_ins = o_ins + e_ins;
    // the score row of a target base as four 16-bit scores {A, C | G, T}; every score against N is -1 = the selector's 0xff bytes
    uint2 *const pk_tab16 = reinterpret_cast<uint2 *>(pk_lds);
    if (threadIdx.x < 5) {
        const int t = threadIdx.x;
        pk_tab16[t] = make_uint2((uint32_t)(uint16_t)(int16_t)prm.mat[t * 5 + 0] | ((uint32_t)(uint16_t)(int16_t)prm.mat[t * 5 + 1] << 16),
                                 (uint32_t)(uint16_t)(int16_t)prm.mat[t * 5 + 2] | ((uint32_t)(uint16_t)(int16_t)prm.mat[t * 5 + 3] << 16));
    }
    __syncthreads();
    const uint32_t OEI = (uint32_t)oe_ins * 0x10001u, OED = (uint32_t)oe_del * 0x10001u, EDX = (uint32_t)e_del * 0x10001u;
    const uint32_t E1X = (uint32_t)e_ins * 0x10001u, E2X = (uint32_t)(2 * e_ins) * 0x10001u;
    const uint32_t NEGP = (uint32_t)(uint16_t)(int16_t)kPkNeg * 0x10001u;
    const int64_t n_list = (int64_t)*n_list_p;
    const unsigned long long kLeaders = 0x1111111111111111ull;    // lane 0 of every task slot
    int64_t pid = 0, pid_end = 0;
    bool exhausted = false;
    bool alive = false;
    // the ticket in hand, staged when it is taken: lane k < kQuadChunk holds the descriptor of its k-th task (s_qh: qlen | h0 << 8 | the
    // first target base << 24; s_w: the clamped band), a refilling quad fetches its own with ds_bpermute
    int64_t pid0 = 0, s_qo = 0, s_to = 0;
    int s_cur = 0, s_tlen = 0, s_w = 0;
    uint32_t s_qh = 0u;
    int cur = 0, qlen = 0, tlen = 0, h0 = 0, w = 0, i = 0, beg = 0, end = 0;
    int mx = 0, max_i = -1, max_j = -1, max_ie = -1, gscore = -1, max_off = 0, tb_next = 4;
    const uint8_t *tr = ref;
    unsigned long long cells = 0;
    // the row in progress (a row may take several iterations: one per window of 32 columns)
    bool start_row = true, row = false;
    int base = 0, h1 = 0, key = -1, hlast = -1, c_max = kPkNeg, c_h = 0;
    int nz_last = 0, nz_first = 256;           // of the row so far: its last column with a non-zero stored cell, plus one (0: none); its first (256: none)
    uint2 tt = make_uint2(0u, 0u);
    int zr = 0;                                // EARLY: every stored cell of a column beyond zr is zero
    uint32_t pot = 0u;                         // EARLY: of the row so far, the largest potential of a stored cell (two 16-bit halves)
#ifdef BWAMS_BSWDBG                 // wave-time of the refill branch and of the pass (printed by run_side under BWAMS_VERBOSE)
    const unsigned long long T0 = __builtin_amdgcn_s_memtime();
    unsigned long long t_refill = 0, t_pass = 0, n_events = 0, n_filled = 0, n_iter = 0, n_rows = 0, n_rule = 0;
#endif

    for (;;) {
        const unsigned long long need_m = __ballot(!alive);
        if (need_m) {
#ifdef BWAMS_BSWDBG
            const unsigned long long Ta = __builtin_amdgcn_s_memtime();
#endif
            if (pid >= pid_end && !exhausted) {
                pid = (int64_t)wave_ticket(head, (unsigned long long)kQuadChunk);
                pid_end = pid + kQuadChunk < n_list ? pid + kQuadChunk : n_list;
                if (pid >= n_list) { exhausted = true; pid_end = pid; }
                // one dependent chain of loads (list entry, task, its two source offsets, the first target base) for the ticket's
                // sixteen tasks, and the band clamp with its two divisions once, sixteen lanes wide
                pid0 = pid;
                if (lane < kQuadChunk && pid + lane < pid_end) {
                    s_cur = list[pid + lane];
                    const bwams_seqpair_t *sp = &pairs[s_cur];
                    const int l2 = sp->len2, hh0 = sp->h0;
                    s_tlen = sp->len1;
                    if (src) { const int64_t id = sp->id; s_qo = src[2 * id]; s_to = src[2 * id + 1]; }
                    else { s_qo = (int64_t)sp->idq; s_to = (int64_t)sp->idr; }
                    uint32_t tb = s_tlen > 0 ? (uint32_t)ref[s_to] : 4u;
                    tb = tb > 4u ? 4u : tb;
                    s_qh = (uint32_t)l2 | ((uint32_t)hh0 << 8) | (tb << 24);          // the class: qlen <= 191, 0 <= h0 < 2^14
                    int ww = w0;
                    int max_ins = (int)((double)(l2 * prm.max_sc + prm.end_bonus - o_ins) / e_ins + 1.);
                    max_ins = max_ins > 1 ? max_ins : 1;
                    ww = ww < max_ins ? ww : max_ins;
                    int max_del = (int)((double)(l2 * prm.max_sc + prm.end_bonus - o_del) / e_del + 1.);
                    max_del = max_del > 1 ? max_del : 1;
                    s_w = ww < max_del ? ww : max_del;
                }
            }
            const int avail = (int)(pid_end - pid);
            const int nq = __popcll(need_m & kLeaders);
            const int rank = __popcll(need_m & kLeaders & ((1ull << (q * LPT)) - 1ull));
            if (avail > 0) {                                              // wave-uniform: nothing to hand out once the list has run dry
                const bool take = !alive && rank < avail;
                // every lane fetches (a bpermute reads nothing from a lane that is switched off), the taking quads keep
                const int sk = take ? (int)(pid - pid0) + rank : 0;
                const int f_cur = __shfl(s_cur, sk), f_tlen = __shfl(s_tlen, sk), f_w = __shfl(s_w, sk);
                const uint32_t f_qh = (uint32_t)__shfl((int)s_qh, sk);
                const int64_t f_qo = shfl64(s_qo, sk), f_to = shfl64(s_to, sk);
                if (take) {
                    cur = f_cur; qlen = (int)(f_qh & 0xffu); h0 = (int)((f_qh >> 8) & 0x3fffu); tlen = f_tlen; w = f_w;
                    tr = ref + f_to;
                    start_row = true;
                    mx = h0; max_i = -1; max_j = -1; max_ie = -1; gscore = -1; max_off = 0;
                    beg = 0; end = qlen; i = 0;
                    if constexpr (EARLY != 0) zr = qlen;
                    alive = tlen > 0;
                    if (!alive && g == 0) {
                        bwams_seqpair_t *o = &pairs[cur];
                        o->score = mx; o->qle = 0; o->tle = 0; o->gtle = 0; o->gscore = -1; o->max_off = 0;
                    }
                    tb_next = (int)(f_qh >> 24);
                }
                // row -1 of the DP and the query of every slot that took a task, one slot at a time with the whole wave: a lane writes one
                // granule of four columns (two pairs), so a query of up to 255 bases is one trip and one memory round trip.  A granule inside
                // the query is one 4-byte load at the task's own bytes (at any alignment, reversed for dir = -1); the granule the query ends
                // in takes byte loads, so no load touches a byte that is not the task's
                for (unsigned long long fill_m = __ballot(take) & kLeaders; fill_m; fill_m &= fill_m - 1ull) {
                    const int sl = __ffsll((long long)fill_m) - 1;                // lane 0 of the slot
                    const int f_qlen = __builtin_amdgcn_readlane(qlen, sl), f_h0 = __builtin_amdgcn_readlane(h0, sl);
                    const uint8_t *const f_q = qer + readlane64(f_qo, sl);
                    uint32_t *const f_hp = pk_lds + 16 + (size_t)((threadIdx.x >> 6) * TPW + (sl >> 2)) * (size_t)((5 * P) / 2 + 6);
                    uint32_t *const f_ep = f_hp + P + 2;
                    uint16_t *const f_sel = reinterpret_cast<uint16_t *>(f_ep + P + 2);
                    const int c0 = 4 * lane, p_last = f_qlen >> 1;
                    // every load is issued before the first of them is waited for: the values meet only behind the branches
                    const bool full = c0 + 3 < f_qlen, edge = !full && c0 < f_qlen;
                    uint32_t v = 0u, b0 = 4u, b1 = 4u, b2 = 4u;
                    if (full) __builtin_memcpy(&v, dir > 0 ? f_q + c0 : f_q - c0 - 3, 4);
                    if (edge) {                                                  // positions past the query's end read its last byte again
                        const int last = f_qlen - 1;
                        b0 = f_q[c0 * dir];
                        b1 = f_q[(c0 + 1 < last ? c0 + 1 : last) * dir];
                        b2 = f_q[(c0 + 2 < last ? c0 + 2 : last) * dir];
                    }
                    b1 = c0 + 1 < f_qlen ? b1 : 4u;
                    b2 = c0 + 2 < f_qlen ? b2 : 4u;
                    const uint32_t qw = full ? (dir > 0 ? v : __builtin_amdgcn_perm(v, v, 0x00010203u)) : (b0 | (b1 << 8) | (b2 << 16) | 0x04000000u);
                    uint32_t hh[2] = {0u, 0u}, ss[2] = {0u, 0u};
    #pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int c = c0 + k;
                        int h = 0;
                        if (c <= f_qlen) { h = f_h0; if (c >= 1) { h = f_h0 - oe_ins - (c - 1) * e_ins; h = h > 0 ? h : 0; } }
                        const uint32_t qb = (qw >> (8 * k)) & 0xffu;
                        const uint32_t sel = qb < 4u ? 2u * qb : 0x0du;
                        hh[k >> 1] |= (uint32_t)h << (16 * (k & 1));
                        ss[k >> 1] |= sel << (8 * (k & 1));
                    }
    #pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const int p = 2 * lane + k;
                        if (p <= p_last) { f_hp[p] = hh[k]; f_ep[p] = 0u; f_sel[p] = (uint16_t)ss[k]; }
                    }
                }
                // the lanes that wrote a row are not the quad that reads it: the writes are done before the pass below begins (the row is
                // this wavefront's alone, so no barrier)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            pid += nq < avail ? nq : avail;
#ifdef BWAMS_BSWDBG
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            t_refill += __builtin_amdgcn_s_memtime() - Ta;
            ++n_events; n_filled += (unsigned long long)(nq < avail ? nq : avail);
#endif
            if (exhausted && !wave_any(alive)) break;
        }
#ifdef BWAMS_BSWDBG
        const unsigned long long Tb = __builtin_amdgcn_s_memtime();
#endif

        // ---- one PASS (a window of 32 columns) of the current row of every live task.  The tasks of a wavefront do not wait for
        // each other at the end of a row: a task whose row needs a second window takes it in the next iteration while the others
        // are already on their next rows, so an iteration costs the same whether one task or all sixteen have a wide band.
        asm volatile("; BSW_PK_PASS_BEGIN");                          // tools/isa_count.py counts between the two markers
        if (alive && start_row) {                                     // row prologue
            int tb = tb_next;
            tb = tb > 4 ? 4 : tb;
            if (i + 1 < tlen) tb_next = tr[(i + 1) * dir];
            tt = pk_tab16[tb];
            if (beg < i - w) beg = i - w;
            if (end > i + w + 1) end = i + w + 1;
            if (end > qlen) end = qlen;
            h1 = 0;
            if (beg == 0) {
                h1 = h0 - (o_del + e_del * (i + 1));
                h1 = h1 < 0 ? 0 : h1;
            }
            row = beg < end;
            key = -1; hlast = -1; nz_last = 0; nz_first = 256;
            c_max = kPkNeg; c_h = 0;
            if constexpr (EARLY != 0) pot = 0u;
            base = beg & ~3;
            start_row = false;
        }
        {
            const bool in = alive && row;
            const int jb = base + g * 8;
            const bool inr = in && jb < cols;
            // the lane's live columns as a bit mask, then as four pair masks
            int lo = beg - jb, hi = end - jb;
            lo = lo < 0 ? 0 : (lo > 8 ? 8 : lo);
            hi = hi < 0 ? 0 : (hi > 8 ? 8 : hi);
            const uint32_t m8 = inr ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
            const uint32_t m8x = m8 | (m8 << 15);                     // bit k also at bit k + 15: an odd column's bit 16 above the even one's before it
            // the window starts at a multiple of FOUR columns (a band of the typical 23 columns then fits one window almost always;
            // at a multiple of eight a fifth of the rows needed a second one): the lane's eight columns are 8-byte aligned in the H and E
            // arrays, 4-byte aligned in the selector bytes.  Lanes without a live column read too (whatever lies there: it is masked)
            const int pj = inr ? (jb >> 1) : 0;
            const uint2 hpa = *reinterpret_cast<const uint2 *>(t_hp + pj), hpb = *reinterpret_cast<const uint2 *>(t_hp + pj + 2);
            const uint2 epa = *reinterpret_cast<const uint2 *>(t_ep + pj), epb = *reinterpret_cast<const uint2 *>(t_ep + pj + 2);
            uint2 sl2;
            sl2.x = *reinterpret_cast<const uint32_t *>(t_sel + pj);
            sl2.y = *reinterpret_cast<const uint32_t *>(t_sel + pj + 2);
            const uint32_t hpv[4] = {hpa.x, hpa.y, hpb.x, hpb.y}, epv[4] = {epa.x, epa.y, epb.x, epb.y};
            // a pair's selector {2 qb0, 2 qb0 + 1, 2 qb1, 2 qb1 + 1} from its two stored bytes (N: 0x0d, 0x0e: both give 0xff)
            const uint32_t slv[4] = {__builtin_amdgcn_perm(sl2.x, sl2.x, 0x01010000u) + 0x01000100u, __builtin_amdgcn_perm(sl2.x, sl2.x, 0x03030202u) + 0x01000100u,
                                     __builtin_amdgcn_perm(sl2.y, sl2.y, 0x01010000u) + 0x01000100u, __builtin_amdgcn_perm(sl2.y, sl2.y, 0x03030202u) + 0x01000100u};
            uint32_t AM[4], M[4], E[4], PX[4], JE[4], JP[4];
            JE[0] = (uint32_t)(jb * e_ins) * 0x10001u + ((uint32_t)e_ins << 16);
            JP[0] = (uint32_t)jb * 0x10001u + 0x00020001u;            // (j + 1, j + 2)
#pragma unroll
            for (int c = 1; c < 4; ++c) { JE[c] = pk::adds(JE[c - 1], E2X); JP[c] = pk::add2(JP[c - 1]); }
            // Stage by stage over the four pairs, not pair by pair: dependent packed (VOP3P) instructions need a wait state between them
            // (the compiler fills it with s_nop 0: 34 per window in the pair-by-pair order), and the four pairs are independent.
            uint32_t Hm[4], T1[4], T2[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {                            // bits 2c and 2c + 1 of m8 at bits 15 and 31, then v_perm's sign selectors 8 and 9
                const uint32_t x = m8x << (15 - 2 * c);
                AM[c] = __builtin_amdgcn_perm(x, x, 0x09090808u);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) { Hm[c] = hpv[c] & AM[c]; E[c] = epv[c] & AM[c]; }
#pragma unroll
            for (int c = 0; c < 4; ++c) T1[c] = pk::add(Hm[c], __builtin_amdgcn_perm(tt.y, tt.x, slv[c]));
#pragma unroll
            for (int c = 0; c < 4; ++c) T2[c] = pk::min1(Hm[c]);
#pragma unroll
            for (int c = 0; c < 4; ++c) M[c] = pk::mul(T1[c], T2[c]);                                   // M = H ? H + S : 0
#pragma unroll
            for (int c = 0; c < 4; ++c) T1[c] = pk::subs(M[c], OEI);
#pragma unroll
            for (int c = 0; c < 4; ++c) T1[c] = pk::max0(T1[c]);
#pragma unroll
            for (int c = 0; c < 4; ++c) T1[c] = pk::add(T1[c], JE[c]);
#pragma unroll
            for (int c = 0; c < 4; ++c) PX[c] = pk::max(T1[c], T1[c] << 16);                            // the pair's inclusive prefix (x >= 0)
#pragma unroll
            for (int c = 1; c < 4; ++c) PX[c] = pk::max(PX[c], pk::hi2(PX[c - 1]));
            // over the four lanes of the task
            int scan = (int)(PX[3] >> 16);
            {
                int t = pk::qdpp<0x90>(scan);                          // quad_perm [0,0,1,2]
                scan = scan > t ? scan : t;
                t = pk::qdpp<0x44>(scan);                              // quad_perm [0,1,0,1]
                scan = scan > t ? scan : t;
            }
            int Lex = pk::qdpp<0x90>(scan);
            Lex = g == 0 ? kPkNeg : Lex;
            Lex = Lex > c_max ? Lex : c_max;
            const uint32_t Lexp = pk::lo2((uint32_t)Lex);
            uint32_t Hn[4], E2[4], F4[4], ME[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) F4[c] = __builtin_amdgcn_alignbit(PX[c], c ? PX[c - 1] : NEGP, 16);      // {prefix up to column j - 1}
#pragma unroll
            for (int c = 0; c < 4; ++c) { F4[c] = pk::max(F4[c], Lexp); E2[c] = pk::subs(M[c], OED); }
#pragma unroll
            for (int c = 0; c < 4; ++c) { F4[c] = pk::sub(F4[c], JE[c]); T1[c] = pk::subs(E[c], EDX); ME[c] = pk::max(M[c], E[c]); }
#pragma unroll
            for (int c = 0; c < 4; ++c) { F4[c] = pk::adds(F4[c], E1X); E2[c] = pk::max(E2[c], T1[c]); }
#pragma unroll
            for (int c = 0; c < 4; ++c) { F4[c] = pk::max0(F4[c]); E2[c] = pk::max0(E2[c]); }                    // F = max(Pex - (j - 1) e_ins, 0)
#pragma unroll
            for (int c = 0; c < 4; ++c) Hn[c] = pk::max(ME[c], F4[c]);
            // what is stored: H(i, j - 1) beside E(i + 1, j); the column to the left of the lane's first comes from the lane before
            const int h3 = (int)(Hn[3] >> 16);
            int hin = pk::qdpp<0x90>(h3);
            hin = g == 0 ? c_h : hin;
            uint32_t HL[4];
            HL[0] = __builtin_amdgcn_alignbit(Hn[0], (uint32_t)hin << 16, 16);
#pragma unroll
            for (int c = 1; c < 4; ++c) HL[c] = __builtin_amdgcn_alignbit(Hn[c], Hn[c - 1], 16);
            if (m8) {
                *reinterpret_cast<uint2 *>(t_hp + pj) = make_uint2(pk::bfi(AM[0], HL[0], hpv[0]), pk::bfi(AM[1], HL[1], hpv[1]));
                *reinterpret_cast<uint2 *>(t_hp + pj + 2) = make_uint2(pk::bfi(AM[2], HL[2], hpv[2]), pk::bfi(AM[3], HL[3], hpv[3]));
                *reinterpret_cast<uint2 *>(t_ep + pj) = make_uint2(pk::bfi(AM[0], E2[0], epv[0]), pk::bfi(AM[1], E2[1], epv[1]));
                *reinterpret_cast<uint2 *>(t_ep + pj + 2) = make_uint2(pk::bfi(AM[2], E2[2], epv[2]), pk::bfi(AM[3], E2[3], epv[3]));
            }
            // row maximum with the last column attaining it; first / last column with a non-zero stored cell
            int lkey = -1;
            // key = H << 8 | (j + 1), one v_perm per column: the bytes {index, H low, H high, 0}.  A dead column contributes
            // (0 << 8 | j + 1) < 256: below every live key of a row whose maximum is positive, and the column of the maximum is
            // not read when the maximum is 0
            if constexpr (EARLY != 0) {
                // per pair the remainders a (qlen - 1 - j) of its two columns; X = max(H, E) of the live columns (E2 of a dead column is 0),
                // X ? X + remainder : 0 as one multiply-add with min(X, 1); below 2^14, as every score of the class
                const uint32_t A2X = (uint32_t)(2 * prm.max_sc) * 0x10001u;
                uint32_t RM[4], X[4], T[4];
                RM[0] = pk::lo2((uint32_t)__mul24(qlen - 1 - jb, prm.max_sc)) - ((uint32_t)prm.max_sc << 16);
#pragma unroll
                for (int c = 1; c < 4; ++c) RM[c] = pk::subs(RM[c - 1], A2X);
#pragma unroll
                for (int c = 0; c < 4; ++c) X[c] = pk::max(Hn[c] & AM[c], E2[c]);
#pragma unroll
                for (int c = 0; c < 4; ++c) T[c] = pk::min1(X[c]);
#pragma unroll
                for (int c = 0; c < 4; ++c) X[c] = pk::mad(T[c], RM[c], X[c]);
                pot = pk::max(pot, pk::max(pk::max(X[0], X[1]), pk::max(X[2], X[3])));
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t ha = Hn[c] & AM[c];
                const int k0 = (int)__builtin_amdgcn_perm(ha, JP[c], 0x0c050400u), k1 = (int)__builtin_amdgcn_perm(ha, JP[c], 0x0c070602u);
                const int kk = k0 > k1 ? k0 : k1;
                lkey = lkey > kk ? lkey : kk;
            }
            {
                // a bit per column of the window that is live and stores a non-zero H or E: per pair {0 | 1, 0 | 1}, the lane's eight as bits
                // 0-7 (even columns from the low halves, odd ones from the high halves), the quad's 32 as one word, the same in its four lanes
                uint32_t NF[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) NF[c] = (HL[c] | E2[c]) & AM[c];
#pragma unroll
                for (int c = 0; c < 4; ++c) NF[c] = pk::min1(NF[c]);
                const uint32_t nx = NF[0] | (NF[1] << 2) | (NF[2] << 4) | (NF[3] << 6);
                const int nl = (int)(((nx | (nx >> 15)) & 0xffu) << (8 * g));
                int nw = nl | pk::qdpp<0xB1>(nl);
                nw |= pk::qdpp<0x4E>(nw);
                // windows come in ascending order: the last one with a bit set has the row's last such column, the first one its first
                const bool any = nw != 0;
                const int fc = any ? base + __builtin_ctz((unsigned)nw) : 256;
                nz_last = any ? base + 32 - __builtin_clz((unsigned)nw) : nz_last;
                nz_first = nz_first < fc ? nz_first : fc;
            }
            lkey = m8 ? lkey : -1;                                  // a lane without a live column contributes nothing
            key = key > lkey ? key : lkey;
            {                                                       // H of column end - 1, once per row
                const int oe = hi - 1;
                if (m8 && jb + hi == end) {
                    uint32_t hv = Hn[0];
                    hv = (oe >> 1) == 1 ? Hn[1] : hv;
                    hv = (oe >> 1) == 2 ? Hn[2] : hv;
                    hv = (oe >> 1) == 3 ? Hn[3] : hv;
                    hlast = (int)((hv >> ((oe & 1) << 4)) & 0xffffu);
                }
            }
            if (in && base == (beg & ~3) && h1 != 0 && g == 0) t_hp16[beg] = (uint16_t)h1;      // eh[beg].h = h1: H(i, beg - 1) of a row that starts at column 0
            // a further window of this row: carry the prefix maximum and the last column's H into the next iteration
            const int pm = pk::qdpp<0xFF>(scan);                       // quad_perm [3,3,3,3]: the task's inclusive total
            const int ch = pk::qdpp<0xFF>(h3);
            const bool more = in && base + LPT * 8 < end;
            if (more) {
                c_max = c_max > pm ? c_max : pm;
                c_h = ch;
                base += LPT * 8;
            }
            // ---- the end of a row
            const int rkey = pk::quad_all_max(key), rhl = pk::quad_all_max(hlast);
            int rpot = 0;
            if constexpr (EARLY != 0) {
                const int a = (int)(pot & 0xffffu), b = (int)(pot >> 16);
                rpot = pk::quad_all_max(a > b ? a : b);
            }
            int last_nz = nz_last - 1;                                  // -1: none
            int first_nz = nz_first;                                    // 256: none (beyond every column)
            if (alive && !more) {
                if (row && h1 != 0) {                                    // column beg stores h1 (see above)
                    first_nz = first_nz < beg ? first_nz : beg;
                    last_nz = last_nz > beg ? last_nz : beg;
                }
                const int m = row ? rkey >> 8 : 0, mj = row ? (rkey & 0xff) - 1 : -1;
                const int h1f = row ? rhl : h1;
                if (g == 0) { t_hp16[end] = (uint16_t)h1f; t_ep16[end] = 0; }   // eh[end] = {h1f, 0}
                if (row) cells += (unsigned long long)(g == 0 ? end - beg : 0);
                const int j_exit = row ? end : beg;
                if (j_exit == qlen) {
                    max_ie = gscore > h1f ? max_ie : i;
                    gscore = gscore > h1f ? gscore : h1f;
                }
                // selects, not branches: mx, max_i, max_j and max_off stay in their registers.  m > mx >= 0 implies m != 0
                const bool better = m > mx;
                const int di = i - max_i, dj = mj - max_j;
                const int zpen = di > dj ? (di - dj) * e_del : (dj - di) * e_ins;
                bool fin = m == 0 || (!better && prm.zdrop > 0 && mx - m - zpen > prm.zdrop);
                {
                    int d = mj - i;
                    d = d < 0 ? -d : d;
                    d = max_off > d ? max_off : d;
                    max_off = better ? d : max_off;
                    max_i = better ? i : max_i;
                    max_j = better ? mj : max_j;
                    mx = better ? m : mx;
                }
                {                                                        // the next row's band; of no account when the task ends here
                    const int nbeg = first_nz < end ? first_nz : end;
                    int jj = last_nz >= nbeg ? last_nz : nbeg - 1;
                    jj = h1f != 0 ? end : jj;
                    if constexpr (EARLY != 0) {
                        // column beg of a row that starts at column 0 stores h1, the source of column 0's cell in the next row (next
                        // row's own first-column value is smaller)
                        int P = h1 + __mul24(qlen, prm.max_sc);
                        P = h1 > 0 ? P : 0;
                        P = P > rpot ? P : rpot;
                        const bool tail_known = end >= zr;                    // nothing alive to the right of this row's band
                        zr = tail_known ? jj : zr;
                        const bool ends = tail_known && P <= mx && P < gscore && (EARLY == 1 || (i & 3) == 3);
#ifdef BWAMS_BSWDBG
                        if (g == 0 && ends && !fin && i + 1 < tlen) ++n_rule;
#endif
                        fin = fin || ends;
                    }
#ifdef BWAMS_BSWDBG
                    if (g == 0) ++n_rows;
#endif
                    beg = nbeg;
                    end = jj + 2 < qlen ? jj + 2 : qlen;
                    ++i;
                    fin = fin || i >= tlen;
                }
                if (fin) {
                    if (g == 0) {
                        bwams_seqpair_t *o = &pairs[cur];
                        o->score = mx; o->qle = max_j + 1; o->tle = max_i + 1; o->gtle = max_ie + 1; o->gscore = gscore; o->max_off = max_off;
                    }
                    alive = false;
                }
                start_row = true;
            }
        }
        asm volatile("; BSW_PK_PASS_END");
#ifdef BWAMS_BSWDBG
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        t_pass += __builtin_amdgcn_s_memtime() - Tb;
        ++n_iter;
#endif
    }
#ifdef BWAMS_BSWDBG
    if (lane == 0) {
        unsigned long long *d = ctr->dbg + 40;
        atomicAdd(&d[0], __builtin_amdgcn_s_memtime() - T0); atomicAdd(&d[1], t_refill); atomicAdd(&d[2], t_pass);
        atomicAdd(&d[3], n_events); atomicAdd(&d[4], n_filled); atomicAdd(&d[5], n_iter); atomicAdd(&d[6], 1ull);
    }
    if (g == 0 && n_rows) { atomicAdd(&ctr->dbg[47], n_rows); atomicAdd(&ctr->dbg[48], n_rule); }     // rows walked, tasks the rule ended
#endif
    for (int o = 32; o > 0; o >>= 1) cells += ((unsigned long long)__shfl_down((unsigned)(cells >> 32), o) << 32) | (unsigned)__shfl_down((unsigned)cells, o);
    if (lane == 0 && cells) atomicAdd(&ctr->bsw_cells, cells);
}

__global__ void bsw_reset_kernel(DevCounters *ctr) {
    for (int i = 0; i < 4; ++i) ctr->bsw_head[i] = 0;      // bsw_cells accumulates until the caller clears it
    for (int i = 0; i < kNumBswClass; ++i) ctr->bsw_cls_cnt[i] = ctr->bsw_cls_head[i] = 0;
}

}  // namespace

// Tasks are binned (bsw_classify_kernel) by query length into five eight-tasks-per-wave launches and, for what is left
// (queries beyond 191 bases, scores beyond 2^14), the one-task-per-wave LDS kernel.  Every launch has its own ticket counter; with auxiliary
// streams they run concurrently, the classes of the longest queries first.  `list` holds kNumBswClass * n task indices.
int launch_bsw(bwams_seqpair_t *pairs, int64_t n, const uint8_t *ref, const uint8_t *qer, int w, const SwParams &prm, int qmax,
               DevCounters *ctr, int cu_count, hipStream_t st, int32_t *list, hipStream_t *aux, hipEvent_t fork, hipEvent_t *join,
               const int64_t *src, int dir, bool early) {
    bsw_reset_kernel<<<1, 1, 0, st>>>(ctr);
    if (n <= 0) return 0;
    bsw_classify_kernel<<<(unsigned)((n + 1023) / 1024), 1024, 0, st>>>(pairs, n, prm.max_sc, list, ctr->bsw_cls_cnt);
    int64_t blocks = (n + kWavesPerBlock - 1) / kWavesPerBlock;
    const int64_t maxb = (int64_t)cu_count * 8;
    if (blocks > maxb) blocks = maxb;
    hipStream_t q[5] = {st, st, st, st, st};
    const int n_aux = aux ? 4 : 0;
    if (n_aux) {
        if (hipEventRecord(fork, st) != hipSuccess) return -1;
        for (int c = 0; c < n_aux; ++c) {
            q[c + 1] = aux[c];
            if (hipStreamWaitEvent(q[c + 1], fork, 0) != hipSuccess) return -1;
        }
    }
    const unsigned B = (unsigned)blocks, T = kWavesPerBlock * 64;
    unsigned long long *cnt = ctr->bsw_cls_cnt, *hd = ctr->bsw_cls_head;
    // once per device: the attribute belongs to the device that is current (a batch on a second GPU of the process needs it too)
    auto pk_lds = [](int cols) { return (size_t)64 + (size_t)kPkWaves * 16 * ((size_t)(cols / 2) * 10 + 24); };
    {
        static std::mutex mu;
        static bool done[64] = {};
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return -1;
        std::lock_guard<std::mutex> g(mu);
        if (dev < 0 || dev >= 64 || !done[dev]) {
            if (hipFuncSetAttribute(reinterpret_cast<const void *>(bsw_qwin_kernel<kBswLpt, kBswWin>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)((size_t)kWavesPerBlock * (64 / kBswLpt) * 192 * 4)) != hipSuccess) return -1;
            if (hipFuncSetAttribute(reinterpret_cast<const void *>(bsw_pk_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pk_lds(192)) != hipSuccess) return -1;
            if (hipFuncSetAttribute(reinterpret_cast<const void *>(bsw_pk_kernel<kPkEarlyForm>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pk_lds(192)) != hipSuccess) return -1;
            if (dev >= 0 && dev < 64) done[dev] = true;
        }
    }
    // every class on a stream of its own, the classes of the longest queries first.  (With two classes per stream and the
    // one-task-per-wave kernel — usually without a single task, but 2048 blocks that wait for a free CU slot — in front of one
    // of them, the kernel trace showed two class launches starting 14 ms late.)
    const bool pk_env = knobs().bsw_pk != 0;       // A-B knob: the 32-bit eight-task kernel
    if (pk_env && bsw_pk_eligible(prm)) {
        static const int kCols[5] = {32, 64, 96, 144, 192};
        const unsigned Bp = (unsigned)((int64_t)B * kWavesPerBlock / kPkWaves);
        // the early exit rests on a positive best score per column; the 32-bit kernels below walk every row whatever the setting
        auto *const kern = early && prm.max_sc > 0 ? bsw_pk_kernel<kPkEarlyForm> : bsw_pk_kernel<0>;
        for (int c = 4; c >= 0; --c)
            kern<<<Bp, kPkWaves * 64, pk_lds(kCols[c]), q[c]>>>(pairs, list + (int64_t)c * n, cnt + c, ref, qer, w, prm, ctr, hd + c, kCols[c], src, dir);
    } else {
    bsw_qwin_kernel<kBswLpt, kBswWin><<<B, T, (size_t)kWavesPerBlock * (64 / kBswLpt) * 192 * 4, q[4]>>>(pairs, list + 4 * n, cnt + 4, ref, qer, w, prm, ctr, hd + 4, 192, src, dir);
    bsw_qwin_kernel<kBswLpt, kBswWin><<<B, T, (size_t)kWavesPerBlock * (64 / kBswLpt) * 144 * 4, q[3]>>>(pairs, list + 3 * n, cnt + 3, ref, qer, w, prm, ctr, hd + 3, 144, src, dir);
    bsw_qwin_kernel<kBswLpt, kBswWin><<<B, T, (size_t)kWavesPerBlock * (64 / kBswLpt) * 96 * 4, q[2]>>>(pairs, list + 2 * n, cnt + 2, ref, qer, w, prm, ctr, hd + 2, 96, src, dir);
    bsw_qwin_kernel<kBswLpt, kBswWin><<<B, T, (size_t)kWavesPerBlock * (64 / kBswLpt) * 64 * 4, q[1]>>>(pairs, list + 1 * n, cnt + 1, ref, qer, w, prm, ctr, hd + 1, 64, src, dir);
    bsw_qwin_kernel<kBswLpt, kBswWin><<<B, T, (size_t)kWavesPerBlock * (64 / kBswLpt) * 32 * 4, q[0]>>>(pairs, list + 0 * n, cnt + 0, ref, qer, w, prm, ctr, hd + 0, 32, src, dir);
    }
    {
        // what neither packed form can take: (h, e) row + query of one task per wave in LDS, fewer waves per block for very long queries.
        // Last on the main stream, persistent waves on a small grid: the class is usually empty.
        const int waves = bsw_lds_waves(qmax);
        if (waves < 1) return -2;                  // a query of more than 18196 bases does not fit a CU's LDS
        const size_t lds = bsw_row_bytes(qmax) * (size_t)waves;
        if (lds > 48 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(bsw_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        int64_t lblocks = (n + waves - 1) / waves;
        const int64_t lcap = qmax > 16 * kQuadCpl[4] - 1 ? maxb : (int64_t)cu_count * 2;     // long queries: this IS the main class
        if (lblocks > lcap) lblocks = lcap;
        bsw_kernel<<<(unsigned)lblocks, waves * 64, lds, q[0]>>>(pairs, n, ref, qer, w, prm, qmax, -1, ctr, &ctr->bsw_head[3], list + 5 * n, cnt + 5, src, dir);
    }
    if (n_aux)
        for (int c = 0; c < n_aux; ++c) {
            if (hipEventRecord(join[c], q[c + 1]) != hipSuccess) return -1;
            if (hipStreamWaitEvent(st, join[c], 0) != hipSuccess) return -1;
        }
    return 0;
}
size_t bsw_list_bytes(int64_t n) { return (size_t)kNumBswClass * (size_t)(n > 0 ? n : 1) * sizeof(int32_t); }

int bsw_lds_waves(int qmax) {
    const size_t waves = kBswLdsMax / bsw_row_bytes(qmax);
    return waves < (size_t)kWavesPerBlock ? (int)waves : kWavesPerBlock;
}

}  // namespace bwams
