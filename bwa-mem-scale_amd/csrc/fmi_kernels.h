// fmi_kernels.h — launch wrappers of the FM-index kernels (fmi_seed.hip, fmi_sal.hip).
#pragma once
#include "common.h"

namespace bwams {

struct SeedLaunch {
    DevFmi fmi;
    const uint8_t *enc;
    const int64_t *cum;
    const uint8_t *skip;          // may be nullptr
    const uint32_t *packed;       // reads packed by launch_pack_reads: read_w words per read
    int read_w, read_cw;          // words per read (multiple of 4) / code words
    int reads_in_lds;             // 1: each lane keeps its current read in LDS
    int debug;                    // diagnostic ablations (env BWAMS_DEBUG); 0 in production
    int64_t nseq;
    int min_seed_len;
    bwams_smem_t *pool;
    int64_t pool_cap;
    DevCounters *ctr;
    uint4 *prev;                  // per-lane previous-interval lists: prev_cap entries x 16 B, lane-contiguous
    int prev_cap;                 // entries per lane
    int64_t prev_threads;         // lanes the scratch was sized for
    // backward phases whose interval list has at least bwd_min_list entries go to smem_bwd_wave_kernel (0 = never)
    BwdItem *bwd_items, *bwd_items_s;   // lists beyond / up to kBwdShortMax entries; bwd_items_cap slots each
    uint4 *bwd_ent;
    int64_t bwd_items_cap, bwd_ent_cap;
    int bwd_min_list;
    int bwd_dry_min_list, bwd_dry_cols, bwd_dry_late_list;   // the same three thresholds once the work queue has run dry
    int bwd_cols, bwd_late_list;  // ... or, later: after bwd_cols columns with bwd_late_list entries still alive
};

// grid sizing shared by batch_create (scratch) and the launches
int seed_block_threads();
int64_t seed_max_threads(int cu_count);
int64_t seed_pool_slack(int cu_count);   // pool slots the launches of one seeding pass can leave unused in partly filled chunks

// enc_qdb bytes -> 2-bit codes + N mask, W words per read
void launch_pack_reads(const uint8_t *enc, const int64_t *cum, int64_t nseq, int W, int cw, uint32_t *packed,
                       hipStream_t st);
// between rounds: snapshot counters (which = 1, 2, 3 after that round; 0 = start) and reset the work cursor
void launch_mark(DevCounters *ctr, int which, hipStream_t st);
// round 1: every pivot of every read (getSMEMsAllPosOneThread)
void launch_smem_round1(const SeedLaunch &a, int cu_count, hipStream_t st);
// round 2: build the work list from round-1 SMEMs, then one pivot per item (getSMEMsOnePosOneThread)
void launch_round2_work(const SeedLaunch &a, Round2Work *work, int64_t work_cap, int split_len,
                        int split_width, int cu_count, hipStream_t st);
void launch_smem_round2(const SeedLaunch &a, const Round2Work *work, int cu_count, hipStream_t st);
// the backward phases rounds 1 / 2 set aside (lists of bwd_min_list entries and more): one wavefront per pivot, one lane per entry
void launch_smem_bwd_wave(const SeedLaunch &a, int cu_count, hipStream_t st);
// round 3: forward-only seeds (bwtSeedStrategyAllPosOneThread)
void launch_smem_round3(const SeedLaunch &a, int max_intv, int cu_count, hipStream_t st);

// FMA table builders (__build_all_smem_table / __build_last_smem_table): one lane per table entry
void launch_build_fma(const DevFmi &f, int all_bp, uint32_t *all_tab, int last_bp, uint4 *last_tab, hipStream_t st);

// sort keys / gather / SA lookup
// key = rid << 2 * pos_bits | m << pos_bits | n, holes with rid = hole_key_rid; pos_bits = 8 or 16 must hold every m and n
void launch_make_keys(const bwams_smem_t *pool, int64_t n, uint64_t *keys, uint32_t *vals, uint32_t hole_key_rid,
                      int pos_bits, hipStream_t st);
void launch_gather_sorted(const bwams_smem_t *pool, const uint32_t *order, int64_t n, bwams_smem_t *sorted,
                          int64_t *sa_cnt, int max_occ, hipStream_t st);
// dense / stride: the index's dense suffix-array table and its stride (1, 2 or 4), or nullptr: every row walks to a sample of the index
void launch_sa_lookup(const DevFmi &f, const bwams_smem_t *sorted, int64_t n_smem, const int64_t *sa_off,
                      int64_t *coord, int64_t coord_cap, int max_occ, DevCounters *ctr, int cu_count,
                      hipStream_t st, const uint64_t *dense = nullptr, int stride = 0);

// The dense suffix-array table of an index (fmi_sal.hip): one 8-byte entry for every row r with r % stride == 0, holding exactly
// what the reference's walk from r produces: bits 0-39 the coordinate (the sample plus the walk's own steps), bit 40 "the walk met
// the sentinel row" (the lookup then yields 0, FMI_search.cpp:2234-2237), bits 41-63 the LF steps the walk took.
constexpr int kSaDenseCoordBits = 40, kSaDenseStepBits = 23;
constexpr uint64_t kSaDenseSentinel = 1ull << kSaDenseCoordBits;
inline int64_t sa_dense_entries(int64_t rows, int stride) { return (rows + stride - 1) / stride; }
// entries [0, n) of the table; *bad (zeroed by the caller) becomes nonzero when a walk's step count does not fit its field
void launch_sa_dense_build(const DevFmi &f, int stride, int64_t n, uint64_t *table, unsigned long long *bad, int cu_count, hipStream_t st);

#ifdef __HIPCC__
// LF-mapping from row sp until a row that is a multiple of S (a power of two), as get_sa_entries_prefetch walks to its samples with
// S = 8: the row reached, the steps taken, and whether the walk stopped at the sentinel row instead (the step that meets it is not counted).
struct SaWalk {
    int64_t sp;
    uint32_t steps;
    bool sentinel;
};
template <int S> __device__ __forceinline__ SaWalk sa_walk(const DevFmi &f, int64_t sp) {
    auto mk64 = [](uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); };
    SaWalk w{sp, 0, false};
    while ((w.sp & (S - 1)) != 0) {
        const uint4 *p = f.cp + ((w.sp >> 6) << 2);
        // the whole block in one round trip: the count of the row's base would otherwise be a second, dependent load
        const uint4 c01 = p[0], c23 = p[1], h01 = p[2], h23 = p[3];
        const int sh = 63 - (int)(w.sp & 63);
        const uint64_t h0 = mk64(h01.x, h01.y), h1 = mk64(h01.z, h01.w);
        const uint64_t h2 = mk64(h23.x, h23.y), h3 = mk64(h23.z, h23.w);
        int b = 4;
        uint64_t hb = 0;
        if ((h0 >> sh) & 1) { b = 0; hb = h0; }
        else if ((h1 >> sh) & 1) { b = 1; hb = h1; }
        else if ((h2 >> sh) & 1) { b = 2; hb = h2; }
        else if ((h3 >> sh) & 1) { b = 3; hb = h3; }
        if (b == 4) { w.sentinel = true; break; }
        const int y = (int)(w.sp & 63);
        const uint64_t mask = y ? (~0ull << (64 - y)) : 0ull;
        const int64_t cnt = (int64_t)(b == 0 ? mk64(c01.x, c01.y) : b == 1 ? mk64(c01.z, c01.w) : b == 2 ? mk64(c23.x, c23.y) : mk64(c23.z, c23.w));
        w.sp = (b == 0 ? f.count[0] : b == 1 ? f.count[1] : b == 2 ? f.count[2] : f.count[3]) + cnt + __popcll(hb & mask);
        w.steps++;
    }
    return w;
}
// the index's 1/8 sample at row sp (a multiple of 8): int8 high byte + uint32 low word
__device__ __forceinline__ int64_t sa_sample(const DevFmi &f, int64_t sp) {
    return ((int64_t)f.sa_ms[sp >> 3] << 32) + (int64_t)f.sa_ls[sp >> 3];
}
#endif

// the search kernels' table: the interleaved form of CP_OCC (piece b of a block = count and string of base b), n_blk blocks of 64 B
size_t cp2_bytes(int64_t n_blk);
void launch_cp2_build(const uint4 *cp, int64_t n_blk, uint4 *cp2, hipStream_t st);

}  // namespace bwams
