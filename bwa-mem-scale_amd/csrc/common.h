// common.h — internal declarations shared by the HIP translation units.
#pragma once

#include <atomic>
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <mutex>
#include <shared_mutex>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/bwams.h"
#include "stage_valid.h"

namespace bwams {

void set_last_error(const std::string &s);

// Every device allocation of the library goes through this: BWAMS_POISON=1 (debugging aid) fills the fresh block with 0xAB bytes and waits
// for the fill, so that a kernel that reads what nothing wrote misbehaves in every run — not only when the allocator hands back a block that
// another chunk left dirty (a fresh process gets zeros).  tests: the whole `-m gpu` suite passes under it.
// Debugging aids and A-B switches, all of them result-neutral: read from the environment ONCE (at the first call into the library; again
// on bwams_debug_reload(), which the tests call after changing a variable) — never per call on the hot host path.  include/bwams.h lists them.
constexpr int kSaDenseDefault = 1;       // profiles/sa_dense.md: the stride table
struct Knobs {
    int verbose = 0;              // BWAMS_VERBOSE: stage times and counters per run on stderr
    int debug = 0;                 // BWAMS_DEBUG: diagnostic ablations of the SMEM search (bit 0: no SMEM is written)
    int poison = 0;                // BWAMS_POISON: fresh device allocations are filled with 0xAB
    int bwd_min_list = 40, bwd_cols = 24, bwd_late_list = 8;                     // BWAMS_BWD_MIN_LIST / _COLS / _LATE_LIST   (fmi_seed.hip: bwd_hand_over)
    int bwd_dry_min_list = 24, bwd_dry_cols = 8, bwd_dry_late_list = 12;         // BWAMS_BWD_DRY_*: the same once the work queue is dry
    int r3_beside = 1;             // BWAMS_SEED_R3_BESIDE: 1 (default) = SMEM round 3 beside round 2 on a stream of its own; 0 = behind it
    int ext_max_rounds = 0;        // BWAMS_EXT_MAX_ROUNDS: cap of the extension rounds (tests force the extend-the-rest fallback)
    int ext_all_rounds = 0;        // BWAMS_EXT_ALL_ROUNDS: never cut the rounds short
    int ext_inplace = 1;           // BWAMS_EXT_INPLACE=0: extension tasks copied into flat buffers
    int dedup_seq = 0;             // BWAMS_DEDUP_SEQ=1: every read through de-duplication's one-lane form
    int dedup_count = 0;           // BWAMS_DEDUP_COUNT=1: de-duplication counts its reads per tier and its patch alignments per variant (tests)
    int pair_count = 0;            // BWAMS_PAIR_COUNT=1: the pairing stage counts its reads per route and its sorts per path (tests)
    int pair_drop_plan = 0;        // BWAMS_PAIR_DROP_PLAN: exercise mate rescue's second pass
    int trace_pair = 0;            // BWAMS_TRACE_PAIR: a synchronisation and a line per launch of the paired-end tail
    int bsw_pk = 1;                // BWAMS_BSW_PK=0: the 32-bit eight-task banded-SW kernel
    int bsw_early = -1;            // BWAMS_BSW_EARLY: the packed kernel's early exit.  Unset: on in bwams_extend_run, off in bwams_bsw_run (whose
                                   // bsw_cells the tests pin to the cells of the full walk); 0: off in both; 1: on in both
    int chain_count = 0;           // BWAMS_CHAIN_COUNT=1: chaining counts its filter routes and the passes of chain_seeds_batch (tests)
    int chain_batch = 1;           // BWAMS_CHAIN_BATCH=0: chaining's wave tier takes one seed at a time (chain_dev.h: chain_seeds_batch)
    int ert_fat = 1;               // BWAMS_ERT_FAT=0: the ERT walk reads the reference's two tables only (no entry + tree-head table)
    int depth_combine = 1;         // BWAMS_DEPTH_COMBINE=0: the depth add issues one atomic per lane (no folding of equal slots inside a wave)
    int pileup_tiled = 1;          // BWAMS_PILEUP_TILED=0: every record of a pileup add goes through the direct kernel (one global atomic per base)
    int qc_lanes = 1;              // BWAMS_QC_LANES=0: the QC add's per-cycle tables come from the plain kernel (one global atomic per base and per quality)
    int recal_lds = 1;             // BWAMS_RECAL_LDS=0: the recalibration add counts through the plain kernel (one global atomic per update)
    int ert_grid = -1, ert_ticket = 1;   // BWAMS_ERT_GRID (blocks per CU, 0 = one block per 256 bases) / BWAMS_ERT_TICKET=0 (round robin)
    int sa_dense = kSaDenseDefault;      // BWAMS_SA_DENSE: stride of an index's dense suffix-array table, 1 / 2 / 4; 0 = never built, never read
    int64_t sa_dense_max_bytes = 0;      // BWAMS_SA_DENSE_MAX_BYTES: a table above it is not built (0: no cap)
    int sort_narrow = 1;                 // BWAMS_SORT_NARROW=0: the SMEM sort keys keep 16-bit position fields whatever the longest read
};
const Knobs &knobs();
void knobs_reload();

// The dense suffix-array tables are a cache that gives way (api_index.hip): every table of an index on `device` is released, for
// good; returns how many were.  dev_malloc calls it when the device is out of memory; bwams_debug_sa_dense_release is the same call.
int sa_dense_release(int device);

// may_yield = false: the dense table's own allocation, which must not release the tables to make room for itself
template <class T> static inline hipError_t dev_malloc(T **p, size_t bytes, bool may_yield = true) {
    const bool poison = knobs().poison != 0;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(p), bytes);
    if (e == hipErrorOutOfMemory && may_yield) {
        int dev = 0;
        (void)hipGetLastError();
        if (hipGetDevice(&dev) == hipSuccess && sa_dense_release(dev) > 0) e = hipMalloc(reinterpret_cast<void **>(p), bytes);
    }
    if (e == hipSuccess && poison && bytes) {
        e = hipMemset(*p, 0xAB, bytes);
        if (e == hipSuccess) e = hipDeviceSynchronize();     // hipMemset on the null stream does not order with non-blocking streams
    }
    return e;
}

// The one owner of a block of device memory (through dev_malloc) or, Host = true, of pinned host memory: move-only, freed by its
// destructor.  alloc() frees and allocates exactly `bytes`; ensure() reallocates only to grow, to `new_cap` bytes or by default to
// `bytes + bytes/8 + 4096`; cap is in bytes.  Growing does not synchronise: a caller whose stream may still read the old block does.
template <class T = void, bool Host = false> struct Buf {
    T *p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(Buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~Buf() { release(); }
    template <class U> U *as() const { return reinterpret_cast<U *>(p); }
    void release() {
        if (p) (void)(Host ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    hipError_t alloc(size_t bytes, bool may_yield = true) {
        release();
        hipError_t e = Host ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : dev_malloc(&p, bytes, may_yield);
        cap = p ? bytes : 0;
        return e;
    }
    hipError_t ensure(size_t bytes, size_t new_cap) { return bytes <= cap ? hipSuccess : alloc(new_cap); }
    hipError_t ensure(size_t bytes) { return ensure(bytes, bytes + bytes / 8 + 4096); }
    hipError_t ensure_n(size_t n) { return ensure(n * sizeof(T)); }     // n elements (a typed buffer): the same call, the same growth
};
template <class T = void> using DevBuf = Buf<T, false>;
template <class T = void> using HostBuf = Buf<T, true>;

#define BWAMS_HIP(call)                                                                  \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess) {                                                          \
            char buf_[512];                                                              \
            snprintf(buf_, sizeof buf_, "%s:%d: %s -> %s", __FILE__, __LINE__, #call,    \
                     hipGetErrorString(e_));                                             \
            bwams::set_last_error(buf_);                                                 \
            return (e_ == hipErrorOutOfMemory) ? BWAMS_ERR_NOMEM : BWAMS_ERR_DEVICE;     \
        }                                                                                \
    } while (0)

// FM-index as the kernels see it (passed by value in the kernarg segment).
// cp points at the reference's CP_OCC array unchanged: block b occupies four
// 16-byte pieces  [cnt0 cnt1] [cnt2 cnt3] [hot0 hot1] [hot2 hot3].
struct DevFmi {
    const uint4 *cp;
    const uint4 *cp2;          // the search kernels' interleaved form of cp (fmi_seed.hip: piece b = count and string of base b), built at the first seeding
    const int8_t *sa_ms;
    const uint32_t *sa_ls;
    const uint8_t *ref;        // .0123 or nullptr
    // FMA direct-lookup tables (reference layouts, src/FMI_search.h:101-135) or nullptr
    const uint32_t *all_smem;  // 4^all_bp entries x 32 words: last_avail, 10 x {k32, l32, s32}, pad
    const uint4 *last_smem;    // 4^last_bp entries x 16 B: bp | kms<<8 | lms<<16 | sms<<24, kls, lls, sls
    int32_t all_bp, last_bp;
    int64_t count[5];
    int64_t sentinel;
    int64_t ref_seq_len;
};

// EMF table as the probe kernel sees it
struct DevEmf {
    const uint4 *seed_table;     // {flags, location, left, right}
    const uint32_t *loc_table;
    const uint8_t *ref;          // .0123
    uint32_t num_seed_entry, num_loc_entry, seq_len;
    int32_t seed_len;
};

// ERT index as the kernels see it: the reference's two files, resident (src/ertindex.cpp writes them)
struct DevErt {
    const uint64_t *kmer;      // <prefix>.kmer_table: 4^K entries
    const uint8_t *mlt;        // <prefix>.mlt_table, padded by 16 bytes
    const uint8_t *ref;        // .0123, both strands
    int64_t ref_len;           // 2 * l_pac
    int32_t K, X, read_len;    // kmerSize, xmerSize, READ_LEN of the build (src/macro.h:204-206, :66)
    uint64_t *cnt_tab;         // hit counts of the subtrees with 20 hits or more: {node address + 1, hits} pairs, open addressing
    int32_t cnt_bits;          // log2 of the number of pairs
    const uint8_t *fat;        // resident, derived once per index (ert_seed.hip: ert_fat_kernel), or null: 64 B per k-mer = its table entry + the
                               // first 56 bytes of its tree, so that a walk's entry and first records are ONE line
};

// device-side counters of one seed run
struct DevCounters {
    unsigned long long n_ext, n_ext_blocks, n_sa_lookups, n_lf_steps;
    unsigned long long n_smem_total;     // append cursor of the SMEM pool (slots handed out, holes included)
    unsigned long long n_smem_valid;     // real SMEMs written
    unsigned long long valid_after[3];   // n_smem_valid when round 1, 2, 3 ended
    unsigned long long n_after_r1, n_after_r2;
    unsigned long long work_head;        // dynamic work queue cursor (reset per kernel)
    unsigned long long n_work2;          // round-2 work items
    unsigned long long overflow;         // SMEM pool overflow flag / needed size
    unsigned long long bsw_cells;
    unsigned long long bsw_head[4];      // ticket counters of the one-task-per-wave banded-SW kernels
    unsigned long long bsw_cls_cnt[6], bsw_cls_head[6];   // banded SW: tasks per query-length class, ticket counters of the class launches
    unsigned long long ext_after[3], blk_after[3];
    unsigned long long emf_nodes, emf_cmp_bytes;     // EMF probe: entries visited, reference bytes compared   // n_ext / n_ext_blocks when round 1, 2, 3 ended
    unsigned long long chain_overflow;   // chaining: B-tree node region exhausted (never expected)
    unsigned long long chain_longread;   // chaining: reads long enough for mem_flt_chained_seeds to re-score seeds
    unsigned long long n_heavy;          // chaining: reads handed to the wave-per-read filter kernel
    unsigned long long chain_class[10];  // chaining: reads with more seeds than the L, L1, M, M1, S, lane-tier, XL, L2, M2 and XL2 limits
    unsigned long long chain_ticket[10]; // chaining: work cursors of the wave kernels
    unsigned long long heavy_tickets[6]; // chaining: work cursors of chain_heavy_kernel's size classes (five used)
    unsigned long long sel_heavy;        // extension: reads of the selection's wave tier
    // extension, the counters of ONE round (bwams_extend_run clears the block with one memset before whoever requests — the plan,
    // then each selection — and copies its first three words back in one copy):
    unsigned long long ext_n_req;        // slots appended to the request list (its cursor)
    unsigned long long ext_n_rest;       // slots behind the requests of the last selection (an upper bound of the undecided seeds)
    unsigned long long ext_n_tasks;      // tasks of the requested slots: left in the low, right in the high 32 bits
    unsigned long long ext_head[2];      // task indices handed out by the build (left, right)
    unsigned long long ext_sel_ticket[3];   // work cursors of the selection's wave tier: the small class, the big class' two passes
    unsigned long long ext_n_retry[2];   // tasks queued for the next band width (left, right)
    unsigned long long dedup_heavy, dedup_ticket, dedup_light;   // dedup: reads for the wave tier, its work cursor, reads for the lane tier
    unsigned long long chain_redo, chain_redo_ticket;   // chaining: reads the ordered-array attempt gave up on, work cursor
    unsigned long long pair_heavy, pair_ticket;   // mem_mark_primary_se: reads of the wave tier, its work cursor
    unsigned long long dbg[80];          // diagnostics printed under BWAMS_VERBOSE (chain_heavy_kernel: size histogram, cycles)
    unsigned long long pair_ticket2;     // mem_mark_primary_se: work cursor of the wave tier's small-LDS instance
    unsigned long long dedup_ticket2, dedup_ticket3;    // dedup: work cursors of the wave tier's smaller instances
    unsigned long long ert_kmer, ert_nodes, ert_ref;   // ERT profile kernel: k-mer entries read, tree records decoded, text bytes compared
    unsigned long long work_head3, n_ext3, n_blk3, n_smem3;   // SMEM round 3 (it may run beside round 2): its own cursor and counts, folded in by mark_kernel(3)
    unsigned long long ert_ticket;       // ERT walk: work cursor of ert_profile_kernel (groups of 64 read positions)
    unsigned long long bwd_items, bwd_entries, bwd_ticket;   // SMEM search: backward phases handed to the wave kernel, their list entries, its work cursor
    unsigned long long bwd_items_s, bwd_ticket_s;            // ... the short lists (smem_bwd_group_kernel): slots handed out, work cursor
    unsigned long long pair_full, pair_fail;   // mate rescue: reads redone with every orientation planned; reads the second pass could not finish (never expected)
    unsigned long long chain_lane_giveup;      // chaining: lane-tier reads that outgrew the leaf form and were chained again through the B-tree in HBM
};

struct StageState;                       // a batch's state behind seeding, stage by stage (stage_state.h)
void stage_state_free(StageState *s);

// bam.hip: a batch's SAM text as BAM records.  Record r is the line that ends at line_end[r]; the counting pass writes size[r]
// (block_size + 4) and, for a line BAM cannot hold, bad[0] = min(read << 8 | reason); the writing pass fills out from rec_off
// (the exclusive scan of size, n_rec + 1 entries) and bam_off[nseq + 1], where each read's records start.
struct BamArgs {
    const char *text;
    const int64_t *line_end, *read_off;
    int64_t n_rec, nseq;
    const char *ctg_names;
    const int32_t *ctg_off, *ctg_sorted;
    int32_t n_ctg;
    int64_t *size;
    const int64_t *rec_off;
    uint8_t *out;
    unsigned long long *bad;
};
void launch_bam_count(const BamArgs &A, int cu_count, hipStream_t st);
void launch_bam_write(const BamArgs &A, int64_t *bam_off, int cu_count, hipStream_t st);

// bam_sort.hip: coordinate sort of n_rec records at bam + rec_off[r] (the buffer holds 16 bytes of slack past the last record).
// keys: coord[r] (the published order) and dkey[r] (refID -1 as n_ref: bam_sort_bits(n_ref) significant bits), idx[r] = r; then,
// after the radix sort of (dkey, idx), permute: coord_out[i] = coord[idx[i]], size[i] its size (scan it into new_off[n_rec + 1]);
// gather: the record idx[i] to dst + new_off[i].
int bam_sort_bits(uint32_t n_ref);
void launch_bam_sort_keys(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, uint32_t n_ref, bwams_bam_coord_t *coord,
                          uint64_t *dkey, uint32_t *idx, int cu_count, hipStream_t st);
void launch_bam_sort_permute(const bwams_bam_coord_t *coord, const uint32_t *idx, int64_t n_rec, bwams_bam_coord_t *coord_out,
                             int64_t *size, int cu_count, hipStream_t st);
void launch_bam_sort_gather(const uint8_t *src, const int64_t *rec_off, const uint32_t *idx, const int64_t *new_off, int64_t n_rec,
                            uint8_t *dst, int cu_count, hipStream_t st);

// bam_query.hip: one piece of a BAM file read by region (rules in include/bwams.h above bwams_bam_file_open).  d[0, n) holds whole
// inflated members behind the carried bytes (16-byte aligned, 64 bytes of slack behind n); the record chain starts at `start` and
// takes the records that begin below `stop`.  regions: rule 2's merged regions on the device, n_regions 0 keeps every record.  The
// kept records go back to back into recs (with the 16 bytes of slack consumer_records documents), their offsets into roff
// (n_kept + 1) and their coords into coords.  All on st, which is drained.
struct BamQueryScratch;                  // the discovery's and the selection's device buffers
BamQueryScratch *bam_query_scratch_new();
void bam_query_scratch_free(BamQueryScratch *s);
struct BamQueryResult {
    int64_t n_rec, n_kept, kept_bytes, n_cand;
    int64_t at;                          // behind the chain's last record
    bool cut, bad;                       // at `at`: a record the end of the buffer cuts off / nothing well formed
    int64_t cut_size;                    // the cut-off record's size when its block_size is there, else 0
    int64_t bad_rec;                     // the first record with refID < -1 or POS outside [-1, 2^31 - 2], or -1
    int64_t bad_rec_at;
    float ms_discover, ms_select, ms_gather;
};
int bam_query_piece(BamQueryScratch *s, const uint8_t *d, int64_t n, int64_t start, int64_t stop, const bwams_pileup_region_t *regions,
                    int32_t n_regions, DevBuf<uint8_t> &recs, DevBuf<int64_t> &roff, DevBuf<bwams_bam_coord_t> &coords, hipEvent_t ev[4],
                    int cu_count, hipStream_t st, BamQueryResult *out);

// bam_merge.hip: one round of several BAM files merged (rules M4 to M8 in include/bwams.h above bwams_bam_file_open_merge).  A child
// is described by where its handle left its current piece; the plan is what the frontier kernel decides and the host reads once a
// round.  check: plan->bad[j] = min(it, the ordinal of a record of child j's new piece whose key is below its predecessor's), and
// last_key[2j + parity] = the piece's last key (two words per child; all zero when a query begins).  frontier: count, base, total.
// rank: for each of the `total` emitted records, at its place in the piece, its source address, size and coord; size[total] = 0.
// bm_scan: the sizes' exclusive scan (total + 1 entries).  gather: the records into dst, which holds 16 bytes of slack as every source does.
constexpr int kBmMaxFiles = 64;          // a lane of the frontier kernel's one wave per file
struct BmChild {
    const bwams_bam_coord_t *coords;     // of its current piece, as are recs and roff
    const uint8_t *recs;
    const int64_t *roff;
    int64_t cur, n;                      // the window: records [cur, n)
    int64_t seen;                        // the ordinal of the piece's record 0 among the child's records of this query
    int32_t open, refilled;              // pieces to come; the piece is new in this round
    int32_t parity, pad_;                // the word of last_key that this piece writes
};
struct BmPlan {
    int64_t count[kBmMaxFiles], base[kBmMaxFiles], total;
    uint64_t frontier;
    int32_t i_star, any_open;
    unsigned long long bad[kBmMaxFiles];
};
void launch_bm_check(const BmChild *kids, int n_kids, int64_t max_n, uint64_t *last_key, BmPlan *plan, int cu_count, hipStream_t st);
void launch_bm_frontier(const BmChild *kids, int n_kids, BmPlan *plan, hipStream_t st);
void launch_bm_rank(const BmChild *kids, int n_kids, const BmPlan *plan, int64_t total, const uint8_t **src, int64_t *size,
                    bwams_bam_coord_t *coords, hipStream_t st);
hipError_t bm_scan(void *tmp, size_t &tmp_bytes, const int64_t *size, int64_t *roff, int64_t n1, hipStream_t st);
void launch_bm_gather(const uint8_t *const *src, const int64_t *roff, int64_t n, uint8_t *dst, int cu_count, hipStream_t st);

// markdup.hip: duplicate marking (rules in include/bwams.h above bwams_bam_templates).  md_templates groups n_rec records (at
// bam + rec_off[r], 16 bytes of slack past the last) into templates: m.n_t templates, m.rtmpl[r] each record's, and the m.n_e ends
// of the templates that have one, in template order, at m.ends; BWAMS_ERR_UNSUPPORTED (last error: the first record concerned) for
// rules 2-3.  md_decide: rule 6 over device ends[0, n_e) into device dup[0, n_t) (zeroed first); counts = pairs, pair duplicates,
// fragment duplicates.  launch_md_apply: FLAG 0x400 of the record at rec_off[i] from dup[rtmpl[perm ? perm[i] : i]] (*n_marked counts
// the records set).  launch_md_gather32 / _gather64: dst[i] = src[idx[i]].
struct MdRec {                           // one record as the template kernel reads it
    int64_t c;                           // unclipped 5' coordinate of a mapped primary (rule 3), else 0
    int32_t rid;
    uint16_t flag, score;                // score: rule 4's, of a mapped primary
};
struct MdTemplates {
    DevBuf<> head, tid, rtmpl, tstart, rec, tend, has, ends, info, tmp;
    DevBuf<> tloc, locs;                 // md_locs: bwams_dup_loc_t per template, and per end (parallel to ends)
    int64_t n_t = 0, n_e = 0;
};
struct MdDecide {
    DevBuf<> k1, k2, ka, kb, i1, i2, info, tmp;
    DevBuf<> e2, opt;                    // the ends with their libraries folded into the refIDs; optical clustering's slot arrays
};
// The groups table on the device (rule 9): the read groups' IDs sorted by bytes, ids[id_off[k], id_off[k + 1]) the k-th of them and
// id_ord[k] its ordinal; rg_lib by ordinal.  walk = 0: no table, no aux walk, every template read group -1 of library n_lib - 1 = 0.
struct MdGroupsDev {
    const uint8_t *ids;
    const int64_t *id_off;
    const int32_t *id_ord, *rg_lib;
    int32_t n_rg, n_lib, walk;
};
// What md_decide does beyond rule 6 when given: loc per end (device; null: one library, no location), d > 0 and optical (device,
// n_t bytes, zeroed by the caller) for rule 12, lib_counts (device, n_lib * 7 words, zeroed by the caller: unpaired and pairs
// examined, unpaired, pair and optical duplicates, then md_lib_recs' two) for rule 13.
struct MdDecideMore {
    const bwams_dup_loc_t *loc;
    int32_t n_lib;
    int64_t d, max_set;
    uint8_t *optical;
    unsigned long long *lib_counts;
};
int md_templates(MdTemplates &m, const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, int cu_count, hipStream_t st);
int md_locs(MdTemplates &m, const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const MdGroupsDev &G, int cu_count, hipStream_t st);
void launch_md_lib_recs(const MdTemplates &m, int64_t n_rec, const bwams_dup_loc_t *tloc, int n_lib, unsigned long long *counts,
                        int cu_count, hipStream_t st);
int md_decide(MdDecide &w, const bwams_dup_end_t *ends, int64_t n_e, int64_t n_t, uint8_t *dup, int64_t counts[3], int cu_count,
              hipStream_t st, const MdDecideMore *more = nullptr);
void launch_md_apply(uint8_t *bam, const int64_t *rec_off, const uint32_t *perm, const uint32_t *rtmpl, const uint8_t *dup, int64_t n_rec,
                     unsigned long long *n_marked, int cu_count, hipStream_t st);
void launch_md_gather32(const uint32_t *src, const uint32_t *idx, int64_t n, uint32_t *dst, int cu_count, hipStream_t st);
void launch_md_gather64(const uint64_t *src, const uint32_t *idx, int64_t n, uint64_t *dst, int cu_count, hipStream_t st);
const char *md_reason_text(int reason);  // the text of refusal reason 0-3 (rules 2-3) or 4 (rule 9's aux walk)

// dup_join.hip: templates joined by read name (rules J1-J9 in include/bwams.h above bwams_dupjoin_open).  One entry per added record,
// as arrays indexed by the record's ordinal: J1's key, L, the MdRec, and rules 9-10 of the record itself.
struct DjEntries {
    DevBuf<uint64_t> k0, k1;
    DevBuf<uint8_t> len;
    DevBuf<MdRec> rec;
    DevBuf<bwams_dup_loc_t> loc;
};
constexpr int64_t kDjEntryBytes = 8 + 8 + 1 + (int64_t)sizeof(MdRec) + (int64_t)sizeof(bwams_dup_loc_t);      // 57 per record
struct DjScratch {                       // of dj_join: freed with the entries
    DevBuf<uint64_t> ka, kb;
    DevBuf<uint32_t> i1, i2, first, tid, tstart;
    DevBuf<uint8_t> head, has;
    DevBuf<bwams_dup_end_t> tend;
    DevBuf<unsigned long long> info;
    DevBuf<> tmp;
    void release() { ka.release(); kb.release(); i1.release(); i2.release(); first.release(); tid.release(); tstart.release();
                     head.release(); has.release(); tend.release(); info.release(); tmp.release(); }
};
struct DjJoined {                        // what dj_join leaves: each record's template, the ends and their locs, each template's loc
    DevBuf<uint32_t> rec_tmpl;
    DevBuf<bwams_dup_end_t> ends;
    DevBuf<bwams_dup_loc_t> locs, tloc;
    int64_t n_t = 0, n_e = 0;
};
// The entries of the n records at bam + rec_off[r] into E's arrays from `base` on (room for base + n is the caller's).  call[0] +=
// the sum of their k0 mod 2^64, call[1] += the sum of (2r + 1) * k0, call[2] = min(call[2], the ordinal of a record whose aux
// fields do not chain) when G.walk.
void launch_dj_entries(const uint8_t *bam, const int64_t *rec_off, int64_t n, int64_t base, const MdGroupsDev &G, DjEntries &E,
                       unsigned long long *call, int cu_count, hipStream_t st);
// J8's check: sum[0] and sum[1] += the two sums of k0 over the n records
void launch_dj_key_sum(const uint8_t *bam, const int64_t *rec_off, int64_t n, unsigned long long *sum, int cu_count, hipStream_t st);
// J2-J4 over entries [0, n): the sorts, the template ordinals, the walks and the ends.  BWAMS_ERR_UNSUPPORTED with `who`, the first
// record concerned and the reason in the last error for rules 2-3.  ms: host-clock milliseconds of the sorts and of the rest.
int dj_join(const DjEntries &E, int64_t n, DjScratch &S, DjJoined &J, const char *who, float ms[2], int cu_count, hipStream_t st);
// rule 13's two record-level counts into counts[lib * 7 + 5 .. 6] and *n_marked += the records whose template is a duplicate
void launch_dj_counts(const MdRec *rec, const uint32_t *rec_tmpl, const bwams_dup_loc_t *tloc, const uint8_t *dup, int64_t n, int n_lib,
                      unsigned long long *counts, unsigned long long *n_marked, int cu_count, hipStream_t st);

// collate.hip: a coordinate-sorted BAM collated by read name (rules C1-C8 in include/bwams.h above bwams_collate_open).  An entry per
// record that waits for its mate, as arrays in ordinal order: the masked key, where the record lies (the pool, or the piece during
// an add), its ordinal, its size and its segment (2 first, 3 last).
struct CoEntries {
    DevBuf<uint64_t> key;
    DevBuf<const uint8_t *> ptr;
    DevBuf<int64_t> ord;
    DevBuf<int32_t> size;
    DevBuf<uint8_t> seg;
};
constexpr int64_t kCoEntryBytes = 8 + 8 + 8 + 4 + 1;       // 29 per waiting record
struct CoEntryArrays {                   // the same, as the kernels take it
    uint64_t *key;
    const uint8_t **ptr;
    int64_t *ord;
    int32_t *size;
    uint8_t *seg;
};
struct CoPlace {                         // what the scans add up: bytes and records
    int64_t bytes, n;
};
// the call words of an add: the first-bad word (ordinal << 3 | reason), the longest run, the pool bytes that died, co_totals' eight
enum { kCoCallBad = 0, kCoCallMaxRun, kCoCallDied, kCoCallWaitBytes, kCoCallWaitN, kCoCallOldBytes, kCoCallOldN, kCoCallPairBytes,
       kCoCallPairN, kCoCallSingleBytes, kCoCallSingleN, kCoCallWords };
enum { kCoReasonBits = 0, kCoReasonSegment = 1 };
// entry: cls[r] (0 skipped, 1 single, 2 first, 3 last, 4 refused by C2), nkey[r] of the paired ones, paired[0, n] for the scan.
// append: the paired records' entries at E[n_pend + place[r]], and idx[i] = i over all N.  match: fate and partner per entry (fate
// zeroed by the caller).  place: the three scans' inputs (N + 1, N - n_pend + 1 and n + 1 slots).  totals: call[kCoCallWaitBytes ..].
// pairs / singles: the copies with their record offsets.  pool: the waiting entries from `from` on copied to dst + (place - sub),
// all waiting entries written to F (F.key null: none), rec_at (or null) the copied records' offsets.
void launch_co_entry(const uint8_t *bam, const int64_t *rec_off, int64_t n, int64_t base, uint64_t mask, uint8_t *cls, uint64_t *nkey,
                     uint32_t *paired, unsigned long long *call, int cu_count, hipStream_t st);
int co_scan_u32(void *tmp, size_t &tmp_bytes, const uint32_t *in, uint32_t *out, int64_t n, hipStream_t st);
int co_scan_place(void *tmp, size_t &tmp_bytes, const CoPlace *in, CoPlace *out, int64_t n, hipStream_t st);
int co_sort(void *tmp, size_t &tmp_bytes, const uint64_t *key, uint64_t *skey, const uint32_t *idx, uint32_t *sidx, int64_t N, hipStream_t st);
void launch_co_append(const uint8_t *bam, const int64_t *rec_off, int64_t n, int64_t base, const uint8_t *cls, const uint64_t *nkey,
                      const uint32_t *place, int64_t n_pend, const CoEntryArrays &E, uint32_t *idx, int64_t N, int cu_count, hipStream_t st);
void launch_co_match(const uint64_t *skey, const uint32_t *sidx, int64_t N, int64_t n_pend, const CoEntryArrays &E, uint8_t *fate,
                     uint32_t *partner, unsigned long long *call, int cu_count, hipStream_t st);
void launch_co_place(const uint8_t *fate, const uint32_t *partner, const int32_t *size, int64_t N, int64_t n_pend, const uint8_t *cls,
                     const int64_t *rec_off, int64_t n, CoPlace *waits, CoPlace *pairs, CoPlace *singles, int cu_count, hipStream_t st);
void launch_co_totals(const CoPlace *waits, const CoPlace *pairs, const CoPlace *singles, int64_t N, int64_t n_pend, int64_t n,
                      unsigned long long *call, hipStream_t st);
void launch_co_pairs(const CoEntryArrays &E, const uint8_t *fate, const uint32_t *partner, const CoPlace *at, int64_t n_pend, int64_t m,
                     uint8_t *dst, int64_t *pair_off, int cu_count, hipStream_t st);
void launch_co_singles(const uint8_t *bam, const int64_t *rec_off, const uint8_t *cls, const CoPlace *at, int64_t n, uint8_t *dst,
                       int64_t *single_off, int cu_count, hipStream_t st);
void launch_co_pool(const CoEntryArrays &E, const uint8_t *fate, const CoPlace *at, int64_t from, int64_t N, uint8_t *dst, int64_t sub,
                    const CoEntryArrays &F, int64_t *rec_at, int cu_count, hipStream_t st);

// samview.hip: BAM records as SAM lines (rules V1-V8 in include/bwams.h above bwams_samview_open).  The reference names lie back to
// back without their NULs, name r being names[name_off[r], name_off[r + 1]).  count: size[r] = (the line's bytes, 1), or (0, 0) for
// a record rule V2 filters or rule V6 refuses, size[n_rec] = (0, 0); *bad = min(*bad, r << 3 | reason - 1).  write: `at` is the
// exclusive scan of size over its n_rec + 1 slots; the lines at text + at[r].bytes, line_off[at[r].n] = at[r].bytes, the end of
// the last line from slot n_rec.
struct SvArgs {
    const uint8_t *bam;
    const int64_t *rec_off;
    int64_t n_rec;
    const uint8_t *names;
    const int64_t *name_off;
    int32_t n_ref;
    uint32_t require, exclude, min_mapq;
    CoPlace *size;
    const CoPlace *at;
    uint8_t *text;
    int64_t *line_off;
    unsigned long long *bad;
};
void launch_samview_count(const SvArgs &A, int cu_count, hipStream_t st);
void launch_samview_write(const SvArgs &A, int cu_count, hipStream_t st);

// api_bam.hip: the offsets of host BAM records bam[0, n_bytes) (n + 1 of them) from their block_size chain, with the checks of
// bwams_bam_upload (every record whole, block_size >= 32, refID >= -1, POS in [-1, 2^31 - 2], name and CIGAR inside the record) and
// the largest refID; BWAMS_ERR_ARG with `who` and the first bad record in the last error.
int bam_record_offsets(const char *who, const void *bam, int64_t n_bytes, std::vector<int64_t> *offsets, int32_t *max_rid);

// The grid of a grid-stride launch: a block per per_block items, at least one and at most per_cu for each compute unit.
inline unsigned grid_of(int64_t items, int64_t per_block, int cu_count, int per_cu = 16) {
    int64_t g = (items + per_block - 1) / per_block;
    const int64_t cap = (int64_t)cu_count * per_cu;
    return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

// depth.hip: depth of coverage (rules in include/bwams.h above bwams_depth_open).  slots: l_ref[r] + 1 int32 per reference from
// slot_off[r] (n_ref + 1 entries, device); differences while records are added, depths after the scan.  check: *bad = min(*bad, index
// of a record with an op code above 8).  add: rule 2's filter and rule 3's stretches of the records at bam + rec_off[r]; *n_counted +=
// the records that passed.  summary: sum / mn / mx per reference (zeroed / INT_MAX / 0 by the caller).  windows: sums[win_off[r] +
// pos / w] (zeroed by the caller).  hist: slots [lo, hi) into hist[0, n_bins) (zeroed by the caller), the last bin open-ended.
// gather: depth[k] = slots[base + start[k]].
constexpr int kDepthHistLds = 4096;      // depths below this are counted in LDS
void launch_depth_check(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, unsigned long long *bad, int cu_count, hipStream_t st);
void launch_depth_add(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const bwams_depth_opt_t &opt, int32_t n_ref,
                      const int64_t *slot_off, int32_t *slots, unsigned long long *n_counted, int combine, int cu_count, hipStream_t st);
void launch_depth_summary(const int32_t *slots, const int64_t *slot_off, int32_t n_ref, int64_t n_slots, unsigned long long *sum,
                          int32_t *mn, int32_t *mx, int cu_count, hipStream_t st);
void launch_depth_windows(const int32_t *slots, const int64_t *slot_off, int32_t n_ref, int64_t n_slots, const int64_t *win_off, int32_t w,
                          unsigned long long *sums, int cu_count, hipStream_t st);
void launch_depth_hist(const int32_t *slots, int64_t lo, int64_t hi, int32_t n_bins, unsigned long long *hist, int cu_count, hipStream_t st);
void launch_depth_gather(const int32_t *slots, int64_t base, const int32_t *start, int64_t n, int32_t *depth, int cu_count, hipStream_t st);

// pileup.hip: per-base allele counts and candidate sites (rules in include/bwams.h above bwams_pileup_open).  counts: kPileupChannels
// uint32 per slot, a slot per region position in region order.  check: bad[0] = min(bad[0], index of a record with an op code above
// 8), bad[1] the same for a counted record whose CIGAR query length is not l_seq, bad[2] for one whose SEQ or QUAL ends behind it.  route: rule 2's filter and each record's way
// (route[r]); tiled != 0 also writes the (tile, record) entries 2r and 2r + 1 into keys / vals, unused ones with the key n_tiles;
// counts[0..2] += records counted, entries, records routed direct.  tiles: the entries sorted by key; heads (min(n_ent, n_tiles)
// slots) and *n_heads (zeroed by the caller) are scratch.  direct: the records with route[r] == kPileupDirect.  sites: the site
// records of the selected slots, calls: rule 13's call records of the selected slots.  ref: rule 7's gather from an index (holes: the .amb holes, ascending, or none).
constexpr int kPileupTile = 1024;        // positions of a tile: 12 channels x 1024 x 4 bytes = 48 KB of a workgroup's LDS; 96 KB with the quality plane
constexpr int kPileupChannels = BWAMS_PILEUP_CHANNELS, kPileupN = BWAMS_PILEUP_N, kPileupDel = BWAMS_PILEUP_DEL, kPileupIns = BWAMS_PILEUP_INS;
enum : uint8_t { kPileupSkip = 0, kPileupTiled = 1, kPileupDirect = 2 };
struct PileupFilter {
    uint32_t exclude;
    int32_t min_mapq, n_ref;
};
struct PileupRegions {                   // device arrays: region k is [beg[k], end[k]) from slot off[k]; reference r's regions are [ref_first[r], ref_first[r + 1])
    const int32_t *beg, *end, *ref_first;
    const int64_t *off;
};
struct PileupSiteTest {                  // rule 8 at slot s: the candidate alleles' bits (0 = no site) and the depth
    const uint32_t *counts;
    const uint8_t *ref;
    uint32_t min_alt, min_permille;
    __host__ __device__ uint32_t kinds(int64_t s, uint32_t *depth) const {
        const uint32_t *c = counts + s * kPileupChannels;
        const uint32_t b = ref[s];
        uint64_t d = c[kPileupDel];
        for (int k = 0; k < 8; ++k) d += c[k];
        *depth = (uint32_t)d;
        if (b > 3) return 0;
        uint32_t out = 0;
        for (uint32_t a = 0; a < 6; ++a) {
            const uint64_t n = a < 4 ? (uint64_t)c[a] + c[a + 4] : c[kPileupDel + (a - 4)];
            if (a != b && n >= min_alt && n * 1000 >= (uint64_t)min_permille * d) out |= 1u << a;
        }
        return out;
    }
    __host__ __device__ bool operator()(int64_t s) const { uint32_t d; return kinds(s, &d) != 0; }
};
// Rule 12's tables over the effective qualities kPileupGlMinQ .. kPileupGlMaxQ, in hundredths of a phred, and rule 13's mismatch cost
// 100 q + kPileupGlMis.  bwams/pileup.py holds the same numbers; tests/test_pileup_calls.py recomputes both and reads these literals.
constexpr int kPileupGlMinQ = 4, kPileupGlMaxQ = 60, kPileupGlMis = 477;
__host__ __device__ __forceinline__ uint32_t pileup_gl_hom(int qe) {
    constexpr uint16_t kPileupGlHom[kPileupGlMaxQ - kPileupGlMinQ + 1] = {
        220, 165, 126, 97, 75, 58, 46, 36, 28, 22, 18, 14, 11, 9, 7, 6, 4, 3, 3, 2, 2, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return kPileupGlHom[qe - kPileupGlMinQ];
}
__host__ __device__ __forceinline__ uint32_t pileup_gl_het(int qe) {
    constexpr uint16_t kPileupGlHet[kPileupGlMaxQ - kPileupGlMinQ + 1] = {
        435, 404, 381, 363, 350, 339, 331, 325, 320, 316, 313, 310, 308, 307, 306, 305, 304, 303, 303, 302, 302, 302, 302, 302, 301, 301,
        301, 301, 301, 301, 301, 301, 301, 301, 301, 301, 301, 301, 301, 301, 301, 301, 301, 301, 301, 301, 301, 301, 301, 301, 301,
        301, 301, 301, 301, 301, 301};
    return kPileupGlHet[qe - kPileupGlMinQ];
}
// The quality plane (rule 11): kPileupChannels uint32 per slot beside the counters, Q[A..T], HOM[A..T], HET[A..T].  `quality` in the
// launches below: the plane, or null for a handle without one (the count-only kernels run, as before the plane existed).
struct PileupQuality {
    uint32_t *sums;
    int32_t no_qual_q;
};
struct PileupCallTest {                  // rule 13 at slot s
    const uint32_t *counts, *sums;
    const uint8_t *ref;
    int32_t min_qual, min_depth;
    // the slot's record but region and pos; false when rule 13 does not apply (reference base 4, or fewer than min_depth bases)
    __host__ __device__ bool genotype(int64_t s, bwams_pileup_call_t *out) const {
        const uint32_t *c = counts + s * kPileupChannels, *q = sums + s * kPileupChannels;
        const int32_t r = ref[s];
        uint64_t n[4], mis[4], depth = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            n[b] = (uint64_t)c[b] + c[b + 4];
            mis[b] = 100 * (uint64_t)q[b] + (uint64_t)kPileupGlMis * n[b];
            depth += n[b];
        }
        if (r > 3 || depth < (uint64_t)min_depth) return false;
        uint64_t cost[10], least = ~0ULL, cost_rr = 0;                   // every loop unrolled: the arrays stay in registers
        int best = 0;
#pragma unroll
        for (int a2 = 0; a2 < 4; ++a2)
#pragma unroll
            for (int a1 = 0; a1 <= a2; ++a1) {
                const int g = a2 * (a2 + 1) / 2 + a1;
                uint64_t x = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) x += b != a1 && b != a2 ? mis[b] : a1 == a2 ? q[BWAMS_PILEUP_HOM + b] : q[BWAMS_PILEUP_HET + b];
                cost[g] = x;
                if (x < least) { least = x; best = g; out->a1 = a1; out->a2 = a2; }    // ascending g: a tie stays with the lowest
                if (a1 == r && a2 == r) cost_rr = x;
            }
        int32_t second = 0x7FFFFFFF;
#pragma unroll
        for (int g = 0; g < 10; ++g) {
            const uint64_t pl = (cost[g] - least + 50) / 100;
            out->pl[g] = pl > 0x7FFFFFFFULL ? 0x7FFFFFFF : (int32_t)pl;
            if (g != best && out->pl[g] < second) second = out->pl[g];
        }
        const uint64_t pl_rr = (cost_rr - least + 50) / 100;
        out->ref = r;
        out->qual = pl_rr > 0x7FFFFFFFULL ? 0x7FFFFFFF : (int32_t)pl_rr;
        out->gq = second < 99 ? second : 99;
        out->depth = (uint32_t)depth;
#pragma unroll
        for (int b = 0; b < 4; ++b) out->n[b] = (uint32_t)n[b];
        return true;
    }
    __host__ __device__ bool operator()(int64_t s) const {
        bwams_pileup_call_t x;
        return genotype(s, &x) && !(x.a1 == x.ref && x.a2 == x.ref) && x.qual >= min_qual;
    }
};
void launch_pileup_check(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const PileupFilter &f, unsigned long long *bad,
                         int cu_count, hipStream_t st);
void launch_pileup_route(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const PileupFilter &f, const PileupRegions &R,
                         uint32_t n_tiles, int tiled, uint32_t *keys, uint32_t *vals, uint8_t *route, unsigned long long *counts,
                         int cu_count, hipStream_t st);
int launch_pileup_tiles(const uint8_t *bam, const int64_t *rec_off, const PileupRegions &R, int min_baseq, const uint32_t *keys,
                        const uint32_t *vals, int64_t n_ent, uint32_t n_tiles, uint32_t *heads, uint32_t *n_heads, int64_t n_slots,
                        uint32_t *counts, const PileupQuality &quality, int cu_count, hipStream_t st);      // -1: the LDS of the quality tile was refused
void launch_pileup_direct(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const PileupRegions &R, int min_baseq,
                          const uint8_t *route, uint32_t *counts, const PileupQuality &quality, int cu_count, hipStream_t st);
void launch_pileup_calls(const PileupCallTest &test, const PileupRegions &R, int32_t n_regions, const int64_t *slots, int64_t n,
                         bwams_pileup_call_t *out, int cu_count, hipStream_t st);
void launch_pileup_sites(const PileupSiteTest &test, const PileupRegions &R, int32_t n_regions, const int64_t *slots, int64_t n,
                         bwams_pileup_site_t *out, int cu_count, hipStream_t st);
void launch_pileup_ref(const PileupRegions &R, int32_t n_regions, const int32_t *reg_ref, int64_t n_slots, const uint8_t *ref0123,
                       const bwams_contig_t *contigs, const int64_t *hole_off, const int32_t *hole_len, int32_t n_holes, uint8_t *out,
                       int cu_count, hipStream_t st);

// pileup_indel.hip: the indel store of a pileup handle (rules 14 to 17).  An event is a 16-byte key and its quality: k0 holds
// slot << 8 | type << 6 | len and seq the packed bases, so the order by (k0, seq) is rule 16's order by (slot, type, len, seq).  diff:
// rule 15's sums as a difference array, four uint32 per entry over n_slots + 1 entries; span: its inclusive scan, four per slot.
struct PileupEvKey {
    uint64_t k0, seq;
    __host__ __device__ int64_t slot() const { return (int64_t)(k0 >> 8); }
    __host__ __device__ int type() const { return (int)(k0 >> 6) & 3; }
    __host__ __device__ int len() const { return (int)k0 & 63; }
};
struct PileupEvLess {
    __host__ __device__ bool operator()(const PileupEvKey &a, const PileupEvKey &b) const { return a.k0 < b.k0 || (a.k0 == b.k0 && a.seq < b.seq); }
};
struct PileupEvEqual {
    __host__ __device__ bool operator()(const PileupEvKey &a, const PileupEvKey &b) const { return a.k0 == b.k0 && a.seq == b.seq; }
};
struct PileupEvSums {                    // a group's n, Q, HOM and HET (rule 16)
    uint64_t n, q, hom, het;
    __host__ __device__ PileupEvSums operator+(const PileupEvSums &o) const { return PileupEvSums{n + o.n, q + o.q, hom + o.hom, het + o.het}; }
};
struct PileupEvSumsOf {                  // an event's share of its group, from its qe
    __host__ __device__ PileupEvSums operator()(uint32_t qe) const { return PileupEvSums{1, qe, pileup_gl_hom((int)qe), pileup_gl_het((int)qe)}; }
};
struct PileupSpan {                      // SPAN_N, SPAN_Q, SPAN_HOM, SPAN_HET, modulo 2^32
    uint32_t v[4];
    __host__ __device__ PileupSpan operator+(const PileupSpan &o) const { return PileupSpan{{v[0] + o.v[0], v[1] + o.v[1], v[2] + o.v[2], v[3] + o.v[3]}}; }
};
struct PileupIndelStore {                // what the event kernels write: the difference array, the events from *n_events on (cap of them)
    uint32_t *diff;
    PileupEvKey *keys;
    uint32_t *qe;
    unsigned long long *n_events;
    int64_t cap;
    int32_t indel_q, max_len;
};
struct PileupIndelTest {                 // rule 16 over the sorted groups: group i is asked, and answers only as the first group of its slot
    const PileupEvKey *keys;
    const PileupEvSums *sums;
    int64_t n_groups;
    const PileupSpan *span;
    const uint8_t *ref;
    int32_t min_qual, min_depth;
    // the slot's record but region, pos and del_ref; false when i is not the first group of its slot, or rule 16 gives no ALT there
    __host__ __device__ bool genotype(int64_t i, bwams_pileup_indel_t *out, uint64_t *depth) const {
        const int64_t s = keys[i].slot();
        if (i > 0 && keys[i - 1].slot() == s) return false;
        const int32_t r = ref[s];
        if (r > 3) return false;
        int64_t alt = -1;
        uint64_t n_alt = 0, total = 0;
        for (int64_t j = i; j < n_groups && keys[j].slot() == s; ++j) {
            const uint64_t n = sums[j].n;
            total += n;
            if (keys[j].type() < BWAMS_PILEUP_EV_OTHER && n > n_alt) { alt = j; n_alt = n; }     // ascending order: a tie stays with the first
        }
        if (alt < 0) return false;
        const PileupSpan sp = span[s];
        const PileupEvSums a = sums[alt];
        const uint64_t cost[3] = {(uint64_t)sp.v[BWAMS_PILEUP_SPAN_HOM] + 100 * a.q + (uint64_t)kPileupGlMis * a.n,
                                  (uint64_t)sp.v[BWAMS_PILEUP_SPAN_HET] + a.het,
                                  100 * (uint64_t)sp.v[BWAMS_PILEUP_SPAN_Q] + (uint64_t)kPileupGlMis * sp.v[BWAMS_PILEUP_SPAN_N] + a.hom};
        const int best = cost[1] < cost[0] ? (cost[2] < cost[1] ? 2 : 1) : (cost[2] < cost[0] ? 2 : 0);
        int32_t second = 0x7FFFFFFF;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const uint64_t pl = (cost[g] - cost[best] + 50) / 100;
            out->pl[g] = pl > 0x7FFFFFFFULL ? 0x7FFFFFFF : (int32_t)pl;
            if (g != best && out->pl[g] < second) second = out->pl[g];
        }
        out->ref = r;
        out->type = keys[alt].type();
        out->len = keys[alt].len();
        out->reserved = 0;
        out->seq = keys[alt].seq;
        out->gt = best;
        out->qual = out->pl[0];
        out->gq = second < 99 ? second : 99;
        *depth = (uint64_t)sp.v[BWAMS_PILEUP_SPAN_N] + total;
        out->depth = (uint32_t)*depth;
        out->n_ref = sp.v[BWAMS_PILEUP_SPAN_N];
        out->n_alt = (uint32_t)n_alt;
        out->n_other = (uint32_t)(total - n_alt);
        return true;
    }
    __host__ __device__ bool operator()(int64_t i) const {
        bwams_pileup_indel_t x;
        uint64_t depth;
        return genotype(i, &x, &depth) && x.gt != 0 && x.qual >= min_qual && depth >= (uint64_t)min_depth;
    }
};
// events: emit == 0 adds to *S.n_events the events the records would append and writes nothing else; emit != 0 appends them and adds
// rule 15's runs to S.diff.  alleles and indel_calls: the records of the groups / of the selected first groups.
void launch_pileup_indel_events(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const PileupFilter &f, const PileupRegions &R,
                                const PileupIndelStore &S, int emit, int cu_count, hipStream_t st);
// rule 18: events_run is the emitting event pass that also writes run[e - first] for every event e it appends (S.cap - first words:
// the slots below the anchor that the run of match ops ending there spans); align shifts the n events at keys / qe / run against
// ref, rewrites their keys in place and corrects diff.
void launch_pileup_indel_events_run(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const PileupFilter &f, const PileupRegions &R,
                                    const PileupIndelStore &S, uint32_t *run, int64_t first, int cu_count, hipStream_t st);
void launch_pileup_indel_align(const PileupRegions &R, int32_t n_regions, const uint8_t *ref, PileupEvKey *keys, const uint32_t *qe,
                               const uint32_t *run, int64_t n, uint32_t *diff, int cu_count, hipStream_t st);
void launch_pileup_indel_alleles(const PileupEvKey *keys, const PileupEvSums *sums, int64_t n_groups, const PileupRegions &R, int32_t n_regions,
                                 bwams_pileup_indel_allele_t *out, int cu_count, hipStream_t st);
void launch_pileup_indel_calls(const PileupIndelTest &test, const PileupRegions &R, int32_t n_regions, const int64_t *groups, int64_t n,
                               bwams_pileup_indel_t *out, int cu_count, hipStream_t st);

// qc.hip: alignment QC (rules in include/bwams.h above bwams_qc_open).  All counters are one block of 64-bit words in HBM, laid out by
// QcLayout: the flag counters, the scalars, then rule 4's six tables.  check: *bad = min(*bad, record << 3 | reason).  records: rules
// 2-5 but tables b and c; lists[c * n_rec ..] gets the indices of class c's filtered-in records with l_seq > 0 and call[] (zeroed by
// the caller) the two list lengths, the two largest l_seq, the records counted and the bases past max_cycle.  cycles: tables b and c
// and the two quality scalars from the lists, by the lane-per-cycle kernel or (lanes == 0) the plain one.
constexpr int kQcIsizeLds = 1024;        // ISIZE bins of a row counted in LDS by the record kernel; the bins from here on go by global atomics
constexpr int kQcSlice = 1024;           // records of a list that one wave of the cycle kernel takes at a time
enum { kQcBadBounds = 0, kQcBadOp = 1, kQcBadSeq = 2, kQcBadAux = 3 };
enum { kQcCallList = 0, kQcCallMaxLen = 2, kQcCallCounted = 4, kQcCallOver = 5, kQcCallWords = 8 };
struct QcLayout {                        // offsets in 64-bit words
    int32_t max_cycle, max_isize;
    uint32_t exclude;
    __host__ __device__ int64_t flags() const { return 0; }
    __host__ __device__ int64_t scalars() const { return 32; }
    __host__ __device__ int64_t rl() const { return 48; }
    __host__ __device__ int64_t qual() const { return rl() + 2 * ((int64_t)max_cycle + 1); }
    __host__ __device__ int64_t base() const { return qual() + 2 * (int64_t)max_cycle * 64; }
    __host__ __device__ int64_t mapq() const { return base() + 2 * (int64_t)max_cycle * 5; }
    __host__ __device__ int64_t isize() const { return mapq() + 256; }
    __host__ __device__ int64_t indel() const { return isize() + 3 * ((int64_t)max_isize + 1); }
    __host__ __device__ int64_t words() const { return indel() + 2 * 65; }
};
void launch_qc_check(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, uint32_t exclude, unsigned long long *bad, int cu_count,
                     hipStream_t st);
void launch_qc_records(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const QcLayout &L, unsigned long long *counters,
                       uint32_t *lists, unsigned long long *call, int cu_count, hipStream_t st);
void launch_qc_cycles(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const QcLayout &L, unsigned long long *counters,
                      const uint32_t *lists, const unsigned long long *call, int lanes, int cu_count, hipStream_t st);

// api_bam.hip: the groups table as the device reads it, uploaded into the caller's buffers (g null: no table, G->walk = 0)
int groups_upload(DevBuf<uint8_t> &g_ids, DevBuf<int64_t> &g_off, DevBuf<int32_t> &g_ord, DevBuf<int32_t> &g_lib,
                  const bwams_dup_groups_t *g, MdGroupsDev *G, hipStream_t st);
// api_bam.hip: md_decide's counts (pairs, pair duplicates, fragment duplicates) as bwams_dup_stats_t; rule 13's rows from the device's
// counts (7 words per library), rule 14 and the percentage added; opt as md_decide takes it (d, 0: off; the largest group examined),
// false for a negative value
void dup_stats(bwams_dup_stats_t *st, int64_t n_t, int64_t n_e, const int64_t cnt[3], float ms);
void lib_rows(bwams_dup_lib_stats_t *rows, int64_t n_lib, const unsigned long long *c);
bool dup_opt_values(const bwams_dup_opt_t *opt, int64_t *d, int64_t *max_set);

// recal.hip: base recalibration tables (rules in include/bwams.h above bwams_recal_open).
// The store: a nibble per reference position, bits 0-2 the reference code 0..4, bit 3 the known-site flag; eight nibbles to a 32-bit
// word, nibble k of a word in bits 4k .. 4k + 3; reference r begins at word ref_word[r] (n_ref + 1 entries), so no word is shared by
// two references.  The tables: one block of 64-bit words, a cell two of them (observations, errors), laid out by RecalLayout.
// check: *bad = min(*bad, record << 3 | reason).  records: rule 4's filter and the read group of each record; key[r] = 2 * group +
// (cycles negative), or n_keys for a record that does not count; call[] (zeroed by the caller) gets the records counted and, per key,
// the largest l_seq (call + kRecalCallMaxLen).  After a sort by key: heads / items turn the sorted keys into the item table of the
// base kernel; bases: the default path; plain: BWAMS_RECAL_LDS=0.
constexpr int kRecalQuals = 94, kRecalContexts = 16;
// rule 6's context of a base b behind its neighbour in sequencing order nb (both 0..3): as read, or complemented under FLAG 0x10
__device__ __forceinline__ int recal_context(int nb, int b, bool rev) { return rev ? 4 * (3 - nb) + (3 - b) : 4 * nb + b; }
constexpr int kRecalSlice = 1024;        // records of one key that a workgroup of the base kernel counts in LDS before it flushes (below 65536: 16-bit cells)
enum { kRecalBadOp = 0, kRecalBadLength = 1, kRecalBadBounds = 2, kRecalBadCycle = 3, kRecalBadAux = 4 };
enum { kRecalCallCounted = 0, kRecalCallBases = 1, kRecalCallItems = 2, kRecalCallMaxLen = 4 };
struct RecalLayout {                     // offsets in 64-bit words
    int32_t n_rg, max_cycle;
    __host__ __device__ int64_t rows() const { return (int64_t)n_rg + 1; }
    __host__ __device__ int64_t cols() const { return 2 * (int64_t)max_cycle + 1; }
    __host__ __device__ int64_t rg() const { return 0; }
    __host__ __device__ int64_t qual() const { return 2 * rows(); }
    __host__ __device__ int64_t cycle() const { return qual() + 2 * rows() * kRecalQuals; }
    __host__ __device__ int64_t context() const { return cycle() + 2 * rows() * kRecalQuals * cols(); }
    __host__ __device__ int64_t words() const { return context() + 2 * rows() * kRecalQuals * kRecalContexts; }
};
struct RecalStore {
    const uint32_t *words;
    const int64_t *ref_word;             // n_ref + 1
    const int32_t *l_ref;
};
struct RecalFilter {
    uint32_t exclude;
    int32_t min_mapq, min_baseq, max_cycle, n_ref;
};
void launch_recal_check(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const RecalFilter &f, int walk_aux, unsigned long long *bad,
                        int cu_count, hipStream_t st);
void launch_recal_records(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const RecalFilter &f, const MdGroupsDev &G,
                          uint32_t n_keys, uint32_t *keys, uint32_t *vals, unsigned long long *call, int cu_count, hipStream_t st);
void launch_recal_items(const uint32_t *keys, int64_t n_rec, uint32_t n_keys, const unsigned long long *call_max_len, uint32_t *key_first,
                        int64_t *item_first, unsigned long long *n_items, hipStream_t st);
void launch_recal_bases(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const RecalFilter &f, const RecalStore &S,
                        const RecalLayout &L, const uint32_t *vals, uint32_t n_keys, const uint32_t *key_first, const int64_t *item_first,
                        const unsigned long long *n_items, unsigned long long *tables, unsigned long long *call, int cu_count, hipStream_t st);
void launch_recal_plain(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const RecalFilter &f, const RecalStore &S,
                        const RecalLayout &L, const uint32_t *keys, uint32_t n_keys, unsigned long long *tables, unsigned long long *call,
                        int cu_count, hipStream_t st);
void launch_recal_set_ref(uint32_t *words, int64_t first_word, const uint8_t *codes, int32_t l_ref, int cu_count, hipStream_t st);
void launch_recal_ref_index(uint32_t *words, const int64_t *ref_word, int32_t n_ref, int64_t n_words, const uint8_t *ref0123,
                            const bwams_contig_t *contigs, const int64_t *hole_off, const int32_t *hole_len, int32_t n_holes, int cu_count,
                            hipStream_t st);
void launch_recal_known(uint32_t *words, const int64_t *ref_word, const bwams_recal_site_t *sites, int64_t n, int cu_count, hipStream_t st);

// recal_apply.hip: the quality model applied to QUAL (rules A to C in include/bwams.h above bwams_recal_model_create).  The model on
// the device: b[row] in [0, 93], dc[row * cols + column] and dx[row * 16 + context] in [-93, 60], row = group * 94 + quality, the
// columns as RecalLayout's.  check: *bad = min(*bad, record << 3 | reason), the reasons kRecalBad* above.  records: key[r] = 2 * group
// + (cycles negative), or n_keys for a record rule A leaves alone; *n_taken (zeroed by the caller) += the records with a key.
// apply: rule C over the records with a key, a wave per record.
struct RecalModelDev {
    const uint8_t *b;
    const int8_t *dc, *dx;
    int32_t n_rg, max_cycle, preserve_below, max_q;
    uint32_t exclude;
    __host__ __device__ int64_t cols() const { return 2 * (int64_t)max_cycle + 1; }
};
void launch_recal_apply_check(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const RecalModelDev &M, int walk_aux,
                              unsigned long long *bad, int cu_count, hipStream_t st);
void launch_recal_apply_records(const uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const RecalModelDev &M, const MdGroupsDev &G,
                                uint32_t n_keys, uint32_t *keys, unsigned long long *n_taken, int cu_count, hipStream_t st);
void launch_recal_apply(uint8_t *bam, const int64_t *rec_off, int64_t n_rec, const RecalModelDev &M, const uint32_t *keys, uint32_t n_keys,
                        int cu_count, hipStream_t st);

// deflate.hip: the device a deflater is bound to; bwams_deflater_run with its work ordered behind what `after` has queued so far
int deflater_device(const bwams_deflater *d);
int deflater_run_after(bwams_deflater *d, hipStream_t after, const void *in, int64_t n_bytes, int in_on_device, void *out, int64_t out_cap,
                       int out_on_device, int32_t flags, int64_t *n_out, bwams_deflate_stats_t *stats);

// banded-SW parameters in kernel form (max_sc = max entry of mat)
struct SwParams {
    int o_del, e_del, o_ins, e_ins, zdrop, end_bonus, max_sc;
    int8_t mat[25];
};

struct Round2Work {
    uint32_t rid;
    int32_t x;
    int32_t min_intv;
};

// A backward phase handed from the lane-per-read SMEM search to the wave-per-pivot kernel (fmi_seed.hip): the pivot and the
// interval list its forward phase left, `num_prev` packed 16-byte entries from `off` of the entry buffer (0 = slot not used).
struct BwdItem {
    uint32_t rid;
    int32_t x;
    int32_t min_intv;
    int32_t num_prev;
    int64_t off;
};

int launch_bsw(bwams_seqpair_t *pairs, int64_t n, const uint8_t *ref, const uint8_t *qer, int w, const SwParams &prm, int qmax,
               DevCounters *ctr, int cu_count, hipStream_t st, int32_t *list, hipStream_t *aux = nullptr, hipEvent_t fork = nullptr,
               hipEvent_t *join = nullptr, const int64_t *src = nullptr, int dir = 1, bool early = false);   // early: bsw_pk_kernel's early exit
size_t bsw_list_bytes(int64_t n_tasks);          // scratch `list` of launch_bsw
int bsw_lds_waves(int qmax);                     // waves per block of launch_bsw's one-task-per-wave kernel; 0: qmax does not fit
void launch_emf_probe(const DevEmf &t, const uint8_t *enc, const int64_t *cum, int64_t nseq, uint32_t *out,
                      uint8_t *code, uint8_t *skip, DevCounters *ctr, hipStream_t st);
// ksw_align2's xtra flags (ksw.h), carried in a task's h0 beside the 16-bit threshold
constexpr int KSW_XBYTE = 0x10000, KSW_XSTOP = 0x20000, KSW_XSUBO = 0x40000, KSW_XSTART = 0x80000;
constexpr int kKswMaxTarget = 20000;     // longest local-SW target: its row-maxima list must fit the LDS of a 4-wave block
int launch_ksw(const bwams_seqpair_t *pairs, int64_t n, const uint8_t *ref, const uint8_t *qer, const SwParams &prm,
                int pmax, int tmax, void *out, DevCounters *ctr, int cu_count, hipStream_t st);

// read input helpers shared with the outer boundary (fastq.hip)
struct SegMove { const char *src; char *dst; int64_t len; };     // one contiguous piece of device memory to copy
int segment_copy(const std::vector<SegMove> &moves, hipStream_t st);
// positions of the '\n' bytes of d_text[0, n_bytes) in HBM (rocPRIM select over a counting iterator, sized by a count first),
// into *ends (allocated here: n_nl + 16 slots)
int line_ends(const char *d_text, int64_t n_bytes, hipStream_t st, DevBuf<int64_t> *ends, int64_t *n_nl);

// trim.hip: read trimming (rules T1 to T9 above bwams_fastq_trim in include/bwams.h).  TrimParams: the options in kernel form, the two
// adapters as bit planes (bit k of a_lo / a_hi[which][k / 64] = the low / high bit of letter k's code).  TrimArrays: a decoded
// chunk's arrays, the offsets in device memory too.  reads: report[i] for every read.  widths: wide[row * (n + 1) + i], rows = name
// bytes, comment bytes, bases that read i brings to the new chunk; gather: the kept reads to offs = the exclusive scans of those rows.
struct TrimParams {
    int32_t trim_front, trim_tail, cut_front, cut_tail, cut_window, cut_quality, overlap, overlap_min, overlap_max_diff, overlap_diff_pct,
        adapter_min_match, adapter_mismatch_per, max_len, min_len, n_limit, qual_floor, low_qual_pct;
    int32_t paired, has_qual;
    int32_t a_len[2];
    unsigned long long a_lo[2][2], a_hi[2][2];
};
struct TrimArrays {
    uint8_t *enc;
    char *qual, *names, *comments;       // qual: nullptr for a chunk without qualities
    const int64_t *cum, *name_off, *comment_off;
};
void launch_trim_reads(const uint8_t *enc, const char *qual, const int64_t *cum, int64_t n_reads, const TrimParams &P, bwams_trim_read_t *report,
                       hipStream_t st);
void launch_trim_widths(const bwams_trim_read_t *report, const int64_t *name_off, const int64_t *comment_off, int64_t n, int64_t *wide,
                        hipStream_t st);
void launch_trim_gather(const bwams_trim_read_t *report, int64_t n, const TrimArrays &in, const int64_t *offs, const TrimArrays &out,
                        hipStream_t st);
// a decoded chunk as FASTQ text: wide[i] = the bytes of read i's record (0 at i = n), emit to off = their exclusive scan
void launch_fastq_text_widths(const TrimArrays &in, int64_t n, int with_comment, int64_t *wide, hipStream_t st);
void launch_fastq_text_emit(const TrimArrays &in, int64_t n, int with_comment, const int64_t *off, char *text, hipStream_t st);

// The reference metadata of an index made from FASTA (fasta_ref.hip): what bns_fasta2bntseq keeps and bns_dump writes.
struct BnsMeta {
    int64_t l_pac = 0;
    std::vector<std::string> names, comments;           // comments: kseq's, empty = none (add1 stores "(null)")
    std::vector<int64_t> ctg_off;
    std::vector<int32_t> ctg_len, ctg_ambs;
    std::vector<int64_t> hole_off;                       // bntamb1_t: offset, len, amb
    std::vector<int32_t> hole_len;
    std::vector<char> hole_amb;
    DevBuf<> d_pac;                                      // the 2-bit .pac, ceil(l_pac / 4) bytes in HBM
};
}  // namespace bwams
// a decoded chunk of reads (fastq.hip: FASTQ / FASTA text; bam_reads.hip: BAM records), resident on its device
struct bwams_fastq {
    int device = 0;
    int64_t n_reads = 0, n_bases = 0, name_bytes = 0, comment_bytes = 0;
    bwams::DevBuf<uint8_t> d_enc;
    bwams::DevBuf<char> d_qual, d_names, d_comments;
    std::vector<int64_t> cum, name_off, comment_off;       // host copies of the three offset arrays
    float ms = 0;
    bool has_qual = true;                                  // false: FASTA text, or BAM records without qualities
    float ms_discover = 0;                                 // bam_reads.hip: the part of ms spent finding the records,
    int64_t n_cand = 0, n_records = 0;                     // the offsets that passed its filter, the records (skipped ones included)
    bwams::DevBuf<char> d_text;                            // api_trim.hip: the chunk as FASTQ text (bwams_fastq_text), text_bytes of it
    int64_t text_bytes = -1;                               // -1: no text yet
    // a decode that fails half way (an allocation, a kernel) drops the handle: whatever it had allocated goes with it
    ~bwams_fastq() {
        if (d_enc.p || d_qual.p || d_names.p || d_comments.p || d_text.p) (void)hipSetDevice(device);
    }
};
namespace bwams {
int fastq_classify(bwams_fastq *f, std::vector<uint8_t> *which);                       // bseq_classify: 1 = an end of a pair
int fastq_subset(bwams_fastq *f, const std::vector<int64_t> &ids, bwams_fastq **out);  // those reads as a chunk of their own
int fastq_interleave(bwams_fastq *f1, bwams_fastq *f2, bwams_fastq **out);             // read k of f1, read k of f2, ...
}  // namespace bwams

struct bwams_index {
    int device = 0;
    bwams::DevFmi fmi{};                         // points at d_cp .. d_ref, or at the caller's memory (bwams_index_from_device: they stay empty)
    int64_t bytes = 0;
    int64_t n_blk = 0, n_sa = 0;
    bwams::DevBuf<> d_cp, d_ms, d_ls, d_ref;
    bwams::DevBuf<> d_cp2;                       // the search kernels' table derived from the CP_OCC array at the first FM-index seeding;
    std::mutex cp2_mu;                           // ... published under this lock once built, freed only by bwams_index_close
    // The dense suffix-array table (fmi_kernels.h), built at the first FM-index seeding with coordinates and released, for good, when
    // the device runs out of memory (DESIGN.md "The dense suffix-array table").  sa_mu guards the four fields: shared to read the
    // pointer and launch the lookup that reads it, exclusive to build and to release.
    bwams::DevBuf<> d_sa_dense;
    std::shared_mutex sa_mu;
    int sa_state = BWAMS_SA_DENSE_ABSENT, sa_stride = 0;
    float sa_build_ms = 0;
    std::atomic<int64_t> sa_bytes{0};            // the table's bytes while it is resident (bwams_debug_sa_dense_state)
    bwams_index();                               // api_index.hip: every index is known to sa_dense_release while it lives
    ~bwams_index();
    bwams::DevBuf<> d_all, d_last;               // FMA tables
    bwams::DevBuf<> d_contigs;                   // bwams_contig_t[n_seqs]; empty = one sequence [0, l_pac)
    int32_t n_seqs = 0;
    bwams::DevBuf<> d_ctg_annos, d_ctg_anno_off;   // bntann1_t.anno for MEM_F_REF_HDR (bwams_index_set_contig_annos)
    bwams::DevBuf<> d_ctg_names, d_ctg_off;      // sequence names for the SAM text (bwams_index_set_contig_names)
    bwams::BnsMeta *bns = nullptr;               // .ann / .amb / .pac of an index made from FASTA (bwams_index_from_fasta), else null
    std::vector<std::string> h_ctg_names;        // host copy of the sequence names (the SAM / BAM headers)
    bwams::DevBuf<> d_ctg_sorted;                // int32 permutation of the names in strcmp order: the BAM encoder's RNAME lookup
    bool ctg_dup = false;                        // two sequences share a name (the BAM entry points refuse the index)
};

namespace bwams {
int bns_save(bwams_index *ix, const char *prefix);     // fasta_ref.hip: writes <prefix>.ann, .amb, .pac
int sa_dense_ensure(bwams_index *ix, int cu_count, hipStream_t st);   // api_index.hip: builds ix's dense table unless it has a state already
int bam_names_index(bwams_index *ix, const char *names, const int32_t *name_off, int32_t n);   // bam.hip, from set_contig_names
}

struct bwams_ert {
    bwams_index *idx = nullptr;
    bwams::DevErt t{};
    bwams::DevBuf<> d_kmer, d_mlt, d_cnt, d_fat;
    int64_t bytes = 0, mlt_bytes = 0, n_big = 0;
    float build_ms[3] = {0, 0, 0};       // bwams_ert_build: sizes, scan + allocation, bytes
};

struct bwams_emf {
    bwams_index *idx = nullptr;
    bwams::DevEmf t{};                   // points at d_seeds / d_loc, or at the caller's table (bwams_emf_from_device: they stay empty)
    bwams::DevBuf<> d_seeds, d_loc;
    int64_t bytes = 0;
    int64_t n_used = 0, n_key = 0, n_other = 0, build_ms = 0;     // bwams_emf_build: distinct L-mers, buckets used, nodes outside their bucket
};

namespace bwams {
int emf_build_device(bwams_emf *e, const uint8_t *ref, int64_t l_pac, int seed_len, double slack, int cu_count, int verbose,
                     int64_t stats[4]);
}

struct bwams_batch {
    template <class T = void> using DevBuf = bwams::DevBuf<T>;
    // what every stage reads
    bwams_index *idx = nullptr;
    hipStream_t stream = nullptr;
    int cu_count = 0;
    int64_t max_reads = 0, max_bases = 0, max_smem = 0, max_sa = 0;
    int64_t pool_cap = 0;                // max_smem + chunk slack
    DevBuf<uint8_t> d_enc;               // the resident reads
    DevBuf<int64_t> d_cum;
    DevBuf<uint8_t> d_skip;
    bool has_skip = false;
    int64_t nseq = 0, nbases = 0;
    int max_read_len = 0;
    // which products are current (stage_valid.h; produced / outdated / has below).  A new batch holds the chunk of no reads.
    uint32_t valid = bwams::bit(bwams::Product::reads);
    DevBuf<bwams::DevCounters> d_ctr;
    bwams::HostBuf<bwams::DevCounters> h_ctr;   // pinned host mirror
    DevBuf<> d_tmp;                      // rocPRIM temporary storage
    bwams_stats_t stats{};

    struct Seed {                        // seeding over the FM-index or the ERT (api_seed.hip); chaining reads the sorted SMEMs and the SA buffers
        DevBuf<bwams_smem_t> d_pool;     // unsorted SMEM pool (append order)
        DevBuf<bwams_smem_t> d_sorted;   // (rid, m, n) order
        DevBuf<uint64_t> d_keys, d_keys2;
        DevBuf<uint32_t> d_vals, d_vals2;
        DevBuf<bwams::Round2Work> d_work2;
        DevBuf<int64_t> d_sa_off, d_sa_cnt;   // max_smem + 1 each
        DevBuf<int64_t> d_sa_coord;      // max_sa
        DevBuf<uint32_t> d_packed;       // packed reads (2-bit codes + N mask)
        int read_w = 0, read_cw = 0;
        DevBuf<uint4> d_prev;            // per-lane scratch of the SMEM search (previous-interval lists)
        int64_t prev_threads = 0;
        int prev_cap = 0;
        DevBuf<bwams::BwdItem> d_bwd_items;   // SMEM search: backward phases with long interval lists (wave-per-pivot kernel)
        DevBuf<uint4> d_bwd_ent;
        int64_t bwd_items_cap = 0, bwd_ent_cap = 0;
        DevBuf<uint8_t> d_ert_prof;      // ERT seeding: match-length planes, (M + 1) x nbases bytes
        DevBuf<uint64_t> d_ert_stk;      // ERT seeding: stacks of the leaf walks (ert_walk_threads x frames words)
        int ert_stk_frames = 0;
        DevBuf<uint32_t> d_ert_redo;     // ERT seeding: seeds whose hits the rank descent could not list (bit per seed)
        hipStream_t seed_aux = nullptr;  // SMEM round 3 runs beside round 2
        hipEvent_t seed_fork = nullptr, seed_join = nullptr;
        int64_t n_smem = 0, n_sa = 0;
        int64_t n_pool_slots = 0;        // SMEM pool slots the last seeding pass handed out (holes included)
        bool with_sa = false;
        bwams_ert *ert = nullptr;        // the last seed run went over this ERT (nullptr: FM-index)
        bwams_seed_opt_t last_opt{};     // of the last seed run (a grown SA buffer re-runs the lookup)
    } sd;
    struct Sw {                          // banded SW and ksw on uploaded pairs (api_sw.hip); the extension stage borrows d_bsw_list
        DevBuf<bwams_seqpair_t> d_pairs;
        DevBuf<uint8_t> d_ref, d_qer;
        DevBuf<int32_t> d_bsw_list;      // task lists of the banded-SW length classes (launch_bsw)
        DevBuf<> d_ksw_out;              // bwams_kswr_t per pair (launch_ksw's output)
        int64_t n_pairs = 0;
        int max_qlen = 0, max_tlen = 0;
    } sw;
    struct Emf {                         // the EMF probe's results (api_emf.hip); mem_perfect2reg reads them
        DevBuf<uint32_t> d_emf_out;      // a word pair per read
        DevBuf<uint8_t> d_emf_code;
        hipEvent_t ev[2] = {};           // around the probe of bwams_emf_run
        unsigned long long emf_nodes = 0, emf_cmp_bytes = 0;
    } emf;
    bwams::StageState *stages = nullptr; // everything behind seeding, created at its first use (get_state)

    enum Ev {                            // the timing events: of a seeding pass (FM-index | ERT), of the two SW entry points
        kEvSeedStart = 0, kEvRoundsDone = 3, kEvSorted = 4, kEvSeedEnd = 5,   // 3-4 the sort, 4-5 the lookup | locate + hits
        kEvR1Start = 8, kEvR1End = 9,    // round-1 kernel | match profiles
        kEvR2Start = 10, kEvR2End = 11,  // round-2 kernel | the three rounds
        kEvR3Start = 12, kEvR3End = 13,  // round-3 kernel | locate
        kEvBswStart = 6, kEvBswEnd = 7, kEvKswStart = 14, kEvKswEnd = 15, kEvCount = 16
    };
    hipEvent_t ev[kEvCount] = {};
};

namespace bwams {
// The validity mask of a batch.  An entry point that replaces product p calls outdated(b, p) once, before it touches device memory,
// and produced(b, p) as its last act; one that reads p refuses the call unless has(b, p).  self = false: p is changed where it
// lies and stays valid, what was computed from it does not.
inline void produced(bwams_batch *b, Product p) { b->valid |= bit(p); }
inline void outdated(bwams_batch *b, Product p, bool self = true) { b->valid &= ~(kDerived.of[(int)p] | (self ? bit(p) : 0u)); }
template <class... P> bool has(const bwams_batch *b, P... p) { return b && (b->valid & bits(p...)) == bits(p...); }   // a null batch has nothing
int check_device(int device);                  // api.hip: the ordinal names a gfx950 device
int tmp_reserve(bwams_batch *b, size_t &tb);   // grows b->d_tmp to tb bytes (the stream drained first) and sets tb to its size (api.hip)
int alloc_smem_buffers(bwams_batch *b, int64_t max_smem);   // api_seed.hip: (re)allocates every buffer sized by max_smem
int alloc_seed_tmp(bwams_batch *b);            // api_seed.hip: d_tmp for the largest sort / scan the batch can issue
// api.hip: `bytes` of device memory to / from a file through the caller's staging buffer of `chunk` bytes
int dev_to_file(FILE *f, const void *dev, size_t bytes, uint8_t *stage, size_t chunk);
int file_to_dev(FILE *f, void *dev, size_t bytes, uint8_t *stage, size_t chunk);
// A file mapped read-only while the object lives (api.hip).  p stays null when the file cannot be opened (!opened), is shorter than
// min_size or cannot be mapped.
struct MappedFile {
    const uint8_t *p = nullptr;
    size_t size = 0;
    bool opened = false;
    explicit MappedFile(const std::string &path, size_t min_size = 1);
    ~MappedFile();
    MappedFile(const MappedFile &) = delete;
    MappedFile &operator=(const MappedFile &) = delete;
};
// A rocPRIM call with the batch's temporary storage: call(nullptr, bytes) asks for the size, call(storage, bytes) runs.  who names
// the entry point and the call in the error text.
template <class F> int with_tmp(bwams_batch *b, const char *who, F &&call) {    // call(void *tmp, size_t &bytes) -> hipError_t
    size_t tb = 0;
    hipError_t e = call(nullptr, tb);
    if (e == hipSuccess) {
        if (int rc = tmp_reserve(b, tb)) return rc;
        e = call(b->d_tmp.p, tb);
    }
    if (e == hipSuccess) return BWAMS_OK;
    set_last_error(std::string(who) + " -> " + hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? BWAMS_ERR_NOMEM : BWAMS_ERR_DEVICE;
}
// The same for a handle that is no batch: its own temporary storage, grown once `st` has drained.
template <class F> int with_tmp(DevBuf<> &tmp, hipStream_t st, const char *who, F &&call) {
    size_t tb = 0;
    hipError_t e = call(nullptr, tb);
    if (e == hipSuccess && (tb > tmp.cap || !tmp.p)) {           // never null: rocPRIM reads a null pointer as the size query
        e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = tmp.alloc(tb > 256 ? tb : 256);
    }
    if (e == hipSuccess) {
        tb = tmp.cap;
        e = call(tmp.p, tb);
    }
    if (e == hipSuccess) return BWAMS_OK;
    set_last_error(std::string(who) + " -> " + hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? BWAMS_ERR_NOMEM : BWAMS_ERR_DEVICE;
}
}
