// stage_state.h — a batch's state behind seeding (bwams_batch::stages), one member per stage, and the host helpers the
// entry-point files share (defined in api_state.hip).  A DevBuf<T> is read as T everywhere; a DevBuf<> holds several
// rows or types and names its layout.  Whether a stage's result is current is not kept here: bwams_batch::valid (stage_valid.h).
#pragma once

#include "chain_kernels.h"

namespace bwams {

// Streams beside the batch's own that a stage forks its launches onto: banded SW uses all four (launch_bsw: five query-length
// classes with the batch's stream), de-duplication three, chaining two (its plan: chain_wave.h), selection one.
constexpr int kAuxStreams = 4;
struct StageState {
    struct ChainStage {                      // chaining, mem_flt_chained_seeds (sw_*), the ERT input translation (et_*)
        DevBuf<int32_t> s_next, f_first, f_kept, f_sel; DevBuf<int2> s_ql; DevBuf<uint2> flt; DevBuf<uint4> f_rec;       // scratch per SA hit
        DevBuf<> crec, nodes;                // chain records / B-tree nodes: chain_rec_bytes(), chain_node_bytes()
        DevBuf<int32_t> n_kept, n_kept_seeds, n_chn, redo; DevBuf<int64_t> read_base; DevBuf<float> frac;                // per read
        DevBuf<uint32_t> okeys, okeys2, ovals, ovals2;                                                                   // per read: the order of the reads
        DevBuf<> wide, chain_off;            // int64 rows of nseq + 1: chains | seeds per read (counts, then offsets)
        DevBuf<> slice;                      // int64 {beg, end} per read
        DevBuf<bwams_chain_t> chains; DevBuf<bwams_chain_seed_t> seeds, seeds2;                                          // results
        DevBuf<int32_t> sw_qb, sw_read, sw_newn; DevBuf<int64_t> sw_rb; DevBuf<bwams_kswr_t> sw_res;                     // mem_flt_chained_seeds (long reads)
        DevBuf<bwams_ert_mem_t> et_mems; DevBuf<int64_t> et_moff, et_hoff, et_cnt, et_off, et_coord; DevBuf<uint64_t> et_hits;   // ERT mode input translation
        DevBuf<bwams_smem_t> et_smem;
        DevBuf<> et_srt;                     // 24-byte sort records (ert_chain.hip)
        int64_t n_chains = 0, n_seeds = 0, nseq = 0, n_redo = 0;
        int64_t counts[kChainCounts] = {};   // bwams_debug_chain_counts: of the last bwams_chain_run / _run_ert
        int64_t lane_counts[2] = {};         // bwams_debug_chain_lane_counts: reads of the lane tier, those that gave the leaf form up
        bool ran = false;                    // ... there was one (bwams_chain_upload clears it)
    } ch;
    struct ExtStage {                        // chain -> alignment regions
        DevBuf<bwams_alnreg_t> regs; DevBuf<uint32_t> srt; DevBuf<int32_t> state, cur, lim;
        DevBuf<> rmax;                       // 2 int64 per chain
        DevBuf<> cnt;                        // 6 int32 rows of task sizes
        DevBuf<> ewide, eoffs;               // 6 int64 rows (sizes, then offsets); mem_flt_chained_seeds borrows them
        DevBuf<> kreg;                       // 32 bytes per seed (ext_aln.hip)
        DevBuf<bwams_seqpair_t> lpairs, rpairs, retry; DevBuf<uint8_t> lref, lqer, rref, rqer;
        DevBuf<> lsrc, rsrc;                 // in place (bwams_extend_run): int64 {query, target} start offsets per task instead of copied bytes
        DevBuf<int32_t> req_list, rtask;     // bwams_extend_run: the slots requested for the next build (appended by whoever requests); per slot its right task
        int64_t n_left = 0, n_right = 0, lref_b = 0, lqer_b = 0, rref_b = 0, rqer_b = 0, n_retry_left = 0, n_retry_right = 0, n_rounds = 0;
        bool tasks_inplace = false;
    } ext;
    struct DedupStage {                      // mem_sort_dedup_patch, mem_pestat's keys
        DevBuf<bwams_alnreg_t> regs, out; DevBuf<int32_t> ord, nout, light;
        DevBuf<> srt;                        // dedup_sortrec_bytes()
        DevBuf<> eh;                         // int2 (h, e) rows: lanes and waves x (longest read + 2)
        DevBuf<> wide;                       // 2 int64 rows of nseq + 1 (widen2), the first scanned
        DevBuf<int64_t> off; DevBuf<unsigned long long> pe_keys, pe_keys2;
        DevBuf<unsigned long long> cnt;      // kDedupCounts words, written only when a run counts (BWAMS_DEDUP_COUNT=1)
        int64_t counts[kDedupCounts] = {};   // ... of the last run
        int64_t n_final = 0; bool counted = false;
    } dd;
    struct PairStage {                       // mate rescue + mem_mark_primary_se + mem_pair
        DevBuf<int32_t> na, anchor, slot, task, tl1, ord, z, nfin, npri, nsw; DevBuf<int64_t> wide, trb, owide, ooff;
        DevBuf<> offs;                       // int64 rows of nseq + 1: aoff | ooff
        DevBuf<> twide, toffs;               // 3 int64 rows of 4 * n_slots + 1
        DevBuf<bwams_seqpair_t> pairs; DevBuf<uint8_t> tref, tqer, full;
        DevBuf<> aln;                        // 7 int32 per task (launch_ksw's output)
        DevBuf<bwams_alnreg_t> pool, out;
        DevBuf<> srt;                        // 24-byte sort records (pair.hip)
        DevBuf<bwams_pair_t> res;
        DevBuf<unsigned long long> cnt;      // kPairCounts words, written only when a run counts (BWAMS_PAIR_COUNT=1)
        int64_t counts[kPairCounts] = {};    // ... of the last run
        int64_t total = 0, tasks = 0, redone = 0; bool single = false, counted = false;
    } pr;
    struct EmfRegStage {                     // mem_perfect2reg (+ mg_*: its merge into the final regions)
        DevBuf<int64_t> wide, off, ooff, mg_wide, mg_off;
        DevBuf<> scr;                        // emfregs_scratch_bytes()
        DevBuf<int32_t> n; DevBuf<uint8_t> rev; DevBuf<bwams_alnreg_t> out, mg_out;
        int64_t total = 0, nseq = 0;
    } er;
    struct AlnStage {                        // mem_reg2aln
        DevBuf<int64_t> need, off; DevBuf<int32_t> cls; DevBuf<uint8_t> scr, only;
        DevBuf<> list;                       // 4 int32 class lists of n + 1
        DevBuf<bwams_aln_t> rec;
        DevBuf<> wide, offs;                 // 2 int64 rows of n + 1: CIGAR operations | MD bytes
        DevBuf<uint32_t> cig; DevBuf<char> md; DevBuf<unsigned long long> cnt;
        int64_t n = 0, ncig = 0, nmd = 0; int source = 0;
    } al;
    struct SamStage {                        // SAM text
        DevBuf<char> names, qual, comm, out; DevBuf<int64_t> noff, coff, len, off; DevBuf<int32_t> mapq; DevBuf<double> logtab;
        DevBuf<> bad;                        // 8 words: unsigned flags at 0 and 2, bwams_reg2aln_run_sam's int64 sum at 1
        int64_t bytes = 0, nseq = 0, nregs = 0;
        int64_t merged_n = -1;               // >= 0: out / off hold that many reads' text merged from two runs (bwams_process_chunk_smart)
        bool has_qual = false, has_comm = false, log_ok = false;
    } sm;
    struct BamStage {                        // BAM records of the SAM text (bwams_bam_run) or uploaded (bwams_bam_upload)
        DevBuf<int64_t> size, roff, off; DevBuf<uint8_t> out; DevBuf<unsigned long long> bad;
        int64_t bytes = 0, nrec = 0, nseq = 0;
        uint32_t nref = 0;                   // refIDs lie in [-1, nref): the index's sequences, or what bwams_bam_upload found
    } bm;
    struct BamSortStage {                    // the records sorted (bwams_bam_sort)
        DevBuf<uint8_t> out; DevBuf<bwams_bam_coord_t> coord, coord0; DevBuf<uint64_t> keys, keys2; DevBuf<uint32_t> idx, idx2;
        DevBuf<int64_t> size, off;
        int64_t bytes = 0, nrec = 0;
    } bs;
    struct MarkdupStage {
        MdTemplates t;                       // templates and ends of the current records (bwams_bam_templates)
        MdDecide decide;                     // the decision's buffers (bwams_bam_markdup)
        DevBuf<uint8_t> dup; DevBuf<unsigned long long> cnt; DevBuf<uint32_t> sorted;
        DevBuf<uint8_t> optical, g_ids; DevBuf<unsigned long long> lib_counts;      // rule 12's marks, the groups table, rule 13's counts
        DevBuf<int64_t> g_off; DevBuf<int32_t> g_ord, g_lib;
        int32_t n_lib = 1;                   // of the last bwams_bam_templates2 (Product::template_locs: t.tloc / t.locs hold the current templates')
    } md;
    DevBuf<int32_t> heavy;        // per read: the wave tier's read list of whichever stage runs (chaining, selection, de-duplication, pairing)
    bwams_mem_opt_t opt{};
    hipEvent_t ev[16] = {};       // 0-1 chain, 2-3 plan+build, 4-5 left, 6-7 right, 8-9 selection (first round each), 10-11 all rounds
    bool ev_ok = false;
    hipStream_t aux[kAuxStreams] = {};   // the stages' concurrent launches (the device's shared set: api_state.hip)
    int aux_device = -1;
    hipEvent_t fork = nullptr, join[kAuxStreams] = {};
};

int get_state(bwams_batch *b, StageState **out);                  // creates b->stages at the first call
int check_opt(const bwams_mem_opt_t *o, const char *who);
int dev_bns(bwams_index *ix, DevBns *out);                         // materialises the one-sequence default
void sw_params(const bwams_mem_opt_t &o, int end_bonus, SwParams *prm);
void sw_params(const bwams_sw_opt_t &o, SwParams *prm);
void launch_widen1(const int32_t *a, int64_t n, int64_t *wide, hipStream_t st);                     // row a of n + 1 as int64, the last 0
void launch_widen2(const int32_t *a, const int32_t *b, int64_t n, int64_t *wide, hipStream_t st);   // rows a | b of n + 1 as int64, the last of each 0
int scan_rows(bwams_batch *b, const int64_t *in, int64_t *out, int rows, int64_t n1);               // exclusive scan of each row of n1
void stage_state_stats(const bwams_batch *b, bwams_stats_t *out);  // timing and counts for bwams_batch_stats (api.hip)

}  // namespace bwams
