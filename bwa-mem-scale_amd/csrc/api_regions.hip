// api_regions.hip — C-ABI entry points of the stages that finish a chunk's regions (include/bwams.h): bwams_dedup_*
// (mem_sort_dedup_patch), bwams_pair_* (mate rescue, mem_mark_primary_se, mem_pair), bwams_emf_regs_* (mem_perfect2reg and its
// merge), bwams_pestat* (mem_pestat) and the test hooks bwams_debug_sort, bwams_debug_ext_regs_upload and
// bwams_debug_dedup_counts and bwams_debug_pair_counts, over dedup.hip, pair.hip, ksw_local.hip and emf_regs.hip.
// No CPU fallback: every entry point runs HIP kernels or returns an error.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

#include <rocprim/rocprim.hpp>

#include "stage_state.h"

using namespace bwams;

extern "C" {
/* ---------------------------------------------- the tail of mem_kernel2_core ---- */

int bwams_dedup_run(bwams_batch_t *b, const bwams_mem_opt_t *opt, int64_t *n_regs) {
    if (!has(b, Product::ext)) {
        set_last_error("bwams_dedup_run: run bwams_extend_run first");
        return BWAMS_ERR_ARG;
    }
    int rc = check_opt(opt, "bwams_dedup_run");
    if (rc) return rc;
    StageState *s = b->stages;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    outdated(b, Product::dedup);
    const int64_t N = s->ch.n_seeds, n1 = s->ch.nseq + 1;
    const int64_t L = b->max_read_len > 1 ? b->max_read_len : 1;
    // strips for the global alignment: as many lanes as 1 GiB of (h, e) rows allows, at most 64 Ki
    int64_t n_lanes = ((int64_t)1 << 30) / ((L + 2) * 8);
    n_lanes = n_lanes > 65536 ? 65536 : n_lanes < 64 ? 64 : n_lanes;
    const int64_t n_waves = (int64_t)b->cu_count * 4, n_waves_small = (int64_t)b->cu_count * 16;
    BWAMS_HIP(s->dd.regs.ensure_n((size_t)(N + 1))); BWAMS_HIP(s->dd.out.ensure_n((size_t)(N + 1))); BWAMS_HIP(s->dd.ord.ensure_n((size_t)(N + 1)));
    BWAMS_HIP(s->dd.srt.ensure(dedup_sortrec_bytes(N)));
    BWAMS_HIP(s->dd.eh.ensure((size_t)(n_lanes + 2 * n_waves + n_waves_small) * (size_t)(L + 2) * 8)); BWAMS_HIP(s->dd.nout.ensure_n((size_t)n1));
    BWAMS_HIP(s->dd.wide.ensure((size_t)n1 * 16)); BWAMS_HIP(s->dd.off.ensure_n((size_t)n1));
    DedupArgs D;
    D.regs = s->dd.regs.p; D.seed_off = s->ch.chain_off.as<int64_t>() + n1; D.enc = b->d_enc.p; D.cum = b->d_cum.p; D.nseq = s->ch.nseq;
    D.ref = b->idx->fmi.ref;
    if ((rc = dev_bns(b->idx, &D.bns))) return rc;
    D.opt = *opt; D.ord = s->dd.ord.p; D.srt = s->dd.srt.p; D.eh = s->dd.eh.as<int2>(); D.eh_lanes = n_lanes; D.max_read_len = (int32_t)L;
    D.n_out = s->dd.nout.p;
    BWAMS_HIP(s->heavy.ensure_n((size_t)n1));
    D.force_seq = knobs().dedup_seq;      // 1: every read through the one-lane form (tests)
    BWAMS_HIP(s->dd.light.ensure_n((size_t)n1));
    D.heavy = s->heavy.p; D.light = s->dd.light.p; D.n_heavy_ctr = &b->d_ctr.p->dedup_heavy; D.ticket = &b->d_ctr.p->dedup_ticket;
    D.n_light_ctr = &b->d_ctr.p->dedup_light; D.ticket2 = &b->d_ctr.p->dedup_ticket2; D.ticket3 = &b->d_ctr.p->dedup_ticket3;
    const bool verbose_dd = knobs().verbose != 0;
    D.dbg = verbose_dd ? b->d_ctr.p->dbg : nullptr;
    if (verbose_dd) BWAMS_HIP(hipMemsetAsync(b->d_ctr.p->dbg, 0, sizeof b->d_ctr.p->dbg, st));
    const bool count_dd = knobs().dedup_count != 0;       // tests: reads per tier, patch alignments per variant (bwams_debug_dedup_counts)
    if (count_dd) {
        BWAMS_HIP(s->dd.cnt.ensure_n((size_t)kDedupCounts));
        BWAMS_HIP(hipMemsetAsync(s->dd.cnt.p, 0, kDedupCounts * sizeof(unsigned long long), st));
    }
    D.cnt = count_dd ? s->dd.cnt.p : nullptr;
    s->dd.counted = false;
    BWAMS_HIP(hipMemsetAsync(&b->d_ctr.p->dedup_heavy, 0, 3 * sizeof(unsigned long long), st));
    BWAMS_HIP(hipMemsetAsync(&b->d_ctr.p->dedup_ticket2, 0, 2 * sizeof(unsigned long long), st));
    BWAMS_HIP(hipEventRecord(s->ev[12], st));
    // work on a copy: bwams_extend_fetch stays valid
    if (N) BWAMS_HIP(hipMemcpyAsync(D.regs, s->ext.regs.p, (size_t)N * sizeof(bwams_alnreg_t), hipMemcpyDeviceToDevice, st));
    BWAMS_HIP(hipMemsetAsync(D.n_out, 0, (size_t)n1 * 4, st));
    if (launch_dedup(D, n_lanes, n_waves, n_waves_small, st, s->aux[0], s->aux[1], s->aux[2], s->fork, s->join[0], s->join[1], s->join[2])) {
        set_last_error("bwams_dedup_run: stream fork/join failed");
        return BWAMS_ERR_DEVICE;
    }
    int64_t total = 0;
    if (s->ch.nseq > 0) {
        launch_widen2(D.n_out, D.n_out, s->ch.nseq, s->dd.wide.as<int64_t>(), st);
        if ((rc = scan_rows(b, s->dd.wide.as<int64_t>(), s->dd.off.p, 1, n1))) return rc;
        launch_dedup_gather(D, s->dd.off.p, s->dd.out.p, st);
        BWAMS_HIP(hipMemcpyAsync(&total, s->dd.off.p + s->ch.nseq, 8, hipMemcpyDeviceToHost, st));
    } else {
        BWAMS_HIP(hipMemsetAsync(s->dd.off.p, 0, 8, st));          // an empty chunk: reg_off = {0}
    }
    BWAMS_HIP(hipEventRecord(s->ev[13], st));
    if (verbose_dd) BWAMS_HIP(hipMemcpyAsync(b->h_ctr.p->dbg, b->d_ctr.p->dbg, sizeof b->d_ctr.p->dbg, hipMemcpyDeviceToHost, st));
    unsigned long long cnt_dd[kDedupCounts] = {};
    if (count_dd) BWAMS_HIP(hipMemcpyAsync(cnt_dd, s->dd.cnt.p, sizeof cnt_dd, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    for (int i = 0; i < kDedupCounts; ++i) s->dd.counts[i] = (int64_t)cnt_dd[i];
    s->dd.counted = count_dd;
    if (verbose_dd) {
        const unsigned long long *d = b->h_ctr.p->dbg;
        fprintf(stderr, "[bwams_dedup_run] largest wave instance: %llu reads, %llu slots, %llu alive; Mcycles: load %.1f sort(end) %.1f pairs %.1f reload %.1f sort(score) %.1f store %.1f; "
                        "longest read: sort(end) %.2f pairs %.2f sort(score) %.2f, whole %.2f (read %llu, %llu regions; %llu patch alignments in %.2f, %llu scan trips); all reads: %llu patch alignments in %.1f\n",
                d[0], d[1], d[2], d[3] / 1e6, d[4] / 1e6, d[5] / 1e6, d[6] / 1e6, d[7] / 1e6, d[8] / 1e6, d[9] / 1e6, d[10] / 1e6, d[11] / 1e6, d[12] / 1e6, d[13], d[14],
                d[15], d[16] / 1e6, d[17], d[18], d[19] / 1e6);
    }
    s->dd.n_final = total;
    if (n_regs) *n_regs = total;
    produced(b, Product::dedup);
    return BWAMS_OK;
}

int bwams_dedup_fetch(bwams_batch_t *b, bwams_alnreg_t *regs, int64_t reg_cap, int64_t *reg_off) {
    if (!has(b, Product::dedup)) {
        set_last_error("bwams_dedup_fetch: run bwams_dedup_run first");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    if (s->dd.n_final > reg_cap) return BWAMS_ERR_CAPACITY;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    if (s->dd.n_final) BWAMS_HIP(hipMemcpyAsync(regs, s->dd.out.p, (size_t)s->dd.n_final * sizeof(bwams_alnreg_t), hipMemcpyDeviceToHost, st));
    if (reg_off) BWAMS_HIP(hipMemcpyAsync(reg_off, s->dd.off.p, (size_t)(s->ch.nseq + 1) * 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    return BWAMS_OK;
}

/* Test hook: what the last bwams_dedup_run counted (include/bwams.h). */
int bwams_debug_dedup_counts(bwams_batch_t *b, int64_t counts[14]) {
    static_assert(kDedupCounts == 14, "include/bwams.h documents 14 counters");
    if (!counts || !has(b, Product::dedup) || !b->stages->dd.counted) {
        set_last_error("bwams_debug_dedup_counts: no bwams_dedup_run with BWAMS_DEDUP_COUNT=1 on this batch");
        return BWAMS_ERR_ARG;
    }
    for (int i = 0; i < kDedupCounts; ++i) counts[i] = b->stages->dd.counts[i];
    return BWAMS_OK;
}

/* Test hook: caller-given regions take the place of the extension stage's regions (include/bwams.h).  Refused: what would make a
 * kernel read outside the reads or the text, and the values on which mem_patch_reg itself divides by zero or converts NaN to int. */
int bwams_debug_ext_regs_upload(bwams_batch_t *b, const bwams_alnreg_t *regs, int64_t n_regs, const int64_t *reg_off, int64_t n_reads) {
    if (!b || n_regs < 0 || n_reads < 0 || !reg_off || (n_regs && !regs)) return BWAMS_ERR_ARG;
    if (!has(b, Product::reads) || n_reads != b->nseq) {
        set_last_error("bwams_debug_ext_regs_upload: n_reads is not the number of reads of the last bwams_seed_upload");
        return BWAMS_ERR_ARG;
    }
    if (reg_off[0] != 0 || reg_off[n_reads] != n_regs) {
        set_last_error("bwams_debug_ext_regs_upload: reg_off must run from 0 to n_regs");
        return BWAMS_ERR_ARG;
    }
    for (int64_t r = 0; r < n_reads; ++r)
        if (reg_off[r + 1] < reg_off[r]) {
            set_last_error("bwams_debug_ext_regs_upload: reg_off decreases at read " + std::to_string(r));
            return BWAMS_ERR_ARG;
        }
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    DevBns bns;
    int rc = dev_bns(b->idx, &bns);
    if (rc) return rc;
    std::vector<int64_t> cum((size_t)n_reads + 1);
    BWAMS_HIP(hipMemcpyAsync(cum.data(), b->d_cum.p, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    for (int64_t r = 0; r < n_reads; ++r) {
        const int64_t len = cum[(size_t)r + 1] - cum[(size_t)r];
        for (int64_t k = reg_off[r]; k < reg_off[r + 1]; ++k) {
            const bwams_alnreg_t &a = regs[k];
            const char *why = nullptr;
            if (a.rid < -1 || a.rid >= bns.n_seqs) why = " has rid outside [-1, number of sequences)";
            else if (a.qe <= a.qb) continue;                   // a purged slot: dropped before anything reads it
            else if (a.qb < 0 || a.qe > len) why = " has a query span outside its read";
            else if (a.rb < 0 || a.re > 2 * bns.l_pac || a.re <= a.rb) why = " has a reference span that is empty or outside the text";
            else if (a.score < 1) why = " has a score below 1";
            if (why) {
                set_last_error("bwams_debug_ext_regs_upload: region " + std::to_string(k) + why);
                return BWAMS_ERR_ARG;
            }
        }
    }
    StageState *s;
    if ((rc = get_state(b, &s))) return rc;
    // the chains and seeds of an earlier run no longer belong to these regions: nothing may extend them again
    outdated(b, Product::chains);
    outdated(b, Product::er);          // beside the graph, as before: regions given by hand are not to meet mem_perfect2reg's of an earlier run
    const int64_t n1 = n_reads + 1;
    BWAMS_HIP(s->ext.regs.ensure_n((size_t)n_regs + 1)); BWAMS_HIP(s->ch.chain_off.ensure((size_t)n1 * 16));
    BWAMS_HIP(s->ch.seeds.ensure_n((size_t)n_regs + 1));     // bwams_extend_fetch reads a word per region from here: zeros
    BWAMS_HIP(hipMemsetAsync(s->ch.seeds.p, 0, ((size_t)n_regs + 1) * sizeof(bwams_chain_seed_t), st));
    if (n_regs) BWAMS_HIP(hipMemcpyAsync(s->ext.regs.p, regs, (size_t)n_regs * sizeof(bwams_alnreg_t), hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipMemsetAsync(s->ch.chain_off.p, 0, (size_t)n1 * 8, st));
    BWAMS_HIP(hipMemcpyAsync(s->ch.chain_off.as<int64_t>() + n1, reg_off, (size_t)n1 * 8, hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    s->ch.n_chains = 0; s->ch.n_seeds = n_regs; s->ch.nseq = n_reads;
    s->ext.n_left = s->ext.n_right = 0; s->ext.tasks_inplace = true;      // no task lists belong to these regions: bwams_extend_tasks_fetch refuses
    produced(b, Product::ext);
    return BWAMS_OK;
}

/* ------------------------------------------------- mate rescue, mem_mark_primary_se, mem_pair ---- */

static int pair_run_impl(bwams_batch_t *b, const bwams_mem_opt_t *opt, const bwams_pestat_t pes[4], int64_t id_base, int32_t flags,
                         int primary5_T, int no_pairing, int64_t *n_regs, int64_t *n_tasks);

int bwams_pair_run(bwams_batch_t *b, const bwams_mem_opt_t *opt, const bwams_pestat_t pes[4], int64_t id_base, int32_t flags,
                   int64_t *n_regs, int64_t *n_tasks) {
    return pair_run_impl(b, opt, pes, id_base, flags, -1, 0, n_regs, n_tasks);
}

int bwams_pair_run_sam(bwams_batch_t *b, const bwams_mem_opt_t *opt, const bwams_sam_opt_t *sam_opt, const bwams_pestat_t pes[4],
                       int64_t id_base, int32_t flags, int64_t *n_regs, int64_t *n_tasks) {
    if (!sam_opt) return pair_run_impl(b, opt, pes, id_base, flags, -1, 0, n_regs, n_tasks);
    if (sam_opt->T < 0) {
        set_last_error("bwams_pair_run_sam: T must not be negative");
        return BWAMS_ERR_ARG;
    }
    if (sam_opt->flag & BWAMS_MEM_F_NO_RESCUE) flags |= BWAMS_PAIR_NO_RESCUE;
    return pair_run_impl(b, opt, pes, id_base, flags, (sam_opt->flag & BWAMS_MEM_F_PRIMARY5) ? sam_opt->T : -1,
                         (sam_opt->flag & BWAMS_MEM_F_NOPAIRING) != 0, n_regs, n_tasks);
}

static int pair_run_impl(bwams_batch_t *b, const bwams_mem_opt_t *opt, const bwams_pestat_t pes[4], int64_t id_base, int32_t flags,
                         int primary5_T, int no_pairing, int64_t *n_regs, int64_t *n_tasks) {
    const int single_end = (flags & BWAMS_PAIR_SINGLE_END) != 0;
    const int no_rescue = (flags & BWAMS_PAIR_NO_RESCUE) || single_end, use_ert = (flags & BWAMS_PAIR_USE_ERT) != 0;
    static const bwams_pestat_t no_pes[4] = {{0, 0, 1, 0, 0., 0.}, {0, 0, 1, 0, 0., 0.}, {0, 0, 1, 0, 0., 0.}, {0, 0, 1, 0, 0., 0.}};
    if (single_end && !pes) pes = no_pes;
    if (!has(b, Product::dedup)) {
        set_last_error("bwams_pair_run: run bwams_dedup_run first");
        return BWAMS_ERR_ARG;
    }
    int rc = check_opt(opt, "bwams_pair_run");
    if (rc) return rc;
    StageState *s = b->stages;
    if (!pes || (!single_end && (s->ch.nseq & 1))) {
        set_last_error("bwams_pair_run: needs the insert-size statistics and an even number of reads (ends of pair p at 2p, 2p + 1)");
        return BWAMS_ERR_ARG;
    }
    int tmax = 1;
    for (int k = 0; k < 4; ++k)
        if (!pes[k].failed && pes[k].high - pes[k].low + b->max_read_len > tmax) tmax = pes[k].high - pes[k].low + b->max_read_len;
    if (!no_rescue && (b->max_read_len > 512 || tmax > kKswMaxTarget)) {
        set_last_error("bwams_pair_run: mate rescue needs reads of at most 512 bases and windows (high - low + read length) of at most 20000");
        return BWAMS_ERR_UNSUPPORTED;
    }
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    outdated(b, Product::pair);
    const int64_t nseq = s->ch.nseq, n1 = nseq + 1;
    BWAMS_HIP(s->pr.na.ensure_n((size_t)n1)); BWAMS_HIP(s->pr.wide.ensure_n((size_t)n1)); BWAMS_HIP(s->pr.offs.ensure((size_t)n1 * 16));
    BWAMS_HIP(s->pr.nfin.ensure_n((size_t)n1)); BWAMS_HIP(s->pr.npri.ensure_n((size_t)n1)); BWAMS_HIP(s->pr.nsw.ensure_n((size_t)n1));
    BWAMS_HIP(s->pr.full.ensure_n((size_t)n1)); BWAMS_HIP(s->pr.owide.ensure_n((size_t)n1)); BWAMS_HIP(s->pr.ooff.ensure_n((size_t)n1));
    BWAMS_HIP(s->pr.res.ensure_n((size_t)(nseq / 2 + 1)));
    PairArgs A;
    A.regs = s->dd.out.p; A.reg_off = s->dd.off.p; A.enc = b->d_enc.p; A.cum = b->d_cum.p; A.nseq = nseq; A.ref = b->idx->fmi.ref;
    if ((rc = dev_bns(b->idx, &A.bns))) return rc;
    A.opt = *opt;
    for (int k = 0; k < 4; ++k) A.pes[k] = pes[k];
    A.id_base = id_base; A.no_rescue = no_rescue ? 1 : 0; A.pass = 0;
    A.drop_plan = knobs().pair_drop_plan;                 // test knob: exercise the second pass
    A.use_ert = use_ert ? 1 : 0; A.single_end = single_end; A.no_pairing = no_pairing; A.primary5_T = primary5_T; A.na = s->pr.na.p;
    int64_t *aoff = s->pr.offs.as<int64_t>(), *ooff = aoff + n1;
    A.aoff = aoff; A.ooff = ooff; A.n_fin = s->pr.nfin.p; A.n_pri = s->pr.npri.p; A.n_sw = s->pr.nsw.p; A.full = s->pr.full.p; A.ctr = b->d_ctr.p;
    A.anchor = nullptr; A.slot_read = nullptr; A.n_slots = 0; A.task = nullptr; A.trb = nullptr; A.tl1 = nullptr; A.aln = nullptr; A.pool = nullptr;
    A.ord = nullptr; A.zbuf = nullptr; A.srt = nullptr; A.heavy = nullptr;
    const bool count_pr = knobs().pair_count != 0;        // tests: reads per route, sorts per path (bwams_debug_pair_counts)
    if (count_pr) {
        BWAMS_HIP(s->pr.cnt.ensure_n((size_t)kPairCounts));
        BWAMS_HIP(hipMemsetAsync(s->pr.cnt.p, 0, kPairCounts * sizeof(unsigned long long), st));
    }
    A.cnt = count_pr ? s->pr.cnt.p : nullptr;
    s->pr.counted = false;
    BWAMS_HIP(hipEventRecord(s->ev[14], st));
    BWAMS_HIP(hipMemsetAsync(A.full, 0, (size_t)n1, st));
    BWAMS_HIP(hipMemsetAsync(&b->d_ctr.p->pair_full, 0, 2 * sizeof(unsigned long long), st));
    // anchors per read, pool capacities
    launch_pair_count(A, s->pr.wide.p, st);
    if ((rc = scan_rows(b, s->pr.wide.p, aoff, 1, n1))) return rc;
    launch_pair_cap(A, s->pr.wide.p, st);
    if ((rc = scan_rows(b, s->pr.wide.p, ooff, 1, n1))) return rc;
    int64_t n_slots = 0, n_pool = 0;
    BWAMS_HIP(hipMemcpyAsync(&n_slots, aoff + nseq, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipMemcpyAsync(&n_pool, ooff + nseq, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    A.n_slots = n_slots;
    const int64_t E1 = 4 * n_slots + 1;
    BWAMS_HIP(s->pr.anchor.ensure_n((size_t)(n_slots + 1))); BWAMS_HIP(s->pr.slot.ensure_n((size_t)(n_slots + 1)));
    BWAMS_HIP(s->pr.task.ensure_n((size_t)E1)); BWAMS_HIP(s->pr.trb.ensure_n((size_t)E1)); BWAMS_HIP(s->pr.tl1.ensure_n((size_t)E1));
    BWAMS_HIP(s->pr.twide.ensure((size_t)E1 * 24)); BWAMS_HIP(s->pr.toffs.ensure((size_t)E1 * 24));
    BWAMS_HIP(s->pr.pool.ensure_n((size_t)(n_pool + 1))); BWAMS_HIP(s->pr.ord.ensure_n((size_t)(n_pool + 1)));
    BWAMS_HIP(s->pr.z.ensure_n((size_t)(n_pool + 1))); BWAMS_HIP(s->pr.srt.ensure((size_t)(n_pool + 1) * 24));
    A.anchor = s->pr.anchor.p; A.slot_read = s->pr.slot.p; A.task = s->pr.task.p; A.trb = s->pr.trb.p; A.tl1 = s->pr.tl1.p; A.pool = s->pr.pool.p;
    A.ord = s->pr.ord.p; A.zbuf = s->pr.z.p; A.srt = s->pr.srt.p;
    const int pr_trace = knobs().trace_pair;     // debugging aid: a synchronisation and a line per launch
#define PR_TRACE(msg) do { if (pr_trace) { BWAMS_HIP(hipStreamSynchronize(st)); fprintf(stderr, "[bwams_pair_run] %s\n", msg); } } while (0)
    PR_TRACE("count / cap done");
    launch_pair_slots(A, st);
    PR_TRACE("slots done");
    BWAMS_HIP(s->heavy.ensure_n((size_t)n1));
    A.heavy = s->heavy.p;
    SwParams prm;
    sw_params(*opt, 0, &prm);
    s->pr.tasks = 0; s->pr.redone = 0;
    for (int pass = 0; pass < 2; ++pass) {
        A.pass = pass;
        int64_t tot[3] = {0, 0, 0};
        launch_pair_plan(A, s->pr.twide.as<int64_t>(), st);
        PR_TRACE("plan done");
        if ((rc = scan_rows(b, s->pr.twide.as<int64_t>(), s->pr.toffs.as<int64_t>(), 3, E1))) return rc;
        for (int r = 0; r < 3; ++r) BWAMS_HIP(hipMemcpyAsync(&tot[r], s->pr.toffs.as<int64_t>() + r * E1 + (E1 - 1), 8, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipStreamSynchronize(st));
        if (tot[1] >= ((int64_t)1 << 31) || tot[2] >= ((int64_t)1 << 31)) {
            set_last_error("bwams_pair_run: rescue windows exceed the 31-bit offsets of SeqPair; use smaller chunks");
            return BWAMS_ERR_CAPACITY;
        }
        BWAMS_HIP(s->pr.pairs.ensure_n((size_t)(tot[0] + 1))); BWAMS_HIP(s->pr.tref.ensure_n((size_t)tot[1] + 64));
        BWAMS_HIP(s->pr.tqer.ensure_n((size_t)tot[2] + 64)); BWAMS_HIP(s->pr.aln.ensure((size_t)(tot[0] + 1) * 28));
        A.aln = s->pr.aln.as<int32_t>();
        launch_pair_build(A, s->pr.toffs.as<int64_t>(), s->pr.pairs.p, s->pr.tref.p, s->pr.tqer.p, b->cu_count, st);
        PR_TRACE("build done");
        if (tot[0] > 0 && launch_ksw(s->pr.pairs.p, tot[0], s->pr.tref.p, s->pr.tqer.p, prm,
                                     ((b->max_read_len + 15) / 16) * 16, tmax, s->pr.aln.p, b->d_ctr.p, b->cu_count, st)) {
            set_last_error("bwams_pair_run: rescue window too long for the local-SW kernel");
            return BWAMS_ERR_UNSUPPORTED;
        }
        PR_TRACE("ksw done");
        BWAMS_HIP(hipMemsetAsync(&b->d_ctr.p->pair_heavy, 0, 2 * sizeof(unsigned long long), st));
        launch_pair_post(A, b->cu_count, st);
#ifdef BWAMS_PAIRDBG
        if (knobs().verbose) {
            unsigned long long d[80];
            BWAMS_HIP(hipStreamSynchronize(st));
            BWAMS_HIP(hipMemcpy(d, b->d_ctr.p->dbg, sizeof d, hipMemcpyDeviceToHost));
            fprintf(stderr, "[pair_post_wave] reads %llu (mean %.0f regions at the end, %.1f anchors, %.1f rescues), %.3f ms of a wave per read (longest %.3f ms); sorts %llu = %.1f per read, %.3f ms per read; "
                    "with equal keys %llu, %.3f ms per read in them\n", d[20], d[20] ? (double)d[27] / d[20] : 0.0, d[20] ? (double)d[28] / d[20] : 0.0, d[20] ? (double)d[29] / d[20] : 0.0,
                    d[20] ? d[24] * 1e-5 / d[20] : 0.0, d[25] * 1e-5, d[21], d[20] ? (double)d[21] / d[20] : 0.0, d[20] ? d[26] * 1e-5 / d[20] : 0.0, d[22], d[20] ? d[23] * 1e-5 / d[20] : 0.0);
            BWAMS_HIP(hipMemsetAsync(b->d_ctr.p->dbg + 20, 0, 10 * sizeof(unsigned long long), st));
        }
#endif
        PR_TRACE("post done");
        s->pr.tasks += tot[0];
        unsigned long long flags[2] = {0, 0};
        BWAMS_HIP(hipMemcpyAsync(flags, &b->d_ctr.p->pair_full, sizeof flags, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipStreamSynchronize(st));
        if (flags[1]) {
            set_last_error("bwams_pair_run: internal error, a rescue alignment was missing in the second pass");
            return BWAMS_ERR_DEVICE;
        }
        if (pass == 0) s->pr.redone = (int64_t)flags[0];
        if (pass == 1 || flags[0] == 0) break;
    }
    // mem_mark_primary_se of every read, regions in final order, then mem_pair
    BWAMS_HIP(hipMemsetAsync(&b->d_ctr.p->pair_heavy, 0, 2 * sizeof(unsigned long long), st));
    BWAMS_HIP(hipMemsetAsync(&b->d_ctr.p->pair_ticket2, 0, sizeof(unsigned long long), st));
    launch_pair_mark(A, b->cu_count, st);
    PR_TRACE("mark done");
    launch_pair_widen(A, s->pr.owide.p, st);
    if ((rc = scan_rows(b, s->pr.owide.p, s->pr.ooff.p, 1, n1))) return rc;
    int64_t total = 0;
    BWAMS_HIP(hipMemcpyAsync(&total, s->pr.ooff.p + nseq, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(s->pr.out.ensure_n((size_t)(total + 1)));
    launch_pair_gather(A, s->pr.ooff.p, s->pr.out.p, st);
    PR_TRACE("gather done");
    launch_pair_reorder5(A, s->pr.ooff.p, s->pr.out.p, st);
    PR_TRACE("reorder5 done");
    if (!single_end) launch_pair_pair(A, s->pr.ooff.p, s->pr.out.p, s->pr.res.p, st);
    PR_TRACE("pair done");
    BWAMS_HIP(hipEventRecord(s->ev[15], st));
    unsigned long long cnt_pr[kPairCounts] = {};
    if (count_pr) BWAMS_HIP(hipMemcpyAsync(cnt_pr, s->pr.cnt.p, sizeof cnt_pr, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    for (int i = 0; i < kPairCounts; ++i) s->pr.counts[i] = (int64_t)cnt_pr[i];
    s->pr.counted = count_pr;
    s->pr.total = total;
    s->pr.single = single_end != 0;
    if (n_regs) *n_regs = total;
    if (n_tasks) *n_tasks = s->pr.tasks;
    produced(b, Product::pair);
    return BWAMS_OK;
}

int bwams_pair_fetch(bwams_batch_t *b, bwams_alnreg_t *regs, int64_t reg_cap, int64_t *reg_off, bwams_pair_t *pairs) {
    if (!has(b, Product::pair)) {
        set_last_error("bwams_pair_fetch: run bwams_pair_run first");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    if (s->pr.total > reg_cap) return BWAMS_ERR_CAPACITY;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    if (regs && s->pr.total) BWAMS_HIP(hipMemcpyAsync(regs, s->pr.out.p, (size_t)s->pr.total * sizeof(bwams_alnreg_t), hipMemcpyDeviceToHost, st));
    if (reg_off) BWAMS_HIP(hipMemcpyAsync(reg_off, s->pr.ooff.p, (size_t)(s->ch.nseq + 1) * 8, hipMemcpyDeviceToHost, st));
    if (pairs && s->ch.nseq > 1 && !s->pr.single) BWAMS_HIP(hipMemcpyAsync(pairs, s->pr.res.p, (size_t)(s->ch.nseq / 2) * sizeof(bwams_pair_t), hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    return BWAMS_OK;
}

/* Test hook: what the last bwams_pair_run counted (include/bwams.h). */
int bwams_debug_pair_counts(bwams_batch_t *b, int64_t counts[15]) {
    static_assert(kPairCounts == 15, "include/bwams.h documents 15 counters");
    if (!counts || !has(b, Product::pair) || !b->stages->pr.counted) {
        set_last_error("bwams_debug_pair_counts: no bwams_pair_run with BWAMS_PAIR_COUNT=1 on this batch");
        return BWAMS_ERR_ARG;
    }
    for (int i = 0; i < kPairCounts; ++i) counts[i] = b->stages->pr.counts[i];
    return BWAMS_OK;
}

/* ------------------------------------------------------------ mem_perfect2reg ---- */

int bwams_emf_regs_run(bwams_batch_t *b, bwams_emf_t *e, const bwams_mem_opt_t *opt, int64_t *n_regs) {
    if (!e || !has(b, Product::probe)) {
        set_last_error("bwams_emf_regs_run: run bwams_emf_run first");
        return BWAMS_ERR_ARG;
    }
    int rc = check_opt(opt, "bwams_emf_regs_run");
    if (rc) return rc;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    StageState *s;
    if ((rc = get_state(b, &s))) return rc;
    outdated(b, Product::er);
    hipStream_t st = b->stream;
    const int64_t nseq = b->nseq, n1 = nseq + 1;
    BWAMS_HIP(s->er.wide.ensure_n((size_t)n1)); BWAMS_HIP(s->er.off.ensure_n((size_t)n1)); BWAMS_HIP(s->er.ooff.ensure_n((size_t)n1));
    BWAMS_HIP(s->er.n.ensure_n((size_t)n1)); BWAMS_HIP(s->er.rev.ensure_n((size_t)n1));
    EmfRegArgs A;
    A.t = e->t; A.perfect = b->emf.d_emf_out.p; A.code = b->emf.d_emf_code.p; A.enc = b->d_enc.p; A.cum = b->d_cum.p; A.nseq = nseq;
    if ((rc = dev_bns(b->idx, &A.bns))) return rc;
    A.opt = *opt; A.scratch = nullptr;
    launch_emfregs_count(A, s->er.wide.p, st);
    if ((rc = scan_rows(b, s->er.wide.p, s->er.off.p, 1, n1))) return rc;
    int64_t n_scr = 0, total = 0;
    BWAMS_HIP(hipMemcpyAsync(&n_scr, s->er.off.p + nseq, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(s->er.scr.ensure(emfregs_scratch_bytes(n_scr)));
    A.scratch = s->er.scr.p;
    launch_emfregs_fill(A, s->er.off.p, s->er.n.p, s->er.rev.p, s->er.wide.p, st);
    if ((rc = scan_rows(b, s->er.wide.p, s->er.ooff.p, 1, n1))) return rc;
    BWAMS_HIP(hipMemcpyAsync(&total, s->er.ooff.p + nseq, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(s->er.out.ensure_n((size_t)(total + 1)));
    launch_emfregs_emit(A, s->er.off.p, s->er.n.p, s->er.ooff.p, s->er.out.p, st);
    BWAMS_HIP(hipGetLastError());
    s->er.total = total; s->er.nseq = nseq;
    if (n_regs) *n_regs = total;
    produced(b, Product::er);
    return BWAMS_OK;
}

int bwams_emf_regs_merge(bwams_batch_t *b, int64_t *n_regs) {
    if (!has(b, Product::er, Product::dedup)) {
        set_last_error("bwams_emf_regs_merge: run bwams_emf_regs_run and bwams_dedup_run of this chunk first");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    outdated(b, Product::dedup, false);                   // the final regions gain the merged ones where they lie
    outdated(b, Product::er);                             // beside the graph: merged once, a second call would add them again
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    const int64_t nseq = s->ch.nseq, n1 = nseq + 1;
    int rc;
    BWAMS_HIP(s->er.mg_wide.ensure_n((size_t)n1)); BWAMS_HIP(s->er.mg_off.ensure_n((size_t)n1));
    launch_emfregs_merge_count(s->dd.off.p, s->er.ooff.p, nseq, s->er.mg_wide.p, st);
    if ((rc = scan_rows(b, s->er.mg_wide.p, s->er.mg_off.p, 1, n1))) return rc;
    const int64_t total = s->dd.n_final + s->er.total;
    BWAMS_HIP(s->er.mg_out.ensure_n((size_t)(total + 1)));
    launch_emfregs_merge(s->dd.out.p, s->dd.off.p, s->er.out.p, s->er.ooff.p, nseq, s->er.mg_off.p, s->er.mg_out.p, st);
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    std::swap(s->dd.out, s->er.mg_out);
    std::swap(s->dd.off, s->er.mg_off);
    s->dd.n_final = total;
    if (n_regs) *n_regs = total;
    return BWAMS_OK;
}

int bwams_emf_regs_fetch(bwams_batch_t *b, bwams_alnreg_t *regs, int64_t reg_cap, int64_t *reg_off, uint8_t *first_is_rev) {
    if (!has(b, Product::er)) {
        set_last_error("bwams_emf_regs_fetch: run bwams_emf_regs_run first");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    if (s->er.total > reg_cap) return BWAMS_ERR_CAPACITY;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    if (s->er.total) BWAMS_HIP(hipMemcpyAsync(regs, s->er.out.p, (size_t)s->er.total * sizeof(bwams_alnreg_t), hipMemcpyDeviceToHost, st));
    if (reg_off) BWAMS_HIP(hipMemcpyAsync(reg_off, s->er.ooff.p, (size_t)(s->er.nseq + 1) * 8, hipMemcpyDeviceToHost, st));
    if (first_is_rev && s->er.nseq) BWAMS_HIP(hipMemcpyAsync(first_is_rev, s->er.rev.p, (size_t)s->er.nseq, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    return BWAMS_OK;
}

/* ------------------------------------------------------------------ mem_pestat ---- */

// the insert-size keys of the qualifying pairs, sorted: orientation << 60 | insert size
static int pestat_keys(bwams_batch *b, StageState *s, const bwams_mem_opt_t *opt, std::vector<unsigned long long> *keys) {
    hipStream_t st = b->stream;
    const int64_t n_pairs = s->ch.nseq >> 1;
    const int64_t l_pac = (b->idx->fmi.ref_seq_len - 1) / 2;
    keys->assign((size_t)(n_pairs > 0 ? n_pairs : 0), ~0ull);
    if (n_pairs <= 0) return BWAMS_OK;
    BWAMS_HIP(s->dd.pe_keys.ensure_n((size_t)n_pairs)); BWAMS_HIP(s->dd.pe_keys2.ensure_n((size_t)n_pairs));
    launch_pestat(s->dd.out.p, s->dd.off.p, n_pairs, l_pac, *opt, s->dd.pe_keys.p, st);
    if (int rc = with_tmp(b, "bwams_pestat: radix_sort_keys", [&](void *tmp, size_t &tb) {
            return rocprim::radix_sort_keys(tmp, tb, s->dd.pe_keys.p, s->dd.pe_keys2.p, (size_t)n_pairs, 0, 64, st);
        })) return rc;
    BWAMS_HIP(hipMemcpyAsync(keys->data(), s->dd.pe_keys2.p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    size_t k = keys->size();
    while (k > 0 && (*keys)[k - 1] == ~0ull) --k;           // pairs that do not qualify sort last
    keys->resize(k);
    return BWAMS_OK;
}

// the reference's arithmetic over each orientation's sorted insert sizes (bwamem_pair.cpp:111-155), as written
static void pestat_from_sorted(const unsigned long long *keys, size_t n, bwams_pestat_t pes[4]) {
    memset(pes, 0, 4 * sizeof(bwams_pestat_t));
    size_t beg[5] = {0, 0, 0, 0, 0};
    {
        size_t k = 0;
        for (int d = 0; d < 4; ++d) {
            beg[d] = k;
            while (k < n && (int)(keys[k] >> 60) == d) ++k;
        }
        beg[4] = k;
    }
    const unsigned long long mask = (1ull << 60) - 1ull;
    int max = 0;
    for (int d = 0; d < 4; ++d) {
        bwams_pestat_t *r = &pes[d];
        const unsigned long long *q = keys + beg[d];
        const size_t qn = beg[d + 1] - beg[d];
        max = max > (int)qn ? max : (int)qn;
        if (qn < 10) { r->failed = 1; continue; }
        const int p25 = (int)(q[(int)(.25 * qn + .499)] & mask);
        const int p75 = (int)(q[(int)(.75 * qn + .499)] & mask);
        r->low = (int)(p25 - 2.0 * (p75 - p25) + .499);
        if (r->low < 1) r->low = 1;
        r->high = (int)(p75 + 2.0 * (p75 - p25) + .499);
        int x = 0;
        size_t k;
        for (k = 0, r->avg = 0; k < qn; ++k) {
            const uint64_t v = q[k] & mask;
            if (v >= (uint64_t)r->low && v <= (uint64_t)r->high) r->avg += v, ++x;
        }
        r->avg /= x;
        for (k = 0, r->std = 0; k < qn; ++k) {
            const uint64_t v = q[k] & mask;
            if (v >= (uint64_t)r->low && v <= (uint64_t)r->high) r->std += (v - r->avg) * (v - r->avg);
        }
        r->std = sqrt(r->std / x);
        r->low = (int)(p25 - 3.0 * (p75 - p25) + .499);
        r->high = (int)(p75 + 3.0 * (p75 - p25) + .499);
        if (r->low > r->avg - 4.0 * r->std) r->low = (int)(r->avg - 4.0 * r->std + .499);
        if (r->high < r->avg + 4.0 * r->std) r->high = (int)(r->avg + 4.0 * r->std + .499);
        if (r->low < 1) r->low = 1;
    }
    for (int d = 0; d < 4; ++d)
        if (pes[d].failed == 0 && (double)(beg[d + 1] - beg[d]) < max * 0.05) pes[d].failed = 1;
}

int bwams_pestat(bwams_batch_t *b, const bwams_mem_opt_t *opt, bwams_pestat_t pes[4]) {
    if (!has(b, Product::dedup) || !pes) {
        set_last_error("bwams_pestat: run bwams_dedup_run first");
        return BWAMS_ERR_ARG;
    }
    int rc = check_opt(opt, "bwams_pestat");
    if (rc) return rc;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    std::vector<unsigned long long> keys;
    if ((rc = pestat_keys(b, b->stages, opt, &keys))) return rc;
    pestat_from_sorted(keys.data(), keys.size(), pes);
    return BWAMS_OK;
}

int bwams_pestat_keys(bwams_batch_t *b, const bwams_mem_opt_t *opt, uint64_t *keys_out, int64_t cap, int64_t *n_keys) {
    if (!has(b, Product::dedup) || !n_keys) {
        set_last_error("bwams_pestat_keys: run bwams_dedup_run first");
        return BWAMS_ERR_ARG;
    }
    int rc = check_opt(opt, "bwams_pestat_keys");
    if (rc) return rc;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    std::vector<unsigned long long> keys;
    if ((rc = pestat_keys(b, b->stages, opt, &keys))) return rc;
    *n_keys = (int64_t)keys.size();
    if ((int64_t)keys.size() > cap) return BWAMS_ERR_CAPACITY;
    if (!keys.empty()) memcpy(keys_out, keys.data(), keys.size() * 8);
    return BWAMS_OK;
}

int bwams_pestat_from_keys(const uint64_t *keys_in, int64_t n, bwams_pestat_t pes[4]) {
    if (n < 0 || (n && !keys_in) || !pes) return BWAMS_ERR_ARG;
    std::vector<unsigned long long> keys(keys_in, keys_in + n);
    std::sort(keys.begin(), keys.end());
    pestat_from_sorted(keys.data(), keys.size(), pes);
    return BWAMS_OK;
}

/* Test hook: the device sorts on caller-given keys (order_out[i] = index of the i-th record after the sort).  which:
 * 0 = mem_ars2 (key k), 1 = mem_ars (s descending, k, q), 2 = the chain filter's (k = weight in [0, 2^30), descending).
 * mode: see bwams.h. */
int bwams_debug_sort(bwams_index_t *ix, const int64_t *k, const int32_t *s, const int32_t *q, int32_t n, int32_t which,
                     int32_t mode, int32_t *order_out) {
    if (!ix || n < 0 || (n && (!k || !s || !q || !order_out))) return BWAMS_ERR_ARG;
    if (which == 2)
        for (int32_t i = 0; i < n; ++i)
            if (k[i] < 0 || k[i] >= (1 << 30)) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(ix->device));
    if (which == 2 ? launch_flt_sort_test(k, n, mode, order_out) : launch_sort_test(k, s, q, n, which, mode, order_out)) {
        set_last_error("bwams_debug_sort: n must be at most 2048 (which = 0, 1) or 1024 (which = 2)");
        return BWAMS_ERR_ARG;
    }
    return BWAMS_OK;
}
}  // extern "C"
