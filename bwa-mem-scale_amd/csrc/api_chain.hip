// api_chain.hip — C-ABI entry points of the chaining stage (include/bwams.h): bwams_index_set_contigs, mem_flt_chained_seeds for
// long reads (flt_chained_seeds), the launch sequence both seed sources share (chain_common), bwams_chain_run, _run_ert, _fetch and
// _upload, over chain.hip, seed_sw.hip and ert_chain.hip on the batch's stream.  No CPU fallback: every entry point runs HIP kernels or returns an error.
#include <cstring>
#include <utility>

#include <rocprim/rocprim.hpp>

#include "stage_state.h"

using namespace bwams;

extern "C" {
int bwams_index_set_contigs(bwams_index_t *ix, const bwams_contig_t *contigs, int32_t n_seqs) {
    if (!ix || !contigs || n_seqs <= 0) return BWAMS_ERR_ARG;
    const int64_t l_pac = (ix->fmi.ref_seq_len - 1) / 2;
    int64_t at = 0;
    for (int32_t i = 0; i < n_seqs; ++i) {
        if (contigs[i].offset != at || contigs[i].len <= 0) {
            set_last_error("bwams_index_set_contigs: sequences must tile [0, l_pac) in order");
            return BWAMS_ERR_ARG;
        }
        at += contigs[i].len;
    }
    if (at != l_pac) {
        set_last_error("bwams_index_set_contigs: sequence lengths do not add up to l_pac");
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(ix->device));
    BWAMS_HIP(ix->d_contigs.alloc((size_t)n_seqs * sizeof(bwams_contig_t)));
    BWAMS_HIP(hipMemcpy(ix->d_contigs.p, contigs, (size_t)n_seqs * sizeof(bwams_contig_t), hipMemcpyHostToDevice));
    ix->n_seqs = n_seqs;
    return BWAMS_OK;
}

// mem_flt_chained_seeds for the chunk's long reads (seed_sw.hip): re-score short seeds with the local-SW
// kernel, drop the weak ones, re-pack the seed array
static int flt_chained_seeds(bwams_batch *b, StageState *s, const bwams_mem_opt_t *opt, const DevBns &bns) {
    if (!b->idx->fmi.ref) {
        set_last_error("bwams_chain_run: reads of ~1100 bases and more need the .0123 reference (mem_flt_chained_seeds)");
        return BWAMS_ERR_ARG;
    }
    int mx = -128, mn = 127;
    for (int i = 0; i < 25; ++i) { mx = mx > opt->mat[i] ? mx : opt->mat[i]; mn = mn < opt->mat[i] ? mn : opt->mat[i]; }
    if (mx <= 0 || (opt->o_ins + opt->e_ins) + (opt->o_del + opt->e_del) <= mx - mn) {
        set_last_error("bwams_chain_run: the local SW of mem_flt_chained_seeds needs max(mat) > 0 and oe_ins + oe_del > max(mat) - min(mat)");
        return BWAMS_ERR_UNSUPPORTED;
    }
    hipStream_t st = b->stream;
    const int64_t N = s->ch.n_seeds, N1 = N + 1, C = s->ch.n_chains, n1 = s->ch.nseq + 1;
    BWAMS_HIP(s->ext.cnt.ensure((size_t)N1 * 6 * 4)); BWAMS_HIP(s->ext.ewide.ensure((size_t)(N1 > C + 1 ? N1 : C + 1) * 6 * 8));
    BWAMS_HIP(s->ext.eoffs.ensure((size_t)(N1 > C + 1 ? N1 : C + 1) * 6 * 8)); BWAMS_HIP(s->ch.sw_qb.ensure_n((size_t)N1));
    BWAMS_HIP(s->ch.sw_rb.ensure_n((size_t)N1)); BWAMS_HIP(s->ch.sw_read.ensure_n((size_t)N1)); BWAMS_HIP(s->ch.sw_newn.ensure_n((size_t)(C + 1)));
    BWAMS_HIP(s->ch.seeds2.ensure_n((size_t)N1));
    SeedSwArgs W;
    W.chains = s->ch.chains.p; W.n_chains = C; W.seeds = s->ch.seeds.p; W.n_seeds = N; W.enc = b->d_enc.p; W.cum = b->d_cum.p; W.nseq = s->ch.nseq;
    W.ref = b->idx->fmi.ref; W.bns = bns; W.opt = *opt; W.cnt = s->ext.cnt.as<int32_t>(); W.win_qb = s->ch.sw_qb.p; W.win_rb = s->ch.sw_rb.p;
    W.seed_read = s->ch.sw_read.p;
    launch_seedsw_plan(W, s->ext.ewide.as<int64_t>(), st);
    int rc = scan_rows(b, s->ext.ewide.as<int64_t>(), s->ext.eoffs.as<int64_t>(), 3, N1);
    if (rc) return rc;
    int64_t tot[3];
    for (int r = 0; r < 3; ++r) BWAMS_HIP(hipMemcpyAsync(&tot[r], s->ext.eoffs.as<int64_t>() + r * N1 + N, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    if (tot[1] >= ((int64_t)1 << 31) || tot[2] >= ((int64_t)1 << 31)) {
        set_last_error("bwams_chain_run: seed re-scoring buffers exceed the 31-bit offsets of SeqPair; use smaller chunks");
        return BWAMS_ERR_CAPACITY;
    }
    BWAMS_HIP(s->ext.lpairs.ensure_n((size_t)(tot[0] + 1))); BWAMS_HIP(s->ext.lqer.ensure_n((size_t)tot[1] + 64));
    BWAMS_HIP(s->ext.lref.ensure_n((size_t)tot[2] + 64)); BWAMS_HIP(s->ch.sw_res.ensure_n((size_t)(tot[0] + 1)));
    if (tot[0] > 0) {
        launch_seedsw_build(W, s->ext.eoffs.as<int64_t>(), s->ext.lpairs.p, s->ext.lref.p, s->ext.lqer.p, b->cu_count, st);
        SwParams prm;
        sw_params(*opt, 0, &prm);
        (void)launch_ksw(s->ext.lpairs.p, tot[0], s->ext.lref.p, s->ext.lqer.p, prm, 208, 200, s->ch.sw_res.p, b->d_ctr.p, b->cu_count, st);
    }
    // keep / drop, new chain lengths, packed offsets (eoffs row 0 still holds the task index of each seed)
    int64_t *cw = s->ext.ewide.as<int64_t>();                // reused: C + 1 entries
    int64_t *coff = s->ext.eoffs.as<int64_t>() + 3 * N1;     // behind the three rows in use
    launch_seedsw_apply(W, s->ext.eoffs.as<int64_t>(), s->ch.sw_res.p, s->ch.sw_newn.p, cw, st);
    if ((rc = scan_rows(b, cw, coff, 1, C + 1))) return rc;
    int64_t new_total = 0;
    BWAMS_HIP(hipMemcpyAsync(&new_total, coff + C, 8, hipMemcpyDeviceToHost, st));
    launch_seedsw_repack(W, s->ch.sw_newn.p, coff, s->ch.seeds2.p, s->ch.chain_off.as<int64_t>(), s->ch.chain_off.as<int64_t>() + n1, st);
    BWAMS_HIP(hipStreamSynchronize(st));
    std::swap(s->ch.seeds, s->ch.seeds2);
    s->ch.n_seeds = new_total;
    return BWAMS_OK;
}

// the seeds of a chunk as the chaining kernels read them: SMEM-like records in (rid, m, n) order and, per record,
// the reference positions to chain (already strided to at most max_occ)
struct SeedView {
    const bwams_smem_t *smem;
    int64_t n_smem;
    const int64_t *sa_off, *sa_coord;
    int64_t n_sa;
    bool one_smem_quirk;        // mem_chain_seeds' `pos < num_smem - 1` (bwamem.cpp:819); mem_chain_new has no such guard
};
static int chain_common(bwams_batch *b, const bwams_mem_opt_t *opt, const SeedView &sv, int64_t *n_chains, int64_t *n_seeds);

int bwams_chain_run(bwams_batch_t *b, const bwams_mem_opt_t *opt, int64_t *n_chains, int64_t *n_seeds) {
    if (b && b->stages) b->stages->ch.ran = false;       // bwams_debug_chain_counts reports the LAST run: a refused one has nothing to report
    if (!has(b, Product::seeds) || !b->sd.with_sa) {
        set_last_error("bwams_chain_run: run bwams_seed_run(with_sa = 1) first");
        return BWAMS_ERR_ARG;
    }
    int rc = check_opt(opt, "bwams_chain_run");
    if (rc) return rc;
    if ((rc = bwams_seed_counts(b, nullptr, nullptr))) return rc;     // sizes of the seed stage (and its overflow check)
    SeedView sv;
    sv.smem = b->sd.d_sorted.p; sv.n_smem = b->sd.n_smem; sv.sa_off = b->sd.d_sa_off.p; sv.sa_coord = b->sd.d_sa_coord.p; sv.n_sa = b->sd.n_sa;
    sv.one_smem_quirk = true;
    return chain_common(b, opt, sv, n_chains, n_seeds);
}

int bwams_chain_run_ert(bwams_batch_t *b, const bwams_mem_opt_t *opt, const bwams_ert_mem_t *mems, const int64_t *mem_off,
                        const uint64_t *hits, const int64_t *hit_off, int64_t *n_chains, int64_t *n_seeds) {
    if (b && b->stages) b->stages->ch.ran = false;
    if (!has(b, Product::reads) || b->nseq <= 0 || !mem_off || !hit_off) {
        set_last_error("bwams_chain_run_ert: upload the reads first (bwams_seed_upload) and pass the MEM / hit offsets");
        return BWAMS_ERR_ARG;
    }
    int rc = check_opt(opt, "bwams_chain_run_ert");
    if (rc) return rc;
    const int64_t nseq = b->nseq, n1 = nseq + 1;
    const int64_t n_mems = mem_off[nseq], n_hits = hit_off[nseq];
    if (mem_off[0] != 0 || hit_off[0] != 0 || n_mems < 0 || n_hits < 0 || (n_mems && !mems) || (n_hits && !hits)) return BWAMS_ERR_ARG;
    for (int64_t r = 0; r < nseq; ++r) {
        if (mem_off[r + 1] < mem_off[r] || hit_off[r + 1] < hit_off[r]) { set_last_error("bwams_chain_run_ert: offsets must be non-decreasing"); return BWAMS_ERR_ARG; }
        const int64_t nh = hit_off[r + 1] - hit_off[r];
        for (int64_t i = mem_off[r]; i < mem_off[r + 1]; ++i) {
            const bwams_ert_mem_t &m = mems[i];
            if (m.start < 0 || m.end <= m.start || m.hitcount < 0 || m.hitbeg < 0 || (int64_t)m.hitbeg + m.hitcount > nh) {
                set_last_error("bwams_chain_run_ert: a MEM with an empty span or a hit slice outside its read's hit array");
                return BWAMS_ERR_ARG;
            }
        }
    }
    BWAMS_HIP(hipSetDevice(b->idx->device));
    StageState *s;
    if ((rc = get_state(b, &s))) return rc;
    hipStream_t st = b->stream;
    BWAMS_HIP(s->ch.et_mems.ensure_n((size_t)(n_mems + 1))); BWAMS_HIP(s->ch.et_moff.ensure_n((size_t)n1));
    BWAMS_HIP(s->ch.et_hoff.ensure_n((size_t)n1)); BWAMS_HIP(s->ch.et_hits.ensure_n((size_t)(n_hits + 1)));
    BWAMS_HIP(s->ch.et_smem.ensure_n((size_t)(n_mems + 1))); BWAMS_HIP(s->ch.et_cnt.ensure_n((size_t)(n_mems + 1)));
    BWAMS_HIP(s->ch.et_off.ensure_n((size_t)(n_mems + 1))); BWAMS_HIP(s->ch.et_srt.ensure((size_t)(n_mems + 1) * 24));
    if (n_mems) BWAMS_HIP(hipMemcpyAsync(s->ch.et_mems.p, mems, (size_t)n_mems * sizeof(bwams_ert_mem_t), hipMemcpyHostToDevice, st));
    if (n_hits) BWAMS_HIP(hipMemcpyAsync(s->ch.et_hits.p, hits, (size_t)n_hits * 8, hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipMemcpyAsync(s->ch.et_moff.p, mem_off, (size_t)n1 * 8, hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipMemcpyAsync(s->ch.et_hoff.p, hit_off, (size_t)n1 * 8, hipMemcpyHostToDevice, st));
    ErtArgs E;
    E.mems = s->ch.et_mems.p; E.mem_off = s->ch.et_moff.p; E.hits = s->ch.et_hits.p; E.hit_off = s->ch.et_hoff.p; E.nseq = nseq; E.n_mems = n_mems;
    E.l_pac = (b->idx->fmi.ref_seq_len - 1) / 2; E.max_occ = opt->max_occ; E.pad_ = 0; E.smem_out = s->ch.et_smem.p; E.cnt = s->ch.et_cnt.p;
    E.srt = s->ch.et_srt.p;
    launch_ert_sort(E, st);
    if ((rc = scan_rows(b, s->ch.et_cnt.p, s->ch.et_off.p, 1, n_mems + 1))) return rc;
    int64_t n_sa = 0;
    BWAMS_HIP(hipMemcpyAsync(&n_sa, s->ch.et_off.p + n_mems, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(s->ch.et_coord.ensure_n((size_t)(n_sa + 1)));
    launch_ert_pick(E, s->ch.et_off.p, s->ch.et_coord.p, st);
    SeedView sv;
    sv.smem = s->ch.et_smem.p; sv.n_smem = n_mems; sv.sa_off = s->ch.et_off.p;
    sv.sa_coord = s->ch.et_coord.p; sv.n_sa = n_sa; sv.one_smem_quirk = false;
    return chain_common(b, opt, sv, n_chains, n_seeds);
}

static int chain_common(bwams_batch *b, const bwams_mem_opt_t *opt, const SeedView &sv, int64_t *n_chains, int64_t *n_seeds) {
    int rc;
    if (b->max_read_len >= 32768) {
        set_last_error("bwams_chain_run: reads of 32768 bases or more are not supported (16-bit query coordinates)");
        return BWAMS_ERR_UNSUPPORTED;
    }
    BWAMS_HIP(hipSetDevice(b->idx->device));
    StageState *s;
    if ((rc = get_state(b, &s))) return rc;
    outdated(b, Product::chains);
    hipStream_t st = b->stream;
    const int64_t nseq = b->nseq, n_sa = sv.n_sa, n1 = nseq + 1;
    const size_t ns = (size_t)(n_sa > 0 ? n_sa : 1);
    BWAMS_HIP(s->ch.s_next.ensure_n(ns)); BWAMS_HIP(s->ch.s_ql.ensure_n(ns)); BWAMS_HIP(s->ch.crec.ensure(chain_rec_bytes(n_sa)));
    BWAMS_HIP(s->ch.flt.ensure_n(ns)); BWAMS_HIP(s->ch.f_rec.ensure_n(ns)); BWAMS_HIP(s->ch.f_first.ensure_n(ns));
    BWAMS_HIP(s->ch.f_kept.ensure_n(ns)); BWAMS_HIP(s->ch.f_sel.ensure_n(ns)); BWAMS_HIP(s->ch.n_chn.ensure_n((size_t)n1));
    BWAMS_HIP(s->heavy.ensure_n((size_t)n1)); BWAMS_HIP(s->ch.redo.ensure_n((size_t)n1)); BWAMS_HIP(s->ch.slice.ensure((size_t)n1 * 16));
    BWAMS_HIP(s->ch.okeys.ensure_n((size_t)n1)); BWAMS_HIP(s->ch.okeys2.ensure_n((size_t)n1)); BWAMS_HIP(s->ch.ovals.ensure_n((size_t)n1));
    BWAMS_HIP(s->ch.ovals2.ensure_n((size_t)n1)); BWAMS_HIP(s->ch.nodes.ensure(chain_node_bytes(n_sa, nseq)));
    BWAMS_HIP(s->ch.n_kept.ensure_n((size_t)n1)); BWAMS_HIP(s->ch.n_kept_seeds.ensure_n((size_t)n1)); BWAMS_HIP(s->ch.read_base.ensure_n((size_t)n1));
    BWAMS_HIP(s->ch.frac.ensure_n((size_t)n1)); BWAMS_HIP(s->ch.wide.ensure((size_t)n1 * 16)); BWAMS_HIP(s->ch.chain_off.ensure((size_t)n1 * 16));

    ChainArgs A;
    A.smem = sv.smem; A.n_smem = sv.n_smem; A.sa_off = sv.sa_off; A.sa_coord = sv.sa_coord; A.cum = b->d_cum.p; A.nseq = nseq;
    if ((rc = dev_bns(b->idx, &A.bns))) return rc;
    A.opt = *opt;
    A.s_next = s->ch.s_next.p; A.s_ql = s->ch.s_ql.p; A.crec = s->ch.crec.p; A.flt = s->ch.flt.p; A.f_rec = s->ch.f_rec.p;
    A.f_first = s->ch.f_first.p; A.f_kept = s->ch.f_kept.p; A.f_sel = s->ch.f_sel.p; A.nodes = s->ch.nodes.p; A.n_kept = s->ch.n_kept.p;
    A.n_kept_seeds = s->ch.n_kept_seeds.p; A.n_chn = s->ch.n_chn.p; A.heavy = s->heavy.p; A.redo = s->ch.redo.p; A.slice = s->ch.slice.as<int64_t>();
    A.order = s->ch.ovals2.p; A.read_base = s->ch.read_base.p; A.frac_rep = s->ch.frac.p; A.ctr = b->d_ctr.p; A.seed_batch = knobs().chain_batch;

    BWAMS_HIP(hipEventRecord(s->ev[0], st));
    // chain_redo, chain_redo_ticket, (pair_heavy, pair_ticket: the pairing stage clears them before it uses them,) dbg[0 .. 19): the filter's
    // size histogram and cycle counts, the two route counts of the counting instances and the sequential form's count, so that they are
    // this run's (bwams_debug_chain_counts).  dbg is shared: the seeding stage's diagnostics use dbg[0 .. 19] and de-duplication's dbg[0 .. 19] as
    // well, each cleared, filled and printed (BWAMS_VERBOSE) within its own run — chaining's filter added to dbg[0 .. 15] on top of whatever they
    // left before this clear existed; nothing reads another stage's figures after a later stage has run.
    static_assert(offsetof(DevCounters, dbg) == offsetof(DevCounters, chain_redo) + 4 * sizeof(unsigned long long), "one memset clears chain_redo .. dbg[18]");
    BWAMS_HIP(hipMemsetAsync(&b->d_ctr.p->chain_redo, 0, 23 * sizeof(unsigned long long), st));
    const bool count_ch = knobs().chain_count != 0;       // tests: reads per filter route, passes of chain_seeds_batch (bwams_debug_chain_counts)
    if (count_ch) BWAMS_HIP(hipMemsetAsync(b->d_ctr.p->dbg + 61, 0, 4 * sizeof(unsigned long long), st));
    BWAMS_HIP(hipMemsetAsync(&b->d_ctr.p->chain_overflow, 0, 29 * sizeof(unsigned long long), st));   // overflow, longread, n_heavy, chain_class[10], chain_ticket[10], heavy_tickets[6]
    BWAMS_HIP(hipMemsetAsync(&b->d_ctr.p->chain_lane_giveup, 0, sizeof(unsigned long long), st));
    // mem_chain_seeds' loop guard `pos < num_smem - 1` (bwamem.cpp:819) makes a work item with exactly
    // one SMEM produce no chain at all
    if ((sv.one_smem_quirk ? sv.n_smem <= 1 : sv.n_smem <= 0) || n_sa == 0) {
        BWAMS_HIP(hipMemsetAsync(s->ch.n_kept.p, 0, (size_t)n1 * 4, st));
        BWAMS_HIP(hipMemsetAsync(s->ch.n_kept_seeds.p, 0, (size_t)n1 * 4, st));
    } else {
        // reads of similar seed count share a wave: sort read ids by descending count
        launch_chain_count(A, s->ch.okeys.p, s->ch.ovals.p, st);
        if ((rc = with_tmp(b, "bwams_chain_run: radix_sort_pairs_desc", [&](void *tmp, size_t &tb) {
                return rocprim::radix_sort_pairs_desc(tmp, tb, s->ch.okeys.p, s->ch.okeys2.p, s->ch.ovals.p, s->ch.ovals2.p, (size_t)nseq, 0, 32, st);
            }))) return rc;
        if (launch_chain(A, s->ch.okeys.p, b->cu_count, st, s->aux, s->fork, s->join, count_ch)) {
            set_last_error("bwams_chain_run: stream fork/join failed");
            return BWAMS_ERR_DEVICE;
        }
    }
    int64_t tot[2] = {0, 0};
    if (nseq > 0) {
        launch_widen2(A.n_kept, A.n_kept_seeds, nseq, s->ch.wide.as<int64_t>(), st);
        if ((rc = scan_rows(b, s->ch.wide.as<int64_t>(), s->ch.chain_off.as<int64_t>(), 2, n1))) return rc;
        BWAMS_HIP(hipMemcpyAsync(&tot[0], s->ch.chain_off.as<int64_t>() + nseq, 8, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipMemcpyAsync(&tot[1], s->ch.chain_off.as<int64_t>() + n1 + nseq, 8, hipMemcpyDeviceToHost, st));
    } else {
        BWAMS_HIP(hipMemsetAsync(s->ch.chain_off.p, 0, (size_t)n1 * 16, st));       // no reads: both offset rows are {0}
    }
    BWAMS_HIP(hipMemcpyAsync(b->h_ctr.p, b->d_ctr.p, sizeof(DevCounters), hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    {
        const bool vb = knobs().verbose != 0;
        if (vb) {
            const unsigned long long *d = b->h_ctr.p->dbg;
            fprintf(stderr, "[bwams_chain_run] filter wave tier: reads by chains <=32 %llu <=64 %llu <=128 %llu <=256 %llu <=512 %llu <=960 %llu more %llu (+ %llu taken sequentially by one lane); "
                            "Mcycles: sequential(HBM) %.1f sort %.1f filter %.1f; chains %llu selected %llu; longest read: sort %.2f filter %.2f Mcycles, most chains %llu, most selected %llu\n",
                    d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[18], d[7] / 1e6, d[8] / 1e6, d[9] / 1e6, d[11], d[10], d[12] / 1e6, d[13] / 1e6, d[14], d[15]);
#ifdef BWAMS_CHAINDBG
            static const char *cn[8] = {"XL", "L", "L2", "L1", "M2", "M", "M1", "S"};
            fprintf(stderr, "[bwams_chain_run] chaining wave tier, per class: reads / mean us / longest us / wave-ms:");
            for (int c = 0; c < 8; ++c) fprintf(stderr, "  %s %llu / %.0f / %.0f / %.1f", cn[c], d[32 + 3 * c], d[32 + 3 * c] ? d[33 + 3 * c] * 1e-2 / d[32 + 3 * c] : 0.0, d[34 + 3 * c] * 1e-2, d[33 + 3 * c] * 1e-5);
            fprintf(stderr, "\n");
            fprintf(stderr, "[bwams_chain_run] wave tier phases, G cycles: preamble %.2f chaining %.2f weights+copy %.2f (sort %.2f filter %.2f: all reads); reads %llu seeds %llu; passes %llu settling %llu seeds (%llu new chains), %llu seeds one by one%s; pass parts, G cycles: batch prologue %.2f search %.2f record+test %.2f settle %.2f commit %.2f one-by-one %.2f\n",
                    d[56] / 1e9, d[57] / 1e9, d[58] / 1e9, d[8] / 1e9, d[9] / 1e9, d[59], d[60], count_ch ? d[61] : 0ull, count_ch ? d[63] : 0ull,
                    count_ch ? d[64] : 0ull, count_ch ? d[62] : 0ull, count_ch ? "" : " (these four are counted under BWAMS_CHAIN_COUNT=1 only)", d[65] / 1e9, d[66] / 1e9, d[67] / 1e9, d[68] / 1e9, d[69] / 1e9, d[70] / 1e9);
#endif
        }
    }
    if (b->h_ctr.p->chain_overflow) {
        set_last_error("bwams_chain_run: internal B-tree node region exhausted");
        return BWAMS_ERR_CAPACITY;
    }
    {
        const DevCounters *h = b->h_ctr.p;
        int64_t *c = s->ch.counts;
        for (int i = 0; i < 10; ++i) c[i] = (int64_t)h->chain_class[i];
        c[10] = (int64_t)h->n_heavy; c[11] = (int64_t)h->chain_redo;
        for (int i = 0; i < 7; ++i) c[12 + i] = (int64_t)h->dbg[i];
        c[19] = (int64_t)h->dbg[18];
        c[20] = count_ch ? (int64_t)h->dbg[16] : -1; c[21] = count_ch ? (int64_t)h->dbg[17] : -1;
        c[22] = count_ch ? (int64_t)h->dbg[61] : -1; c[23] = count_ch ? (int64_t)h->dbg[63] : -1;
        c[24] = count_ch ? (int64_t)h->dbg[64] : -1; c[25] = count_ch ? (int64_t)h->dbg[62] : -1;
        const bool chained = !((sv.one_smem_quirk ? sv.n_smem <= 1 : sv.n_smem <= 0) || n_sa == 0);      // (else no kernel ran)
        s->ch.lane_counts[0] = chained ? nseq - (int64_t)h->chain_class[5] : 0;
        s->ch.lane_counts[1] = (int64_t)h->chain_lane_giveup;
        s->ch.ran = true;
    }
    const bool has_long = b->h_ctr.p->chain_longread != 0;
    s->ch.n_redo = (int64_t)b->h_ctr.p->chain_redo;
    s->ch.n_chains = tot[0]; s->ch.n_seeds = tot[1]; s->ch.nseq = nseq;
    BWAMS_HIP(s->ch.chains.ensure_n((size_t)(tot[0] + 1))); BWAMS_HIP(s->ch.seeds.ensure_n((size_t)(tot[1] + 1)));
    if (tot[0] > 0) launch_chain_emit(A, s->ch.chain_off.as<int64_t>(), s->ch.chain_off.as<int64_t>() + n1, s->ch.chains.p, s->ch.seeds.p, st);
    if (has_long && tot[0] > 0 && (rc = flt_chained_seeds(b, s, opt, A.bns))) return rc;
    BWAMS_HIP(hipEventRecord(s->ev[1], st));
    BWAMS_HIP(hipGetLastError());
    s->opt = *opt;
    if (n_chains) *n_chains = s->ch.n_chains;
    if (n_seeds) *n_seeds = s->ch.n_seeds;
    produced(b, Product::chains);
    return BWAMS_OK;
}

int bwams_chain_fetch(bwams_batch_t *b, bwams_chain_t *chains, int64_t chain_cap, bwams_chain_seed_t *seeds,
                      int64_t seed_cap, int64_t *chain_off) {
    if (!has(b, Product::chains)) {
        set_last_error("bwams_chain_fetch: no chains on the device");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    if (s->ch.n_chains > chain_cap || s->ch.n_seeds > seed_cap) return BWAMS_ERR_CAPACITY;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    if (s->ch.n_chains) BWAMS_HIP(hipMemcpyAsync(chains, s->ch.chains.p, (size_t)s->ch.n_chains * sizeof(bwams_chain_t), hipMemcpyDeviceToHost, st));
    if (s->ch.n_seeds) BWAMS_HIP(hipMemcpyAsync(seeds, s->ch.seeds.p, (size_t)s->ch.n_seeds * sizeof(bwams_chain_seed_t), hipMemcpyDeviceToHost, st));
    if (chain_off) BWAMS_HIP(hipMemcpyAsync(chain_off, s->ch.chain_off.p, (size_t)(s->ch.nseq + 1) * 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    return BWAMS_OK;
}

/* Test hook: routes and passes of the last chaining run (include/bwams.h). */
int bwams_debug_chain_counts(bwams_batch_t *b, int64_t counts[26]) {
    static_assert(kChainCounts == 26, "include/bwams.h documents 26 counters");
    if (!counts || !has(b, Product::chains) || !b->stages->ch.ran) {
        set_last_error("bwams_debug_chain_counts: no bwams_chain_run / bwams_chain_run_ert on this batch");
        return BWAMS_ERR_ARG;
    }
    for (int i = 0; i < kChainCounts; ++i) counts[i] = b->stages->ch.counts[i];
    return BWAMS_OK;
}

/* Test hook: the lane tier of the last chaining run (include/bwams.h). */
int bwams_debug_chain_lane_counts(bwams_batch_t *b, int64_t counts[2]) {
    if (!counts || !has(b, Product::chains) || !b->stages->ch.ran) {
        set_last_error("bwams_debug_chain_lane_counts: no bwams_chain_run / bwams_chain_run_ert on this batch");
        return BWAMS_ERR_ARG;
    }
    counts[0] = b->stages->ch.lane_counts[0]; counts[1] = b->stages->ch.lane_counts[1];
    return BWAMS_OK;
}

int bwams_chain_upload(bwams_batch_t *b, const bwams_chain_t *chains, int64_t n_chains, const bwams_chain_seed_t *seeds,
                       int64_t n_seeds, const int64_t *chain_off) {
    if (!b || !chain_off || n_chains < 0 || n_seeds < 0 || (n_chains && (!chains || !seeds))) return BWAMS_ERR_ARG;
    if (!has(b, Product::reads) || b->nseq <= 0) {
        set_last_error("bwams_chain_upload: upload the reads first (bwams_seed_upload)");
        return BWAMS_ERR_ARG;
    }
    const int64_t nseq = b->nseq, n1 = nseq + 1;
    if (chain_off[0] != 0 || chain_off[nseq] != n_chains) return BWAMS_ERR_ARG;
    // seeds must be laid out chain after chain, chains read after read (what bwams_chain_fetch returns)
    int64_t at = 0;
    std::string bad;
    int64_t *soff = new int64_t[(size_t)n1];
    for (int64_t r = 0; r < nseq && bad.empty(); ++r) {
        soff[r] = at;
        if (chain_off[r + 1] < chain_off[r]) bad = "chain_off must be non-decreasing";
        for (int64_t j = chain_off[r]; j < chain_off[r + 1] && bad.empty(); ++j) {
            if (chains[j].seqid != r) bad = "chain.seqid does not match chain_off";
            else if (chains[j].seed_off != at || chains[j].n < 0) bad = "chain.seed_off must enumerate the seed array in order";
            at += chains[j].n;
        }
    }
    soff[nseq] = at;
    if (bad.empty() && at != n_seeds) bad = "seed counts do not add up";
    if (!bad.empty()) {
        delete[] soff;
        set_last_error("bwams_chain_upload: " + bad);
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(b->idx->device));
    StageState *s;
    int rc = get_state(b, &s);
    if (rc) { delete[] soff; return rc; }
    outdated(b, Product::chains);
    hipStream_t st = b->stream;
    BWAMS_HIP(s->ch.chain_off.ensure((size_t)n1 * 16)); BWAMS_HIP(s->ch.chains.ensure_n((size_t)(n_chains + 1)));
    BWAMS_HIP(s->ch.seeds.ensure_n((size_t)(n_seeds + 1)));
    BWAMS_HIP(hipMemcpyAsync(s->ch.chain_off.p, chain_off, (size_t)n1 * 8, hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipMemcpyAsync(s->ch.chain_off.as<int64_t>() + n1, soff, (size_t)n1 * 8, hipMemcpyHostToDevice, st));
    if (n_chains) BWAMS_HIP(hipMemcpyAsync(s->ch.chains.p, chains, (size_t)n_chains * sizeof(bwams_chain_t), hipMemcpyHostToDevice, st));
    if (n_seeds) BWAMS_HIP(hipMemcpyAsync(s->ch.seeds.p, seeds, (size_t)n_seeds * sizeof(bwams_chain_seed_t), hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    delete[] soff;
    s->ch.n_chains = n_chains; s->ch.n_seeds = n_seeds; s->ch.nseq = nseq;
    s->ch.ran = false;
    produced(b, Product::chains);
    return BWAMS_OK;
}
}  // extern "C"
