// api_sam.hip — C-ABI entry points of the SAM side (include/bwams.h): bwams_reg2aln_* (mem_reg2aln, the host's mem_approx_mapq_se),
// the test hooks bwams_debug_regs_upload, bwams_debug_pair_regs_upload and bwams_debug_aln_lists, bwams_index_set_contig_names and _annos, bwams_sam_upload, _run,
// _run_emf, _run_pe, _fetch and _fetch_bgzf, over reg2aln.hip and sam_text.hip.  No CPU fallback: every entry point runs HIP kernels or returns an error.
#include <cmath>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "stage_state.h"

using namespace bwams;

extern "C" {
/* ------------------------------------------------------------- mem_reg2aln ---- */

// mem_approx_mapq_se (bwamem.cpp:1983-2008) on the host: a dozen double operations per region, with the C library's log
static int approx_mapq_se(const bwams_mem_opt_t *opt, const bwams_alnreg_t *a) {
    int mapq, l, sub = a->sub ? a->sub : opt->min_seed_len * opt->a;
    double identity;
    const int coef_len = opt->mapq_coef_len;
    const double coef_fac = coef_len > 0 ? log((double)coef_len) : 0.;
    sub = a->csub > sub ? a->csub : sub;
    if (sub >= a->score) return 0;
    l = a->qe - a->qb > a->re - a->rb ? a->qe - a->qb : (int)(a->re - a->rb);
    identity = 1. - (double)(l * opt->a - a->score) / (opt->a + opt->b) / l;
    if (a->score == 0) mapq = 0;
    else if (coef_len > 0) {
        double tmp = l < coef_len ? 1. : coef_fac / log(l);
        tmp *= identity * identity;
        mapq = (int)(6.02 * (a->score - sub) / opt->a * tmp * tmp + .499);
    } else {
        mapq = (int)(30.0 * (1. - (double)sub / a->score) * log(a->seedcov) + .499);
        mapq = identity < 0.95 ? (int)(mapq * identity * identity + .499) : mapq;
    }
    if (a->sub_n > 0) mapq -= (int)(4.343 * log(a->sub_n + 1) + .499);
    if (mapq > 60) mapq = 60;
    if (mapq < 0) mapq = 0;
    mapq = (int)(mapq * (1. - a->frac_rep) + .499);
    return mapq;
}

static int reg2aln_impl(bwams_batch_t *b, const bwams_mem_opt_t *opt, int32_t source, const uint8_t *only, int64_t *n_aln,
                        int64_t *n_cigar_ops, int64_t *md_bytes) {
    if (source < 0 || source > 1 || !has(b, source ? Product::pair : Product::dedup)) {
        set_last_error("bwams_reg2aln_run: run bwams_dedup_run (source 0) or bwams_pair_run (source 1) first");
        return BWAMS_ERR_ARG;
    }
    int rc = check_opt(opt, "bwams_reg2aln_run");
    if (rc) return rc;
    if (!b->idx->fmi.ref) {
        set_last_error("bwams_reg2aln_run: the index was opened without its .0123 reference");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    outdated(b, Product::al);
    const int64_t n = source ? s->pr.total : s->dd.n_final;
    RegAlnArgs A;
    memset(&A, 0, sizeof A);
    A.regs = source ? s->pr.out.p : s->dd.out.p; A.reg_off = source ? s->pr.ooff.p : s->dd.off.p; A.n_regs = n; A.nseq = s->ch.nseq;
    A.enc = b->d_enc.p; A.cum = b->d_cum.p; A.ref = b->idx->fmi.ref;
    if ((rc = dev_bns(b->idx, &A.bns))) return rc;
    A.opt = *opt; A.only = only;
    const int64_t n1 = n + 1;
    BWAMS_HIP(s->al.need.ensure_n((size_t)n1)); BWAMS_HIP(s->al.cls.ensure_n((size_t)n1)); BWAMS_HIP(s->al.off.ensure_n((size_t)n1));
    BWAMS_HIP(s->al.list.ensure((size_t)n1 * 4 * 4)); BWAMS_HIP(s->al.rec.ensure_n((size_t)n1)); BWAMS_HIP(s->al.wide.ensure((size_t)(2 * n1) * 8));
    BWAMS_HIP(s->al.offs.ensure((size_t)(2 * n1) * 8)); BWAMS_HIP(s->al.cnt.ensure_n(32));
    A.need = s->al.need.p; A.cls = s->al.cls.p; A.scr_off = s->al.off.p;
    A.list = s->al.list.as<int32_t>(); A.n_list = s->al.cnt.p; A.rec = s->al.rec.p;
    int64_t tot[2] = {0, 0};
    if (n > 0) {
        BWAMS_HIP(hipMemsetAsync(s->al.cnt.p, 0, 256, st));
        BWAMS_HIP(hipMemsetAsync(s->al.need.p + n, 0, 8, st));
        launch_aln_plan(A, st);
        if ((rc = scan_rows(b, A.need, s->al.off.p, 1, n1))) return rc;
        int64_t scr_bytes = 0;
        BWAMS_HIP(hipMemcpyAsync(&scr_bytes, s->al.off.p + n, 8, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipStreamSynchronize(st));
        BWAMS_HIP(s->al.scr.ensure_n((size_t)scr_bytes + 64));
        A.scr = s->al.scr.p;
        launch_aln_run(A, b->cu_count, st);
        launch_aln_sizes(A, s->al.wide.as<int64_t>(), st);
        if ((rc = scan_rows(b, s->al.wide.as<int64_t>(), s->al.offs.as<int64_t>(), 2, n1))) return rc;
        BWAMS_HIP(hipMemcpyAsync(&tot[0], s->al.offs.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipMemcpyAsync(&tot[1], s->al.offs.as<int64_t>() + n1 + n, 8, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipStreamSynchronize(st));
        BWAMS_HIP(s->al.cig.ensure_n((size_t)(tot[0] + 1))); BWAMS_HIP(s->al.md.ensure_n((size_t)tot[1] + 16));
        launch_aln_gather(A, s->al.offs.as<int64_t>(), s->al.cig.p, s->al.md.p, st);
        BWAMS_HIP(hipStreamSynchronize(st));
        BWAMS_HIP(hipGetLastError());
#ifdef BWAMS_ALNDBG
        if (knobs().verbose) {
            unsigned long long c[32];
            BWAMS_HIP(hipMemcpy(c, s->al.cnt.p, 256, hipMemcpyDeviceToHost));
            fprintf(stderr, "[reg2aln] regions %lld: class lists %llu / %llu / %llu / %llu; wave kernel: %llu regions, per region setup %.1f us, DP %.1f us (%.2f DPs, mean band %.1f, %.0f rows), "
                    "traceback %.1f us, NM/MD + record %.1f us, slowest region %.1f us\n", (long long)n, c[0], c[1], c[2], c[3], c[8], c[8] ? c[9] * 1e-2 / c[8] : 0.0, c[8] ? c[10] * 1e-2 / c[8] : 0.0,
                    c[8] ? (double)c[13] / c[8] : 0.0, c[13] ? (double)c[14] / c[13] : 0.0, c[8] ? (double)c[15] / c[8] : 0.0, c[8] ? c[11] * 1e-2 / c[8] : 0.0, c[8] ? c[12] * 1e-2 / c[8] : 0.0, c[16] * 1e-2);
        }
#endif
    }
    s->al.n = n; s->al.ncig = tot[0]; s->al.nmd = tot[1]; s->al.source = source;
    s->opt = *opt;
    if (n_aln) *n_aln = n;
    if (n_cigar_ops) *n_cigar_ops = tot[0];
    if (md_bytes) *md_bytes = tot[1];
    produced(b, Product::al);
    return BWAMS_OK;
}

int bwams_reg2aln_run(bwams_batch_t *b, const bwams_mem_opt_t *opt, int32_t source, int64_t *n_aln, int64_t *n_cigar_ops,
                      int64_t *md_bytes) {
    return reg2aln_impl(b, opt, source, nullptr, n_aln, n_cigar_ops, md_bytes);
}

int bwams_reg2aln_run_sam(bwams_batch_t *b, const bwams_mem_opt_t *opt, const bwams_sam_opt_t *sopt, const bwams_pestat_t *pes,
                          int64_t *n_aln, int64_t *n_needed, int64_t *n_cigar_ops, int64_t *md_bytes) {
    if (!sopt || !has(b, Product::pair) || b->stages->pr.single == (pes != nullptr)) {
        set_last_error("bwams_reg2aln_run_sam: run bwams_pair_run first (BWAMS_PAIR_SINGLE_END and pes = NULL, or the paired-end form and its pes)");
        return BWAMS_ERR_ARG;
    }
    int rc = check_opt(opt, "bwams_reg2aln_run_sam");
    if (rc) return rc;
    StageState *s = b->stages;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    const int64_t n = s->pr.total;
    BWAMS_HIP(s->al.only.ensure_n((size_t)n + 64));
    BWAMS_HIP(hipMemsetAsync(s->al.only.p, 0, (size_t)n + 1, st));
    SamArgs A;
    memset(&A, 0, sizeof A);
    A.regs = s->pr.out.p; A.reg_off = s->pr.ooff.p; A.n_regs = n; A.nseq = s->ch.nseq; A.opt = *opt; A.sopt = *sopt;
    A.pairs = pes ? s->pr.res.p : nullptr;
    if (pes) memcpy(A.pes, pes, sizeof A.pes);
    launch_sam_need(A, s->al.only.p, b->cu_count, st);
    if (n_needed) {
        // a count for the caller (and the bench): one reduction over the mask
        BWAMS_HIP(s->sm.bad.ensure(64));
        int64_t *d_sum = s->sm.bad.as<int64_t>() + 1;
        if ((rc = with_tmp(b, "bwams_reg2aln_run_sam: reduce", [&](void *tmp, size_t &tb) {
                return rocprim::reduce(tmp, tb, s->al.only.p, d_sum, (int64_t)0, (size_t)(n > 0 ? n : 0), rocprim::plus<int64_t>(), st);
            }))) return rc;
        BWAMS_HIP(hipMemcpyAsync(n_needed, d_sum, 8, hipMemcpyDeviceToHost, st));
    }
    return reg2aln_impl(b, opt, 1, s->al.only.p, n_aln, n_cigar_ops, md_bytes);
}

int bwams_reg2aln_fetch(bwams_batch_t *b, bwams_aln_t *aln, int64_t aln_cap, uint32_t *cigar, int64_t cigar_cap, char *md, int64_t md_cap) {
    if (!has(b, Product::al)) {
        set_last_error("bwams_reg2aln_fetch: run bwams_reg2aln_run first");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    if (s->al.n > aln_cap || s->al.ncig > cigar_cap || s->al.nmd > md_cap) return BWAMS_ERR_CAPACITY;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    std::vector<bwams_alnreg_t> regs((size_t)s->al.n);
    if (s->al.n) {
        BWAMS_HIP(hipMemcpyAsync(aln, s->al.rec.p, (size_t)s->al.n * sizeof(bwams_aln_t), hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipMemcpyAsync(regs.data(), s->al.source ? s->pr.out.p : s->dd.out.p, (size_t)s->al.n * sizeof(bwams_alnreg_t),
                                 hipMemcpyDeviceToHost, st));
        if (s->al.ncig) BWAMS_HIP(hipMemcpyAsync(cigar, s->al.cig.p, (size_t)s->al.ncig * 4, hipMemcpyDeviceToHost, st));
        if (s->al.nmd) BWAMS_HIP(hipMemcpyAsync(md, s->al.md.p, (size_t)s->al.nmd, hipMemcpyDeviceToHost, st));
    }
    BWAMS_HIP(hipStreamSynchronize(st));
    for (int64_t k = 0; k < s->al.n; ++k)
        if (aln[k].rid >= 0) aln[k].mapq = regs[(size_t)k].secondary < 0 ? approx_mapq_se(&s->opt, &regs[(size_t)k]) : 0;
    return BWAMS_OK;
}

/* Test hooks: caller-given regions take the place of the de-duplication stage's final regions (include/bwams.h).  Only what
 * would make a kernel read outside the reads is refused; the reference side of a region is aln_plan_kernel's to judge.  for_pairing:
 * also what would make a pairing kernel index outside the sequence table or compute on nonsense. */
static int regs_upload(bwams_batch_t *b, const bwams_alnreg_t *regs, int64_t n_regs, const int64_t *reg_off, int64_t n_reads, bool for_pairing) {
    const std::string who = for_pairing ? "bwams_debug_pair_regs_upload" : "bwams_debug_regs_upload";
    if (!b || n_regs < 0 || n_reads < 0 || !reg_off || (n_regs && !regs)) return BWAMS_ERR_ARG;
    if (!has(b, Product::reads) || n_reads != b->nseq) {
        set_last_error(who + ": n_reads is not the number of reads of the last bwams_seed_upload");
        return BWAMS_ERR_ARG;
    }
    if (reg_off[0] != 0 || reg_off[n_reads] != n_regs) {
        set_last_error(who + ": reg_off must run from 0 to n_regs");
        return BWAMS_ERR_ARG;
    }
    for (int64_t r = 0; r < n_reads; ++r)
        if (reg_off[r + 1] < reg_off[r]) {
            set_last_error(who + ": reg_off decreases at read " + std::to_string(r));
            return BWAMS_ERR_ARG;
        }
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    std::vector<int64_t> cum((size_t)n_reads + 1);
    BWAMS_HIP(hipMemcpyAsync(cum.data(), b->d_cum.p, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    for (int64_t r = 0; r < n_reads; ++r) {
        const int64_t len = cum[(size_t)r + 1] - cum[(size_t)r];
        for (int64_t k = reg_off[r]; k < reg_off[r + 1]; ++k)
            if (regs[k].qb < 0 || regs[k].qe > len || regs[k].qb > regs[k].qe) {
                set_last_error(who + ": region " + std::to_string(k) + " has a query span outside its read");
                return BWAMS_ERR_ARG;
            }
    }
    if (for_pairing) {
        DevBns bns;
        if (int rc = dev_bns(b->idx, &bns)) return rc;
        for (int64_t k = 0; k < n_regs; ++k) {
            const bwams_alnreg_t &a = regs[k];
            const char *why = nullptr;
            if (a.rid < 0 || a.rid >= bns.n_seqs) why = " has rid outside [0, number of sequences)";
            else if (a.rb < 0 || a.re <= a.rb || a.re > 2 * bns.l_pac) why = " has a reference span that is empty or outside the text";
            else if (a.score < 0) why = " has a negative score";
            if (why) {
                set_last_error(who + ": region " + std::to_string(k) + why);
                return BWAMS_ERR_ARG;
            }
        }
    }
    StageState *s;
    int rc = get_state(b, &s);
    if (rc) return rc;
    outdated(b, Product::dedup);
    outdated(b, Product::er);          // beside the graph, as before: regions given by hand are not to meet mem_perfect2reg's of an earlier run
    BWAMS_HIP(s->dd.out.ensure_n((size_t)n_regs + 1)); BWAMS_HIP(s->dd.off.ensure_n((size_t)n_reads + 1));
    if (n_regs) BWAMS_HIP(hipMemcpyAsync(s->dd.out.p, regs, (size_t)n_regs * sizeof(bwams_alnreg_t), hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipMemcpyAsync(s->dd.off.p, reg_off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    s->dd.n_final = n_regs; s->ch.nseq = n_reads;
    produced(b, Product::dedup);
    return BWAMS_OK;
}
int bwams_debug_regs_upload(bwams_batch_t *b, const bwams_alnreg_t *regs, int64_t n_regs, const int64_t *reg_off, int64_t n_reads) {
    return regs_upload(b, regs, n_regs, reg_off, n_reads, false);
}
int bwams_debug_pair_regs_upload(bwams_batch_t *b, const bwams_alnreg_t *regs, int64_t n_regs, const int64_t *reg_off, int64_t n_reads) {
    return regs_upload(b, regs, n_regs, reg_off, n_reads, true);
}

/* Test hook: the lengths of the four region lists of the last bwams_reg2aln_run (include/bwams.h). */
int bwams_debug_aln_lists(bwams_batch_t *b, int64_t counts[4]) {
    if (!counts || !has(b, Product::al)) {
        set_last_error("bwams_debug_aln_lists: run bwams_reg2aln_run first");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (s->al.n > 0) {                                     // a run over no regions launches nothing and leaves the counters alone
        BWAMS_HIP(hipSetDevice(b->idx->device));
        unsigned long long c[4];
        BWAMS_HIP(hipMemcpyAsync(c, s->al.cnt.p, sizeof c, hipMemcpyDeviceToHost, b->stream));
        BWAMS_HIP(hipStreamSynchronize(b->stream));
        for (int i = 0; i < 4; ++i) counts[i] = (int64_t)c[i];
    }
    return BWAMS_OK;
}

/* ------------------------------------------------------------ SAM text (single-end) ---- */

int bwams_index_set_contig_names(bwams_index_t *ix, const char *names, const int32_t *name_off) {
    if (!ix || !names || !name_off) return BWAMS_ERR_ARG;
    DevBns bns;
    int rc = dev_bns(ix, &bns);                 // materialises the one-sequence default
    if (rc) return rc;
    const int32_t n = ix->n_seqs;
    for (int32_t i = 0; i < n; ++i)
        if (name_off[i] < 0 || name_off[i + 1] <= name_off[i] || names[name_off[i + 1] - 1] != 0) {
            set_last_error("bwams_index_set_contig_names: names must be NUL-terminated, back to back, name_off[n_seqs + 1] ascending");
            return BWAMS_ERR_ARG;
        }
    BWAMS_HIP(hipSetDevice(ix->device));
    ix->d_ctg_names.release(); ix->d_ctg_off.release();
    BWAMS_HIP(ix->d_ctg_names.alloc((size_t)name_off[n]));
    BWAMS_HIP(ix->d_ctg_off.alloc((size_t)(n + 1) * 4));
    BWAMS_HIP(hipMemcpy(ix->d_ctg_names.p, names, (size_t)name_off[n], hipMemcpyHostToDevice));
    BWAMS_HIP(hipMemcpy(ix->d_ctg_off.p, name_off, (size_t)(n + 1) * 4, hipMemcpyHostToDevice));
    return bam_names_index(ix, names, name_off, n);
}

int bwams_index_set_contig_annos(bwams_index_t *ix, const char *annos, const int32_t *anno_off) {
    if (!ix || !annos || !anno_off) return BWAMS_ERR_ARG;
    DevBns bns;
    int rc = dev_bns(ix, &bns);
    if (rc) return rc;
    const int32_t n = ix->n_seqs;
    for (int32_t i = 0; i < n; ++i)
        if (anno_off[i] < 0 || anno_off[i + 1] <= anno_off[i] || annos[anno_off[i + 1] - 1] != 0) {
            set_last_error("bwams_index_set_contig_annos: annotations must be NUL-terminated, back to back, anno_off[n_seqs + 1] ascending");
            return BWAMS_ERR_ARG;
        }
    BWAMS_HIP(hipSetDevice(ix->device));
    ix->d_ctg_annos.release(); ix->d_ctg_anno_off.release();
    BWAMS_HIP(ix->d_ctg_annos.alloc((size_t)anno_off[n]));
    BWAMS_HIP(ix->d_ctg_anno_off.alloc((size_t)(n + 1) * 4));
    BWAMS_HIP(hipMemcpy(ix->d_ctg_annos.p, annos, (size_t)anno_off[n], hipMemcpyHostToDevice));
    BWAMS_HIP(hipMemcpy(ix->d_ctg_anno_off.p, anno_off, (size_t)(n + 1) * 4, hipMemcpyHostToDevice));
    return BWAMS_OK;
}

int bwams_sam_upload(bwams_batch_t *b, const char *names, const int64_t *name_off, const char *quals, const char *comments,
                     const int64_t *comment_off) {
    if (!b || !names || !name_off || (comments && !comment_off)) {
        set_last_error("bwams_sam_upload: names and their offsets are required; comments come with offsets");
        return BWAMS_ERR_ARG;
    }
    if (!has(b, Product::reads) || b->nseq <= 0) {
        set_last_error("bwams_sam_upload: upload the reads first (bwams_seed_upload)");
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(b->idx->device));
    StageState *s;
    int rc = get_state(b, &s);
    if (rc) return rc;
    hipStream_t st = b->stream;
    const int64_t nseq = b->nseq, n1 = nseq + 1;
    if (name_off[0] != 0 || (comments && comment_off[0] != 0)) {
        set_last_error("bwams_sam_upload: offsets start at 0");
        return BWAMS_ERR_ARG;
    }
    outdated(b, Product::names);
    BWAMS_HIP(s->sm.names.ensure_n((size_t)name_off[nseq] + 16)); BWAMS_HIP(s->sm.noff.ensure_n((size_t)n1));
    BWAMS_HIP(hipMemcpyAsync(s->sm.names.p, names, (size_t)name_off[nseq], hipMemcpyDefault, st));
    BWAMS_HIP(hipMemcpyAsync(s->sm.noff.p, name_off, (size_t)n1 * 8, hipMemcpyHostToDevice, st));
    s->sm.has_qual = quals != nullptr;
    if (quals) {
        BWAMS_HIP(s->sm.qual.ensure_n((size_t)b->nbases + 16));
        BWAMS_HIP(hipMemcpyAsync(s->sm.qual.p, quals, (size_t)b->nbases, hipMemcpyDefault, st));
    }
    s->sm.has_comm = comments != nullptr;
    if (comments) {
        BWAMS_HIP(s->sm.comm.ensure_n((size_t)comment_off[nseq] + 16)); BWAMS_HIP(s->sm.coff.ensure_n((size_t)n1));
        BWAMS_HIP(hipMemcpyAsync(s->sm.comm.p, comments, (size_t)comment_off[nseq], hipMemcpyDefault, st));
        BWAMS_HIP(hipMemcpyAsync(s->sm.coff.p, comment_off, (size_t)n1 * 8, hipMemcpyHostToDevice, st));
    }
    BWAMS_HIP(hipStreamSynchronize(st));
    s->sm.nseq = nseq;
    produced(b, Product::names);
    return BWAMS_OK;
}

static int sam_run_impl(bwams_batch_t *b, const bwams_mem_opt_t *opt, const bwams_sam_opt_t *sopt, const bwams_pestat_t *pes,
                        int64_t *sam_bytes, bwams_emf_t *emf = nullptr) {
    const bool pe = pes != nullptr;
    if (!sopt || !has(b, Product::al) || b->stages->al.source != 1 || b->stages->pr.single == pe) {
        set_last_error(pe ? "bwams_sam_run_pe: run bwams_pair_run (paired-end) and bwams_reg2aln_run(source 1) first"
                          : "bwams_sam_run: run bwams_pair_run(BWAMS_PAIR_SINGLE_END) and bwams_reg2aln_run(source 1) first");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    if (pe && (s->ch.nseq & 1)) return BWAMS_ERR_ARG;
    if (!has(b, Product::names)) {
        set_last_error("bwams_sam_run: run bwams_sam_upload for this chunk first");
        return BWAMS_ERR_ARG;
    }
    if (!b->idx->d_ctg_names.p) {
        set_last_error("bwams_sam_run: the index has no sequence names (bwams_index_set_contig_names)");
        return BWAMS_ERR_ARG;
    }
    int rc = check_opt(opt, "bwams_sam_run");
    if (rc) return rc;
    // MEM_F_PRIMARY5 / MEM_F_NO_RESCUE act in bwams_pair_run_sam, before the text; MEM_F_NOPAIRING there and in the proper-pair flag
    if (sopt->flag & ~(BWAMS_MEM_F_ALL | BWAMS_MEM_F_NO_MULTI | BWAMS_MEM_F_SOFTCLIP | BWAMS_MEM_F_KEEP_SUPP_MAPQ | BWAMS_MEM_F_PRIMARY5 |
                       BWAMS_MEM_F_NOPAIRING | BWAMS_MEM_F_NO_RESCUE | BWAMS_MEM_F_REF_HDR)) {
        set_last_error("bwams_sam_run: MEM_F_PE / MEM_F_SMARTPE (the caller's business) and MEM_F_XB are not built");
        return BWAMS_ERR_UNSUPPORTED;
    }
    if ((sopt->flag & BWAMS_MEM_F_REF_HDR) && !b->idx->d_ctg_annos.p) {
        set_last_error("bwams_sam_run: MEM_F_REF_HDR needs the sequences' annotations (bwams_index_set_contig_annos)");
        return BWAMS_ERR_ARG;
    }
    if (!memchr(sopt->rg_id, 0, sizeof sopt->rg_id)) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    outdated(b, Product::sam); s->sm.merged_n = -1;
    const int64_t nseq = s->ch.nseq, n1 = nseq + 1, n = s->al.n;
    constexpr int kLogN = 1 << 16;
    if (!s->sm.log_ok) {                                   // log(i) with the C library's log, as the reference's host code computes it
        std::vector<double> lt((size_t)kLogN);
        for (int i = 0; i < kLogN; ++i) lt[(size_t)i] = log((double)i);
        BWAMS_HIP(s->sm.logtab.ensure_n((size_t)kLogN));
        BWAMS_HIP(hipMemcpy(s->sm.logtab.p, lt.data(), (size_t)kLogN * 8, hipMemcpyHostToDevice));
        s->sm.log_ok = true;
    }
    BWAMS_HIP(s->sm.mapq.ensure_n((size_t)(n + 1))); BWAMS_HIP(s->sm.len.ensure_n((size_t)n1)); BWAMS_HIP(s->sm.off.ensure_n((size_t)n1));
    BWAMS_HIP(s->sm.bad.ensure(64));
    SamArgs A;
    memset(&A, 0, sizeof A);
    A.regs = s->pr.out.p; A.reg_off = s->pr.ooff.p; A.n_regs = n; A.nseq = nseq; A.rec = s->al.rec.p; A.cig = s->al.cig.p; A.md = s->al.md.p;
    A.enc = b->d_enc.p; A.cum = b->d_cum.p; A.names = s->sm.names.p; A.name_off = s->sm.noff.p; A.quals = s->sm.has_qual ? s->sm.qual.p : nullptr;
    A.comments = s->sm.has_comm ? s->sm.comm.p : nullptr; A.comment_off = s->sm.has_comm ? s->sm.coff.p : nullptr;
    A.ctg_names = b->idx->d_ctg_names.as<const char>(); A.ctg_off = b->idx->d_ctg_off.as<const int32_t>();
    A.ctg_annos = b->idx->d_ctg_annos.as<const char>(); A.ctg_anno_off = b->idx->d_ctg_anno_off.as<const int32_t>(); A.opt = *opt; A.sopt = *sopt;
    A.logtab = s->sm.logtab.p; A.logtab_n = kLogN; A.coef_fac = opt->mapq_coef_len > 0 ? log((double)opt->mapq_coef_len) : 0.;
    if (emf) {
        if (!has(b, Product::er)) {
            set_last_error("bwams_sam_run_emf: run bwams_emf_run and bwams_emf_regs_run for this chunk first");
            return BWAMS_ERR_ARG;
        }
        A.er_regs = s->er.out.p; A.er_off = s->er.ooff.p; A.er_seed_len = emf->t.seed_len;
    }
    {
        DevBns bns_;
        if ((rc = dev_bns(b->idx, &bns_))) return rc;
        A.contigs = bns_.contigs;
    }
    A.pairs = pe ? s->pr.res.p : nullptr;
    if (pe) memcpy(A.pes, pes, sizeof A.pes);
    A.bns_l_pac = (b->idx->fmi.ref_seq_len - 1) / 2; A.mapq = s->sm.mapq.p; A.bad = s->sm.bad.as<unsigned long long>(); A.len = s->sm.len.p;
    A.out_off = s->sm.off.p; A.out = nullptr;
    BWAMS_HIP(hipMemsetAsync(s->sm.bad.p, 0, 24, st));
    BWAMS_HIP(hipMemsetAsync(s->sm.len.p + nseq, 0, 8, st));
    launch_sam_mapq(A, st);
    launch_sam_text(A, false, b->cu_count, st);
    if ((rc = scan_rows(b, A.len, s->sm.off.p, 1, n1))) return rc;
    int64_t total = 0;
    unsigned long long bad = 0, bad_names = 0;
    BWAMS_HIP(hipMemcpyAsync(&total, s->sm.off.p + nseq, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipMemcpyAsync(&bad, s->sm.bad.p, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipMemcpyAsync(&bad_names, s->sm.bad.as<unsigned long long>() + 2, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    if (bad_names) {
        set_last_error("bwams_sam_run_pe: paired reads have different names (" + std::to_string(bad_names) + " pair(s)); the reference stops here");
        return BWAMS_ERR_ARG;
    }
    if (bad) {
        set_last_error("bwams_sam_run: an alignment longer than 65535 bases or more than 65534 competing pairings (mapping quality table)");
        return BWAMS_ERR_UNSUPPORTED;
    }
    BWAMS_HIP(s->sm.out.ensure_n((size_t)total + 16));
    A.out = s->sm.out.p;
    launch_sam_text(A, true, b->cu_count, st);
    BWAMS_HIP(hipStreamSynchronize(st));
    BWAMS_HIP(hipGetLastError());
    s->sm.bytes = total; s->sm.nregs = n;
    if (sam_bytes) *sam_bytes = total;
    produced(b, Product::sam);
    return BWAMS_OK;
}

int bwams_sam_run(bwams_batch_t *b, const bwams_mem_opt_t *opt, const bwams_sam_opt_t *sopt, int64_t *sam_bytes) {
    return sam_run_impl(b, opt, sopt, nullptr, sam_bytes);
}

int bwams_sam_run_emf(bwams_batch_t *b, const bwams_mem_opt_t *opt, const bwams_sam_opt_t *sopt, bwams_emf_t *emf, int64_t *sam_bytes) {
    if (!emf) return BWAMS_ERR_ARG;
    return sam_run_impl(b, opt, sopt, nullptr, sam_bytes, emf);
}

int bwams_sam_run_pe(bwams_batch_t *b, const bwams_mem_opt_t *opt, const bwams_sam_opt_t *sopt, const bwams_pestat_t pes[4],
                     int64_t *sam_bytes) {
    if (!pes) return BWAMS_ERR_ARG;
    return sam_run_impl(b, opt, sopt, pes, sam_bytes);
}

int bwams_sam_fetch(bwams_batch_t *b, char *sam, int64_t cap, int64_t *read_off, int32_t *mapq, int64_t mapq_cap) {
    if (!has(b, Product::sam)) {
        set_last_error("bwams_sam_fetch: run bwams_sam_run first");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    if ((sam && s->sm.bytes > cap) || (mapq && s->sm.nregs > mapq_cap)) return BWAMS_ERR_CAPACITY;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    if (sam && s->sm.bytes) BWAMS_HIP(hipMemcpyAsync(sam, s->sm.out.p, (size_t)s->sm.bytes, hipMemcpyDeviceToHost, st));
    const int64_t n_out = s->sm.merged_n >= 0 ? s->sm.merged_n : s->ch.nseq;
    if (read_off) BWAMS_HIP(hipMemcpyAsync(read_off, s->sm.off.p, (size_t)(n_out + 1) * 8, hipMemcpyDeviceToHost, st));
    if (mapq && s->sm.nregs) BWAMS_HIP(hipMemcpyAsync(mapq, s->sm.mapq.p, (size_t)s->sm.nregs * 4, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    return BWAMS_OK;
}

int bwams_sam_fetch_bgzf(bwams_batch_t *b, bwams_deflater_t *d, void *out, int64_t cap, int32_t flags, int64_t *n_out) {
    if (!d || !has(b, Product::sam)) {
        set_last_error("bwams_sam_fetch_bgzf: run bwams_sam_run first");
        return BWAMS_ERR_ARG;
    }
    if (deflater_device(d) != b->idx->device) {
        set_last_error("bwams_sam_fetch_bgzf: the deflater is on device " + std::to_string(deflater_device(d)) + ", the batch on device " +
                       std::to_string(b->idx->device));
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    return deflater_run_after(d, b->stream, s->sm.out.p, s->sm.bytes, 1, out, cap, 0, flags, n_out, nullptr);
}
}  // extern "C"
