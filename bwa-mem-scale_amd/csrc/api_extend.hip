// api_extend.hip — C-ABI entry points of the chain-to-alignment stage (include/bwams.h): the plan, the task builds (ext_*), one
// side's banded SW with its retries (run_side), bwams_extend_build, _run, _fetch and _tasks_fetch, over ext_aln.hip and
// bsw_extend.hip on the batch's stream.  No CPU fallback: every entry point runs HIP kernels or returns an error.
#include <cstddef>

#include "stage_state.h"

using namespace bwams;

extern "C" {
static int ext_args(bwams_batch *b, StageState *s, const bwams_mem_opt_t *opt, ExtArgs *A) {
    const int64_t n1 = s->ch.nseq + 1;
    A->chains = s->ch.chains.p; A->n_chains = s->ch.n_chains; A->seeds = s->ch.seeds.p; A->n_seeds = s->ch.n_seeds;
    A->chain_off = s->ch.chain_off.as<int64_t>(); A->seed_off = s->ch.chain_off.as<int64_t>() + n1; A->enc = b->d_enc.p; A->cum = b->d_cum.p;
    A->nseq = s->ch.nseq; A->ref = b->idx->fmi.ref;
    int rc = dev_bns(b->idx, &A->bns);
    if (rc) return rc;
    A->opt = *opt; A->regs = s->ext.regs.p; A->srt = s->ext.srt.p; A->rmax = s->ext.rmax.as<int64_t>(); A->cnt = s->ext.cnt.as<int32_t>();
    A->ctr = b->d_ctr.p; A->state = s->ext.state.p; A->kreg = s->ext.kreg.p; A->cur = s->ext.cur.p; A->lim = s->ext.lim.p; A->sel_heavy = s->heavy.p;
    A->n_sel_heavy = &b->d_ctr.p->sel_heavy; A->sel_ticket = b->d_ctr.p->ext_sel_ticket; A->req_list = s->ext.req_list.p; A->rtask = nullptr;
    return BWAMS_OK;
}

// The counters of one round (DevCounters: ext_n_req .. ext_n_retry) are one block: one memset clears them.
static hipError_t ext_round_clear(bwams_batch *b) {
    DevCounters *c = b->d_ctr.p;
    return hipMemsetAsync(&c->ext_n_req, 0, (size_t)((char *)(c->ext_n_retry + 2) - (char *)&c->ext_n_req), b->stream);
}
// ... and what the host needs of them — requests, slots behind them, the requests' left and right tasks — is one copy.
static int ext_round_fetch(bwams_batch *b, int64_t *n_req, int64_t *n_rest, int64_t *n_l, int64_t *n_r) {
    DevCounters *h = b->h_ctr.p;
    BWAMS_HIP(hipMemcpyAsync(&h->ext_n_req, &b->d_ctr.p->ext_n_req, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, b->stream));
    BWAMS_HIP(hipStreamSynchronize(b->stream));
    *n_req = (int64_t)h->ext_n_req; *n_rest = (int64_t)h->ext_n_rest;
    *n_l = (int64_t)(h->ext_n_tasks & 0xffffffffull); *n_r = (int64_t)(h->ext_n_tasks >> 32);
    return BWAMS_OK;
}

// allocate the per-seed arrays and run the plan kernel (windows, seed order, regions, task sizes, the first requests)
static int ext_plan(bwams_batch *b, StageState *s, const bwams_mem_opt_t *opt, int extend_all, ExtArgs *A) {
    const int64_t N1 = s->ch.n_seeds + 1, n1 = s->ch.nseq + 1;
    BWAMS_HIP(s->ext.regs.ensure_n((size_t)N1)); BWAMS_HIP(s->ext.srt.ensure_n((size_t)N1));
    BWAMS_HIP(s->ext.rmax.ensure((size_t)(s->ch.n_chains + 1) * 16)); BWAMS_HIP(s->ext.cnt.ensure((size_t)N1 * 6 * 4));
    BWAMS_HIP(s->ext.state.ensure_n((size_t)N1)); BWAMS_HIP(s->ext.kreg.ensure((size_t)N1 * 32)); BWAMS_HIP(s->ext.cur.ensure_n((size_t)n1));
    BWAMS_HIP(s->ext.lim.ensure_n((size_t)n1)); BWAMS_HIP(s->heavy.ensure_n((size_t)n1));
    // the request list: a slot is requested at most once in a run, so every slot fits; entries beyond the cursor of the round in
    // hand (a larger chunk's, an earlier round's) are never read
    BWAMS_HIP(s->ext.req_list.ensure_n((size_t)N1)); BWAMS_HIP(s->ext.rtask.ensure_n((size_t)N1));
    int rc = ext_args(b, s, opt, A);
    if (rc) return rc;
    BWAMS_HIP(hipMemsetAsync(&b->d_ctr.p->sel_heavy, 0, sizeof(unsigned long long), b->stream));
    BWAMS_HIP(ext_round_clear(b));
    launch_ext_heavy_list(*A, b->stream);
    BWAMS_HIP(hipMemsetAsync(s->ext.cur.p, 0, (size_t)n1 * 4, b->stream));
    BWAMS_HIP(hipMemsetAsync(s->ext.lim.p, 0, (size_t)n1 * 4, b->stream));
    launch_ext_plan(*A, extend_all, b->stream);
    return BWAMS_OK;
}

// Tasks in flat buffers (the SeqPair boundary): the six rows of task sizes of n slots — list[i], or with list == nullptr the requested
// ones among all n = n_seeds slots — are scanned for task indices and byte offsets, so the tasks come in the order of the slots given.
static int ext_build_flat(bwams_batch *b, StageState *s, const ExtArgs &A, const int32_t *list, int64_t n, int64_t tot[6]) {
    hipStream_t st = b->stream;
    const int64_t n1 = n + 1;
    BWAMS_HIP(s->ext.ewide.ensure((size_t)n1 * 6 * 8)); BWAMS_HIP(s->ext.eoffs.ensure((size_t)n1 * 6 * 8));
    launch_ext_widen(A, list, n, s->ext.ewide.as<int64_t>(), st);
    int rc = scan_rows(b, s->ext.ewide.as<int64_t>(), s->ext.eoffs.as<int64_t>(), 6, n1);
    if (rc) return rc;
    for (int r = 0; r < 6; ++r) BWAMS_HIP(hipMemcpyAsync(&tot[r], s->ext.eoffs.as<int64_t>() + r * n1 + n, 8, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    for (int r : {1, 2, 4, 5})
        if (tot[r] >= ((int64_t)1 << 31)) {
            set_last_error("extension task buffers exceed the 31-bit offsets of SeqPair; use smaller chunks");
            return BWAMS_ERR_CAPACITY;
        }
    s->ext.n_left = tot[0]; s->ext.lqer_b = tot[1]; s->ext.lref_b = tot[2];
    s->ext.n_right = tot[3]; s->ext.rqer_b = tot[4]; s->ext.rref_b = tot[5];
    BWAMS_HIP(s->ext.lpairs.ensure_n((size_t)(tot[0] + 1))); BWAMS_HIP(s->ext.rpairs.ensure_n((size_t)(tot[3] + 1)));
    const int64_t mx = tot[0] > tot[3] ? tot[0] : tot[3];
    BWAMS_HIP(s->ext.retry.ensure_n((size_t)(mx + 1)));
    s->ext.tasks_inplace = false;
    BWAMS_HIP(s->ext.lqer.ensure_n((size_t)tot[1] + 64)); BWAMS_HIP(s->ext.lref.ensure_n((size_t)tot[2] + 64));
    BWAMS_HIP(s->ext.rqer.ensure_n((size_t)tot[4] + 64)); BWAMS_HIP(s->ext.rref.ensure_n((size_t)tot[5] + 64));
    if (tot[0] + tot[3] > 0)
        launch_ext_build(A, list, n, s->ext.eoffs.as<int64_t>(), s->ext.lpairs.p, s->ext.lref.p, s->ext.lqer.p, s->ext.rpairs.p, s->ext.rref.p,
                         s->ext.rqer.p, nullptr, nullptr, st);
    return BWAMS_OK;
}

// One round's tasks, built from the request list: n_req slots with n_l left and n_r right tasks, all three known to the host from the
// round trip that ended the previous round (or followed the plan).  In place nothing is scanned and nothing but the list is read:
// the build reserves task indices as it goes.  BWAMS_EXT_INPLACE=0 scans the requested slots' sizes for the flat buffers' offsets.
static int ext_build_round(bwams_batch *b, StageState *s, const ExtArgs &A, int64_t n_req, int64_t n_l, int64_t n_r, bool inplace) {
    if (!inplace) {
        int64_t tot[6] = {0, 0, 0, 0, 0, 0};
        if (int rc = ext_build_flat(b, s, A, A.req_list, n_req, tot)) return rc;
        if (tot[0] != n_l || tot[3] != n_r) {
            set_last_error("bwams_extend_run: the request list and its task counters disagree");
            return BWAMS_ERR_DEVICE;
        }
        return BWAMS_OK;
    }
    s->ext.n_left = n_l; s->ext.n_right = n_r;
    s->ext.lqer_b = s->ext.lref_b = s->ext.rqer_b = s->ext.rref_b = 0;
    BWAMS_HIP(s->ext.lpairs.ensure_n((size_t)(n_l + 1))); BWAMS_HIP(s->ext.rpairs.ensure_n((size_t)(n_r + 1)));
    const int64_t mx = n_l > n_r ? n_l : n_r;
    BWAMS_HIP(s->ext.retry.ensure_n((size_t)(mx + 1)));
    s->ext.tasks_inplace = true;               // no bytes are copied: 16 bytes of offsets per task
    BWAMS_HIP(s->ext.lsrc.ensure((size_t)(n_l + 1) * 16)); BWAMS_HIP(s->ext.rsrc.ensure((size_t)(n_r + 1) * 16));
    if (n_l + n_r > 0) launch_ext_build(A, A.req_list, n_req, nullptr, s->ext.lpairs.p, nullptr, nullptr, s->ext.rpairs.p,
                         nullptr, nullptr, s->ext.lsrc.as<int64_t>(), s->ext.rsrc.as<int64_t>(), b->stream);
    return BWAMS_OK;
}

int bwams_extend_build(bwams_batch_t *b, const bwams_mem_opt_t *opt, int64_t *n_left, int64_t *n_right) {
    if (!has(b, Product::chains)) {
        set_last_error("bwams_extend_build: run bwams_chain_run (or bwams_chain_upload) first");
        return BWAMS_ERR_ARG;
    }
    if (!b->idx->fmi.ref) {
        set_last_error("bwams_extend_build: the index was opened without its .0123 reference");
        return BWAMS_ERR_ARG;
    }
    int rc = check_opt(opt, "bwams_extend_build");
    if (rc) return rc;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    StageState *s = b->stages;
    outdated(b, Product::built);
    hipStream_t st = b->stream;
    ExtArgs A;
    BWAMS_HIP(hipEventRecord(s->ev[2], st));
    if ((rc = ext_plan(b, s, opt, 1, &A))) return rc;           // every seed, as the reference builds them
    int64_t tot[6];
    if ((rc = ext_build_flat(b, s, A, nullptr, s->ch.n_seeds, tot))) return rc;
    BWAMS_HIP(hipEventRecord(s->ev[3], st));
    BWAMS_HIP(hipGetLastError());
    s->opt = *opt;
    if (n_left) *n_left = tot[0];
    if (n_right) *n_right = tot[3];
    produced(b, Product::built);
    return BWAMS_OK;
}

// one side: extend at w, settle, re-run the unsettled tasks at 2w (MAX_BAND_TRY = 2, bwamem.cpp:79)
static int run_side(bwams_batch *b, StageState *s, const ExtArgs &A, int right, int64_t *n_retry_out) {
    hipStream_t st = b->stream;
    bwams_seqpair_t *pairs = right ? s->ext.rpairs.p : s->ext.lpairs.p;
    // in place: the sequences are read where they lie (the chunk's base codes, the resident .0123 text), backwards on the left side
    const bool ip = s->ext.tasks_inplace;
    const uint8_t *ref = ip ? A.ref : (right ? s->ext.rref.p : s->ext.lref.p);
    const uint8_t *qer = ip ? A.enc : (right ? s->ext.rqer.p : s->ext.lqer.p);
    const int64_t *src = ip ? (right ? s->ext.rsrc.as<int64_t>() : s->ext.lsrc.as<int64_t>()) : nullptr;
    const int dir = ip && !right ? -1 : 1;
    const int64_t n = right ? s->ext.n_right : s->ext.n_left;
    SwParams prm;
    sw_params(A.opt, right ? A.opt.pen_clip3 : A.opt.pen_clip5, &prm);
    const int qmax = b->max_read_len > 1 ? b->max_read_len : 1;
    if (n == 0) return BWAMS_OK;
    unsigned long long *d_nretry = &b->d_ctr.p->ext_n_retry[right], *h_nretry = &b->h_ctr.p->ext_n_retry[right];   // cleared with the round's counters
    bwams_seqpair_t *rp = A.rtask ? s->ext.rpairs.p : nullptr;       // a settled left task hands its score to the slot's right task
    if (bsw_list_bytes(n) > b->sw.d_bsw_list.cap) BWAMS_HIP(hipStreamSynchronize(st));   // the last launch may still read the lists
    BWAMS_HIP(b->sw.d_bsw_list.ensure(bsw_list_bytes(n), bsw_list_bytes(n + n / 4 + 1024)));
    const bool verbose_bsw = knobs().verbose != 0;
    const bool early = knobs().bsw_early != 0;          // a task stops once no later row can change its result (BWAMS_BSW_EARLY=0: every row)
    if (verbose_bsw) BWAMS_HIP(hipMemsetAsync(b->d_ctr.p->dbg + 40, 0, 10 * sizeof(unsigned long long), st));
    if (int lrc = launch_bsw(pairs, n, ref, qer, A.opt.w, prm, qmax, b->d_ctr.p, b->cu_count, st, b->sw.d_bsw_list.p, s->aux, s->fork, s->join, src, dir, early)) {
        set_last_error(lrc == -2 ? "banded SW: a query longer than ~18000 bases does not fit the LDS kernel" : "banded SW: stream fork/join failed");
        return lrc == -2 ? BWAMS_ERR_UNSUPPORTED : BWAMS_ERR_DEVICE;
    }
    launch_ext_post(A, right, pairs, n, A.opt.w, 0, s->ext.retry.p, d_nretry, rp, st);
    BWAMS_HIP(hipMemcpyAsync(h_nretry, d_nretry, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    if (verbose_bsw) {               // filled only by a build of bsw_extend.hip with -DBWAMS_BSWDBG
        unsigned long long d[10];
        BWAMS_HIP(hipMemcpy(d, b->d_ctr.p->dbg + 40, sizeof d, hipMemcpyDeviceToHost));
        if (d[6])
            fprintf(stderr, "[run_side] bsw_pk_kernel, %s, %lld tasks: %llu waves, Mticks of wave-time %.2f, in the refill branch %.2f (%.1f %%), in the pass %.2f; "
                            "%llu refill events, %llu slots filled, %llu iterations, %llu rows, %llu tasks ended early\n",
                    right ? "right" : "left", (long long)n, d[6], d[0] / 1e6, d[1] / 1e6, 100. * (double)d[1] / (double)d[0], d[2] / 1e6, d[3], d[4], d[5], d[7], d[8]);
    }
    const unsigned long long nr = *h_nretry;
    if (nr) {
        if (launch_bsw(s->ext.retry.p, (int64_t)nr, ref, qer, A.opt.w << 1, prm, qmax, b->d_ctr.p, b->cu_count, st, b->sw.d_bsw_list.p, s->aux, s->fork, s->join, src, dir, early)) return BWAMS_ERR_DEVICE;
        launch_ext_post(A, right, s->ext.retry.p, (int64_t)nr, A.opt.w << 1, 1, nullptr, d_nretry, rp, st);
    }
    *n_retry_out += (int64_t)nr;
    return BWAMS_OK;
}

// Rounds of (build the requested tasks, extend left, extend right, select).  Round 0 extends the first
// seed visited of every chain; a later round extends the seeds the selection found it must keep but
// that had not been extended yet.  After kMaxRounds everything still undecided is extended at once.
//
// A round costs what it extends, not what the chunk holds: whoever requests a slot (the plan, the selection, the
// extend-the-rest kernel) appends it to the request list and adds its task counts to the round's counters, the build
// starts a lane per list entry and reserves task indices as it goes (the order of the tasks inside a round is
// unspecified; results go back by (seqid, regid)), and one copy of three words after the selection tells the host
// whether another round runs and how large its buffers must be.  The host waits three times per round: after each
// side for the retry count (the right side starts from the left side's settled scores), after the selection for
// the next round's sizes — and once after the plan, once more when the rest is requested.  One list serves every
// round: a round's build has consumed it before that round's selection, which alone appends, clears its cursor.
int bwams_extend_run(bwams_batch_t *b, const bwams_mem_opt_t *opt, int64_t *n_regs) {
    if (!has(b, Product::chains)) {
        set_last_error("bwams_extend_run: run bwams_chain_run (or bwams_chain_upload) first");
        return BWAMS_ERR_ARG;
    }
    if (!b->idx->fmi.ref) {
        set_last_error("bwams_extend_run: the index was opened without its .0123 reference");
        return BWAMS_ERR_ARG;
    }
    int rc = check_opt(opt, "bwams_extend_run");
    if (rc) return rc;
    int kMaxRounds = 6;
    if (knobs().ext_max_rounds > 0) kMaxRounds = knobs().ext_max_rounds;      // test knob: force the extend-the-rest fallback
    const bool adaptive_off = knobs().ext_all_rounds != 0;                    // test knob: never cut the rounds short
    const bool inplace_on = knobs().ext_inplace != 0;                          // A-B knob: 0 = copy the tasks' bytes into flat buffers
    StageState *s = b->stages;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    outdated(b, Product::built);                                // the run plans and builds its own tasks over the flat lists' buffers
    ExtArgs A;
    BWAMS_HIP(hipEventRecord(s->ev[10], st));
    BWAMS_HIP(hipMemsetAsync(&b->d_ctr.p->bsw_cells, 0, sizeof(unsigned long long), st));      // DP cells of this run, all rounds
    BWAMS_HIP(hipEventRecord(s->ev[2], st));
    if ((rc = ext_plan(b, s, opt, opt->extend_all != 0, &A))) return rc;
    A.rtask = s->ext.rtask.p;
    int64_t tot_left = 0, tot_right = 0;
    s->ext.n_retry_left = s->ext.n_retry_right = 0;
    int64_t n_req = 0, n_rest = 0, n_l = 0, n_r = 0;          // what the round in hand builds: known before it starts
    if ((rc = ext_round_fetch(b, &n_req, &n_rest, &n_l, &n_r))) return rc;
    int round = 0;
    for (;; ++round) {
        if ((rc = ext_build_round(b, s, A, n_req, n_l, n_r, inplace_on))) return rc;
        if (round == 0) { BWAMS_HIP(hipEventRecord(s->ev[3], st)); BWAMS_HIP(hipEventRecord(s->ev[4], st)); }
        tot_left += n_l; tot_right += n_r;
        if ((rc = run_side(b, s, A, 0, &s->ext.n_retry_left))) return rc;
        if (round == 0) { BWAMS_HIP(hipEventRecord(s->ev[5], st)); BWAMS_HIP(hipEventRecord(s->ev[6], st)); }
        if ((rc = run_side(b, s, A, 1, &s->ext.n_retry_right))) return rc;
        if (round == 0) { BWAMS_HIP(hipEventRecord(s->ev[7], st)); BWAMS_HIP(hipEventRecord(s->ev[8], st)); }
        BWAMS_HIP(ext_round_clear(b));                         // the list's cursor, the task counts, the build's and the walk's cursors, the retry counts
        const bool verbose_sel = knobs().verbose != 0;
        if (verbose_sel) BWAMS_HIP(hipMemsetAsync(b->d_ctr.p->dbg, 0, sizeof b->d_ctr.p->dbg, st));
        if (s->ch.n_seeds && launch_ext_select(A, b->cu_count, st, s->aux, s->fork, s->join)) {
            set_last_error("bwams_extend_run: stream fork/join failed");
            return BWAMS_ERR_DEVICE;
        }
        if (verbose_sel) {           // filled only by a build of ext_aln.hip with -DBWAMS_SELDBG
            unsigned long long d[16];
            BWAMS_HIP(hipMemcpyAsync(d, b->d_ctr.p->dbg, sizeof d, hipMemcpyDeviceToHost, st));
            BWAMS_HIP(hipStreamSynchronize(st));
            if (d[0])
                fprintf(stderr, "[bwams_extend_run] selection walk, round %d: %llu reads, Mticks total %.2f fetch %.2f bulk scan %.2f ordered part %.2f (of it keep-anyway %.2f); "
                                "%llu slots, %llu keep-anyway calls; longest read: %.3f Mticks (fetch %.3f bulk %.3f ordered %.3f, of it keep-anyway %.3f), %llu slots "
                                "%llu calls, %llu kept regions\n",
                        round, d[0], d[1] / 1e6, d[2] / 1e6, d[3] / 1e6, d[4] / 1e6, d[5] / 1e6, d[6], d[7], d[8] / 1e6, d[9] / 1e6, d[10] / 1e6, d[11] / 1e6,
                        d[12] / 1e6, d[13], d[14], d[15]);
        }
        if (round == 0) BWAMS_HIP(hipEventRecord(s->ev[9], st));
        if ((rc = ext_round_fetch(b, &n_req, &n_rest, &n_l, &n_r))) return rc;
        if (n_req == 0) break;
        // A round costs the launches and the selection's walk of the heaviest reads whatever it holds.  When the seeds still
        // undecided — at most n_rest, the slots behind this round's requests — are few beside what
        // has been extended already, extending them all now (as the reference does with every seed) is cheaper than the rounds
        // that would sort out which of them are dead.
        const bool few_left = !adaptive_off && (n_req + n_rest) * 32 < tot_left + tot_right;
        if (round + 1 >= kMaxRounds || few_left) {
            launch_ext_request_rest(A, st);                    // appends behind the selection's requests
            if ((rc = ext_round_fetch(b, &n_req, &n_rest, &n_l, &n_r))) return rc;
        }
    }
    BWAMS_HIP(hipEventRecord(s->ev[11], st));
    BWAMS_HIP(hipGetLastError());
    s->ext.n_rounds = round + 1;
    s->ext.n_left = tot_left; s->ext.n_right = tot_right;
    s->opt = *opt;
    if (n_regs) *n_regs = s->ch.n_seeds;
    produced(b, Product::ext);
    return BWAMS_OK;
}

int bwams_extend_fetch(bwams_batch_t *b, bwams_alnreg_t *regs, int64_t reg_cap, int64_t *reg_off, int32_t *seed_aln) {
    if (!has(b, Product::ext) && !has(b, Product::built)) {
        set_last_error("bwams_extend_fetch: no regions on the device");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    if (s->ch.n_seeds > reg_cap) return BWAMS_ERR_CAPACITY;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    if (s->ch.n_seeds) BWAMS_HIP(hipMemcpyAsync(regs, s->ext.regs.p, (size_t)s->ch.n_seeds * sizeof(bwams_alnreg_t), hipMemcpyDeviceToHost, st));
    if (reg_off) BWAMS_HIP(hipMemcpyAsync(reg_off, s->ch.chain_off.as<int64_t>() + (s->ch.nseq + 1), (size_t)(s->ch.nseq + 1) * 8, hipMemcpyDeviceToHost, st));
    if (seed_aln && s->ch.n_seeds)
        BWAMS_HIP(hipMemcpy2DAsync(seed_aln, 4, reinterpret_cast<const char *>(s->ch.seeds.p) + offsetof(bwams_chain_seed_t, aln),
                                   sizeof(bwams_chain_seed_t), 4, (size_t)s->ch.n_seeds, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    return BWAMS_OK;
}

int bwams_extend_tasks_fetch(bwams_batch_t *b, int32_t side, bwams_seqpair_t *pairs, int64_t pair_cap, uint8_t *ref,
                             int64_t ref_cap, uint8_t *qer, int64_t qer_cap, int64_t *n_pairs, int64_t *ref_bytes,
                             int64_t *qer_bytes) {
    if ((!has(b, Product::built) && !has(b, Product::ext)) || (side != 0 && side != 1)) {
        set_last_error("bwams_extend_tasks_fetch: no task lists on the device");
        return BWAMS_ERR_ARG;
    }
    if (b->stages->ext.tasks_inplace) {
        set_last_error("bwams_extend_tasks_fetch: bwams_extend_run extends in place and builds no flat task buffers; bwams_extend_build does");
        return BWAMS_ERR_ARG;
    }
    StageState *s = b->stages;
    const int64_t n = side ? s->ext.n_right : s->ext.n_left, rb = side ? s->ext.rref_b : s->ext.lref_b, qb = side ? s->ext.rqer_b : s->ext.lqer_b;
    if (n_pairs) *n_pairs = n;
    if (ref_bytes) *ref_bytes = rb;
    if (qer_bytes) *qer_bytes = qb;
    if (n > pair_cap || rb > ref_cap || qb > qer_cap) return BWAMS_ERR_CAPACITY;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    if (n) BWAMS_HIP(hipMemcpyAsync(pairs, side ? s->ext.rpairs.p : s->ext.lpairs.p, (size_t)n * sizeof(bwams_seqpair_t), hipMemcpyDeviceToHost, st));
    if (rb) BWAMS_HIP(hipMemcpyAsync(ref, side ? s->ext.rref.p : s->ext.lref.p, (size_t)rb, hipMemcpyDeviceToHost, st));
    if (qb) BWAMS_HIP(hipMemcpyAsync(qer, side ? s->ext.rqer.p : s->ext.lqer.p, (size_t)qb, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    return BWAMS_OK;
}
}  // extern "C"
