// api_seed.hip — C-ABI entry points of seeding (include/bwams.h): the reads made resident (bwams_seed_upload), a pass over the
// FM-index (bwams_seed_run) or over an ERT (bwams_seed_run_ert), each run again with grown buffers when the chunk needs more, and
// the counts and results of the pass (bwams_seed_counts, bwams_seed_fetch; bwams_seed_fmi = all of it in one call).
#include <algorithm>
#include <cstring>
#include <mutex>

#include <rocprim/rocprim.hpp>

#include "fmi_kernels.h"
#include "ert_kernels.h"
#include "stage_state.h"

namespace bwams {

// (re)allocate every buffer whose size follows max_smem; the batch grows them when a chunk needs more
int alloc_smem_buffers(bwams_batch *b, int64_t max_smem) {
    b->sd.d_pool.release(); b->sd.d_sorted.release(); b->sd.d_keys.release(); b->sd.d_keys2.release(); b->sd.d_vals.release();   // all of the old set
    b->sd.d_vals2.release(); b->sd.d_work2.release(); b->sd.d_sa_off.release(); b->sd.d_sa_cnt.release();                     // goes first
    b->max_smem = max_smem;
    // the pool is handed out in per-wave chunks: room for every wave's partly filled last chunk
    // of each of the five emitting launches on top of the max_smem real records
    b->pool_cap = b->max_smem + seed_pool_slack(b->cu_count);
    BWAMS_HIP(b->sd.d_pool.alloc((size_t)b->pool_cap * sizeof(bwams_smem_t)));
    BWAMS_HIP(b->sd.d_sorted.alloc((size_t)b->max_smem * sizeof(bwams_smem_t)));
    BWAMS_HIP(b->sd.d_keys.alloc((size_t)b->pool_cap * 8));
    BWAMS_HIP(b->sd.d_keys2.alloc((size_t)b->pool_cap * 8));
    BWAMS_HIP(b->sd.d_vals.alloc((size_t)b->pool_cap * 4));
    BWAMS_HIP(b->sd.d_vals2.alloc((size_t)b->pool_cap * 4));
    BWAMS_HIP(b->sd.d_work2.alloc((size_t)b->pool_cap * sizeof(Round2Work)));
    BWAMS_HIP(b->sd.d_sa_off.alloc((size_t)(b->max_smem + 1) * 8));
    BWAMS_HIP(b->sd.d_sa_cnt.alloc((size_t)(b->max_smem + 1) * 8));
    return BWAMS_OK;
}

// rocPRIM temporary storage for the largest sort / scan this batch can issue
int alloc_seed_tmp(bwams_batch *b) {
    size_t t1 = 0, t2 = 0;
    (void)rocprim::radix_sort_pairs(nullptr, t1, b->sd.d_keys.p, b->sd.d_keys2.p, b->sd.d_vals.p, b->sd.d_vals2.p,
                              (size_t)b->max_smem, 0, 64, b->stream);
    (void)rocprim::exclusive_scan(nullptr, t2, b->sd.d_sa_cnt.p, b->sd.d_sa_off.p, (int64_t)0, (size_t)b->max_smem + 1,
                            rocprim::plus<int64_t>(), b->stream);
    BWAMS_HIP(b->d_tmp.alloc(std::max(t1, t2)));
    return BWAMS_OK;
}

namespace {

// The tail of a pass: n_keys pool slots (the FM-index pass: holes included) sorted by key, the n real records gathered in (rid, m, n) order
int sort_pool(bwams_batch *b, const char *who, int64_t n_keys, int64_t n, int64_t *sa_cnt, int max_occ) {
    bwams_batch::Seed &sd = b->sd;
    hipStream_t st = b->stream;
    // key = rid << 2w | m << w | n; chunk holes carry rid = nseq and sort behind every read.  m and n are positions in a read: w = 8
    // when the batch's longest read has at most 255 bases (36 key bits for a chunk of 1 M 150-base reads, 52 with w = 16)
    const int w = b->max_read_len <= 255 && knobs().sort_narrow ? 8 : 16;
    launch_make_keys(sd.d_pool.p, n_keys, sd.d_keys.p, sd.d_vals.p, (uint32_t)b->nseq, w, st);
    int rid_bits = 1;
    while (((int64_t)1 << rid_bits) <= b->nseq) rid_bits++;
    if (int rc = with_tmp(b, who, [&](void *tmp, size_t &tb) {     // the temporary size depends on the size / bit range: ask for this call
            return rocprim::radix_sort_pairs(tmp, tb, sd.d_keys.p, sd.d_keys2.p, sd.d_vals.p, sd.d_vals2.p, (size_t)n_keys, 0, 2 * w + rid_bits, st);
        })) return rc;
    launch_gather_sorted(sd.d_pool.p, sd.d_vals2.p, n, sd.d_sorted.p, sa_cnt, max_occ, st);
    return BWAMS_OK;
}

// The lookups of the last pass' n sorted SMEMs, as the pass and the re-run behind a grown SA buffer (bwams_seed_counts) launch them
// The index's dense table is read and the kernel that reads it launched under the shared lock: a release on another thread then
// waits for this launch before it frees (api_index.hip: sa_dense_release).  Nothing allocates in here.
void fm_lookup(bwams_batch *b, int64_t n) {
    bwams_batch::Seed &sd = b->sd;
    bwams_index *ix = b->idx;
    std::shared_lock<std::shared_mutex> lock(ix->sa_mu);
    const bool use = ix->sa_state == BWAMS_SA_DENSE_BUILT && knobs().sa_dense != 0;
    launch_sa_lookup(ix->fmi, sd.d_sorted.p, n, sd.d_sa_off.p, sd.d_sa_coord.p, b->max_sa, sd.last_opt.max_occ, b->d_ctr.p, b->cu_count, b->stream,
                     use ? ix->d_sa_dense.as<const uint64_t>() : nullptr, ix->sa_stride);
}
void ert_locate(bwams_batch *b, int64_t n) {
    bwams_batch::Seed &sd = b->sd;
    launch_ert_locate(sd.ert->t, b->d_enc.p, b->d_cum.p, sd.d_sorted.p, n, sd.with_sa ? sd.d_sa_cnt.p : nullptr, sd.last_opt.max_occ, b->d_ctr.p,
                      sd.d_ert_stk.p, sd.ert_stk_frames, b->cu_count, b->stream);
}
int ert_gather(bwams_batch *b, int64_t n) {
    bwams_batch::Seed &sd = b->sd;
    const int64_t cap = n + n / 4 + 1024;                   // the seeds to redo: a bit per seed
    BWAMS_HIP(sd.d_ert_redo.ensure((size_t)((n + 31) / 32) * 4, (size_t)((cap + 31) / 32) * 4));
    launch_ert_gather(sd.ert->t, sd.d_sorted.p, n, sd.d_sa_off.p, sd.d_sa_coord.p, b->max_sa, sd.last_opt.max_occ, b->d_ctr.p, sd.d_ert_stk.p,
                      sd.ert_stk_frames, sd.d_ert_redo.p, b->max_sa, b->cu_count, b->stream);
    return BWAMS_OK;
}

// The SMEM and SA buffers grow on demand: the kernels keep counting when a buffer is full, so one
// overflowing pass tells the size the chunk needs and the stage is simply run again.
template <class F> int run_growing(bwams_batch *b, F &&once) {
    int rc = once();
    if (rc == BWAMS_ERR_CAPACITY && (b->sd.n_smem > b->max_smem || b->sd.n_pool_slots > b->pool_cap)) {
        BWAMS_HIP(hipStreamSynchronize(b->stream));
        // the slots handed out (holes included) bound what the chunk needs whatever filled the pool
        const int64_t seen = std::max(b->sd.n_smem, b->sd.n_pool_slots - seed_pool_slack(b->cu_count));
        const int64_t need = std::max(seen, b->max_smem) + seen / 4 + 1024;
        if ((rc = alloc_smem_buffers(b, need))) return rc;
        b->d_tmp.release();                         // rocPRIM scratch is re-queried per call
        rc = once();
    }
    return rc;
}

}  // namespace
}  // namespace bwams

using namespace bwams;

extern "C" {

int bwams_seed_upload(bwams_batch_t *b, const uint8_t *enc, const int64_t *cum, const uint8_t *skip,
                      int64_t nseq) {
    if (!b || !enc || !cum || nseq < 0) return BWAMS_ERR_ARG;
    if (nseq > b->max_reads) {
        set_last_error("bwams_seed_upload: more reads than the batch was created for");
        return BWAMS_ERR_CAPACITY;
    }
    const int64_t base0 = cum[0];
    const int64_t nb = cum[nseq] - base0;
    if (base0 != 0 || nb > b->max_bases || nb < 0) {
        set_last_error("bwams_seed_upload: cum_len must start at 0 and fit max_bases");
        return nb > b->max_bases ? BWAMS_ERR_CAPACITY : BWAMS_ERR_ARG;
    }
    int mx = 0;
    for (int64_t i = 0; i < nseq; ++i) {
        const int64_t l = cum[i + 1] - cum[i];
        if (l < 0 || l > 0xfffe) {
            set_last_error("bwams_seed_upload: read length must be in [0, 65534]");
            return BWAMS_ERR_UNSUPPORTED;
        }
        if (l > mx) mx = (int)l;
    }
    outdated(b, Product::reads);
    BWAMS_HIP(hipSetDevice(b->idx->device));
    b->nseq = nseq;
    b->nbases = nb;
    b->max_read_len = mx;
    b->has_skip = skip != nullptr;
    // enc may already live in this GPU's memory (a caller that keeps several chunks resident): the copy kind is inferred
    if (nb) BWAMS_HIP(hipMemcpyAsync(b->d_enc.p, enc, (size_t)nb, hipMemcpyDefault, b->stream));
    BWAMS_HIP(hipMemcpyAsync(b->d_cum.p, cum, (size_t)(nseq + 1) * 8, hipMemcpyHostToDevice, b->stream));
    if (skip && nseq) BWAMS_HIP(hipMemcpyAsync(b->d_skip.p, skip, (size_t)nseq, hipMemcpyHostToDevice, b->stream));
    // the source buffers belong to the caller: do not return before they are consumed
    BWAMS_HIP(hipStreamSynchronize(b->stream));

    // packed form of the reads: 16 bases per code word + 32 bases per N-mask word, padded to 4 words
    {
        const int cw = (mx + 15) / 16, mw = (mx + 31) / 32;
        int W = ((cw + mw + 3) / 4) * 4;
        if (W < 4) W = 4;
        b->sd.read_w = W;
        b->sd.read_cw = cw;
        const int64_t need = (int64_t)W * (nseq > 0 ? nseq : 1);
        BWAMS_HIP(b->sd.d_packed.ensure((size_t)need * 4, (size_t)need * 4));
    }
    // per-lane scratch for the previous-interval lists: (longest read + 1) entries per lane
    const int cap = mx + 1;
    const int64_t threads = seed_max_threads(b->cu_count);
    if (cap > b->sd.prev_cap || threads > b->sd.prev_threads) {
        const size_t n = (size_t)cap * (size_t)threads;
        BWAMS_HIP(b->sd.d_prev.alloc(n * 16));
        b->sd.prev_cap = cap;
        b->sd.prev_threads = threads;
    }
    // backward phases with long interval lists (smem_bwd_wave_kernel): a slot per read and eight list entries per read cover
    // what uniform and repeat-rich genomes produce several times over; when they are full a pivot simply stays on its lane
    // (two item arrays of bi slots in one allocation: long lists, short lists; once a launch drains every backward phase leaves its
    // lane, about half a pivot per read in flight, profiles/r04_notes.md)
    const int64_t bi = std::max<int64_t>(nseq, 4096) * 2, be = std::max<int64_t>(nseq, 4096) * 24;
    if (bi > b->sd.bwd_items_cap) {
        b->sd.d_bwd_items.release(); b->sd.d_bwd_ent.release(); b->sd.bwd_items_cap = b->sd.bwd_ent_cap = 0;
        BWAMS_HIP(b->sd.d_bwd_items.alloc((size_t)bi * 2 * sizeof(BwdItem)));
        BWAMS_HIP(b->sd.d_bwd_ent.alloc((size_t)be * 16));
        b->sd.bwd_items_cap = bi;
        b->sd.bwd_ent_cap = be;
    }
    produced(b, Product::reads);
    return BWAMS_OK;
}

static int seed_run_once(bwams_batch_t *b, const bwams_seed_opt_t *opt, int with_sa) {
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    b->sd.with_sa = with_sa != 0;
    b->sd.n_smem = b->sd.n_sa = 0;

    // the search kernels' table, built once per index at its first FM-index seeding (ERT-only jobs never pay for it).  Batches of other
    // threads may seed the same index: it is published only after its build has finished, and nothing frees it before bwams_index_close.
    const uint4 *cp2 = nullptr;
    {
        bwams_index *ix = b->idx;
        std::lock_guard<std::mutex> lock(ix->cp2_mu);
        if (!ix->d_cp2.p) {
            DevBuf<> t;
            BWAMS_HIP(t.alloc(cp2_bytes(ix->n_blk)));
            launch_cp2_build(ix->fmi.cp, ix->n_blk, t.as<uint4>(), st);
            BWAMS_HIP(hipStreamSynchronize(st));
            ix->d_cp2 = std::move(t);
        }
        cp2 = ix->d_cp2.as<const uint4>();
    }
    // the lookup's dense table, the same way: once per index, at its first FM-index seeding that wants coordinates
    if (with_sa)
        if (int rc = sa_dense_ensure(b->idx, b->cu_count, st)) return rc;
    SeedLaunch a;
    a.fmi = b->idx->fmi;
    a.fmi.cp2 = cp2;
    a.enc = b->d_enc.p;
    a.cum = b->d_cum.p;
    a.skip = b->has_skip ? b->d_skip.p : nullptr;
    a.nseq = b->nseq;
    a.packed = b->sd.d_packed.p;
    a.read_w = b->sd.read_w;
    a.read_cw = b->sd.read_cw;
    a.reads_in_lds = b->sd.read_w <= 40;      // 40 words x 256 lanes x 4 B = 40 KB per workgroup
    a.debug = knobs().debug;
    a.min_seed_len = opt->min_seed_len;
    a.pool = b->sd.d_pool.p;
    a.pool_cap = b->pool_cap;
    a.ctr = b->d_ctr.p;
    a.prev = b->sd.d_prev.p;
    a.prev_cap = b->sd.prev_cap;
    a.prev_threads = b->sd.prev_threads;
    a.bwd_items = b->sd.d_bwd_items.p;
    a.bwd_items_s = b->sd.d_bwd_items.p + b->sd.bwd_items_cap;
    a.bwd_ent = b->sd.d_bwd_ent.p;
    a.bwd_items_cap = b->sd.bwd_items_cap;
    a.bwd_ent_cap = b->sd.bwd_ent_cap;
    {   // hand-over thresholds (fmi_seed.hip, bwd_hand_over; profiles/r03_notes.md 86): 40 entries at the forward end, or 8 still alive
        // after 24 columns; BWAMS_BWD_MIN_LIST=0: every backward phase stays on its lane
        const Knobs &kn = knobs();                           // the tests lower them so that toy genomes reach the kernels behind the search
        a.bwd_min_list = kn.bwd_min_list;
        a.bwd_cols = kn.bwd_cols;
        a.bwd_late_list = kn.bwd_late_list;
        // once the work queue has run dry: 24 entries at the forward end, or 12 alive after 8 columns (profiles/r03_notes.md 96)
        a.bwd_dry_min_list = kn.bwd_dry_min_list;
        a.bwd_dry_cols = kn.bwd_dry_cols;
        a.bwd_dry_late_list = kn.bwd_dry_late_list;
    }
    const int split_len = (int)(opt->min_seed_len * opt->split_factor + .499);

    BWAMS_HIP(hipMemsetAsync(b->d_ctr.p, 0, sizeof(DevCounters), st));
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvSeedStart], st));
    launch_pack_reads(b->d_enc.p, b->d_cum.p, b->nseq, b->sd.read_w, b->sd.read_cw, b->sd.d_packed.p, st);
    launch_mark(b->d_ctr.p, 0, st);
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvR1Start], st));
    if (b->nseq > 0) launch_smem_round1(a, b->cu_count, st);
#ifdef BWAMS_BWDDBG
    static hipEvent_t dbg_ev = nullptr;
    if (!dbg_ev) BWAMS_HIP(hipEventCreate(&dbg_ev));
    BWAMS_HIP(hipEventRecord(dbg_ev, st));
#endif
    if (b->nseq > 0) launch_smem_bwd_wave(a, b->cu_count, st);
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvR1End], st));
    launch_mark(b->d_ctr.p, 1, st);
    if (b->nseq > 0) launch_round2_work(a, b->sd.d_work2.p, b->pool_cap, split_len, opt->split_width, b->cu_count, st);
    // Round 3 reads nothing of rounds 1 and 2 (bwtSeedStrategyAllPosOneThread walks every read from position 0): it runs beside
    // round 2 on a stream of its own and fills the tail in which round 2's slowest reads keep few lanes busy.  Its extensions and
    // SMEMs are counted apart (n_ext3 / n_blk3 / n_smem3), so that the per-round figures stay exact.
    SeedLaunch a3 = a;
    a3.min_seed_len = opt->min_seed_len + 1;
    const bool r3 = b->nseq > 0 && opt->max_mem_intv > 0;
    const bool r3_beside = r3 && knobs().r3_beside != 0;
    if (r3_beside) {
        BWAMS_HIP(hipEventRecord(b->sd.seed_fork, st));
        BWAMS_HIP(hipStreamWaitEvent(b->sd.seed_aux, b->sd.seed_fork, 0));
        BWAMS_HIP(hipEventRecord(b->ev[b->kEvR3Start], b->sd.seed_aux));
        launch_smem_round3(a3, opt->max_mem_intv, b->cu_count, b->sd.seed_aux);
        BWAMS_HIP(hipEventRecord(b->ev[b->kEvR3End], b->sd.seed_aux));
        BWAMS_HIP(hipEventRecord(b->sd.seed_join, b->sd.seed_aux));
    }
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvR2Start], st));
    if (b->nseq > 0) launch_smem_round2(a, b->sd.d_work2.p, b->cu_count, st);
    if (b->nseq > 0) launch_smem_bwd_wave(a, b->cu_count, st);
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvR2End], st));
    if (r3_beside) BWAMS_HIP(hipStreamWaitEvent(st, b->sd.seed_join, 0));
    launch_mark(b->d_ctr.p, 2, st);
    if (!r3_beside) {
        BWAMS_HIP(hipEventRecord(b->ev[b->kEvR3Start], st));
        if (r3) launch_smem_round3(a3, opt->max_mem_intv, b->cu_count, st);
        BWAMS_HIP(hipEventRecord(b->ev[b->kEvR3End], st));
    }
    launch_mark(b->d_ctr.p, 3, st);
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvRoundsDone], st));
    BWAMS_HIP(hipGetLastError());
    // the SMEM count sizes the sort: one small read-back
    BWAMS_HIP(hipMemcpyAsync(b->h_ctr.p, b->d_ctr.p, sizeof(DevCounters), hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
#ifdef BWAMS_BWDDBG
    if (knobs().verbose) {
        const unsigned long long *d = b->h_ctr.p->dbg;
        { float m1 = 0, m2 = 0; (void)hipEventElapsedTime(&m1, b->ev[b->kEvR1Start], dbg_ev); (void)hipEventElapsedTime(&m2, dbg_ev, b->ev[b->kEvR1End]);
          fprintf(stderr, "[smem_r1] search kernel %.3f ms, the two backward kernels behind it %.3f ms\n", m1, m2); }
        fprintf(stderr, "[bwd_wave] rounds 1+2: items %llu, column batches %llu (%.1f per item), waves with work %llu: busy mean %.3f ms max %.3f ms, "
                "of it between items (ticket, item, list, read) %.1f %%, per column batch %.2f us\n", d[0], d[1], d[0] ? (double)d[1] / d[0] : 0.0, d[5],
                d[5] ? d[2] / (double)d[5] * 1e-5 : 0.0, d[4] * 1e-5, d[2] ? 100.0 * d[3] / d[2] : 0.0, d[1] ? (d[2] - d[3]) * 1e-2 / d[1] : 0.0);
        fprintf(stderr, "[bwd_group] rounds 1+2: items %llu, wave-iterations %llu (groups live per iteration %.2f), waves with work %llu: busy mean %.3f ms max %.3f ms; "
                "first in %.3f last out %.3f ms after round 1's start; [bwd_wave] first in %.3f last out %.3f\n", d[68], d[69], d[69] ? (double)d[70] / d[69] : 0.0, d[72],
                d[72] ? d[71] * 1e-5 / d[72] : 0.0, d[73] * 1e-5, (~d[75] - ~d[8]) * 1e-5, (d[74] - ~d[8]) * 1e-5, (~d[7] - ~d[8]) * 1e-5, (d[6] - ~d[8]) * 1e-5);
        fprintf(stderr, "[bwd_group] extensions %llu of %llu (rounds 1+2)\n", d[76], (unsigned long long)b->h_ctr.p->ext_after[1]);
        const unsigned long long t0 = ~d[8], tdry = ~d[9];
        fprintf(stderr, "[smem_r1] waves %llu: read queue dry at %.3f ms, last wave out at %.3f ms, mean wave life %.3f ms (%.3f ms of it after the queue ran dry); "
                "iterations %llu, lanes extending per iteration %.1f\n", d[12], (tdry - t0) * 1e-5, (d[10] - t0) * 1e-5, d[12] ? d[11] * 1e-5 / d[12] : 0.0,
                d[12] ? d[15] * 1e-5 / d[12] : 0.0, d[13], d[13] ? (double)d[14] / d[13] : 0.0);
        fprintf(stderr, "[smem_r1] waves leaving per 0.4 ms:");
        for (int i = 0; i < 48; ++i) if (d[16 + i]) fprintf(stderr, " %.1f:%llu", i * 0.4, d[16 + i]);
        fprintf(stderr, "\n[smem_r1] wave-iterations after the wave first saw the queue dry: %llu, with one lane extending %llu (max per wave %llu), with 2-4 lanes %llu\n", d[64], d[65], d[67], d[66]);
    }
#endif
    const int64_t n_slots = (int64_t)b->h_ctr.p->n_smem_total;      // pool slots handed out (holes included)
    const int64_t n = (int64_t)b->h_ctr.p->n_smem_valid;           // real SMEMs
    b->sd.n_smem = n;
    b->sd.n_pool_slots = n_slots;
    if (n > b->max_smem || n_slots > b->pool_cap) {
        set_last_error("SMEM pool overflow: need " + std::to_string(n) + " slots");
        produced(b, Product::seeds);                           // the counts of an overflowing pass are there to read (bwams_seed_counts)
        return BWAMS_ERR_CAPACITY;
    }
    if (n_slots > 0)
        if (int rc = sort_pool(b, "bwams_seed_run: radix_sort_pairs", n_slots, n, with_sa ? b->sd.d_sa_cnt.p : nullptr, opt->max_occ)) return rc;
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvSorted], st));
    if (with_sa && n > 0) {
        BWAMS_HIP(hipMemsetAsync(b->sd.d_sa_cnt.p + n, 0, 8, st));
        if (int rc = scan_rows(b, b->sd.d_sa_cnt.p, b->sd.d_sa_off.p, 1, n + 1)) return rc;
        fm_lookup(b, n);
    }
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvSeedEnd], st));
    BWAMS_HIP(hipGetLastError());
    produced(b, Product::seeds);
    return BWAMS_OK;
}

int bwams_seed_run(bwams_batch_t *b, const bwams_seed_opt_t *opt, int with_sa) {
    if (!b || !opt) return BWAMS_ERR_ARG;
    if (!has(b, Product::reads)) {
        set_last_error("bwams_seed_run: upload the reads first (bwams_seed_upload)");
        return BWAMS_ERR_ARG;
    }
    outdated(b, Product::seeds);
    b->sd.last_opt = *opt;
    b->sd.ert = nullptr;
    return run_growing(b, [&] { return seed_run_once(b, opt, with_sa); });
}

int bwams_seed_counts(bwams_batch_t *b, int64_t *n_smem, int64_t *n_sa) {
    if (!has(b, Product::seeds)) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    BWAMS_HIP(hipMemcpyAsync(b->h_ctr.p, b->d_ctr.p, sizeof(DevCounters), hipMemcpyDeviceToHost, b->stream));
    BWAMS_HIP(hipStreamSynchronize(b->stream));
    b->sd.n_sa = b->sd.with_sa ? (int64_t)b->h_ctr.p->n_sa_lookups : 0;
    if (n_smem) *n_smem = b->sd.n_smem;
    if (n_sa) *n_sa = b->sd.n_sa;
    if (b->sd.n_smem > b->max_smem) return BWAMS_ERR_CAPACITY;
    if (b->sd.n_sa > b->max_sa) {
        // the lookup kernel counted every coordinate but stored only max_sa of them: grow and run it again
        b->max_sa = b->sd.n_sa + b->sd.n_sa / 8 + 1024;
        BWAMS_HIP(b->sd.d_sa_coord.alloc((size_t)b->max_sa * 8));
        BWAMS_HIP(hipMemsetAsync(&b->d_ctr.p->n_sa_lookups, 0, 2 * sizeof(unsigned long long), b->stream));   // + n_lf_steps
        if (b->sd.ert) {
            ert_locate(b, b->sd.n_smem);
            if (int rrc = ert_gather(b, b->sd.n_smem)) return rrc;
            launch_ert_clear(b->sd.d_sorted.p, b->sd.n_smem, b->stream);
        } else
            fm_lookup(b, b->sd.n_smem);
        BWAMS_HIP(hipEventRecord(b->ev[b->kEvSeedEnd], b->stream));
        BWAMS_HIP(hipMemcpyAsync(b->h_ctr.p, b->d_ctr.p, sizeof(DevCounters), hipMemcpyDeviceToHost, b->stream));
        BWAMS_HIP(hipStreamSynchronize(b->stream));
        b->sd.n_sa = (int64_t)b->h_ctr.p->n_sa_lookups;
        if (n_sa) *n_sa = b->sd.n_sa;
        if (b->sd.n_sa > b->max_sa) {
            set_last_error("SA coordinate buffer overflow: need " + std::to_string(b->sd.n_sa));
            return BWAMS_ERR_CAPACITY;
        }
    }
    return BWAMS_OK;
}

int bwams_seed_fetch(bwams_batch_t *b, bwams_smem_t *smem_out, int64_t smem_cap, int64_t *sa_coord,
                     int64_t sa_cap, int64_t *sa_off) {
    if (!has(b, Product::seeds)) return BWAMS_ERR_ARG;
    int64_t ns = 0, na = 0;
    int rc = bwams_seed_counts(b, &ns, &na);
    if (rc) return rc;
    if (ns > smem_cap || (sa_coord && na > sa_cap)) {
        set_last_error("bwams_seed_fetch: caller buffers too small");
        return BWAMS_ERR_CAPACITY;
    }
    if (smem_out && ns)
        BWAMS_HIP(hipMemcpyAsync(smem_out, b->sd.d_sorted.p, (size_t)ns * sizeof(bwams_smem_t), hipMemcpyDeviceToHost,
                                 b->stream));
    if (sa_coord && sa_off && b->sd.with_sa) {
        if (ns) {
            BWAMS_HIP(hipMemcpyAsync(sa_off, b->sd.d_sa_off.p, (size_t)(ns + 1) * 8, hipMemcpyDeviceToHost, b->stream));
            if (na)
                BWAMS_HIP(hipMemcpyAsync(sa_coord, b->sd.d_sa_coord.p, (size_t)na * 8, hipMemcpyDeviceToHost, b->stream));
        } else {
            sa_off[0] = 0;
        }
    }
    BWAMS_HIP(hipStreamSynchronize(b->stream));
    return BWAMS_OK;
}

int bwams_seed_fmi(bwams_batch_t *b, const uint8_t *enc, const int64_t *cum, const uint8_t *skip, int64_t nseq,
                   const bwams_seed_opt_t *opt, bwams_smem_t *smem_out, int64_t smem_cap, int64_t *n_smem,
                   int64_t *sa_coord, int64_t sa_cap, int64_t *sa_off, int64_t *n_sa) {
    int rc = bwams_seed_upload(b, enc, cum, skip, nseq);
    if (rc) return rc;
    const int with_sa = sa_coord && sa_off;
    rc = bwams_seed_run(b, opt, with_sa);
    if (rc) {
        if (n_smem) *n_smem = b->sd.n_smem;
        return rc;
    }
    rc = bwams_seed_counts(b, n_smem, n_sa);
    if (rc) return rc;
    return bwams_seed_fetch(b, smem_out, smem_cap, sa_coord, sa_cap, sa_off);
}

static int ert_run_once(bwams_batch_t *b, bwams_ert_t *e, const bwams_seed_opt_t *opt, int with_sa, int M) {
    BWAMS_HIP(hipSetDevice(b->idx->device));
    hipStream_t st = b->stream;
    b->sd.with_sa = with_sa != 0;
    b->sd.n_smem = b->sd.n_sa = 0;
    const size_t need = ert_prof_bytes(b->nbases);
    BWAMS_HIP(b->sd.d_ert_prof.ensure(need, need + need / 8));
    const int frames = 2 * (e->t.read_len + 2);      // the counting walk keeps two words per level
    const size_t part_bytes = ert_count_bytes();      // partial counters sit behind the stacks
    if (frames > b->sd.ert_stk_frames) {
        BWAMS_HIP(b->sd.d_ert_stk.alloc((size_t)ert_walk_threads(b->cu_count) * (size_t)frames * 8 + part_bytes));
        b->sd.ert_stk_frames = frames;
        BWAMS_HIP(hipMemsetAsync(b->sd.d_ert_stk.p + (size_t)ert_walk_threads(b->cu_count) * (size_t)frames, 0, part_bytes, b->stream));
    }
    const uint8_t *skip = b->has_skip ? b->d_skip.p : nullptr;
    BWAMS_HIP(hipMemsetAsync(b->d_ctr.p, 0, sizeof(DevCounters), st));
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvSeedStart], st));
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvR1Start], st));
    launch_ert_profile(e->t, b->d_enc.p, b->d_cum.p, skip, b->nseq, b->nbases, M, b->sd.d_ert_prof.p, b->d_ctr.p,
                       (unsigned long long *)(b->sd.d_ert_stk.p + (size_t)ert_walk_threads(b->cu_count) * (size_t)b->sd.ert_stk_frames), b->cu_count, st);
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvR1End], st));
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvR2Start], st));
    launch_ert_select(b->sd.d_ert_prof.p, b->d_cum.p, skip, b->nseq, b->nbases, M, *opt, b->sd.d_pool.p, b->pool_cap, b->d_ctr.p, b->cu_count, st);
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvR2End], st));
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvRoundsDone], st));
    BWAMS_HIP(hipGetLastError());
    BWAMS_HIP(hipMemcpyAsync(&b->d_ctr.p->n_smem_valid, &b->d_ctr.p->n_smem_total, 8, hipMemcpyDeviceToDevice, st));
    for (int k = 0; k < 3; ++k)      // the rounds are not separate launches here: all seeds are reported under round 1
        BWAMS_HIP(hipMemcpyAsync(&b->d_ctr.p->valid_after[k], &b->d_ctr.p->n_smem_total, 8, hipMemcpyDeviceToDevice, st));
    BWAMS_HIP(hipMemcpyAsync(b->h_ctr.p, b->d_ctr.p, sizeof(DevCounters), hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    const int64_t n = (int64_t)b->h_ctr.p->n_smem_total;
    b->sd.n_smem = n;
    if (n > b->max_smem || n > b->pool_cap) {
        set_last_error("SMEM pool overflow: need " + std::to_string(n) + " slots");
        produced(b, Product::seeds);                           // as in seed_run_once
        return BWAMS_ERR_CAPACITY;
    }
    if (n > 0)
        if (int rc = sort_pool(b, "bwams_seed_run_ert: radix_sort_pairs", n, n, nullptr, opt->max_occ)) return rc;
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvSorted], st));
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvR3Start], st));
    ert_locate(b, n);
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvR3End], st));
    if (with_sa && n > 0) {
        BWAMS_HIP(hipMemsetAsync(b->sd.d_sa_cnt.p + n, 0, 8, st));
        if (int rc = scan_rows(b, b->sd.d_sa_cnt.p, b->sd.d_sa_off.p, 1, n + 1)) return rc;
        if (int rrc = ert_gather(b, n)) return rrc;
    }
    launch_ert_clear(b->sd.d_sorted.p, n, st);
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvSeedEnd], st));
    BWAMS_HIP(hipGetLastError());
    produced(b, Product::seeds);
    return BWAMS_OK;
}

int bwams_seed_run_ert(bwams_batch_t *b, bwams_ert_t *e, const bwams_seed_opt_t *opt, int with_sa) {
    if (!b || !e || !opt) return BWAMS_ERR_ARG;
    if (!has(b, Product::reads)) {
        set_last_error("bwams_seed_run_ert: upload the reads first (bwams_seed_upload)");
        return BWAMS_ERR_ARG;
    }
    if (e->idx != b->idx) {
        set_last_error("bwams_seed_run_ert: table and batch belong to different indexes");
        return BWAMS_ERR_ARG;
    }
    const int M = opt->split_width + 1 > opt->max_mem_intv ? opt->split_width + 1 : opt->max_mem_intv;
    if (opt->min_seed_len < e->t.K + e->t.X || M > 20 || M < 1) {
        set_last_error("bwams_seed_run_ert: needs min_seed_len >= kmer + xmer size, split_width < 20 and max_mem_intv <= 20 "
                       "(the trees store hit counts below 20 only)");
        return BWAMS_ERR_UNSUPPORTED;
    }
    if (b->max_read_len > 255 || b->max_read_len > e->t.read_len) {
        set_last_error("bwams_seed_run_ert: a read is longer than the read length the ERT was built for");
        return BWAMS_ERR_UNSUPPORTED;
    }
    outdated(b, Product::seeds);
    b->sd.last_opt = *opt;
    b->sd.ert = e;
    return run_growing(b, [&] { return ert_run_once(b, e, opt, with_sa, M); });
}

}  // extern "C"
