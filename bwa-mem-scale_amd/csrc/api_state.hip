// api_state.hip — the stage state of a batch (stage_state.h) and what the entry-point files share: the per-device auxiliary
// stream set, state creation (get_state) and release (stage_state_free), check_opt, dev_bns,
// sw_params, scan_rows with the widen kernels behind launch_widen1 / launch_widen2, and stage_state_stats for bwams_batch_stats.
#include <cstring>
#include <map>

#include <rocprim/rocprim.hpp>

#include "stage_state.h"

namespace bwams {

// The auxiliary streams are ONE set per device, shared by its batches (reference-counted).  A process gets four hardware queues
// from the runtime (the library sets nothing); the runtime puts every new stream on the least used of them, and a queue completes
// its packets in order.  A batch with a set of its own made nine streams per batch, and with three batches on a device (two chunks
// in flight + the caller's) a slot's copies landed behind another slot's kernels or not, depending on the order in which the
// process had created its streams (4.5 .. 5.6 Mreads/s streaming in a process that had created other batches before, 7.3 .. 7.6
// in a fresh one).  The set holds what the widest stage forks onto (kAuxStreams: banded SW's four); a stage that wants an order
// between two launches puts them on one stream and does not count on two streams sharing a queue.  Sharing is safe: every use is
// fork event -> launches -> join event, and a stream is a total order.
struct AuxSet { hipStream_t q[kAuxStreams] = {}; int refs = 0; };
static std::mutex g_aux_mu;
static std::map<int, AuxSet> g_aux;
static int aux_acquire(int device, hipStream_t *out) {
    std::lock_guard<std::mutex> g(g_aux_mu);
    AuxSet &a = g_aux[device];
    if (a.refs == 0)
        for (auto &q : a.q) BWAMS_HIP(hipStreamCreateWithFlags(&q, hipStreamNonBlocking));
    ++a.refs;
    for (int i = 0; i < kAuxStreams; ++i) out[i] = a.q[i];
    return BWAMS_OK;
}
static void aux_release(int device) {
    std::lock_guard<std::mutex> g(g_aux_mu);
    auto it = g_aux.find(device);
    if (it == g_aux.end()) return;
    if (--it->second.refs == 0) {
        for (auto &q : it->second.q) if (q) (void)hipStreamDestroy(q);
        g_aux.erase(it);
    }
}

void stage_state_free(StageState *s) {
    if (!s) return;
    if (s->ev_ok) {
        for (auto &e : s->ev) (void)hipEventDestroy(e);
        for (auto &e : s->join) (void)hipEventDestroy(e);
        (void)hipEventDestroy(s->fork);
        if (s->aux_device >= 0) aux_release(s->aux_device);
    }
    delete s;
}

namespace {

__global__ void widen1_kernel(const int32_t *a, int64_t n, int64_t *wide) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g > n) return;
    wide[g] = g < n ? (int64_t)a[g] : 0;
}
__global__ void widen2_kernel(const int32_t *a, const int32_t *b, int64_t n, int64_t *wide) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= 2 * (n + 1)) return;
    const int64_t row = g / (n + 1), i = g - row * (n + 1);
    wide[g] = i < n ? (int64_t)(row ? b[i] : a[i]) : 0;
}

}  // namespace

void launch_widen1(const int32_t *a, int64_t n, int64_t *wide, hipStream_t st) {
    widen1_kernel<<<(unsigned)((n + 256) / 256), 256, 0, st>>>(a, n, wide);
}
void launch_widen2(const int32_t *a, const int32_t *b, int64_t n, int64_t *wide, hipStream_t st) {
    widen2_kernel<<<(unsigned)((2 * (n + 1) + 255) / 256), 256, 0, st>>>(a, b, n, wide);
}

int scan_rows(bwams_batch *b, const int64_t *in, int64_t *out, int rows, int64_t n1) {
    for (int r = 0; r < rows; ++r)
        if (int rc = with_tmp(b, "scan_rows: exclusive_scan", [&](void *tmp, size_t &tb) {
                return rocprim::exclusive_scan(tmp, tb, in + r * n1, out + r * n1, (int64_t)0, (size_t)n1, rocprim::plus<int64_t>(), b->stream);
            })) return rc;
    return BWAMS_OK;
}

int get_state(bwams_batch *b, StageState **out) {
    if (!b->stages) {
        b->stages = new StageState();
        for (auto &e : b->stages->ev) BWAMS_HIP(hipEventCreate(&e));
        for (auto &e : b->stages->join) BWAMS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        BWAMS_HIP(hipEventCreateWithFlags(&b->stages->fork, hipEventDisableTiming));
        b->stages->ev_ok = true;
        if (int rc = aux_acquire(b->idx->device, b->stages->aux)) return rc;
        b->stages->aux_device = b->idx->device;
    }
    *out = b->stages;
    return BWAMS_OK;
}

int check_opt(const bwams_mem_opt_t *o, const char *who) {
    if (!o || o->e_del <= 0 || o->e_ins <= 0 || o->max_occ <= 0 || o->w < 0) {
        set_last_error(std::string(who) + ": null options, non-positive gap extension penalty or max_occ");
        return BWAMS_ERR_ARG;
    }
    return BWAMS_OK;
}

int dev_bns(bwams_index *ix, DevBns *out) {
    const int64_t l_pac = (ix->fmi.ref_seq_len - 1) / 2;
    if (!ix->d_contigs.p) {                     // default: one sequence spanning the whole text
        bwams_contig_t c;
        c.offset = 0; c.len = (int32_t)l_pac; c.is_alt = 0;
        if (l_pac > 0x7fffffffLL) {
            set_last_error("the index holds more than 2^31 bases: call bwams_index_set_contigs with the real sequences");
            return BWAMS_ERR_ARG;
        }
        BWAMS_HIP(ix->d_contigs.alloc(sizeof c));
        BWAMS_HIP(hipMemcpy(ix->d_contigs.p, &c, sizeof c, hipMemcpyHostToDevice));
        ix->n_seqs = 1;
    }
    out->contigs = ix->d_contigs.as<const bwams_contig_t>();
    out->n_seqs = ix->n_seqs;
    out->l_pac = l_pac;
    return BWAMS_OK;
}

template <class Opt> static void sw_fill(const Opt &o, int end_bonus, SwParams *prm) {
    prm->o_del = o.o_del; prm->e_del = o.e_del; prm->o_ins = o.o_ins; prm->e_ins = o.e_ins;
    prm->zdrop = o.zdrop; prm->end_bonus = end_bonus;
    int mx = 0;
    for (int i = 0; i < 25; ++i) {
        prm->mat[i] = o.mat[i];
        mx = mx > o.mat[i] ? mx : o.mat[i];
    }
    prm->max_sc = mx;
}
void sw_params(const bwams_mem_opt_t &o, int end_bonus, SwParams *prm) { sw_fill(o, end_bonus, prm); }
void sw_params(const bwams_sw_opt_t &o, SwParams *prm) { sw_fill(o, o.end_bonus, prm); }

void stage_state_stats(const bwams_batch *b, bwams_stats_t *out) {
    const StageState *s = b->stages;
    if (!s) return;
    out->n_chains = s->ch.n_chains; out->n_chain_seeds = s->ch.n_seeds; out->n_chain_redo = s->ch.n_redo;
    out->n_left = s->ext.n_left; out->n_right = s->ext.n_right;
    out->n_retry_left = s->ext.n_retry_left; out->n_retry_right = s->ext.n_retry_right;
    auto el = [&](int a, int b, float *dst) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, s->ev[a], s->ev[b]) == hipSuccess) *dst = ms;
    };
    el(0, 1, &out->ms_chain);
    el(2, 3, &out->ms_ext_plan);
    if (has(b, Product::ext)) {
        el(4, 5, &out->ms_ext_left);
        el(6, 7, &out->ms_ext_right);
        el(8, 9, &out->ms_ext_purge);
        el(10, 11, &out->ms_ext_total);
        out->n_ext_rounds = s->ext.n_rounds;
    }
    if (has(b, Product::dedup)) { el(12, 13, &out->ms_dedup); out->n_final_regs = s->dd.n_final; }
    if (has(b, Product::pair)) {
        el(14, 15, &out->ms_pair);
        out->n_pair_tasks = s->pr.tasks; out->n_pair_redone = s->pr.redone; out->n_pair_regs = s->pr.total;
    }
    (void)hipGetLastError();
}
}  // namespace bwams
