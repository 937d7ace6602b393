// api_sw.hip — C-ABI entry points of the two Smith-Waterman kernels on pairs the caller uploads (include/bwams.h): banded
// extension (bwams_bsw_upload, _run, _fetch; bwams_bsw_extend = the three) and mate rescue's local alignment (bwams_ksw_align).
#include "stage_state.h"

using namespace bwams;

extern "C" {

int bwams_bsw_upload(bwams_batch_t *b, const bwams_seqpair_t *pairs, int64_t n, const uint8_t *ref,
                     int64_t ref_bytes, const uint8_t *qer, int64_t qer_bytes) {
    if (!b || n < 0 || (n && (!pairs || !ref || !qer))) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    int qmax = 1, tmax = 1;
    for (int64_t i = 0; i < n; ++i) {
        const bwams_seqpair_t &p = pairs[i];
        if (p.len1 < 0 || p.len2 < 0 || p.idr < 0 || p.idq < 0 || (int64_t)p.idr + p.len1 > ref_bytes ||
            (int64_t)p.idq + p.len2 > qer_bytes) {
            set_last_error("bwams_bsw_upload: pair " + std::to_string(i) + " points outside the sequence buffers");
            return BWAMS_ERR_ARG;
        }
        if (p.len2 > qmax) qmax = p.len2;
        if (p.len1 > tmax) tmax = p.len1;
    }
    if (bsw_lds_waves(qmax) < 1) {                    // the limit launch_bsw has: one wave's row within a CU's LDS
        set_last_error("bwams_bsw_upload: query of " + std::to_string(qmax) + " bases, longer than the LDS-resident kernel supports (18196)");
        return BWAMS_ERR_UNSUPPORTED;
    }
    auto grow = [](auto &buf, int64_t need, size_t elem) { return buf.ensure((size_t)need * elem, (size_t)(need + need / 4 + 1024) * elem); };
    BWAMS_HIP(grow(b->sw.d_pairs, n, sizeof(bwams_seqpair_t)));
    BWAMS_HIP(grow(b->sw.d_ref, ref_bytes + 64, 1));
    BWAMS_HIP(grow(b->sw.d_qer, qer_bytes + 64, 1));
    if (n) {
        BWAMS_HIP(hipMemcpyAsync(b->sw.d_pairs.p, pairs, (size_t)n * sizeof(bwams_seqpair_t), hipMemcpyHostToDevice, b->stream));
        BWAMS_HIP(hipMemcpyAsync(b->sw.d_ref.p, ref, (size_t)ref_bytes, hipMemcpyHostToDevice, b->stream));
        BWAMS_HIP(hipMemcpyAsync(b->sw.d_qer.p, qer, (size_t)qer_bytes, hipMemcpyHostToDevice, b->stream));
        BWAMS_HIP(hipStreamSynchronize(b->stream));
    }
    b->sw.n_pairs = n;
    b->sw.max_qlen = qmax;
    b->sw.max_tlen = tmax;
    return BWAMS_OK;
}

int bwams_bsw_run(bwams_batch_t *b, int32_t w, const bwams_sw_opt_t *o) {
    if (!b || !o) return BWAMS_ERR_ARG;
    if (o->e_ins <= 0 || o->e_del <= 0) {
        set_last_error("bwams_bsw_run: gap extension penalties must be positive");
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(b->idx->device));
    SwParams prm;
    sw_params(*o, &prm);
    BWAMS_HIP(hipMemsetAsync(&b->d_ctr.p->bsw_cells, 0, sizeof(unsigned long long), b->stream));
    const size_t list_bytes = b->sw.n_pairs > 0 ? bsw_list_bytes(b->sw.n_pairs) : 0;
    if (list_bytes > b->sw.d_bsw_list.cap) BWAMS_HIP(hipStreamSynchronize(b->stream));     // the last launch may still read the lists
    BWAMS_HIP(b->sw.d_bsw_list.ensure(list_bytes, bsw_list_bytes(b->sw.n_pairs + b->sw.n_pairs / 4 + 1024)));
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvBswStart], b->stream));
    if (launch_bsw(b->sw.d_pairs.p, b->sw.n_pairs, b->sw.d_ref.p, b->sw.d_qer.p, w, prm, b->sw.max_qlen, b->d_ctr.p, b->cu_count, b->stream, b->sw.d_bsw_list.p,
                   nullptr, nullptr, nullptr, nullptr, 1, knobs().bsw_early == 1)) {     // the early exit only on request: bsw_cells is the full walk's otherwise
        set_last_error("bwams_bsw_run: a query longer than ~18000 bases does not fit the LDS kernel");
        return BWAMS_ERR_UNSUPPORTED;
    }
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvBswEnd], b->stream));
    BWAMS_HIP(hipGetLastError());
    return BWAMS_OK;
}

int bwams_bsw_fetch(bwams_batch_t *b, bwams_seqpair_t *pairs, int64_t n) {
    if (!b || n != b->sw.n_pairs) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    if (n) BWAMS_HIP(hipMemcpyAsync(pairs, b->sw.d_pairs.p, (size_t)n * sizeof(bwams_seqpair_t), hipMemcpyDeviceToHost, b->stream));
    BWAMS_HIP(hipStreamSynchronize(b->stream));
    return BWAMS_OK;
}

int bwams_bsw_extend(bwams_batch_t *b, bwams_seqpair_t *pairs, int64_t n, const uint8_t *ref, int64_t ref_bytes,
                     const uint8_t *qer, int64_t qer_bytes, int32_t w, const bwams_sw_opt_t *opt) {
    int rc = bwams_bsw_upload(b, pairs, n, ref, ref_bytes, qer, qer_bytes);
    if (rc) return rc;
    rc = bwams_bsw_run(b, w, opt);
    if (rc) return rc;
    return bwams_bsw_fetch(b, pairs, n);
}

int bwams_ksw_align(bwams_batch_t *b, const bwams_seqpair_t *pairs, int64_t n, const uint8_t *ref, int64_t ref_bytes,
                    const uint8_t *qer, int64_t qer_bytes, const bwams_sw_opt_t *o, bwams_kswr_t *out) {
    if (!b || !o || (n && !out)) return BWAMS_ERR_ARG;
    int mx = -128, mn = 127;
    for (int i = 0; i < 25; ++i) {
        mx = mx > o->mat[i] ? mx : o->mat[i];
        mn = mn < o->mat[i] ? mn : o->mat[i];
    }
    if (mx <= 0 || o->e_ins <= 0 || o->e_del <= 0 ||
        (o->o_ins + o->e_ins) + (o->o_del + o->e_del) <= mx - mn) {
        set_last_error("bwams_ksw_align: needs max(mat) > 0 and oe_ins + oe_del > max(mat) - min(mat) "
                       "(an insertion directly followed by a deletion must not beat a mismatch)");
        return BWAMS_ERR_UNSUPPORTED;
    }
    int rc = bwams_bsw_upload(b, pairs, n, ref, ref_bytes, qer, qer_bytes);
    if (rc) return rc;
    if (b->sw.max_qlen > 512 || b->sw.max_tlen > kKswMaxTarget) {
        set_last_error("bwams_ksw_align: query longer than 512 or target longer than 20000 "
                       "(the reference's kswv bounds are 512 / 2048, src/kswv.h:54-55)");
        return BWAMS_ERR_UNSUPPORTED;
    }
    BWAMS_HIP(hipSetDevice(b->idx->device));
    BWAMS_HIP(b->sw.d_ksw_out.ensure((size_t)n * sizeof(bwams_kswr_t), (size_t)(n + n / 4 + 256) * sizeof(bwams_kswr_t)));
    SwParams prm;
    sw_params(*o, &prm);                              // max_sc = mx: the check above has mx > 0
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvKswStart], b->stream));
    if (launch_ksw(b->sw.d_pairs.p, n, b->sw.d_ref.p, b->sw.d_qer.p, prm, ((b->sw.max_qlen + 15) / 16) * 16, b->sw.max_tlen, b->sw.d_ksw_out.p,
                   b->d_ctr.p, b->cu_count, b->stream)) {
        set_last_error("bwams_ksw_align: target too long for the LDS of one block");
        return BWAMS_ERR_UNSUPPORTED;
    }
    BWAMS_HIP(hipEventRecord(b->ev[b->kEvKswEnd], b->stream));
    BWAMS_HIP(hipGetLastError());
    if (n) BWAMS_HIP(hipMemcpyAsync(out, b->sw.d_ksw_out.p, (size_t)n * sizeof(bwams_kswr_t), hipMemcpyDeviceToHost, b->stream));
    BWAMS_HIP(hipStreamSynchronize(b->stream));
    return BWAMS_OK;
}

}  // extern "C"
