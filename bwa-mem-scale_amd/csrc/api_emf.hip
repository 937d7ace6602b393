// api_emf.hip — C-ABI entry points of the exact-match filter (include/bwams.h): the EMF table handle (from host or device
// arrays, from a `.perfect.<L>` file, built on the GPU; info, fetch, save, close) and its probe of a batch's reads
// (bwams_emf_run on the resident reads, bwams_emf_probe on uploaded ones, bwams_emf_fetch).
#include <cstring>

#include "common.h"

using namespace bwams;

extern "C" {

int bwams_emf_from_host(bwams_index_t *ix, int32_t seed_len, uint32_t seq_len, const uint32_t *loc_table,
                        uint32_t num_loc_entry, const bwams_seed_entry_t *seed_table, uint32_t num_seed_entry,
                        bwams_emf_t **out) {
    if (!ix || !out || !seed_table || !num_seed_entry || seed_len <= 0 || (num_loc_entry && !loc_table)) return BWAMS_ERR_ARG;
    if (!ix->fmi.ref) {
        set_last_error("bwams_emf_from_host: the index was opened without its .0123 reference");
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(ix->device));
    bwams_emf *e = new bwams_emf();
    e->idx = ix;
    const size_t bs = (size_t)num_seed_entry * 16, bl = (size_t)(num_loc_entry ? num_loc_entry : 1) * 4;
    hipError_t he = e->d_seeds.alloc(bs);
    if (he == hipSuccess) he = e->d_loc.alloc(bl);
    if (he == hipSuccess) he = hipMemcpy(e->d_seeds.p, seed_table, bs, hipMemcpyHostToDevice);
    if (he == hipSuccess && num_loc_entry) he = hipMemcpy(e->d_loc.p, loc_table, (size_t)num_loc_entry * 4, hipMemcpyHostToDevice);
    if (he != hipSuccess) {                     // a table is tens of GiB: do not strand the half that was made
        set_last_error(std::string("bwams_emf_from_host: ") + hipGetErrorString(he));
        bwams_emf_close(e);
        return he == hipErrorOutOfMemory ? BWAMS_ERR_NOMEM : BWAMS_ERR_DEVICE;
    }
    e->t.seed_table = e->d_seeds.as<const uint4>();
    e->t.loc_table = e->d_loc.as<const uint32_t>();
    e->t.ref = ix->fmi.ref;
    e->t.num_seed_entry = num_seed_entry;
    e->t.num_loc_entry = num_loc_entry;
    e->t.seq_len = seq_len;
    e->t.seed_len = seed_len;
    e->bytes = (int64_t)(bs + bl);
    *out = e;
    return BWAMS_OK;
}

int bwams_emf_open(bwams_index_t *ix, const char *path, bwams_emf_t **out) {
    if (!ix || !path || !out) return BWAMS_ERR_ARG;
    MappedFile mf(path, 64);
    if (!mf.opened) { set_last_error(std::string("cannot open ") + path); return BWAMS_ERR_IO; }
    if (!mf.p) { set_last_error(std::string(path) + ": cannot map"); return BWAMS_ERR_IO; }
    const uint8_t *m = mf.p;
    // perfect_table_t header (src/perfect.h:188-213)
    int32_t seed_len; uint32_t n_loc, n_seed, seq_len;
    memcpy(&seed_len, m, 4); memcpy(&n_loc, m + 4, 4); memcpy(&n_seed, m + 8, 4); memcpy(&seq_len, m + 40, 4);
    if (mf.size != 64 + (size_t)n_loc * 4 + (size_t)n_seed * 16) {
        set_last_error(std::string(path) + ": size does not match its header");
        return BWAMS_ERR_IO;
    }
    return bwams_emf_from_host(ix, seed_len, seq_len, reinterpret_cast<const uint32_t *>(m + 64), n_loc,
                               reinterpret_cast<const bwams_seed_entry_t *>(m + 64 + (size_t)n_loc * 4), n_seed, out);
}

int bwams_emf_from_device(bwams_index_t *ix, int32_t seed_len, uint32_t seq_len, const uint32_t *loc_table_dev,
                          uint32_t num_loc_entry, const bwams_seed_entry_t *seed_table_dev, uint32_t num_seed_entry,
                          bwams_emf_t **out) {
    if (!ix || !out || !seed_table_dev || !num_seed_entry || seed_len <= 0 || !ix->fmi.ref) return BWAMS_ERR_ARG;
    bwams_emf *e = new bwams_emf();
    e->idx = ix;
    e->t.seed_table = reinterpret_cast<const uint4 *>(seed_table_dev);
    e->t.loc_table = loc_table_dev;
    e->t.ref = ix->fmi.ref;
    e->t.num_seed_entry = num_seed_entry;
    e->t.num_loc_entry = num_loc_entry;
    e->t.seq_len = seq_len;
    e->t.seed_len = seed_len;
    e->bytes = (int64_t)num_seed_entry * 16 + (int64_t)num_loc_entry * 4;
    *out = e;
    return BWAMS_OK;
}

// the probe's per-read results: a word pair and a code byte per read
static int emf_out_ensure(bwams_batch_t *b, int64_t nseq) {
    if ((size_t)nseq <= b->emf.d_emf_code.cap) return BWAMS_OK;
    b->emf.d_emf_out.release();
    b->emf.d_emf_code.release();
    const size_t cap = (size_t)(nseq + nseq / 8 + 256);
    BWAMS_HIP(b->emf.d_emf_out.alloc(cap * 8));
    BWAMS_HIP(b->emf.d_emf_code.alloc(cap));
    return BWAMS_OK;
}

/* Resident form: probe the reads uploaded by bwams_seed_upload and set the batch's skip flags on the
 * device, so that the following bwams_seed_run leaves the matched reads out. */
int bwams_emf_run(bwams_batch_t *b, bwams_emf_t *e) {
    if (!b || !e || e->idx != b->idx || !has(b, Product::reads)) return BWAMS_ERR_ARG;
    outdated(b, Product::probe);
    BWAMS_HIP(hipSetDevice(b->idx->device));
    const int64_t nseq = b->nseq;
    if (int rc = emf_out_ensure(b, nseq)) return rc;
    hipStream_t st = b->stream;
    BWAMS_HIP(hipMemsetAsync(&b->d_ctr.p->emf_nodes, 0, 16, st));
    BWAMS_HIP(hipEventRecord(b->emf.ev[0], st));
    launch_emf_probe(e->t, b->d_enc.p, b->d_cum.p, nseq, b->emf.d_emf_out.p, b->emf.d_emf_code.p, b->d_skip.p, b->d_ctr.p, st);
    BWAMS_HIP(hipEventRecord(b->emf.ev[1], st));
    // seed_run clears the counters: keep the probe's own
    BWAMS_HIP(hipMemcpyAsync(&b->h_ctr.p->emf_nodes, &b->d_ctr.p->emf_nodes, 16, hipMemcpyDeviceToHost, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    b->emf.emf_nodes = b->h_ctr.p->emf_nodes;
    b->emf.emf_cmp_bytes = b->h_ctr.p->emf_cmp_bytes;
    BWAMS_HIP(hipGetLastError());
    b->has_skip = true;
    produced(b, Product::probe);
    return BWAMS_OK;
}

int bwams_emf_fetch(bwams_batch_t *b, bwams_perfect_t *out, uint8_t *code) {
    if (!has(b, Product::probe)) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    if (b->nseq) {
        if (out) BWAMS_HIP(hipMemcpyAsync(out, b->emf.d_emf_out.p, (size_t)b->nseq * 8, hipMemcpyDeviceToHost, b->stream));
        if (code) BWAMS_HIP(hipMemcpyAsync(code, b->emf.d_emf_code.p, (size_t)b->nseq, hipMemcpyDeviceToHost, b->stream));
    }
    BWAMS_HIP(hipStreamSynchronize(b->stream));
    return BWAMS_OK;
}

int bwams_emf_build(bwams_index_t *ix, int32_t seed_len, double slack, bwams_emf_t **out) {
    if (!ix || !out || seed_len < 16 || seed_len > 255 || !(slack >= 1.0 && slack <= 4.0)) {
        set_last_error("bwams_emf_build: seed length must be in [16, 255], slack in [1, 4]");
        return BWAMS_ERR_ARG;
    }
    if (!ix->fmi.ref) {
        set_last_error("bwams_emf_build: the index holds no .0123 reference");
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(ix->device));
    hipDeviceProp_t prop;
    BWAMS_HIP(hipGetDeviceProperties(&prop, ix->device));
    const int64_t l_pac = (ix->fmi.ref_seq_len - 1) / 2;
    if (l_pac < seed_len) {
        set_last_error("bwams_emf_build: the reference is shorter than the seed length");
        return BWAMS_ERR_ARG;
    }
    bwams_emf *e = new bwams_emf();
    e->idx = ix;
    int64_t st[4] = {0, 0, 0, 0};
    const int rc = emf_build_device(e, ix->fmi.ref, l_pac, seed_len, slack, prop.multiProcessorCount, knobs().verbose != 0, st);
    if (rc) { bwams_emf_close(e); return rc; }
    e->n_used = st[0]; e->n_key = st[1]; e->n_other = st[2]; e->build_ms = st[3];
    *out = e;
    return BWAMS_OK;
}

int bwams_emf_info(const bwams_emf_t *e, int32_t *seed_len, uint32_t *num_seed_entry, uint32_t *num_loc_entry, int64_t *n_used, int64_t *n_key,
                   int64_t *build_ms) {
    if (!e) return BWAMS_ERR_ARG;
    if (seed_len) *seed_len = e->t.seed_len;
    if (num_seed_entry) *num_seed_entry = e->t.num_seed_entry;
    if (num_loc_entry) *num_loc_entry = e->t.num_loc_entry;
    if (n_used) *n_used = e->n_used;
    if (n_key) *n_key = e->n_key;
    if (build_ms) *build_ms = e->build_ms;
    return BWAMS_OK;
}

int bwams_emf_table_fetch(bwams_emf_t *e, uint32_t *loc_table, bwams_seed_entry_t *seed_table) {
    if (!e) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(e->idx->device));
    if (loc_table && e->t.num_loc_entry) BWAMS_HIP(hipMemcpy(loc_table, e->t.loc_table, (size_t)e->t.num_loc_entry * 4, hipMemcpyDeviceToHost));
    if (seed_table) BWAMS_HIP(hipMemcpy(seed_table, e->t.seed_table, (size_t)e->t.num_seed_entry * 16, hipMemcpyDeviceToHost));
    return BWAMS_OK;
}

/* <path> in the reference's `.perfect.<L>` layout (perfect.h:188-213): 64-byte header, loc_table, seed_table */
int bwams_emf_save(bwams_emf_t *e, const char *path) {
    if (!e || !path) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(e->idx->device));
    FILE *f = fopen(path, "wb");
    if (!f) { set_last_error(std::string("bwams_emf_save: cannot create ") + path); return BWAMS_ERR_IO; }
    unsigned char hdr[64];
    memset(hdr, 0, sizeof hdr);
    const int32_t sl = e->t.seed_len;
    const uint32_t a[3] = {e->t.num_loc_entry, e->t.num_seed_entry, e->t.num_seed_entry};
    const uint32_t b3[3] = {e->t.seq_len, (uint32_t)e->n_used, (uint32_t)e->n_key};
    memcpy(hdr, &sl, 4); memcpy(hdr + 4, a, 12); memcpy(hdr + 40, b3, 12);
    int rc = fwrite(hdr, 1, 64, f) == 64 ? BWAMS_OK : BWAMS_ERR_IO;
    const size_t chunk = (size_t)256 << 20;
    HostBuf<uint8_t> stage;
    if (rc == BWAMS_OK && stage.alloc(chunk) != hipSuccess) rc = BWAMS_ERR_NOMEM;
    if (rc == BWAMS_OK) rc = dev_to_file(f, e->t.loc_table, (size_t)e->t.num_loc_entry * 4, stage.p, chunk);
    if (rc == BWAMS_OK) rc = dev_to_file(f, e->t.seed_table, (size_t)e->t.num_seed_entry * 16, stage.p, chunk);
    stage.release();
    fclose(f);
    if (rc) set_last_error(std::string("bwams_emf_save: writing ") + path + " failed");
    return rc;
}

int bwams_emf_close(bwams_emf_t *e) {
    if (!e) return BWAMS_OK;
    (void)hipSetDevice(e->idx->device);
    delete e;
    return BWAMS_OK;
}

int bwams_emf_probe(bwams_batch_t *b, bwams_emf_t *e, const uint8_t *enc, const int64_t *cum, int64_t nseq,
                    bwams_perfect_t *out, uint8_t *code) {
    if (!b || !e || !cum || nseq < 0 || (nseq && (!enc || !out || !code))) return BWAMS_ERR_ARG;
    if (e->idx != b->idx) {
        set_last_error("bwams_emf_probe: table and batch belong to different indexes");
        return BWAMS_ERR_ARG;
    }
    const int64_t nb = cum[nseq] - cum[0];
    if (cum[0] != 0 || nseq > b->max_reads || nb > b->max_bases) return BWAMS_ERR_CAPACITY;
    // the caller's reads overwrite the resident ones and the probe's words, and nothing beside them is brought up to date: whatever
    // follows needs a new bwams_seed_upload
    outdated(b, Product::reads);
    BWAMS_HIP(hipSetDevice(b->idx->device));
    if (int rc = emf_out_ensure(b, nseq)) return rc;
    hipStream_t st = b->stream;
    if (nb) BWAMS_HIP(hipMemcpyAsync(b->d_enc.p, enc, (size_t)nb, hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipMemcpyAsync(b->d_cum.p, cum, (size_t)(nseq + 1) * 8, hipMemcpyHostToDevice, st));
    launch_emf_probe(e->t, b->d_enc.p, b->d_cum.p, nseq, b->emf.d_emf_out.p, b->emf.d_emf_code.p, nullptr, nullptr, st);
    BWAMS_HIP(hipGetLastError());
    if (nseq) {
        BWAMS_HIP(hipMemcpyAsync(out, b->emf.d_emf_out.p, (size_t)nseq * 8, hipMemcpyDeviceToHost, st));
        BWAMS_HIP(hipMemcpyAsync(code, b->emf.d_emf_code.p, (size_t)nseq, hipMemcpyDeviceToHost, st));
    }
    BWAMS_HIP(hipStreamSynchronize(st));
    return BWAMS_OK;
}

}  // extern "C"
