// api_index.hip — C-ABI entry points of the FM-index handle (include/bwams.h): an index from host or device arrays, from the
// reference's files (bwams_index_open), built on the GPU (bwams_index_build); its fetch, save and close; and the FMA tables on it.
#include <cstring>

#include "fmi_kernels.h"

namespace bwams {
int fmi_build_device(bwams_index *ix, const uint8_t *d_fw, int64_t l_pac, int keep_ref, int64_t chunk_rows, int verbose,
                     bwams_build_stats_t *bs);                   // fmi_build.hip

// Every live index, for sa_dense_release.  Lock order: g_ix_mu, then an index's sa_mu; nothing allocates under either but the
// table's own build, which does not come back here (dev_malloc's may_yield = false).
static std::mutex g_ix_mu;
static std::vector<bwams_index *> g_ix;
}

bwams_index::bwams_index() {
    std::lock_guard<std::mutex> reg(bwams::g_ix_mu);
    bwams::g_ix.push_back(this);
}
bwams_index::~bwams_index() {
    std::lock_guard<std::mutex> reg(bwams::g_ix_mu);
    for (size_t i = 0; i < bwams::g_ix.size(); ++i)
        if (bwams::g_ix[i] == this) { bwams::g_ix.erase(bwams::g_ix.begin() + i); break; }
}

namespace bwams {

// The caller's current device is `device` (dev_malloc: the device it allocates on).  A lookup that reads a table was launched under
// the shared lock, so once the exclusive lock is held every such launch is queued and the device synchronisation waits for it.
int sa_dense_release(int device) {
    int n = 0;
    std::lock_guard<std::mutex> reg(g_ix_mu);
    for (bwams_index *ix : g_ix) {
        if (ix->device != device) continue;
        std::unique_lock<std::shared_mutex> lock(ix->sa_mu);
        if (ix->sa_state != BWAMS_SA_DENSE_BUILT) continue;
        (void)hipDeviceSynchronize();
        ix->d_sa_dense.release();
        ix->sa_bytes = 0;
        ix->sa_state = BWAMS_SA_DENSE_YIELDED;           // for the rest of the index's life: no rebuild, nothing thrashes
        if (knobs().verbose) fprintf(stderr, "[sa_dense] device %d out of memory: the table of stride %d gave way\n", device, ix->sa_stride);
        ++n;
    }
    return n;
}

// The table of ix, built at its first FM-index seeding that wants coordinates.  A table that is switched off, above the cap, not
// allocatable or not representable leaves the index walking (state "refused"): no error.
int sa_dense_ensure(bwams_index *ix, int cu_count, hipStream_t st) {
    const Knobs &kn = knobs();
    if (kn.sa_dense == 0) return BWAMS_OK;
    {
        std::shared_lock<std::shared_mutex> lock(ix->sa_mu);
        if (ix->sa_state != BWAMS_SA_DENSE_ABSENT) return BWAMS_OK;
    }
    std::unique_lock<std::shared_mutex> lock(ix->sa_mu);
    if (ix->sa_state != BWAMS_SA_DENSE_ABSENT) return BWAMS_OK;
    const int stride = kn.sa_dense;
    const int64_t n = sa_dense_entries(ix->fmi.ref_seq_len, stride), bytes = n * 8;
    ix->sa_stride = stride;
    if (kn.sa_dense_max_bytes > 0 && bytes > kn.sa_dense_max_bytes) {
        ix->sa_state = BWAMS_SA_DENSE_REFUSED;
        return BWAMS_OK;
    }
    DevBuf<> t;
    if (t.alloc((size_t)bytes + 8, false) != hipSuccess) {            // + the build's flag word; never through the yielding path
        (void)hipGetLastError();
        ix->sa_state = BWAMS_SA_DENSE_REFUSED;
        if (kn.verbose) fprintf(stderr, "[sa_dense] no room for %.1f GiB: the index keeps the walk\n", bytes / 1073741824.0);
        return BWAMS_OK;
    }
    unsigned long long *d_bad = reinterpret_cast<unsigned long long *>(t.as<uint64_t>() + n), bad = 0;
    hipEvent_t ev[2];
    BWAMS_HIP(hipEventCreate(&ev[0]));
    BWAMS_HIP(hipEventCreate(&ev[1]));
    hipError_t e = hipMemsetAsync(d_bad, 0, 8, st);
    if (e == hipSuccess) e = hipEventRecord(ev[0], st);
    if (e == hipSuccess) {
        launch_sa_dense_build(ix->fmi, stride, n, t.as<uint64_t>(), d_bad, cu_count, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ev[1], st);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    float ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
    BWAMS_HIP(e);
    ix->sa_build_ms = ms;
    if (bad) {
        fprintf(stderr, "[sa_dense] a walk of this index does not fit the table's %d-bit step field: the index keeps the walk\n", kSaDenseStepBits);
        ix->sa_state = BWAMS_SA_DENSE_REFUSED;
        return BWAMS_OK;
    }
    ix->d_sa_dense = std::move(t);
    ix->sa_bytes = bytes;
    ix->sa_state = BWAMS_SA_DENSE_BUILT;
    if (kn.verbose) fprintf(stderr, "[sa_dense] stride %d: %lld entries, %.2f GiB, built in %.1f ms\n", stride, (long long)n, bytes / 1073741824.0, ms);
    return BWAMS_OK;
}

}  // namespace bwams

using namespace bwams;

extern "C" {

static int index_finish(bwams_index *ix, const bwams_fmi_desc_t *d, const void *cp, const void *ms, const void *ls, const void *ref) {
    ix->fmi.cp = reinterpret_cast<const uint4 *>(cp);
    ix->fmi.cp2 = nullptr;
    ix->fmi.sa_ms = reinterpret_cast<const int8_t *>(ms);
    ix->fmi.sa_ls = reinterpret_cast<const uint32_t *>(ls);
    ix->fmi.ref = reinterpret_cast<const uint8_t *>(ref);
    if (d->ref_seq_len >= ((int64_t)1 << 36)) {
        set_last_error("text longer than 2^36 rows is not supported by the 36-bit interval packing");
        return BWAMS_ERR_UNSUPPORTED;
    }
    for (int i = 0; i < 5; ++i) ix->fmi.count[i] = d->count[i];
    ix->fmi.sentinel = d->sentinel_index;
    ix->fmi.ref_seq_len = d->ref_seq_len;
    return BWAMS_OK;
}

int bwams_index_from_host(const bwams_fmi_desc_t *d, int device, bwams_index_t **out) {
    if (!d || !out || !d->cp_occ || !d->sa_ms_byte || !d->sa_ls_word || d->ref_seq_len <= 0) {
        set_last_error("bwams_index_from_host: null or empty descriptor");
        return BWAMS_ERR_ARG;
    }
    int rc = check_device(device);
    if (rc) return rc;
    BWAMS_HIP(hipSetDevice(device));
    bwams_index *ix = new bwams_index();
    ix->device = device;
    ix->n_blk = (d->ref_seq_len >> 6) + 1;
    ix->n_sa = (d->ref_seq_len >> 3) + 1;
    const size_t b_cp = (size_t)ix->n_blk * 64, b_ms = (size_t)ix->n_sa, b_ls = (size_t)ix->n_sa * 4;
    const size_t b_ref = d->ref_0123 ? (size_t)(d->ref_seq_len - 1) : 0;
    // a failed allocation or copy must not strand the multi-GB buffers already made: close the handle on the way out
    auto up = [&](DevBuf<> *dst, const void *src, size_t bytes) -> hipError_t {
        hipError_t e = dst->alloc(bytes + 64);               // slack: kernels read whole aligned words
        return e != hipSuccess ? e : hipMemcpy(dst->p, src, bytes, hipMemcpyHostToDevice);
    };
    hipError_t ue = up(&ix->d_cp, d->cp_occ, b_cp);
    if (ue == hipSuccess) ue = up(&ix->d_ms, d->sa_ms_byte, b_ms);
    if (ue == hipSuccess) ue = up(&ix->d_ls, d->sa_ls_word, b_ls);
    if (ue == hipSuccess && b_ref) ue = up(&ix->d_ref, d->ref_0123, b_ref);
    if (ue != hipSuccess) {
        bwams_index_close(ix);
        BWAMS_HIP(ue);
    }
    ix->bytes = (int64_t)(b_cp + b_ms + b_ls + b_ref);
    int frc = index_finish(ix, d, ix->d_cp.p, ix->d_ms.p, ix->d_ls.p, ix->d_ref.p);
    if (frc) { bwams_index_close(ix); return frc; }
    *out = ix;
    return BWAMS_OK;
}

int bwams_index_from_device(const bwams_fmi_desc_t *d, int device, bwams_index_t **out) {
    if (!d || !out || !d->cp_occ || !d->sa_ms_byte || !d->sa_ls_word || d->ref_seq_len <= 0) {
        set_last_error("bwams_index_from_device: null or empty descriptor");
        return BWAMS_ERR_ARG;
    }
    int rc = check_device(device);
    if (rc) return rc;
    bwams_index *ix = new bwams_index();
    ix->device = device;
    ix->n_blk = (d->ref_seq_len >> 6) + 1;
    ix->n_sa = (d->ref_seq_len >> 3) + 1;
    ix->bytes = ix->n_blk * 64 + ix->n_sa * 5 + (d->ref_0123 ? d->ref_seq_len - 1 : 0);
    int frc = index_finish(ix, d, d->cp_occ, d->sa_ms_byte, d->sa_ls_word, d->ref_0123);
    if (frc) { bwams_index_close(ix); return frc; }
    *out = ix;
    return BWAMS_OK;
}

// <prefix>.bwt.2bit.64 and, when it is there, <prefix>.0123: mapped while they are uploaded
static int index_open_fmi(const char *prefix, int device, bwams_index_t **out) {
    const std::string path = std::string(prefix) + ".bwt.2bit.64";
    MappedFile mf(path, 56);
    if (!mf.opened) { set_last_error("cannot open " + path); return BWAMS_ERR_IO; }
    if (mf.size < 56) { set_last_error(path + ": truncated"); return BWAMS_ERR_IO; }
    if (!mf.p) { set_last_error("mmap failed: " + path); return BWAMS_ERR_IO; }
    const uint8_t *m = mf.p;
    bwams_fmi_desc_t d;
    memset(&d, 0, sizeof d);
    memcpy(&d.ref_seq_len, m, 8);
    int64_t cnt[5];
    memcpy(cnt, m + 8, 40);
    for (int i = 0; i < 5; ++i) d.count[i] = cnt[i] + 1;   // as the reference loader does (FMI_search.cpp:880-883)
    const int64_t n_blk = (d.ref_seq_len >> 6) + 1, n_sa = (d.ref_seq_len >> 3) + 1;
    const size_t need = 48 + (size_t)n_blk * 64 + (size_t)n_sa * 5 + 8;
    if (d.ref_seq_len <= 0 || mf.size != need) { set_last_error(path + ": size does not match its header"); return BWAMS_ERR_IO; }
    size_t o = 48;
    d.cp_occ = reinterpret_cast<const bwams_cp_occ_t *>(m + o);
    o += (size_t)n_blk * 64;
    d.sa_ms_byte = reinterpret_cast<const int8_t *>(m + o);
    o += (size_t)n_sa;
    // sa_ls_word is not 4-byte aligned in the file in general: stage through an aligned copy
    std::vector<uint32_t> ls((size_t)n_sa);
    memcpy(ls.data(), m + o, (size_t)n_sa * 4);
    d.sa_ls_word = ls.data();
    o += (size_t)n_sa * 4;
    memcpy(&d.sentinel_index, m + o, 8);

    MappedFile rm(std::string(prefix) + ".0123");                   // optional
    d.ref_0123 = rm.size == (size_t)(d.ref_seq_len - 1) ? rm.p : nullptr;
    return bwams_index_from_host(&d, device, out);
}

int bwams_index_open(const char *prefix, int device, bwams_index_t **out) {
    if (!prefix || !out) return BWAMS_ERR_ARG;
    int rc = index_open_fmi(prefix, device, out);
    if (rc) return rc;
    // optional FMA tables written by `bwa-mem2.scale smem-table` (src/FMI_search.cpp:228-277)
    MappedFile ma(std::string(prefix) + ".all_smem.11"), ml(std::string(prefix) + ".last_smem.13");
    if (ma.p && ml.p && ma.size == ((size_t)1 << 22) * 128 && ml.size == ((size_t)1 << 26) * 16)
        rc = bwams_index_set_fma(*out, ma.p, 11, ml.p, 13);
    return rc;
}

int bwams_index_build(const uint8_t *fw, int64_t l_pac, int fw_on_device, int device, int keep_ref, int64_t chunk_rows,
                      bwams_build_stats_t *stats, bwams_index_t **out) {
    if (!fw || !out || l_pac <= 0) {
        set_last_error("bwams_index_build: null or empty sequence");
        return BWAMS_ERR_ARG;
    }
    int rc = check_device(device);
    if (rc) return rc;
    BWAMS_HIP(hipSetDevice(device));
    DevBuf<uint8_t> staged;
    if (!fw_on_device) {
        BWAMS_HIP(staged.alloc((size_t)l_pac));
        BWAMS_HIP(hipMemcpy(staged.p, fw, (size_t)l_pac, hipMemcpyHostToDevice));
    }
    bwams_index *ix = new bwams_index();
    ix->device = device;
    rc = fmi_build_device(ix, staged.p ? staged.p : fw, l_pac, keep_ref, chunk_rows, knobs().verbose != 0, stats);
    staged.release();
    if (rc) { bwams_index_close(ix); return rc; }
    *out = ix;
    return BWAMS_OK;
}

int bwams_index_fetch(bwams_index_t *ix, bwams_cp_occ_t *cp_occ, int8_t *sa_ms_byte, uint32_t *sa_ls_word, uint8_t *ref_0123,
                      bwams_fmi_desc_t *d) {
    if (!ix) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(ix->device));
    if (cp_occ) BWAMS_HIP(hipMemcpy(cp_occ, ix->fmi.cp, (size_t)ix->n_blk * 64, hipMemcpyDeviceToHost));
    if (sa_ms_byte) BWAMS_HIP(hipMemcpy(sa_ms_byte, ix->fmi.sa_ms, (size_t)ix->n_sa, hipMemcpyDeviceToHost));
    if (sa_ls_word) BWAMS_HIP(hipMemcpy(sa_ls_word, ix->fmi.sa_ls, (size_t)ix->n_sa * 4, hipMemcpyDeviceToHost));
    if (ref_0123) {
        if (!ix->fmi.ref) {
            set_last_error("bwams_index_fetch: the index holds no .0123 text");
            return BWAMS_ERR_ARG;
        }
        BWAMS_HIP(hipMemcpy(ref_0123, ix->fmi.ref, (size_t)(ix->fmi.ref_seq_len - 1), hipMemcpyDeviceToHost));
    }
    if (d) {
        memset(d, 0, sizeof *d);
        d->ref_seq_len = ix->fmi.ref_seq_len;
        for (int i = 0; i < 5; ++i) d->count[i] = ix->fmi.count[i];
        d->sentinel_index = ix->fmi.sentinel;
    }
    return BWAMS_OK;
}

int bwams_index_save(bwams_index_t *ix, const char *prefix) {
    if (!ix || !prefix) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(ix->device));
    const size_t kSlab = (size_t)256 << 20;
    std::vector<uint8_t> slab(kSlab);
    auto stream_out = [&](FILE *f, const void *dev, size_t bytes) { return dev_to_file(f, dev, bytes, slab.data(), kSlab); };
    std::string path = std::string(prefix) + ".bwt.2bit.64";
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) {
        set_last_error("cannot create " + path);
        return BWAMS_ERR_IO;
    }
    int64_t hdr[6];
    hdr[0] = ix->fmi.ref_seq_len;
    for (int i = 0; i < 5; ++i) hdr[1 + i] = ix->fmi.count[i] - 1;          // the file holds them without the loader's +1
    int rc = fwrite(hdr, 8, 6, f) == 6 ? BWAMS_OK : BWAMS_ERR_IO;
    if (!rc) rc = stream_out(f, ix->fmi.cp, (size_t)ix->n_blk * 64);
    if (!rc) rc = stream_out(f, ix->fmi.sa_ms, (size_t)ix->n_sa);
    if (!rc) rc = stream_out(f, ix->fmi.sa_ls, (size_t)ix->n_sa * 4);
    const int64_t sent = ix->fmi.sentinel;
    if (!rc && fwrite(&sent, 8, 1, f) != 1) rc = BWAMS_ERR_IO;
    if (fclose(f) != 0 && !rc) rc = BWAMS_ERR_IO;
    if (!rc && ix->fmi.ref) {
        path = std::string(prefix) + ".0123";
        f = fopen(path.c_str(), "wb");
        if (!f) rc = BWAMS_ERR_IO;
        else {
            rc = stream_out(f, ix->fmi.ref, (size_t)(ix->fmi.ref_seq_len - 1));
            if (fclose(f) != 0 && !rc) rc = BWAMS_ERR_IO;
        }
    }
    if (rc == BWAMS_ERR_IO) set_last_error("write failed: " + path);
    if (!rc && ix->bns) rc = bns_save(ix, prefix);
    return rc;
}

int bwams_index_close(bwams_index_t *ix) {
    if (!ix) return BWAMS_OK;
    (void)hipSetDevice(ix->device);
    delete ix->bns;
    delete ix;
    return BWAMS_OK;
}

// the index's own arrays: what it derives at its first seeding (the search kernels' table, the dense suffix-array table) is not in
// here — a fresh handle and a used one of the same index report the same (bwams_debug_sa_dense_state reports the dense table's bytes)
int64_t bwams_index_bytes(const bwams_index_t *ix) { return ix ? ix->bytes : 0; }

int bwams_debug_sa_dense_state(bwams_index_t *ix, int32_t *state, int32_t *stride, int64_t *bytes, float *build_ms) {
    if (!ix) return BWAMS_ERR_ARG;
    std::shared_lock<std::shared_mutex> lock(ix->sa_mu);
    if (state) *state = ix->sa_state;
    if (stride) *stride = ix->sa_stride;
    if (bytes) *bytes = ix->sa_bytes.load();
    if (build_ms) *build_ms = ix->sa_build_ms;
    return BWAMS_OK;
}

int bwams_debug_sa_dense_fetch(bwams_index_t *ix, uint64_t *out, int64_t cap, int64_t *n) {
    if (!ix || !n) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(ix->device));
    std::shared_lock<std::shared_mutex> lock(ix->sa_mu);                // the table cannot give way under the copy
    if (ix->sa_state != BWAMS_SA_DENSE_BUILT) {
        set_last_error("bwams_debug_sa_dense_fetch: the index holds no dense table");
        return BWAMS_ERR_ARG;
    }
    *n = sa_dense_entries(ix->fmi.ref_seq_len, ix->sa_stride);
    if (!out) return BWAMS_OK;
    if (cap < *n) return BWAMS_ERR_CAPACITY;
    BWAMS_HIP(hipMemcpy(out, ix->d_sa_dense.p, (size_t)*n * 8, hipMemcpyDeviceToHost));
    return BWAMS_OK;
}

int bwams_debug_sa_dense_release(int device, int32_t *n_released) {
    int rc = check_device(device);
    if (rc) return rc;
    BWAMS_HIP(hipSetDevice(device));
    const int n = sa_dense_release(device);
    if (n_released) *n_released = n;
    return BWAMS_OK;
}

/* ------------------------------------------------------------------- FMA ---- */

static int fma_alloc(bwams_index *ix, int all_bp, int last_bp) {
    if (all_bp < 2 || all_bp > 11 || last_bp < 2 || last_bp > 13) {
        set_last_error("FMA depths must be 2..11 (all_smem) and 2..13 (last_smem)");
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(ix->device));
    ix->d_all.release();
    ix->d_last.release();
    ix->fmi.all_smem = nullptr;
    ix->fmi.last_smem = nullptr;
    BWAMS_HIP(ix->d_all.alloc(((size_t)1 << (2 * all_bp)) * 128));
    BWAMS_HIP(ix->d_last.alloc(((size_t)1 << (2 * last_bp)) * 16));
    return BWAMS_OK;
}

static void fma_attach(bwams_index *ix, int all_bp, int last_bp) {
    ix->fmi.all_smem = ix->d_all.as<const uint32_t>();
    ix->fmi.last_smem = ix->d_last.as<const uint4>();
    ix->fmi.all_bp = all_bp;
    ix->fmi.last_bp = last_bp;
}

int bwams_index_build_fma(bwams_index_t *ix, int all_bp, int last_bp) {
    if (!ix) return BWAMS_ERR_ARG;
    int rc = fma_alloc(ix, all_bp, last_bp);
    if (rc) return rc;
    launch_build_fma(ix->fmi, all_bp, ix->d_all.as<uint32_t>(), last_bp, ix->d_last.as<uint4>(), nullptr);
    BWAMS_HIP(hipGetLastError());
    BWAMS_HIP(hipDeviceSynchronize());
    fma_attach(ix, all_bp, last_bp);
    return BWAMS_OK;
}

int bwams_index_set_fma(bwams_index_t *ix, const void *all_smem, int all_bp, const void *last_smem, int last_bp) {
    if (!ix) return BWAMS_ERR_ARG;
    if (!all_smem || !last_smem) {                         // detach: FM-index only
        ix->fmi.all_smem = nullptr;
        ix->fmi.last_smem = nullptr;
        return BWAMS_OK;
    }
    int rc = fma_alloc(ix, all_bp, last_bp);
    if (rc) return rc;
    BWAMS_HIP(hipMemcpy(ix->d_all.p, all_smem, ((size_t)1 << (2 * all_bp)) * 128, hipMemcpyHostToDevice));
    BWAMS_HIP(hipMemcpy(ix->d_last.p, last_smem, ((size_t)1 << (2 * last_bp)) * 16, hipMemcpyHostToDevice));
    fma_attach(ix, all_bp, last_bp);
    return BWAMS_OK;
}

int bwams_index_fetch_fma(bwams_index_t *ix, void *all_smem, void *last_smem) {
    if (!ix || !ix->d_all.p || !ix->d_last.p) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(ix->device));
    if (all_smem) BWAMS_HIP(hipMemcpy(all_smem, ix->d_all.p, ((size_t)1 << (2 * ix->fmi.all_bp)) * 128, hipMemcpyDeviceToHost));
    if (last_smem) BWAMS_HIP(hipMemcpy(last_smem, ix->d_last.p, ((size_t)1 << (2 * ix->fmi.last_bp)) * 16, hipMemcpyDeviceToHost));
    return BWAMS_OK;
}

}  // extern "C"
