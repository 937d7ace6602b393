// api_ert.hip — C-ABI entry points of the ERT table handle (include/bwams.h): the reference's kmer_table / mlt_table from host
// arrays, from its files or built on the GPU; info, fetch, save, close; and the two tables derived per handle, the hit-count
// table and the entry + tree-head table (bwams_ert_set_fat).  Seeding over the handle is in api_seed.hip.
#include "ert_kernels.h"

using namespace bwams;

extern "C" {

// A loaded index starts with an empty hit-count table (filled as big subtrees are counted for the first time); sized
// from the tree bytes: a four-way node with 20 or more hits below it stands for at least some hundred bytes of trees.
static int ert_count_table(bwams_ert *e) {
    int bits = 16;
    while (bits < 26 && ((int64_t)1 << bits) < e->mlt_bytes / 256) bits++;
    BWAMS_HIP(e->d_cnt.alloc((size_t)16 << bits));
    BWAMS_HIP(hipMemset(e->d_cnt.p, 0, (size_t)16 << bits));
    e->t.cnt_tab = e->d_cnt.as<uint64_t>();
    e->t.cnt_bits = bits;
    e->bytes += (int64_t)16 << bits;
    return BWAMS_OK;
}
// the resident entry + tree-head table (DevErt::fat): 64 bytes per k-mer, derived from the two tables once per index
static int ert_fat_table(bwams_ert *e) {
    if (!knobs().ert_fat) return BWAMS_OK;
    const size_t bytes = (size_t)64 << (2 * e->t.K);
    BWAMS_HIP(e->d_fat.alloc(bytes));
    launch_ert_fat(e->t, e->mlt_bytes, e->d_fat.as<uint8_t>(), 0);
    BWAMS_HIP(hipDeviceSynchronize());
    BWAMS_HIP(hipGetLastError());
    e->t.fat = e->d_fat.as<const uint8_t>();
    e->bytes += (int64_t)bytes;
    return BWAMS_OK;
}

// the handle of the two resident tables (d_kmer, d_mlt), and the two tables derived from them; closes the handle when it fails
static int ert_finish(bwams_ert *e, int K, int X, int read_len, int64_t mlt_bytes, bwams_ert_t **out) {
    e->t.kmer = e->d_kmer.as<const uint64_t>();
    e->t.mlt = e->d_mlt.as<const uint8_t>();
    e->t.ref = e->idx->fmi.ref;
    e->t.ref_len = e->idx->fmi.ref_seq_len - 1;
    e->t.K = K; e->t.X = X; e->t.read_len = read_len;
    e->bytes = (int64_t)(((size_t)1 << (2 * K)) * 8) + mlt_bytes + 16;
    e->mlt_bytes = mlt_bytes;
    int rc = ert_count_table(e);
    if (!rc) rc = ert_fat_table(e);
    if (rc) { bwams_ert_close(e); return rc; }
    *out = e;
    return BWAMS_OK;
}

int bwams_ert_from_host(bwams_index_t *ix, const uint64_t *kmer_table, int32_t kmer_size, int32_t xmer_size,
                        int32_t read_len, const uint8_t *mlt_table, int64_t mlt_bytes, bwams_ert_t **out) {
    if (!ix || !out || !kmer_table || (mlt_bytes && !mlt_table) || mlt_bytes < 0) return BWAMS_ERR_ARG;
    if (kmer_size < 2 || kmer_size > 15 || xmer_size < 1 || xmer_size > 8 || read_len < kmer_size + xmer_size) {
        set_last_error("bwams_ert_from_host: k-mer size must be in [2, 15], x-mer size in [1, 8]");
        return BWAMS_ERR_ARG;
    }
    if (!ix->fmi.ref) {
        set_last_error("bwams_ert_from_host: the index was opened without its .0123 reference");
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(ix->device));
    bwams_ert *e = new bwams_ert();
    e->idx = ix;
    const size_t nk = (size_t)1 << (2 * kmer_size);
    hipError_t he = e->d_kmer.alloc(nk * 8);
    if (he == hipSuccess) he = e->d_mlt.alloc((size_t)mlt_bytes + 16);
    if (he == hipSuccess) he = hipMemcpy(e->d_kmer.p, kmer_table, nk * 8, hipMemcpyHostToDevice);
    if (he == hipSuccess && mlt_bytes) he = hipMemcpy(e->d_mlt.p, mlt_table, (size_t)mlt_bytes, hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemset(e->d_mlt.as<uint8_t>() + mlt_bytes, 0, 16);
    if (he != hipSuccess) {
        set_last_error(std::string("bwams_ert_from_host: ") + hipGetErrorString(he));
        bwams_ert_close(e);
        return he == hipErrorOutOfMemory ? BWAMS_ERR_NOMEM : BWAMS_ERR_DEVICE;
    }
    return ert_finish(e, kmer_size, xmer_size, read_len, mlt_bytes, out);
}

int bwams_ert_open(bwams_index_t *ix, const char *prefix, int32_t read_len, bwams_ert_t **out) {
    if (!ix || !prefix || !out) return BWAMS_ERR_ARG;
    if (!ix->fmi.ref) {
        set_last_error("bwams_ert_open: the index was opened without its .0123 reference");
        return BWAMS_ERR_ARG;
    }
    const int K = 15, X = 4;                       // kmerSize / xmerSize, src/macro.h:204-206
    const std::string fk = std::string(prefix) + ".kmer_table", fm = std::string(prefix) + ".mlt_table";
    FILE *f1 = fopen(fk.c_str(), "rb"), *f2 = fopen(fm.c_str(), "rb");
    if (!f1 || !f2) {
        if (f1) fclose(f1);
        if (f2) fclose(f2);
        set_last_error("bwams_ert_open: cannot open " + (f1 ? fm : fk));
        return BWAMS_ERR_IO;
    }
    fseek(f2, 0, SEEK_END);
    const int64_t mlt_bytes = (int64_t)ftell(f2);
    fseek(f2, 0, SEEK_SET);
    BWAMS_HIP(hipSetDevice(ix->device));
    bwams_ert *e = new bwams_ert();
    e->idx = ix;
    const size_t nk = (size_t)1 << (2 * K);
    int rc = BWAMS_OK;
    const size_t chunk = (size_t)256 << 20;          // streamed through one pinned staging buffer
    HostBuf<uint8_t> stage;
    hipError_t he = e->d_kmer.alloc(nk * 8);
    if (he == hipSuccess) he = e->d_mlt.alloc((size_t)mlt_bytes + 16);
    if (he == hipSuccess) he = stage.alloc(chunk);
    if (he != hipSuccess) rc = he == hipErrorOutOfMemory ? BWAMS_ERR_NOMEM : BWAMS_ERR_DEVICE;
    if (rc == BWAMS_OK) rc = file_to_dev(f1, e->d_kmer.p, nk * 8, stage.p, chunk);
    if (rc == BWAMS_OK) rc = file_to_dev(f2, e->d_mlt.p, (size_t)mlt_bytes, stage.p, chunk);
    if (rc == BWAMS_OK && hipMemset(e->d_mlt.as<uint8_t>() + mlt_bytes, 0, 16) != hipSuccess) rc = BWAMS_ERR_DEVICE;
    fclose(f1); fclose(f2);
    stage.release();
    if (rc != BWAMS_OK) {
        set_last_error("bwams_ert_open: reading " + fk + " / " + fm + " failed");
        bwams_ert_close(e);
        return rc;
    }
    return ert_finish(e, K, X, read_len, mlt_bytes, out);
}

int bwams_ert_build(bwams_index_t *ix, int32_t kmer_size, int32_t xmer_size, int32_t read_len, int32_t hit_threshold,
                    bwams_ert_t **out) {
    if (!ix || !out) return BWAMS_ERR_ARG;
    if (kmer_size < 2 || kmer_size > 15 || xmer_size < 1 || xmer_size > 8 || read_len < kmer_size + xmer_size || read_len > 255 ||
        hit_threshold < 1) {
        set_last_error("bwams_ert_build: k-mer size must be in [2, 15], x-mer size in [1, 8], read length in [k + x, 255]");
        return BWAMS_ERR_ARG;
    }
    if (!ix->fmi.ref) {
        set_last_error("bwams_ert_build: the index holds no .0123 reference (leaf expansion reads it)");
        return BWAMS_ERR_ARG;
    }
    BWAMS_HIP(hipSetDevice(ix->device));
    hipDeviceProp_t prop;
    BWAMS_HIP(hipGetDeviceProperties(&prop, ix->device));
    bwams_ert *e = new bwams_ert();
    e->idx = ix;
    const int rc = ert_build_device(e, ix->fmi, kmer_size, xmer_size, read_len, hit_threshold, prop.multiProcessorCount,
                                    knobs().verbose != 0);
    if (rc) { bwams_ert_close(e); return rc; }
    if (int crc = ert_fat_table(e)) { bwams_ert_close(e); return crc; }
    *out = e;
    return BWAMS_OK;
}

int bwams_ert_info(const bwams_ert_t *e, int32_t *kmer_size, int32_t *xmer_size, int32_t *read_len, int64_t *mlt_bytes,
                   float build_ms[3]) {
    if (!e) return BWAMS_ERR_ARG;
    if (kmer_size) *kmer_size = e->t.K;
    if (xmer_size) *xmer_size = e->t.X;
    if (read_len) *read_len = e->t.read_len;
    if (mlt_bytes) *mlt_bytes = e->mlt_bytes;
    if (build_ms) for (int i = 0; i < 3; ++i) build_ms[i] = e->build_ms[i];
    return BWAMS_OK;
}

int bwams_ert_fetch(bwams_ert_t *e, uint64_t *kmer_table, uint8_t *mlt_table) {
    if (!e) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(e->idx->device));
    if (kmer_table) BWAMS_HIP(hipMemcpy(kmer_table, e->d_kmer.p, ((size_t)1 << (2 * e->t.K)) * 8, hipMemcpyDeviceToHost));
    if (mlt_table && e->mlt_bytes) BWAMS_HIP(hipMemcpy(mlt_table, e->d_mlt.p, (size_t)e->mlt_bytes, hipMemcpyDeviceToHost));
    return BWAMS_OK;
}

int bwams_ert_save(bwams_ert_t *e, const char *prefix) {
    if (!e || !prefix) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(e->idx->device));
    const size_t chunk = (size_t)256 << 20;
    HostBuf<uint8_t> stage;
    BWAMS_HIP(stage.alloc(chunk));
    int rc = BWAMS_OK;
    auto stream_out = [&](const std::string &path, const void *src, size_t total) {
        FILE *f = fopen(path.c_str(), "wb");
        if (!f) { rc = BWAMS_ERR_IO; set_last_error("bwams_ert_save: cannot create " + path); return; }
        rc = dev_to_file(f, src, total, stage.p, chunk);
        if (rc == BWAMS_ERR_IO) set_last_error("bwams_ert_save: short write to " + path);
        fclose(f);
    };
    stream_out(std::string(prefix) + ".kmer_table", e->d_kmer.p, ((size_t)1 << (2 * e->t.K)) * 8);
    if (rc == BWAMS_OK) stream_out(std::string(prefix) + ".mlt_table", e->d_mlt.p, (size_t)e->mlt_bytes);
    return rc;
}

int bwams_ert_close(bwams_ert_t *e) {
    if (!e) return BWAMS_OK;
    (void)hipSetDevice(e->idx->device);
    delete e;
    return BWAMS_OK;
}

int64_t bwams_ert_bytes(const bwams_ert_t *e) { return e ? e->bytes : 0; }

int bwams_ert_set_fat(bwams_ert_t *e, int32_t on) {
    if (!e) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(e->idx->device));
    BWAMS_HIP(hipDeviceSynchronize());                   // no walk is reading it
    if (on) {
        if (e->d_fat.p) return BWAMS_OK;
        const size_t bytes = (size_t)64 << (2 * e->t.K);
        BWAMS_HIP(e->d_fat.alloc(bytes));
        launch_ert_fat(e->t, e->mlt_bytes, e->d_fat.as<uint8_t>(), 0);
        BWAMS_HIP(hipDeviceSynchronize());
        e->t.fat = e->d_fat.as<const uint8_t>();
        e->bytes += (int64_t)bytes;
        return BWAMS_OK;
    }
    if (e->d_fat.p) {
        e->d_fat.release();
        e->t.fat = nullptr;
        e->bytes -= (int64_t)64 << (2 * e->t.K);
    }
    return BWAMS_OK;
}

}  // extern "C"
