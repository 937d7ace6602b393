// api.hip — what every entry-point file of the C-ABI (include/bwams.h) stands on: the knobs, the error text, the device check,
// device memory to and from files, mapped files, the batch's rocPRIM storage; and the batch itself: create, destroy, sync, stats.
// There is no CPU fallback behind the C-ABI: every entry point either runs the HIP kernels on a gfx950 device or returns an error code.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstring>

#include "stage_state.h"

namespace bwams {

static Knobs g_knobs;
static std::once_flag g_knobs_once;
static int env_int(const char *name, int dflt) { const char *e = getenv(name); return e && *e ? atoi(e) : dflt; }
void knobs_reload() {
    Knobs k;
    { const char *vb = getenv("BWAMS_VERBOSE"); k.verbose = vb && *vb && *vb != '0'; }
    k.debug = env_int("BWAMS_DEBUG", 0);
    k.poison = env_int("BWAMS_POISON", 0);
    k.bwd_min_list = env_int("BWAMS_BWD_MIN_LIST", k.bwd_min_list); k.bwd_cols = env_int("BWAMS_BWD_COLS", k.bwd_cols);
    k.bwd_late_list = env_int("BWAMS_BWD_LATE_LIST", k.bwd_late_list);
    k.bwd_dry_min_list = env_int("BWAMS_BWD_DRY_MIN_LIST", k.bwd_dry_min_list); k.bwd_dry_cols = env_int("BWAMS_BWD_DRY_COLS", k.bwd_dry_cols);
    k.bwd_dry_late_list = env_int("BWAMS_BWD_DRY_LATE_LIST", k.bwd_dry_late_list);
    k.r3_beside = env_int("BWAMS_SEED_R3_BESIDE", 1);
    k.ext_max_rounds = env_int("BWAMS_EXT_MAX_ROUNDS", 0); k.ext_all_rounds = getenv("BWAMS_EXT_ALL_ROUNDS") != nullptr;
    k.ext_inplace = env_int("BWAMS_EXT_INPLACE", 1);
    k.dedup_seq = env_int("BWAMS_DEDUP_SEQ", 0) == 1;
    k.dedup_count = env_int("BWAMS_DEDUP_COUNT", 0) == 1;
    k.pair_count = env_int("BWAMS_PAIR_COUNT", 0) == 1;
    k.pair_drop_plan = getenv("BWAMS_PAIR_DROP_PLAN") != nullptr;
    k.trace_pair = env_int("BWAMS_TRACE_PAIR", 0);
    k.bsw_pk = env_int("BWAMS_BSW_PK", 1);
    k.bsw_early = env_int("BWAMS_BSW_EARLY", -1);
    k.chain_batch = env_int("BWAMS_CHAIN_BATCH", 1);
    k.chain_count = env_int("BWAMS_CHAIN_COUNT", 0) == 1;
    k.depth_combine = env_int("BWAMS_DEPTH_COMBINE", 1);
    k.pileup_tiled = env_int("BWAMS_PILEUP_TILED", 1);
    k.qc_lanes = env_int("BWAMS_QC_LANES", 1);
    k.recal_lds = env_int("BWAMS_RECAL_LDS", 1);
    k.ert_ticket = env_int("BWAMS_ERT_TICKET", 1); k.ert_grid = env_int("BWAMS_ERT_GRID", -1); k.ert_fat = env_int("BWAMS_ERT_FAT", 1);
    k.sa_dense = env_int("BWAMS_SA_DENSE", kSaDenseDefault);
    if (k.sa_dense != 0 && k.sa_dense != 1 && k.sa_dense != 2 && k.sa_dense != 4) k.sa_dense = kSaDenseDefault;
    { const char *mb = getenv("BWAMS_SA_DENSE_MAX_BYTES"); k.sa_dense_max_bytes = mb && *mb ? atoll(mb) : 0; }
    k.sort_narrow = env_int("BWAMS_SORT_NARROW", 1);
    g_knobs = k;
}
const Knobs &knobs() {
    std::call_once(g_knobs_once, knobs_reload);
    return g_knobs;
}

static thread_local std::string g_last_error;
void set_last_error(const std::string &s) { g_last_error = s; }

int check_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_last_error(std::string("no HIP device: ") + hipGetErrorString(e));
        return BWAMS_ERR_DEVICE;
    }
    if (device < 0 || device >= n) {
        set_last_error("device ordinal out of range");
        return BWAMS_ERR_ARG;
    }
    hipDeviceProp_t p;
    BWAMS_HIP(hipGetDeviceProperties(&p, device));
    if (std::string(p.gcnArchName).rfind("gfx950", 0) != 0) {
        set_last_error(std::string("device is ") + p.gcnArchName + ", this library is built for gfx950 only");
        return BWAMS_ERR_DEVICE;
    }
    return BWAMS_OK;
}

int tmp_reserve(bwams_batch *b, size_t &tb) {
    if (tb > b->d_tmp.cap) {
        BWAMS_HIP(hipStreamSynchronize(b->stream));
        BWAMS_HIP(b->d_tmp.alloc(tb));
    }
    tb = b->d_tmp.cap;
    return BWAMS_OK;
}

int dev_to_file(FILE *f, const void *dev, size_t bytes, uint8_t *stage, size_t chunk) {
    for (size_t o = 0; o < bytes; o += chunk) {
        const size_t n = std::min(chunk, bytes - o);
        BWAMS_HIP(hipMemcpy(stage, (const uint8_t *)dev + o, n, hipMemcpyDeviceToHost));
        if (fwrite(stage, 1, n, f) != n) return BWAMS_ERR_IO;
    }
    return BWAMS_OK;
}
int file_to_dev(FILE *f, void *dev, size_t bytes, uint8_t *stage, size_t chunk) {
    for (size_t o = 0; o < bytes; o += chunk) {
        const size_t n = std::min(chunk, bytes - o);
        if (fread(stage, 1, n, f) != n) return BWAMS_ERR_IO;
        BWAMS_HIP(hipMemcpy((uint8_t *)dev + o, stage, n, hipMemcpyHostToDevice));
    }
    return BWAMS_OK;
}

MappedFile::MappedFile(const std::string &path, size_t min_size) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return;
    opened = true;
    struct stat st;
    if (fstat(fd, &st) == 0) size = (size_t)st.st_size;
    if (size >= min_size && size > 0) {
        void *m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m != MAP_FAILED) p = (const uint8_t *)m;
    }
    close(fd);
}
MappedFile::~MappedFile() {
    if (p) munmap((void *)p, size);
}
}  // namespace bwams

using namespace bwams;

extern "C" {

const char *bwams_strerror(int code) {
    switch (code) {
        case BWAMS_OK: return "ok";
        case BWAMS_ERR_DEVICE: return "no usable gfx950 device / HIP error";
        case BWAMS_ERR_IO: return "index file missing or malformed";
        case BWAMS_ERR_ARG: return "invalid argument";
        case BWAMS_ERR_CAPACITY: return "output buffer too small";
        case BWAMS_ERR_NOMEM: return "out of memory";
        case BWAMS_ERR_UNSUPPORTED: return "unsupported input";
    }
    return "unknown error";
}

const char *bwams_last_error(void) { return g_last_error.c_str(); }

// the debugging aids and A-B switches are read from the environment once; tests change a variable and call this
int bwams_debug_reload(void) { (void)bwams::knobs(); bwams::knobs_reload(); return BWAMS_OK; }

int bwams_device_count(int *n) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *n = 0;
        set_last_error(hipGetErrorString(e));
        return BWAMS_ERR_DEVICE;
    }
    *n = c;
    return BWAMS_OK;
}

// everything of bwams_batch_create that can fail half way: the caller destroys the handle (streams, events and the buffers made so
// far) when this returns an error
static int batch_create_fill(bwams_batch *b, bwams_index_t *ix, int64_t max_reads, int64_t max_bases, int64_t max_smem, int64_t max_sa) {
    b->idx = ix;
    b->max_reads = max_reads;
    b->max_bases = max_bases;
    b->max_smem = max_smem > 0 ? max_smem : 24 * max_reads + 1024;
    b->max_sa = max_sa > 0 ? max_sa : 64 * max_reads + 1024;
    hipDeviceProp_t prop;
    BWAMS_HIP(hipGetDeviceProperties(&prop, ix->device));
    b->cu_count = prop.multiProcessorCount;
    BWAMS_HIP(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    BWAMS_HIP(hipStreamCreateWithFlags(&b->sd.seed_aux, hipStreamNonBlocking));
    BWAMS_HIP(hipEventCreateWithFlags(&b->sd.seed_fork, hipEventDisableTiming));
    BWAMS_HIP(hipEventCreateWithFlags(&b->sd.seed_join, hipEventDisableTiming));
    for (auto &e : b->ev) BWAMS_HIP(hipEventCreate(&e));
    for (auto &e : b->emf.ev) BWAMS_HIP(hipEventCreate(&e));

    BWAMS_HIP(b->d_enc.alloc((size_t)max_bases + 64));
    BWAMS_HIP(b->d_cum.alloc((size_t)(max_reads + 1) * 8));
    BWAMS_HIP(b->d_skip.alloc((size_t)max_reads));
    if (int arc = alloc_smem_buffers(b, b->max_smem)) return arc;
    BWAMS_HIP(b->sd.d_sa_coord.alloc((size_t)b->max_sa * 8));
    BWAMS_HIP(b->d_ctr.alloc(sizeof(DevCounters)));
    BWAMS_HIP(b->h_ctr.alloc(sizeof(DevCounters)));
    BWAMS_HIP(hipMemset(b->d_ctr.p, 0, sizeof(DevCounters)));

    return alloc_seed_tmp(b);
}

int bwams_batch_create(bwams_index_t *ix, int64_t max_reads, int64_t max_bases, int64_t max_smem,
                       int64_t max_sa, bwams_batch_t **out) {
    if (!ix || !out || max_reads <= 0 || max_bases <= 0) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(ix->device));
    bwams_batch *b = new bwams_batch();
    const int rc = batch_create_fill(b, ix, max_reads, max_bases, max_smem, max_sa);
    if (rc) {                                   // (the message of the failing call stays in bwams_last_error)
        b->idx = ix;
        bwams_batch_destroy(b);
        return rc;
    }
    *out = b;
    return BWAMS_OK;
}

int bwams_batch_destroy(bwams_batch_t *b) {
    if (!b) return BWAMS_OK;
    (void)hipSetDevice(b->idx->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    if (b->stages) stage_state_free(b->stages);
    for (auto &e : b->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : b->emf.ev)
        if (e) (void)hipEventDestroy(e);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    if (b->sd.seed_aux) (void)hipStreamDestroy(b->sd.seed_aux);
    if (b->sd.seed_fork) (void)hipEventDestroy(b->sd.seed_fork);
    if (b->sd.seed_join) (void)hipEventDestroy(b->sd.seed_join);
    delete b;
    return BWAMS_OK;
}

int bwams_batch_sync(bwams_batch_t *b) {
    if (!b) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipStreamSynchronize(b->stream));
    return BWAMS_OK;
}

int bwams_batch_stats(bwams_batch_t *b, bwams_stats_t *out) {
    if (!b || !out) return BWAMS_ERR_ARG;
    BWAMS_HIP(hipSetDevice(b->idx->device));
    BWAMS_HIP(hipMemcpyAsync(b->h_ctr.p, b->d_ctr.p, sizeof(DevCounters), hipMemcpyDeviceToHost, b->stream));
    BWAMS_HIP(hipStreamSynchronize(b->stream));
    bwams_stats_t s;
    memset(&s, 0, sizeof s);
    const DevCounters &c = *b->h_ctr.p;
    s.n_ext = (int64_t)c.n_ext;
    s.n_ext_blocks = (int64_t)c.n_ext_blocks;
    s.n_sa_lookups = (int64_t)c.n_sa_lookups;
    s.n_lf_steps = (int64_t)c.n_lf_steps;
    s.n_smem[0] = (int64_t)c.valid_after[0];
    s.n_smem[1] = (int64_t)(c.valid_after[1] - c.valid_after[0]);
    s.n_smem[2] = (int64_t)(c.valid_after[2] - c.valid_after[1]);
    s.bsw_cells = (int64_t)c.bsw_cells;
    for (int i = 0; i < 3; ++i) {
        s.n_ext_round[i] = (int64_t)(c.ext_after[i] - (i ? c.ext_after[i - 1] : 0));
        s.n_blk_round[i] = (int64_t)(c.blk_after[i] - (i ? c.blk_after[i - 1] : 0));
    }
    auto el = [&](int a, int bb, float *dst) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, b->ev[a], b->ev[bb]) == hipSuccess) *dst = ms;
    };
    if (has(b, Product::seeds)) {
        el(b->kEvR1Start, b->kEvR1End, &s.ms_smem_r1);
        el(b->kEvR2Start, b->kEvR2End, &s.ms_smem_r2);
        el(b->kEvR3Start, b->kEvR3End, &s.ms_smem_r3);
        el(b->kEvRoundsDone, b->kEvSorted, &s.ms_sort);
        el(b->kEvSorted, b->kEvSeedEnd, &s.ms_sal);
        el(b->kEvSeedStart, b->kEvSeedEnd, &s.ms_seed_total);
    }
    el(b->kEvBswStart, b->kEvBswEnd, &s.ms_bsw);
    el(b->kEvKswStart, b->kEvKswEnd, &s.ms_ksw);
    if (float ms = 0; hipEventElapsedTime(&ms, b->emf.ev[0], b->emf.ev[1]) == hipSuccess) s.ms_emf = ms;
    s.ert_kmer_lookups = (int64_t)c.ert_kmer;
    s.ert_node_reads = (int64_t)c.ert_nodes;
    s.ert_ref_bytes = (int64_t)c.ert_ref;
    s.emf_nodes = (int64_t)b->emf.emf_nodes;
    s.emf_cmp_bytes = (int64_t)b->emf.emf_cmp_bytes;
    stage_state_stats(b, &s);
    (void)hipGetLastError();
    *out = s;
    return BWAMS_OK;
}

}  // extern "C"
