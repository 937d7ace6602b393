// api_process.hip — mem_process_seqs through the public C-ABI (include/bwams.h): the process_* stage sequences, bwams_process_reads*
// and bwams_process_chunk* (FASTQ text or BAM records), and beside them bwams_host_alloc, _free and bwams_batch_device.  The stage state is touched only for an
// empty chunk (process_empty) and for the merged text of bwams_process_chunk_smart.
#include <cstring>

#include "stage_state.h"

using namespace bwams;

extern "C" {
// The outer boundary for one chunk, text to text: what kt_pipeline's step 0 parsing and step 1 (mem_process_seqs, src/bwamem.cpp:1850-1980)
// do between the decompressed FASTQ bytes and seqs[i].sam, as a sequence of the stages' entry points.
// worker_bwt + worker_aln for the chunk the batch holds (reads and names uploaded): EMF, seeding, chaining, extension, de-duplication
static int process_stage1(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo) {
    int rc;
    int64_t t0 = 0, t1 = 0;
    if (emf) {                                            // kernel 0 of mem_kernel1_core: is_pm[], then mem_perfect2reg for the resolved reads
        if ((rc = bwams_emf_run(b, emf))) return rc;
        if ((rc = bwams_emf_regs_run(b, emf, mo, &t0))) return rc;
    }
    if ((rc = ert ? bwams_seed_run_ert(b, ert, so, 1) : bwams_seed_run(b, so, 1))) return rc;
    if ((rc = bwams_chain_run(b, mo, &t0, &t1))) return rc;
    if ((rc = bwams_extend_run(b, mo, &t0))) return rc;
    return bwams_dedup_run(b, mo, &t0);
}

// worker_sam: primary marking / mate rescue + pairing, mem_reg2aln of what is printed, the SAM text.  pes: the chunk's statistics
// (paired-end; mem_pestat runs between the two stages, over the WHOLE chunk: bwamem.cpp:1881-1891).  id_base: n_processed for
// single-end, n_processed >> 1 for paired-end, plus the reads / pairs of the chunk in front of this batch when the chunk is sharded.
static int process_stage2(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_mem_opt_t *mo, const bwams_sam_opt_t *sam_opt,
                          int32_t paired, const bwams_pestat_t *pes, int64_t id_base, int32_t flags, int64_t *sam_bytes) {
    int rc;
    int64_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;
    if (!paired) {
        if ((rc = bwams_pair_run_sam(b, mo, sam_opt, nullptr, id_base, BWAMS_PAIR_SINGLE_END, &t0, &t1))) return rc;
        if ((rc = bwams_reg2aln_run_sam(b, mo, sam_opt, nullptr, &t0, &t1, &t2, &t3))) return rc;
        return emf ? bwams_sam_run_emf(b, mo, sam_opt, emf, sam_bytes) : bwams_sam_run(b, mo, sam_opt, sam_bytes);
    }
    if (emf && (rc = bwams_emf_regs_merge(b, &t0))) return rc;            // worker_sam gives the resolved ends their regions (:1689-1702)
    if ((rc = bwams_pair_run_sam(b, mo, sam_opt, pes, id_base, (flags & BWAMS_PAIR_NO_RESCUE) | (ert ? BWAMS_PAIR_USE_ERT : 0), &t0, &t1))) return rc;
    if ((rc = bwams_reg2aln_run_sam(b, mo, sam_opt, pes, &t0, &t1, &t2, &t3))) return rc;
    return bwams_sam_run_pe(b, mo, sam_opt, pes, sam_bytes);
}

static void process_empty(bwams_batch_t *b, int64_t *sam_bytes) {      // an empty chunk: no reads, no text
    outdated(b, Product::reads, false);                   // the chunk of no reads takes the resident chunk's place
    b->nseq = 0;
    if (StageState *s = b->stages) {
        s->sm.bytes = 0; s->sm.nregs = 0; s->ch.nseq = 0; s->sm.merged_n = -1;
        produced(b, Product::sam);                        // its text, of no bytes, is there to fetch
    }
    if (sam_bytes) *sam_bytes = 0;
}

// mem_process_seqs for the chunk the batch holds
static int process_uploaded(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo,
                            const bwams_sam_opt_t *sam_opt, int32_t paired, const bwams_pestat_t *pes0, int64_t n_processed, int32_t flags,
                            int64_t *sam_bytes) {
    int rc = process_stage1(b, emf, ert, so, mo);
    if (rc) return rc;
    bwams_pestat_t pes[4];
    if (paired) {
        if (pes0) memcpy(pes, pes0, sizeof pes);
        else if ((rc = bwams_pestat(b, mo, pes))) return rc;          // mem_pestat sees the regions of worker_aln only (bwamem.cpp:1881-1891)
    }
    return process_stage2(b, emf, ert, mo, sam_opt, paired, paired ? pes : nullptr, paired ? n_processed >> 1 : n_processed, flags, sam_bytes);
}

// mem_process_seqs for a decoded chunk (fq is closed here): the stage calls in worker order
static int process_decoded(bwams_batch_t *b, bwams_fastq_t *fq, int64_t n, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so,
                           const bwams_mem_opt_t *mo, const bwams_sam_opt_t *sam_opt, int32_t paired, const bwams_pestat_t *pes0,
                           int64_t n_processed, int32_t flags, int64_t *sam_bytes) {
    if (n == 0) {
        bwams_fastq_close(fq);
        process_empty(b, sam_bytes);
        return BWAMS_OK;
    }
    const int rc = bwams_fastq_to_batch_opt(fq, b, (flags & BWAMS_CHUNK_COPY_COMMENT) ? 1 : 0);      // process(): comments only with `mem -C`
    bwams_fastq_close(fq);
    if (rc) return rc;
    return process_uploaded(b, emf, ert, so, mo, sam_opt, paired, pes0, n_processed, flags, sam_bytes);
}

// the reads and their names into the batch: bwams_seed_upload + bwams_sam_upload
static int upload_reads(bwams_batch_t *b, const uint8_t *enc_qdb, const int64_t *cum_len, int64_t n_reads, const char *names,
                        const int64_t *name_off, const char *quals, const char *comments, const int64_t *comment_off) {
    if (int rc = bwams_seed_upload(b, enc_qdb, cum_len, nullptr, (int32_t)n_reads)) return rc;
    return bwams_sam_upload(b, names, name_off, quals, comments, comment_off);
}

// mem_process_seqs for a chunk that arrives the way the reference hands it over — parsed records (bseq1_t: name, comment, seq, qual),
// here as flat arrays: enc_qdb / cum_len as bwams_seed_upload takes them, names / quals / comments as bwams_sam_upload takes them.
int bwams_process_reads(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo,
                        const bwams_sam_opt_t *sam_opt, const uint8_t *enc_qdb, const int64_t *cum_len, int64_t n_reads, const char *names,
                        const int64_t *name_off, const char *quals, const char *comments, const int64_t *comment_off, int32_t paired,
                        const bwams_pestat_t *pes0, int64_t n_processed, int32_t flags, int64_t *sam_bytes) {
    if (!b || !so || !mo || !sam_opt || n_reads < 0 || (n_reads > 0 && (!enc_qdb || !cum_len || !names || !name_off))) {
        set_last_error("bwams_process_reads: batch, options, reads and names are required");
        return BWAMS_ERR_ARG;
    }
    if (paired && (n_reads & 1)) {
        set_last_error("bwams_process_reads: a paired-end chunk holds an even number of reads (ends interleaved)");
        return BWAMS_ERR_ARG;
    }
    if (n_reads == 0) { process_empty(b, sam_bytes); return BWAMS_OK; }
    if (int rc = upload_reads(b, enc_qdb, cum_len, n_reads, names, name_off, quals, comments, comment_off)) return rc;
    return process_uploaded(b, emf, ert, so, mo, sam_opt, paired, pes0, n_processed, flags, sam_bytes);
}

// The same in two halves, for a chunk sharded over several batches (one per GPU): stage 1 up to the regions mem_pestat reads, then —
// after the caller has merged the shards' bwams_pestat_keys with bwams_pestat_from_keys — stage 2 with the chunk's statistics and this
// shard's first read / pair id.  bwams_process_reads == _stage1 + bwams_pestat + _stage2 on one batch.
int bwams_process_reads_stage1(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo,
                               const uint8_t *enc_qdb, const int64_t *cum_len, int64_t n_reads, const char *names, const int64_t *name_off,
                               const char *quals, const char *comments, const int64_t *comment_off) {
    if (!b || !so || !mo || n_reads < 0 || (n_reads > 0 && (!enc_qdb || !cum_len || !names || !name_off))) {
        set_last_error("bwams_process_reads_stage1: batch, options, reads and names are required");
        return BWAMS_ERR_ARG;
    }
    if (n_reads == 0) { process_empty(b, nullptr); return BWAMS_OK; }
    if (int rc = upload_reads(b, enc_qdb, cum_len, n_reads, names, name_off, quals, comments, comment_off)) return rc;
    return process_stage1(b, emf, ert, so, mo);
}

// Stage 1 itself in two halves, so that a pipeline can put the next chunk's reads and names into one batch (PCIe) while another batch
// of the same device computes: _upload = bwams_seed_upload + bwams_sam_upload, _stage1_run = worker_bwt + worker_aln on what it left.
int bwams_process_reads_upload(bwams_batch_t *b, const uint8_t *enc_qdb, const int64_t *cum_len, int64_t n_reads, const char *names,
                               const int64_t *name_off, const char *quals, const char *comments, const int64_t *comment_off) {
    if (!b || n_reads < 0 || (n_reads > 0 && (!enc_qdb || !cum_len || !names || !name_off))) {
        set_last_error("bwams_process_reads_upload: batch, reads and names are required");
        return BWAMS_ERR_ARG;
    }
    if (n_reads == 0) { process_empty(b, nullptr); return BWAMS_OK; }
    return upload_reads(b, enc_qdb, cum_len, n_reads, names, name_off, quals, comments, comment_off);
}

int bwams_process_reads_stage1_run(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo) {
    if (!b || !so || !mo) {
        set_last_error("bwams_process_reads_stage1_run: batch and options are required");
        return BWAMS_ERR_ARG;
    }
    if (b->nseq == 0) return BWAMS_OK;
    return process_stage1(b, emf, ert, so, mo);
}

int bwams_batch_device(const bwams_batch_t *b, int32_t *device) {
    if (!b || !b->idx || !device) return BWAMS_ERR_ARG;
    *device = b->idx->device;
    return BWAMS_OK;
}

int bwams_process_reads_stage2(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_mem_opt_t *mo, const bwams_sam_opt_t *sam_opt,
                               int32_t paired, const bwams_pestat_t *pes, int64_t id_base, int32_t flags, int64_t *sam_bytes) {
    if (!b || !mo || !sam_opt || (paired && !pes)) {
        set_last_error("bwams_process_reads_stage2: batch, options and (paired-end) the chunk's statistics are required");
        return BWAMS_ERR_ARG;
    }
    if (b->nseq == 0) { process_empty(b, sam_bytes); return BWAMS_OK; }
    return process_stage2(b, emf, ert, mo, sam_opt, paired, pes, id_base, flags, sam_bytes);
}

// Page-locked host memory for the buffers that cross PCIe every chunk (reads and names up, SAM text down): the copies of
// bwams_seed_upload / bwams_sam_upload / bwams_sam_fetch then run at the link's rate instead of through a pageable bounce buffer.
int bwams_host_alloc(size_t bytes, void **out) {
    if (!out) return BWAMS_ERR_ARG;
    *out = nullptr;
    BWAMS_HIP(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return BWAMS_OK;
}
int bwams_host_free(void *p) {
    if (p) BWAMS_HIP(hipHostFree(p));
    return BWAMS_OK;
}

// bwams_process_chunk behind its decode (fq is closed here): `who` names the entry point in the error text
static int chunk_decoded(const char *who, bwams_batch_t *b, bwams_fastq_t *fq, int64_t n, bwams_emf_t *emf, bwams_ert_t *ert,
                         const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo, const bwams_sam_opt_t *sam_opt, int32_t paired,
                         const bwams_pestat_t *pes0, int64_t n_processed, int32_t flags, int64_t *n_reads, int64_t *sam_bytes) {
    if (paired && (n & 1)) {
        bwams_fastq_close(fq);
        set_last_error(std::string(who) + ": a paired-end chunk holds an even number of reads (ends interleaved)");
        return BWAMS_ERR_ARG;
    }
    const int rc = process_decoded(b, fq, n, emf, ert, so, mo, sam_opt, paired, pes0, n_processed, flags, sam_bytes);
    if (!rc && n_reads) *n_reads = n;
    return rc;
}

int bwams_process_chunk(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo,
                        const bwams_sam_opt_t *sam_opt, const char *fastq, int64_t n_bytes, int32_t paired, const bwams_pestat_t *pes0,
                        int64_t n_processed, int32_t flags, int64_t *n_reads, int64_t *sam_bytes) {
    if (!b || !so || !mo || !sam_opt || !fastq || n_bytes < 0) {
        set_last_error("bwams_process_chunk: batch, options and text are required");
        return BWAMS_ERR_ARG;
    }
    bwams_fastq_t *fq = nullptr;
    int64_t n = 0, nb = 0;
    int rc = bwams_fastq_decode(b->idx->device, fastq, n_bytes, &fq, &n, &nb);
    if (rc) return rc;
    return chunk_decoded("bwams_process_chunk", b, fq, n, emf, ert, so, mo, sam_opt, paired, pes0, n_processed, flags, n_reads, sam_bytes);
}

// The same chunk already decoded (and perhaps trimmed: api_trim.hip) by the caller
int bwams_process_chunk_decoded(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo,
                                const bwams_sam_opt_t *sam_opt, bwams_fastq_t *fq, int32_t paired, const bwams_pestat_t *pes0,
                                int64_t n_processed, int32_t flags, int64_t *n_reads, int64_t *sam_bytes) {
    if (!b || !so || !mo || !sam_opt || !fq || (paired != 0 && paired != 1) || fq->device != b->idx->device) {
        bwams_fastq_close(fq);
        set_last_error("bwams_process_chunk_decoded: batch, options and a chunk decoded on the batch's device are required; paired is 0 or 1");
        return BWAMS_ERR_ARG;
    }
    return chunk_decoded("bwams_process_chunk_decoded", b, fq, fq->n_reads, emf, ert, so, mo, sam_opt, paired, pes0, n_processed, flags, n_reads,
                         sam_bytes);
}

// The same chunk given as BAM records (bam_reads.hip decodes them to the same handle)
int bwams_process_chunk_bam(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo,
                            const bwams_sam_opt_t *sam_opt, const void *bam, int64_t n_bytes, const char *tags, int32_t paired,
                            const bwams_pestat_t *pes0, int64_t n_processed, int32_t flags, int64_t *n_reads, int64_t *sam_bytes) {
    if (!b || !so || !mo || !sam_opt || !bam || n_bytes < 0) {
        set_last_error("bwams_process_chunk_bam: batch, options and records are required");
        return BWAMS_ERR_ARG;
    }
    bwams_fastq_t *fq = nullptr;
    int64_t n = 0, nb = 0;
    int rc = bwams_bam_reads_decode(b->idx->device, bam, n_bytes, tags, &fq, &n, &nb, nullptr);
    if (rc) return rc;
    return chunk_decoded("bwams_process_chunk_bam", b, fq, n, emf, ert, so, mo, sam_opt, paired, pes0, n_processed, flags, n_reads, sam_bytes);
}

// A paired-end chunk read from two files (bseq_read_orig with ks2, src/bwa.cpp:275-318): record k of the first text and record k of the
// second are the ends of pair k.
int bwams_process_chunk2(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo,
                         const bwams_sam_opt_t *sam_opt, const char *fastq1, int64_t n_bytes1, const char *fastq2, int64_t n_bytes2,
                         const bwams_pestat_t *pes0, int64_t n_processed, int32_t flags, int64_t *n_reads, int64_t *sam_bytes) {
    if (!b || !so || !mo || !sam_opt || !fastq1 || !fastq2 || n_bytes1 < 0 || n_bytes2 < 0) {
        set_last_error("bwams_process_chunk2: batch, options and the two texts are required");
        return BWAMS_ERR_ARG;
    }
    bwams_fastq_t *f1 = nullptr, *f2 = nullptr, *fq = nullptr;
    int64_t n1 = 0, n2 = 0, nb = 0;
    int rc = bwams_fastq_decode(b->idx->device, fastq1, n_bytes1, &f1, &n1, &nb);
    if (rc) return rc;
    if ((rc = bwams_fastq_decode(b->idx->device, fastq2, n_bytes2, &f2, &n2, &nb))) { bwams_fastq_close(f1); return rc; }
    if (n1 != n2 || bwams_fastq_has_qual(f1) != bwams_fastq_has_qual(f2)) {
        bwams_fastq_close(f1); bwams_fastq_close(f2);
        set_last_error("bwams_process_chunk2: the two texts must hold the same number of records of one kind (" + std::to_string(n1) + " and " +
                       std::to_string(n2) + "): cut both files at the same record");
        return BWAMS_ERR_ARG;
    }
    rc = fastq_interleave(f1, f2, &fq);
    bwams_fastq_close(f1); bwams_fastq_close(f2);
    if (rc) return rc;
    rc = process_decoded(b, fq, 2 * n1, emf, ert, so, mo, sam_opt, 1, pes0, n_processed, flags, sam_bytes);
    if (!rc && n_reads) *n_reads = 2 * n1;
    return rc;
}

// process()'s MEM_F_SMARTPE branch (src/fastmap.cpp:378-414): bseq_classify splits the chunk into the reads that stand alone and the
// interleaved pairs; mem_process_seqs runs on the first set as single-end (ids from n_processed) and on the second as paired-end (ids
// from n_processed + the number of single reads, pes0); every read's text returns to its place in the chunk.  Behind the decode
// (fq is closed here), shared by the text and the BAM entry points.
static int chunk_smart_decoded(bwams_batch_t *b, bwams_fastq_t *fq, int64_t n, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so,
                               const bwams_mem_opt_t *mo, const bwams_sam_opt_t *sam_opt, const bwams_pestat_t *pes0, int64_t n_processed,
                               int32_t flags, int64_t *n_reads, int64_t *n_single, int64_t *sam_bytes) {
    int rc;
    std::vector<uint8_t> which;
    if ((rc = fastq_classify(fq, &which))) { bwams_fastq_close(fq); return rc; }
    std::vector<int64_t> ids[2];
    for (int64_t i = 0; i < n; ++i) ids[which[(size_t)i]].push_back(i);
    DevBuf<char> held[2];                                // the text of each run, kept while the batch does the other,
    std::vector<int64_t> held_off[2];                    // and where its reads start
    hipStream_t st = b->stream;
    for (int k = 0; k < 2; ++k) {
        held_off[k].assign(ids[k].size() + 1, 0);
        if (ids[k].empty()) continue;
        bwams_fastq_t *sub = nullptr;
        if ((rc = fastq_subset(fq, ids[k], &sub))) { bwams_fastq_close(fq); return rc; }
        int64_t bytes = 0;
        rc = process_decoded(b, sub, (int64_t)ids[k].size(), emf, ert, so, mo, sam_opt, k, k ? pes0 : nullptr,
                             n_processed + (k ? (int64_t)ids[0].size() : 0), flags, &bytes);
        if (rc) { bwams_fastq_close(fq); return rc; }
        StageState *s = b->stages;
        hipError_t e = held[k].alloc((size_t)bytes + 16);
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(held[k].p, s->sm.out.p, (size_t)bytes, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(held_off[k].data(), s->sm.off.p, held_off[k].size() * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { bwams_fastq_close(fq); BWAMS_HIP(e); }
    }
    bwams_fastq_close(fq);
    if (n_reads) *n_reads = n;
    if (n_single) *n_single = (int64_t)ids[0].size();
    StageState *s;
    if ((rc = get_state(b, &s))) return rc;
    outdated(b, Product::sam);                            // the last run's text makes way for the whole chunk's
    // every read's block back to its place in the chunk (ret->seqs[sep[k][i].id].sam = sep[k][i].sam)
    std::vector<int64_t> off((size_t)n + 1, 0);
    std::vector<int64_t> rank((size_t)n, 0);
    for (int k = 0; k < 2; ++k)
        for (size_t j = 0; j < ids[k].size(); ++j) rank[(size_t)ids[k][j]] = (int64_t)j;
    for (int64_t i = 0; i < n; ++i) {
        const std::vector<int64_t> &h = held_off[which[(size_t)i]];
        const size_t j = (size_t)rank[(size_t)i];
        off[(size_t)i + 1] = off[(size_t)i] + (h[j + 1] - h[j]);
    }
    const int64_t total = off[(size_t)n];
    BWAMS_HIP(s->sm.out.ensure_n((size_t)total + 16)); BWAMS_HIP(s->sm.off.ensure_n((size_t)(n + 1)));
    std::vector<SegMove> mv;
    mv.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int k = which[(size_t)i];
        const size_t j = (size_t)rank[(size_t)i];
        mv.push_back({held[k].p + held_off[k][j], s->sm.out.p + off[(size_t)i], held_off[k][j + 1] - held_off[k][j]});
    }
    if ((rc = segment_copy(mv, st))) return rc;
    BWAMS_HIP(hipMemcpyAsync(s->sm.off.p, off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    BWAMS_HIP(hipStreamSynchronize(st));
    s->sm.bytes = total; s->sm.nregs = 0; s->sm.merged_n = n;
    if (sam_bytes) *sam_bytes = total;
    produced(b, Product::sam);
    return BWAMS_OK;
}

int bwams_process_chunk_smart(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo,
                              const bwams_sam_opt_t *sam_opt, const char *fastq, int64_t n_bytes, const bwams_pestat_t *pes0,
                              int64_t n_processed, int32_t flags, int64_t *n_reads, int64_t *n_single, int64_t *sam_bytes) {
    if (!b || !so || !mo || !sam_opt || !fastq || n_bytes < 0) {
        set_last_error("bwams_process_chunk_smart: batch, options and text are required");
        return BWAMS_ERR_ARG;
    }
    bwams_fastq_t *fq = nullptr;
    int64_t n = 0, nb = 0;
    int rc = bwams_fastq_decode(b->idx->device, fastq, n_bytes, &fq, &n, &nb);
    if (rc) return rc;
    return chunk_smart_decoded(b, fq, n, emf, ert, so, mo, sam_opt, pes0, n_processed, flags, n_reads, n_single, sam_bytes);
}

int bwams_process_chunk_bam_smart(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo,
                                  const bwams_sam_opt_t *sam_opt, const void *bam, int64_t n_bytes, const char *tags,
                                  const bwams_pestat_t *pes0, int64_t n_processed, int32_t flags, int64_t *n_reads, int64_t *n_single,
                                  int64_t *sam_bytes) {
    if (!b || !so || !mo || !sam_opt || !bam || n_bytes < 0) {
        set_last_error("bwams_process_chunk_bam_smart: batch, options and records are required");
        return BWAMS_ERR_ARG;
    }
    bwams_fastq_t *fq = nullptr;
    int64_t n = 0, nb = 0;
    int rc = bwams_bam_reads_decode(b->idx->device, bam, n_bytes, tags, &fq, &n, &nb, nullptr);
    if (rc) return rc;
    return chunk_smart_decoded(b, fq, n, emf, ert, so, mo, sam_opt, pes0, n_processed, flags, n_reads, n_single, sam_bytes);
}
}  // extern "C"
