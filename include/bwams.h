/*
 * bwams.h — C-ABI of the MI355X-native BWA-MEM seed-and-extend hot path.
 *
 * Plain pointers and sizes only; no C++ or torch types.  Each entry point names
 * the reference interface it replaces (file:line under /root/reference) — these
 * are exactly the call sites a reference maintainer re-binds.
 *
 * Conventions
 *   - every function returns 0 (BWAMS_OK) or a negative error code; the library
 *     never exits the process and never falls back to a CPU path.  A missing or
 *     unusable GPU is BWAMS_ERR_DEVICE.
 *   - the caller owns all host buffers; the library owns device memory.
 *   - output order is input order (SMEMs sorted by (rid, m, n) as
 *     mem_collect_smem leaves them; extension results written back in place).
 *   - a handle is bound to one GPU and one HIP stream; calls on one handle are
 *     serialised by the caller (the reference has one mem_process_seqs call in
 *     flight per pipeline slot, src/fastmap.cpp:475-491).  Use one handle per
 *     host thread / per GPU.
 */
#ifndef BWAMS_H
#define BWAMS_H

#include <stddef.h>
#include <stdint.h>
#include "bwams_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BWAMS_OK               0
#define BWAMS_ERR_DEVICE      -1   /* no usable gfx950 device / HIP runtime error */
#define BWAMS_ERR_IO          -2   /* index file missing or malformed */
#define BWAMS_ERR_ARG         -3   /* invalid argument */
#define BWAMS_ERR_CAPACITY    -4   /* an output buffer is too small; *n_* holds the need */
#define BWAMS_ERR_NOMEM       -5
#define BWAMS_ERR_UNSUPPORTED -6

typedef struct bwams_index bwams_index_t;   /* FM-index resident in one GPU's HBM */
typedef struct bwams_batch bwams_batch_t;   /* stream + device work buffers for one chunk of reads */
typedef struct bwams_emf bwams_emf_t;       /* exact-match filter table resident in HBM */

const char *bwams_strerror(int code);
/* Text of the last HIP / IO error on this thread. */
const char *bwams_last_error(void);
/* Debugging aids and A-B switches (environment; all result-neutral; read ONCE at the first call into the library, and again by
 * bwams_debug_reload(), which a test calls after changing one):
 *   BWAMS_VERBOSE=1 stage times / counters on stderr    BWAMS_POISON=1 fresh device allocations filled with 0xAB
 *   BWAMS_BWD_MIN_LIST / _COLS / _LATE_LIST, BWAMS_BWD_DRY_MIN_LIST / _DRY_COLS / _DRY_LATE_LIST  when a backward phase of the SMEM search
 *     leaves its lane (entries at the forward end; columns run and entries alive; the same once the read queue is dry; MIN_LIST=0: never)
 *   BWAMS_SEED_R3_BESIDE=0 (SMEM round 3 behind round 2 instead of beside it), BWAMS_DEBUG (SMEM search ablations)
 *   BWAMS_EXT_MAX_ROUNDS, BWAMS_EXT_ALL_ROUNDS, BWAMS_EXT_INPLACE=0, BWAMS_BSW_PK=0, BWAMS_CHAIN_BATCH=0   extension rounds and kernel variants
 *   BWAMS_DEDUP_SEQ=1, BWAMS_PAIR_DROP_PLAN, BWAMS_TRACE_PAIR   fallback paths forced by tests (tests/test_gpu_dedup_limits.py runs its batches under
 *     BWAMS_DEDUP_SEQ=1 as well); a line per launch of the paired-end tail
 *   BWAMS_DEDUP_COUNT=1   bwams_dedup_run counts its reads per tier and its patch alignments per variant (bwams_debug_dedup_counts)
 *   BWAMS_PAIR_COUNT=1   bwams_pair_run counts its reads per route and its sorts per path (bwams_debug_pair_counts)
 *   BWAMS_CHAIN_COUNT=1   bwams_chain_run / _run_ert count their reads per filter route and the passes of the wave tier (bwams_debug_chain_counts)
 *   BWAMS_DEPTH_COMBINE=0   the depth add issues one atomic per lane instead of folding equal slots inside a wave (tools/depth_rate.py)
 *   BWAMS_PILEUP_TILED=0    every record of a pileup add goes through the direct kernel, one global atomic per base (tools/pileup_rate.py)
 *   BWAMS_QC_LANES=0        the QC add's per-cycle tables come from the plain kernel, one global atomic per base and per quality (tools/qc_rate.py)
 *   BWAMS_RECAL_LDS=0       the recalibration add counts through the plain kernel, one global atomic per update (tools/recal_rate.py)
 *   BWAMS_ERT_GRID, BWAMS_ERT_FAT=0, BWAMS_ERT_TICKET=0   ERT walk launch shape        BWAMS_HOST_THREADS   host threads of mem_process_seqs' staging (6)
 *   BWAMS_SA_DENSE=0 / 1 / 2 / 4   stride of the dense suffix-array table an index derives at its first FM-index seeding with coordinates
 *     (8 bytes for every stride-th row; the lookup then takes at most stride - 1 LF steps of its own); 0: never built, never read
 *   BWAMS_SA_DENSE_MAX_BYTES   a table above it is not built and the index keeps the walk (default: no cap)
 *   BWAMS_SORT_NARROW=0   the SMEM sort keys keep 16-bit position fields whatever the batch's longest read */
int bwams_debug_reload(void);
int bwams_device_count(int *n);

/* ---------------------------------------------------------------- index ---- */

/* Host-side description of an FM-index, as FMI_search holds it after
 * load_index (src/FMI_search.cpp:1251-1370): count[] already has the +1. */
typedef struct bwams_fmi_desc {
    int64_t ref_seq_len;               /* 2*l_pac + 1 */
    int64_t count[5];
    const bwams_cp_occ_t *cp_occ;      /* (ref_seq_len >> 6) + 1 blocks */
    const int8_t  *sa_ms_byte;         /* (ref_seq_len >> 3) + 1 */
    const uint32_t *sa_ls_word;        /* (ref_seq_len >> 3) + 1 */
    int64_t sentinel_index;
    const uint8_t *ref_0123;           /* 2*l_pac bytes or NULL (load_ref_string, src/fastmap.cpp:813) */
} bwams_fmi_desc_t;

/* Replaces FMI_search::load_index (src/FMI_search.cpp:1251) + load_ref_string
 * (src/fastmap.cpp:813): reads <prefix>.bwt.2bit.64 (and <prefix>.0123 when
 * present) and uploads them to GPU `device`. */
int bwams_index_open(const char *prefix, int device, bwams_index_t **out);

/* Same, from arrays already in host memory (e.g. the reference's own loaded
 * FMI_search members or its /dev/shm segments, src/bwa_shm.cpp). */
int bwams_index_from_host(const bwams_fmi_desc_t *desc, int device, bwams_index_t **out);

/* Same, adopting arrays that already live in this GPU's memory (not copied, not
 * freed by close).  Lets an on-device index builder hand over without PCIe. */
int bwams_index_from_device(const bwams_fmi_desc_t *desc_with_device_pointers, int device,
                            bwams_index_t **out);

/* FMA direct-lookup tables (all_smem_t / last_smem_t, src/FMI_search.h:101-135; used at
 * src/FMI_search.cpp:1414-1463 and :1705-1750).  build = `bwa-mem2.scale smem-table` on the GPU
 * (one lane per table entry); set = upload tables read from <prefix>.all_smem.11 / .last_smem.13
 * (NULL, NULL detaches them); fetch = download (to write those files).  The reference's depths
 * are all_bp = 11 and last_bp = 13; smaller depths are accepted for testing.  bwams_index_open
 * loads the two files when they exist next to the index. */
int bwams_index_build_fma(bwams_index_t *idx, int all_bp, int last_bp);
int bwams_index_set_fma(bwams_index_t *idx, const void *all_smem, int all_bp, const void *last_smem, int last_bp);
int bwams_index_fetch_fma(bwams_index_t *idx, void *all_smem, void *last_smem);

/* FM-index construction on the GPU.  Replaces `bwa-mem2.scale index`'s FMI_search::build_index +
 * build_fm_index (src/FMI_search.cpp:774-849, :611-771; driver src/main.cpp -> bwa_index, src/bwtindex.cpp):
 * text = fw || revcomp(fw), suffix array (prefix doubling on the device instead of host SA-IS), BWT,
 * CP_OCC, SA samples.  The arrays equal the reference's byte for byte (they are functions of the suffix
 * array).  fw: l_pac base codes 0..3, one per byte (N already replaced, as bns_fasta2bntseq does), in host
 * memory or — fw_on_device != 0 — in this GPU's memory.  Texts up to 2^36 rows (GRCh38: 6.4 G rows, ~150 GB
 * of HBM while building).  chunk_rows bounds the rows sorted at once (0 = 2^30).  stats may be NULL. */
typedef struct bwams_build_stats {
    int64_t rows;                      /* 2*l_pac + 1 */
    int32_t chunks, rounds;            /* key-space chunks of the first pass; doubling rounds after it */
    int64_t unresolved_after_first;    /* rows still tied after the 29-base pass */
    float ms_first_pass, ms_outputs;   /* device time of the first pass / of BWT + CP_OCC + SA samples */
} bwams_build_stats_t;
int bwams_index_build(const uint8_t *fw, int64_t l_pac, int fw_on_device, int device, int keep_ref,
                      int64_t chunk_rows, bwams_build_stats_t *stats, bwams_index_t **out);
/* The resident arrays back to the host (any pointer may be NULL), e.g. to write the reference's files
 * or to hand them to a CPU reader.  desc receives the scalars (count[] with the loader's +1). */
int bwams_index_fetch(bwams_index_t *idx, bwams_cp_occ_t *cp_occ, int8_t *sa_ms_byte, uint32_t *sa_ls_word,
                      uint8_t *ref_0123, bwams_fmi_desc_t *desc);
/* Writes <prefix>.bwt.2bit.64 (and <prefix>.0123 when the index holds the text) in the reference's format
 * (src/FMI_search.cpp:629-763, :796-829), streaming from HBM; on a handle from bwams_index_from_fasta also <prefix>.ann, .amb
 * and .pac (bns_dump and bns_fasta2bntseq's .pac, src/bntseq.cpp:83-112, :356-366). */
int bwams_index_save(bwams_index_t *idx, const char *prefix);

/* Indexing a reference FASTA on the GPU.  Replaces bns_fasta2bntseq (src/bntseq.cpp:269-372) + FMI_search::build_index as
 * bwa_idx_build_mem2 chains them (src/bwtindex.cpp:377-394): the text (plain FASTA, in host memory or — text_on_device != 0 — in
 * this GPU's memory) is parsed as kseq_read parses it, every base code >= 4 becomes lrand48() & 3 after srand48(11) in global base
 * order, and the 2-bit codes go to bwams_index_build's builder without leaving HBM.  The handle carries its sequences as
 * bwams_index_set_contigs / _set_contig_names / _set_contig_annos would set them (annotations as bns_restore reads them back), and
 * the .ann / .amb / .pac content, which bwams_index_save then writes besides .bwt.2bit.64 and .0123 — byte for byte what
 * `bwa-mem2.scale index` writes.  Refused: a line starting with '+' (FASTQ) and a sequence over INT32_MAX bases
 * (BWAMS_ERR_UNSUPPORTED); text without a '>' / '@' header or without bases (BWAMS_ERR_ARG).  No handle is left on an error. */
typedef struct bwams_fasta_stats {
    int64_t l_pac;                     /* bases of the forward strand */
    int32_t n_seqs, n_holes;           /* sequences; runs of one ambiguous byte (the .amb records) */
    int64_t n_ambig_bases;             /* bases with an nst_nt4_table code >= 4 (each took one lrand48 draw) */
    float ms_host_read;                /* file read and inflate (bwams_index_from_fasta_file; 0 otherwise) */
    float ms_upload;                   /* host text to HBM (0 when the text was already on the device) */
    float ms_device_pack;              /* text in HBM -> codes, .pac and holes, headers to the host */
    float ms_fm_build;                 /* the FM-index build from the codes */
    bwams_build_stats_t build;
} bwams_fasta_stats_t;
int bwams_index_from_fasta(int device, const char *text, int64_t n_bytes, int text_on_device, int keep_ref, int64_t chunk_rows,
                           bwams_fasta_stats_t *stats, bwams_index_t **out);
/* The same from a plain or gzip file (zlib, inflated into page-locked memory). */
int bwams_index_from_fasta_file(const char *path, int device, int keep_ref, int64_t chunk_rows, bwams_fasta_stats_t *stats,
                                bwams_index_t **out);
/* BGZF (blocked gzip, SAMv1 §4.1: what bgzip writes) inflated on the GPU — replaces gzread() for such input.  The host walks the
 * member headers (BSIZE, CRC32, ISIZE); each member is inflated (RFC 1951: stored, fixed and dynamic blocks, with zlib's checks of
 * the codes) by one wave, and its CRC32 and ISIZE are checked, always.  max_in_bytes / max_out_bytes (each >= 65536): the compressed
 * bytes and the host-output bytes one call takes at most.  The handle is bound to `device`; one caller at a time. */
typedef struct bwams_inflater bwams_inflater_t;
typedef struct bwams_inflate_stats {
    int64_t members, in_bytes, out_bytes;
    float ms_upload, ms_kernel, ms_download;     /* device events */
} bwams_inflate_stats_t;
int bwams_inflater_create(int device, int64_t max_in_bytes, int64_t max_out_bytes, bwams_inflater_t **out);
/* Inflates the whole BGZF members at the front of gz[0, n_bytes) into out (host memory, or this device's memory when out_on_device)
 * in file order. It stops at a member cut off by the end of the buffer and at the first member that would not fit out_cap (or
 * max_in_bytes / max_out_bytes). *n_consumed / *n_out say how far it got (0 / 0: give it more bytes). BWAMS_ERR_UNSUPPORTED: not
 * BGZF (a later member that is not BGZF ends the call in front of it). BWAMS_ERR_CAPACITY: the first member does not fit.
 * BWAMS_ERR_IO: damaged data; bwams_last_error names the member (index and byte offset, counted over every call on this handle),
 * nothing is consumed, and out is written only in the ranges of the members that checked out. */
int bwams_inflater_run(bwams_inflater_t *f, const uint8_t *gz, int64_t n_bytes, void *out, int64_t out_cap, int out_on_device,
                       int64_t *n_consumed, int64_t *n_out, bwams_inflate_stats_t *stats);
int bwams_inflater_destroy(bwams_inflater_t *f);
/* Plain gzip (RFC 1952: one DEFLATE stream, or a few members, with no table of member sizes — what `gzip` writes) inflated on the GPU
 * (csrc/gunzip.hip).  The compressed bytes of a call are cut into pieces of piece_bytes (>= 4096; 0: 256 KiB); a block start is
 * searched in each piece, every piece is decoded at once with the unknown 32 KiB in front of it as markers, and the markers are
 * resolved afterwards.  The candidates are hints: a piece is used only when its predecessor's decode ended exactly on its start, so the
 * output is a sequential decoder's on any input.  max_in_bytes (>= piece_bytes) / max_out_bytes (>= 65536): the compressed bytes one
 * call looks at and the text bytes one call produces at most.  BGZF is gzip: this handle inflates it too.  One caller at a time. */
typedef struct bwams_gunzip bwams_gunzip_t;
typedef struct bwams_gunzip_stats {
    int64_t members, pieces, pieces_dropped, recounts, in_bytes, out_bytes, trailing_bytes;   /* members: those that ended in this call */
    float ms_upload, ms_find, ms_count, ms_decode, ms_window, ms_resolve, ms_download;        /* device events */
} bwams_gunzip_stats_t;
int bwams_gunzip_create(int device, int64_t max_in_bytes, int64_t max_out_bytes, int32_t piece_bytes, bwams_gunzip_t **out);
/* A handle is fed one file in order, in calls of any size; it keeps where in the stream it is (a header, DEFLATE data at bit 0-7 of
 * the first unconsumed byte, a trailer), the 32 KiB window (on the device) and the current member's CRC32 and length.  A call inflates
 * gz[0, n_bytes) into out (host memory, or this device's memory when out_on_device) up to the last block boundary of the confirmed
 * chain of pieces whose output fits out_cap and max_out_bytes.  *n_consumed counts whole bytes: the caller presents the rest again,
 * followed by more; `last` = 1 says that no bytes follow.  0 with 0 / 0: give it more bytes.  BWAMS_ERR_UNSUPPORTED: the first bytes
 * are no gzip header.  BWAMS_ERR_CAPACITY: not even the first piece's output fits, or no block boundary lies inside max_in_bytes.
 * BWAMS_ERR_IO: damaged data (a refused code, a distance too far back, CRC32 or ISIZE that do not match, a bad member header), or a
 * stream that ends inside a member when `last` is set; bwams_last_error names the member and the byte offset, counted over all
 * calls, and nothing of that call is consumed.  Bytes behind a member that are no gzip header are ignored, as gzread ignores them,
 * and counted in trailing_bytes. */
int bwams_gunzip_run(bwams_gunzip_t *g, const uint8_t *gz, int64_t n_bytes, int32_t last, void *out, int64_t out_cap,
                     int out_on_device, int64_t *n_consumed, int64_t *n_out, bwams_gunzip_stats_t *stats);
int bwams_gunzip_destroy(bwams_gunzip_t *g);
/* BGZF written on the GPU: the output side's counterpart of the inflater.  The text is cut every 65280 bytes from its byte 0 (bgzip's
 * and htslib's cut; the last member is partial) and each piece becomes one standalone gzip member with bgzip's header: one RFC 1951
 * block, stored, fixed or dynamic Huffman, whichever has the fewest bits (input that does not compress is stored: its length + 31
 * bytes), LZ77 matches inside the member only, CRC32 and ISIZE computed on the device.  Members come out contiguous and in input order,
 * and their bytes depend only on the input bytes (not on max_in_bytes, the number of launches or where input and output lie).
 * max_in_bytes (>= 65280): the input one launch takes; larger input runs in several launches with the same output.  The handle is
 * bound to `device`; one caller at a time. */
typedef struct bwams_deflater bwams_deflater_t;
typedef struct bwams_deflate_stats {
    int64_t members, in_bytes, out_bytes;
    float ms_upload, ms_kernel, ms_download;     /* device events */
} bwams_deflate_stats_t;
#define BWAMS_DEFLATE_EOF 0x1                    /* append the 28-byte BGZF EOF member */
int64_t bwams_deflate_bound(int64_t n_bytes);    /* n + 31 * ceil(n / 65280) + 28: the most bwams_deflater_run can write */
int bwams_deflater_create(int device, int64_t max_in_bytes, bwams_deflater_t **out);
/* Compresses all of in[0, n_bytes) (host memory, or this device's memory when in_on_device) into out (host, or this device's memory
 * when out_on_device); *n_out: the bytes written.  Members never span two calls, so the outputs of consecutive calls concatenate into one
 * BGZF stream.  n_bytes = 0 writes nothing (or only the EOF member).  BWAMS_ERR_CAPACITY, with nothing written and *n_out = the bound:
 * out_cap < bwams_deflate_bound(n_bytes).  BWAMS_ERR_ARG: a null handle, in or out, or unknown flags. */
int bwams_deflater_run(bwams_deflater_t *d, const void *in, int64_t n_bytes, int in_on_device, void *out, int64_t out_cap,
                       int out_on_device, int32_t flags, int64_t *n_out, bwams_deflate_stats_t *stats);
int bwams_deflater_destroy(bwams_deflater_t *d);
/* bns_restore (src/bntseq.cpp:114-246) onto a handle, e.g. one from bwams_index_open: reads <prefix>.ann, checks the .amb header
 * against it (a mismatched pair is BWAMS_ERR_IO), reads <prefix>.alt when present, and sets the sequences (with is_alt), their
 * names and annotations.  The .ann must describe the index's l_pac (BWAMS_ERR_ARG otherwise). */
int bwams_index_load_bns(bwams_index_t *idx, const char *prefix);

int bwams_index_close(bwams_index_t *idx);
/* Device bytes of the index's own arrays.  What it derives at its first seeding is not counted here: the same index reports the
 * same number before and after (the dense suffix-array table's bytes: bwams_debug_sa_dense_state below). */
int64_t bwams_index_bytes(const bwams_index_t *idx);

/* The dense suffix-array table of an index: a cache derived from the index at its first bwams_seed_run with coordinates
 * (BWAMS_SA_DENSE, BWAMS_SA_DENSE_MAX_BYTES above), one 64-bit entry for every row r with r % stride == 0: bits 0-39 the
 * coordinate the reference's walk from r produces, bit 40 set when that walk meets the sentinel row (the lookup yields 0), bits
 * 41-63 the LF steps of the walk.  When ANY device allocation of the library runs out of memory, the tables of the indexes on
 * that device are released and the allocation is tried once more; a released index walks for the rest of its life.  Results and
 * counters are the same in every state. */
enum { BWAMS_SA_DENSE_ABSENT = 0,     /* not built (yet, or BWAMS_SA_DENSE=0) */
       BWAMS_SA_DENSE_BUILT = 1,
       BWAMS_SA_DENSE_REFUSED = 2,    /* above the cap, no room for it, or a walk too long for the step field: the index walks */
       BWAMS_SA_DENSE_YIELDED = 3 };  /* released to make room: the index walks */
/* Test hooks (not part of the drop-in surface).  _state: the state above, the stride (0 before a build was tried), the table's
 * bytes while it is resident, the build kernel's time; any pointer may be null.  _fetch: *n = the table's entries, copied to out
 * when out is given (cap entries; BWAMS_ERR_CAPACITY when too few); BWAMS_ERR_ARG unless the state is BUILT.  _release: the routine
 * the allocator calls on out-of-memory, for `device`; *n_released = tables released. */
int bwams_debug_sa_dense_state(bwams_index_t *idx, int32_t *state, int32_t *stride, int64_t *bytes, float *build_ms);
int bwams_debug_sa_dense_fetch(bwams_index_t *idx, uint64_t *out, int64_t cap, int64_t *n);
int bwams_debug_sa_dense_release(int device, int32_t *n_released);

/* ---------------------------------------------------------------- batch ---- */

/* Work buffers sized for up to max_reads reads / max_bases bases per call.
 * max_smem / max_sa are the initial sizes of the SMEM and SA-coordinate buffers (0 = library
 * default: 24 SMEMs and 64 coordinates per read on average).  They are not limits: a chunk that
 * needs more makes the stage run a second time on grown buffers (the kernels keep counting when
 * a buffer is full).  The host buffers of bwams_seed_fmi / bwams_seed_fetch are the caller's and
 * still yield BWAMS_ERR_CAPACITY when too small.
 *
 * Order of calls on a batch.  A batch holds one chunk, and each stage's result is computed from earlier ones: the reads
 * (bwams_seed_upload) -> seeds (bwams_seed_run / _run_ert) -> chains -> extension -> de-duplication -> pairing -> alignment records
 * (bwams_reg2aln_run*) -> SAM text -> BAM records -> their sort and their templates; beside that line the names (bwams_sam_upload,
 * after the reads, read by the text only) and the exact-match probe (bwams_emf_run, after the reads) with its regions
 * (bwams_emf_regs_run, read by bwams_emf_regs_merge and bwams_sam_run_emf).  Running or uploading a stage again replaces its result
 * and invalidates everything computed from it: a call that needs an invalidated result returns BWAMS_ERR_ARG with the text it has for
 * a stage that never ran ("run ... first") until the stages between have run again, in order.  New reads (bwams_seed_upload, and
 * bwams_emf_probe, which uploads reads of its own and so needs a bwams_seed_upload behind it) invalidate everything else the batch
 * holds, BAM records of bwams_bam_upload included.  Results that do not derive from one another stay: a seed run keeps the probe,
 * its regions and the names; new names keep the alignment records; bwams_bam_sort keeps the text.  A refused call changes nothing. */
int bwams_batch_create(bwams_index_t *idx, int64_t max_reads, int64_t max_bases,
                       int64_t max_smem, int64_t max_sa, bwams_batch_t **out);
int bwams_batch_destroy(bwams_batch_t *b);

/* -------------------------------------------------------------- seeding ---- */

/* One-call seeding on host buffers.  Replaces, for a whole chunk,
 *   mem_collect_smem            (src/bwamem.cpp:648-786; called at :1321) and
 *   get_sa_entries_prefetch     (src/FMI_search.cpp:2261; called at src/bwamem.cpp:861).
 *
 *   enc_qdb   concatenated reads, one base code per byte (0..3, >=4 = N)
 *   cum_len   nseq+1 offsets into enc_qdb (query_cum_len_ar, widened to 64 bit)
 *   skip      optional nseq flags; non-zero = read resolved by the exact-match
 *             filter, not seeded (seq_[l].perfect.exist, src/bwamem.cpp:674-689)
 *   smem_out  SMEMs of all reads ordered by (rid, m, n); smem_cap slots
 *   sa_coord  reference coordinates of each SMEM's sampled occurrences, in SMEM
 *             order; SMEM i owns sa_coord[sa_off[i] .. sa_off[i+1])
 *   sa_off    n_smem+1 entries (so at least smem_cap+1 slots)
 * sa_coord/sa_off may be NULL to skip the SA step. */
int bwams_seed_fmi(bwams_batch_t *b,
                   const uint8_t *enc_qdb, const int64_t *cum_len, const uint8_t *skip,
                   int64_t nseq, const bwams_seed_opt_t *opt,
                   bwams_smem_t *smem_out, int64_t smem_cap, int64_t *n_smem,
                   int64_t *sa_coord, int64_t sa_cap, int64_t *sa_off, int64_t *n_sa);

/* The same in three steps, so that reads stay resident in HBM across calls and
 * uploads/downloads can overlap other work: upload -> run (asynchronous on the
 * batch's stream) -> fetch (synchronises). */
/* (enc_qdb may be a host pointer or a pointer into this GPU's memory; cum_len and skip are host arrays.) */
int bwams_seed_upload(bwams_batch_t *b, const uint8_t *enc_qdb, const int64_t *cum_len,
                      const uint8_t *skip, int64_t nseq);
int bwams_seed_run(bwams_batch_t *b, const bwams_seed_opt_t *opt, int with_sa);
int bwams_seed_counts(bwams_batch_t *b, int64_t *n_smem, int64_t *n_sa);   /* synchronises */
int bwams_seed_fetch(bwams_batch_t *b, bwams_smem_t *smem_out, int64_t smem_cap,
                     int64_t *sa_coord, int64_t sa_cap, int64_t *sa_off);

/* ------------------------------------------------------------ extension ---- */

/* Banded Smith-Waterman seed extension over n tasks.  Replaces the six call
 * sites BandedPairWiseSW::{scalarBandedSWAWrapper,getScores16,getScores8}
 * (src/bwamem.cpp:3229,3297,3366,3445,3510,3581): fills score, tle, gtle, qle,
 * gscore, max_off of every pair in place with the values of scalarBandedSWA
 * (src/bandedSWA.cpp:116-237).  ref/qer are the flat seqBufRef/seqBufQer byte
 * buffers of ref_bytes/qer_bytes bytes. */
int bwams_bsw_extend(bwams_batch_t *b, bwams_seqpair_t *pairs, int64_t n,
                     const uint8_t *ref, int64_t ref_bytes,
                     const uint8_t *qer, int64_t qer_bytes,
                     int32_t w, const bwams_sw_opt_t *opt);

/* Resident form: upload once, run (async), fetch.  A query (len2) of more than 18196 bases
 * is refused with BWAMS_ERR_UNSUPPORTED: the tasks the packed kernels cannot take run one
 * per wavefront with the query's row in LDS, and one wavefront's row must fit a CU's 160 KiB
 * (the bound of the extension inside bwams_extend_run too). */
int bwams_bsw_upload(bwams_batch_t *b, const bwams_seqpair_t *pairs, int64_t n,
                     const uint8_t *ref, int64_t ref_bytes, const uint8_t *qer, int64_t qer_bytes);
int bwams_bsw_run(bwams_batch_t *b, int32_t w, const bwams_sw_opt_t *opt);
int bwams_bsw_fetch(bwams_batch_t *b, bwams_seqpair_t *pairs, int64_t n);

/* ------------------------------------------------------------------- EMF ---- */

/* Exact-match filter.  open/from_host replace load_perfect_table (src/perfect_map.cpp:344):
 * <prefix>.perfect.<L> = 64-byte header, u32 loc_table[], seed_entry_t seed_table[]
 * (src/perfect.h:188-213, :772-822).  The index must hold its .0123 reference. */
int bwams_emf_open(bwams_index_t *idx, const char *path, bwams_emf_t **out);
int bwams_emf_from_host(bwams_index_t *idx, int32_t seed_len, uint32_t seq_len, const uint32_t *loc_table,
                        uint32_t num_loc_entry, const bwams_seed_entry_t *seed_table, uint32_t num_seed_entry,
                        bwams_emf_t **out);
/* adopt a table that already lives in this GPU's memory (not copied, not freed) */
int bwams_emf_from_device(bwams_index_t *idx, int32_t seed_len, uint32_t seq_len, const uint32_t *loc_table_dev,
                          uint32_t num_loc_entry, const bwams_seed_entry_t *seed_table_dev, uint32_t num_seed_entry,
                          bwams_emf_t **out);
/* Builds the table on the GPU from the resident forward reference (replaces `bwa-mem2.scale perfect-index`,
 * src/perfect_index.cpp): every L-mer of the forward strand, canonical orientation, one bucket per hash value with its
 * L-mers in ascending order (root in the bucket's slot, the others in free slots), further locations of repeated L-mers
 * in loc_table.  num_seed_entry = slack x l_pac (the reference uses 1.1).  The table is the reference's format and is
 * probed identically; the placement of collision nodes differs from the reference builder's (which is order dependent). */
int bwams_emf_build(bwams_index_t *idx, int32_t seed_len, double slack, bwams_emf_t **out);
int bwams_emf_info(const bwams_emf_t *emf, int32_t *seed_len, uint32_t *num_seed_entry, uint32_t *num_loc_entry, int64_t *n_used,
                   int64_t *n_key, int64_t *build_ms);
/* the two arrays back to the host (either may be NULL) / the `<prefix>.perfect.<L>` file (src/perfect.h:188-213) */
int bwams_emf_table_fetch(bwams_emf_t *emf, uint32_t *loc_table, bwams_seed_entry_t *seed_table);
int bwams_emf_save(bwams_emf_t *emf, const char *path);
int bwams_emf_close(bwams_emf_t *emf);

/* Replaces the kernel-0 loop of mem_kernel1_core (src/bwamem.cpp:1245-1272): for every read
 * out[i] = seqs[i].perfect and code[i] = the return value of find_perfect_match_entry
 * (src/perfect_map.cpp:638-659; 0 no table / read shorter than L, 1 read has N, 2 not matched,
 * 3 forward match, 4 reverse-complement match, 5 seed matched but not the whole read).
 * `code[i] == 3 || code[i] == 4` is the `skip` flag bwams_seed_fmi takes. */
int bwams_emf_probe(bwams_batch_t *b, bwams_emf_t *emf, const uint8_t *enc_qdb, const int64_t *cum_len,
                    int64_t nseq, bwams_perfect_t *out, uint8_t *code);

/* Resident form: probe the reads uploaded by bwams_seed_upload and set the skip flags on the device,
 * so that the next bwams_seed_run leaves the matched reads out; fetch returns the probe results. */
int bwams_emf_run(bwams_batch_t *b, bwams_emf_t *emf);
int bwams_emf_fetch(bwams_batch_t *b, bwams_perfect_t *out, uint8_t *code);

/* ------------------------------------------------- alignments for SAM (f3) ---- */

/* CIGAR, NM, MD, position and mapping quality of every final region of the chunk.  Replaces, per region, mem_reg2aln
 * (src/bwamem.cpp:2533-2628; called from mem_reg2sam, :2318, and mem_sam_pe, src/bwamem_pair.cpp) with what it calls:
 * bwa_gen_cigar2 (src/bwa.cpp:380-467) -> ksw_global2 with traceback (src/ksw.cpp:558-668), and mem_approx_mapq_se
 * (src/bwamem.cpp:1983-2008).  source 0: the regions bwams_dedup_run left (single-end), 1: those of bwams_pair_run.
 * fetch returns one bwams_aln_t per region in region order, the CIGAR pool (uint32 opLen << 4 | op) and the MD pool
 * (NUL-terminated strings); the XA string and the SAM text stay on the host. */
int bwams_reg2aln_run(bwams_batch_t *b, const bwams_mem_opt_t *opt, int32_t source, int64_t *n_aln, int64_t *n_cigar_ops,
                      int64_t *md_bytes);
/* The same for the regions of bwams_pair_run (source 1), restricted to what the SAM text will read — as the reference, which calls
 * mem_reg2aln from mem_reg2sam / mem_gen_alt / mem_sam_pe only for the records it prints, the members of their XA strings, the paired
 * regions and the mate records (src/bwamem.cpp:2100-2120, src/bwamem_extra.cpp:150-160, src/bwamem_pair.cpp:753-796).  The set follows
 * from the regions, the pairing result and sopt alone; the other regions (two thirds on the bench chunk) keep an unmapped record
 * (rid = -1).  pes = NULL for single-end chunks.  bwams_sam_run / bwams_sam_run_pe with the same sopt then produce the same text as
 * after bwams_reg2aln_run. */
int bwams_reg2aln_run_sam(bwams_batch_t *b, const bwams_mem_opt_t *opt, const bwams_sam_opt_t *sopt, const bwams_pestat_t *pes,
                          int64_t *n_aln, int64_t *n_needed, int64_t *n_cigar_ops, int64_t *md_bytes);
int bwams_reg2aln_fetch(bwams_batch_t *b, bwams_aln_t *aln, int64_t aln_cap, uint32_t *cigar, int64_t cigar_cap, char *md,
                        int64_t md_cap);

/* ------------------------------------------------------ SAM text, single-end ---- *
 * The text worker_sam's single-end branch leaves in seqs[i].sam (src/bwamem.cpp:1836-1844): per read, mem_reg2sam
 * (src/bwamem.cpp:2091-2150: which regions become records, supplementary flag 0x800 / 0x10000, the mapq cap of later records),
 * mem_gen_alt (src/bwamem_extra.cpp:123-187: the XA strings) and mem_aln2sam with m = NULL (src/bwamem.cpp:2380-2531: the
 * eleven fields, NM / MD / AS / XS / RG / SA / pa / XA tags, the comment), with mem_approx_mapq_se (:1983-2008) evaluated on the
 * device.  Call order for a chunk: ... bwams_dedup_run, bwams_pair_run(BWAMS_PAIR_SINGLE_END) (= mem_mark_primary_se),
 * bwams_reg2aln_run(source 1), bwams_sam_upload (names / qualities / comments of the chunk: the bseq1_t fields the hot path
 * never needed), bwams_sam_run, bwams_sam_fetch.  MEM_F_PRIMARY5 (mem_reorder_primary5) acts in bwams_pair_run_sam, MEM_F_REF_HDR (XR:Z:)
 * needs bwams_index_set_contig_annos first; both are built.
 * Paired-end chunks: bwams_sam_run_pe; chunks with reads the EMF resolved: bwams_sam_run_emf (both below). */
/* names of the index's sequences (bntann1_t.name): NUL-terminated, back to back; name_off[n_seqs + 1], name_off[i] = start of
 * name i.  Call after bwams_index_set_contigs (or on a one-sequence index). */
int bwams_index_set_contig_names(bwams_index_t *ix, const char *names, const int32_t *name_off);
/* bntann1_t.anno of the index's sequences, laid out like the names (an empty string = no annotation): what MEM_F_REF_HDR (`mem -V`)
 * prints as XR:Z: (src/bwamem.cpp:2522-2529, :2218-2225).  A text run with that flag and no annotations set is refused. */
int bwams_index_set_contig_annos(bwams_index_t *ix, const char *annos, const int32_t *anno_off);
/* names: the reads' names back to back (no terminators), name_off[nseq + 1]; quals: one byte per base laid out like the reads
 * (cum_len), or NULL ('*'); comments (+ comment_off[nseq + 1], an empty comment = none) or NULL. */
int bwams_sam_upload(bwams_batch_t *b, const char *names, const int64_t *name_off, const char *quals, const char *comments,
                     const int64_t *comment_off);
int bwams_sam_run(bwams_batch_t *b, const bwams_mem_opt_t *opt, const bwams_sam_opt_t *sopt, int64_t *sam_bytes);
/* bwams_sam_run for a chunk that went through the exact-match filter: a read bwams_emf_regs_run resolved in THIS chunk gets the
 * records of mem_perfect2sam_cont / mem_aln2sam_perfect (src/bwamem.cpp:2280-2325, :2153-2227: MAPQ 60, <l_seq>M, NM 0, AS = l_seq * a,
 * XS = AS when there is a second location, secondaries only with MEM_F_ALL, ALT locations last) as worker_sam's `perfect.exist`
 * branch (src/bwamem.cpp:1786-1797) writes them; every other read goes through mem_reg2sam as in bwams_sam_run.  (Paired-end chunks
 * need nothing special: worker_sam turns resolved ends into regions — bwams_emf_regs_run — and calls mem_sam_pe.) */
int bwams_sam_run_emf(bwams_batch_t *b, const bwams_mem_opt_t *opt, const bwams_sam_opt_t *sopt, bwams_emf_t *emf, int64_t *sam_bytes);
/* The paired-end text: mem_sam_pe from the call of mem_pair on (src/bwamem_pair.cpp:686-833 = the tail of mem_sam_pe_batch_post,
 * :1070-1190) for every pair of the chunk (reads 2p, 2p + 1), after bwams_pair_run (mate rescue, marks, mem_pair) and
 * bwams_reg2aln_run(source 1): the multi-hit test, q_pe / q_se with the +40 and tandem-repeat caps, the edits of the paired regions
 * (sub, secondary = -2, the secondary_all switch before XA), the ALT hit, flags 0x1 / 0x2 / 0x8 / 0x20 / 0x40 / 0x80, RNEXT / PNEXT /
 * TLEN, MC:Z, an unmapped end at its mate's coordinates; or the no_pairing branch (proper-pair flag from mem_infer_dir and pes, then
 * mem_reg2sam per end with the mate's record).  pes = what bwams_pestat returned for the chunk.  MEM_F_NOPAIRING is not built. */
int bwams_sam_run_pe(bwams_batch_t *b, const bwams_mem_opt_t *opt, const bwams_sam_opt_t *sopt, const bwams_pestat_t pes[4],
                     int64_t *sam_bytes);
/* sam: the text of all reads in read order (cap >= sam_bytes); read_off[nseq + 1]: where a read's lines start; mapq: the
 * device-side mem_approx_mapq_se of every region (region order of bwams_reg2aln_fetch).  Any of the three may be NULL. */
int bwams_sam_fetch(bwams_batch_t *b, char *sam, int64_t cap, int64_t *read_off, int32_t *mapq, int64_t mapq_cap);
/* The batch's SAM text (after bwams_sam_run / _run_pe / _run_emf or bwams_process_chunk*) compressed where it lies by `d`, after the
 * work queued on the batch's stream: BGZF members into host memory out[0, cap), as bwams_deflater_run writes them (flags:
 * BWAMS_DEFLATE_EOF).  They inflate to exactly what bwams_sam_fetch returns.  BWAMS_ERR_ARG: no SAM run yet, or d on another device. */
int bwams_sam_fetch_bgzf(bwams_batch_t *b, bwams_deflater_t *d, void *out, int64_t cap, int32_t flags, int64_t *n_out);

/* ------------------------------------------------------------- BAM ---- *
 * The batch's SAM text, whichever run made it (bwams_sam_run / _run_pe / _run_emf, bwams_process_chunk / _chunk2 / _chunk_smart), as
 * BAM alignment records (SAMv1 §4.2), one per line in text order, encoded on the device where the text lies, with htslib's rules
 * (sam_parse1 + bam_write1): refID / next_refID = the sequence's index in the index's order (-1 for '*', RNEXT '=' is refID), 0-based
 * POS / PNEXT, bin = reg2bin(pos, end) with end = pos + the CIGAR's reference length (pos + 1 when unmapped, CIGAR '*' or length 0),
 * read name + one NUL, SEQ in 4-bit codes (high nibble first), QUAL - 33 (0xFF bytes when '*'), aux fields in text order with the
 * smallest integer type (c / s / i when negative, C / S / I otherwise), f as (float)strtod.  bwams/bam.py restates the rules.
 * BWAMS_ERR_UNSUPPORTED, nothing kept, bwams_last_error naming the earliest read concerned: text BAM cannot hold, all of it from the
 * user — a read name over 254 bytes, a copied FASTQ comment (BWAMS_CHUNK_COPY_COMMENT, mem -C) that is not TG:T:value fields of type
 * A, i, f, Z or H (Illumina's "1:N:0:ACGT"; B arrays are refused too), an integer outside int32 / uint32, more than 65535 CIGAR
 * operations.  BWAMS_ERR_ARG: no SAM run yet, an index without sequence names, or one where two sequences share a name. */
int bwams_bam_run(bwams_batch_t *b, int64_t *bam_bytes, int64_t *n_records);
/* bam: the records of the last bwams_bam_run (cap >= bam_bytes, BWAMS_ERR_CAPACITY otherwise); read_off[n + 1]: where each read's
 * records start (n = the reads of the SAM text, as for bwams_sam_fetch).  Either may be NULL. */
int bwams_bam_fetch(bwams_batch_t *b, void *bam, int64_t cap, int64_t *read_off);
/* The records compressed where they lie, as bwams_sam_fetch_bgzf compresses the text (BWAMS_DEFLATE_EOF; a record may span two
 * members, which SAMv1 §4.1 allows). */
int bwams_bam_fetch_bgzf(bwams_batch_t *b, bwams_deflater_t *d, void *out, int64_t cap, int32_t flags, int64_t *n_out);
/* Coordinate sort of the batch's BAM records where they lie (csrc/bam_sort.hip), in the order bwams_bam_coord_t's key defines
 * (include/bwams_types.h; bwams/bam.py restates it).
 * _upload: host records bam[0, n_bytes) become the batch's records, as if bwams_bam_run had made them (any BAM, e.g. another
 * aligner's; a fresh batch will do).  The block_size chain is checked: every record has block_size >= 32, its name and CIGAR
 * inside it, refID >= -1 and -1 <= POS <= 2^31 - 2, and the chain ends exactly at n_bytes; BWAMS_ERR_ARG otherwise, nothing kept.
 * After an upload each record counts as one read: bwams_bam_fetch's read_off holds n_records + 1 entries, the records' offsets.
 * _sort: BWAMS_ERR_ARG before any bwams_bam_run or _upload.  The unsorted records (bwams_bam_fetch, _fetch_bgzf) stay as they are;
 * a second call on records it has sorted already returns at once.  *n_records may be NULL.
 * _sorted_fetch: the sorted records (cap >= the bytes of bwams_bam_run / _upload, BWAMS_ERR_CAPACITY otherwise) and their
 * n_records coords in sorted order; either pointer may be NULL.  BWAMS_ERR_ARG before a _sort of the current records. */
int bwams_bam_upload(bwams_batch_t *b, const void *bam, int64_t n_bytes, int64_t *n_records);
int bwams_bam_sort(bwams_batch_t *b, int64_t *n_records);
int bwams_bam_sorted_fetch(bwams_batch_t *b, void *bam, int64_t cap, bwams_bam_coord_t *coords);
/* Duplicate marking (csrc/markdup.hip): Picard MarkDuplicates' rules for query-grouped input — default SUM_OF_BASE_QUALITIES scoring,
 * no barcodes.  Rules 1-8 are one library without optical duplicate detection (the calls without a 2 or 3 in their names); rules 9-15
 * below them add read groups, libraries, optical duplicates and the metrics file.  bwams/markdup.py restates all of them.
 *  1. Template: a maximal run of consecutive records with byte-equal read names, in the batch's unsorted order.  This is the order
 *     bwams_bam_run produces, and the order an uploaded BAM is given in.  A template never spans two batches or two sorter puts.
 *  2. Primary: FLAG has neither 0x100 nor 0x800.  A primary's segment is "only" when 0x1 is clear.  When 0x1 is set, it is "first"
 *     for 0x40 and "last" for 0x80.  A template is refused with BWAMS_ERR_UNSUPPORTED in any of these cases, and bwams_last_error
 *     names the first record concerned: two primaries of one segment (for example, two adjacent single-end reads that share a
 *     name); a paired primary with neither or both of 0x40/0x80; paired and unpaired primaries mixed.  (The record concerned is
 *     the one at which a walk over the template in order meets the fault: the second primary of a segment, the paired primary
 *     without a single segment bit, the first primary whose 0x1 differs from the template's first primary's.)
 *  3. Unclipped 5' coordinate of a mapped primary (0x4 clear), 0-based: forward: POS - (the S and H lengths before the first other
 *     op); reverse (0x10): POS + rlen - 1 + (the S and H lengths after the last other op), where rlen is the sum of the M/D/N/=/X
 *     lengths, taken as 1 when it is 0.  A coordinate outside [-2^31, 2^31) is refused as in rule 2, and so is a mapped primary
 *     with refID -1.
 *  4. Score of a mapped primary: the sum of its QUAL values that are >= 15, capped at 16383 (Picard's Short.MAX_VALUE / 2).  It is 0
 *     when QUAL is absent (0xFF).  A pair's score is the sum of its two ends' scores.
 *  5. Ends: Pair: a template whose two primaries ("first" and "last") are both mapped.  End 1 is the end with the smaller (refID,
 *     coordinate); on a tie it is the earlier record.  The pair key is (ref1, c1, strand1, ref2, c2, strand2), so FR and RF at the
 *     same places are different keys.  Fragment: any other template with exactly one mapped primary.  The fragment key is (ref, c,
 *     strand).  Each end of a pair is also a paired fragment under its own fragment key, for rule 6 only.
 *  6. Decision.  The tie-break "earlier" below means input order: the batch's record order, and across sorter puts, seq first.
 *     Pairs with equal keys: the pair with the highest score is kept.  Ties go to the earlier template.  Every other pair is a
 *     duplicate.  Fragments with equal keys: if the group holds any paired fragment, every unpaired fragment in it is a duplicate.
 *     Otherwise the highest score is kept, ties go to the earlier template, and the rest are duplicates.
 *  7. Marking: every record of a duplicate template gets FLAG 0x400.  That includes its primaries, its secondary and supplementary
 *     records, and the unmapped mate of a duplicate fragment.  This is what Picard does on query-grouped input.  Every other record
 *     has 0x400 cleared.  Templates with no mapped primary are never duplicates.  Nothing but that one FLAG bit changes, so sizes,
 *     bins and the BAI stay the same.
 *  8. Counts (bwams_dup_stats_t): templates: all templates; unpaired_examined / unpaired_duplicates: fragments, and the fragments
 *     marked; pairs_examined / pair_duplicates: pairs (not reads), and the pairs marked; records_marked: records that end up with
 *     0x400 set; ms_decide: host clock around the decision.  Picard's PERCENT_DUPLICATION is (unpaired_duplicates +
 *     2 pair_duplicates) / (unpaired_examined + 2 pairs_examined).
 * _templates: groups the batch's current records (bwams_bam_run / _upload) into templates and computes their ends on the device:
 * *n_templates, and *n_ends (one per template with a mapped primary, in template order); either may be NULL.  Rules 1-3 refuse here
 * (BWAMS_ERR_UNSUPPORTED).  BWAMS_ERR_ARG before any bwams_bam_run or _upload.  More than 2^32 - 1 records: BWAMS_ERR_UNSUPPORTED.
 * _templates_fetch (after _templates on the current records): the n_ends ends (cap >= n_ends, BWAMS_ERR_CAPACITY otherwise) and each
 * record's template ordinal, in record order, or with sorted = 1 in the order of bwams_bam_sort (BWAMS_ERR_ARG before a sort of the
 * current records); either pointer may be NULL.
 * bwams_dup_decide: rule 6 on `device` over host ends[0, n_ends) of templates [0, n_templates): dup[t] = 1 for every duplicate
 * template, 0 otherwise (n_templates bytes, host memory).  Each template has at most one end.  Every tmpl must lie in
 * [0, n_templates), ref1 in [0, 2^30), ref2 in [-1, 2^30), score in [0, 32767] and strands in [0, 3] (bit 1 only with an end 2):
 * BWAMS_ERR_ARG otherwise, with the first bad end in bwams_last_error.  The decision's device buffers (about 110 B per end) that do
 * not fit: BWAMS_ERR_NOMEM.  *st (may be NULL): rule 8's counts, records_marked 0.
 * _markdup: the batch alone is the whole input: _templates, the decision and the marking, all in HBM.  The unsorted records and the
 * sorted copy, when the current records have one, are marked, so bwams_bam_fetch, _fetch_bgzf, _sort and _sorted_fetch all see the
 * flags.  A second call gives the same records.  *st may be NULL.
 *
 * Read groups, libraries, optical duplicates and the metrics (Picard where Picard is definite; where a choice was made the rule says so):
 *  9. Read groups and libraries.  A groups table (bwams_dup_groups_t) is made from SAM header text.  Every @RG line gives a read group
 *     whose ordinal is the line's place among the @RG lines.  Its ID is required: a line without one, or two lines with one ID, is
 *     BWAMS_ERR_ARG.  Its LB is optional.  Libraries are the distinct LB values in order of first appearance, ordinals from 0; after
 *     them comes one more, "Unknown Library", which always exists, so n_lib = distinct LBs + 1.  With no table n_lib = 1 and
 *     everything is "Unknown Library".  A record's read group is the value of its first aux field with tag RG and type Z, found by
 *     walking the aux fields by their types (SAMv1 §4.2.4: A c C s S i I f Z H B) to the record's end.  A field of unknown type
 *     (or a B array of unknown element type), or one that runs past block_size, refuses the batch as rules 2-3 do, with a fifth
 *     reason, "aux fields do not chain to the record's end"; rules 2-3 are checked over the whole batch first, so this
 *     reason names the first such record of a batch they accept.  Only one record per template is walked: its first primary in record order, or its first record
 *     when it has no primary; and only when a table is given (choice: without one no read group can be looked up, and the calls of
 *     rules 1-8 keep accepting what they accept).  That record's read group is the template's; ordinal -1 means no RG field or a
 *     value not in the table.  The template's library is its read group's; ordinal -1 and read groups without LB belong to
 *     "Unknown Library".
 * 10. Location, from the name of the record rule 9 names (without its NUL), split at ':'.  Exactly 5 fields: tile, x, y are fields
 *     2, 3, 4 (from 0).  Exactly 7 or 8 fields: fields 4, 5, 6.  Any other count: no location.  A field's value is an optional '-',
 *     then the decimal digits up to the first byte that is not a digit; the rest is ignored and no digits gives 0.  A value outside
 *     int32 means no location.
 * 11. Keys.  The library ordinal is the most significant part of the pair key and of the fragment key of rules 5-6: equal places in
 *     two libraries are not duplicates of each other.  (The decision folds it into the refIDs, library * (largest refID + 1) + refID,
 *     which must stay below 2^31: BWAMS_ERR_UNSUPPORTED otherwise.)
 * 12. Optical duplicates, for a distance d > 0 (Picard's default is 100, and 2500 for patterned flow cells; 0 turns it off).  Only
 *     pairs are examined.  In a group of pairs with equal key that holds between 2 and max_set members (Picard: 300000), two members
 *     are close when both have a location, their read-group ordinals are equal (-1 equals -1), their tiles are equal, and
 *     |x - x'| <= d and |y - y'| <= d, the differences taken in 64 bits.  Clusters are the connected components of "close"; a member
 *     with no location is a cluster of its own.  A cluster's representative is the group's kept pair (rule 6) if it is in the
 *     cluster, otherwise the member with the smallest template ordinal.  Every other member is an optical duplicate, so a group's
 *     optical count is the sum over its clusters of (size - 1).  (Picard switches between two algorithms at a group size of 4; both
 *     give this count.)  Nothing is written into the records: Picard's default TAGGING_POLICY is DontTag.
 * 13. Per-library counts (bwams_dup_lib_stats_t), each attributed to the template's library: unpaired_examined, pairs_examined,
 *     unpaired_duplicates, pair_duplicates as in rule 8; pair_optical_duplicates: rule 12; secondary_or_supplementary: records with
 *     0x100 or 0x800 set and 0x4 clear; unmapped: records with 0x4 set; percent_duplication: rule 8's formula, 0 when the denominator
 *     is 0; estimated_library_size: rule 14, -1 for none.  Summed over libraries, the first four equal bwams_dup_stats_t's.
 * 14. Estimated library size: Picard's estimateLibrarySize, on the host in doubles with the C library's exp.  n = pairs_examined -
 *     pair_optical_duplicates, c = pairs_examined - pair_duplicates.  None if n <= 0, n - c <= 0 or c <= 0.  Otherwise, with
 *     f(x) = c/x - 1 + exp(-n/x): m = 1.0, M = 100.0; while f(M*c) > 0: M *= 10.0; 40 times: r = (m + M) / 2, u = f(r*c), stop if
 *     u == 0, m = r if u > 0 else M = r; the result is (int64)(c * (m + M) / 2.0).  (1000, 900) gives 4660 and (2, 1) gives 1.
 * 15. Metrics text, Picard's layout: a line "## htsjdk.samtools.metrics.StringHeader"; a line "# " and the caller's text; a line
 *     "## METRICS CLASS\tpicard.sam.DuplicationMetrics"; the column line LIBRARY UNPAIRED_READS_EXAMINED READ_PAIRS_EXAMINED
 *     SECONDARY_OR_SUPPLEMENTARY_RDS UNMAPPED_READS UNPAIRED_READ_DUPLICATES READ_PAIR_DUPLICATES READ_PAIR_OPTICAL_DUPLICATES
 *     PERCENT_DUPLICATION ESTIMATED_LIBRARY_SIZE, tab-separated; one row per library that has any count above zero, in ordinal order;
 *     an empty line.  PERCENT_DUPLICATION is printed as %.6f; ESTIMATED_LIBRARY_SIZE is left empty when there is none.  Picard's
 *     histogram section is not written.
 * The DT tag, REMOVE_DUPLICATES and barcode / UMI keys are out of scope.
 * bwams_dup_groups_create: the table of header_text[0, n_text) (lines end at '\n', a '\r' before it dropped; fields are split at
 * tabs); _info: its read groups and libraries (either pointer may be NULL); _library: library lib's name, owned by the table (NULL
 * table: "Unknown Library" for 0), NULL outside [0, n_lib); _destroy (NULL allowed).  A host object; calls that take one only read it.
 * _templates2: _templates, then rules 9-10 on the device for every template: the template's read group, library and location.
 * groups may be NULL.  _templates_fetch_loc (after _templates2 on the current records, BWAMS_ERR_ARG otherwise): one bwams_dup_loc_t
 * per end, parallel to _templates_fetch's ends (cap >= n_ends, BWAMS_ERR_CAPACITY otherwise).  _lib_record_counts (after _templates
 * or _templates2): rule 13's two record-level counts of the batch per library (one library after _templates), n_lib values each;
 * either pointer may be NULL; cap_lib < n_lib is BWAMS_ERR_CAPACITY.
 * bwams_dup_decide2: bwams_dup_decide with rules 11-13.  loc: one per end, or NULL for library 0 and no location; every loc.lib must
 * lie in [0, n_lib) and has in {0, 1} (BWAMS_ERR_ARG naming the first such end).  opt may be NULL: optical detection off;
 * max_optical_set 0 means 300000; a negative value is BWAMS_ERR_ARG.  optical (n_templates bytes, may be NULL): 1 for every optical
 * duplicate.  lib_stats (n_lib rows, may be NULL): rule 13, the two record-level counts 0.
 * _markdup2: _markdup with a table and options: everything in HBM, *st and lib_stats[0, n_lib) (either may be NULL; cap_lib < n_lib
 * is BWAMS_ERR_CAPACITY) with all counts filled.  With groups NULL and optical detection off it is _markdup: the same kernels, the
 * same records, the same *st.
 * bwams_dup_library_size: rule 14, -1 for none.  bwams_dup_metrics_text: rule 15 into out[0, cap) for lib_stats[0, n_lib) (n_lib must
 * be the table's, 1 for a NULL table: BWAMS_ERR_ARG otherwise); comment may be NULL; *n_out: the bytes written, or needed with
 * BWAMS_ERR_CAPACITY, as bwams_sam_header. */
int bwams_bam_templates(bwams_batch_t *b, int64_t *n_templates, int64_t *n_ends);
int bwams_dup_groups_create(const char *header_text, int64_t n_text, bwams_dup_groups_t **out);
int bwams_dup_groups_info(const bwams_dup_groups_t *g, int64_t *n_rg, int64_t *n_lib);
const char *bwams_dup_groups_library(const bwams_dup_groups_t *g, int64_t lib);
void bwams_dup_groups_destroy(bwams_dup_groups_t *g);
int bwams_bam_templates2(bwams_batch_t *b, const bwams_dup_groups_t *groups, int64_t *n_templates, int64_t *n_ends);
int bwams_bam_templates_fetch_loc(bwams_batch_t *b, bwams_dup_loc_t *loc, int64_t cap);
int bwams_bam_lib_record_counts(bwams_batch_t *b, int64_t *secondary_or_supplementary, int64_t *unmapped, int64_t cap_lib);
int bwams_dup_decide2(int device, const bwams_dup_end_t *ends, const bwams_dup_loc_t *loc, int64_t n_ends, int64_t n_templates,
                      int64_t n_lib, const bwams_dup_opt_t *opt, uint8_t *dup, uint8_t *optical, bwams_dup_lib_stats_t *lib_stats);
int bwams_bam_markdup2(bwams_batch_t *b, const bwams_dup_groups_t *groups, const bwams_dup_opt_t *opt, bwams_dup_stats_t *st,
                       bwams_dup_lib_stats_t *lib_stats, int64_t cap_lib);
int64_t bwams_dup_library_size(int64_t n, int64_t c);
int bwams_dup_metrics_text(const bwams_dup_groups_t *g, const bwams_dup_lib_stats_t *lib_stats, int64_t n_lib, const char *comment,
                           char *out, int64_t cap, int64_t *n_out);
int bwams_bam_templates_fetch(bwams_batch_t *b, bwams_dup_end_t *ends, int64_t cap, uint32_t *rec_tmpl, int32_t sorted);
int bwams_dup_decide(int device, const bwams_dup_end_t *ends, int64_t n_ends, int64_t n_templates, uint8_t *dup, bwams_dup_stats_t *st);
int bwams_bam_markdup(bwams_batch_t *b, bwams_dup_stats_t *st);
/* bwa_print_sam_hdr into out[0, cap): "@SQ\tSN:<name>\tLN:<len>" per sequence ("\tAH:*" for ALT sequences) unless hdr_line holds @SQ
 * lines of its own; then hdr_line and a newline (mem -H text and the @RG line, as main_mem builds it); then pg_line as given (it carries
 * its own newline).  hdr_line / pg_line may be NULL.  *n_out: the bytes written, or needed with BWAMS_ERR_CAPACITY. */
int bwams_sam_header(const bwams_index_t *idx, const char *hdr_line, const char *pg_line, char *out, int64_t cap, int64_t *n_out);
/* The BAM header block (SAMv1 §4.2): "BAM\1", l_text, the header text (n_text bytes, no NUL added), n_ref and, per sequence of the
 * index in index order (what refID counts), l_name (with its NUL), the name and l_ref.  *n_out as for bwams_sam_header. */
int bwams_bam_header(const bwams_index_t *idx, const char *text, int64_t n_text, void *out, int64_t cap, int64_t *n_out);

/* ------------------------------------------------------------- read input ---- *
 * A buffer of FASTQ text (host or this GPU's memory) becomes the arrays bwams_seed_upload and bwams_sam_upload take: replaces, per
 * record, kseq_read (src/kseq.h:358-400), trim_readno and kseq2bseq1 (src/bwa.cpp:74-153) as bseq_read_orig (src/bwa.cpp:266-335)
 * calls them, and the base encoding of mem_kernel1_core (src/bwamem.cpp:1232, nst_nt4_table).  Built for FASTQ in the four-lines-per-record
 * shape and for FASTA text (first byte '>', sequences over any number of lines, blank lines skipped; no qualities: bwams_fastq_has_qual = 0);
 * multi-line or mixed FASTQ input, a quality string of another length than its sequence, or a '-' among the bases return
 * BWAMS_ERR_UNSUPPORTED (read such a file on the host).  The buffer must hold whole records; gz decompression and the chunking by
 * base count stay with the caller.  Names come without their "/<digit>" suffix; a read's comment is the header line after the
 * first white-space character (empty = none). */
typedef struct bwams_fastq bwams_fastq_t;
int bwams_fastq_decode(int device, const char *text, int64_t n_bytes, bwams_fastq_t **out, int64_t *n_reads, int64_t *n_bases);
int bwams_fastq_info(const bwams_fastq_t *f, int64_t *n_reads, int64_t *n_bases, int64_t *name_bytes, int64_t *comment_bytes, float *ms);
int bwams_fastq_has_qual(const bwams_fastq_t *f);      /* 0: FASTA text (bseq1_t.qual == NULL for every read) */
/* any pointer may be NULL; enc / quals hold n_bases bytes, cum / name_off / comment_off n_reads + 1 entries */
int bwams_fastq_fetch(bwams_fastq_t *f, uint8_t *enc, int64_t *cum, char *names, int64_t *name_off, char *quals, char *comments,
                      int64_t *comment_off);
/* bwams_seed_upload + bwams_sam_upload of the decoded chunk, device to device.  The reference drops the comments unless `mem -C` was
 * given (process(), src/fastmap.cpp:335-342): copy_comment = 0 does the same; bwams_fastq_to_batch keeps them. */
int bwams_fastq_to_batch(bwams_fastq_t *f, bwams_batch_t *b);
int bwams_fastq_to_batch_opt(bwams_fastq_t *f, bwams_batch_t *b, int32_t copy_comment);
int bwams_fastq_close(bwams_fastq_t *f);

/* ------------------------------------------------------------- BAM as read input ---- *
 * BAM alignment records (SAMv1 §4.2, back to back, no header block; host or this device's memory) as a decoded chunk: what
 * `samtools fastq` (htslib's bam2fq) hands to `bwa mem`, computed on the device (csrc/bam_reads.hip).  bwams/bam_reads.py restates
 * the rules.  The result is an ordinary bwams_fastq_t: bwams_fastq_info / _has_qual / _fetch / _to_batch / _to_batch_opt / _close
 * work on it unchanged.
 *  1. Records.  Record 0 starts at byte 0, record k + 1 at start_k + 4 + block_size_k.  A record is well formed when block_size >= 32,
 *     l_read_name >= 1, l_seq >= 0, 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq <= block_size, the name's last byte is
 *     NUL and the record ends at or before n_bytes; the chain must end exactly at n_bytes.  Anything else is BWAMS_ERR_ARG, no handle
 *     is left, and bwams_last_error names the earliest bad record's ordinal and byte offset ("record K at byte Q").  refID, POS, bin,
 *     MAPQ, the mate fields and the CIGAR's content are not looked at.  The records are checked before anything of rules 2-6.
 *  2. Kept records.  Records with FLAG 0x100 or 0x800 are skipped (`samtools fastq`'s default -F 0x900); all others become reads, in
 *     record order.  *n_records counts all records, *n_reads the kept ones.
 *  3. Bases.  The 4-bit codes 1, 2, 4, 8 (A, C, G, T) become 0, 1, 2, 3, every other code 4 (nst_nt4_table of the letter).  With FLAG
 *     0x10 the read is reverse-complemented: base i of the read is 3 - c of base l_seq - 1 - i when c < 4, and 4 otherwise.
 *  4. Qualities.  QUAL + 33, reversed with 0x10.  A record whose first QUAL byte is 0xFF has none.  No kept record with qualities:
 *     bwams_fastq_has_qual = 0, as for FASTA text.  Some with and some without: BWAMS_ERR_UNSUPPORTED, naming the first kept record
 *     that differs from the first kept record.  A kept record with l_seq == 0: BWAMS_ERR_UNSUPPORTED.
 *  5. Names.  The name bytes as stored, without the NUL.  No "/<digit>" trimming (samtools would append "/1" or "/2", and bwa would
 *     strip just that).
 *  6. Comments.  tags: NULL, "", or two-letter tags back to back ("RGBCRX"); an odd length or more than 32 tags is BWAMS_ERR_ARG.
 *     For each listed tag, in list order, the record's first aux field with that tag becomes TG:T:value; the fields are joined by
 *     tabs — the form `mem -C` appends and bwams_bam_run accepts.  Types A, Z, H are copied; c / C / s / S / i / I are printed as :i:
 *     decimal.  A listed tag of type f or B is BWAMS_ERR_UNSUPPORTED.  With a non-empty list every aux field of a kept record is
 *     walked: a field of an unknown type, or one that runs past its record, is BWAMS_ERR_ARG.  No listed tag present: no comment.
 *     Within one record rule 4 is checked before rule 6; among records the earliest one decides, and bwams_last_error names it.
 *  7. No kept read at all (n_bytes == 0, or everything skipped): what bwams_fastq_decode returns for a text without records.
 * Scratch memory that does not fit is BWAMS_ERR_NOMEM and leaves nothing behind.  Inputs of 2^36 bytes or more: BWAMS_ERR_UNSUPPORTED.
 * bwams_bam_reads_info (a handle of bwams_bam_reads_decode; BWAMS_ERR_ARG otherwise): the device time of finding the records and of
 * everything behind it (measure, scans, emit), the offsets that passed the filter of the record search, and the records found. */
int bwams_bam_reads_decode(int device, const void *bam, int64_t n_bytes, const char *tags, bwams_fastq_t **out, int64_t *n_reads,
                           int64_t *n_bases, int64_t *n_records);
int bwams_bam_reads_info(const bwams_fastq_t *f, float *ms_discover, float *ms_emit, int64_t *n_candidates, int64_t *n_records);

/* ------------------------------------------------------------- read trimming ---- *
 * A decoded chunk in, an ordinary decoded chunk out (csrc/trim.hip): adapter read-through, low-quality ends and reads not worth
 * mapping leave the chunk before it reaches the batch.  `in` is left untouched; *out is a bwams_fastq_t like any other
 * (bwams_fastq_info / _has_qual / _fetch / _to_batch / _to_batch_opt / _text / _close work on it unchanged; the `ms` of bwams_fastq_info
 * is the device time of the trim's kernels and scans, without the report's copy to the host between them).  Names and comments of
 * the kept reads are copied byte for byte, in input order; has_qual is that of `in`.  The model is fastp's defaults, but no parity
 * with any tool's output is claimed: bwams/trim.py restates the rules, and the device's arrays, report and stats equal it entry for
 * entry.
 * A read is codes c[0, n) and qualities q[i] = byte - 33 (0 when the byte is below 33); code 4 is N.  With paired, reads 2k and 2k + 1
 * are the two ends.  The steps run in this order on the current read, each on what the one before left:
 *  T1 fixed.  trim_front bases leave the 5' end, trim_tail the 3' end; nothing left: the read is empty.
 *  T2 quality windows (a chunk with qualities, n > 0).  w = min(cut_window, n), S(i, j) the sum of q over [i, j).  cut_front: s is the
 *     smallest s in [0, n - w] with S(s, s + w) >= w * cut_quality; none: the read is empty; otherwise s advances while q[s] <
 *     cut_quality and the read becomes [s, n).  cut_tail, after cut_front and with w taken anew: e is the largest e in [w, n] with
 *     S(e - w, e) >= w * cut_quality; none: empty; otherwise e falls while q[e - 1] < cut_quality and the read becomes [0, e).
 *  T3 overlap (paired, overlap != 0, both ends at most BWAMS_TRIM_OVERLAP_MAX_LEN long; a longer pair skips T3 and is counted).
 *     a = end 1 (n1 bases), b = the reverse complement of end 2 (n2 bases; 4 stays 4).  A candidate insert length I pairs a[i] with
 *     b[i + n2 - I] for i in [lo, hi), lo = max(0, I - n2), hi = min(n1, I), ov = hi - lo; a position is a mismatch when the codes
 *     differ or either is 4, d counts them.  I passes when ov >= overlap_min, d <= overlap_max_diff and 100 d <= overlap_diff_pct * ov.
 *     Of all I in [overlap_min, n1 + n2 - overlap_min] the LARGEST that passes is the pair's insert; each end is cut to min(n, I)
 *     (nothing is cut when I is at least both lengths: the insert still counts as found).
 *  T4 adapter by sequence: a single read, and each end of a pair for which T3 found no insert (off, skipped, or no I passed), against
 *     adapter1 (end 1, single reads) or adapter2 (end 2); an empty adapter: no step.  With the adapter A of m letters, for p from 0 to
 *     n - adapter_min_match: cmp = min(n - p, m), d = #{k < cmp: c[p + k] != A[k] or c[p + k] == 4}; the smallest p with
 *     d * adapter_mismatch_per <= cmp cuts the read to p bases.
 *  T5 max_len > 0: n = min(n, max_len).
 *  T6 filters, per end, the first that fails being the end's reason: LEN n < min_len; N more than n_limit bases of code 4; QUAL (with
 *     qualities) 100 * #{q < qual_floor} > low_qual_pct * n.  A single read that fails is dropped; a pair is dropped when either end
 *     fails, and an end that itself passes gets the reason MATE.
 *  T7 report, one entry per read of `in`: start / len, what T1-T5 left, in the input read's coordinates (a dropped read's too; an
 *     empty read has len 0); insert, T3's I or 0 (both ends carry it); reason; removed[k], the bases step k took from this read (k:
 *     BWAMS_TRIM_STEP_*), and steps, bit k set when removed[k] > 0, BWAMS_TRIM_STEP_SKIPPED on both ends of a pair that skipped T3.
 *  T8 stats: every number is a function of the report (and the input lengths): pairs_insert counts the pairs with insert > 0,
 *     pairs_skipped those with BWAMS_TRIM_STEP_SKIPPED, step_reads[k] / step_bases[k] the reads with removed[k] > 0 and the sum of
 *     removed[k], dropped[r - 1] the reads with reason r.
 *  T9 refusals, before anything is allocated: BWAMS_ERR_ARG, bwams_last_error naming the field, for an option outside its range (the
 *     counts and limits are >= 0, cut_window is in 1..64, overlap_min / adapter_min_match / adapter_mismatch_per / min_len are >= 1),
 *     an adapter with a letter other than A, C, G, T or without a NUL in its 129 bytes, or paired with an odd number of reads.  A
 *     chunk from which nothing survives gives a valid chunk of 0 reads.  With every step off and filters that pass everything
 *     (min_len 1: an empty read never survives), *out equals `in` array for array.
 * Not built: adapter auto-detection, base correction inside the overlap, polyG / polyX tails, UMIs, fixed trims per end, chunks that
 * mix single reads and pairs (`mem -p` smart pairing), and the compiled mem_process_seqs() path (it returns one text per input read). */
#define BWAMS_TRIM_OVERLAP_MAX_LEN 1024
enum { BWAMS_TRIM_KEPT = 0, BWAMS_TRIM_LEN = 1, BWAMS_TRIM_N = 2, BWAMS_TRIM_QUAL = 3, BWAMS_TRIM_MATE = 4 };
enum { BWAMS_TRIM_STEP_FIXED = 0, BWAMS_TRIM_STEP_CUT_FRONT = 1, BWAMS_TRIM_STEP_CUT_TAIL = 2, BWAMS_TRIM_STEP_OVERLAP = 3,
       BWAMS_TRIM_STEP_ADAPTER = 4, BWAMS_TRIM_STEP_MAX_LEN = 5, BWAMS_TRIM_N_STEPS = 6 };
#define BWAMS_TRIM_STEP_SKIPPED 0x40
typedef struct bwams_trim_opt {
    int32_t trim_front, trim_tail;                                         /* T1: 0, 0 */
    int32_t cut_front, cut_tail, cut_window, cut_quality;                  /* T2: 0, 1, 4, 20 */
    int32_t overlap, overlap_min, overlap_max_diff, overlap_diff_pct;      /* T3: 1, 30, 5, 20 */
    int32_t adapter_min_match, adapter_mismatch_per;                       /* T4: 4, 8 */
    int32_t max_len;                                                       /* T5: 0 = none */
    int32_t min_len, n_limit, qual_floor, low_qual_pct;                    /* T6: 15, 5, 15, 40 */
    char adapter1[129], adapter2[129];                                     /* T4: NUL-terminated, A / C / G / T, empty = none */
    char pad_[2];
} bwams_trim_opt_t;                                                        /* 328 bytes */
typedef struct bwams_trim_read {
    int32_t start, len, insert;
    uint8_t reason, steps, pad_[2];
    int32_t removed[BWAMS_TRIM_N_STEPS];
} bwams_trim_read_t;                                                       /* 40 bytes */
typedef struct bwams_trim_stats {
    int64_t reads_in, bases_in, reads_out, bases_out, pairs_insert, pairs_skipped;
    int64_t step_reads[BWAMS_TRIM_N_STEPS], step_bases[BWAMS_TRIM_N_STEPS];
    int64_t dropped[4];                                                    /* LEN, N, QUAL, MATE */
} bwams_trim_stats_t;                                                      /* 176 bytes */
int bwams_trim_opt_default(bwams_trim_opt_t *o);
int bwams_fastq_trim(bwams_fastq_t *in, const bwams_trim_opt_t *opt, int32_t paired, bwams_fastq_t **out,
                     bwams_trim_read_t *report /* n_reads(in) entries or NULL */, bwams_trim_stats_t *stats /* or NULL */);
/* A decoded chunk as FASTQ text (`fastp -o`), in device memory owned by the handle until it is closed (a second call replaces the
 * first call's text): with qualities "@name[ comment]\nSEQ\n+\nQUAL\n" per read, without them ">name[ comment]\nSEQ\n"; the codes
 * 0..4 become ACGTN; the comment (with_comment != 0 and the read has one) follows one space.  Names are written as held: the "/1" and
 * "/2" suffixes that bwams_fastq_decode removed do not come back.  bwams_fastq_text_fetch copies the last text to the host
 * (BWAMS_ERR_CAPACITY when cap is below its size, BWAMS_ERR_ARG without a text). */
int bwams_fastq_text(bwams_fastq_t *f, int32_t with_comment, const char **d_text, int64_t *n_bytes);
int bwams_fastq_text_fetch(bwams_fastq_t *f, char *out, int64_t cap);

/* ----------------------------------------------------------- mate rescue ---- */

/* Local Smith-Waterman of mate rescue over n tasks: out[i] = ksw_align2(len2, qer + idq,
 * len1, ref + idr, 5, mat, o_del, e_del, o_ins, e_ins, xtra = pairs[i].h0, 0)
 * (src/ksw.cpp:347-381).  Replaces the body of mem_sam_pe_batch
 * (src/bwamem_pair.cpp:880-979: kswv::getScores8/16 phase 0, host-side reversal, phase 1)
 * and the scalar call in mem_matesw (src/bwamem_pair.cpp:217).  The sequence buffers are
 * not modified.  Needs oe_ins + oe_del > max(mat) - min(mat) (true for every bwa-mem
 * scoring scheme), queries <= 512 and targets <= 20000 bases (the row-maxima list of a target must fit one CU's LDS). */
int bwams_ksw_align(bwams_batch_t *b, const bwams_seqpair_t *pairs, int64_t n,
                    const uint8_t *ref, int64_t ref_bytes, const uint8_t *qer, int64_t qer_bytes,
                    const bwams_sw_opt_t *opt, bwams_kswr_t *out);

/* Test hook (not part of the drop-in surface): the device sorts (ksort.h's introsort, csrc/ksort.h) as the wave tiers run
 * them, on caller-given keys of n <= 2048 records (which = 0, 1: what the largest instance of de-duplication's wave tier keeps in
 * LDS) or n <= 1024 (which = 2); order_out[i] = index of the i-th record after the sort.  which: 0 = mem_ars2
 * (key k = re), 1 = mem_ars (s = score descending, k = rb, q = qb), both as the de-duplication kernel's wave tier sorts; 2 =
 * the chain filter's order (k = weight in [0, 2^30), descending; s and q ignored) as the many-chain reads are sorted.  mode: 0
 * = as the kernels choose (which 0, 1: rank sort, operation-exact introsort when keys tie; which 2 has no such shortcut: as
 * mode 1), 1 = the wave-parallel operation-exact introsort always, 2 = ksort.h's sequential introsort on one lane (over a copy
 * in global memory); 3 / 4 = modes 1 / 2 with a depth budget of 2, so that the comb-sort fallback of the depth limit sorts
 * nearly everything (the two must agree; the order is not ksort's). */
int bwams_debug_sort(bwams_index_t *idx, const int64_t *k, const int32_t *s, const int32_t *q, int32_t n, int32_t which,
                     int32_t mode, int32_t *order_out);

/* Test hook (not part of the drop-in surface): caller-given regions take the place of the batch's final regions of the
 * de-duplication stage.  Called after bwams_seed_upload of the reads; bwams_reg2aln_run(b, opt, 0, ...) and
 * bwams_reg2aln_fetch then run on these regions as on real ones, and the results of later stages (pairing, alignment
 * records, the EMF's regions, SAM text, BAM) count as outdated.  The chains and extension results of an earlier run stay as
 * they are: they no longer belong to these regions, and the hook is not to be mixed with entry points that read them.  regs[reg_off[r] .. reg_off[r + 1]) belong to read r.  Returns BWAMS_ERR_ARG and
 * launches nothing when n_reads is not the uploaded read count, when reg_off does not run non-decreasing from 0 to n_regs,
 * or when a region has qb < 0, qe beyond its read or qb > qe (a kernel would read outside the reads).  The reference side
 * (rb, re) and every other field go through untouched: what mem_reg2aln / bwa_gen_cigar2 reject becomes the unmapped record. */
int bwams_debug_regs_upload(bwams_batch_t *b, const bwams_alnreg_t *regs, int64_t n_regs, const int64_t *reg_off, int64_t n_reads);

/* Test hook (not part of the drop-in surface): caller-given regions take the place of the batch's regions of the extension
 * stage, in front of de-duplication.  Called after bwams_seed_upload of the reads; bwams_dedup_run and bwams_dedup_fetch then run
 * on these regions as on real ones.  The chains of an earlier run and everything downstream (final regions, pairing, alignment
 * records, the EMF's regions, SAM text, BAM) count as outdated; of the extension's own results bwams_extend_fetch returns the
 * uploaded regions with a seed_aln of zeros, and bwams_extend_tasks_fetch refuses (no task lists belong to them).  regs[reg_off[r] .. reg_off[r + 1]) are the slots of read r; a
 * slot with qe <= qb is a purged one and passes as it is (qb = qe = -1 included).  Returns BWAMS_ERR_ARG, launches nothing and
 * leaves the batch as it was when n_reads is not the uploaded read count, when reg_off does not run non-decreasing from 0 to
 * n_regs, when a live region (qe > qb) has qb < 0, qe beyond its read, rb < 0, re > 2 l_pac, re <= rb or score < 1, or when any
 * region has rid outside [-1, number of sequences).  Besides what would make a kernel read outside the reads or the text, the
 * excluded values are those on which the reference itself divides by zero or converts NaN to int (mem_patch_reg's expected
 * scores: a sum of two spans that is zero, a ratio against an expected score of zero). */
int bwams_debug_ext_regs_upload(bwams_batch_t *b, const bwams_alnreg_t *regs, int64_t n_regs, const int64_t *reg_off, int64_t n_reads);

/* Test hook (not part of the drop-in surface): what the last bwams_dedup_run on this batch did, when it ran with
 * BWAMS_DEDUP_COUNT=1 (BWAMS_ERR_ARG otherwise; a run without the variable launches kernel instances that hold no counting code).
 * Reads: counts[0] finished by the triage kernel (at most one live region), [1] by the lane tier (up to 16 slots), [2], [3],
 * [4] by the wave tier's instances for (16, 128], (128, 512] and (512, 2048] slots across the wavefront, [5] by the one-lane
 * form inside the wave kernels (more than 2048 slots, or BWAMS_DEDUP_SEQ=1).  Patch alignments (mem_patch_reg candidates that
 * pass the coordinate tests): [6] the gap-free shortcut, [7] one lane with the row in global memory, [8] the wavefront with the
 * row in LDS (queries of 256 bases and more), [9] .. [12] the wavefront with the row in registers, queries below 64, 128, 192
 * and 256 bases; [13] how many of [9] .. [12] the early exit ended. */
int bwams_debug_dedup_counts(bwams_batch_t *b, int64_t counts[14]);

/* Test hook (not part of the drop-in surface): bwams_debug_regs_upload for the pairing stage.  Called after bwams_seed_upload of
 * the reads; bwams_pair_run, bwams_pair_run_sam (all flags, BWAMS_PAIR_SINGLE_END included) and bwams_pair_fetch then run on
 * these regions as on real ones.  It does what bwams_debug_regs_upload does and refuses what that hook refuses; additionally it
 * returns BWAMS_ERR_ARG, launches nothing and leaves the batch as it was when a region has rid outside [0, number of
 * sequences), not 0 <= rb < re <= 2 l_pac, or score < 0: what would make a pairing kernel (or mem_pair itself) index outside the
 * sequence table or compute on nonsense. */
int bwams_debug_pair_regs_upload(bwams_batch_t *b, const bwams_alnreg_t *regs, int64_t n_regs, const int64_t *reg_off, int64_t n_reads);

/* Test hook (not part of the drop-in surface): the routes the last bwams_chain_run / bwams_chain_run_ert on this batch sent its
 * reads through (BWAMS_ERR_ARG when there was none, or bwams_chain_upload came after it).  Always: counts[0 .. 9] reads with more
 * seeds than the limits of class L (1700), L1 (850), M (512), M1 (256), S (128), of the lane tier (32), of class XL (4096), L2
 * (1275), M2 (665) and XL2 (13000) — seeds as chaining sees them, after the max_occ pick, skipped ones included; all ten stay 0
 * in a 256-read block without a read beyond the lane tier; [10] reads handed to the many-chain filter kernel; [11] reads the
 * ordered-array attempt gave up on (a chain position repeated: chained again with the B-tree); [12 .. 18] reads sorted and
 * filtered by a whole wavefront, by chains at or above min_chain_weight: up to 32, 64, 128, 256, 512, 960, more; [19] reads
 * beyond 3840 chains, which one lane of the filter kernel sorts and filters sequentially (not in [12 .. 18]).  Only when the run
 * had BWAMS_CHAIN_COUNT=1 (-1 otherwise: a run without the variable launches kernel instances that hold no counting code): [20]
 * reads whose sort and filter ran in the chaining wave's own LDS (part of [12 .. 18]); [21] reads one lane sorted and filtered
 * sequentially at the end of chaining (at most 16 chains); the wave tier's 64-seed passes: [22] passes, [23] seeds they
 * settled, [24] chains they started, [25] seeds taken one at a time instead.  A refused run leaves nothing to report. */
int bwams_debug_chain_counts(bwams_batch_t *b, int64_t counts[26]);

/* Test hook (not part of the drop-in surface): the lane tier of the last bwams_chain_run / bwams_chain_run_ert on this batch
 * (BWAMS_ERR_ARG when bwams_debug_chain_counts would refuse).  counts[0]: reads of at most 32 seeds, the ones without a seed
 * included — a lane each chains them with the B-tree's root leaf in registers and the chain records in LDS; counts[1]: those
 * among them that needed a tenth chain, gave that form up and were chained again, from their first seed, with the B-tree in
 * global memory.  Counted in every run. */
int bwams_debug_chain_lane_counts(bwams_batch_t *b, int64_t counts[2]);

/* Test hook (not part of the drop-in surface): what the last bwams_pair_run / bwams_pair_run_sam on this batch did, when it ran
 * with BWAMS_PAIR_COUNT=1 (BWAMS_ERR_ARG otherwise; a run without the variable launches kernel instances that hold no counting
 * code).  Mate rescue, visits of a read's list per route (a read the second pass redoes is visited in both passes and counted in
 * both; [14] says how many of the visits were the second pass's): counts[0] one lane (pool capacity = regions + 4 per anchor of
 * the mate, up to 16), [1] a wavefront with the list in LDS (capacity up to 1024), [2] one lane inside the wave kernel (capacity
 * above 1024), [3] the ERT variant (BWAMS_PAIR_USE_ERT: always one lane).  Sorts of the wave tier [1]: [4] by rank (lists up to
 * 96), [5] by the bitonic network, [6] how many of [4] + [5] found equal keys and were ended by the operation-exact introsort.
 * [7] regions inserted by the rescue, over all routes and visits.  mem_mark_primary_se, reads per route by their final region
 * count: [8] one lane (up to 24), [9] the wave instance for (24, 256], [10] the one for (256, 2048], [11] one lane inside the
 * latter (more than 2048); lists the wave instances ordered [12] by rank (up to 96), [13] by the network.  A no-rescue or
 * single-end run still sends every read through [0] .. [3] (nothing to insert), so their sum is the read count of the first pass. */
int bwams_debug_pair_counts(bwams_batch_t *b, int64_t counts[15]);

/* Test hook (not part of the drop-in surface): how many regions the last bwams_reg2aln_run gave to each of its four
 * dynamic-programming launches.  counts[0]: lane per region with a 32-column ring in LDS; counts[1]: wave per region, bands
 * of at most 63 on the first try; counts[2]: wave per region, wider bands and the regions whose retry outgrew the ring;
 * counts[3]: lane per region with the row in global memory (queries of 512 bases and more that came through 1 or 2). */
int bwams_debug_aln_lists(bwams_batch_t *b, int64_t counts[4]);

/* ------------------------------------------------------------- counters ---- */

/* Event counts of the last seed run on this batch (the same events the oracle
 * counts) and per-kernel device times from HIP events recorded
 * on the batch's stream (ms_smem_r1/r2/r3 bracket the search kernel of that round
 * alone).  Synchronises. */
typedef struct bwams_stats {
    int64_t n_ext;            /* backwardExt evaluations */
    int64_t n_ext_blocks;     /* CP_OCC blocks they touch: 1 when k and k+s share a block, else 2 */
    int64_t n_sa_lookups;     /* suffix-array rows looked up */
    int64_t n_lf_steps;       /* LF steps the REFERENCE walks for them (to its 1/8 samples): the same number whether the lookup
                                 walked them or read them from the index's dense table (BWAMS_SA_DENSE) */
    int64_t n_smem[3];        /* SMEMs from round 1, 2, 3 */
    int64_t bsw_cells;        /* DP cells actually computed by the last bsw run.  With the packed kernel's early exit (on in bwams_extend_run
                                 unless BWAMS_BSW_EARLY=0; in bwams_bsw_run only with BWAMS_BSW_EARLY=1) a task stops once no later row can
                                 change its six outputs, so the count lies below that of scalarBandedSWA's full walk */
    int64_t n_ext_round[3];   /* n_ext split by round */
    int64_t n_blk_round[3];   /* n_ext_blocks split by round */
    float   ms_smem_r1, ms_smem_r2, ms_smem_r3, ms_sort, ms_sal, ms_seed_total;
    float   ms_bsw;
    float   ms_ksw;
    float   ms_tasks;
    float   ms_emf;
    int64_t emf_nodes;        /* EMF probe: seed entries visited */
    int64_t emf_cmp_bytes;    /* EMF probe: reference bytes compared */
    /* chaining / chain-to-alignment (last bwams_chain_run / bwams_extend_run) */
    int64_t n_chains, n_chain_seeds;
    int64_t n_left, n_right;              /* extension tasks built */
    int64_t n_retry_left, n_retry_right;  /* tasks re-run at twice the band width */
    float   ms_chain, ms_ext_plan, ms_ext_left, ms_ext_right, ms_ext_purge, ms_ext_total;   /* left/right/purge: first round */
    int64_t n_ext_rounds;                 /* extension rounds of the last bwams_extend_run */
    int64_t n_final_regs;                 /* regions left by the last bwams_dedup_run */
    float   ms_dedup;
    float   ms_pair;                      /* last bwams_pair_run, all of it */
    int64_t n_pair_tasks;                 /* rescue alignments (ksw_align2 calls) of the last bwams_pair_run */
    int64_t n_pair_redone;                /* reads whose rescue was redone with every orientation planned */
    int64_t n_pair_regs;                  /* regions after rescue */
    int64_t n_chain_redo;                 /* reads of the last chaining run in which a chain position repeated: chained again
                                           * with the exact B-tree instead of the ordered array */
    /* last bwams_seed_run_ert: events of the walk kernel (ms_smem_r1 = that kernel, ms_smem_r2 = the three rounds over the
     * profiles, ms_smem_r3 = locating the seeds' hits, ms_sal = locating + listing the hits) */
    int64_t ert_kmer_lookups;             /* 8-byte k-mer table entries read */
    int64_t ert_node_reads;               /* tree records decoded (x-mer entry, node head, leaf record / pointer) */
    int64_t ert_ref_bytes;                /* .0123 bytes compared by leaf expansion */
} bwams_stats_t;
int bwams_batch_stats(bwams_batch_t *b, bwams_stats_t *out);

/* ------------------------------------------------------------------------- *
 * ERT seeding: replaces the per-read block of mem_kernel1_core_ert (src/bwamem.cpp:1122-1193: get_seeds /
 * get_seeds_prefix, reseed / reseed_prefix, last, ks_introsort) and the hit sampling of mem_chain_new
 * (src/bwamem.cpp:993-1004), for a whole chunk.
 * ------------------------------------------------------------------------- */
typedef struct bwams_ert bwams_ert_t;

/* The two files `bwa-mem2 index -a ert` writes (src/ertindex.cpp:773-943), as host arrays: kmer_table = 4^kmer_size
 * 8-byte entries, mlt_table = the radix trees.  kmer_size / xmer_size / read_len are the build's kmerSize (15),
 * xmerSize (4) and READ_LEN (src/macro.h:204-206, :66); other values exist for test-sized indexes.  The index handle
 * must hold the .0123 reference (leaf expansion reads it).  The tables are copied into HBM. */
int bwams_ert_from_host(bwams_index_t *idx, const uint64_t *kmer_table, int32_t kmer_size, int32_t xmer_size,
                        int32_t read_len, const uint8_t *mlt_table, int64_t mlt_bytes, bwams_ert_t **out);
/* The same from <prefix>.kmer_table and <prefix>.mlt_table (kmerSize 15, xmerSize 4), streamed into HBM. */
int bwams_ert_open(bwams_index_t *idx, const char *prefix, int32_t read_len, bwams_ert_t **out);
/* Builds the two tables on the GPU from the resident FM-index (replaces buildKmerTrees, src/ertindex.cpp:773-943):
 * the same bytes the reference writes for kmerSize = kmer_size, xmerSize = xmer_size, readLength = read_len and
 * HIT_THRESHOLD = hit_threshold (15, 4, READ_LEN, 256 in src/macro.h).  The index must hold its .0123 reference. */
/* BWAMS_ERR_UNSUPPORTED for a text the format cannot hold (and the reference's writer does not finish on): a string of read_len bases
 * with 65536 occurrences or more (16-bit leaf counts, ertindex.cpp:336-352), a k-mer whose tree reaches 64 MiB (26-bit pointers, :452) */
int bwams_ert_build(bwams_index_t *idx, int32_t kmer_size, int32_t xmer_size, int32_t read_len, int32_t hit_threshold,
                    bwams_ert_t **out);
/* geometry, tree bytes and the build's kernel times (sizes, scan + allocation, bytes; 0 when loaded) */
int bwams_ert_info(const bwams_ert_t *ert, int32_t *kmer_size, int32_t *xmer_size, int32_t *read_len, int64_t *mlt_bytes,
                   float build_ms[3]);
/* copies the tables to the host (either pointer may be NULL) / writes <prefix>.kmer_table and <prefix>.mlt_table */
int bwams_ert_fetch(bwams_ert_t *ert, uint64_t *kmer_table, uint8_t *mlt_table);
int bwams_ert_save(bwams_ert_t *ert, const char *prefix);
int bwams_ert_close(bwams_ert_t *ert);
int64_t bwams_ert_bytes(const bwams_ert_t *ert);
/* The walk's resident entry + tree-head table (64 B per k-mer, derived from the two tables when the handle is made unless BWAMS_ERT_FAT=0:
 * a walk's entry and first records are one line): on = 0 gives its memory back — 64 GiB at k = 15, which a GPU that also holds the EMF
 * wants for its chunks in flight —, on = 1 derives it again.  The results do not depend on it. */
int bwams_ert_set_fat(bwams_ert_t *ert, int32_t on);

/* bwams_seed_run over the ERT instead of the FM-index: same inputs (bwams_seed_upload), same outputs
 * (bwams_seed_counts / bwams_seed_fetch, then bwams_chain_run): the SMEMs of the three seeding rounds in
 * (rid, m, n) order with s = number of hits (k and l are 0: there is no BWT interval), and the sampled hit
 * positions where the FM path puts the suffix-array coordinates.  BWAMS_ERR_UNSUPPORTED when
 * min_seed_len < kmer_size + xmer_size, when split_width + 1 or max_mem_intv exceed 20 (the trees store hit counts
 * below 20 only, src/ertindex.cpp:455-461) or when a read is longer than read_len / 255 bases.
 *
 * Against mem_kernel1_core_ert (bwamem.cpp:1122-1193; restated function by function in oracle/ert_walk_oracle.c): the same MEMs and,
 * per MEM, the same sampled hit coordinates — also for MEMs found by the backward walk and for hits > max_occ, because the
 * reference re-gathers those hits in forward (= suffix-array) order (ertseeding.cpp:644-648) — with ONE exception: a read whose
 * placement at a hit would cross the junction of the forward and the reverse-complement strand of the text.  There get_seq
 * (ertseeding.cpp:455-472) returns nothing and the reference emits matches that are not maximal; this call follows FM-index
 * seeding (the true SMEMs).  Seeds that bridge the junction are dropped by bns_intv2rid in chaining either way. */
int bwams_seed_run_ert(bwams_batch_t *b, bwams_ert_t *ert, const bwams_seed_opt_t *opt, int with_sa);

/* ------------------------------------------------------------------------- *
 * Chaining and chain-to-alignment: replace, for a whole chunk,
 *   mem_chain_seeds + mem_chain_flt (+ the short-read early-out of mem_flt_chained_seeds),
 *     called from mem_kernel1_core, src/bwamem.cpp:1341-1372
 *   mem_chain2aln_across_reads_V2, src/bwamem.cpp:2773-3760, called from mem_kernel2_core
 * ------------------------------------------------------------------------- */

/* The reference sequences of the index (bntseq_t::anns: offset, len, is_alt), needed by
 * bns_intv2rid / bns_fetch_seq_v2.  Without this call the index is one sequence [0, l_pac). */
int bwams_index_set_contigs(bwams_index_t *idx, const bwams_contig_t *contigs, int32_t n_seqs);

/* Chain the seeds the last bwams_seed_run(with_sa = 1) left on the device and filter the chains.
 * Results stay resident; counts are returned.  For reads long enough (5.5 ln L <= 0.05 L, L >= ~1100)
 * mem_flt_chained_seeds' re-scoring of short seeds (mem_seed_sw -> ksw_align2) runs as well; that step
 * needs the index's .0123 reference and, like bwams_ksw_align, oe_ins + oe_del > max(mat) - min(mat). */
int bwams_chain_run(bwams_batch_t *b, const bwams_mem_opt_t *opt, int64_t *n_chains, int64_t *n_seeds);
/* ERT mode: the same stage fed by the reference's ERT walk instead of the FM-index seeding.  Replaces, in
 * mem_kernel1_core_ert (src/bwamem.cpp:1193-1203), ks_introsort(mem_smem_sort_lt) + mem_chain_new (:961-1050) +
 * mem_chain_flt + mem_flt_chained_seeds for the whole chunk; the walk itself (get_seeds / reseed / last,
 * src/ertseeding.cpp) is not built here and stays on the host.  mems: the walk's mem_t records as it leaves them
 * (unsorted), grouped by read (mem_off[nseq + 1]); hits: the reads' hit arrays back to back (hit_off[nseq + 1];
 * mem.hitbeg is relative to its read's slice).  The reads must have been uploaded (bwams_seed_upload).  Results as
 * for bwams_chain_run: bwams_chain_fetch, bwams_extend_run, ... */
int bwams_chain_run_ert(bwams_batch_t *b, const bwams_mem_opt_t *opt, const bwams_ert_mem_t *mems, const int64_t *mem_off,
                        const uint64_t *hits, const int64_t *hit_off, int64_t *n_chains, int64_t *n_seeds);
/* chains grouped by read (chain_off[nseq + 1]) in mem_chain_flt's output order; the seeds of
 * chain c are seeds[c.seed_off .. + c.n) in the order mem_chain_seeds appended them. */
int bwams_chain_fetch(bwams_batch_t *b, bwams_chain_t *chains, int64_t chain_cap, bwams_chain_seed_t *seeds,
                      int64_t seed_cap, int64_t *chain_off);
/* Host-input variant for a caller that keeps chaining on the host: upload chain_ar. */
int bwams_chain_upload(bwams_batch_t *b, const bwams_chain_t *chains, int64_t n_chains, const bwams_chain_seed_t *seeds,
                       int64_t n_seeds, const int64_t *chain_off);

/* Build the extension tasks of the resident chains (phase 1 of mem_chain2aln_across_reads_V2);
 * bwams_extend_run then extends left (band w, retry at 2w), right (h0 = left score), settles the
 * regions and purges covered seeds.  One region per seed, grouped by read (reg_off[nseq + 1]). */
int bwams_extend_build(bwams_batch_t *b, const bwams_mem_opt_t *opt, int64_t *n_left, int64_t *n_right);
int bwams_extend_run(bwams_batch_t *b, const bwams_mem_opt_t *opt, int64_t *n_regs);
int bwams_extend_fetch(bwams_batch_t *b, bwams_alnreg_t *regs, int64_t reg_cap, int64_t *reg_off, int32_t *seed_aln);
/* The tail of mem_kernel2_core (src/bwamem.cpp:1446-1481) on the regions of bwams_extend_run: purged regions
 * dropped, mem_sort_dedup_patch (redundant hits removed, colinear neighbours merged by mem_patch_reg's global
 * alignment, identical hits removed; result ordered by score, rb, qb), the ALT mark.  Needs mask_level_redun in
 * the options.  The extension's regions stay available to bwams_extend_fetch. */
int bwams_dedup_run(bwams_batch_t *b, const bwams_mem_opt_t *opt, int64_t *n_regs);
int bwams_dedup_fetch(bwams_batch_t *b, bwams_alnreg_t *regs, int64_t reg_cap, int64_t *reg_off);
/* mem_perfect2reg with get_perfect_locations and perfect_dedup_patch (src/perfect_map.cpp:659-869), for every read
 * the last bwams_emf_run resolved (code FW_MATCHED / RC_MATCHED): all its exact locations as full-length regions
 * (grouped by read, reg_off[nseq + 1]); first_is_rev[r] = mem_perfect2reg's return value (strand of the first one). */
int bwams_emf_regs_run(bwams_batch_t *b, bwams_emf_t *emf, const bwams_mem_opt_t *opt, int64_t *n_regs);
/* Paired-end chunks: worker_sam gives an end the EMF resolved its regions (mem_perfect2reg, src/bwamem.cpp:1689-1702) before mem_sam_pe.
 * After bwams_dedup_run (and bwams_pestat: mem_pestat ran before, on the regions of worker_aln alone) this appends the regions of
 * bwams_emf_regs_run to the final regions of their reads; bwams_pair_run and what follows then see both. */
int bwams_emf_regs_merge(bwams_batch_t *b, int64_t *n_regs);
int bwams_emf_regs_fetch(bwams_batch_t *b, bwams_alnreg_t *regs, int64_t reg_cap, int64_t *reg_off, uint8_t *first_is_rev);

/* mem_pestat (src/bwamem_pair.cpp:89-156; called at src/bwamem.cpp:1888) over the final regions of
 * bwams_dedup_run: reads 2i and 2i+1 are the two ends of pair i.  pes[4] = orientations FF, FR, RF, RR.
 * The per-pair work (cal_sub, mem_infer_dir) and the sort run on the device; the percentile / mean / std
 * arithmetic over the sorted insert sizes is the reference's sequential double-precision loop, on the host. */
int bwams_pestat(bwams_batch_t *b, const bwams_mem_opt_t *opt, bwams_pestat_t pes[4]);
/* The same in two halves, for a chunk whose pairs are sharded over several batches / GPUs: mem_pestat is a statistic
 * of the WHOLE chunk, the one step of the path where shards exchange data.  bwams_pestat_keys returns one key per
 * qualifying pair of this batch (orientation << 60 | insert size; n_keys <= nseq / 2, BWAMS_ERR_CAPACITY if cap is
 * smaller); the caller concatenates the keys of all shards (an all-gather) and every shard calls
 * bwams_pestat_from_keys (host only, any order of keys) on the union: bit-identical to the unsharded result. */
int bwams_pestat_keys(bwams_batch_t *b, const bwams_mem_opt_t *opt, uint64_t *keys, int64_t cap, int64_t *n_keys);
int bwams_pestat_from_keys(const uint64_t *keys, int64_t n, bwams_pestat_t pes[4]);
/* The paired-end tail of worker_sam up to the pairing decision, for the chunk whose final regions bwams_dedup_run
 * left on the device (reads 2p and 2p + 1 = the ends of pair p):
 *   - mate rescue: mem_sam_pe_batch_pre -> mem_matesw_batch_pre (src/bwamem_pair.cpp:838-870, :1193-1355: anchors
 *     scoring within pen_unpaired of an end's best hit, at most max_matesw; one window per orientation that is not
 *     failed and has no consistent hit yet), the batched ksw_align2 of mem_sam_pe_batch (:880-979), and
 *     mem_sam_pe_batch_post -> mem_matesw_batch_post (:981-1042, :1497-1601: insertion by score and
 *     mem_sort_dedup_patch(opt, 0, 0, 0, ..) after each alignment), or its useErt form (BWAMS_PAIR_USE_ERT);
 *   - mem_mark_primary_se (src/bwamem.cpp:1905-1980) of both ends with ids (id_base + p) << 1 | end;
 *   - mem_pair (src/bwamem_pair.cpp:366-427) when both ends have a primary hit.
 * pes[4] is mem_pestat's result (bwams_pestat) or the caller's (-I); id_base = n_processed >> 1 of the chunk.
 * flags: BWAMS_PAIR_* below.  bwams_pair_fetch returns the regions per read as mem_sam_pe_batch_post holds them
 * before its MAPQ / SAM part (grouped by read, reg_off[nseq + 1]) and one bwams_pair_t per pair.
 * The insert-size term of mem_pair is double arithmetic through log / erfc of the device math library. */
#define BWAMS_PAIR_NO_RESCUE 1   /* MEM_F_NO_RESCUE */
#define BWAMS_PAIR_SINGLE_END 4  /* single-end chunk: just mem_mark_primary_se(opt, n, a, id_base + read) of every read, as mem_reg2sam
                                    does (src/bwamem.cpp:2318-2330); pes may be NULL, no rescue, no pairing, any number of reads */
#define BWAMS_PAIR_USE_ERT   2   /* mem_sam_pe_batch_post's useErt branch (ERT-mode runs): the mate's list is sorted by end
                                  * position, rescue goes through mem_matesw_batch_post_ert (insertion by end, mem_dedup_patch),
                                  * and one mem_sort_dedup_patch or score sort closes each end (src/bwamem_pair.cpp:1017-1041) */
int bwams_pair_run(bwams_batch_t *b, const bwams_mem_opt_t *opt, const bwams_pestat_t pes[4], int64_t id_base, int32_t flags,
                   int64_t *n_regs, int64_t *n_tasks);
/* The same with the flags of mem_opt_t that act between the marking and the SAM text taken from sam_opt->flag:
 *   - MEM_F_PRIMARY5 (`mem -5`): mem_reorder_primary5(sam_opt->T, a) (src/bwamem.cpp:2009-2031) of every read right after
 *     mem_mark_primary_se — in mem_sam_pe before mem_pair (src/bwamem_pair.cpp:1060-1063), in worker_sam's single-end branch
 *     before mem_reg2sam (src/bwamem.cpp:1840);
 *   - MEM_F_NOPAIRING (`mem -P`): mem_pair is not called (src/bwamem_pair.cpp:1066): score 0, z = -1 in every bwams_pair_t;
 *   - MEM_F_NO_RESCUE (`mem -S`): as BWAMS_PAIR_NO_RESCUE.
 * sam_opt == NULL is bwams_pair_run. */
int bwams_pair_run_sam(bwams_batch_t *b, const bwams_mem_opt_t *opt, const bwams_sam_opt_t *sam_opt, const bwams_pestat_t pes[4],
                       int64_t id_base, int32_t flags, int64_t *n_regs, int64_t *n_tasks);
int bwams_pair_fetch(bwams_batch_t *b, bwams_alnreg_t *regs, int64_t reg_cap, int64_t *reg_off, bwams_pair_t *pairs);
/* the task lists as built (side 0 = left, 1 = right), for inspection */
int bwams_extend_tasks_fetch(bwams_batch_t *b, int32_t side, bwams_seqpair_t *pairs, int64_t pair_cap, uint8_t *ref,
                             int64_t ref_cap, uint8_t *qer, int64_t qer_cap, int64_t *n_pairs, int64_t *ref_bytes,
                             int64_t *qer_bytes);

int bwams_batch_sync(bwams_batch_t *b);

/* -------------------------------------------------------- the outer boundary ---- *
 * One chunk, text to text: what kt_pipeline's step 0 parsing (bseq_read_orig, src/bwa.cpp:266-335) and step 1 (mem_process_seqs,
 * src/bwamem.cpp:1850-1980: worker_bwt, worker_aln, mem_pestat, worker_sam) do between the decompressed FASTQ bytes of whole records and
 * seqs[i].sam — the sequence of the stage calls of this header.  fastq: host or device memory, four lines per
 * record, the two ends of a pair interleaved when paired != 0; emf / ert: NULL or the resident tables (ert selects ERT seeding and the
 * useErt form of mate rescue); pes0: NULL = infer the insert-size statistics from the chunk (mem_pestat), as mem_process_seqs does;
 * n_processed: reads processed before this chunk (the hash seeds of mem_mark_primary_se / mem_pair); flags: BWAMS_PAIR_NO_RESCUE
 * (MEM_F_NO_RESCUE) and BWAMS_CHUNK_COPY_COMMENT (`mem -C`: without it the comments of the FASTQ headers are dropped, src/fastmap.cpp:335-342).
 * sam_opt->flag carries the reference's MEM_F_* bits: MEM_F_ALL / NO_MULTI / SOFTCLIP / KEEP_SUPP_MAPQ / REF_HDR act in the text, MEM_F_PRIMARY5 /
 * NOPAIRING / NO_RESCUE before it (bwams_pair_run_sam); MEM_F_PE and MEM_F_SMARTPE are the caller's choice of entry point (paired, _smart).
 * The text stays on the device: bwams_sam_fetch(b, buf, sam_bytes, read_off, NULL, 0) returns it with one offset per read.  The batch must
 * have been created for at least the chunk's reads and bases, the index must carry its sequence names.  Inputs the device path refuses
 * (multi-line FASTQ records, unsupported flags) return BWAMS_ERR_UNSUPPORTED: run that chunk on the host. */
int bwams_process_chunk(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo,
                        const bwams_sam_opt_t *sam_opt, const char *fastq, int64_t n_bytes, int32_t paired, const bwams_pestat_t *pes0,
                        int64_t n_processed, int32_t flags, int64_t *n_reads, int64_t *sam_bytes);
/* The paired-end chunk as two texts (`bwa mem ref R1.fq R2.fq`: bseq_read_orig with a second file, src/bwa.cpp:275-318): record k of
 * fastq1 and record k of fastq2 are the ends of pair k.  Both texts must hold the same number of records (the caller cuts the two files at
 * the same record; the reference stops with a warning when one file runs out). */
int bwams_process_chunk2(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo,
                         const bwams_sam_opt_t *sam_opt, const char *fastq1, int64_t n_bytes1, const char *fastq2, int64_t n_bytes2,
                         const bwams_pestat_t *pes0, int64_t n_processed, int32_t flags, int64_t *n_reads, int64_t *sam_bytes);
/* process()'s MEM_F_SMARTPE branch (`mem -p`, src/fastmap.cpp:378-414): the chunk may mix reads that stand alone with interleaved
 * pairs.  bseq_classify (src/bwa.cpp:346-362: two neighbours carrying one name are a pair, taken greedily from the left) splits it;
 * the single reads go through mem_process_seqs as single-end with ids from n_processed, the pairs as paired-end with ids from
 * n_processed + *n_single and pes0; every read's text returns to its place.  bwams_sam_fetch(b, buf, sam_bytes, read_off, NULL, 0)
 * returns the merged text with *n_reads + 1 offsets (no per-region MAPQ after a merge). */
int bwams_process_chunk_smart(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo,
                              const bwams_sam_opt_t *sam_opt, const char *fastq, int64_t n_bytes, const bwams_pestat_t *pes0,
                              int64_t n_processed, int32_t flags, int64_t *n_reads, int64_t *n_single, int64_t *sam_bytes);
#define BWAMS_CHUNK_COPY_COMMENT 0x100
/* bwams_process_chunk / _chunk_smart with bwams_bam_reads_decode in place of bwams_fastq_decode: bam[0, n_bytes) are whole BAM records
 * (host or device memory, no header block), tags as for bwams_bam_reads_decode (the comments reach the SAM text only with
 * BWAMS_CHUNK_COPY_COMMENT).  With paired, kept reads 2k and 2k + 1 are the two ends, in file order — what `samtools fastq | bwa mem -p`
 * does; a coordinate-sorted BAM is collated first (`samtools collate`) by bwams_collate_t below, whose `pairs` output in device memory
 * is such input.  Everything behind the decode is bwams_process_chunk's. */
int bwams_process_chunk_bam(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo,
                            const bwams_sam_opt_t *sam_opt, const void *bam, int64_t n_bytes, const char *tags, int32_t paired,
                            const bwams_pestat_t *pes0, int64_t n_processed, int32_t flags, int64_t *n_reads, int64_t *sam_bytes);
int bwams_process_chunk_bam_smart(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo,
                                  const bwams_sam_opt_t *sam_opt, const void *bam, int64_t n_bytes, const char *tags,
                                  const bwams_pestat_t *pes0, int64_t n_processed, int32_t flags, int64_t *n_reads, int64_t *n_single,
                                  int64_t *sam_bytes);
/* bwams_process_chunk behind its decode, for a chunk the caller decoded (bwams_fastq_decode, bwams_bam_reads_decode) and perhaps
 * trimmed (bwams_fastq_trim): decode, then trim, then map.  fq is consumed: closed here whatever the outcome.  paired is 0 or 1 (no
 * smart pairing of a decoded chunk).  *n_reads: the reads of fq.  n_processed counts the reads that reached the mapper before this
 * chunk: after trimming, the KEPT reads of the chunks before (the reads the text numbers), not the reads of the input files. */
int bwams_process_chunk_decoded(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo,
                                const bwams_sam_opt_t *sam_opt, bwams_fastq_t *fq /* consumed */, int32_t paired, const bwams_pestat_t *pes0,
                                int64_t n_processed, int32_t flags, int64_t *n_reads, int64_t *sam_bytes);

/* mem_process_seqs (src/bwamem.cpp:1850-1903) for a chunk that arrives the way the reference hands it over: parsed records (bseq1_t:
 * name, comment, seq, qual — src/bwa.h:76-86), here as flat arrays — enc_qdb / cum_len as bwams_seed_upload takes them, names (NUL
 * terminated or not: name_off[i + 1] - name_off[i] bytes each), quals (cum_len's layout, NULL when the reads carry none) and comments as
 * bwams_sam_upload takes them.  The compiled caller with the reference's own signature is bwa-mem-scale_amd/host/mem_process_seqs_hip.cpp.
 * Text out as bwams_process_chunk: bwams_sam_fetch. */
int bwams_process_reads(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo,
                        const bwams_sam_opt_t *sam_opt, const uint8_t *enc_qdb, const int64_t *cum_len, int64_t n_reads, const char *names,
                        const int64_t *name_off, const char *quals, const char *comments, const int64_t *comment_off, int32_t paired,
                        const bwams_pestat_t *pes0, int64_t n_processed, int32_t flags, int64_t *sam_bytes);
/* The same in two halves, for a chunk sharded over several batches (one per GPU; host/chunk_multi.cpp drives them): stage 1 = worker_bwt +
 * worker_aln (up to the regions mem_pestat reads); the caller merges the shards' bwams_pestat_keys with bwams_pestat_from_keys — mem_pestat
 * is a statistic of the WHOLE chunk (bwamem.cpp:1881-1891); stage 2 = worker_sam with the chunk's statistics and the shard's first read id
 * (single-end: n_processed + reads in front of the shard) or pair id (paired-end: (n_processed >> 1) + pairs in front of it). */
int bwams_process_reads_stage1(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo,
                               const uint8_t *enc_qdb, const int64_t *cum_len, int64_t n_reads, const char *names, const int64_t *name_off,
                               const char *quals, const char *comments, const int64_t *comment_off);
int bwams_process_reads_stage2(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_mem_opt_t *mo, const bwams_sam_opt_t *sam_opt,
                               int32_t paired, const bwams_pestat_t *pes, int64_t id_base, int32_t flags, int64_t *sam_bytes);
/* Stage 1 in two halves (bwams_process_reads_stage1 == _upload + _stage1_run): what crosses PCIe, and what computes.  A pipeline puts chunk
 * i + 1 into one batch while another batch of the same device runs chunk i (the reference overlaps reading, computing and writing of
 * consecutive chunks with its `-i` pipeline threads, src/fastmap.cpp:307-468; host/chunk_multi.cpp does the same over batches). */
int bwams_process_reads_upload(bwams_batch_t *b, const uint8_t *enc_qdb, const int64_t *cum_len, int64_t n_reads, const char *names,
                               const int64_t *name_off, const char *quals, const char *comments, const int64_t *comment_off);
int bwams_process_reads_stage1_run(bwams_batch_t *b, bwams_emf_t *emf, bwams_ert_t *ert, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo);
int bwams_batch_device(const bwams_batch_t *b, int32_t *device);      /* the device of the batch's index */
/* One chunk over n batches — one per GPU, each on a replica of the index — behind one call (host/chunk_multi.cpp): the chunk is cut into n
 * contiguous shards on read (paired-end: pair) boundaries (bwams_shard_bounds: sizes differ by at most one unit, larger shards first), one
 * host thread drives each batch through stage 1, the shards' pestat keys are merged in-process (no collective), stage 2 runs per shard with
 * the chunk's statistics and the shard's first id, and bwams_multi_fetch returns the text in read order with n_reads + 1 offsets.
 * emf / ert: NULL, or one handle per batch (on that batch's device).  Results are byte-identical to one batch processing the whole chunk. */
typedef struct bwams_multi bwams_multi_t;
int bwams_shard_bounds(int64_t n_reads, int32_t n_shards, int32_t paired, int64_t *bounds /* n_shards + 1 */);
int bwams_multi_create(bwams_batch_t *const *batches, bwams_emf_t *const *emf, bwams_ert_t *const *ert, int32_t n, bwams_multi_t **out);
int bwams_multi_process_reads(bwams_multi_t *m, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo, const bwams_sam_opt_t *sam_opt,
                              const uint8_t *enc_qdb, const int64_t *cum_len, int64_t n_reads, const char *names, const int64_t *name_off,
                              const char *quals, const char *comments, const int64_t *comment_off, int32_t paired, const bwams_pestat_t *pes0,
                              int64_t n_processed, int32_t flags, int64_t *sam_bytes);
int bwams_multi_fetch(bwams_multi_t *m, char *sam, int64_t cap, int64_t *read_off);
/* bwams_multi_process_reads in its two halves: _upload cuts the chunk and puts every shard into its batch (the shards' threads, side by
 * side; nothing computes), _compute runs stage 1, the pestat merge and stage 2.  With two bwams_multi over the same devices a caller
 * uploads chunk i + 1 through one while the other computes chunk i (host/mem_process_seqs_hip.cpp: mem_process_seqs_stage / _collect). */
int bwams_multi_upload(bwams_multi_t *m, const uint8_t *enc_qdb, const int64_t *cum_len, int64_t n_reads, const char *names,
                       const int64_t *name_off, const char *quals, const char *comments, const int64_t *comment_off, int32_t paired);
int bwams_multi_compute(bwams_multi_t *m, const bwams_seed_opt_t *so, const bwams_mem_opt_t *mo, const bwams_sam_opt_t *sam_opt,
                        const bwams_pestat_t *pes0, int64_t n_processed, int32_t flags, int64_t *sam_bytes);
const char *bwams_multi_error(const bwams_multi_t *m);       /* which shard failed, and why */
int bwams_multi_destroy(bwams_multi_t *m);
/* The file ends of the pipeline (host/fastq_io.cpp).  bwams_reader: a background thread inflates a gz or plain FASTQ / FASTA file (zlib,
 * as the reference's kseq over gzFile) into n_buffers page-locked chunk buffers and cuts chunks where bseq_read_orig cuts them
 * (src/bwa.cpp:266-335): records until the chunk holds chunk_bases bases and, paired, an even number of reads — chunk i holds exactly
 * the reads of the reference's chunk i with the same -K.  _next returns 0 and the chunk (text of whole records; feed it to
 * bwams_process_chunk, or to bwams_bseq_parse + mem_process_seqs), 1 at the end of the file, < 0 on an error (_error says what);
 * the buffer is the caller's until _release.  buffer_bytes 0: 3 bytes per base + 64 MiB.
 * bwams_writer: n_shards output streams ("<path>.<s>.sam"; one stream = `path` itself), each written by its own thread in
 * sequence-number order — the per-GPU output shards behind a sharded job, or the one SAM stream of step 2 (src/fastmap.cpp:437-461). */
typedef struct bwams_reader bwams_reader_t;
typedef struct bwams_writer bwams_writer_t;
int bwams_reader_open(const char *path, int64_t chunk_bases, int32_t paired, int64_t buffer_bytes, int32_t n_buffers, bwams_reader_t **out);
int bwams_reader_next(bwams_reader_t *r, const char **text, int64_t *n_bytes, int64_t *n_reads, int64_t *n_bases);
int bwams_reader_release(bwams_reader_t *r, const char *text);
const char *bwams_reader_error(const bwams_reader_t *r);
int bwams_reader_close(bwams_reader_t *r);
/* The same reader, with a BGZF file inflated on `device` (bwams_inflater_run into the chunk buffer; read(2) into page-locked
 * staging): chunks byte-identical to bwams_reader_open's.  Any other file (plain gzip, uncompressed) is read exactly as
 * bwams_reader_open reads it, and bwams_reader_info says device_inflate = 0.  The reader's own thread sets the device. */
int bwams_reader_open_device(const char *path, int device, int64_t chunk_bases, int32_t paired, int64_t buffer_bytes,
                             int32_t n_buffers, bwams_reader_t **out);
/* bwams_reader_open_device with flags.  BWAMS_READER_GUNZIP: a gzip file that is not BGZF is inflated on `device` too
 * (bwams_gunzip_run into the chunk buffer), and bwams_reader_info says device_inflate = 2; the chunks are the same bytes.  flags = 0:
 * bwams_reader_open_device exactly. */
#define BWAMS_READER_GUNZIP 0x1
int bwams_reader_open_device2(const char *path, int device, int64_t chunk_bases, int32_t paired, int64_t buffer_bytes,
                              int32_t n_buffers, uint32_t flags, bwams_reader_t **out);
typedef struct bwams_reader_stats {
    int32_t device_inflate;                      /* 1: BGZF on the GPU; 2: plain gzip on the GPU; 0: zlib on the reader's thread */
    int64_t in_bytes, out_bytes;                 /* file bytes read so far, text bytes inflated so far */
    float ms_read, ms_inflate;                   /* reader thread: read(2) (device path only), inflate */
} bwams_reader_stats_t;
int bwams_reader_info(const bwams_reader_t *r, bwams_reader_stats_t *out);
/* A BAM file as read input: BGZF inflated on `device` as bwams_reader_open_device inflates it (device < 0: zlib on the reader's thread,
 * gzread reads BGZF).  Open parses the header block (magic, l_text, text, n_ref, the references; it may span many members) before the
 * reader's thread starts: a wrong magic is BWAMS_ERR_UNSUPPORTED, a header cut off by the end of the file BWAMS_ERR_IO.
 * bwams_reader_next returns whole BAM records (no header) for bwams_process_chunk_bam / bwams_bam_reads_decode; n_reads counts the
 * kept records (neither 0x100 nor 0x800), n_bases is the sum of their l_seq.  The cut is bwams_reader_open's, evaluated right after
 * each kept record (skipped records that follow go to the next chunk): chunk i holds exactly the reads of chunk i of
 * bwams_reader_open over the equivalent FASTQ.  A record that is not well formed (rule 1 of bwams_bam_reads_decode) is BWAMS_ERR_IO,
 * with its ordinal in bwams_reader_error.  bwams_reader_bam_header: the header text (not NUL terminated; it lives as long as the
 * reader — its @RG lines may go into bwams_sam_header's hdr_line) and the number of references; BWAMS_ERR_ARG for a reader of text.
 * The mem_process_seqs / bwams_bseq_parse path stays FASTQ-only. */
int bwams_reader_open_bam(const char *path, int device, int64_t chunk_bases, int32_t paired, int64_t buffer_bytes, int32_t n_buffers,
                          bwams_reader_t **out);
int bwams_reader_bam_header(const bwams_reader_t *r, const char **text, int64_t *n_text, int32_t *n_ref);
int bwams_writer_open(const char *path, int32_t n_shards, bwams_writer_t **out);
int bwams_writer_put(bwams_writer_t *w, int32_t shard, int64_t seq, const char *text, int64_t n_bytes);
int bwams_writer_close(bwams_writer_t *w);       /* waits until everything handed over in order is on disk */
/* A BGZF writer: shards named as bwams_writer_open names them, with ".sam.gz" in place of ".sam".  Every shard's thread owns a deflater
 * on `device` and compresses the text of each bwams_writer_put (a put's members never span into the next put);
 * bwams_writer_put_bgzf hands over members already made (e.g. by bwams_sam_fetch_bgzf, without the EOF member), written in the same
 * sequence order.  bwams_writer_close appends the EOF member to every shard. */
int bwams_writer_open_bgzf(const char *path, int32_t n_shards, int device, bwams_writer_t **out);
int bwams_writer_put_bgzf(bwams_writer_t *w, int32_t shard, int64_t seq, const uint8_t *members, int64_t n_bytes);
/* A BAM writer: shards named as bwams_writer_open names them, with ".bam" in place of ".sam".  Every shard starts with bam_header
 * (bwams_bam_header's block, n bytes) compressed into members of its own on `device`, so that the first record starts a member; then
 * the members of bwams_writer_put_bgzf (e.g. from bwams_bam_fetch_bgzf, without the EOF member) in sequence order; bwams_writer_close
 * appends the EOF member.  bwams_writer_put (text) on a BAM writer is BWAMS_ERR_ARG. */
int bwams_writer_open_bam(const char *path, int32_t n_shards, int device, const void *bam_header, int64_t n, bwams_writer_t **out);
/* A coordinate-sorted BAM file and, with BWAMS_SORT_BAI, its index <path>.bai (SAMv1 §5.2): what `samtools sort` and
 * `samtools index` make of the unsorted stream (host/bam_sort.cpp).  Each put is one sorted run tagged with its sequence number
 * `seq` (the run's place in input order); any thread may put, in any order.  Runs stay in host memory up to mem_bytes and are
 * spilled raw beyond that to "<tmp_prefix>.<n>.run" (tmp_prefix NULL: "<path>.tmp"); close removes them, on success and on error.
 * _put: records[0, n_bytes) with their coords (as bwams_bam_sorted_fetch returns them); BWAMS_ERR_ARG for keys out of order, sizes
 * that do not chain the records to n_bytes, a refID >= the header's n_ref, an end past 2^29 with BWAMS_SORT_BAI, or a seq put before.
 * _put_batch: bwams_bam_sort on the batch (at once when it is sorted already), its records fetched straight into the run.
 * _close: k-way merge by (key, seq, index in the run); the header block (bwams_bam_header's) in members of its own, then the merged
 * records cut every 65280 bytes from their first byte into members made by a deflater on `device`, then the EOF member.  The
 * bytes of the file and of the index depend only on the records and their seq numbers (not on put order, threads, mem_bytes or
 * spilling); bwams/bai.py restates the index.  BWAMS_SORT_BAI with a reference longer than 2^29 bases: BWAMS_ERR_UNSUPPORTED at
 * open (BAI cannot hold it).
 * With BWAMS_SORT_MARKDUP the file is also duplicate-marked (the rules above bwams_bam_templates), over every put as one input:
 * _put is BWAMS_ERR_ARG (sorted host records carry no template grouping); _put_batch also runs bwams_bam_templates on the batch
 * (its refusals pass through) and keeps the batch's ends and each record's template ordinal in sorted order (4 B per record, kept
 * and spilled with the run).  The ends (32 B per template) stay in host memory and are not counted in mem_bytes.  At close the
 * runs' template ordinals are offset by a base taken in seq order, one bwams_dup_decide runs on `device` (BWAMS_ERR_NOMEM when it
 * does not fit in HBM), and the merge sets or clears 0x400 in each record as it copies it.  Without the flag FLAG passes through
 * (a batch marked with bwams_bam_markdup keeps its marks).  0x400 changes no size, bin or index byte.
 * _close2: _close, and the marking's counts in *dup (zeros without BWAMS_SORT_MARKDUP); either stats pointer may be NULL.
 * _close(s, st) is _close2(s, st, NULL). */
typedef struct bwams_sorter bwams_sorter_t;
#define BWAMS_SORT_BAI 0x1                       /* also write <path>.bai */
#define BWAMS_SORT_MARKDUP 0x2                   /* mark duplicates over all puts (FLAG 0x400) */
int bwams_sorter_open(const char *path, int device, const void *bam_header, int64_t n_header, const char *tmp_prefix, int64_t mem_bytes,
                      int32_t flags, bwams_sorter_t **out);
int bwams_sorter_put(bwams_sorter_t *s, int64_t seq, const void *records, int64_t n_bytes, const bwams_bam_coord_t *coords,
                     int64_t n_records);
int bwams_sorter_put_batch(bwams_sorter_t *s, int64_t seq, bwams_batch_t *b);
int bwams_sorter_close(bwams_sorter_t *s, bwams_sorter_stats_t *stats);   /* stats may be NULL */
int bwams_sorter_close2(bwams_sorter_t *s, bwams_sorter_stats_t *stats, bwams_dup_stats_t *dup);
/* _set_markdup: the groups table (copied; may be NULL) and the options (may be NULL: optical detection off) of a sorter opened with
 * BWAMS_SORT_MARKDUP, before its first put: BWAMS_ERR_ARG otherwise.  Every put_batch then runs bwams_bam_templates2 with the table
 * and keeps the put's bwams_dup_loc_t beside its ends (24 B per end, host memory, outside mem_bytes) and its two record-level counts
 * per library; a library ordinal means the same in every put, the table being the sorter's.
 * _close3: _close2 through bwams_dup_decide2 over all the puts, with rule 13's rows in lib_stats[0, n_lib) (may be NULL; cap_lib <
 * n_lib is BWAMS_ERR_CAPACITY and leaves the sorter open).  Without _set_markdup: one library, no optical duplicates, the two record-level counts 0,
 * _close2's file. */
int bwams_sorter_set_markdup(bwams_sorter_t *s, const bwams_dup_groups_t *groups, const bwams_dup_opt_t *opt);
int bwams_sorter_close3(bwams_sorter_t *s, bwams_sorter_stats_t *stats, bwams_dup_stats_t *dup, bwams_dup_lib_stats_t *lib_stats,
                        int64_t cap_lib);
/* Depth of coverage (csrc/depth.hip, csrc/api_depth.hip, host/depth_text.cpp): per-base depth accumulated on the device from a
 * batch's BAM records, from host records, or from the sorted BAM writer's merged stream; finished once, then queried.  The rules
 * are this library's own, modelled on `samtools depth` without -s and on `mosdepth --fast-mode`; no byte parity with either is
 * claimed.  bwams/depth.py restates them in numpy and is what the tests compare against.
 *  1. References.  The handle is made from n_ref lengths, l_ref[r] >= 0.  Depth is defined for positions [0, l_ref[r]) of each
 *     reference.  The handle holds sum(l_ref) + n_ref 32-bit counters in HBM (12.4 GB at GRCh38 size); when they do not fit the
 *     open returns BWAMS_ERR_NOMEM.
 *  2. Which records count.  A record counts when (FLAG & exclude) == 0 (default exclude 0x704: unmapped, secondary, QC-fail,
 *     duplicate), MAPQ >= min_mapq (default 0), 0 <= refID < n_ref, and n_cigar_op > 0.  Supplementary records count unless the
 *     caller excludes 0x800.  A record that does not count is skipped; it does not refuse the call.
 *  3. What a record covers.  The CIGAR is walked from POS: M, = and X cover their length and advance; D advances, and covers only
 *     with count_deletions; N advances without covering; I, S, H and P do neither.  Positions below 0 or at or past l_ref[refID] are
 *     clipped, not refused: a record that runs off the end of its reference covers up to the end.  Only the CIGAR field counts; a
 *     long CIGAR parked in a CG tag is not looked up.  A record with an op code above 8 refuses the whole call with BWAMS_ERR_ARG,
 *     whether it would count or not (choice: the check does not depend on the filter); bwams_last_error names the first such
 *     record; nothing of that call is added (all records are checked first, then added).
 *  4. No mate-overlap correction: every record counts by itself, as in `samtools depth` without -s.  Correcting for overlapping
 *     mates is out of scope.
 *  5. Accumulation.  Depth is the sum over all added records, in any order, over any number of calls.  More than 2^31 - 1 records
 *     added in total (counted or not): BWAMS_ERR_UNSUPPORTED, and nothing of that call is added.
 *  6. State.  _finish turns the accumulated counters into depths, in place (a second _finish does nothing).  After it an add is
 *     BWAMS_ERR_ARG; before it a query is BWAMS_ERR_ARG.  _reset zeroes the handle for reuse, finished or not.
 *  7. Summary per reference: length; bases, the sum of the depth as int64; min; max.  min and max are 0 for a reference of length 0.
 *  8. Histogram for one reference, or for ref = -1 all references: hist[v] is the number of positions of depth v for v < n_bins - 1,
 *     hist[n_bins - 1] the number of positions at or above n_bins - 1.  Counts are int64; 2 <= n_bins <= 2^20.
 *  9. Windows of w >= 1 bases: reference r has ceil(l_ref[r] / w) windows, the references' windows follow each other in reference
 *     order, a reference's last window may be short, a reference of length 0 has none.  A window's value is the int64 sum of the
 *     depth in it; the mean exists in the text only.
 * 10. Runs over [beg, end) of one reference (0 <= beg <= end <= l_ref[ref]): a run is a maximal stretch of equal depth inside the
 *     range; start[k] is its first position and depth[k] its depth.  Zero-depth runs are included.  The first run starts at beg,
 *     also when beg lies inside a longer run.  When the runs do not fit cap: BWAMS_ERR_CAPACITY with *n the number needed.
 * 11. Text (bwams_depth_text; names: n_ref names, each ending in NUL, back to back).  Three texts:
 *     BWAMS_DEPTH_TEXT_SUMMARY: a header line, one row per reference, a `total` row; chrom, length, bases, mean, min, max separated by
 *       tabs; mean = bases / length printed with %.2f, 0.00 for length 0; the total row's min and max are over the references of
 *       length > 0 (0 when there is none).  Two references c1 (10 bases, depths 2 2 2 2 2 0 0 0 0 1) and c2 (length 0):
 *         "chrom\tlength\tbases\tmean\tmin\tmax\n" "c1\t10\t11\t1.10\t0\t2\n" "c2\t0\t0\t0.00\t0\t0\n" "total\t10\t11\t1.10\t0\t2\n"
 *     BWAMS_DEPTH_TEXT_DIST (arg: n_bins of rule 8, 0 for 1024): chrom, depth, and the fraction of positions at or above that depth
 *       printed with %.4f; rows from the largest occupied bin down to 0; a `total` block first, then a block per reference; a
 *       reference (or a total) of length 0 has no rows.  The same handle:
 *         "total\t2\t0.5000\n" "total\t1\t0.6000\n" "total\t0\t1.0000\n" "c1\t2\t0.5000\n" "c1\t1\t0.6000\n" "c1\t0\t1.0000\n"
 *     BWAMS_DEPTH_TEXT_WINDOWS (arg: w of rule 9): a BED line per window: chrom, start, end, mean = sum / (end - start) with %.2f.
 *       The same handle, w = 4: "c1\t0\t4\t2.00\n" "c1\t4\t8\t0.50\n" "c1\t8\t10\t0.50\n"
 *     A per-base BED file is out of scope (tens of gigabytes of text at 30x); rule 10's arrays are the interface for that.
 * bwams_depth_open: a zeroed handle on `device` (opt may be NULL; exclude above 0xFFFF, reserved != 0, n_ref < 0 or a negative
 * length: BWAMS_ERR_ARG).  _close (NULL allowed).  _add_batch: the batch's current BAM records (bwams_bam_run / _upload left them,
 * BWAMS_ERR_ARG before either), read in HBM; the batch must be on the handle's device (BWAMS_ERR_ARG); after bwams_bam_markdup the
 * records carry 0x400, so duplicates drop out by rule 2.  _add_records: host records bam[0, n_bytes), uploaded; their block_size
 * chain is checked as bwams_bam_upload checks it (BWAMS_ERR_ARG).  *n_counted (may be NULL): the records of this call that rule 2
 * let through.  _summary: n_ref rows (cap < n_ref: BWAMS_ERR_CAPACITY).  _hist: ref in [-1, n_ref).  _windows: *n (may be NULL) the
 * number of windows, needed or written; sums may be NULL to ask for it; cap too small: BWAMS_ERR_CAPACITY.  _runs: start and depth
 * may both be NULL to ask for *n.  _fetch: the depths of [beg, end) of one reference, for tests and small regions.  _text: `what`
 * of rule 11 into out[0, cap); *n: the bytes written, or needed with BWAMS_ERR_CAPACITY, as bwams_sam_header.
 * bwams_sorter_set_depth: before the sorter's first put (BWAMS_ERR_ARG later, for a handle on another device, or when the handle's
 * lengths differ from the sorter header's).  The close then adds every record of the merged stream AS WRITTEN, that is after the
 * merge has set or cleared 0x400, so a sorter with BWAMS_SORT_MARKDUP gives duplicate-free depth.  The records are uploaded a second
 * time, in whole records: one that straddles two deflate pieces is counted once, with its final flag, so the result does not
 * depend on where the pieces cut the stream.  Close does not call _finish: the caller may add further files.  The file and the
 * index are byte for byte what they are without the call.  An add that fails ends the close with its error (rule 3: a record of
 * the merged stream with an op code above 8 is BWAMS_ERR_ARG), with the file written up to the piece before it and no index: a
 * sorter without a handle would have written those records; check them first when they come from elsewhere.
 * bwams_depth_text with BWAMS_DEPTH_TEXT_DIST runs one histogram per reference and holds (n_ref + 1) * n_bins int64 on the host:
 * meant for tens to thousands of references; for an assembly of 100 000 contigs ask bwams_depth_hist for the references wanted. */
#define BWAMS_DEPTH_TEXT_SUMMARY 0
#define BWAMS_DEPTH_TEXT_DIST 1
#define BWAMS_DEPTH_TEXT_WINDOWS 2
int bwams_depth_open(int device, const int32_t *l_ref, int32_t n_ref, const bwams_depth_opt_t *opt, bwams_depth_t **out);
int bwams_depth_close(bwams_depth_t *d);
int bwams_depth_reset(bwams_depth_t *d);
int bwams_depth_add_batch(bwams_depth_t *d, bwams_batch_t *b, int64_t *n_counted);
int bwams_depth_add_records(bwams_depth_t *d, const void *bam, int64_t n_bytes, int64_t *n_counted);
int bwams_depth_finish(bwams_depth_t *d);
int bwams_depth_summary(bwams_depth_t *d, bwams_depth_ref_t *rows, int64_t cap);
int bwams_depth_hist(bwams_depth_t *d, int32_t ref, int64_t *hist, int32_t n_bins);
int bwams_depth_windows(bwams_depth_t *d, int32_t w, int64_t *sums, int64_t cap, int64_t *n);
int bwams_depth_runs(bwams_depth_t *d, int32_t ref, int32_t beg, int32_t end, int32_t *start, int32_t *depth, int64_t cap, int64_t *n);
int bwams_depth_fetch(bwams_depth_t *d, int32_t ref, int32_t beg, int32_t end, int32_t *depth);
int bwams_depth_text(bwams_depth_t *d, const char *names, int32_t what, int32_t arg, char *out, int64_t cap, int64_t *n);
int bwams_sorter_set_depth(bwams_sorter_t *s, bwams_depth_t *d);
/* Pileup (csrc/pileup.hip, csrc/api_pileup.hip, host/pileup_text.cpp, host/pileup_vcf.cpp): per-base allele counts of SEQ and QUAL against the reference,
 * accumulated on the device from a batch's BAM records, from host records, or from the sorted BAM writer's merged stream, and the
 * candidate variant sites they give.  The rules are this library's own, modelled on the defaults of `samtools mpileup`; no byte
 * parity with it is claimed.  bwams/pileup.py restates them in numpy and is what the tests compare against.
 *  1. Regions.  The handle is opened over n_ref reference lengths and a list of regions (ref, beg, end) with
 *     0 <= beg < end <= l_ref[ref], sorted by (ref, beg) and not overlapping (touching regions are allowed); anything else is
 *     BWAMS_ERR_ARG.  An empty list means one region per reference of length > 0.  Counters exist only for region positions,
 *     concatenated in region order: a slot per position.  A slot holds 12 uint32 channels: A+ C+ G+ T+ A- C- G- T- (+ forward, - when
 *     FLAG has 0x10), then N, DEL, INS, and one reserved channel that stays 0.  That is 48 bytes per position (a human chromosome is
 *     12 GB), so a whole genome does not fit beside an index and regions are how a caller walks it.  When the counters do not fit,
 *     the open returns BWAMS_ERR_NOMEM.
 *  2. Which records count.  Depth rule 2's filter: (FLAG & exclude) == 0 (default 0x704), MAPQ >= min_mapq (default 0),
 *     0 <= refID < n_ref and n_cigar_op > 0; in addition l_seq > 0 (a record with SEQ `*` is skipped).  A record that does not count
 *     is skipped; it does not refuse the call.
 *  3. Validity.  All records of a call are checked before anything is added.  An op code above 8 is BWAMS_ERR_ARG, whether the filter
 *     would let the record through or not, as in depth rule 3.  A record that passes rule 2's filter whose CIGAR query length (the
 *     lengths of M I S = X) differs from l_seq, or whose SEQ or QUAL ends behind the record's block_size, is BWAMS_ERR_ARG too.
 *     bwams_last_error names the first such record (the op code when one record has both).  Nothing of that call is added.
 *  4. The walk from POS.  M, = and X: each base adds 1 to the channel of its 4-bit SEQ code and strand; codes 1, 2, 4 and 8 are A, C,
 *     G and T, every other code, 0 (`=`) included, goes to N, which has no strand.  A base counts only if its quality is >=
 *     min_baseq (default 13); a record without qualities (first QUAL byte 0xFF) passes every min_baseq.  D adds 1 to DEL at each
 *     deleted position, with no quality test.  N advances without counting.  Every I op adds 1 to INS at the position before the
 *     insertion, whatever its length and quality, and only when a reference-consuming op (M D N = X, of any length) precedes it in
 *     that record: an insertion that opens the alignment is not counted.  S advances the query only; H and P do nothing.
 *     Positions outside every region, below 0, or at or past the reference's end are dropped one by one: a record may span
 *     several regions and the gaps between them.  Only the CIGAR field counts (no CG tag).
 *  5. No mate-overlap correction, as depth rule 4: where two mates overlap, both count.
 *  6. Accumulation.  The counters hold the sum over all adds, in any order, over any number of calls, modulo 2^32.  More than
 *     2^31 - 1 records given in total (counted or not) is BWAMS_ERR_UNSUPPORTED, and nothing of that call is added; nor is anything
 *     when an allocation of the add fails (BWAMS_ERR_NOMEM).  After BWAMS_ERR_DEVICE the counters are undefined until _reset.
 *     There is no finish step: a query sees everything added before it.  _reset zeroes the counters (the reference bases stay).
 *  7. Reference bases: one code 0..4 per slot (0..3 = A C G T, 4 = N), all 4 before the first _set_ref*.  They come from host codes
 *     for one region (_set_ref; a code above 4 is BWAMS_ERR_ARG), or from an opened index (_set_ref_index), which gathers the
 *     forward strand of the index's .0123 bytes on the device by the contig table; BWAMS_ERR_ARG when the index has no .0123 or no
 *     contigs, is on another device, or when its contig lengths differ from l_ref.  For an index made from FASTA
 *     (bwams_index_from_fasta*) the .amb holes become 4.  For ANY OTHER index the bases that the index holds in place of N stay:
 *     such an index does not know where its Ns were.
 *  8. Candidate sites.  At a slot with reference base b < 4, depth is the sum of the eight base channels plus DEL (N and INS are not
 *     part of it).  An allele is one of the three bases other than b (both strands summed), DEL, or INS.  An allele is a candidate
 *     when its count >= min_alt (default 2) and count * 1000 >= min_permille * depth (default 200), in integer arithmetic.  A slot
 *     with at least one candidate allele is a site; a slot whose reference base is 4 is none.  bwams_pileup_sites returns the sites
 *     of all regions in slot order as bwams_pileup_site_t records (include/bwams_types.h): region, pos, ref, kinds (bits 0-3: A C G T as
 *     alternate alleles, bit 4: DEL, bit 5: INS), depth, c[12].  The sites are found with rocprim::select, as the depth runs are.
 *  9. Text (bwams_pileup_text; names: n_ref names, each ending in NUL, back to back).  A header line, then a tab-separated row per
 *     site: chrom, 1-based position, ref letter (ACGTN), depth, the eleven live channels in rule 1's order, and the candidate alleles
 *     separated by commas in the order of rule 8's bits (A C G T DEL INS).  Reference c1 = ACGTACGT, one region over it, seven records
 *     of quality 30: 8M ACGTACGT at 0; 8M ACTTACGT at 0, once forward and once with FLAG 0x10; 2M1D2M GTCG at 2, twice;
 *     2M2I2M ACTTGT at 4, twice:
 *       "chrom\tpos\tref\tdepth\tA+\tC+\tG+\tT+\tA-\tC-\tG-\tT-\tN\tDEL\tINS\talt\n"
 *       "c1\t3\tG\t5\t0\t0\t3\t1\t0\t0\t0\t1\t0\t0\t0\tT\n" "c1\t5\tA\t7\t4\t0\t0\t0\t1\t0\t0\t0\t0\t2\t0\tDEL\n"
 *       "c1\t6\tC\t7\t0\t6\t0\t0\t0\t1\t0\t0\t0\t0\t2\tINS\n"
 *     Quality-weighted sums, genotype costs, SNV calls and their VCF text are rules 10 to 13, for a handle with a quality plane.
 *     Indel alleles, their genotypes and VCF rows are rules 14 to 17, for a handle with an indel store.
 * 10. Effective quality (a handle with a quality plane: bwams_pileup_set_quality).  A base that rule 4 counts in one of the eight base
 *     channels has the effective quality qe = clamp(min(q, MAPQ), 4, 60), where q is its QUAL byte, or no_qual_q (default 30) for a
 *     record whose first QUAL byte is 0xFF.  min_baseq is tested on the raw byte as in rule 4, before this.  N, DEL and INS add
 *     nothing to the plane.
 * 11. The sums.  The plane holds 12 uint32 per slot beside the counters (48 bytes more per position): for each base b of A C G T,
 *     both strands together, Q[b] = sum of qe, HOM[b] = sum of T_HOM[qe] and HET[b] = sum of T_HET[qe], in the order Q[A..T],
 *     HOM[A..T], HET[A..T] (BWAMS_PILEUP_Q, _HOM, _HET + b).  They accumulate as rule 6's counters do: any order, any number of
 *     calls, modulo 2^32.  The largest addend is T_HET[4] = 435, so no sum wraps below a depth of 2^32 / 435, which lies above 2^22:
 *     a caller with a depth above 2^22 gets what wrapped sums give (bwams/pileup.py wraps the same way).
 * 12. The tables.  The unit is a hundredth of a phred: -1000 log10(p), rounded half to even, with e = 10^(-q / 10).  T_HOM[q] is
 *     the cost of p = 1 - e, a base under a homozygous genotype of its own allele; T_HET[q] that of p = (1 - e) / 2 + e / 6, a base
 *     under a heterozygous genotype that holds its allele.  A base under a genotype without its allele has p = e / 3, which costs
 *     exactly 100 q + 477 for every integer q and needs no table.  For q = 4 .. 60:
 *       T_HOM = 220 165 126 97 75 58 46 36 28 22 18 14 11 9 7 6 4 3 3 2 2 1 1 1 1 1, then 0 for q = 30 .. 60
 *       T_HET = 435 404 381 363 350 339 331 325 320 316 313 310 308 307 306 305 304 303 303 302 302 302 302 302, then 301 for
 *               q = 28 .. 60
 *     (computed with 60 decimal digits; no entry lies within 0.002 of a rounding boundary).  csrc/common.h holds them as integer
 *     literals, bwams/pileup.py restates them, and tests/test_pileup_calls.py recomputes both.  There is no floating point between
 *     the records and a call.
 * 13. Genotype costs and calls, at a slot whose reference base is r < 4 and whose base depth is at least min_depth (default 1).
 *     n[b] is channel b plus channel b + 4; the base depth n = sum of n[b] leaves out DEL, N and INS; MIS[b] = 100 Q[b] + 477 n[b].
 *     The ten diploid genotypes (a1 <= a2 by base code) have the index g = a2 (a2 + 1) / 2 + a1, VCF's order over A C G T:
 *     AA AC CC AG CG GG AT CT GT TT.  cost(g) is the sum over the four bases b of HOM[b] when g is homozygous b b, of HET[b] when g
 *     is heterozygous and b one of its alleles, and of MIS[b] when b is no allele of g, in uint64 from the uint32 sums.
 *     pl[g] = (cost(g) - least cost + 50) / 100 by integer division, uncapped, as int32 saturating at 2^31 - 1.  The genotype is
 *     the g of least cost, a tie going to the lowest g; qual = pl[g(r, r)]; gq = min(99, the least pl over the other nine
 *     genotypes).  A slot is a CALL when its genotype is not (r, r) and qual >= min_qual (default 20).  There is no prior on
 *     heterozygosity and no model of strand bias or of overlapping mates (rule 5): every base is an independent observation, and
 *     min_qual is the caller's lever.  bwams_pileup_calls returns the calls of all regions in slot order as bwams_pileup_call_t
 *     records (include/bwams_types.h): region, pos, ref, a1, a2, qual, gq, depth, n[4], pl[10]; they are counted and selected with
 *     rocprim::reduce and rocprim::select, as the sites are.
 *     VCF (bwams_pileup_vcf; names as in rule 9, sample: the name of the one sample column).  The header lines
 *     ##fileformat=VCFv4.2, ##source=bwams, one ##contig=<ID=name,length=L> per reference, ##INFO DP (1, Integer), ##FORMAT GT (1,
 *     String), AD (R, Integer), DP (1, Integer), GQ (1, Integer) and PL (G, Integer), and the #CHROM line; then a row per call.  ALT
 *     is the genotype's alleles other than the reference, in base order, one or two; GT their indices (0 the reference, 1 and 2 the
 *     ALTs) as a/b with a <= b; AD is n over REF and the ALTs; PL the pl of the genotypes over (REF, ALTs) in VCF's order, three
 *     values or six.  Rule 9's seven records with MAPQ 60: slot 2 (reference G) has three G and two T of quality 30, so
 *     cost(GG) = 2 * 3477 = 6954, cost(GT) = 5 * 301 = 1505 and cost(TT) = 3 * 3477 = 10431, pl is 54 / 0 / 89, and the only row is
 *       "c1\t3\t.\tG\tT\t54\t.\tDP=5\tGT:AD:DP:GQ:PL\t0/1:3,2:5:54:54,0,89\n"
 * 14. Events (a handle with an indel store: bwams_pileup_set_indels; the store is independent of the quality plane).  In each record
 *     that rule 2 counts (rule 3 is checked for the whole call first), every I or D op that a reference-consuming op (M D N = X, of
 *     any length) precedes gives one event at the ANCHOR, the reference position just before the op: rule 4's INS condition, for D
 *     too.  An I or D that opens the alignment gives none; the DEL and INS channels are untouched by all of this.  An event whose
 *     anchor is in no region slot is dropped.  An event has a type (0 DEL, 1 INS, 2 OTHER), a length and a sequence: for an insertion
 *     the op's SEQ bases packed 2 bits each, base j at bits 2j and 2j + 1, codes 1 2 4 8 as 0 1 2 3, the bits above 2 len zero; 0
 *     for a deletion.  An event becomes OTHER, with len 0 and seq 0, when its length exceeds max_len (1..32, default 32: what a
 *     64-bit sequence word holds), when an inserted base is not A, C, G or T, or when it is a deletion whose last deleted position
 *     is not in the anchor's region.  Its quality is qe = clamp(min(MAPQ, indel_q), 4, 60), indel_q in 0..93, default 40; base
 *     qualities and min_baseq play no part.  Adjacent I and D ops give two events at one anchor.
 * 15. Span sums (reference support).  A record that rule 2 counts SPANS slot s when positions s and s + 1 both lie inside one
 *     maximal run of consecutive M/=/X ops of its CIGAR (any other op, of any length, ends a run); s + 1 may lie outside every
 *     region.  Per slot four uint32 sums, SPAN_N, SPAN_Q, SPAN_HOM and SPAN_HET (BWAMS_PILEUP_SPAN_*), get 1, qe, T_HOM[qe] and
 *     T_HET[qe] with rule 14's qe.  They accumulate as rule 6 has it, modulo 2^32.
 * 16. Alleles and genotype, at a slot with reference base r < 4.  The events at the slot group by (type, len, seq); a group has n,
 *     Q = sum of qe, HOM = sum of T_HOM[qe] and HET = sum of T_HET[qe], each in uint64.  The groups are ordered by (type, len, seq),
 *     seq compared unsigned.  ALT is the type-0 or type-1 group with the largest n, a tie going to the first in that order; a slot
 *     with no such group is no call.  n_other counts every other event at the slot.  MIS_x = 100 Q_x + 477 n_x.  In uint64:
 *       cost(RR) = SPAN_HOM + MIS_ALT,  cost(RA) = SPAN_HET + HET_ALT,  cost(AA) = SPAN_MIS + HOM_ALT.
 *     pl, the genotype, qual = pl[RR] and gq follow rule 13: + 50 then / 100, saturating int32, a tie to the lowest of RR RA AA,
 *     gq = min(99, the least other pl).  depth = SPAN_N + n_ALT + n_other.  A slot is a CALL when the genotype is not RR, qual >=
 *     min_qual (default 20) and depth >= min_depth (default 1).  There is NO realignment and no model of homopolymers, tandem
 *     repeats, strands or mate overlap.  Without rule 18 the alleles are taken as the CIGARs give them, and two reads that place the
 *     same deletion one base apart are two alleles at two slots; with it they are one allele at the leftmost placement the
 *     reference allows inside the region, and nothing more is done: reads are not aligned again, and two events that a read could
 *     have expressed as one stay two.
 * 17. Records and text.  bwams_pileup_indel_calls returns the calls in slot order as bwams_pileup_indel_t records (include/bwams_types.h):
 *     region, pos (the anchor), ref, type, len, seq, gt (1 het, 2 hom-alt), qual, gq, depth, n_ref (SPAN_N), n_alt, n_other, pl[3],
 *     del_ref[32] (the reference codes 0..4 of the deleted positions, 0 elsewhere).  bwams_pileup_indel_alleles returns EVERY group
 *     of every slot, OTHER included and whatever the slot's reference base, in (slot, type, len, seq) order as
 *     bwams_pileup_indel_allele_t: region, pos, type, len, seq, n, q, hom, het.  VCF rows: a deletion has REF = the anchor letter
 *     plus the deleted letters (ACGTN) and ALT = the anchor letter; an insertion has REF = the anchor letter and ALT = the anchor
 *     letter plus the sequence.  INFO is DP=depth;INDEL, FORMAT GT:AD:DP:GQ:PL, GT 0/1 or 1/1, AD n_ref,n_alt, three PL values.
 *     Rule 9's seven records with MAPQ 60 and the default options: qe = 40, MIS = 4477 a read, HOM = 0 and HET = 301.  Slot 3 has
 *     3 spanning reads and 2 deletions of 1: cost(RR) = 8954, cost(RA) = 3 * 301 + 2 * 301 = 1505, cost(AA) = 13431.  Slot 5 has 5
 *     spanning reads and 2 insertions of TT: cost(RR) = 8954, cost(RA) = 2107, cost(AA) = 22385.  The two rows:
 *       "c1\t4\t.\tTA\tT\t74\t.\tDP=5;INDEL\tGT:AD:DP:GQ:PL\t0/1:3,2:5:74:74,0,119\n"
 *       "c1\t6\t.\tC\tCTT\t68\t.\tDP=7;INDEL\tGT:AD:DP:GQ:PL\t0/1:5,2:7:68:68,0,203\n"
 * 18. Left-alignment (a handle with an indel store on which bwams_pileup_set_indel_leftalign(p, 1) was called; every region's
 *     reference bases must be in place before the records, see below).  Rule 14 classifies the event first, on the CIGAR's anchor.
 *     An event of type DEL or INS (not OTHER) and length L >= 1 with anchor a in the region [beg, end) is then shifted.  Let X[p] be
 *     the reference code at p for p <= a; for a deletion the reference code for p > a too; for an insertion X[a + 1 + i] is inserted
 *     base i, i < L.  The shift k is the largest value such that for every j < k: a - j - 1 >= beg, X[a - j] == X[a + L - j], and
 *     neither code is 4 (an N matches nothing, itself included).  The event is stored at a' = a - k with its type and length; an
 *     insertion's sequence becomes X[a' + 1 .. a' + L], packed as rule 14 packs it (the inserted bases rotated by k modulo L).  An
 *     event of length 0 and an OTHER event are stored as rule 14 has them.  The shift NEVER LEAVES THE ANCHOR'S REGION, even where
 *     another region ends at beg: a region that begins inside a repeat gives that region's leftmost placement, not the genome's.
 *     A shift that runs into an N ends with the N as the anchor (the test that fails is the one that reads it), where rule 16 makes
 *     no call; the allele record still shows the event there.
 *     Span sums: when the op directly before the event's op is M, = or X, that run of match ops ends at a, and the record does NOT
 *     span the slots s with a' <= s < a that rule 15 gave it through that run; rule 15 holds everywhere else.  (Otherwise a read
 *     whose deletion moved left would be reference support at the slot where it is now ALT.)  Only that run is clipped: an event
 *     behind any other op (N, D, P, or the second of two adjacent I and D ops) clips nothing, and earlier runs of the record are
 *     left alone even where the shift crosses them.  The sums stay modulo 2^32 and no sum goes below zero: what is taken back was
 *     added by the same record.  The DEL and INS channels of rule 4 stay where the CIGAR put them.  Rules 16 and 17 are unchanged
 *     and work on the shifted events; del_ref and the VCF's REF and ALT come from the shifted anchor.  This is the reference-only
 *     normalisation of `bcftools norm` (Tan et al. 2015) applied to each event by itself: no realignment, no repeat model.
 *     Rule 9's records do not move under it (c1 = ACGTACGT repeats nothing), and rule 17's two rows stand as they are:
 *       "c1\t4\t.\tTA\tT\t74\t.\tDP=5;INDEL\tGT:AD:DP:GQ:PL\t0/1:3,2:5:74:74,0,119\n"
 *       "c1\t6\t.\tC\tCTT\t68\t.\tDP=7;INDEL\tGT:AD:DP:GQ:PL\t0/1:5,2:7:68:68,0,203\n"
 *     Reference c2 = TCAAAAGT, MAPQ 60, three records at 0: 8M; 5M1D2M, anchor 4, which moves by 3; 3M1D4M, anchor 2, which moves
 *     by 1.  Both deletions are one allele at slot 1; the first read's span over 0..3 shrinks to slot 0, the second's over 0..1
 *     too, and only the 8M read spans slot 1: cost(RR) = 8954, cost(RA) = 301 + 602, cost(AA) = 4477.  The one row (without the
 *     rule: two rows of QUAL 36 at 3 and 5):
 *       "c2\t2\t.\tCA\tC\t81\t.\tDP=3;INDEL\tGT:AD:DP:GQ:PL\t0/1:1,2:3:36:81,0,36\n"
 * bwams_pileup_open: a zeroed handle on `device` (opt may be NULL for the defaults; exclude above 0xFFFF, min_baseq outside [0, 255],
 * min_alt < 1, min_permille outside [0, 1000], reserved != 0, n_ref < 0, a negative length or rule 1: BWAMS_ERR_ARG).  _close (NULL
 * allowed).  _add_batch: the batch's current BAM records (bwams_bam_run / _upload left them, BWAMS_ERR_ARG before either), read in
 * HBM; the batch must be on the handle's device; after bwams_bam_markdup the records carry 0x400, so duplicates drop out by rule 2.
 * _add_records: host records bam[0, n_bytes), uploaded; their block_size chain is checked as bwams_bam_upload checks it
 * (BWAMS_ERR_ARG).  *n_counted (may be NULL): the records of this call that rule 2 let through.
 * _set_ref: the region's end - beg codes.  _fetch: the counters of positions [beg, end) of the region's reference, inside the region,
 * 12 per position: for tests and small ranges.  _sites: *n (may be NULL) the number of sites, found or needed; sites may be NULL to
 * ask for it; cap too small: BWAMS_ERR_CAPACITY.  min_alt and min_permille: rule 8's thresholds for this query, a negative value
 * for the handle's.  _text: rule 9 into out[0, cap); *n: the bytes written, or needed with BWAMS_ERR_CAPACITY, as bwams_sam_header.
 * _set_quality: the quality plane of rules 10 to 13, allocated beside the counters and zeroed (opt may be NULL for {20, 1, 30, 0};
 * min_qual < 0, min_depth < 1, no_qual_q outside [0, 93] or reserved != 0: BWAMS_ERR_ARG; BWAMS_ERR_NOMEM when the plane does not
 * fit, as rule 1 has it for the counters).  It is legal only while the counters are zero, before the first add or directly after
 * _reset (BWAMS_ERR_ARG otherwise); calling it again then replaces the options and zeroes the plane, which stays for the life of the
 * handle; _reset zeroes both planes.  A handle on which it was never called behaves in every call as if the plane did not exist, and
 * its adds run the count-only kernels.  _fetch_quality: the sums of positions [beg, end), 12 per position, as _fetch.  _calls: as
 * _sites; min_qual and min_depth: rule 13's thresholds for this query, a negative value for the handle's (min_depth 0:
 * BWAMS_ERR_ARG).  _vcf: rule 13's text into out[0, cap), as _text.  _fetch_quality, _calls and _vcf on a handle without a plane:
 * BWAMS_ERR_ARG.
 * _set_indels: the indel store of rules 14 to 17, independent of the quality plane: rule 15's sums (32 bytes more per position, the
 * sums and their difference array) allocated and zeroed, and an empty event list (opt may be NULL for {20, 1, 40, 32, 0}; min_qual
 * < 0, min_depth < 1, indel_q outside [0, 93], max_len outside [1, 32] or reserved != 0: BWAMS_ERR_ARG; BWAMS_ERR_UNSUPPORTED for a
 * handle of 2^32 slots or more; BWAMS_ERR_NOMEM when the sums do not fit).  Legal only while the counters are zero, as _set_quality;
 * calling it again then replaces the options, zeroes the sums and empties the events; _reset zeroes the sums and empties the events.
 * A handle on which it was never called behaves in every call exactly as before, and its adds launch exactly the kernels they
 * launched.  With the store, an add first counts the events its records give and grows the event buffer (16 bytes of key and 4 of
 * quality per event, the events held kept) before any counter of the call moves: BWAMS_ERR_NOMEM there adds nothing.
 * _set_indel_leftalign: rule 18 on (1) or off (0) for the adds that follow.  Legal only on a handle with an indel store and while the
 * counters are zero, as _set_indels (BWAMS_ERR_ARG on a handle without the store, after an add, or for any other value of `on`);
 * _set_indels called again turns it off, since that call replaces the store's options; _reset keeps it.  A handle on which it is
 * off behaves, and launches, exactly as one that never made the call.  On a left-aligning handle the reference comes first: an add
 * while any region has had neither _set_ref nor _set_ref_index is BWAMS_ERR_ARG, and nothing of that call is added; _set_ref and
 * _set_ref_index after an add and before _reset are BWAMS_ERR_ARG, because the events held were shifted against the bases in
 * place.  (Neither refusal exists on any other handle.)  Its adds run an event pass that also notes, in four transient bytes per
 * event sized with the event buffer before anything moves, how far the match run before the event reaches, and then
 * pileup_indel_align_kernel over the events of that add; _indel_info's ms_indel includes both.
 * _fetch_span: rule 15's sums of positions [beg, end), four per position, as _fetch.  _indel_alleles and _indel_calls: as _sites
 * (*n found or needed, a NULL array to ask, BWAMS_ERR_CAPACITY); min_qual and min_depth as in _calls, a negative value for the
 * store's.  _indel_vcf: rule 13's header with the line ##INFO=<ID=INDEL,Number=0,Type=Flag,...> after DP, then rule 17's rows, as
 * _text.  _vcf_all needs both the quality plane and the indel store (BWAMS_ERR_ARG otherwise): that same header, then the SNV rows
 * of _vcf (min_qual, min_depth) and the indel rows (indel_min_qual, indel_min_depth) merged by position, the SNV first where both
 * stand at one position; _vcf itself stays byte for byte what it is.  _indel_info: the events held, the capacity of their buffer in
 * events, and of the last add the events appended and the device time of the indel kernels; a test and measurement hook.
 * _fetch_span, _indel_alleles, _indel_calls, _indel_vcf, _vcf_all and _indel_info on a handle without the store: BWAMS_ERR_ARG.
 * The queries sort the events with rocprim::merge_sort, reduce runs of one key with rocprim::reduce_by_key and scan the sums'
 * difference array with rocprim::inclusive_scan; all three are cached until the next add or _reset.
 * _info: the positions of a tile of the add (below), the handle's regions and slots, and of the last add the records counted, the
 * (tile, record) entries, the records routed direct and the device time: a test and measurement hook, like bwams_debug_chain_counts.
 * An add cuts the slots into tiles.  A record whose slots lie in one or two tiles is counted in LDS by the workgroup that owns
 * the tile and the tile is added to HBM once; a record that touches more tiles (a long read, an N skip) goes to a kernel that issues
 * a global atomic per base, and so does every record under BWAMS_PILEUP_TILED=0 (the A/B baseline; the counters are the same).
 * With a quality plane a tile holds both planes and a counted base adds four values, in either kernel; the routing is the same.
 * bwams_sorter_set_pileup: the conditions and guarantees of bwams_sorter_set_depth: before the sorter's first put (BWAMS_ERR_ARG later,
 * for a handle on another device, or when the handle's lengths differ from the sorter header's); the close adds every record of the
 * merged stream AS WRITTEN, after the merge has set or cleared 0x400, in whole records (one cut by a deflate piece's end is counted
 * once); the file and the index are byte for byte what they are without the call; an add that fails ends the close with its error.
 * A sorter may have a depth handle, a pileup handle, or both: both see the same whole records.  A handle with a quality plane set on
 * a sorter receives the sums through the same add: the close leaves it ready for _calls and _vcf.  A handle with an indel store set
 * on a sorter receives the events and the span sums through that add too, with no further call: the close leaves it ready for
 * _indel_calls and, with both, _vcf_all. */
int bwams_pileup_open(int device, const int32_t *l_ref, int32_t n_ref, const bwams_pileup_region_t *regions, int32_t n_regions,
                      const bwams_pileup_opt_t *opt, bwams_pileup_t **out);
int bwams_pileup_close(bwams_pileup_t *p);
int bwams_pileup_reset(bwams_pileup_t *p);
int bwams_pileup_add_batch(bwams_pileup_t *p, bwams_batch_t *b, int64_t *n_counted);
int bwams_pileup_add_records(bwams_pileup_t *p, const void *bam, int64_t n_bytes, int64_t *n_counted);
int bwams_pileup_set_ref(bwams_pileup_t *p, int32_t region, const uint8_t *codes);
int bwams_pileup_set_ref_index(bwams_pileup_t *p, const bwams_index_t *ix);
int bwams_pileup_fetch(bwams_pileup_t *p, int32_t region, int32_t beg, int32_t end, uint32_t *counts);
int bwams_pileup_sites(bwams_pileup_t *p, int32_t min_alt, int32_t min_permille, bwams_pileup_site_t *sites, int64_t cap, int64_t *n);
int bwams_pileup_text(bwams_pileup_t *p, const char *names, int32_t min_alt, int32_t min_permille, char *out, int64_t cap, int64_t *n);
int bwams_pileup_info(const bwams_pileup_t *p, bwams_pileup_info_t *info);
int bwams_pileup_set_quality(bwams_pileup_t *p, const bwams_pileup_gl_opt_t *opt);
int bwams_pileup_fetch_quality(bwams_pileup_t *p, int32_t region, int32_t beg, int32_t end, uint32_t *sums);
int bwams_pileup_calls(bwams_pileup_t *p, int32_t min_qual, int32_t min_depth, bwams_pileup_call_t *calls, int64_t cap, int64_t *n);
int bwams_pileup_vcf(bwams_pileup_t *p, const char *names, const char *sample, int32_t min_qual, int32_t min_depth, char *out, int64_t cap,
                     int64_t *n);
int bwams_pileup_set_indels(bwams_pileup_t *p, const bwams_pileup_indel_opt_t *opt);
int bwams_pileup_set_indel_leftalign(bwams_pileup_t *p, int32_t on);
int bwams_pileup_fetch_span(bwams_pileup_t *p, int32_t region, int32_t beg, int32_t end, uint32_t *sums);
int bwams_pileup_indel_alleles(bwams_pileup_t *p, bwams_pileup_indel_allele_t *alleles, int64_t cap, int64_t *n);
int bwams_pileup_indel_calls(bwams_pileup_t *p, int32_t min_qual, int32_t min_depth, bwams_pileup_indel_t *calls, int64_t cap, int64_t *n);
int bwams_pileup_indel_vcf(bwams_pileup_t *p, const char *names, const char *sample, int32_t min_qual, int32_t min_depth, char *out, int64_t cap,
                           int64_t *n);
int bwams_pileup_vcf_all(bwams_pileup_t *p, const char *names, const char *sample, int32_t min_qual, int32_t min_depth, int32_t indel_min_qual,
                         int32_t indel_min_depth, char *out, int64_t cap, int64_t *n);
int bwams_pileup_indel_info(const bwams_pileup_t *p, bwams_pileup_indel_info_t *info);
int bwams_sorter_set_pileup(bwams_sorter_t *s, bwams_pileup_t *p);
/* Alignment QC (csrc/qc.hip, csrc/api_qc.hip, host/qc_text.cpp): the flag counts, insert sizes and per-cycle tables that a pipeline
 * reads off a finished BAM, accumulated on the device from a batch's BAM records, from host records, or from the sorted BAM
 * writer's merged stream.  Every value is an integer count.  The rules are this library's own, modelled on `samtools flagstat` and
 * `samtools stats`; no byte parity with either is claimed.  bwams/qc.py restates them in numpy and is what the tests compare against.
 *  1. Validity.  All records of a call are checked before anything is added.  For ANY record, whether rule 3's filter would count it
 *     or not: l_seq < 0, or a CIGAR that ends behind the record's block_size (`bounds`); a CIGAR op code above 8 (`op`, as depth
 *     rule 3).  For a record that passes rule 3's filter: SEQ or QUAL ending behind the record (`bounds`).  For a record that passes
 *     the filter and is mapped (no 0x4): an aux area that cannot be walked (`aux`): a field whose type byte is not one of
 *     A c C s S i I f Z H B, a B field whose subtype is not one of c C s S i I f, a field that runs past the record, or a Z or H field
 *     with no NUL inside the record.  Any of these makes the call BWAMS_ERR_ARG; bwams_last_error names the first such record and
 *     the reason; within one record the order is CIGAR bounds, op, SEQ / QUAL bounds, aux.  Nothing of the call is added.
 *  2. Flag counters.  Every record is counted, with no filter, in class 0, or in class 1 when FLAG has 0x200 (QC-fail).  Sixteen per
 *     class, in the order of the BWAMS_QC_FLAG_* indices: total; primary (neither 0x100 nor 0x800); secondary (0x100); supplementary
 *     (0x800 without 0x100); duplicates (0x400); primary_duplicates; mapped (not 0x4); primary_mapped; and over PRIMARY records with
 *     0x1: paired; read1 (0x40); read2 (0x80); properly_paired (0x2 and not 0x4); both_mapped (neither 0x4 nor 0x8); singletons (0x8
 *     and not 0x4); mate_other_ref (both mapped and next_refID != refID); mate_other_ref_mapq5 (the same with MAPQ >= 5).
 *  3. Filter.  Every table and scalar below takes only records with (FLAG & exclude) == 0; the default exclude, 0x900, counts each
 *     read once.  A record's class is 1 when FLAG has 0x80 (last fragment), otherwise 0.  Cycles are numbered in the read's original
 *     direction: for a record with 0x10, base i is cycle l_seq - 1 - i and the base is complemented.  Cycles at or past max_cycle are
 *     dropped from tables b and c and counted in bases_over (once per base).
 *  4. Tables, each a flat int64 array of the shape given (bwams_qc_table's `what`):
 *     a. BWAMS_QC_TABLE_RL    [2][max_cycle + 1]: 1 at min(l_seq, max_cycle).
 *     b. BWAMS_QC_TABLE_QUAL  [2][max_cycle][64]: 1 per base at min(quality, 63).  A record whose first QUAL byte is 0xFF adds nothing
 *        here and, when l_seq > 0, 1 to no_qual.
 *     c. BWAMS_QC_TABLE_BASE  [2][max_cycle][5]: A C G T N; the SEQ codes 1, 2, 4 and 8 are the bases, every other code is N.
 *     d. BWAMS_QC_TABLE_MAPQ  [256]: over mapped records (not 0x4).
 *     e. BWAMS_QC_TABLE_ISIZE [3][max_isize + 1], the rows inward, outward, other: over records with 0x1 and neither 0x4 nor 0x8, with
 *        refID == next_refID >= 0 and TLEN > 0 (which counts a pair once); 1 at min(TLEN, max_isize).  The row is `other` when 0x10
 *        and 0x20 are both set or both clear; otherwise, with POS <= next_pos, inward for a forward record and outward for a reverse
 *        one, and with POS > next_pos the other way round.
 *     f. BWAMS_QC_TABLE_INDEL [2][65], insertions then deletions: over mapped records, every I or D op of length n >= 1 adds 1 at
 *        min(n, 64).
 *  5. Scalars (the BWAMS_QC_* indices of bwams_qc_summary_t.scalars), under the same filter, every sum exact: reads; bases (the sum of
 *     l_seq); mapped; bases_mapped (the lengths of M I = X ops of mapped records); clipped (the lengths of S ops of mapped records);
 *     nm_sum and nm_missing over mapped records: NM is the first aux field tagged NM of type c C s S i or I with a value >= 0, and a
 *     record with no such field adds 1 to nm_missing; qual_sum (unclamped) and qual_bases over the bases table b takes; bases_over;
 *     no_qual.  The rest are reserved and stay 0.
 *  6. Accumulation.  64-bit counters in HBM, summed over any number of adds in any order; more than 2^31 - 1 records in ONE call is
 *     BWAMS_ERR_UNSUPPORTED with nothing added.  There is no finish step: a query sees everything added before it.  _reset zeroes.
 *  7. Text (bwams_qc_text).  A ratio a / b below is (double)a / (double)b.
 *     BWAMS_QC_TEXT_FLAGSTAT: sixteen lines "<class 0> + <class 1> <label>\n" in rule 2's order; a percentage is 100.0 * a / b printed
 *       with %.2f%%, or N/A when b is 0: mapped over total, primary mapped over primary, properly paired and singletons over paired.
 *       The example below:
 *         "9 + 1 in total (QC-passed reads + QC-failed reads)\n" "8 + 1 primary\n" "0 + 0 secondary\n" "1 + 0 supplementary\n"
 *         "0 + 1 duplicates\n" "0 + 1 primary duplicates\n" "8 + 1 mapped (88.89% : 100.00%)\n"
 *         "7 + 1 primary mapped (87.50% : 100.00%)\n" "8 + 0 paired in sequencing\n" "5 + 0 read1\n" "3 + 0 read2\n"
 *         "2 + 0 properly paired (25.00% : N/A)\n" "6 + 0 with itself and mate mapped\n" "1 + 0 singletons (12.50% : N/A)\n"
 *         "2 + 0 with mate mapped to a different chr\n" "1 + 0 with mate mapped to a different chr (mapQ>=5)\n"
 *     BWAMS_QC_TEXT_STATS: tab-separated lines, each tagged in its first column, in this order:
 *       SN <name> <value>: the eleven scalars under rule 5's names, then error_rate = nm_sum / bases_mapped with %.6e (0 with no
 *         mapped bases), average_quality = qual_sum / qual_bases with %.1f (0 with none), and insert_size_n, _mean, _sd, _median over
 *         the bins BELOW max_isize of all three rows together: n the count, S1 the sum of x * c and S2 of x * x * c as exact
 *         integers; mean S1 / n with %.1f; sd sqrt((double)(n * S2 - S1 * S1)) / (double)n with %.1f, the numerator formed in
 *         128-bit integers before the one conversion (they hold it for any n up to 2^40); median the smallest x whose cumulative count reaches (n + 1) / 2 (integer
 *         division); with n = 0 the three print 0.
 *       RL <length> <class 0> <class 1>: the occupied lengths.
 *       FFQ <cycle, from 1> <64 counts>: class 0's table b, a row per cycle up to its last occupied one; LFQ: class 1's.
 *       GCC <cycle, from 1> <A C G T N of class 0> <A C G T N of class 1>: a row per cycle up to the last occupied one of either.
 *       MAPQ <mapq> <count>, IS <size> <inward> <outward> <other>, ID <length> <insertions> <deletions>: the occupied rows.
 *     Example, with opt {0x900, 64, 100, 0}; each record is (FLAG, refID, POS, MAPQ, next_refID, next_pos, TLEN, CIGAR, SEQ, QUAL, NM),
 *     `-` for QUAL meaning 0xFF bytes and for NM no such field:
 *       (99,0,10,60,0,110,104,4M,ACGT,[30,30,20,10],0)      (147,0,110,60,0,10,-104,2M1I2M,ACGTA,[40,40,30,20,10],1)
 *       (73,0,50,30,0,50,0,1S3M,NACG,[2,30,30,30],1)        (133,0,50,0,0,50,0,*,TTT,[10,10,10],-)
 *       (2064,0,200,5,-1,-1,0,2M2D1M2H,ACG,[30,30,30],2)    (1536,0,5,0,-1,-1,0,3M,GGG,-,0)
 *       (81,0,300,60,0,340,42,2M,CC,[30,70],-)              (97,0,400,4,1,7,0,2M,AT,[30,30],0)
 *       (161,1,7,9,0,400,0,2M,GG,[30,30],0)                 (65,0,500,60,0,520,22,2M,AA,[30,30],0)
 *     flags {9,8,0,1,0,0,8,7,8,5,3,2,6,1,2,1} and {1,1,0,0,1,1,1,1,0,...}; the STATS text (a row's 64 counts shortened here to its
 *     occupied bins as bin:count; tests/test_qc.py holds the text in full):
 *       "SN\treads\t9\n" "SN\tbases\t27\n" "SN\tmapped\t8\n" "SN\tbases_mapped\t23\n" "SN\tclipped\t1\n" "SN\tnm_sum\t2\n"
 *       "SN\tnm_missing\t1\n" "SN\tqual_sum\t632\n" "SN\tqual_bases\t24\n" "SN\tbases_over\t0\n" "SN\tno_qual\t1\n"
 *       "SN\terror_rate\t8.695652e-02\n" "SN\taverage_quality\t26.3\n" "SN\tinsert_size_n\t2\n" "SN\tinsert_size_mean\t32.0\n"
 *       "SN\tinsert_size_sd\t10.0\n" "SN\tinsert_size_median\t22\n" "RL\t2\t3\t1\n" "RL\t3\t1\t1\n" "RL\t4\t2\t0\n" "RL\t5\t0\t1\n"
 *       FFQ 1 {2:1 30:3 63:1}  2 {30:5}  3 {20:1 30:1}  4 {10:1 30:1}       LFQ 1 {10:2 30:1}  2 {10:1 20:1 30:1}  3 {10:1 30:1}  4 {40:1}  5 {40:1}
 *       "GCC\t1\t3\t0\t2\t0\t1\t0\t0\t1\t2\t0\n" "GCC\t2\t2\t1\t2\t1\t0\t1\t0\t1\t1\t0\n" "GCC\t3\t0\t1\t2\t0\t0\t0\t1\t0\t1\t0\n"
 *       "GCC\t4\t0\t0\t1\t1\t0\t0\t0\t1\t0\t0\n" "GCC\t5\t0\t0\t0\t0\t0\t0\t0\t0\t1\t0\n"
 *       "MAPQ\t0\t1\n" "MAPQ\t4\t1\n" "MAPQ\t9\t1\n" "MAPQ\t30\t1\n" "MAPQ\t60\t4\n"
 *       "IS\t22\t0\t0\t1\n" "IS\t42\t0\t1\t0\n" "IS\t100\t1\t0\t0\n" "ID\t1\t1\t0\n"
 * bwams_qc_open: a zeroed handle on `device`; no reference lengths are needed; opt may be NULL for the defaults; max_cycle not a
 * multiple of 64 in [64, 4096], max_isize outside [1, 2^20], exclude above 0xFFFF or reserved != 0: BWAMS_ERR_ARG.  _close (NULL
 * allowed).  _add_batch: the batch's current BAM records (bwams_bam_run / _upload left them, BWAMS_ERR_ARG before either), read in
 * HBM; the batch must be on the handle's device.  _add_records: host records bam[0, n_bytes), uploaded; their block_size chain is
 * checked as bwams_bam_upload checks it (BWAMS_ERR_ARG).  *n_counted (may be NULL): the records of this call that rule 3's filter
 * let through.  _summary: rules 2 and 5.  _table: `what` of rule 4 into out[0, cap); *n (may be NULL) the number of int64 values,
 * written or needed; out may be NULL to ask for it; cap too small: BWAMS_ERR_CAPACITY.  _text: `what` of rule 7 into out[0, cap); *n:
 * the bytes written, or needed with BWAMS_ERR_CAPACITY, as bwams_pileup_text.  _info: a test and measurement hook, like
 * bwams_pileup_info (include/bwams_types.h).
 * An add runs three kernels.  qc_check_kernel: a lane per record, rule 1.  qc_record_kernel: a lane per record reads the head, walks
 * the CIGAR and the aux fields; the flag counters, MAPQ, INDEL, RL and the ISIZE bins below isize_lds are counted in LDS and flushed
 * once per workgroup; it also lists the filtered-in records per class.  qc_cycle_kernel: tables b and c without an atomic per base:
 * a wave owns a class, a block of 64 cycles and a slice of the class's list, a lane one cycle, whose 64 quality bins are a row of
 * LDS that no other lane touches.  Under BWAMS_QC_LANES=0 a plain kernel takes the listed records instead, with one global atomic
 * per base and per quality (the A/B baseline; the counters are the same).
 * bwams_sorter_set_qc: the conditions and guarantees of bwams_sorter_set_depth, without the length check (the handle has no
 * references): before the sorter's first put (BWAMS_ERR_ARG later, or for a handle on another device); the close adds every record of
 * the merged stream AS WRITTEN, after the merge has set or cleared 0x400, in whole records (one cut by a deflate piece's end is
 * counted once); the file and the index are byte for byte what they are without the call; an add that fails ends the close with its
 * error.  A sorter may have any of the depth, pileup and QC handles, alone or together: all see the same whole records. */
#define BWAMS_QC_TABLE_RL 0
#define BWAMS_QC_TABLE_QUAL 1
#define BWAMS_QC_TABLE_BASE 2
#define BWAMS_QC_TABLE_MAPQ 3
#define BWAMS_QC_TABLE_ISIZE 4
#define BWAMS_QC_TABLE_INDEL 5
#define BWAMS_QC_TEXT_FLAGSTAT 0
#define BWAMS_QC_TEXT_STATS 1
int bwams_qc_open(int device, const bwams_qc_opt_t *opt, bwams_qc_t **out);
int bwams_qc_close(bwams_qc_t *q);
int bwams_qc_reset(bwams_qc_t *q);
int bwams_qc_add_batch(bwams_qc_t *q, bwams_batch_t *b, int64_t *n_counted);
int bwams_qc_add_records(bwams_qc_t *q, const void *bam, int64_t n_bytes, int64_t *n_counted);
int bwams_qc_summary(bwams_qc_t *q, bwams_qc_summary_t *out);
int bwams_qc_table(bwams_qc_t *q, int32_t what, int64_t *out, int64_t cap, int64_t *n);
int bwams_qc_text(bwams_qc_t *q, int32_t what, char *out, int64_t cap, int64_t *n);
int bwams_qc_info(const bwams_qc_t *q, bwams_qc_info_t *info);
int bwams_sorter_set_qc(bwams_sorter_t *s, bwams_qc_t *q);
/* Base recalibration tables (csrc/recal.hip, csrc/api_recal.hip, host/recal_text.cpp): the counting half of base quality score
 * recalibration.  Every aligned base is compared with the reference and counted, as an observation and possibly as an error, per read
 * group, reported quality, machine cycle and dinucleotide context; positions of known variation are left out.  Accumulated on the
 * device from a batch's BAM records, from host records, or from the sorted BAM writer's merged stream.  Every value is an integer
 * count.  The rules are this library's own, modelled on the defaults of GATK BaseRecalibrator for the base-substitution event; no byte
 * parity with GATK's report is claimed.  bwams/recal.py restates them in numpy and is what the tests compare against.  The empirical
 * quality and the rewriting of QUAL are not part of this handle: they are the model and the apply handle of "Applying base
 * recalibration" below, which take these tables.
 *  1. Handle.  Opened on a device over n_ref reference lengths, an optional groups table (bwams_dup_groups_t; NULL: no read groups)
 *     and options: exclude (default 0x704, within 16 bits), min_mapq (1), min_baseq (6, in [0, 93]), max_cycle (500, at least 1),
 *     reserved (0).  Anything else, n_ref < 0 or a negative length is BWAMS_ERR_ARG.  The handle owns rule 6's four tables and a store
 *     of one nibble per position of every reference: the reference code 0..4 in bits 0-2, the known-site flag in bit 3, eight
 *     positions to a 32-bit word, every reference beginning a new word: l / 2 bytes for l positions (1.55 GB for GRCh38), so the
 *     whole genome sits beside an index.  BWAMS_ERR_NOMEM when the store or the tables do not fit.
 *  2. Reference.  Every code is 4 (N) until set.  _set_ref: host codes 0..4 for one whole reference (a code above 4: BWAMS_ERR_ARG,
 *     nothing set).  _set_ref_index: gathered on the device from the forward strand of an opened index's .0123 by the contig table,
 *     under the conditions of pileup rule 7 (BWAMS_ERR_ARG when the index has no .0123 or no contigs, is on another device, or its
 *     contig lengths differ); the .amb holes of an index made from FASTA become 4.  Neither touches the flags.
 *  3. Known sites.  _add_known takes n intervals (ref, beg, end) with 0 <= ref < n_ref and 0 <= beg < end <= l_ref[ref], in any order,
 *     overlapping freely.  A bad interval is BWAMS_ERR_ARG, bwams_last_error names the first, and nothing of that call is set.  The
 *     flags are the union over all calls.  _reset zeroes the tables and keeps the reference and the flags.
 *  4. Which records count.  (FLAG & exclude) == 0, MAPQ >= min_mapq, 0 <= refID < n_ref, n_cigar_op > 0, l_seq > 0 and a first QUAL
 *     byte other than 0xFF.  A record that fails is skipped, not refused.  Supplementary records count, as they do in GATK.
 *  5. Validity.  All records of a call are checked before anything is added.  BWAMS_ERR_ARG, bwams_last_error naming the first such
 *     record and its reason: an op code above 8, in ANY record (`op`); and for a record that passes rule 4, in this order: SEQ or QUAL
 *     ending behind the record's block_size (`bounds`; this comes before rule 4's look at the first QUAL byte, which such a record
 *     does not hold); a CIGAR query length (the lengths of M I S = X) other than l_seq (`length`); l_seq > max_cycle (`cycle`; GATK
 *     throws here too); and, when the handle has a groups table, aux fields that do not chain to the record's end as markdup rule 9
 *     walks them (`aux`).  Without a table the aux fields are not read.
 *  6. Keys and tables.  Read group g: the ordinal in the table of the record's first RG:Z value; n_rg for a record without RG:Z or with
 *     one the table does not hold; with no table n_rg = 0 and every record is in row 0.  Quality q = min(QUAL byte, 93).  Cycle of
 *     SEQ index i (0-based in SEQ as stored; soft clips are part of SEQ, hard clips are not): c = i + 1, or c = l_seq - i with FLAG
 *     0x10; negated when FLAG has both 0x1 and 0x80.  Context: two bases in sequencing order, (SEQ[i-1], SEQ[i]), or with 0x10
 *     (complement of SEQ[i+1], complement of SEQ[i]); it exists only when the neighbour exists and both codes are among 1, 2, 4, 8
 *     (the neighbour may lie in a clip or an insertion); the key is 4 * first + second with A C G T as 0..3.  Every cell of a
 *     table is two int64, observations then errors:
 *       BWAMS_RECAL_TABLE_RG      [n_rg + 1]
 *       BWAMS_RECAL_TABLE_QUAL    [n_rg + 1][94]
 *       BWAMS_RECAL_TABLE_CYCLE   [n_rg + 1][94][2 * max_cycle + 1], column c + max_cycle; the middle column stays 0
 *       BWAMS_RECAL_TABLE_CONTEXT [n_rg + 1][94][16]
 *  7. Which bases count.  A base is an observation when its op is M, = or X, its SEQ code is 1, 2, 4 or 8, its QUAL byte is at least
 *     min_baseq, its position lies in [0, l_ref), the reference code there is below 4 and the known flag there is clear.  It is also
 *     an error when it differs from the reference base.  A base without a context counts in the other three tables only.  I, D, N,
 *     S, H and P only advance; insertion and deletion events are out of scope.
 *     Example: reference c1 = ACGTACGT, one @RG ID:a; record 1: 8M ACGTACGT at 0, forward, quality 30, RG:Z:a; record 2: 8M ACTTACGT
 *     at 0 with FLAG 0x10, quality 30, RG:Z:a (the machine read ACGTAAGT).  RG[a] = 16 observations, 1 error; CYCLE[a][30][cycle 6] =
 *     2 observations, 1 error; CONTEXT[a][30][AA] = 1 observation, 1 error; no other error anywhere.  With position 2 flagged as
 *     known the error and both observations at that position vanish.
 *  8. Accumulation.  As pileup rule 6: the tables hold the sums over any number of adds in any order; there is no finish step; more
 *     than 2^31 - 1 records given in total is BWAMS_ERR_UNSUPPORTED with nothing of that call added; after BWAMS_ERR_DEVICE the
 *     tables are undefined until _reset.
 *  9. Queries.  _table: table `what` of rule 6 as int64 pairs into out[0, cap); *n (may be NULL) the number of int64 values, written
 *     or needed; out may be NULL to ask for it; cap too small: BWAMS_ERR_CAPACITY.  _info: a test and measurement hook
 *     (bwams_recal_info_t, include/bwams_types.h).
 * 10. Text.  _text writes tab-separated rows, only those with observations > 0, in table order:
 *       "RG\t<id>\t<obs>\t<err>\n"  "QUAL\t<id>\t<q>\t<obs>\t<err>\n"  "CYCLE\t<id>\t<q>\t<cycle>\t<obs>\t<err>\n"
 *       "CONTEXT\t<id>\t<q>\t<XY>\t<obs>\t<err>\n"
 *     <id> is the read group's ID in `names`, a groups table with the handle's number of read groups (NULL for a handle opened
 *     without one; anything else is BWAMS_ERR_ARG), and `*` for the last row.  The example gives "CONTEXT\ta\t30\tAA\t1\t1\n".  *n: the
 *     bytes written, or needed with BWAMS_ERR_CAPACITY, as bwams_qc_text.
 * bwams_recal_open, _close (NULL allowed), _reset, _add_batch and _add_records: as their bwams_pileup_ namesakes; the groups table is
 * copied, the caller may destroy it.  *n_counted (may be NULL): the records of this call that rule 4 let through.
 * An add checks (recal_check_kernel, a lane per record), finds each record's read group and lists the counted records by (read
 * group, sign of the cycles) with a radix sort, and then counts without a global atomic per base: a workgroup of recal_base_kernel owns
 * a read group, a block of 64 cycles and a slice of the group's records, a lane one cycle of a record; CYCLE and CONTEXT are counted
 * in LDS and flushed once per workgroup and slice, QUAL and RG folded from CYCLE at the flush.  Under BWAMS_RECAL_LDS=0 a plain kernel
 * takes the records instead, a lane per base and one global atomic per update (the A/B baseline; the tables are the same).
 * bwams_sorter_set_recal: the conditions and guarantees of bwams_sorter_set_depth: before the sorter's first put (BWAMS_ERR_ARG later,
 * for a handle on another device, or when the handle's lengths differ from the sorter header's); the close adds every record of the
 * merged stream AS WRITTEN, after the merge has set or cleared 0x400, so duplicates drop out by `exclude`, in whole records (one cut
 * by a deflate piece's end is counted once); the file and the index are byte for byte what they are without the call; an add that
 * fails ends the close with its error.  A sorter may have any of the depth, pileup, QC and recalibration handles, alone or together.
 * bwams_dup_groups_rg_id: the ID of read group rg of a groups table (NULL outside [0, n_rg) or without a table), as
 * bwams_dup_groups_library gives a library's name. */
#define BWAMS_RECAL_TABLE_RG 0
#define BWAMS_RECAL_TABLE_QUAL 1
#define BWAMS_RECAL_TABLE_CYCLE 2
#define BWAMS_RECAL_TABLE_CONTEXT 3
int bwams_recal_open(int device, const int32_t *l_ref, int32_t n_ref, const bwams_dup_groups_t *groups, const bwams_recal_opt_t *opt,
                     bwams_recal_t **out);
int bwams_recal_close(bwams_recal_t *r);
int bwams_recal_reset(bwams_recal_t *r);
int bwams_recal_add_batch(bwams_recal_t *r, bwams_batch_t *b, int64_t *n_counted);
int bwams_recal_add_records(bwams_recal_t *r, const void *bam, int64_t n_bytes, int64_t *n_counted);
int bwams_recal_set_ref(bwams_recal_t *r, int32_t ref, const uint8_t *codes);
int bwams_recal_set_ref_index(bwams_recal_t *r, const bwams_index_t *ix);
int bwams_recal_add_known(bwams_recal_t *r, const bwams_recal_site_t *sites, int64_t n);
int bwams_recal_table(bwams_recal_t *r, int32_t what, int64_t *out, int64_t cap, int64_t *n);
int bwams_recal_text(bwams_recal_t *r, const bwams_dup_groups_t *names, char *out, int64_t cap, int64_t *n);
int bwams_recal_info(const bwams_recal_t *r, bwams_recal_info_t *info);
int bwams_sorter_set_recal(bwams_sorter_t *s, bwams_recal_t *r);
const char *bwams_dup_groups_rg_id(const bwams_dup_groups_t *g, int64_t rg);
/* Applying base recalibration (host/recal_model.cpp, csrc/recal_apply.hip, csrc/api_recal_apply.hip): the other half of base quality
 * score recalibration.  A quality model is made on the host from the four tables above, and an apply handle rewrites the QUAL bytes
 * of BAM records on the device with it.  The flow has two passes: count (bwams_recal_add_*), then bwams_recal_model_from, then apply.
 * The rules are this library's own, in the spirit of GATK's hierarchical model: read group, then reported quality, then cycle and
 * context deltas, sparse cells shrunk towards their parent; no parity with GATK's output is claimed.  Every value is an exact
 * integer: no floating point and no libm call stands between the tables and the new bytes.  bwams/recal_apply.py restates all of it
 * in Python integers and numpy and is what the tests compare against.
 * The model.
 *   Constants, committed as literals in host/recal_model.cpp and returned by bwams_recal_model_constants (S[k] at S[k - 1]):
 *     S[k], k = 1..60: the largest integer s with s^20 <= 2^320 * 10^(2k - 1), that is floor(2^16 * 10^((2k - 1) / 20));
 *     P[q], q = 0..93: the largest integer p with p^10 * 10^q <= 2^400, that is floor(2^40 * 10^(-q / 10)).
 *   phred(num, den, cap) = the number of k in 1..cap with num * S[k] <= den << 16: round(-10 log10(num / den)) clamped to [0, cap].
 *   post(n, e, Qp) = phred((e << 40) + m * P[Qp], (n + m) << 40, max_q): the quality of a cell of n observations and e errors after
 *     m = prior_obs pseudo-observations at the prior quality Qp in [0, 93].  post(0, 0, q) = min(q, max_q).
 *   Options (bwams_recal_model_opt_t; NULL: {0, 6, 60, 1024, 0}): exclude within 16 bits, preserve_below in [0, 93], max_q in [1, 60],
 *     prior_obs in [1, 2^20], reserved 0; anything else is BWAMS_ERR_ARG.  A negative count, a cell with more errors than
 *     observations, or a count of 2^40 or more is BWAMS_ERR_UNSUPPORTED: below 2^40 every product above stays below 2^128.
 *   Values, for each row g in [0, n_rg] (n_rg: the row of records without a known read group):
 *     RG       with RG[g].obs > 0: E = sum over q of QUAL[g][q].obs * P[q]; Qrep[g] = phred(E, RG[g].obs << 40, max_q);
 *              QG[g] = post(RG[g], Qrep[g]); G[g] = QG[g] - Qrep[g].  Otherwise Qrep = QG = -1 and G = 0.
 *     QUAL     Qp = clamp(q + G[g], 0, 93); B[g][q] = post(QUAL[g][q], Qp) for a cell with observations, else Qp.
 *     CYCLE    DC[g][q][c] = post(CYCLE[g][q][c], B[g][q]) - B[g][q] for a cell with observations, else 0;
 *     CONTEXT  DX[g][q][x] likewise.  Every delta lies in [-93, 60].
 *   Example: the tables of the example of recalibration rule 7, default options: Qrep[a] = 30, QG[a] = 27, G[a] = -3; B[a][30] = 25,
 *   B[a][37] = 34 (no data), B[*][30] = 30; DC[a][30] is -1 at cycle 6 and DX[a][30] is -1 at AA, every other delta is 0.
 *   bwams_recal_model_create takes the four tables as int64 pairs, laid out as bwams_recal_table returns them; _model_from fetches
 *   them from a handle.  _model_table: `what` and the capacity protocol of bwams_recal_table, int16 values: RG [n_rg + 1][3] =
 *   (Qrep, QG, G); QUAL B [n_rg + 1][94]; CYCLE DC [n_rg + 1][94][2 * max_cycle + 1]; CONTEXT DX [n_rg + 1][94][16].  _model_destroy:
 *   NULL allowed.  A model is plain host memory and is not tied to a device.
 * Applying it.  bwams_recal_apply_open copies the model (B and the deltas as bytes) and the groups table to a device; the model and
 * the table may be destroyed afterwards.  groups may be NULL only for a model with n_rg = 0; a table whose number of read groups is
 * not the model's is BWAMS_ERR_ARG.  _close: NULL allowed.
 *  A. Which records are rewritten.  (FLAG & exclude) == 0, l_seq > 0 and a first QUAL byte other than 0xFF.  Unmapped records,
 *     duplicates and secondary records are rewritten too, as in GATK; MAPQ, refID and the CIGAR's content are not looked at.  Every
 *     other record stays byte for byte.
 *  B. Validity.  All records of a call are checked before any byte is written; BWAMS_ERR_ARG, bwams_last_error naming the first bad
 *     record and its reason, and the caller's bytes and the batch's records unchanged.  For a record that passes the FLAG and l_seq
 *     conditions of A, in this order: SEQ or QUAL ending behind the record's block_size (`bounds`; before the look at the first QUAL
 *     byte); l_seq > the model's max_cycle (`cycle`); and, with a groups table, aux fields that do not chain to the record's end
 *     (`aux`).
 *  C. Which bases.  A base whose QUAL byte is below preserve_below keeps it.  Every other base of a rewritten record gets
 *     clamp(B[g][q] + DC[g][q][cycle] + DX[g][q][context], 1, max_q) with q = min(byte, 93) and g, cycle and context exactly as
 *     recalibration rule 6 defines them; where that rule gives no context (the first base in sequencing order; a base whose own code
 *     or whose neighbour's is not A, C, G or T) DX counts as 0.  The base's own SEQ code does not otherwise matter.  Nothing but QUAL
 *     bytes changes and no record changes its size.  Applying twice is NOT idempotent: the second pass reads the first one's output
 *     as reported qualities.
 *     Example: on the two records of that example, record 1 becomes 25 everywhere but stored index 5 (cycle 6), which becomes 24;
 *     record 2 becomes 25 everywhere but stored index 2 (its cycle 6, context AA), which becomes 23 = 25 - 1 - 1.  With a model of
 *     all-zero tables every byte b >= 6 becomes min(b, 93, max_q): 200 becomes 60.
 * bwams_recal_apply_records rewrites host records in place (their block_size chain is checked as bwams_recal_add_records checks it).
 * bwams_recal_apply_batch rewrites the batch's BAM records where they lie (of bwams_bam_run or bwams_bam_upload; BWAMS_ERR_ARG
 * before either), and their sorted copy when the current records have one, as bwams_bam_markdup does: bwams_bam_fetch, _fetch_bgzf,
 * _sort and _sorted_fetch all see the new bytes.  The templates of bwams_bam_templates are outdated by it.  *n_rewritten (may be
 * NULL): the records rule A took.
 * The kernels: a check (a lane per record), a record kernel for the read group and the key 2 * group + (cycles negative), and
 * recal_apply_kernel, a wave per rewritten record and a lane per base, the model's three values of a base by global loads (a model
 * is some 30 KB a read group at 150 cycles and stays in cache) and one byte store.  A second rewrite kernel that staged the model's
 * rows in LDS over records sorted by key was measured against it, was slower, and is not in the library.  _info: a
 * test and measurement hook (bwams_recal_apply_info_t, include/bwams_types.h).
 * Out of scope: applying inside the sorted BAM writer (its counting happens at close, so no model can exist before its stream is
 * written); OQ tags; quantised output qualities; insertion and deletion events; a model read back from bwams_recal_text. */
int bwams_recal_model_create(const int64_t *rg, const int64_t *qual, const int64_t *cycle, const int64_t *context, int32_t n_rg,
                             int32_t max_cycle, const bwams_recal_model_opt_t *opt, bwams_recal_model_t **out);
int bwams_recal_model_from(bwams_recal_t *r, const bwams_recal_model_opt_t *opt, bwams_recal_model_t **out);
int bwams_recal_model_table(const bwams_recal_model_t *m, int32_t what, int16_t *out, int64_t cap, int64_t *n);
int bwams_recal_model_constants(int64_t S[60], int64_t P[94]);
int bwams_recal_model_destroy(bwams_recal_model_t *m);
int bwams_recal_apply_open(int device, const bwams_recal_model_t *model, const bwams_dup_groups_t *groups, bwams_recal_apply_t **out);
int bwams_recal_apply_close(bwams_recal_apply_t *a);
int bwams_recal_apply_records(bwams_recal_apply_t *a, void *bam, int64_t n_bytes, int64_t *n_rewritten);
int bwams_recal_apply_batch(bwams_recal_apply_t *a, bwams_batch_t *b, int64_t *n_rewritten);
int bwams_recal_apply_info(const bwams_recal_apply_t *a, bwams_recal_apply_info_t *info);

/* ------------------------------------------------ BAM file by region ---- */

/* A coordinate-sorted BAM file and its BAI (what bwams_sorter_close writes, or any other writer) read back as device records: the
 * handle turns (file, index, regions) into pieces of records in HBM, which bwams_bam_file_fetch copies out and the five record
 * consumers (depth, pileup, QC, recalibration and its apply) take where they lie.  bwams/bai.py restates the rules (overlapping,
 * plan).  The file is untrusted input: everything below that can be wrong with it is an error return.
 *  1. Overlap.  A record overlaps region (ref, beg, end) when its refID == ref, POS < end and its end > beg; the end is
 *     bwams_bam_coord_t's: POS + the CIGAR's reference length, or POS + 1 for FLAG 0x4, no CIGAR or a reference length of 0.
 *  2. Regions.  0 <= ref < n_ref and 0 <= beg < end each (BWAMS_ERR_ARG otherwise); in any order, overlapping or not.  They are
 *     sorted by (ref, beg) and merged per reference where they overlap or touch before anything else, so a record that overlaps
 *     several regions comes back once.  Records come back in file order.
 *  3. Plan.  For every merged region: the chunks of the bins of reg2bins over [beg, end) (SAMv1 section 5.3; levels that the
 *     coordinate overruns give no bin, and pseudo-bin 37450 is never a source of chunks) that end past the linear index's offset of
 *     beg's 16 kb window (the window index clamped to the last entry; an empty linear index gives offset 0), each chunk's start
 *     clipped to that offset.  The chunks of all regions are sorted by virtual offset and those that touch or overlap merged into
 *     disjoint intervals.  bwams_bai_plan returns exactly these intervals from the bytes of a BAI (host only, no device; *n_chunks
 *     their number, BWAMS_ERR_CAPACITY when cap is smaller; n_regions 0 gives none; n_ref is the index's).
 *  4. Whole file (n_regions 0).  One interval from the first record behind the header to the end of the data; every record is kept,
 *     unplaced ones (refID -1) included, and no index is needed.
 *  5. Pieces.  Within an interval a piece is a run of whole BGZF members whose inflated size fits piece_bytes (0: 128 MiB; a piece
 *     costs the inflater one call, so few large ones are faster; the handle holds some ten times piece_bytes of device memory).
 *     Bytes behind the last whole record of a piece are carried, on the device, in front of the next piece of the same interval.  The
 *     record chain of an interval's first piece starts at the in-block offset of the interval's start and stops at the interval's
 *     end offset.  A piece may yield 0 records; *done is set together with the last piece, which may be empty.  A single record
 *     larger than piece_bytes is BWAMS_ERR_CAPACITY, with its size in the text.
 *  6. Refusals.  No index and n_regions > 0: BWAMS_ERR_ARG.  An index whose n_ref differs from the header's, or that is cut off:
 *     BWAMS_ERR_IO at open.  A chunk that points past the file or not at a member, a member that fails CRC or ISIZE, a chain
 *     that reaches a position where no well-formed record starts (rule 1 of bwams_bam_reads_decode; a record cut off by the end
 *     of a piece is the carry, not an error, while members follow), a record with refID < -1 or POS outside [-1, 2^31 - 2]:
 *     BWAMS_ERR_IO from bwams_bam_file_next, with the file offset of the piece and the record's ordinal in the query; the query is
 *     over then.  _next, _fetch and the consumers' _file calls before _query, _fetch and those before the first _next, or any of
 *     them after a _next that followed the last piece: BWAMS_ERR_ARG with a text.  A consumer on another device: refused as a
 *     batch on another device is.
 * bwams_bam_file_open: bai_path NULL takes <path>.bai when it can be read and no index otherwise.  _header and _refs: the header
 * text (not NUL terminated; it lives as long as the handle), n_ref, and the references' lengths (cap >= n_ref).  _query starts a
 * query and ends the one before; _next makes the next piece current (*n_records, *n_bytes: its kept records); _fetch copies the
 * current piece's records (cap >= *n_bytes, BWAMS_ERR_CAPACITY otherwise) and, when coords is not NULL, their *n_records coords to
 * the host.  The consumers' _add_file calls add the current piece exactly as their _add_records calls add host records, with the
 * same checks and counts; bwams_recal_apply_file rewrites the piece where it lies, so that _fetch then returns the new bytes.  The
 * piece stays current until the next _next or _query.  One caller at a time.
 * The kernels: the record discovery of bwams_bam_reads_decode (csrc/bam_discover.h) from an offset to an offset; a select kernel, a
 * lane per record, with the merged regions in LDS; two scans; the sorter's gather into the handle's record buffer.  _info: a test
 * and measurement hook (bwams_bam_file_info_t, include/bwams_types.h).
 * A sixth consumer of the pieces is the join handle below: bwams_dupjoin_add_file and bwams_dupjoin_apply_file; a seventh the
 * collate handle behind it: bwams_collate_add_file.
 * An eighth is the SAM view (bwams_samview_add_file).  Several files as one stream: bwams_bam_file_open_merge below, whose handle
 * every call here takes unchanged.
 * Out of scope: CRAM, CSI and tabix indexes, unsorted input beyond whole-file mode, writing; of the merge: renaming @RG IDs that
 * collide, files whose reference lists differ, prefetching a child's next piece while the current round merges, one inflater call
 * over members of several files, a writer that takes an ordered stream directly (bwams_sorter_put merges its runs once more). */
int bwams_bam_file_open(const char *path, const char *bai_path, int device, int64_t piece_bytes, bwams_bam_file_t **out);
int bwams_bam_file_header(const bwams_bam_file_t *f, const char **text, int64_t *n_text, int32_t *n_ref);
int bwams_bam_file_refs(const bwams_bam_file_t *f, int32_t *l_ref, int32_t cap);
int bwams_bam_file_query(bwams_bam_file_t *f, const bwams_pileup_region_t *regions, int32_t n_regions);
int bwams_bam_file_next(bwams_bam_file_t *f, int64_t *n_records, int64_t *n_bytes, int32_t *done);
int bwams_bam_file_fetch(bwams_bam_file_t *f, void *bam, int64_t cap, bwams_bam_coord_t *coords);
int bwams_bam_file_info(const bwams_bam_file_t *f, bwams_bam_file_info_t *info);
int bwams_bam_file_close(bwams_bam_file_t *f);
int bwams_depth_add_file(bwams_depth_t *d, bwams_bam_file_t *f, int64_t *n_counted);
int bwams_pileup_add_file(bwams_pileup_t *p, bwams_bam_file_t *f, int64_t *n_counted);
int bwams_qc_add_file(bwams_qc_t *q, bwams_bam_file_t *f, int64_t *n_counted);
int bwams_recal_add_file(bwams_recal_t *r, bwams_bam_file_t *f, int64_t *n_counted);
int bwams_recal_apply_file(bwams_recal_apply_t *a, bwams_bam_file_t *f, int64_t *n_rewritten);
int bwams_bai_plan(const void *bai, int64_t n_bai, const bwams_pileup_region_t *regions, int32_t n_regions, uint64_t *chunk_beg,
                   uint64_t *chunk_end, int64_t cap, int64_t *n_chunks);

/* Several coordinate-sorted BAM files (a sample's lanes, flow cells, the shards bwams_writer_* and bwams_multi_* write) merged as one
 * record stream, what `samtools merge` gives: bwams_bam_file_open_merge returns a bwams_bam_file_t that is the merge of n_files files.
 * Each child file is inflated and its records are found in HBM as above; HIP kernels (csrc/bam_merge.hip) merge the children's
 * pieces into pieces in coordinate order, which _query / _next / _fetch, the eight _add_file calls, bwams_recal_apply_file and
 * bwams_dupjoin_apply_file take as they take one file's.  _header, _header_block and _refs give the merged header, _info the sums
 * over the children, _close closes them.  bwams/merge.py restates the rules (merge_records, merge_header, rounds).
 *  M1. Inputs.  n_files in [1, 64] (a lane of one wave per file), every path given; BWAMS_ERR_ARG otherwise.  bai_paths may be
 *      NULL and so may each entry: bwams_bam_file_open's rule per file.  The handle opens and owns its children on `device`, each
 *      with piece size child_bytes: opt->child_bytes, or with 0 / opt NULL piece_bytes / n_files rounded down to a multiple of 65536
 *      (piece_bytes 0: 128 MiB).  child_bytes below 65536: BWAMS_ERR_ARG, the text giving the smallest piece_bytes that would do.
 *      opt->reserved != 0: BWAMS_ERR_ARG.  A child that cannot be opened: that child's code, "file k (path): " before its text.
 *  M2. References.  Every file must have file 0's n_ref and per reference the same name bytes and length: BWAMS_ERR_UNSUPPORTED at
 *      open otherwise, naming the file, the reference's ordinal and what differs.  No refID is ever rewritten.
 *  M3. Header text (bwams_bam_header_merge, host only, host/bam_merge_header.cpp).  A text's lines end at '\n'; NUL padding behind
 *      the text and empty lines are no lines; every line is written with its '\n'.  The @HD line and all @SQ lines come from file 0
 *      as they are (those of the other files are not looked at: M2 compares the binary lists).  Then, for file 0, 1, ...: every other
 *      line in file order that is not byte-equal to a line already taken.  An @RG line whose ID equals an ID already taken, with
 *      other bytes: BWAMS_ERR_UNSUPPORTED naming both files and the ID (samtools merge renames the ID and rewrites RG:Z; silently
 *      changing library membership is worse than refusing).  An @PG line in that situation is dropped and counted in *pg_dropped
 *      (two lanes through one pipeline always collide here, and the ID that records may name still exists).  The block written is a
 *      BAM header block as bwams_bam_file_header_block gives it: magic, l_text, text, n_ref, file 0's references.  *n_out: its size,
 *      BWAMS_ERR_CAPACITY when cap is smaller (bwams_bai_plan's convention).  A block that is cut off or has another magic:
 *      BWAMS_ERR_ARG, naming the file.  Bytes behind a block's last reference are not looked at.
 *  M4. Order.  The merged stream of the whole file holds every record of every file once, that of a query every kept record once,
 *      ordered by (bwams_bam_coord_t.key, file index, ordinal within the file), each record byte for byte and with its coord: what
 *      bwams_sorter_close gives when file k is put as the run with seq = k.
 *  M5. Sorted input is checked, not assumed.  A file's kept records must have non-decreasing keys, also across its pieces.  The
 *      first violation ends the query with BWAMS_ERR_IO from _next: "file k (path): record r: key below its predecessor's", r the
 *      ordinal among that file's kept records of this query (when several files break the rule in one round: the lowest file).
 *  M6. Query.  _query passes the same regions to every child.  n_regions > 0 with a child that has no index: BWAMS_ERR_ARG naming
 *      the file.  Bad regions are refused by file 0 for all and leave the last query's state, as on one file; a query that a
 *      later file refuses (an I/O error) comes back with the file prefix and leaves the handle without a query.  A child's error
 *      from _next comes back with the file prefix and ends the query.  Rule 6's refusals by state hold
 *      with the same texts.
 *  M7. Rounds, defined so that the output cannot depend on timing.  Each child has a WINDOW, the not yet emitted tail of its current
 *      piece, and is OPEN while it has pieces to come.  Before a round every open child with an empty window is advanced, again
 *      while its pieces come back empty.  L_j: the key of the last record in open child j's window; F = min L_j; i* the smallest j
 *      with L_j = F.  Child j emits its window's records with key < F and, when j <= i*, those with key = F.  With no open child
 *      every window is emitted whole, and that round's piece is the last.  The emitted records in M4's order are the handle's next
 *      piece; it may be empty.  Why j <= i*: an open child j < i* has L_j > F, so all its records of key F are in its window, and
 *      a closed child's are too; child i* empties its window in every round, so a run of equal keys longer than a piece (all
 *      unplaced reads of a file share one key) makes progress.
 *  M8. Pieces are a function of the input: their boundaries depend only on the files' bytes, the query and child_bytes, so two
 *      queries give the same pieces (rule J8 of the join holds in pass 2).  A piece holds at most the sum of the children's current
 *      pieces, each at most 2 x child_bytes (carry plus inflated); the output buffers grow on demand, and a failed allocation is
 *      BWAMS_ERR_NOMEM with the size asked for and ends the query.  The children that need a piece in one round are advanced
 *      concurrently, a host thread each and at most 16 at a time (each child has its own stream and inflater), which decides nothing.
 *  M9. bwams_bam_merge_info (bwams_bam_merge_info_t, include/bwams_types.h): a test and measurement hook; on a plain handle
 *      BWAMS_ERR_ARG.
 * The kernels of a round, on the handle's stream, the children read in place: bm_check (M5, a lane per record of a new piece),
 * bm_frontier (one wave, a lane per child: F, i*, each child's emit count by binary search, a wave prefix sum), bm_rank (a lane per
 * emitted record: its place from K - 1 binary searches over the other children's keys), one rocPRIM scan of the sizes, bm_gather
 * (kGroup lanes per record from K source buffers). */
int bwams_bam_file_open_merge(const char *const *paths, const char *const *bai_paths, int32_t n_files, int device, int64_t piece_bytes,
                              const bwams_bam_merge_opt_t *opt, bwams_bam_file_t **out);
int bwams_bam_merge_info(const bwams_bam_file_t *f, bwams_bam_merge_info_t *info);
int bwams_bam_header_merge(const void *const *blocks, const int64_t *n_block, int32_t n_files, void *out, int64_t cap, int64_t *n_out,
                           int32_t *pg_dropped);
/* ------------------------------ Duplicate marking, templates joined by name ---- */

/* Duplicate marking of records that are NOT query-grouped (csrc/dup_join.hip): a coordinate-sorted BAM of another aligner, of an older
 * run, or one written without BWAMS_SORT_MARKDUP.  A sixth record consumer, bwams_dupjoin_t, on one device, used in two passes over
 * the same records: pass 1 adds every piece and keeps a small entry per record in HBM; _finish joins the entries into templates by
 * read name and decides; pass 2 sets or clears 0x400 in each piece where it lies.  After bwams_dupjoin_apply_file,
 * bwams_bam_file_fetch returns the marked bytes and their coords, bwams_sorter_put takes them as they are, and the other consumers'
 * _add_file on the same piece sees the marks.  bwams/markdup.py restates the rules (name_key, join, mark_joined).
 * Rules 2 to 15 of "Duplicate marking" (above bwams_bam_templates) hold unchanged except where a rule below says otherwise.  "Add
 * order" is the order of the _add_* calls, then record order within each; a record's ORDINAL is its 0-based place in add order.
 *  J1. Name key.  L = l_read_name - 1, the name without its NUL.  For each of two seeds S0 = 0x9e3779b97f4a7c15 and S1 =
 *      0xc2b2ae3d27d4eb4f: h = S ^ L; then for i in [0, max(1, ceil(L / 8))): h = fmix64(h ^ w_i), where w_i is the name's bytes
 *      [8i, 8i + 8) as a little-endian 64-bit word, zero-padded past L, and fmix64 is MurmurHash3's finalizer (h ^= h >> 33; h *=
 *      0xff51afd7ed558ccd; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53; h ^= h >> 33; mod 2^64).  The key is (k0, k1).  "r1" gives
 *      (f725c5a0830ac16d, b55003a821483129).  Names of at most 8 bytes cannot collide within one length: one bijective step.
 *  J2. Template: all added records with equal (L, k0, k1), adjacent or not.  This replaces rule 1.  Its ordinal is its rank by the
 *      ordinal of its first record.  Two different names with equal L and key would be taken for one template (among 2^32 names
 *      the chance of any such pair is below 2^-65, but the file is untrusted input and such names can be constructed): the
 *      consequence is a wrong 0x400 or a refusal by rule 2, never an access out of bounds, since no index the kernels store through
 *      depends on a name.  More than 2^32 - 1 records: BWAMS_ERR_UNSUPPORTED.
 *  J3. The walk.  Rules 2 to 5 are applied to a template's records in ordinal order: "the earlier record" of rule 5 is the one with
 *      the smaller ordinal, and "the first record concerned" of rule 2 is the smallest ordinal at which any template's walk meets a
 *      fault.  Consequence: two primaries of one segment that share a name are refused wherever they lie (for example two
 *      single-end reads of one name at two places of a sorted file), where the adjacent-run rule takes them for two templates when
 *      they are apart.
 *  J4. Read group, library, location.  Rules 9 and 10 take the template's first primary in add order, or its first record when it has
 *      no primary.  With a groups table EVERY added record's aux fields are walked at the add (aux_first_rg), also those of records
 *      rule 9 never names: a record that does not chain refuses that add with BWAMS_ERR_UNSUPPORTED and the fifth reason ("aux fields
 *      do not chain to the record's end"), naming the smallest such ordinal, and the handle is left as it was before the add.
 *      Without a table no aux field is read.
 *  J5. Decision and tie-breaks.  Rule 6 and rules 11 to 13 apply, through the same kernels over device ends (no round trip of the
 *      ends through the host).  "Earlier template" means the smaller template ordinal of J2.
 *  J6. Marking.  Rule 7 applies: every record of a duplicate template is marked, secondary, supplementary and unmapped-mate records
 *      included, wherever they lie in the file.  This is what the query-grouped path does; it is more than Picard does on
 *      coordinate-sorted input, where records that are not primaries keep their flags.
 *  J7. Defined over what was added.  A paired primary whose mate was never added makes a fragment, so a region query in pass 1 gives
 *      marks that hold only for those records.  The whole file (n_regions 0) is the intended input.
 *  J8. Pass 2.  Apply call i takes the records of add i.  Before any byte is written, a check kernel compares the piece's record
 *      count, the sum mod 2^64 of its k0 and the sum of (2r + 1) * k0 over its records r = 0, 1, ... (a plain sum cannot see two
 *      names exchanged) with what add i left; a mismatch is BWAMS_ERR_ARG with a text, nothing is written, and the same apply may be
 *      tried again.
 *  J9. States: empty -> adding -> finished.  BWAMS_ERR_ARG with a text for _add_* after _finish, for _apply_* or _fetch before it, for
 *      an apply past the last add, and for a file on another device.  A refusal at _finish (rules 2 and 3) leaves the handle fit
 *      only for _reset or _close.  _reset returns to empty and keeps the table and the options.
 * Counts: bwams_dup_stats_t and the bwams_dup_lib_stats_t rows (may be NULL; cap_lib < n_lib: BWAMS_ERR_CAPACITY) come complete
 * from _finish; records_marked is the number of records whose template is a duplicate, known before pass 2.
 * bwams_dup_metrics_text takes the rows unchanged.
 * bwams_dupjoin_open: groups (copied) and opt may both be NULL.  _add_records / _add_file: *n_added the records of the add; an add
 * of no records is an add.  _fetch (after _finish): the ends and their locs (cap_ends), each record's template by ordinal (cap_rec),
 * dup and optical per template (cap_tmpl); any pointer may be NULL; a capacity too small for a pointer given is
 * BWAMS_ERR_CAPACITY.  _apply_records rewrites host records in place; _apply_file the file's current piece in HBM; *n_marked the
 * records that now carry 0x400.  _key: J1 on the host (n in [0, 254]).  bwams_bam_file_header_block: the file's BAM header as
 * bwams_sorter_open takes it (it lives as long as the file handle).
 * Memory: 57 bytes of device memory per record while adding (the key 16, L 1, the coordinate, refID, FLAG and score 16, the
 * record's library, read group and location 24), in arrays grown by half; _finish adds 33 bytes per record of sort scratch and rocPRIM's
 * own, and frees all of it but 4 bytes per record (rec_tmpl) and 2 per template.  What does not fit is BWAMS_ERR_NOMEM with the size
 * asked for.  _info: a test and measurement hook (bwams_dupjoin_info_t, include/bwams_types.h).
 * Out of scope: batches (a batch's templates are adjacent: bwams_bam_markdup serves them); lifting bwams_sorter_put's refusal under
 * BWAMS_SORT_MARKDUP (the follow-up this handle makes possible); storing names to verify keys; the DT tag, REMOVE_DUPLICATES, UMIs.
 * Several files (the lanes of a library): both passes over a handle of bwams_bam_file_open_merge, whose pieces are the same in
 * both (rule M8), so that J8 holds. */
int bwams_dupjoin_open(int device, const bwams_dup_groups_t *groups, const bwams_dup_opt_t *opt, bwams_dupjoin_t **out);
int bwams_dupjoin_reset(bwams_dupjoin_t *j);
int bwams_dupjoin_close(bwams_dupjoin_t *j);
int bwams_dupjoin_add_records(bwams_dupjoin_t *j, const void *bam, int64_t n_bytes, int64_t *n_added);
int bwams_dupjoin_add_file(bwams_dupjoin_t *j, bwams_bam_file_t *f, int64_t *n_added);
int bwams_dupjoin_finish(bwams_dupjoin_t *j, bwams_dup_stats_t *st, bwams_dup_lib_stats_t *lib_stats, int64_t cap_lib);
int bwams_dupjoin_fetch(bwams_dupjoin_t *j, bwams_dup_end_t *ends, bwams_dup_loc_t *loc, int64_t cap_ends, uint32_t *rec_tmpl,
                        int64_t cap_rec, uint8_t *dup, uint8_t *optical, int64_t cap_tmpl);
int bwams_dupjoin_apply_records(bwams_dupjoin_t *j, void *bam, int64_t n_bytes, int64_t *n_marked);
int bwams_dupjoin_apply_file(bwams_dupjoin_t *j, bwams_bam_file_t *f, int64_t *n_marked);
int bwams_dupjoin_info(const bwams_dupjoin_t *j, bwams_dupjoin_info_t *info);
int bwams_dupjoin_key(const void *name, int32_t n, uint64_t key[2]);
int bwams_bam_file_header_block(const bwams_bam_file_t *f, const void **block, int64_t *n);

/* ------------------------------ Collating a coordinate-sorted BAM by read name ---- */

/* Re-aligning an existing BAM starts from a coordinate-sorted file, while a paired chunk of bwams_process_chunk_bam wants the two
 * ends of a pair next to each other.  A seventh record consumer, bwams_collate_t, on one device, joins mates while the file streams
 * through (csrc/collate.hip): each add gives back the pairs it completed and its single reads, and keeps only the records that still
 * wait for their mate in device memory.  In a coordinate-sorted file most mates lie a few hundred bases apart, so that set stays
 * small.  bwams/collate.py restates the rules with a dict.
 * "Add order" and a record's 64-bit ORDINAL are as for bwams_dupjoin_t: the order of the _add_* calls, then record order within each;
 * every added record has an ordinal, skipped ones included.  There is no 2^32 limit on ordinals.
 *  C1. Kept records.  Records with FLAG 0x100 or 0x800 are skipped and counted; they never enter the pool.  This is rule 2 of
 *      bwams_bam_reads_decode: they would not become reads anyway.
 *  C2. Segment.  A kept record with 0x1 clear is SINGLE.  With 0x1 set it is FIRST when 0x40 is set and 0x80 clear, LAST when 0x80
 *      is set and 0x40 clear; 0x1 with both or neither of 0x40 and 0x80 is refused (C6).
 *  C3. The walk, defined sequentially; the device reproduces it exactly.  A table `pending` holds at most one record per name, a
 *      name being its bytes without the NUL, compared byte for byte.  Kept records are taken in ordinal order.  A single is emitted at
 *      once.  A paired record R whose name is not pending becomes pending.  When the name is pending with a record P of the other
 *      segment, the pair (first, last) is emitted and the name leaves the table.  When P is of the same segment the add is refused
 *      (C6).  A record whose name's pair was emitted before simply waits again and ends as an orphan: nothing remembers emitted names.
 *  C4. Output of an add: two byte strings of whole records, each record byte for byte as it came in; no bit is set or cleared.
 *      `pairs`: every pair this add completed, the first record then the last, in the order of the ordinals of the records that
 *      completed them.  `singles`: the add's singles in ordinal order.  So any prefix of `pairs` that ends on a pair boundary is
 *      input for bwams_process_chunk_bam with paired = 1, and `singles` with paired = 0.
 *  C5. Finish.  _finish sets `pairs` to empty and `singles` to the pending records in ordinal order (the orphans); the table is
 *      empty afterwards.  Then adds are refused with BWAMS_ERR_ARG and a text until _reset.  Over a whole run the outputs of all adds
 *      and of the finish hold every kept record exactly once.
 *  C6. Refusals.  BWAMS_ERR_UNSUPPORTED with the text "record K" and the reason, K being the smallest ordinal at which the sequential
 *      walk meets a fault of C2 or C3, whichever rule it is.  The handle (pending set, counters, previous output) is left exactly as
 *      before the add.  Malformed record chains are refused as the other consumers' _add_records refuse them, a file on another
 *      device as their _add_file does.
 *  C7. Keys are a device, not a rule.  The kernels group candidates by rule J1's k0; a pair is only made after the two names were
 *      compared byte by byte, length included.  A key collision, which can be constructed in untrusted input, costs time (a run of
 *      equal keys is walked in the square of its length) and never a wrong pair.  bwams_collate_opt_t.key_mask (default all ones) is
 *      ANDed onto the key before grouping: a test hook that makes the collision path reachable; mask 0 puts every record into one run.
 *  C8. Pool.  Pending records live in a device pool that grows on demand, in blocks that are never moved to grow: their bytes, and
 *      an entry of 29 bytes each (masked key, address, ordinal, size, segment).  opt.pool_bytes > 0 caps the bytes of pending
 *      records: an add after which more would wait is BWAMS_ERR_NOMEM with the size asked for in the text and leaves the handle as
 *      before the add; so does a device allocation that fails.  An add moves pool bytes only when it compacts: the records still
 *      waiting are copied into one fresh block and the old blocks are freed, which takes the live bytes once more for that moment.  It
 *      compacts when the dead bytes exceed the live bytes, or when the pool's used bytes would otherwise pass the cap.  Without a
 *      cap bytes_compacted <= bytes_pooled holds at all times: each pooled byte dies once, and a compaction moves fewer live bytes
 *      than the dead bytes it retires.  Every buffer the copies read has the 16 bytes of slack behind it that bwams_bam_sort asks for.
 * bwams_collate_open: opt may be NULL (no cap, every key bit); reserved != 0 or pool_bytes < 0 is BWAMS_ERR_ARG.  _reset returns to
 * empty and keeps the options; _close takes NULL.  _add_records: host records; _add_file: the file's current piece, where it lies;
 * *n_added the records of the add, skipped ones included; an add of no records is an add.  There is no _add_batch: a batch's records
 * are grouped already.  _finish: *n_orphans.  _out: device pointers to the output of the last add or finish, valid until the next
 * _add_*, _finish, _reset or _close; before any add the output is empty.  _fetch copies that output to the host: pairs and singles
 * (their capacities in bytes), pair_off with 2 * n_pairs + 1 record offsets and single_off with n_singles + 1; any pointer may be
 * NULL; a capacity too small for a pointer given is BWAMS_ERR_CAPACITY.  _info: a test and measurement hook (bwams_collate_info_t,
 * include/bwams_types.h).
 * Memory: the pending records' bytes, 29 bytes of entry each (twice while an add writes the next entries), the output of one add,
 * and per add 49 bytes of scratch per record of the piece and 53 per entry sorted, pending ones included (85 for the piece's own
 * paired records), kept between adds, beside rocPRIM's own.
 * Out of scope: spilling the pool to host memory; a reader thread that collates (bwams_reader_open_bam stays as it is); name-sorted
 * output (`samtools sort -n`); keeping secondary and supplementary records; a device hash table in place of
 * the sort (the follow-up if a measurement points at the sort). */
int bwams_collate_open(int device, const bwams_collate_opt_t *opt, bwams_collate_t **out);
int bwams_collate_reset(bwams_collate_t *c);
int bwams_collate_close(bwams_collate_t *c);
int bwams_collate_add_records(bwams_collate_t *c, const void *bam, int64_t n_bytes, int64_t *n_added);
int bwams_collate_add_file(bwams_collate_t *c, bwams_bam_file_t *f, int64_t *n_added);
int bwams_collate_finish(bwams_collate_t *c, int64_t *n_orphans);
int bwams_collate_out(const bwams_collate_t *c, bwams_collate_out_t *out);
int bwams_collate_fetch(bwams_collate_t *c, void *pairs, int64_t cap_pairs, int64_t *pair_off, void *singles, int64_t cap_singles,
                        int64_t *single_off);
int bwams_collate_info(const bwams_collate_t *c, bwams_collate_info_t *info);

/* ------------------------------ Viewing BAM records as SAM text ---- */

/* The way back from BAM bytes to SAM text: `samtools view` on records that lie in device memory.  An eighth record consumer,
 * bwams_samview_t, on one device (csrc/samview.hip, the inverse of csrc/bam.hip): each add of BAM records gives their SAM lines in
 * device memory, to be fetched as text, compressed where they lie, or handed on by pointer.  bwams/samview.py restates the rules.
 * The yardsticks are SAMv1 sections 1.4 and 4.2, htslib's sam_format1 rules as restated there, hand-written (record, line) pairs,
 * and the round trip through this library's own encoder; nothing here was run against htslib.
 *  V1. Output model, as bwams_collate_t's.  An add replaces the handle's output with the lines of that add's records, in record
 *      order.  Each line ends in '\n'; line_off has n_lines + 1 entries.  The output stays valid until the next _add_* or _close;
 *      before any add it is empty.  An add of no records is an add.  All offsets are 64-bit.
 *  V2. Filter (`samtools view -f / -F / -q`).  A record gives a line iff (FLAG & flag_require) == flag_require, (FLAG &
 *      flag_exclude) == 0 and MAPQ >= min_mapq.  Other records are counted as filtered and give no bytes.  *n_lines counts the lines.
 *  V3. The eleven fields, tab separated.  QNAME: the l_read_name - 1 bytes as they are.  FLAG in decimal.  RNAME: the reference's
 *      name, or `*` for refID -1.  POS + 1.  MAPQ.  CIGAR: <len><op> over MIDNSHP=X, or `*` for n_cigar_op == 0.  RNEXT: `*` for next
 *      refID -1, `=` when equal to refID (and not -1), else the name.  PNEXT + 1.  TLEN, signed.  SEQ through =ACMGRSVTWYHKDBN, high
 *      nibble first, or `*` for l_seq == 0.  QUAL + 33, or `*` when l_seq == 0 or the first quality byte is 0xFF.
 *  V4. Aux fields, in record order, each behind a tab.  A gives TG:A:c.  c C s S i I all give TG:i:<decimal>.  Z and H give TG:Z: /
 *      TG:H: and the bytes up to the NUL.  f gives TG:f: and rule V5.  B gives TG:B:<subtype>, then ,<value> per element, formatted by
 *      the subtype's own rule; a count of 0 gives TG:B:c and nothing more.
 *  V5. Floats.  The text is what C's "%g" gives for the value widened to double: six significant digits, round-half-even on the exact
 *      value; trailing zeros and a bare point removed; scientific form d.ddddde±XX (at least two exponent digits) when the decimal
 *      exponent is below -4 or at least 6; inf, -inf, nan, -nan (the sign bit, as glibc prints it), 0 and -0.  No floating-point
 *      arithmetic computes it: csrc/fmt_g.h does it in integer arithmetic on the float's mantissa and exponent, for the kernels and
 *      for bwams_fmt_float alike.  At most 13 bytes come out.
 *  V6. Refusals.  The counting pass decides before a byte of output is written: BWAMS_ERR_UNSUPPORTED with "record K" and the reason,
 *      K being the smallest 0-based ordinal within the add at which any of these holds:
 *        1. refID or next refID outside [-1, n_ref);
 *        2. l_read_name == 0, the name's last byte not NUL, or a NUL inside it;
 *        3. a CIGAR op code above 8;
 *        4. l_seq < 0, or name + CIGAR + SEQ + QUAL pass the record's end;
 *        5. the aux fields do not chain to the record's end, exactly as the other consumers decide it (a type that is none of
 *           A c C s S i I f Z H B, a B subtype that is none of c C s S i I f, a field past the end, a Z or H without its NUL): so
 *           type `d` is refused here as everywhere else.
 *      When several hold at record K the reason given is the first in the order 1, 4, 2, 3, 5: what 4 refuses cannot be read for
 *      the others.  Filtered records are checked too.  A refused add leaves the handle's previous output and counters exactly as
 *      they were.  Malformed record chains, a missing batch product, and a batch or file on another device are refused as the
 *      other consumers refuse them (BWAMS_ERR_ARG).
 *  V7. Nothing is interpreted.  Tabs or newlines inside a name or a Z value come out as they are; a CG:B:I long-CIGAR tag is
 *      printed as a tag; the bin is ignored.
 *  V8. Memory, all kept between adds and grown on demand: the output text, line_off, 32 bytes per record of an add (its size and
 *      its place, as bytes and lines), rocPRIM's scan scratch, the reference names.  A failed allocation is BWAMS_ERR_NOMEM with
 *      the size asked for and leaves the handle as before.
 * bwams_samview_open: bam_header is a BAM header block (bwams_bam_header builds one, bwams_bam_file_header_block and
 * bwams_sorter_open hand one over); the reference names and n_ref come from it and go to the device once.  A block that is cut off
 * or has the wrong magic is BWAMS_ERR_ARG.  opt may be NULL (keep everything); reserved != 0 is BWAMS_ERR_ARG.  _close takes NULL.
 * _add_records: host records; _add_batch: the batch's current BAM records; _add_file: the file's current piece; all where they
 * lie.  _out: device pointers, rule V1.  _fetch copies text (cap bytes; too small is BWAMS_ERR_CAPACITY) and the n_lines + 1
 * offsets to the host; either pointer may be NULL.  _fetch_bgzf is bwams_sam_fetch_bgzf for this text: the deflater reads the
 * device text, same `flags`.  _info: a test and measurement hook.  bwams_fmt_float: rule V5 on the host, no device needed; out gets
 * *n bytes and a NUL behind them.
 * Out of scope: type `d`; expanding a CG tag into the CIGAR; region text parsing in C (regions stay bwams_pileup_region_t);
 * `--rf` / `-G` / subsampling; a writer thread; CRAM; load balance for very long reads (one lane group owns a whole record). */
int bwams_samview_open(int device, const void *bam_header, int64_t n_header, const bwams_samview_opt_t *opt, bwams_samview_t **out);
int bwams_samview_close(bwams_samview_t *v);
int bwams_samview_add_records(bwams_samview_t *v, const void *bam, int64_t n_bytes, int64_t *n_lines);
int bwams_samview_add_batch(bwams_samview_t *v, bwams_batch_t *b, int64_t *n_lines);
int bwams_samview_add_file(bwams_samview_t *v, bwams_bam_file_t *f, int64_t *n_lines);
int bwams_samview_out(const bwams_samview_t *v, bwams_samview_out_t *out);
int bwams_samview_fetch(bwams_samview_t *v, char *text, int64_t cap, int64_t *line_off);
int bwams_samview_fetch_bgzf(bwams_samview_t *v, bwams_deflater_t *d, void *out, int64_t cap, int32_t flags, int64_t *n_out);
int bwams_samview_info(const bwams_samview_t *v, bwams_samview_info_t *info);
int bwams_fmt_float(float x, char out[16], int32_t *n);

/* Page-locked host memory (hipHostMalloc) for the buffers that cross PCIe every chunk: reads, names and qualities up, SAM text down. */
int bwams_host_alloc(size_t bytes, void **out);
int bwams_host_free(void *p);

#ifdef __cplusplus
}
#endif
#endif /* BWAMS_H */
