/*
 * bwams_types.h — plain-old-data records that cross the C-ABI boundary.
 *
 * Every record is byte-for-byte the layout the reference keeps in host memory,
 * so a reference-side caller can hand its own arrays to the library without a
 * conversion pass.  Reference definitions (file:line under /root/reference):
 *   CP_OCC     src/FMI_search.h:64-68     (64 B checkpoint block, 64 BWT rows)
 *   SMEM       src/FMI_search.h:85-93     (40 B without DEBUG)
 *   SeqPair    src/bandedSWA.h:90-99      (56 B)
 *   mem_opt_t  src/bwamem.h:89-124        (only the fields the hot path reads)
 */
#ifndef BWAMS_TYPES_H
#define BWAMS_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One checkpoint of the FM-index: occurrence counts of A,C,G,T in BWT[0, 64*blk)
 * followed by four one-hot bit strings; bit (63-j) of one_hot_bwt_str[c] is set
 * iff BWT[64*blk + j] == c.  The sentinel row and the padding rows set no bit. */
typedef struct bwams_cp_occ {
    int64_t  cp_count[4];
    uint64_t one_hot_bwt_str[4];
} bwams_cp_occ_t;

/* Bi-directional interval of the query span [m, n] (inclusive):
 * k = first BWT row of the forward pattern, l = first row of its reverse
 * complement, s = interval size. */
typedef struct bwams_smem {
    uint32_t rid;
    uint32_t m, n;
    uint32_t pad_;      /* the reference struct has 4 B of alignment padding here */
    int64_t  k, l, s;
} bwams_smem_t;

/* One extension task.  idr/idq are byte offsets into the flat reference/query
 * buffers (one base code 0..4 per byte); len1 = target length, len2 = query
 * length, h0 = initial score.  The last six fields are outputs. */
typedef struct bwams_seqpair {
    int32_t idr, idq, id;
    int32_t len1, len2;
    int32_t h0;
    int32_t seqid, regid;
    int32_t score, tle, gtle, qle;
    int32_t gscore, max_off;
} bwams_seqpair_t;

/* Seeding options: the subset of mem_opt_t read by mem_collect_smem
 * (src/bwamem.cpp:648-786) and mem_chain_seeds' SA step (src/bwamem.cpp:861-873).
 * Defaults: src/bwamem.cpp:135-171. */
typedef struct bwams_seed_opt {
    int32_t min_seed_len;   /* -k, default 19 */
    float   split_factor;   /* -r, default 1.5 */
    int32_t split_width;    /* default 10 */
    int32_t max_mem_intv;   /* default 20; 0 disables round 3 */
    int32_t max_occ;        /* -c, default 500 */
} bwams_seed_opt_t;

/* Extension options: the BandedPairWiseSW constructor arguments
 * (src/bandedSWA.cpp:48-52).  mat is the 5x5 substitution matrix filled by
 * bwa_fill_scmat (src/bwa.cpp) from a (match) and b (mismatch). */
typedef struct bwams_sw_opt {
    int32_t o_del, e_del, o_ins, e_ins;
    int32_t zdrop;
    int32_t end_bonus;
    int8_t  mat[25];
    int8_t  pad_[3];
} bwams_sw_opt_t;

/* EMF seed table entry and probe result: the reference's seed_entry_t (src/perfect.h:93-108)
 * and bseq1_perfect_t (src/perfect.h:153-160: flags bit0 valid, bit1 reverse-complement match,
 * bits 2.. index of the multi-location list). */
typedef struct bwams_seed_entry {
    uint32_t flags, location, left, right;
} bwams_seed_entry_t;
typedef struct bwams_perfect {
    uint32_t flags, location;
} bwams_perfect_t;

/* Result of the local Smith-Waterman of mate rescue: the reference's kswr_t
 * (src/ksw.h:43-48).  Unset values are -1. */
typedef struct bwams_kswr {
    int32_t score;          /* best score */
    int32_t te, qe;         /* target / query end (inclusive) */
    int32_t score2, te2;    /* second best score and its target end */
    int32_t tb, qb;         /* target / query start */
} bwams_kswr_t;

/* ---- chaining and chain-to-alignment (mem_chain_seeds .. mem_chain2aln_across_reads_V2) ---- */

/* One reference sequence: the fields of bntann1_t (src/bntseq.h) the hot path reads. */
typedef struct bwams_contig {
    int64_t offset;         /* start on the forward strand */
    int32_t len;
    int32_t is_alt;
} bwams_contig_t;

/* The subset of mem_opt_t (src/bwamem.h:89-124) read by chaining, chain filtering, task
 * construction and the post-extension bookkeeping.  Defaults: src/bwamem.cpp:135-171. */
typedef struct bwams_mem_opt {
    int32_t a;                          /* match score, default 1 */
    int32_t o_del, e_del, o_ins, e_ins; /* 6, 1, 6, 1 */
    int32_t pen_clip5, pen_clip3;       /* 5, 5 */
    int32_t w;                          /* band width, 100 */
    int32_t zdrop;                      /* 100 */
    int32_t min_seed_len;               /* 19 */
    int32_t min_chain_weight;           /* 0 */
    int32_t max_chain_extend;           /* 1<<30 */
    int32_t max_occ;                    /* 500 */
    int32_t max_chain_gap;              /* 10000 */
    float   mask_level;                 /* 0.50 */
    float   drop_ratio;                 /* 0.50 */
    int8_t  mat[25];
    int8_t  pad_[3];
    /* Not a mem_opt_t field.  0 (default): a seed that an earlier kept region already explains is
     * purged WITHOUT being extended — the reference extends it first and discards the result
     * (mem_kernel2_core drops purged regions, src/bwamem.cpp:1446-1456), so every kept region and
     * every purge decision is unchanged; only the contents of purged regions differ.
     * 1: extend every seed, purged regions hold the reference's dead values too. */
    int32_t extend_all;
    float   mask_level_redun;           /* mem_opt_t again: 0.95, read by mem_sort_dedup_patch */
    int32_t max_ins;                    /* 10000, read by mem_pestat */
    int32_t b;                          /* mismatch penalty, 4: mem_mark_primary_se and mem_pair read a + b */
    int32_t pen_unpaired;               /* 17: anchors of mate rescue score >= best - pen_unpaired */
    int32_t max_matesw;                 /* 50: anchors per end that mate rescue tries */
    int32_t mapq_coef_len;              /* mapQ_coef_len, 50 (mapQ_coef_fac = log(mapQ_coef_len)): read by mem_approx_mapq_se */
} bwams_mem_opt_t;

/* mem_pestat_t (src/bwamem.h:178-182), same layout. */
typedef struct bwams_pestat {
    int32_t low, high;      /* bounds within which a pair counts as properly paired */
    int32_t failed;         /* non-zero: orientation not supported by enough data */
    int32_t pad_;
    double  avg, std;
} bwams_pestat_t;

/* The pairing decision for one read pair: what mem_sam_pe_batch_post (src/bwamem_pair.cpp:981-1098) has in hand
 * after mate rescue, mem_mark_primary_se of both ends and mem_pair (:366-427).  z[] / sub / n_sub are those of
 * mem_pair and are meaningful only when score > 0 (otherwise the reference leaves them unset; here 0 / -1). */
typedef struct bwams_pair {
    int32_t score;          /* mem_pair's return value o; 0: no proper pair (or an end without a primary hit) */
    int32_t sub, n_sub;     /* second best pairing score, pairings within max(a+b, o_del+e_del, o_ins+e_ins) of it */
    int32_t z[2];           /* index of the paired region in each end's list, -1 when unset */
    int32_t n_pri[2];       /* mem_mark_primary_se's return value of each end (regions on the primary assembly) */
    int32_t n_matesw;       /* mem_matesw's return values summed: rescue alignments this pair consumed */
} bwams_pair_t;

/* mem_t (src/ertseeding.h:62-78), 56 B, same field offsets: one maximal exact match found by the reference's ERT walk
 * and the slice [hitbeg, hitbeg + hitcount) of the read's hit array that belongs to it. */
typedef struct bwams_ert_mem {
    uint8_t forward;        /* found by forward search (hits are reference coordinates as they are) */
    uint8_t pad_[3];
    int32_t start, end;     /* [start, end) in the read */
    int32_t rc_start, rc_end;
    int32_t skip_ref_fetch;
    int32_t fetch_leaves;   /* hits were gathered from the leaves: coordinates as they are, like forward */
    int32_t hitbeg, hitcount;
    int32_t end_correction; /* backward search: bases by which the match ran past its start position */
    int32_t is_multi_hit;
    int32_t c_pivot, p_pivot, pp_pivot;     /* pivot_t */
} bwams_ert_mem_t;

/* mem_seed_t (src/bwamem.h:129-140), 32 B, same field offsets. */
typedef struct bwams_chain_seed {
    int64_t rbeg;
    int32_t qbeg, len, score;
    int8_t  done;
    int8_t  pad0_[3];
    int32_t aln;            /* index of this seed's region within its read's region list */
    int32_t pad1_;
} bwams_chain_seed_t;

/* mem_chain_t (src/bwamem.h:142-149), 48 B, same field offsets; the seeds pointer is replaced
 * by the index of the chain's first seed in the flat seed array (seeds of a chain are contiguous,
 * in the order mem_chain_seeds appended them). */
typedef struct bwams_chain {
    int32_t  seqid, cseed;
    int32_t  n, m, first, rid;
    uint32_t w_kept_alt;    /* w: bits 0-28, kept: bits 29-30, is_alt: bit 31 */
    float    frac_rep;
    int64_t  pos;
    int64_t  seed_off;
} bwams_chain_t;
#define BWAMS_CHAIN_W(c)      ((c).w_kept_alt & 0x1fffffffu)
#define BWAMS_CHAIN_KEPT(c)   (((c).w_kept_alt >> 29) & 3u)
#define BWAMS_CHAIN_IS_ALT(c) ((c).w_kept_alt >> 31)

/* mem_alnreg_t (src/bwamem.h:153-174), 112 B, same field offsets; the chain pointer is replaced
 * by the index of the chain in the flat chain array.  Fields the extension stage does not set
 * are zero, as after the reference's memset. */
typedef struct bwams_alnreg {
    int64_t  rb, re;
    int32_t  qb, qe;
    int32_t  rid;
    int32_t  pad0_;
    int64_t  chain;
    int32_t  score, truesc, sub, alt_sc, csub, sub_n;
    int32_t  w, seedcov, secondary, secondary_all, seedlen0;
    int32_t  n_comp_is_alt;
    float    frac_rep;
    int32_t  pad1_;
    uint64_t hash;
    int32_t  flg;
    int32_t  pad2_;
} bwams_alnreg_t;

/* mem_aln_t (src/bwamem.h:184-194) as mem_reg2aln fills it, with the bit fields widened and the CIGAR / MD pointer replaced
 * by offsets into the flat CIGAR (uint32 opLen << 4 | op, op: MIDSH = 01234) and MD (NUL-terminated strings) pools. */
typedef struct bwams_aln {
    int64_t  pos;            /* forward-strand 5'-end position within the sequence */
    int32_t  rid;            /* sequence index; < 0 for the unmapped record */
    int32_t  flag;           /* 0x4 unmapped, 0x100 secondary */
    int32_t  is_rev, is_alt, mapq, NM;
    int32_t  n_cigar, md_len;        /* md_len counts the terminating NUL */
    int64_t  cigar_off, md_off;
    int32_t  score, sub, alt_sc;
    int32_t  pad_;
} bwams_aln_t;

/* What mem_reg2sam / mem_gen_alt / mem_aln2sam read beyond bwams_mem_opt_t: fields of mem_opt_t (src/bwamem.h:89-124,
 * defaults src/bwamem.cpp:135-171) and the read-group id (bwa_rg_id, src/bwa.cpp). */
#define BWAMS_MEM_F_NOPAIRING      0x4      /* bwams_pair_run_sam, mem_sam_pe's proper-pair flag of unpaired ends */
#define BWAMS_MEM_F_ALL            0x8
#define BWAMS_MEM_F_NO_MULTI       0x10
#define BWAMS_MEM_F_NO_RESCUE      0x20     /* bwams_pair_run_sam */
#define BWAMS_MEM_F_REF_HDR        0x100    /* XR:Z:<annotation> on every record (bwams_index_set_contig_annos first) */
#define BWAMS_MEM_F_SOFTCLIP       0x200
#define BWAMS_MEM_F_PRIMARY5       0x800    /* bwams_pair_run_sam (the text itself does not read it) */
#define BWAMS_MEM_F_KEEP_SUPP_MAPQ 0x1000
typedef struct bwams_sam_opt {
    int32_t T;                  /* minimum score to output, 30 */
    int32_t flag;               /* BWAMS_MEM_F_* (the reference's MEM_F_* values) */
    float   XA_drop_ratio;      /* 0.80 */
    int32_t max_XA_hits;        /* 5 */
    int32_t max_XA_hits_alt;    /* 200 */
    char    rg_id[256];         /* "" = no RG:Z tag */
} bwams_sam_opt_t;

/* One BAM record's place in coordinate order (samtools sort's default): key = (uint64)(uint32)refID << 32 |
 * (uint64)(uint32)(pos + 1) << 1 | (FLAG & 0x10 ? 1 : 0) — refID -1 (unplaced) last, then POS, then the reverse-strand bit; records
 * of equal key keep their input order.  end = pos + the CIGAR's reference length (M/D/N/=/X), or pos + 1 when the record is
 * unmapped, has no CIGAR or a reference length of 0 (the end reg2bin takes); size = block_size + 4. */
typedef struct bwams_bam_coord {
    uint64_t key;
    int32_t  end;
    int32_t  size;
} bwams_bam_coord_t;

/* What bwams_sorter_close did: runs put, records merged, runs (and their bytes: records + coords) spilled to temporary files,
 * the output's bytes, and host-clock milliseconds of the k-way merge, the deflate calls and the file writes. */
typedef struct bwams_sorter_stats {
    int64_t runs, records, spilled_runs, spilled_bytes, out_bytes;
    float   ms_merge, ms_deflate, ms_write;
} bwams_sorter_stats_t;

/* One template's duplicate-marking end (include/bwams.h, "Duplicate marking"): tmpl is the template's ordinal in input order;
 * (ref1, pos1) is end 1's refID and unclipped 5' coordinate (0-based), (ref2, pos2) end 2's, ref2 = -1 for a fragment (pos2 = 0);
 * score is the template's score (a pair's: both ends' summed); strands: bit 0 end 1 reverse, bit 1 end 2 reverse. */
typedef struct bwams_dup_end {
    int64_t tmpl;
    int32_t ref1, pos1, ref2, pos2;
    int32_t score, strands;
} bwams_dup_end_t;

/* What duplicate marking found (rule 8): templates; fragments examined and marked; pairs (not reads) examined and marked; records
 * that end up with FLAG 0x400; host-clock milliseconds around the decision. */
typedef struct bwams_dup_stats {
    int64_t templates, unpaired_examined, unpaired_duplicates, pairs_examined, pair_duplicates, records_marked;
    float   ms_decide;
    int32_t pad_;
} bwams_dup_stats_t;

/* Options of the decision (rule 12): optical_distance is d, 0 for no optical duplicate detection (Picard: 100, 2500 for patterned
 * flow cells); max_optical_set is the largest group examined, 0 for Picard's 300000. */
typedef struct bwams_dup_opt {
    int32_t optical_distance;
    int32_t pad_;
    int64_t max_optical_set;
} bwams_dup_opt_t;

/* One end's library, read group and flow-cell location (rules 9-10), parallel to bwams_dup_end_t: lib in [0, n_lib), rg the read
 * group's ordinal or -1; has is 1 when the read name gives a location (tile, x, y) and 0 otherwise, and then tile, x and y are 0. */
typedef struct bwams_dup_loc {
    int32_t lib, rg, tile, x, y, has;
} bwams_dup_loc_t;

/* One library's row of the metrics (rule 13).  estimated_library_size is -1 when rule 14 gives none. */
typedef struct bwams_dup_lib_stats {
    int64_t unpaired_examined, pairs_examined, secondary_or_supplementary, unmapped, unpaired_duplicates, pair_duplicates,
            pair_optical_duplicates, estimated_library_size;
    double  percent_duplication;
} bwams_dup_lib_stats_t;

/* The read groups and libraries of a SAM header (rule 9): a host object. */
typedef struct bwams_dup_groups bwams_dup_groups_t;

/* Depth of coverage (include/bwams.h, "Depth of coverage").  A depth handle lives on one device. */
typedef struct bwams_depth bwams_depth_t;

/* Rule 2's filter and rule 3's choice: records with any bit of exclude set in FLAG, or MAPQ below min_mapq, do not count;
 * count_deletions != 0 makes D cover.  reserved must be 0.  A NULL pointer means {0x704, 0, 0, 0}. */
typedef struct bwams_depth_opt {
    uint32_t exclude;
    int32_t  min_mapq;
    int32_t  count_deletions;
    int32_t  reserved;
} bwams_depth_opt_t;

/* One reference's row of the summary (rule 7): its length, the sum of its depths, and the smallest and largest depth. */
typedef struct bwams_depth_ref {
    int64_t length, bases;
    int32_t min, max;
} bwams_depth_ref_t;

/* Pileup (include/bwams.h, "Pileup").  A pileup handle lives on one device. */
typedef struct bwams_pileup bwams_pileup_t;

/* Rule 1: positions [beg, end) of reference `ref`. */
typedef struct bwams_pileup_region {
    int32_t ref, beg, end;
} bwams_pileup_region_t;

/* Rule 2's filter, rule 4's base quality and rule 8's thresholds.  reserved must be 0.  A NULL pointer means
 * {0x704, 0, 13, 2, 200, 0}. */
typedef struct bwams_pileup_opt {
    uint32_t exclude;
    int32_t  min_mapq;
    int32_t  min_baseq;          /* 0..255 */
    int32_t  min_alt;            /* >= 1 */
    int32_t  min_permille;       /* 0..1000 */
    int32_t  reserved;
} bwams_pileup_opt_t;

/* The channels of a slot (rule 1), as indices into its 12 counters. */
#define BWAMS_PILEUP_CHANNELS 12
#define BWAMS_PILEUP_N   8
#define BWAMS_PILEUP_DEL 9
#define BWAMS_PILEUP_INS 10

/* One candidate site (rule 8): the region's index in the handle's list, the position on the region's reference, the reference
 * base (0..3), the candidate alleles (bits 0-3: A C G T, bit 4: DEL, bit 5: INS), rule 8's depth and the slot's counters. */
typedef struct bwams_pileup_site {
    int32_t  region, pos, ref;
    uint32_t kinds, depth;
    uint32_t c[BWAMS_PILEUP_CHANNELS];
} bwams_pileup_site_t;

/* Rules 10 and 13: the thresholds of a call and the quality of a record without qualities.  reserved must be 0.  A NULL pointer
 * means {20, 1, 30, 0}. */
typedef struct bwams_pileup_gl_opt {
    int32_t min_qual;            /* >= 0 */
    int32_t min_depth;           /* >= 1 */
    int32_t no_qual_q;           /* 0..93 */
    int32_t reserved;
} bwams_pileup_gl_opt_t;

/* The sums of a slot's quality plane (rule 11), as indices into its 12 values: Q, HOM and HET of base b at these + b. */
#define BWAMS_PILEUP_Q   0
#define BWAMS_PILEUP_HOM 4
#define BWAMS_PILEUP_HET 8

/* One SNV call (rule 13): the region's index in the handle's list, the position on the region's reference, the reference base
 * (0..3), the genotype's alleles a1 <= a2 (0..3), QUAL, GQ, the base depth, n[b] of the four bases and the ten pl in VCF order. */
typedef struct bwams_pileup_call {
    int32_t  region, pos, ref, a1, a2, qual, gq;
    uint32_t depth;
    uint32_t n[4];
    int32_t  pl[10];
} bwams_pileup_call_t;

/* bwams_pileup_info: the tile of the tiled path in positions, the handle's slots, and of the last add the records rule 2 let
 * through, the (tile, record) entries of the tiled path and the records that went to the direct kernel.  ms_check and ms_add are
 * for measurement only (tools/pileup_rate.py), nothing a caller should build on: the device time between events around rule 3's
 * check and around everything from the routing to the last counter update. */
typedef struct bwams_pileup_info {
    int32_t tile, n_regions;
    int64_t n_slots, n_counted, n_entries, n_direct;
    float   ms_check, ms_add;
} bwams_pileup_info_t;

/* Rules 14 and 16: the thresholds of an indel call, the cap on an event's quality and the longest allele kept apart.  reserved must
 * be 0.  A NULL pointer means {20, 1, 40, 32, 0}. */
typedef struct bwams_pileup_indel_opt {
    int32_t min_qual;            /* >= 0 */
    int32_t min_depth;           /* >= 1 */
    int32_t indel_q;             /* 0..93 */
    int32_t max_len;             /* 1..32 */
    int32_t reserved;
} bwams_pileup_indel_opt_t;

/* The type of an event (rule 14) and the four span sums of a slot (rule 15), as indices into its four values. */
#define BWAMS_PILEUP_EV_DEL   0
#define BWAMS_PILEUP_EV_INS   1
#define BWAMS_PILEUP_EV_OTHER 2
#define BWAMS_PILEUP_SPAN_N   0
#define BWAMS_PILEUP_SPAN_Q   1
#define BWAMS_PILEUP_SPAN_HOM 2
#define BWAMS_PILEUP_SPAN_HET 3
#define BWAMS_PILEUP_INDEL_MAX 32

/* One indel call (rule 17): the region's index in the handle's list, the anchor's position on the region's reference, the anchor's
 * reference base (0..3), the ALT allele (type 0 or 1, len, seq as rule 14 packs it; 0 for a deletion), gt (1 het, 2 hom-alt), QUAL,
 * GQ, rule 16's depth, the spanning reads, the ALT's events and the other events, pl of RR RA AA, and for a deletion the reference
 * codes 0..4 of the len deleted positions (0 elsewhere).  reserved is 0. */
typedef struct bwams_pileup_indel {
    int32_t  region, pos, ref, type, len, reserved;
    uint64_t seq;
    int32_t  gt, qual, gq;
    uint32_t depth, n_ref, n_alt, n_other;
    int32_t  pl[3];
    uint8_t  del_ref[BWAMS_PILEUP_INDEL_MAX];
} bwams_pileup_indel_t;

/* One allele group of a slot (rule 16): the anchor, (type, len, seq), the events n and the sums of qe, T_HOM[qe] and T_HET[qe]. */
typedef struct bwams_pileup_indel_allele {
    int32_t  region, pos, type, len;
    uint64_t seq;
    uint64_t n, q, hom, het;
} bwams_pileup_indel_allele_t;

/* bwams_pileup_indel_info: the events held and the capacity of their buffer in events, and of the last add the events appended and
 * the device time of the indel kernels (the count pass and the event pass); for tests and measurement only, as bwams_pileup_info. */
typedef struct bwams_pileup_indel_info {
    int64_t n_events, cap_events, n_appended;
    float   ms_indel;
    int32_t reserved;
} bwams_pileup_indel_info_t;

/* Alignment QC (include/bwams.h, "Alignment QC").  A QC handle lives on one device. */
typedef struct bwams_qc bwams_qc_t;

/* Rule 3's filter and the sizes of rule 4's tables: max_cycle a multiple of 64 in [64, 4096], max_isize in [1, 2^20].  reserved must
 * be 0.  A NULL pointer means {0x900, 512, 8000, 0}. */
typedef struct bwams_qc_opt {
    uint32_t exclude;
    int32_t  max_cycle;
    int32_t  max_isize;
    int32_t  reserved;
} bwams_qc_opt_t;

/* Rule 2's counters as indices into flags[class], rule 5's as indices into scalars. */
#define BWAMS_QC_FLAG_TOTAL 0
#define BWAMS_QC_FLAG_PRIMARY 1
#define BWAMS_QC_FLAG_SECONDARY 2
#define BWAMS_QC_FLAG_SUPPLEMENTARY 3
#define BWAMS_QC_FLAG_DUPLICATES 4
#define BWAMS_QC_FLAG_PRIMARY_DUPLICATES 5
#define BWAMS_QC_FLAG_MAPPED 6
#define BWAMS_QC_FLAG_PRIMARY_MAPPED 7
#define BWAMS_QC_FLAG_PAIRED 8
#define BWAMS_QC_FLAG_READ1 9
#define BWAMS_QC_FLAG_READ2 10
#define BWAMS_QC_FLAG_PROPERLY_PAIRED 11
#define BWAMS_QC_FLAG_BOTH_MAPPED 12
#define BWAMS_QC_FLAG_SINGLETONS 13
#define BWAMS_QC_FLAG_MATE_OTHER_REF 14
#define BWAMS_QC_FLAG_MATE_OTHER_REF_MAPQ5 15
#define BWAMS_QC_READS 0
#define BWAMS_QC_BASES 1
#define BWAMS_QC_MAPPED 2
#define BWAMS_QC_BASES_MAPPED 3
#define BWAMS_QC_CLIPPED 4
#define BWAMS_QC_NM_SUM 5
#define BWAMS_QC_NM_MISSING 6
#define BWAMS_QC_QUAL_SUM 7
#define BWAMS_QC_QUAL_BASES 8
#define BWAMS_QC_BASES_OVER 9
#define BWAMS_QC_NO_QUAL 10

/* flags[0]: records without FLAG 0x200, flags[1]: with it (rule 2); scalars: rule 5, entries 11..15 stay 0. */
typedef struct bwams_qc_summary {
    int64_t flags[2][16];
    int64_t scalars[16];
} bwams_qc_summary_t;

/* bwams_qc_info: the ISIZE bins of a row that the record kernel counts in LDS, the records of a slice of the cycle kernel, and of the
 * last add the records given, the records rule 3's filter let through and the bases past max_cycle.  ms_check and ms_add are for
 * measurement only (tools/qc_rate.py): the device time between events around rule 1's check and around the kernels that count. */
typedef struct bwams_qc_info {
    int32_t isize_lds, slice;
    int64_t n_records, n_counted, bases_over;
    float   ms_check, ms_add;
} bwams_qc_info_t;

/* Base recalibration tables (include/bwams.h, "Base recalibration tables").  A handle lives on one device. */
typedef struct bwams_recal bwams_recal_t;

/* Rule 1's options: exclude within 16 bits, min_baseq in [0, 93], max_cycle >= 1, reserved 0.  A NULL pointer means
 * {0x704, 1, 6, 500, 0}. */
typedef struct bwams_recal_opt {
    uint32_t exclude;
    int32_t  min_mapq;
    int32_t  min_baseq;
    int32_t  max_cycle;
    int32_t  reserved;
} bwams_recal_opt_t;

/* One interval of known variation (rule 3): positions [beg, end) of reference ref, 0-based. */
typedef struct bwams_recal_site {
    int32_t ref, beg, end;
} bwams_recal_site_t;

/* bwams_recal_info: which path the last add took (1: the LDS kernel, 0: the plain one), the records of a slice of the LDS kernel, of
 * the last add the records given, the records rule 4 let through and the bases rule 7 observed, and the bytes of the handle's
 * per-position store.  ms_check and ms_add are for measurement only (tools/recal_rate.py): the device time between events around
 * rule 5's check and around the kernels that count. */
typedef struct bwams_recal_info {
    int32_t lds, slice;
    int64_t n_records, n_counted, n_bases, store_bytes;
    float   ms_check, ms_add;
} bwams_recal_info_t;

/* The quality model and its application (include/bwams.h, "Applying base recalibration").  A model is a host object; an apply handle
 * lives on one device. */
typedef struct bwams_recal_model bwams_recal_model_t;
typedef struct bwams_recal_apply bwams_recal_apply_t;

/* The model's options: exclude within 16 bits, preserve_below in [0, 93], max_q in [1, 60], prior_obs in [1, 2^20], reserved 0.  A
 * NULL pointer means {0, 6, 60, 1024, 0}. */
typedef struct bwams_recal_model_opt {
    uint32_t exclude;
    int32_t  preserve_below;
    int32_t  max_q;
    int32_t  prior_obs;
    int32_t  reserved;
} bwams_recal_model_opt_t;

/* bwams_recal_apply_info: of the last apply the records given and the records rewritten, and the bytes of the model on the device.
 * ms_check and ms_apply are for measurement only (tools/recal_apply_rate.py): the device time between events around rule B's check
 * and around the kernels that rewrite (for a batch with a sorted copy: both rewrites). */
typedef struct bwams_recal_apply_info {
    int64_t n_records, n_rewritten, model_bytes;
    float   ms_check, ms_apply;
} bwams_recal_apply_info_t;

/* A BAM file read back by region (include/bwams.h, "BAM file by region").  A file handle lives on one device. */
typedef struct bwams_bam_file bwams_bam_file_t;

/* bwams_bam_file_info: totals since the last bwams_bam_file_query.  intervals: the plan's; members and compressed_bytes: what was
 * read of the file and inflated to inflated_bytes; candidates: offsets that passed the discovery's filter; records_seen: records of
 * the chains, records_kept: those rule 1 kept; pieces; carried: bytes moved in front of a next piece.  The times are for measurement
 * only (tools/bam_query_rate.py): ms_read and ms_inflate by the host clock around pread and bwams_inflater_run, the others device
 * time between events around the discovery, the select kernel with its scans, and the compaction with the gather. */
typedef struct bwams_bam_file_info {
    int64_t intervals, members, compressed_bytes, inflated_bytes, candidates, records_seen, records_kept, pieces, carried;
    float   ms_read, ms_inflate, ms_discover, ms_select, ms_gather;
    int32_t pad_;
} bwams_bam_file_info_t;

/* bwams_bam_file_open_merge's options (include/bwams.h, rule M1).  child_bytes: the piece size of every child, 0 = piece_bytes /
 * n_files rounded down to a multiple of 65536; reserved must be 0.  Without options: child_bytes 0. */
typedef struct bwams_bam_merge_opt {
    int64_t child_bytes;
    int32_t reserved, pad_;
} bwams_bam_merge_opt_t;

/* bwams_bam_merge_info (rule M9): n_files and child_bytes of the handle; since the last bwams_bam_file_query the rounds, the refills
 * (successful bwams_bam_file_next calls on children), the records and bytes emitted, the largest piece in records and in bytes, and
 * the most records any child's window held unemitted after a round; pg_dropped: the @PG lines rule M3 dropped at open.  The times
 * are for measurement only (tools/bam_merge_rate.py): device time between events around the check, frontier, rank, scan and gather
 * of all rounds (the host's read of the plan and the growth of the output buffers, between frontier and rank, are in none of them),
 * and ms_refill by the host clock around the children's bwams_bam_file_next calls. */
typedef struct bwams_bam_merge_info {
    int64_t n_files, child_bytes, rounds, refills, records, bytes, max_piece_records, max_piece_bytes, max_window_left;
    int32_t pg_dropped, pad_;
    float   ms_check, ms_frontier, ms_rank, ms_scan, ms_gather, ms_refill;
} bwams_bam_merge_info_t;

/* Duplicate marking with templates joined by name (include/bwams.h, above bwams_dupjoin_open).  A join handle lives on one device. */
typedef struct bwams_dupjoin bwams_dupjoin_t;

/* bwams_dupjoin_info: records added, templates and ends (after _finish), adds, applies done since _finish, the bytes of device memory
 * the handle holds now (the entries while adding; rec_tmpl, dup, optical, the ends and their locs once finished; the upload buffer of
 * the _records calls), the bytes an entry takes per record while adding (57), and the state (0 empty, 1 adding, 2 finished, 3
 * refused at _finish).  The times are for measurement only (tools/dup_join_rate.py): ms_add and ms_apply device time between events
 * around the kernels of all adds and of all applies; ms_sort, ms_ends and ms_decide the host clock around _finish's three sorts, its
 * head flags to the selects, and md_decide with the counts. */
typedef struct bwams_dupjoin_info {
    int64_t records, templates, ends, adds, applied, hbm_bytes, entry_bytes;
    int32_t state, pad_;
    float   ms_add, ms_sort, ms_ends, ms_decide, ms_apply, pad2_;
} bwams_dupjoin_info_t;

/* A coordinate-sorted BAM collated by read name (include/bwams.h, above bwams_collate_open).  A collate handle lives on one device. */
typedef struct bwams_collate bwams_collate_t;

/* bwams_collate_open's options.  pool_bytes: 0 = no cap, > 0 = the most bytes of waiting records the pool may hold (rule C8);
 * key_mask: ANDed onto a name's key before grouping (rule C7; a test hook).  Without options: no cap, all ones. */
typedef struct bwams_collate_opt {
    int64_t  pool_bytes;
    uint64_t key_mask;
    uint32_t reserved[2];
} bwams_collate_opt_t;

/* bwams_collate_out: the output of the last add or finish in device memory (rule C4), whole records back to back. */
typedef struct bwams_collate_out {
    const void *pairs;
    int64_t     pairs_bytes, n_pairs;
    const void *singles;
    int64_t     singles_bytes, n_singles;
} bwams_collate_out_t;

/* bwams_collate_info: totals since open or the last reset.  records: all added (= the next ordinal); skipped: rule C1's; pairs and
 * singles: emitted by the adds; orphans: emitted by _finish; pending and pending_bytes: the records that wait now; pool_capacity:
 * the bytes of the pool's blocks; bytes_pooled: record bytes ever put into the pool; compactions and bytes_compacted: rule C8;
 * max_run: the longest run of equal masked keys the match kernel walked; adds: successful ones; state: 0 empty, 1 adding, 2
 * finished.  The times are for measurement only (tools/collate_rate.py), device time between events over all adds: ms_entry the
 * entry kernel, its scan and the append, ms_group the sort, ms_match the match kernel, ms_place the placement with its three
 * scans, ms_copy the three copies. */
typedef struct bwams_collate_info {
    int64_t records, skipped, pairs, singles, orphans, pending, pending_bytes, pool_capacity, bytes_pooled, compactions, bytes_compacted,
            max_run, adds;
    int32_t state, pad_;
    float   ms_entry, ms_group, ms_match, ms_place, ms_copy, pad2_;
} bwams_collate_info_t;

/* BAM records viewed as SAM text (include/bwams.h, above bwams_samview_open).  A view handle lives on one device. */
typedef struct bwams_samview bwams_samview_t;

/* bwams_samview_open's options: rule V2's filter, `samtools view -f / -F / -q`.  Without options every record gives a line. */
typedef struct bwams_samview_opt {
    uint32_t flag_require, flag_exclude;
    int32_t  min_mapq;
    uint32_t reserved;
} bwams_samview_opt_t;

/* bwams_samview_out: the lines of the last add in device memory (rule V1).  line_off has n_lines + 1 entries, line k being
 * text[line_off[k], line_off[k + 1]) with its newline; n_records: the records of that add, filtered ones included.  text is NULL
 * when there are no bytes; line_off is never NULL. */
typedef struct bwams_samview_out {
    const char    *text;
    int64_t        n_bytes;
    const int64_t *line_off;
    int64_t        n_lines, n_records;
} bwams_samview_out_t;

/* bwams_samview_info: totals since open over the successful adds.  records: all added; lines: the records that gave a line;
 * filtered: those rule V2 dropped (records = lines + filtered); bytes: the text written; adds: successful ones.  The times are for
 * measurement only (tools/samview_rate.py), device time between events over all adds: ms_count the counting pass with its scan,
 * ms_write the writing pass. */
typedef struct bwams_samview_info {
    int64_t records, lines, filtered, bytes, adds;
    float   ms_count, ms_write;
} bwams_samview_info_t;

#ifdef __cplusplus
}
#endif

#endif /* BWAMS_TYPES_H */
