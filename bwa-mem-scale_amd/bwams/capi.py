"""ctypes binding of the C-ABI in include/bwams.h (libbwams.so).

Used by the tests and bench.py; a reference-side caller would bind the same
symbols from C++.  There is no fallback: if the library or a
gfx950 device is missing, calls raise BwamsError.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("BWAMS_LIB") or os.path.join(PKG, "_build", "libbwams.so")     # BWAMS_LIB: A/B runs of another build

SMEM_DTYPE = np.dtype([("rid", "<u4"), ("m", "<u4"), ("n", "<u4"), ("pad_", "<u4"),
                       ("k", "<i8"), ("l", "<i8"), ("s", "<i8")])
SEQPAIR_DTYPE = np.dtype([(n, "<i4") for n in
                          ("idr", "idq", "id", "len1", "len2", "h0", "seqid", "regid",
                           "score", "tle", "gtle", "qle", "gscore", "max_off")])

# every symbol include/bwams.h declares
SYMBOLS = [
    "bwams_strerror", "bwams_last_error", "bwams_device_count", "bwams_debug_reload",
    "bwams_index_open", "bwams_index_from_host", "bwams_index_from_device", "bwams_index_close",
    "bwams_debug_sa_dense_state", "bwams_debug_sa_dense_fetch", "bwams_debug_sa_dense_release",
    "bwams_index_bytes", "bwams_index_build", "bwams_index_fetch", "bwams_index_save", "bwams_reg2aln_run", "bwams_reg2aln_run_sam", "bwams_reg2aln_fetch",
    "bwams_index_set_contig_names", "bwams_index_set_contig_annos", "bwams_sam_upload", "bwams_sam_run", "bwams_sam_run_pe", "bwams_sam_run_emf", "bwams_sam_fetch",
    "bwams_process_chunk", "bwams_process_chunk_smart", "bwams_process_chunk2", "bwams_emf_regs_merge", "bwams_fastq_decode", "bwams_fastq_info", "bwams_fastq_has_qual", "bwams_fastq_fetch", "bwams_fastq_to_batch", "bwams_fastq_to_batch_opt", "bwams_fastq_close", "bwams_batch_create", "bwams_batch_destroy", "bwams_seed_fmi",
    "bwams_seed_upload", "bwams_seed_run", "bwams_seed_counts", "bwams_seed_fetch",
    "bwams_ert_from_host", "bwams_ert_open", "bwams_ert_close", "bwams_ert_bytes", "bwams_ert_set_fat", "bwams_seed_run_ert",
    "bwams_ert_build", "bwams_ert_info", "bwams_ert_fetch", "bwams_ert_save", "bwams_debug_sort", "bwams_debug_regs_upload", "bwams_debug_aln_lists",
    "bwams_debug_ext_regs_upload", "bwams_debug_dedup_counts", "bwams_debug_pair_regs_upload", "bwams_debug_pair_counts", "bwams_debug_chain_counts", "bwams_debug_chain_lane_counts",
    "bwams_emf_build", "bwams_emf_info", "bwams_emf_table_fetch", "bwams_emf_save",
    "bwams_bsw_extend", "bwams_bsw_upload", "bwams_bsw_run", "bwams_bsw_fetch",
    "bwams_batch_stats", "bwams_batch_sync", "bwams_ksw_align",
    "bwams_index_build_fma", "bwams_index_set_fma", "bwams_index_fetch_fma",
    "bwams_index_from_fasta", "bwams_index_from_fasta_file", "bwams_index_load_bns",
    "bwams_emf_open", "bwams_emf_from_host", "bwams_emf_close", "bwams_emf_probe",
    "bwams_emf_from_device", "bwams_emf_run", "bwams_emf_fetch",
    "bwams_index_set_contigs", "bwams_chain_run", "bwams_chain_fetch", "bwams_chain_upload",
    "bwams_extend_build", "bwams_extend_run", "bwams_extend_fetch", "bwams_extend_tasks_fetch",
    "bwams_process_reads", "bwams_process_reads_stage1", "bwams_process_reads_stage2", "bwams_host_alloc", "bwams_host_free",
    "bwams_reader_open", "bwams_reader_next", "bwams_reader_release", "bwams_reader_error", "bwams_reader_close",
    "bwams_inflater_create", "bwams_inflater_run", "bwams_inflater_destroy", "bwams_reader_open_device", "bwams_reader_info",
    "bwams_gunzip_create", "bwams_gunzip_run", "bwams_gunzip_destroy", "bwams_reader_open_device2",
    "bwams_deflate_bound", "bwams_deflater_create", "bwams_deflater_run", "bwams_deflater_destroy", "bwams_sam_fetch_bgzf",
    "bwams_writer_open_bgzf", "bwams_writer_put_bgzf",
    "bwams_bam_run", "bwams_bam_fetch", "bwams_bam_fetch_bgzf", "bwams_sam_header", "bwams_bam_header", "bwams_writer_open_bam",
    "bwams_writer_open", "bwams_writer_put", "bwams_writer_close",
    "bwams_bam_upload", "bwams_bam_sort", "bwams_bam_sorted_fetch",
    "bwams_sorter_open", "bwams_sorter_put", "bwams_sorter_put_batch", "bwams_sorter_close", "bwams_sorter_close2",
    "bwams_bam_templates", "bwams_bam_templates_fetch", "bwams_dup_decide", "bwams_bam_markdup",
    "bwams_dup_groups_create", "bwams_dup_groups_info", "bwams_dup_groups_library", "bwams_dup_groups_destroy",
    "bwams_bam_templates2", "bwams_bam_templates_fetch_loc", "bwams_bam_lib_record_counts", "bwams_dup_decide2", "bwams_bam_markdup2",
    "bwams_dup_library_size", "bwams_dup_metrics_text", "bwams_sorter_set_markdup", "bwams_sorter_close3",
    "bwams_bam_reads_decode", "bwams_bam_reads_info", "bwams_process_chunk_bam", "bwams_process_chunk_bam_smart",
    "bwams_reader_open_bam", "bwams_reader_bam_header",
    "bwams_trim_opt_default", "bwams_fastq_trim", "bwams_fastq_text", "bwams_fastq_text_fetch", "bwams_process_chunk_decoded",
    "bwams_process_reads_upload", "bwams_process_reads_stage1_run", "bwams_batch_device", "bwams_multi_upload", "bwams_multi_compute",
    "bwams_shard_bounds", "bwams_multi_create", "bwams_multi_process_reads", "bwams_multi_fetch", "bwams_multi_error", "bwams_multi_destroy",
    "bwams_depth_open", "bwams_depth_close", "bwams_depth_reset", "bwams_depth_add_batch", "bwams_depth_add_records", "bwams_depth_finish",
    "bwams_depth_summary", "bwams_depth_hist", "bwams_depth_windows", "bwams_depth_runs", "bwams_depth_fetch", "bwams_depth_text",
    "bwams_sorter_set_depth",
    "bwams_pileup_open", "bwams_pileup_close", "bwams_pileup_reset", "bwams_pileup_add_batch", "bwams_pileup_add_records", "bwams_pileup_set_ref",
    "bwams_pileup_set_ref_index", "bwams_pileup_fetch", "bwams_pileup_sites", "bwams_pileup_text", "bwams_pileup_info", "bwams_sorter_set_pileup",
    "bwams_pileup_set_quality", "bwams_pileup_fetch_quality", "bwams_pileup_calls", "bwams_pileup_vcf",
    "bwams_pileup_set_indels", "bwams_pileup_fetch_span", "bwams_pileup_indel_alleles", "bwams_pileup_indel_calls", "bwams_pileup_indel_vcf",
    "bwams_pileup_vcf_all", "bwams_pileup_indel_info", "bwams_pileup_set_indel_leftalign",
    "bwams_qc_open", "bwams_qc_close", "bwams_qc_reset", "bwams_qc_add_batch", "bwams_qc_add_records", "bwams_qc_summary", "bwams_qc_table",
    "bwams_qc_text", "bwams_qc_info", "bwams_sorter_set_qc",
    "bwams_recal_open", "bwams_recal_close", "bwams_recal_reset", "bwams_recal_add_batch", "bwams_recal_add_records", "bwams_recal_set_ref",
    "bwams_recal_set_ref_index", "bwams_recal_add_known", "bwams_recal_table", "bwams_recal_text", "bwams_recal_info",
    "bwams_sorter_set_recal", "bwams_dup_groups_rg_id",
    "bwams_recal_model_create", "bwams_recal_model_from", "bwams_recal_model_table", "bwams_recal_model_constants", "bwams_recal_model_destroy",
    "bwams_recal_apply_open", "bwams_recal_apply_close", "bwams_recal_apply_records", "bwams_recal_apply_batch", "bwams_recal_apply_info",
    "bwams_bam_file_open", "bwams_bam_file_header", "bwams_bam_file_refs", "bwams_bam_file_query", "bwams_bam_file_next", "bwams_bam_file_fetch",
    "bwams_bam_file_info", "bwams_bam_file_close", "bwams_depth_add_file", "bwams_pileup_add_file", "bwams_qc_add_file", "bwams_recal_add_file",
    "bwams_recal_apply_file", "bwams_bai_plan",
    "bwams_dupjoin_open", "bwams_dupjoin_reset", "bwams_dupjoin_close", "bwams_dupjoin_add_records", "bwams_dupjoin_add_file",
    "bwams_dupjoin_finish", "bwams_dupjoin_fetch", "bwams_dupjoin_apply_records", "bwams_dupjoin_apply_file", "bwams_dupjoin_info",
    "bwams_dupjoin_key", "bwams_bam_file_header_block",
    "bwams_bam_file_open_merge", "bwams_bam_merge_info", "bwams_bam_header_merge",
    "bwams_collate_open", "bwams_collate_reset", "bwams_collate_close", "bwams_collate_add_records", "bwams_collate_add_file",
    "bwams_collate_finish", "bwams_collate_out", "bwams_collate_fetch", "bwams_collate_info",
    "bwams_samview_open", "bwams_samview_close", "bwams_samview_add_records", "bwams_samview_add_batch", "bwams_samview_add_file",
    "bwams_samview_out", "bwams_samview_fetch", "bwams_samview_fetch_bgzf", "bwams_samview_info", "bwams_fmt_float",
    "bwams_dedup_run", "bwams_dedup_fetch", "bwams_chain_run_ert", "bwams_pestat", "bwams_pestat_keys", "bwams_pestat_from_keys", "bwams_pair_run", "bwams_pair_run_sam", "bwams_pair_fetch", "bwams_emf_regs_run", "bwams_emf_regs_fetch",
]
ERT_MEM_DTYPE = np.dtype([("forward", "u1"), ("pad_", "u1", (3,)), ("start", "<i4"), ("end", "<i4"), ("rc_start", "<i4"),
                          ("rc_end", "<i4"), ("skip_ref_fetch", "<i4"), ("fetch_leaves", "<i4"), ("hitbeg", "<i4"),
                          ("hitcount", "<i4"), ("end_correction", "<i4"), ("is_multi_hit", "<i4"), ("c_pivot", "<i4"),
                          ("p_pivot", "<i4"), ("pp_pivot", "<i4")])
assert ERT_MEM_DTYPE.itemsize == 56
PAIR_DTYPE = np.dtype([("score", "<i4"), ("sub", "<i4"), ("n_sub", "<i4"), ("z", "<i4", (2,)), ("n_pri", "<i4", (2,)),
                       ("n_matesw", "<i4")])
assert PAIR_DTYPE.itemsize == 32
PESTAT_DTYPE = np.dtype([("low", "<i4"), ("high", "<i4"), ("failed", "<i4"), ("pad_", "<i4"), ("avg", "<f8"), ("std", "<f8")])

# records of include/bwams_types.h (layouts of bntann1_t's subset, mem_seed_t, mem_chain_t, mem_alnreg_t)
CONTIG_DTYPE = np.dtype([("offset", "<i8"), ("len", "<i4"), ("is_alt", "<i4")])
CHAIN_SEED_DTYPE = np.dtype([("rbeg", "<i8"), ("qbeg", "<i4"), ("len", "<i4"), ("score", "<i4"), ("done", "i1"),
                             ("pad0_", "i1", 3), ("aln", "<i4"), ("pad1_", "<i4")])
CHAIN_DTYPE = np.dtype([("seqid", "<i4"), ("cseed", "<i4"), ("n", "<i4"), ("m", "<i4"), ("first", "<i4"), ("rid", "<i4"),
                        ("w_kept_alt", "<u4"), ("frac_rep", "<f4"), ("pos", "<i8"), ("seed_off", "<i8")])
ALNREG_DTYPE = np.dtype([("rb", "<i8"), ("re", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("rid", "<i4"), ("pad0_", "<i4"),
                         ("chain", "<i8"), ("score", "<i4"), ("truesc", "<i4"), ("sub", "<i4"), ("alt_sc", "<i4"),
                         ("csub", "<i4"), ("sub_n", "<i4"), ("w", "<i4"), ("seedcov", "<i4"), ("secondary", "<i4"),
                         ("secondary_all", "<i4"), ("seedlen0", "<i4"), ("n_comp_is_alt", "<i4"), ("frac_rep", "<f4"),
                         ("pad1_", "<i4"), ("hash", "<u8"), ("flg", "<i4"), ("pad2_", "<i4")])
ALN_DTYPE = np.dtype([("pos", "<i8"), ("rid", "<i4"), ("flag", "<i4"), ("is_rev", "<i4"), ("is_alt", "<i4"), ("mapq", "<i4"),
                      ("NM", "<i4"), ("n_cigar", "<i4"), ("md_len", "<i4"), ("cigar_off", "<i8"), ("md_off", "<i8"),
                      ("score", "<i4"), ("sub", "<i4"), ("alt_sc", "<i4"), ("pad_", "<i4")])
assert ALN_DTYPE.itemsize == 72
BAM_COORD_DTYPE = np.dtype([("key", "<u8"), ("end", "<i4"), ("size", "<i4")])      # bwams_bam_coord_t
DUP_END_DTYPE = np.dtype([("tmpl", "<i8"), ("ref1", "<i4"), ("pos1", "<i4"), ("ref2", "<i4"), ("pos2", "<i4"), ("score", "<i4"),
                          ("strands", "<i4")])                                    # bwams_dup_end_t
assert DUP_END_DTYPE.itemsize == 32
DUP_LOC_DTYPE = np.dtype([(n, "<i4") for n in ("lib", "rg", "tile", "x", "y", "has")])                      # bwams_dup_loc_t
DUP_LIB_STATS_DTYPE = np.dtype([(n, "<i8") for n in ("unpaired_examined", "pairs_examined", "secondary_or_supplementary", "unmapped",
                                                     "unpaired_duplicates", "pair_duplicates", "pair_optical_duplicates",
                                                     "estimated_library_size")] + [("percent_duplication", "<f8")])   # bwams_dup_lib_stats_t
DEPTH_REF_DTYPE = np.dtype([("length", "<i8"), ("bases", "<i8"), ("min", "<i4"), ("max", "<i4")])         # bwams_depth_ref_t
assert DEPTH_REF_DTYPE.itemsize == 24
PILEUP_REGION_DTYPE = np.dtype([("ref", "<i4"), ("beg", "<i4"), ("end", "<i4")])                          # bwams_pileup_region_t
PILEUP_SITE_DTYPE = np.dtype([("region", "<i4"), ("pos", "<i4"), ("ref", "<i4"), ("kinds", "<u4"), ("depth", "<u4"),
                              ("c", "<u4", (12,))])                                                      # bwams_pileup_site_t
PILEUP_CALL_DTYPE = np.dtype([("region", "<i4"), ("pos", "<i4"), ("ref", "<i4"), ("a1", "<i4"), ("a2", "<i4"), ("qual", "<i4"), ("gq", "<i4"),
                              ("depth", "<u4"), ("n", "<u4", (4,)), ("pl", "<i4", (10,))])               # bwams_pileup_call_t
assert PILEUP_REGION_DTYPE.itemsize == 12 and PILEUP_SITE_DTYPE.itemsize == 68 and PILEUP_CALL_DTYPE.itemsize == 88
PILEUP_INDEL_DTYPE = np.dtype([("region", "<i4"), ("pos", "<i4"), ("ref", "<i4"), ("type", "<i4"), ("len", "<i4"), ("reserved", "<i4"),
                               ("seq", "<u8"), ("gt", "<i4"), ("qual", "<i4"), ("gq", "<i4"), ("depth", "<u4"), ("n_ref", "<u4"), ("n_alt", "<u4"),
                               ("n_other", "<u4"), ("pl", "<i4", (3,)), ("del_ref", "u1", (32,))])       # bwams_pileup_indel_t
PILEUP_INDEL_ALLELE_DTYPE = np.dtype([("region", "<i4"), ("pos", "<i4"), ("type", "<i4"), ("len", "<i4"), ("seq", "<u8"), ("n", "<u8"),
                                      ("q", "<u8"), ("hom", "<u8"), ("het", "<u8")])                      # bwams_pileup_indel_allele_t
assert PILEUP_INDEL_DTYPE.itemsize == 104 and PILEUP_INDEL_ALLELE_DTYPE.itemsize == 56
assert DUP_LOC_DTYPE.itemsize == 24 and DUP_LIB_STATS_DTYPE.itemsize == 72
assert CONTIG_DTYPE.itemsize == 16 and CHAIN_SEED_DTYPE.itemsize == 32 and CHAIN_DTYPE.itemsize == 48
assert ALNREG_DTYPE.itemsize == 112


class BwamsError(RuntimeError):
    def __init__(self, code: int, where: str, detail: str = ""):
        self.code = code
        super().__init__(f"{where}: error {code} {detail}")


class SeedOpt(C.Structure):
    _fields_ = [("min_seed_len", C.c_int32), ("split_factor", C.c_float),
                ("split_width", C.c_int32), ("max_mem_intv", C.c_int32), ("max_occ", C.c_int32)]


class SwOpt(C.Structure):
    _fields_ = [("o_del", C.c_int32), ("e_del", C.c_int32), ("o_ins", C.c_int32),
                ("e_ins", C.c_int32), ("zdrop", C.c_int32), ("end_bonus", C.c_int32),
                ("mat", C.c_int8 * 25), ("pad_", C.c_int8 * 3)]


class MemOpt(C.Structure):
    """bwams_mem_opt_t: the subset of mem_opt_t read by chaining and chain-to-alignment."""
    _fields_ = [("a", C.c_int32), ("o_del", C.c_int32), ("e_del", C.c_int32), ("o_ins", C.c_int32), ("e_ins", C.c_int32),
                ("pen_clip5", C.c_int32), ("pen_clip3", C.c_int32), ("w", C.c_int32), ("zdrop", C.c_int32),
                ("min_seed_len", C.c_int32), ("min_chain_weight", C.c_int32), ("max_chain_extend", C.c_int32),
                ("max_occ", C.c_int32), ("max_chain_gap", C.c_int32), ("mask_level", C.c_float),
                ("drop_ratio", C.c_float), ("mat", C.c_int8 * 25), ("pad_", C.c_int8 * 3), ("extend_all", C.c_int32), ("mask_level_redun", C.c_float), ("max_ins", C.c_int32),
                ("b", C.c_int32), ("pen_unpaired", C.c_int32), ("max_matesw", C.c_int32), ("mapq_coef_len", C.c_int32)]


class FmiDesc(C.Structure):
    _fields_ = [("ref_seq_len", C.c_int64), ("count", C.c_int64 * 5),
                ("cp_occ", C.c_void_p), ("sa_ms_byte", C.c_void_p), ("sa_ls_word", C.c_void_p),
                ("sentinel_index", C.c_int64), ("ref_0123", C.c_void_p)]


class Fastq:
    """A decoded FASTQ buffer resident on the GPU (bwams_fastq_t)."""

    def __init__(self, text, device: int = 0, n_bytes: int | None = None):
        """text: bytes (host) or an int device address with n_bytes."""
        self.h = C.c_void_p()
        self.n_records = None
        if text is None:                              # bam_reads_decode fills the handle in
            return
        n, nb = C.c_int64(0), C.c_int64(0)
        if isinstance(text, int):
            rc = lib().bwams_fastq_decode(device, C.c_void_p(text), C.c_int64(n_bytes), C.byref(self.h), C.byref(n), C.byref(nb))
        else:
            rc = lib().bwams_fastq_decode(device, text, C.c_int64(len(text)), C.byref(self.h), C.byref(n), C.byref(nb))
        _chk(rc, "bwams_fastq_decode")
        self.n_reads, self.n_bases = n.value, nb.value

    def info(self):
        n, nb, nn, nc, ms = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_float(0)
        _chk(lib().bwams_fastq_info(self.h, C.byref(n), C.byref(nb), C.byref(nn), C.byref(nc), C.byref(ms)), "bwams_fastq_info")
        return dict(n_reads=n.value, n_bases=nb.value, name_bytes=nn.value, comment_bytes=nc.value, ms=ms.value)

    def fetch(self):
        i = self.info()
        n1 = i["n_reads"] + 1
        enc = np.zeros(max(i["n_bases"], 1), np.uint8); qual = np.zeros(max(i["n_bases"], 1), np.uint8)
        names = np.zeros(max(i["name_bytes"], 1), np.uint8); comm = np.zeros(max(i["comment_bytes"], 1), np.uint8)
        cum = np.zeros(n1, np.int64); noff = np.zeros(n1, np.int64); coff = np.zeros(n1, np.int64)
        _chk(lib().bwams_fastq_fetch(self.h, _p(enc), _p(cum), _p(names), _p(noff), _p(qual), _p(comm), _p(coff)), "bwams_fastq_fetch")
        nb_, cb_ = bytes(names[:i["name_bytes"]]), bytes(comm[:i["comment_bytes"]])
        return dict(n=i["n_reads"], enc=enc[:i["n_bases"]], cum=cum, quals=qual[:i["n_bases"]] if lib().bwams_fastq_has_qual(self.h) else None,
                    names=[nb_[noff[k]:noff[k + 1]] for k in range(i["n_reads"])],
                    comments=[cb_[coff[k]:coff[k + 1]] or None for k in range(i["n_reads"])])

    def to_batch(self, batch: "Batch"):
        """bwams_seed_upload + bwams_sam_upload of the decoded chunk, device to device."""
        _chk(lib().bwams_fastq_to_batch(self.h, batch.h), "bwams_fastq_to_batch")
        batch._nseq = self.n_reads

    def trim(self, opt: "TrimOpt | None" = None, paired: bool = False, report: bool = True):
        """bwams_fastq_trim -> (the trimmed chunk, a new Fastq; the report (TRIM_READ_DTYPE) or None; the stats as trim.stats_of's dict).
        This chunk is left as it is."""
        opt = opt if opt is not None else trim_opt()
        g = Fastq(None)
        rep = np.zeros(self.n_reads, TRIM_READ_DTYPE) if report else None
        st = TrimStats()
        _chk(lib().bwams_fastq_trim(self.h, C.byref(opt), 1 if paired else 0, C.byref(g.h), _p(rep) if report and self.n_reads else None,
                                    C.byref(st)), "bwams_fastq_trim")
        g.n_reads, g.n_bases = st.reads_out, st.bases_out
        return g, rep, st.as_dict()

    def text(self, with_comment: bool = True, fetch: bool = True):
        """bwams_fastq_text: the chunk as FASTQ (or FASTA) text -> bytes, or (device address, n_bytes) with fetch=False; the device
        text lives until the next call or close()."""
        d, n = C.c_void_p(), C.c_int64(0)
        _chk(lib().bwams_fastq_text(self.h, 1 if with_comment else 0, C.byref(d), C.byref(n)), "bwams_fastq_text")
        if not fetch:
            return d.value, n.value
        buf = np.zeros(max(n.value, 1), np.uint8)
        _chk(lib().bwams_fastq_text_fetch(self.h, _p(buf), n.value), "bwams_fastq_text_fetch")
        return bytes(buf[:n.value])

    def close(self):
        if self.h:
            lib().bwams_fastq_close(self.h)
            self.h = C.c_void_p()


TRIM_READ_DTYPE = np.dtype([("start", "<i4"), ("len", "<i4"), ("insert", "<i4"), ("reason", "u1"), ("steps", "u1"), ("pad_", "u1", (2,)),
                            ("removed", "<i4", (6,))])                                                   # bwams_trim_read_t
assert TRIM_READ_DTYPE.itemsize == 40


class TrimOpt(C.Structure):
    """bwams_trim_opt_t (trim_opt() gives the defaults)"""
    _fields_ = [(n, C.c_int32) for n in ("trim_front", "trim_tail", "cut_front", "cut_tail", "cut_window", "cut_quality", "overlap",
                                         "overlap_min", "overlap_max_diff", "overlap_diff_pct", "adapter_min_match", "adapter_mismatch_per",
                                         "max_len", "min_len", "n_limit", "qual_floor", "low_qual_pct")] + \
               [("adapter1", C.c_char * 129), ("adapter2", C.c_char * 129), ("pad_", C.c_char * 2)]


class TrimStats(C.Structure):
    """bwams_trim_stats_t"""
    _fields_ = [(n, C.c_int64) for n in ("reads_in", "bases_in", "reads_out", "bases_out", "pairs_insert", "pairs_skipped")] + \
               [("step_reads", C.c_int64 * 6), ("step_bases", C.c_int64 * 6), ("dropped", C.c_int64 * 4)]

    def as_dict(self) -> dict:
        return {n: (list(getattr(self, n)) if n in ("step_reads", "step_bases", "dropped") else getattr(self, n)) for n, _ in self._fields_}


def trim_opt(like=None, **kw) -> TrimOpt:
    """bwams_trim_opt_default, then the fields of `like` (any object with TrimOpt's fields, such as trim.Opt), then the keywords"""
    o = TrimOpt()
    _chk(lib().bwams_trim_opt_default(C.byref(o)), "bwams_trim_opt_default")
    for n, _ in TrimOpt._fields_[:-1]:
        if like is not None:
            setattr(o, n, getattr(like, n))
        if n in kw:
            setattr(o, n, kw[n])
    return o


class SamOpt(C.Structure):
    """bwams_sam_opt_t"""
    _fields_ = [("T", C.c_int32), ("flag", C.c_int32), ("XA_drop_ratio", C.c_float), ("max_XA_hits", C.c_int32),
                ("max_XA_hits_alt", C.c_int32), ("rg_id", C.c_char * 256)]


def default_sam_opt(flag: int = 0, rg_id: bytes = b"") -> SamOpt:
    """mem_opt_init defaults (src/bwamem.cpp:135-171)."""
    return SamOpt(30, flag, 0.80, 5, 200, rg_id)


class Stats(C.Structure):
    _fields_ = [("n_ext", C.c_int64), ("n_ext_blocks", C.c_int64), ("n_sa_lookups", C.c_int64),
                ("n_lf_steps", C.c_int64), ("n_smem", C.c_int64 * 3), ("bsw_cells", C.c_int64),
                ("n_ext_round", C.c_int64 * 3), ("n_blk_round", C.c_int64 * 3),
                ("ms_smem_r1", C.c_float), ("ms_smem_r2", C.c_float), ("ms_smem_r3", C.c_float),
                ("ms_sort", C.c_float), ("ms_sal", C.c_float), ("ms_seed_total", C.c_float),
                ("ms_bsw", C.c_float), ("ms_ksw", C.c_float), ("ms_tasks", C.c_float), ("ms_emf", C.c_float),
                ("emf_nodes", C.c_int64), ("emf_cmp_bytes", C.c_int64),
                ("n_chains", C.c_int64), ("n_chain_seeds", C.c_int64), ("n_left", C.c_int64), ("n_right", C.c_int64),
                ("n_retry_left", C.c_int64), ("n_retry_right", C.c_int64),
                ("ms_chain", C.c_float), ("ms_ext_plan", C.c_float), ("ms_ext_left", C.c_float),
                ("ms_ext_right", C.c_float), ("ms_ext_purge", C.c_float), ("ms_ext_total", C.c_float),
                ("n_ext_rounds", C.c_int64), ("n_final_regs", C.c_int64), ("ms_dedup", C.c_float), ("ms_pair", C.c_float),
                ("n_pair_tasks", C.c_int64), ("n_pair_redone", C.c_int64), ("n_pair_regs", C.c_int64), ("n_chain_redo", C.c_int64),
                ("ert_kmer_lookups", C.c_int64), ("ert_node_reads", C.c_int64), ("ert_ref_bytes", C.c_int64)]


class BuildStats(C.Structure):
    _fields_ = [("rows", C.c_int64), ("chunks", C.c_int32), ("rounds", C.c_int32), ("unresolved_after_first", C.c_int64),
                ("ms_first_pass", C.c_float), ("ms_outputs", C.c_float)]


class FastaStats(C.Structure):
    _fields_ = [("l_pac", C.c_int64), ("n_seqs", C.c_int32), ("n_holes", C.c_int32), ("n_ambig_bases", C.c_int64),
                ("ms_host_read", C.c_float), ("ms_upload", C.c_float), ("ms_device_pack", C.c_float), ("ms_fm_build", C.c_float),
                ("build", BuildStats)]


class InflateStats(C.Structure):
    _fields_ = [("members", C.c_int64), ("in_bytes", C.c_int64), ("out_bytes", C.c_int64),
                ("ms_upload", C.c_float), ("ms_kernel", C.c_float), ("ms_download", C.c_float)]


class GunzipStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("members", "pieces", "pieces_dropped", "recounts", "in_bytes", "out_bytes", "trailing_bytes")] + \
               [(n, C.c_float) for n in ("ms_upload", "ms_find", "ms_count", "ms_decode", "ms_window", "ms_resolve", "ms_download")]


class ReaderStats(C.Structure):
    _fields_ = [("device_inflate", C.c_int32), ("in_bytes", C.c_int64), ("out_bytes", C.c_int64),
                ("ms_read", C.c_float), ("ms_inflate", C.c_float)]


class Inflater:
    """BGZF inflated on one GPU (bwams_inflater_t)."""

    def __init__(self, device: int = 0, max_in_bytes: int = 32 << 20, max_out_bytes: int = 64 << 20):
        self.h = C.c_void_p()
        self.max_out = max_out_bytes
        _chk(lib().bwams_inflater_create(device, max_in_bytes, max_out_bytes, C.byref(self.h)), "bwams_inflater_create")

    def run_raw(self, gz, out, out_cap: int, on_device: bool):
        """bwams_inflater_run as is: gz bytes (or an address with its length as (addr, n)), out an address.  Returns
        (rc, n_consumed, n_out, InflateStats)."""
        used, n_out, st = C.c_int64(0), C.c_int64(0), InflateStats()
        ptr, n = (C.c_void_p(gz[0]), gz[1]) if isinstance(gz, tuple) else (gz, len(gz))
        rc = lib().bwams_inflater_run(self.h, ptr, n, C.c_void_p(out), out_cap, int(on_device), C.byref(used), C.byref(n_out),
                                      C.byref(st))
        return rc, used.value, n_out.value, st

    def run(self, gz: bytes, out_cap: int | None = None):
        """The whole members at the front of gz, inflated to host memory (out_cap: default max_out_bytes): (text bytes, n_consumed,
        InflateStats)."""
        cap = out_cap if out_cap is not None else self.max_out
        buf = C.create_string_buffer(max(cap, 1))
        rc, used, n, st = self.run_raw(gz, C.addressof(buf), cap, False)
        _chk(rc, "bwams_inflater_run")
        return buf.raw[:n], used, st

    def close(self):
        if self.h:
            lib().bwams_inflater_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeflateStats(C.Structure):
    _fields_ = [("members", C.c_int64), ("in_bytes", C.c_int64), ("out_bytes", C.c_int64),
                ("ms_upload", C.c_float), ("ms_kernel", C.c_float), ("ms_download", C.c_float)]


DEFLATE_EOF = 0x1                # BWAMS_DEFLATE_EOF: append the BGZF EOF member


def deflate_bound(n_bytes: int) -> int:
    """bwams_deflate_bound: the most bwams_deflater_run writes for n_bytes of input."""
    return lib().bwams_deflate_bound(n_bytes)


class Deflater:
    """BGZF written on one GPU (bwams_deflater_t)."""

    def __init__(self, device: int = 0, max_in_bytes: int = 32 << 20):
        self.h = C.c_void_p()
        self.device = device
        _chk(lib().bwams_deflater_create(device, max_in_bytes, C.byref(self.h)), "bwams_deflater_create")

    def run_raw(self, data, out, out_cap: int, in_on_device: bool = False, out_on_device: bool = False, flags: int = 0):
        """bwams_deflater_run as is: data bytes (or an address with its length as (addr, n)), out an address.  Returns
        (rc, n_out, DeflateStats)."""
        n_out, st = C.c_int64(0), DeflateStats()
        ptr, n = (C.c_void_p(data[0]), data[1]) if isinstance(data, tuple) else (data, len(data))
        rc = lib().bwams_deflater_run(self.h, ptr, n, int(in_on_device), C.c_void_p(out), out_cap, int(out_on_device), flags,
                                      C.byref(n_out), C.byref(st))
        return rc, n_out.value, st

    def run(self, data, eof: bool = False):
        """data (bytes, or (device address, n)) as BGZF members in host memory: (bytes, DeflateStats)."""
        n = data[1] if isinstance(data, tuple) else len(data)
        cap = deflate_bound(n)
        buf = C.create_string_buffer(cap)
        rc, got, st = self.run_raw(data, C.addressof(buf), cap, isinstance(data, tuple), False, DEFLATE_EOF if eof else 0)
        _chk(rc, "bwams_deflater_run")
        return buf.raw[:got], st

    def close(self):
        if self.h:
            lib().bwams_deflater_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def writer_open_bam(path: str, n_shards: int, device: int, bam_header: bytes) -> C.c_void_p:
    """bwams_writer_open_bam: a bwams_writer_t handle (bwams_writer_put_bgzf / _close as for bwams_writer_open_bgzf)."""
    w = C.c_void_p()
    _chk(lib().bwams_writer_open_bam(path.encode(), n_shards, device, bytes(bam_header), len(bam_header), C.byref(w)),
         "bwams_writer_open_bam")
    return w


SORT_BAI = 0x1                   # BWAMS_SORT_BAI: also write <path>.bai
SORT_MARKDUP = 0x2               # BWAMS_SORT_MARKDUP: mark duplicates over all puts


class DupStats(C.Structure):
    """bwams_dup_stats_t (rule 8 of duplicate marking)."""
    _fields_ = [("templates", C.c_int64), ("unpaired_examined", C.c_int64), ("unpaired_duplicates", C.c_int64),
                ("pairs_examined", C.c_int64), ("pair_duplicates", C.c_int64), ("records_marked", C.c_int64),
                ("ms_decide", C.c_float), ("pad_", C.c_int32)]

    def counts(self) -> dict:
        """the counts as a dict (without ms_decide), to compare with bwams.markdup's stats"""
        return {f: getattr(self, f) for f, _ in self._fields_ if f not in ("ms_decide", "pad_")}


def dup_decide(device: int, ends, n_templates: int):
    """Rule 6 on the device over ends (DUP_END_DTYPE) of n_templates templates (bwams_dup_decide) -> (dup: uint8 per template, DupStats)."""
    ends = np.ascontiguousarray(ends, DUP_END_DTYPE)
    dup = np.zeros(max(n_templates, 1), np.uint8)
    st = DupStats()
    _chk(lib().bwams_dup_decide(device, _p(ends), len(ends), n_templates, _p(dup), C.byref(st)), "bwams_dup_decide")
    return dup[:n_templates], st


class DupOpt(C.Structure):
    """bwams_dup_opt_t: optical_distance 0 turns optical duplicate detection off; max_optical_set 0 means 300000."""
    _fields_ = [("optical_distance", C.c_int32), ("pad_", C.c_int32), ("max_optical_set", C.c_int64)]


class DupGroups:
    """The read groups and libraries of SAM header text (bwams_dup_groups_t, rule 9 of duplicate marking)."""

    def __init__(self, header_text):
        text = header_text.encode() if isinstance(header_text, str) else bytes(header_text)
        self.h = C.c_void_p()
        _chk(lib().bwams_dup_groups_create(text, len(text), C.byref(self.h)), "bwams_dup_groups_create")
        n_rg, n_lib = C.c_int64(0), C.c_int64(0)
        _chk(lib().bwams_dup_groups_info(self.h, C.byref(n_rg), C.byref(n_lib)), "bwams_dup_groups_info")
        self.n_rg, self.n_lib = n_rg.value, n_lib.value

    def library(self, k: int):
        name = lib().bwams_dup_groups_library(self.h, k)
        return None if name is None else name.decode("latin-1")

    def rg_id(self, k: int):
        name = lib().bwams_dup_groups_rg_id(self.h, k)
        return None if name is None else name.decode("latin-1")

    @property
    def libraries(self) -> list:
        return [self.library(k) for k in range(self.n_lib)]

    def close(self):
        h, self.h = self.h, C.c_void_p()
        if h:
            lib().bwams_dup_groups_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _groups_h(groups):
    return groups.h if groups is not None else None


def _dup_opt(distance: int, max_set: int):
    return DupOpt(distance, 0, max_set)


def lib_rows(lib_stats) -> list:
    """DUP_LIB_STATS_DTYPE rows as the dicts bwams.markdup's decide2 / mark2 give"""
    return [{k: (float(r[k]) if k == "percent_duplication" else int(r[k])) for k in DUP_LIB_STATS_DTYPE.names} for r in lib_stats]


def dup_decide2(device: int, ends, locs, n_templates: int, n_lib: int = 1, distance: int = 0, max_set: int = 0, opt=True):
    """bwams_dup_decide2 over ends (DUP_END_DTYPE) and locs (DUP_LOC_DTYPE, or None) -> (dup, optical: uint8 per template, rows:
    DUP_LIB_STATS_DTYPE per library).  opt=False passes a NULL bwams_dup_opt_t."""
    ends = np.ascontiguousarray(ends, DUP_END_DTYPE)
    if locs is not None:
        locs = np.ascontiguousarray(locs, DUP_LOC_DTYPE)
        assert len(locs) == len(ends)
    dup, optical = np.zeros(max(n_templates, 1), np.uint8), np.zeros(max(n_templates, 1), np.uint8)
    rows = np.zeros(max(n_lib, 1), DUP_LIB_STATS_DTYPE)
    o = _dup_opt(distance, max_set)
    _chk(lib().bwams_dup_decide2(device, _p(ends), _p(locs) if locs is not None else None, len(ends), n_templates, n_lib,
                                 C.byref(o) if opt else None, _p(dup), _p(optical), _p(rows)), "bwams_dup_decide2")
    return dup[:n_templates], optical[:n_templates], rows[:n_lib]


def dup_library_size(n: int, c: int):
    """Rule 14 (bwams_dup_library_size): the estimate, or None."""
    v = lib().bwams_dup_library_size(n, c)
    return None if v < 0 else v


def _text(fn, *args) -> str:
    """The text of a library function whose last arguments are (out, cap, n): asked for its size with no buffer (BWAMS_ERR_CAPACITY
    gives it), then for the text."""
    n = C.c_int64(0)
    rc = fn(*args, None, 0, C.byref(n))
    if rc != -4:
        _chk(rc, fn.__name__)
    buf = C.create_string_buffer(max(n.value, 1))
    _chk(fn(*args, buf, n.value, C.byref(n)), fn.__name__)
    return buf.raw[:n.value].decode("latin-1")


def dup_metrics_text(groups, lib_stats, comment: str = "") -> str:
    """Rule 15 (bwams_dup_metrics_text) of DUP_LIB_STATS_DTYPE rows."""
    rows = np.ascontiguousarray(lib_stats, DUP_LIB_STATS_DTYPE)
    return _text(lib().bwams_dup_metrics_text, _groups_h(groups), _p(rows), len(rows), comment.encode())


class _Handle:
    """A library handle in .h that the function named by _close gives back, once."""
    _close = ""

    def _call(self, name: str, *args) -> None:
        _chk(getattr(lib(), name)(self.h, *args), name)

    def _info(self, name: str, struct) -> dict:
        i = struct()
        self._call(name, C.byref(i))
        return {k: getattr(i, k) for k, _ in struct._fields_}

    def close(self):
        h, self.h = self.h, C.c_void_p()
        if h:
            _chk(getattr(lib(), self._close)(h), self._close)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Consumer(_Handle):
    """A handle that BAM records are added to, through the functions _prefix + "_add_batch", "_add_records" and "_reset"."""
    _prefix = ""

    def add_batch(self, batch: "Batch") -> int:
        """The batch's current BAM records, read in HBM; -> the records that counted."""
        n = C.c_int64(0)
        self._call(self._prefix + "_add_batch", batch.h, C.byref(n))
        return n.value

    def add_records(self, records: bytes) -> int:
        records = bytes(records)
        n = C.c_int64(0)
        self._call(self._prefix + "_add_records", records, len(records), C.byref(n))
        return n.value

    def add_file(self, bam_file: "BamFile") -> int:
        """The current piece of a BamFile, read in HBM; -> the records that counted."""
        n = C.c_int64(0)
        self._call(self._prefix + "_add_file", bam_file.h, C.byref(n))
        return n.value

    def reset(self) -> None:
        self._call(self._prefix + "_reset")


class SorterStats(C.Structure):
    _fields_ = [("runs", C.c_int64), ("records", C.c_int64), ("spilled_runs", C.c_int64), ("spilled_bytes", C.c_int64),
                ("out_bytes", C.c_int64), ("ms_merge", C.c_float), ("ms_deflate", C.c_float), ("ms_write", C.c_float)]


class Sorter:
    """A coordinate-sorted BAM file (and its .bai) from sorted runs (bwams_sorter_t)."""

    def __init__(self, path: str, device: int, bam_header: bytes, tmp_prefix: str | None = None, mem_bytes: int = 4 << 30,
                 bai: bool = True, markdup: bool = False):
        self.h = C.c_void_p()
        hdr = bytes(bam_header)
        flags = (SORT_BAI if bai else 0) | (SORT_MARKDUP if markdup else 0)
        _chk(lib().bwams_sorter_open(path.encode(), device, hdr, len(hdr), tmp_prefix.encode() if tmp_prefix else None, mem_bytes,
                                     flags, C.byref(self.h)), "bwams_sorter_open")

    def put(self, seq: int, records: bytes, coords) -> None:
        """One sorted run: records (bytes) and their coords (BAM_COORD_DTYPE)."""
        records = bytes(records)
        coords = np.ascontiguousarray(coords, BAM_COORD_DTYPE)
        _chk(lib().bwams_sorter_put(self.h, seq, records, len(records), _p(coords), len(coords)), "bwams_sorter_put")

    def put_batch(self, seq: int, batch: "Batch") -> None:
        _chk(lib().bwams_sorter_put_batch(self.h, seq, batch.h), "bwams_sorter_put_batch")

    def set_markdup(self, groups=None, distance: int = 0, max_set: int = 0) -> None:
        """bwams_sorter_set_markdup: the groups table (a DupGroups or None; copied) and the optical options, before the first put."""
        o = _dup_opt(distance, max_set)
        _chk(lib().bwams_sorter_set_markdup(self.h, _groups_h(groups), C.byref(o)), "bwams_sorter_set_markdup")
        self._n_lib = groups.n_lib if groups is not None else 1

    def set_depth(self, depth: "Depth") -> None:
        """bwams_sorter_set_depth: close adds the merged stream, as written, to the handle; before the first put."""
        _chk(lib().bwams_sorter_set_depth(self.h, depth.h), "bwams_sorter_set_depth")

    def set_pileup(self, pileup: "Pileup") -> None:
        """bwams_sorter_set_pileup: close adds the merged stream, as written, to the handle; before the first put."""
        _chk(lib().bwams_sorter_set_pileup(self.h, pileup.h), "bwams_sorter_set_pileup")

    def set_qc(self, qc: "Qc") -> None:
        """bwams_sorter_set_qc: close adds the merged stream, as written, to the handle; before the first put."""
        _chk(lib().bwams_sorter_set_qc(self.h, qc.h), "bwams_sorter_set_qc")

    def set_recal(self, recal: "Recal") -> None:
        """bwams_sorter_set_recal: close adds the merged stream, as written, to the handle; before the first put."""
        _chk(lib().bwams_sorter_set_recal(self.h, recal.h), "bwams_sorter_set_recal")

    def close3(self) -> SorterStats:
        """bwams_sorter_close3: close()'s stats, .dup, and rule 13's rows as .lib (DUP_LIB_STATS_DTYPE)."""
        st, dup = SorterStats(), DupStats()
        rows = np.zeros(getattr(self, "_n_lib", 1), DUP_LIB_STATS_DTYPE)
        h, self.h = self.h, C.c_void_p()
        if h:
            _chk(lib().bwams_sorter_close3(h, C.byref(st), C.byref(dup), _p(rows), len(rows)), "bwams_sorter_close3")
        st.dup, st.lib = dup, rows
        return st

    def close(self) -> SorterStats:
        """bwams_sorter_close2: the sorter's stats, with the duplicate-marking counts as .dup (a DupStats, zeros without markdup)."""
        st, dup = SorterStats(), DupStats()
        h, self.h = self.h, C.c_void_p()
        if h:
            _chk(lib().bwams_sorter_close2(h, C.byref(st), C.byref(dup)), "bwams_sorter_close2")
        st.dup = dup
        return st

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DepthOpt(C.Structure):
    _fields_ = [("exclude", C.c_uint32), ("min_mapq", C.c_int32), ("count_deletions", C.c_int32), ("reserved", C.c_int32)]


class Depth(_Consumer):
    """Per-base depth of coverage on one GPU (bwams_depth_t): add, finish once, query."""
    _prefix, _close = "bwams_depth", "bwams_depth_close"

    def __init__(self, l_ref, device: int = 0, exclude: int = 0x704, min_mapq: int = 0, count_deletions: bool = False):
        self.h = C.c_void_p()
        self.l_ref = np.ascontiguousarray(l_ref, np.int32)
        o = DepthOpt(exclude, min_mapq, int(count_deletions), 0)
        _chk(lib().bwams_depth_open(device, _p(self.l_ref), len(self.l_ref), C.byref(o), C.byref(self.h)), "bwams_depth_open")

    def finish(self) -> "Depth":
        _chk(lib().bwams_depth_finish(self.h), "bwams_depth_finish")
        return self

    def summary(self) -> np.ndarray:
        rows = np.zeros(len(self.l_ref), DEPTH_REF_DTYPE)
        _chk(lib().bwams_depth_summary(self.h, _p(rows), len(rows)), "bwams_depth_summary")
        return rows

    def hist(self, ref: int, n_bins: int) -> np.ndarray:
        h = np.zeros(max(n_bins, 1), np.int64)
        _chk(lib().bwams_depth_hist(self.h, ref, _p(h), n_bins), "bwams_depth_hist")
        return h

    def windows(self, w: int) -> np.ndarray:
        n = C.c_int64(0)
        _chk(lib().bwams_depth_windows(self.h, w, None, 0, C.byref(n)), "bwams_depth_windows")
        sums = np.zeros(n.value, np.int64)
        _chk(lib().bwams_depth_windows(self.h, w, _p(sums), len(sums), C.byref(n)), "bwams_depth_windows")
        return sums

    def runs(self, ref: int, beg: int, end: int, cap: int | None = None):
        """(start, depth) of rule 10; cap: the arrays' size (default: asked for first)."""
        n = C.c_int64(0)
        if cap is None:
            _chk(lib().bwams_depth_runs(self.h, ref, beg, end, None, None, 0, C.byref(n)), "bwams_depth_runs")
            cap = n.value
        start, depth = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
        rc = lib().bwams_depth_runs(self.h, ref, beg, end, _p(start), _p(depth), cap, C.byref(n))
        self.n_runs = n.value
        _chk(rc, "bwams_depth_runs")
        return start[:n.value], depth[:n.value]

    def fetch(self, ref: int, beg: int = 0, end: int | None = None) -> np.ndarray:
        end = int(self.l_ref[ref]) if end is None else end
        out = np.zeros(max(end - beg, 1), np.int32)
        _chk(lib().bwams_depth_fetch(self.h, ref, beg, end, _p(out)), "bwams_depth_fetch")
        return out[:max(end - beg, 0)]

    def text(self, names, what: int, arg: int = 0) -> str:
        """bwams_depth_text: what = 0 summary, 1 distribution (arg: n_bins), 2 windows BED (arg: w)."""
        flat = b"".join((n if isinstance(n, bytes) else n.encode()) + b"\0" for n in names)
        return _text(lib().bwams_depth_text, self.h, flat, what, arg)


class PileupOpt(C.Structure):
    _fields_ = [("exclude", C.c_uint32), ("min_mapq", C.c_int32), ("min_baseq", C.c_int32), ("min_alt", C.c_int32),
                ("min_permille", C.c_int32), ("reserved", C.c_int32)]


class PileupGlOpt(C.Structure):
    _fields_ = [("min_qual", C.c_int32), ("min_depth", C.c_int32), ("no_qual_q", C.c_int32), ("reserved", C.c_int32)]


class PileupInfo(C.Structure):
    _fields_ = [("tile", C.c_int32), ("n_regions", C.c_int32), ("n_slots", C.c_int64), ("n_counted", C.c_int64), ("n_entries", C.c_int64),
                ("n_direct", C.c_int64), ("ms_check", C.c_float), ("ms_add", C.c_float)]


class PileupIndelOpt(C.Structure):
    _fields_ = [("min_qual", C.c_int32), ("min_depth", C.c_int32), ("indel_q", C.c_int32), ("max_len", C.c_int32), ("reserved", C.c_int32)]


class PileupIndelInfo(C.Structure):
    _fields_ = [("n_events", C.c_int64), ("cap_events", C.c_int64), ("n_appended", C.c_int64), ("ms_indel", C.c_float), ("reserved", C.c_int32)]


class Pileup(_Consumer):
    """Per-base allele counts over regions on one GPU (bwams_pileup_t): add, then fetch, sites or text at any time."""
    _prefix, _close = "bwams_pileup", "bwams_pileup_close"

    def __init__(self, l_ref, regions=(), device: int = 0, exclude: int = 0x704, min_mapq: int = 0, min_baseq: int = 13, min_alt: int = 2,
                 min_permille: int = 200):
        self.h = C.c_void_p()
        self.l_ref = np.ascontiguousarray(l_ref, np.int32)
        reg = np.zeros(len(regions), PILEUP_REGION_DTYPE)
        for k, (r, b, e) in enumerate(regions):
            reg[k] = (r, b, e)
        o = PileupOpt(exclude, min_mapq, min_baseq, min_alt, min_permille, 0)
        _chk(lib().bwams_pileup_open(device, _p(self.l_ref), len(self.l_ref), _p(reg), len(reg), C.byref(o), C.byref(self.h)),
             "bwams_pileup_open")
        self.regions = [tuple(int(v) for v in r) for r in regions] or [(r, 0, int(n)) for r, n in enumerate(self.l_ref) if n > 0]

    def set_ref(self, region: int, codes) -> None:
        """The reference codes (0..4) of one region, end - beg of them."""
        r, b, e = self.regions[region]
        codes = np.ascontiguousarray(codes, np.uint8)
        assert len(codes) == e - b
        _chk(lib().bwams_pileup_set_ref(self.h, region, _p(codes)), "bwams_pileup_set_ref")

    def set_ref_index(self, index: "Index") -> None:
        _chk(lib().bwams_pileup_set_ref_index(self.h, index.h), "bwams_pileup_set_ref_index")

    def fetch(self, region: int, beg: int | None = None, end: int | None = None) -> np.ndarray:
        """uint32[end - beg, 12]: the counters of positions [beg, end) of the region (default: all of it)."""
        r, b, e = self.regions[region]
        beg, end = b if beg is None else beg, e if end is None else end
        out = np.zeros((max(end - beg, 1), 12), np.uint32)
        _chk(lib().bwams_pileup_fetch(self.h, region, beg, end, _p(out)), "bwams_pileup_fetch")
        return out[:max(end - beg, 0)]

    def sites(self, min_alt: int = -1, min_permille: int = -1, cap: int | None = None) -> np.ndarray:
        """PILEUP_SITE_DTYPE records of rule 8; cap: the array's size (default: asked for first).  .n_sites: found or needed."""
        n = C.c_int64(0)
        if cap is None:
            _chk(lib().bwams_pileup_sites(self.h, min_alt, min_permille, None, 0, C.byref(n)), "bwams_pileup_sites")
            cap = n.value
        out = np.zeros(max(cap, 1), PILEUP_SITE_DTYPE)
        rc = lib().bwams_pileup_sites(self.h, min_alt, min_permille, _p(out), cap, C.byref(n))
        self.n_sites = n.value
        _chk(rc, "bwams_pileup_sites")
        return out[:n.value]

    def text(self, names, min_alt: int = -1, min_permille: int = -1) -> str:
        flat = b"".join((n if isinstance(n, bytes) else n.encode()) + b"\0" for n in names)
        return _text(lib().bwams_pileup_text, self.h, flat, min_alt, min_permille)

    def set_quality(self, min_qual: int = 20, min_depth: int = 1, no_qual_q: int = 30) -> None:
        """bwams_pileup_set_quality: the quality plane beside the counters, zeroed; only while the counters are zero."""
        o = PileupGlOpt(min_qual, min_depth, no_qual_q, 0)
        _chk(lib().bwams_pileup_set_quality(self.h, C.byref(o)), "bwams_pileup_set_quality")

    def fetch_quality(self, region: int, beg: int | None = None, end: int | None = None) -> np.ndarray:
        """uint32[end - beg, 12]: the sums Q[A..T], HOM[A..T], HET[A..T] of positions [beg, end) of the region (default: all of it)."""
        r, b, e = self.regions[region]
        beg, end = b if beg is None else beg, e if end is None else end
        out = np.zeros((max(end - beg, 1), 12), np.uint32)
        _chk(lib().bwams_pileup_fetch_quality(self.h, region, beg, end, _p(out)), "bwams_pileup_fetch_quality")
        return out[:max(end - beg, 0)]

    def calls(self, min_qual: int = -1, min_depth: int = -1, cap: int | None = None) -> np.ndarray:
        """PILEUP_CALL_DTYPE records of rule 13; cap: the array's size (default: asked for first).  .n_calls: found or needed."""
        n = C.c_int64(0)
        if cap is None:
            _chk(lib().bwams_pileup_calls(self.h, min_qual, min_depth, None, 0, C.byref(n)), "bwams_pileup_calls")
            cap = n.value
        out = np.zeros(max(cap, 1), PILEUP_CALL_DTYPE)
        rc = lib().bwams_pileup_calls(self.h, min_qual, min_depth, _p(out), cap, C.byref(n))
        self.n_calls = n.value
        _chk(rc, "bwams_pileup_calls")
        return out[:n.value]

    def vcf(self, names, sample, min_qual: int = -1, min_depth: int = -1) -> str:
        flat = b"".join((n if isinstance(n, bytes) else n.encode()) + b"\0" for n in names)
        return _text(lib().bwams_pileup_vcf, self.h, flat, sample if isinstance(sample, bytes) else sample.encode(), min_qual, min_depth)

    def info(self) -> dict:
        """bwams_pileup_info: tile, n_regions, n_slots, and of the last add n_counted, n_entries, n_direct, ms_check, ms_add."""
        return self._info("bwams_pileup_info", PileupInfo)

    def set_indels(self, min_qual: int = 20, min_depth: int = 1, indel_q: int = 40, max_len: int = 32) -> None:
        """bwams_pileup_set_indels: the indel store (rules 14 to 17), empty; only while the counters are zero."""
        o = PileupIndelOpt(min_qual, min_depth, indel_q, max_len, 0)
        _chk(lib().bwams_pileup_set_indels(self.h, C.byref(o)), "bwams_pileup_set_indels")

    def set_indel_leftalign(self, on: bool = True) -> None:
        """bwams_pileup_set_indel_leftalign: rule 18 for the adds that follow; needs the store, zero counters, and the reference before the records."""
        _chk(lib().bwams_pileup_set_indel_leftalign(self.h, int(on)), "bwams_pileup_set_indel_leftalign")

    def fetch_span(self, region: int, beg: int | None = None, end: int | None = None) -> np.ndarray:
        """uint32[end - beg, 4]: SPAN_N, SPAN_Q, SPAN_HOM, SPAN_HET of positions [beg, end) of the region (default: all of it)."""
        r, b, e = self.regions[region]
        beg, end = b if beg is None else beg, e if end is None else end
        out = np.zeros((max(end - beg, 1), 4), np.uint32)
        _chk(lib().bwams_pileup_fetch_span(self.h, region, beg, end, _p(out)), "bwams_pileup_fetch_span")
        return out[:max(end - beg, 0)]

    def indel_alleles(self, cap: int | None = None) -> np.ndarray:
        """PILEUP_INDEL_ALLELE_DTYPE records of rule 17, every group; cap: the array's size (default: asked for first)."""
        n = C.c_int64(0)
        if cap is None:
            _chk(lib().bwams_pileup_indel_alleles(self.h, None, 0, C.byref(n)), "bwams_pileup_indel_alleles")
            cap = n.value
        out = np.zeros(max(cap, 1), PILEUP_INDEL_ALLELE_DTYPE)
        rc = lib().bwams_pileup_indel_alleles(self.h, _p(out), cap, C.byref(n))
        self.n_alleles = n.value
        _chk(rc, "bwams_pileup_indel_alleles")
        return out[:n.value]

    def indel_calls(self, min_qual: int = -1, min_depth: int = -1, cap: int | None = None) -> np.ndarray:
        """PILEUP_INDEL_DTYPE records of rule 16; cap: the array's size (default: asked for first).  .n_indel_calls: found or needed."""
        n = C.c_int64(0)
        if cap is None:
            _chk(lib().bwams_pileup_indel_calls(self.h, min_qual, min_depth, None, 0, C.byref(n)), "bwams_pileup_indel_calls")
            cap = n.value
        out = np.zeros(max(cap, 1), PILEUP_INDEL_DTYPE)
        rc = lib().bwams_pileup_indel_calls(self.h, min_qual, min_depth, _p(out), cap, C.byref(n))
        self.n_indel_calls = n.value
        _chk(rc, "bwams_pileup_indel_calls")
        return out[:n.value]

    def indel_vcf(self, names, sample, min_qual: int = -1, min_depth: int = -1) -> str:
        flat = b"".join((n if isinstance(n, bytes) else n.encode()) + b"\0" for n in names)
        return _text(lib().bwams_pileup_indel_vcf, self.h, flat, sample if isinstance(sample, bytes) else sample.encode(), min_qual, min_depth)

    def vcf_all(self, names, sample, min_qual: int = -1, min_depth: int = -1, indel_min_qual: int = -1, indel_min_depth: int = -1) -> str:
        """bwams_pileup_vcf_all: the SNV rows and the indel rows under one header; needs the quality plane and the indel store."""
        flat = b"".join((n if isinstance(n, bytes) else n.encode()) + b"\0" for n in names)
        return _text(lib().bwams_pileup_vcf_all, self.h, flat, sample if isinstance(sample, bytes) else sample.encode(), min_qual, min_depth,
                     indel_min_qual, indel_min_depth)

    def indel_info(self) -> dict:
        """bwams_pileup_indel_info: n_events, cap_events, and of the last add n_appended and ms_indel."""
        return self._info("bwams_pileup_indel_info", PileupIndelInfo)


class QcOpt(C.Structure):
    _fields_ = [("exclude", C.c_uint32), ("max_cycle", C.c_int32), ("max_isize", C.c_int32), ("reserved", C.c_int32)]


class QcSummary(C.Structure):
    _fields_ = [("flags", C.c_int64 * 16 * 2), ("scalars", C.c_int64 * 16)]


class QcInfo(C.Structure):
    _fields_ = [("isize_lds", C.c_int32), ("slice", C.c_int32), ("n_records", C.c_int64), ("n_counted", C.c_int64),
                ("bases_over", C.c_int64), ("ms_check", C.c_float), ("ms_add", C.c_float)]


class Qc(_Consumer):
    """Alignment QC on one GPU (bwams_qc_t): flag counts, insert sizes and per-cycle tables; add, then query at any time."""
    _prefix, _close = "bwams_qc", "bwams_qc_close"

    def __init__(self, device: int = 0, exclude: int = 0x900, max_cycle: int = 512, max_isize: int = 8000):
        self.h = C.c_void_p()
        self.max_cycle, self.max_isize = max_cycle, max_isize
        o = QcOpt(exclude, max_cycle, max_isize, 0)
        _chk(lib().bwams_qc_open(device, C.byref(o), C.byref(self.h)), "bwams_qc_open")

    def add_batch(self, batch: "Batch") -> int:
        """The batch's current BAM records, read in HBM; -> the records that rule 3's filter let through."""
        return super().add_batch(batch)

    def summary(self):
        """(flags int64[2, 16], scalars int64[16]) of rules 2 and 5"""
        s = QcSummary()
        _chk(lib().bwams_qc_summary(self.h, C.byref(s)), "bwams_qc_summary")
        return np.array(s.flags, np.int64).reshape(2, 16), np.array(s.scalars, np.int64)

    def table(self, what: int) -> np.ndarray:
        """int64, flat: table `what` of rule 4 (0 RL, 1 QUAL, 2 BASE, 3 MAPQ, 4 ISIZE, 5 INDEL)"""
        n = C.c_int64(0)
        _chk(lib().bwams_qc_table(self.h, what, None, 0, C.byref(n)), "bwams_qc_table")
        out = np.zeros(n.value, np.int64)
        _chk(lib().bwams_qc_table(self.h, what, _p(out), len(out), C.byref(n)), "bwams_qc_table")
        return out

    def text(self, what: int) -> str:
        """bwams_qc_text: what = 0 the flagstat lines, 1 the stats sections."""
        return _text(lib().bwams_qc_text, self.h, what)

    def info(self) -> dict:
        """bwams_qc_info: isize_lds, slice, and of the last add n_records, n_counted, bases_over, ms_check, ms_add."""
        return self._info("bwams_qc_info", QcInfo)


class RecalOpt(C.Structure):
    _fields_ = [("exclude", C.c_uint32), ("min_mapq", C.c_int32), ("min_baseq", C.c_int32), ("max_cycle", C.c_int32), ("reserved", C.c_int32)]


class RecalInfo(C.Structure):
    _fields_ = [("lds", C.c_int32), ("slice", C.c_int32), ("n_records", C.c_int64), ("n_counted", C.c_int64), ("n_bases", C.c_int64),
                ("store_bytes", C.c_int64), ("ms_check", C.c_float), ("ms_add", C.c_float)]


RECAL_SITE_DTYPE = np.dtype([("ref", "<i4"), ("beg", "<i4"), ("end", "<i4")])


class Recal(_Consumer):
    """Base recalibration tables on one GPU (bwams_recal_t): set the reference and the known sites, add, then query at any time."""
    _prefix, _close = "bwams_recal", "bwams_recal_close"

    def __init__(self, l_ref, groups=None, device: int = 0, exclude: int = 0x704, min_mapq: int = 1, min_baseq: int = 6,
                 max_cycle: int = 500):
        self.h = C.c_void_p()
        self.l_ref = np.ascontiguousarray(l_ref, np.int32)
        self.groups = groups                                                             # a DupGroups or None; names the text's rows
        self.n_rg, self.max_cycle = (groups.n_rg if groups is not None else 0), max_cycle
        o = RecalOpt(exclude, min_mapq, min_baseq, max_cycle, 0)
        _chk(lib().bwams_recal_open(device, _p(self.l_ref), len(self.l_ref), _groups_h(groups), C.byref(o), C.byref(self.h)),
             "bwams_recal_open")

    def add_batch(self, batch: "Batch") -> int:
        """The batch's current BAM records, read in HBM; -> the records that rule 4 let through."""
        return super().add_batch(batch)

    def set_ref(self, ref: int, codes) -> None:
        """The codes (0..4) of one whole reference."""
        codes = np.ascontiguousarray(codes, np.uint8)
        assert len(codes) == self.l_ref[ref]
        _chk(lib().bwams_recal_set_ref(self.h, ref, _p(codes)), "bwams_recal_set_ref")

    def set_ref_index(self, index: "Index") -> None:
        _chk(lib().bwams_recal_set_ref_index(self.h, index.h), "bwams_recal_set_ref_index")

    def add_known(self, sites) -> None:
        """Intervals (ref, beg, end) of known variation."""
        a = np.zeros(len(sites), RECAL_SITE_DTYPE)
        for k, (r, b, e) in enumerate(sites):
            a[k] = (r, b, e)
        _chk(lib().bwams_recal_add_known(self.h, _p(a), len(a)), "bwams_recal_add_known")

    def table(self, what: int) -> np.ndarray:
        """int64 pairs (observations, errors) in the shape of rule 6: 0 RG, 1 QUAL, 2 CYCLE, 3 CONTEXT"""
        n = C.c_int64(0)
        _chk(lib().bwams_recal_table(self.h, what, None, 0, C.byref(n)), "bwams_recal_table")
        out = np.zeros(n.value, np.int64)
        _chk(lib().bwams_recal_table(self.h, what, _p(out), len(out), C.byref(n)), "bwams_recal_table")
        shape = [(), (94,), (94, 2 * self.max_cycle + 1), (94, 16)][what]
        return out.reshape((self.n_rg + 1,) + shape + (2,))

    def text(self) -> str:
        return _text(lib().bwams_recal_text, self.h, _groups_h(self.groups))

    def info(self) -> dict:
        """bwams_recal_info: lds, slice, store_bytes, and of the last add n_records, n_counted, n_bases, ms_check, ms_add."""
        return self._info("bwams_recal_info", RecalInfo)


class RecalModelOpt(C.Structure):
    _fields_ = [("exclude", C.c_uint32), ("preserve_below", C.c_int32), ("max_q", C.c_int32), ("prior_obs", C.c_int32), ("reserved", C.c_int32)]


class RecalApplyInfo(C.Structure):
    _fields_ = [("n_records", C.c_int64), ("n_rewritten", C.c_int64), ("model_bytes", C.c_int64), ("ms_check", C.c_float),
                ("ms_apply", C.c_float)]


def recal_model_constants():
    """bwams_recal_model_constants: (S[1..60], P[0..93]) as the library holds them"""
    s, p = np.zeros(60, np.int64), np.zeros(94, np.int64)
    _chk(lib().bwams_recal_model_constants(_p(s), _p(p)), "bwams_recal_model_constants")
    return s, p


class RecalModel(_Handle):
    """The quality model of base recalibration (bwams_recal_model_t, a host object): RecalModel(tables, max_cycle) from the four
    count tables in the shapes Recal.table gives, or RecalModel.of(recal) from a handle's tables."""
    _close = "bwams_recal_model_destroy"

    def __init__(self, tables, max_cycle: int, exclude: int = 0, preserve_below: int = 6, max_q: int = 60, prior_obs: int = 1024,
                 _from: "Recal | None" = None):
        self.h = C.c_void_p()
        o = RecalModelOpt(exclude, preserve_below, max_q, prior_obs, 0)
        if _from is not None:
            _chk(lib().bwams_recal_model_from(_from.h, C.byref(o), C.byref(self.h)), "bwams_recal_model_from")
            self.n_rg = _from.n_rg
        else:
            t = [np.ascontiguousarray(x, np.int64) for x in tables]
            self.n_rg = t[0].shape[0] - 1
            _chk(lib().bwams_recal_model_create(_p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), self.n_rg, max_cycle, C.byref(o), C.byref(self.h)),
                 "bwams_recal_model_create")
        self.max_cycle = max_cycle

    @classmethod
    def of(cls, recal: "Recal", **opt) -> "RecalModel":
        return cls(None, recal.max_cycle, _from=recal, **opt)

    def table(self, what: int) -> np.ndarray:
        """int16: 0 RG [n_rg + 1][3] = (Qrep, QG, G), 1 QUAL B [n_rg + 1][94], 2 CYCLE DC [..][94][2 max_cycle + 1], 3 CONTEXT DX [..][94][16]"""
        n = C.c_int64(0)
        _chk(lib().bwams_recal_model_table(self.h, what, None, 0, C.byref(n)), "bwams_recal_model_table")
        out = np.zeros(n.value, np.int16)
        _chk(lib().bwams_recal_model_table(self.h, what, _p(out), len(out), C.byref(n)), "bwams_recal_model_table")
        return out.reshape((self.n_rg + 1,) + [(3,), (94,), (94, 2 * self.max_cycle + 1), (94, 16)][what])


class RecalApply(_Handle):
    """A model on one GPU (bwams_recal_apply_t): rewrites the QUAL bytes of host records or of a batch's BAM records."""
    _close = "bwams_recal_apply_close"

    def __init__(self, model: RecalModel, groups=None, device: int = 0):
        self.h = C.c_void_p()
        _chk(lib().bwams_recal_apply_open(device, model.h, _groups_h(groups), C.byref(self.h)), "bwams_recal_apply_open")

    def records(self, records: bytes):
        """-> (the records with their new QUAL, the records rewritten)"""
        buf = np.frombuffer(bytes(records), np.uint8).copy()
        n = C.c_int64(0)
        _chk(lib().bwams_recal_apply_records(self.h, _p(buf), len(buf), C.byref(n)), "bwams_recal_apply_records")
        return buf.tobytes(), n.value

    def batch(self, batch: "Batch") -> int:
        """The batch's current BAM records, and their sorted copy when there is one, rewritten in HBM; -> the records rewritten."""
        n = C.c_int64(0)
        _chk(lib().bwams_recal_apply_batch(self.h, batch.h, C.byref(n)), "bwams_recal_apply_batch")
        return n.value

    def file(self, bam_file: "BamFile") -> int:
        """The current piece of a BamFile rewritten in HBM (BamFile.fetch then gives the new bytes); -> the records rewritten."""
        n = C.c_int64(0)
        _chk(lib().bwams_recal_apply_file(self.h, bam_file.h, C.byref(n)), "bwams_recal_apply_file")
        return n.value

    def info(self) -> dict:
        """bwams_recal_apply_info: model_bytes, and of the last apply n_records, n_rewritten, ms_check, ms_apply."""
        return self._info("bwams_recal_apply_info", RecalApplyInfo)


class BamFileInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("intervals", "members", "compressed_bytes", "inflated_bytes", "candidates", "records_seen",
                                         "records_kept", "pieces", "carried")] + \
               [(n, C.c_float) for n in ("ms_read", "ms_inflate", "ms_discover", "ms_select", "ms_gather")] + [("pad_", C.c_int32)]


class BamMergeOpt(C.Structure):
    _fields_ = [("child_bytes", C.c_int64), ("reserved", C.c_int32), ("pad_", C.c_int32)]


class BamMergeInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_files", "child_bytes", "rounds", "refills", "records", "bytes", "max_piece_records",
                                         "max_piece_bytes", "max_window_left")] + [("pg_dropped", C.c_int32), ("pad_", C.c_int32)] + \
               [(n, C.c_float) for n in ("ms_check", "ms_frontier", "ms_rank", "ms_scan", "ms_gather", "ms_refill")]


def bam_header_merge(blocks) -> tuple[bytes, int]:
    """bwams_bam_header_merge: (the merged BAM header block, the @PG lines dropped) of the files' header blocks (host only)."""
    blocks = [bytes(b) for b in blocks]
    ptr = (C.c_char_p * max(len(blocks), 1))(*blocks)
    sizes = (C.c_int64 * max(len(blocks), 1))(*[len(b) for b in blocks])
    n, dropped = C.c_int64(0), C.c_int32(0)
    rc = lib().bwams_bam_header_merge(ptr, sizes, len(blocks), None, 0, C.byref(n), C.byref(dropped))
    if rc != -4:
        _chk(rc, "bwams_bam_header_merge")
    out = C.create_string_buffer(max(n.value, 1))
    _chk(lib().bwams_bam_header_merge(ptr, sizes, len(blocks), out, n.value, C.byref(n), C.byref(dropped)), "bwams_bam_header_merge")
    return out.raw[:n.value], dropped.value


def _regions(regions):
    a = np.zeros(len(regions), PILEUP_REGION_DTYPE)
    for k, (r, b, e) in enumerate(regions):
        a[k] = (r, b, e)
    return a


def bai_plan(bai: bytes, regions) -> list:
    """bwams_bai_plan: rule 3's intervals [(beg, end), ...] of virtual offsets from the bytes of a BAI (host only)."""
    bai = bytes(bai)
    a = _regions(regions)
    n = C.c_int64(0)
    rc = lib().bwams_bai_plan(bai, len(bai), _p(a), len(a), None, None, 0, C.byref(n))
    if rc != -4:
        _chk(rc, "bwams_bai_plan")
    b, e = np.zeros(max(n.value, 1), np.uint64), np.zeros(max(n.value, 1), np.uint64)
    _chk(lib().bwams_bai_plan(bai, len(bai), _p(a), len(a), _p(b), _p(e), n.value, C.byref(n)), "bwams_bai_plan")
    return [(int(x), int(y)) for x, y in zip(b[:n.value], e[:n.value])]


class BamFile(_Handle):
    """A coordinate-sorted BAM file read back by region on one GPU (bwams_bam_file_t): query, then next() until done; fetch() or a
    consumer's add_file() takes the current piece."""
    _close = "bwams_bam_file_close"

    def __init__(self, path: str, bai_path: str | None = None, device: int = 0, piece_bytes: int = 0):
        self.h = C.c_void_p()
        _chk(lib().bwams_bam_file_open(path.encode(), bai_path.encode() if bai_path else None, device, piece_bytes, C.byref(self.h)),
             "bwams_bam_file_open")
        self.n_records = self.n_bytes = 0

    @classmethod
    def merge(cls, paths, bai_paths=None, device: int = 0, piece_bytes: int = 0, child_bytes: int = 0, reserved: int = 0) -> "BamFile":
        """bwams_bam_file_open_merge: the coordinate-sorted files at `paths` as one record stream in coordinate order; every other
        call is the same as on one file.  bai_paths: None, or a path or None per file."""
        paths = [p.encode() for p in paths]
        ptr = (C.c_char_p * max(len(paths), 1))(*paths)
        bai = None
        if bai_paths is not None:
            bai = (C.c_char_p * max(len(paths), 1))(*[b.encode() if b else None for b in bai_paths])
        opt = BamMergeOpt(child_bytes, reserved, 0)
        f = cls.__new__(cls)
        f.h = C.c_void_p()
        f.n_records = f.n_bytes = 0
        _chk(lib().bwams_bam_file_open_merge(ptr, bai, len(paths), device, piece_bytes, C.byref(opt) if child_bytes or reserved else None,
                                             C.byref(f.h)), "bwams_bam_file_open_merge")
        return f

    def merge_info(self) -> dict:
        """bwams_bam_merge_info: a merged handle's counts and stage times since the last query"""
        return self._info("bwams_bam_merge_info", BamMergeInfo)

    def header(self) -> tuple[bytes, int]:
        """(the header text, n_ref)"""
        t, n, nr = C.c_void_p(), C.c_int64(0), C.c_int32(0)
        self._call("bwams_bam_file_header", C.byref(t), C.byref(n), C.byref(nr))
        return C.string_at(t, n.value) if n.value else b"", nr.value

    def header_block(self) -> bytes:
        """the file's BAM header (magic to the last reference) as Sorter takes it"""
        b, n = C.c_void_p(), C.c_int64(0)
        self._call("bwams_bam_file_header_block", C.byref(b), C.byref(n))
        return C.string_at(b, n.value) if n.value else b""

    def refs(self) -> np.ndarray:
        """the references' lengths"""
        out = np.zeros(max(self.header()[1], 1), np.int32)
        self._call("bwams_bam_file_refs", _p(out), len(out))
        return out[:self.header()[1]]

    def query(self, regions=()) -> "BamFile":
        """regions: (ref, beg, end) triples; none: the whole file"""
        a = _regions(regions)
        self._call("bwams_bam_file_query", _p(a), len(a))
        return self

    def next(self) -> bool:
        """Makes the next piece current (.n_records, .n_bytes); -> done"""
        n, nb, done = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        self._call("bwams_bam_file_next", C.byref(n), C.byref(nb), C.byref(done))
        self.n_records, self.n_bytes = n.value, nb.value
        return bool(done.value)

    def fetch(self):
        """-> (the current piece's records, their coords as BAM_COORD_DTYPE)"""
        buf = np.zeros(max(self.n_bytes, 1), np.uint8)
        coords = np.zeros(max(self.n_records, 1), BAM_COORD_DTYPE)
        self._call("bwams_bam_file_fetch", _p(buf), self.n_bytes, _p(coords))
        return buf[:self.n_bytes].tobytes(), coords[:self.n_records]

    def pieces(self):
        """Iterates over the query's pieces: each is current while the loop body runs."""
        done = False
        while not done:
            done = self.next()
            yield self

    def read(self, regions=()):
        """The whole query fetched: (records, coords)"""
        self.query(regions)
        got = [p.fetch() for p in self.pieces()]
        return b"".join(r for r, _ in got), np.concatenate([c for _, c in got])

    def info(self) -> dict:
        """bwams_bam_file_info: the totals since the last query"""
        return self._info("bwams_bam_file_info", BamFileInfo)


class DupJoinInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("records", "templates", "ends", "adds", "applied", "hbm_bytes", "entry_bytes")] + \
               [("state", C.c_int32), ("pad_", C.c_int32)] + \
               [(n, C.c_float) for n in ("ms_add", "ms_sort", "ms_ends", "ms_decide", "ms_apply", "pad2_")]


def dupjoin_key(name: bytes) -> tuple[int, int]:
    """bwams_dupjoin_key: rule J1's (k0, k1) of a read name, computed by the library on the host"""
    name = bytes(name)
    key = (C.c_uint64 * 2)()
    _chk(lib().bwams_dupjoin_key(name, len(name), key), "bwams_dupjoin_key")
    return int(key[0]), int(key[1])


class DupJoin(_Consumer):
    """Duplicate marking of records that are not query-grouped (bwams_dupjoin_t): templates joined by name.  Pass 1: add_records /
    add_file over every piece; finish(); pass 2: apply_records / apply_file over the same pieces in the same order."""
    _close = "bwams_dupjoin_close"
    _prefix = "bwams_dupjoin"

    def __init__(self, groups=None, device: int = 0, distance: int = 0, max_set: int = 0, opt=True):
        self.h = C.c_void_p()
        o = _dup_opt(distance, max_set)
        self.n_lib = groups.n_lib if groups is not None else 1
        _chk(lib().bwams_dupjoin_open(device, _groups_h(groups), C.byref(o) if opt else None, C.byref(self.h)), "bwams_dupjoin_open")

    def add_batch(self, batch: "Batch") -> int:
        raise NotImplementedError("a batch's templates are adjacent: Batch.bam_markdup2 serves them")

    def finish(self):
        """-> (DupStats, rule 13's rows as DUP_LIB_STATS_DTYPE)"""
        st = DupStats()
        rows = np.zeros(self.n_lib, DUP_LIB_STATS_DTYPE)
        self._call("bwams_dupjoin_finish", C.byref(st), _p(rows), len(rows))
        return st, rows

    def fetch(self):
        """-> (ends: DUP_END_DTYPE, locs: DUP_LOC_DTYPE, rec_tmpl: uint32 by ordinal, dup, optical: uint8 per template)"""
        i = self.info()
        ends, locs = np.zeros(max(i["ends"], 1), DUP_END_DTYPE), np.zeros(max(i["ends"], 1), DUP_LOC_DTYPE)
        rt = np.zeros(max(i["records"], 1), np.uint32)
        dup, optical = np.zeros(max(i["templates"], 1), np.uint8), np.zeros(max(i["templates"], 1), np.uint8)
        self._call("bwams_dupjoin_fetch", _p(ends), _p(locs), i["ends"], _p(rt), i["records"], _p(dup), _p(optical), i["templates"])
        return ends[:i["ends"]], locs[:i["ends"]], rt[:i["records"]], dup[:i["templates"]], optical[:i["templates"]]

    def apply_records(self, records: bytes):
        """-> (the records of the next add with 0x400 set or cleared, the records marked)"""
        buf = np.frombuffer(bytes(records), np.uint8).copy()
        n = C.c_int64(0)
        self._call("bwams_dupjoin_apply_records", _p(buf), len(buf), C.byref(n))
        return buf.tobytes(), n.value

    def apply_file(self, bam_file: "BamFile") -> int:
        """Marks the BamFile's current piece where it lies; -> the records marked"""
        n = C.c_int64(0)
        self._call("bwams_dupjoin_apply_file", bam_file.h, C.byref(n))
        return n.value

    def info(self) -> dict:
        return self._info("bwams_dupjoin_info", DupJoinInfo)


class CollateOpt(C.Structure):
    _fields_ = [("pool_bytes", C.c_int64), ("key_mask", C.c_uint64), ("reserved", C.c_uint32 * 2)]


class CollateOut(C.Structure):
    _fields_ = [("pairs", C.c_void_p), ("pairs_bytes", C.c_int64), ("n_pairs", C.c_int64), ("singles", C.c_void_p),
                ("singles_bytes", C.c_int64), ("n_singles", C.c_int64)]


class CollateInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("records", "skipped", "pairs", "singles", "orphans", "pending", "pending_bytes", "pool_capacity",
                                         "bytes_pooled", "compactions", "bytes_compacted", "max_run", "adds")] + \
               [("state", C.c_int32), ("pad_", C.c_int32)] + \
               [(n, C.c_float) for n in ("ms_entry", "ms_group", "ms_match", "ms_place", "ms_copy", "pad2_")]


class Collate(_Consumer):
    """A coordinate-sorted BAM collated by read name (bwams_collate_t): add_records / add_file per piece, each followed by out() or
    fetch() for the pairs it completed and its singles; finish() leaves the orphans as the singles."""
    _close = "bwams_collate_close"
    _prefix = "bwams_collate"

    def __init__(self, device: int = 0, pool_bytes: int = 0, key_mask: int = (1 << 64) - 1, opt=True):
        self.h = C.c_void_p()
        o = CollateOpt(pool_bytes, key_mask)
        _chk(lib().bwams_collate_open(device, C.byref(o) if opt else None, C.byref(self.h)), "bwams_collate_open")

    def add_batch(self, batch: "Batch") -> int:
        raise NotImplementedError("a batch's records are grouped already")

    def finish(self) -> int:
        """-> the orphans, which out() and fetch() now give as the singles"""
        n = C.c_int64(0)
        self._call("bwams_collate_finish", C.byref(n))
        return n.value

    def out(self) -> CollateOut:
        """The output of the last add or finish in device memory: .pairs and .singles are device addresses (None when empty),
        valid until the next add, finish, reset or close.  (out.pairs, out.pairs_bytes) is what Batch.process_chunk_bam takes."""
        o = CollateOut()
        self._call("bwams_collate_out", C.byref(o))
        return o

    def fetch(self):
        """-> (pairs: bytes, pair_off: int64[2 * n_pairs + 1], singles: bytes, single_off: int64[n_singles + 1])"""
        o = self.out()
        pairs, singles = np.zeros(max(o.pairs_bytes, 1), np.uint8), np.zeros(max(o.singles_bytes, 1), np.uint8)
        poff, soff = np.zeros(2 * o.n_pairs + 1, np.int64), np.zeros(o.n_singles + 1, np.int64)
        self._call("bwams_collate_fetch", _p(pairs), o.pairs_bytes, _p(poff), _p(singles), o.singles_bytes, _p(soff))
        return pairs[:o.pairs_bytes].tobytes(), poff, singles[:o.singles_bytes].tobytes(), soff

    def info(self) -> dict:
        return self._info("bwams_collate_info", CollateInfo)


class SamViewOpt(C.Structure):
    _fields_ = [("flag_require", C.c_uint32), ("flag_exclude", C.c_uint32), ("min_mapq", C.c_int32), ("reserved", C.c_uint32)]


class SamViewOut(C.Structure):
    _fields_ = [("text", C.c_void_p), ("n_bytes", C.c_int64), ("line_off", C.c_void_p), ("n_lines", C.c_int64), ("n_records", C.c_int64)]


class SamViewInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("records", "lines", "filtered", "bytes", "adds")] + \
               [(n, C.c_float) for n in ("ms_count", "ms_write")]


class SamView(_Consumer):
    """BAM records viewed as SAM text (bwams_samview_t): add_records / add_batch / add_file (-> the lines), each followed by out(),
    fetch() or fetch_bgzf() for the lines of that add."""
    _close = "bwams_samview_close"
    _prefix = "bwams_samview"

    def __init__(self, bam_header: bytes, device: int = 0, require: int = 0, exclude: int = 0, min_mapq: int = 0, reserved: int = 0,
                 opt=True):
        self.h = C.c_void_p()
        hdr = bytes(bam_header)
        o = SamViewOpt(require, exclude, min_mapq, reserved)
        _chk(lib().bwams_samview_open(device, hdr, len(hdr), C.byref(o) if opt else None, C.byref(self.h)), "bwams_samview_open")

    def reset(self) -> None:
        raise NotImplementedError("a view keeps nothing between adds")

    def out(self) -> SamViewOut:
        """The lines of the last add in device memory: .text and .line_off are device addresses (.text None when empty), valid
        until the next add or close."""
        o = SamViewOut()
        self._call("bwams_samview_out", C.byref(o))
        return o

    def fetch(self, cap: int | None = None):
        """-> (text: bytes, line_off: int64[n_lines + 1]); cap: the capacity offered instead of the text's size"""
        o = self.out()
        text, off = np.zeros(max(o.n_bytes, 1), np.uint8), np.zeros(o.n_lines + 1, np.int64)
        self._call("bwams_samview_fetch", _p(text), o.n_bytes if cap is None else cap, _p(off))
        return text[:o.n_bytes].tobytes(), off

    def fetch_bgzf(self, deflater: "Deflater", eof: bool = False) -> bytes:
        """The lines of the last add as BGZF members, compressed on the device where they lie (bwams_samview_fetch_bgzf)."""
        cap = deflate_bound(self.out().n_bytes)
        buf = C.create_string_buffer(cap)
        n = C.c_int64(0)
        self._call("bwams_samview_fetch_bgzf", deflater.h, C.addressof(buf), cap, DEFLATE_EOF if eof else 0, C.byref(n))
        return buf.raw[:n.value]

    def info(self) -> dict:
        return self._info("bwams_samview_info", SamViewInfo)


def fmt_float(x) -> bytes:
    """Rule V5 (bwams_fmt_float): the text of a float as "%g" prints it; x is a number, or an int taken as the float's 32 bits when
    given as np.uint32.  No device is needed."""
    v = np.array([x], np.uint32).view(np.float32) if isinstance(x, np.uint32) else np.array([x], np.float32)
    buf = C.create_string_buffer(16)
    n = C.c_int32(0)
    _chk(lib().bwams_fmt_float(C.c_float.from_buffer_copy(v.tobytes()), buf, C.byref(n)), "bwams_fmt_float")
    return buf.raw[:n.value]


class Gunzipper:
    """Plain gzip inflated on one GPU (bwams_gunzip_t): one file, fed in order."""

    def __init__(self, device: int = 0, max_in_bytes: int = 32 << 20, max_out_bytes: int = 64 << 20, piece_bytes: int = 0):
        self.h = C.c_void_p()
        self.max_out = max_out_bytes
        _chk(lib().bwams_gunzip_create(device, max_in_bytes, max_out_bytes, piece_bytes, C.byref(self.h)), "bwams_gunzip_create")

    def run_raw(self, gz, last: bool, out, out_cap: int, on_device: bool):
        """bwams_gunzip_run as is: gz bytes (or (addr, n)), out an address.  Returns (rc, n_consumed, n_out, GunzipStats)."""
        used, n_out, st = C.c_int64(0), C.c_int64(0), GunzipStats()
        ptr, n = (C.c_void_p(gz[0]), gz[1]) if isinstance(gz, tuple) else (gz, len(gz))
        rc = lib().bwams_gunzip_run(self.h, ptr, n, int(last), C.c_void_p(out), out_cap, int(on_device), C.byref(used),
                                    C.byref(n_out), C.byref(st))
        return rc, used.value, n_out.value, st

    def run(self, gz: bytes, last: bool = True, out_cap: int | None = None):
        """One call with a host output (out_cap: default max_out_bytes): (text bytes, n_consumed, GunzipStats)."""
        cap = out_cap if out_cap is not None else self.max_out
        buf = C.create_string_buffer(max(cap, 1))
        rc, used, n, st = self.run_raw(gz, last, C.addressof(buf), cap, False)
        _chk(rc, "bwams_gunzip_run")
        return buf.raw[:n], used, st

    def close(self):
        if self.h:
            lib().bwams_gunzip_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def reader_open_device(path: str, device: int, chunk_bases: int, paired: bool = False, buffer_bytes: int = 0,
                       n_buffers: int = 2) -> C.c_void_p:
    """bwams_reader_open_device: a bwams_reader_t handle (bwams_reader_next / _release / _close as for bwams_reader_open)."""
    r = C.c_void_p()
    _chk(lib().bwams_reader_open_device(path.encode(), device, chunk_bases, int(paired), buffer_bytes, n_buffers, C.byref(r)),
         "bwams_reader_open_device")
    return r


READER_GUNZIP = 0x1          # BWAMS_READER_GUNZIP


def reader_open_device2(path: str, device: int, chunk_bases: int, paired: bool = False, buffer_bytes: int = 0, n_buffers: int = 2,
                        flags: int = 0) -> C.c_void_p:
    """bwams_reader_open_device2: bwams_reader_open_device with flags (READER_GUNZIP: plain gzip inflated on the device too)."""
    r = C.c_void_p()
    _chk(lib().bwams_reader_open_device2(path.encode(), device, chunk_bases, int(paired), buffer_bytes, n_buffers, flags, C.byref(r)),
         "bwams_reader_open_device2")
    return r


def bam_reads_decode(device: int, records, tags: bytes = b"", n_bytes: int | None = None) -> Fastq:
    """bwams_bam_reads_decode: BAM records (bytes, or an int device address with n_bytes) as a decoded chunk.  The Fastq also carries
    n_records (skipped records included)."""
    fq = Fastq(None)
    n, nb, nr = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    if isinstance(records, int):
        src = C.c_void_p(records)
    else:
        src, n_bytes = C.cast(C.c_char_p(records), C.c_void_p), len(records)
        fq._keep = records
    _chk(lib().bwams_bam_reads_decode(device, src, n_bytes, tags or None, C.byref(fq.h), C.byref(n), C.byref(nb), C.byref(nr)),
         "bwams_bam_reads_decode")
    fq.n_reads, fq.n_bases, fq.n_records = n.value, nb.value, nr.value
    return fq


def bam_reads_info(fq: Fastq) -> dict:
    """bwams_bam_reads_info: device ms of the record search and of what follows it, the filter's candidates, the records."""
    a, b, nc, nr = C.c_float(0), C.c_float(0), C.c_int64(0), C.c_int64(0)
    _chk(lib().bwams_bam_reads_info(fq.h, C.byref(a), C.byref(b), C.byref(nc), C.byref(nr)), "bwams_bam_reads_info")
    return dict(ms_discover=a.value, ms_emit=b.value, n_candidates=nc.value, n_records=nr.value)


def reader_open_bam(path: str, device: int, chunk_bases: int, paired: bool = False, buffer_bytes: int = 0,
                    n_buffers: int = 2) -> C.c_void_p:
    """bwams_reader_open_bam: a bwams_reader_t handle over a BAM file (device < 0: zlib); chunks of whole BAM records."""
    r = C.c_void_p()
    _chk(lib().bwams_reader_open_bam(path.encode(), device, chunk_bases, int(paired), buffer_bytes, n_buffers, C.byref(r)),
         "bwams_reader_open_bam")
    return r


def reader_bam_header(r) -> tuple[bytes, int]:
    """bwams_reader_bam_header: (header text, number of references)."""
    text, n, n_ref = C.c_void_p(), C.c_int64(0), C.c_int32(0)
    _chk(lib().bwams_reader_bam_header(r, C.byref(text), C.byref(n), C.byref(n_ref)), "bwams_reader_bam_header")
    return C.string_at(text, n.value) if n.value else b"", n_ref.value


def reader_open(path: str, chunk_bases: int, paired: bool = False, buffer_bytes: int = 0, n_buffers: int = 2) -> C.c_void_p:
    """bwams_reader_open: a bwams_reader_t handle over a gz or plain FASTQ / FASTA file."""
    r = C.c_void_p()
    _chk(lib().bwams_reader_open(path.encode(), chunk_bases, int(paired), buffer_bytes, n_buffers, C.byref(r)), "bwams_reader_open")
    return r


def reader_chunks(r):
    """Every chunk of a reader as (bytes, n_reads, n_bases), each buffer released at once; closes the reader.  A reader's error
    raises BwamsError with bwams_reader_error's text."""
    L = lib()
    out = []
    try:
        while True:
            text, nb, n, bases = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0)
            rc = L.bwams_reader_next(r, C.byref(text), C.byref(nb), C.byref(n), C.byref(bases))
            if rc == 1:
                return out
            if rc:
                raise BwamsError(rc, "bwams_reader_next", L.bwams_reader_error(r).decode())
            out.append((C.string_at(text, nb.value), n.value, bases.value))
            L.bwams_reader_release(r, text)
    finally:
        L.bwams_reader_close(r)


def reader_info(r) -> ReaderStats:
    st = ReaderStats()
    _chk(lib().bwams_reader_info(r, C.byref(st)), "bwams_reader_info")
    return st


def pestat_from_keys(keys) -> np.ndarray:
    """mem_pestat's arithmetic over the insert-size keys of a whole chunk (host only; keys in any order)."""
    keys = np.ascontiguousarray(keys, np.uint64)
    pes = np.zeros(4, PESTAT_DTYPE)
    _chk(lib().bwams_pestat_from_keys(_p(keys), len(keys), _p(pes)), "bwams_pestat_from_keys")
    return pes


def default_seed_opt() -> SeedOpt:
    """mem_opt_init defaults (/root/reference/src/bwamem.cpp:135-171)."""
    return SeedOpt(19, 1.5, 10, 20, 500)


def default_sw_opt(end_bonus: int = 5, a: int = 1, b: int = 4) -> SwOpt:
    o = SwOpt(6, 1, 6, 1, 100, end_bonus)
    k = 0
    for i in range(4):
        for j in range(4):
            o.mat[k] = a if i == j else -b
            k += 1
        o.mat[k] = -1
        k += 1
    for j in range(5):
        o.mat[k] = -1
        k += 1
    return o


def default_mem_opt(a: int = 1, b: int = 4) -> MemOpt:
    """mem_opt_init defaults (/root/reference/src/bwamem.cpp:135-171)."""
    o = MemOpt(a, 6, 1, 6, 1, 5, 5, 100, 100, 19, 0, 1 << 30, 500, 10000, 0.5, 0.5)
    o.mask_level_redun = 0.95
    o.max_ins = 10000
    o.b, o.pen_unpaired, o.max_matesw = b, 17, 50
    o.mapq_coef_len = 50
    sw = default_sw_opt(5, a, b)
    for i in range(25):
        o.mat[i] = sw.mat[i]
    return o


def build(force: bool = False) -> str:
    """Compile libbwams.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    csrc = os.path.join(PKG, "csrc")
    cmd = ["make", "-s", "-C", csrc, "-j4"]
    if force:
        subprocess.check_call(["make", "-s", "-C", csrc, "clean"])
    subprocess.check_call(cmd)
    return LIB_PATH


_lib = None


def lib():
    """Load libbwams.so (must have been built; raises if it is missing)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BwamsError(-1, "libbwams.so", f"not built: {LIB_PATH} (run __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
        L.bwams_strerror.restype = C.c_char_p
        L.bwams_strerror.argtypes = [C.c_int]
        L.bwams_last_error.restype = C.c_char_p
        L.bwams_device_count.argtypes = [vp]
        L.bwams_index_open.argtypes = [C.c_char_p, C.c_int, vp]
        L.bwams_index_from_host.argtypes = [vp, C.c_int, vp]
        L.bwams_index_from_device.argtypes = [vp, C.c_int, vp]
        L.bwams_index_close.argtypes = [vp]
        L.bwams_index_build.argtypes = [vp, i64, C.c_int, C.c_int, C.c_int, i64, vp, vp]
        L.bwams_index_fetch.argtypes = [vp, vp, vp, vp, vp, vp]
        L.bwams_index_save.argtypes = [vp, C.c_char_p]
        L.bwams_index_from_fasta.argtypes = [C.c_int, vp, i64, C.c_int, C.c_int, i64, vp, vp]
        L.bwams_index_from_fasta_file.argtypes = [C.c_char_p, C.c_int, C.c_int, i64, vp, vp]
        L.bwams_index_load_bns.argtypes = [vp, C.c_char_p]
        L.bwams_inflater_create.argtypes = [C.c_int, i64, i64, vp]
        L.bwams_inflater_run.argtypes = [vp, vp, i64, vp, i64, C.c_int, vp, vp, vp]
        L.bwams_inflater_destroy.argtypes = [vp]
        L.bwams_reader_open_device.argtypes = [C.c_char_p, C.c_int, i64, i32, i64, i32, vp]
        L.bwams_reader_info.argtypes = [vp, vp]
        L.bwams_gunzip_create.argtypes = [C.c_int, i64, i64, i32, vp]
        L.bwams_gunzip_run.argtypes = [vp, vp, i64, i32, vp, i64, C.c_int, vp, vp, vp]
        L.bwams_gunzip_destroy.argtypes = [vp]
        L.bwams_reader_open_device2.argtypes = [C.c_char_p, C.c_int, i64, i32, i64, i32, C.c_uint32, vp]
        L.bwams_reader_open.argtypes = [C.c_char_p, i64, i32, i64, i32, vp]
        L.bwams_reader_next.argtypes = [vp, vp, vp, vp, vp]
        L.bwams_reader_release.argtypes = [vp, vp]
        L.bwams_reader_error.restype = C.c_char_p
        L.bwams_reader_error.argtypes = [vp]
        L.bwams_reader_close.argtypes = [vp]
        L.bwams_reader_open_bam.argtypes = [C.c_char_p, C.c_int, i64, i32, i64, i32, vp]
        L.bwams_reader_bam_header.argtypes = [vp, vp, vp, vp]
        L.bwams_bam_reads_decode.argtypes = [C.c_int, vp, i64, C.c_char_p, vp, vp, vp, vp]
        L.bwams_bam_reads_info.argtypes = [vp, vp, vp, vp, vp]
        L.bwams_process_chunk_bam.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, C.c_char_p, i32, vp, i64, i32, vp, vp]
        L.bwams_process_chunk_bam_smart.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, C.c_char_p, vp, i64, i32, vp, vp, vp]
        L.bwams_trim_opt_default.argtypes = [vp]
        L.bwams_fastq_trim.argtypes = [vp, vp, i32, vp, vp, vp]
        L.bwams_fastq_text.argtypes = [vp, i32, vp, vp]
        L.bwams_fastq_text_fetch.argtypes = [vp, vp, i64]
        L.bwams_process_chunk_decoded.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp, i64, i32, vp, vp]
        L.bwams_deflate_bound.restype = i64
        L.bwams_deflate_bound.argtypes = [i64]
        L.bwams_deflater_create.argtypes = [C.c_int, i64, vp]
        L.bwams_deflater_run.argtypes = [vp, vp, i64, C.c_int, vp, i64, C.c_int, i32, vp, vp]
        L.bwams_deflater_destroy.argtypes = [vp]
        L.bwams_sam_fetch_bgzf.argtypes = [vp, vp, vp, i64, i32, vp]
        L.bwams_writer_open_bgzf.argtypes = [C.c_char_p, i32, C.c_int, vp]
        L.bwams_writer_put_bgzf.argtypes = [vp, i32, i64, vp, i64]
        L.bwams_bam_run.argtypes = [vp, vp, vp]
        L.bwams_bam_fetch.argtypes = [vp, vp, i64, vp]
        L.bwams_bam_fetch_bgzf.argtypes = [vp, vp, vp, i64, i32, vp]
        L.bwams_sam_header.argtypes = [vp, C.c_char_p, C.c_char_p, vp, i64, vp]
        L.bwams_bam_header.argtypes = [vp, C.c_char_p, i64, vp, i64, vp]
        L.bwams_writer_open_bam.argtypes = [C.c_char_p, i32, C.c_int, C.c_char_p, i64, vp]
        L.bwams_bam_upload.argtypes = [vp, vp, i64, vp]
        L.bwams_bam_sort.argtypes = [vp, vp]
        L.bwams_bam_sorted_fetch.argtypes = [vp, vp, i64, vp]
        L.bwams_sorter_open.argtypes = [C.c_char_p, C.c_int, vp, i64, C.c_char_p, i64, i32, vp]
        L.bwams_sorter_put.argtypes = [vp, i64, vp, i64, vp, i64]
        L.bwams_sorter_put_batch.argtypes = [vp, i64, vp]
        L.bwams_sorter_close.argtypes = [vp, vp]
        L.bwams_sorter_close2.argtypes = [vp, vp, vp]
        L.bwams_bam_templates.argtypes = [vp, vp, vp]
        L.bwams_bam_templates_fetch.argtypes = [vp, vp, i64, vp, i32]
        L.bwams_dup_decide.argtypes = [C.c_int, vp, i64, i64, vp, vp]
        L.bwams_bam_markdup.argtypes = [vp, vp]
        L.bwams_dup_groups_create.argtypes = [C.c_char_p, i64, vp]
        L.bwams_dup_groups_info.argtypes = [vp, vp, vp]
        L.bwams_dup_groups_library.argtypes = [vp, i64]
        L.bwams_dup_groups_library.restype = C.c_char_p
        L.bwams_dup_groups_destroy.argtypes = [vp]
        L.bwams_dup_groups_destroy.restype = None
        L.bwams_bam_templates2.argtypes = [vp, vp, vp, vp]
        L.bwams_bam_templates_fetch_loc.argtypes = [vp, vp, i64]
        L.bwams_bam_lib_record_counts.argtypes = [vp, vp, vp, i64]
        L.bwams_dup_decide2.argtypes = [C.c_int, vp, vp, i64, i64, i64, vp, vp, vp, vp]
        L.bwams_bam_markdup2.argtypes = [vp, vp, vp, vp, vp, i64]
        L.bwams_dup_library_size.argtypes = [i64, i64]
        L.bwams_dup_library_size.restype = i64
        L.bwams_dup_metrics_text.argtypes = [vp, vp, i64, C.c_char_p, vp, i64, vp]
        L.bwams_sorter_set_markdup.argtypes = [vp, vp, vp]
        L.bwams_sorter_close3.argtypes = [vp, vp, vp, vp, i64]
        L.bwams_depth_open.argtypes = [C.c_int, vp, i32, vp, vp]
        L.bwams_depth_close.argtypes = [vp]
        L.bwams_depth_reset.argtypes = [vp]
        L.bwams_depth_add_batch.argtypes = [vp, vp, vp]
        L.bwams_depth_add_records.argtypes = [vp, vp, i64, vp]
        L.bwams_depth_finish.argtypes = [vp]
        L.bwams_depth_summary.argtypes = [vp, vp, i64]
        L.bwams_depth_hist.argtypes = [vp, i32, vp, i32]
        L.bwams_depth_windows.argtypes = [vp, i32, vp, i64, vp]
        L.bwams_depth_runs.argtypes = [vp, i32, i32, i32, vp, vp, i64, vp]
        L.bwams_depth_fetch.argtypes = [vp, i32, i32, i32, vp]
        L.bwams_depth_text.argtypes = [vp, vp, i32, i32, vp, i64, vp]
        L.bwams_sorter_set_depth.argtypes = [vp, vp]
        L.bwams_pileup_open.argtypes = [C.c_int, vp, i32, vp, i32, vp, vp]
        L.bwams_pileup_close.argtypes = [vp]
        L.bwams_pileup_reset.argtypes = [vp]
        L.bwams_pileup_add_batch.argtypes = [vp, vp, vp]
        L.bwams_pileup_add_records.argtypes = [vp, vp, i64, vp]
        L.bwams_pileup_set_ref.argtypes = [vp, i32, vp]
        L.bwams_pileup_set_ref_index.argtypes = [vp, vp]
        L.bwams_pileup_fetch.argtypes = [vp, i32, i32, i32, vp]
        L.bwams_pileup_sites.argtypes = [vp, i32, i32, vp, i64, vp]
        L.bwams_pileup_text.argtypes = [vp, vp, i32, i32, vp, i64, vp]
        L.bwams_pileup_info.argtypes = [vp, vp]
        L.bwams_sorter_set_pileup.argtypes = [vp, vp]
        L.bwams_pileup_set_quality.argtypes = [vp, vp]
        L.bwams_pileup_fetch_quality.argtypes = [vp, i32, i32, i32, vp]
        L.bwams_pileup_calls.argtypes = [vp, i32, i32, vp, i64, vp]
        L.bwams_pileup_vcf.argtypes = [vp, vp, C.c_char_p, i32, i32, vp, i64, vp]
        L.bwams_pileup_set_indels.argtypes = [vp, vp]
        L.bwams_pileup_set_indel_leftalign.argtypes = [vp, i32]
        L.bwams_pileup_fetch_span.argtypes = [vp, i32, i32, i32, vp]
        L.bwams_pileup_indel_alleles.argtypes = [vp, vp, i64, vp]
        L.bwams_pileup_indel_calls.argtypes = [vp, i32, i32, vp, i64, vp]
        L.bwams_pileup_indel_vcf.argtypes = [vp, vp, C.c_char_p, i32, i32, vp, i64, vp]
        L.bwams_pileup_vcf_all.argtypes = [vp, vp, C.c_char_p, i32, i32, i32, i32, vp, i64, vp]
        L.bwams_pileup_indel_info.argtypes = [vp, vp]
        L.bwams_qc_open.argtypes = [C.c_int, vp, vp]
        L.bwams_qc_close.argtypes = [vp]
        L.bwams_qc_reset.argtypes = [vp]
        L.bwams_qc_add_batch.argtypes = [vp, vp, vp]
        L.bwams_qc_add_records.argtypes = [vp, vp, i64, vp]
        L.bwams_qc_summary.argtypes = [vp, vp]
        L.bwams_qc_table.argtypes = [vp, i32, vp, i64, vp]
        L.bwams_qc_text.argtypes = [vp, i32, vp, i64, vp]
        L.bwams_qc_info.argtypes = [vp, vp]
        L.bwams_sorter_set_qc.argtypes = [vp, vp]
        L.bwams_recal_open.argtypes = [C.c_int, vp, i32, vp, vp, vp]
        L.bwams_recal_close.argtypes = [vp]
        L.bwams_recal_reset.argtypes = [vp]
        L.bwams_recal_add_batch.argtypes = [vp, vp, vp]
        L.bwams_recal_add_records.argtypes = [vp, vp, i64, vp]
        L.bwams_recal_set_ref.argtypes = [vp, i32, vp]
        L.bwams_recal_set_ref_index.argtypes = [vp, vp]
        L.bwams_recal_add_known.argtypes = [vp, vp, i64]
        L.bwams_recal_table.argtypes = [vp, i32, vp, i64, vp]
        L.bwams_recal_text.argtypes = [vp, vp, vp, i64, vp]
        L.bwams_recal_info.argtypes = [vp, vp]
        L.bwams_sorter_set_recal.argtypes = [vp, vp]
        L.bwams_recal_model_create.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp]
        L.bwams_recal_model_from.argtypes = [vp, vp, vp]
        L.bwams_recal_model_table.argtypes = [vp, i32, vp, i64, vp]
        L.bwams_recal_model_constants.argtypes = [vp, vp]
        L.bwams_recal_model_destroy.argtypes = [vp]
        L.bwams_recal_apply_open.argtypes = [C.c_int, vp, vp, vp]
        L.bwams_recal_apply_close.argtypes = [vp]
        L.bwams_recal_apply_records.argtypes = [vp, vp, i64, vp]
        L.bwams_recal_apply_batch.argtypes = [vp, vp, vp]
        L.bwams_recal_apply_info.argtypes = [vp, vp]
        L.bwams_bam_file_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int, i64, vp]
        L.bwams_bam_file_header.argtypes = [vp, vp, vp, vp]
        L.bwams_bam_file_refs.argtypes = [vp, vp, i32]
        L.bwams_bam_file_query.argtypes = [vp, vp, i32]
        L.bwams_bam_file_next.argtypes = [vp, vp, vp, vp]
        L.bwams_bam_file_fetch.argtypes = [vp, vp, i64, vp]
        L.bwams_bam_file_info.argtypes = [vp, vp]
        L.bwams_bam_file_close.argtypes = [vp]
        for name in ("bwams_depth_add_file", "bwams_pileup_add_file", "bwams_qc_add_file", "bwams_recal_add_file", "bwams_recal_apply_file"):
            getattr(L, name).argtypes = [vp, vp, vp]
        L.bwams_bai_plan.argtypes = [vp, i64, vp, i32, vp, vp, i64, vp]
        L.bwams_bam_file_header_block.argtypes = [vp, vp, vp]
        L.bwams_bam_file_open_merge.argtypes = [vp, vp, i32, C.c_int, i64, vp, vp]
        L.bwams_bam_merge_info.argtypes = [vp, vp]
        L.bwams_bam_header_merge.argtypes = [vp, vp, i32, vp, i64, vp, vp]
        L.bwams_dupjoin_open.argtypes = [C.c_int, vp, vp, vp]
        L.bwams_dupjoin_reset.argtypes = [vp]
        L.bwams_dupjoin_close.argtypes = [vp]
        L.bwams_dupjoin_add_records.argtypes = [vp, vp, i64, vp]
        L.bwams_dupjoin_add_file.argtypes = [vp, vp, vp]
        L.bwams_dupjoin_finish.argtypes = [vp, vp, vp, i64]
        L.bwams_dupjoin_fetch.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp, i64]
        L.bwams_dupjoin_apply_records.argtypes = [vp, vp, i64, vp]
        L.bwams_dupjoin_apply_file.argtypes = [vp, vp, vp]
        L.bwams_dupjoin_info.argtypes = [vp, vp]
        L.bwams_dupjoin_key.argtypes = [C.c_char_p, i32, vp]
        L.bwams_collate_open.argtypes = [C.c_int, vp, vp]
        L.bwams_collate_reset.argtypes = [vp]
        L.bwams_collate_close.argtypes = [vp]
        L.bwams_collate_add_records.argtypes = [vp, vp, i64, vp]
        L.bwams_collate_add_file.argtypes = [vp, vp, vp]
        L.bwams_collate_finish.argtypes = [vp, vp]
        L.bwams_collate_out.argtypes = [vp, vp]
        L.bwams_collate_fetch.argtypes = [vp, vp, i64, vp, vp, i64, vp]
        L.bwams_collate_info.argtypes = [vp, vp]
        L.bwams_samview_open.argtypes = [C.c_int, vp, i64, vp, vp]
        L.bwams_samview_close.argtypes = [vp]
        L.bwams_samview_add_records.argtypes = [vp, vp, i64, vp]
        L.bwams_samview_add_batch.argtypes = [vp, vp, vp]
        L.bwams_samview_add_file.argtypes = [vp, vp, vp]
        L.bwams_samview_out.argtypes = [vp, vp]
        L.bwams_samview_fetch.argtypes = [vp, vp, i64, vp]
        L.bwams_samview_fetch_bgzf.argtypes = [vp, vp, vp, i64, i32, vp]
        L.bwams_samview_info.argtypes = [vp, vp]
        L.bwams_fmt_float.argtypes = [C.c_float, vp, vp]
        L.bwams_dup_groups_rg_id.argtypes = [vp, i64]
        L.bwams_dup_groups_rg_id.restype = C.c_char_p
        L.bwams_reg2aln_run.argtypes = [vp, vp, i32, vp, vp, vp]
        L.bwams_reg2aln_fetch.argtypes = [vp, vp, i64, vp, i64, vp, i64]
        L.bwams_debug_regs_upload.argtypes = [vp, vp, i64, vp, i64]
        L.bwams_debug_aln_lists.argtypes = [vp, vp]
        L.bwams_debug_ext_regs_upload.argtypes = [vp, vp, i64, vp, i64]
        L.bwams_debug_dedup_counts.argtypes = [vp, vp]
        L.bwams_debug_pair_regs_upload.argtypes = [vp, vp, i64, vp, i64]
        L.bwams_debug_pair_counts.argtypes = [vp, vp]
        L.bwams_debug_chain_counts.argtypes = [vp, vp]
        L.bwams_debug_chain_lane_counts.argtypes = [vp, vp]
        L.bwams_index_build_fma.argtypes = [vp, C.c_int, C.c_int]
        L.bwams_index_set_fma.argtypes = [vp, vp, C.c_int, vp, C.c_int]
        L.bwams_index_fetch_fma.argtypes = [vp, vp, vp]
        L.bwams_index_bytes.restype = i64
        L.bwams_index_bytes.argtypes = [vp]
        L.bwams_debug_sa_dense_state.argtypes = [vp, vp, vp, vp, vp]
        L.bwams_debug_sa_dense_fetch.argtypes = [vp, vp, i64, vp]
        L.bwams_debug_sa_dense_release.argtypes = [C.c_int, vp]
        L.bwams_batch_create.argtypes = [vp, i64, i64, i64, i64, vp]
        L.bwams_batch_destroy.argtypes = [vp]
        L.bwams_seed_fmi.argtypes = [vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, vp]
        L.bwams_seed_upload.argtypes = [vp, vp, vp, vp, i64]
        L.bwams_index_set_contigs.argtypes = [vp, vp, i32]
        L.bwams_chain_run.argtypes = [vp, vp, vp, vp]
        L.bwams_chain_fetch.argtypes = [vp, vp, i64, vp, i64, vp]
        L.bwams_chain_upload.argtypes = [vp, vp, i64, vp, i64, vp]
        L.bwams_extend_build.argtypes = [vp, vp, vp, vp]
        L.bwams_extend_run.argtypes = [vp, vp, vp]
        L.bwams_extend_fetch.argtypes = [vp, vp, i64, vp, vp]
        L.bwams_extend_tasks_fetch.argtypes = [vp, i32, vp, i64, vp, i64, vp, i64, vp, vp, vp]
        L.bwams_dedup_run.argtypes = [vp, vp, vp]
        L.bwams_dedup_fetch.argtypes = [vp, vp, i64, vp]
        L.bwams_pestat.argtypes = [vp, vp, vp]
        L.bwams_chain_run_ert.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
        L.bwams_pestat_keys.argtypes = [vp, vp, vp, C.c_int64, vp]
        L.bwams_pestat_from_keys.argtypes = [vp, C.c_int64, vp]
        L.bwams_pair_run.argtypes = [vp, vp, vp, C.c_int64, C.c_int32, vp, vp]
        L.bwams_pair_fetch.argtypes = [vp, vp, C.c_int64, vp, vp]
        L.bwams_emf_regs_run.argtypes = [vp, vp, vp, vp]
        L.bwams_emf_regs_fetch.argtypes = [vp, vp, i64, vp, vp]
        L.bwams_seed_run.argtypes = [vp, vp, C.c_int]
        L.bwams_seed_counts.argtypes = [vp, vp, vp]
        L.bwams_seed_fetch.argtypes = [vp, vp, i64, vp, i64, vp]
        L.bwams_bsw_extend.argtypes = [vp, vp, i64, vp, i64, vp, i64, i32, vp]
        L.bwams_bsw_upload.argtypes = [vp, vp, i64, vp, i64, vp, i64]
        L.bwams_bsw_run.argtypes = [vp, i32, vp]
        L.bwams_bsw_fetch.argtypes = [vp, vp, i64]
        L.bwams_ksw_align.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, vp]
        L.bwams_emf_open.argtypes = [vp, C.c_char_p, vp]
        L.bwams_emf_from_host.argtypes = [vp, i32, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp]
        L.bwams_emf_close.argtypes = [vp]
        L.bwams_emf_from_device.argtypes = [vp, i32, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp]
        L.bwams_emf_run.argtypes = [vp, vp]
        L.bwams_emf_fetch.argtypes = [vp, vp, vp]
        L.bwams_emf_probe.argtypes = [vp, vp, vp, vp, i64, vp, vp]
        L.bwams_ert_from_host.argtypes = [vp, vp, i32, i32, i32, vp, i64, vp]
        L.bwams_ert_open.argtypes = [vp, C.c_char_p, i32, vp]
        L.bwams_ert_close.argtypes = [vp]
        L.bwams_ert_bytes.restype = i64
        L.bwams_ert_bytes.argtypes = [vp]
        L.bwams_seed_run_ert.argtypes = [vp, vp, vp, C.c_int]
        L.bwams_ert_build.argtypes = [vp, i32, i32, i32, i32, vp]
        L.bwams_ert_info.argtypes = [vp, vp, vp, vp, vp, vp]
        L.bwams_ert_fetch.argtypes = [vp, vp, vp]
        L.bwams_ert_save.argtypes = [vp, C.c_char_p]
        L.bwams_debug_sort.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
        L.bwams_emf_build.argtypes = [vp, i32, C.c_double, vp]
        L.bwams_emf_info.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.bwams_emf_table_fetch.argtypes = [vp, vp, vp]
        L.bwams_emf_save.argtypes = [vp, C.c_char_p]
        L.bwams_batch_stats.argtypes = [vp, vp]
        L.bwams_batch_sync.argtypes = [vp]
        _lib = L
    return _lib


def _chk(rc: int, where: str):
    if rc != 0:
        L = lib()
        raise BwamsError(rc, where, f"({L.bwams_strerror(rc).decode()}) {L.bwams_last_error().decode()}")


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Index:
    """FM-index resident in one GPU's HBM."""

    def __init__(self, handle, keep=None):
        self.h = handle
        self._keep = keep

    @classmethod
    def open(cls, prefix: str, device: int = 0) -> "Index":
        h = C.c_void_p()
        _chk(lib().bwams_index_open(prefix.encode(), device, C.byref(h)), "bwams_index_open")
        return cls(h)

    @classmethod
    def from_host(cls, idx, device: int = 0) -> "Index":
        """idx: bwams.fmindex.FMIndex of numpy arrays."""
        cp = np.ascontiguousarray(idx.cp_occ)
        ms = np.ascontiguousarray(idx.sa_ms_byte)
        ls = np.ascontiguousarray(idx.sa_ls_word)
        ref = np.ascontiguousarray(idx.ref_0123) if idx.ref_0123 is not None else None
        d = FmiDesc(int(idx.ref_seq_len), (C.c_int64 * 5)(*[int(x) for x in idx.count]),
                    cp.ctypes.data, ms.ctypes.data, ls.ctypes.data, int(idx.sentinel_index),
                    ref.ctypes.data if ref is not None else None)
        h = C.c_void_p()
        _chk(lib().bwams_index_from_host(C.byref(d), device, C.byref(h)), "bwams_index_from_host")
        return cls(h)

    @classmethod
    def from_device(cls, idx, device: int = 0) -> "Index":
        """idx: FMIndex whose arrays are torch tensors on `device` (kept alive here)."""
        ref = idx.ref_0123
        d = FmiDesc(int(idx.ref_seq_len), (C.c_int64 * 5)(*[int(x) for x in idx.count]),
                    idx.cp_occ.data_ptr(), idx.sa_ms_byte.data_ptr(), idx.sa_ls_word.data_ptr(),
                    int(idx.sentinel_index), ref.data_ptr() if ref is not None else None)
        h = C.c_void_p()
        _chk(lib().bwams_index_from_device(C.byref(d), device, C.byref(h)), "bwams_index_from_device")
        return cls(h, keep=idx)

    @classmethod
    def build(cls, genome, device: int = 0, keep_ref: bool = True, chunk_rows: int = 0) -> "Index":
        """FM-index of fw || revcomp(fw) built on the GPU (bwams_index_build).  genome: numpy uint8 codes 0..3, or a torch
        uint8 tensor already on `device`."""
        h = C.c_void_p()
        st = BuildStats()
        if isinstance(genome, np.ndarray):
            g = np.ascontiguousarray(genome, dtype=np.uint8)
            _chk(lib().bwams_index_build(_p(g), len(g), 0, device, int(keep_ref), chunk_rows, C.byref(st), C.byref(h)), "bwams_index_build")
        else:
            g = genome.contiguous()
            _chk(lib().bwams_index_build(g.data_ptr(), g.numel(), 1, device, int(keep_ref), chunk_rows, C.byref(st), C.byref(h)),
                 "bwams_index_build")
        ix = cls(h)
        ix.build_stats = st
        return ix

    @classmethod
    def from_fasta(cls, text, device: int = 0, keep_ref: bool = True, chunk_rows: int = 0) -> "Index":
        """bns_fasta2bntseq + the FM-index build on the GPU (bwams_index_from_fasta).  text: FASTA bytes, or a torch uint8 tensor
        already on `device`.  The handle carries its contigs, names and annotations and writes .ann / .amb / .pac on save."""
        h = C.c_void_p()
        st = FastaStats()
        if isinstance(text, (bytes, bytearray, memoryview)):
            t = bytes(text)
            _chk(lib().bwams_index_from_fasta(device, t, len(t), 0, int(keep_ref), chunk_rows, C.byref(st), C.byref(h)),
                 "bwams_index_from_fasta")
        else:
            t = text.contiguous()
            _chk(lib().bwams_index_from_fasta(device, t.data_ptr(), t.numel(), 1, int(keep_ref), chunk_rows, C.byref(st), C.byref(h)),
                 "bwams_index_from_fasta")
        ix = cls(h)
        ix.fasta_stats = st
        return ix

    @classmethod
    def from_fasta_file(cls, path: str, device: int = 0, keep_ref: bool = True, chunk_rows: int = 0) -> "Index":
        """The same from a plain or gzip FASTA file (bwams_index_from_fasta_file)."""
        h = C.c_void_p()
        st = FastaStats()
        _chk(lib().bwams_index_from_fasta_file(path.encode(), device, int(keep_ref), chunk_rows, C.byref(st), C.byref(h)),
             "bwams_index_from_fasta_file")
        ix = cls(h)
        ix.fasta_stats = st
        return ix

    def load_bns(self, prefix: str):
        """bns_restore onto this handle: contigs (with .alt flags), names and annotations from <prefix>.ann / .amb / .alt."""
        _chk(lib().bwams_index_load_bns(self.h, prefix.encode()), "bwams_index_load_bns")

    def fetch(self, with_ref: bool = True):
        """The resident arrays as a bwams.fmindex.FMIndex of numpy arrays (for the file writer / the CPU oracle)."""
        from bwams import fmindex
        d = FmiDesc()
        _chk(lib().bwams_index_fetch(self.h, None, None, None, None, C.byref(d)), "bwams_index_fetch")
        L = int(d.ref_seq_len)
        cp = np.empty(((L >> 6) + 1, 8), dtype=np.uint64)
        ms = np.empty((L >> 3) + 1, dtype=np.int8)
        ls = np.empty((L >> 3) + 1, dtype=np.uint32)
        ref = np.empty(L - 1, dtype=np.uint8) if with_ref else None
        _chk(lib().bwams_index_fetch(self.h, _p(cp), _p(ms), _p(ls), _p(ref), C.byref(d)), "bwams_index_fetch")
        return fmindex.FMIndex(L, np.array(list(d.count), dtype=np.int64), cp, ms, ls, int(d.sentinel_index), ref)

    def save(self, prefix: str):
        _chk(lib().bwams_index_save(self.h, prefix.encode()), "bwams_index_save")

    def build_fma(self, all_bp: int = 11, last_bp: int = 13):
        _chk(lib().bwams_index_build_fma(self.h, all_bp, last_bp), "bwams_index_build_fma")
        self._fma = (all_bp, last_bp)

    def set_fma(self, all_tab, all_bp, last_tab, last_bp):
        if all_tab is None:
            _chk(lib().bwams_index_set_fma(self.h, None, 0, None, 0), "bwams_index_set_fma")
            return
        a = np.ascontiguousarray(all_tab); l = np.ascontiguousarray(last_tab)
        _chk(lib().bwams_index_set_fma(self.h, _p(a), all_bp, _p(l), last_bp), "bwams_index_set_fma")
        self._fma = (all_bp, last_bp)

    def fetch_fma(self):
        all_bp, last_bp = self._fma
        a = np.zeros((4 ** all_bp, 32), dtype=np.uint32)
        l = np.zeros((4 ** last_bp, 4), dtype=np.uint32)
        _chk(lib().bwams_index_fetch_fma(self.h, _p(a), _p(l)), "bwams_index_fetch_fma")
        return a, l

    def set_contigs(self, contigs):
        c = np.ascontiguousarray(contigs, dtype=CONTIG_DTYPE)
        _chk(lib().bwams_index_set_contigs(self.h, _p(c), len(c)), "bwams_index_set_contigs")

    def set_contig_names(self, names):
        """Sequence names for the SAM text (list of bytes / str, one per sequence set with set_contigs)."""
        blob, off = bytearray(), []
        for nm in names:
            off.append(len(blob))
            blob += (nm if isinstance(nm, bytes) else nm.encode()) + b"\0"
        off.append(len(blob))
        off = np.asarray(off, np.int32)
        _chk(lib().bwams_index_set_contig_names(self.h, bytes(blob), _p(off)), "bwams_index_set_contig_names")

    def _header(self, fn, name, *args) -> bytes:
        n = C.c_int64(0)
        rc = fn(self.h, *args, None, 0, C.byref(n))
        if rc != -4:                                       # BWAMS_ERR_CAPACITY gives the size
            _chk(rc, name)
        buf = C.create_string_buffer(max(n.value, 1))
        _chk(fn(self.h, *args, buf, n.value, C.byref(n)), name)
        return buf.raw[:n.value]

    def sam_header(self, hdr_line=None, pg_line=None) -> bytes:
        """bwa_print_sam_hdr as bytes (bwams_sam_header): @SQ lines (unless hdr_line has its own), hdr_line + newline, pg_line."""
        enc = lambda x: x.encode() if isinstance(x, str) else x
        return self._header(lib().bwams_sam_header, "bwams_sam_header", enc(hdr_line), enc(pg_line))

    def bam_header(self, text: bytes) -> bytes:
        """The BAM header block of `text` and the index's sequences (bwams_bam_header)."""
        return self._header(lib().bwams_bam_header, "bwams_bam_header", bytes(text), len(text))

    def set_contig_annos(self, annos):
        """bntann1_t.anno of every sequence (b"" = none): the XR:Z: tags of MEM_F_REF_HDR (0x100)."""
        blob, off = bytearray(), []
        for a in annos:
            off.append(len(blob))
            blob += (a if isinstance(a, bytes) else a.encode()) + b"\0"
        off.append(len(blob))
        off = np.asarray(off, np.int32)
        _chk(lib().bwams_index_set_contig_annos(self.h, bytes(blob), _p(off)), "bwams_index_set_contig_annos")

    def debug_sort(self, k, s, q, which: int, mode: int = 0):
        """order of a device sort (test hook).  which 0, 1: the region sorts of the de-duplication's wave tier (keys k, s, q);
        2: the chain filter's (k = weight in [0, 2^30), descending; s and q ignored).  mode: see bwams.h"""
        k = np.ascontiguousarray(k, np.int64); s = np.ascontiguousarray(s, np.int32); q = np.ascontiguousarray(q, np.int32)
        out = np.zeros(len(k), np.int32)
        _chk(lib().bwams_debug_sort(self.h, _p(k), _p(s), _p(q), len(k), which, mode, _p(out)), "bwams_debug_sort")
        return out

    @property
    def nbytes(self) -> int:
        return lib().bwams_index_bytes(self.h)

    def sa_dense_state(self):
        """(state, stride, bytes, build_ms) of the dense suffix-array table; state as SA_DENSE_STATES names it (test hook)"""
        st, sr, nb, ms = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_float(0)
        _chk(lib().bwams_debug_sa_dense_state(self.h, C.byref(st), C.byref(sr), C.byref(nb), C.byref(ms)), "bwams_debug_sa_dense_state")
        return SA_DENSE_STATES[st.value], sr.value, nb.value, ms.value

    def sa_dense_fetch(self) -> np.ndarray:
        """the dense suffix-array table as uint64 entries: coordinate | sentinel << 40 | steps << 41 (test hook; small indexes)"""
        n = C.c_int64(0)
        _chk(lib().bwams_debug_sa_dense_fetch(self.h, None, 0, C.byref(n)), "bwams_debug_sa_dense_fetch")
        out = np.zeros(n.value, np.uint64)
        _chk(lib().bwams_debug_sa_dense_fetch(self.h, _p(out), len(out), C.byref(n)), "bwams_debug_sa_dense_fetch")
        return out

    def close(self):
        if self.h:
            lib().bwams_index_close(self.h)
            self.h = None


SA_DENSE_STATES = ("absent", "built", "refused", "yielded")


def sa_dense_release(device: int = 0) -> int:
    """what the library's allocator does when `device` is out of memory: every dense suffix-array table there is released (test hook)"""
    n = C.c_int32(0)
    _chk(lib().bwams_debug_sa_dense_release(device, C.byref(n)), "bwams_debug_sa_dense_release")
    return n.value


class Emf:
    """EMF table resident in HBM (bwams.emf.EmfTable or a <prefix>.perfect.<L> file)."""

    def __init__(self, index: Index, table=None, path: str | None = None, device_table=None):
        self.index = index
        self.h = C.c_void_p()
        self._keep = device_table
        if device_table is not None:          # EmfTable of torch tensors on the index's GPU
            t = device_table
            _chk(lib().bwams_emf_from_device(index.h, t.seed_len, t.seq_len, t.loc_table.data_ptr(), t.loc_table.numel(),
                                             t.seed_table.data_ptr(), t.seed_table.shape[0], C.byref(self.h)),
                 "bwams_emf_from_device")
        elif path is not None:
            _chk(lib().bwams_emf_open(index.h, path.encode(), C.byref(self.h)), "bwams_emf_open")
        else:
            loc = np.ascontiguousarray(table.loc_table, dtype=np.uint32)
            seeds = np.ascontiguousarray(table.seed_table, dtype=np.uint32)
            _chk(lib().bwams_emf_from_host(index.h, table.seed_len, table.seq_len, _p(loc), len(loc), _p(seeds),
                                           len(seeds), C.byref(self.h)), "bwams_emf_from_host")

    @classmethod
    def build(cls, index: Index, seed_len: int = 150, slack: float = 1.1) -> "Emf":
        """bwams_emf_build: the table from the resident forward reference, on the GPU"""
        self = cls.__new__(cls)
        self.index = index
        self._keep = None
        self.h = C.c_void_p()
        _chk(lib().bwams_emf_build(index.h, seed_len, slack, C.byref(self.h)), "bwams_emf_build")
        return self

    def info(self):
        sl, ne, nl = C.c_int32(0), C.c_uint32(0), C.c_uint32(0)
        nu, nk, ms = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _chk(lib().bwams_emf_info(self.h, C.byref(sl), C.byref(ne), C.byref(nl), C.byref(nu), C.byref(nk), C.byref(ms)), "bwams_emf_info")
        return {"seed_len": sl.value, "num_seed_entry": ne.value, "num_loc_entry": nl.value, "n_used": nu.value, "n_key": nk.value,
                "build_ms": ms.value}

    def fetch_table(self):
        i = self.info()
        loc = np.zeros(max(i["num_loc_entry"], 1), dtype=np.uint32)
        seeds = np.zeros((i["num_seed_entry"], 4), dtype=np.uint32)
        _chk(lib().bwams_emf_table_fetch(self.h, _p(loc), _p(seeds)), "bwams_emf_table_fetch")
        return loc[:i["num_loc_entry"]], seeds

    def save(self, path: str):
        _chk(lib().bwams_emf_save(self.h, path.encode()), "bwams_emf_save")

    def close(self):
        if self.h:
            lib().bwams_emf_close(self.h)
            self.h = None


class Ert:
    """ERT index resident in HBM: the reference's <prefix>.kmer_table / <prefix>.mlt_table, from files or host arrays."""

    def __init__(self, index: Index, kmer_table=None, mlt_table=None, kmer: int = 15, xmer: int = 4, read_len: int = 151,
                 prefix: str | None = None):
        self.index = index
        self.h = C.c_void_p()
        if prefix is not None:
            _chk(lib().bwams_ert_open(index.h, prefix.encode(), read_len, C.byref(self.h)), "bwams_ert_open")
        else:
            kt = np.ascontiguousarray(kmer_table, dtype=np.uint64)
            mt = np.ascontiguousarray(mlt_table, dtype=np.uint8)
            assert len(kt) == 4 ** kmer
            _chk(lib().bwams_ert_from_host(index.h, _p(kt), kmer, xmer, read_len, _p(mt), len(mt), C.byref(self.h)),
                 "bwams_ert_from_host")

    @classmethod
    def build(cls, index: Index, kmer: int = 15, xmer: int = 4, read_len: int = 151, hit_threshold: int = 256) -> "Ert":
        """bwams_ert_build: the tables from the resident FM-index, on the GPU"""
        self = cls.__new__(cls)
        self.index = index
        self.h = C.c_void_p()
        _chk(lib().bwams_ert_build(index.h, kmer, xmer, read_len, hit_threshold, C.byref(self.h)), "bwams_ert_build")
        return self

    def info(self):
        k, x, rl, nb = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0)
        ms = (C.c_float * 3)()
        _chk(lib().bwams_ert_info(self.h, C.byref(k), C.byref(x), C.byref(rl), C.byref(nb), ms), "bwams_ert_info")
        return {"kmer": k.value, "xmer": x.value, "read_len": rl.value, "mlt_bytes": nb.value, "build_ms": list(ms)}

    def fetch(self, pad: int = 0):
        """-> (kmer_table, mlt_table); with pad the returned tree array is a view of a buffer `pad` bytes longer (a host
        reader that loads 5- / 8-byte fields near the end needs no copy of a 48 GB array to be safe)"""
        i = self.info()
        kt = np.zeros(4 ** i["kmer"], dtype=np.uint64)
        mt = np.zeros(max(i["mlt_bytes"], 1) + pad, dtype=np.uint8)
        _chk(lib().bwams_ert_fetch(self.h, _p(kt), _p(mt)), "bwams_ert_fetch")
        return kt, mt[:i["mlt_bytes"]]

    def save(self, prefix: str):
        _chk(lib().bwams_ert_save(self.h, prefix.encode()), "bwams_ert_save")

    def nbytes(self) -> int:
        return int(lib().bwams_ert_bytes(self.h))

    def set_fat(self, on: bool):
        """keep (derive again) or give back the walk's resident entry + tree-head table (bwams_ert_set_fat)"""
        _chk(lib().bwams_ert_set_fat(self.h, 1 if on else 0), "bwams_ert_set_fat")

    def close(self):
        if self.h:
            lib().bwams_ert_close(self.h)
            self.h = None


class Batch:
    def __init__(self, index: Index, max_reads: int, max_bases: int, max_smem: int = 0, max_sa: int = 0):
        self.index = index
        self.h = C.c_void_p()
        _chk(lib().bwams_batch_create(index.h, max_reads, max_bases, max_smem, max_sa, C.byref(self.h)),
             "bwams_batch_create")
        self.max_reads = max_reads
        self.max_smem = max_smem if max_smem > 0 else 24 * max_reads + 1024
        self.max_sa = max_sa if max_sa > 0 else 64 * max_reads + 1024

    def seed(self, enc, cum, opt: SeedOpt | None = None, skip=None, with_sa: bool = True):
        """Seeding on host buffers: (smems, sa_coord, sa_off).  Upload, run, then download into arrays of
        exactly the produced size (the one-call C entry point needs caller buffers of capacity size)."""
        opt = opt or default_seed_opt()
        self.seed_upload(enc, cum, skip)
        self.seed_run(opt, with_sa)
        sm, coord, off = self.seed_fetch()
        if with_sa:
            return sm, coord, off
        return sm, None, None

    def seed_onecall(self, enc, cum, opt: SeedOpt | None = None, skip=None, with_sa: bool = True):
        """bwams_seed_fmi with capacity-sized caller buffers (what a reference-side caller does)."""
        opt = opt or default_seed_opt()
        enc = np.ascontiguousarray(enc, dtype=np.uint8)
        cum = np.ascontiguousarray(cum, dtype=np.int64)
        sk = np.ascontiguousarray(skip, dtype=np.uint8) if skip is not None else None
        nseq = len(cum) - 1
        sm = np.empty(self.max_smem, dtype=SMEM_DTYPE)
        ns, na = C.c_int64(0), C.c_int64(0)
        coord = np.empty(self.max_sa, dtype=np.int64) if with_sa else None
        off = np.empty(self.max_smem + 1, dtype=np.int64) if with_sa else None
        _chk(lib().bwams_seed_fmi(self.h, _p(enc), _p(cum), _p(sk), nseq, C.byref(opt), _p(sm), self.max_smem,
                                  C.byref(ns), _p(coord), self.max_sa, _p(off), C.byref(na)), "bwams_seed_fmi")
        n = ns.value
        if with_sa:
            return sm[:n].copy(), coord[:na.value].copy(), off[:n + 1].copy()
        return sm[:n].copy(), None, None

    # resident form
    def seed_upload(self, enc, cum, skip=None):
        enc = np.ascontiguousarray(enc, dtype=np.uint8)
        cum = np.ascontiguousarray(cum, dtype=np.int64)
        sk = np.ascontiguousarray(skip, dtype=np.uint8) if skip is not None else None
        _chk(lib().bwams_seed_upload(self.h, _p(enc), _p(cum), _p(sk), len(cum) - 1), "bwams_seed_upload")
        self._nseq = len(cum) - 1

    def seed_upload_device(self, enc_ptr: int, cum, skip=None):
        """Same, with the read bytes already in this GPU's memory (enc_ptr = device address of the chunk's first base)."""
        cum = np.ascontiguousarray(cum, dtype=np.int64)
        sk = np.ascontiguousarray(skip, dtype=np.uint8) if skip is not None else None
        _chk(lib().bwams_seed_upload(self.h, C.c_void_p(enc_ptr), _p(cum), _p(sk), len(cum) - 1), "bwams_seed_upload")
        self._nseq = len(cum) - 1

    def seed_run(self, opt: SeedOpt | None = None, with_sa: bool = True):
        opt = opt or default_seed_opt()
        _chk(lib().bwams_seed_run(self.h, C.byref(opt), 1 if with_sa else 0), "bwams_seed_run")

    def seed_run_ert(self, ert: "Ert", opt: SeedOpt | None = None, with_sa: bool = True):
        """Seeding over the ERT: same outputs as seed_run (seed_fetch, chain_run follow unchanged)."""
        opt = opt or default_seed_opt()
        _chk(lib().bwams_seed_run_ert(self.h, ert.h, C.byref(opt), 1 if with_sa else 0), "bwams_seed_run_ert")

    def seed_counts(self):
        ns, na = C.c_int64(0), C.c_int64(0)
        _chk(lib().bwams_seed_counts(self.h, C.byref(ns), C.byref(na)), "bwams_seed_counts")
        return ns.value, na.value

    def seed_fetch(self):
        ns, na = self.seed_counts()
        sm = np.zeros(max(ns, 1), dtype=SMEM_DTYPE)
        coord = np.zeros(max(na, 1), dtype=np.int64)
        off = np.zeros(ns + 1, dtype=np.int64)
        _chk(lib().bwams_seed_fetch(self.h, _p(sm), len(sm), _p(coord), len(coord), _p(off)), "bwams_seed_fetch")
        return sm[:ns], coord[:na], off

    def bsw(self, pairs, ref, qer, w: int, opt: SwOpt | None = None):
        opt = opt or default_sw_opt()
        p = np.ascontiguousarray(pairs).copy()
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        qer = np.ascontiguousarray(qer, dtype=np.uint8)
        _chk(lib().bwams_bsw_extend(self.h, _p(p), len(p), _p(ref), len(ref), _p(qer), len(qer), w, C.byref(opt)),
             "bwams_bsw_extend")
        return p

    def bsw_upload(self, pairs, ref, qer):
        p = np.ascontiguousarray(pairs)
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        qer = np.ascontiguousarray(qer, dtype=np.uint8)
        _chk(lib().bwams_bsw_upload(self.h, _p(p), len(p), _p(ref), len(ref), _p(qer), len(qer)), "bwams_bsw_upload")
        self._n_pairs = len(p)

    def bsw_run(self, w: int, opt: SwOpt | None = None):
        opt = opt or default_sw_opt()
        _chk(lib().bwams_bsw_run(self.h, w, C.byref(opt)), "bwams_bsw_run")

    def bsw_fetch(self):
        p = np.zeros(self._n_pairs, dtype=SEQPAIR_DTYPE)
        _chk(lib().bwams_bsw_fetch(self.h, _p(p), len(p)), "bwams_bsw_fetch")
        return p

    def chain_run(self, opt: MemOpt | None = None):
        """mem_chain_seeds + mem_chain_flt over the resident seeds -> (n_chains, n_seeds)."""
        opt = opt or default_mem_opt()
        nc, ns = C.c_int64(0), C.c_int64(0)
        _chk(lib().bwams_chain_run(self.h, C.byref(opt), C.byref(nc), C.byref(ns)), "bwams_chain_run")
        self._n_chain = (nc.value, ns.value)
        return self._n_chain

    def chain_fetch(self):
        nc, ns = self._n_chain
        chains = np.zeros(nc, CHAIN_DTYPE)
        seeds = np.zeros(ns, CHAIN_SEED_DTYPE)
        off = np.zeros(self._nseq + 1, np.int64)
        _chk(lib().bwams_chain_fetch(self.h, _p(chains), nc, _p(seeds), ns, _p(off)), "bwams_chain_fetch")
        return chains, seeds, off

    def chain_upload(self, chains, seeds, chain_off):
        chains = np.ascontiguousarray(chains, dtype=CHAIN_DTYPE)
        seeds = np.ascontiguousarray(seeds, dtype=CHAIN_SEED_DTYPE)
        chain_off = np.ascontiguousarray(chain_off, np.int64)
        _chk(lib().bwams_chain_upload(self.h, _p(chains), len(chains), _p(seeds), len(seeds), _p(chain_off)),
             "bwams_chain_upload")
        self._n_chain = (len(chains), len(seeds))

    def extend_build(self, opt: MemOpt | None = None):
        opt = opt or default_mem_opt()
        nl, nr = C.c_int64(0), C.c_int64(0)
        _chk(lib().bwams_extend_build(self.h, C.byref(opt), C.byref(nl), C.byref(nr)), "bwams_extend_build")
        return nl.value, nr.value

    def extend_run(self, opt: MemOpt | None = None) -> int:
        opt = opt or default_mem_opt()
        n = C.c_int64(0)
        _chk(lib().bwams_extend_run(self.h, C.byref(opt), C.byref(n)), "bwams_extend_run")
        return n.value

    def extend_fetch(self):
        """-> (regs, reg_off, seed_aln)"""
        n = self._n_chain[1]
        regs = np.zeros(n, ALNREG_DTYPE)
        off = np.zeros(self._nseq + 1, np.int64)
        aln = np.zeros(n, np.int32)
        _chk(lib().bwams_extend_fetch(self.h, _p(regs), n, _p(off), _p(aln)), "bwams_extend_fetch")
        return regs, off, aln

    def dedup_run(self, opt: MemOpt | None = None) -> int:
        """The tail of mem_kernel2_core (mem_sort_dedup_patch ...) over the regions of extend_run."""
        opt = opt or default_mem_opt()
        n = C.c_int64(0)
        _chk(lib().bwams_dedup_run(self.h, C.byref(opt), C.byref(n)), "bwams_dedup_run")
        self._n_final = n.value
        return n.value

    def dedup_fetch(self):
        regs = np.zeros(self._n_final, ALNREG_DTYPE)
        off = np.zeros(self._nseq + 1, np.int64)
        _chk(lib().bwams_dedup_fetch(self.h, _p(regs), self._n_final, _p(off)), "bwams_dedup_fetch")
        return regs, off

    def emf_regs(self, emf: "Emf", opt: MemOpt | None = None):
        """mem_perfect2reg for the reads the last emf_run resolved -> (regs, reg_off, first_is_rev)."""
        opt = opt or default_mem_opt()
        n = C.c_int64(0)
        _chk(lib().bwams_emf_regs_run(self.h, emf.h, C.byref(opt), C.byref(n)), "bwams_emf_regs_run")
        regs = np.zeros(n.value, ALNREG_DTYPE)
        off = np.zeros(self._nseq + 1, np.int64)
        rev = np.zeros(self._nseq, np.uint8)
        _chk(lib().bwams_emf_regs_fetch(self.h, _p(regs), n.value, _p(off), _p(rev)), "bwams_emf_regs_fetch")
        return regs, off, rev

    def pestat(self, opt: MemOpt | None = None):
        """mem_pestat over the final regions (reads 2i, 2i+1 = pair i) -> 4 records FF, FR, RF, RR."""
        opt = opt or default_mem_opt()
        pes = np.zeros(4, PESTAT_DTYPE)
        _chk(lib().bwams_pestat(self.h, C.byref(opt), _p(pes)), "bwams_pestat")
        return pes

    def chain_run_ert(self, mems, mem_off, hits, hit_off, opt: MemOpt | None = None):
        """ERT mode: chain the MEMs / hits of the reference's ERT walk (reads uploaded with seed_upload)
        -> (chains, chain seeds)."""
        opt = opt or default_mem_opt()
        mems = np.ascontiguousarray(mems, ERT_MEM_DTYPE)
        mem_off = np.ascontiguousarray(mem_off, np.int64)
        hits = np.ascontiguousarray(hits, np.uint64)
        hit_off = np.ascontiguousarray(hit_off, np.int64)
        nc, ns = C.c_int64(0), C.c_int64(0)
        _chk(lib().bwams_chain_run_ert(self.h, C.byref(opt), _p(mems), _p(mem_off), _p(hits), _p(hit_off), C.byref(nc), C.byref(ns)),
             "bwams_chain_run_ert")
        self._n_chain = (nc.value, ns.value)
        return self._n_chain

    def reg2aln(self, opt: MemOpt | None = None, source: int = 0):
        """mem_reg2aln over the final regions (source 0: after dedup_run; 1: after pair_run): (records, CIGAR pool, MD pool)."""
        opt = opt or default_mem_opt()
        n, nc, nm = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _chk(lib().bwams_reg2aln_run(self.h, C.byref(opt), source, C.byref(n), C.byref(nc), C.byref(nm)), "bwams_reg2aln_run")
        aln = np.zeros(max(n.value, 1), ALN_DTYPE)
        cig = np.zeros(max(nc.value, 1), np.uint32)
        md = np.zeros(max(nm.value, 1), np.uint8)
        _chk(lib().bwams_reg2aln_fetch(self.h, _p(aln), len(aln), _p(cig), len(cig), _p(md), len(md)), "bwams_reg2aln_fetch")
        return aln[:n.value], cig[:nc.value], md[:nm.value]

    def debug_regs_upload(self, regs, reg_off):
        """Test hook: regs (ALNREG_DTYPE, grouped by read through reg_off) become the final regions reg2aln(opt, 0) runs on."""
        regs = np.ascontiguousarray(regs, ALNREG_DTYPE)
        reg_off = np.ascontiguousarray(reg_off, np.int64)
        _chk(lib().bwams_debug_regs_upload(self.h, _p(regs), len(regs), _p(reg_off), len(reg_off) - 1), "bwams_debug_regs_upload")
        self._n_final = len(regs)

    PAIR_COUNTS = ("post_lane", "post_wave", "post_one_lane", "post_ert", "sort_rank", "sort_net", "sort_intro", "inserted", "mark_lane",
                   "mark_wave256", "mark_wave2048", "mark_one_lane", "mark_rank", "mark_net", "post_second")

    def debug_pair_regs_upload(self, regs, reg_off):
        """Test hook: debug_regs_upload for the pairing stage (pair_run, mark_primary_se, pair_fetch run on these regions); refuses
        also a rid outside the sequences, a reference span that is empty or outside the text, a negative score."""
        regs = np.ascontiguousarray(regs, ALNREG_DTYPE)
        reg_off = np.ascontiguousarray(reg_off, np.int64)
        _chk(lib().bwams_debug_pair_regs_upload(self.h, _p(regs), len(regs), _p(reg_off), len(reg_off) - 1), "bwams_debug_pair_regs_upload")
        self._n_final = len(regs)

    def debug_pair_counts(self):
        """Test hook: what the last pair_run / mark_primary_se under BWAMS_PAIR_COUNT=1 did, as a dict over PAIR_COUNTS (visits per
        rescue route, sorts per path, regions inserted, reads per marking route; include/bwams.h)."""
        cnt = np.zeros(len(self.PAIR_COUNTS), np.int64)
        _chk(lib().bwams_debug_pair_counts(self.h, _p(cnt)), "bwams_debug_pair_counts")
        return dict(zip(self.PAIR_COUNTS, cnt.tolist()))

    CHAIN_COUNTS = ("gt_L", "gt_L1", "gt_M", "gt_M1", "gt_S", "gt_lane", "gt_XL", "gt_L2", "gt_M2", "gt_XL2", "n_heavy", "redo",
                    "flt32", "flt64", "flt128", "flt256", "flt512", "flt960", "flt_more", "flt_seq", "in_wave", "lane_seq", "passes", "pass_seeds",
                    "pass_new", "one_by_one")

    def debug_chain_counts(self):
        """Test hook: the routes of the last chain_run / chain_run_ert as a dict over CHAIN_COUNTS (reads beyond each seed-count
        limit, many-chain and redo reads, the wave filter's size histogram; under BWAMS_CHAIN_COUNT=1 also the in-wave and
        one-lane filter routes and the pass counters, -1 otherwise; include/bwams.h)."""
        cnt = np.zeros(len(self.CHAIN_COUNTS), np.int64)
        _chk(lib().bwams_debug_chain_counts(self.h, _p(cnt)), "bwams_debug_chain_counts")
        return dict(zip(self.CHAIN_COUNTS, cnt.tolist()))

    def debug_chain_lane_counts(self):
        """Test hook: (reads of the lane tier, those among them that gave the leaf form up) of the last chain_run /
        chain_run_ert (include/bwams.h)."""
        cnt = np.zeros(2, np.int64)
        _chk(lib().bwams_debug_chain_lane_counts(self.h, _p(cnt)), "bwams_debug_chain_lane_counts")
        return int(cnt[0]), int(cnt[1])

    DEDUP_COUNTS = ("triage", "lane", "wave128", "wave512", "wave2048", "one_lane", "shortcut", "hbm", "lds", "reg1", "reg2", "reg3", "reg4", "early")

    def debug_ext_regs_upload(self, regs, reg_off):
        """Test hook: regs (ALNREG_DTYPE, a read's slots grouped through reg_off) become the regions dedup_run runs on."""
        regs = np.ascontiguousarray(regs, ALNREG_DTYPE)
        reg_off = np.ascontiguousarray(reg_off, np.int64)
        _chk(lib().bwams_debug_ext_regs_upload(self.h, _p(regs), len(regs), _p(reg_off), len(reg_off) - 1), "bwams_debug_ext_regs_upload")

    def debug_dedup_counts(self):
        """Test hook: what the last dedup_run under BWAMS_DEDUP_COUNT=1 did, as a dict over DEDUP_COUNTS (reads per tier, patch
        alignments per variant, early exits)."""
        cnt = np.zeros(len(self.DEDUP_COUNTS), np.int64)
        _chk(lib().bwams_debug_dedup_counts(self.h, _p(cnt)), "bwams_debug_dedup_counts")
        return dict(zip(self.DEDUP_COUNTS, cnt.tolist()))

    def debug_aln_lists(self):
        """Test hook: regions per launch of the last reg2aln (ring, wave 1, wave 2 with the requeued ones, row in global memory)."""
        cnt = np.zeros(4, np.int64)
        _chk(lib().bwams_debug_aln_lists(self.h, _p(cnt)), "bwams_debug_aln_lists")
        return cnt

    def sam_upload(self, names, quals=None, comments=None):
        """Names (list of bytes), qualities (uint8 array laid out like the reads, or None), comments (list of bytes / None, or
        None) of the uploaded chunk: what mem_aln2sam prints besides the alignment."""
        nb = b"".join(names)
        noff = np.zeros(len(names) + 1, np.int64)
        noff[1:] = np.cumsum([len(x) for x in names])
        cb, coff = None, None
        if comments is not None:
            cs = [c or b"" for c in comments]
            cb = b"".join(cs)
            coff = np.zeros(len(cs) + 1, np.int64)
            coff[1:] = np.cumsum([len(x) for x in cs])
        q = np.ascontiguousarray(quals, np.uint8) if quals is not None else None
        _chk(lib().bwams_sam_upload(self.h, nb, _p(noff), _p(q) if q is not None else None, cb, _p(coff) if coff is not None else None),
             "bwams_sam_upload")

    def sam_run(self, opt: MemOpt | None = None, sopt=None) -> int:
        """mem_reg2sam of every read (single-end; after mark_primary_se and reg2aln(source=1)) -> bytes of SAM text."""
        opt = opt or default_mem_opt()
        sopt = sopt or default_sam_opt()
        n = C.c_int64(0)
        _chk(lib().bwams_sam_run(self.h, C.byref(opt), C.byref(sopt), C.byref(n)), "bwams_sam_run")
        self._sam_bytes = n.value
        return n.value

    def process_chunk(self, fastq, paired: bool = False, emf=None, ert=None, seed_opt=None, opt: MemOpt | None = None, sopt=None,
                      pes=None, n_processed: int = 0, flags: int = 0, copy_comment: bool = False, fetch: bool = True):
        """mem_process_seqs for one chunk, text to text (bwams_process_chunk) -> (SAM text, read_off), or the byte count with
        fetch=False.  fastq: bytes, or (device address, n_bytes) for text already in this GPU's memory."""
        seed_opt = seed_opt or default_seed_opt()
        opt = opt or default_mem_opt()
        sopt = sopt or default_sam_opt()
        n, nb = C.c_int64(0), C.c_int64(0)
        pp = _p(np.ascontiguousarray(pes, PESTAT_DTYPE)) if pes is not None else None
        src, nbytes = (C.c_void_p(fastq[0]), fastq[1]) if isinstance(fastq, tuple) else (fastq, len(fastq))
        _chk(lib().bwams_process_chunk(self.h, emf.h if emf is not None else None, ert.h if ert is not None else None, C.byref(seed_opt),
                                       C.byref(opt), C.byref(sopt), src, C.c_int64(nbytes), 1 if paired else 0, pp,
                                       C.c_int64(n_processed), flags | (0x100 if copy_comment else 0), C.byref(n), C.byref(nb)), "bwams_process_chunk")
        self._nseq, self._sam_bytes = n.value, nb.value
        if not fetch:
            return nb.value
        text, off, _ = self.sam_fetch()
        return text, off

    def process_reads(self, enc, cum, names, name_off, quals=None, comments=None, comment_off=None, paired: bool = False, emf=None,
                      ert=None, seed_opt=None, opt: MemOpt | None = None, sopt=None, pes=None, n_processed: int = 0, flags: int = 0,
                      fetch: bool = True):
        """mem_process_seqs for a chunk of parsed records (bwams_process_reads: the form the reference hands over) -> (SAM text,
        read_off), or the byte count with fetch=False."""
        seed_opt = seed_opt or default_seed_opt()
        opt = opt or default_mem_opt()
        sopt = sopt or default_sam_opt()
        a = _flat_records(enc, cum, names, name_off, quals, comments, comment_off)
        nb = C.c_int64(0)
        pp = _p(np.ascontiguousarray(pes, PESTAT_DTYPE)) if pes is not None else None
        _chk(lib().bwams_process_reads(self.h, emf.h if emf is not None else None, ert.h if ert is not None else None, C.byref(seed_opt),
                                       C.byref(opt), C.byref(sopt), *a, 1 if paired else 0, pp, C.c_int64(n_processed), flags, C.byref(nb)),
             "bwams_process_reads")
        self._nseq, self._sam_bytes = len(cum) - 1, nb.value
        if not fetch:
            return nb.value
        text, off, _ = self.sam_fetch()
        return text, off

    def process_chunk2(self, fastq1: bytes, fastq2: bytes, emf=None, ert=None, seed_opt=None, opt: MemOpt | None = None, sopt=None, pes=None,
                       n_processed: int = 0, flags: int = 0, copy_comment: bool = False):
        """A paired-end chunk given as the two files' texts (bwams_process_chunk2) -> (SAM text, read_off)."""
        seed_opt = seed_opt or default_seed_opt()
        opt = opt or default_mem_opt()
        sopt = sopt or default_sam_opt()
        n, nb = C.c_int64(0), C.c_int64(0)
        pp = _p(np.ascontiguousarray(pes, PESTAT_DTYPE)) if pes is not None else None
        _chk(lib().bwams_process_chunk2(self.h, emf.h if emf is not None else None, ert.h if ert is not None else None, C.byref(seed_opt),
                                        C.byref(opt), C.byref(sopt), fastq1, C.c_int64(len(fastq1)), fastq2, C.c_int64(len(fastq2)), pp,
                                        C.c_int64(n_processed), flags | (0x100 if copy_comment else 0), C.byref(n), C.byref(nb)),
             "bwams_process_chunk2")
        self._nseq, self._sam_bytes = n.value, nb.value
        text, off, _ = self.sam_fetch()
        return text, off

    def process_chunk_smart(self, fastq, emf=None, ert=None, seed_opt=None, opt: MemOpt | None = None, sopt=None, pes=None,
                            n_processed: int = 0, flags: int = 0, copy_comment: bool = False):
        """process()'s MEM_F_SMARTPE branch for one chunk (bwams_process_chunk_smart): single reads and interleaved pairs mixed
        -> (SAM text, read_off, number of single reads)."""
        seed_opt = seed_opt or default_seed_opt()
        opt = opt or default_mem_opt()
        sopt = sopt or default_sam_opt()
        n, n0, nb = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        pp = _p(np.ascontiguousarray(pes, PESTAT_DTYPE)) if pes is not None else None
        src, nbytes = (C.c_void_p(fastq[0]), fastq[1]) if isinstance(fastq, tuple) else (fastq, len(fastq))
        _chk(lib().bwams_process_chunk_smart(self.h, emf.h if emf is not None else None, ert.h if ert is not None else None, C.byref(seed_opt),
                                             C.byref(opt), C.byref(sopt), src, C.c_int64(nbytes), pp, C.c_int64(n_processed),
                                             flags | (0x100 if copy_comment else 0), C.byref(n), C.byref(n0), C.byref(nb)),
             "bwams_process_chunk_smart")
        self._nseq, self._sam_bytes = n.value, nb.value
        text, off, _ = self.sam_fetch()
        return text, off, n0.value

    def process_chunk_bam(self, records, tags: bytes = b"", paired: bool = False, emf=None, ert=None, seed_opt=None, opt: MemOpt | None = None,
                          sopt=None, pes=None, n_processed: int = 0, flags: int = 0, copy_comment: bool = False, fetch: bool = True):
        """bwams_process_chunk_bam: process_chunk for a chunk of BAM records (bytes, or (device address, n_bytes)); tags as for
        bam_reads_decode -> (SAM text, read_off), or the byte count with fetch=False."""
        seed_opt = seed_opt or default_seed_opt()
        opt = opt or default_mem_opt()
        sopt = sopt or default_sam_opt()
        n, nb = C.c_int64(0), C.c_int64(0)
        pp = _p(np.ascontiguousarray(pes, PESTAT_DTYPE)) if pes is not None else None
        src, nbytes = (C.c_void_p(records[0]), records[1]) if isinstance(records, tuple) else (C.cast(C.c_char_p(records), C.c_void_p), len(records))
        _chk(lib().bwams_process_chunk_bam(self.h, emf.h if emf is not None else None, ert.h if ert is not None else None, C.byref(seed_opt),
                                           C.byref(opt), C.byref(sopt), src, nbytes, tags or None, 1 if paired else 0, pp, n_processed,
                                           flags | (0x100 if copy_comment else 0), C.byref(n), C.byref(nb)), "bwams_process_chunk_bam")
        self._nseq, self._sam_bytes = n.value, nb.value
        if not fetch:
            return nb.value
        text, off, _ = self.sam_fetch()
        return text, off

    def process_chunk_decoded(self, fq: "Fastq", paired: bool = False, emf=None, ert=None, seed_opt=None, opt: MemOpt | None = None, sopt=None,
                              pes=None, n_processed: int = 0, flags: int = 0, copy_comment: bool = False, fetch: bool = True):
        """bwams_process_chunk_decoded: process_chunk for a chunk already decoded (and perhaps trimmed); fq is consumed ->
        (SAM text, read_off), or the byte count with fetch=False."""
        seed_opt = seed_opt or default_seed_opt()
        opt = opt or default_mem_opt()
        sopt = sopt or default_sam_opt()
        n, nb = C.c_int64(0), C.c_int64(0)
        pp = _p(np.ascontiguousarray(pes, PESTAT_DTYPE)) if pes is not None else None
        h, fq.h = fq.h, C.c_void_p()
        _chk(lib().bwams_process_chunk_decoded(self.h, emf.h if emf is not None else None, ert.h if ert is not None else None, C.byref(seed_opt),
                                               C.byref(opt), C.byref(sopt), h, 1 if paired else 0, pp, n_processed,
                                               flags | (0x100 if copy_comment else 0), C.byref(n), C.byref(nb)), "bwams_process_chunk_decoded")
        self._nseq, self._sam_bytes = n.value, nb.value
        if not fetch:
            return nb.value
        text, off, _ = self.sam_fetch()
        return text, off

    def process_chunk_bam_smart(self, records, tags: bytes = b"", emf=None, ert=None, seed_opt=None, opt: MemOpt | None = None, sopt=None,
                                pes=None, n_processed: int = 0, flags: int = 0, copy_comment: bool = False):
        """bwams_process_chunk_bam_smart: process_chunk_smart for BAM records -> (SAM text, read_off, number of single reads)."""
        seed_opt = seed_opt or default_seed_opt()
        opt = opt or default_mem_opt()
        sopt = sopt or default_sam_opt()
        n, n0, nb = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        pp = _p(np.ascontiguousarray(pes, PESTAT_DTYPE)) if pes is not None else None
        src, nbytes = (C.c_void_p(records[0]), records[1]) if isinstance(records, tuple) else (C.cast(C.c_char_p(records), C.c_void_p), len(records))
        _chk(lib().bwams_process_chunk_bam_smart(self.h, emf.h if emf is not None else None, ert.h if ert is not None else None,
                                                 C.byref(seed_opt), C.byref(opt), C.byref(sopt), src, nbytes, tags or None, pp, n_processed,
                                                 flags | (0x100 if copy_comment else 0), C.byref(n), C.byref(n0), C.byref(nb)),
             "bwams_process_chunk_bam_smart")
        self._nseq, self._sam_bytes = n.value, nb.value
        text, off, _ = self.sam_fetch()
        return text, off, n0.value

    def sam_run_emf(self, emf: "Emf", opt: MemOpt | None = None, sopt=None) -> int:
        """sam_run for a chunk that went through emf_run + emf_regs_run: resolved reads get mem_perfect2sam_cont's records."""
        opt = opt or default_mem_opt()
        sopt = sopt or default_sam_opt()
        n = C.c_int64(0)
        _chk(lib().bwams_sam_run_emf(self.h, C.byref(opt), C.byref(sopt), emf.h, C.byref(n)), "bwams_sam_run_emf")
        self._sam_bytes = n.value
        return n.value

    def sam_run_pe(self, pes, opt: MemOpt | None = None, sopt=None) -> int:
        """mem_sam_pe's text of every pair (after pair_run and reg2aln(source=1)) -> bytes of SAM text."""
        opt = opt or default_mem_opt()
        sopt = sopt or default_sam_opt()
        pes = np.ascontiguousarray(pes, PESTAT_DTYPE)
        n = C.c_int64(0)
        _chk(lib().bwams_sam_run_pe(self.h, C.byref(opt), C.byref(sopt), _p(pes), C.byref(n)), "bwams_sam_run_pe")
        self._sam_bytes = n.value
        return n.value

    def sam_fetch(self, n_regs: int = 0):
        """(SAM text as bytes, read_off[nseq + 1], device-side mapq per region)."""
        buf = np.zeros(max(self._sam_bytes, 1), np.uint8)
        off = np.zeros(self._nseq + 1, np.int64)
        mq = np.zeros(max(n_regs, 1), np.int32)
        _chk(lib().bwams_sam_fetch(self.h, _p(buf), len(buf), _p(off), _p(mq) if n_regs else None, len(mq)), "bwams_sam_fetch")
        return bytes(buf[:self._sam_bytes]), off, mq[:n_regs]

    def sam_fetch_bgzf(self, deflater: "Deflater", eof: bool = False) -> bytes:
        """The SAM text of the last SAM run as BGZF members, compressed on the device where it lies (bwams_sam_fetch_bgzf)."""
        cap = deflate_bound(getattr(self, "_sam_bytes", 0))
        buf = C.create_string_buffer(cap)
        n = C.c_int64(0)
        _chk(lib().bwams_sam_fetch_bgzf(self.h, deflater.h, C.addressof(buf), cap, DEFLATE_EOF if eof else 0, C.byref(n)),
             "bwams_sam_fetch_bgzf")
        return buf.raw[:n.value]

    def bam_run(self) -> tuple[int, int]:
        """The SAM text of the last SAM run as BAM records on the device (bwams_bam_run): (bytes, records)."""
        nb, nr = C.c_int64(0), C.c_int64(0)
        _chk(lib().bwams_bam_run(self.h, C.byref(nb), C.byref(nr)), "bwams_bam_run")
        self._bam_bytes = nb.value
        self._bam_uploaded = None
        self._bam_nrec = nr.value
        return nb.value, nr.value

    def bam_upload(self, records: bytes) -> int:
        """Host BAM records (block_size included, back to back) become the batch's records (bwams_bam_upload): their number."""
        records = bytes(records)
        n = C.c_int64(0)
        _chk(lib().bwams_bam_upload(self.h, records, len(records), C.byref(n)), "bwams_bam_upload")
        self._bam_bytes = len(records)
        self._bam_uploaded = n.value
        self._bam_nrec = n.value
        return n.value

    def bam_sort(self) -> int:
        """The batch's BAM records in coordinate order, on the device (bwams_bam_sort): their number."""
        n = C.c_int64(0)
        _chk(lib().bwams_bam_sort(self.h, C.byref(n)), "bwams_bam_sort")
        self._bam_sorted = n.value
        return n.value

    def bam_sorted_fetch(self):
        """(sorted records as bytes, their coords as a BAM_COORD_DTYPE array) of the last bam_sort."""
        buf = np.empty(max(self._bam_bytes, 1), np.uint8)
        coords = np.zeros(max(self._bam_sorted, 1), BAM_COORD_DTYPE)
        _chk(lib().bwams_bam_sorted_fetch(self.h, _p(buf), len(buf), _p(coords)), "bwams_bam_sorted_fetch")
        return buf[:self._bam_bytes].tobytes(), coords[:self._bam_sorted]

    def bam_templates(self) -> tuple[int, int]:
        """The batch's BAM records grouped into templates, their duplicate-marking ends on the device (bwams_bam_templates):
        (templates, ends)."""
        nt, ne = C.c_int64(0), C.c_int64(0)
        _chk(lib().bwams_bam_templates(self.h, C.byref(nt), C.byref(ne)), "bwams_bam_templates")
        self._md_ends = ne.value
        return nt.value, ne.value

    def bam_templates_fetch(self, sorted: bool = False):
        """(ends as DUP_END_DTYPE, each record's template ordinal: in record order, or in bam_sort's order with sorted=True) of the
        last bam_templates (bwams_bam_templates_fetch)."""
        n_rec = self._bam_nrec
        ends = np.zeros(max(self._md_ends, 1), DUP_END_DTYPE)
        rt = np.zeros(max(n_rec, 1), np.uint32)
        _chk(lib().bwams_bam_templates_fetch(self.h, _p(ends), len(ends), _p(rt), 1 if sorted else 0), "bwams_bam_templates_fetch")
        return ends[:self._md_ends], rt[:n_rec]

    def bam_markdup(self) -> "DupStats":
        """Duplicate marking of the batch's BAM records where they lie, the unsorted records and the sorted copy (bwams_bam_markdup)."""
        st = DupStats()
        _chk(lib().bwams_bam_markdup(self.h, C.byref(st)), "bwams_bam_markdup")
        return st

    def bam_templates2(self, groups=None) -> tuple[int, int]:
        """bam_templates, and each template's read group, library and location on the device (bwams_bam_templates2); groups is a
        DupGroups or None."""
        nt, ne = C.c_int64(0), C.c_int64(0)
        _chk(lib().bwams_bam_templates2(self.h, _groups_h(groups), C.byref(nt), C.byref(ne)), "bwams_bam_templates2")
        self._md_ends = ne.value
        return nt.value, ne.value

    def bam_templates_fetch_loc(self):
        """One DUP_LOC_DTYPE row per end of the last bam_templates2 (bwams_bam_templates_fetch_loc)."""
        loc = np.zeros(max(self._md_ends, 1), DUP_LOC_DTYPE)
        _chk(lib().bwams_bam_templates_fetch_loc(self.h, _p(loc), len(loc)), "bwams_bam_templates_fetch_loc")
        return loc[:self._md_ends]

    def bam_lib_record_counts(self, n_lib: int = 1):
        """(secondary_or_supplementary, unmapped) records per library of the last bam_templates / bam_templates2."""
        a, u = np.zeros(n_lib, np.int64), np.zeros(n_lib, np.int64)
        _chk(lib().bwams_bam_lib_record_counts(self.h, _p(a), _p(u), n_lib), "bwams_bam_lib_record_counts")
        return a, u

    def bam_markdup2(self, groups=None, distance: int = 0, max_set: int = 0, opt=True, cap_lib: int | None = None):
        """bwams_bam_markdup2 -> (DupStats, rows: DUP_LIB_STATS_DTYPE per library).  opt=False passes a NULL bwams_dup_opt_t."""
        st = DupStats()
        n_lib = groups.n_lib if groups is not None else 1
        rows = np.zeros(max(n_lib if cap_lib is None else cap_lib, 1), DUP_LIB_STATS_DTYPE)
        o = _dup_opt(distance, max_set)
        _chk(lib().bwams_bam_markdup2(self.h, _groups_h(groups), C.byref(o) if opt else None, C.byref(st), _p(rows),
                                      n_lib if cap_lib is None else cap_lib), "bwams_bam_markdup2")
        return st, rows[:n_lib]

    def bam_fetch(self, n_reads: int | None = None):
        """(records of the last bam_run, n + 1 per-read offsets); n_reads defaults to the reads of the last SAM run (after a
        bam_upload: its records, each counted as one read)."""
        if n_reads is None and getattr(self, "_bam_uploaded", None) is not None:
            n_reads = self._bam_uploaded
        n = self._nseq if n_reads is None else n_reads
        buf = np.empty(max(self._bam_bytes, 1), np.uint8)
        off = np.zeros(n + 1, np.int64)
        _chk(lib().bwams_bam_fetch(self.h, _p(buf), len(buf), _p(off)), "bwams_bam_fetch")
        return buf[:self._bam_bytes].tobytes(), off

    def bam_fetch_bgzf(self, deflater: "Deflater", eof: bool = False) -> bytes:
        """The records of the last bam_run as BGZF members, compressed where they lie (bwams_bam_fetch_bgzf)."""
        cap = deflate_bound(getattr(self, "_bam_bytes", 0))
        buf = C.create_string_buffer(cap)
        n = C.c_int64(0)
        _chk(lib().bwams_bam_fetch_bgzf(self.h, deflater.h, C.addressof(buf), cap, DEFLATE_EOF if eof else 0, C.byref(n)),
             "bwams_bam_fetch_bgzf")
        return buf.raw[:n.value]

    def reg2aln_sam(self, opt: MemOpt | None = None, sopt=None, pes=None, fetch: bool = True):
        """mem_reg2aln of the regions the SAM text needs only (after mark_primary_se, or pair_run with its pes) ->
        (records, CIGAR pool, MD pool, number of regions aligned); skipped regions hold an unmapped record."""
        opt = opt or default_mem_opt()
        sopt = sopt or default_sam_opt()
        n, nn, nc, nm = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        pp = _p(np.ascontiguousarray(pes, PESTAT_DTYPE)) if pes is not None else None
        _chk(lib().bwams_reg2aln_run_sam(self.h, C.byref(opt), C.byref(sopt), pp, C.byref(n), C.byref(nn), C.byref(nc), C.byref(nm)),
             "bwams_reg2aln_run_sam")
        if not fetch:
            return n.value, nn.value
        aln = np.zeros(max(n.value, 1), ALN_DTYPE)
        cig = np.zeros(max(nc.value, 1), np.uint32)
        md = np.zeros(max(nm.value, 1), np.uint8)
        _chk(lib().bwams_reg2aln_fetch(self.h, _p(aln), len(aln), _p(cig), len(cig), _p(md), len(md)), "bwams_reg2aln_fetch")
        return aln[:n.value], cig[:nc.value], md[:nm.value], nn.value

    def pestat_keys(self, opt: MemOpt | None = None) -> np.ndarray:
        """One key per qualifying pair of this batch (orientation << 60 | insert size), sorted."""
        opt = opt or default_mem_opt()
        keys = np.zeros(max(self._nseq // 2, 1), np.uint64)
        n = C.c_int64(0)
        _chk(lib().bwams_pestat_keys(self.h, C.byref(opt), _p(keys), len(keys), C.byref(n)), "bwams_pestat_keys")
        return keys[:n.value].copy()

    def mark_primary_se(self, opt: MemOpt | None = None, id_base: int = 0, sopt=None):
        """Single-end chunk: mem_mark_primary_se of every read's final regions (then pair_fetch / reg2aln(source=1)); sopt carries
        MEM_F_PRIMARY5 and its T (bwams_pair_run_sam)."""
        opt = opt or default_mem_opt()
        n, nt = C.c_int64(0), C.c_int64(0)
        _chk(lib().bwams_pair_run_sam(self.h, C.byref(opt), C.byref(sopt) if sopt is not None else None, None, C.c_int64(id_base), 4,
                                      C.byref(n), C.byref(nt)), "bwams_pair_run_sam")
        self._n_pair_regs = n.value
        return n.value

    def pair_run(self, pes, opt: MemOpt | None = None, id_base: int = 0, no_rescue: bool = False, use_ert: bool = False, sopt=None):
        """Mate rescue + mem_mark_primary_se + mem_pair over the final regions (reads 2p, 2p+1 = pair p)
        -> (regions, rescue alignments).  sopt: MEM_F_PRIMARY5 / MEM_F_NOPAIRING / MEM_F_NO_RESCUE of its flag (bwams_pair_run_sam)."""
        opt = opt or default_mem_opt()
        pes = np.ascontiguousarray(pes, PESTAT_DTYPE)
        n, nt = C.c_int64(0), C.c_int64(0)
        _chk(lib().bwams_pair_run_sam(self.h, C.byref(opt), C.byref(sopt) if sopt is not None else None, _p(pes), C.c_int64(id_base),
                                      int(no_rescue) | (int(use_ert) << 1), C.byref(n), C.byref(nt)), "bwams_pair_run_sam")
        self._n_pair_regs = n.value
        return n.value, nt.value

    def pair_fetch(self):
        """-> (regs, reg_off, pairs) as mem_sam_pe_batch_post holds them before its MAPQ / SAM part."""
        regs = np.zeros(self._n_pair_regs, ALNREG_DTYPE)
        off = np.zeros(self._nseq + 1, np.int64)
        pairs = np.zeros(self._nseq // 2, PAIR_DTYPE)
        _chk(lib().bwams_pair_fetch(self.h, _p(regs), len(regs), _p(off), _p(pairs)), "bwams_pair_fetch")
        return regs, off, pairs

    def extend_tasks_fetch(self, side: int):
        n, rb, qb = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        rc = lib().bwams_extend_tasks_fetch(self.h, side, None, 0, None, 0, None, 0, C.byref(n), C.byref(rb), C.byref(qb))
        if rc not in (0, -4):
            _chk(rc, "bwams_extend_tasks_fetch")
        pairs = np.zeros(n.value, SEQPAIR_DTYPE)
        ref = np.zeros(rb.value, np.uint8)
        qer = np.zeros(qb.value, np.uint8)
        _chk(lib().bwams_extend_tasks_fetch(self.h, side, _p(pairs), n.value, _p(ref), rb.value, _p(qer), qb.value,
                                            C.byref(n), C.byref(rb), C.byref(qb)), "bwams_extend_tasks_fetch")
        return pairs, ref, qer

    def ksw_align(self, pairs, ref, qer, opt: SwOpt | None = None):
        """Mate-rescue local SW: int32[n, 7] = score, te, qe, score2, te2, tb, qb (pairs[i].h0 = xtra)."""
        opt = opt or default_sw_opt()
        p = np.ascontiguousarray(pairs)
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        qer = np.ascontiguousarray(qer, dtype=np.uint8)
        out = np.zeros((len(p), 7), dtype=np.int32)
        _chk(lib().bwams_ksw_align(self.h, _p(p), len(p), _p(ref), len(ref), _p(qer), len(qer), C.byref(opt), _p(out)),
             "bwams_ksw_align")
        return out

    def emf_probe(self, emf: Emf, enc, cum):
        """(perfect uint32[n, 2] = flags, location; code uint8[n])."""
        enc = np.ascontiguousarray(enc, dtype=np.uint8)
        cum = np.ascontiguousarray(cum, dtype=np.int64)
        n = len(cum) - 1
        out = np.zeros((max(n, 1), 2), dtype=np.uint32)
        code = np.zeros(max(n, 1), dtype=np.uint8)
        _chk(lib().bwams_emf_probe(self.h, emf.h, _p(enc), _p(cum), n, _p(out), _p(code)), "bwams_emf_probe")
        return out[:n], code[:n]

    def emf_regs_merge(self) -> int:
        """Paired-end: the regions of the EMF-resolved reads join the final regions (after dedup_run and pestat, before pair_run)."""
        n = C.c_int64(0)
        _chk(lib().bwams_emf_regs_merge(self.h, C.byref(n)), "bwams_emf_regs_merge")
        return n.value

    def emf_run(self, emf: Emf):
        _chk(lib().bwams_emf_run(self.h, emf.h), "bwams_emf_run")

    def emf_fetch(self, n: int):
        out = np.zeros((max(n, 1), 2), dtype=np.uint32)
        code = np.zeros(max(n, 1), dtype=np.uint8)
        _chk(lib().bwams_emf_fetch(self.h, _p(out), _p(code)), "bwams_emf_fetch")
        return out[:n], code[:n]

    def stats(self) -> Stats:
        s = Stats()
        _chk(lib().bwams_batch_stats(self.h, C.byref(s)), "bwams_batch_stats")
        return s

    def sync(self):
        _chk(lib().bwams_batch_sync(self.h), "bwams_batch_sync")

    def close(self):
        if self.h:
            lib().bwams_batch_destroy(self.h)
            self.h = None


class _Kept(tuple):
    """an argument tuple that owns the arrays its pointers point into: alive as long as the caller's local holds it"""
    def __new__(cls, args, keep):
        t = super().__new__(cls, args)
        t.keep = keep
        return t


def _flat_records(enc, cum, names, name_off, quals, comments, comment_off):
    """the argument block (enc, cum, n, names, name_off, quals, comments, comment_off) of bwams_process_reads and its relatives;
    the converted arrays live in the returned tuple (hold it in a local until the C call has returned: ctypes releases the GIL)"""
    enc = np.ascontiguousarray(enc, np.uint8)
    cum = np.ascontiguousarray(cum, np.int64)
    names = np.ascontiguousarray(names, np.uint8)
    name_off = np.ascontiguousarray(name_off, np.int64)
    q = np.ascontiguousarray(quals, np.uint8) if quals is not None else None
    c = np.ascontiguousarray(comments, np.uint8) if comments is not None else None
    co = np.ascontiguousarray(comment_off, np.int64) if comment_off is not None else None
    return _Kept((_p(enc), _p(cum), C.c_int64(len(cum) - 1), _p(names), _p(name_off), _p(q), _p(c), _p(co)), (enc, cum, names, name_off, q, c, co))


def debug_reload():
    """re-read the library's debugging aids / A-B switches from the environment (they are parsed once otherwise)"""
    lib().bwams_debug_reload()


def shard_bounds(n_reads: int, n_shards: int, paired: bool = False) -> np.ndarray:
    """bwams_shard_bounds: where the shards of a chunk begin (n_shards + 1 read indices)"""
    b = np.zeros(n_shards + 1, np.int64)
    _chk(lib().bwams_shard_bounds(C.c_int64(n_reads), n_shards, 1 if paired else 0, _p(b)), "bwams_shard_bounds")
    return b


class Multi:
    """One chunk over several batches (one per GPU, or several on one GPU) behind one call: host/chunk_multi.cpp."""

    def __init__(self, batches, emfs=None, erts=None):
        self.batches = list(batches)
        n = len(self.batches)
        arr = (C.c_void_p * n)(*[b.h for b in self.batches])
        ea = (C.c_void_p * n)(*[e.h for e in emfs]) if emfs else None
        ra = (C.c_void_p * n)(*[e.h for e in erts]) if erts else None
        self.h = C.c_void_p()
        _chk(lib().bwams_multi_create(arr, ea, ra, n, C.byref(self.h)), "bwams_multi_create")
        self._n = 0

    def process_reads(self, enc, cum, names, name_off, quals=None, comments=None, comment_off=None, paired: bool = False, seed_opt=None,
                      opt: MemOpt | None = None, sopt=None, pes=None, n_processed: int = 0, flags: int = 0):
        """-> (SAM text of the chunk in read order, read_off[n + 1])"""
        seed_opt = seed_opt or default_seed_opt()
        opt = opt or default_mem_opt()
        sopt = sopt or default_sam_opt()
        a = _flat_records(enc, cum, names, name_off, quals, comments, comment_off)
        nb = C.c_int64(0)
        pp = _p(np.ascontiguousarray(pes, PESTAT_DTYPE)) if pes is not None else None
        L = lib()
        L.bwams_multi_error.restype = C.c_char_p
        rc = L.bwams_multi_process_reads(self.h, C.byref(seed_opt), C.byref(opt), C.byref(sopt), *a, 1 if paired else 0, pp,
                                         C.c_int64(n_processed), flags, C.byref(nb))
        if rc:
            raise BwamsError(rc, "bwams_multi_process_reads", (L.bwams_multi_error(self.h) or b"").decode())
        n = len(cum) - 1
        buf = np.zeros(max(nb.value, 1), np.uint8)
        off = np.zeros(n + 1, np.int64)
        _chk(L.bwams_multi_fetch(self.h, _p(buf), C.c_int64(nb.value), _p(off)), "bwams_multi_fetch")
        return buf[:nb.value].tobytes(), off

    def close(self):
        if self.h:
            lib().bwams_multi_destroy(self.h)
            self.h = None


_PINNED = {}          # address of a pinned_array's memory -> its finalizer (pinned_free runs it early)


def pinned_array(n: int, dtype=np.uint8) -> np.ndarray:
    """a numpy view of page-locked host memory (bwams_host_alloc).  Free it with pinned_free(arr) when done; an array that is simply
    dropped is freed when it is garbage collected (a finalizer that may run late, at interpreter exit)"""
    dt = np.dtype(dtype)
    p = C.c_void_p()
    _chk(lib().bwams_host_alloc(C.c_size_t(max(n, 1) * dt.itemsize), C.byref(p)), "bwams_host_alloc")
    buf = (C.c_uint8 * (max(n, 1) * dt.itemsize)).from_address(p.value)
    arr = np.frombuffer(buf, dtype=dt, count=n)
    import weakref
    _PINNED[p.value] = weakref.finalize(buf, lambda a=p.value: lib().bwams_host_free(C.c_void_p(a)))
    return arr


def pinned_free(arr: np.ndarray) -> None:
    """give a pinned_array's memory back now (the array must not be used afterwards)"""
    fin = _PINNED.pop(arr.ctypes.data, None)
    if fin is not None:
        fin()


# ---------------------------------------------------------------------------------------------------------------------------------
# The compiled outer boundary (bwa-mem-scale_amd/host/mem_process_seqs_hip.cpp) driven from Python: the reference's own records
# (bseq1_t, mem_opt_t: the layout mirrors of host/bwamem_hip.h) through mem_process_seqs() and the pipeline's two other steps.
# The host layer has C++ linkage, as mem_process_seqs has in the reference; its symbols are looked up by name in the library.
BSEQ1_DTYPE = np.dtype([("l_seq", "<i4"), ("id", "<i4"), ("strbuf", "<u8"), ("name", "<u8"), ("comment", "<u8"), ("seq", "<u8"),
                        ("qual", "<u8"), ("sam", "<u8"), ("perfect", "<u8")])
assert BSEQ1_DTYPE.itemsize == 64
WORK_ITEM = 512          # BATCH_SIZE, src/macro.h:63: reads per seqs[].sam string


class MemOptT(C.Structure):
    """mem_opt_t (src/bwamem.h:89-124, built without AFF): 176 bytes"""
    _fields_ = [("a", C.c_int), ("b", C.c_int), ("o_del", C.c_int), ("e_del", C.c_int), ("o_ins", C.c_int), ("e_ins", C.c_int),
                ("pen_unpaired", C.c_int), ("pen_clip5", C.c_int), ("pen_clip3", C.c_int), ("w", C.c_int), ("zdrop", C.c_int),
                ("max_mem_intv", C.c_uint64), ("T", C.c_int), ("flag", C.c_int), ("min_seed_len", C.c_int), ("min_chain_weight", C.c_int),
                ("max_chain_extend", C.c_int), ("split_factor", C.c_float), ("split_width", C.c_int), ("max_occ", C.c_int),
                ("max_chain_gap", C.c_int), ("n_threads", C.c_int), ("chunk_size", C.c_int64), ("mask_level", C.c_float),
                ("drop_ratio", C.c_float), ("XA_drop_ratio", C.c_float), ("mask_level_redun", C.c_float), ("mapQ_coef_len", C.c_float),
                ("mapQ_coef_fac", C.c_int), ("max_ins", C.c_int), ("max_matesw", C.c_int), ("max_XA_hits", C.c_int),
                ("max_XA_hits_alt", C.c_int), ("mat", C.c_int8 * 25)]


assert C.sizeof(MemOptT) == 176


def mem_opt_init(paired: bool = False) -> MemOptT:
    """mem_opt_init (src/bwamem.cpp:135-171) + bwa_fill_scmat"""
    import math
    o = MemOptT()
    o.a, o.b, o.o_del, o.o_ins, o.e_del, o.e_ins, o.w, o.T, o.zdrop = 1, 4, 6, 6, 1, 1, 100, 30, 100
    o.pen_unpaired, o.pen_clip5, o.pen_clip3, o.max_mem_intv, o.min_seed_len, o.split_width = 17, 5, 5, 20, 19, 10
    o.max_occ, o.max_chain_gap, o.max_ins, o.mask_level, o.drop_ratio = 500, 10000, 10000, 0.50, 0.50
    o.XA_drop_ratio, o.split_factor, o.chunk_size, o.n_threads, o.max_XA_hits, o.max_XA_hits_alt = 0.80, 1.5, 10000000, 1, 5, 200
    o.max_matesw, o.mask_level_redun, o.min_chain_weight, o.max_chain_extend, o.mapQ_coef_len = 50, 0.95, 0, 1 << 30, 50
    o.mapQ_coef_fac = int(math.log(o.mapQ_coef_len))
    k = 0
    for i in range(4):
        for j in range(4):
            o.mat[k] = o.a if i == j else -o.b
            k += 1
        o.mat[k] = -1
        k += 1
    for _ in range(5):
        o.mat[k] = -1
        k += 1
    if paired:
        o.flag |= 0x2
    return o


_host_syms = None


def _host_sym(name: str):
    """the host layer's function `name` (C++ linkage: looked up among the library's dynamic symbols by its mangled prefix)"""
    global _host_syms
    if _host_syms is None:
        out = subprocess.check_output(["nm", "-D", "--defined-only", LIB_PATH]).decode()
        _host_syms = [ln.split()[-1] for ln in out.splitlines() if " T _Z" in ln]
    key = f"_Z{len(name)}{name}"
    hit = [m for m in _host_syms if m.startswith(key) and (len(m) == len(key) or not m[len(key)].islower())]
    if len(hit) != 1:
        raise BwamsError(-3, name, f"host-layer symbol not found or ambiguous: {hit}")
    f = getattr(lib(), hit[0])
    f.restype = C.c_int
    return f


class Seqs:
    """A chunk as the reference holds it between kt_pipeline's steps: a bseq1_t array whose strings live in this object's buffers."""

    def __init__(self, reads: np.ndarray, first_id: int = 0, name_fmt: bytes = b"r%08d", quals: bool = True, name_ids=None):
        """reads: (n, RL) base codes 0..4; names are name_fmt % (first_id + i), or % name_ids[i] (paired-end: the pair's number)"""
        n, RL = reads.shape
        self.n = n
        self.seq = np.zeros((n, RL + 1), np.uint8)
        self.seq[:, :RL] = np.frombuffer(b"ACGTN", np.uint8)[reads]
        w = len(name_fmt % 0) + 1
        self.names = np.zeros((n, w), np.uint8)
        ids = first_id + np.arange(n, dtype=np.int64) if name_ids is None else np.asarray(name_ids, np.int64)
        head = name_fmt.split(b"%")[0]
        nd = w - 1 - len(head)
        self.names[:, :len(head)] = np.frombuffer(head, np.uint8)
        for d in range(nd):
            self.names[:, len(head) + d] = ord("0") + (ids // 10 ** (nd - 1 - d)) % 10
        self.qual = None
        if quals:
            self.qual = np.zeros((n, RL + 1), np.uint8)
            self.qual[:, :RL] = ord("I")
        self.arr = np.zeros(n, BSEQ1_DTYPE)
        self.arr["l_seq"] = RL
        self.arr["id"] = ids.astype(np.int32)
        self.arr["name"] = self.names.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(w)
        self.arr["seq"] = self.seq.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(RL + 1)
        if quals:
            self.arr["qual"] = self.qual.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(RL + 1)

    @property
    def ptr(self):
        return C.c_void_p(self.arr.ctypes.data)

    def drop_sam(self) -> int:
        """free the work items' strings unread (a writer that costs nothing); returns their total length"""
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        libc.strlen.argtypes = [C.c_void_p]
        libc.strlen.restype = C.c_size_t
        total = 0
        for i in range(0, self.n, WORK_ITEM):
            p = int(self.arr["sam"][i])
            if not p:
                raise BwamsError(-3, "drop_sam", f"work item {i // WORK_ITEM} left no text")
            total += libc.strlen(C.c_void_p(p))
            libc.free(C.c_void_p(p))
            self.arr["sam"][i] = 0
        return total

    def take_sam(self) -> bytes:
        """the chunk's SAM text (the work items' strings joined, as step 2 writes them), the strings freed"""
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        parts = []
        for i in range(0, self.n, WORK_ITEM):
            p = int(self.arr["sam"][i])
            if not p:
                raise BwamsError(-3, "take_sam", f"work item {i // WORK_ITEM} left no text")
            parts.append(C.string_at(p))
            libc.free(C.c_void_p(p))
            self.arr["sam"][i] = 0
        return b"".join(parts)


class Worker:
    """bwams_worker (host/bwamem_hip.h): the resident index set of every device and `depth` chunks in flight."""

    def __init__(self, indexes, max_reads: int, max_bases: int, emfs=None, erts=None, depth: int = 1, rg_id: bytes = b""):
        n = len(indexes)
        ia = (C.c_void_p * n)(*[x.h for x in indexes])
        ea = (C.c_void_p * n)(*[e.h for e in emfs]) if emfs else None
        ra = (C.c_void_p * n)(*[e.h for e in erts]) if erts else None
        self.h = C.c_void_p()
        _chk(_host_sym("bwams_worker_create_multi")(ia, ea, ra, n, depth, C.c_int64(max_reads), C.c_int64(max_bases), rg_id, C.byref(self.h)),
             "bwams_worker_create_multi")
        self._keep = (indexes, emfs, erts)

    def _err(self, rc, what):
        if rc:
            f = _host_sym("bwams_worker_error")
            f.restype = C.c_char_p
            raise BwamsError(rc, what, (f(self.h) or b"").decode())

    def set_deferred_collect(self, on: bool):
        _host_sym("bwams_worker_set_deferred_collect")(self.h, 1 if on else 0)

    def stage(self, opt: MemOptT, seqs: Seqs):
        self._err(_host_sym("mem_process_seqs_stage")(C.byref(opt), seqs.n, seqs.ptr, self.h), "mem_process_seqs_stage")

    def process(self, opt: MemOptT, n_processed: int, seqs: Seqs, pes0=None):
        pp = _p(np.ascontiguousarray(pes0, PESTAT_DTYPE)) if pes0 is not None else None
        self._err(_host_sym("bwams_worker_process")(C.byref(opt), C.c_int64(n_processed), seqs.n, seqs.ptr, pp, self.h), "mem_process_seqs")

    def collect(self, opt: MemOptT, seqs: Seqs):
        self._err(_host_sym("mem_process_seqs_collect")(C.byref(opt), seqs.n, seqs.ptr, self.h), "mem_process_seqs_collect")

    def close(self):
        if self.h:
            f = _host_sym("bwams_worker_destroy")
            f.restype = None
            f(self.h)
            self.h = None
