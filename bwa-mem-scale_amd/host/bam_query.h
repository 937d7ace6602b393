// bam_query.h — the host side of a BAM file read back by region (include/bwams.h, "BAM file by region"): the BAM header block, the
// BAI parse, rule 2's merge of the regions, rule 3's plan, and the file of bwams_bam_file_t cut into pieces of whole BGZF members.
// Plain C++ over include/bwams.h: host/bam_query.cpp holds the definitions, csrc/api_bam_file.hip the device side of the handle,
// host/fastq_io.cpp shares the header parse, tools/bai_plan_check.cpp builds the planner alone.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "bwams.h"

namespace bwams {

// The BAM header block (magic, l_text, text, n_ref, then l_name / name / l_ref per reference) read from the start of an inflated
// stream.  read(dst, want, err): up to `want` more bytes of the stream, 0 at its end, a negative BWAMS_ERR_* with a text in err.
// hb receives every byte read, the header and what came behind it; h->end is where the first record starts in hb.
struct BamHeader {
    std::string text;
    int32_t n_ref = 0;
    std::vector<int32_t> l_ref;
    size_t end = 0;
};
using BamHeaderRead = std::function<int64_t(char *dst, int64_t want, std::string &err)>;
int bam_header_read(const BamHeaderRead &read, int64_t step, std::vector<char> *hb, BamHeader *h, std::string *err);

// A BAI (SAMv1 section 5.2) parsed with every count checked against the buffer.  Reference r's bin k is bin[k] with the chunks
// [first[k], first[k + 1]) of beg / end; pseudo-bin 37450 stays among them.
struct BaiRef {
    std::vector<uint32_t> bin;
    std::vector<int64_t> first;
    std::vector<uint64_t> beg, end, lin;
};
struct Bai {
    std::vector<BaiRef> refs;
    uint64_t n_no_coor = 0;
};
int bai_parse(const void *bai, int64_t n_bai, Bai *out, std::string *err);      // BWAMS_ERR_IO with a text: not a BAI, or cut off

// Rule 2: the regions checked against n_ref, sorted by (ref, beg) and merged per reference where they overlap or touch.
int regions_merge(const bwams_pileup_region_t *regions, int32_t n_regions, int32_t n_ref, std::vector<bwams_pileup_region_t> *out,
                  std::string *err);
// Rule 3: the disjoint intervals of virtual offsets, ascending, that hold every record overlapping a merged region.
void bai_plan(const Bai &bai, const std::vector<bwams_pileup_region_t> &merged, std::vector<uint64_t> *beg, std::vector<uint64_t> *end);

// One piece of the current query as the device side receives it: whole members of one interval inflated behind the carried bytes.
struct BamPiece {
    int64_t file_off = 0;            // of the piece's first member
    int64_t members = 0, n_in = 0, n_out = 0;
    int64_t start = 0;               // first piece of an interval: where its record chain starts in the inflated bytes (else 0)
    int64_t stop = -1;               // the interval's end in the inflated bytes when it lies in this piece, else -1
    bool first = false, last = false;    // of its interval
    float ms_read = 0, ms_inflate = 0;   // host clock
};

// The file of a bwams_bam_file_t: descriptor, header, index, the plan of the current query and where the next piece starts.
struct BamFileHost {
    std::string path;
    int fd = -1;
    int64_t file_size = 0;
    BamHeader hdr;
    std::vector<char> header_block;  // the header as the file holds it, inflated: magic to the last reference's l_ref
    uint64_t first_voff = 0;         // the first record behind the header
    bool has_index = false;
    Bai bai;
    int64_t piece_bytes = 0, stage_cap = 0;
    uint8_t *stage = nullptr;        // page-locked: the compressed bytes of a piece
    bwams_inflater_t *inf = nullptr;
    std::vector<uint64_t> iv_beg, iv_end;    // the plan
    size_t iv = 0;                   // the interval the next piece belongs to
    int64_t at = -1;                 // file offset of its next member; -1: the interval has not begun
    BamFileHost() = default;
    BamFileHost(const BamFileHost &) = delete;
    BamFileHost &operator=(const BamFileHost &) = delete;
    ~BamFileHost();
    // who: the entry point named in error texts.  Errors leave a text in bwams_last_error through set_error.
    int open(const char *path, const char *bai_path, int device, int64_t piece_bytes, std::string *err);
    int query(const bwams_pileup_region_t *regions, int32_t n_regions, std::vector<bwams_pileup_region_t> *merged, std::string *err);
    bool exhausted() const { return iv >= iv_beg.size(); }
    // The next piece of the current interval, inflated to dev_out (device memory of the handle's device, piece_bytes of room).
    int next_piece(void *dev_out, BamPiece *p, std::string *err);
};

// host/bam_merge_header.cpp: the header block of n_files files merged (include/bwams.h, above bwams_bam_file_open_merge, rules M2 and
// M3) from their header blocks (magic to the last reference's l_ref; bytes behind that are not looked at).  *pg_dropped (may be
// null): the @PG lines M3 dropped.  BWAMS_ERR_ARG for a block that is cut off or has the wrong magic, BWAMS_ERR_UNSUPPORTED for
// reference lists that differ and for an @RG ID taken with other bytes; the text in *err.
int bam_header_merge(const void *const *blocks, const int64_t *n_block, int32_t n_files, std::string *out, int32_t *pg_dropped,
                     std::string *err);

}  // namespace bwams
