// bam_sort.cpp — the sorted BAM writer (bwams_sorter): what `samtools sort` and `samtools index` do behind the unsorted stream.
//
// Every put is one run, already in coordinate order (bwams_bam_sort sorted it on the GPU), tagged with its sequence number.  Runs
// stay in host memory up to mem_bytes; past that a run is spilled raw (its coords, then its records) to "<tmp_prefix>.<n>.run".
// Close merges the runs k ways by (key, seq, index in the run) — the stable sort of the runs concatenated in seq order — reading
// spilled runs through bounded buffers, and hands the merged record stream to a bwams_deflater in pieces of whole 65280-byte
// members, so that member m holds record-stream bytes [65280 m, 65280 (m + 1)) whatever the piece size, and every record's virtual
// offset follows from the members' sizes.  The index (SAMv1 §5.2; bwams/bai.py restates it byte for byte) is built during the
// merge from the coords, the records' FLAG and those sizes, as htslib's hts_idx_push / hts_idx_finish build it:
//   * per reference, a chunk [first record's start, last record's end) of virtual offsets for every stretch of records of one bin
//     (bin = reg2bin(beg, end) with beg = max(POS, 0) and end = max(end, beg + 1)); a chunk that starts in the compressed block where
//     its bin's previous chunk ends is merged into it;
//   * the 16 kb linear index: the start of the first record (placed, mapped or not) that covers each window; empty windows in front
//     of the first record take the reference's first offset, the others their left neighbour's;
//   * pseudo-bin 37450: (first record's start, last record's end), (n_mapped, n_unmapped) — unmapped = FLAG 0x4, placed here;
//   * bins in ascending order; references without records have no bins and no linear index; n_no_coor at the end.
// Virtual offsets: a record starting at record-stream byte x is at (member of x) << 16 | x % 65280; one ending before byte y at
// (member of y - 1) << 16 | ((y - 1) % 65280 + 1), the end of that member's data rather than the start of the next member.
// With BWAMS_SORT_MARKDUP every put_batch also keeps its batch's duplicate-marking ends (host memory, outside mem_bytes) and each
// record's template ordinal in sorted order (with the run: in memory, or spilled after its records).  Close offsets each run's
// ordinals by the templates of the runs before it in seq order, runs one bwams_dup_decide over all the ends, and sets or clears
// FLAG 0x400 (bit 2 of the record's byte 19) in the merge buffer as each record is copied; the index does not read that bit.
// After bwams_sorter_set_markdup a put_batch runs bwams_bam_templates2 with the sorter's copy of the groups table and also keeps the
// put's bwams_dup_loc_t per end and its two record-level counts per library; close3 hands ends and locs to bwams_dup_decide2 and adds
// the puts' record-level counts to its rows.
// After bwams_sorter_set_depth, _set_pileup, _set_qc and / or _set_recal close also hands the merged stream, as written, to those
// handles: every flushed piece goes to bwams_depth_add_records, bwams_pileup_add_records, bwams_qc_add_records and
// bwams_recal_add_records in whole records; the bytes of a record that the piece's
// end cuts wait in a carry buffer for the next piece, so the record is added once, with its final flag, wherever the pieces cut.
// Plain C++ over the C-ABI (no HIP header), like fastq_io.cpp.
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <set>
#include <string>
#include <vector>

#include "bwams.h"
#include "depth_host.h"
#include "pileup_host.h"
#include "qc_host.h"
#include "recal_host.h"
#include "dup_groups.h"

namespace {

using Clock = std::chrono::steady_clock;
float ms_since(Clock::time_point t0) { return std::chrono::duration<float, std::milli>(Clock::now() - t0).count(); }

constexpr int64_t kMember = 65280;                    // record-stream bytes per BGZF member
constexpr int64_t kPiece = 256 * kMember;             // bytes per deflater call (16.7 MB)
constexpr int64_t kSpillCoords = 1 << 16;             // a spilled run's read buffers: coords, and record bytes
constexpr int64_t kSpillBytes = 8 << 20;
constexpr uint32_t kMaxBai = 1u << 29;
constexpr uint32_t kPseudoBin = 37450;
const uint8_t kBgzfEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0,
                              0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

uint32_t rd32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }

struct Run {
    int64_t seq = 0, n_rec = 0, n_bytes = 0;
    std::unique_ptr<uint8_t[]> recs;                  // in memory; empty when spilled
    std::vector<bwams_bam_coord_t> coords;
    std::string path;                                 // spilled: coords, then records (then, with markdup, template ordinals)
    std::vector<uint32_t> tmpl;                       // markdup: each record's template ordinal, in sorted order (empty when spilled)
    std::vector<bwams_dup_end_t> ends;                // markdup: the batch's ends, tmpl local to the run
    int64_t n_tmpl = 0;
    std::vector<bwams_dup_loc_t> loc;                 // after set_markdup: parallel to ends
    std::vector<int64_t> rec_counts;                  // after set_markdup: secondary_or_supplementary[n_lib], then unmapped[n_lib]
};

// One run's records in order: from memory, or from its spill file through bounded buffers.
struct Cursor {
    const Run *r = nullptr;
    int fd = -1;
    int64_t i = 0, at = 0;                            // the current record and its offset in the run's records
    std::vector<bwams_bam_coord_t> cb;                // spilled: coords [c0, c0 + cb.size())
    int64_t c0 = 0;
    std::vector<uint8_t> rb;                          // spilled: record bytes [b0, b0 + bn)
    int64_t b0 = 0, bn = 0;
    std::vector<uint32_t> tb;                         // spilled, markdup: template ordinals [t0, t0 + tb.size())
    int64_t t0 = 0;

    bool pread_all(void *dst, int64_t n, int64_t off) {
        for (int64_t got = 0; got < n;) {
            const ssize_t k = ::pread(fd, static_cast<uint8_t *>(dst) + got, (size_t)(n - got), (off_t)(off + got));
            if (k <= 0) return false;
            got += k;
        }
        return true;
    }
    bool coord(bwams_bam_coord_t *c) {
        if (r->recs) { *c = r->coords[(size_t)i]; return true; }
        if (i < c0 || i >= c0 + (int64_t)cb.size()) {
            c0 = i;
            cb.resize((size_t)std::min(kSpillCoords, r->n_rec - i));
            if (!pread_all(cb.data(), (int64_t)cb.size() * 16, i * 16)) return false;
        }
        *c = cb[(size_t)(i - c0)];
        return true;
    }
    const uint8_t *bytes(int64_t size) {
        if (r->recs) return r->recs.get() + at;
        if (at < b0 || at + size > b0 + bn) {
            b0 = at;
            bn = std::min(std::max(kSpillBytes, size), r->n_bytes - at);
            if ((int64_t)rb.size() < bn) rb.resize((size_t)bn);
            if (!pread_all(rb.data(), bn, r->n_rec * 16 + at)) return nullptr;
        }
        return rb.data() + (at - b0);
    }
    bool tmpl(uint32_t *t) {
        if (r->recs) { *t = r->tmpl[(size_t)i]; return true; }
        if (i < t0 || i >= t0 + (int64_t)tb.size()) {
            t0 = i;
            tb.resize((size_t)std::min(kSpillCoords, r->n_rec - i));
            if (!pread_all(tb.data(), (int64_t)tb.size() * 4, r->n_rec * 16 + r->n_bytes + i * 4)) return false;
        }
        *t = tb[(size_t)(i - t0)];
        return true;
    }
};

uint32_t reg2bin(int64_t beg, int64_t end) {        // SAMv1 §5.3
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// The BAI of the merged stream, record by record in file order (the rules are at the top of the file).
struct Bai {
    struct Chunk { uint64_t b, e; };
    struct Ref {
        std::map<uint32_t, std::vector<Chunk>> bins;
        std::vector<uint64_t> lin;
        uint64_t off_beg = 0, off_end = 0, n_mapped = 0, n_unmapped = 0;
        bool any = false;
    };
    static constexpr uint64_t kUnset = ~0ULL;
    std::vector<Ref> refs;
    int64_t cur = -1;
    uint32_t cur_bin = 0;
    Chunk chunk{0, 0};
    bool open_chunk = false;
    uint64_t n_no_coor = 0;

    static void add(Ref &r, uint32_t bin, Chunk c) {
        std::vector<Chunk> &v = r.bins[bin];
        if (!v.empty() && (c.b >> 16) <= (v.back().e >> 16)) v.back().e = std::max(v.back().e, c.e);
        else v.push_back(c);
    }
    void end_ref() {
        if (cur >= 0 && open_chunk) add(refs[(size_t)cur], cur_bin, chunk);
        open_chunk = false;
        cur = -1;
    }
    void push(uint64_t key, int32_t end, uint32_t flag, uint64_t vb, uint64_t ve) {
        const uint32_t rid = (uint32_t)(key >> 32);
        if (rid == 0xFFFFFFFFu) { end_ref(); ++n_no_coor; return; }
        if ((int64_t)rid != cur) { end_ref(); cur = rid; }
        Ref &r = refs[rid];
        const int64_t pos = (int64_t)((key >> 1) & 0x7FFFFFFF) - 1;
        const int64_t beg = std::max<int64_t>(pos, 0), e = std::max<int64_t>(end, beg + 1);
        const uint32_t bin = reg2bin(beg, e);
        if (!r.any) { r.any = true; r.off_beg = vb; }
        r.off_end = ve;
        if (flag & 4) ++r.n_unmapped;
        else ++r.n_mapped;
        if (open_chunk && bin == cur_bin) {
            chunk.e = ve;
        } else {
            if (open_chunk) add(r, cur_bin, chunk);
            cur_bin = bin;
            chunk = {vb, ve};
            open_chunk = true;
        }
        const int64_t w0 = beg >> 14, w1 = (e - 1) >> 14;
        if ((int64_t)r.lin.size() <= w1) r.lin.resize((size_t)w1 + 1, kUnset);
        for (int64_t w = w0; w <= w1; ++w)
            if (r.lin[(size_t)w] == kUnset) r.lin[(size_t)w] = vb;
    }
    std::string finish() {
        end_ref();
        std::string s("BAI\1", 4);
        auto u32 = [&](uint32_t v) { s.append(reinterpret_cast<const char *>(&v), 4); };
        auto u64 = [&](uint64_t v) { s.append(reinterpret_cast<const char *>(&v), 8); };
        u32((uint32_t)refs.size());
        for (Ref &r : refs) {
            if (!r.any) { u32(0); u32(0); continue; }
            u32((uint32_t)r.bins.size() + 1);
            for (const auto &kv : r.bins) {
                u32(kv.first);
                u32((uint32_t)kv.second.size());
                for (const Chunk &c : kv.second) { u64(c.b); u64(c.e); }
            }
            u32(kPseudoBin); u32(2);
            u64(r.off_beg); u64(r.off_end); u64(r.n_mapped); u64(r.n_unmapped);
            size_t l = 0;
            for (; l < r.lin.size() && r.lin[l] == kUnset; ++l) r.lin[l] = r.off_beg;
            for (; l < r.lin.size(); ++l)
                if (r.lin[l] == kUnset) r.lin[l] = r.lin[l - 1];
            u32((uint32_t)r.lin.size());
            for (uint64_t v : r.lin) u64(v);
        }
        u64(n_no_coor);
        return s;
    }
};

}  // namespace

struct bwams_sorter {
    std::string path, tmp_prefix;
    int device = 0;
    int32_t flags = 0;
    int64_t mem_bytes = 0, mem_used = 0;
    std::vector<int32_t> l_ref;                       // of the header's references
    std::string header_gz;                            // the header block as members of its own
    FILE *fp = nullptr;
    bwams_deflater_t *def = nullptr;
    std::mutex mu;
    std::set<int64_t> seqs;
    std::vector<std::unique_ptr<Run>> runs;
    int64_t n_spill = 0, spilled_bytes = 0;
    bool any_put = false;                             // a put or put_batch was called
    bool md_set = false, has_groups = false;          // bwams_sorter_set_markdup: its table (copied) and options
    bwams_dup_groups groups;
    bwams_dup_opt_t opt{};
    bwams_depth_t *depth = nullptr;                   // bwams_sorter_set_depth: close adds the merged stream to it (the caller's handle)
    bwams_pileup_t *pileup = nullptr;                 // bwams_sorter_set_pileup: the same
    bwams_qc_t *qc = nullptr;                         // bwams_sorter_set_qc: the same
    bwams_recal_t *recal = nullptr;                   // bwams_sorter_set_recal: the same
    int64_t n_lib() const { return has_groups ? (int64_t)groups.libs.size() : 1; }
};

namespace {

void cleanup(bwams_sorter *s) {
    for (auto &r : s->runs)
        if (!r->path.empty()) ::unlink(r->path.c_str());
    if (s->fp) fclose(s->fp);
    if (s->def) bwams_deflater_destroy(s->def);
    delete s;
}

bool write_all(int fd, const void *p, int64_t n) {
    for (int64_t put = 0; put < n;) {
        const ssize_t k = ::write(fd, static_cast<const uint8_t *>(p) + put, (size_t)(n - put));
        if (k <= 0) return false;
        put += k;
    }
    return true;
}

// the checks of bwams_sorter_put on a run: sizes chain the records to n_bytes, keys in order, refIDs known, BAI-sized ends
int check_run(const bwams_sorter *s, const uint8_t *rec, int64_t n_bytes, const bwams_bam_coord_t *c, int64_t n) {
    int64_t at = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t sz = c[i].size;
        if (sz < 36 || sz > n_bytes - at || (int64_t)rd32(rec + at) + 4 != sz) return BWAMS_ERR_ARG;
        if (i && c[i].key < c[i - 1].key) return BWAMS_ERR_ARG;
        const uint32_t rid = (uint32_t)(c[i].key >> 32);
        if (rid != 0xFFFFFFFFu) {
            if (rid >= s->l_ref.size()) return BWAMS_ERR_ARG;
            if ((s->flags & BWAMS_SORT_BAI) && (int64_t)c[i].end > (int64_t)kMaxBai) return BWAMS_ERR_ARG;
        }
        at += sz;
    }
    return at == n_bytes ? BWAMS_OK : BWAMS_ERR_ARG;
}

// hand a checked run over: refused for a seq put before; kept in memory within mem_bytes, else spilled
int take_run(bwams_sorter *s, std::unique_ptr<Run> r) {
    const int64_t need = r->n_bytes + r->n_rec * 16 + (int64_t)r->tmpl.size() * 4;
    int64_t spill = -1;
    {
        std::lock_guard<std::mutex> g(s->mu);
        if (!s->seqs.insert(r->seq).second) return BWAMS_ERR_ARG;
        if (s->mem_used + need > s->mem_bytes) spill = s->n_spill++;
        else s->mem_used += need;
    }
    if (spill >= 0) {
        r->path = s->tmp_prefix + "." + std::to_string(spill) + ".run";
        const int fd = ::open(r->path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0600);
        const bool ok = fd >= 0 && write_all(fd, r->coords.data(), r->n_rec * 16) && write_all(fd, r->recs.get(), r->n_bytes) &&
                        write_all(fd, r->tmpl.data(), (int64_t)r->tmpl.size() * 4);
        if (fd >= 0) ::close(fd);
        r->recs.reset();
        r->coords = std::vector<bwams_bam_coord_t>();
        r->tmpl = std::vector<uint32_t>();
        std::lock_guard<std::mutex> g(s->mu);
        s->spilled_bytes += need;
        s->runs.push_back(std::move(r));               // its file is removed at close even when the write failed
        return ok ? BWAMS_OK : BWAMS_ERR_IO;
    }
    std::lock_guard<std::mutex> g(s->mu);
    s->runs.push_back(std::move(r));
    return BWAMS_OK;
}

// the members of gz[0, n): their sizes (BSIZE + 1) appended to *sizes
bool member_sizes(const uint8_t *gz, int64_t n, std::vector<int64_t> *sizes) {
    for (int64_t p = 0; p < n;) {
        if (n - p < 18 || gz[p] != 0x1f || gz[p + 1] != 0x8b) return false;
        const int64_t xlen = gz[p + 10] | gz[p + 11] << 8;
        int64_t bsize = -1;
        for (int64_t q = p + 12; q + 4 <= p + 12 + xlen;) {
            const int64_t slen = gz[q + 2] | gz[q + 3] << 8;
            if (gz[q] == 'B' && gz[q + 1] == 'C' && slen == 2) bsize = gz[q + 4] | gz[q + 5] << 8;
            q += 4 + slen;
        }
        if (bsize < 0) return false;
        sizes->push_back(bsize + 1);
        p += bsize + 1;
    }
    return true;
}

// bwams_sorter_set_depth, _set_pileup, _set_qc, _set_recal: handle h, a `kind` handle in the texts, goes into *slot; device gives the
// handle's, l_ref its reference lengths (null: it has none to compare)
template <class H>
int sorter_set(bwams_sorter_t *s, H *h, H *bwams_sorter::*slot, const char *who, const std::string &kind, int (*device)(const H *),
               const std::vector<int32_t> &(*l_ref)(const H *)) {
    const std::string why = !s || !h ? "a sorter and a " + kind + " handle are required"
                            : device(h) != s->device ? "the " + kind + " handle is on another device than the sorter"
                            : l_ref && l_ref(h) != s->l_ref ? "the " + kind + " handle's reference lengths are not the sorter header's" : "";
    if (!why.empty()) {
        bwams::set_last_error(std::string(who) + ": " + why);
        return BWAMS_ERR_ARG;
    }
    std::lock_guard<std::mutex> g(s->mu);
    if (s->any_put) {
        bwams::set_last_error(std::string(who) + ": called after the sorter's first put");
        return BWAMS_ERR_ARG;
    }
    s->*slot = h;
    return BWAMS_OK;
}

}  // namespace

extern "C" {

int bwams_sorter_open(const char *path, int device, const void *bam_header, int64_t n_header, const char *tmp_prefix, int64_t mem_bytes,
                      int32_t flags, bwams_sorter_t **out) {
    if (!path || !out || !bam_header || n_header < 12 || mem_bytes < 0 || (flags & ~(BWAMS_SORT_BAI | BWAMS_SORT_MARKDUP)) || device < 0) return BWAMS_ERR_ARG;
    *out = nullptr;
    const uint8_t *h = static_cast<const uint8_t *>(bam_header);
    if (memcmp(h, "BAM\1", 4) != 0) return BWAMS_ERR_ARG;
    std::vector<int32_t> l_ref;
    {                                                   // the header block's references, checked before any device work
        const int64_t l_text = (int32_t)rd32(h + 4);
        if (l_text < 0 || 12 + l_text > n_header) return BWAMS_ERR_ARG;
        int64_t p = 8 + l_text;
        const int64_t n_ref = (int32_t)rd32(h + p);
        p += 4;
        if (n_ref < 0) return BWAMS_ERR_ARG;
        for (int64_t i = 0; i < n_ref; ++i) {
            if (n_header - p < 4) return BWAMS_ERR_ARG;
            const int64_t l_name = (int32_t)rd32(h + p);
            if (l_name < 1 || n_header - p - 4 < l_name + 4) return BWAMS_ERR_ARG;
            const int32_t lr = (int32_t)rd32(h + p + 4 + l_name);
            if (lr < 0) return BWAMS_ERR_ARG;
            if ((flags & BWAMS_SORT_BAI) && (uint32_t)lr > kMaxBai) return BWAMS_ERR_UNSUPPORTED;
            l_ref.push_back(lr);
            p += 8 + l_name;
        }
        if (p != n_header) return BWAMS_ERR_ARG;
    }
    bwams_sorter *s = nullptr;
    try {
        s = new bwams_sorter();
        s->path = path;
        s->tmp_prefix = tmp_prefix ? std::string(tmp_prefix) : s->path + ".tmp";
        s->device = device;
        s->flags = flags;
        s->mem_bytes = mem_bytes;
        s->l_ref.swap(l_ref);
        if (int rc = bwams_deflater_create(device, 32 << 20, &s->def)) { s->def = nullptr; cleanup(s); return rc; }
        s->header_gz.resize((size_t)bwams_deflate_bound(n_header));
        int64_t got = 0;
        if (int rc = bwams_deflater_run(s->def, bam_header, n_header, 0, &s->header_gz[0], (int64_t)s->header_gz.size(), 0, 0, &got, nullptr)) {
            cleanup(s);
            return rc;
        }
        s->header_gz.resize((size_t)got);
        s->fp = fopen(path, "wb");
        if (!s->fp) { cleanup(s); return BWAMS_ERR_IO; }
        setvbuf(s->fp, nullptr, _IOFBF, 8 << 20);
    } catch (...) {
        if (s) cleanup(s);
        return BWAMS_ERR_NOMEM;
    }
    *out = s;
    return BWAMS_OK;
}

int bwams_sorter_put(bwams_sorter_t *s, int64_t seq, const void *records, int64_t n_bytes, const bwams_bam_coord_t *coords,
                     int64_t n_records) {
    if (!s || seq < 0 || n_bytes < 0 || n_records < 0 || (n_bytes && !records) || (n_records && !coords)) return BWAMS_ERR_ARG;
    { std::lock_guard<std::mutex> g(s->mu); s->any_put = true; }
    if (s->flags & BWAMS_SORT_MARKDUP) return BWAMS_ERR_ARG;            // sorted host records carry no template grouping
    const uint8_t *rec = static_cast<const uint8_t *>(records);
    if (int rc = check_run(s, rec, n_bytes, coords, n_records)) return rc;
    try {
        auto r = std::make_unique<Run>();
        r->seq = seq; r->n_rec = n_records; r->n_bytes = n_bytes;
        r->recs.reset(new uint8_t[(size_t)std::max<int64_t>(n_bytes, 1)]);
        if (n_bytes) memcpy(r->recs.get(), rec, (size_t)n_bytes);
        r->coords.assign(coords, coords + n_records);
        return take_run(s, std::move(r));
    } catch (...) {
        return BWAMS_ERR_NOMEM;
    }
}

int bwams_sorter_put_batch(bwams_sorter_t *s, int64_t seq, bwams_batch_t *b) {
    if (!s || !b || seq < 0) return BWAMS_ERR_ARG;
    int64_t n = 0, n_t = 0, n_e = 0;
    { std::lock_guard<std::mutex> g(s->mu); s->any_put = true; }
    if (int rc = bwams_bam_sort(b, &n)) return rc;
    const bool md = (s->flags & BWAMS_SORT_MARKDUP) != 0;
    if (md)
        if (int rc = s->md_set ? bwams_bam_templates2(b, s->has_groups ? &s->groups : nullptr, &n_t, &n_e) : bwams_bam_templates(b, &n_t, &n_e))
            return rc;
    try {
        auto r = std::make_unique<Run>();
        r->seq = seq; r->n_rec = n;
        r->coords.resize((size_t)n);
        if (int rc = bwams_bam_sorted_fetch(b, nullptr, 0, r->coords.data())) return rc;
        for (const bwams_bam_coord_t &c : r->coords) r->n_bytes += c.size;
        r->recs.reset(new uint8_t[(size_t)std::max<int64_t>(r->n_bytes, 1)]);
        if (int rc = bwams_bam_sorted_fetch(b, r->recs.get(), r->n_bytes, nullptr)) return rc;
        if (int rc = check_run(s, r->recs.get(), r->n_bytes, r->coords.data(), n)) return rc;
        if (md) {
            r->n_tmpl = n_t;
            r->ends.resize((size_t)n_e);
            r->tmpl.resize((size_t)n);
            if (int rc = bwams_bam_templates_fetch(b, r->ends.data(), n_e, r->tmpl.data(), 1)) return rc;
            if (s->md_set) {
                const int64_t n_lib = s->n_lib();
                r->loc.resize((size_t)n_e);
                r->rec_counts.resize((size_t)(2 * n_lib));
                if (int rc = bwams_bam_templates_fetch_loc(b, r->loc.data(), n_e)) return rc;
                if (int rc = bwams_bam_lib_record_counts(b, r->rec_counts.data(), r->rec_counts.data() + n_lib, n_lib)) return rc;
            }
        }
        return take_run(s, std::move(r));
    } catch (...) {
        return BWAMS_ERR_NOMEM;
    }
}

int bwams_sorter_close(bwams_sorter_t *s, bwams_sorter_stats_t *stats) { return bwams_sorter_close2(s, stats, nullptr); }

int bwams_sorter_close2(bwams_sorter_t *s, bwams_sorter_stats_t *stats, bwams_dup_stats_t *dup_stats) {
    return bwams_sorter_close3(s, stats, dup_stats, nullptr, 0);
}

int bwams_sorter_set_markdup(bwams_sorter_t *s, const bwams_dup_groups_t *groups, const bwams_dup_opt_t *opt) {
    if (!s || !(s->flags & BWAMS_SORT_MARKDUP)) return BWAMS_ERR_ARG;
    if (opt && (opt->optical_distance < 0 || opt->max_optical_set < 0)) return BWAMS_ERR_ARG;
    std::lock_guard<std::mutex> g(s->mu);
    if (s->any_put) return BWAMS_ERR_ARG;
    try {
        s->has_groups = groups != nullptr;
        s->groups = groups ? *groups : bwams_dup_groups();
    } catch (...) {
        return BWAMS_ERR_NOMEM;
    }
    s->opt = opt ? *opt : bwams_dup_opt_t{};
    s->md_set = true;
    return BWAMS_OK;
}

int bwams_sorter_set_depth(bwams_sorter_t *s, bwams_depth_t *d) {
    return sorter_set(s, d, &bwams_sorter::depth, "bwams_sorter_set_depth", "depth", bwams::depth_device, bwams::depth_l_ref);
}

int bwams_sorter_set_pileup(bwams_sorter_t *s, bwams_pileup_t *p) {
    return sorter_set(s, p, &bwams_sorter::pileup, "bwams_sorter_set_pileup", "pileup", bwams::pileup_device, bwams::pileup_l_ref);
}

int bwams_sorter_set_qc(bwams_sorter_t *s, bwams_qc_t *q) {
    return sorter_set<bwams_qc_t>(s, q, &bwams_sorter::qc, "bwams_sorter_set_qc", "QC", bwams::qc_device, nullptr);
}

int bwams_sorter_set_recal(bwams_sorter_t *s, bwams_recal_t *r) {
    return sorter_set(s, r, &bwams_sorter::recal, "bwams_sorter_set_recal", "recalibration", bwams::recal_device, bwams::recal_l_ref);
}

int bwams_sorter_close3(bwams_sorter_t *s, bwams_sorter_stats_t *stats, bwams_dup_stats_t *dup_stats, bwams_dup_lib_stats_t *lib_stats,
                        int64_t cap_lib) {
    if (!s) return BWAMS_ERR_ARG;
    if (lib_stats && cap_lib < s->n_lib()) return BWAMS_ERR_CAPACITY;
    for (int64_t l = 0; lib_stats && l < s->n_lib(); ++l) {                      // without BWAMS_SORT_MARKDUP the rows stay like this
        memset(&lib_stats[l], 0, sizeof lib_stats[l]);
        lib_stats[l].estimated_library_size = -1;
    }
    const Clock::time_point t_all = Clock::now();
    float ms_deflate = 0, ms_write = 0, ms_decide = 0;
    int rc = BWAMS_OK;
    int64_t n_records = 0, file_pos = 0, n_marked = 0;
    const bool md = (s->flags & BWAMS_SORT_MARKDUP) != 0;
    bwams_dup_stats_t dst;
    memset(&dst, 0, sizeof dst);
    try {
        std::vector<int64_t> base(s->runs.size(), 0);                           // markdup: each run's first template ordinal
        std::vector<uint8_t> dup;
        if (md) {
            const Clock::time_point t0 = Clock::now();
            std::vector<size_t> by_seq(s->runs.size());
            for (size_t k = 0; k < by_seq.size(); ++k) by_seq[k] = k;
            std::sort(by_seq.begin(), by_seq.end(), [&](size_t a, size_t b) { return s->runs[a]->seq < s->runs[b]->seq; });
            int64_t n_t = 0, n_e = 0;
            for (size_t k : by_seq) { base[k] = n_t; n_t += s->runs[k]->n_tmpl; n_e += (int64_t)s->runs[k]->ends.size(); }
            std::vector<bwams_dup_end_t> ends;
            std::vector<bwams_dup_loc_t> loc;
            ends.reserve((size_t)n_e);
            if (s->md_set) loc.reserve((size_t)n_e);
            for (size_t k : by_seq) {
                for (bwams_dup_end_t e : s->runs[k]->ends) { e.tmpl += base[k]; ends.push_back(e); }
                if (s->md_set) loc.insert(loc.end(), s->runs[k]->loc.begin(), s->runs[k]->loc.end());
            }
            dup.resize((size_t)std::max<int64_t>(n_t, 1));
            if (!s->md_set && !lib_stats) {
                rc = bwams_dup_decide(s->device, ends.data(), n_e, n_t, dup.data(), &dst);
            } else {                                                             // rules 11-13: the rows, and the totals from them
                const int64_t n_lib = s->n_lib();
                std::vector<bwams_dup_lib_stats_t> own((size_t)n_lib);
                bwams_dup_lib_stats_t *rows = lib_stats ? lib_stats : own.data();
                rc = bwams_dup_decide2(s->device, ends.data(), s->md_set ? loc.data() : nullptr, n_e, n_t, n_lib, &s->opt, dup.data(), nullptr,
                                       rows);
                for (int64_t l = 0; l < n_lib && !rc; ++l) {
                    for (auto &r : s->runs)
                        if (!r->rec_counts.empty()) {
                            rows[l].secondary_or_supplementary += r->rec_counts[(size_t)l];
                            rows[l].unmapped += r->rec_counts[(size_t)(n_lib + l)];
                        }
                    dst.unpaired_examined += rows[l].unpaired_examined; dst.unpaired_duplicates += rows[l].unpaired_duplicates;
                    dst.pairs_examined += rows[l].pairs_examined; dst.pair_duplicates += rows[l].pair_duplicates;
                }
            }
            dst.templates = n_t;
            ms_decide = ms_since(t0);
        }
        Clock::time_point t = Clock::now();
        if (fwrite(s->header_gz.data(), 1, s->header_gz.size(), s->fp) != s->header_gz.size()) rc = BWAMS_ERR_IO;
        ms_write += ms_since(t);
        file_pos = (int64_t)s->header_gz.size();
        std::vector<Cursor> cur(s->runs.size());
        using Head = std::pair<std::pair<uint64_t, int64_t>, size_t>;           // (key, seq), run
        std::priority_queue<Head, std::vector<Head>, std::greater<Head>> heap;
        for (size_t k = 0; k < s->runs.size() && !rc; ++k) {
            cur[k].r = s->runs[k].get();
            if (!s->runs[k]->path.empty() && (cur[k].fd = ::open(s->runs[k]->path.c_str(), O_RDONLY)) < 0) rc = BWAMS_ERR_IO;
            bwams_bam_coord_t c;
            if (!rc && cur[k].r->n_rec) {
                if (!cur[k].coord(&c)) rc = BWAMS_ERR_IO;
                else heap.push({{c.key, cur[k].r->seq}, k});
            }
        }
        Bai bai;
        bai.refs.resize(s->l_ref.size());
        struct Pending { uint64_t key; int32_t end; uint32_t flag; int64_t x, size; };
        std::vector<Pending> pend;
        size_t pend_done = 0;
        std::vector<int64_t> mcoff;                                              // file offset of every record member
        std::vector<uint8_t> buf((size_t)kPiece);
        std::vector<uint8_t> gz((size_t)bwams_deflate_bound(kPiece));
        std::vector<int64_t> sizes;
        int64_t fill = 0, flushed = 0;                                           // bytes in buf, record-stream bytes flushed
        // set_depth, set_pileup, set_qc, set_recal: the stream up to fed_at is handed on; whole_end is the end of the last record copied whole and open_end
        // that of the record being copied; carry holds stream bytes [fed_at, flushed) of the record that the last piece's end cut
        int64_t fed_at = 0, whole_end = 0, open_end = 0, carry_end = 0;
        std::vector<uint8_t> carry;
        auto consume = [&](const uint8_t *recs, int64_t n_bytes) -> int {        // whole records, to every consumer the sorter has
            if (s->depth)
                if (int e = bwams_depth_add_records(s->depth, recs, n_bytes, nullptr)) return e;
            if (s->pileup)
                if (int e = bwams_pileup_add_records(s->pileup, recs, n_bytes, nullptr)) return e;
            if (s->qc)
                if (int e = bwams_qc_add_records(s->qc, recs, n_bytes, nullptr)) return e;
            if (s->recal)
                if (int e = bwams_recal_add_records(s->recal, recs, n_bytes, nullptr)) return e;
            return BWAMS_OK;
        };
        auto feed = [&]() -> int {
            if (whole_end > fed_at) {
                int64_t from = fed_at;
                if (from < flushed) {                                            // the cut record ends in this piece
                    carry.insert(carry.end(), buf.data(), buf.data() + (carry_end - flushed));
                    if (int e = consume(carry.data(), (int64_t)carry.size())) return e;
                    carry.clear();
                    from = carry_end;
                }
                if (whole_end > from)
                    if (int e = consume(buf.data() + (from - flushed), whole_end - from)) return e;
                fed_at = whole_end;
            }
            if (flushed + fill > fed_at) {                                       // the piece ends inside a record
                const int64_t from = std::max(fed_at, flushed);
                carry.insert(carry.end(), buf.data() + (from - flushed), buf.data() + fill);
                carry_end = open_end;
            }
            return BWAMS_OK;
        };
        auto flush = [&]() -> int {
            if (fill == 0) return BWAMS_OK;
            if (s->depth || s->pileup || s->qc || s->recal)
                if (int e = feed()) return e;
            Clock::time_point t0 = Clock::now();
            int64_t got = 0;
            if (int e = bwams_deflater_run(s->def, buf.data(), fill, 0, gz.data(), (int64_t)gz.size(), 0, 0, &got, nullptr)) return e;
            ms_deflate += ms_since(t0);
            sizes.clear();
            if (!member_sizes(gz.data(), got, &sizes)) return BWAMS_ERR_DEVICE;
            for (int64_t sz : sizes) { mcoff.push_back(file_pos); file_pos += sz; }
            t0 = Clock::now();
            if (fwrite(gz.data(), 1, (size_t)got, s->fp) != (size_t)got) return BWAMS_ERR_IO;
            ms_write += ms_since(t0);
            flushed += fill;
            fill = 0;
            if (s->flags & BWAMS_SORT_BAI) {
                for (; pend_done < pend.size() && pend[pend_done].x + pend[pend_done].size <= flushed; ++pend_done) {
                    const Pending &q = pend[pend_done];
                    const int64_t y = q.x + q.size - 1;
                    bai.push(q.key, q.end, q.flag, (uint64_t)mcoff[(size_t)(q.x / kMember)] << 16 | (uint64_t)(q.x % kMember),
                             (uint64_t)mcoff[(size_t)(y / kMember)] << 16 | (uint64_t)(y % kMember + 1));
                }
                pend.erase(pend.begin(), pend.begin() + (std::ptrdiff_t)pend_done);
                pend_done = 0;
            }
            return BWAMS_OK;
        };
        int64_t x = 0;                                                           // record-stream offset of the next record
        while (!rc && !heap.empty()) {
            const size_t k = heap.top().second;
            heap.pop();
            Cursor &c = cur[k];
            bwams_bam_coord_t cd;
            const uint8_t *p = nullptr;
            if (!c.coord(&cd) || !(p = c.bytes(cd.size))) { rc = BWAMS_ERR_IO; break; }
            if (s->flags & BWAMS_SORT_BAI) pend.push_back({cd.key, cd.end, (uint32_t)(p[18] | p[19] << 8), x, cd.size});
            bool d = false;
            if (md) {
                uint32_t t = 0;
                if (!c.tmpl(&t)) { rc = BWAMS_ERR_IO; break; }
                d = dup[(size_t)(base[k] + t)] != 0;
                n_marked += d;
            }
            open_end = x + cd.size;
            for (int64_t done = 0; done < cd.size && !rc;) {                   // a record larger than the piece goes in parts
                const int64_t k2 = std::min<int64_t>(cd.size - done, kPiece - fill);
                memcpy(buf.data() + fill, p + done, (size_t)k2);
                if (md && done <= 19 && 19 < done + k2) {                      // FLAG's high byte: 0x400 is its bit 2
                    uint8_t &f = buf[(size_t)(fill + 19 - done)];
                    f = (uint8_t)((f & ~4u) | (d ? 4u : 0u));
                }
                fill += k2;
                done += k2;
                if (done == cd.size) whole_end = open_end;
                if (fill == kPiece) rc = flush();
            }
            x += cd.size;
            ++n_records;
            c.at += cd.size;
            if (++c.i < c.r->n_rec) {
                if (!c.coord(&cd)) rc = BWAMS_ERR_IO;
                else heap.push({{cd.key, c.r->seq}, k});
            }
        }
        if (!rc) rc = flush();
        for (Cursor &c : cur)
            if (c.fd >= 0) ::close(c.fd);
        t = Clock::now();
        if (!rc && fwrite(kBgzfEof, 1, sizeof kBgzfEof, s->fp) != sizeof kBgzfEof) rc = BWAMS_ERR_IO;
        file_pos += sizeof kBgzfEof;
        if (fclose(s->fp) && !rc) rc = BWAMS_ERR_IO;
        s->fp = nullptr;
        if (!rc && (s->flags & BWAMS_SORT_BAI)) {
            const std::string idx = bai.finish();
            FILE *f = fopen((s->path + ".bai").c_str(), "wb");
            if (!f || fwrite(idx.data(), 1, idx.size(), f) != idx.size()) rc = BWAMS_ERR_IO;
            if (f && fclose(f) && !rc) rc = BWAMS_ERR_IO;
        }
        ms_write += ms_since(t);
    } catch (...) {
        rc = BWAMS_ERR_NOMEM;
    }
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->runs = (int64_t)s->runs.size();
        stats->records = n_records;
        for (auto &r : s->runs) stats->spilled_runs += !r->path.empty();
        stats->spilled_bytes = s->spilled_bytes;
        stats->out_bytes = file_pos;
        stats->ms_deflate = ms_deflate;
        stats->ms_write = ms_write;
        stats->ms_merge = std::max(0.f, ms_since(t_all) - ms_deflate - ms_write - ms_decide);
    }
    if (dup_stats) {
        *dup_stats = dst;
        if (md) { dup_stats->records_marked = n_marked; dup_stats->ms_decide = ms_decide; }
    }
    cleanup(s);
    return rc;
}

}  // extern "C"
