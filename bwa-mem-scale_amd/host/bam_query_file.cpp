// bam_query_file.cpp — the file of a bwams_bam_file_t (include/bwams.h, "BAM file by region", rules 4 to 6): open (header block,
// index), the plan of a query, and the pieces: pread of an interval's whole BGZF members into page-locked staging, their headers
// walked here (BSIZE, ISIZE: the file is untrusted, every offset is checked against what was read), bwams_inflater_run into device
// memory behind the carried bytes.  No reader thread: profiles/bam_query.md has the read's share of a piece.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstring>

#include "bam_query.h"

namespace bwams {
namespace {

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The BGZF member at g[0, n): 0 with *total (the whole member) and *isize, 1 when n bytes do not hold it, -1 when it is no BGZF member.
int member_at(const uint8_t *g, int64_t n, int64_t *total, int64_t *isize) {
    if (n < 18) return 1;
    if (g[0] != 31 || g[1] != 139 || g[2] != 8 || !(g[3] & 4)) return -1;
    const int64_t xlen = g[10] | g[11] << 8;
    if (n < 12 + xlen) return 1;
    int64_t bsize = -1;
    for (int64_t q = 12; q + 4 <= 12 + xlen; q += 4 + (g[q + 2] | g[q + 3] << 8))
        if (g[q] == 'B' && g[q + 1] == 'C' && (g[q + 2] | g[q + 3] << 8) == 2 && q + 6 <= 12 + xlen) { bsize = g[q + 4] | g[q + 5] << 8; break; }
    if (bsize < 0 || bsize + 1 < 12 + xlen + 8) return -1;
    *total = bsize + 1;
    if (n < *total) return 1;
    const uint8_t *t = g + *total - 4;
    *isize = (int64_t)((uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24);
    return 0;
}

bool read_file(const std::string &path, std::vector<uint8_t> *out) {
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) return false;
    struct stat st;
    bool ok = fstat(fd, &st) == 0;
    if (ok) {
        out->resize((size_t)st.st_size);
        int64_t got = 0;
        while (ok && got < (int64_t)out->size()) {
            const ssize_t k = pread(fd, out->data() + got, out->size() - (size_t)got, got);
            if (k <= 0) ok = false;
            else got += k;
        }
    }
    ::close(fd);
    return ok;
}

}  // namespace

BamFileHost::~BamFileHost() {
    if (inf) bwams_inflater_destroy(inf);
    if (stage) bwams_host_free(stage);
    if (fd >= 0) ::close(fd);
}

int BamFileHost::open(const char *path_, const char *bai_path, int device, int64_t piece, std::string *err) {
    path = path_;
    piece_bytes = piece;
    fd = ::open(path_, O_RDONLY);
    struct stat st;
    if (fd < 0 || fstat(fd, &st) != 0) { *err = path + ": cannot be opened"; return BWAMS_ERR_IO; }
    file_size = (int64_t)st.st_size;
    // stored members are their data + 26 bytes; room for one member more than the inflated bytes a piece holds
    stage_cap = piece_bytes + (piece_bytes / 65280 + 2) * 64 + 65536;
    if (int rc = bwams_host_alloc((size_t)stage_cap, reinterpret_cast<void **>(&stage))) { *err = bwams_last_error(); return rc; }
    if (int rc = bwams_inflater_create(device, stage_cap, std::max<int64_t>(piece_bytes, 65536), &inf)) { *err = bwams_last_error(); return rc; }
    // the header block: a member at a time, inflated to the host, so that the first record's virtual offset is known
    std::vector<int64_t> coff, ustart;
    int64_t file_at = 0, u_at = 0;
    std::vector<char> hb;
    std::vector<uint8_t> one(65536);
    const int rc = bam_header_read(
        [&](char *dst, int64_t want, std::string &e) -> int64_t {
            while (file_at < file_size) {
                const int64_t n = std::min<int64_t>(65536, file_size - file_at);
                if (pread(fd, stage, (size_t)n, file_at) != (ssize_t)n) { e = path + ": read error at byte " + std::to_string(file_at); return BWAMS_ERR_IO; }
                int64_t total = 0, isize = 0;
                const int m = member_at(stage, n, &total, &isize);
                if (m < 0) { e = path + ": not BGZF at byte " + std::to_string(file_at); return BWAMS_ERR_UNSUPPORTED; }
                if (m > 0) { e = path + ": the file ends inside the BGZF member at byte " + std::to_string(file_at); return BWAMS_ERR_IO; }
                if (isize > 65536 || isize > want) { e = path + ": BGZF member at byte " + std::to_string(file_at) + ": ISIZE " + std::to_string(isize); return BWAMS_ERR_IO; }
                int64_t used = 0, got = 0;
                if (int r = bwams_inflater_run(inf, stage, total, one.data(), 65536, 0, &used, &got, nullptr)) { e = path + ": " + bwams_last_error(); return r; }
                if (used != total || got != isize) { e = path + ": BGZF member at byte " + std::to_string(file_at) + " did not inflate"; return BWAMS_ERR_IO; }
                coff.push_back(file_at);
                ustart.push_back(u_at);
                file_at += total;
                u_at += isize;
                if (isize == 0) continue;                    // an empty member: the next one
                memcpy(dst, one.data(), (size_t)isize);
                return isize;
            }
            return 0;
        },
        65536, &hb, &hdr, err);
    if (rc) return rc;
    header_block.assign(hb.begin(), hb.begin() + (std::ptrdiff_t)hdr.end);
    // the first record: in the member that holds byte hdr.end, or at the start of the one behind the members read
    first_voff = (uint64_t)file_at << 16;
    for (size_t k = 0; k < coff.size(); ++k) {
        const int64_t u_end = k + 1 < coff.size() ? ustart[k + 1] : u_at;
        if ((int64_t)hdr.end >= ustart[k] && (int64_t)hdr.end < u_end) { first_voff = (uint64_t)coff[k] << 16 | (uint64_t)((int64_t)hdr.end - ustart[k]); break; }
    }
    // the index: the named one, else <path>.bai when it is there
    std::vector<uint8_t> raw;
    std::string ip = bai_path ? bai_path : path + ".bai";
    if (read_file(ip, &raw)) {
        if (int r = bai_parse(raw.data(), (int64_t)raw.size(), &bai, err)) { *err = ip + ": " + *err; return r; }
        if ((int64_t)bai.refs.size() != hdr.n_ref) {
            *err = ip + ": the index has " + std::to_string(bai.refs.size()) + " references, the BAM header " + std::to_string(hdr.n_ref);
            return BWAMS_ERR_IO;
        }
        has_index = true;
    } else if (bai_path) {
        *err = ip + ": cannot be read";
        return BWAMS_ERR_IO;
    }
    return BWAMS_OK;
}

int BamFileHost::query(const bwams_pileup_region_t *regions, int32_t n_regions, std::vector<bwams_pileup_region_t> *merged, std::string *err) {
    merged->clear();
    if (n_regions < 0 || (n_regions && !regions)) { *err = "n_regions >= 0 regions are required"; return BWAMS_ERR_ARG; }
    if (n_regions && !has_index) { *err = "a region query needs an index, and " + path + " was opened without one"; return BWAMS_ERR_ARG; }
    if (int rc = regions_merge(regions, n_regions, hdr.n_ref, merged, err)) return rc;
    if (n_regions == 0) {                                    // rule 4: from the first record to the end of the data
        iv_beg.assign(1, first_voff);
        iv_end.assign(1, (uint64_t)file_size << 16);
        if (iv_beg[0] >= iv_end[0]) { iv_beg.clear(); iv_end.clear(); }
    } else {
        bai_plan(bai, *merged, &iv_beg, &iv_end);
    }
    iv = 0;
    at = -1;
    return BWAMS_OK;
}

int BamFileHost::next_piece(void *dev_out, BamPiece *p, std::string *err) {
    *p = BamPiece{};
    const int64_t coff_b = (int64_t)(iv_beg[iv] >> 16), uoff_b = (int64_t)(iv_beg[iv] & 0xFFFF);
    const int64_t coff_e = (int64_t)(iv_end[iv] >> 16), uoff_e = (int64_t)(iv_end[iv] & 0xFFFF);
    auto bad = [&](int64_t off, const std::string &why) {
        *err = path + ": interval " + std::to_string(iv) + " of the plan, file offset " + std::to_string(off) + ": " + why;
        return BWAMS_ERR_IO;
    };
    // a chunk's end with an in-member offset names a member that must lie inside the file; one without ends in front of coff_e
    if (coff_b >= file_size || coff_e > file_size || (uoff_e > 0 && coff_e >= file_size) || coff_e < coff_b)
        return bad(coff_e > file_size || (uoff_e > 0 && coff_e >= file_size) ? coff_e : coff_b,
                   "a chunk of the index points past the file (" + std::to_string(file_size) + " bytes)");
    p->first = at < 0;
    if (p->first) at = coff_b;
    p->file_off = at;
    p->start = p->first ? uoff_b : 0;
    const int64_t limit = std::min(file_size, uoff_e > 0 ? coff_e + 65536 : coff_e);
    const int64_t want = std::min(stage_cap, limit - at);
    double t0 = now_ms();
    int64_t got = 0;
    while (got < want) {
        const ssize_t k = pread(fd, stage + got, (size_t)(want - got), at + got);
        if (k < 0) return bad(at + got, "read error");
        if (k == 0) break;
        got += k;
    }
    p->ms_read = (float)(now_ms() - t0);
    int64_t q = 0, out = 0;
    while (!p->last) {
        if (at + q == coff_e && uoff_e == 0) { p->last = true; p->stop = out; break; }
        if (at + q > coff_e) return bad(at + q, "the chunk's end (file offset " + std::to_string(coff_e) + ") is not the start of a BGZF member");
        int64_t total = 0, isize = 0;
        const int m = member_at(stage + q, got - q, &total, &isize);
        if (m < 0) return bad(at + q, "not a BGZF member");
        if (m > 0) {
            if (p->members) break;                           // cut off by the staging buffer: the next piece
            return bad(at + q, "the file ends inside a BGZF member");
        }
        if (isize > 65536) return bad(at + q, "ISIZE " + std::to_string(isize) + " is over 65536");
        if (out + isize > piece_bytes) break;
        if (p->first && p->members == 0 && uoff_b > isize) return bad(at + q, "the chunk starts at byte " + std::to_string(uoff_b) + " of a member of " + std::to_string(isize));
        if (at + q == coff_e) {                              // the interval's last member
            if (uoff_e > isize) return bad(at + q, "the chunk ends at byte " + std::to_string(uoff_e) + " of a member of " + std::to_string(isize));
            p->last = true;
            p->stop = out + uoff_e;
        }
        q += total;
        out += isize;
        ++p->members;
    }
    p->n_in = q;
    if (q) {
        t0 = now_ms();
        int64_t used = 0;
        if (int rc = bwams_inflater_run(inf, stage, q, dev_out, piece_bytes, 1, &used, &p->n_out, nullptr)) {
            *err = path + ": piece at file offset " + std::to_string(at) + ": " + bwams_last_error();
            return rc == BWAMS_ERR_IO || rc == BWAMS_ERR_UNSUPPORTED ? BWAMS_ERR_IO : rc;
        }
        p->ms_inflate = (float)(now_ms() - t0);
        if (used != q || p->n_out != out) return bad(at, "its members did not inflate to the sizes their trailers name");
    }
    at += q;
    if (p->last) { ++iv; at = -1; }
    return BWAMS_OK;
}

}  // namespace bwams
