// fastq_io.cpp — the file ends of the pipeline around mem_process_seqs(): a reader thread that inflates a (gz or plain) FASTQ / FASTA
// file into page-locked chunk buffers cut where bseq_read_orig cuts its chunks, and a writer thread per output shard.
//
// Reference: kt_pipeline's step 0 is bseq_read_orig (/root/reference/src/bwa.cpp:266-335) over kseq_read on a gzFile — records are read
// until the chunk holds chunk_size BASES (and, for interleaved pairs, an even number of reads), one reader, inflate and parse on the
// same thread; step 2 is fputs() of every work item's string to ONE stream (src/fastmap.cpp:437-461).  Here:
//   * bwams_reader: a background thread inflates (zlib's gzread: gz and plain text alike) into a ring of page-locked buffers
//     (bwams_host_alloc: the chunk then goes up at the link's rate, or is parsed in place) and cuts chunks at the same records — the
//     records are found by lines with kseq_read's grammar (header; sequence lines up to the '+' line; quality lines until the quality is
//     as long as the sequence; '>' records without quality), so chunk i of this reader holds exactly the reads of chunk i of the
//     reference's with the same -K.  Reading chunk i + 1 overlaps whatever the caller does with chunk i.
//   * bwams_writer: one output stream per shard (per GPU: "<prefix>.<s>.sam", or a single file), each with a thread that writes the
//     texts handed to it in sequence-number order — a shard's file is in read order; concatenating the shards' files of a job that gave
//     shard s the s-th contiguous slice of every chunk is NOT read order across chunks (that is what the single-stream form is for).
//   * where the text comes from is a Source: zlib's gzread (bwams_reader_open, and bwams_reader_open_device on any file that is not
//     BGZF), plain gzip inflated on a GPU (bwams_reader_open_device2 with BWAMS_READER_GUNZIP: bwams_gunzip_run), or BGZF members
//     inflated on a GPU (bwams_reader_open_device: read(2) into page-locked staging, bwams_inflater_run into
//     the chunk buffer behind the carried bytes).  The cut loop is the same for both, so their chunks are the same bytes.
//   * bwams_reader_open_bam: the same Sources under a BAM file.  Open parses the header block on the caller's thread; the reader's
//     thread then cuts chunks of whole BAM records, hopping along block_size where the text loop scans lines (one_bam_record), with
//     the same cut.  Such chunks go to bwams_process_chunk_bam; bwams_bseq_parse below stays FASTQ-only.
// Host C++ only.  zlib is the reference's own dependency for this step (Makefile: -lz).
#include <fcntl.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "bwams.h"
#include "bam_query.h"

namespace {

struct Chunk {
    char *buf = nullptr;          // page-locked, cap bytes
    int64_t cap = 0, n_bytes = 0, n_reads = 0, n_bases = 0;
    bool eof = false;
};

// One record of kseq_read's grammar starting at p (a '@' or '>' line) in [p, end): returns the position behind the record (the start
// of the next header, blank lines skipped) or -1 when the text ends inside the record (more input is needed); *bases = its l_seq.
// `final`: the input has ended, so a record that runs to the end of the text is complete.  -2: text the grammar does not start a
// record with (the serial reader would scan it byte by byte).
int64_t one_record(const char *t, int64_t p, int64_t end, bool final, int64_t *bases) {
    auto line_end = [&](int64_t a) -> int64_t {
        const void *q = memchr(t + a, '\n', (size_t)(end - a));
        return q ? (const char *)q - t : -1;
    };
    if (t[p] != '@' && t[p] != '>') return -2;
    int64_t e = line_end(p);
    if (e < 0) { if (!final) return -1; *bases = 0; return end; }
    int64_t a = e + 1, l_seq = 0;
    bool plus = false;
    while (a < end) {                                   // sequence lines
        const char c = t[a];
        if (c == '\n') { ++a; continue; }
        if (c == '+') { plus = true; break; }
        if (c == '>' || c == '@') break;
        e = line_end(a);
        int64_t le = e < 0 ? end : e;
        if (e < 0 && !final) return -1;
        int64_t len = le - a;
        if (len > 0 && l_seq + len > 1 && t[le - 1] == '\r') --len;
        l_seq += len;
        a = e < 0 ? end : e + 1;
    }
    if (a >= end && !final) return -1;                  // the next line may still belong to the record
    *bases = l_seq;
    if (!plus) return a;                                // FASTA-like record (or the end of the text)
    e = line_end(a);                                    // the '+' line
    if (e < 0) return final ? -2 : -1;
    a = e + 1;
    int64_t l_qual = 0;
    do {
        if (a >= end) return final ? -2 : -1;           // truncated quality (kseq_read's -2)
        e = line_end(a);
        if (e < 0 && !final) return -1;
        const int64_t le = e < 0 ? end : e;
        int64_t len = le - a;
        if (len > 0 && l_qual + len > 1 && t[le - 1] == '\r') --len;
        l_qual += len;
        a = e < 0 ? end : e + 1;
    } while (l_qual < l_seq);
    if (l_qual != l_seq) return -2;
    while (a < end && (t[a] == '\n' || (t[a] == '\r' && a + 1 < end && t[a + 1] == '\n'))) a += t[a] == '\n' ? 1 : 2;   // blank lines
    if (a >= end && !final) return -1;                  // (whether blank lines or the next header follow is not known yet)
    return a;
}

// One BAM record at p in [p, end) (rule 1 of bwams_bam_reads_decode, include/bwams.h): the position behind it, -1 when more input is
// needed, -2 when no well-formed record starts here.  *kept: FLAG has neither 0x100 nor 0x800; *bases: its l_seq; *size: 4 + block_size
// once that is known (the caller tells a record larger than its buffer from one the file cuts off).
int64_t one_bam_record(const char *t, int64_t p, int64_t end, bool *kept, int64_t *bases, int64_t *size) {
    const unsigned char *u = reinterpret_cast<const unsigned char *>(t) + p;
    auto u32 = [&](int at) { return (uint32_t)u[at] | (uint32_t)u[at + 1] << 8 | (uint32_t)u[at + 2] << 16 | (uint32_t)u[at + 3] << 24; };
    *size = 0;
    if (p + 4 > end) return -1;
    const int64_t block_size = u32(0);
    if (block_size < 32) return -2;
    *size = 4 + block_size;
    if (p + 36 > end) return -1;
    const int64_t l_name = u[12], n_cig = u[16] | u[17] << 8, flag = u[18] | u[19] << 8, l_seq = (int32_t)u32(20);
    if (l_name < 1 || l_seq < 0 || 32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq > block_size) return -2;
    if (p + 4 + block_size > end) return -1;
    if (u[35 + l_name] != 0) return -2;
    *kept = !(flag & 0x900);
    *bases = l_seq;
    return p + 4 + block_size;
}

using Clock = std::chrono::steady_clock;
float ms_since(Clock::time_point t0) { return std::chrono::duration<float, std::milli>(Clock::now() - t0).count(); }

// The reader's text: read() puts up to `want` bytes at dst and returns how many, 0 at the end of the file, < 0 on an error (err says
// what).  `step`: the most one read() is asked for.
struct Source {
    int64_t step = 8 << 20;
    bwams_reader_stats_t st{};
    virtual ~Source() {}
    virtual int64_t read(char *dst, int64_t want, std::string &err) = 0;
};

struct ZlibSource : Source {
    gzFile fp = nullptr;
    ~ZlibSource() override { if (fp) gzclose(fp); }
    int64_t read(char *dst, int64_t want, std::string &err) override {
        const auto t0 = Clock::now();
        const int got = gzread(fp, dst, (unsigned)want);
        st.ms_inflate += ms_since(t0);
        if (got < 0) { int e_ = 0; err = gzerror(fp, &e_); return BWAMS_ERR_IO; }
        st.out_bytes += got;
        st.in_bytes = gzoffset(fp);
        return got;
    }
};

// BGZF: compressed bytes by read(2) into page-locked staging, whole members inflated on the GPU into the chunk buffer.  A request
// smaller than a member (the chunk buffer's last bytes) is served from one member inflated into `spill`.
struct BgzfSource : Source {
    std::string path;
    int fd = -1;
    bwams_inflater_t *inf = nullptr;
    char *zbuf = nullptr;                                  // page-locked
    int64_t zcap = 0, zpos = 0, zend = 0;
    bool file_end = false;
    std::vector<char> spill = std::vector<char>(65536);
    int64_t spill_pos = 0, spill_end = 0;
    ~BgzfSource() override {
        if (inf) bwams_inflater_destroy(inf);
        if (zbuf) bwams_host_free(zbuf);
        if (fd >= 0) close(fd);
    }
    int64_t read(char *dst, int64_t want, std::string &err) override {
        if (spill_pos < spill_end) {
            const int64_t n = std::min(want, spill_end - spill_pos);
            memcpy(dst, spill.data() + spill_pos, (size_t)n);
            spill_pos += n;
            return n;
        }
        for (;;) {
            if (zend > zpos) {
                const bool direct = want >= (int64_t)spill.size();
                int64_t used = 0, n_out = 0;
                const auto t0 = Clock::now();
                const int rc = bwams_inflater_run(inf, reinterpret_cast<const uint8_t *>(zbuf + zpos), zend - zpos, direct ? dst : spill.data(),
                                                  direct ? want : (int64_t)spill.size(), 0, &used, &n_out, nullptr);
                st.ms_inflate += ms_since(t0);
                if (rc) { err = path + ": " + bwams_last_error(); return rc; }
                if (used) {
                    zpos += used;
                    st.out_bytes += n_out;
                    if (n_out == 0) continue;                      // EOF members only
                    if (direct) return n_out;
                    spill_pos = 0;
                    spill_end = n_out;
                    return read(dst, want, err);
                }
            }
            if (file_end) {
                if (zend > zpos) { err = path + ": the file ends inside a BGZF member"; return BWAMS_ERR_IO; }
                return 0;
            }
            memmove(zbuf, zbuf + zpos, (size_t)(zend - zpos));
            zend -= zpos;
            zpos = 0;
            const auto t0 = Clock::now();
            const ssize_t got = ::read(fd, zbuf + zend, (size_t)(zcap - zend));
            st.ms_read += ms_since(t0);
            if (got < 0) { err = path + ": read failed"; return BWAMS_ERR_IO; }
            if (got == 0) file_end = true;
            zend += got;
            st.in_bytes += got;
        }
    }
};

// Plain gzip: compressed bytes by read(2) into page-locked staging, bwams_gunzip_run into the chunk buffer.  A call consumes whole
// bytes up to a block boundary; the rest is presented again with what the file gives next.  A request smaller than a piece may
// inflate to (kSpill bytes) is served from `spill`.
struct GunzipSource : Source {
    static constexpr int64_t kSpill = 4 << 20;
    std::string path;
    int fd = -1;
    bwams_gunzip_t *gun = nullptr;
    char *zbuf = nullptr;                                  // page-locked
    int64_t zcap = 0, zpos = 0, zend = 0;
    bool file_end = false, done = false;
    std::vector<char> spill = std::vector<char>((size_t)kSpill);
    int64_t spill_pos = 0, spill_end = 0;
    ~GunzipSource() override {
        if (gun) bwams_gunzip_destroy(gun);
        if (zbuf) bwams_host_free(zbuf);
        if (fd >= 0) close(fd);
    }
    int64_t read(char *dst, int64_t want, std::string &err) override {
        if (spill_pos < spill_end) {
            const int64_t n = std::min(want, spill_end - spill_pos);
            memcpy(dst, spill.data() + spill_pos, (size_t)n);
            spill_pos += n;
            return n;
        }
        for (;;) {
            if (done) return 0;
            if (zend > zpos || file_end) {
                const bool direct = want >= kSpill;
                int64_t used = 0, n_out = 0;
                const auto t0 = Clock::now();
                int rc = bwams_gunzip_run(gun, reinterpret_cast<const uint8_t *>(zbuf + zpos), zend - zpos, file_end, direct ? dst : spill.data(),
                                          direct ? want : kSpill, 0, &used, &n_out, nullptr);
                st.ms_inflate += ms_since(t0);
                if (rc == BWAMS_ERR_CAPACITY && direct && want < step) {       // the chunk buffer's last bytes: through the spill
                    rc = bwams_gunzip_run(gun, reinterpret_cast<const uint8_t *>(zbuf + zpos), zend - zpos, file_end, spill.data(), kSpill, 0,
                                          &used, &n_out, nullptr);
                    if (!rc && n_out) {
                        zpos += used;
                        st.out_bytes += n_out;
                        spill_pos = 0;
                        spill_end = n_out;
                        return read(dst, want, err);
                    }
                }
                if (rc) {
                    err = path + ": " + bwams_last_error();
                    if (rc == BWAMS_ERR_CAPACITY) err += " (open the file without BWAMS_READER_GUNZIP)";
                    return rc;
                }
                zpos += used;
                st.out_bytes += n_out;
                if (n_out) {
                    if (direct) return n_out;
                    spill_pos = 0;
                    spill_end = n_out;
                    return read(dst, want, err);
                }
                if (file_end && used == 0) { done = true; return 0; }
                if (used) continue;
            }
            if (zpos == 0 && zend == zcap) { err = path + ": no DEFLATE block boundary inside the staging buffer (open the file without BWAMS_READER_GUNZIP)"; return BWAMS_ERR_CAPACITY; }
            memmove(zbuf, zbuf + zpos, (size_t)(zend - zpos));
            zend -= zpos;
            zpos = 0;
            const auto t0 = Clock::now();
            const ssize_t got = ::read(fd, zbuf + zend, (size_t)(zcap - zend));
            st.ms_read += ms_since(t0);
            if (got < 0) { err = path + ": read failed"; return BWAMS_ERR_IO; }
            if (got == 0) file_end = true;
            zend += got;
            st.in_bytes += got;
        }
    }
};

// the first two bytes of a gzip file
bool is_gzip(const char *path) {
    unsigned char h[2];
    FILE *fp = fopen(path, "rb");
    if (!fp) return false;
    const size_t n = fread(h, 1, sizeof h, fp);
    fclose(fp);
    return n == 2 && h[0] == 31 && h[1] == 139;
}

// the first bytes of a BGZF file: a gzip header with FEXTRA only and a 'BC' subfield
bool is_bgzf(const char *path) {
    unsigned char h[64];
    FILE *fp = fopen(path, "rb");
    if (!fp) return false;
    const size_t n = fread(h, 1, sizeof h, fp);
    fclose(fp);
    if (n < 18 || h[0] != 31 || h[1] != 139 || h[2] != 8 || h[3] != 4) return false;
    const size_t xend = 12 + (size_t)(h[10] | h[11] << 8);
    for (size_t q = 12; q + 4 <= xend && q + 6 <= n; q += 4 + (size_t)(h[q + 2] | h[q + 3] << 8))
        if (h[q] == 'B' && h[q + 1] == 'C' && (h[q + 2] | h[q + 3] << 8) == 2) return true;
    return false;
}

}  // namespace

struct bwams_reader {
    std::unique_ptr<Source> src;
    int64_t chunk_bases = 0;
    int paired = 0;
    std::vector<Chunk> ring;
    std::deque<int> free_q, ready_q;
    std::mutex mu;
    std::condition_variable cv;
    std::thread th;
    bool stop = false, done = false;
    int rc = BWAMS_OK;
    std::string err;
    // carry: bytes inflated but not yet part of a chunk
    std::vector<char> carry;
    bwams_reader_stats_t stats{};                       // src->st as of the last read, under stat_mu
    bool bam = false;                                   // bwams_reader_open_bam: chunks of BAM records
    std::string bam_text;                               // its header text,
    int32_t bam_n_ref = 0;                              // the number of references,
    int64_t bam_records = 0;                            // and the records cut so far (the ordinal in an error text)
    mutable std::mutex stat_mu;
};

static void reader_main(bwams_reader *r) {
    bool file_end = false;
    for (;;) {
        int slot = -1;
        {
            std::unique_lock<std::mutex> g(r->mu);
            r->cv.wait(g, [r] { return r->stop || !r->free_q.empty(); });
            if (r->stop) break;
            slot = r->free_q.front();
            r->free_q.pop_front();
        }
        Chunk &c = r->ring[(size_t)slot];
        int64_t have = (int64_t)r->carry.size();
        if (have > c.cap) { r->rc = BWAMS_ERR_CAPACITY; r->err = "a record larger than the chunk buffer"; }
        if (have) memcpy(c.buf, r->carry.data(), (size_t)have);
        r->carry.clear();
        int64_t pos = 0, reads = 0, bases = 0;
        bool full = false;
        while (!full && !r->rc) {
            // parse what is there
            while (r->bam && pos < have) {                                   // BAM: hop along block_size
                bool kept = false;
                int64_t b = 0, size = 0;
                const int64_t nx = one_bam_record(c.buf, pos, have, &kept, &b, &size);
                if (nx == -1) {
                    if (size > c.cap - 1) { r->rc = BWAMS_ERR_CAPACITY; r->err = "a record larger than the chunk buffer"; }
                    break;
                }
                if (nx == -2) { r->rc = BWAMS_ERR_IO; r->err = "BAM record " + std::to_string(r->bam_records) + " is not well formed"; break; }
                pos = nx; ++r->bam_records;
                if (!kept) continue;
                ++reads; bases += b;
                if (bases >= r->chunk_bases && (!r->paired || (reads & 1) == 0)) { full = true; break; }     // the same cut, after a kept record
            }
            while (!r->bam && pos < have) {
                if (c.buf[pos] == '\n') { ++pos; continue; }                 // blank lines in front of a header
                int64_t b = 0;
                const int64_t nx = one_record(c.buf, pos, have, file_end, &b);
                if (nx == -1) break;
                if (nx == -2) { r->rc = BWAMS_ERR_UNSUPPORTED; r->err = "text that is not FASTQ / FASTA records near byte " + std::to_string(pos) + " of a chunk"; break; }
                pos = nx; ++reads; bases += b;
                if (bases >= r->chunk_bases && (!r->paired || (reads & 1) == 0)) { full = true; break; }     // bseq_read_orig's cut
            }
            if (full || r->rc || (file_end && pos >= have)) break;
            if (file_end) {                                                  // an incomplete last record
                if (pos < have) { r->rc = BWAMS_ERR_IO; r->err = "the file ends inside a record"; }
                break;
            }
            if (have >= c.cap - 1) { r->rc = BWAMS_ERR_CAPACITY; r->err = "chunk buffer too small for " + std::to_string(r->chunk_bases) + " bases of records"; break; }
            const int64_t want = std::min<int64_t>(c.cap - 1 - have, r->src->step);      // one byte of slack: bwams_bseq_parse may put a NUL behind the text
            int64_t got;
            {
                std::string e_;
                got = r->src->read(c.buf + have, want, e_);
                std::lock_guard<std::mutex> g(r->stat_mu);
                r->stats = r->src->st;
                if (got < 0) { r->rc = (int)got; r->err = e_; break; }
            }
            if (got == 0) file_end = true;
            have += got;
        }
        c.n_bytes = pos; c.n_reads = reads; c.n_bases = bases;
        c.eof = file_end && pos >= have && reads == 0;
        if (!r->rc && have > pos) r->carry.assign(c.buf + pos, c.buf + have);
        {
            std::lock_guard<std::mutex> g(r->mu);
            r->ready_q.push_back(slot);
            if (r->rc || c.eof) r->done = true;
        }
        r->cv.notify_all();
        if (r->rc || c.eof) break;
    }
}

int bwams_reader_close(bwams_reader_t *r) {
    if (!r) return BWAMS_OK;
    {
        std::lock_guard<std::mutex> g(r->mu);
        r->stop = true;
    }
    r->cv.notify_all();
    if (r->th.joinable()) r->th.join();
    for (Chunk &c : r->ring) if (c.buf) bwams_host_free(c.buf);
    delete r;
    return BWAMS_OK;
}

static int reader_start(bwams_reader *r, int64_t chunk_bases, int32_t paired, int64_t buffer_bytes, int32_t n_buffers) {
    r->chunk_bases = chunk_bases;
    r->paired = paired;
    // a record of 150 bases is ~ 320 bytes of text: 2.6 bytes per base and room for the record that crosses the limit
    const int64_t cap = buffer_bytes > 0 ? buffer_bytes : chunk_bases * 3 + (64 << 20);
    r->ring.resize((size_t)n_buffers);
    for (int i = 0; i < n_buffers; ++i) {
        void *p = nullptr;
        if (int rc = bwams_host_alloc((size_t)cap, &p)) return rc;
        r->ring[(size_t)i].buf = static_cast<char *>(p);
        r->ring[(size_t)i].cap = cap;
        r->free_q.push_back(i);
    }
    r->th = std::thread(reader_main, r);
    return BWAMS_OK;
}

static int zlib_source(const char *path, std::unique_ptr<Source> *out) {
    auto z = std::unique_ptr<ZlibSource>(new ZlibSource());
    z->fp = gzopen(path, "rb");
    if (!z->fp) return BWAMS_ERR_IO;
    gzbuffer(z->fp, 1 << 20);
    *out = std::move(z);
    return BWAMS_OK;
}

// The Source of bwams_reader_open_device: BGZF members inflated on `device`, anything else through zlib
static int device_source(const char *path, int device, std::unique_ptr<Source> *out, uint32_t flags = 0) {
    constexpr int64_t kIn = 32 << 20, kOut = 64 << 20;     // one call: up to 32 MiB of members, 64 MiB of text
    if (device >= 0 && (flags & BWAMS_READER_GUNZIP) && !is_bgzf(path) && is_gzip(path)) {
        // a call's parallelism is its pieces: 32 MiB of gzip in pieces of 32 KiB (a zlib block of FASTQ is some 20 KB) is a
        // thousand decoders, and some 60 MiB of FASTQ text (a call takes the pieces whose text fits kOut)
        constexpr int64_t kGzIn = 32 << 20;
        constexpr int32_t kPiece = 32 << 10;
        auto b = std::unique_ptr<GunzipSource>(new GunzipSource());
        b->path = path;
        b->st.device_inflate = 2;
        b->step = kOut;
        b->fd = open(path, O_RDONLY);
        if (b->fd < 0) return BWAMS_ERR_IO;
        if (int rc = bwams_host_alloc((size_t)kGzIn, reinterpret_cast<void **>(&b->zbuf))) return rc;
        b->zcap = kGzIn;
        if (int rc = bwams_gunzip_create(device, kGzIn, kOut, kPiece, &b->gun)) return rc;
        *out = std::move(b);
        return BWAMS_OK;
    }
    if (device < 0 || !is_bgzf(path)) return zlib_source(path, out);
    auto b = std::unique_ptr<BgzfSource>(new BgzfSource());
    b->path = path;
    b->st.device_inflate = 1;
    b->step = kOut;
    b->fd = open(path, O_RDONLY);
    if (b->fd < 0) return BWAMS_ERR_IO;
    if (int rc = bwams_host_alloc((size_t)kIn, reinterpret_cast<void **>(&b->zbuf))) return rc;
    b->zcap = kIn;
    if (int rc = bwams_inflater_create(device, kIn, kOut, &b->inf)) return rc;
    *out = std::move(b);
    return BWAMS_OK;
}

int bwams_reader_open(const char *path, int64_t chunk_bases, int32_t paired, int64_t buffer_bytes, int32_t n_buffers, bwams_reader_t **out) {
    if (!path || !out || chunk_bases <= 0 || n_buffers < 1 || n_buffers > 16) return BWAMS_ERR_ARG;
    *out = nullptr;
    bwams_reader *r = nullptr;
    try {
        r = new bwams_reader();
        if (int rc = zlib_source(path, &r->src)) { delete r; return rc; }
        if (int rc = reader_start(r, chunk_bases, paired, buffer_bytes, n_buffers)) { bwams_reader_close(r); return rc; }
    } catch (...) {
        if (r) bwams_reader_close(r);
        return BWAMS_ERR_NOMEM;
    }
    *out = r;
    return BWAMS_OK;
}

int bwams_reader_open_device(const char *path, int device, int64_t chunk_bases, int32_t paired, int64_t buffer_bytes,
                             int32_t n_buffers, bwams_reader_t **out) {
    return bwams_reader_open_device2(path, device, chunk_bases, paired, buffer_bytes, n_buffers, 0, out);
}

int bwams_reader_open_device2(const char *path, int device, int64_t chunk_bases, int32_t paired, int64_t buffer_bytes,
                              int32_t n_buffers, uint32_t flags, bwams_reader_t **out) {
    if (!path || !out || chunk_bases <= 0 || n_buffers < 1 || n_buffers > 16 || (flags & ~(uint32_t)BWAMS_READER_GUNZIP)) return BWAMS_ERR_ARG;
    *out = nullptr;
    bwams_reader *r = nullptr;
    try {
        r = new bwams_reader();
        if (int rc = device_source(path, device, &r->src, flags)) { delete r; return rc; }
        if (int rc = reader_start(r, chunk_bases, paired, buffer_bytes, n_buffers)) { bwams_reader_close(r); return rc; }
    } catch (...) {
        if (r) bwams_reader_close(r);
        return BWAMS_ERR_NOMEM;
    }
    *out = r;
    return BWAMS_OK;
}

// The BAM header block from the start of the stream (bam_header_read, host/bam_query.cpp: the parse a bwams_bam_file_t shares).  What
// was inflated behind it becomes the reader's carry.
static int bam_header_parse(bwams_reader *r) {
    std::vector<char> hb;
    bwams::BamHeader h;
    const int rc = bwams::bam_header_read(
        [r](char *dst, int64_t want, std::string &e) {
            const int64_t got = r->src->read(dst, want, e);
            r->stats = r->src->st;
            return got;
        },
        r->src->step, &hb, &h, &r->err);
    if (rc) return rc;
    r->bam_text = h.text;
    r->bam_n_ref = h.n_ref;
    r->carry.assign(hb.begin() + (std::ptrdiff_t)h.end, hb.end());
    return BWAMS_OK;
}

int bwams_reader_open_bam(const char *path, int device, int64_t chunk_bases, int32_t paired, int64_t buffer_bytes, int32_t n_buffers,
                          bwams_reader_t **out) {
    if (!path || !out || chunk_bases <= 0 || n_buffers < 1 || n_buffers > 16) return BWAMS_ERR_ARG;
    *out = nullptr;
    bwams_reader *r = nullptr;
    try {
        r = new bwams_reader();
        r->bam = true;
        if (int rc = device_source(path, device, &r->src)) { delete r; return rc; }
        if (int rc = bam_header_parse(r)) { delete r; return rc; }
        // a BAM record of 150 bases is ~ 1.6 bytes per base; the text reader's default (3 per base + 64 MiB) is room enough
        if (int rc = reader_start(r, chunk_bases, paired, buffer_bytes, n_buffers)) { bwams_reader_close(r); return rc; }
    } catch (...) {
        if (r) bwams_reader_close(r);
        return BWAMS_ERR_NOMEM;
    }
    *out = r;
    return BWAMS_OK;
}

int bwams_reader_bam_header(const bwams_reader_t *r, const char **text, int64_t *n_text, int32_t *n_ref) {
    if (!r || !r->bam) return BWAMS_ERR_ARG;
    if (text) *text = r->bam_text.data();
    if (n_text) *n_text = (int64_t)r->bam_text.size();
    if (n_ref) *n_ref = r->bam_n_ref;
    return BWAMS_OK;
}

int bwams_reader_info(const bwams_reader_t *r, bwams_reader_stats_t *out) {
    if (!r || !out) return BWAMS_ERR_ARG;
    std::lock_guard<std::mutex> g(r->stat_mu);
    *out = r->stats;
    out->device_inflate = r->src->st.device_inflate;
    return BWAMS_OK;
}

// The next chunk: its text (whole records, page-locked), bytes, reads and bases.  Returns 1 at the end of the file (no chunk), a
// negative code on a read / format error (bwams_reader_error).  The buffer stays the caller's until bwams_reader_release.
int bwams_reader_next(bwams_reader_t *r, const char **text, int64_t *n_bytes, int64_t *n_reads, int64_t *n_bases) {
    if (!r || !text) return BWAMS_ERR_ARG;
    int slot;
    {
        std::unique_lock<std::mutex> g(r->mu);
        r->cv.wait(g, [r] { return !r->ready_q.empty() || (r->done && r->ready_q.empty()); });
        if (r->ready_q.empty()) return r->rc ? r->rc : 1;
        slot = r->ready_q.front();
        r->ready_q.pop_front();
    }
    Chunk &c = r->ring[(size_t)slot];
    if (r->rc) return r->rc;
    if (c.eof) return 1;
    *text = c.buf;
    if (n_bytes) *n_bytes = c.n_bytes;
    if (n_reads) *n_reads = c.n_reads;
    if (n_bases) *n_bases = c.n_bases;
    return BWAMS_OK;
}

int bwams_reader_release(bwams_reader_t *r, const char *text) {
    if (!r || !text) return BWAMS_ERR_ARG;
    for (size_t i = 0; i < r->ring.size(); ++i)
        if (r->ring[i].buf == text) {
            {
                std::lock_guard<std::mutex> g(r->mu);
                r->free_q.push_back((int)i);
            }
            r->cv.notify_all();
            return BWAMS_OK;
        }
    return BWAMS_ERR_ARG;
}

const char *bwams_reader_error(const bwams_reader_t *r) { return r ? r->err.c_str() : ""; }

// ------------------------------------------------------------------------------------------------------------------------- writer
struct bwams_writer {
    struct Piece {
        std::string bytes;
        bool members = false;                         // BGZF members already made (bwams_writer_put_bgzf): written as they are
    };
    struct Shard {
        FILE *fp = nullptr;
        std::thread th;
        std::mutex mu;
        std::condition_variable cv;
        std::map<int64_t, Piece> pending;             // sequence number -> text (written when its turn comes)
        int64_t next = 0;
        bool stop = false;
        int rc = BWAMS_OK;
        bwams_deflater_t *def = nullptr;              // BGZF writer: text is compressed on this shard's thread
        std::string gz;                               // its output buffer
    };
    std::vector<Shard *> sh;
    bool bgzf = false;
    bool bam = false;                                 // a BAM writer: members only (bwams_writer_put refuses text)
};

static const uint8_t kBgzfEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0,
                                     0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

static void writer_main(bwams_writer::Shard *s) {
    for (;;) {
        bwams_writer::Piece p;
        {
            std::unique_lock<std::mutex> g(s->mu);
            s->cv.wait(g, [s] { return s->stop || s->pending.count(s->next); });
            auto it = s->pending.find(s->next);
            if (it == s->pending.end()) { if (s->stop) return; continue; }
            p.bytes.swap(it->second.bytes);
            p.members = it->second.members;
            s->pending.erase(it);
            ++s->next;
        }
        const std::string *out = &p.bytes;
        if (s->def && !p.members && !p.bytes.empty()) {
            const int64_t n = (int64_t)p.bytes.size();
            int64_t got = 0;
            s->gz.resize((size_t)bwams_deflate_bound(n));
            if (int rc = bwams_deflater_run(s->def, p.bytes.data(), n, 0, &s->gz[0], (int64_t)s->gz.size(), 0, 0, &got, nullptr)) {
                s->rc = rc;
                got = 0;
            }
            s->gz.resize((size_t)got);
            out = &s->gz;
        }
        if (!out->empty() && fwrite(out->data(), 1, out->size(), s->fp) != out->size()) s->rc = BWAMS_ERR_IO;
        s->cv.notify_all();
    }
}

int bwams_writer_close(bwams_writer_t *w) {
    if (!w) return BWAMS_OK;
    int rc = BWAMS_OK;
    for (auto *s : w->sh) {
        if (!s) continue;
        {
            std::unique_lock<std::mutex> g(s->mu);
            s->cv.wait(g, [s] { return s->pending.empty() || s->rc; });       // everything handed over in order has been written
            s->stop = true;
        }
        s->cv.notify_all();
        if (s->th.joinable()) s->th.join();
        if (s->fp && w->bgzf && !s->rc && fwrite(kBgzfEof, 1, sizeof kBgzfEof, s->fp) != sizeof kBgzfEof) s->rc = BWAMS_ERR_IO;
        if (s->fp && fclose(s->fp)) rc = BWAMS_ERR_IO;
        if (s->def) bwams_deflater_destroy(s->def);
        if (s->rc) rc = s->rc;
        delete s;
    }
    delete w;
    return rc;
}

// n_shards == 1: `path` is the file.  n_shards > 1: "<path>.<s>.sam" (BGZF: ".sam.gz", BAM: ".bam"), s = 0 .. n_shards - 1 (one per
// GPU).  device >= 0: a BGZF writer, each shard with a deflater on that device.  bam_header: a BAM writer; every shard starts with
// the header block compressed into members of its own, so that the first record starts a member.
static int writer_open(const char *path, int32_t n_shards, int device, bwams_writer_t **out, const void *bam_header = nullptr,
                       int64_t n_header = 0) {
    if (!path || !out || n_shards < 1 || n_shards > 64) return BWAMS_ERR_ARG;
    *out = nullptr;
    bwams_writer *w = nullptr;
    try {
        w = new bwams_writer();
        w->bgzf = device >= 0;
        w->bam = bam_header != nullptr;
        std::string hdr;
        if (w->bam && n_header > 0) {
            bwams_deflater_t *d = nullptr;
            if (int rc = bwams_deflater_create(device, 32 << 20, &d)) { delete w; return rc; }
            hdr.resize((size_t)bwams_deflate_bound(n_header));
            int64_t got = 0;
            const int rc = bwams_deflater_run(d, bam_header, n_header, 0, &hdr[0], (int64_t)hdr.size(), 0, 0, &got, nullptr);
            bwams_deflater_destroy(d);
            if (rc) { delete w; return rc; }
            hdr.resize((size_t)got);
        }
        for (int s = 0; s < n_shards; ++s) {
            auto *x = new bwams_writer::Shard();
            w->sh.push_back(x);
            if (w->bgzf)
                if (int rc = bwams_deflater_create(device, 32 << 20, &x->def)) { bwams_writer_close(w); return rc; }
            const std::string name = n_shards == 1 ? std::string(path)
                                                   : std::string(path) + "." + std::to_string(s) + (w->bam ? ".bam" : w->bgzf ? ".sam.gz" : ".sam");
            x->fp = fopen(name.c_str(), "wb");
            if (!x->fp) { bwams_writer_close(w); return BWAMS_ERR_IO; }
            setvbuf(x->fp, nullptr, _IOFBF, 8 << 20);
            if (!hdr.empty() && fwrite(hdr.data(), 1, hdr.size(), x->fp) != hdr.size()) { bwams_writer_close(w); return BWAMS_ERR_IO; }
            x->th = std::thread(writer_main, x);
        }
    } catch (...) {
        if (w) bwams_writer_close(w);
        return BWAMS_ERR_NOMEM;
    }
    *out = w;
    return BWAMS_OK;
}

int bwams_writer_open(const char *path, int32_t n_shards, bwams_writer_t **out) { return writer_open(path, n_shards, -1, out); }

int bwams_writer_open_bgzf(const char *path, int32_t n_shards, int device, bwams_writer_t **out) {
    if (device < 0) return BWAMS_ERR_ARG;
    return writer_open(path, n_shards, device, out);
}

int bwams_writer_open_bam(const char *path, int32_t n_shards, int device, const void *bam_header, int64_t n, bwams_writer_t **out) {
    if (device < 0 || !bam_header || n < 4 || memcmp(bam_header, "BAM\1", 4) != 0) return BWAMS_ERR_ARG;
    return writer_open(path, n_shards, device, out, bam_header, n);
}

// Hand shard `shard` the text with sequence number `seq` (0, 1, 2 ... per shard, any arrival order); the bytes are copied, the call
// returns at once, the shard's thread writes seq 0, 1, 2 ... in that order.
static int writer_put(bwams_writer_t *w, int32_t shard, int64_t seq, const char *bytes, int64_t n_bytes, bool members) {
    if (!w || shard < 0 || shard >= (int32_t)w->sh.size() || seq < 0 || n_bytes < 0 || (n_bytes && !bytes)) return BWAMS_ERR_ARG;
    auto *s = w->sh[(size_t)shard];
    try {
        bwams_writer::Piece p;
        p.bytes.assign(bytes ? bytes : "", (size_t)n_bytes);
        p.members = members;
        std::lock_guard<std::mutex> g(s->mu);
        if (seq < s->next || s->pending.count(seq)) return BWAMS_ERR_ARG;
        s->pending.emplace(seq, std::move(p));
    } catch (...) {
        return BWAMS_ERR_NOMEM;
    }
    s->cv.notify_all();
    return s->rc;
}

int bwams_writer_put(bwams_writer_t *w, int32_t shard, int64_t seq, const char *text, int64_t n_bytes) {
    if (w && w->bam) return BWAMS_ERR_ARG;           // text would corrupt a BAM stream
    return writer_put(w, shard, seq, text, n_bytes, false);
}

// Members already made go to a BGZF writer's shard as they are, in the same sequence order as the text of bwams_writer_put.
int bwams_writer_put_bgzf(bwams_writer_t *w, int32_t shard, int64_t seq, const uint8_t *members, int64_t n_bytes) {
    if (w && !w->bgzf) return BWAMS_ERR_ARG;
    return writer_put(w, shard, seq, reinterpret_cast<const char *>(members), n_bytes, true);
}

// ------------------------------------------------------------------------------------------------- step 0 for mem_process_seqs()
// bseq_read_orig's records from a chunk's text, IN PLACE: the strings of seqs[i] point into `text`, which is cut up with NULs
// (kseq2bseq1 strdup()s them, src/bwa.cpp:74-153; here the chunk buffer plays strbuf's part and lives until the chunk is written).
// Sequence and quality lines of wrapped records are joined in place.  copy_comment = 0: comments are dropped as process() drops them
// without `mem -C` (src/fastmap.cpp:356-363).  Returns the number of records (n_reads expected), or a negative code.
#include "bwamem_hip.h"

static inline bool is_space_c(unsigned char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

int64_t bwams_bseq_parse(char *t, int64_t n_bytes, int64_t n_reads, bseq1_t *seqs, int copy_comment) {
    if (!t || !seqs || n_bytes < 0 || n_reads < 0) return BWAMS_ERR_ARG;
    const int64_t end = n_bytes;
    auto line_end = [&](int64_t a) -> int64_t {
        const void *q = a < end ? memchr(t + a, '\n', (size_t)(end - a)) : nullptr;
        return q ? (const char *)q - t : end;
    };
    int64_t p = 0, n = 0;
    while (p < end && n < n_reads) {
        if (t[p] == '\n' || t[p] == '\r') { ++p; continue; }
        if (t[p] != '@' && t[p] != '>') return BWAMS_ERR_UNSUPPORTED;
        bseq1_t &s = seqs[n];
        memset(&s, 0, sizeof s);
        int64_t e = line_end(p);
        // header: name up to the first isspace(), the rest of the line is the comment (one trailing '\r' dropped when longer than 1)
        int64_t q = p + 1;
        while (q < e && !is_space_c((unsigned char)t[q])) ++q;
        int64_t l_name = q - (p + 1);
        char *name = t + p + 1;
        int64_t l_comment = 0;
        char *comment = nullptr;
        if (q < e) { comment = t + q + 1; l_comment = e - (q + 1); if (l_comment > 1 && comment[l_comment - 1] == '\r') --l_comment; }
        if (l_name > 2 && name[l_name - 2] == '/' && name[l_name - 1] >= '0' && name[l_name - 1] <= '9') l_name -= 2;      // trim_readno
        int64_t a = e < end ? e + 1 : end;
        name[l_name] = 0;                                  // (the byte behind the name is the delimiter, a '/' or the line's '\n')
        if (comment) comment[l_comment] = 0;
        // sequence lines, joined at `dst`
        char *seq = t + a;
        int64_t l_seq = 0;
        bool plus = false;
        while (a < end) {
            const char c = t[a];
            if (c == '\n') { ++a; continue; }
            if (c == '+') { plus = true; break; }
            if (c == '>' || c == '@') break;
            e = line_end(a);
            int64_t len = e - a;
            if (len > 0 && l_seq + len > 1 && t[e - 1] == '\r') --len;
            if (seq + l_seq != t + a) memmove(seq + l_seq, t + a, (size_t)len);
            l_seq += len;
            a = e < end ? e + 1 : end;
        }
        char *qual = nullptr;
        if (plus) {
            e = line_end(a);
            a = e < end ? e + 1 : end;
            qual = t + a;
            int64_t l_qual = 0;
            do {
                if (a >= end) return BWAMS_ERR_IO;         // truncated quality: the reader's -2
                e = line_end(a);
                int64_t len = e - a;
                if (len > 0 && l_qual + len > 1 && t[e - 1] == '\r') --len;
                if (qual + l_qual != t + a) memmove(qual + l_qual, t + a, (size_t)len);
                l_qual += len;
                a = e < end ? e + 1 : end;
            } while (l_qual < l_seq);
            if (l_qual != l_seq) return BWAMS_ERR_IO;
            if (l_qual > 0) qual[l_qual] = 0;                    // lands on the last line's '\n' (or '\r'), never behind the record
            if (l_qual == 0) qual = nullptr;               // kseq2bseq1: an empty quality string is no quality string
        }
        // the NUL behind the sequence: the joined sequence ends at or before the '\n' of its last line (or at the '+' / next header when
        // the record has no bases: then that byte must stay, and an empty string is taken from the header line's own terminator)
        if (l_seq > 0) seq[l_seq] = 0; else seq = name + l_name;
        s.name = name;
        s.comment = (copy_comment && comment && l_comment > 0) ? comment : nullptr;
        s.seq = seq;
        s.qual = qual;
        s.l_seq = (int)l_seq;
        s.id = (int)n;
        ++n;
        p = a;
    }
    return n;
}
