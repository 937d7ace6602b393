// inflate.hip — BGZF input inflated on the device: RFC 1951 DEFLATE, one wave per member.
//
// Replaces the gzread() behind kseq (the reference inflates every compressed input with zlib on one thread) for BGZF files, the
// blocked gzip of SAMv1 §4.1: a chain of independent gzip members, each at most 64 KiB in and out, whose header carries the member's
// compressed size (the 'BC' extra subfield).  The host walks that header chain (O(members), ~26 bytes read per 64 KiB), reads BSIZE,
// CRC32 and ISIZE, and gives every member its output offset by an exclusive scan of the ISIZEs.  The device does the rest.
//
// Mapping.  One 64-lane workgroup per member, every lane running the same decoder on the same (wave-uniform) state:
//   * the member's compressed bytes come through a 4 KiB LDS window that the 64 lanes reload together; the bit buffer is 64 bits;
//   * its output is built in a 64 KiB LDS buffer (a member never inflates to more), so back-references read LDS only;
//   * code tables are built in LDS by all lanes: a first-level table of 2^10 (literal/length) or 2^8 (distance) entries, and for the
//     rare longer code the canonical count/symbol walk; validity follows zlib's inflate_table (over-subscribed and incomplete codes
//     refused, except the single code of length 1; symbols 286/287 and distances 30/31 refused when decoded);
//   * a literal is one lane's LDS byte store; a match is copied 64 bytes per step (an overlap, distance < length, reads i % distance);
//   * CRC32 is wave-parallel: a lane per 1/64 of the output with a byte table in LDS, the lanes' remainders joined by x^(8n) mod P;
//   * only a member whose CRC32 and ISIZE check out is written to HBM, in dwords, inside [out_off, out_off + ISIZE).
// Every read stays inside the member's input range (bytes past it read as 0 and count as an overrun) and every write inside its
// output range, so damaged input gives a status per member, never a fault.  LDS ~73 KiB: two members per CU.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "crc32.h"
#include "inflate_common.h"

using namespace bwams;

namespace {

constexpr int kOutMax = 65536;           // a BGZF member inflates to at most 64 KiB
using Bits = BitsT<int>;                 // byte positions inside one member

struct Member {                          // one BGZF member as the kernel sees it (32 bytes)
    int64_t in_off;                      // its DEFLATE data in the input buffer
    int64_t out_off;                     // where its ISIZE bytes go
    int32_t in_len, isize;
    uint32_t crc;
    int32_t pad_;
};

struct Lds {
    uint8_t out[kOutMax];
    uint8_t in[kInWin];
    uint16_t ltab[1 << kLRoot], dtab[1 << kDRoot];
    uint16_t lsym[288], dsym[32], lcnt[16], dcnt[16], off[16], next[16];
    uint8_t lens[320];
    uint32_t crc_tab[256], part[64];
};

__device__ int inflate_member(Lds &s, const uint8_t *__restrict__ in, int in_len, int isize, int lane) {
    Bits b{0, 0, 0, 0};
    window_load(s, in, in_len, 0, lane);
    const Code lc{s.ltab, s.lcnt, s.lsym, kLRoot}, dc{s.dtab, s.dcnt, s.dsym, kDRoot}, cc{s.ltab, s.lcnt, s.lsym, 7};
    int pos = 0, last = 0;
    while (!last) {
        refill(b, s, in, in_len, lane);
        if ((int64_t)b.ip * 8 - b.bc > (int64_t)in_len * 8) return ST_OVERRUN;
        last = (int)take(b, 1);
        const int type = (int)take(b, 2);
        if (type == 0) {                              // stored
            take(b, b.bc & 7);
            const uint32_t len = take(b, 16), nlen = take(b, 16);
            if (len != (~nlen & 0xffffu)) return ST_STORED_LEN;
            const int p = b.ip - b.bc / 8;            // the byte behind NLEN
            if (p + (int)len > in_len) return ST_OVERRUN;
            if (pos + (int)len > isize) return ST_OVERFLOW;
            __syncthreads();
            for (int i = lane; i < (int)len; i += 64) s.out[pos + i] = in[p + i];
            pos += (int)len;
            b.bb = 0; b.bc = 0; b.ip = p + (int)len;
            continue;
        }
        if (type == 3) return ST_BTYPE;
        int rc;
        if (type == 1) {                              // fixed codes
            __syncthreads();
            for (int i = lane; i < 320; i += 64) s.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
            if ((rc = build(s, s.lens, 288, lc, false, lane))) return rc;
            if ((rc = build(s, s.lens + 288, 32, dc, false, lane))) return rc;
        } else {                                      // dynamic codes
            const int nlen = (int)take(b, 5) + 257, ndist = (int)take(b, 5) + 1, ncode = (int)take(b, 4) + 4;
            if (nlen > 286 || ndist > 30) return ST_COUNTS;
            refill(b, s, in, in_len, lane);
            __syncthreads();
            if (lane < 19) s.lens[lane] = 0;
            __syncthreads();
            for (int i = 0; i < ncode; ++i) {
                const uint8_t v = (uint8_t)take(b, 3);
                if (lane == 0) s.lens[kClOrder[i]] = v;
            }
            if (build(s, s.lens, 19, cc, true, lane)) return ST_CODE_LENS;
            int n = 0, prev = 0;
            while (n < nlen + ndist) {
                if (b.bc < 32) refill(b, s, in, in_len, lane);
                if ((int64_t)b.ip * 8 - b.bc > (int64_t)in_len * 8) return ST_OVERRUN;
                const int sym = decode(b, cc);
                if (sym < 0) return ST_CODE_LENS;
                if (sym < 16) {
                    if (lane == 0) s.lens[n] = (uint8_t)sym;
                    prev = sym;
                    ++n;
                    continue;
                }
                int v, rep;
                if (sym == 16) {
                    if (n == 0) return ST_REPEAT;
                    v = prev; rep = 3 + (int)take(b, 2);
                } else if (sym == 17) {
                    v = 0; rep = 3 + (int)take(b, 3);
                } else {
                    v = 0; rep = 11 + (int)take(b, 7);
                }
                if (n + rep > nlen + ndist) return ST_REPEAT;
                for (int i = lane; i < rep; i += 64) s.lens[n + i] = (uint8_t)v;
                prev = v;
                n += rep;
            }
            __syncthreads();
            if (s.lens[256] == 0) return ST_NO_EOB;
            if ((rc = build(s, s.lens, nlen, lc, false, lane))) return rc;
            if ((rc = build(s, s.lens + nlen, ndist, dc, false, lane))) return rc;
        }
        for (;;) {                                    // the block's symbols
            if (b.bc < 48) refill(b, s, in, in_len, lane);
            if ((int64_t)b.ip * 8 - b.bc > (int64_t)in_len * 8) return ST_OVERRUN;
            int sym = decode(b, lc);
            if (sym < 0) return ST_BAD_LITLEN;
            if (sym < 256) {
                if (pos >= isize) return ST_OVERFLOW;
                if (lane == 0) s.out[pos] = (uint8_t)sym;
                ++pos;
                continue;
            }
            if (sym == 256) break;
            sym -= 257;
            if (sym >= 29) return ST_BAD_LITLEN;
            const int len = kLenBase[sym] + (int)take(b, kLenExtra[sym]);
            const int dsym = decode(b, dc);
            if (dsym < 0 || dsym >= 30) return ST_BAD_DIST;
            const int dist = kDistBase[dsym] + (int)take(b, kDistExtra[dsym]);
            if (dist > pos) return ST_FAR;
            if (pos + len > isize) return ST_OVERFLOW;
            __syncthreads();                          // the literals and matches before this one are in LDS
            const int from = pos - dist;
            if (dist >= len) {
                for (int i = lane; i < len; i += 64) s.out[pos + i] = s.out[from + i];
            } else {
                for (int i = lane; i < len; i += 64) s.out[pos + i] = s.out[from + i % dist];
            }
            pos += len;
        }
    }
    take(b, b.bc & 7);
    const int64_t used = (int64_t)b.ip - b.bc / 8;
    if (used > in_len) return ST_OVERRUN;
    if (used < in_len) return ST_TRAILING;
    if (pos != isize) return ST_ISIZE;
    return ST_OK;
}

__global__ __launch_bounds__(64) void inflate_kernel(const uint8_t *__restrict__ in, const Member *__restrict__ mem,
                                                     uint8_t *__restrict__ out, int32_t *__restrict__ status) {
    __shared__ Lds s;
    const int lane = (int)threadIdx.x;
    const Member m = mem[blockIdx.x];
    crc32_table<64>(s.crc_tab, lane);
    int st = inflate_member(s, in + m.in_off, m.in_len, m.isize, lane);
    if (st == ST_OK) {
        __syncthreads();
        if (crc32_lds<64>(s.out, m.isize, s.crc_tab, s.part, lane) != m.crc) st = ST_CRC;
    }
    if (st == ST_OK) {                                 // to HBM: bytes up to a 4-byte boundary, then dwords, then the tail
        uint8_t *o = out + m.out_off;
        const int n = m.isize;
        const int head = min((int)((4 - ((uintptr_t)o & 3)) & 3), n);
        if (lane < head) o[lane] = s.out[lane];
        const int nw = (n - head) >> 2;
        uint32_t *ow = reinterpret_cast<uint32_t *>(o + head);
        for (int w = lane; w < nw; w += 64) {
            const int q = head + 4 * w;
            ow[w] = (uint32_t)s.out[q] | (uint32_t)s.out[q + 1] << 8 | (uint32_t)s.out[q + 2] << 16 | (uint32_t)s.out[q + 3] << 24;
        }
        const int t = head + 4 * nw;
        if (t + lane < n) o[t + lane] = s.out[t + lane];
    }
    if (lane == 0) status[blockIdx.x] = st;
}

inline uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

enum Hdr { HDR_OK, HDR_SHORT, HDR_NOT_BGZF, HDR_BAD };

// A BGZF member header at p (n bytes there): *hdr = bytes of the header, *total = BSIZE + 1.  HDR_SHORT: the bytes there could be the
// start of one, more are needed.
Hdr bgzf_header(const uint8_t *p, int64_t n, int *hdr, int *total) {
    static const uint8_t magic[4] = {31, 139, 8, 4};      // ID1 ID2 CM FLG (FEXTRA only)
    for (int i = 0; i < 4; ++i) {
        if (i >= n) return HDR_SHORT;
        if (p[i] != magic[i]) return HDR_NOT_BGZF;
    }
    if (n < 12) return HDR_SHORT;
    const int xlen = p[10] | p[11] << 8;
    if (xlen < 6) return HDR_NOT_BGZF;
    if (n < 12 + xlen) return HDR_SHORT;
    int bsize = -1;
    for (int q = 12; q + 4 <= 12 + xlen;) {
        const int slen = p[q + 2] | p[q + 3] << 8;
        if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2 && q + 6 <= 12 + xlen) bsize = p[q + 4] | p[q + 5] << 8;
        q += 4 + slen;
    }
    if (bsize < 0) return HDR_NOT_BGZF;
    *hdr = 12 + xlen;
    *total = bsize + 1;
    return *total < *hdr + 8 ? HDR_BAD : HDR_OK;
}

}  // namespace

struct bwams_inflater {
    int device = 0;
    int64_t max_in = 0, max_out = 0, max_members = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev[4] = {};
    bwams::DevBuf<uint8_t> d_in, d_out;
    bwams::DevBuf<Member> d_mem;
    bwams::HostBuf<Member> h_mem;                     // h_mem / h_status page-locked
    bwams::DevBuf<int32_t> d_status;
    bwams::HostBuf<int32_t> h_status;
    int64_t members_done = 0, bytes_done = 0;         // over every call: a handle fed one file in order names the file's members
    std::vector<int64_t> at;                          // this call's members: where each starts in gz
};

extern "C" {

int bwams_inflater_destroy(bwams_inflater_t *f) {
    if (!f) return BWAMS_OK;
    (void)hipSetDevice(f->device);
    if (f->st) (void)hipStreamSynchronize(f->st);
    for (auto e : f->ev) if (e) (void)hipEventDestroy(e);
    if (f->st) (void)hipStreamDestroy(f->st);
    delete f;
    return BWAMS_OK;
}

int bwams_inflater_create(int device, int64_t max_in_bytes, int64_t max_out_bytes, bwams_inflater_t **out) {
    if (!out) return BWAMS_ERR_ARG;
    *out = nullptr;
    if (max_in_bytes < kOutMax || max_out_bytes < kOutMax || max_in_bytes > ((int64_t)1 << 40) || max_out_bytes > ((int64_t)1 << 40)) {
        set_last_error("bwams_inflater_create: max_in_bytes and max_out_bytes must be at least 65536 (one BGZF member)");
        return BWAMS_ERR_ARG;
    }
    if (int rc = device_ok(device)) return rc;
    BWAMS_HIP(hipSetDevice(device));
    auto *f = new bwams_inflater();
    f->device = device;
    f->max_in = max_in_bytes;
    f->max_out = max_out_bytes;
    f->max_members = max_in_bytes / 28 + 1;           // a member takes at least 28 bytes (the EOF member's size)
    auto fail = [&](hipError_t e) {
        set_last_error(std::string("bwams_inflater_create: ") + hipGetErrorString(e));
        bwams_inflater_destroy(f);
        return e == hipErrorOutOfMemory ? BWAMS_ERR_NOMEM : BWAMS_ERR_DEVICE;
    };
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&f->st, hipStreamNonBlocking)) != hipSuccess) return fail(e);
    for (auto &x : f->ev)
        if ((e = hipEventCreate(&x)) != hipSuccess) return fail(e);
    if ((e = f->d_in.alloc((size_t)max_in_bytes)) != hipSuccess) return fail(e);
    if ((e = f->d_out.alloc((size_t)max_out_bytes)) != hipSuccess) return fail(e);
    if ((e = f->d_mem.alloc(sizeof(Member) * (size_t)f->max_members)) != hipSuccess) return fail(e);
    if ((e = f->d_status.alloc(sizeof(int32_t) * (size_t)f->max_members)) != hipSuccess) return fail(e);
    if ((e = f->h_mem.alloc(sizeof(Member) * (size_t)f->max_members)) != hipSuccess) return fail(e);
    if ((e = f->h_status.alloc(sizeof(int32_t) * (size_t)f->max_members)) != hipSuccess) return fail(e);
    *out = f;
    return BWAMS_OK;
}

int bwams_inflater_run(bwams_inflater_t *f, const uint8_t *gz, int64_t n_bytes, void *out, int64_t out_cap, int out_on_device,
                       int64_t *n_consumed, int64_t *n_out, bwams_inflate_stats_t *stats) {
    if (!f || (!gz && n_bytes) || n_bytes < 0 || out_cap < 0 || (!out && out_cap)) return BWAMS_ERR_ARG;
    if (n_consumed) *n_consumed = 0;
    if (n_out) *n_out = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    BWAMS_HIP(hipSetDevice(f->device));
    // the header chain: whole members that fit max_in, out_cap and (host output) the staging buffer
    const int64_t out_lim = out_on_device ? out_cap : std::min(out_cap, f->max_out);
    int64_t p = 0, o = 0, nm = 0;
    auto where = [&](int64_t i, int64_t at) {
        return "BGZF member " + std::to_string(f->members_done + i) + " at byte " + std::to_string(f->bytes_done + at) + ": ";
    };
    while (p < n_bytes && nm < f->max_members) {
        int hdr = 0, total = 0;
        const Hdr h = bgzf_header(gz + p, n_bytes - p, &hdr, &total);
        if (h == HDR_SHORT) break;
        if (h == HDR_NOT_BGZF) {
            if (nm) break;                            // the members in front of it still go
            set_last_error(where(0, p) + "not BGZF (a gzip header with FEXTRA only and a 'BC' extra subfield)");
            return BWAMS_ERR_UNSUPPORTED;
        }
        if (h == HDR_BAD) {
            set_last_error(where(nm, p) + "BSIZE smaller than its header and trailer");
            return BWAMS_ERR_IO;
        }
        if (p + total > n_bytes) break;               // cut off by the end of the buffer
        const uint32_t isize = rd32(gz + p + total - 4);
        if (isize > (uint32_t)kOutMax) {
            set_last_error(where(nm, p) + "ISIZE " + std::to_string(isize) + " is over 65536");
            return BWAMS_ERR_IO;
        }
        if (o + (int64_t)isize > out_lim || p + total > f->max_in) {
            if (nm) break;
            set_last_error("bwams_inflater_run: the first member (" + std::to_string(isize) + " bytes) does not fit out_cap " +
                           std::to_string(out_cap));
            return BWAMS_ERR_CAPACITY;
        }
        if ((int64_t)f->at.size() <= nm) f->at.resize((size_t)nm + 1);
        f->at[(size_t)nm] = p;
        Member &m = f->h_mem.p[nm];
        m.in_off = p + hdr;
        m.in_len = total - hdr - 8;
        m.out_off = o;
        m.isize = (int32_t)isize;
        m.crc = rd32(gz + p + total - 8);
        m.pad_ = 0;
        p += total;
        o += isize;
        ++nm;
    }
    if (nm == 0) return BWAMS_OK;
    uint8_t *d_out = out_on_device ? static_cast<uint8_t *>(out) : f->d_out.p;
    BWAMS_HIP(hipEventRecord(f->ev[0], f->st));
    BWAMS_HIP(hipMemcpyAsync(f->d_in.p, gz, (size_t)p, hipMemcpyHostToDevice, f->st));
    BWAMS_HIP(hipMemcpyAsync(f->d_mem.p, f->h_mem.p, sizeof(Member) * (size_t)nm, hipMemcpyHostToDevice, f->st));
    BWAMS_HIP(hipEventRecord(f->ev[1], f->st));
    hipLaunchKernelGGL(inflate_kernel, dim3((unsigned)nm), dim3(64), 0, f->st, f->d_in.p, f->d_mem.p, d_out, f->d_status.p);
    BWAMS_HIP(hipGetLastError());
    BWAMS_HIP(hipEventRecord(f->ev[2], f->st));
    BWAMS_HIP(hipMemcpyAsync(f->h_status.p, f->d_status.p, sizeof(int32_t) * (size_t)nm, hipMemcpyDeviceToHost, f->st));
    BWAMS_HIP(hipStreamSynchronize(f->st));
    for (int64_t i = 0; i < nm; ++i)
        if (f->h_status.p[i] != ST_OK) {
            set_last_error(where(i, f->at[(size_t)i]) + status_text(f->h_status.p[i]));
            return BWAMS_ERR_IO;
        }
    if (!out_on_device && o) BWAMS_HIP(hipMemcpyAsync(out, f->d_out.p, (size_t)o, hipMemcpyDeviceToHost, f->st));
    BWAMS_HIP(hipEventRecord(f->ev[3], f->st));
    BWAMS_HIP(hipEventSynchronize(f->ev[3]));
    if (stats) {
        stats->members = nm;
        stats->in_bytes = p;
        stats->out_bytes = o;
        BWAMS_HIP(hipEventElapsedTime(&stats->ms_upload, f->ev[0], f->ev[1]));
        BWAMS_HIP(hipEventElapsedTime(&stats->ms_kernel, f->ev[1], f->ev[2]));
        BWAMS_HIP(hipEventElapsedTime(&stats->ms_download, f->ev[2], f->ev[3]));
    }
    f->members_done += nm;
    f->bytes_done += p;
    if (n_consumed) *n_consumed = p;
    if (n_out) *n_out = o;
    return BWAMS_OK;
}

}  // extern "C"
