// bam_query.cpp — what a region query of a BAM file decides on the host before any byte is read (include/bwams.h, "BAM file by
// region", rules 2 and 3): the BAM header block, the BAI parsed with every count checked against the buffer, the regions sorted and
// merged, and the plan — the disjoint intervals of virtual offsets to inflate.  bwams/bai.py restates the plan (plan()); the file and
// its pieces are host/bam_query_file.cpp.  No device, no library call: tools/bai_plan_check.cpp builds this file alone.
#include <algorithm>
#include <cstring>

#include "bam_query.h"

namespace bwams {

int bam_header_read(const BamHeaderRead &read, int64_t step, std::vector<char> *hb_, BamHeader *h, std::string *err) {
    std::vector<char> &hb = *hb_;
    bool file_end = false;
    auto need = [&](size_t n) -> int {                       // 0: hb holds n bytes
        while (hb.size() < n) {
            if (file_end) { *err = "the file ends inside the BAM header"; return BWAMS_ERR_IO; }
            const size_t have = hb.size();
            const int64_t want = std::max<int64_t>(1 << 20, (int64_t)std::min<size_t>(n - have, (size_t)step));
            hb.resize(have + (size_t)want);
            const int64_t got = read(hb.data() + have, want, *err);
            hb.resize(have + (size_t)std::max<int64_t>(got, 0));
            if (got < 0) return (int)got;
            if (got == 0) file_end = true;
        }
        return BWAMS_OK;
    };
    auto i32 = [&](size_t at) {
        const unsigned char *u = reinterpret_cast<const unsigned char *>(hb.data()) + at;
        return (int32_t)((uint32_t)u[0] | (uint32_t)u[1] << 8 | (uint32_t)u[2] << 16 | (uint32_t)u[3] << 24);
    };
    if (int rc = need(4)) return rc;
    if (memcmp(hb.data(), "BAM\1", 4) != 0) { *err = "not a BAM file (no BAM\\1 magic)"; return BWAMS_ERR_UNSUPPORTED; }
    if (int rc = need(8)) return rc;
    const int64_t l_text = i32(4);
    if (l_text < 0) { *err = "BAM header: negative l_text"; return BWAMS_ERR_IO; }
    if (int rc = need((size_t)(12 + l_text))) return rc;
    h->text.assign(hb.data() + 8, (size_t)l_text);
    const int32_t n_ref = i32((size_t)(8 + l_text));
    if (n_ref < 0) { *err = "BAM header: negative n_ref"; return BWAMS_ERR_IO; }
    size_t p = (size_t)(12 + l_text);
    h->l_ref.clear();
    for (int32_t k = 0; k < n_ref; ++k) {
        if (int rc = need(p + 4)) return rc;
        const int64_t l_name = i32(p);
        if (l_name < 1) { *err = "BAM header: reference " + std::to_string(k) + " without a name"; return BWAMS_ERR_IO; }
        if (int rc = need(p + 8 + (size_t)l_name)) return rc;
        h->l_ref.push_back(i32(p + 4 + (size_t)l_name));
        p += 8 + (size_t)l_name;
    }
    h->n_ref = n_ref;
    h->end = p;
    return BWAMS_OK;
}

int bai_parse(const void *bai, int64_t n_bai, Bai *out, std::string *err) {
    const uint8_t *b = static_cast<const uint8_t *>(bai);
    int64_t p = 0;
    auto cut = [&](const char *what) {
        *err = std::string("BAI: cut off inside ") + what + " at byte " + std::to_string(p) + " of " + std::to_string(n_bai);
        return BWAMS_ERR_IO;
    };
    auto room = [&](int64_t bytes) { return bytes >= 0 && bytes <= n_bai - p; };
    auto u32 = [&]() {
        const uint32_t v = (uint32_t)b[p] | (uint32_t)b[p + 1] << 8 | (uint32_t)b[p + 2] << 16 | (uint32_t)b[p + 3] << 24;
        p += 4;
        return v;
    };
    auto u64 = [&]() {
        const uint64_t lo = u32();
        return lo | (uint64_t)u32() << 32;
    };
    out->refs.clear();
    if (!bai || n_bai < 0 || !room(8)) return cut("the magic and n_ref");
    if (memcmp(b, "BAI\1", 4) != 0) { *err = "not a BAI (no BAI\\1 magic)"; return BWAMS_ERR_IO; }
    p = 4;
    const int64_t n_ref = (int32_t)u32();
    if (n_ref < 0 || n_ref > (n_bai - p) / 8) return cut("the references");      // a reference takes 8 bytes at the least
    out->refs.resize((size_t)n_ref);
    for (int64_t r = 0; r < n_ref; ++r) {
        BaiRef &R = out->refs[(size_t)r];
        if (!room(4)) return cut("n_bin");
        const int64_t n_bin = (int32_t)u32();
        if (n_bin < 0 || n_bin > (n_bai - p) / 8) return cut("the bins");
        R.bin.reserve((size_t)n_bin);
        R.first.assign(1, 0);
        for (int64_t k = 0; k < n_bin; ++k) {
            if (!room(8)) return cut("a bin");
            const uint32_t bin = u32();
            const int64_t n_chunk = (int32_t)u32();
            if (n_chunk < 0 || n_chunk > (n_bai - p) / 16) return cut("a bin's chunks");
            for (int64_t c = 0; c < n_chunk; ++c) {
                R.beg.push_back(u64());
                R.end.push_back(u64());
            }
            R.bin.push_back(bin);
            R.first.push_back((int64_t)R.beg.size());
        }
        if (!room(4)) return cut("n_intv");
        const int64_t n_intv = (int32_t)u32();
        if (n_intv < 0 || n_intv > (n_bai - p) / 8) return cut("the linear index");
        R.lin.resize((size_t)n_intv);
        for (int64_t k = 0; k < n_intv; ++k) R.lin[(size_t)k] = u64();
    }
    if (!room(8)) return cut("n_no_coor");
    out->n_no_coor = u64();
    return BWAMS_OK;
}

int regions_merge(const bwams_pileup_region_t *regions, int32_t n_regions, int32_t n_ref, std::vector<bwams_pileup_region_t> *out,
                  std::string *err) {
    out->clear();
    if (n_regions < 0 || (n_regions && !regions)) { *err = "n_regions >= 0 regions are required"; return BWAMS_ERR_ARG; }
    for (int32_t k = 0; k < n_regions; ++k) {
        const bwams_pileup_region_t &g = regions[k];
        if (g.ref < 0 || g.ref >= n_ref || g.beg < 0 || g.beg >= g.end) {
            *err = "region " + std::to_string(k) + " (" + std::to_string(g.ref) + ", " + std::to_string(g.beg) + ", " + std::to_string(g.end) +
                   "): 0 <= ref < n_ref (" + std::to_string(n_ref) + ") and 0 <= beg < end are required";
            return BWAMS_ERR_ARG;
        }
    }
    std::vector<bwams_pileup_region_t> v(regions, regions + n_regions);
    std::sort(v.begin(), v.end(), [](const bwams_pileup_region_t &a, const bwams_pileup_region_t &b) {
        return a.ref != b.ref ? a.ref < b.ref : a.beg != b.beg ? a.beg < b.beg : a.end < b.end;
    });
    for (const bwams_pileup_region_t &g : v) {
        if (!out->empty() && out->back().ref == g.ref && g.beg <= out->back().end) out->back().end = std::max(out->back().end, g.end);
        else out->push_back(g);
    }
    return BWAMS_OK;
}

void bai_plan(const Bai &bai, const std::vector<bwams_pileup_region_t> &merged, std::vector<uint64_t> *beg, std::vector<uint64_t> *end) {
    std::vector<std::pair<uint64_t, uint64_t>> ch;
    for (const bwams_pileup_region_t &g : merged) {
        if (g.ref < 0 || (size_t)g.ref >= bai.refs.size()) continue;
        const BaiRef &R = bai.refs[(size_t)g.ref];
        const uint64_t min_off = R.lin.empty() ? 0 : R.lin[std::min<size_t>((size_t)g.beg >> 14, R.lin.size() - 1)];
        const uint32_t b = (uint32_t)g.beg, e = (uint32_t)g.end - 1;
        for (size_t k = 0; k < R.bin.size(); ++k) {
            const uint32_t bin = R.bin[k];
            // reg2bins(beg, end) as a test of one bin; it never names pseudo-bin 37450 (the last real bin is 37448)
            bool in = bin == 0;
            const struct { int shift; uint32_t first, next; } level[5] = {{26, 1, 9}, {23, 9, 73}, {20, 73, 585}, {17, 585, 4681}, {14, 4681, 37449}};
            for (const auto &l : level)
                if (bin >= l.first && bin < l.next) in = bin - l.first >= (b >> l.shift) && bin - l.first <= (e >> l.shift);
            if (!in) continue;
            for (int64_t c = R.first[k]; c < R.first[k + 1]; ++c) {
                const uint64_t cb = std::max(R.beg[(size_t)c], min_off), ce = R.end[(size_t)c];
                if (ce > min_off && cb < ce) ch.emplace_back(cb, ce);
            }
        }
    }
    std::sort(ch.begin(), ch.end());
    beg->clear();
    end->clear();
    for (const auto &c : ch) {
        if (!end->empty() && c.first <= end->back()) end->back() = std::max(end->back(), c.second);
        else { beg->push_back(c.first); end->push_back(c.second); }
    }
}

}  // namespace bwams
