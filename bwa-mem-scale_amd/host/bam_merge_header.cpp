// bam_merge_header.cpp — the header of several coordinate-sorted BAM files merged (include/bwams.h, above bwams_bam_file_open_merge,
// rules M2 and M3): the reference lists compared, the text lines united, the block written.  Plain C++ over the blocks' bytes, no
// device: bwams_bam_header_merge (csrc/api_bam_file.hip) and the merged handle's open call it, tools/bam_header_merge_check.cpp
// builds it alone.  Every length in a block is checked against the block's size before anything behind it is read.
#include <algorithm>
#include <cstring>
#include <map>
#include <set>

#include "bam_query.h"

namespace bwams {
namespace {

struct Ref {
    std::string name;                // l_name bytes, the NUL among them
    int32_t l_ref = 0;
};
struct Parsed {
    std::string text;
    std::vector<Ref> refs;
};

bool rd32(const uint8_t *b, int64_t n, int64_t at, int32_t *v) {
    if (at < 0 || n < 4 || at > n - 4) return false;
    memcpy(v, b + at, 4);
    return true;
}

int parse(const void *block, int64_t n, int32_t k, Parsed *out, std::string *err) {
    const std::string who = "file " + std::to_string(k) + ": ";
    const uint8_t *b = static_cast<const uint8_t *>(block);
    auto cut = [&]() { *err = who + "the header block is cut off"; return BWAMS_ERR_ARG; };
    if (!b || n < 8) return cut();
    if (memcmp(b, "BAM\1", 4) != 0) { *err = who + "the header block does not start with the BAM magic"; return BWAMS_ERR_ARG; }
    int32_t l_text = 0, n_ref = 0;
    rd32(b, n, 4, &l_text);
    if (l_text < 0 || (int64_t)l_text > n - 8) return cut();
    out->text.assign(reinterpret_cast<const char *>(b) + 8, (size_t)l_text);
    int64_t p = 8 + (int64_t)l_text;
    if (!rd32(b, n, p, &n_ref) || n_ref < 0) return cut();
    p += 4;
    for (int32_t r = 0; r < n_ref; ++r) {
        int32_t l_name = 0;
        if (!rd32(b, n, p, &l_name) || l_name < 0 || (int64_t)l_name > n - p - 8) return cut();
        Ref x;
        x.name.assign(reinterpret_cast<const char *>(b) + p + 4, (size_t)l_name);
        rd32(b, n, p + 4 + l_name, &x.l_ref);
        out->refs.push_back(std::move(x));
        p += 8 + (int64_t)l_name;
    }
    return BWAMS_OK;
}

// the text's lines without their newlines: NUL padding behind the text and empty lines are no lines
std::vector<std::string> lines_of(const std::string &text) {
    size_t end = text.size();
    while (end && text[end - 1] == '\0') --end;
    std::vector<std::string> out;
    for (size_t p = 0; p < end;) {
        size_t q = text.find('\n', p);
        if (q == std::string::npos || q > end) q = end;
        if (q > p) out.emplace_back(text, p, q - p);
        p = q + 1;
    }
    return out;
}

bool id_of(const std::string &line, std::string *id) {
    for (size_t p = line.find('\t'); p != std::string::npos; p = line.find('\t', p + 1))
        if (line.compare(p + 1, 3, "ID:") == 0) {
            const size_t q = line.find('\t', p + 1);
            *id = line.substr(p + 4, q == std::string::npos ? std::string::npos : q - p - 4);
            return true;
        }
    return false;
}

void put32(std::string *s, int32_t v) { s->append(reinterpret_cast<const char *>(&v), 4); }

}  // namespace

int bam_header_merge(const void *const *blocks, const int64_t *n_block, int32_t n_files, std::string *out, int32_t *pg_dropped,
                     std::string *err) {
    if (!blocks || !n_block || n_files < 1 || n_files > 64) { *err = "1 to 64 header blocks are required"; return BWAMS_ERR_ARG; }
    std::vector<Parsed> P((size_t)n_files);
    for (int32_t k = 0; k < n_files; ++k)
        if (int rc = parse(blocks[k], n_block[k], k, &P[(size_t)k], err)) return rc;
    const std::vector<Ref> &r0 = P[0].refs;
    for (int32_t k = 1; k < n_files; ++k) {          // M2
        const std::vector<Ref> &rk = P[(size_t)k].refs;
        if (rk.size() != r0.size()) {
            *err = "file " + std::to_string(k) + " has " + std::to_string(rk.size()) + " references, file 0 has " + std::to_string(r0.size());
            return BWAMS_ERR_UNSUPPORTED;
        }
        for (size_t r = 0; r < r0.size(); ++r) {
            const std::string where = "file " + std::to_string(k) + ": reference " + std::to_string(r) + ": its ";
            if (rk[r].name != r0[r].name) { *err = where + "name differs from file 0's"; return BWAMS_ERR_UNSUPPORTED; }
            if (rk[r].l_ref != r0[r].l_ref) {
                *err = where + "length " + std::to_string(rk[r].l_ref) + " differs from file 0's " + std::to_string(r0[r].l_ref);
                return BWAMS_ERR_UNSUPPORTED;
            }
        }
    }
    std::vector<std::string> taken_order;            // M3
    std::set<std::string> taken;
    const std::vector<std::string> first = lines_of(P[0].text);
    for (const std::string &ln : first)
        if (ln.compare(0, 3, "@HD") == 0) { taken_order.push_back(ln); break; }
    for (const std::string &ln : first)
        if (ln.compare(0, 3, "@SQ") == 0) taken_order.push_back(ln);
    taken.insert(taken_order.begin(), taken_order.end());
    std::map<std::string, int32_t> ids[2];           // @RG, @PG: ID -> the file that gave it
    int32_t dropped = 0;
    for (int32_t k = 0; k < n_files; ++k)
        for (const std::string &ln : lines_of(P[(size_t)k].text)) {
            const bool rg = ln.compare(0, 3, "@RG") == 0, pg = ln.compare(0, 3, "@PG") == 0;
            if (ln.compare(0, 3, "@HD") == 0 || ln.compare(0, 3, "@SQ") == 0 || taken.count(ln)) continue;
            std::string id;
            if ((rg || pg) && id_of(ln, &id)) {
                auto &m = ids[pg ? 1 : 0];
                auto it = m.find(id);
                if (it != m.end()) {
                    if (pg) { ++dropped; continue; }
                    *err = "file " + std::to_string(k) + ": @RG ID " + id + " is file " + std::to_string(it->second) + "'s with other bytes";
                    return BWAMS_ERR_UNSUPPORTED;
                }
                m.emplace(id, k);
            }
            taken.insert(ln);
            taken_order.push_back(ln);
        }
    std::string text;
    for (const std::string &ln : taken_order) { text += ln; text += '\n'; }
    if (text.size() > 0x7FFFFFFF) { *err = "the merged header text exceeds 2^31 - 1 bytes"; return BWAMS_ERR_UNSUPPORTED; }
    out->assign("BAM\1", 4);
    put32(out, (int32_t)text.size());
    *out += text;
    put32(out, (int32_t)r0.size());
    for (const Ref &r : r0) {
        put32(out, (int32_t)r.name.size());
        *out += r.name;
        put32(out, r.l_ref);
    }
    if (pg_dropped) *pg_dropped = dropped;
    return BWAMS_OK;
}

}  // namespace bwams
