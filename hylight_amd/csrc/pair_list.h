// pair_list.h - the pair list of hlmi_polish_pairs / hlmi_polish_reads_pairs (include/hylight_mi.h: "List file format",
// "Meaning"): the scan of the list's text and the set of listed pairs hlmi_polish_pairs tests its rows against.  The fused call
// parses the same text on the device (polish_pairs.hip) and must agree with this scan.  Nothing of HIP's is included:
// tests/capi/polish_pairs_host_check.cpp compiles this header with the host compiler alone.
#pragma once
#include <cstdint>
#include <string>
#include <string_view>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace hlmi {
namespace pol {

struct PairLine {
    std::string_view a, b;           // fields 1 and 6 (views into the scanned text)
};

// Lines end at '\n' (a last line without one counts; a '\r' stays in its field), fields are split at TAB, fields 1 and 6 are
// taken.  -> 0, or the 1-based number of the first line with fewer than 6 fields (an empty line is one); `out` then holds the
// lines in front of it.
inline uint64_t scan_pair_list(std::string_view d, std::vector<PairLine> &out) {
    uint64_t line = 0;
    for (size_t pos = 0; pos < d.size();) {
        size_t e = d.find('\n', pos);
        if (e == std::string_view::npos) e = d.size();
        ++line;
        const std::string_view L = d.substr(pos, e - pos);
        PairLine pl;
        int field = 1;
        size_t start = 0;
        for (size_t k = 0; k <= L.size() && field <= 6; ++k) {
            if (k < L.size() && L[k] != '\t') continue;
            if (field == 1) pl.a = L.substr(start, k - start);
            if (field == 6) pl.b = L.substr(start, k - start);
            ++field;
            start = k + 1;
        }
        if (field <= 6) return line;
        out.push_back(pl);
        pos = e + 1;
    }
    return 0;
}

// ids of the names a call knows: the records of its reads and of its contigs, one id per distinct name
struct KnownNames {
    std::unordered_map<std::string_view, uint32_t> id;       // views into names the caller keeps alive
    void add(const std::vector<std::string> &names) {
        for (const std::string &n : names) id.emplace(n, (uint32_t)id.size());
    }
    int64_t find(std::string_view n) const {
        const auto it = id.find(n);
        return it == id.end() ? -1 : (int64_t)it->second;
    }
};

// The listed pairs, both orders of each; the two counters of hlmi_polish_pstats that the list alone decides.
struct PairSet {
    std::unordered_set<uint64_t> keys;       // id_a << 32 | id_b
    uint64_t listed = 0, unknown = 0;
    bool has(uint32_t a, uint32_t b) const { return keys.count((uint64_t)a << 32 | b) != 0; }
};

inline PairSet make_pair_set(const std::vector<PairLine> &lines, const KnownNames &known) {
    PairSet s;
    for (const PairLine &l : lines) {
        const int64_t a = known.find(l.a), b = known.find(l.b);
        if (a < 0 || b < 0) { ++s.unknown; continue; }
        if (a == b) continue;                                 // one name twice: no row can be meant (qname == tname is skipped first)
        if (s.keys.insert((uint64_t)a << 32 | (uint64_t)b).second) {
            s.keys.insert((uint64_t)b << 32 | (uint64_t)a);
            ++s.listed;
        }
    }
    return s;
}

}  // namespace pol
}  // namespace hlmi
